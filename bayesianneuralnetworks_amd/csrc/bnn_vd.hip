// bnn_vd.hip -- K23: sparse variational dropout (VariationalDropoutLinear, nn/dense.py; Molchanov, Ashukha, Vetrov 2017).
// Every weight has the posterior N(theta, sigma^2), parametrised by theta and log sigma^2, and a log-uniform prior.  With
//     s2 = exp(log_sigma2),   log_alpha = clamp(log_sigma2 - ln(theta^2), -8, 8)     (theta = 0: +8)
// the layer is K10's layer on another variance plane (m = x theta^T + mu_b, v = x^2 s2^T + sigma_b^2, y_s = m + sqrt(v + 1e-16)
// eps_s; bnn_lrt_forward, bnn_lrt_backward_epilogue, bnn_lrt_backward_input and bnn_moments_forward take s2 unchanged).  New here:
//     bnn_vd_prepare           s2 (and the bias variance) in one launch; with a threshold the masked planes and their count
//     bnn_vd_backward_weight   K10's weight-gradient tile and host function (k_lrt's LRT_WGRAD, lrt_backward_weight) with this
//                              posterior's chain factor: g_theta = acc1, g_log_sigma2 = acc2 exp(log_sigma2) (ChainLogSigma2)
//     bnn_vd_kl_forward        sum_e KL_e per tensor, KL_e = k1 sigmoid(-(k2 + k3 log_alpha)) + 0.5 log1p(exp(-log_alpha))
//     bnn_vd_kl_backward       its gradient in theta and log_sigma2
// log_alpha and everything derived from it is evaluated in fp64 on the device (as bnn_moments_elu evaluates its moments):
// ln(theta^2) = 2 ln|theta| reaches 200 for a denormal theta, where an fp32 difference log_sigma2 - ln(theta^2) carries an
// absolute error of 1e-5 into a function of slope 0.5.  In fp64 what is left is the rounding of the results to fp32.
#include "bnn_lrt_tile.hpp"
#include "bnn_kl_body.hpp"

#include <cmath>

namespace bnn {

constexpr double kVdK1 = 0.63576, kVdK2 = 1.87320, kVdK3 = 1.48695;
constexpr double kVdClamp = 8.0;

// log_sigma2 - ln(theta^2), not yet clamped: +inf for theta = 0
__device__ __forceinline__ double vd_log_alpha_raw(float theta, float ls2)
{
    return (double)ls2 - 2.0 * log(fabs((double)theta));
}

__device__ __forceinline__ double vd_clamp(double la) { return la < -kVdClamp ? -kVdClamp : la > kVdClamp ? kVdClamp : la; }

__device__ __forceinline__ double vd_kl_elem(float theta, float ls2)
{
    const double la = vd_clamp(vd_log_alpha_raw(theta, ls2));
    // k1 sigmoid(-z), not k1 - k1 sigmoid(z): no cancellation at the upper end
    return kVdK1 / (1.0 + exp(kVdK2 + kVdK3 * la)) + 0.5 * log1p(exp(-la));
}

// dKL_e / dlog_alpha where the clamp is not active (la inside [-8, 8]), exactly 0 elsewhere (theta = 0 included)
__device__ __forceinline__ double vd_kl_dla(double la_raw)
{
    if (!(la_raw >= -kVdClamp && la_raw <= kVdClamp)) return 0.0;
    const double s = 1.0 / (1.0 + exp(-(kVdK2 + kVdK3 * la_raw)));
    return -kVdK1 * kVdK3 * s * (1.0 - s) - 0.5 / (1.0 + exp(la_raw));
}

// ---- operands: s2 = exp(log_sigma2), the bias variance, and with MASK the planes with log_alpha > threshold zeroed + their count.
// The count is integer: one wave popcount per wave and iteration, one integer atomic per workgroup onto a word the host entry
// zeroed in-stream -- a sum of integers, the same whatever the order.
template <bool MASK>
__global__ __launch_bounds__(256) void k_vd_prepare(const float *__restrict__ theta, const float *__restrict__ ls2, int64_t n_w,
                                                    const float *__restrict__ rho_b, float *__restrict__ s2_b, int64_t n_b,
                                                    float threshold, float *__restrict__ theta_out, float *__restrict__ s2_out,
                                                    unsigned long long *__restrict__ count_out)
{
    __shared__ unsigned int wave_count[4];
    unsigned int mine = 0;                                                  // lane 0 of each wave: dropped elements it saw
    const int64_t total = n_w + n_b;
    const int64_t stride = (int64_t)gridDim.x * 256;
    // every wave runs the same number of iterations (the ballot below wants whole waves)
    for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < total; t0 += stride) {
        const int64_t t = t0 + threadIdx.x;
        bool drop = false;
        if (t < n_w) {
            const float l = ls2[t];
            float s2 = expf(l);
            if constexpr (MASK) {
                float th = theta[t];
                drop = vd_clamp(vd_log_alpha_raw(th, l)) > (double)threshold;
                if (drop) { th = 0.f; s2 = 0.f; }
                theta_out[t] = th;
            } else if (theta_out) {
                theta_out[t] = theta[t];
            }
            s2_out[t] = s2;
        } else if (t < total) {
            const float s = sigma_lrt(rho_b[t - n_w]);
            s2_b[t - n_w] = s * s;
        }
        if constexpr (MASK) mine += (unsigned int)__popcll(__ballot(drop));
    }
    if constexpr (MASK) {
        if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned int c = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
            if (c) atomicAdd(count_out, (unsigned long long)c);
        }
    }
}

// ---- KL: K3's launch pair on this posterior.  First pass: 2048-scalar workgroups, a thread adds eight consecutive elements in index
// order (fp64), the workgroup's 256 thread sums go through the wave shuffle tree and LDS in kl_block_reduce's order -- on the
// doubles themselves (kl_block_reduce takes an fp32 thread sum) -- into one double partial; second pass: one workgroup adds a
// tensor's partials in a fixed order.  No float atomics: identical calls give identical bits.
struct VdTensorDev {
    const float *theta, *ls2;
    float *g_theta, *g_ls2;     // backward only
    int64_t n;
    int32_t first_block;        // first workgroup of this tensor within the launch
    int32_t index;              // backward: the tensor's index in the call (upstream[index])
};
struct VdLaunch {
    VdTensorDev t[kKlMaxPerLaunch];
    int32_t ntensors;
    int32_t partial_base;
};
struct VdFinal {
    int32_t first[kKlMaxTensors + 1];
    int32_t ntensors;
};

__device__ __forceinline__ int vd_find_tensor(const VdLaunch &L, int block)
{
    int t = 0;
    for (int i = 1; i < L.ntensors; ++i)
        if (block >= L.t[i].first_block) t = i;
    return t;
}

__global__ __launch_bounds__(kKlThreads) void k_vd_kl_partial(const VdLaunch L, double *__restrict__ partials)
{
    __shared__ double red[kKlThreads / 64];
    const VdTensorDev &T = L.t[vd_find_tensor(L, (int)blockIdx.x)];
    const int64_t e = (int64_t)((int)blockIdx.x - T.first_block) * kKlChunk + (int64_t)threadIdx.x * 8;
    const bool vec = ((reinterpret_cast<uintptr_t>(T.theta) | reinterpret_cast<uintptr_t>(T.ls2)) & 15u) == 0;
    double acc = 0.0;
    if (vec && e + 8 <= T.n) {
        const float4 a0 = *reinterpret_cast<const float4 *>(T.theta + e), a1 = *reinterpret_cast<const float4 *>(T.theta + e + 4);
        const float4 l0 = *reinterpret_cast<const float4 *>(T.ls2 + e), l1 = *reinterpret_cast<const float4 *>(T.ls2 + e + 4);
        acc += vd_kl_elem(a0.x, l0.x); acc += vd_kl_elem(a0.y, l0.y); acc += vd_kl_elem(a0.z, l0.z); acc += vd_kl_elem(a0.w, l0.w);
        acc += vd_kl_elem(a1.x, l1.x); acc += vd_kl_elem(a1.y, l1.y); acc += vd_kl_elem(a1.z, l1.z); acc += vd_kl_elem(a1.w, l1.w);
    } else {
        for (int j = 0; j < 8; ++j)
            if (e + j < T.n) acc += vd_kl_elem(T.theta[e + j], T.ls2[e + j]);
    }
    const double d = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kKlThreads / 64; ++w) s += red[w];
        partials[L.partial_base + (int)blockIdx.x] = s;
    }
}

// wave w adds the partials of tensors w, w + 4, ...: lane-strided, then the shuffle tree
__global__ __launch_bounds__(kKlThreads) void k_vd_kl_final(const VdFinal F, const double *__restrict__ partials, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    for (int t = threadIdx.x >> 6; t < F.ntensors; t += kKlThreads / 64) {
        double a = 0.0;
        for (int i = F.first[t] + lane; i < F.first[t + 1]; i += 64) a += partials[i];
        a = wave_sum(a);
        if (lane == 0) out[t] = (float)a;
    }
}

__global__ __launch_bounds__(kKlThreads) void k_vd_kl_backward(const VdLaunch L, const float *__restrict__ upstream, int accumulate)
{
    const VdTensorDev &T = L.t[vd_find_tensor(L, (int)blockIdx.x)];
    const int64_t base = (int64_t)((int)blockIdx.x - T.first_block) * kKlChunk;
    const double sc = (double)upstream[T.index] / (double)T.n;
#pragma unroll 1
    for (int it = 0; it < kKlPerThread; ++it) {
        const int64_t e = base + (int64_t)it * kKlThreads + threadIdx.x;
        if (e < T.n) {
            const float th = T.theta[e];
            const double d = vd_kl_dla(vd_log_alpha_raw(th, T.ls2[e]));
            // d == 0 where the clamp is active, theta = 0 among those: 0, not 0 * inf
            const float gl = (float)(sc * d);
            const float gt = d == 0.0 ? 0.f : (float)(sc * d * (-2.0 / (double)th));
            if (accumulate) { T.g_theta[e] += gt; T.g_ls2[e] += gl; }
            else { T.g_theta[e] = gt; T.g_ls2[e] = gl; }
        }
    }
}

static inline int64_t vd_chunks(int64_t n) { return (n + kKlChunk - 1) / kKlChunk; }

static int vd_validate(const bnn_vd_tensor_t *tensors, int ntensors, const char *who)
{
    if (!tensors) { set_error("%s: NULL tensor list", who); return BNN_E_NULL; }
    if (ntensors < 1) { set_error("%s: ntensors must be in [1, %d]", who, kKlMaxTensors); return BNN_E_SHAPE; }
    if (ntensors > kKlMaxTensors) { set_error("%s: ntensors must be in [1, %d]", who, kKlMaxTensors); return BNN_E_UNSUPPORTED; }
    int64_t blocks = 0;
    for (int t = 0; t < ntensors; ++t) {
        if (!tensors[t].theta || !tensors[t].log_sigma2) { set_error("%s: tensor %d NULL", who, t); return BNN_E_NULL; }
        if (tensors[t].n < 1) { set_error("%s: tensor %d empty", who, t); return BNN_E_SHAPE; }
        if (misaligned(tensors[t].theta, 3) || misaligned(tensors[t].log_sigma2, 3)) {
            set_error("%s: tensor %d misaligned pointer", who, t);
            return BNN_E_ALIGN;
        }
        blocks += vd_chunks(tensors[t].n);
    }
    if (blocks > 0x7FFFFFFF) { set_error("%s: too many elements", who); return BNN_E_RANGE; }
    return BNN_OK;
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_vd_prepare(const float *theta, const float *log_sigma2, int64_t n_w, const float *rho_b, float *s2_b, int64_t n_b,
                   float threshold, float *theta_out, float *s2_out, int64_t *count_out, void *stream)
{
    const char *who = "bnn_vd_prepare";
    const bool mask = threshold < INFINITY;                 // (false for NaN: refused below)
    if (!log_sigma2 || !s2_out || (n_b > 0 && (!rho_b || !s2_b))) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (threshold != threshold) { set_error("%s: threshold is NaN", who); return BNN_E_RANGE; }
    if ((mask || theta_out) && !theta) { set_error("%s: NULL theta", who); return BNN_E_NULL; }
    if (mask && (!theta_out || !count_out)) { set_error("%s: a finite threshold needs theta_out and count_out", who); return BNN_E_NULL; }
    if (n_w < 1 || n_b < 0) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (misaligned(theta, 3) || misaligned(log_sigma2, 3) || misaligned(rho_b, 3) || misaligned(s2_b, 3) || misaligned(theta_out, 3) ||
        misaligned(s2_out, 3) || misaligned(count_out, 7)) {
        set_error("%s: misaligned pointer (count_out: 8 bytes)", who);
        return BNN_E_ALIGN;
    }
    int64_t blocks = (n_w + n_b + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipStream_t st = (hipStream_t)stream;
    if (mask) {
        const int rc = (int)hipMemsetAsync(count_out, 0, 8, st);
        if (rc) { set_error("%s: hipMemsetAsync failed (%d)", who, rc); return rc; }
        hipLaunchKernelGGL(k_vd_prepare<true>, dim3((unsigned)blocks), dim3(256), 0, st, theta, log_sigma2, n_w, rho_b, s2_b, n_b,
                           threshold, theta_out, s2_out, reinterpret_cast<unsigned long long *>(count_out));
    } else {
        hipLaunchKernelGGL(k_vd_prepare<false>, dim3((unsigned)blocks), dim3(256), 0, st, theta, log_sigma2, n_w, rho_b, s2_b, n_b,
                           threshold, theta_out, s2_out, (unsigned long long *)nullptr);
    }
    return check_launch(who);
}

// K10's weight gradient with this posterior's chain factor: lrt_backward_weight (bnn_lrt.hip) is the whole entry -- the checks,
// k_lrt<T, LRT_WGRAD, ChainLogSigma2> and the bias sums; g_theta has bnn_lrt_backward_weight's g_mu_w bits on the same x, g_m, g_v.
// ChainLogSigma2 (bnn_device.hpp) is the chain factor of K24's slab reduce as well: where log_sigma2 < -87, expf a denormal,
// g_log_sigma2 is the fp64 product rounded once (this entry multiplied by the denormal expf before it shared that code).
int bnn_vd_backward_weight(const void *x, int64_t ldx, const float *g_m, const float *g_v, const float *log_sigma2, float *g_theta,
                           float *g_log_sigma2, const float *rho_b, float *g_mu_b, float *g_rho_b, int64_t M, int64_t N, int64_t K,
                           int compute, int flags, void *stream)
{
    return lrt_backward_weight<ChainLogSigma2>("bnn_vd_backward_weight", x, ldx, g_m, g_v, log_sigma2, g_theta, g_log_sigma2, rho_b,
                                               g_mu_b, g_rho_b, M, N, K, compute, flags, (hipStream_t)stream);
}

int64_t bnn_vd_kl_workspace_bytes(const bnn_vd_tensor_t *tensors, int ntensors)
{
    if (!tensors || ntensors < 1 || ntensors > kKlMaxTensors) return -1;
    int64_t blocks = 0;
    for (int t = 0; t < ntensors; ++t) {
        if (tensors[t].n < 1) return -1;
        blocks += vd_chunks(tensors[t].n);
    }
    return blocks > 0x7FFFFFFF ? -1 : 8 * blocks;
}

int bnn_vd_kl_forward(const bnn_vd_tensor_t *tensors, int ntensors, float *out, void *workspace, void *stream)
{
    const char *who = "bnn_vd_kl_forward";
    int rc = vd_validate(tensors, ntensors, who);
    if (rc) return rc;
    if (!out || !workspace) { set_error("%s: NULL out / workspace", who); return BNN_E_NULL; }
    if (misaligned(out, 3) || misaligned(workspace, 7)) { set_error("%s: misaligned out / workspace (8 bytes)", who); return BNN_E_ALIGN; }
    hipStream_t st = (hipStream_t)stream;
    double *partials = reinterpret_cast<double *>(workspace);
    VdFinal F{};
    F.ntensors = ntensors;
    int32_t pbase = 0;
    for (int g0 = 0; g0 < ntensors; g0 += kKlMaxPerLaunch) {
        VdLaunch L{};
        const int cnt = ntensors - g0 < kKlMaxPerLaunch ? ntensors - g0 : kKlMaxPerLaunch;
        L.ntensors = cnt;
        L.partial_base = pbase;
        int32_t blocks = 0;
        for (int i = 0; i < cnt; ++i) {
            const bnn_vd_tensor_t &s = tensors[g0 + i];
            L.t[i].theta = s.theta; L.t[i].ls2 = s.log_sigma2; L.t[i].n = s.n;
            L.t[i].first_block = blocks; L.t[i].index = g0 + i;
            F.first[g0 + i] = pbase + blocks;
            blocks += (int32_t)vd_chunks(s.n);
        }
        hipLaunchKernelGGL(k_vd_kl_partial, dim3((unsigned)blocks), dim3(kKlThreads), 0, st, L, partials);
        rc = check_launch(who);
        if (rc) return rc;
        pbase += blocks;
    }
    F.first[ntensors] = pbase;
    hipLaunchKernelGGL(k_vd_kl_final, dim3(1), dim3(kKlThreads), 0, st, F, partials, out);
    return check_launch(who);
}

int bnn_vd_kl_backward(const bnn_vd_tensor_t *tensors, int ntensors, const float *upstream, float *const *g_theta,
                       float *const *g_log_sigma2, int accumulate, void *stream)
{
    const char *who = "bnn_vd_kl_backward";
    int rc = vd_validate(tensors, ntensors, who);
    if (rc) return rc;
    if (!upstream || !g_theta || !g_log_sigma2) { set_error("%s: NULL upstream / gradient lists", who); return BNN_E_NULL; }
    if (misaligned(upstream, 3)) { set_error("%s: misaligned upstream", who); return BNN_E_ALIGN; }
    for (int t = 0; t < ntensors; ++t) {
        if (!g_theta[t] || !g_log_sigma2[t]) { set_error("%s: tensor %d NULL gradient", who, t); return BNN_E_NULL; }
        if (misaligned(g_theta[t], 3) || misaligned(g_log_sigma2[t], 3)) { set_error("%s: tensor %d misaligned gradient", who, t); return BNN_E_ALIGN; }
    }
    hipStream_t st = (hipStream_t)stream;
    for (int g0 = 0; g0 < ntensors; g0 += kKlMaxPerLaunch) {
        VdLaunch L{};
        const int cnt = ntensors - g0 < kKlMaxPerLaunch ? ntensors - g0 : kKlMaxPerLaunch;
        L.ntensors = cnt;
        int32_t blocks = 0;
        for (int i = 0; i < cnt; ++i) {
            const bnn_vd_tensor_t &s = tensors[g0 + i];
            L.t[i].theta = s.theta; L.t[i].ls2 = s.log_sigma2; L.t[i].n = s.n;
            L.t[i].g_theta = g_theta[g0 + i]; L.t[i].g_ls2 = g_log_sigma2[g0 + i];
            L.t[i].first_block = blocks; L.t[i].index = g0 + i;
            blocks += (int32_t)vd_chunks(s.n);
        }
        hipLaunchKernelGGL(k_vd_kl_backward, dim3((unsigned)blocks), dim3(kKlThreads), 0, st, L, upstream, accumulate);
        rc = check_launch(who);
        if (rc) return rc;
    }
    return BNN_OK;
}

}  // extern "C"
