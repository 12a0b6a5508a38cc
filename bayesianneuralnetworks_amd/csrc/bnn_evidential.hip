// bnn_evidential.hip -- K13: evidential regression (Amini et al. 2020, "Deep Evidential Regression"): the Normal-Inverse-Gamma
// head's activation, its loss with all four gradients in one pass, and the MC-mixture uncertainty of S such heads.
//   replaces  NormalInverseGaussianLinear's split / softplus / offsets (pytorch_bayesian/nn/dense.py:141-162),
//             NormalInverseGaussianLoss.forward and its autograd (nn/loss.py:54-69),
//             NormalInverseGaussianUncertainty (nn/loss.py:72-79) over the samples of a Bayesian trunk.
//
// bnn_nig_head_forward / _backward: z (rows, 4 D) -> gamma | 1e-10 + softplus | 1 + 1e-10 + softplus | 1e-10 + softplus, four
// contiguous (rows, D) tensors, one launch each way.  Softplus is torch's (beta 1, threshold 20) on the accurate log1pf(expf())
// of K10 / K11.  A workgroup is (TR rows) x (TD lanes along the 4 D columns); the segment of a column comes from three compares,
// so there is no index division; with D % 4 == 0 and 16-B aligned pointers a lane moves four columns per access.
//
// bnn_nig_loss: with r = y - gamma, omega = 2 beta (1 + upsilon), A = upsilon r^2 + omega, x = upsilon r^2 / omega:
//   term    = 0.5 ln(pi / upsilon) + alpha log1p(x) + 0.5 ln A + [lgamma(alpha) - lgamma(alpha + 0.5)] + lambda |r| (2 upsilon + alpha)
//   g_gamma = -2 (alpha + 0.5) upsilon r / A - lambda sign(r) (2 upsilon + alpha)                     (sign(0) = 0, as torch.abs)
//   g_ups   = -0.5 / upsilon + alpha r^2 / (A (1 + upsilon)) + 0.5 (r^2 + 2 beta) / A + 2 lambda |r|
//   g_alpha = log1p(x) + [psi(alpha) - psi(alpha + 0.5)] + lambda |r|
//   g_beta  = (1 + upsilon) / A - alpha upsilon r^2 / (beta A)
// each over n.  These are the reference's -alpha ln omega + (alpha + 0.5) ln A and its derivatives with the parts that are
// proportional to alpha and cancel taken out by hand.  The two bracketed differences cancel ~alpha ln alpha / 0.5 ln alpha and
// ~2 alpha ln alpha digits: every element is evaluated in fp64 (lgamma from the device library, digamma below), which leaves
// them > 9 digits at alpha = 1e6.  At the example's shape (128 elements) the launches decide; at 4 M elements the fp64
// evaluation, not memory, bounds the kernel (DESIGN.md section 4 K13 has the measured times).
// Per-thread sums fp64, one partial per workgroup, k_nig_loss_final adds them in a fixed order: bitwise reproducible.
//
// bnn_mc_evidential: the moments of the equal-weight mixture of S NIG heads over a leading MC axis (law of total variance), with
// a_s = beta / (alpha - 1), e_s = a_s / upsilon in fp32 exactly as the module computes them:
//   mean = (1/S) sum gamma_s,  aleatoric = (1/S) sum a_s,  epistemic = (1/S) sum e_s + Var_s(gamma_s),  total = their sum.
// Var_s(gamma_s) as in bnn_mc_regression: on gamma_s - gamma_0, fp64, clamped at 0; the two work splits and their launch shapes
// are bnn_mc_parts.hpp's (narrow: lane = (row, sample), G lanes a row, a fixed xor tree; wide: a lane owns 4-quantity chunks
// over all samples in order).
#include "bnn_mc_parts.hpp"

namespace bnn {

// ---------------------------------------------------------------------------------------------- the head
constexpr int kNigThreads = 256;
constexpr int kNigHeadMaxBlocks = 2048;     // row tiles per launch (grid-stride above)

__device__ __forceinline__ float nig_act(float z, int seg)
{
    if (seg == 0) return z;
    const float sp = z > 20.0f ? z : log1pf(expf(z));
    return seg == 2 ? sp + 1.0f : sp + 1e-10f;             // alpha: torch adds the Python scalar 1 + 1e-10, which is 1.0f
}

// CPL columns per lane (1, or 4 with 16-B accesses when D % 4 == 0); W = 4 D columns; a lane's columns lie in one segment.
template <int CPL>
__global__ __launch_bounds__(kNigThreads) void k_nig_head_fwd(const float *__restrict__ z, int64_t rows, int D, int tdlog,
                                                              float *__restrict__ o0, float *__restrict__ o1,
                                                              float *__restrict__ o2, float *__restrict__ o3)
{
    const int TD = 1 << tdlog, TR = kNigThreads >> tdlog;
    const int td = (int)threadIdx.x & (TD - 1), tr = (int)threadIdx.x >> tdlog;
    const int W = 4 * D;
    for (int64_t r = (int64_t)blockIdx.x * TR + tr; r < rows; r += (int64_t)gridDim.x * TR) {
        const float *zr = z + r * W;
        for (int c = td * CPL; c < W; c += TD * CPL) {
            const int seg = (c >= D) + (c >= 2 * D) + (c >= 3 * D);
            float *o = seg == 0 ? o0 : seg == 1 ? o1 : seg == 2 ? o2 : o3;
            o += r * D + (c - seg * D);
            if constexpr (CPL == 4) {
                const float4 v = *reinterpret_cast<const float4 *>(zr + c);
                *reinterpret_cast<float4 *>(o) = make_float4(nig_act(v.x, seg), nig_act(v.y, seg), nig_act(v.z, seg), nig_act(v.w, seg));
            } else {
                o[0] = nig_act(zr[c], seg);
            }
        }
    }
}

template <int CPL>
__global__ __launch_bounds__(kNigThreads) void k_nig_head_bwd(const float *__restrict__ z, const float *__restrict__ g0,
                                                              const float *__restrict__ g1, const float *__restrict__ g2,
                                                              const float *__restrict__ g3, int64_t rows, int D, int tdlog,
                                                              float *__restrict__ gz)
{
    const int TD = 1 << tdlog, TR = kNigThreads >> tdlog;
    const int td = (int)threadIdx.x & (TD - 1), tr = (int)threadIdx.x >> tdlog;
    const int W = 4 * D;
    for (int64_t r = (int64_t)blockIdx.x * TR + tr; r < rows; r += (int64_t)gridDim.x * TR) {
        for (int c = td * CPL; c < W; c += TD * CPL) {
            const int seg = (c >= D) + (c >= 2 * D) + (c >= 3 * D);
            const float *g = seg == 0 ? g0 : seg == 1 ? g1 : seg == 2 ? g2 : g3;
            const int64_t at = r * W + c;
            if constexpr (CPL == 4) {
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (g) {
                    o = *reinterpret_cast<const float4 *>(g + r * D + (c - seg * D));
                    if (seg) {
                        const float4 v = *reinterpret_cast<const float4 *>(z + at);
                        o.x *= dsigma_lrt(v.x); o.y *= dsigma_lrt(v.y); o.z *= dsigma_lrt(v.z); o.w *= dsigma_lrt(v.w);
                    }
                }
                *reinterpret_cast<float4 *>(gz + at) = o;
            } else {
                float o = 0.f;
                if (g) {
                    o = g[r * D + (c - seg * D)];
                    if (seg) o *= dsigma_lrt(z[at]);
                }
                gz[at] = o;
            }
        }
    }
}

struct NigHeadPlan { int tdlog, grid; };

static NigHeadPlan nig_head_plan(int64_t rows, int D, int cpl)
{
    NigHeadPlan P{};
    const int lanes = 4 * D / cpl;                          // lanes a row can use
    while ((1 << P.tdlog) < lanes && P.tdlog < 8) ++P.tdlog;
    const int TR = kNigThreads >> P.tdlog;
    const int64_t tiles = (rows + TR - 1) / TR;
    P.grid = (int)(tiles < kNigHeadMaxBlocks ? tiles : kNigHeadMaxBlocks);
    return P;
}

static int nig_head_check(const char *who, int64_t rows, int D)
{
    if (rows < 1 || D < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (D > 4096) { set_error("%s: D above 4096", who); return BNN_E_RANGE; }
    if (rows > 0x7FFFFFFF) { set_error("%s: more than 2^31 - 1 rows", who); return BNN_E_RANGE; }
    return BNN_OK;
}

// ---------------------------------------------------------------------------------------------- the loss
constexpr int kNigLossMaxBlocks = 1024;     // workgroups per launch = fp64 partials in the workspace (grid-stride above)
constexpr double kPi = 3.14159265358979323846;

// psi(x), x > 0: upward recurrence psi(x) = psi(x + 1) - 1 / x to an argument >= 6, then the asymptotic series
// ln x - 1/(2x) - sum B_2k / (2k x^2k) through x^-14 (the first term left out, 3617 / (8160 x^16), is < 2e-13 at x = 6).
__device__ __forceinline__ double digamma_f64(double x)
{
    if (!(x > 0.0)) return __builtin_nan("");                // (also bounds the recurrence: at most six steps)
    double acc = 0.0;
    while (x < 6.0) {
        acc -= 1.0 / x;
        x += 1.0;
    }
    const double i = 1.0 / x, i2 = i * i;
    double s = -1.0 / 12.0;
    s = __builtin_fma(s, i2, 691.0 / 32760.0);
    s = __builtin_fma(s, i2, -1.0 / 132.0);
    s = __builtin_fma(s, i2, 1.0 / 240.0);
    s = __builtin_fma(s, i2, -1.0 / 252.0);
    s = __builtin_fma(s, i2, 1.0 / 120.0);
    s = __builtin_fma(s, i2, -1.0 / 12.0);
    return acc + (log(x) - 0.5 * i + s * i2);
}

__global__ __launch_bounds__(kNigThreads) void k_nig_loss(const float *__restrict__ gamma, const float *__restrict__ upsilon,
                                                          const float *__restrict__ alpha, const float *__restrict__ beta,
                                                          const float *__restrict__ y, int64_t n, double lambda, double inv_n,
                                                          float *__restrict__ g_gamma, float *__restrict__ g_upsilon,
                                                          float *__restrict__ g_alpha, float *__restrict__ g_beta,
                                                          double *__restrict__ partial)
{
    __shared__ double red[kNigThreads / 64];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kNigThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNigThreads) {
        const double g = gamma[i], u = upsilon[i], a = alpha[i], b = beta[i];
        const double r = (double)y[i] - g;
        const double r2 = r * r, ar = fabs(r);
        const double omega = 2.0 * b * (1.0 + u);
        const double A = __builtin_fma(u, r2, omega);
        const double l1p = log1p(u * r2 / omega);
        const double evid = 2.0 * u + a;
        acc += 0.5 * log(kPi / u) + a * l1p + 0.5 * log(A) + (lgamma(a) - lgamma(a + 0.5)) + lambda * ar * evid;
        const double iA = 1.0 / A;
        if (g_gamma) {
            const double sg = r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0);
            g_gamma[i] = (float)((-2.0 * (a + 0.5) * u * r * iA - lambda * sg * evid) * inv_n);
        }
        if (g_upsilon)
            g_upsilon[i] = (float)((-0.5 / u + a * r2 * iA / (1.0 + u) + 0.5 * (r2 + 2.0 * b) * iA + 2.0 * lambda * ar) * inv_n);
        if (g_alpha) g_alpha[i] = (float)((l1p + (digamma_f64(a) - digamma_f64(a + 0.5)) + lambda * ar) * inv_n);
        if (g_beta) g_beta[i] = (float)(((1.0 + u) * iA - a * u * r2 * iA / b) * inv_n);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kNigThreads) void k_nig_loss_final(const double *__restrict__ partial, int nparts, double inv_n,
                                                                float *__restrict__ loss)
{
    __shared__ double red[kNigThreads / 64];
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kNigThreads) a += partial[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_n);
}

// workgroups of the main launch: a function of n alone, so that the workspace query and the launch agree
static int nig_loss_blocks(int64_t n)
{
    const int64_t b = (n + kNigThreads - 1) / kNigThreads;
    return (int)(b < kNigLossMaxBlocks ? b : kNigLossMaxBlocks);
}

// ---------------------------------------------------------------------------------------------- the MC mixture
struct EviArgs {
    const float *gamma, *upsilon, *alpha, *beta;
    int64_t stride;         // elements between samples
    int64_t rows;
    int nsamples, D;
    int vec;                // wide split: 16-B loads / stores are aligned
    float *mean, *total, *aleatoric, *epistemic;
};

struct EviSums { double sd, sd2, sa, se; };

// one sample's contribution of one quantity: the head's own (aleatoric, epistemic) in fp32 as the module computes them, and
// d = gamma - gamma_0 in fp64
__device__ __forceinline__ void evi_acc(float g, float ref, float u, float a, float b, EviSums &s)
{
    const float al = b / (a - 1.0f);
    const float ep = al / u;
    const double d = (double)g - (double)ref;
    s.sd += d;
    s.sd2 = __builtin_fma(d, d, s.sd2);
    s.sa += (double)al;
    s.se += (double)ep;
}

__device__ __forceinline__ Moments evi_finish(float ref, const EviSums &s, double inv_S)
{
    const double md = s.sd * inv_S;
    double var = __builtin_fma(-md, md, s.sd2 * inv_S);
    var = var > 0.0 ? var : 0.0;
    const double ale = s.sa * inv_S;
    const double epi = s.se * inv_S + var;
    Moments o;
    o.mean = (float)((double)ref + md);
    o.total = (float)(ale + epi);
    o.ale = (float)ale;
    o.epi = (float)epi;
    return o;
}

// narrow (D <= 16): lane = (row, sl), sl = lane & (G - 1) takes samples sl, sl + G, ...; NV >= D value slots per lane.
template <int NV>
__global__ __launch_bounds__(kUncThreads) void k_evi_narrow(EviArgs A, int glog, int rpb)
{
    const NarrowLane L(glog, rpb);
    const int G = L.G, sl = L.sl;
    const int D = A.D, S = A.nsamples;
    const double inv_S = 1.0 / (double)S;
    for (int64_t rb = blockIdx.x; rb * rpb < A.rows; rb += gridDim.x) {
        const int64_t r = rb * rpb + L.lr;
        const bool live = L.live(r, A.rows);
        const bool work = live && sl < S;
        // sample 0's gamma: lane sl == 0 of the group loads it; every lane of the wave takes part in the shuffle
        float ref[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float g0 = (live && sl == 0 && i < D) ? A.gamma[r * D + i] : 0.f;
            ref[i] = __shfl(g0, L.lead, 64);
        }
        EviSums sum[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) sum[i] = EviSums{0.0, 0.0, 0.0, 0.0};
        if (work) {
            for (int s = sl; s < S; s += G) {
                const int64_t at = (int64_t)s * A.stride + r * D;
                float g[NV], u[NV], a[NV], b[NV];
#pragma unroll
                for (int i = 0; i < NV; ++i)
                    if (i < D) { g[i] = A.gamma[at + i]; u[i] = A.upsilon[at + i]; a[i] = A.alpha[at + i]; b[i] = A.beta[at + i]; }
#pragma unroll
                for (int i = 0; i < NV; ++i)
                    if (i < D) evi_acc(g[i], ref[i], u[i], a[i], b[i], sum[i]);
            }
        }
        // the G lanes of a row: a fixed xor tree (every lane of the group ends with the same bits)
        for (int o = 1; o < G; o <<= 1) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (i < D) {
                    sum[i].sd += __shfl_xor(sum[i].sd, o, 64);
                    sum[i].sd2 += __shfl_xor(sum[i].sd2, o, 64);
                    sum[i].sa += __shfl_xor(sum[i].sa, o, 64);
                    sum[i].se += __shfl_xor(sum[i].se, o, 64);
                }
        }
        if (live && sl == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (i < D) store_moments(A, r * D + i, evi_finish(ref[i], sum[i], inv_S));
        }
    }
}

// wide (16 < D <= 4096): TPR threads per row (64: a wave, four rows per workgroup; 256: the workgroup), NCH 4-quantity chunks
// per thread, chunk k of thread t at quantities 4 (t + k TPR) .. + 3; all samples in sample order, no reduction across lanes.
template <int TPR, int NCH>
__global__ __launch_bounds__(kUncThreads) void k_evi_wide(EviArgs A)
{
    constexpr int NV = 4 * NCH;
    constexpr int RPB = kUncThreads / TPR;
    const int t = (int)threadIdx.x % TPR;
    const int D = A.D, S = A.nsamples;
    const double inv_S = 1.0 / (double)S;
    for (int64_t rb = blockIdx.x; rb * RPB < A.rows; rb += gridDim.x) {
        const int64_t r = rb * RPB + (int)threadIdx.x / TPR;
        if (r >= A.rows) continue;
        const int64_t o0 = r * D;
        // pad: what a slot outside the row holds (a finite head: aleatoric 0)
        auto load4 = [&](const float *q, float pad, float (&v)[NV]) { row_load<NV, TPR>(q, D, A.vec, t, pad, v); };
        float ref[NV];
        load4(A.gamma + o0, 0.f, ref);
        EviSums sum[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) sum[i] = EviSums{0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < S; ++s) {
            const int64_t at = (int64_t)s * A.stride + o0;
            float g[NV], u[NV], a[NV], b[NV];
            load4(A.gamma + at, 0.f, g);
            load4(A.upsilon + at, 1.f, u);
            load4(A.alpha + at, 2.f, a);
            load4(A.beta + at, 0.f, b);
#pragma unroll
            for (int i = 0; i < NV; ++i) evi_acc(g[i], ref[i], u[i], a[i], b[i], sum[i]);
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            Moments o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = evi_finish(ref[4 * k + j], sum[4 * k + j], inv_S);
            store_moments4(A, o0, 4 * (t + k * TPR), D, o);
        }
    }
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_nig_head_forward(const float *z, int64_t rows, int D, float *gamma, float *upsilon, float *alpha, float *beta,
                         void *stream)
{
    const char *who = "bnn_nig_head_forward";
    if (!z || !gamma || !upsilon || !alpha || !beta) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    const int rc = nig_head_check(who, rows, D);
    if (rc) return rc;
    const bool vec = D % 4 == 0 && al16(z) && al16(gamma) && al16(upsilon) && al16(alpha) && al16(beta);
    const NigHeadPlan P = nig_head_plan(rows, D, vec ? 4 : 1);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(k_nig_head_fwd<4>, dim3((unsigned)P.grid), dim3(kNigThreads), 0, st, z, rows, D, P.tdlog, gamma, upsilon,
                           alpha, beta);
    else
        hipLaunchKernelGGL(k_nig_head_fwd<1>, dim3((unsigned)P.grid), dim3(kNigThreads), 0, st, z, rows, D, P.tdlog, gamma, upsilon,
                           alpha, beta);
    return check_launch(who);
}

int bnn_nig_head_backward(const float *z, const float *g_gamma, const float *g_upsilon, const float *g_alpha,
                          const float *g_beta, int64_t rows, int D, float *g_z, void *stream)
{
    const char *who = "bnn_nig_head_backward";
    if (!z || !g_z) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    const int rc = nig_head_check(who, rows, D);
    if (rc) return rc;
    const bool vec = D % 4 == 0 && al16(z) && al16(g_z) && al16(g_gamma) && al16(g_upsilon) && al16(g_alpha) && al16(g_beta);
    const NigHeadPlan P = nig_head_plan(rows, D, vec ? 4 : 1);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(k_nig_head_bwd<4>, dim3((unsigned)P.grid), dim3(kNigThreads), 0, st, z, g_gamma, g_upsilon, g_alpha,
                           g_beta, rows, D, P.tdlog, g_z);
    else
        hipLaunchKernelGGL(k_nig_head_bwd<1>, dim3((unsigned)P.grid), dim3(kNigThreads), 0, st, z, g_gamma, g_upsilon, g_alpha,
                           g_beta, rows, D, P.tdlog, g_z);
    return check_launch(who);
}

int64_t bnn_nig_loss_workspace_bytes(int64_t n)
{
    if (n < 1) { set_error("bnn_nig_loss_workspace_bytes: bad extent"); return 0; }
    return 8 * (int64_t)nig_loss_blocks(n);
}

int bnn_nig_loss(const float *gamma, const float *upsilon, const float *alpha, const float *beta, const float *y, int64_t n,
                 double reg_lambda, float *loss, float *g_gamma, float *g_upsilon, float *g_alpha, float *g_beta,
                 void *workspace, void *stream)
{
    const char *who = "bnn_nig_loss";
    if (!gamma || !upsilon || !alpha || !beta || !y || !loss || !workspace) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (n < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) { set_error("%s: workspace not 8-byte aligned", who); return BNN_E_ALIGN; }
    const int blocks = nig_loss_blocks(n);
    const double inv_n = 1.0 / (double)n;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nig_loss, dim3((unsigned)blocks), dim3(kNigThreads), 0, st, gamma, upsilon, alpha, beta, y, n,
                       reg_lambda, inv_n, g_gamma, g_upsilon, g_alpha, g_beta, reinterpret_cast<double *>(workspace));
    const int rc = check_launch(who);
    if (rc) return rc;
    hipLaunchKernelGGL(k_nig_loss_final, dim3(1), dim3(kNigThreads), 0, st, reinterpret_cast<const double *>(workspace), blocks,
                       inv_n, loss);
    return check_launch(who);
}

int bnn_mc_evidential(const float *gamma, const float *upsilon, const float *alpha, const float *beta, int64_t sample_stride,
                      int nsamples, int64_t rows, int D, float *mean, float *total, float *aleatoric, float *epistemic,
                      void *stream)
{
    const TailNames N{"bnn_mc_evidential", "D above 4096", "sample_stride below rows * D"};
    if (!gamma || !upsilon || !alpha || !beta || !mean || !total || !aleatoric || !epistemic) {
        set_error("%s: NULL pointer", N.who);
        return BNN_E_NULL;
    }
    int rc = tail_check_extents(N, 1, nsamples, rows, D);
    if (!rc) rc = tail_check_stride(N, nsamples, sample_stride, rows, D);
    if (rc) return rc;
    EviArgs A{};
    A.gamma = gamma; A.upsilon = upsilon; A.alpha = alpha; A.beta = beta;
    A.stride = sample_stride;
    A.rows = rows;
    A.nsamples = nsamples;
    A.D = D;
    A.vec = tail_vec(D, nsamples, sample_stride, {gamma, upsilon, alpha, beta, mean, total, aleatoric, epistemic});
    A.mean = mean; A.total = total; A.aleatoric = aleatoric; A.epistemic = epistemic;
    hipStream_t st = (hipStream_t)stream;
    if (D <= kUncNarrow) {
        const NarrowPlan P = narrow_plan(nsamples, rows, 0);
        if (D == 1) hipLaunchKernelGGL(k_evi_narrow<1>, P.grid, dim3(kUncThreads), 0, st, A, P.glog, P.rpb);
        else if (D <= 4) hipLaunchKernelGGL(k_evi_narrow<4>, P.grid, dim3(kUncThreads), 0, st, A, P.glog, P.rpb);
        else hipLaunchKernelGGL(k_evi_narrow<kUncNarrow>, P.grid, dim3(kUncThreads), 0, st, A, P.glog, P.rpb);
        return check_launch(N.who);
    }
    const WidePlan P = wide_plan(D, D, rows, 0);
    wide_dispatch(P, [&](auto T, auto NC) {
        hipLaunchKernelGGL((k_evi_wide<T.value, NC.value>), P.grid, dim3(kUncThreads), 0, st, A);
    });
    return check_launch(N.who);
}

}  // extern "C"
