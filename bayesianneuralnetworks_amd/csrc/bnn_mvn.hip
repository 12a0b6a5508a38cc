// bnn_mvn.hip -- the full-covariance posterior (WeightMultivariateNormal, MultivariateNormalLinear) on the MC-batched path:
// the keyed draw of all S samples, its backward with the uniforms re-created from the key, and the closed-form KL against an
// isotropic prior with its backward (MVN contract, include/bnn_hip.h).
//
// Work split, every kernel: a workgroup owns (tensor, row o, part p); wave w of part p takes the triangle rows
// i = p + P (w + 4 t), and its lanes stride the columns j of row i four at a time (lane l: j = 4 l + 256 c .. + 3).  Which
// lane adds which column, and the xor-butterfly over the lanes, depend on K alone -- so a drawn value does not depend on S,
// sample0, P or the grid.  Only the lower triangle of `scale` is read.
#include <cmath>

#include "bnn_mvn_dev.hpp"

namespace bnn {

constexpr int kMvnThreads = 256;
constexpr int kMvnWaves = kMvnThreads / 64;
constexpr int kMvnMaxTensors = 8;
constexpr int kMvnLdsBytes = 64 * 1024;     // dynamic LDS per workgroup: the draw's uniforms, the backward's uniforms + g_w rows
constexpr int kMvnMaxSamplesPerPass = 16;
constexpr int kMvnTargetBlocks = 2048;      // parts per row: about 8 workgroups per CU over the whole launch

// mvn_softplus / mvn_v / mvn_l (bnn_mvn_dev.hpp): the draw, its backward and the KL all take L or V from THOSE functions.

struct MvnDev {
    const float *mu, *scale;
    float *out;
    const float *g_w;
    float *g_mu, *g_scale;
    int64_t ss;                 // sample stride of out / g_w (elements)
    uint32_t rows, cols, parts, vec;
    RngDev rng;
};

struct MvnLaunch {
    MvnDev t[kMvnMaxTensors];
    uint32_t block0[kMvnMaxTensors + 1];
    int n, S, sc;               // tensors, samples, samples per pass
};

struct MvnKlDev {
    const float *mu, *scale;
    float *g_mu, *g_scale;
    uint32_t rows, cols, parts, vec;
    float m0, inv_var, ln_sigma;
    uint32_t ws0;               // first workspace slot of this tensor's partial sums
};

struct MvnKlLaunch {
    MvnKlDev t[kMvnMaxTensors];
    uint32_t block0[kMvnMaxTensors + 1];
    int n;
    double *ws;
    float *out;
    const float *up;
};

template <typename D>
__device__ __forceinline__ int mvn_tensor_of(const D *t, const uint32_t *block0, int n)
{
    int k = 0;
    while (k + 1 < n && blockIdx.x >= block0[k + 1]) ++k;
    return k;
}

// four consecutive lower-triangle values of row `srow` from column j0 (j0 <= i), zero beyond i (and beyond K)
__device__ __forceinline__ void mvn_load4(const float *srow, uint32_t j0, uint32_t i, uint32_t K, bool vec, float (&v)[4])
{
    if (vec) {      // K % 4 == 0 and a 16-B aligned tensor: j0 + 3 < K
        const float4 q = *reinterpret_cast<const float4 *>(srow + j0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (j0 + k <= i) ? srow[j0 + k] : 0.f;
    }
    (void)K;
}

// The next sample's row of an LDS block: the address stays one VGPR stepped by the pitch (without the empty asm the compiler
// keeps one SGPR offset per unrolled sample, and the 8- and 16-sample kernels spill SGPRs)
__device__ __forceinline__ const float *mvn_next_row(const float *q, uint32_t pitch)
{
    q += pitch;
    asm volatile("" : "+v"(q));
    return q;
}

// The uniforms u_s[o][j] of samples c0 .. c0 + ns - 1 into lds[s * Kp + j]; columns K .. Kp - 1 and the rows ns .. nrows - 1
// zero, so that the unrolled sample loops need no per-sample predicate (a zero row adds fma(g, 0, a) = a)
__device__ __forceinline__ void mvn_fill_u(float *lds, const RngDev &rng, uint32_t ed, uint32_t o, uint32_t K, uint32_t Kp,
                                           int c0, int ns, int nrows)
{
    const uint32_t e0 = o * K;
    const uint32_t q0 = e0 >> 2, nq = ((e0 + K - 1) >> 2) - q0 + 1;
    for (uint32_t idx = threadIdx.x; idx < nq * (uint32_t)ns; idx += kMvnThreads) {
        const uint32_t s = idx / nq, q = q0 + (idx - s * nq);
        const float4 u = drop_u4(rng, ed, q, rng.sample0 + (uint32_t)c0 + s);
        const float uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t e = 4u * q + (uint32_t)k;
            if (e >= e0 && e - e0 < K) lds[s * Kp + (e - e0)] = uu[k];
        }
    }
    const uint32_t pad = Kp - K;
    for (uint32_t idx = threadIdx.x; idx < pad * (uint32_t)ns; idx += kMvnThreads)
        lds[(idx / pad) * Kp + K + idx % pad] = 0.f;
    for (uint32_t idx = threadIdx.x; idx < (uint32_t)(nrows - ns) * Kp; idx += kMvnThreads) lds[(uint32_t)ns * Kp + idx] = 0.f;
}

// The sum over the 64 lanes of acc[s] for every s at once: the first log2 NS levels of the xor butterfly exchange half of the
// remaining samples (a lane keeps one half, its partner the other), the rest are plain butterfly levels -- NS - 1 + 6 - log2 NS
// shuffles instead of 6 NS.  Every sample's tree is the butterfly's (pairs at xor 32, then 16, ...), so the value is the same
// bits for any NS.  -> sample lane >> (6 - log2 NS), complete in the lanes whose low 6 - log2 NS bits are zero.
template <int NS>
__device__ __forceinline__ float mvn_lane_sums(float (&acc)[NS], uint32_t lane)
{
    constexpr int LG = NS == 1 ? 0 : NS == 2 ? 1 : NS == 4 ? 2 : NS == 8 ? 3 : 4;
    static_assert((1 << LG) == NS, "NS: 1, 2, 4, 8 or 16");
#pragma unroll
    for (int t = 0; t < LG; ++t) {
        const int n = NS >> t, o = 32 >> t;
        const bool hi = (lane & (uint32_t)o) != 0;
#pragma unroll
        for (int k = 0; k < n / 2; ++k) {
            const float send = hi ? acc[k] : acc[k + n / 2];
            const float keep = hi ? acc[k + n / 2] : acc[k];
            acc[k] = keep + __shfl_xor(send, o, 64);
        }
    }
    float v = acc[0];
#pragma unroll
    for (int o = 32 >> LG; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// w_s[o][i] = mu[o][i] + sum_{j <= i} L[o][i][j] u_s[o][j], every tensor of the launch, every sample
template <int NS>
__global__ __launch_bounds__(kMvnThreads) void k_mvn_draw(MvnLaunch P)
{
    extern __shared__ __attribute__((aligned(16))) float u_lds[];
    const int t = mvn_tensor_of(P.t, P.block0, P.n);
    const MvnDev &d = P.t[t];
    const uint32_t b = blockIdx.x - P.block0[t];
    const uint32_t o = b / d.parts, p = b - o * d.parts;
    const uint32_t K = d.cols, Kp = (K + 3u) & ~3u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ed = rng_epoch_dev(d.rng);
    const float *sbase = d.scale + (int64_t)o * K * K;
    const float *mrow = d.mu + (int64_t)o * K;
    const bool vec = d.vec != 0;
    for (int c0 = 0; c0 < P.S; c0 += P.sc) {
        const int ns = min(P.sc, P.S - c0);
        __syncthreads();
        mvn_fill_u(u_lds, d.rng, ed, o, K, Kp, c0, ns, NS);
        __syncthreads();
        for (uint32_t i = p + d.parts * wave; i < K; i += d.parts * kMvnWaves) {
            const float *srow = sbase + (int64_t)i * K;
            float acc[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] = 0.f;
            for (uint32_t j0 = 4u * lane; j0 <= i; j0 += 256u) {
                float v[4];
                mvn_load4(srow, j0, i, K, vec, v);
                float l[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) l[k] = (j0 + k <= i) ? mvn_l(v[k], j0 + k == i) : 0.f;
                const float *uq = u_lds + j0;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float4 u = *reinterpret_cast<const float4 *>(uq);
                    uq = mvn_next_row(uq, Kp);
                    acc[s] = __builtin_fmaf(l[0], u.x, acc[s]);
                    acc[s] = __builtin_fmaf(l[1], u.y, acc[s]);
                    acc[s] = __builtin_fmaf(l[2], u.z, acc[s]);
                    acc[s] = __builtin_fmaf(l[3], u.w, acc[s]);
                }
            }
            const float r = mvn_lane_sums<NS>(acc, lane);
            constexpr uint32_t kSh = NS == 1 ? 6 : NS == 2 ? 5 : NS == 4 ? 4 : NS == 8 ? 3 : 2;     // 6 - log2 NS
            const uint32_t s = lane >> kSh;
            if ((lane & ((1u << kSh) - 1u)) == 0 && (int)s < ns)
                d.out[(int64_t)(c0 + (int)s) * d.ss + (int64_t)o * K + i] = mrow[i] + r;
        }
    }
}

// g_mu = sum_s g_w[s];  g_scale[i][j] = (sum_s g_w[s][i] u_s[j]) sigmoid(scale) / (2 L) for j <= i, 0 above.  Samples in order,
// one fma chain per element (carried through g_scale between passes when S needs more than one).
template <int NS>
__global__ __launch_bounds__(kMvnThreads) void k_mvn_draw_bwd(MvnLaunch P)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int t = mvn_tensor_of(P.t, P.block0, P.n);
    const MvnDev &d = P.t[t];
    const uint32_t b = blockIdx.x - P.block0[t];
    const uint32_t o = b / d.parts, p = b - o * d.parts;
    const uint32_t K = d.cols, Kp = (K + 3u) & ~3u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ed = rng_epoch_dev(d.rng);
    const float *sbase = d.scale + (int64_t)o * K * K;
    float *gbase = d.g_scale + (int64_t)o * K * K;
    const float *gw = d.g_w + (int64_t)o * K;
    const bool vec = d.vec != 0;
    float *u_lds = lds, *g_lds = lds + NS * Kp;
    if (p == 0) {
        for (uint32_t i = threadIdx.x; i < K; i += kMvnThreads) {
            float a = 0.f;
            for (int s = 0; s < P.S; ++s) a += gw[(int64_t)s * d.ss + i];
            d.g_mu[(int64_t)o * K + i] = a;
        }
    }
    for (int c0 = 0; c0 < P.S; c0 += P.sc) {
        const int ns = min(P.sc, P.S - c0);
        const bool first = c0 == 0, last = c0 + ns >= P.S;
        __syncthreads();
        mvn_fill_u(u_lds, d.rng, ed, o, K, Kp, c0, ns, NS);
        for (uint32_t idx = threadIdx.x; idx < (uint32_t)NS * Kp; idx += kMvnThreads) {
            const uint32_t s = idx / Kp, i = idx - s * Kp;
            g_lds[idx] = (i < K && s < (uint32_t)ns) ? gw[(int64_t)(c0 + s) * d.ss + i] : 0.f;
        }
        __syncthreads();
        for (uint32_t i = p + d.parts * wave; i < K; i += d.parts * kMvnWaves) {
            const float *srow = sbase + (int64_t)i * K;
            float *grow = gbase + (int64_t)i * K;
            float gi[NS];
            const float *gq = g_lds + i;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                gi[s] = *gq;
                gq = mvn_next_row(gq, Kp);
            }
            for (uint32_t j0 = 4u * lane; j0 < K; j0 += 256u) {
                float a[4] = {0.f, 0.f, 0.f, 0.f};
                if (j0 <= i) {
                    if (!first) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) a[k] = (j0 + k <= i) ? grow[j0 + k] : 0.f;
                    }
                    const float *uq = u_lds + j0;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const float4 u = *reinterpret_cast<const float4 *>(uq);
                        uq = mvn_next_row(uq, Kp);
                        a[0] = __builtin_fmaf(gi[s], u.x, a[0]);
                        a[1] = __builtin_fmaf(gi[s], u.y, a[1]);
                        a[2] = __builtin_fmaf(gi[s], u.z, a[2]);
                        a[3] = __builtin_fmaf(gi[s], u.w, a[3]);
                    }
                    if (last) {
                        float v[4];
                        mvn_load4(srow, j0, i, K, vec, v);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (j0 + k <= i) {
                                const float l = mvn_l(v[k], j0 + k == i);
                                a[k] = a[k] * (dsoftplus(v[k]) / (2.0f * l));
                            } else {
                                a[k] = 0.f;
                            }
                        }
                    }
                } else if (!first) {
                    continue;           // above the diagonal: zeros written by the first pass
                }
                if (vec) {
                    *reinterpret_cast<float4 *>(grow + j0) = make_float4(a[0], a[1], a[2], a[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (j0 + k < K) grow[j0 + k] = (j0 + k <= i) ? a[k] : 0.f;
                }
            }
        }
    }
}

// Per workgroup: sum over its triangle rows i of 0.5 inv_var (sum_{j <= i} V_ij^2 + (mu_i - m0)^2) - ln V_ii, in fp64 from the
// lanes' fp32 row sums; waves summed in order.  ws[ws0 + b].
__global__ __launch_bounds__(kMvnThreads) void k_mvn_kl_partial(MvnKlLaunch P)
{
    __shared__ double wsum[kMvnWaves];
    const int t = mvn_tensor_of(P.t, P.block0, P.n);
    const MvnKlDev &d = P.t[t];
    const uint32_t b = blockIdx.x - P.block0[t];
    const uint32_t o = b / d.parts, p = b - o * d.parts;
    const uint32_t K = d.cols;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float *sbase = d.scale + (int64_t)o * K * K;
    const float *mrow = d.mu + (int64_t)o * K;
    const bool vec = d.vec != 0;
    double acc = 0.0;
    for (uint32_t i = p + d.parts * wave; i < K; i += d.parts * kMvnWaves) {
        const float *srow = sbase + (int64_t)i * K;
        float r = 0.f;
        for (uint32_t j0 = 4u * lane; j0 <= i; j0 += 256u) {
            float v[4];
            mvn_load4(srow, j0, i, K, vec, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (j0 + k <= i) {
                    const float V = mvn_v(v[k], j0 + k == i);
                    r = __builtin_fmaf(V, V, r);
                }
            }
        }
        double row = 0.5 * (double)d.inv_var * (double)r;
        if (lane == 0) {
            const double dm = (double)mrow[i] - (double)d.m0;
            row += 0.5 * (double)d.inv_var * dm * dm - (double)logf(mvn_v(srow[i], true));
        }
        acc += row;
    }
    acc = wave_sum(acc);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kMvnWaves; ++w) s += wsum[w];
        P.ws[d.ws0 + b] = s;
    }
}

// One workgroup per tensor: out[t] = (sum of its partials in slot order + rows K (ln sigma0 - 1/2)) / rows
__global__ __launch_bounds__(kMvnThreads) void k_mvn_kl_final(MvnKlLaunch P)
{
    __shared__ double wsum[kMvnWaves];
    const MvnKlDev &d = P.t[blockIdx.x];
    const uint32_t nb = d.rows * d.parts;
    const double *w = P.ws + d.ws0;
    double a = 0.0;
    for (uint32_t k = threadIdx.x; k < nb; k += kMvnThreads) a += w[k];
    a = wave_sum(a);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wsum[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < kMvnWaves; ++k) s += wsum[k];
        s += (double)d.rows * (double)d.cols * ((double)d.ln_sigma - 0.5);
        P.out[blockIdx.x] = (float)(s / (double)d.rows);
    }
}

// g_mu = g (mu - m0) inv_var;  g_scale = g (V inv_var - [i == j] / V_ii) sigmoid(scale) on the lower triangle, 0 above;
// g = up[t] / rows
__global__ __launch_bounds__(kMvnThreads) void k_mvn_kl_bwd(MvnKlLaunch P)
{
    const int t = mvn_tensor_of(P.t, P.block0, P.n);
    const MvnKlDev &d = P.t[t];
    const uint32_t b = blockIdx.x - P.block0[t];
    const uint32_t o = b / d.parts, p = b - o * d.parts;
    const uint32_t K = d.cols;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float g = (P.up ? P.up[t] : 1.0f) / (float)d.rows;
    const float *sbase = d.scale + (int64_t)o * K * K;
    float *gbase = d.g_scale + (int64_t)o * K * K;
    const bool vec = d.vec != 0;
    for (uint32_t i = p + d.parts * wave; i < K; i += d.parts * kMvnWaves) {
        const float *srow = sbase + (int64_t)i * K;
        float *grow = gbase + (int64_t)i * K;
        if (lane == 0) {
            const int64_t e = (int64_t)o * K + i;
            d.g_mu[e] = g * ((d.mu[e] - d.m0) * d.inv_var);
        }
        for (uint32_t j0 = 4u * lane; j0 < K; j0 += 256u) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if (j0 <= i) {
                float v[4];
                mvn_load4(srow, j0, i, K, vec, v);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (j0 + k <= i) {
                        const bool diag = j0 + k == i;
                        const float V = mvn_v(v[k], diag);
                        const float dv = diag ? V * d.inv_var - 1.0f / V : V * d.inv_var;
                        a[k] = g * (dv * dsoftplus(v[k]));
                    }
                }
            }
            if (vec) {
                *reinterpret_cast<float4 *>(grow + j0) = make_float4(a[0], a[1], a[2], a[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j0 + k < K) grow[j0 + k] = a[k];
            }
        }
    }
}

static inline bool mvn_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline bool mvn_aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// parts per row: enough workgroups for the machine, at least 2 triangle rows per wave
static inline uint32_t mvn_parts(int64_t rows, int64_t cols)
{
    int64_t p = (kMvnTargetBlocks + rows - 1) / rows;
    const int64_t cap = (cols + 2 * kMvnWaves - 1) / (2 * kMvnWaves);
    if (p > cap) p = cap;
    if (p < 1) p = 1;
    return (uint32_t)p;
}

static int mvn_check_extent(const char *who, int k, int64_t rows, int64_t cols)
{
    if (rows < 1 || cols < 1) { set_error("%s: tensor %d: bad extent", who, k); return BNN_E_SHAPE; }
    if (rows * cols >= ((int64_t)1 << 32) || rows * cols * cols >= ((int64_t)1 << 62)) {
        set_error("%s: tensor %d: rows * cols >= 2^32", who, k);
        return BNN_E_RANGE;
    }
    return BNN_OK;
}

// shared by the draw and its backward (which holds the g_w rows in LDS next to the uniforms: twice the LDS per sample)
static int mvn_prepare(const char *who, const bnn_mvn_tensor_t *tensors, int ntensors, int nsamples, bool backward,
                       MvnLaunch &L, int &sc, uint32_t &blocks)
{
    if (!tensors) { set_error("%s: NULL tensors", who); return BNN_E_NULL; }
    if (ntensors < 1 || ntensors > kMvnMaxTensors) { set_error("%s: 1 .. %d tensors", who, kMvnMaxTensors); return BNN_E_SHAPE; }
    if (nsamples < 1) { set_error("%s: nsamples < 1", who); return BNN_E_SHAPE; }
    if (nsamples > 0xFFFF) { set_error("%s: more than 65535 samples", who); return BNN_E_RANGE; }
    const int lds_rows = backward ? 2 : 1;
    // samples per pass: a power of two (the kernel's unrolled sample count; the LDS rows beyond S are zero)
    sc = 1;
    while (sc < nsamples && sc < kMvnMaxSamplesPerPass) sc <<= 1;
    int64_t total = 0;
    L = MvnLaunch{};
    for (int k = 0; k < ntensors; ++k) {
        const bnn_mvn_tensor_t &x = tensors[k];
        int rc = mvn_check_extent(who, k, x.rows, x.cols);
        if (rc) return rc;
        if (!x.mu || !x.scale || (!backward && !x.out) || (backward && (!x.g_w || !x.g_mu || !x.g_scale))) {
            set_error("%s: tensor %d: NULL pointer", who, k);
            return BNN_E_NULL;
        }
        const void *ps[4] = {x.mu, x.scale, backward ? (const void *)x.g_w : (const void *)x.out, backward ? x.g_scale : nullptr};
        for (const void *q : ps)
            if (q && !mvn_aligned4(q)) { set_error("%s: tensor %d: misaligned pointer", who, k); return BNN_E_ALIGN; }
        if (backward && !mvn_aligned4(x.g_mu)) { set_error("%s: tensor %d: misaligned pointer", who, k); return BNN_E_ALIGN; }
        if (x.sample_stride < 0 || (nsamples > 1 && x.sample_stride < x.rows * x.cols)) {
            set_error("%s: tensor %d: bad sample stride", who, k);
            return BNN_E_SHAPE;
        }
        rc = check_rng(&x.rng, nsamples);
        if (rc) { set_error("%s: tensor %d: bad rng", who, k); return rc; }
        const int64_t Kp = (x.cols + 3) / 4 * 4;
        const int64_t fit = kMvnLdsBytes / (4 * Kp * lds_rows);
        if (fit < 1) { set_error("%s: tensor %d: %lld columns do not fit the workgroup's LDS", who, k, (long long)x.cols); return BNN_E_RANGE; }
        while (sc > fit) sc >>= 1;
        MvnDev &d = L.t[k];
        d.mu = x.mu; d.scale = x.scale; d.out = x.out; d.g_w = x.g_w; d.g_mu = x.g_mu; d.g_scale = x.g_scale;
        d.ss = x.sample_stride;
        d.rows = (uint32_t)x.rows; d.cols = (uint32_t)x.cols;
        d.parts = mvn_parts(x.rows, x.cols);
        d.vec = (x.cols % 4 == 0 && mvn_aligned16(x.scale) && (!backward || mvn_aligned16(x.g_scale))) ? 1u : 0u;
        d.rng = make_rng(&x.rng);
        L.block0[k] = (uint32_t)total;
        total += x.rows * (int64_t)d.parts;
        if (total >= ((int64_t)1 << 31)) { set_error("%s: grid too large", who); return BNN_E_RANGE; }
    }
    L.block0[ntensors] = (uint32_t)total;
    L.n = ntensors;
    L.S = nsamples;
    L.sc = sc;
    blocks = (uint32_t)total;
    return BNN_OK;
}

static int64_t mvn_lds_bytes(const MvnLaunch &L, int lds_rows)
{
    uint32_t kp = 0;
    for (int k = 0; k < L.n; ++k) {
        const uint32_t v = (L.t[k].cols + 3u) & ~3u;
        if (v > kp) kp = v;
    }
    return (int64_t)4 * kp * L.sc * lds_rows;
}

#define BNN_MVN_DISPATCH(KERNEL, NSV, GRID, LDS, ST, ARG)                                                         \
    do {                                                                                                        \
        if ((NSV) <= 1) hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(kMvnThreads), LDS, ST, ARG);                  \
        else if ((NSV) <= 2) hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(kMvnThreads), LDS, ST, ARG);             \
        else if ((NSV) <= 4) hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(kMvnThreads), LDS, ST, ARG);             \
        else if ((NSV) <= 8) hipLaunchKernelGGL(KERNEL<8>, GRID, dim3(kMvnThreads), LDS, ST, ARG);             \
        else hipLaunchKernelGGL(KERNEL<16>, GRID, dim3(kMvnThreads), LDS, ST, ARG);                            \
    } while (0)

static int mvn_kl_prepare(const char *who, const bnn_mvn_kl_tensor_t *tensors, int ntensors, bool backward, MvnKlLaunch &L,
                          uint32_t &blocks)
{
    if (!tensors) { set_error("%s: NULL tensors", who); return BNN_E_NULL; }
    if (ntensors < 1 || ntensors > kMvnMaxTensors) { set_error("%s: 1 .. %d tensors", who, kMvnMaxTensors); return BNN_E_SHAPE; }
    L = MvnKlLaunch{};
    int64_t total = 0;
    for (int k = 0; k < ntensors; ++k) {
        const bnn_mvn_kl_tensor_t &x = tensors[k];
        int rc = mvn_check_extent(who, k, x.rows, x.cols);
        if (rc) return rc;
        if (!x.mu || !x.scale || (backward && (!x.g_mu || !x.g_scale))) { set_error("%s: tensor %d: NULL pointer", who, k); return BNN_E_NULL; }
        if (!mvn_aligned4(x.mu) || !mvn_aligned4(x.scale) || (backward && (!mvn_aligned4(x.g_mu) || !mvn_aligned4(x.g_scale)))) {
            set_error("%s: tensor %d: misaligned pointer", who, k);
            return BNN_E_ALIGN;
        }
        if (!(x.prior_sigma > 0.0f) || !(x.prior_sigma < 3.0e38f) || !(x.prior_mu == x.prior_mu)) {
            set_error("%s: tensor %d: prior sigma must be positive and finite", who, k);
            return BNN_E_RANGE;
        }
        MvnKlDev &d = L.t[k];
        d.mu = x.mu; d.scale = x.scale; d.g_mu = x.g_mu; d.g_scale = x.g_scale;
        d.rows = (uint32_t)x.rows; d.cols = (uint32_t)x.cols;
        d.parts = mvn_parts(x.rows, x.cols);
        d.vec = (x.cols % 4 == 0 && mvn_aligned16(x.scale) && (!backward || mvn_aligned16(x.g_scale))) ? 1u : 0u;
        d.m0 = x.prior_mu;
        d.inv_var = (float)(1.0 / ((double)x.prior_sigma * (double)x.prior_sigma));
        d.ln_sigma = (float)std::log((double)x.prior_sigma);
        d.ws0 = (uint32_t)total;
        L.block0[k] = (uint32_t)total;
        total += x.rows * (int64_t)d.parts;
        if (total >= ((int64_t)1 << 31)) { set_error("%s: grid too large", who); return BNN_E_RANGE; }
    }
    L.block0[ntensors] = (uint32_t)total;
    L.n = ntensors;
    blocks = (uint32_t)total;
    return BNN_OK;
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_mvn_draw(const bnn_mvn_tensor_t *tensors, int ntensors, int nsamples, void *stream)
{
    const char *who = "bnn_mvn_draw";
    MvnLaunch L;
    int sc = 0;
    uint32_t blocks = 0;
    int rc = mvn_prepare(who, tensors, ntensors, nsamples, false, L, sc, blocks);
    if (rc) return rc;
    BNN_MVN_DISPATCH(k_mvn_draw, sc, dim3(blocks), (size_t)mvn_lds_bytes(L, 1), (hipStream_t)stream, L);
    return check_launch(who);
}

int bnn_mvn_draw_backward(const bnn_mvn_tensor_t *tensors, int ntensors, int nsamples, void *stream)
{
    const char *who = "bnn_mvn_draw_backward";
    MvnLaunch L;
    int sc = 0;
    uint32_t blocks = 0;
    int rc = mvn_prepare(who, tensors, ntensors, nsamples, true, L, sc, blocks);
    if (rc) return rc;
    BNN_MVN_DISPATCH(k_mvn_draw_bwd, sc, dim3(blocks), (size_t)mvn_lds_bytes(L, 2), (hipStream_t)stream, L);
    return check_launch(who);
}

int64_t bnn_mvn_kl_workspace_bytes(const bnn_mvn_kl_tensor_t *tensors, int ntensors)
{
    if (!tensors || ntensors < 1 || ntensors > kMvnMaxTensors) return -1;
    int64_t n = 0;
    for (int k = 0; k < ntensors; ++k) {
        if (tensors[k].rows < 1 || tensors[k].cols < 1) return -1;
        n += tensors[k].rows * (int64_t)mvn_parts(tensors[k].rows, tensors[k].cols);
    }
    return 8 * n;
}

int bnn_mvn_kl(const bnn_mvn_kl_tensor_t *tensors, int ntensors, float *out, void *workspace, int64_t workspace_bytes,
               void *stream)
{
    const char *who = "bnn_mvn_kl";
    MvnKlLaunch L;
    uint32_t blocks = 0;
    int rc = mvn_kl_prepare(who, tensors, ntensors, false, L, blocks);
    if (rc) return rc;
    if (!out || !workspace) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) || !mvn_aligned4(out)) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    if (workspace_bytes < 8 * (int64_t)blocks) { set_error("%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
                                                           (long long)(8 * (int64_t)blocks)); return BNN_E_SHAPE; }
    L.ws = static_cast<double *>(workspace);
    L.out = out;
    hipLaunchKernelGGL(k_mvn_kl_partial, dim3(blocks), dim3(kMvnThreads), 0, (hipStream_t)stream, L);
    rc = check_launch(who);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mvn_kl_final, dim3(ntensors), dim3(kMvnThreads), 0, (hipStream_t)stream, L);
    return check_launch(who);
}

int bnn_mvn_kl_backward(const bnn_mvn_kl_tensor_t *tensors, int ntensors, const float *upstream, void *stream)
{
    const char *who = "bnn_mvn_kl_backward";
    MvnKlLaunch L;
    uint32_t blocks = 0;
    int rc = mvn_kl_prepare(who, tensors, ntensors, true, L, blocks);
    if (rc) return rc;
    if (upstream && !mvn_aligned4(upstream)) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    L.up = upstream;
    hipLaunchKernelGGL(k_mvn_kl_bwd, dim3(blocks), dim3(kMvnThreads), 0, (hipStream_t)stream, L);
    return check_launch(who);
}

}  // extern "C"
