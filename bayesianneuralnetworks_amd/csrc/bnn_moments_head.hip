// bnn_moments_head.hip -- K21: the head of a sampling-free pass.  The moments of MultivariateNormalLinear (the reference's
// sampler: w_o = mu_o + L_o u, u ~ U[0, 1)^K, L = sqrt(tril(softplus(scale)) + 1e-10 I) element by element), the N x N covariance
// of a dense head's outputs per batch row, and a sampler that draws logits with that covariance.  Inference only, fp32 VALU
// kernels (the work is tiny next to the trunk), fp32 in both compute modes.  No atomics and no split reductions: every sum is one
// ascending fma chain, identical calls give identical bits.  The formulas are include/bnn_hip.h's (K21).
#include "bnn_mvn_dev.hpp"

namespace bnn {

constexpr float kTwelfth = 1.0f / 12.0f;        // the variance of U[0, 1)

// ---- 1. prepare: E_w, G_w = E_w^2 + D, E_b, C_b -- one thread per weight row (o, k) / per bias pair (o >= p)
struct MvnPrepArgs {
    const float *mu_w, *scale_w, *mu_b, *scale_b;
    float *E_w, *G_w, *E_b, *C_b;
    int64_t nw;                 // O K
    uint32_t O, K, wblocks;
};

__global__ __launch_bounds__(256) void k_moments_mvn_prepare(const MvnPrepArgs A)
{
    if (blockIdx.x < A.wblocks) {
        const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (e >= A.nw) return;
        const uint32_t k = (uint32_t)(e % A.K);
        const float *srow = A.scale_w + e * A.K;            // row k of L_o: scale_w[o][k][0 .. k]
        float s1 = 0.f, s2 = 0.f;
        for (uint32_t j = 0; j <= k; ++j) {
            const float l = mvn_l(srow[j], j == k);
            s1 += l;
            s2 = __builtin_fmaf(l, l, s2);
        }
        const float E = __builtin_fmaf(0.5f, s1, A.mu_w[e]);
        A.E_w[e] = E;
        A.G_w[e] = __builtin_fmaf(E, E, kTwelfth * s2);
        return;
    }
    const int64_t e = (int64_t)(blockIdx.x - A.wblocks) * 256 + threadIdx.x;
    if (e >= (int64_t)A.O * A.O) return;
    const uint32_t o = (uint32_t)(e / A.O), p = (uint32_t)(e % A.O);
    if (p > o) return;
    const float *ro = A.scale_b + (int64_t)o * A.O, *rp = A.scale_b + (int64_t)p * A.O;
    float c = 0.f, s1 = 0.f;
    for (uint32_t j = 0; j <= p; ++j) {                     // (L_b L_b^T)[o][p]: columns 0 .. min(o, p) = p
        const float lo = mvn_l(ro[j], j == o), lp = mvn_l(rp[j], j == p);
        c = __builtin_fmaf(lo, lp, c);
        s1 += lo;
    }
    c *= kTwelfth;
    A.C_b[(int64_t)o * A.O + p] = c;
    A.C_b[(int64_t)p * A.O + o] = c;
    if (p == o) A.E_b[o] = __builtin_fmaf(0.5f, s1, A.mu_b[o]);
}

// ---- 2. forward: a workgroup owns (64 batch rows, one output o).  Thread (r, c) = (tid / 4, tid % 4) keeps t_j = sum_{k >= j}
// a_m[r][k] L_o[k][j] for the 16 columns j = j0 + 16 c .. + 15 of the current 64-column slab in registers while the rows k >= j0 of
// L_o pass through LDS in panels of 32, formed from scale_w on the fly (once per element per workgroup; nothing above the diagonal
// is read).  The first slab's sweep sees every k, so its c == 0 lanes also run the two dot products sum_k a_m E_w and sum_k a_v G_w.
// The quadratic form sum_j t_j^2 is one chain in ascending j: the four lanes of a row take turns, slab after slab.
constexpr int kHeadRows = 64;       // batch rows per workgroup
constexpr int kHeadSlab = 64;       // columns j per sweep
constexpr int kHeadPanel = 32;      // rows k per LDS panel
constexpr int kHeadCols = kHeadSlab / 4;
constexpr int kHeadMaxK = 4096;

struct MvnFwdArgs {
    const float *a_m, *a_v;
    int64_t lda;
    const float *scale_w, *E_w, *G_w, *E_b, *C_b;
    float *out_m, *out_v;
    int32_t B, O, K;
};

__global__ __launch_bounds__(256) void k_moments_mvn_forward(const MvnFwdArgs A)
{
    __shared__ __attribute__((aligned(16))) float l_lds[kHeadPanel][kHeadSlab];
    __shared__ float am_lds[kHeadRows][kHeadPanel + 1];
    __shared__ float av_lds[kHeadRows][kHeadPanel + 1];
    __shared__ float e_lds[kHeadPanel], g_lds[kHeadPanel];

    const int tid = threadIdx.x;
    const int r = tid >> 2, c = tid & 3;
    const int o = blockIdx.x;
    const int b0 = blockIdx.y * kHeadRows;
    const int K = A.K;
    const float *sbase = A.scale_w + (int64_t)o * K * K;
    const bool var = A.a_v != nullptr;

    float q = 0.f, m = 0.f, s = 0.f;
    for (int j0 = 0; j0 < K; j0 += kHeadSlab) {
        float t[kHeadCols];
#pragma unroll
        for (int i = 0; i < kHeadCols; ++i) t[i] = 0.f;
        const bool first = j0 == 0;
        for (int k0 = j0; k0 < K; k0 += kHeadPanel) {
            __syncthreads();
            {   // L panel: rows k0 .. k0 + 31, columns j0 .. j0 + 63; zero above the diagonal and beyond K
                const int jj = tid & 63;
                const int j = j0 + jj;
#pragma unroll
                for (int i = 0; i < kHeadPanel / 4; ++i) {
                    const int kk = (tid >> 6) + 4 * i;
                    const int k = k0 + kk;
                    l_lds[kk][jj] = (k < K && j <= k) ? mvn_l(sbase[(int64_t)k * K + j], j == k) : 0.f;
                }
            }
            {   // a_m (and in the first slab a_v) panel: 64 batch rows x 32 k
                const int kk = tid & 31;
                const int k = k0 + kk;
#pragma unroll
                for (int i = 0; i < kHeadRows / 8; ++i) {
                    const int rr = (tid >> 5) + 8 * i;
                    const bool in = k < K && b0 + rr < A.B;
                    const int64_t off = (int64_t)(b0 + rr) * A.lda + k;
                    am_lds[rr][kk] = in ? A.a_m[off] : 0.f;
                    if (first) av_lds[rr][kk] = (in && var) ? A.a_v[off] : 0.f;
                }
            }
            if (first && tid < kHeadPanel) {
                const int k = k0 + tid;
                e_lds[tid] = k < K ? A.E_w[(int64_t)o * K + k] : 0.f;
                g_lds[tid] = k < K ? A.G_w[(int64_t)o * K + k] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int kk = 0; kk < kHeadPanel; ++kk) {
                const float a = am_lds[r][kk];
                const float4 *lp = reinterpret_cast<const float4 *>(&l_lds[kk][kHeadCols * c]);
#pragma unroll
                for (int i = 0; i < kHeadCols / 4; ++i) {
                    const float4 l = lp[i];
                    t[4 * i + 0] = __builtin_fmaf(a, l.x, t[4 * i + 0]);
                    t[4 * i + 1] = __builtin_fmaf(a, l.y, t[4 * i + 1]);
                    t[4 * i + 2] = __builtin_fmaf(a, l.z, t[4 * i + 2]);
                    t[4 * i + 3] = __builtin_fmaf(a, l.w, t[4 * i + 3]);
                }
            }
            if (first && c == 0) {
                for (int kk = 0; kk < kHeadPanel; ++kk) {
                    m = __builtin_fmaf(am_lds[r][kk], e_lds[kk], m);
                    s = __builtin_fmaf(av_lds[r][kk], g_lds[kk], s);
                }
            }
        }
        // q += sum_j t_j^2 over this slab's columns, ascending: lane c = 0, then 1, 2, 3 of the row (columns beyond K hold t = 0)
#pragma unroll
        for (int turn = 0; turn < 4; ++turn) {
            float qq = q;
#pragma unroll
            for (int i = 0; i < kHeadCols; ++i) qq = __builtin_fmaf(t[i], t[i], qq);
            q = __shfl(qq, (tid & 60 & 63) + turn, 64);
        }
    }
    if (c == 0 && b0 + r < A.B) {
        float v = __builtin_fmaf(kTwelfth, q, s);
        if (A.E_b) {
            m += A.E_b[o];
            v += A.C_b[(int64_t)o * A.O + o];
        }
        const int64_t e = (int64_t)(b0 + r) * A.O + o;
        A.out_m[e] = m;
        A.out_v[e] = v;
    }
}

// ---- 3. head covariance: a workgroup owns one batch row; its threads stride the pairs o > p and keep one fma chain over k per pair
// (at most two pairs per thread at N = 32), E and a_v passing through LDS in chunks of 128 columns.  Both triangles are written from
// the one computed value; the diagonal is var's bits.
constexpr int kCovMaxN = 32;
constexpr int kCovChunk = 128;
constexpr int kCovPairs = (kCovMaxN * (kCovMaxN - 1) / 2 + 255) / 256;

struct HeadCovArgs {
    const float *a_v;
    int64_t lda;
    const float *E, *C_b, *var;
    float *cov;
    int32_t N, K;
};

__global__ __launch_bounds__(256) void k_moments_head_cov(const HeadCovArgs A)
{
    __shared__ float e_lds[kCovMaxN][kCovChunk + 1];
    __shared__ float av_lds[kCovChunk];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int N = A.N, K = A.K;
    const int npairs = N * (N - 1) / 2;
    int po[kCovPairs], pp[kCovPairs];
    float acc[kCovPairs];
#pragma unroll
    for (int i = 0; i < kCovPairs; ++i) {
        // pair index -> (o, p), o > p: row o of the strict lower triangle starts at o (o - 1) / 2
        const int idx = tid + 256 * i;
        int o = 1;
        while ((o + 1) * o / 2 <= idx && o < N - 1) ++o;
        po[i] = o;
        pp[i] = idx - o * (o - 1) / 2;
        acc[i] = 0.f;
    }
    if (A.a_v) {
        for (int k0 = 0; k0 < K; k0 += kCovChunk) {
            const int nk = min(kCovChunk, K - k0);
            __syncthreads();
            for (int idx = tid; idx < N * kCovChunk; idx += 256) {
                const int n = idx / kCovChunk, kk = idx - n * kCovChunk;
                e_lds[n][kk] = kk < nk ? A.E[(int64_t)n * K + k0 + kk] : 0.f;
            }
            if (tid < kCovChunk) av_lds[tid] = tid < nk ? A.a_v[b * A.lda + k0 + tid] : 0.f;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < kCovPairs; ++i) {
                if (tid + 256 * i >= npairs) continue;
                const float *eo = e_lds[po[i]], *ep = e_lds[pp[i]];
                float a = acc[i];
                for (int kk = 0; kk < nk; ++kk) a = __builtin_fmaf(eo[kk] * ep[kk], av_lds[kk], a);
                acc[i] = a;
            }
        }
    }
    float *cb = A.cov + b * N * N;
#pragma unroll
    for (int i = 0; i < kCovPairs; ++i) {
        if (tid + 256 * i >= npairs) continue;
        const int o = po[i], p = pp[i];
        float cval = acc[i];
        if (A.C_b) cval += A.C_b[o * N + p];
        cb[o * N + p] = cval;
        cb[p * N + o] = cval;
    }
    if (tid < N) cb[tid * N + tid] = A.var[b * N + tid];
}

// ---- 4. correlated draws: y_s[b, :] = m[b, :] + Lc_b eps_s[b, :].  32 lanes own one row b (lane i: output i): the lower Cholesky
// factor of cov[b] in fp64 in LDS, column by column (a pivot <= 0 gives a zero column), then per sample the eps of the row's N
// elements (eps1 on e = b N + n: bnn_moments_sample's values on the same key) and the fp64 product, rounded once.
constexpr int kSampleRows = 4;      // rows per workgroup of 128 threads

__global__ __launch_bounds__(32 * kSampleRows) void k_moments_sample_cov(const float *__restrict__ m, const float *__restrict__ cov,
                                                                         float *__restrict__ y, uint32_t rows, int N, int S, RngDev rng)
{
    __shared__ double lc[kSampleRows][kCovMaxN][kCovMaxN + 1];
    __shared__ float eps[kSampleRows][kCovMaxN];
    const int w = threadIdx.x >> 5, i = threadIdx.x & 31;
    const uint32_t b = blockIdx.x * kSampleRows + w;
    const bool on = b < rows && i < N;
    const uint32_t ed = rng_epoch_dev(rng);
    const float *cb = cov + (int64_t)b * N * N;
    for (int j = 0; j < N; ++j) {
        double sum = 0.0;
        if (on && i >= j) {
            sum = (double)cb[i * N + j];
            for (int k = 0; k < j; ++k) sum = __builtin_fma(-lc[w][i][k], lc[w][j][k], sum);
        }
        if (on && i == j) lc[w][j][j] = sum > 0.0 ? __builtin_sqrt(sum) : 0.0;
        __syncthreads();
        if (on && i > j) {
            const double d = lc[w][j][j];
            lc[w][i][j] = d > 0.0 ? sum / d : 0.0;
        }
        __syncthreads();
    }
    const double mi = on ? (double)m[(int64_t)b * N + i] : 0.0;
    const int64_t ss = (int64_t)rows * N;
    for (int s = 0; s < S; ++s) {
        __syncthreads();
        if (on) eps[w][i] = eps1(rng, ed, (uint64_t)b * N + i, rng.sample0 + (uint32_t)s);
        __syncthreads();
        if (on) {
            double a = 0.0;
            for (int k = 0; k <= i; ++k) a = __builtin_fma(lc[w][i][k], (double)eps[w][k], a);
            y[(int64_t)s * ss + (int64_t)b * N + i] = (float)(mi + a);
        }
    }
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_mvn_moments_prepare(const float *mu_w, const float *scale_w, const float *mu_b, const float *scale_b, float *E_w, float *G_w,
                            float *E_b, float *C_b, int64_t O, int64_t K, void *stream)
{
    const char *who = "bnn_mvn_moments_prepare";
    if (!mu_w || !scale_w || !E_w || !G_w) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    const int nb = (mu_b != nullptr) + (scale_b != nullptr) + (E_b != nullptr) + (C_b != nullptr);
    if (nb != 0 && nb != 4) { set_error("%s: NULL pointer (mu_b, scale_b, E_b, C_b: all or none)", who); return BNN_E_NULL; }
    if (O < 1 || K < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (K > kHeadMaxK) { set_error("%s: K = %lld (at most %d)", who, (long long)K, kHeadMaxK); return BNN_E_RANGE; }
    if (O >= ((int64_t)1 << 15) || O * K >= ((int64_t)1 << 31)) { set_error("%s: O >= 2^15 or O K >= 2^31", who); return BNN_E_RANGE; }
    if (nb && O > kHeadMaxK) { set_error("%s: a bias of %lld elements (at most %d)", who, (long long)O, kHeadMaxK); return BNN_E_RANGE; }
    if (misaligned(mu_w, 3) || misaligned(scale_w, 3) || misaligned(mu_b, 3) || misaligned(scale_b, 3) || misaligned(E_w, 3) ||
        misaligned(G_w, 3) || misaligned(E_b, 3) || misaligned(C_b, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    MvnPrepArgs A{};
    A.mu_w = mu_w; A.scale_w = scale_w; A.mu_b = mu_b; A.scale_b = scale_b;
    A.E_w = E_w; A.G_w = G_w; A.E_b = E_b; A.C_b = C_b;
    A.nw = O * K;
    A.O = (uint32_t)O; A.K = (uint32_t)K;
    A.wblocks = (uint32_t)((O * K + 255) / 256);
    const uint32_t bblocks = nb ? (uint32_t)((O * O + 255) / 256) : 0u;
    hipLaunchKernelGGL(k_moments_mvn_prepare, dim3(A.wblocks + bblocks), dim3(256), 0, (hipStream_t)stream, A);
    return check_launch(who);
}

int bnn_mvn_moments_forward(const float *a_m, const float *a_v, int64_t lda, const float *scale_w, const float *E_w, const float *G_w,
                            const float *E_b, const float *C_b, float *out_m, float *out_v, int64_t B, int64_t O, int64_t K,
                            void *stream)
{
    const char *who = "bnn_mvn_moments_forward";
    if (!a_m || !scale_w || !E_w || !G_w || !out_m || !out_v || (E_b == nullptr) != (C_b == nullptr)) {
        set_error("%s: NULL pointer", who);
        return BNN_E_NULL;
    }
    if (B < 0 || O < 1 || K < 1 || lda < K) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (K > kHeadMaxK) { set_error("%s: K = %lld (at most %d)", who, (long long)K, kHeadMaxK); return BNN_E_RANGE; }
    if (B > (int64_t)kHeadRows * 65535 || O >= ((int64_t)1 << 15)) { set_error("%s: B > 64 * 65535 or O >= 2^15", who); return BNN_E_RANGE; }
    if (misaligned(a_m, 3) || misaligned(a_v, 3) || misaligned(scale_w, 3) || misaligned(E_w, 3) || misaligned(G_w, 3) ||
        misaligned(E_b, 3) || misaligned(C_b, 3) || misaligned(out_m, 3) || misaligned(out_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (B == 0) return BNN_OK;
    MvnFwdArgs A{};
    A.a_m = a_m; A.a_v = a_v; A.lda = lda;
    A.scale_w = scale_w; A.E_w = E_w; A.G_w = G_w; A.E_b = E_b; A.C_b = C_b;
    A.out_m = out_m; A.out_v = out_v;
    A.B = (int32_t)B; A.O = (int32_t)O; A.K = (int32_t)K;
    const dim3 g((unsigned)O, (unsigned)((B + kHeadRows - 1) / kHeadRows));
    hipLaunchKernelGGL(k_moments_mvn_forward, g, dim3(256), 0, (hipStream_t)stream, A);
    return check_launch(who);
}

int bnn_moments_head_cov(const float *a_v, int64_t lda, const float *E, const float *C_b, const float *var, float *cov, int64_t B,
                         int64_t N, int64_t K, void *stream)
{
    const char *who = "bnn_moments_head_cov";
    if (!var || !cov || (a_v && !E)) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (B < 0 || N < 1 || K < 1 || (a_v && lda < K)) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (N > kCovMaxN) { set_error("%s: N = %lld (at most %d)", who, (long long)N, kCovMaxN); return BNN_E_RANGE; }
    if (B >= ((int64_t)1 << 31) || K >= ((int64_t)1 << 26)) { set_error("%s: B >= 2^31 or K >= 2^26", who); return BNN_E_RANGE; }
    if (misaligned(a_v, 3) || misaligned(E, 3) || misaligned(C_b, 3) || misaligned(var, 3) || misaligned(cov, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (B == 0) return BNN_OK;
    HeadCovArgs A{};
    A.a_v = a_v; A.lda = lda; A.E = E; A.C_b = C_b; A.var = var; A.cov = cov;
    A.N = (int32_t)N; A.K = (int32_t)K;
    hipLaunchKernelGGL(k_moments_head_cov, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, A);
    return check_launch(who);
}

int bnn_moments_sample_cov(const float *m, const float *cov, float *y, int64_t rows, int64_t N, int nsamples, const bnn_rng_t *rng,
                           int flags, void *stream)
{
    const char *who = "bnn_moments_sample_cov";
    if (!m || !cov || !y) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (!rng) { set_error("%s: NULL rng", who); return BNN_E_NULL; }
    if (rows < 0 || N < 1 || nsamples < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (N > kCovMaxN) { set_error("%s: N = %lld (at most %d)", who, (long long)N, kCovMaxN); return BNN_E_RANGE; }
    if (nsamples > 0xFFFF) { set_error("%s: more than 65535 samples", who); return BNN_E_RANGE; }
    if (rows * N >= ((int64_t)1 << 32)) { set_error("%s: one sample has 2^32 output elements or more", who); return BNN_E_RANGE; }
    const int rc = check_rng(rng, nsamples);
    if (rc) { set_error("%s: bad rng", who); return rc; }
    if (flags) { set_error("%s: unknown flag (the samples are fp32)", who); return BNN_E_UNSUPPORTED; }
    if (misaligned(m, 3) || misaligned(cov, 3) || misaligned(y, 3)) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    if (rows == 0) return BNN_OK;
    const unsigned blocks = (unsigned)((rows + kSampleRows - 1) / kSampleRows);
    hipLaunchKernelGGL(k_moments_sample_cov, dim3(blocks), dim3(32 * kSampleRows), 0, (hipStream_t)stream, m, cov, y, (uint32_t)rows,
                       (int)N, nsamples, make_rng(rng));
    return check_launch(who);
}

}  // extern "C"
