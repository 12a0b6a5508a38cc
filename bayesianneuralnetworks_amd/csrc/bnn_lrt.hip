// bnn_lrt.hip -- K10: the local-reparameterization dense layer (LocalReparamLinear, nn/dense.py; Kingma, Salimans,
// Welling 2015).  For independent Gaussian w, b the pre-activation is Gaussian per output element:
//     m = x mu_w^T + mu_b,   v = x^2 (sigma_w^2)^T + sigma_b^2,   y_s = m + sqrt(v + 1e-16) eps_s
// with one eps per OUTPUT element and MC sample: eps[e = b N + n] of the layer's noise key, sample sample0 + s (the RNG contract
// of include/bnn_hip.h; eps4 / eps1 of bnn_device.hpp, the device function every other consumer calls).  No weight is drawn.
//
// Three uses of the paired-contraction tile of bnn_lrt_tile.hpp, two planes per operand, the second one either a second tensor
// or the square of the first:
//     forward          P = (mu_w, sigma_w^2)        Q = (x, x^2)          y[b][n]   = acc1 + mu_b + sqrt(acc2 + sigma_b^2 + 1e-16) eps
//     input gradient   P = (mu_w, sigma_w^2)^T      Q = (g_m, g_v)        gx[b][k]  = acc1 + 2 x[b][k] acc2
//     weight gradient  P = (x, x^2)^T               Q = (g_m, g_v)^T      g_mu[n][k] = acc1,  g_rho[n][k] = CHAIN(acc2, rho[n][k])
// CHAIN is the posterior's chain factor (bnn_device.hpp): ChainRho here, 2 sigma sigmoid(rho); ChainLogSigma2 for K23's posterior
// N(theta, exp(log_sigma2)) (bnn_vd.hip), whose weight gradient is the same tile, the same host function (lrt_backward_weight).
// The forward asks for one aligned eps quad per lane, MFMA tile and sample.  BK = 64 (bf16) / 32 (fp32).
#include "bnn_lrt_tile.hpp"

namespace bnn {

enum { LRT_FWD = 0, LRT_DGRAD = 1, LRT_WGRAD = 2 };

struct LrtArgs {
    const void *p1, *p2;        // P planes (p2 NULL: the square of p1); rows index i
    const void *q1, *q2;        // Q planes; rows index j
    int64_t ldp, ldq;
    int32_t I, J, C;            // output extents (i: contiguous in memory) and the contraction length
    int32_t x_bf16;             // the activation operand (Q of the forward, P of the weight gradient) is bf16
    void *out;                  // y / gx / g_mu
    float *out2;                // v (forward, may be NULL) / g_rho or g_log_sigma2
    const float *e1, *e2;       // forward: mu_b, sigma_b^2 (both or neither); weight gradient: e1 = rho_w or log_sigma2
    const void *x;              // input gradient: the layer input (2 x g)
    int64_t ldx;
    int32_t out_bf16;           // forward: y is bf16; input gradient: gx is bf16
    int32_t S, shared;          // forward: samples; shared input (samples loop in the epilogue) or sample = blockIdx.z
    RngDev rng;
};

// T = float (fp32 compute, BK = 32) or uint16_t (bf16 compute, BK = 64); CHAIN: the weight gradient's epilogue only
template <typename T, int MODE, typename CHAIN = ChainRho>
__global__ __launch_bounds__(kLrtThreads) void k_lrt(const LrtArgs A)
{
    constexpr bool BF = sizeof(T) == 2;
    constexpr int BK = BF ? 64 : 32;
    constexpr int LDK = BF ? BK + 8 : BK + 1;       // bf16: rows stay 16-byte aligned for the 8-element fragment read
    constexpr int EPT = BK / 4;
    constexpr bool P_TR = MODE != LRT_FWD, Q_TR = MODE == LRT_WGRAD;
    constexpr bool P_SQ = MODE == LRT_WGRAD, Q_SQ = MODE == LRT_FWD;
    __shared__ __attribute__((aligned(16))) T lds[4 * kLrtTile * LDK];
    T *lp = lds, *lq = lds + 2 * kLrtTile * LDK;

    const int i0 = blockIdx.x * kLrtTile, j0 = blockIdx.y * kLrtTile;
    const int z = MODE == LRT_FWD ? (int)blockIdx.z : 0;            // forward, per-sample input: rows z J .. z J + J - 1 of x
    const bool p_bf = MODE == LRT_WGRAD && A.x_bf16, q_bf = MODE == LRT_FWD && A.x_bf16;
    const void *q1 = A.q1;
    if (MODE == LRT_FWD && z) q1 = reinterpret_cast<const char *>(A.q1) + (int64_t)z * A.J * A.ldq * (q_bf ? 2 : 4);

    f32x4 acc1[2][2], acc2[2][2];
    lrt_zero(acc1, acc2);
    float rp1[EPT], rp2[EPT] = {}, rq1[EPT], rq2[EPT] = {};
    auto fetch = [&](int c0) {
        lrt_fetch<P_TR, BK>(rp1, A.p1, p_bf, A.ldp, i0, A.I, c0, A.C);
        if constexpr (!P_SQ) lrt_fetch<P_TR, BK>(rp2, A.p2, false, A.ldp, i0, A.I, c0, A.C);
        lrt_fetch<Q_TR, BK>(rq1, q1, q_bf, A.ldq, j0, A.J, c0, A.C);
        if constexpr (!Q_SQ) lrt_fetch<Q_TR, BK>(rq2, A.q2, false, A.ldq, j0, A.J, c0, A.C);
    };
    fetch(0);
    for (int c0 = 0; c0 < A.C; c0 += BK) {
        if constexpr (BF) {                 // one loop: P, then Q costs the bf16 weight gradient 12 registers
            lrt_stage2<T, P_TR, P_SQ, Q_TR, Q_SQ, 2, BK, LDK>(lp, lq, rp1, rp2, rq1, rq2);
        } else {                            // P, then Q: one loop costs the fp32 weight gradient 3.5 % at 4096 x 1200 x 1200
            lrt_stage<T, P_TR, P_SQ, 2, BK, LDK>(lp, rp1, rp2);
            lrt_stage<T, Q_TR, Q_SQ, 2, BK, LDK>(lq, rq1, rq2);
        }
        __syncthreads();
        if (c0 + BK < A.C) fetch(c0 + BK);
        lrt_mfma_block<T, 2, BK, LDK>(acc1, acc2, lp, lq);
        __syncthreads();
    }

    const bool vec = (A.I & 3) == 0;
    const uint32_t ed = MODE == LRT_FWD ? rng_epoch_dev(A.rng) : 0u;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            LrtQuad q;
            if (!lrt_quad(q, a, b, A.I, A.J)) continue;
            float r1[4] = {acc1[a][b][0], acc1[a][b][1], acc1[a][b][2], acc1[a][b][3]};
            float r2[4] = {acc2[a][b][0], acc2[a][b][1], acc2[a][b][2], acc2[a][b][3]};
            const int64_t o = (int64_t)q.j * A.I + q.i;
            if constexpr (MODE == LRT_FWD) {
                float sd[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (A.e1 && r < q.ni) { r1[r] += A.e1[q.i + r]; r2[r] += A.e2[q.i + r]; }
                    sd[r] = sqrtf(r2[r] + 1e-16f);
                }
                const int64_t zo = (int64_t)z * A.J * A.I + o;
                if (A.out2) lrt_store4(A.out2 + zo, r2, vec, q.ni);
                const uint32_t e = (uint32_t)q.j * (uint32_t)A.I + (uint32_t)q.i;   // b N + n within the sample
                const int ns = A.shared ? A.S : 1;
                for (int s = 0; s < ns; ++s) {
                    float y[4];
                    lrt_noise4(y, r1, sd, A.rng, ed, e, A.rng.sample0 + (uint32_t)(A.shared ? s : z), vec, q.ni);
                    lrt_store4(A.out, A.out_bf16 != 0, A.shared ? (int64_t)s * A.J * A.I + o : zo, y, vec, q.ni);
                }
            } else if constexpr (MODE == LRT_DGRAD) {
                float g[4];
                for (int r = 0; r < q.ni; ++r) {
                    const float xv = lrt_ld(A.x, (int64_t)q.j * A.ldx + q.i + r, A.x_bf16 != 0);
                    g[r] = __builtin_fmaf(2.0f * xv, r2[r], r1[r]);
                }
                lrt_store4(A.out, A.out_bf16 != 0, o, g, vec, q.ni);
            } else {
                float g[4];
                for (int r = 0; r < q.ni; ++r) g[r] = CHAIN::apply(r2[r], A.e1[o + r]);
                lrt_store4x2(reinterpret_cast<float *>(A.out) + o, r1, A.out2 + o, g, vec, q.ni);
            }
        }
}

// sigma^2 of the weight and the bias posterior in one launch (element t < n_w: the weight)
__global__ __launch_bounds__(256) void k_lrt_prepare(const float *__restrict__ rho_w, float *__restrict__ s2_w, int64_t n_w,
                                                     const float *__restrict__ rho_b, float *__restrict__ s2_b, int64_t n_b)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_w + n_b; t += (int64_t)gridDim.x * 256) {
        if (t < n_w) { const float s = sigma_lrt(rho_w[t]); s2_w[t] = s * s; }
        else { const float s = sigma_lrt(rho_b[t - n_w]); s2_b[t - n_w] = s * s; }
    }
}

// g_m = sum_s gy_s, g_v = sum_s gy_s eps_s / (2 sqrt(v + 1e-16)): one thread per quad of the sample's b N + n index.
// SUM (shared input): the samples are added in sample order, v is one sample's; otherwise sample = blockIdx.y.
template <bool SUM>
__global__ __launch_bounds__(256) void k_lrt_bwd_epilogue(const void *__restrict__ gy, int gy_bf16, const float *__restrict__ v,
                                                          float *__restrict__ g_m, float *__restrict__ g_v, uint32_t n, int S, RngDev rng)
{
    const uint32_t ed = rng_epoch_dev(rng);
    const uint32_t nq = (n + 3u) >> 2;
    const int s0 = SUM ? 0 : (int)blockIdx.y;
    const int s1 = SUM ? S : s0 + 1;
    const int64_t vo = SUM ? 0 : (int64_t)s0 * n;
    for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        float inv[4], am[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t e = 4u * q + (uint32_t)j;
            inv[j] = e < n ? 0.5f / sqrtf(v[vo + e] + 1e-16f) : 0.f;
        }
        for (int s = s0; s < s1; ++s) {
            const float4 z = eps4(rng, ed, q, rng.sample0 + (uint32_t)s);
            const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t e = 4u * q + (uint32_t)j;
                if (e < n) {
                    const float g = lrt_ld(gy, (int64_t)s * n + e, gy_bf16 != 0);
                    am[j] += g;
                    av[j] += g * zz[j] * inv[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t e = 4u * q + (uint32_t)j;
            if (e < n) { g_m[vo + e] = am[j]; g_v[vo + e] = av[j]; }
        }
    }
}

// bias: g_mu_b[n] = sum_rows g_m, g_rho_b[n] = (sum_rows g_v) 2 sigma_b sigmoid(rho_b).  64 columns x 4 row groups per
// workgroup; group g adds rows g, g + 4, ... in order, the four partial sums are added in group order.
__global__ __launch_bounds__(256) void k_lrt_bias_grad(const float *__restrict__ g_m, const float *__restrict__ g_v, int64_t M, int N,
                                                       const float *__restrict__ rho_b, float *__restrict__ g_mu_b, float *__restrict__ g_rho_b)
{
    __shared__ float pm[4][64], pv[4][64];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    float sm = 0.f, sv = 0.f;
    if (n < N)
        for (int64_t r = g; r < M; r += 4) { sm += g_m[r * N + n]; sv += g_v[r * N + n]; }
    pm[g][c] = sm;
    pv[g][c] = sv;
    __syncthreads();
    if (g == 0 && n < N) {
        const float tm = ((pm[0][c] + pm[1][c]) + pm[2][c]) + pm[3][c];
        const float tv = ((pv[0][c] + pv[1][c]) + pv[2][c]) + pv[3][c];
        const float rho = rho_b[n];
        g_mu_b[n] = tm;
        g_rho_b[n] = tv * (2.0f * sigma_lrt(rho) * dsigma_lrt(rho));
    }
}

template <int MODE, typename CHAIN = ChainRho>
static int lrt_launch(const char *who, const LrtArgs &A, int compute, unsigned gz, hipStream_t st)
{
    const dim3 g((unsigned)((A.I + kLrtTile - 1) / kLrtTile), (unsigned)((A.J + kLrtTile - 1) / kLrtTile), gz), b(kLrtThreads);
    if (compute == BNN_COMPUTE_BF16) hipLaunchKernelGGL((k_lrt<uint16_t, MODE, CHAIN>), g, b, 0, st, A);
    else hipLaunchKernelGGL((k_lrt<float, MODE, CHAIN>), g, b, 0, st, A);
    return check_launch(who);
}

int lrt_bias_grad_launch(const char *who, const float *g_m, const float *g_v, int64_t M, int64_t N, const float *rho_b, float *g_mu_b,
                         float *g_rho_b, hipStream_t st)
{
    hipLaunchKernelGGL(k_lrt_bias_grad, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, st, g_m, g_v, M, (int)N, rho_b, g_mu_b, g_rho_b);
    return check_launch(who);
}

// The weight gradient of a local-reparameterization dense layer, K10's entry and K23's (bnn_vd.hip): the checks, the LRT_WGRAD
// tile with the posterior's CHAIN in its epilogue, the bias sums.  par_w: rho_w or log_sigma2; g_mean_w / g_par_w: the gradients of
// the weight's mean and of par_w.
template <typename CHAIN>
int lrt_backward_weight(const char *who, const void *x, int64_t ldx, const float *g_m, const float *g_v, const float *par_w,
                        float *g_mean_w, float *g_par_w, const float *rho_b, float *g_mu_b, float *g_rho_b, int64_t M, int64_t N,
                        int64_t K, int compute, int flags, hipStream_t st)
{
    const bool bias = rho_b || g_mu_b || g_rho_b;
    if (!x || !g_m || !g_v || !par_w || !g_mean_w || !g_par_w || (bias && (!rho_b || !g_mu_b || !g_rho_b))) {
        set_error("%s: NULL pointer", who);
        return BNN_E_NULL;
    }
    if (N < 1 || K < 1 || M < 0 || ldx < K) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (M > 0x7FFFFFFF || N > (int64_t)kLrtTile * 65535 || K > 0x7FFFFFFF) { set_error("%s: extent outside the supported range", who); return BNN_E_RANGE; }
    if (compute != BNN_COMPUTE_F32 && compute != BNN_COMPUTE_BF16) { set_error("%s: unknown compute mode", who); return BNN_E_DTYPE; }
    if ((flags & BNN_FLAG_X_BF16) && compute != BNN_COMPUTE_BF16) {
        set_error("%s: bf16 activations need the bf16 compute mode", who);
        return BNN_E_UNSUPPORTED;
    }
    if (misaligned(x, (flags & BNN_FLAG_X_BF16) ? 1 : 3) || misaligned(g_m, 3) || misaligned(g_v, 3) || misaligned(par_w, 3) ||
        misaligned(g_mean_w, 15) || misaligned(g_par_w, 15) || misaligned(rho_b, 3) || misaligned(g_mu_b, 3) || misaligned(g_rho_b, 3)) {
        set_error("%s: misaligned pointer (the two weight gradients: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    LrtArgs A{};
    A.p1 = x; A.p2 = nullptr; A.ldp = ldx;
    A.q1 = g_m; A.q2 = g_v; A.ldq = N;
    A.I = (int32_t)K; A.J = (int32_t)N; A.C = (int32_t)M;        // M == 0: no k-tile runs, the gradients are stored as zeros
    A.x_bf16 = (flags & BNN_FLAG_X_BF16) ? 1 : 0;
    A.out = g_mean_w; A.out2 = g_par_w; A.e1 = par_w;
    const int rc = lrt_launch<LRT_WGRAD, CHAIN>(who, A, compute, 1u, st);
    if (rc || !bias) return rc;
    return lrt_bias_grad_launch(who, g_m, g_v, M, N, rho_b, g_mu_b, g_rho_b, st);
}

// bnn_vd.hip's (ChainRho's is bnn_lrt_backward_weight's, below)
template int lrt_backward_weight<ChainLogSigma2>(const char *, const void *, int64_t, const float *, const float *, const float *,
                                                 float *, float *, const float *, float *, float *, int64_t, int64_t, int64_t, int, int,
                                                 hipStream_t);

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_lrt_prepare(const float *rho_w, float *s2_w, int64_t n_w, const float *rho_b, float *s2_b, int64_t n_b, void *stream)
{
    const char *who = "bnn_lrt_prepare";
    if (!rho_w || !s2_w || (n_b > 0 && (!rho_b || !s2_b))) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (n_w < 1 || n_b < 0) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (misaligned(rho_w, 3) || misaligned(s2_w, 3) || misaligned(rho_b, 3) || misaligned(s2_b, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    int64_t blocks = (n_w + n_b + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_lrt_prepare, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rho_w, s2_w, n_w, rho_b, s2_b, n_b);
    return check_launch(who);
}

int bnn_lrt_forward(const void *x, int64_t ldx, const float *mu_w, const float *s2_w, const float *mu_b, const float *s2_b,
                    void *y, float *v_out, int64_t B, int64_t N, int64_t K, int nsamples, int shared_x,
                    const bnn_rng_t *rng, int compute, int flags, void *stream)
{
    const char *who = "bnn_lrt_forward";
    if (!x || !mu_w || !s2_w || !y || (mu_b == nullptr) != (s2_b == nullptr)) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (!rng) { set_error("%s: NULL rng", who); return BNN_E_NULL; }
    int rc = lrt_check_extents(who, B, N, K);
    if (rc) return rc;
    if (nsamples < 1 || ldx < K) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (nsamples > 0xFFFF) { set_error("%s: more than 65535 samples", who); return BNN_E_RANGE; }
    if (B * N >= ((int64_t)1 << 32)) { set_error("%s: one sample has 2^32 output elements or more", who); return BNN_E_RANGE; }
    rc = check_rng(rng, nsamples);
    if (rc) { set_error("%s: bad rng", who); return rc; }
    if (compute != BNN_COMPUTE_F32 && compute != BNN_COMPUTE_BF16) { set_error("%s: unknown compute mode", who); return BNN_E_DTYPE; }
    if ((flags & (BNN_FLAG_X_BF16 | BNN_FLAG_Y_BF16)) && compute != BNN_COMPUTE_BF16) {
        set_error("%s: bf16 activations need the bf16 compute mode", who);
        return BNN_E_UNSUPPORTED;
    }
    if (misaligned(x, (flags & BNN_FLAG_X_BF16) ? 1 : 3) || misaligned(mu_w, 3) || misaligned(s2_w, 3) || misaligned(mu_b, 3) ||
        misaligned(s2_b, 3) || misaligned(y, 15) || misaligned(v_out, 15)) {
        set_error("%s: misaligned pointer (y and v: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    if (B == 0) return BNN_OK;
    LrtArgs A{};
    A.p1 = mu_w; A.p2 = s2_w; A.ldp = K;
    A.q1 = x; A.q2 = nullptr; A.ldq = ldx;
    A.I = (int32_t)N; A.J = (int32_t)B; A.C = (int32_t)K;
    A.x_bf16 = (flags & BNN_FLAG_X_BF16) ? 1 : 0;
    A.out = y; A.out2 = v_out; A.e1 = mu_b; A.e2 = s2_b;
    A.out_bf16 = (flags & BNN_FLAG_Y_BF16) ? 1 : 0;
    A.S = nsamples; A.shared = shared_x ? 1 : 0;
    A.rng = make_rng(rng);
    return lrt_launch<LRT_FWD>(who, A, compute, shared_x ? 1u : (unsigned)nsamples, (hipStream_t)stream);
}

int bnn_lrt_backward_epilogue(const void *gy, const float *v, float *g_m, float *g_v, int64_t B, int64_t N, int nsamples,
                              int shared_x, const bnn_rng_t *rng, int flags, void *stream)
{
    const char *who = "bnn_lrt_backward_epilogue";
    if (!gy || !v || !g_m || !g_v) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (!rng) { set_error("%s: NULL rng", who); return BNN_E_NULL; }
    if (B < 0 || N < 1 || nsamples < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (nsamples > 0xFFFF) { set_error("%s: more than 65535 samples", who); return BNN_E_RANGE; }
    if (B * N >= ((int64_t)1 << 32)) { set_error("%s: one sample has 2^32 output elements or more", who); return BNN_E_RANGE; }
    const int rc = check_rng(rng, nsamples);
    if (rc) { set_error("%s: bad rng", who); return rc; }
    if (misaligned(gy, (flags & BNN_FLAG_X_BF16) ? 1 : 3) || misaligned(v, 3) || misaligned(g_m, 3) || misaligned(g_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (B == 0) return BNN_OK;
    const uint32_t n = (uint32_t)(B * N);
    int64_t blocks = ((int64_t)n + 1023) / 1024;
    if (blocks > 4096) blocks = 4096;
    const RngDev rd = make_rng(rng);
    const int bf = (flags & BNN_FLAG_X_BF16) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (shared_x) hipLaunchKernelGGL((k_lrt_bwd_epilogue<true>), dim3((unsigned)blocks), dim3(256), 0, st, gy, bf, v, g_m, g_v, n, nsamples, rd);
    else hipLaunchKernelGGL((k_lrt_bwd_epilogue<false>), dim3((unsigned)blocks, (unsigned)nsamples), dim3(256), 0, st, gy, bf, v, g_m, g_v, n, nsamples, rd);
    return check_launch(who);
}

int bnn_lrt_backward_input(const float *g_m, const float *g_v, const float *mu_w, const float *s2_w, const void *x, int64_t ldx,
                           void *gx, int64_t M, int64_t N, int64_t K, int compute, int flags, void *stream)
{
    const char *who = "bnn_lrt_backward_input";
    if (!g_m || !g_v || !mu_w || !s2_w || !x || !gx) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    int rc = lrt_check_extents(who, M, N, K);
    if (rc) return rc;
    if (ldx < K) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (compute != BNN_COMPUTE_F32 && compute != BNN_COMPUTE_BF16) { set_error("%s: unknown compute mode", who); return BNN_E_DTYPE; }
    if ((flags & (BNN_FLAG_X_BF16 | BNN_FLAG_Y_BF16)) && compute != BNN_COMPUTE_BF16) {
        set_error("%s: bf16 activations need the bf16 compute mode", who);
        return BNN_E_UNSUPPORTED;
    }
    if (misaligned(g_m, 3) || misaligned(g_v, 3) || misaligned(mu_w, 3) || misaligned(s2_w, 3) ||
        misaligned(x, (flags & BNN_FLAG_X_BF16) ? 1 : 3) || misaligned(gx, 15)) {
        set_error("%s: misaligned pointer (gx: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    if (M == 0) return BNN_OK;
    LrtArgs A{};
    A.p1 = mu_w; A.p2 = s2_w; A.ldp = K;
    A.q1 = g_m; A.q2 = g_v; A.ldq = N;
    A.I = (int32_t)K; A.J = (int32_t)M; A.C = (int32_t)N;
    A.x = x; A.ldx = ldx;
    A.x_bf16 = (flags & BNN_FLAG_X_BF16) ? 1 : 0;
    A.out = gx;
    A.out_bf16 = (flags & BNN_FLAG_Y_BF16) ? 1 : 0;
    return lrt_launch<LRT_DGRAD>(who, A, compute, 1u, (hipStream_t)stream);
}

int bnn_lrt_backward_weight(const void *x, int64_t ldx, const float *g_m, const float *g_v, const float *rho_w, float *g_mu_w,
                            float *g_rho_w, const float *rho_b, float *g_mu_b, float *g_rho_b, int64_t M, int64_t N, int64_t K,
                            int compute, int flags, void *stream)
{
    return lrt_backward_weight<ChainRho>("bnn_lrt_backward_weight", x, ldx, g_m, g_v, rho_w, g_mu_w, g_rho_w, rho_b, g_mu_b, g_rho_b,
                                         M, N, K, compute, flags, (hipStream_t)stream);
}

}  // extern "C"
