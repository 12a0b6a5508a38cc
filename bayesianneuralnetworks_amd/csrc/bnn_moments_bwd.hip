// bnn_moments_bwd.hip -- K18: the backward of K16's dense moment layer (bnn_moments.hip), for training without sampling
// (Wu et al. 2019).  With G_m, G_v the (B, N) gradients with respect to
//     m = a_m mu_w^T + mu_b,   v = a_m^2 (sigma_w^2)^T + a_v (mu_w^2 + sigma_w^2)^T + sigma_b^2
// the gradients of a layer whose input carries a variance are
//     g_a_m  = G_m mu_w + 2 a_m (.) (G_v sigma_w^2)            g_a_v = G_v (mu_w^2 + sigma_w^2)              contraction over n
//     g_mu_w = G_m^T a_m + 2 mu_w (.) (G_v^T a_v)              g_s2_w = G_v^T (a_m^2 + a_v)                  over the rows, in row order
//     g_rho_w = g_s2_w 2 sigma_w sigmoid(rho_w);   bias: k_lrt_bias_grad (bnn_lrt.hip) as it is
// Both have one shape on the tile of bnn_lrt_tile.hpp (BK = 32): P planes (p1, p2, fma(p1, p1, p2)) -- the third formed in fp32
// by the loader before any rounding, as the forward forms mu_w^2 + sigma_w^2 --, Q planes (G_m, G_v) with G_v serving twice
// (staged once), three accumulator sets (lrt_mfma_block3), and the epilogue out1 = acc1 + 2 x (.) acc2, out2 = acc3 [chain]:
//     input gradient    P = (mu_w, sigma_w^2)^T    Q = (G_m, G_v)      x = a_m
//     weight gradient   P = (a_m, a_v)^T           Q = (G_m, G_v)^T    x = mu_w,   out2 times 2 sigma_w sigmoid(rho_w)
// bf16 compute: the five planes rounded to bf16 (RNE) as they are staged, fp32 accumulate; fp32: the ordered fma chain of
// v_mfma_f32_16x16x4_f32.  No atomics, no split contraction: identical calls give identical bits.
// A deterministic input (a_v NULL) has K10's backward: the host calls bnn_lrt_backward_input / _weight, there is no kernel here.
// k_moments_relu_bwd: the backward of the moment-matched ReLU on the forward's own terms (bnn_moments_act.hpp).
// k_moments_elu_bwd (K19): the same for the moment-matched ELU, in fp64 like its forward.  The conv layers' contraction backward is
// k_moments_conv3d_bwd in bnn_conv3d.hip.
#include "bnn_lrt_tile.hpp"
#include "bnn_moments_act.hpp"

namespace bnn {

enum { MOMB_INPUT = 0, MOMB_WEIGHT = 1 };

struct MomBwdArgs {
    const float *p1, *p2;       // P planes, element (i, c) at p[c ldp + i]
    const float *q1, *q2;       // G_m, G_v: (rows, N), row pitch N
    int64_t ldp;
    int32_t I, J, C;            // output extents (i: contiguous in memory, = K) and the contraction length
    const float *x;             // the epilogue's factor, element (j, i) at x[j ldx + i]
    int64_t ldx;
    const float *rho;           // weight gradient: rho_w (N, K)
    float *out1, *out2;         // (J, I)
};

// T = float (fp32 compute) or uint16_t (bf16 compute)
template <typename T, int MODE>
__global__ __launch_bounds__(kLrtThreads) void k_moments_bwd(const MomBwdArgs A)
{
    constexpr bool BF = sizeof(T) == 2;
    constexpr int BK = 32;
    constexpr int LDK = BF ? BK + 8 : BK + 1;       // bf16: rows stay 16-byte aligned for the 8-element fragment read
    constexpr int EPT = BK / 4;
    constexpr bool Q_TR = MODE == MOMB_WEIGHT;      // input gradient: Q rows are rows of G (contraction index n contiguous)
    __shared__ __attribute__((aligned(16))) T lds[5 * kLrtTile * LDK];
    T *lp = lds, *lq = lds + 3 * kLrtTile * LDK;

    const int i0 = blockIdx.x * kLrtTile, j0 = blockIdx.y * kLrtTile;
    const int64_t ldq = MODE == MOMB_WEIGHT ? A.J : A.C;            // N

    f32x4 acc1[2][2], acc2[2][2], acc3[2][2];
    lrt_zero(acc1, acc2);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc3[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    float rp1[EPT], rp2[EPT], rq1[EPT], rq2[EPT];
    auto fetch = [&](int c0) {
        lrt_fetch<true, BK>(rp1, A.p1, false, A.ldp, i0, A.I, c0, A.C);
        lrt_fetch<true, BK>(rp2, A.p2, false, A.ldp, i0, A.I, c0, A.C);
        lrt_fetch<Q_TR, BK>(rq1, A.q1, false, ldq, j0, A.J, c0, A.C);
        lrt_fetch<Q_TR, BK>(rq2, A.q2, false, ldq, j0, A.J, c0, A.C);
    };
    fetch(0);
    for (int c0 = 0; c0 < A.C; c0 += BK) {
        lrt_stage<T, true, false, 3, BK, LDK>(lp, rp1, rp2);
        lrt_stage<T, Q_TR, false, 2, BK, LDK>(lq, rq1, rq2);
        __syncthreads();
        if (c0 + BK < A.C) fetch(c0 + BK);
        lrt_mfma_block3<T, BK, LDK>(acc1, acc2, acc3, lp, lq);
        __syncthreads();
    }

    const bool vec = (A.I & 3) == 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            LrtQuad q;
            if (!lrt_quad(q, a, b, A.I, A.J)) continue;
            const int64_t o = (int64_t)q.j * A.I + q.i;
            float r1[4] = {0.f, 0.f, 0.f, 0.f}, r2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (r >= q.ni) continue;
                r1[r] =__builtin_fmaf(2.0f * A.x[(int64_t)q.j * A.ldx + q.i + r], acc2[a][b][r], acc1[a][b][r]);
                r2[r] = acc3[a][b][r];
                if constexpr (MODE == MOMB_WEIGHT) {
                    const float rho = A.rho[o + r];
                    r2[r] *= 2.0f * sigma_lrt(rho) * dsigma_lrt(rho);
                }
            }
            lrt_store4x2(A.out1 + o, r1, A.out2 + o, r2, vec, q.ni);
        }
}

// (g_m, g_v) of the pre-activation from (g_out_m, g_out_v) of the moment-matched ReLU's outputs; in place on the gradients allowed
__global__ __launch_bounds__(256) void k_moments_relu_bwd(const float *m, const float *v, const float *gom, const float *gov, float *gm,
                                                          float *gv, int64_t n)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        float a, b;
        moments_relu_bwd_dev(m[t], v[t], gom[t], gov[t], a, b);
        gm[t] = a;
        gv[t] = b;
    }
}

// the same for the moment-matched ELU (K19; moments_elu_bwd_dev evaluates in fp64, like the forward)
__global__ __launch_bounds__(256) void k_moments_elu_bwd(const float *m, const float *v, const float *gom, const float *gov, float *gm,
                                                         float *gv, int64_t n, float alpha)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        float a, b;
        moments_elu_bwd_dev(m[t], v[t], alpha, gom[t], gov[t], a, b);
        gm[t] = a;
        gv[t] = b;
    }
}

template <int MODE>
static int momb_launch(const char *who, const MomBwdArgs &A, int compute, hipStream_t st)
{
    const dim3 g((unsigned)((A.I + kLrtTile - 1) / kLrtTile), (unsigned)((A.J + kLrtTile - 1) / kLrtTile)), b(kLrtThreads);
    if (compute == BNN_COMPUTE_BF16) hipLaunchKernelGGL((k_moments_bwd<uint16_t, MODE>), g, b, 0, st, A);
    else hipLaunchKernelGGL((k_moments_bwd<float, MODE>), g, b, 0, st, A);
    return check_launch(who);
}

static int momb_check_mode(const char *who, int compute, int flags)
{
    if (compute != BNN_COMPUTE_F32 && compute != BNN_COMPUTE_BF16) { set_error("%s: unknown compute mode", who); return BNN_E_DTYPE; }
    if (flags) { set_error("%s: unknown flag (every operand and every gradient is fp32)", who); return BNN_E_UNSUPPORTED; }
    return BNN_OK;
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_moments_backward_input(const float *g_m, const float *g_v, const float *mu_w, const float *s2_w, const float *a_m, int64_t lda,
                               float *g_a_m, float *g_a_v, int64_t B, int64_t N, int64_t K, int compute, int flags, void *stream)
{
    const char *who = "bnn_moments_backward_input";
    if (!g_m || !g_v || !mu_w || !s2_w || !a_m || !g_a_m || !g_a_v) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (lda < K) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    int rc = lrt_check_extents(who, B, N, K);
    if (rc) return rc;
    rc = momb_check_mode(who, compute, flags);
    if (rc) return rc;
    if (misaligned(g_m, 3) || misaligned(g_v, 3) || misaligned(mu_w, 3) || misaligned(s2_w, 3) || misaligned(a_m, 3) ||
        misaligned(g_a_m, 15) || misaligned(g_a_v, 15)) {
        set_error("%s: misaligned pointer (g_a_m and g_a_v: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    if (B == 0) return BNN_OK;
    MomBwdArgs A{};
    A.p1 = mu_w; A.p2 = s2_w; A.ldp = K;
    A.q1 = g_m; A.q2 = g_v;
    A.I = (int32_t)K; A.J = (int32_t)B; A.C = (int32_t)N;
    A.x = a_m; A.ldx = lda;
    A.out1 = g_a_m; A.out2 = g_a_v;
    return momb_launch<MOMB_INPUT>(who, A, compute, (hipStream_t)stream);
}

int bnn_moments_backward_weight(const float *a_m, const float *a_v, int64_t lda, const float *g_m, const float *g_v, const float *mu_w,
                                const float *rho_w, float *g_mu_w, float *g_rho_w, const float *rho_b, float *g_mu_b, float *g_rho_b,
                                int64_t B, int64_t N, int64_t K, int compute, int flags, void *stream)
{
    const char *who = "bnn_moments_backward_weight";
    const bool bias = rho_b || g_mu_b || g_rho_b;
    if (!a_m || !a_v || !g_m || !g_v || !mu_w || !rho_w || !g_mu_w || !g_rho_w || (bias && (!rho_b || !g_mu_b || !g_rho_b))) {
        set_error("%s: NULL pointer", who);
        return BNN_E_NULL;
    }
    if (N < 1 || K < 1 || B < 0 || lda < K) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (B > (int64_t)kLrtTile * 65535 || N > (int64_t)kLrtTile * 65535 || K > 0x7FFFFFFF) {
        set_error("%s: extent outside the supported range (rows, N <= 64 * 65535, K < 2^31)", who);
        return BNN_E_RANGE;
    }
    const int rc = momb_check_mode(who, compute, flags);
    if (rc) return rc;
    if (misaligned(a_m, 3) || misaligned(a_v, 3) || misaligned(g_m, 3) || misaligned(g_v, 3) || misaligned(mu_w, 3) ||
        misaligned(rho_w, 3) || misaligned(g_mu_w, 15) || misaligned(g_rho_w, 15) || misaligned(rho_b, 3) || misaligned(g_mu_b, 3) ||
        misaligned(g_rho_b, 3)) {
        set_error("%s: misaligned pointer (g_mu_w and g_rho_w: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    MomBwdArgs A{};
    A.p1 = a_m; A.p2 = a_v; A.ldp = lda;
    A.q1 = g_m; A.q2 = g_v;
    A.I = (int32_t)K; A.J = (int32_t)N; A.C = (int32_t)B;        // B == 0: no k-tile runs, the gradients are stored as zeros
    A.x = mu_w; A.ldx = K;
    A.rho = rho_w;
    A.out1 = g_mu_w; A.out2 = g_rho_w;
    const int rl = momb_launch<MOMB_WEIGHT>(who, A, compute, (hipStream_t)stream);
    if (rl || !bias) return rl;
    return lrt_bias_grad_launch(who, g_m, g_v, B, N, rho_b, g_mu_b, g_rho_b, (hipStream_t)stream);
}

int bnn_moments_relu_backward(const float *m, const float *v, const float *g_out_m, const float *g_out_v, float *g_m, float *g_v,
                              int64_t n, void *stream)
{
    const char *who = "bnn_moments_relu_backward";
    if (!m || !v || !g_out_m || !g_out_v || !g_m || !g_v) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (n < 0) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (misaligned(m, 3) || misaligned(v, 3) || misaligned(g_out_m, 3) || misaligned(g_out_v, 3) || misaligned(g_m, 3) ||
        misaligned(g_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (n == 0) return BNN_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_moments_relu_bwd, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m, v, g_out_m, g_out_v, g_m, g_v, n);
    return check_launch(who);
}

int bnn_moments_elu_backward(const float *m, const float *v, const float *g_out_m, const float *g_out_v, float *g_m, float *g_v,
                             int64_t n, float alpha, void *stream)
{
    const char *who = "bnn_moments_elu_backward";
    if (!m || !v || !g_out_m || !g_out_v || !g_m || !g_v) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (n < 0) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (!(alpha >= 0.0f) || alpha > 3.0e38f) { set_error("%s: alpha must be finite and >= 0", who); return BNN_E_RANGE; }
    if (misaligned(m, 3) || misaligned(v, 3) || misaligned(g_out_m, 3) || misaligned(g_out_v, 3) || misaligned(g_m, 3) ||
        misaligned(g_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (n == 0) return BNN_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_moments_elu_bwd, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m, v, g_out_m, g_out_v, g_m, g_v, n,
                       alpha);
    return check_launch(who);
}

}  // extern "C"
