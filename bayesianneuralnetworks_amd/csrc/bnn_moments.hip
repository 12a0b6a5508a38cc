// bnn_moments.hip -- K16: sampling-free inference by moment propagation through dense layers (Frey & Hinton 1999;
// Hernandez-Lobato & Adams 2015; Wu et al. 2019).  A layer takes a mean and a variance per input element, independent across
// elements, and hands on the mean and variance of its pre-activation for independent Gaussian w ~ N(mu_w, sigma_w^2),
// b ~ N(mu_b, sigma_b^2):
//     m = a_m mu_w^T + mu_b
//     v = a_m^2 (sigma_w^2)^T + a_v (mu_w^2 + sigma_w^2)^T + sigma_b^2          (second term absent for a deterministic input)
// Every addend of v is non-negative: no difference of second moments is formed.
//
// The contraction tile of bnn_lrt_tile.hpp with BK = 32 and, for an input that carries a variance, three planes per operand:
//     P planes (MFMA A)   mu_w,  sigma_w^2,  [mu_w^2 + sigma_w^2]      Q planes (MFMA B)   a_m,  a_m^2,  [a_v]
// The two variance contractions add into ONE accumulator set, so a lane holds K10's 32 accumulator registers.
// Epilogue: + mu_b / + sigma_b^2, then (BNN_FLAG_RELU) the moment-matched ReLU moments_relu_dev (bnn_moments_act.hpp) -- the
// function the standalone launch calls, so fused and standalone agree bit for bit.  Outputs fp32 (B, N).
// The elementwise launches k_moments_relu / k_moments_elu (K17: the conv tile's epilogue functions, bnn_conv3d.hip) live here too.
#include "bnn_lrt_tile.hpp"
#include "bnn_moments_act.hpp"

namespace bnn {

struct MomArgs {
    const void *a_m;            // (B, K) fp32 or (deterministic input, bf16 compute) bf16, row pitch lda
    const float *a_v;           // (B, K) fp32, row pitch lda; NULL in the deterministic instantiation
    int64_t lda;
    const float *mu_w, *s2_w;   // (N, K)
    const float *mu_b, *s2_b;   // (N), both or neither
    float *out_m, *out_v;       // (B, N)
    int32_t B, N, K;
    int32_t a_bf16, relu;
};

// T = float (fp32 compute) or uint16_t (bf16 compute); VAR: the input carries a variance (three contractions instead of two)
template <typename T, bool VAR>
__global__ __launch_bounds__(kLrtThreads) void k_moments(const MomArgs A)
{
    constexpr bool BF = sizeof(T) == 2;
    constexpr int BK = 32;
    constexpr int LDK = BF ? BK + 8 : BK + 1;       // bf16: rows stay 16-byte aligned for the 8-element fragment read
    constexpr int EPT = BK / 4;
    constexpr int NPL = VAR ? 3 : 2;                // planes per operand
    __shared__ __attribute__((aligned(16))) T lds[2 * NPL * kLrtTile * LDK];
    T *lp = lds, *lq = lds + NPL * kLrtTile * LDK;

    const int i0 = blockIdx.x * kLrtTile, j0 = blockIdx.y * kLrtTile;
    const bool a_bf = !VAR && A.a_bf16;

    f32x4 accm[2][2], accv[2][2];
    lrt_zero(accm, accv);
    float rmu[EPT], rs2[EPT], ram[EPT], rav[EPT] = {};
    auto fetch = [&](int c0) {
        lrt_fetch<false, BK>(rmu, A.mu_w, false, A.K, i0, A.N, c0, A.K);
        lrt_fetch<false, BK>(rs2, A.s2_w, false, A.K, i0, A.N, c0, A.K);
        lrt_fetch<false, BK>(ram, A.a_m, a_bf, A.lda, j0, A.B, c0, A.K);
        if constexpr (VAR) lrt_fetch<false, BK>(rav, A.a_v, false, A.lda, j0, A.B, c0, A.K);
    };
    fetch(0);
    for (int c0 = 0; c0 < A.K; c0 += BK) {
        lrt_stage2<T, false, false, false, true, NPL, BK, LDK>(lp, lq, rmu, rs2, ram, rav);
        __syncthreads();
        if (c0 + BK < A.K) fetch(c0 + BK);
        lrt_mfma_block<T, NPL, BK, LDK>(accm, accv, lp, lq);
        __syncthreads();
    }

    const bool vec = (A.N & 3) == 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            LrtQuad q;
            if (!lrt_quad(q, a, b, A.N, A.B)) continue;
            float rm[4] = {accm[a][b][0], accm[a][b][1], accm[a][b][2], accm[a][b][3]};
            float rv[4] = {accv[a][b][0], accv[a][b][1], accv[a][b][2], accv[a][b][3]};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (A.mu_b && r < q.ni) { rm[r] += A.mu_b[q.i + r]; rv[r] += A.s2_b[q.i + r]; }
                if (A.relu) moments_relu_dev(rm[r], rv[r], rm[r], rv[r]);
            }
            const int64_t o = (int64_t)q.j * A.N + q.i;
            lrt_store4x2(A.out_m + o, rm, A.out_v + o, rv, vec, q.ni);
        }
}

// the same ReLU as an elementwise launch (in place allowed: every element is read before it is written, by its own thread)
__global__ __launch_bounds__(256) void k_moments_relu(const float *m, const float *v, float *om, float *ov, int64_t n)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        float a, b;
        moments_relu_dev(m[t], v[t], a, b);
        om[t] = a;
        ov[t] = b;
    }
}

// the moment-matched ELU (moments_elu_dev, bnn_moments_act.hpp) as an elementwise launch; in place allowed, as above
__global__ __launch_bounds__(256) void k_moments_elu(const float *m, const float *v, float *om, float *ov, int64_t n, float alpha)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        float a, b;
        moments_elu_dev(m[t], v[t], alpha, a, b);
        om[t] = a;
        ov[t] = b;
    }
}

// y_s[e] = m[e] + sqrt(v[e] + 1e-16) eps_s[e]: one thread per quad of the flat index e = b N + n, all S samples (lrt_noise4: the
// fma and the eps quad of K10's epilogue).  VEC: n % 4 == 0, 16-byte loads and stores.
template <bool VEC>
__global__ __launch_bounds__(256) void k_moments_sample(const float *__restrict__ m, const float *__restrict__ v, float *__restrict__ y,
                                                        uint32_t n, int S, RngDev rng)
{
    const uint32_t ed = rng_epoch_dev(rng);
    const uint32_t nq = (n + 3u) >> 2;
    for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const uint32_t e0 = 4u * q;
        const int ne = n - e0 < 4u ? (int)(n - e0) : 4;
        float mm[4] = {0.f, 0.f, 0.f, 0.f}, sd[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            const float4 m4 = *reinterpret_cast<const float4 *>(m + e0), v4 = *reinterpret_cast<const float4 *>(v + e0);
            mm[0] = m4.x; mm[1] = m4.y; mm[2] = m4.z; mm[3] = m4.w;
            sd[0] = v4.x; sd[1] = v4.y; sd[2] = v4.z; sd[3] = v4.w;
        } else {
            for (int r = 0; r < ne; ++r) { mm[r] = m[e0 + r]; sd[r] = v[e0 + r]; }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sd[r] = sqrtf(sd[r] + 1e-16f);
        for (int s = 0; s < S; ++s) {
            float yy[4];
            lrt_noise4(yy, mm, sd, rng, ed, e0, rng.sample0 + (uint32_t)s, true, 4);
            lrt_store4(y + (int64_t)s * n + e0, yy, VEC, ne);
        }
    }
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_moments_forward(const void *a_m, const float *a_v, int64_t lda, const float *mu_w, const float *s2_w, const float *mu_b,
                        const float *s2_b, float *out_m, float *out_v, int64_t B, int64_t N, int64_t K, int compute, int flags,
                        void *stream)
{
    const char *who = "bnn_moments_forward";
    if (!a_m || !mu_w || !s2_w || !out_m || !out_v || (mu_b == nullptr) != (s2_b == nullptr)) {
        set_error("%s: NULL pointer", who);
        return BNN_E_NULL;
    }
    if (lda < K) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    const int rc = lrt_check_extents(who, B, N, K);
    if (rc) return rc;
    if (compute != BNN_COMPUTE_F32 && compute != BNN_COMPUTE_BF16) { set_error("%s: unknown compute mode", who); return BNN_E_DTYPE; }
    if (flags & ~(BNN_FLAG_RELU | BNN_FLAG_X_BF16)) { set_error("%s: unknown flag", who); return BNN_E_UNSUPPORTED; }
    if ((flags & BNN_FLAG_X_BF16) && (compute != BNN_COMPUTE_BF16 || a_v)) {
        set_error("%s: a bf16 a_m needs the bf16 compute mode and a deterministic input (hidden moments are fp32)", who);
        return BNN_E_UNSUPPORTED;
    }
    if (misaligned(a_m, (flags & BNN_FLAG_X_BF16) ? 1 : 3) || misaligned(a_v, 3) || misaligned(mu_w, 3) ||
        misaligned(s2_w, 3) || misaligned(mu_b, 3) || misaligned(s2_b, 3) || misaligned(out_m, 15) ||
        misaligned(out_v, 15)) {
        set_error("%s: misaligned pointer (out_m and out_v: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    if (B == 0) return BNN_OK;
    MomArgs A{};
    A.a_m = a_m; A.a_v = a_v; A.lda = lda;
    A.mu_w = mu_w; A.s2_w = s2_w; A.mu_b = mu_b; A.s2_b = s2_b;
    A.out_m = out_m; A.out_v = out_v;
    A.B = (int32_t)B; A.N = (int32_t)N; A.K = (int32_t)K;
    A.a_bf16 = (flags & BNN_FLAG_X_BF16) ? 1 : 0;
    A.relu = (flags & BNN_FLAG_RELU) ? 1 : 0;
    const dim3 g((unsigned)((N + kLrtTile - 1) / kLrtTile), (unsigned)((B + kLrtTile - 1) / kLrtTile)), b(kLrtThreads);
    hipStream_t st = (hipStream_t)stream;
    if (compute == BNN_COMPUTE_BF16) {
        if (a_v) hipLaunchKernelGGL((k_moments<uint16_t, true>), g, b, 0, st, A);
        else hipLaunchKernelGGL((k_moments<uint16_t, false>), g, b, 0, st, A);
    } else {
        if (a_v) hipLaunchKernelGGL((k_moments<float, true>), g, b, 0, st, A);
        else hipLaunchKernelGGL((k_moments<float, false>), g, b, 0, st, A);
    }
    return check_launch(who);
}

int bnn_moments_relu(const float *m, const float *v, float *out_m, float *out_v, int64_t n, void *stream)
{
    const char *who = "bnn_moments_relu";
    if (!m || !v || !out_m || !out_v) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (n < 0) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (misaligned(m, 3) || misaligned(v, 3) || misaligned(out_m, 3) || misaligned(out_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (n == 0) return BNN_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_moments_relu, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m, v, out_m, out_v, n);
    return check_launch(who);
}

int bnn_moments_elu(const float *m, const float *v, float *out_m, float *out_v, int64_t n, float alpha, void *stream)
{
    const char *who = "bnn_moments_elu";
    if (!m || !v || !out_m || !out_v) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (n < 0) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (!(alpha >= 0.0f) || alpha > 3.0e38f) { set_error("%s: alpha must be finite and >= 0", who); return BNN_E_RANGE; }
    if (misaligned(m, 3) || misaligned(v, 3) || misaligned(out_m, 3) || misaligned(out_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (n == 0) return BNN_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_moments_elu, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m, v, out_m, out_v, n, alpha);
    return check_launch(who);
}

int bnn_moments_sample(const float *m, const float *v, float *y, int64_t rows, int64_t N, int nsamples, const bnn_rng_t *rng,
                       int flags, void *stream)
{
    const char *who = "bnn_moments_sample";
    if (!m || !v || !y) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (!rng) { set_error("%s: NULL rng", who); return BNN_E_NULL; }
    if (rows < 0 || N < 1 || nsamples < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (nsamples > 0xFFFF) { set_error("%s: more than 65535 samples", who); return BNN_E_RANGE; }
    if (rows >= ((int64_t)1 << 32) || N >= ((int64_t)1 << 32) || rows * N >= ((int64_t)1 << 32)) {
        set_error("%s: one sample has 2^32 output elements or more", who);
        return BNN_E_RANGE;
    }
    const int rc = check_rng(rng, nsamples);
    if (rc) { set_error("%s: bad rng", who); return rc; }
    if (flags) { set_error("%s: unknown flag (the samples are fp32)", who); return BNN_E_UNSUPPORTED; }
    if (misaligned(m, 15) || misaligned(v, 15) || misaligned(y, 15)) {
        set_error("%s: misaligned pointer (m, v, y: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    if (rows == 0) return BNN_OK;
    const uint32_t n = (uint32_t)(rows * N);
    int64_t blocks = ((int64_t)n + 1023) / 1024;
    if (blocks > 4096) blocks = 4096;
    const RngDev rd = make_rng(rng);
    hipStream_t st = (hipStream_t)stream;
    if ((n & 3u) == 0) hipLaunchKernelGGL((k_moments_sample<true>), dim3((unsigned)blocks), dim3(256), 0, st, m, v, y, n, nsamples, rd);
    else hipLaunchKernelGGL((k_moments_sample<false>), dim3((unsigned)blocks), dim3(256), 0, st, m, v, y, n, nsamples, rd);
    return check_launch(who);
}

}  // extern "C"
