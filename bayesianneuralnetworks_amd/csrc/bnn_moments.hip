// bnn_moments.hip -- K16: sampling-free inference by moment propagation through dense layers (Frey & Hinton 1999;
// Hernandez-Lobato & Adams 2015; Wu et al. 2019).  A layer takes a mean and a variance per input element, independent across
// elements, and hands on the mean and variance of its pre-activation for independent Gaussian w ~ N(mu_w, sigma_w^2),
// b ~ N(mu_b, sigma_b^2):
//     m = a_m mu_w^T + mu_b
//     v = a_m^2 (sigma_w^2)^T + a_v (mu_w^2 + sigma_w^2)^T + sigma_b^2          (second term absent for a deterministic input)
// Every addend of v is non-negative: no difference of second moments is formed.
//
// One tile on K10's skeleton (bnn_lrt.hip): 64 x 64 outputs, 4 waves of 32 x 32, operands through registers, one LDS stage with
// the next tile's global loads issued before the MFMAs of the current one.  Three contractions from one pass over the operands:
//     P planes (MFMA A)   mu_w,  sigma_w^2,  mu_w^2 + sigma_w^2        Q planes (MFMA B)   a_m,  a_m^2,  a_v
// The derived planes (fma(mu_w, mu_w, sigma_w^2) and a_m a_m) are formed in fp32 by the loader as it stages them, before any bf16
// rounding.  The two variance contractions add into ONE accumulator set, so a lane holds K10's 32 accumulator registers.
// bf16 compute: all planes rounded to bf16 (RNE) as they are written to LDS, v_mfma_f32_16x16x32_bf16.  fp32: v_mfma_f32_16x16x4_f32.
// Epilogue: + mu_b / + sigma_b^2, then (BNN_FLAG_RELU) the moment-matched ReLU moments_relu_dev -- the function the standalone
// launch calls, so fused and standalone agree bit for bit.  Outputs fp32 (B, N), 16-byte stores (scalar when N % 4 != 0).
// No atomics, no split of the contraction: identical calls give identical bits.
#include "bnn_lrt_tile.hpp"

namespace bnn {

// ReLU of a Gaussian pre-activation N(m, v) by moment matching, s = sqrt(v), alpha = m / s, Phi / phi the standard normal cdf / pdf:
//     mean' = s (alpha Phi + phi)
//     var'  = v (Phi + alpha^2 Phi Phi_c + alpha phi (Phi_c - Phi) - phi^2),   Phi_c = Phi(-alpha),   clamped at 0
// (E[y^2] - mean'^2 with m^2 never subtracted from m^2 + v).  Beyond |alpha| = 40 Phi_c and phi are zero in fp32 and the form is
// its own limit: the input passes (alpha > 0) or (0, 0) comes out; v == 0 (alpha infinite or 0 / 0) takes that branch too.
__device__ __forceinline__ void moments_relu_dev(float m, float v, float &om, float &ov)
{
    const float s = sqrtf(v);
    const float alpha = m / s;
    if (!(fabsf(alpha) < 40.0f)) {
        om = fmaxf(m, 0.0f);
        ov = m > 0.0f ? v : 0.0f;
        return;
    }
    const float cdf = 0.5f * erfcf(-0.70710678118654752f * alpha);
    const float cdc = 0.5f * erfcf(0.70710678118654752f * alpha);
    const float pdf = 0.39894228040143268f * expf(-0.5f * alpha * alpha);
    om = s * (alpha * cdf + pdf);
    const float r = cdf + alpha * alpha * cdf * cdc + alpha * pdf * (cdc - cdf) - pdf * pdf;
    ov = fmaxf(v * r, 0.0f);
}

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
    constexpr int PL = kLrtTile * LDK;
    __shared__ __attribute__((aligned(16))) T lds[2 * NPL * PL];
    T *lp = lds, *lq = lds + NPL * PL;              // P planes: mu_w, s2_w, [mu_w^2 + s2_w]; Q planes: a_m, a_m^2, [a_v]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int i0 = blockIdx.x * kLrtTile, j0 = blockIdx.y * kLrtTile;
    const bool a_bf = !VAR && A.a_bf16;

    f32x4 accm[2][2], accv[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { accm[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; accv[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    float rmu[EPT], rs2[EPT], ram[EPT], rav[EPT] = {};
    auto fetch = [&](int c0) {
        lrt_fetch<false, BK>(rmu, A.mu_w, false, A.K, i0, A.N, c0, A.K);
        lrt_fetch<false, BK>(rs2, A.s2_w, false, A.K, i0, A.N, c0, A.K);
        lrt_fetch<false, BK>(ram, A.a_m, a_bf, A.lda, j0, A.B, c0, A.K);
        if constexpr (VAR) lrt_fetch<false, BK>(rav, A.a_v, false, A.lda, j0, A.B, c0, A.K);
    };
    fetch(0);
    for (int c0 = 0; c0 < A.K; c0 += BK) {
#pragma unroll
        for (int it = 0; it < EPT; ++it) {
            const int idx = it * kLrtThreads + (int)threadIdx.x;
            const int o = (idx / BK) * LDK + idx % BK;
            lp[o] = lrt_cvt<T>(rmu[it]);
            lp[PL + o] = lrt_cvt<T>(rs2[it]);
            lq[o] = lrt_cvt<T>(ram[it]);
            lq[PL + o] = lrt_cvt<T>(ram[it] * ram[it]);
            if constexpr (VAR) {
                lp[2 * PL + o] = lrt_cvt<T>(__builtin_fmaf(rmu[it], rmu[it], rs2[it]));
                lq[2 * PL + o] = lrt_cvt<T>(rav[it]);
            }
        }
        __syncthreads();
        if (c0 + BK < A.K) fetch(c0 + BK);
        const int pr = (wi * 32 + (lane & 15)) * LDK, qr = (wj * 32 + (lane & 15)) * LDK;
        if constexpr (BF) {
#pragma unroll
            for (int kk = 0; kk < BK / 32; ++kk) {
                const int ko = kk * 32 + 8 * (lane >> 4);
                s16x8 fp[NPL][2], fq[NPL][2];
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        fp[pl][a] = *reinterpret_cast<const s16x8 *>(lp + pl * PL + pr + a * 16 * LDK + ko);
                        fq[pl][a] = *reinterpret_cast<const s16x8 *>(lq + pl * PL + qr + a * 16 * LDK + ko);
                    }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        accm[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fp[0][a]),
                                                                             __builtin_bit_cast(bf16x8, fq[0][b]), accm[a][b], 0, 0, 0);
                        accv[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fp[1][a]),
                                                                             __builtin_bit_cast(bf16x8, fq[1][b]), accv[a][b], 0, 0, 0);
                    }
                if constexpr (VAR) {
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int b = 0; b < 2; ++b)
                            accv[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fp[2][a]),
                                                                                 __builtin_bit_cast(bf16x8, fq[2][b]), accv[a][b], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                const int ko = kk * 4 + (lane >> 4);
                float fp[NPL][2], fq[NPL][2];
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        fp[pl][a] = lp[pl * PL + pr + a * 16 * LDK + ko];
                        fq[pl][a] = lq[pl * PL + qr + a * 16 * LDK + ko];
                    }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        accm[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fp[0][a], fq[0][b], accm[a][b], 0, 0, 0);
                        accv[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fp[1][a], fq[1][b], accv[a][b], 0, 0, 0);
                    }
                if constexpr (VAR) {
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int b = 0; b < 2; ++b)
                            accv[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fp[2][a], fq[2][b], accv[a][b], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ----- epilogue: lane holds out[j][i .. i + 3], i = i0 + 32 wi + 16 a + 4 (lane >> 4), j = j0 + 32 wj + 16 b + (lane & 15)
    const bool vec = (A.N & 3) == 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i = i0 + wi * 32 + a * 16 + 4 * (lane >> 4);
            const int j = j0 + wj * 32 + b * 16 + (lane & 15);
            if (i >= A.N || j >= A.B) continue;
            const int ni = A.N - i < 4 ? A.N - i : 4;
            float rm[4] = {accm[a][b][0], accm[a][b][1], accm[a][b][2], accm[a][b][3]};
            float rv[4] = {accv[a][b][0], accv[a][b][1], accv[a][b][2], accv[a][b][3]};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (A.mu_b && r < ni) { rm[r] += A.mu_b[i + r]; rv[r] += A.s2_b[i + r]; }
                if (A.relu) moments_relu_dev(rm[r], rv[r], rm[r], rv[r]);
            }
            float *mo = A.out_m + (int64_t)j * A.N + i, *vo = A.out_v + (int64_t)j * A.N + i;
            if (vec) {
                *reinterpret_cast<float4 *>(mo) = make_float4(rm[0], rm[1], rm[2], rm[3]);
                *reinterpret_cast<float4 *>(vo) = make_float4(rv[0], rv[1], rv[2], rv[3]);
            } else {
                for (int r = 0; r < ni; ++r) { mo[r] = rm[r]; vo[r] = rv[r]; }
            }
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

// y_s[e] = m[e] + sqrt(v[e] + 1e-16) eps_s[e]: one thread per quad of the flat index e = b N + n, all S samples (K10's epilogue
// as a launch of its own: the same fma, the same eps quad).  VEC: n % 4 == 0, 16-byte loads and stores.
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
            const float4 z = eps4(rng, ed, q, rng.sample0 + (uint32_t)s);
            const float yy[4] = {__builtin_fmaf(sd[0], z.x, mm[0]), __builtin_fmaf(sd[1], z.y, mm[1]),
                                 __builtin_fmaf(sd[2], z.z, mm[2]), __builtin_fmaf(sd[3], z.w, mm[3])};
            float *yo = y + (int64_t)s * n + e0;
            if (VEC) *reinterpret_cast<float4 *>(yo) = make_float4(yy[0], yy[1], yy[2], yy[3]);
            else for (int r = 0; r < ne; ++r) yo[r] = yy[r];
        }
    }
}

static inline bool mom_misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

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
    if (B < 0 || N < 1 || K < 1 || lda < K) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (B > 0x7FFFFFFF || N > 0x7FFFFFFF || K > 0x7FFFFFFF || (B + kLrtTile - 1) / kLrtTile > 65535) {
        set_error("%s: extent outside the supported range (rows <= 64 * 65535, N, K < 2^31)", who);
        return BNN_E_RANGE;
    }
    if (compute != BNN_COMPUTE_F32 && compute != BNN_COMPUTE_BF16) { set_error("%s: unknown compute mode", who); return BNN_E_DTYPE; }
    if (flags & ~(BNN_FLAG_RELU | BNN_FLAG_X_BF16)) { set_error("%s: unknown flag", who); return BNN_E_UNSUPPORTED; }
    if ((flags & BNN_FLAG_X_BF16) && (compute != BNN_COMPUTE_BF16 || a_v)) {
        set_error("%s: a bf16 a_m needs the bf16 compute mode and a deterministic input (hidden moments are fp32)", who);
        return BNN_E_UNSUPPORTED;
    }
    if (mom_misaligned(a_m, (flags & BNN_FLAG_X_BF16) ? 1 : 3) || mom_misaligned(a_v, 3) || mom_misaligned(mu_w, 3) ||
        mom_misaligned(s2_w, 3) || mom_misaligned(mu_b, 3) || mom_misaligned(s2_b, 3) || mom_misaligned(out_m, 15) ||
        mom_misaligned(out_v, 15)) {
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
    if (mom_misaligned(m, 3) || mom_misaligned(v, 3) || mom_misaligned(out_m, 3) || mom_misaligned(out_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (n == 0) return BNN_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_moments_relu, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m, v, out_m, out_v, n);
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
    if (mom_misaligned(m, 15) || mom_misaligned(v, 15) || mom_misaligned(y, 15)) {
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
