// bnn_lrt_tile.hpp -- the 64 x 64 register-staged contraction tile of K10 (bnn_lrt.hip), K16 (bnn_moments.hip) and K18
// (bnn_moments_bwd.hip: three accumulator sets, lrt_mfma_block3).
// One tile computes contractions that share an operand pass: acc1 += P0 Q0^T and acc2 += P1 Q1^T [+ P2 Q2^T], where a plane of an
// operand is a tensor or is derived from the operand's other planes in fp32 as the loader writes LDS (lrt_stage).  P sits in the
// MFMA's A position, so a lane's four accumulator registers are four CONSECUTIVE elements of the output's contiguous dimension i
// (lrt_quad): a 16-byte store, one aligned eps quad (scalar stores and single eps when that extent is not a multiple of 4).
// 4 waves of 32 x 32 (2 x 2 MFMA tiles x 2 accumulator sets = 32 accumulator registers), operands through registers (lrt_fetch;
// the conversion and the derived planes happen there), one LDS stage of NPL planes per operand with the next K-block's global
// loads issued before the MFMAs of the current one:
//     fetch(0);  for each K-block { lrt_stage P, Q (or lrt_stage2);  barrier;  fetch(next);  lrt_mfma_block;  barrier }
// bf16 compute: planes rounded to bf16 (RNE) as they are written to LDS, v_mfma_f32_16x16x32_bf16.  fp32: v_mfma_f32_16x16x4_f32,
// an ordered fp32 fma chain over the contraction index.  No atomics, no split of the contraction: identical calls give identical
// bits, and a value does not depend on the grid.  Grid: x over i, y over j.
#pragma once
#include "bnn_device.hpp"

namespace bnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr int kLrtTile = 64;
constexpr int kLrtThreads = 256;

// rows index j, N the contiguous output extent i, K the contraction length
static inline int lrt_check_extents(const char *who, int64_t M, int64_t N, int64_t K)
{
    if (M < 0 || N < 1 || K < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (M > 0x7FFFFFFF || N > 0x7FFFFFFF || K > 0x7FFFFFFF || (M + kLrtTile - 1) / kLrtTile > 65535) {
        set_error("%s: extent outside the supported range (rows <= 64 * 65535, N, K < 2^31)", who);
        return BNN_E_RANGE;
    }
    return BNN_OK;
}

__device__ __forceinline__ float lrt_ld(const void *p, int64_t i, bool bf)
{
    return bf ? __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(p)[i] << 16) : reinterpret_cast<const float *>(p)[i];
}

// One thread's share of a 64 x BK operand tile.  TR = false: the contraction index is contiguous in memory (element (r, c) at
// p[r ld + c]; a wave reads runs of BK consecutive c).  TR = true: the row index is (element (r, c) at p[c ld + r]; a wave reads
// 64 consecutive r).  Out-of-range elements are zero.
template <bool TR, int BK>
__device__ __forceinline__ void lrt_fetch(float (&v)[BK / 4], const void *p, bool bf, int64_t ld, int row0, int rows, int c0, int cdim)
{
#pragma unroll
    for (int it = 0; it < BK / 4; ++it) {
        const int idx = it * kLrtThreads + (int)threadIdx.x;
        const int r = TR ? idx % kLrtTile : idx / BK;
        const int c = TR ? idx / kLrtTile : idx % BK;
        const bool ok = row0 + r < rows && c0 + c < cdim;
        const int64_t off = TR ? (int64_t)(c0 + c) * ld + (row0 + r) : (int64_t)(row0 + r) * ld + (c0 + c);
        v[it] = ok ? lrt_ld(p, off, bf) : 0.f;
    }
}

template <typename T> __device__ __forceinline__ T lrt_cvt(float v);
template <> __device__ __forceinline__ float lrt_cvt<float>(float v) { return v; }
template <> __device__ __forceinline__ uint16_t lrt_cvt<uint16_t>(float v) { return f2bf(v); }

// Plane pl of an operand from what lrt_fetch left in registers (a, b), formed in fp32 before any bf16 rounding.  Plane 0 is a;
//     SQ (one tensor and its square)   a^2,  [b]               otherwise (two tensors)   b,  [fma(a, a, b)]
template <typename T, bool SQ, int PL> __device__ __forceinline__ T lrt_plane(float a, float b)
{
    return lrt_cvt<T>(PL == 0 ? a : PL == 1 ? (SQ ? a * a : b) : (SQ ? b : __builtin_fmaf(a, a, b)));
}

// registers -> LDS: one thread's share of the NPL planes of one operand (plane pl at l + pl 64 LDK)
template <typename T, bool TR, bool SQ, int NPL, int BK, int LDK>
__device__ __forceinline__ void lrt_stage(T *l, const float (&r1)[BK / 4], const float (&r2)[BK / 4])
{
    constexpr int PL = kLrtTile * LDK;
#pragma unroll
    for (int it = 0; it < BK / 4; ++it) {
        const int idx = it * kLrtThreads + (int)threadIdx.x;
        T *d = l + (TR ? (idx % kLrtTile) * LDK + idx / kLrtTile : (idx / BK) * LDK + idx % BK);
        d[0] = lrt_plane<T, SQ, 0>(r1[it], r2[it]);
        d[PL] = lrt_plane<T, SQ, 1>(r1[it], r2[it]);
        if constexpr (NPL == 3) d[2 * PL] = lrt_plane<T, SQ, 2>(r1[it], r2[it]);
    }
}

// The same for both operands in one loop (K16, K10 in bf16): with three planes the fp32 writes of an element then pair up
// (ds_write2st64_b32) where two lrt_stage calls leave a third of them single, 2.5 % of the 1200 x 1200 layer.  K10's fp32
// kernels are the other way round: one loop costs the weight gradient 3.5 % against P, then Q (4096 x 1200 x 1200).
template <typename T, bool P_TR, bool P_SQ, bool Q_TR, bool Q_SQ, int NPL, int BK, int LDK>
__device__ __forceinline__ void lrt_stage2(T *lp, T *lq, const float (&p1)[BK / 4], const float (&p2)[BK / 4], const float (&q1)[BK / 4],
                                          const float (&q2)[BK / 4])
{
    constexpr int PL = kLrtTile * LDK;
#pragma unroll
    for (int it = 0; it < BK / 4; ++it) {
        const int idx = it * kLrtThreads + (int)threadIdx.x;
        const int tr = (idx % kLrtTile) * LDK + idx / kLrtTile, nt = (idx / BK) * LDK + idx % BK;
        T *dp = lp + (P_TR ? tr : nt), *dq = lq + (Q_TR ? tr : nt);
        dp[0] = lrt_plane<T, P_SQ, 0>(p1[it], p2[it]);
        dp[PL] = lrt_plane<T, P_SQ, 1>(p1[it], p2[it]);
        dq[0] = lrt_plane<T, Q_SQ, 0>(q1[it], q2[it]);
        dq[PL] = lrt_plane<T, Q_SQ, 1>(q1[it], q2[it]);
        if constexpr (NPL == 3) {
            dp[2 * PL] = lrt_plane<T, P_SQ, 2>(p1[it], p2[it]);
            dq[2 * PL] = lrt_plane<T, Q_SQ, 2>(q1[it], q2[it]);
        }
    }
}

__device__ __forceinline__ void lrt_zero(f32x4 (&acc1)[2][2], f32x4 (&acc2)[2][2])
{
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { acc1[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; acc2[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; }
}

// one lane's MFMA fragment at p: fp32 one element of the 4-deep step, bf16 eight consecutive of the 32-deep one
__device__ __forceinline__ float lrt_frag(const float *p) { return *p; }
__device__ __forceinline__ s16x8 lrt_frag(const uint16_t *p) { return *reinterpret_cast<const s16x8 *>(p); }
__device__ __forceinline__ f32x4 lrt_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 lrt_mfma(s16x8 a, s16x8 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// The MFMAs of one staged K-block: plane 0 pairs into acc1, planes 1 and 2 into acc2; per kk the plane-0 and plane-1 MFMAs of
// every (a, b), then the plane-2 ones.
template <typename T, int NPL, int BK, int LDK>
__device__ __forceinline__ void lrt_mfma_block(f32x4 (&acc1)[2][2], f32x4 (&acc2)[2][2], const T *lp, const T *lq)
{
    constexpr int PL = kLrtTile * LDK;
    constexpr int KS = sizeof(T) == 2 ? 32 : 4;             // contraction elements per MFMA; a lane holds KS / 4 consecutive ones
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pr = ((wave >> 1) * 32 + (lane & 15)) * LDK, qr = ((wave & 1) * 32 + (lane & 15)) * LDK;
#pragma unroll
    for (int kk = 0; kk < BK / KS; ++kk) {
        const int ko = kk * KS + (KS / 4) * (lane >> 4);
        decltype(lrt_frag(lp)) fp[NPL][2], fq[NPL][2];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                fp[pl][a] = lrt_frag(lp + pl * PL + pr + a * 16 * LDK + ko);
                fq[pl][a] = lrt_frag(lq + pl * PL + qr + a * 16 * LDK + ko);
            }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                acc1[a][b] = lrt_mfma(fp[0][a], fq[0][b], acc1[a][b]);
                acc2[a][b] = lrt_mfma(fp[1][a], fq[1][b], acc2[a][b]);
            }
        if constexpr (NPL == 3) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc2[a][b] = lrt_mfma(fp[2][a], fq[2][b], acc2[a][b]);
        }
    }
}

// Three accumulator sets (K18, bnn_moments_bwd.hip): three P planes against two Q planes, Q's second plane serving twice --
//     acc1 += P0 Q0^T,   acc2 += P1 Q1^T,   acc3 += P2 Q1^T
// per kk the plane-0 and plane-1 MFMAs of every (a, b), then the plane-2 ones, as lrt_mfma_block orders them.  48 accumulator
// registers per lane; LDS holds 3 + 2 planes.
template <typename T, int BK, int LDK>
__device__ __forceinline__ void lrt_mfma_block3(f32x4 (&acc1)[2][2], f32x4 (&acc2)[2][2], f32x4 (&acc3)[2][2], const T *lp, const T *lq)
{
    constexpr int PL = kLrtTile * LDK;
    constexpr int KS = sizeof(T) == 2 ? 32 : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pr = ((wave >> 1) * 32 + (lane & 15)) * LDK, qr = ((wave & 1) * 32 + (lane & 15)) * LDK;
#pragma unroll
    for (int kk = 0; kk < BK / KS; ++kk) {
        const int ko = kk * KS + (KS / 4) * (lane >> 4);
        decltype(lrt_frag(lp)) fp[3][2], fq[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) fp[pl][a] = lrt_frag(lp + pl * PL + pr + a * 16 * LDK + ko);
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) fq[pl][a] = lrt_frag(lq + pl * PL + qr + a * 16 * LDK + ko);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                acc1[a][b] = lrt_mfma(fp[0][a], fq[0][b], acc1[a][b]);
                acc2[a][b] = lrt_mfma(fp[1][a], fq[1][b], acc2[a][b]);
            }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc3[a][b] = lrt_mfma(fp[2][a], fq[1][b], acc3[a][b]);
    }
}

// bnn_lrt.hip: the bias gradients of K10 and K18, k_lrt_bias_grad on (M, N) g_m / g_v (no checks)
int lrt_bias_grad_launch(const char *who, const float *g_m, const float *g_v, int64_t M, int64_t N, const float *rho_b, float *g_mu_b,
                         float *g_rho_b, hipStream_t st);

// bnn_lrt.hip: the weight gradient of K10 (CHAIN = ChainRho, par_w = rho_w) and K23 (ChainLogSigma2, par_w = log_sigma2) -- every
// check of the two entries, k_lrt<T, LRT_WGRAD, CHAIN>, the bias sums.  Instantiated there for these two.
template <typename CHAIN>
int lrt_backward_weight(const char *who, const void *x, int64_t ldx, const float *g_m, const float *g_v, const float *par_w,
                        float *g_mean_w, float *g_par_w, const float *rho_b, float *g_mu_b, float *g_rho_b, int64_t M, int64_t N,
                        int64_t K, int compute, int flags, hipStream_t st);

// Epilogue: MFMA tile (a, b) of a lane holds out[j][i .. i + 3], i = i0 + 32 wi + 16 a + 4 (lane >> 4), j = j0 + 32 wj + 16 b +
// (lane & 15); ni of the four lie inside I.  false: none does.
struct LrtQuad { int i, j, ni; };

__device__ __forceinline__ bool lrt_quad(LrtQuad &q, int a, int b, int I, int J)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    q.i = blockIdx.x * kLrtTile + (wave >> 1) * 32 + a * 16 + 4 * (lane >> 4);
    q.j = blockIdx.y * kLrtTile + (wave & 1) * 32 + b * 16 + (lane & 15);
    if (q.i >= I || q.j >= J) return false;
    q.ni = I - q.i < 4 ? I - q.i : 4;
    return true;
}

// four consecutive outputs of one row: one 16-byte (bf16: 8-byte) store when the contiguous extent is a multiple of 4 (vec),
// else the ni that exist
__device__ __forceinline__ void lrt_store4(float *o, const float (&r)[4], bool vec, int ni)
{
    if (vec) *reinterpret_cast<float4 *>(o) = make_float4(r[0], r[1], r[2], r[3]);
    else for (int k = 0; k < ni; ++k) o[k] = r[k];
}

__device__ __forceinline__ void lrt_store4(uint16_t *o, const float (&r)[4], bool vec, int ni)
{
    if (vec) *reinterpret_cast<uint2 *>(o) = make_uint2(pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]));
    else for (int k = 0; k < ni; ++k) o[k] = f2bf(r[k]);
}

// two fp32 outputs at the same place (a mean and a variance, g_mu and g_rho)
__device__ __forceinline__ void lrt_store4x2(float *o1, const float (&r1)[4], float *o2, const float (&r2)[4], bool vec, int ni)
{
    if (vec) {
        *reinterpret_cast<float4 *>(o1) = make_float4(r1[0], r1[1], r1[2], r1[3]);
        *reinterpret_cast<float4 *>(o2) = make_float4(r2[0], r2[1], r2[2], r2[3]);
    } else {
        for (int k = 0; k < ni; ++k) { o1[k] = r1[k]; o2[k] = r2[k]; }
    }
}

__device__ __forceinline__ void lrt_store4(void *out, bool bf, int64_t off, const float (&r)[4], bool vec, int ni)
{
    if (bf) lrt_store4(reinterpret_cast<uint16_t *>(out) + off, r, vec, ni);
    else lrt_store4(reinterpret_cast<float *>(out) + off, r, vec, ni);
}

// y = m + sd eps (sd = sqrt(v + 1e-16)) for elements e .. e + 3 of one sample's noise index: one eps quad when e is a multiple of
// 4 (quad), else the first ni values one by one
__device__ __forceinline__ void lrt_noise4(float (&y)[4], const float (&m)[4], const float (&sd)[4], const RngDev &rng, uint32_t ed,
                                           uint32_t e, uint32_t sample, bool quad, int ni)
{
    if (quad) {
        const float4 z = eps4(rng, ed, e >> 2, sample);
        y[0] = __builtin_fmaf(sd[0], z.x, m[0]); y[1] = __builtin_fmaf(sd[1], z.y, m[1]);
        y[2] = __builtin_fmaf(sd[2], z.z, m[2]); y[3] = __builtin_fmaf(sd[3], z.w, m[3]);
    } else {
        for (int r = 0; r < ni; ++r) y[r] = __builtin_fmaf(sd[r], eps1(rng, ed, (uint64_t)e + r, sample), m[r]);
    }
}

}  // namespace bnn
