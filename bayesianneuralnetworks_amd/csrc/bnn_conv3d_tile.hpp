// bnn_conv3d_tile.hpp -- the 128 x 64 x 32 implicit-GEMM tile of the conv3d kernels in bnn_conv3d.hip: K7 / K9 (k_conv3d), K11
// (k_lrt_conv3d), K17 (k_moments_conv3d) and K19 (k_moments_conv3d_bwd).  C[m][n] = sum_r A(m, r) B(n, r), 4 waves of 64 x 32:
//   FWD   m = (b, od, oh, ow), n = o, r = (c, kd, kh, kw): A gathered from an input (im2col in the loader's address arithmetic,
//         padding reads zero), B = weight rows.
//   DGRAD m = (b, id, ih, iw), n = c, r = (o, kd, kh, kw): A gathered from an output gradient (taps no stride step reaches read
//         zero), B = the same weights read transposed.
//   WGRAD m = (c, kd, kh, kw), n = o, r = (b, od, oh, ow): A = the forward's gather, B = output-gradient rows.  The reduction is
//         split into slabs of whole k-tiles (c3_extents).
// What is here exists once: the block and row decode, the two gather walkers and the two B walkers (they compute validity and
// offsets and hand each element to the kernel's functor, which decides what to load), the MFMA fragments, the two-barrier
// prefetch loop, and the epilogue's lane-to-(m, n) map.  A kernel keeps which tensors its LDS planes are, how a derived plane is
// formed, and its epilogue arithmetic.  An operand has one or more planes in LDS (plane h of A at As + h C3_BM LDK, of B at
// Bs + h C3_BN LDK).  bf16 compute: operands rounded to bf16 as they are written to LDS (st_lds), v_mfma_f32_16x16x32_bf16.
// fp32: v_mfma_f32_16x16x4_f32, the reduction a k-ordered fp32 fma chain per tile.  Indices inside one sample are 32-bit.
#pragma once
#include "bnn_device.hpp"

namespace bnn {

constexpr int C3_BM = 128, C3_BN = 64, C3_BK = 32, C3_THREADS = 256;
enum { C3_FWD = 0, C3_DGRAD = 1, C3_WGRAD = 2 };

// n / d for n < 2^31 by multiply-high and shift (d >= 1)
struct FastDiv { uint32_t d, mul, shift; };

static FastDiv make_div(uint32_t d)
{
    FastDiv f;
    f.d = d;
    uint32_t s = 0;
    while (s < 32 && (1ull << s) < d) ++s;
    f.shift = s;
    f.mul = (uint32_t)(((1ull << 32) * ((1ull << s) - d)) / d + 1);
    return f;
}

__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv &f) { return (__umulhi(n, f.mul) + n) >> f.shift; }

struct Conv3dGeo {
    int32_t B, C, D, H, W, O, KD, KH, KW, OD, OH, OW;
    int32_t sd, sh, sw, pd, ph, pw, dd, dh, dw, groups, Cg, Ng;
    int32_t T, K, P, Pin;                    // taps, Cg * taps, OD OH OW, D H W
    FastDiv fOW, fOH, fP, fW, fH, fPin, fKW, fKH, fT, fsd, fsh, fsw;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// KS: reduction elements per MFMA (a lane holds KS / 4 consecutive ones: its fragment)
template <typename T> struct Op;
template <> struct Op<float> {
    static constexpr int LDK = C3_BK + 4, KS = 4;
    typedef float frag;
    __device__ static float ld(const void *p, int64_t i) { return static_cast<const float *>(p)[i]; }
};
template <> struct Op<uint16_t> {
    static constexpr int LDK = C3_BK + 8, KS = 32;    // 80-B rows: the 16-B fragment reads stay aligned
    typedef s16x8 frag;
    __device__ static float ld(const void *p, int64_t i)
    {
        return __uint_as_float((uint32_t)static_cast<const uint16_t *>(p)[i] << 16);
    }
};

__device__ __forceinline__ void st_lds(float *p, float v) { *p = v; }
__device__ __forceinline__ void st_lds(uint16_t *p, float v) { *p = f2bf(v); }

// ---- where a thread stands in the tile
// A loader: row ar of the tile, reduction offsets ah * 16 .. + 15 of each k-tile.  B loader: reduction offset bk, rows bn + 8 i.
// MFMAs and epilogue: wave (wm, wn) owns rows wm * 64 .. + 63, columns wn * 32 .. + 31.
struct C3Tile { int lane, wm, wn, ar, ah, bk, bn; int32_t m0, n0; };

__device__ __forceinline__ C3Tile c3_tile()
{
    C3Tile t;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    t.lane = tid & 63; t.wm = wave & 1; t.wn = wave >> 1;
    t.ar = tid & (C3_BM - 1); t.ah = __builtin_amdgcn_readfirstlane(tid >> 7);
    t.bk = tid & (C3_BK - 1); t.bn = tid >> 5;
    t.m0 = blockIdx.x * C3_BM; t.n0 = blockIdx.y * C3_BN;
    return t;
}

// the block's (sample, group, slab) out of blockIdx.z = (sample * groups + group) [* nslab + slab: WGRAD]
struct C3Block { int s, grp, slab; };

template <int MODE> __device__ __forceinline__ C3Block c3_block(const Conv3dGeo &g, int nslab)
{
    C3Block k;
    int z = blockIdx.z;
    k.slab = 0;
    if (MODE == C3_WGRAD) { k.slab = z % nslab; z /= nslab; }
    k.grp = z % g.groups;
    k.s = z / g.groups;
    return k;
}

// the contraction's extents and the block's share [rbeg, rend) of the reduction (WGRAD: slab `slab` of `chunk` positions)
struct C3Extents { int32_t M, N, rbeg, rend; };

template <int MODE> __device__ __forceinline__ C3Extents c3_extents(const Conv3dGeo &g, int slab, int32_t chunk)
{
    C3Extents e;
    e.M = MODE == C3_FWD ? g.B * g.P : MODE == C3_DGRAD ? g.B * g.Pin : g.K;
    e.N = MODE == C3_DGRAD ? g.Cg : g.Ng;
    e.rbeg = 0;
    e.rend = MODE == C3_FWD ? g.K : MODE == C3_DGRAD ? g.Ng * g.T : g.B * g.P;
    if (MODE == C3_WGRAD) {
        e.rbeg = slab * chunk;
        e.rend = min(e.rend, e.rbeg + chunk);
    }
    return e;
}

// ---- A: row am of the contraction.  FWD / DGRAD: the gather origin (z0, z1, z2) and element base of its (image, group), idx =
// the image; WGRAD: the row's tap (scaled by the dilation, less the padding) and the base of its channel, idx = the channel
// within the group.  A row past M is not ok and gathers nothing.
struct C3Row { bool ok; int32_t abase, z0, z1, z2, idx; };

template <int MODE> __device__ __forceinline__ C3Row c3_row_origin(const Conv3dGeo &g, int32_t am, int32_t M, int grp)
{
    C3Row w{am < M, 0, 0, 0, 0, 0};
    if (MODE == C3_FWD && w.ok) {
        const uint32_t b = fdiv(am, g.fP), p = am - b * g.P;
        const uint32_t q = fdiv(p, g.fOW), ow = p - q * g.OW, od = fdiv(q, g.fOH), oh = q - od * g.OH;
        w.z0 = od * g.sd - g.pd; w.z1 = oh * g.sh - g.ph; w.z2 = ow * g.sw - g.pw;
        w.abase = (b * g.C + grp * g.Cg) * g.Pin;
        w.idx = (int32_t)b;
    } else if (MODE == C3_DGRAD && w.ok) {
        const uint32_t b = fdiv(am, g.fPin), p = am - b * g.Pin;
        const uint32_t q = fdiv(p, g.fW), iw = p - q * g.W, id = fdiv(q, g.fH), ih = q - id * g.H;
        w.z0 = id + g.pd; w.z1 = ih + g.ph; w.z2 = iw + g.pw;
        w.abase = (b * g.O + grp * g.Ng) * g.P;
        w.idx = (int32_t)b;
    } else if (MODE == C3_WGRAD && w.ok) {
        const uint32_t c = fdiv(am, g.fT), t = am - c * g.T;
        const uint32_t q = fdiv(t, g.fKW), kw = t - q * g.KW, kd = fdiv(q, g.fKH), kh = q - kd * g.KH;
        w.z0 = kd * g.dd - g.pd; w.z1 = kh * g.dh - g.ph; w.z2 = kw * g.dw - g.pw;
        w.abase = (grp * g.Cg + c) * g.Pin;
        w.idx = (int32_t)c;
    }
    return w;
}

// FWD / DGRAD gather: reduction indices r .. r + 15 = (channel, kd, kh, kw), stepped with carries.  f(j, ok, off, c): element
// off (32-bit) of one sample's gathered tensor when ok, a zero otherwise; c the channel (FWD: input, DGRAD: output) in the group.
template <int MODE, typename F>
__device__ __forceinline__ void c3_gather_taps(const Conv3dGeo &g, const C3Row &w, int32_t r, int32_t rend, F &&f)
{
    static_assert(MODE == C3_FWD || MODE == C3_DGRAD, "WGRAD walks positions: c3_gather_positions");
    uint32_t c = 0, kd = 0, kh = 0, kw = 0;
    if (r < rend) {
        c = fdiv(r, g.fT);
        const uint32_t t = r - c * g.T, q = fdiv(t, g.fKW);
        kw = t - q * g.KW; kd = fdiv(q, g.fKH); kh = q - kd * g.KH;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        bool ok = w.ok && r + j < rend;
        int32_t off = 0;
        if (MODE == C3_FWD) {
            const int32_t id = w.z0 + (int32_t)kd * g.dd, ih = w.z1 + (int32_t)kh * g.dh, iw = w.z2 + (int32_t)kw * g.dw;
            ok = ok && (uint32_t)id < (uint32_t)g.D && (uint32_t)ih < (uint32_t)g.H && (uint32_t)iw < (uint32_t)g.W;
            off = (int32_t)c * g.Pin + (id * g.H + ih) * g.W + iw;
        } else {
            const int32_t nd = w.z0 - (int32_t)kd * g.dd, nh = w.z1 - (int32_t)kh * g.dh, nw = w.z2 - (int32_t)kw * g.dw;
            ok = ok && nd >= 0 && nh >= 0 && nw >= 0;
            const uint32_t od = fdiv(ok ? nd : 0, g.fsd), oh = fdiv(ok ? nh : 0, g.fsh), ow = fdiv(ok ? nw : 0, g.fsw);
            ok = ok && (int32_t)(od * g.sd) == nd && (int32_t)(oh * g.sh) == nh && (int32_t)(ow * g.sw) == nw &&
                 od < (uint32_t)g.OD && oh < (uint32_t)g.OH && ow < (uint32_t)g.OW;
            off = (int32_t)c * g.P + (int32_t)((od * g.OH + oh) * g.OW + ow);
        }
        f(j, ok, w.abase + off, c);
        if (++kw == (uint32_t)g.KW) { kw = 0; if (++kh == (uint32_t)g.KH) { kh = 0; if (++kd == (uint32_t)g.KD) { kd = 0; ++c; } } }
    }
}

// WGRAD gather: reduction indices r .. r + 15 = output positions (b, od, oh, ow), stepped with carries.  f(j, ok, off, b):
// element off (64-bit) of one image set's input when ok, a zero otherwise; b the image.
template <typename F>
__device__ __forceinline__ void c3_gather_positions(const Conv3dGeo &g, const C3Row &w, int32_t r, int32_t rend, F &&f)
{
    uint32_t b = 0, od = 0, oh = 0, ow = 0;
    if (r < rend) {
        b = fdiv(r, g.fP);
        const uint32_t p = r - b * g.P, q = fdiv(p, g.fOW);
        ow = p - q * g.OW; od = fdiv(q, g.fOH); oh = q - od * g.OH;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int32_t id = (int32_t)(od * g.sd) + w.z0, ih = (int32_t)(oh * g.sh) + w.z1, iw = (int32_t)(ow * g.sw) + w.z2;
        const bool ok = w.ok && r + j < rend && (uint32_t)id < (uint32_t)g.D && (uint32_t)ih < (uint32_t)g.H &&
                        (uint32_t)iw < (uint32_t)g.W;
        f(j, ok, (int64_t)b * g.C * g.Pin + w.abase + (id * g.H + ih) * g.W + iw, b);
        if (++ow == (uint32_t)g.OW) { ow = 0; if (++oh == (uint32_t)g.OH) { oh = 0; if (++od == (uint32_t)g.OD) { od = 0; ++b; } } }
    }
}

// ---- B: reduction index r = r0 + bk, rows n = n0 + bn + 8 i.
// FWD / DGRAD: weight rows of an O x K tensor, FWD w[o][r], DGRAD r = (o, tap): w[o][c][tap] read transposed.  f(i, ok, off).
template <int MODE, typename F>
__device__ __forceinline__ void c3_weight_rows(const Conv3dGeo &g, const C3Tile &t, int32_t N, int grp, int32_t r, int32_t rend, F &&f)
{
    static_assert(MODE == C3_FWD || MODE == C3_DGRAD, "WGRAD's B is the output gradient: c3_grad_rows");
    const bool rok = r < rend;
    const int64_t wb = (int64_t)grp * g.Ng * g.K;
    int32_t roff = r;
    int32_t nstride = g.K;
    if (MODE == C3_DGRAD) {
        const uint32_t o = fdiv(rok ? r : 0, g.fT);
        roff = (int32_t)(o * g.K + (r - o * g.T));
        nstride = g.T;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int32_t n = t.n0 + t.bn + 8 * i;
        f(i, rok && n < N, wb + (int64_t)n * nstride + roff);
    }
}

// WGRAD: rows of one image set's (B, O, P) output gradient at position r = (b, p).  f(i, ok, off, b, n).
template <typename F>
__device__ __forceinline__ void c3_grad_rows(const Conv3dGeo &g, const C3Tile &t, int32_t N, int grp, int32_t r, int32_t rend, F &&f)
{
    const bool rok = r < rend;
    uint32_t b = 0, p = 0;
    if (rok) { b = fdiv(r, g.fP); p = r - b * g.P; }
    const int64_t o0 = ((int64_t)b * g.O + (int64_t)grp * g.Ng) * g.P + p;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int32_t n = t.n0 + t.bn + 8 * i;
        f(i, rok && n < N, o0 + (int64_t)n * g.P, b, n);
    }
}

// a thread's LDS slots: its 16 A elements are consecutive at c3_lds_a, its B element i is at c3_lds_b + 8 i LDK (plane 0)
template <typename T> __device__ __forceinline__ T *c3_lds_a(T *As, const C3Tile &t) { return As + t.ar * Op<T>::LDK + t.ah * 16; }
template <typename T> __device__ __forceinline__ T *c3_lds_b(T *Bs, const C3Tile &t) { return Bs + t.bn * Op<T>::LDK + t.bk; }

// ---- MFMAs.  A lane's fragments of MFMA step kk of a staged k-tile (C3_BK / KS steps): rows wm * 64 + 16 i + (lane & 15) of an
// A plane, wn * 32 + 16 j + (lane & 15) of a B plane; its four accumulator registers of block (i, j) are
// C[wm * 64 + 16 i + (lane >> 4) * 4 + q][wn * 32 + 16 j + (lane & 15)].
template <int NS> __device__ __forceinline__ void c3_zero(f32x4 (&acc)[NS][4][2])
{
#pragma unroll
    for (int h = 0; h < NS; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[h][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ float c3_ld_frag(const float *p) { return *p; }
__device__ __forceinline__ s16x8 c3_ld_frag(const uint16_t *p) { return *reinterpret_cast<const s16x8 *>(p); }

template <typename T> __device__ __forceinline__ void c3_frag_a(typename Op<T>::frag (&fa)[4], const T *A, const C3Tile &t, int kk)
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
        fa[i] = c3_ld_frag(A + (t.wm * 64 + i * 16 + (t.lane & 15)) * Op<T>::LDK + kk * Op<T>::KS + (t.lane >> 4) * (Op<T>::KS / 4));
}

template <typename T> __device__ __forceinline__ void c3_frag_b(typename Op<T>::frag (&fb)[2], const T *Bt, const C3Tile &t, int kk)
{
#pragma unroll
    for (int j = 0; j < 2; ++j)
        fb[j] = c3_ld_frag(Bt + (t.wn * 32 + j * 16 + (t.lane & 15)) * Op<T>::LDK + kk * Op<T>::KS + (t.lane >> 4) * (Op<T>::KS / 4));
}

__device__ __forceinline__ f32x4 c3_mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 c3_mma(s16x8 a, s16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

template <typename T>
__device__ __forceinline__ void c3_mfma(f32x4 (&acc)[4][2], const typename Op<T>::frag (&fa)[4], const typename Op<T>::frag (&fb)[2])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = c3_mma(fa[i], fb[j], acc[i][j]);
}

// one staged k-tile of NPL plane pairs: plane h of A against plane h of B into acc[min(h, NS - 1)], MFMA step outer, plane inner
template <typename T, int NPL, int NS>
__device__ __forceinline__ void c3_mfma_planes(f32x4 (&acc)[NS][4][2], const T *As, const T *Bs, const C3Tile &t)
{
#pragma unroll
    for (int kk = 0; kk < C3_BK / Op<T>::KS; ++kk) {
#pragma unroll
        for (int h = 0; h < NPL; ++h) {
            typename Op<T>::frag fa[4], fb[2];
            c3_frag_a<T>(fa, As + h * C3_BM * Op<T>::LDK, t, kk);
            c3_frag_b<T>(fb, Bs + h * C3_BN * Op<T>::LDK, t, kk);
            c3_mfma<T>(acc[h < NS ? h : NS - 1], fa, fb);
        }
    }
}

// ---- the prefetch loop over nsum passes ("samples") of the k-tiles of [rbeg, rend): fetch(sm, r0) loads k-tile r0 of pass sm
// into the kernel's registers, store() writes them to LDS, compute() issues the tile's MFMAs, end(sm) runs after the last
// k-tile of pass sm.
struct C3NoEnd { __device__ __forceinline__ void operator()(int) const {} };

template <typename Fetch, typename Store, typename Compute, typename End = C3NoEnd>
__device__ __forceinline__ void c3_pipeline(int nsum, int32_t rbeg, int32_t rend, Fetch &&fetch, Store &&store, Compute &&compute,
                                            End &&end = End())
{
    const int ntile = rend > rbeg ? (rend - rbeg + C3_BK - 1) / C3_BK : 0;
    const int nstep = nsum * ntile;
    if (nstep > 0) fetch(0, rbeg);
    int sm = 0, tl = 0;                                 // the (pass, k-tile) of this step
    for (int step = 0; step < nstep; ++step) {
        __syncthreads();                                // the previous tile's fragment reads are done
        store();
        __syncthreads();
        const bool last = tl + 1 == ntile;
        const int nsm = last ? sm + 1 : sm, ntl = last ? 0 : tl + 1;
        if (step + 1 < nstep) fetch(nsm, rbeg + ntl * C3_BK);      // the next tile's loads fly under this tile's MFMAs
        compute();
        if (last) end(sm);
        sm = nsm; tl = ntl;
    }
}

// ---- epilogue: the lane's columns, and per column its quads of four consecutive rows or its single rows
template <typename F> __device__ __forceinline__ void c3_each_col(const C3Tile &t, int32_t N, F &&f)          // f(j, n)
{
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int32_t n = t.n0 + t.wn * 32 + j * 16 + (t.lane & 15);
        if (n >= N) continue;
        f(j, n);
    }
}

template <typename F> __device__ __forceinline__ void c3_each_quad(const C3Tile &t, int32_t M, F &&f)         // f(i, mq): rows mq + q
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int32_t mq = t.m0 + t.wm * 64 + i * 16 + (t.lane >> 4) * 4;
        if (mq >= M) continue;
        f(i, mq);
    }
}

template <typename F> __device__ __forceinline__ void c3_each_row(const C3Tile &t, int32_t M, F &&f)          // f(i, q, m)
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int32_t m = t.m0 + t.wm * 64 + i * 16 + (t.lane >> 4) * 4 + q;
            if (m >= M) continue;
            f(i, q, m);
        }
}

// element (b CH + ch) P + p of a (B, CH, P) tensor for row m = b P + p.  A quad runs along p: with c3_vec(P) it is four
// consecutive, 16-byte aligned elements of one image and channel.
__device__ __forceinline__ uint32_t c3_elem(uint32_t m, const FastDiv &fP, int32_t P, int32_t CH, int32_t ch)
{
    const uint32_t b = fdiv(m, fP);
    return (b * (uint32_t)CH + (uint32_t)ch) * (uint32_t)P + (m - b * (uint32_t)P);
}

__device__ __forceinline__ bool c3_vec(int32_t P) { return (P & 3) == 0; }

}  // namespace bnn
