// bnn_conv3d.hip -- NormalConv3d (pytorch_bayesian/nn/conv.py:122-142) on drawn weights as implicit GEMMs, forward and backward,
// and the conv kernels that reuse its tile: Flipout (K9), local reparameterization (K11), moment propagation (K17, K19).
//
// The tile -- the three contractions FWD / DGRAD / WGRAD, their gathers, the MFMA blocks, the prefetch loop, the epilogue's
// lane map -- is bnn_conv3d_tile.hpp; a kernel here says which tensors its LDS planes are and what its epilogue computes.
// K7 (k_conv3d): A = the gather, B = the sample's drawn weight row (FWD, DGRAD) or gy (WGRAD).  FWD adds the drawn bias; DGRAD
// with a shared input sums its S samples inside the reduction loop, in sample order; WGRAD's slabs (gridDim.z) are added in
// slab order by k_conv3d_slab_sum.  Every sum is in a fixed order and there are no atomics: two identical calls give identical
// bits.  The host refuses a per-sample tensor of 2^31 elements or more.
//
// FLIP (FlipOutNormalConv3d, pytorch_bayesian/nn/conv.py:237-251, groups == 1): every tile runs TWO contractions on one pass over
// the gathers -- the mean weights, and the stddev weights with the per-example signs applied as the second copy of an operand is
// written to LDS (x 1.0 / -1.0, exact in both modes).  Signs: sg[s][b][O + C] (R = [0, O), S = [O, O + C)), sample stride sg_ss.
//   FWD   A2 = A (.) S_s[b][c]; epilogue acc + R_s[b][o] acc2.  One sample per workgroup (a shared input recomputes the mean
//         contraction per sample: the kernel is gather-bound and the second MFMA set rides on the same LDS tiles).
//   DGRAD A2 = gy (.) R_s[b][o]; at the end of each sample acc += S_s[b][c] acc2, acc2 = 0 (a shared input: in sample order).
//   WGRAD A2 = x (.) S_s[b][c], B2 = gy (.) R_s[b][o]; both partials to slabs [slab][s][mean | stddev][O][K], then
//         k_conv3d_flip_wsum adds slabs and samples in a fixed order and applies softplus'.
#include "bnn_conv3d_tile.hpp"
#include "bnn_moments_act.hpp"

#include <algorithm>

namespace bnn {

struct Conv3dArgs {
    const float *x; int64_t x_ss;            // fp32 NCDHW, sample stride (0: shared)
    const float *gy;                         // fp32 S x B x O x P
    const void *w; int64_t w_ss;             // S x O x K (bf16 or fp32), sample stride
    const float *bias; int64_t b_ss;         // FWD: S x O drawn bias or NULL
    float *out;                              // FWD: y; DGRAD: gx; WGRAD: slab base (or gw when nslab == 1)
    int32_t S, shared, nslab, chunk;         // WGRAD: slabs per (sample, group), reduction positions per slab (% C3_BK == 0)
    const float *sg; int64_t sg_ss;          // FLIP: signs B x (O + C) per sample, sample stride (0: one set for all)
    int64_t w_std;                           // FLIP: element offset of the stddev row in w
};

template <typename T, int MODE, bool FLIP = false>
__global__ __launch_bounds__(C3_THREADS) void k_conv3d(const Conv3dGeo g, const Conv3dArgs a)
{
    constexpr int LDK = Op<T>::LDK;
    constexpr int NT = FLIP ? 2 : 1;         // operand copies in LDS: plain, and (FLIP) signed / stddev
    __shared__ __attribute__((aligned(16))) T As[NT * C3_BM * LDK];
    __shared__ __attribute__((aligned(16))) T Bs[NT * C3_BN * LDK];
    const int32_t OC = g.O + g.C;            // FLIP: one example's signs

    const C3Tile t = c3_tile();
    const C3Block k = c3_block<MODE>(g, a.nslab);
    const int s = k.s, grp = k.grp;          // s: DGRAD with a shared input: 0 (the samples are summed in the loop)
    const C3Extents e = c3_extents<MODE>(g, k.slab, a.chunk);
    const int nsum = (MODE == C3_DGRAD && a.shared) ? a.S : 1;
    const C3Row row = c3_row_origin<MODE>(g, t.m0 + t.ar, e.M, grp);
    // FLIP: the row's signs -- FWD S_s[b][.], DGRAD R_s[b][.] (indexed by the reduction's channel), WGRAD S_s[.][c] (by its image)
    const int32_t arow_sg = MODE == C3_FWD ? row.idx * OC + g.O : MODE == C3_DGRAD ? row.idx * OC : g.O + row.idx;

    float va[16], sa[16], vb[8], vb2[8];          // sa, vb2: FLIP only (dead otherwise)
    auto fetch = [&](int sm, int32_t r0) {
        const float *sgs = FLIP ? a.sg + (int64_t)(s + sm) * a.sg_ss + arow_sg : nullptr;
        if constexpr (MODE == C3_WGRAD) {
            const float *x = a.x + (int64_t)s * a.x_ss;
            c3_gather_positions(g, row, r0 + t.ah * 16, e.rend, [&](int j, bool ok, int64_t off, uint32_t b) {
                va[j] = ok ? x[off] : 0.f;
                if constexpr (FLIP) sa[j] = ok ? sgs[(int32_t)b * OC] : 0.f;
            });
            const float *gy = a.gy + (int64_t)s * g.B * g.O * g.P;
            const float *rs = FLIP ? a.sg + (int64_t)s * a.sg_ss : nullptr;
            c3_grad_rows(g, t, e.N, grp, r0 + t.bk, e.rend, [&](int i, bool ok, int64_t off, uint32_t b, int32_t n) {
                vb[i] = ok ? gy[off] : 0.f;
                if constexpr (FLIP) vb2[i] = ok ? vb[i] * rs[(int64_t)b * OC + n] : 0.f;
            });
        } else {
            const float *src = MODE == C3_FWD ? a.x + (int64_t)s * a.x_ss : a.gy + (int64_t)(s + sm) * g.B * g.O * g.P;
            c3_gather_taps<MODE>(g, row, r0 + t.ah * 16, e.rend, [&](int j, bool ok, int32_t off, uint32_t c) {
                va[j] = ok ? src[off] : 0.f;
                if constexpr (FLIP) sa[j] = ok ? sgs[c] : 0.f;
            });
            const int64_t ws = (int64_t)(s + sm) * a.w_ss;
            c3_weight_rows<MODE>(g, t, e.N, grp, r0 + t.bk, e.rend, [&](int i, bool ok, int64_t off) {
                vb[i] = ok ? Op<T>::ld(a.w, ws + off) : 0.f;
                if constexpr (FLIP) vb2[i] = ok ? Op<T>::ld(a.w, a.w_std + ws + off) : 0.f;
            });
        }
    };

    auto store = [&]() {
        T *pa = c3_lds_a(As, t), *pb = c3_lds_b(Bs, t);
#pragma unroll
        for (int j = 0; j < 16; ++j) st_lds(pa + j, va[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) st_lds(pb + 8 * i * LDK, vb[i]);
        if constexpr (FLIP) {
#pragma unroll
            for (int j = 0; j < 16; ++j) st_lds(pa + C3_BM * LDK + j, va[j] * sa[j]);   // x +-1: exact, then rounded as the plain copy
#pragma unroll
            for (int i = 0; i < 8; ++i) st_lds(pb + (C3_BN + 8 * i) * LDK, vb2[i]);
        }
    };

    f32x4 acc[NT][4][2];
    c3_zero(acc);
    auto compute = [&]() { c3_mfma_planes<T, NT, NT>(acc, As, Bs, t); };

    if constexpr (FLIP && MODE == C3_DGRAD) {
        // acc += S_smp[b][c] acc2 at the end of sample smp's reduction (lane rows m, columns n = c as in the epilogue); the
        // elements outside (M, N) hold zeros in both sets
        auto fold = [&](int sm) {
            const float *sgs = a.sg + (int64_t)(s + sm) * a.sg_ss + g.O;
            c3_each_col(t, e.N, [&](int j, int32_t n) {
                c3_each_row(t, e.M, [&](int i, int q, int32_t m) {
                    const float sgn = sgs[(int32_t)fdiv(m, g.fPin) * OC + n];
                    acc[0][i][j][q] = __builtin_fmaf(sgn, acc[NT - 1][i][j][q], acc[0][i][j][q]);
                    acc[NT - 1][i][j][q] = 0.f;
                });
            });
        };
        c3_pipeline(nsum, e.rbeg, e.rend, fetch, store, compute, fold);
    } else {
        c3_pipeline(nsum, e.rbeg, e.rend, fetch, store, compute);
    }

    c3_each_col(t, e.N, [&](int j, int32_t n) {
        float bias = 0.f;
        if (MODE == C3_FWD && a.bias) bias = a.bias[(int64_t)s * a.b_ss + grp * g.Ng + n];
        c3_each_row(t, e.M, [&](int i, int q, int32_t m) {
            const float v = acc[0][i][j][q];
            if (MODE == C3_FWD && FLIP) {
                const float r = a.sg[(int64_t)s * a.sg_ss + (int32_t)fdiv(m, g.fP) * OC + n];
                a.out[(int64_t)s * g.B * g.O * g.P + c3_elem(m, g.fP, g.P, g.O, n)] = __builtin_fmaf(r, acc[NT - 1][i][j][q], v);
            } else if (MODE == C3_WGRAD && FLIP) {
                // slab [slab][s][mean | stddev][o][k]
                const int64_t el = (((int64_t)k.slab * a.S + s) * 2 * g.O + n) * g.K + m;
                a.out[el] = v;
                a.out[el + (int64_t)g.O * g.K] = acc[NT - 1][i][j][q];
            } else if (MODE == C3_FWD) {
                a.out[(int64_t)s * g.B * g.O * g.P + c3_elem(m, g.fP, g.P, g.O, grp * g.Ng + n)] = v + bias;
            } else if (MODE == C3_DGRAD) {
                a.out[(int64_t)s * g.B * g.C * g.Pin + c3_elem(m, g.fPin, g.Pin, g.C, grp * g.Cg + n)] = v;
            } else {
                // slab [slab][s][o][k] (gw itself when there is one slab)
                a.out[(((int64_t)k.slab * a.S + s) * g.O + grp * g.Ng + n) * g.K + m] = v;
            }
        });
    });
}

// gw[e] = sum of the slabs in slab order
__global__ __launch_bounds__(256) void k_conv3d_slab_sum(const float *__restrict__ slabs, int64_t slab_stride, int nslab,
                                                        float *__restrict__ gw, int64_t n)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float v = 0.f;
    for (int k = 0; k < nslab; ++k) v += slabs[(int64_t)k * slab_stride + e];
    gw[e] = v;
}

// FLIP: g_mean[e] = sum_s sum_slab mean partials, g_scale[e] = (sum_s sum_slab stddev partials) softplus'(rho[e]); samples in
// order, each sample's slabs in slab order
__global__ __launch_bounds__(256) void k_conv3d_flip_wsum(const float *__restrict__ slabs, int nslab, int S, const float *__restrict__ rho,
                                                         float *__restrict__ g_mean, float *__restrict__ g_scale, int64_t n)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float gm = 0.f, gs = 0.f;
    for (int s = 0; s < S; ++s) {
        float vm = 0.f, vs = 0.f;
        for (int k = 0; k < nslab; ++k) {
            const float *p = slabs + (((int64_t)k * S + s) * 2) * n + e;
            vm += p[0];
            vs += p[n];
        }
        gm += vm;
        gs += vs;
    }
    g_mean[e] = gm;
    g_scale[e] = gs * dsoftplus(rho[e]);
}

// gb[s][o] = sum over (b, position) of gy[s][b][o][.]: one workgroup per (s, o), fixed strided partials and a fixed tree
__global__ __launch_bounds__(256) void k_conv3d_bias_grad(const float *__restrict__ gy, float *__restrict__ gb, int32_t B, int32_t O,
                                                         int32_t P)
{
    __shared__ float red[256];
    const int o = blockIdx.x, s = blockIdx.y;
    float v = 0.f;
    for (int32_t b = 0; b < B; ++b) {
        const float *row = gy + (((int64_t)s * B + b) * O + o) * P;
        for (int32_t p = threadIdx.x; p < P; p += 256) v += row[p];
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) gb[(int64_t)s * O + o] = red[0];
}

// ---- K11: the local-reparameterization conv tile (LocalReparamConv1d / 2d / 3d, nn/conv.py) -------------------------------
// m = conv(x, mu_w) + mu_b, v = conv(x^2, sigma_w^2) + sigma_b^2, y_s = m + sqrt(v + 1e-16) eps_s with one eps per output element
// and MC sample (LRT-conv noise contract, include/bnn_hip.h).  The tile (bnn_conv3d_tile.hpp) with TWO contractions on one pass
// over the gathers, like K7's Flipout instantiation; the second copy of an operand is its square (taken in fp32, then rounded as
// the plain copy) or a second tensor:
//   FWD   A = gather(x), A2 = A^2; B = mu_w, B2 = sigma_w^2.  Epilogue: v (stored for the backward) and the S samples -- a shared
//         input is contracted ONCE and the workgroup stores S tiles; a per-sample input has the sample in the grid.
//   DGRAD A = gather(g_m), A2 = gather(g_v); B, B2 = the same weights read transposed.  Epilogue: acc + 2 x acc2.
//   WGRAD A = gather(x), A2 = A^2; B = g_m, B2 = g_v.  Every slab adds its share of the positions of every image set in set order;
//         both partials to slabs [slab][mean | variance][O][K], k_lrt_conv_wsum<CHAIN> adds the slabs and applies the posterior's chain factor.
// The weights (mu_w, sigma_w^2) are fp32 in memory in both modes; the bf16 mode rounds them, like every operand, as they are
// written to LDS.
struct LrtConvArgs {
    const float *x;                          // FWD: the input; DGRAD: the input (2 x in the epilogue); WGRAD: the input
    int64_t x_ss;                            // FWD: sample stride (0: shared); DGRAD / WGRAD: B C Pin (one image set)
    const float *g1, *g2;                    // DGRAD / WGRAD: g_m, g_v, (sets, B, O, P)
    const float *w1, *w2;                    // FWD / DGRAD: mu_w, sigma_w^2, O x K
    const float *b1, *b2;                    // FWD: mu_b, sigma_b^2 (both or neither)
    float *out, *out2;                       // FWD: y, v (may be NULL); DGRAD: gx; WGRAD: slab base
    int32_t S, shared, nslab, chunk;         // FWD: samples; DGRAD / WGRAD: image sets
    RngDev rng;
};

template <typename T, int MODE>
__global__ __launch_bounds__(C3_THREADS) void k_lrt_conv3d(const Conv3dGeo g, const LrtConvArgs a)
{
    constexpr int LDK = Op<T>::LDK;
    __shared__ __attribute__((aligned(16))) T As[2 * C3_BM * LDK];
    __shared__ __attribute__((aligned(16))) T Bs[2 * C3_BN * LDK];

    const C3Tile t = c3_tile();
    const C3Block k = c3_block<MODE>(g, a.nslab);
    const int s = k.s, grp = k.grp;          // s: the sample or image set; FWD with a shared input, WGRAD: 0
    const C3Extents e = c3_extents<MODE>(g, k.slab, a.chunk);
    const int nsum = MODE == C3_WGRAD ? a.S : 1;
    const int64_t gset = (int64_t)g.B * g.O * g.P;       // one image set of g_m / g_v / y
    const C3Row row = c3_row_origin<MODE>(g, t.m0 + t.ar, e.M, grp);

    // va: the plain copy; va2: DGRAD only, the second tensor (FWD / WGRAD square va as they store it)
    float va[16], va2[16], vb[8], vb2[8];
    auto fetch = [&](int sm, int32_t r0) {
        if constexpr (MODE == C3_WGRAD) {
            const float *x = a.x + (int64_t)sm * a.x_ss;           // image set sm
            c3_gather_positions(g, row, r0 + t.ah * 16, e.rend,
                                [&](int j, bool ok, int64_t off, uint32_t) { va[j] = ok ? x[off] : 0.f; });
            c3_grad_rows(g, t, e.N, grp, r0 + t.bk, e.rend, [&](int i, bool ok, int64_t off, uint32_t, int32_t) {
                vb[i] = ok ? a.g1[(int64_t)sm * gset + off] : 0.f;
                vb2[i] = ok ? a.g2[(int64_t)sm * gset + off] : 0.f;
            });
        } else {
            const float *src = MODE == C3_FWD ? a.x + (int64_t)s * a.x_ss : a.g1 + (int64_t)s * gset;
            const float *src2 = MODE == C3_FWD ? nullptr : a.g2 + (int64_t)s * gset;
            c3_gather_taps<MODE>(g, row, r0 + t.ah * 16, e.rend, [&](int j, bool ok, int32_t off, uint32_t) {
                va[j] = ok ? src[off] : 0.f;
                if constexpr (MODE == C3_DGRAD) va2[j] = ok ? src2[off] : 0.f;
            });
            c3_weight_rows<MODE>(g, t, e.N, grp, r0 + t.bk, e.rend, [&](int i, bool ok, int64_t off) {
                vb[i] = ok ? a.w1[off] : 0.f;
                vb2[i] = ok ? a.w2[off] : 0.f;
            });
        }
    };

    auto store = [&]() {
        T *pa = c3_lds_a(As, t), *pb = c3_lds_b(Bs, t);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            st_lds(pa + j, va[j]);
            st_lds(pa + C3_BM * LDK + j, MODE == C3_DGRAD ? va2[j] : va[j] * va[j]);   // the square in fp32, then rounded as the plain copy
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            st_lds(pb + 8 * i * LDK, vb[i]);
            st_lds(pb + (C3_BN + 8 * i) * LDK, vb2[i]);
        }
    };

    f32x4 acc[2][4][2];
    c3_zero(acc);
    c3_pipeline(nsum, e.rbeg, e.rend, fetch, store, [&]() { c3_mfma_planes<T, 2, 2>(acc, As, Bs, t); });

    if constexpr (MODE == C3_FWD) {
        // a lane's quad runs along the output position p: with P % 4 == 0 it is one aligned eps quad of one image and channel
        const bool vec = c3_vec(g.P);
        const uint32_t ed = rng_epoch_dev(a.rng);
        const int ns = a.shared ? a.S : 1;
        c3_each_col(t, e.N, [&](int j, int32_t n) {
            const int32_t o = grp * g.Ng + n;
            const float mb = a.b1 ? a.b1[o] : 0.f, sb = a.b1 ? a.b2[o] : 0.f;
            c3_each_quad(t, e.M, [&](int i, int32_t mq) {
                float r1[4], r2[4], sd[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    r1[q] = acc[0][i][j][q] + mb;
                    r2[q] = acc[1][i][j][q] + sb;
                    sd[q] = sqrtf(r2[q] + 1e-16f);
                }
                if (vec) {
                    const uint32_t e0 = c3_elem(mq, g.fP, g.P, g.O, o);          // the quad stays inside one image and channel
                    if (a.out2) *reinterpret_cast<float4 *>(a.out2 + (int64_t)s * gset + e0) = make_float4(r2[0], r2[1], r2[2], r2[3]);
                    for (int u = 0; u < ns; ++u) {
                        const int smp = a.shared ? u : s;
                        const float4 e4 = eps4(a.rng, ed, e0 >> 2, a.rng.sample0 + (uint32_t)smp);
                        *reinterpret_cast<float4 *>(a.out + (int64_t)smp * gset + e0) =
                            make_float4(__builtin_fmaf(sd[0], e4.x, r1[0]), __builtin_fmaf(sd[1], e4.y, r1[1]),
                                        __builtin_fmaf(sd[2], e4.z, r1[2]), __builtin_fmaf(sd[3], e4.w, r1[3]));
                    }
                } else {
                    uint32_t el[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) el[q] = c3_elem(min(mq + q, e.M - 1), g.fP, g.P, g.O, o);
                    const int nq = e.M - mq < 4 ? e.M - mq : 4;
                    if (a.out2)
                        for (int q = 0; q < nq; ++q) a.out2[(int64_t)s * gset + el[q]] = r2[q];
                    for (int u = 0; u < ns; ++u) {
                        const int smp = a.shared ? u : s;
                        for (int q = 0; q < nq; ++q)
                            a.out[(int64_t)smp * gset + el[q]] =
                                __builtin_fmaf(sd[q], eps1(a.rng, ed, (uint64_t)el[q], a.rng.sample0 + (uint32_t)smp), r1[q]);
                    }
                }
            });
        });
    } else {
        c3_each_col(t, e.N, [&](int j, int32_t n) {
            c3_each_row(t, e.M, [&](int i, int q, int32_t m) {
                if (MODE == C3_DGRAD) {
                    const int64_t idx = (int64_t)s * a.x_ss + c3_elem(m, g.fPin, g.Pin, g.C, grp * g.Cg + n);
                    a.out[idx] = __builtin_fmaf(2.0f * a.x[idx], acc[1][i][j][q], acc[0][i][j][q]);
                } else {
                    // slab [slab][mean | variance][o][k]
                    const int64_t el = (((int64_t)k.slab * 2) * g.O + grp * g.Ng + n) * g.K + m;
                    a.out[el] = acc[0][i][j][q];
                    a.out[el + (int64_t)g.O * g.K] = acc[1][i][j][q];
                }
            });
        });
    }
}

// K11 and K24: g_mean[e] = sum of the mean slabs in slab order, g_par[e] = CHAIN(sum of the variance slabs, par[e]) -- the
// posterior's chain factor (bnn_device.hpp): ChainRho on rho_w (LocalReparamConvNd), ChainLogSigma2 on log_sigma2
// (VariationalDropoutConvNd).  The slab sums do not depend on it: g_theta of the one has g_mu_w's bits of the other.
template <typename CHAIN>
__global__ __launch_bounds__(256) void k_lrt_conv_wsum(const float *__restrict__ slabs, int nslab, const float *__restrict__ par,
                                                      float *__restrict__ g_mean, float *__restrict__ g_par, int64_t n)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float gm = 0.f, gv = 0.f;
    for (int k = 0; k < nslab; ++k) {
        const float *p = slabs + (int64_t)k * 2 * n + e;
        gm += p[0];
        gv += p[n];
    }
    const float p = par[e];
    g_mean[e] = gm;
    g_par[e] = CHAIN::apply(gv, p);
}

// g_mu_b[o] = sum over (image, position) of g_m, g_rho_b[o] = (the same sum of g_v) 2 sigma_b sigmoid(rho_b): one workgroup per
// o, fixed strided partials (images in order) and a fixed tree.  rows = every image of every set.
__global__ __launch_bounds__(256) void k_lrt_conv_bias_grad(const float *__restrict__ g_m, const float *__restrict__ g_v, int64_t rows,
                                                           int32_t O, int32_t P, const float *__restrict__ rho_b,
                                                           float *__restrict__ g_mu_b, float *__restrict__ g_rho_b)
{
    __shared__ float rm[256], rv[256];
    const int o = blockIdx.x;
    float sm = 0.f, sv = 0.f;
    for (int64_t b = 0; b < rows; ++b) {
        const int64_t row = (b * O + o) * P;
        for (int32_t p = threadIdx.x; p < P; p += 256) { sm += g_m[row + p]; sv += g_v[row + p]; }
    }
    rm[threadIdx.x] = sm;
    rv[threadIdx.x] = sv;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { rm[threadIdx.x] += rm[threadIdx.x + w]; rv[threadIdx.x] += rv[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float r = rho_b[o];
        g_mu_b[o] = rm[0];
        g_rho_b[o] = rv[0] * (2.0f * sigma_lrt(r) * dsigma_lrt(r));
    }
}

// ---- K17: moment propagation through a convolution (sampling-free inference; NormalConv / LocalReparamConv 1d / 2d / 3d inside
// BayesianNetworkModule.predictive_moments).  Input and output hold a mean and a variance per element, independent across elements:
//     m = conv(a_m, mu_w) + mu_b
//     v = conv(a_m^2, sigma_w^2) + conv(a_v, mu_w^2 + sigma_w^2) + sigma_b^2          (second term absent for a deterministic input)
// Every addend of v is non-negative.  The tile's FWD contraction (groups in the grid) with K16's planes: A planes a_m, a_m^2,
// [a_v]; B planes mu_w, sigma_w^2, [fma(mu_w, mu_w, sigma_w^2)], the derived planes formed in fp32 as they are staged (before any
// bf16 rounding).  Both variance contractions add into ONE accumulator set: a lane holds K11's 64 accumulator registers.
// Epilogue: + mu_b / + sigma_b^2, then moments_relu_dev or moments_elu_dev (bnn_moments_act.hpp: the standalone launches'
// functions, so fused and standalone agree bit for bit); fp32 (B, O, P) stores.
// No sample axis, no rng, no atomics, no split reduction: identical calls give identical bits.
struct MomConvArgs {
    const float *a_m, *a_v;                  // (B, C, D, H, W); a_v NULL in the deterministic instantiation
    const float *w1, *w2;                    // mu_w, sigma_w^2, O x K
    const float *b1, *b2;                    // mu_b, sigma_b^2 (both or neither)
    float *out_m, *out_v;                    // (B, O, OD, OH, OW)
    int32_t act;                             // 0, BNN_FLAG_RELU or BNN_FLAG_ELU
    float elu_alpha;
};

template <typename T, bool VAR>
__global__ __launch_bounds__(C3_THREADS) void k_moments_conv3d(const Conv3dGeo g, const MomConvArgs a)
{
    constexpr int LDK = Op<T>::LDK;
    constexpr int NPL = VAR ? 3 : 2;                 // planes per operand
    __shared__ __attribute__((aligned(16))) T As[NPL * C3_BM * LDK];
    __shared__ __attribute__((aligned(16))) T Bs[NPL * C3_BN * LDK];

    const C3Tile t = c3_tile();
    const int grp = c3_block<C3_FWD>(g, 1).grp;
    const C3Extents e = c3_extents<C3_FWD>(g, 0, 0);
    const C3Row row = c3_row_origin<C3_FWD>(g, t.m0 + t.ar, e.M, grp);

    float va[16], va2[16], vb[8], vb2[8];            // va2: a_v (VAR only; dead otherwise)
    auto fetch = [&](int, int32_t r0) {
        c3_gather_taps<C3_FWD>(g, row, r0 + t.ah * 16, e.rend, [&](int j, bool ok, int32_t off, uint32_t) {
            va[j] = ok ? a.a_m[off] : 0.f;
            if constexpr (VAR) va2[j] = ok ? a.a_v[off] : 0.f;
        });
        c3_weight_rows<C3_FWD>(g, t, e.N, grp, r0 + t.bk, e.rend, [&](int i, bool ok, int64_t off) {
            vb[i] = ok ? a.w1[off] : 0.f;
            vb2[i] = ok ? a.w2[off] : 0.f;
        });
    };

    // the derived planes in fp32, then rounded as the plain copies
    auto store = [&]() {
        T *pa = c3_lds_a(As, t), *pb = c3_lds_b(Bs, t);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            st_lds(pa + j, va[j]);
            st_lds(pa + C3_BM * LDK + j, va[j] * va[j]);
            if constexpr (VAR) st_lds(pa + 2 * C3_BM * LDK + j, va2[j]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            st_lds(pb + 8 * i * LDK, vb[i]);
            st_lds(pb + (C3_BN + 8 * i) * LDK, vb2[i]);
            if constexpr (VAR) st_lds(pb + (2 * C3_BN + 8 * i) * LDK, __builtin_fmaf(vb[i], vb[i], vb2[i]));
        }
    };

    f32x4 acc[2][4][2];                              // [mean | variance]: planes 1 and 2 both add into acc[1]
    c3_zero(acc);
    c3_pipeline(1, e.rbeg, e.rend, fetch, store, [&]() { c3_mfma_planes<T, NPL, 2>(acc, As, Bs, t); });

    // a lane's quad runs along the output position p: with P % 4 == 0 it is four consecutive elements of one image and channel
    const bool vec = c3_vec(g.P);
    c3_each_col(t, e.N, [&](int j, int32_t n) {
        const int32_t o = grp * g.Ng + n;
        const float mb = a.b1 ? a.b1[o] : 0.f, sb = a.b1 ? a.b2[o] : 0.f;
        c3_each_quad(t, e.M, [&](int i, int32_t mq) {
            float r1[4], r2[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                r1[q] = acc[0][i][j][q] + mb;
                r2[q] = acc[1][i][j][q] + sb;
            }
            if (a.act == BNN_FLAG_RELU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) moments_relu_dev(r1[q], r2[q], r1[q], r2[q]);
            } else if (a.act == BNN_FLAG_ELU) {
#pragma unroll 1
                for (int q = 0; q < 4; ++q) moments_elu_dev(r1[q], r2[q], a.elu_alpha, r1[q], r2[q]);
            }
            if (vec) {
                const uint32_t e0 = c3_elem(mq, g.fP, g.P, g.O, o);              // the quad stays inside one image and channel
                *reinterpret_cast<float4 *>(a.out_m + e0) = make_float4(r1[0], r1[1], r1[2], r1[3]);
                *reinterpret_cast<float4 *>(a.out_v + e0) = make_float4(r2[0], r2[1], r2[2], r2[3]);
            } else {
                const int nq = e.M - mq < 4 ? e.M - mq : 4;
                for (int q = 0; q < nq; ++q) {
                    const uint32_t el = c3_elem(mq + q, g.fP, g.P, g.O, o);
                    a.out_m[el] = r1[q];
                    a.out_v[el] = r2[q];
                }
            }
        });
    });
}

// ---- K19: the backward of K17's contraction, for training conv nets without sampling.  With G_m, G_v the (B, O, P) gradients
// with respect to m and v above, convT the transposed contraction and the sums over (image, position) in that order:
//     g_a_m  = convT(G_m, mu_w) + 2 a_m (.) convT(G_v, sigma_w^2)             g_a_v  = convT(G_v, mu_w^2 + sigma_w^2)
//     g_mu_w = sum gather(a_m) G_m + 2 mu_w (.) sum gather(a_v) G_v            g_s2_w = sum gather(a_m^2 + a_v) G_v
// K18's shape (P planes (p1, p2, fma(p1, p1, p2)), Q planes (G_m, G_v) with G_v serving twice, THREE accumulator sets: 96
// accumulator registers per lane) on the tile's DGRAD and WGRAD contractions:
//   DGRAD A = gather(G_m), gather(G_v); B = mu_w^T, sigma_w^2^T and their derived plane.  acc1 = A1 B1, acc2 = A2 B2, acc3 = A2 B3.
//         Epilogue: g_a_m = acc1 + 2 a_m acc2, g_a_v = acc3; a lane's quad runs along the input position (16-byte stores when
//         D H W % 4 == 0).
//   WGRAD A = gather(a_m), gather(a_v) and their derived plane; B = G_m, G_v.  acc1 = A1 B1, acc2 = A2 B2, acc3 = A3 B2.  Slabs
//         [slab][3][O][K] on wgrad_split; k_moments_conv_wsum adds them in slab order and writes g_mu_w = S1 + 2 mu_w S2 and
//         g_rho_w = S3 2 sigma_w sigmoid(rho_w).
// The derived plane is formed in fp32: the bf16 mode rounds it (RNE) into an LDS plane of its own as it is staged; the fp32
// mode forms it from the two fragments it has just read (the same value), so its LDS is K11's.  G_v is staged once and read by
// two MFMA streams.  No sample axis, no atomics, fixed order: identical calls give identical bits.  A deterministic input
// (a_v absent) has K11's backward (bnn_conv3d_lrt_backward_input / _weight with one image set): there is no kernel for it here.
struct MomConvBwdArgs {
    const float *g1, *g2;                    // G_m, G_v, (B, O, P)
    const float *w1, *w2;                    // DGRAD: mu_w, sigma_w^2, O x K
    const float *a_m, *a_v;                  // (B, C, D, H, W); DGRAD reads a_m alone (its epilogue)
    float *out, *out2;                       // DGRAD: g_a_m, g_a_v; WGRAD: out = slab base
    int32_t nslab, chunk;                    // WGRAD: slabs per group, reduction positions per slab (% C3_BK == 0)
};

template <typename T, int MODE>
__global__ __launch_bounds__(C3_THREADS) void k_moments_conv3d_bwd(const Conv3dGeo g, const MomConvBwdArgs a)
{
    static_assert(MODE == C3_DGRAD || MODE == C3_WGRAD, "the forward is k_moments_conv3d");
    constexpr int LDK = Op<T>::LDK;
    constexpr bool BF = sizeof(T) == 2, WG = MODE == C3_WGRAD;
    constexpr int NA = BF && WG ? 3 : 2, NB = BF && !WG ? 3 : 2;     // planes in LDS (the derived one: bf16 only)
    __shared__ __attribute__((aligned(16))) T As[NA * C3_BM * LDK];
    __shared__ __attribute__((aligned(16))) T Bs[NB * C3_BN * LDK];

    const C3Tile t = c3_tile();
    const C3Block k = c3_block<MODE>(g, a.nslab);
    const int grp = k.grp;
    const C3Extents e = c3_extents<MODE>(g, k.slab, a.chunk);
    const C3Row row = c3_row_origin<MODE>(g, t.m0 + t.ar, e.M, grp);

    // va, va2: DGRAD gather(G_m), gather(G_v); WGRAD gather(a_m), gather(a_v)
    float va[16], va2[16], vb[8], vb2[8];
    auto fetch = [&](int, int32_t r0) {
        if constexpr (WG) {
            c3_gather_positions(g, row, r0 + t.ah * 16, e.rend, [&](int j, bool ok, int64_t off, uint32_t) {
                va[j] = ok ? a.a_m[off] : 0.f;
                va2[j] = ok ? a.a_v[off] : 0.f;
            });
            c3_grad_rows(g, t, e.N, grp, r0 + t.bk, e.rend, [&](int i, bool ok, int64_t off, uint32_t, int32_t) {
                vb[i] = ok ? a.g1[off] : 0.f;
                vb2[i] = ok ? a.g2[off] : 0.f;
            });
        } else {
            c3_gather_taps<MODE>(g, row, r0 + t.ah * 16, e.rend, [&](int j, bool ok, int32_t off, uint32_t) {
                va[j] = ok ? a.g1[off] : 0.f;
                va2[j] = ok ? a.g2[off] : 0.f;
            });
            c3_weight_rows<MODE>(g, t, e.N, grp, r0 + t.bk, e.rend, [&](int i, bool ok, int64_t off) {
                vb[i] = ok ? a.w1[off] : 0.f;
                vb2[i] = ok ? a.w2[off] : 0.f;
            });
        }
    };

    // the derived plane in fp32, then rounded as the plain copies (bf16 mode; the fp32 mode forms it from the fragments)
    auto store = [&]() {
        T *pa = c3_lds_a(As, t), *pb = c3_lds_b(Bs, t);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            st_lds(pa + j, va[j]);
            st_lds(pa + C3_BM * LDK + j, va2[j]);
            if constexpr (NA == 3) st_lds(pa + 2 * C3_BM * LDK + j, __builtin_fmaf(va[j], va[j], va2[j]));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            st_lds(pb + 8 * i * LDK, vb[i]);
            st_lds(pb + (C3_BN + 8 * i) * LDK, vb2[i]);
            if constexpr (NB == 3) st_lds(pb + (2 * C3_BN + 8 * i) * LDK, __builtin_fmaf(vb[i], vb[i], vb2[i]));
        }
    };

    f32x4 acc[3][4][2];
    c3_zero(acc);
    auto compute = [&]() {
        if constexpr (BF) {
            // stream h: A plane, B plane -- (0, 0), (1, 1), then G_v's plane again with the derived one
#pragma unroll
            for (int h = 0; h < 3; ++h) {
                const int ha = h < 2 ? h : (WG ? 2 : 1), hb = h < 2 ? h : (WG ? 1 : 2);
                typename Op<T>::frag fa[4], fb[2];
                c3_frag_a<T>(fa, As + ha * C3_BM * LDK, t, 0);
                c3_frag_b<T>(fb, Bs + hb * C3_BN * LDK, t, 0);
                c3_mfma<T>(acc[h], fa, fb);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < C3_BK / 4; ++kk) {
                float fa[3][4], fb[3][2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    c3_frag_a<T>(fa[h], As + h * C3_BM * LDK, t, kk);
                    c3_frag_b<T>(fb[h], Bs + h * C3_BN * LDK, t, kk);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[2][i] = WG ? __builtin_fmaf(fa[0][i], fa[0][i], fa[1][i]) : fa[1][i];
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[2][j] = WG ? fb[1][j] : __builtin_fmaf(fb[0][j], fb[0][j], fb[1][j]);
#pragma unroll
                for (int h = 0; h < 3; ++h) c3_mfma<T>(acc[h], fa[h], fb[h]);
            }
        }
    };
    c3_pipeline(1, e.rbeg, e.rend, fetch, store, compute);

    if constexpr (WG) {
        c3_each_col(t, e.N, [&](int j, int32_t n) {
            c3_each_row(t, e.M, [&](int i, int q, int32_t m) {
                // slab [slab][3][o][k]
                const int64_t plane = (int64_t)g.O * g.K, el = ((int64_t)k.slab * 3 * g.O + grp * g.Ng + n) * g.K + m;
                a.out[el] = acc[0][i][j][q];
                a.out[el + plane] = acc[1][i][j][q];
                a.out[el + 2 * plane] = acc[2][i][j][q];
            });
        });
    } else {
        // a lane's quad runs along the input position: with Pin % 4 == 0 it is four consecutive elements of one image and channel
        const bool vec = c3_vec(g.Pin);
        c3_each_col(t, e.N, [&](int j, int32_t n) {
            c3_each_quad(t, e.M, [&](int i, int32_t mq) {
                if (vec) {
                    const uint32_t e0 = c3_elem(mq, g.fPin, g.Pin, g.C, grp * g.Cg + n);
                    float r1[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) r1[q] = __builtin_fmaf(2.0f * a.a_m[e0 + q], acc[1][i][j][q], acc[0][i][j][q]);
                    *reinterpret_cast<float4 *>(a.out + e0) = make_float4(r1[0], r1[1], r1[2], r1[3]);
                    *reinterpret_cast<float4 *>(a.out2 + e0) =
                        make_float4(acc[2][i][j][0], acc[2][i][j][1], acc[2][i][j][2], acc[2][i][j][3]);
                } else {
                    const int nq = e.M - mq < 4 ? e.M - mq : 4;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (q >= nq) continue;
                        const uint32_t el = c3_elem(mq + q, g.fPin, g.Pin, g.C, grp * g.Cg + n);
                        a.out[el] = __builtin_fmaf(2.0f * a.a_m[el], acc[1][i][j][q], acc[0][i][j][q]);
                        a.out2[el] = acc[2][i][j][q];
                    }
                }
            });
        });
    }
}

// g_mu_w[e] = S1 + 2 mu_w[e] S2, g_rho_w[e] = S3 2 sigma sigmoid(rho_w[e]); S1, S2, S3 the sums of the three slab planes in slab order
__global__ __launch_bounds__(256) void k_moments_conv_wsum(const float *__restrict__ slabs, int nslab, const float *__restrict__ mu,
                                                          const float *__restrict__ rho, float *__restrict__ g_mu,
                                                          float *__restrict__ g_rho, int64_t n)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int k = 0; k < nslab; ++k) {
        const float *p = slabs + (int64_t)k * 3 * n + e;
        s1 += p[0];
        s2 += p[n];
        s3 += p[2 * n];
    }
    const float r = rho[e];
    g_mu[e] = __builtin_fmaf(2.0f * mu[e], s2, s1);
    g_rho[e] = s3 * (2.0f * sigma_lrt(r) * dsigma_lrt(r));
}

static int conv3d_geo(const char *who, const bnn_conv3d_shape_t *sh, int nsamples, int compute, Conv3dGeo &g)
{
    if (!sh) { set_error("%s: NULL shape", who); return BNN_E_NULL; }
    if (sh->B < 1 || sh->C < 1 || sh->D < 1 || sh->H < 1 || sh->W < 1 || sh->O < 1 || sh->KD < 1 || sh->KH < 1 || sh->KW < 1 ||
        sh->stride_d < 1 || sh->stride_h < 1 || sh->stride_w < 1 || sh->dil_d < 1 || sh->dil_h < 1 || sh->dil_w < 1 ||
        sh->pad_d < 0 || sh->pad_h < 0 || sh->pad_w < 0 || sh->groups < 1 || sh->C % sh->groups || sh->O % sh->groups || nsamples < 1) {
        set_error("%s: bad extent", who);
        return BNN_E_SHAPE;
    }
    if (compute != BNN_COMPUTE_F32 && compute != BNN_COMPUTE_BF16) { set_error("%s: unknown compute mode", who); return BNN_E_DTYPE; }
    const int64_t lim = 0x7FFFFFFF;
    if (sh->D > lim || sh->H > lim || sh->W > lim || sh->KD > lim || sh->KH > lim || sh->KW > lim || sh->stride_d > lim ||
        sh->stride_h > lim || sh->stride_w > lim || sh->dil_d > lim || sh->dil_h > lim || sh->dil_w > lim || sh->pad_d > lim ||
        sh->pad_h > lim || sh->pad_w > lim) {
        set_error("%s: an extent of 2^31 or more", who);
        return BNN_E_RANGE;
    }
    const int64_t OD = (sh->D + 2 * sh->pad_d - sh->dil_d * (sh->KD - 1) - 1) / sh->stride_d + 1;
    const int64_t OH = (sh->H + 2 * sh->pad_h - sh->dil_h * (sh->KH - 1) - 1) / sh->stride_h + 1;
    const int64_t OW = (sh->W + 2 * sh->pad_w - sh->dil_w * (sh->KW - 1) - 1) / sh->stride_w + 1;
    if (sh->D + 2 * sh->pad_d < sh->dil_d * (sh->KD - 1) + 1 || sh->H + 2 * sh->pad_h < sh->dil_h * (sh->KH - 1) + 1 ||
        sh->W + 2 * sh->pad_w < sh->dil_w * (sh->KW - 1) + 1 || OD < 1 || OH < 1 || OW < 1) {
        set_error("%s: kernel larger than the padded input", who);
        return BNN_E_SHAPE;
    }
    // one sample's tensors and index arithmetic stay below 2^31 (padded origins and reach included)
    const double B = (double)sh->B, T = (double)sh->KD * sh->KH * sh->KW;
    const double Pin = (double)sh->D * sh->H * sh->W, P = (double)OD * OH * OW;
    if (B * sh->C * Pin >= 2147483647.0 || B * sh->O * P >= 2147483647.0 || (double)sh->O * (sh->C / sh->groups) * T >= 2147483647.0 ||
        (double)(sh->D + sh->pad_d) * sh->H * sh->W >= 2147483647.0 || (double)sh->pad_d + sh->dil_d * (double)sh->KD >= 2147483647.0 ||
        (double)sh->pad_h + sh->dil_h * (double)sh->KH >= 2147483647.0 || (double)sh->pad_w + sh->dil_w * (double)sh->KW >= 2147483647.0 ||
        (double)OD * sh->stride_d + sh->D >= 2147483647.0 || (double)OH * sh->stride_h + sh->H >= 2147483647.0 ||
        (double)OW * sh->stride_w + sh->W >= 2147483647.0 || (double)sh->C * Pin + Pin >= 2147483647.0) {
        set_error("%s: a per-sample tensor of 2^31 elements or more", who);
        return BNN_E_RANGE;
    }
    if ((int64_t)nsamples * sh->groups > 65535) { set_error("%s: nsamples * groups > 65535", who); return BNN_E_RANGE; }
    g.B = (int32_t)sh->B; g.C = (int32_t)sh->C; g.D = (int32_t)sh->D; g.H = (int32_t)sh->H; g.W = (int32_t)sh->W; g.O = (int32_t)sh->O;
    g.KD = (int32_t)sh->KD; g.KH = (int32_t)sh->KH; g.KW = (int32_t)sh->KW;
    g.OD = (int32_t)OD; g.OH = (int32_t)OH; g.OW = (int32_t)OW;
    g.sd = (int32_t)sh->stride_d; g.sh = (int32_t)sh->stride_h; g.sw = (int32_t)sh->stride_w;
    g.pd = (int32_t)sh->pad_d; g.ph = (int32_t)sh->pad_h; g.pw = (int32_t)sh->pad_w;
    g.dd = (int32_t)sh->dil_d; g.dh = (int32_t)sh->dil_h; g.dw = (int32_t)sh->dil_w;
    g.groups = (int32_t)sh->groups; g.Cg = g.C / g.groups; g.Ng = g.O / g.groups;
    g.T = g.KD * g.KH * g.KW; g.K = g.Cg * g.T; g.P = g.OD * g.OH * g.OW; g.Pin = g.D * g.H * g.W;
    g.fOW = make_div(g.OW); g.fOH = make_div(g.OH); g.fP = make_div(g.P);
    g.fW = make_div(g.W); g.fH = make_div(g.H); g.fPin = make_div(g.Pin);
    g.fKW = make_div(g.KW); g.fKH = make_div(g.KH); g.fT = make_div(g.T);
    g.fsd = make_div(g.sd); g.fsh = make_div(g.sh); g.fsw = make_div(g.sw);
    return BNN_OK;
}

static int check_w(const char *who, const void *w, int64_t w_ss, const Conv3dGeo &g, int nsamples, int compute)
{
    if (!w) { set_error("%s: NULL weights", who); return BNN_E_NULL; }
    if (w_ss < 0 || (nsamples > 1 && w_ss > 0 && w_ss < (int64_t)g.O * g.K)) { set_error("%s: bad weight sample stride", who); return BNN_E_SHAPE; }
    if (reinterpret_cast<uintptr_t>(w) & (compute == BNN_COMPUTE_BF16 ? 1u : 3u)) { set_error("%s: misaligned weights", who); return BNN_E_ALIGN; }
    return BNN_OK;
}

// slabs of the weight gradient's reduction: about 1024 workgroups in all, at most 16 slabs, whole k-tiles each
static void wgrad_split(const Conv3dGeo &g, int nsamples, int &nslab, int &chunk)
{
    const int64_t R = (int64_t)g.B * g.P;
    const int64_t tiles = (int64_t)((g.K + C3_BM - 1) / C3_BM) * ((g.Ng + C3_BN - 1) / C3_BN) * nsamples * g.groups;
    int64_t want = (1024 + tiles - 1) / tiles;
    const int64_t ktiles = (R + C3_BK - 1) / C3_BK;
    want = std::min<int64_t>(std::min<int64_t>(want, 16), ktiles);
    while (want > 1 && (int64_t)nsamples * g.groups * want > 65535) --want;
    const int64_t per = (ktiles + want - 1) / want;
    chunk = (int)(per * C3_BK);
    nslab = (int)((R + chunk - 1) / chunk);
}

// One launch of a tile kernel, the compute mode's instantiation of the pair: x over the rows of the mode's contraction, y over
// its columns (c3_extents), z = nz, what the kernel's c3_block decodes.
template <int MODE, typename Args>
static void launch_tile(void (*kbf16)(Conv3dGeo, Args), void (*kf32)(Conv3dGeo, Args), const Conv3dGeo &g, const Args &a, int compute,
                        int64_t nz, hipStream_t st)
{
    const int64_t M = MODE == C3_FWD ? (int64_t)g.B * g.P : MODE == C3_DGRAD ? (int64_t)g.B * g.Pin : g.K;
    const int32_t N = MODE == C3_DGRAD ? g.Cg : g.Ng;
    const dim3 grid((unsigned)((M + C3_BM - 1) / C3_BM), (unsigned)((N + C3_BN - 1) / C3_BN), (unsigned)nz);
    const auto kernel = compute == BNN_COMPUTE_BF16 ? kbf16 : kf32;
    hipLaunchKernelGGL(kernel, grid, dim3(C3_THREADS), 0, st, g, a);
}

template <int MODE, bool FLIP = false>
static void launch(const Conv3dGeo &g, const Conv3dArgs &a, int compute, int64_t nz, hipStream_t st)
{
    launch_tile<MODE>(k_conv3d<uint16_t, MODE, FLIP>, k_conv3d<float, MODE, FLIP>, g, a, compute, nz, st);
}

// the Flipout entries' shared checks: K7's index ranges (conv3d_geo), groups == 1, the signs' layout
static int flip_geo(const char *who, const bnn_conv3d_shape_t *sh, int nsamples, int compute, Conv3dGeo &g)
{
    int rc = conv3d_geo(who, sh, nsamples, compute, g);
    if (rc) return rc;
    if (g.groups != 1) { set_error("%s: groups != 1", who); return BNN_E_UNSUPPORTED; }
    if ((double)g.B * (g.O + g.C) >= 2147483647.0) { set_error("%s: B (O + C) signs of 2^31 or more", who); return BNN_E_RANGE; }
    return BNN_OK;
}

static int check_signs(const char *who, const float *sg, int64_t sg_ss, const Conv3dGeo &g, int nsamples)
{
    if (!sg) { set_error("%s: NULL signs", who); return BNN_E_NULL; }
    if (sg_ss < 0 || (nsamples > 1 && sg_ss > 0 && sg_ss < (int64_t)g.B * (g.O + g.C))) {
        set_error("%s: bad sign sample stride", who);
        return BNN_E_SHAPE;
    }
    if (misaligned(sg, 3)) { set_error("%s: misaligned signs", who); return BNN_E_ALIGN; }
    return BNN_OK;
}

// [mean | stddev] rows: the stddev row starts one padded row (bf16: a multiple of 8 elements) after the mean row
static int64_t flip_w_std(const Conv3dGeo &g, int compute)
{
    const int64_t n = (int64_t)g.O * g.K;
    return compute == BNN_COMPUTE_BF16 ? (n + 7) / 8 * 8 : n;
}

// K11 (LocalReparamConv1d / 2d / 3d)
template <int MODE>
static void lrt_conv_launch(const Conv3dGeo &g, const LrtConvArgs &a, int compute, int64_t nz, hipStream_t st)
{
    launch_tile<MODE>(k_lrt_conv3d<uint16_t, MODE>, k_lrt_conv3d<float, MODE>, g, a, compute, nz, st);
}

// K11 / K24: the weight gradient of a local-reparameterization conv layer -- the checks, the paired slabs, their reduce with the
// posterior's CHAIN, the bias sums.  par_w: rho_w or log_sigma2; g_mean_w / g_par_w: the gradients of the weight's mean and of par_w.
template <typename CHAIN>
static int lrt_conv_backward_weight(const char *who, const float *x, const float *g_m, const float *g_v, const float *par_w,
                                    float *g_mean_w, float *g_par_w, const float *rho_b, float *g_mu_b, float *g_rho_b,
                                    const bnn_conv3d_shape_t *shape, int nsets, int compute, void *workspace, int64_t workspace_bytes,
                                    hipStream_t st)
{
    Conv3dGeo g;
    int rc = conv3d_geo(who, shape, nsets, compute, g);
    if (rc) return rc;
    const bool bias = rho_b || g_mu_b || g_rho_b;
    if (!x || !g_m || !g_v || !par_w || !g_mean_w || !g_par_w || (bias && (!rho_b || !g_mu_b || !g_rho_b))) {
        set_error("%s: NULL pointer", who);
        return BNN_E_NULL;
    }
    if (misaligned(x, 3) || misaligned(g_m, 3) || misaligned(g_v, 3) || misaligned(par_w, 3) || misaligned(g_mean_w, 3) ||
        misaligned(g_par_w, 3) || misaligned(rho_b, 3) || misaligned(g_mu_b, 3) || misaligned(g_rho_b, 3) || misaligned(workspace, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    int nslab, chunk;
    wgrad_split(g, 1, nslab, chunk);           // one image set: every slab walks all of them
    const int64_t n = (int64_t)g.O * g.K;
    if (!workspace || workspace_bytes < (int64_t)nslab * 2 * n * (int64_t)sizeof(float)) {
        set_error("%s: workspace of bnn_conv3d_lrt_backward_weight_workspace_bytes bytes needed", who);
        return BNN_E_UNSUPPORTED;
    }
    LrtConvArgs a{};
    a.x = x; a.x_ss = (int64_t)g.B * g.C * g.Pin; a.g1 = g_m; a.g2 = g_v; a.out = static_cast<float *>(workspace);
    a.S = nsets; a.nslab = nslab; a.chunk = chunk;
    lrt_conv_launch<C3_WGRAD>(g, a, compute, g.groups * nslab, st);
    if ((rc = check_launch(who))) return rc;
    hipLaunchKernelGGL(k_lrt_conv_wsum<CHAIN>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       static_cast<const float *>(workspace), nslab, par_w, g_mean_w, g_par_w, n);
    if ((rc = check_launch(who)) || !bias) return rc;
    hipLaunchKernelGGL(k_lrt_conv_bias_grad, dim3((unsigned)g.O), dim3(256), 0, st, g_m, g_v, (int64_t)nsets * g.B, g.O, g.P, rho_b,
                       g_mu_b, g_rho_b);
    return check_launch(who);
}

// K17: the instantiation with the a_v planes for an input that carries a variance
static void mom_conv_launch(const Conv3dGeo &g, const MomConvArgs &a, int compute, hipStream_t st)
{
    if (a.a_v) launch_tile<C3_FWD>(k_moments_conv3d<uint16_t, true>, k_moments_conv3d<float, true>, g, a, compute, g.groups, st);
    else launch_tile<C3_FWD>(k_moments_conv3d<uint16_t, false>, k_moments_conv3d<float, false>, g, a, compute, g.groups, st);
}

// K19
template <int MODE>
static void mom_conv_bwd_launch(const Conv3dGeo &g, const MomConvBwdArgs &a, int compute, int64_t nz, hipStream_t st)
{
    launch_tile<MODE>(k_moments_conv3d_bwd<uint16_t, MODE>, k_moments_conv3d_bwd<float, MODE>, g, a, compute, nz, st);
}

// K17 / K19: the shape with B == 0 admitted (every check runs on one image; the entry launches no tile)
static int conv3d_geo_b0(const char *who, const bnn_conv3d_shape_t *shape, int compute, Conv3dGeo &g, bool &empty)
{
    if (!shape) { set_error("%s: NULL shape", who); return BNN_E_NULL; }
    bnn_conv3d_shape_t sh = *shape;
    empty = sh.B == 0;
    if (empty) sh.B = 1;
    return conv3d_geo(who, &sh, 1, compute, g);
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_conv3d_forward_drawn(const float *x, int64_t x_sample_stride, const void *w, int64_t w_sample_stride,
                             const float *b, int64_t b_sample_stride, float *y, const bnn_conv3d_shape_t *shape,
                             int nsamples, int compute, void *stream)
{
    const char *who = "bnn_conv3d_forward_drawn";
    Conv3dGeo g;
    int rc = conv3d_geo(who, shape, nsamples, compute, g);
    if (rc) return rc;
    if (!x || !y) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if ((rc = check_w(who, w, w_sample_stride, g, nsamples, compute))) return rc;
    if (x_sample_stride < 0 || b_sample_stride < 0) { set_error("%s: negative sample stride", who); return BNN_E_SHAPE; }
    if (misaligned(x, 3) || misaligned(y, 3) || misaligned(b, 3)) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    Conv3dArgs a{};
    a.x = x; a.x_ss = x_sample_stride; a.w = w; a.w_ss = w_sample_stride; a.bias = b; a.b_ss = b_sample_stride; a.out = y;
    a.S = nsamples; a.shared = x_sample_stride == 0;
    launch<C3_FWD>(g, a, compute, nsamples * g.groups, (hipStream_t)stream);
    return check_launch(who);
}

int bnn_conv3d_backward_input(const float *gy, const void *w, int64_t w_sample_stride, float *gx, int shared_x,
                              const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *stream)
{
    const char *who = "bnn_conv3d_backward_input";
    Conv3dGeo g;
    int rc = conv3d_geo(who, shape, nsamples, compute, g);
    if (rc) return rc;
    if (!gy || !gx) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if ((rc = check_w(who, w, w_sample_stride, g, nsamples, compute))) return rc;
    if (misaligned(gy, 3) || misaligned(gx, 3)) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    Conv3dArgs a{};
    a.gy = gy; a.w = w; a.w_ss = w_sample_stride; a.out = gx; a.S = nsamples; a.shared = shared_x ? 1 : 0;
    launch<C3_DGRAD>(g, a, compute, (shared_x ? 1 : nsamples) * g.groups, (hipStream_t)stream);
    return check_launch(who);
}

int64_t bnn_conv3d_backward_weight_workspace_bytes(const bnn_conv3d_shape_t *shape, int nsamples)
{
    Conv3dGeo g;
    if (conv3d_geo("bnn_conv3d_backward_weight_workspace_bytes", shape, nsamples, BNN_COMPUTE_F32, g)) return -1;
    int nslab, chunk;
    wgrad_split(g, nsamples, nslab, chunk);
    return nslab > 1 ? (int64_t)nslab * nsamples * g.O * g.K * (int64_t)sizeof(float) : 0;
}

int bnn_conv3d_backward_weight(const float *x, int64_t x_sample_stride, const float *gy, float *gw, float *gb,
                               const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    const char *who = "bnn_conv3d_backward_weight";
    Conv3dGeo g;
    int rc = conv3d_geo(who, shape, nsamples, compute, g);
    if (rc) return rc;
    if (!gy || (gw && !x) || (!gw && !gb)) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (x_sample_stride < 0) { set_error("%s: negative sample stride", who); return BNN_E_SHAPE; }
    if (misaligned(x, 3) || misaligned(gy, 3) || misaligned(gw, 3) || misaligned(gb, 3) || misaligned(workspace, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    hipStream_t st = (hipStream_t)stream;
    if (gw) {
        int nslab, chunk;
        wgrad_split(g, nsamples, nslab, chunk);
        const int64_t n = (int64_t)nsamples * g.O * g.K;
        if (nslab > 1 && (!workspace || workspace_bytes < nslab * n * (int64_t)sizeof(float))) {
            set_error("%s: workspace of bnn_conv3d_backward_weight_workspace_bytes bytes needed", who);
            return BNN_E_UNSUPPORTED;
        }
        Conv3dArgs a{};
        a.x = x; a.x_ss = x_sample_stride; a.gy = gy; a.out = nslab > 1 ? static_cast<float *>(workspace) : gw;
        a.S = nsamples; a.nslab = nslab; a.chunk = chunk;
        launch<C3_WGRAD>(g, a, compute, nsamples * g.groups * nslab, st);
        if ((rc = check_launch(who))) return rc;
        if (nslab > 1) {
            hipLaunchKernelGGL(k_conv3d_slab_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const float *>(workspace), n,
                               nslab, gw, n);
            if ((rc = check_launch(who))) return rc;
        }
    }
    if (gb) {
        hipLaunchKernelGGL(k_conv3d_bias_grad, dim3((unsigned)g.O, (unsigned)nsamples), dim3(256), 0, st, gy, gb, g.B, g.O, g.P);
        if ((rc = check_launch(who))) return rc;
    }
    return BNN_OK;
}

int bnn_conv3d_flipout_forward(const float *x, int64_t x_sample_stride, const void *w, const float *signs, int64_t sign_sample_stride,
                               float *y, const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *stream)
{
    const char *who = "bnn_conv3d_flipout_forward";
    Conv3dGeo g;
    int rc = flip_geo(who, shape, nsamples, compute, g);
    if (rc) return rc;
    if (!x || !y) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if ((rc = check_w(who, w, 0, g, nsamples, compute))) return rc;
    if ((rc = check_signs(who, signs, sign_sample_stride, g, nsamples))) return rc;
    if (x_sample_stride < 0) { set_error("%s: negative sample stride", who); return BNN_E_SHAPE; }
    if (misaligned(x, 3) || misaligned(y, 3)) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    Conv3dArgs a{};
    a.x = x; a.x_ss = x_sample_stride; a.w = w; a.w_std = flip_w_std(g, compute); a.out = y;
    a.sg = signs; a.sg_ss = sign_sample_stride; a.S = nsamples; a.shared = x_sample_stride == 0;
    launch<C3_FWD, true>(g, a, compute, nsamples, (hipStream_t)stream);
    return check_launch(who);
}

int bnn_conv3d_flipout_backward_input(const float *gy, const void *w, const float *signs, int64_t sign_sample_stride, float *gx,
                                      int shared_x, const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *stream)
{
    const char *who = "bnn_conv3d_flipout_backward_input";
    Conv3dGeo g;
    int rc = flip_geo(who, shape, nsamples, compute, g);
    if (rc) return rc;
    if (!gy || !gx) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if ((rc = check_w(who, w, 0, g, nsamples, compute))) return rc;
    if ((rc = check_signs(who, signs, sign_sample_stride, g, nsamples))) return rc;
    if (misaligned(gy, 3) || misaligned(gx, 3)) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    Conv3dArgs a{};
    a.gy = gy; a.w = w; a.w_std = flip_w_std(g, compute); a.out = gx; a.S = nsamples; a.shared = shared_x ? 1 : 0;
    a.sg = signs; a.sg_ss = sign_sample_stride;
    launch<C3_DGRAD, true>(g, a, compute, shared_x ? 1 : nsamples, (hipStream_t)stream);
    return check_launch(who);
}

int64_t bnn_conv3d_flipout_backward_weight_workspace_bytes(const bnn_conv3d_shape_t *shape, int nsamples)
{
    Conv3dGeo g;
    if (flip_geo("bnn_conv3d_flipout_backward_weight_workspace_bytes", shape, nsamples, BNN_COMPUTE_F32, g)) return -1;
    int nslab, chunk;
    wgrad_split(g, nsamples, nslab, chunk);
    return (int64_t)nslab * nsamples * 2 * g.O * g.K * (int64_t)sizeof(float);
}

int bnn_conv3d_flipout_backward_weight(const float *x, int64_t x_sample_stride, const float *gy, const float *signs,
                                       int64_t sign_sample_stride, const float *rho, float *g_mean, float *g_scale,
                                       const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *workspace,
                                       int64_t workspace_bytes, void *stream)
{
    const char *who = "bnn_conv3d_flipout_backward_weight";
    Conv3dGeo g;
    int rc = flip_geo(who, shape, nsamples, compute, g);
    if (rc) return rc;
    if (!x || !gy || !rho || !g_mean || !g_scale) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if ((rc = check_signs(who, signs, sign_sample_stride, g, nsamples))) return rc;
    if (x_sample_stride < 0) { set_error("%s: negative sample stride", who); return BNN_E_SHAPE; }
    if (misaligned(x, 3) || misaligned(gy, 3) || misaligned(rho, 3) || misaligned(g_mean, 3) || misaligned(g_scale, 3) || misaligned(workspace, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    int nslab, chunk;
    wgrad_split(g, nsamples, nslab, chunk);
    const int64_t n = (int64_t)g.O * g.K;
    if (!workspace || workspace_bytes < (int64_t)nslab * nsamples * 2 * n * (int64_t)sizeof(float)) {
        set_error("%s: workspace of bnn_conv3d_flipout_backward_weight_workspace_bytes bytes needed", who);
        return BNN_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    Conv3dArgs a{};
    a.x = x; a.x_ss = x_sample_stride; a.gy = gy; a.out = static_cast<float *>(workspace);
    a.S = nsamples; a.nslab = nslab; a.chunk = chunk; a.sg = signs; a.sg_ss = sign_sample_stride;
    launch<C3_WGRAD, true>(g, a, compute, nsamples * nslab, st);
    if ((rc = check_launch(who))) return rc;
    hipLaunchKernelGGL(k_conv3d_flip_wsum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const float *>(workspace),
                       nslab, nsamples, rho, g_mean, g_scale, n);
    return check_launch(who);
}

// ---- K11 entries (LocalReparamConv1d / 2d / 3d) ----------------------------------------------------------------------------
int bnn_conv3d_lrt_forward(const float *x, int64_t x_sample_stride, const float *mu_w, const float *s2_w, const float *mu_b,
                           const float *s2_b, float *y, float *v_out, const bnn_conv3d_shape_t *shape, int nsamples,
                           const bnn_rng_t *rng, int compute, void *stream)
{
    const char *who = "bnn_conv3d_lrt_forward";
    Conv3dGeo g;
    int rc = conv3d_geo(who, shape, nsamples, compute, g);
    if (rc) return rc;
    if (!x || !mu_w || !s2_w || !y || (mu_b == nullptr) != (s2_b == nullptr)) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (!rng) { set_error("%s: NULL rng", who); return BNN_E_NULL; }
    if (x_sample_stride < 0) { set_error("%s: negative sample stride", who); return BNN_E_SHAPE; }
    if ((rc = check_rng(rng, nsamples))) { set_error("%s: bad rng", who); return rc; }
    if (misaligned(x, 3) || misaligned(mu_w, 3) || misaligned(s2_w, 3) || misaligned(mu_b, 3) || misaligned(s2_b, 3) ||
        misaligned(y, 15) || misaligned(v_out, 15)) {
        set_error("%s: misaligned pointer (y and v: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    LrtConvArgs a{};
    a.x = x; a.x_ss = x_sample_stride; a.w1 = mu_w; a.w2 = s2_w; a.b1 = mu_b; a.b2 = s2_b; a.out = y; a.out2 = v_out;
    a.S = nsamples; a.shared = x_sample_stride == 0;
    a.rng = make_rng(rng);
    lrt_conv_launch<C3_FWD>(g, a, compute, (a.shared ? 1 : nsamples) * g.groups, (hipStream_t)stream);
    return check_launch(who);
}

int bnn_conv3d_lrt_backward_input(const float *g_m, const float *g_v, const float *mu_w, const float *s2_w, const float *x,
                                  float *gx, const bnn_conv3d_shape_t *shape, int nsets, int compute, void *stream)
{
    const char *who = "bnn_conv3d_lrt_backward_input";
    Conv3dGeo g;
    int rc = conv3d_geo(who, shape, nsets, compute, g);
    if (rc) return rc;
    if (!g_m || !g_v || !mu_w || !s2_w || !x || !gx) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (misaligned(g_m, 3) || misaligned(g_v, 3) || misaligned(mu_w, 3) || misaligned(s2_w, 3) || misaligned(x, 3) || misaligned(gx, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    LrtConvArgs a{};
    a.g1 = g_m; a.g2 = g_v; a.w1 = mu_w; a.w2 = s2_w; a.x = x; a.x_ss = (int64_t)g.B * g.C * g.Pin; a.out = gx; a.S = nsets;
    lrt_conv_launch<C3_DGRAD>(g, a, compute, nsets * g.groups, (hipStream_t)stream);
    return check_launch(who);
}

int64_t bnn_conv3d_lrt_backward_weight_workspace_bytes(const bnn_conv3d_shape_t *shape, int nsets)
{
    Conv3dGeo g;
    if (conv3d_geo("bnn_conv3d_lrt_backward_weight_workspace_bytes", shape, nsets, BNN_COMPUTE_F32, g)) return -1;
    int nslab, chunk;
    wgrad_split(g, 1, nslab, chunk);           // one image set: every slab walks all of them
    return (int64_t)nslab * 2 * g.O * g.K * (int64_t)sizeof(float);
}

int bnn_conv3d_lrt_backward_weight(const float *x, const float *g_m, const float *g_v, const float *rho_w, float *g_mu_w,
                                   float *g_rho_w, const float *rho_b, float *g_mu_b, float *g_rho_b,
                                   const bnn_conv3d_shape_t *shape, int nsets, int compute, void *workspace,
                                   int64_t workspace_bytes, void *stream)
{
    return lrt_conv_backward_weight<ChainRho>("bnn_conv3d_lrt_backward_weight", x, g_m, g_v, rho_w, g_mu_w, g_rho_w, rho_b, g_mu_b,
                                              g_rho_b, shape, nsets, compute, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- K24 entry (VariationalDropoutConv1d / 2d / 3d): K11's launches, the slab reduce with the chain factor of log_sigma2 --------
int bnn_conv3d_vd_backward_weight(const float *x, const float *g_m, const float *g_v, const float *log_sigma2, float *g_theta,
                                  float *g_log_sigma2, const float *rho_b, float *g_mu_b, float *g_rho_b,
                                  const bnn_conv3d_shape_t *shape, int nsets, int compute, void *workspace,
                                  int64_t workspace_bytes, void *stream)
{
    return lrt_conv_backward_weight<ChainLogSigma2>("bnn_conv3d_vd_backward_weight", x, g_m, g_v, log_sigma2, g_theta, g_log_sigma2,
                                                    rho_b, g_mu_b, g_rho_b, shape, nsets, compute, workspace, workspace_bytes,
                                                    (hipStream_t)stream);
}

// ---- K17 entry (moment propagation through NormalConv / LocalReparamConv 1d / 2d / 3d) ---------------------------------------
int bnn_conv3d_moments_forward(const float *a_m, const float *a_v, const float *mu_w, const float *s2_w, const float *mu_b,
                               const float *s2_b, float *out_m, float *out_v, const bnn_conv3d_shape_t *shape, int compute,
                               int flags, float elu_alpha, void *stream)
{
    const char *who = "bnn_conv3d_moments_forward";
    Conv3dGeo g;
    bool empty;                                 // no images: every other check still runs, nothing is launched
    const int rc = conv3d_geo_b0(who, shape, compute, g, empty);
    if (rc) return rc;
    if (!a_m || !mu_w || !s2_w || !out_m || !out_v || (mu_b == nullptr) != (s2_b == nullptr)) {
        set_error("%s: NULL pointer (mu_b and s2_b: both or neither)", who);
        return BNN_E_NULL;
    }
    if (flags & ~(BNN_FLAG_RELU | BNN_FLAG_ELU)) { set_error("%s: unknown flag", who); return BNN_E_UNSUPPORTED; }
    if ((flags & BNN_FLAG_RELU) && (flags & BNN_FLAG_ELU)) {
        set_error("%s: BNN_FLAG_RELU and BNN_FLAG_ELU together", who);
        return BNN_E_UNSUPPORTED;
    }
    if ((flags & BNN_FLAG_ELU) && (!(elu_alpha >= 0.0f) || elu_alpha > 3.0e38f)) {
        set_error("%s: elu_alpha must be finite and >= 0", who);
        return BNN_E_RANGE;
    }
    if (misaligned(a_m, 3) || misaligned(a_v, 3) || misaligned(mu_w, 3) || misaligned(s2_w, 3) || misaligned(mu_b, 3) ||
        misaligned(s2_b, 3) || misaligned(out_m, 15) || misaligned(out_v, 15)) {
        set_error("%s: misaligned pointer (out_m and out_v: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    if ((g.Ng + C3_BN - 1) / C3_BN > 65535) { set_error("%s: more than 64 * 65535 output channels per group", who); return BNN_E_RANGE; }
    if (empty) return BNN_OK;
    MomConvArgs a{};
    a.a_m = a_m; a.a_v = a_v; a.w1 = mu_w; a.w2 = s2_w; a.b1 = mu_b; a.b2 = s2_b; a.out_m = out_m; a.out_v = out_v;
    a.act = flags & (BNN_FLAG_RELU | BNN_FLAG_ELU);
    a.elu_alpha = elu_alpha;
    mom_conv_launch(g, a, compute, (hipStream_t)stream);
    return check_launch(who);
}

// ---- K19 entries (the backward of bnn_conv3d_moments_forward for an input that carries a variance) ----------------------------
// the shape with B == 0 admitted and the grid's y range
static int momb_conv_geo(const char *who, const bnn_conv3d_shape_t *shape, int compute, Conv3dGeo &g, bool &empty)
{
    const int rc = conv3d_geo_b0(who, shape, compute, g, empty);
    if (rc) return rc;
    if ((g.Ng + C3_BN - 1) / C3_BN > 65535 || (g.Cg + C3_BN - 1) / C3_BN > 65535) {
        set_error("%s: more than 64 * 65535 channels per group", who);
        return BNN_E_RANGE;
    }
    return BNN_OK;
}

int bnn_conv3d_moments_backward_input(const float *g_m, const float *g_v, const float *mu_w, const float *s2_w, const float *a_m,
                                      float *g_a_m, float *g_a_v, const bnn_conv3d_shape_t *shape, int compute, void *stream)
{
    const char *who = "bnn_conv3d_moments_backward_input";
    Conv3dGeo g;
    bool empty;
    const int rc = momb_conv_geo(who, shape, compute, g, empty);
    if (rc) return rc;
    if (!g_m || !g_v || !mu_w || !s2_w || !a_m || !g_a_m) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (!g_a_v) {
        set_error("%s: NULL g_a_v (a deterministic input takes bnn_conv3d_lrt_backward_input with nsets = 1)", who);
        return BNN_E_NULL;
    }
    if (misaligned(g_m, 3) || misaligned(g_v, 3) || misaligned(mu_w, 3) || misaligned(s2_w, 3) || misaligned(a_m, 3) ||
        misaligned(g_a_m, 15) || misaligned(g_a_v, 15)) {
        set_error("%s: misaligned pointer (g_a_m and g_a_v: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    if (empty) return BNN_OK;
    MomConvBwdArgs a{};
    a.g1 = g_m; a.g2 = g_v; a.w1 = mu_w; a.w2 = s2_w; a.a_m = a_m; a.out = g_a_m; a.out2 = g_a_v;
    mom_conv_bwd_launch<C3_DGRAD>(g, a, compute, g.groups, (hipStream_t)stream);
    return check_launch(who);
}

int64_t bnn_conv3d_moments_wgrad_workspace(const bnn_conv3d_shape_t *shape)
{
    Conv3dGeo g;
    bool empty;
    if (momb_conv_geo("bnn_conv3d_moments_wgrad_workspace", shape, BNN_COMPUTE_F32, g, empty)) return -1;
    int nslab, chunk;
    wgrad_split(g, 1, nslab, chunk);
    return (int64_t)nslab * 3 * g.O * g.K * (int64_t)sizeof(float);
}

int bnn_conv3d_moments_backward_weight(const float *a_m, const float *a_v, const float *g_m, const float *g_v, const float *mu_w,
                                       const float *rho_w, float *g_mu_w, float *g_rho_w, const float *rho_b, float *g_mu_b,
                                       float *g_rho_b, const bnn_conv3d_shape_t *shape, int compute, void *workspace,
                                       int64_t workspace_bytes, void *stream)
{
    const char *who = "bnn_conv3d_moments_backward_weight";
    Conv3dGeo g;
    bool empty;
    int rc = momb_conv_geo(who, shape, compute, g, empty);
    if (rc) return rc;
    const bool bias = rho_b || g_mu_b || g_rho_b;
    if (!a_m || !g_m || !g_v || !mu_w || !rho_w || !g_mu_w || !g_rho_w || (bias && (!rho_b || !g_mu_b || !g_rho_b))) {
        set_error("%s: NULL pointer (rho_b, g_mu_b and g_rho_b: all or none)", who);
        return BNN_E_NULL;
    }
    if (!a_v) {
        set_error("%s: NULL a_v (a deterministic input takes bnn_conv3d_lrt_backward_weight with nsets = 1)", who);
        return BNN_E_NULL;
    }
    if (misaligned(a_m, 3) || misaligned(a_v, 3) || misaligned(g_m, 3) || misaligned(g_v, 3) || misaligned(mu_w, 3) ||
        misaligned(rho_w, 3) || misaligned(g_mu_w, 15) || misaligned(g_rho_w, 15) || misaligned(rho_b, 3) || misaligned(g_mu_b, 3) ||
        misaligned(g_rho_b, 3) || misaligned(workspace, 3)) {
        set_error("%s: misaligned pointer (g_mu_w and g_rho_w: 16 bytes)", who);
        return BNN_E_ALIGN;
    }
    int nslab, chunk;
    wgrad_split(g, 1, nslab, chunk);
    const int64_t n = (int64_t)g.O * g.K;
    if (!workspace || workspace_bytes < (int64_t)nslab * 3 * n * (int64_t)sizeof(float)) {
        set_error("%s: workspace of bnn_conv3d_moments_wgrad_workspace bytes needed", who);
        return BNN_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    if (empty) nslab = 0;                         // no images: no slab is written, the reduce stores zeros
    else {
        MomConvBwdArgs a{};
        a.a_m = a_m; a.a_v = a_v; a.g1 = g_m; a.g2 = g_v; a.out = static_cast<float *>(workspace);
        a.nslab = nslab; a.chunk = chunk;
        mom_conv_bwd_launch<C3_WGRAD>(g, a, compute, g.groups * nslab, st);
        if ((rc = check_launch(who))) return rc;
    }
    hipLaunchKernelGGL(k_moments_conv_wsum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const float *>(workspace),
                       nslab, mu_w, rho_w, g_mu_w, g_rho_w, n);
    if ((rc = check_launch(who)) || !bias) return rc;
    hipLaunchKernelGGL(k_lrt_conv_bias_grad, dim3((unsigned)g.O), dim3(256), 0, st, g_m, g_v, (int64_t)(empty ? 0 : g.B), g.O, g.P, rho_b,
                       g_mu_b, g_rho_b);
    return check_launch(who);
}

}  // extern "C"
