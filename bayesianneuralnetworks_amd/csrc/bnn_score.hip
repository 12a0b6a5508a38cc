// bnn_score.hip -- an MC forward scored against its labels in ONE launch (K14): per row the predictive mean, the negative
// log-likelihood of the MC predictive, the expected per-sample NLL (the ELBO's data term), the Brier score, the confidence, the
// prediction and the entropy; plus (optional) a device accumulator that carries their sums and the calibration / rejection
// histograms across the batches of a test set.
// replaces  the host loop of examples/*/prune.py:52-65 (stack, mean, argmax, compare, sum on the host batch after batch)
//
// The row reductions are bnn_uncertainty.hip's (bnn_mc_parts.hpp): z_s = the sum over the parts of addend (part * S + s) in
// HeadPartials.logits()'s order, p_s = softmax(z_s) (LOGITS) or z_s (PROBS), the sums over samples fp64 in a fixed order, the
// narrow (classes <= 16: a lane per (row, sample)) and wide (a wave or the workgroup per row) work splits.  `mean` and
// `entropy` are therefore the bits bnn_mc_uncertainty gives as `mean` and `total`.  What a sample adds here:
//   LOGITS  log2 p_s[y] = t_y - log2 Z  (t = (z - max) log2 e, Z = sum 2^t): the same v_log_f32 the per-sample entropy of K4 takes.
//           expected_nll sums -(log2 p_s[y]) in fp64.  nll is the log-sum-exp of log2 p_s[y] over the samples, kept as
//           (M, A): A = sum_s 2^(log2 p_s[y] - M) in fp64 with M an INTEGER >= every exponent seen, so that raising M rescales
//           A by an exact power of two -- the result does not depend on how often the maximum moved, and two partial sums
//           merge exactly (the narrow split's lanes).  It stays finite where p_s[y] underflows fp32.
//   PROBS   expected_nll sums -log2(p_s[y] + 1e-10); nll = -ln(mean[y] + 1e-10), the log as K4 takes the mean's entropy term
//           (v_log_f32 on the fp32-rounded mean).
// A target outside [0, classes) -- compared as the int64 it is -- reads column 0 instead and makes the row's nll, expected_nll
// and brier NaN; nothing else changes.
//
// The accumulator: the launch leaves five words per row in `workspace` (nll, expected_nll, brier, confidence as written, and
// the row's two bins + its correct bit), and a second one-workgroup launch adds them to `state`: the three fp64 sums
// lane-strided in row order then a fixed tree, the counts as integers in LDS, the confidence sums in 2^-31 fixed point (integer
// adds: order-free).  No float atomics, no global atomics: bitwise reproducible.
#include "bnn_mc_parts.hpp"

namespace bnn {

constexpr int kScoreMaxBins = 128;
struct ScoreArgs {
    UncArgs u;                              // u.mean may be NULL; u.total / aleatoric / epistemic unused
    const int64_t *target;
    float *nll, *expected_nll, *brier, *confidence, *entropy;
    int64_t *prediction;
    float *rec;                             // workspace: 5 x rows words (NULL without a state)
    int conf_bins, ent_bins;
    double ent_scale;                       // ent_bins / ln(classes)
};

// What the row's last lane writes once the row's sums are known.  m_y: the fp64 mean at the label (PROBS).
template <int KIND>
__device__ __forceinline__ void score_row_out(const ScoreArgs &A, int64_t r, bool ok, int64_t y64, const Lse &L, double enll_bits,
                                              double m_y, double brier, double tot_bits, float conf, int pred)
{
    const int S = A.u.nsamples;
    const float nan = __builtin_nanf("");
    double nll;
    if constexpr (KIND == BNN_UNC_LOGITS) nll = lse_nll(L, S);
    else nll = -kLn2 * (double)__builtin_amdgcn_logf((float)m_y + 1e-10f);
    const float f_nll = ok ? (float)nll : nan;
    const float f_enll = ok ? (float)(enll_bits * kLn2 / (double)S) : nan;
    const float f_brier = ok ? (float)brier : nan;
    const float f_ent = (float)(tot_bits * kLn2);
    const bool correct = ok && (int64_t)pred == y64;
    if (A.nll) A.nll[r] = f_nll;
    if (A.expected_nll) A.expected_nll[r] = f_enll;
    if (A.brier) A.brier[r] = f_brier;
    if (A.confidence) A.confidence[r] = conf;
    if (A.prediction) A.prediction[r] = (int64_t)pred;
    if (A.entropy) A.entropy[r] = f_ent;
    if (A.rec) {
        // the bins of the fp32 values just written, in fp64: min(bins - 1, floor(confidence bins)), clamp(floor(entropy / ln C bins))
        const double cb = floor((double)conf * (double)A.conf_bins), eb = floor((double)f_ent * A.ent_scale);
        const int cbin = cb >= (double)A.conf_bins ? A.conf_bins - 1 : (cb >= 0.0 ? (int)cb : 0);      // (NaN: bin 0)
        const int ebin = eb >= (double)A.ent_bins ? A.ent_bins - 1 : (eb >= 0.0 ? (int)eb : 0);
        const int64_t R = A.u.rows;
        A.rec[r] = f_nll;
        A.rec[R + r] = f_enll;
        A.rec[2 * R + r] = f_brier;
        A.rec[3 * R + r] = conf;
        reinterpret_cast<uint32_t *>(A.rec)[4 * R + r] = ((uint32_t)ebin << 16) | ((uint32_t)cbin << 1) | (correct ? 1u : 0u);
    }
}

// ---------------------------------------------------------------------------------------------- narrow: classes <= 16
// k_unc_narrow's split: lane = (row, sl), sl = lane & (G - 1) takes samples sl, sl + G, ...
template <int KIND, bool FUSED>
__global__ __launch_bounds__(kUncThreads) void k_score_narrow(ScoreArgs A, int glog, int rpb, uint32_t *advance_epoch,
                                                              uint32_t advance_inc)
{
    constexpr int NV = kUncNarrow;
    unc_advance(advance_epoch, advance_inc);
    const int nwork = (int)gridDim.x;
    const NarrowLane lane(glog, rpb);
    const int G = lane.G, sl = lane.sl;
    const int C = A.u.classes, S = A.u.nsamples;
    for (int64_t rb = blockIdx.x; rb * rpb < A.u.rows; rb += nwork) {
        const int64_t r = rb * rpb + lane.lr;
        const bool live = lane.live(r, A.u.rows);
        double acc[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = 0.0;
        double eacc = 0.0;                                          // sum of -log2 p_s[y]
        Lse L{kLseEmpty, 0.0};
        const int64_t y64 = live ? A.target[r] : 0;
        const bool ok = y64 >= 0 && y64 < (int64_t)C;               // compared before any narrowing
        const int yc = ok ? (int)y64 : 0;
        if (live && sl < S) {
            const float *row = A.u.y + r * C;
            float z[NV], zn[NV];
            auto load = [&](int s, float (&v)[NV]) {
                if constexpr (FUSED) {
                    parts_sum<NV, 1, 8>(A.u.nparts, A.u.part_stride, A.u.classes, row + (int64_t)s * A.u.stride, 0, v);
                } else {
                    row_load<NV, 1>(row + (int64_t)s * A.u.stride, C, 0, 0, 0.f, v);
                }
            };
            load(sl, z);
            for (int s = sl; s < S; s += G) {
                if (!FUSED && s + G < S) load(s + G, zn);           // next sample's loads in flight meanwhile
                if constexpr (KIND == BNN_UNC_LOGITS) {
                    float m = z[0];
#pragma unroll
                    for (int i = 1; i < NV; ++i) if (i < C) m = fmaxf(m, z[i]);
                    float Z = 0.f, ty = 0.f;
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        if (i < C) {
                            const float t = (z[i] - m) * kLog2e;   // <= 0
                            const float e = __builtin_amdgcn_exp2f(t);
                            Z += e;
                            if (i == yc) ty = t;
                            z[i] = e;
                        }
                    }
                    const float inv = 1.0f / Z;                     // Z >= 1: the max contributes e = 1
                    const float lZ = __builtin_amdgcn_logf(Z);
                    eacc += (double)(lZ - ty);                      // as bnn_softmax_xent's row loss: ln(sum e) - (x[y] - max)
                    lse_add(L, ty - lZ);
#pragma unroll
                    for (int i = 0; i < NV; ++i) if (i < C) acc[i] += (double)(z[i] * inv);
                } else {
                    float zy = 0.f;
#pragma unroll
                    for (int i = 0; i < NV; ++i)
                        if (i < C) {
                            if (i == yc) zy = z[i];
                            acc[i] += (double)z[i];
                        }
                    eacc -= (double)__builtin_amdgcn_logf(zy + 1e-10f);
                }
                if (FUSED) {
                    if (s + G < S) load(s + G, z);
                } else {
#pragma unroll
                    for (int i = 0; i < NV; ++i) z[i] = zn[i];
                }
            }
        }
        // the G lanes of a row: a fixed xor tree (every lane of the group ends with the same bits)
        for (int o = 1; o < G; o <<= 1) {
#pragma unroll
            for (int i = 0; i < NV; ++i) if (i < C) acc[i] += __shfl_xor(acc[i], o, 64);
            eacc += __shfl_xor(eacc, o, 64);
            if constexpr (KIND == BNN_UNC_LOGITS) {
                const int M2 = __shfl_xor(L.M, o, 64);
                const double A2 = __shfl_xor(L.A, o, 64);
                lse_merge(L, M2, A2);
            }
        }
        if (live && sl == 0) {
            double tot = 0.0, brier = 0.0, m_y = 0.0;
            float conf = -__builtin_huge_valf();
            int pred = 0;
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (i < C) {
                    const double m = acc[i] / (double)S;
                    const float mf = (float)m;
                    if (A.u.mean) A.u.mean[r * C + i] = mf;
                    tot += total_term_bits<KIND>(m);
                    const double d = m - (i == yc ? 1.0 : 0.0);
                    brier += d * d;
                    if (i == yc) m_y = m;
                    if (mf > conf || i == 0) { conf = mf; pred = i; }      // the lowest class attaining the maximum
                }
            score_row_out<KIND>(A, r, ok, y64, L, eacc, m_y, brier, tot, conf, pred);
        }
    }
}

// ---------------------------------------------------------------------------------------------- wide: classes <= 4096
// (value, class) of the row's largest fp32 mean, the lowest class among equals; every thread returns the same pair.
template <int TPR>
__device__ __forceinline__ void row_argmax(float &v, int &c, float *slot_v, int *slot_c)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o, 64);
        const int c2 = __shfl_xor(c, o, 64);
        if (v2 > v || (v2 == v && c2 < c)) { v = v2; c = c2; }
    }
    if constexpr (TPR == 256) {
        if ((threadIdx.x & 63) == 0) { slot_v[threadIdx.x >> 6] = v; slot_c[threadIdx.x >> 6] = c; }
        __syncthreads();
        v = slot_v[0]; c = slot_c[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float v2 = slot_v[w];
            const int c2 = slot_c[w];
            if (v2 > v || (v2 == v && c2 < c)) { v = v2; c = c2; }
        }
    }
}

// k_unc_wide's split: TPR threads per row (64: a wave, four rows per workgroup; 256: the workgroup), NCH 4-class chunks per
// thread.  Every thread of a row reads the label's column itself (one address per row: a broadcast), so the per-sample label
// terms cost no reduction.  Unfused: held to 128 registers, so that four workgroups share a CU as k_unc_wide's do (the bandwidth
// shape's 1024 workgroups then run in one round on 256 CUs).
template <int KIND, bool FUSED, int TPR, int NCH>
__global__ __launch_bounds__(kUncThreads, FUSED ? 1 : 4) void k_score_wide(ScoreArgs A, uint32_t *advance_epoch, uint32_t advance_inc)
{
    constexpr int NV = 4 * NCH;
    constexpr int RPB = kUncThreads / TPR;
    __shared__ float red_m[2][4];
    __shared__ float red_f[2][8];
    __shared__ double red_d[8];
    __shared__ double red_y[8];
    __shared__ float red_av[4];
    __shared__ int red_ac[4];
    unc_advance(advance_epoch, advance_inc);
    const int nwork = (int)gridDim.x;
    const int t = (int)threadIdx.x % TPR;
    const int C = A.u.classes, S = A.u.nsamples;
    for (int64_t rb = blockIdx.x; rb * RPB < A.u.rows; rb += nwork) {
        const int64_t r = rb * RPB + (int)threadIdx.x / TPR;
        if (r >= A.u.rows) continue;                                // (TPR 64: a whole wave; TPR 256: the whole workgroup)
        const float *row = A.u.y + r * C;
        const int64_t y64 = A.target[r];
        const bool ok = y64 >= 0 && y64 < (int64_t)C;               // compared before any narrowing
        const int yc = ok ? (int)y64 : 0;
        double acc[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = 0.0;
        double eacc = 0.0;
        Lse L{kLseEmpty, 0.0};
        float z[NV], zn[NV], zy, zyn = 0.f;
        auto load = [&](int s, float (&v)[NV], float &vy) {
            const float *q = row + (int64_t)s * A.u.stride;
            if constexpr (FUSED) {
                parts_sum<NV, TPR, (NV >= 16 ? 2 : 32 / NV)>(A.u.nparts, A.u.part_stride, A.u.classes, q, t, v);
                float one[1];
                parts_sum<1, 1, 8>(A.u.nparts, A.u.part_stride, 1, q + yc, 0, one);
                vy = one[0];
            } else {
                vy = q[yc];
                // row_load's body, written out: through the helper <LOGITS, false, 64, 2> and <PROBS, false, 64, 2> come out with
                // other register counts (88 -> 87, 77 -> 76), and this launch's timings were taken on the code as it is
                if (A.u.vec) {
#pragma unroll
                    for (int k = 0; k < NCH; ++k) {
                        const int c = 4 * (t + k * TPR);
                        const float4 f = c < C ? *reinterpret_cast<const float4 *>(q + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                        v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        const int c = unc_col<TPR>(t, i);
                        v[i] = c < C ? q[c] : 0.f;
                    }
                }
            }
        };
        load(0, z, zy);
        for (int s = 0; s < S; ++s) {
            if (!FUSED && s + 1 < S) load(s + 1, zn, zyn);          // next sample's loads in flight meanwhile
            if constexpr (KIND == BNN_UNC_LOGITS) {
                const int par = s & 1;
                float m = -__builtin_huge_valf();
#pragma unroll
                for (int i = 0; i < NV; ++i) if (unc_col<TPR>(t, i) < C) m = fmaxf(m, z[i]);
                m = row_max<TPR>(m, red_m[par]);
                float Z = 0.f, unused = 0.f;
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    if (unc_col<TPR>(t, i) < C) {
                        const float e = __builtin_amdgcn_exp2f((z[i] - m) * kLog2e);
                        Z += e;
                        z[i] = e;
                    } else {
                        z[i] = 0.f;
                    }
                }
                row_sum2<TPR>(Z, unused, red_f[par]);
                const float inv = 1.0f / Z;
                const float lZ = __builtin_amdgcn_logf(Z), ty = (zy - m) * kLog2e;
                eacc += (double)(lZ - ty);
                lse_add(L, ty - lZ);
#pragma unroll
                for (int i = 0; i < NV; ++i) acc[i] += (double)(z[i] * inv);
            } else {
#pragma unroll
                for (int i = 0; i < NV; ++i) acc[i] += (double)z[i];   // (0 outside the row)
                eacc -= (double)__builtin_amdgcn_logf(zy + 1e-10f);
            }
            if (FUSED) {
                if (s + 1 < S) load(s + 1, z, zy);
            } else {
#pragma unroll
                for (int i = 0; i < NV; ++i) z[i] = zn[i];
                zy = zyn;
            }
        }
        double tot = 0.0, brier = 0.0, m_y = 0.0, unused = 0.0;
        float conf = -__builtin_huge_valf();
        int pred = 0x7FFFFFFF;
        float *mrow = A.u.mean ? A.u.mean + r * C : nullptr;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = 4 * (t + k * TPR);
            float mf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double m = acc[4 * k + j] / (double)S;
                mf[j] = (float)m;
                if (c + j < C) {
                    tot += total_term_bits<KIND>(m);
                    const double d = m - (c + j == yc ? 1.0 : 0.0);
                    brier += d * d;
                    if (c + j == yc) m_y = m;
                    if (mf[j] > conf || pred == 0x7FFFFFFF) { conf = mf[j]; pred = c + j; }     // ascending classes: the lowest
                }
            }
            if (mrow) {
                if (A.u.vec) {
                    if (c < C) *reinterpret_cast<float4 *>(mrow + c) = make_float4(mf[0], mf[1], mf[2], mf[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (c + j < C) mrow[c + j] = mf[j];
                }
            }
        }
        row_sum2<TPR>(tot, brier, red_d);
        if constexpr (KIND == BNN_UNC_PROBS) row_sum2<TPR>(m_y, unused, red_y);      // one thread holds it, the rest add 0
        row_argmax<TPR>(conf, pred, red_av, red_ac);
        if (t == 0) score_row_out<KIND>(A, r, ok, y64, L, eacc, m_y, brier, tot, conf, pred);
    }
}

// ---------------------------------------------------------------------------------------------- the accumulator
constexpr int kAccThreads = 1024;
constexpr int kAccUnroll = 4;
constexpr int kAccCopies = 16;              // private histograms: a confident test set puts every row of a wave into one bin

// One workgroup adds the launch's per-row words to `state` (layout: include/bnn_hip.h).  A thread takes rows tid, tid + 1024,
// ...; the loads of four of them are in flight before the first is used (the pass is latency-bound at evaluation batches).
// The histograms are integers in LDS, one copy per (lane & 15) with the copy as the fastest index: lanes that share a bin add
// to 16 banks, 4 deep, instead of 64 deep to one address.
__global__ __launch_bounds__(kAccThreads) void k_score_accumulate(const float *__restrict__ rec, int64_t rows, int conf_bins,
                                                                  int ent_bins, double *__restrict__ state)
{
    constexpr int NW = kAccThreads / 64;
    __shared__ unsigned cnt[4][kScoreMaxBins][kAccCopies];          // confidence: count, correct; entropy: count, correct
    __shared__ unsigned long long csum[kScoreMaxBins][kAccCopies];  // sum of confidence, 2^-31 units
    __shared__ double red[3][NW];
    for (int i = threadIdx.x; i < 4 * kScoreMaxBins * kAccCopies; i += kAccThreads) (&cnt[0][0][0])[i] = 0u;
    for (int i = threadIdx.x; i < kScoreMaxBins * kAccCopies; i += kAccThreads) (&csum[0][0])[i] = 0ull;
    __syncthreads();
    const uint32_t *bits = reinterpret_cast<const uint32_t *>(rec) + 4 * rows;
    const int cp = (int)threadIdx.x & (kAccCopies - 1);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int64_t i0 = threadIdx.x; i0 < rows; i0 += (int64_t)kAccThreads * kAccUnroll) {
        float v0[kAccUnroll], v1[kAccUnroll], v2[kAccUnroll], vc[kAccUnroll];
        uint32_t vb[kAccUnroll];
#pragma unroll
        for (int u = 0; u < kAccUnroll; ++u) {
            const int64_t i = i0 + (int64_t)u * kAccThreads;
            const bool in = i < rows;
            v0[u] = in ? rec[i] : 0.f;
            v1[u] = in ? rec[rows + i] : 0.f;
            v2[u] = in ? rec[2 * rows + i] : 0.f;
            vc[u] = in ? rec[3 * rows + i] : 0.f;
            vb[u] = in ? bits[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kAccUnroll; ++u) {
            if (i0 + (int64_t)u * kAccThreads >= rows) break;
            a0 += (double)v0[u];
            a1 += (double)v1[u];
            a2 += (double)v2[u];
            const uint32_t b = vb[u];
            const int cbin = (int)((b >> 1) & (kScoreMaxBins - 1)), ebin = (int)((b >> 16) & (kScoreMaxBins - 1));
            const unsigned correct = b & 1u;
            // a probability: clamped to [0, 2] (NaN: 0), exact in 2^-31 units from 2^-8 up, within 2^-32 below
            const float cl = vc[u] > 0.f ? (vc[u] < 2.f ? vc[u] : 2.f) : 0.f;
            atomicAdd(&cnt[0][cbin][cp], 1u);
            atomicAdd(&cnt[1][cbin][cp], correct);
            atomicAdd(&csum[cbin][cp], (unsigned long long)__double2ll_rn((double)cl * 2147483648.0));
            atomicAdd(&cnt[2][ebin][cp], 1u);
            atomicAdd(&cnt[3][ebin][cp], correct);
        }
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a0; red[1][threadIdx.x >> 6] = a1; red[2][threadIdx.x >> 6] = a2; }
    __syncthreads();
    const int b = (int)threadIdx.x;
    auto total = [&](int which, int bin) {
        unsigned t = 0u;
        for (int c = 0; c < kAccCopies; ++c) t += cnt[which][bin][c];
        return t;
    };
    if (b == 0) state[0] += (double)rows;
    if (b >= 1 && b < 4) {
        double t = 0.0;
        for (int w = 0; w < NW; ++w) t += red[b - 1][w];            // the waves' sums in wave order
        state[b] += t;
    }
    if (b == 64) {                                                  // (another wave than the sums')
        unsigned t = 0u;
        for (int k = 0; k < conf_bins; ++k) t += total(1, k);
        state[4] += (double)t;
    }
    if (b < conf_bins) {
        unsigned long long sc = 0ull;
        for (int c = 0; c < kAccCopies; ++c) sc += csum[b][c];
        double *p = state + 5 + 3 * b;
        p[0] += (double)total(0, b);
        p[1] += (double)sc * (1.0 / 2147483648.0);
        p[2] += (double)total(1, b);
    }
    if (b < ent_bins) {
        double *p = state + 5 + 3 * conf_bins + 2 * b;
        p[0] += (double)total(2, b);
        p[1] += (double)total(3, b);
    }
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int64_t bnn_mc_score_state_doubles(int conf_bins, int ent_bins)
{
    if (conf_bins < 1 || ent_bins < 1 || conf_bins > kScoreMaxBins || ent_bins > kScoreMaxBins) {
        set_error("bnn_mc_score_state_doubles: bins outside 1 .. %d", kScoreMaxBins);
        return 0;
    }
    return 5 + 3 * (int64_t)conf_bins + 2 * (int64_t)ent_bins;
}

int64_t bnn_mc_score_workspace_bytes(int64_t rows)
{
    if (rows < 1 || rows > 0x7FFFFFFF) { set_error("bnn_mc_score_workspace_bytes: bad extent"); return 0; }
    return 20 * rows;
}

int bnn_mc_score(const float *y, int64_t addend_stride, int nparts, int nsamples, int64_t rows, int classes, int kind,
                 const int64_t *target, float *mean, float *nll, float *expected_nll, float *brier, float *confidence,
                 int64_t *prediction, float *entropy, double *state, int conf_bins, int ent_bins, void *workspace,
                 uint32_t *advance_epoch, uint32_t advance_inc, void *stream)
{
    const TailNames N{"bnn_mc_score", "more than 4096 classes", "addend_stride below rows * classes"};
    const char *who = N.who;
    if (!y || !target) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    int rc = tail_check_extents(N, nparts, nsamples, rows, classes);
    if (rc) return rc;
    if (classes < 2) { set_error("%s: fewer than 2 classes (the entropy is normalised by ln C)", who); return BNN_E_RANGE; }
    if (kind != BNN_UNC_LOGITS && kind != BNN_UNC_PROBS) { set_error("%s: unknown kind %d", who, kind); return BNN_E_RANGE; }
    const int64_t naddends = (int64_t)nparts * nsamples;
    rc = tail_check_stride(N, naddends, addend_stride, rows, classes);
    if (rc) return rc;
    if (state) {
        if (conf_bins < 1 || ent_bins < 1) { set_error("%s: fewer than 1 bin", who); return BNN_E_SHAPE; }
        if (conf_bins > kScoreMaxBins || ent_bins > kScoreMaxBins) { set_error("%s: more than %d bins", who, kScoreMaxBins); return BNN_E_RANGE; }
        if (!workspace) { set_error("%s: a state needs the workspace", who); return BNN_E_NULL; }
        if ((reinterpret_cast<uintptr_t>(state) & 7u) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0) {
            set_error("%s: state not 8-byte or workspace not 4-byte aligned", who);
            return BNN_E_ALIGN;
        }
    }
    ScoreArgs A{};
    A.u = unc_args(y, addend_stride, nparts, nsamples, rows, classes, tail_vec(classes, naddends, addend_stride, {y, mean}),
                   mean, nullptr, nullptr, nullptr);
    A.target = target;
    A.nll = nll; A.expected_nll = expected_nll; A.brier = brier; A.confidence = confidence; A.entropy = entropy;
    A.prediction = prediction;
    A.rec = state ? reinterpret_cast<float *>(workspace) : nullptr;
    A.conf_bins = conf_bins;
    A.ent_bins = ent_bins;
    A.ent_scale = state ? (double)ent_bins / log((double)classes) : 0.0;
    hipStream_t st = (hipStream_t)stream;
    if (classes <= kUncNarrow) {
        const NarrowPlan P = narrow_plan(nsamples, rows, 0);
        kind_dispatch<BNN_UNC_LOGITS, BNN_UNC_PROBS>(kind, nparts > 1, [&](auto K, auto FU) {
            hipLaunchKernelGGL((k_score_narrow<K.value, FU.value>), P.grid, dim3(kUncThreads), 0, st, A, P.glog, P.rpb, advance_epoch,
                               advance_inc);
        });
    } else {
        const WidePlan P = wide_plan(classes, classes, rows, 0);
        kind_dispatch<BNN_UNC_LOGITS, BNN_UNC_PROBS>(kind, nparts > 1, [&](auto K, auto FU) {
            wide_dispatch(P, [&](auto T, auto NC) {
                hipLaunchKernelGGL((k_score_wide<K.value, FU.value, T.value, NC.value>), P.grid, dim3(kUncThreads), 0, st, A,
                                   advance_epoch, advance_inc);
            });
        });
    }
    rc = check_launch(who);
    if (rc || !state) return rc;
    hipLaunchKernelGGL(k_score_accumulate, dim3(1), dim3(kAccThreads), 0, st, reinterpret_cast<const float *>(workspace), rows,
                       conf_bins, ent_bins, state);
    return check_launch(who);
}

}  // extern "C"
