// bnn_uncertainty.hip -- predictive uncertainty of an MC forward in ONE launch: the predictive mean, its entropy (total),
// the expected per-sample entropy (aleatoric) and their difference (epistemic: the mutual information / BALD score).
// replaces  preds = model(x); agg = torch.stack(preds).mean(0); Entropy(dim=-1)(agg)   examples/MNIST/uncertainty.py:47-52
//
// Per row r of (rows, classes) and MC sample s:  z_s = sum over the parts of addend (part * S + s), in HeadPartials.logits()'s
// order; p_s = softmax(z_s) (LOGITS) or z_s as given (PROBS).  The per-sample entropies and p_s are accumulated in fp64 in a
// fixed sample order (lane-strided, then a fixed shuffle tree): no float atomics, bitwise reproducible.
//
// Two work splits, both with the per-sample terms in fp32 and one transcendental per element (v_exp_f32 for LOGITS -- the
// entropy comes from log-sum-exp, one v_log_f32 per (sample, row) -- v_log_f32 for PROBS):
//   narrow (classes <= 16: every classifier head here): a lane holds one (row, sample)'s classes in registers; G lanes share
//           a row (G = the next power of two >= S, <= 64), so a wave covers up to 64 / G rows and no per-sample reduction
//           crosses lanes; the G lanes' fp64 sums meet in a shuffle tree at the end.
//   wide   (classes <= 4096): a wave (classes <= 1024) or the workgroup (above) per row, a lane holding 4-class chunks c0 =
//           4 (lane + k TPR) (16-B loads); per sample one max and one (sum e, sum e t) reduction (__shfl_xor, + LDS across
//           the four waves), the next sample's loads in flight meanwhile.
// The optional tails are those of k_mc_sum_kl: block 0 bumps the device epoch, one extra workgroup runs KL's second pass.
#include "bnn_mc_parts.hpp"

namespace bnn {

// ---------------------------------------------------------------------------------------------- narrow: classes <= 16
// Lane = (row, sl): sl = lane & (G - 1) takes samples sl, sl + G, ...  FUSED: the logits are a fused head's partials.
// rpb rows per workgroup (<= 256 / G): a small grid leaves lanes idle so that its loads spread over more CUs.
template <int KIND, bool FUSED>
__global__ __launch_bounds__(kUncThreads) void k_unc_narrow(UncArgs A, int glog, int rpb, int has_kl, uint32_t *advance_epoch,
                                                            uint32_t advance_inc, KlFinal F, const double *__restrict__ partials,
                                                            float *__restrict__ kl_out)
{
    constexpr int NV = kUncNarrow;
    const int nwork = (int)gridDim.x - has_kl;
    if (unc_tails(nwork, advance_epoch, advance_inc, F, partials, kl_out)) return;
    const int G = 1 << glog, sl = (int)threadIdx.x & (G - 1);
    const int C = A.classes, S = A.nsamples;
    const int lr = (int)threadIdx.x >> glog;
    for (int64_t rb = blockIdx.x; rb * rpb < A.rows; rb += nwork) {
        const int64_t r = rb * rpb + lr;
        const bool live = lr < rpb && r < A.rows;
        double acc[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = 0.0;
        double hacc = 0.0;                                          // sum of per-sample entropies, bits
        if (live && sl < S) {
            const float *row = A.y + r * C;
            float z[NV], zn[NV];
            auto load = [&](int s, float (&v)[NV]) {
                if constexpr (FUSED) {
                    parts_sum<NV, 1, 8>(A.nparts, A.part_stride, A.classes, row + (int64_t)s * A.stride, 0, v);
                } else {
#pragma unroll
                    for (int i = 0; i < NV; ++i) v[i] = i < C ? row[(int64_t)s * A.stride + i] : 0.f;
                }
            };
            load(sl, z);
            for (int s = sl; s < S; s += G) {
                if (!FUSED && s + G < S) load(s + G, zn);           // next sample's loads in flight meanwhile
                if constexpr (KIND == BNN_UNC_LOGITS) {
                    float m = z[0];
#pragma unroll
                    for (int i = 1; i < NV; ++i) if (i < C) m = fmaxf(m, z[i]);
                    float Z = 0.f, W = 0.f;
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        if (i < C) {
                            const float t = (z[i] - m) * kLog2e;   // <= 0
                            const float e = __builtin_amdgcn_exp2f(t);
                            Z += e;
                            W = __builtin_fmaf(e, t, W);
                            z[i] = e;
                        }
                    }
                    const float inv = 1.0f / Z;                     // Z >= 1: the max contributes e = 1
                    hacc += (double)(__builtin_amdgcn_logf(Z) - W * inv);   // H = log2 Z - sum p t, bits
#pragma unroll
                    for (int i = 0; i < NV; ++i) if (i < C) acc[i] += (double)(z[i] * inv);
                } else {
                    float h = 0.f;
#pragma unroll
                    for (int i = 0; i < NV; ++i)
                        if (i < C) {
                            h = __builtin_fmaf(z[i], __builtin_amdgcn_logf(z[i] + 1e-10f), h);
                            acc[i] += (double)z[i];
                        }
                    hacc -= (double)h;
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
            hacc += __shfl_xor(hacc, o, 64);
        }
        if (live && sl == 0) {
            double tot = 0.0;
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (i < C) {
                    const double m = acc[i] / (double)S;
                    A.mean[r * C + i] = (float)m;
                    tot += total_term_bits<KIND>(m);
                }
            tot *= kLn2;
            const double ale = hacc * kLn2 / (double)S;
            A.total[r] = (float)tot;
            A.aleatoric[r] = (float)ale;
            A.epistemic[r] = (float)(tot - ale);
        }
    }
}

// ---------------------------------------------------------------------------------------------- wide: classes <= 4096
// TPR threads per row (64: a wave, four rows per workgroup; 256: the workgroup), NCH 4-class chunks per thread.
template <int KIND, bool FUSED, int TPR, int NCH>
__global__ __launch_bounds__(kUncThreads) void k_unc_wide(UncArgs A, int has_kl, uint32_t *advance_epoch, uint32_t advance_inc,
                                                          KlFinal F, const double *__restrict__ partials, float *__restrict__ kl_out)
{
    constexpr int NV = 4 * NCH;
    constexpr int RPB = kUncThreads / TPR;
    __shared__ float red_m[2][4];
    __shared__ float red_f[2][8];
    __shared__ double red_d[8];
    const int nwork = (int)gridDim.x - has_kl;
    if (unc_tails(nwork, advance_epoch, advance_inc, F, partials, kl_out)) return;
    const int t = (int)threadIdx.x % TPR;
    const int C = A.classes, S = A.nsamples;
    for (int64_t rb = blockIdx.x; rb * RPB < A.rows; rb += nwork) {
        const int64_t r = rb * RPB + (int)threadIdx.x / TPR;
        if (r >= A.rows) continue;                                  // (TPR 64: a whole wave; TPR 256: the whole workgroup)
        const float *row = A.y + r * C;
        double acc[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = 0.0;
        double hacc = 0.0;
        float z[NV], zn[NV];
        auto load = [&](int s, float (&v)[NV]) {
            const float *q = row + (int64_t)s * A.stride;
            if constexpr (FUSED) {
                parts_sum<NV, TPR, (NV >= 16 ? 2 : 32 / NV)>(A.nparts, A.part_stride, A.classes, q, t, v);
            } else if (A.vec) {
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
        };
        load(0, z);
        for (int s = 0; s < S; ++s) {
            if (!FUSED && s + 1 < S) load(s + 1, zn);               // next sample's loads in flight meanwhile
            const int par = s & 1;
            if constexpr (KIND == BNN_UNC_LOGITS) {
                float m = -__builtin_huge_valf();
#pragma unroll
                for (int i = 0; i < NV; ++i) if (unc_col<TPR>(t, i) < C) m = fmaxf(m, z[i]);
                m = row_max<TPR>(m, red_m[par]);
                float Z = 0.f, W = 0.f;
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    if (unc_col<TPR>(t, i) < C) {
                        const float tt = (z[i] - m) * kLog2e;
                        const float e = __builtin_amdgcn_exp2f(tt);
                        Z += e;
                        W = __builtin_fmaf(e, tt, W);
                        z[i] = e;
                    } else {
                        z[i] = 0.f;
                    }
                }
                row_sum2<TPR>(Z, W, red_f[par]);
                const float inv = 1.0f / Z;
                hacc += (double)(__builtin_amdgcn_logf(Z) - W * inv);
#pragma unroll
                for (int i = 0; i < NV; ++i) acc[i] += (double)(z[i] * inv);
            } else {
                float h = 0.f, unused = 0.f;
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    if (unc_col<TPR>(t, i) < C) h = __builtin_fmaf(z[i], __builtin_amdgcn_logf(z[i] + 1e-10f), h);
                    acc[i] += (double)z[i];                         // (0 outside the row)
                }
                row_sum2<TPR>(h, unused, red_f[par]);
                hacc -= (double)h;
            }
            if (FUSED) {
                if (s + 1 < S) load(s + 1, z);
            } else {
#pragma unroll
                for (int i = 0; i < NV; ++i) z[i] = zn[i];
            }
        }
        double tot = 0.0, unused = 0.0;
        float *mrow = A.mean + r * C;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = 4 * (t + k * TPR);
            float mf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double m = acc[4 * k + j] / (double)S;
                mf[j] = (float)m;
                if (c + j < C) tot += total_term_bits<KIND>(m);
            }
            if (A.vec) {
                if (c < C) *reinterpret_cast<float4 *>(mrow + c) = make_float4(mf[0], mf[1], mf[2], mf[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (c + j < C) mrow[c + j] = mf[j];
            }
        }
        row_sum2<TPR>(tot, unused, red_d);
        if (t == 0) {
            tot *= kLn2;
            const double ale = hacc * kLn2 / (double)S;
            A.total[r] = (float)tot;
            A.aleatoric[r] = (float)ale;
            A.epistemic[r] = (float)(tot - ale);
        }
    }
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_mc_uncertainty(const float *y, int64_t addend_stride, int nparts, int nsamples, int64_t rows, int classes, int kind,
                       float *mean, float *total, float *aleatoric, float *epistemic, uint32_t *advance_epoch,
                       uint32_t advance_inc, const bnn_kl_tensor_t *kl_tensors, int kl_ntensors, float kl_n_batches,
                       float *kl_out, const void *kl_workspace, void *stream)
{
    if (!y || !mean || !total || !aleatoric || !epistemic) { set_error("bnn_mc_uncertainty: NULL pointer"); return BNN_E_NULL; }
    if (nparts < 1 || nsamples < 1 || rows < 1 || classes < 1) { set_error("bnn_mc_uncertainty: bad extent"); return BNN_E_SHAPE; }
    if (nsamples > 65536) { set_error("bnn_mc_uncertainty: more than 65536 samples"); return BNN_E_RANGE; }
    if (classes > 4096) { set_error("bnn_mc_uncertainty: more than 4096 classes"); return BNN_E_RANGE; }
    if (rows > 0x7FFFFFFF) { set_error("bnn_mc_uncertainty: more than 2^31 - 1 rows"); return BNN_E_RANGE; }
    if (kind != BNN_UNC_LOGITS && kind != BNN_UNC_PROBS) { set_error("bnn_mc_uncertainty: unknown kind %d", kind); return BNN_E_RANGE; }
    if ((int64_t)nparts * nsamples > 1 && addend_stride < rows * classes) {
        set_error("bnn_mc_uncertainty: addend_stride below rows * classes");
        return BNN_E_SHAPE;
    }
    KlFinal F{};
    const int has_kl = kl_tensors != nullptr;
    if (has_kl) {
        const int rc = kl_final_plan(kl_tensors, kl_ntensors, kl_n_batches, kl_out, kl_workspace, F, "bnn_mc_uncertainty");
        if (rc) return rc;
    }
    UncArgs A{};
    A.y = y;
    A.stride = addend_stride;
    A.part_stride = (int64_t)nsamples * addend_stride;
    A.rows = rows;
    A.nparts = nparts;
    A.nsamples = nsamples;
    A.classes = classes;
    A.vec = classes % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15u) == 0 && (reinterpret_cast<uintptr_t>(mean) & 15u) == 0 &&
            (addend_stride % 4 == 0 || (int64_t)nparts * nsamples == 1);
    A.mean = mean; A.total = total; A.aleatoric = aleatoric; A.epistemic = epistemic;
    const bool fused = nparts > 1;
    const double *ws = reinterpret_cast<const double *>(kl_workspace);
    hipStream_t st = (hipStream_t)stream;
    auto grid = [&](int64_t work) { return dim3((unsigned)((work < kUncMaxBlocks ? work : kUncMaxBlocks) + has_kl)); };
    if (classes <= kUncNarrow) {
        int glog = 0;
        while ((1 << glog) < nsamples && glog < 6) ++glog;
        // a workgroup's four waves issue their scattered loads through one CU: below 256 workgroups, fewer rows per workgroup
        // (the step's tail, 512 rows x 8 samples: 16 workgroups of 32 rows -> 256 of 2)
        int rpb = kUncThreads >> glog;
        while (rpb > 1 && (rows + rpb - 1) / rpb < 256) rpb >>= 1;
        const dim3 g = grid((rows + rpb - 1) / rpb);
#define UNC_NARROW(K, FU) hipLaunchKernelGGL((k_unc_narrow<K, FU>), g, dim3(kUncThreads), 0, st, A, glog, rpb, has_kl, advance_epoch, \
                                             advance_inc, F, ws, kl_out)
        if (kind == BNN_UNC_LOGITS) { if (fused) UNC_NARROW(BNN_UNC_LOGITS, true); else UNC_NARROW(BNN_UNC_LOGITS, false); }
        else { if (fused) UNC_NARROW(BNN_UNC_PROBS, true); else UNC_NARROW(BNN_UNC_PROBS, false); }
#undef UNC_NARROW
        return check_launch("bnn_mc_uncertainty");
    }
    // wide: a wave per row up to 1024 classes (<= 16 per lane), the workgroup per row above
    const int tpr = classes <= 1024 ? 64 : 256;
    const int nch = (classes + 4 * tpr - 1) / (4 * tpr);
    const dim3 g = grid((rows + kUncThreads / tpr - 1) / (kUncThreads / tpr));
#define UNC_WIDE(K, FU, T, N) hipLaunchKernelGGL((k_unc_wide<K, FU, T, N>), g, dim3(kUncThreads), 0, st, A, has_kl, advance_epoch, \
                                                 advance_inc, F, ws, kl_out)
#define UNC_WIDE_K(K, FU)                                                            \
    do {                                                                             \
        if (tpr == 64) {                                                             \
            if (nch == 1) UNC_WIDE(K, FU, 64, 1);                                    \
            else if (nch == 2) UNC_WIDE(K, FU, 64, 2);                               \
            else UNC_WIDE(K, FU, 64, 4);                                             \
        } else {                                                                     \
            if (nch <= 2) UNC_WIDE(K, FU, 256, 2);                                   \
            else UNC_WIDE(K, FU, 256, 4);                                            \
        }                                                                            \
    } while (0)
    if (kind == BNN_UNC_LOGITS) { if (fused) UNC_WIDE_K(BNN_UNC_LOGITS, true); else UNC_WIDE_K(BNN_UNC_LOGITS, false); }
    else { if (fused) UNC_WIDE_K(BNN_UNC_PROBS, true); else UNC_WIDE_K(BNN_UNC_PROBS, false); }
#undef UNC_WIDE_K
#undef UNC_WIDE
    return check_launch("bnn_mc_uncertainty");
}

}  // extern "C"
