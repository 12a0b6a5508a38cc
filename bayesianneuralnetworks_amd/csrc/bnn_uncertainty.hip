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
    const NarrowLane L(glog, rpb);
    const int G = L.G, sl = L.sl;
    const int C = A.classes, S = A.nsamples;
    for (int64_t rb = blockIdx.x; rb * rpb < A.rows; rb += nwork) {
        const int64_t r = rb * rpb + L.lr;
        const bool live = L.live(r, A.rows);
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
                    row_load<NV, 1>(row + (int64_t)s * A.stride, C, 0, 0, 0.f, v);
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
                // row_load's body, written out: through the helper <LOGITS, false, 256, 2> and <PROBS, false, 64, 2> come out with
                // other register counts (74 -> 70, 60 -> 59), and this launch's timings were taken on the code as it is
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
    const TailNames N{"bnn_mc_uncertainty", "more than 4096 classes", "addend_stride below rows * classes"};
    if (!y || !mean || !total || !aleatoric || !epistemic) { set_error("%s: NULL pointer", N.who); return BNN_E_NULL; }
    int rc = tail_check_extents(N, nparts, nsamples, rows, classes);
    if (rc) return rc;
    if (kind != BNN_UNC_LOGITS && kind != BNN_UNC_PROBS) { set_error("%s: unknown kind %d", N.who, kind); return BNN_E_RANGE; }
    const int64_t naddends = (int64_t)nparts * nsamples;
    rc = tail_check_stride(N, naddends, addend_stride, rows, classes);
    if (rc) return rc;
    KlFinal F{};
    const int has_kl = kl_tensors != nullptr;
    if (has_kl) {
        rc = kl_final_plan(kl_tensors, kl_ntensors, kl_n_batches, kl_out, kl_workspace, F, N.who);
        if (rc) return rc;
    }
    const UncArgs A = unc_args(y, addend_stride, nparts, nsamples, rows, classes, tail_vec(classes, naddends, addend_stride, {y, mean}),
                               mean, total, aleatoric, epistemic);
    const double *ws = reinterpret_cast<const double *>(kl_workspace);
    hipStream_t st = (hipStream_t)stream;
    if (classes <= kUncNarrow) {
        const NarrowPlan P = narrow_plan(nsamples, rows, has_kl);
        kind_dispatch<BNN_UNC_LOGITS, BNN_UNC_PROBS>(kind, nparts > 1, [&](auto K, auto FU) {
            hipLaunchKernelGGL((k_unc_narrow<K.value, FU.value>), P.grid, dim3(kUncThreads), 0, st, A, P.glog, P.rpb, has_kl,
                               advance_epoch, advance_inc, F, ws, kl_out);
        });
        return check_launch(N.who);
    }
    const WidePlan P = wide_plan(classes, classes, rows, has_kl);
    kind_dispatch<BNN_UNC_LOGITS, BNN_UNC_PROBS>(kind, nparts > 1, [&](auto K, auto FU) {
        wide_dispatch(P, [&](auto T, auto NC) {
            hipLaunchKernelGGL((k_unc_wide<K.value, FU.value, T.value, NC.value>), P.grid, dim3(kUncThreads), 0, st, A, has_kl,
                               advance_epoch, advance_inc, F, ws, kl_out);
        });
    });
    return check_launch(N.who);
}

}  // extern "C"
