// bnn_regression.hip -- the tail of a REGRESSION MC pass, as bnn_uncertainty.hip is the tail of a classification one.
//
// bnn_mc_regression: the moments of the equal-weight mixture of the S per-sample predictives in ONE launch (law of total
// variance).  replaces  the mean / aleatoric / epistemic bands of examples/Simple/uncertainty.py over torch.stack(preds)
// Per row and predicted quantity d, with m_s the per-sample mean and v_s the per-sample variance (0 for VALUES, exp of the
// second half for MEAN_LOGVAR -- one v_exp_f32 --, the second half as given for MEAN_VAR):
//   mean = (1/S) sum m_s,  aleatoric = (1/S) sum v_s,  epistemic = (1/S) sum (m_s - mean)^2,  total = aleatoric + epistemic.
// The variance of the means is taken on d_s = m_s - m_0 (sample 0's value), fp64: mean = m_0 + sum d / S, epistemic =
// sum d^2 / S - (sum d / S)^2.  On the raw values that difference cancels |m|^2 / var digits (fp32 inputs near 4096 with spread
// 1e-2: wrong in the 4th - 5th digit even in fp64); shifted, it cancels only (m_0 - mean)^2 / var, a few units for any sample
// drawn from the same distribution as the rest.  S = 1 gives d = 0: exactly 0.  A negative rounding residue is clamped to 0.
// All sums over samples are fp64 in a fixed order (lane-strided, then a fixed shuffle tree): no float atomics, bitwise
// reproducible.  Two work splits, with the launch shapes of bnn_mc_parts.hpp:
//   narrow (width <= 16: every regression head here): a lane holds one (row, sample)'s values in registers; G lanes share a row
//           (G = the next power of two >= S, <= 64); sample 0's means reach the group by one shuffle per quantity, the G lanes'
//           fp64 sums meet in a shuffle tree at the end.
//   wide   (width <= 4096): a wave (width <= 1024) or the workgroup (above) per row, a lane holding 4-quantity chunks (16-B
//           loads) over ALL samples in sample order, the next sample's loads in flight meanwhile -- no reduction crosses lanes.
// The optional tails are those of k_mc_sum_kl: block 0 bumps the device epoch, one extra workgroup runs KL's second pass.
//
// bnn_gaussian_nll: the heteroscedastic Gaussian likelihood that trains a (mean, log-variance) head, loss and gradient in one
// pass over y, as bnn_softmax_xent is for cross-entropy.
#include "bnn_mc_parts.hpp"

namespace bnn {

// ---------------------------------------------------------------------------------------------- narrow: width <= 16
// Lane = (row, sl): sl = lane & (G - 1) takes samples sl, sl + G, ...  A.classes is the row width, D the predicted quantities
// (width, or width / 2 with the variances' half D columns behind the means').  FUSED: y is a fused head's partials.
template <int KIND, bool FUSED>
__global__ __launch_bounds__(kUncThreads) void k_reg_narrow(UncArgs A, int D, int glog, int rpb, int has_kl, uint32_t *advance_epoch,
                                                            uint32_t advance_inc, KlFinal F, const double *__restrict__ partials,
                                                            float *__restrict__ kl_out)
{
    constexpr bool VAR = KIND != BNN_REG_VALUES;
    constexpr int NV = VAR ? kUncNarrow / 2 : kUncNarrow;
    const int nwork = (int)gridDim.x - has_kl;
    if (unc_tails(nwork, advance_epoch, advance_inc, F, partials, kl_out)) return;
    const NarrowLane L(glog, rpb);
    const int G = L.G, sl = L.sl;
    const int W = A.classes, S = A.nsamples;
    const double inv_S = 1.0 / (double)S;
    for (int64_t rb = blockIdx.x; rb * rpb < A.rows; rb += nwork) {
        const int64_t r = rb * rpb + L.lr;
        const bool live = L.live(r, A.rows);
        const bool work = live && sl < S;
        const float *row = A.y + r * W;
        float m[NV], v[NV], mn[NV], vn[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) m[i] = v[i] = mn[i] = vn[i] = 0.f;
        auto load = [&](int s, float (&a)[NV], float (&b)[NV]) {
            const float *q = row + (int64_t)s * A.stride;
            if constexpr (FUSED) {
                parts_sum<NV, 1, 8>(A.nparts, A.part_stride, D, q, 0, a);
                if constexpr (VAR) parts_sum<NV, 1, 8>(A.nparts, A.part_stride, D, q + D, 0, b);
            } else {
                row_load<NV, 1>(q, D, 0, 0, 0.f, a);
                if constexpr (VAR) row_load<NV, 1>(q + D, D, 0, 0, 0.f, b);
            }
        };
        if (work) load(sl, m, v);
        // sample 0's means: lane sl == 0 of the group holds them (S >= 1); every lane of the wave takes part in the shuffle
        float ref[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) ref[i] = __shfl(m[i], L.lead, 64);
        double sd[NV], sd2[NV], sv[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) sd[i] = sd2[i] = sv[i] = 0.0;
        if (work) {
            for (int s = sl; s < S; s += G) {
                if (!FUSED && s + G < S) load(s + G, mn, vn);       // next sample's loads in flight meanwhile
#pragma unroll
                for (int i = 0; i < NV; ++i)
                    if (i < D) reg_acc<KIND>(m[i], ref[i], v[i], sd[i], sd2[i], sv[i]);
                if (FUSED) {
                    if (s + G < S) load(s + G, m, v);
                } else {
#pragma unroll
                    for (int i = 0; i < NV; ++i) { m[i] = mn[i]; v[i] = vn[i]; }
                }
            }
        }
        // the G lanes of a row: a fixed xor tree (every lane of the group ends with the same bits)
        for (int o = 1; o < G; o <<= 1) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (i < D) {
                    sd[i] += __shfl_xor(sd[i], o, 64);
                    sd2[i] += __shfl_xor(sd2[i], o, 64);
                    if constexpr (VAR) sv[i] += __shfl_xor(sv[i], o, 64);
                }
        }
        if (live && sl == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (i < D) store_moments(A, r * D + i, reg_finish(ref[i], sd[i], sd2[i], sv[i], inv_S));
        }
    }
}

// ---------------------------------------------------------------------------------------------- wide: width <= 4096
// TPR threads per row (64: a wave, four rows per workgroup; 256: the workgroup), NCH 4-quantity chunks per thread: chunk k of
// thread t is quantities 4 (t + k TPR) .. + 3 -- their means at that column, their variances D columns further on.
template <int KIND, bool FUSED, int TPR, int NCH>
__global__ __launch_bounds__(kUncThreads) void k_reg_wide(UncArgs A, int D, int has_kl, uint32_t *advance_epoch, uint32_t advance_inc,
                                                          KlFinal F, const double *__restrict__ partials, float *__restrict__ kl_out)
{
    constexpr bool VAR = KIND != BNN_REG_VALUES;
    constexpr int NV = 4 * NCH;
    constexpr int RPB = kUncThreads / TPR;
    const int nwork = (int)gridDim.x - has_kl;
    if (unc_tails(nwork, advance_epoch, advance_inc, F, partials, kl_out)) return;
    const int t = (int)threadIdx.x % TPR;
    const int W = A.classes, S = A.nsamples;
    const double inv_S = 1.0 / (double)S;
    for (int64_t rb = blockIdx.x; rb * RPB < A.rows; rb += nwork) {
        const int64_t r = rb * RPB + (int)threadIdx.x / TPR;
        if (r >= A.rows) continue;
        const float *row = A.y + r * W;
        float m[NV], v[NV], mn[NV], vn[NV], ref[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = vn[i] = 0.f;
        auto load = [&](int s, float (&a)[NV], float (&b)[NV]) {
            const float *q = row + (int64_t)s * A.stride;
            if constexpr (FUSED) {
                parts_sum<NV, TPR, (NV >= 16 ? 2 : 32 / NV)>(A.nparts, A.part_stride, D, q, t, a);
                if constexpr (VAR) parts_sum<NV, TPR, (NV >= 16 ? 2 : 32 / NV)>(A.nparts, A.part_stride, D, q + D, t, b);
            } else {
                row_load<NV, TPR>(q, D, A.vec, t, 0.f, a);
                if constexpr (VAR) row_load<NV, TPR>(q + D, D, A.vec, t, 0.f, b);
            }
        };
        double sd[NV], sd2[NV], sv[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) sd[i] = sd2[i] = sv[i] = 0.0;
        load(0, m, v);
#pragma unroll
        for (int i = 0; i < NV; ++i) ref[i] = m[i];
        for (int s = 0; s < S; ++s) {
            if (!FUSED && s + 1 < S) load(s + 1, mn, vn);           // next sample's loads in flight meanwhile
#pragma unroll
            for (int i = 0; i < NV; ++i) reg_acc<KIND>(m[i], ref[i], v[i], sd[i], sd2[i], sv[i]);     // (0 outside the row)
            if (FUSED) {
                if (s + 1 < S) load(s + 1, m, v);
            } else {
#pragma unroll
                for (int i = 0; i < NV; ++i) { m[i] = mn[i]; v[i] = vn[i]; }
            }
        }
        const int64_t o0 = r * D;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            Moments o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = reg_finish(ref[4 * k + j], sd[4 * k + j], sd2[4 * k + j], sv[4 * k + j], inv_S);
            store_moments4(A, o0, 4 * (t + k * TPR), D, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------- Gaussian NLL
// y (S, rows, 2 D): means then log-variances; target (rows, D), read once per sample (from L2 after the first).  With r = t - m,
// s the log-variance, N = S rows D:  term = 0.5 (s + r^2 e^-s);  g_m = -r e^-s / N;  g_s = 0.5 (1 - r^2 e^-s) / N.
// A workgroup is (TR rows) x (TD lanes along D), TD = 1 << tdlog; blockIdx.y strides the samples, blockIdx.x the row tiles.
// Terms in fp32, each thread's sum and the workgroup's in fp64, one partial per workgroup; k_nll_final adds them in index order.
constexpr int kNllThreads = 256;
constexpr int kNllMaxX = 2048;              // row tiles per launch (grid-stride above)
constexpr int kNllMaxBlocks = 8192;         // workgroups per launch = fp64 partials in the workspace

__global__ __launch_bounds__(kNllThreads) void k_nll(const float *__restrict__ y, const float *__restrict__ target,
                                                     float *__restrict__ gy, double *__restrict__ partial, int S, int64_t rows,
                                                     int D, int tdlog, float inv_N)
{
    __shared__ double red[kNllThreads / 64];
    const int TD = 1 << tdlog, TR = kNllThreads >> tdlog;
    const int td = (int)threadIdx.x & (TD - 1), tr = (int)threadIdx.x >> tdlog;
    double acc = 0.0;
    for (int s = blockIdx.y; s < S; s += gridDim.y) {
        for (int64_t r = (int64_t)blockIdx.x * TR + tr; r < rows; r += (int64_t)gridDim.x * TR) {
            const int64_t base = ((int64_t)s * rows + r) * (2 * (int64_t)D);
            const float *yr = y + base;
            const float *tg = target + r * D;
            float a = 0.f;
            for (int d = td; d < D; d += TD) {
                const float lv = yr[D + d];
                const float res = tg[d] - yr[d];
                const float w = res * __builtin_amdgcn_exp2f(-lv * kLog2e);
                const float q = res * w;                            // r^2 e^-s
                a += 0.5f * (lv + q);
                if (gy) {
                    gy[base + d] = -w * inv_N;
                    gy[base + D + d] = (0.5f - 0.5f * q) * inv_N;
                }
            }
            acc += (double)a;
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kNllThreads) void k_nll_final(const double *__restrict__ partial, int n, double inv_N, float *__restrict__ loss)
{
    __shared__ double red[kNllThreads / 64];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += kNllThreads) a += partial[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_N);
}

struct NllPlan { int tdlog, gx, gy; };

// the launch shape: a function of (nsamples, rows, width) alone, so that the workspace query and the launch agree
static NllPlan nll_plan(int64_t nsamples, int64_t rows, int width)
{
    NllPlan P{};
    const int D = width / 2;
    while ((1 << P.tdlog) < D && P.tdlog < 8) ++P.tdlog;
    const int TR = kNllThreads >> P.tdlog;
    const int64_t tiles = (rows + TR - 1) / TR;
    P.gx = (int)(tiles < kNllMaxX ? tiles : kNllMaxX);
    const int64_t room = kNllMaxBlocks / P.gx;
    P.gy = (int)(nsamples < room ? nsamples : room);
    return P;
}

static int nll_check(const char *who, int64_t nsamples, int64_t rows, int width)
{
    if (nsamples < 1 || rows < 1 || width < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (nsamples > 65536) { set_error("%s: more than 65536 samples", who); return BNN_E_RANGE; }
    if (width > 4096) { set_error("%s: width above 4096", who); return BNN_E_RANGE; }
    if (rows > 0x7FFFFFFF) { set_error("%s: more than 2^31 - 1 rows", who); return BNN_E_RANGE; }
    if (width % 2) { set_error("%s: odd width %d (means then log-variances)", who, width); return BNN_E_SHAPE; }
    return BNN_OK;
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_mc_regression(const float *y, int64_t addend_stride, int nparts, int nsamples, int64_t rows, int width, int kind,
                      float *mean, float *total, float *aleatoric, float *epistemic, uint32_t *advance_epoch,
                      uint32_t advance_inc, const bnn_kl_tensor_t *kl_tensors, int kl_ntensors, float kl_n_batches,
                      float *kl_out, const void *kl_workspace, void *stream)
{
    const TailNames N{"bnn_mc_regression", "width above 4096", "addend_stride below rows * width"};
    if (!y || !mean || !total || !aleatoric || !epistemic) { set_error("%s: NULL pointer", N.who); return BNN_E_NULL; }
    int rc = tail_check_extents(N, nparts, nsamples, rows, width);
    if (rc) return rc;
    if (kind != BNN_REG_VALUES && kind != BNN_REG_MEAN_LOGVAR && kind != BNN_REG_MEAN_VAR) {
        set_error("%s: unknown kind %d", N.who, kind);
        return BNN_E_RANGE;
    }
    if (kind != BNN_REG_VALUES && width % 2) { set_error("%s: odd width %d for a (mean, variance) layout", N.who, width); return BNN_E_SHAPE; }
    const int64_t naddends = (int64_t)nparts * nsamples;
    rc = tail_check_stride(N, naddends, addend_stride, rows, width);
    if (rc) return rc;
    KlFinal F{};
    const int has_kl = kl_tensors != nullptr;
    if (has_kl) {
        rc = kl_final_plan(kl_tensors, kl_ntensors, kl_n_batches, kl_out, kl_workspace, F, N.who);
        if (rc) return rc;
    }
    const int D = kind == BNN_REG_VALUES ? width : width / 2;
    // 16-B loads of both halves and 16-B stores of every output: D % 4 == 0 (then width % 4 == 0 as well)
    const int vec = tail_vec(D, naddends, addend_stride, {y, mean, total, aleatoric, epistemic});
    const UncArgs A = unc_args(y, addend_stride, nparts, nsamples, rows, width, vec, mean, total, aleatoric, epistemic);
    const double *ws = reinterpret_cast<const double *>(kl_workspace);
    hipStream_t st = (hipStream_t)stream;
    if (width <= kUncNarrow) {
        const NarrowPlan P = narrow_plan(nsamples, rows, has_kl);
        kind_dispatch<BNN_REG_VALUES, BNN_REG_MEAN_LOGVAR, BNN_REG_MEAN_VAR>(kind, nparts > 1, [&](auto K, auto FU) {
            hipLaunchKernelGGL((k_reg_narrow<K.value, FU.value>), P.grid, dim3(kUncThreads), 0, st, A, D, P.glog, P.rpb, has_kl,
                               advance_epoch, advance_inc, F, ws, kl_out);
        });
        return check_launch(N.who);
    }
    const WidePlan P = wide_plan(width, D, rows, has_kl);
    kind_dispatch<BNN_REG_VALUES, BNN_REG_MEAN_LOGVAR, BNN_REG_MEAN_VAR>(kind, nparts > 1, [&](auto K, auto FU) {
        // VALUES: D = width, up to 4 chunks per thread; the (mean, variance) layouts: D = width / 2, at most 2
        wide_dispatch<(K.value == BNN_REG_VALUES ? 4 : 2)>(P, [&](auto T, auto NC) {
            hipLaunchKernelGGL((k_reg_wide<K.value, FU.value, T.value, NC.value>), P.grid, dim3(kUncThreads), 0, st, A, D, has_kl,
                               advance_epoch, advance_inc, F, ws, kl_out);
        });
    });
    return check_launch(N.who);
}

int64_t bnn_gaussian_nll_workspace_bytes(int64_t nsamples, int64_t rows, int width)
{
    if (nll_check("bnn_gaussian_nll_workspace_bytes", nsamples, rows, width)) return 0;
    const NllPlan P = nll_plan(nsamples, rows, width);
    return 8 * (int64_t)P.gx * P.gy;
}

int bnn_gaussian_nll(const float *y, int nsamples, int64_t rows, int width, const float *target, float *loss, float *g_y,
                     void *workspace, void *stream)
{
    const char *who = "bnn_gaussian_nll";
    if (!y || !target || !loss || !workspace) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    const int rc = nll_check(who, nsamples, rows, width);
    if (rc) return rc;
    const NllPlan P = nll_plan(nsamples, rows, width);
    const int D = width / 2;
    const double inv_N = 1.0 / ((double)nsamples * (double)rows * (double)D);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nll, dim3((unsigned)P.gx, (unsigned)P.gy), dim3(kNllThreads), 0, st, y, target, g_y,
                       reinterpret_cast<double *>(workspace), nsamples, rows, D, P.tdlog, (float)inv_N);
    const int rc2 = check_launch(who);
    if (rc2) return rc2;
    hipLaunchKernelGGL(k_nll_final, dim3(1), dim3(kNllThreads), 0, st, reinterpret_cast<const double *>(workspace), P.gx * P.gy,
                       inv_N, loss);
    return check_launch(who);
}

}  // extern "C"
