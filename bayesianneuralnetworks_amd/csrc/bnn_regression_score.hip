// bnn_regression_score.hip -- a REGRESSION MC forward scored against its targets in ONE launch (K15), as bnn_score.hip scores a
// classification one: per row and predicted quantity the predictive mean and variance (bnn_mc_regression's bits), the squared
// error, the negative log-likelihood of the MC predictive -- the equal-weight mixture of the S per-sample Gaussians --, that of
// the moment-matched Gaussian, the mixture's CRPS and its probability integral transform; plus (optional) a device accumulator
// that carries their sums and the PIT histogram, per quantity, across the batches of a test set.
//
// With t the target, (m_s, v_s) bnn_mc_regression's per-sample mean and variance, sg_s = sqrt(v_s), z_s = (t - m_s) / sg_s:
//   nll   = -(logsumexp_s l_s - ln S),  l_s = -(ln 2 pi + ln v_s + z_s^2) / 2: bnn_score.hip's integer-exponent log-sum-exp in
//           base 2.  MEAN_LOGVAR: ln v_s is the input s itself and z_s = (t - m_s) e^(-s / 2), finite down to s = -176.
//           VALUES has no density: nll is written with gaussian_nll's bits.
//   crps  = (1/S) sum_s A(t - m_s, v_s) - (1 / 2 S^2) sum_i sum_j A(m_i - m_j, v_i + v_j)      (Grimit et al. 2006)
//           A(mu, sg^2) = mu erf(mu / sg sqrt 2) + sg sqrt(2 / pi) e^(-mu^2 / 2 sg^2),  A(mu, 0) = |mu|
//   pit   = (1/S) sum_s erfc(-z_s / sqrt 2) / 2;  a point mass (sg_s = 0) adds [t > m_s] + [t == m_s] / 2
// The terms are fp32 (erff / erfcf, v_exp_f32, v_log_f32, v_sqrt_f32); every sum over samples or pairs is fp64 in a fixed order.
// A negative or NaN variance reaches crps and pit through its square root and nll through an explicit test.
//
// The pair sum: A is symmetric, so sample i takes the partners i + 1 .. i + (S - 1) / 2 (mod S) -- and i + S / 2 for i < S / 2
// when S is even --, every unordered pair once with the same count for every i, and adds the diagonal A(0, 2 v_i); the total is
// diagonal + 2 x the rest.  The partners' (m, v) are READ AGAIN: from y, which the O(S) pass has just pulled through L2, or --
// a fused head's partials -- from the rows that pass staged in `workspace` after adding the parts once.  Nothing of a row's S
// samples has to fit in LDS or registers, so S up to 1024 takes the same code.  Work splits (bnn_mc_parts.hpp):
//   narrow (width <= 16): lane = (row, sl) as k_reg_narrow; lane sl owns the pair sum's rows i = sl, sl + G, ...; the staged
//           rows of a group were written by its other lanes: one workgroup barrier between the two passes.
//   wide   a lane holds its 4-quantity chunks over all samples as k_reg_wide and reads back only what it staged itself.
// The sums a row's lanes hold meet in k_reg_narrow's xor tree; `mean` and `variance` go through reg_acc / reg_moments in
// bnn_mc_regression's order, hence its bits.
//
// The accumulator: the launch leaves six words per element in `workspace` (sq_err, nll, gaussian_nll, crps, variance, pit as
// written) and a second launch of D workgroups adds quantity d's column to `state`: five fp64 sums lane-strided in row order
// then a fixed tree, the PIT counts as integers in LDS.  No float atomics, no global atomics: bitwise reproducible.
#include "bnn_mc_parts.hpp"

namespace bnn {

constexpr int kRsMaxBins = 128;
constexpr int kRsMaxSamples = 1024;         // the pair sum is quadratic in S
constexpr int kRsRecWords = 6;
constexpr float kLog2TwoPi = 2.65149612947231880f;
constexpr float kRsqrt2 = 0.70710678118654752f;
constexpr float kSqrt2OverPi = 0.79788456080286536f;

struct RegScoreArgs {
    UncArgs u;                              // u.mean / u.total: mean / variance (may be NULL); aleatoric / epistemic unused
    const float *target;
    float *sq_err, *nll, *gnll, *crps, *pit;
    float *stage;                           // workspace: a fused head's summed rows (S, rows, width); NULL for stacked outputs
    float *rec;                             // workspace: 6 x rows x D words (NULL without a state)
    int stage_vec;                          // wide split: 16-B loads of the staged rows are aligned
    int tvec;                               //             and of the targets
};

// what one predicted quantity sums over the samples
struct RsSums {
    double sd, sd2, sv;                     // reg_acc's
    double a1, pit, pair;                   // sum A(t - m_s, v_s), sum Phi(z_s), sum_i sum_j A(m_i - m_j, v_i + v_j)
    Lse L;                                  // log2 of the per-sample densities
};

__device__ __forceinline__ void rs_zero(RsSums &q)
{
    q.sd = q.sd2 = q.sv = q.a1 = q.pit = q.pair = 0.0;
    q.L = Lse{kLseEmpty, 0.0};
}

// A(mu, sg^2) for sg > 0, z = mu / sg
__device__ __forceinline__ float gauss_a(float mu, float sg, float z)
{
    return mu * erff(z * kRsqrt2) + sg * kSqrt2OverPi * __builtin_amdgcn_exp2f(-0.5f * kLog2e * z * z);
}

// A(mu, vv) of a pair: vv = v_i + v_j (negative or NaN: NaN through the root)
__device__ __forceinline__ float pair_a(float mu, float vv)
{
    if (vv == 0.f) return fabsf(mu);
    const float sg = __builtin_sqrtf(vv);
    return gauss_a(mu, sg, mu / sg);
}

// one sample's terms against the target t: raw = the second half's value (unused for VALUES)
template <int KIND>
__device__ __forceinline__ void rs_sample(float m, float raw, float t, RsSums &q)
{
    const float r = t - m;
    float sg = 0.f, z = 0.f;
    if constexpr (KIND == BNN_REG_MEAN_LOGVAR) {
        const float h = 0.5f * kLog2e * raw;
        sg = __builtin_amdgcn_exp2f(h);
        z = r * __builtin_amdgcn_exp2f(-h);
        lse_add(q.L, -0.5f * (kLog2TwoPi + kLog2e * (raw + z * z)));
    } else if constexpr (KIND == BNN_REG_MEAN_VAR) {
        sg = __builtin_sqrtf(raw);
        z = r / sg;
        lse_add(q.L, raw > 0.f ? -0.5f * (kLog2TwoPi + __builtin_amdgcn_logf(raw) + kLog2e * z * z) : __builtin_nanf(""));
    }
    if (sg == 0.f) {                        // a point mass
        q.a1 += (double)fabsf(r);
        q.pit += t > m ? 1.0 : (t == m ? 0.5 : 0.0);
    } else {
        q.a1 += (double)gauss_a(r, sg, z);
        q.pit += (double)(0.5f * erfcf(-z * kRsqrt2));
    }
}

// the pair sum's row i against partner j, one quantity
template <int KIND>
__device__ __forceinline__ float rs_pair(float mi, float vi, float mj, float vj)
{
    if constexpr (KIND == BNN_REG_VALUES) return fabsf(mi - mj);
    return pair_a(mi - mj, reg_var<KIND>(vi) + reg_var<KIND>(vj));
}

// partners of row i of the pair sum: every unordered pair of 0 .. S - 1 is some row's (i, i + k mod S), 1 <= k <= count
__device__ __forceinline__ int rs_partners(int i, int S)
{
    return ((S - 1) >> 1) + ((S & 1) == 0 && i < (S >> 1) ? 1 : 0);
}

// What one lane writes for element `at` = r D + d once the element's sums are known.
template <int KIND>
__device__ __forceinline__ void rs_finish(const RegScoreArgs &A, int64_t at, float ref, float t, const RsSums &q, double inv_S)
{
    const int S = A.u.nsamples;
    const float nan = __builtin_nanf("");
    const Moments64 mo = reg_moments(ref, q.sd, q.sd2, q.sv, inv_S);
    const double V = mo.ale + mo.epi;
    const float f_mean = (float)mo.mean, f_var = (float)V;
    const double e = mo.mean - (double)t;
    const double g = V == 0.0 ? (double)nan : 0.5 * (log(6.283185307179586477 * V) + e * e / V);
    double nll = g;
    if constexpr (KIND != BNN_REG_VALUES) nll = lse_nll(q.L, S);
    const bool ok = t == t;                 // a NaN target: the element's five scores are NaN
    const float f_sq = ok ? (float)(e * e) : nan;
    const float f_nll = ok ? (float)nll : nan;
    const float f_g = ok ? (float)g : nan;
    const float f_crps = ok ? (float)(q.a1 * inv_S - q.pair * (0.5 * inv_S * inv_S)) : nan;
    const float f_pit = ok ? (float)(q.pit * inv_S) : nan;
    if (A.u.mean) A.u.mean[at] = f_mean;
    if (A.u.total) A.u.total[at] = f_var;
    if (A.sq_err) A.sq_err[at] = f_sq;
    if (A.nll) A.nll[at] = f_nll;
    if (A.gnll) A.gnll[at] = f_g;
    if (A.crps) A.crps[at] = f_crps;
    if (A.pit) A.pit[at] = f_pit;
    if (A.rec) {
        const int64_t n = A.u.rows * (int64_t)(KIND == BNN_REG_VALUES ? A.u.classes : A.u.classes / 2);
        A.rec[at] = f_sq;
        A.rec[n + at] = f_nll;
        A.rec[2 * n + at] = f_g;
        A.rec[3 * n + at] = f_crps;
        A.rec[4 * n + at] = f_var;
        A.rec[5 * n + at] = f_pit;
    }
}

// ---------------------------------------------------------------------------------------------- narrow: width <= 16
// k_reg_narrow's split: lane = (row, sl), sl = lane & (G - 1) takes samples sl, sl + G, ... in both passes.
template <int KIND, bool FUSED>
__global__ __launch_bounds__(kUncThreads) void k_rscore_narrow(RegScoreArgs A, int D, int glog, int rpb, uint32_t *advance_epoch,
                                                               uint32_t advance_inc)
{
    constexpr bool VAR = KIND != BNN_REG_VALUES;
    constexpr int NV = VAR ? kUncNarrow / 2 : kUncNarrow;
    unc_advance(advance_epoch, advance_inc);
    const int nwork = (int)gridDim.x;
    const NarrowLane L(glog, rpb);
    const int G = L.G, sl = L.sl;
    const int W = A.u.classes, S = A.u.nsamples;
    const double inv_S = 1.0 / (double)S;
    const float *src = FUSED ? A.stage : A.u.y;
    const int64_t src_stride = FUSED ? A.u.rows * W : A.u.stride;
    for (int64_t rb = blockIdx.x; rb * rpb < A.u.rows; rb += nwork) {
        const int64_t r = rb * rpb + L.lr;
        const bool live = L.live(r, A.u.rows);
        const bool work = live && sl < S;
        const float *row = A.u.y + r * W;
        float m[NV], v[NV], mn[NV], vn[NV], t[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) m[i] = v[i] = mn[i] = vn[i] = t[i] = 0.f;
        if (live) row_load<NV, 1>(A.target + r * D, D, 0, 0, 0.f, t);
        auto load = [&](int s, float (&a)[NV], float (&b)[NV]) {
            const float *q = row + (int64_t)s * A.u.stride;
            if constexpr (FUSED) {
                parts_sum<NV, 1, 8>(A.u.nparts, A.u.part_stride, D, q, 0, a);
                if constexpr (VAR) parts_sum<NV, 1, 8>(A.u.nparts, A.u.part_stride, D, q + D, 0, b);
                float *o = A.stage + ((int64_t)s * A.u.rows + r) * W;       // the parts added once: the pair sum reads this
#pragma unroll
                for (int i = 0; i < NV; ++i)
                    if (i < D) {
                        o[i] = a[i];
                        if constexpr (VAR) o[D + i] = b[i];
                    }
            } else {
                row_load<NV, 1>(q, D, 0, 0, 0.f, a);
                if constexpr (VAR) row_load<NV, 1>(q + D, D, 0, 0, 0.f, b);
            }
        };
        if (work) load(sl, m, v);
        float ref[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) ref[i] = __shfl(m[i], L.lead, 64);
        RsSums q[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) rs_zero(q[i]);
        if (work) {
            for (int s = sl; s < S; s += G) {
                if (!FUSED && s + G < S) load(s + G, mn, vn);       // next sample's loads in flight meanwhile
#pragma unroll
                for (int i = 0; i < NV; ++i)
                    if (i < D) {
                        reg_acc<KIND>(m[i], ref[i], v[i], q[i].sd, q[i].sd2, q[i].sv);
                        rs_sample<KIND>(m[i], v[i], t[i], q[i]);
                    }
                if (FUSED) {
                    if (s + G < S) load(s + G, m, v);
                } else {
#pragma unroll
                    for (int i = 0; i < NV; ++i) { m[i] = mn[i]; v[i] = vn[i]; }
                }
            }
        }
        if constexpr (FUSED) __syncthreads();                       // the group's staged rows: written by its other lanes
        if (work) {
            const float *prow = src + r * W;
            auto pload = [&](int s, float (&a)[NV], float (&b)[NV]) {
                row_load<NV, 1>(prow + (int64_t)s * src_stride, D, 0, 0, 0.f, a);
                if constexpr (VAR) row_load<NV, 1>(prow + (int64_t)s * src_stride + D, D, 0, 0, 0.f, b);
            };
            for (int i = sl; i < S; i += G) {
                float mi[NV], vi[NV], mj[NV], vj[NV];
                double acc[NV];
#pragma unroll
                for (int c = 0; c < NV; ++c) { vi[c] = vj[c] = 0.f; acc[c] = 0.0; }
                pload(i, mi, vi);
                const int n = rs_partners(i, S);
                int j = i;
                for (int k = 0; k < n; ++k) {
                    j = j + 1 == S ? 0 : j + 1;
                    pload(j, mj, vj);
#pragma unroll
                    for (int c = 0; c < NV; ++c)
                        if (c < D) acc[c] += (double)rs_pair<KIND>(mi[c], vi[c], mj[c], vj[c]);
                }
#pragma unroll
                for (int c = 0; c < NV; ++c)
                    if (c < D) q[c].pair += (double)rs_pair<KIND>(mi[c], vi[c], mi[c], vi[c]) + 2.0 * acc[c];
            }
        }
        // the G lanes of a row: a fixed xor tree (every lane of the group ends with the same bits)
        for (int o = 1; o < G; o <<= 1) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (i < D) {
                    q[i].sd += __shfl_xor(q[i].sd, o, 64);
                    q[i].sd2 += __shfl_xor(q[i].sd2, o, 64);
                    q[i].a1 += __shfl_xor(q[i].a1, o, 64);
                    q[i].pit += __shfl_xor(q[i].pit, o, 64);
                    q[i].pair += __shfl_xor(q[i].pair, o, 64);
                    if constexpr (VAR) {
                        q[i].sv += __shfl_xor(q[i].sv, o, 64);
                        const int M2 = __shfl_xor(q[i].L.M, o, 64);
                        const double A2 = __shfl_xor(q[i].L.A, o, 64);
                        lse_merge(q[i].L, M2, A2);
                    }
                }
        }
        if (live && sl == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (i < D) rs_finish<KIND>(A, r * D + i, ref[i], t[i], q[i], inv_S);
        }
    }
}

// ---------------------------------------------------------------------------------------------- wide: width <= 4096
// k_reg_wide's split: TPR threads per row, NCH 4-quantity chunks per thread, all samples in sample order in both passes.
template <int KIND, bool FUSED, int TPR, int NCH>
__global__ __launch_bounds__(kUncThreads) void k_rscore_wide(RegScoreArgs A, int D, uint32_t *advance_epoch, uint32_t advance_inc)
{
    constexpr bool VAR = KIND != BNN_REG_VALUES;
    constexpr int NV = 4 * NCH;
    constexpr int RPB = kUncThreads / TPR;
    unc_advance(advance_epoch, advance_inc);
    const int nwork = (int)gridDim.x;
    const int th = (int)threadIdx.x % TPR;
    const int W = A.u.classes, S = A.u.nsamples;
    const double inv_S = 1.0 / (double)S;
    const float *src = FUSED ? A.stage : A.u.y;
    const int64_t src_stride = FUSED ? A.u.rows * W : A.u.stride;
    const int src_vec = FUSED ? A.stage_vec : A.u.vec;
    for (int64_t rb = blockIdx.x; rb * RPB < A.u.rows; rb += nwork) {
        const int64_t r = rb * RPB + (int)threadIdx.x / TPR;
        if (r >= A.u.rows) continue;
        const float *row = A.u.y + r * W;
        float m[NV], v[NV], mn[NV], vn[NV], ref[NV], t[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = vn[i] = 0.f;
        row_load<NV, TPR>(A.target + r * D, D, A.tvec, th, 0.f, t);
        auto load = [&](int s, float (&a)[NV], float (&b)[NV]) {
            const float *q = row + (int64_t)s * A.u.stride;
            if constexpr (FUSED) {
                parts_sum<NV, TPR, (NV >= 16 ? 2 : 32 / NV)>(A.u.nparts, A.u.part_stride, D, q, th, a);
                if constexpr (VAR) parts_sum<NV, TPR, (NV >= 16 ? 2 : 32 / NV)>(A.u.nparts, A.u.part_stride, D, q + D, th, b);
                float *o = A.stage + ((int64_t)s * A.u.rows + r) * W;       // this lane's columns: it alone reads them back
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int c = unc_col<TPR>(th, i);
                    if (c < D) {
                        o[c] = a[i];
                        if constexpr (VAR) o[D + c] = b[i];
                    }
                }
            } else {
                row_load<NV, TPR>(q, D, A.u.vec, th, 0.f, a);
                if constexpr (VAR) row_load<NV, TPR>(q + D, D, A.u.vec, th, 0.f, b);
            }
        };
        RsSums q[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) rs_zero(q[i]);
        load(0, m, v);
#pragma unroll
        for (int i = 0; i < NV; ++i) ref[i] = m[i];
        for (int s = 0; s < S; ++s) {
            if (!FUSED && s + 1 < S) load(s + 1, mn, vn);           // next sample's loads in flight meanwhile
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (unc_col<TPR>(th, i) < D) {
                    reg_acc<KIND>(m[i], ref[i], v[i], q[i].sd, q[i].sd2, q[i].sv);
                    rs_sample<KIND>(m[i], v[i], t[i], q[i]);
                }
            if (FUSED) {
                if (s + 1 < S) load(s + 1, m, v);
            } else {
#pragma unroll
                for (int i = 0; i < NV; ++i) { m[i] = mn[i]; v[i] = vn[i]; }
            }
        }
        const float *prow = src + r * W;
        auto pload = [&](int s, float (&a)[NV], float (&b)[NV]) {
            row_load<NV, TPR>(prow + (int64_t)s * src_stride, D, src_vec, th, 0.f, a);
            if constexpr (VAR) row_load<NV, TPR>(prow + (int64_t)s * src_stride + D, D, src_vec, th, 0.f, b);
        };
        for (int i = 0; i < S; ++i) {
            float mi[NV], vi[NV], mj[NV], vj[NV];
            double acc[NV];
#pragma unroll
            for (int c = 0; c < NV; ++c) { vi[c] = vj[c] = 0.f; acc[c] = 0.0; }
            pload(i, mi, vi);
            const int n = rs_partners(i, S);
            int j = i;
            for (int k = 0; k < n; ++k) {
                j = j + 1 == S ? 0 : j + 1;
                pload(j, mj, vj);
#pragma unroll
                for (int c = 0; c < NV; ++c)
                    if (unc_col<TPR>(th, c) < D) acc[c] += (double)rs_pair<KIND>(mi[c], vi[c], mj[c], vj[c]);
            }
#pragma unroll
            for (int c = 0; c < NV; ++c)
                if (unc_col<TPR>(th, c) < D) q[c].pair += (double)rs_pair<KIND>(mi[c], vi[c], mi[c], vi[c]) + 2.0 * acc[c];
        }
        const int64_t o0 = r * D;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = unc_col<TPR>(th, i);
            if (c < D) rs_finish<KIND>(A, o0 + c, ref[i], t[i], q[i], inv_S);
        }
    }
}

// ---------------------------------------------------------------------------------------------- the accumulator
constexpr int kRsAccThreads = 256;

// Workgroup d adds quantity d's column of the launch's words to its part of `state` (layout: include/bnn_hip.h).  A thread
// takes rows tid, tid + 256, ...; the waves' sums meet in wave order.
__global__ __launch_bounds__(kRsAccThreads) void k_rscore_accumulate(const float *__restrict__ rec, int64_t rows, int D, int bins,
                                                                     double *__restrict__ state)
{
    constexpr int NW = kRsAccThreads / 64;
    constexpr int NS = kRsRecWords - 1;
    __shared__ unsigned cnt[kRsMaxBins];
    __shared__ double red[NS][NW];
    const int d = (int)blockIdx.x;
    for (int i = threadIdx.x; i < bins; i += kRsAccThreads) cnt[i] = 0u;
    __syncthreads();
    const int64_t n = rows * D;
    double a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += kRsAccThreads) {
        const int64_t at = r * D + d;
#pragma unroll
        for (int k = 0; k < NS; ++k) a[k] += (double)rec[k * n + at];
        const float p = rec[NS * n + at];
        if (p == p) {                                               // a NaN pit counts in n and in no bin
            const double b = floor((double)p * (double)bins);
            const int bin = b >= (double)bins ? bins - 1 : (b >= 0.0 ? (int)b : 0);
            atomicAdd(&cnt[bin], 1u);
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        a[k] = wave_sum(a[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = a[k];
    }
    __syncthreads();
    double *st = state + (int64_t)d * (kRsRecWords + bins);
    const int b = (int)threadIdx.x;
    if (b == 0) st[0] += (double)rows;
    if (b >= 1 && b <= NS) {
        double s = 0.0;
        for (int w = 0; w < NW; ++w) s += red[b - 1][w];            // the waves' sums in wave order
        st[b] += s;
    }
    for (int i = b; i < bins; i += kRsAccThreads) st[kRsRecWords + i] += (double)cnt[i];
}

// the extents of a call, shared by the workspace query and the launch; 0 = fine
static int rs_check(const TailNames &N, int nparts, int nsamples, int64_t rows, int width, int kind)
{
    int rc = tail_check_extents(N, nparts, nsamples, rows, width);
    if (rc) return rc;
    if (nsamples > kRsMaxSamples) { set_error("%s: more than %d samples (the pair sum is quadratic in them)", N.who, kRsMaxSamples); return BNN_E_RANGE; }
    if (kind != BNN_REG_VALUES && kind != BNN_REG_MEAN_LOGVAR && kind != BNN_REG_MEAN_VAR) {
        set_error("%s: unknown kind %d", N.who, kind);
        return BNN_E_RANGE;
    }
    if (kind != BNN_REG_VALUES && width % 2) { set_error("%s: odd width %d for a (mean, variance) layout", N.who, width); return BNN_E_SHAPE; }
    return BNN_OK;
}

// floats of the workspace's two parts: a fused head's staged rows, then the accumulator's words
static void rs_workspace(int nparts, int nsamples, int64_t rows, int width, int kind, int with_state, int64_t &stage, int64_t &rec)
{
    const int D = kind == BNN_REG_VALUES ? width : width / 2;
    stage = nparts > 1 ? (int64_t)nsamples * rows * width : 0;
    rec = with_state ? kRsRecWords * rows * D : 0;
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int64_t bnn_mc_regression_score_state_doubles(int D, int pit_bins)
{
    if (D < 1 || D > 4096 || pit_bins < 1 || pit_bins > kRsMaxBins) {
        set_error("bnn_mc_regression_score_state_doubles: D outside 1 .. 4096 or bins outside 1 .. %d", kRsMaxBins);
        return 0;
    }
    return (int64_t)D * (kRsRecWords + pit_bins);
}

int64_t bnn_mc_regression_score_workspace_bytes(int nparts, int nsamples, int64_t rows, int width, int kind, int with_state)
{
    const TailNames N{"bnn_mc_regression_score_workspace_bytes", "width above 4096", ""};
    if (rs_check(N, nparts, nsamples, rows, width, kind)) return 0;
    int64_t stage, rec;
    rs_workspace(nparts, nsamples, rows, width, kind, with_state, stage, rec);
    return 4 * (stage + rec);
}

int bnn_mc_regression_score(const float *y, int64_t addend_stride, int nparts, int nsamples, int64_t rows, int width, int kind,
                            const float *target, float *mean, float *variance, float *sq_err, float *nll, float *gaussian_nll,
                            float *crps, float *pit, double *state, int pit_bins, void *workspace, uint32_t *advance_epoch,
                            uint32_t advance_inc, void *stream)
{
    const TailNames N{"bnn_mc_regression_score", "width above 4096", "addend_stride below rows * width"};
    const char *who = N.who;
    if (!y || !target) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    int rc = rs_check(N, nparts, nsamples, rows, width, kind);
    if (rc) return rc;
    const int64_t naddends = (int64_t)nparts * nsamples;
    rc = tail_check_stride(N, naddends, addend_stride, rows, width);
    if (rc) return rc;
    if (state) {
        if (pit_bins < 1) { set_error("%s: fewer than 1 bin", who); return BNN_E_SHAPE; }
        if (pit_bins > kRsMaxBins) { set_error("%s: more than %d bins", who, kRsMaxBins); return BNN_E_RANGE; }
    }
    int64_t stage, rec;
    rs_workspace(nparts, nsamples, rows, width, kind, state != nullptr, stage, rec);
    if (stage + rec > 0 && !workspace) { set_error("%s: this call needs the workspace", who); return BNN_E_NULL; }
    if ((reinterpret_cast<uintptr_t>(state) & 7u) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0) {
        set_error("%s: state not 8-byte or workspace not 4-byte aligned", who);
        return BNN_E_ALIGN;
    }
    const int D = kind == BNN_REG_VALUES ? width : width / 2;
    RegScoreArgs A{};
    // 16-B loads of both halves: D % 4 == 0 (then width % 4 == 0 as well); the outputs are stored one by one
    A.u = unc_args(y, addend_stride, nparts, nsamples, rows, width, tail_vec(D, naddends, addend_stride, {y}), mean, variance,
                   nullptr, nullptr);
    A.target = target;
    A.sq_err = sq_err; A.nll = nll; A.gnll = gaussian_nll; A.crps = crps; A.pit = pit;
    float *ws = reinterpret_cast<float *>(workspace);
    A.stage = stage ? ws : nullptr;
    A.rec = rec ? ws + stage : nullptr;
    A.stage_vec = tail_vec(D, 1, 0, {workspace});
    A.tvec = tail_vec(D, 1, 0, {target});
    hipStream_t st = (hipStream_t)stream;
    if (width <= kUncNarrow) {
        const NarrowPlan P = narrow_plan(nsamples, rows, 0);
        kind_dispatch<BNN_REG_VALUES, BNN_REG_MEAN_LOGVAR, BNN_REG_MEAN_VAR>(kind, nparts > 1, [&](auto K, auto FU) {
            hipLaunchKernelGGL((k_rscore_narrow<K.value, FU.value>), P.grid, dim3(kUncThreads), 0, st, A, D, P.glog, P.rpb,
                               advance_epoch, advance_inc);
        });
    } else {
        const WidePlan P = wide_plan(width, D, rows, 0);
        kind_dispatch<BNN_REG_VALUES, BNN_REG_MEAN_LOGVAR, BNN_REG_MEAN_VAR>(kind, nparts > 1, [&](auto K, auto FU) {
            // VALUES: D = width, up to 4 chunks per thread; the (mean, variance) layouts: D = width / 2, at most 2
            wide_dispatch<(K.value == BNN_REG_VALUES ? 4 : 2)>(P, [&](auto T, auto NC) {
                hipLaunchKernelGGL((k_rscore_wide<K.value, FU.value, T.value, NC.value>), P.grid, dim3(kUncThreads), 0, st, A, D,
                                   advance_epoch, advance_inc);
            });
        });
    }
    rc = check_launch(who);
    if (rc || !state) return rc;
    hipLaunchKernelGGL(k_rscore_accumulate, dim3((unsigned)D), dim3(kRsAccThreads), 0, st, A.rec, rows, D, pit_bins, state);
    return check_launch(who);
}

}  // extern "C"
