// bnn_mc_parts.hpp -- the skeleton the one-launch MC tails over (S, rows, width) outputs share (bnn_uncertainty.hip:
// classification, bnn_score.hip: classification against labels, bnn_regression.hip: regression, bnn_regression_score.hip:
// regression against targets, bnn_evidential.hip: the NIG mixture).  Host: the argument checks, the launch arguments with their `vec` rule, the narrow and wide launch plans and the
// dispatch of a plan / a (kind, fused) pair to a kernel instantiation.  Device: the narrow split's lane geometry, the row
// loader, a fused head's partials added in bnn_mc_sum's order, the four-moment stores, the epoch / KL tails of the launch, and
// the classification tails' row reductions, the log-sum-exp over samples the two scoring tails share and the moments the two
// regression tails share.  What else a sample contributes -- the arithmetic -- stays in each tail's own file.
#pragma once
#include <initializer_list>
#include <type_traits>
#include "bnn_device.hpp"
#include "bnn_kl_body.hpp"
#include "bnn_mc.hpp"

namespace bnn {

constexpr int kUncThreads = 256;
constexpr int kUncNarrow = 16;              // row width a lane of the narrow split holds
constexpr int kUncMaxBlocks = 1 << 20;      // work workgroups per launch (grid-stride above)
constexpr float kLog2e = 1.44269504088896341f;
static_assert(kUncThreads == kKlThreads, "the KL tail runs as one workgroup of this launch");

struct UncArgs {
    const float *y;
    int64_t stride;         // elements between addends
    int64_t part_stride;    // nsamples * stride: between the parts of one sample
    int64_t rows;
    int nparts, nsamples, classes;      // classes: the row width
    int vec;                // wide split: 16-B loads / stores are aligned (classes % 4 == 0, y / stride / mean aligned)
    float *mean, *total, *aleatoric, *epistemic;
};

// ------------------------------------------------------------------------------------------------------------ host side
static inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// What an entry calls itself and its arguments in messages.
struct TailNames { const char *who, *too_wide, *stride_low; };

// The extents every tail takes: BNN_E_SHAPE below 1, BNN_E_RANGE above what the kernels index.
static inline int tail_check_extents(const TailNames &N, int nparts, int nsamples, int64_t rows, int width)
{
    if (nparts < 1 || nsamples < 1 || rows < 1 || width < 1) { set_error("%s: bad extent", N.who); return BNN_E_SHAPE; }
    if (nsamples > 65536) { set_error("%s: more than 65536 samples", N.who); return BNN_E_RANGE; }
    if (width > 4096) { set_error("%s: %s", N.who, N.too_wide); return BNN_E_RANGE; }
    if (rows > 0x7FFFFFFF) { set_error("%s: more than 2^31 - 1 rows", N.who); return BNN_E_RANGE; }
    return BNN_OK;
}

// Addends may not overlap (a single addend has no stride).  Its own call, so that an entry's kind / layout checks (BNN_E_RANGE)
// come between the two and a call with several bad arguments keeps its code.
static inline int tail_check_stride(const TailNames &N, int64_t naddends, int64_t stride, int64_t rows, int width)
{
    if (naddends > 1 && stride < rows * width) { set_error("%s: %s", N.who, N.stride_low); return BNN_E_SHAPE; }
    return BNN_OK;
}

// The wide split's 16-B loads / stores are aligned: `quantities` (what a chunk counts: the row width, or D with the variances'
// half behind) a multiple of 4, the addends a multiple of 4 apart, every pointer of `aligned` on 16 B (NULL counts as aligned).
static inline int tail_vec(int quantities, int64_t naddends, int64_t stride, std::initializer_list<const void *> aligned)
{
    bool ok = quantities % 4 == 0 && (stride % 4 == 0 || naddends == 1);
    for (const void *p : aligned) ok = ok && al16(p);
    return ok;
}

static inline UncArgs unc_args(const float *y, int64_t stride, int nparts, int nsamples, int64_t rows, int width, int vec,
                               float *mean, float *total, float *aleatoric, float *epistemic)
{
    UncArgs A{};
    A.y = y;
    A.stride = stride;
    A.part_stride = (int64_t)nsamples * stride;
    A.rows = rows;
    A.nparts = nparts;
    A.nsamples = nsamples;
    A.classes = width;
    A.vec = vec;
    A.mean = mean; A.total = total; A.aleatoric = aleatoric; A.epistemic = epistemic;
    return A;
}

static inline dim3 tail_grid(int64_t work, int has_kl)
{
    return dim3((unsigned)((work < kUncMaxBlocks ? work : kUncMaxBlocks) + has_kl));    // has_kl: KL's second pass, one more
}

// narrow (width <= kUncNarrow): G = 1 << glog lanes share a row (the next power of two >= nsamples, <= 64), rpb rows per
// workgroup.  A workgroup's four waves issue their scattered loads through one CU: below 256 workgroups, fewer rows per
// workgroup (the step's tail, 512 rows x 8 samples: 16 workgroups of 32 rows -> 256 of 2).
struct NarrowPlan { int glog, rpb; dim3 grid; };

static inline NarrowPlan narrow_plan(int nsamples, int64_t rows, int has_kl)
{
    NarrowPlan P{};
    while ((1 << P.glog) < nsamples && P.glog < 6) ++P.glog;
    P.rpb = kUncThreads >> P.glog;
    while (P.rpb > 1 && (rows + P.rpb - 1) / P.rpb < 256) P.rpb >>= 1;
    P.grid = tail_grid((rows + P.rpb - 1) / P.rpb, has_kl);
    return P;
}

// wide: a wave per row up to width 1024, the workgroup per row above; nch 4-quantity chunks per thread (<= 16 quantities).
struct WidePlan { int tpr, nch; dim3 grid; };

static inline WidePlan wide_plan(int width, int quantities, int64_t rows, int has_kl)
{
    WidePlan P{};
    P.tpr = width <= 1024 ? 64 : 256;
    P.nch = (quantities + 4 * P.tpr - 1) / (4 * P.tpr);
    P.grid = tail_grid((rows + kUncThreads / P.tpr - 1) / (kUncThreads / P.tpr), has_kl);
    return P;
}

template <int V> using ic = std::integral_constant<int, V>;

// f(ic<TPR>, ic<NCH>) for the plan: (64, 1 | 2 | 4) or (256, 2 | 4).  MAXCH 2: a caller whose plans never exceed two chunks (the
// (mean, variance) layouts: D = width / 2), so that NCH = 4 is not instantiated for it.
template <int MAXCH = 4, typename F>
static inline void wide_dispatch(const WidePlan &P, F &&f)
{
    if (P.tpr == 64) {
        if (P.nch == 1) return f(ic<64>{}, ic<1>{});
        if (P.nch == 2 || MAXCH == 2) return f(ic<64>{}, ic<2>{});
        if constexpr (MAXCH == 4) return f(ic<64>{}, ic<4>{});
    } else {
        if (P.nch <= 2 || MAXCH == 2) return f(ic<256>{}, ic<2>{});
        if constexpr (MAXCH == 4) return f(ic<256>{}, ic<4>{});
    }
}

// f(ic<KIND>, bool_constant<fused>) for the one of KINDS that `kind` is (the entry has checked that it is one).
template <int... KINDS, typename F>
static inline void kind_dispatch(int kind, bool fused, F &&f)
{
    auto one = [&](auto K) {
        if (kind != K.value) return;
        if (fused) f(K, std::true_type{});
        else f(K, std::false_type{});
    };
    (one(ic<KINDS>{}), ...);
}

// ---------------------------------------------------------------------------------------------------------- device side
// narrow split: lane = (row lr of the workgroup's rpb, sl): sl = lane & (G - 1) takes samples sl, sl + G, ...; `lead`: the wave
// lane that holds sample 0 of this lane's row.
struct NarrowLane {
    int G, sl, lr, lead, rpb;
    __device__ __forceinline__ NarrowLane(int glog, int rpb_)
        : G(1 << glog), sl((int)threadIdx.x & (G - 1)), lr((int)threadIdx.x >> glog), lead(((int)threadIdx.x & 63) & ~(G - 1)), rpb(rpb_) {}
    __device__ __forceinline__ bool live(int64_t r, int64_t rows) const { return lr < rpb && r < rows; }
};

// Column of value slot i of a lane: 4-column chunks, chunk k at 4 * (lead + k * STEP).  Narrow: lead 0, STEP 1 -> slot i = column i.
template <int STEP>
__device__ __forceinline__ int unc_col(int lead, int i) { return 4 * (lead + (i >> 2) * STEP) + (i & 3); }

// Columns [0, C) at q into a lane's slots, `pad` outside the row: 16-B loads when `vec`, else scalar ones.  Wide: STEP = TPR,
// lead = the thread of the row.  The narrow split's load is STEP 1, lead 0, vec 0.
template <int NV, int STEP>
__device__ __forceinline__ void row_load(const float *q, int C, int vec, int lead, float pad, float (&v)[NV])
{
    if (vec) {
#pragma unroll
        for (int k = 0; k < NV / 4; ++k) {
            const int c = 4 * (lead + k * STEP);
            const float4 f = c < C ? *reinterpret_cast<const float4 *>(q + c) : make_float4(pad, pad, pad, pad);
            v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = unc_col<STEP>(lead, i);
            v[i] = c < C ? q[c] : pad;
        }
    }
}

// a[i] = 0.f + q[p0 ps + c_i] + ... + q[(p1 - 1) ps + c_i] in part order, PB parts' loads in flight.  Padding with 0.f is exact
// (a sum that starts at +0 is never -0), as in mc_sum_split_body.
template <int NV, int STEP, int PB>
__device__ __forceinline__ void seq_parts(const float *__restrict__ q, int64_t ps, int p0, int p1, int lead, int C, float (&a)[NV])
{
#pragma unroll
    for (int i = 0; i < NV; ++i) a[i] = 0.f;
    for (int p = p0; p < p1; p += PB) {
        float v[PB][NV];
#pragma unroll
        for (int j = 0; j < PB; ++j)
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = unc_col<STEP>(lead, i);
                v[j][i] = (p + j < p1 && c < C) ? q[(int64_t)(p + j) * ps + c] : 0.f;
            }
#pragma unroll
        for (int j = 0; j < PB; ++j)
#pragma unroll
            for (int i = 0; i < NV; ++i) a[i] += v[j][i];
    }
}

// Columns [0, C) at q of one sample from a fused head's partials (q = y + s * stride + row * width [+ column offset]), the parts
// `ps` elements apart: bnn_mc_sum's order over `nparts` addends -- sequential up to kMcSplitAbove, else four sequential quarters
// added left to right -- so the values are the bits HeadPartials.logits() stores.
template <int NV, int STEP, int PB>
__device__ __forceinline__ void parts_sum(int nparts, int64_t ps, int C, const float *__restrict__ q, int lead, float (&z)[NV])
{
    if (nparts <= kMcSplitAbove) {
        seq_parts<NV, STEP, PB>(q, ps, 0, nparts, lead, C, z);
        return;
    }
    const int per = (nparts + 3) >> 2;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        const int s0 = w * per < nparts ? w * per : nparts;
        const int s1 = s0 + per < nparts ? s0 + per : nparts;
        float g[NV];
        seq_parts<NV, STEP, PB>(q, ps, s0, s1, lead, C, g);
#pragma unroll
        for (int i = 0; i < NV; ++i) z[i] = w == 0 ? g[i] : z[i] + g[i];
    }
}

// One predicted quantity of a regression tail; each of the four outputs is (rows, D).
struct Moments { float mean, total, ale, epi; };

// (Args: UncArgs, or a tail's own arguments with the same four outputs and `vec`)
template <typename Args>
__device__ __forceinline__ void store_moments(const Args &A, int64_t at, const Moments &o)
{
    A.mean[at] = o.mean;
    A.total[at] = o.total;
    A.aleatoric[at] = o.ale;
    A.epistemic[at] = o.epi;
}

// The wide split's store of one 4-quantity chunk at column c of a row whose outputs start at o0: 16-B stores when A.vec.
template <typename Args>
__device__ __forceinline__ void store_moments4(const Args &A, int64_t o0, int c, int D, const Moments (&o)[4])
{
    if (A.vec) {
        if (c < D) {
            *reinterpret_cast<float4 *>(A.mean + o0 + c) = make_float4(o[0].mean, o[1].mean, o[2].mean, o[3].mean);
            *reinterpret_cast<float4 *>(A.total + o0 + c) = make_float4(o[0].total, o[1].total, o[2].total, o[3].total);
            *reinterpret_cast<float4 *>(A.aleatoric + o0 + c) = make_float4(o[0].ale, o[1].ale, o[2].ale, o[3].ale);
            *reinterpret_cast<float4 *>(A.epistemic + o0 + c) = make_float4(o[0].epi, o[1].epi, o[2].epi, o[3].epi);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < D) store_moments(A, o0 + c + j, o[j]);
    }
}

// The launch's first tail: one thread bumps the device epoch.
__device__ __forceinline__ void unc_advance(uint32_t *advance_epoch, uint32_t advance_inc)
{
    if (advance_epoch && blockIdx.x == 0 && threadIdx.x == 0) advance_epoch[0] += advance_inc;
}

// The launch's two tails; true = this workgroup ran the KL pass and is done.
__device__ __forceinline__ bool unc_tails(int nwork, uint32_t *advance_epoch, uint32_t advance_inc, const KlFinal &F,
                                          const double *__restrict__ partials, float *__restrict__ kl_out)
{
    if ((int)blockIdx.x == nwork) {
        kl_final_body(F, partials, kl_out);
        return true;
    }
    unc_advance(advance_epoch, advance_inc);
    return false;
}

// ---- shared by the classification tails (bnn_uncertainty.hip, bnn_score.hip)
constexpr double kLn2 = 0.693147180559945309417;

// Entropy of the per-row mean in bits, one class: -m log2 m (LOGITS, 0 log 0 = 0) / -m log2(m + 1e-10) (PROBS, the
// reference's Entropy convention).  The log is v_log_f32 on the fp32-rounded mean; a term below 2^-100 is dropped (<= 1e-28).
template <int KIND>
__device__ __forceinline__ double total_term_bits(double m)
{
    const float mf = (float)m;
    if constexpr (KIND == BNN_UNC_LOGITS) return mf > 0x1p-100f ? -m * (double)__builtin_amdgcn_logf(mf) : 0.0;
    return -m * (double)__builtin_amdgcn_logf(mf + 1e-10f);
}

// Row reductions over TPR threads: the wave's xor tree, then (TPR 256) the four waves' values in a fixed order through LDS.
// Every thread returns the same bits.  `slot`: LDS of this reduction (alternating per sample, so one barrier suffices).
template <int TPR>
__device__ __forceinline__ float row_max(float v, float *slot)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if constexpr (TPR == 256) {
        if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
        __syncthreads();
        v = fmaxf(fmaxf(slot[0], slot[1]), fmaxf(slot[2], slot[3]));
    }
    return v;
}

template <int TPR, typename T>
__device__ __forceinline__ void row_sum2(T &a, T &b, T *slot)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if constexpr (TPR == 256) {
        if ((threadIdx.x & 63) == 0) { slot[threadIdx.x >> 6] = a; slot[4 + (threadIdx.x >> 6)] = b; }
        __syncthreads();
        a = (slot[0] + slot[1]) + (slot[2] + slot[3]);
        b = (slot[4] + slot[5]) + (slot[6] + slot[7]);
    }
}


// ---- shared by the tails that take a log-sum-exp over the samples (bnn_score.hip, bnn_regression_score.hip)
constexpr int kLseEmpty = -(1 << 28);       // exponent of an empty log-sum-exp (A = 0)
constexpr int kLseShift = -2000;            // a rescale below 2^-2000 is 0 in fp64 anyway

// running log-sum-exp in base 2 over a row's samples
struct Lse { int M; double A; };

__device__ __forceinline__ void lse_add(Lse &L, float lp)
{
    if (lp != lp) { L.A = (double)lp; return; }                     // NaN in, NaN out
    if (!(lp >= -1.0e6f)) return;                                   // no mass
    const int c = (int)ceilf(lp);
    if (c > L.M) {
        const int d = L.M - c;
        L.A = ldexp(L.A, d > kLseShift ? d : kLseShift);
        L.M = c;
    }
    L.A += (double)__builtin_amdgcn_exp2f(lp - (float)L.M);
}

// the two operands' exact rescales, one commutative add: both lanes of an xor pair end with the same bits
__device__ __forceinline__ void lse_merge(Lse &L, int M2, double A2)
{
    const int M = L.M > M2 ? L.M : M2;
    const int d1 = L.M - M, d2 = M2 - M;
    L.A = ldexp(L.A, d1 > kLseShift ? d1 : kLseShift) + ldexp(A2, d2 > kLseShift ? d2 : kLseShift);
    L.M = M;
}

// -ln of the MC predictive at the label, LOGITS: -ln 2 (M + log2(A / S)), the log as total_term_bits takes it (v_log_f32 on the
// fp32-rounded A / S in (2^-17, 1]: M carries the range); +inf where no sample gave the label any mass
__device__ __forceinline__ double lse_nll(const Lse &L, int S)
{
    return -kLn2 * ((double)L.M + (double)__builtin_amdgcn_logf((float)(L.A / (double)S)));
}

// ---- shared by the regression tails (bnn_regression.hip, bnn_regression_score.hip)
template <int KIND>
__device__ __forceinline__ float reg_var(float v)
{
    if constexpr (KIND == BNN_REG_MEAN_LOGVAR) return __builtin_amdgcn_exp2f(v * kLog2e);
    return v;
}

// one sample's contribution of one quantity: d = m - m_0 in fp64 (exact for fp32 operands less than 2^29 apart in exponent)
template <int KIND>
__device__ __forceinline__ void reg_acc(float m, float ref, float v, double &sd, double &sd2, double &sv)
{
    const double d = (double)m - (double)ref;
    sd += d;
    sd2 = __builtin_fma(d, d, sd2);
    if constexpr (KIND != BNN_REG_VALUES) sv += (double)reg_var<KIND>(v);
}

// the fp64 moments of one quantity before they are rounded: mean, aleatoric, epistemic (total = ale + epi)
struct Moments64 { double mean, ale, epi; };

__device__ __forceinline__ Moments64 reg_moments(float ref, double sd, double sd2, double sv, double inv_S)
{
    const double md = sd * inv_S;
    double epi = __builtin_fma(-md, md, sd2 * inv_S);
    epi = epi > 0.0 ? epi : 0.0;
    return Moments64{(double)ref + md, sv * inv_S, epi};
}

__device__ __forceinline__ Moments reg_finish(float ref, double sd, double sd2, double sv, double inv_S)
{
    const Moments64 q = reg_moments(ref, sd, sd2, sv, inv_S);
    Moments o;
    o.mean = (float)q.mean;
    o.total = (float)(q.ale + q.epi);
    o.ale = (float)q.ale;
    o.epi = (float)q.epi;
    return o;
}

}  // namespace bnn
