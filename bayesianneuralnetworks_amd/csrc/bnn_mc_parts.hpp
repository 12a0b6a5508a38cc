// bnn_mc_parts.hpp -- what the one-launch MC tails over (S, rows, width) outputs share (bnn_uncertainty.hip: classification,
// bnn_score.hip: classification against labels, bnn_regression.hip: regression): the launch arguments, a fused head's partials
// added in bnn_mc_sum's order, the epoch / KL tails of the launch, and the classification tails' row reductions.
#pragma once
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

// Column of value slot i of a lane: 4-column chunks, chunk k at 4 * (lead + k * STEP).  Narrow: lead 0, STEP 1 -> slot i = column i.
template <int STEP>
__device__ __forceinline__ int unc_col(int lead, int i) { return 4 * (lead + (i >> 2) * STEP) + (i & 3); }

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

// The launch's two tails; true = this workgroup ran the KL pass and is done.
__device__ __forceinline__ bool unc_tails(int nwork, uint32_t *advance_epoch, uint32_t advance_inc, const KlFinal &F,
                                          const double *__restrict__ partials, float *__restrict__ kl_out)
{
    if ((int)blockIdx.x == nwork) {
        kl_final_body(F, partials, kl_out);
        return true;
    }
    if (advance_epoch && blockIdx.x == 0 && threadIdx.x == 0) advance_epoch[0] += advance_inc;
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

}  // namespace bnn
