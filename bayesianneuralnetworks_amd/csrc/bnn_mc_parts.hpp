// bnn_mc_parts.hpp -- what the one-launch MC tails over (S, rows, width) outputs share (bnn_uncertainty.hip: classification,
// bnn_regression.hip: regression): the launch arguments, a fused head's partials added in bnn_mc_sum's order, and the epoch / KL
// tails of the launch.
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

}  // namespace bnn
