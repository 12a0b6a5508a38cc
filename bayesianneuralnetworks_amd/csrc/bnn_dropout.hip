// bnn_dropout.hip -- MC dropout on the MC-batched path: the keyed mask of the RNG contract's mask part (include/bnn_hip.h)
// applied to a stacked (S, rows, F) activation or fanned out from a shared (rows, F) one, and its backward.  Streaming
// kernels: one thread per quad of 4 consecutive elements of a sample's r * F + f index (one drop_u4 per quad and sample);
// the mask is never stored -- the backward re-creates it from the key.
#include "bnn_device.hpp"

namespace bnn {

constexpr int kDropThreads = 256;
constexpr int kDropMaxBlocks = 4096;

struct DropParams {
    const void *x;
    int64_t x_sample_stride, ldx;   // elements; x_sample_stride unused when FAN
    void *y;
    int64_t y_sample_stride, ldy;
    uint32_t F, n;                  // features per row, rows * F (< 2^32)
    int32_t S;
    int32_t chunk;                  // FAN: samples per blockIdx.y
    float p, scale;
    RngDev rng;
};

template <int DT>
__device__ __forceinline__ float ld1(const void *b, int64_t i)
{
    if constexpr (DT == BNN_F32) return reinterpret_cast<const float *>(b)[i];
    else return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(b)[i] << 16);
}

template <int DT>
__device__ __forceinline__ void st1(void *b, int64_t i, float v)
{
    if constexpr (DT == BNN_F32) reinterpret_cast<float *>(b)[i] = v;
    else reinterpret_cast<uint16_t *>(b)[i] = f2bf(v);
}

// FAN: x is shared; the thread reads its quad once and writes it to samples blockIdx.y * chunk .. + chunk - 1 (chunk = S when y
// aliases x -- y[0] == x -- so that every copy is written from a value read before any store).
// Otherwise gridDim.y = S, sample s = blockIdx.y, and y may alias x element for element.
template <int DT, bool FAN>
__global__ __launch_bounds__(kDropThreads) void k_mc_dropout(const DropParams P)
{
    const uint32_t ed = rng_epoch_dev(P.rng);
    const uint32_t nq = (P.n + 3u) >> 2;
    const bool contig = P.ldx == (int64_t)P.F && P.ldy == (int64_t)P.F;
    const int s0 = FAN ? (int)blockIdx.y * P.chunk : (int)blockIdx.y;
    const int s1 = FAN ? (s0 + P.chunk < P.S ? s0 + P.chunk : P.S) : s0 + 1;
    const char *xs = reinterpret_cast<const char *>(P.x) + (FAN ? 0 : (int64_t)s0 * P.x_sample_stride * (DT == BNN_F32 ? 4 : 2));
    for (uint32_t q = blockIdx.x * kDropThreads + threadIdx.x; q < nq; q += gridDim.x * kDropThreads) {
        int64_t xo[4], yo[4];
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t e = 4u * q + (uint32_t)j;
            if (contig) { xo[j] = e; yo[j] = e; }
            else {
                const uint32_t r = e / P.F, f = e - r * P.F;
                xo[j] = (int64_t)r * P.ldx + f;
                yo[j] = (int64_t)r * P.ldy + f;
            }
            v[j] = e < P.n ? ld1<DT>(xs, xo[j]) : 0.f;
        }
        for (int s = s0; s < s1; ++s) {
            const float4 u = drop_u4(P.rng, ed, q, P.rng.sample0 + (uint32_t)s);
            const float uu[4] = {u.x, u.y, u.z, u.w};
            char *ys = reinterpret_cast<char *>(P.y) + (int64_t)s * P.y_sample_stride * (DT == BNN_F32 ? 4 : 2);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4u * q + (uint32_t)j < P.n) st1<DT>(ys, yo[j], drop_apply(v[j], uu[j], P.p, P.scale));
        }
    }
}

// gx = mask (.) gy * scale (fp32, contiguous rows).  SUM: gx (rows, F) = sum over s = 0 .. S - 1 in that order, fp32.
template <bool SUM>
__global__ __launch_bounds__(kDropThreads) void k_mc_dropout_bwd(const float *__restrict__ gy, int64_t gy_ss,
                                                                 float *__restrict__ gx, int64_t gx_ss, uint32_t n, int S,
                                                                 float p, float scale, RngDev rng)
{
    const uint32_t ed = rng_epoch_dev(rng);
    const uint32_t nq = (n + 3u) >> 2;
    const int s0 = SUM ? 0 : (int)blockIdx.y;
    const int s1 = SUM ? S : s0 + 1;
    for (uint32_t q = blockIdx.x * kDropThreads + threadIdx.x; q < nq; q += gridDim.x * kDropThreads) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int s = s0; s < s1; ++s) {
            const float4 u = drop_u4(rng, ed, q, rng.sample0 + (uint32_t)s);
            const float uu[4] = {u.x, u.y, u.z, u.w};
            const float *g = gy + (int64_t)s * gy_ss;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t e = 4u * q + (uint32_t)j;
                if (e < n) acc[j] += drop_apply(g[e], uu[j], p, scale);
            }
        }
        float *o = gx + (SUM ? 0 : (int64_t)s0 * gx_ss);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t e = 4u * q + (uint32_t)j;
            if (e < n) o[e] = acc[j];
        }
    }
}

static inline float drop_scale(float p) { return p < 1.f ? 1.f / (1.f - p) : 0.f; }

static inline unsigned drop_grid(uint32_t n)
{
    int64_t b = ((int64_t)n + 4 * kDropThreads - 1) / (4 * kDropThreads);
    if (b < 1) b = 1;
    if (b > kDropMaxBlocks) b = kDropMaxBlocks;
    return (unsigned)b;
}

// shared checks of the mask entries: p, sample count, extent, key
int check_dropout_args(const char *who, int64_t rows, int64_t F, int nsamples, float p, const bnn_rng_t *rng)
{
    if (!rng) { set_error("%s: NULL rng", who); return BNN_E_NULL; }
    if (!(p >= 0.f && p <= 1.f)) { set_error("%s: dropout probability has to be between 0 and 1", who); return BNN_E_RANGE; }
    if (rows < 0 || F < 1 || nsamples < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (nsamples > 0xFFFF) { set_error("%s: more than 65535 samples", who); return BNN_E_RANGE; }
    if (rows * F >= ((int64_t)1 << 32) || F > 0x7FFFFFFF) { set_error("%s: one sample has 2^32 elements or more", who); return BNN_E_RANGE; }
    const int rc = check_rng(rng, nsamples);
    if (rc) { set_error("%s: bad rng", who); return rc; }
    return BNN_OK;
}

// the forward launch with row pitches (callers have checked the arguments); fan: x shared, y[s] for every sample
int mc_dropout_launch(const char *who, const void *x, int64_t x_sample_stride, int64_t ldx, void *y, int64_t y_sample_stride,
                      int64_t ldy, int64_t rows, int64_t F, int nsamples, bool fan, float p, int dtype, const bnn_rng_t *rng,
                      hipStream_t st)
{
    if (rows == 0) return BNN_OK;
    DropParams P{};
    P.x = x; P.x_sample_stride = x_sample_stride; P.ldx = ldx;
    P.y = y; P.y_sample_stride = y_sample_stride; P.ldy = ldy;
    P.F = (uint32_t)F; P.n = (uint32_t)(rows * F); P.S = nsamples;
    P.p = p; P.scale = drop_scale(p);
    P.rng = make_rng(rng);
    // fan-out: the samples are split over gridDim.y until there are ~2048 workgroups (the Titanic layer, 1024 x 256 x 100 samples:
    // 256 workgroups each writing 100 samples otherwise) -- unless y aliases x, where one thread must write every copy
    const unsigned gx = drop_grid(P.n);
    unsigned gy = fan ? 1u : (unsigned)nsamples;
    P.chunk = nsamples;
    if (fan && y != x) {
        int64_t parts = 2048 / (int64_t)gx;
        if (parts > nsamples) parts = nsamples;
        if (parts < 1) parts = 1;
        P.chunk = (int32_t)((nsamples + parts - 1) / parts);
        gy = (unsigned)((nsamples + P.chunk - 1) / P.chunk);
    }
    const dim3 g(gx, gy), b(kDropThreads);
    if (dtype == BNN_F32) {
        if (fan) hipLaunchKernelGGL((k_mc_dropout<BNN_F32, true>), g, b, 0, st, P);
        else hipLaunchKernelGGL((k_mc_dropout<BNN_F32, false>), g, b, 0, st, P);
    } else {
        if (fan) hipLaunchKernelGGL((k_mc_dropout<BNN_BF16, true>), g, b, 0, st, P);
        else hipLaunchKernelGGL((k_mc_dropout<BNN_BF16, false>), g, b, 0, st, P);
    }
    return check_launch(who);
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_mc_dropout(const void *x, int64_t x_sample_stride, void *y, int64_t y_sample_stride, int64_t rows, int64_t features,
                   int nsamples, float p, int dtype, const bnn_rng_t *rng, void *stream)
{
    const char *who = "bnn_mc_dropout";
    if (!x || !y) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    int rc = check_dropout_args(who, rows, features, nsamples, p, rng);
    if (rc) return rc;
    if (dtype != BNN_F32 && dtype != BNN_BF16) { set_error("%s: dtype must be BNN_F32 or BNN_BF16", who); return BNN_E_DTYPE; }
    const int64_t n = rows * features;
    if (x_sample_stride < 0 || (x_sample_stride != 0 && x_sample_stride < n) || (nsamples > 1 && y_sample_stride < n) || y_sample_stride < 0) {
        set_error("%s: bad sample stride", who);
        return BNN_E_SHAPE;
    }
    const uintptr_t am = dtype == BNN_F32 ? 3u : 1u;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & am) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    return mc_dropout_launch(who, x, x_sample_stride, features, y, y_sample_stride, features, rows, features, nsamples,
                             x_sample_stride == 0, p, dtype, rng, (hipStream_t)stream);
}

int bnn_mc_dropout_backward(const float *gy, int64_t gy_sample_stride, float *gx, int64_t gx_sample_stride, int64_t rows,
                            int64_t features, int nsamples, float p, int sum_samples, const bnn_rng_t *rng, void *stream)
{
    const char *who = "bnn_mc_dropout_backward";
    if (!gy || !gx) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    int rc = check_dropout_args(who, rows, features, nsamples, p, rng);
    if (rc) return rc;
    const int64_t n = rows * features;
    if ((nsamples > 1 && gy_sample_stride < n) || gy_sample_stride < 0 || (!sum_samples && nsamples > 1 && gx_sample_stride < n) || gx_sample_stride < 0) {
        set_error("%s: bad sample stride", who);
        return BNN_E_SHAPE;
    }
    if ((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(gx)) & 3u) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    if (n == 0) return BNN_OK;
    const float scale = drop_scale(p);
    const RngDev rd = make_rng(rng);
    const dim3 g(drop_grid((uint32_t)n), sum_samples ? 1u : (unsigned)nsamples), b(kDropThreads);
    hipStream_t st = (hipStream_t)stream;
    if (sum_samples) hipLaunchKernelGGL((k_mc_dropout_bwd<true>), g, b, 0, st, gy, gy_sample_stride, gx, gx_sample_stride, (uint32_t)n, nsamples, p, scale, rd);
    else hipLaunchKernelGGL((k_mc_dropout_bwd<false>), g, b, 0, st, gy, gy_sample_stride, gx, gx_sample_stride, (uint32_t)n, nsamples, p, scale, rd);
    return check_launch(who);
}

}  // extern "C"
