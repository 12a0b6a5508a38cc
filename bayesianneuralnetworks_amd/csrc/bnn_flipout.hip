// bnn_flipout.hip -- Flipout on the MC-batched path: the keyed signs of the RNG contract's sign part (include/bnn_hip.h) written
// out as +-1 rows (the fp32 mode, the training paths, the 1-d / 3-d layers), and the backward of the sign-outer-product draw
// (bnn_draw_multi kind BNN_DRAW_FLIPOUT) with the signs re-created from the key.  The fused bf16 conv makes its signs itself (bnn_dense.hip).
#include "bnn_device.hpp"

namespace bnn {

constexpr int kFlipThreads = 256;
constexpr int kFlipMaxBlocks = 4096;

// one thread per quad of 4 consecutive elements of a sample's r * width + j index, blockIdx.y = sample
__global__ __launch_bounds__(kFlipThreads) void k_flipout_signs(float *__restrict__ out, int64_t out_ss, uint32_t n, RngDev rng)
{
    const uint32_t ed = rng_epoch_dev(rng);
    const uint32_t nq = (n + 3u) >> 2;
    const uint32_t s = blockIdx.y;
    float *o = out + (int64_t)s * out_ss;
    for (uint32_t q = blockIdx.x * kFlipThreads + threadIdx.x; q < nq; q += gridDim.x * kFlipThreads) {
        const float4 u = drop_u4(rng, ed, q, rng.sample0 + s);
        const float uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4u * q + (uint32_t)j < n) o[4u * q + (uint32_t)j] = flip_sign(uu[j]);
    }
}

// g_mu = sum_s g_w[s], g_rho = sum_s g_w[s] R_s[o] S_s[k] sigmoid(rho): one thread per weight, samples in order
__global__ __launch_bounds__(kFlipThreads) void k_flipout_weight_bwd(const float *__restrict__ g_w, int64_t g_ss,
                                                                    const float *__restrict__ rho, float *__restrict__ g_mu,
                                                                    float *__restrict__ g_rho, uint32_t O, uint32_t K, int S,
                                                                    RngDev rng)
{
    const uint32_t ed = rng_epoch_dev(rng);
    const uint64_t n = (uint64_t)O * K;
    for (uint64_t i = (uint64_t)blockIdx.x * kFlipThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFlipThreads) {
        const uint32_t o = (uint32_t)(i / K), k = (uint32_t)(i - (uint64_t)o * K);
        float am = 0.f, ar = 0.f;
        for (int s = 0; s < S; ++s) {
            const uint32_t smp = rng.sample0 + (uint32_t)s;
            const float e = flip_sign(drop_u1(rng, ed, o, smp)) * flip_sign(drop_u1(rng, ed, O + k, smp));
            const float g = g_w[(int64_t)s * g_ss + (int64_t)i];
            am += g;
            ar = fmaf(g, e, ar);
        }
        g_mu[i] = am;
        g_rho[i] = ar * dsoftplus(rho[i]);
    }
}

static inline unsigned flip_grid(int64_t items)
{
    int64_t b = (items + kFlipThreads - 1) / kFlipThreads;
    if (b < 1) b = 1;
    if (b > kFlipMaxBlocks) b = kFlipMaxBlocks;
    return (unsigned)b;
}

int check_flip_args(const char *who, int64_t rows, int64_t width, int nsamples, const bnn_rng_t *rng)
{
    if (!rng) { set_error("%s: NULL rng", who); return BNN_E_NULL; }
    if (rows < 0 || width < 1 || nsamples < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    if (nsamples > 0xFFFF) { set_error("%s: more than 65535 samples", who); return BNN_E_RANGE; }
    if (rows * width >= ((int64_t)1 << 32) || width > 0x7FFFFFFF) { set_error("%s: one sample has 2^32 signs or more", who); return BNN_E_RANGE; }
    const int rc = check_rng(rng, nsamples);
    if (rc) { set_error("%s: bad rng", who); return rc; }
    return BNN_OK;
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_flipout_signs(float *out, int64_t out_sample_stride, int64_t rows, int64_t width, int nsamples, const bnn_rng_t *rng,
                      void *stream)
{
    const char *who = "bnn_flipout_signs";
    if (!out) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    int rc = check_flip_args(who, rows, width, nsamples, rng);
    if (rc) return rc;
    const int64_t n = rows * width;
    if (out_sample_stride < 0 || (nsamples > 1 && out_sample_stride < n)) { set_error("%s: bad sample stride", who); return BNN_E_SHAPE; }
    if (reinterpret_cast<uintptr_t>(out) & 3u) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    if (n == 0) return BNN_OK;
    hipLaunchKernelGGL(k_flipout_signs, dim3(flip_grid((n + 3) / 4), (unsigned)nsamples), dim3(kFlipThreads), 0, (hipStream_t)stream,
                       out, out_sample_stride, (uint32_t)n, make_rng(rng));
    return check_launch(who);
}

int bnn_flipout_weight_backward(const float *g_w, int64_t g_w_sample_stride, const float *rho, float *g_mu, float *g_rho,
                                int64_t O, int64_t K, int nsamples, const bnn_rng_t *rng, void *stream)
{
    const char *who = "bnn_flipout_weight_backward";
    if (!g_w || !rho || !g_mu || !g_rho) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (O < 1 || K < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    int rc = check_flip_args(who, 1, O + K, nsamples, rng);
    if (rc) return rc;
    if (g_w_sample_stride < 0 || (nsamples > 1 && g_w_sample_stride < O * K)) { set_error("%s: bad sample stride", who); return BNN_E_SHAPE; }
    if ((reinterpret_cast<uintptr_t>(g_w) | reinterpret_cast<uintptr_t>(rho) | reinterpret_cast<uintptr_t>(g_mu) |
         reinterpret_cast<uintptr_t>(g_rho)) & 3u) { set_error("%s: misaligned pointer", who); return BNN_E_ALIGN; }
    hipLaunchKernelGGL(k_flipout_weight_bwd, dim3(flip_grid(O * K)), dim3(kFlipThreads), 0, (hipStream_t)stream,
                       g_w, g_w_sample_stride, rho, g_mu, g_rho, (uint32_t)O, (uint32_t)K, nsamples, make_rng(rng));
    return check_launch(who);
}

}  // extern "C"
