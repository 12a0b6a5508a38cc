// bnn_moments_dropout.hip -- K22: MC dropout in a moment pass, folded through the activation behind it.  The layer's output is
// y = f(b z / q) = b f(z / q) for z ~ N(m, v), b ~ Bernoulli(q), q = 1 - p and f(0) = 0 (identity, ReLU, ELU), so with (M, V) the
// moments of f at N(m / q, v / q^2)
//     mean' = q M,    var' = q V + q p M^2
// exactly -- a dropped unit is a spike at zero, not a Gaussian, and the activation sees the spike (moments_dropout_dev,
// bnn_moments_act.hpp, on moments_relu_dev / moments_elu_dev).  Backward: moments_dropout_bwd_dev on the activations' own
// backwards.  Elementwise, one element per thread iteration, scalar loads (any element alignment), in place allowed: every
// element is read before it is written, by its own thread.  ACT is a template argument: the identity and the ReLU keep their
// fp32 register footprint, only the ELU instantiation pays the fp64 evaluation.
#include "bnn_moments_act.hpp"

namespace bnn {

template <int ACT>
__global__ __launch_bounds__(256) void k_moments_dropout(const float *m, const float *v, float *om, float *ov, int64_t n, float p,
                                                         float alpha)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        float a, b;
        moments_dropout_dev(m[t], v ? v[t] : 0.0f, p, ACT, alpha, a, b);
        om[t] = a;
        ov[t] = b;
    }
}

// g_v may be NULL with a deterministic input (v NULL): the variance's gradient has nowhere to go
template <int ACT>
__global__ __launch_bounds__(256) void k_moments_dropout_bwd(const float *m, const float *v, const float *gom, const float *gov,
                                                             float *gm, float *gv, int64_t n, float p, float alpha)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        float a, b;
        moments_dropout_bwd_dev(m[t], v ? v[t] : 0.0f, p, ACT, alpha, gom[t], gov[t], a, b);
        gm[t] = a;
        if (gv) gv[t] = b;
    }
}

static int dropout_check(const char *who, int64_t n, float p, int act, float alpha)
{
    if (n < 0) { set_error("%s: n must be >= 0", who); return BNN_E_RANGE; }
    if (!(p >= 0.0f && p <= 1.0f)) { set_error("%s: p must lie in [0, 1]", who); return BNN_E_RANGE; }
    if (act != 0 && act != BNN_FLAG_RELU && act != BNN_FLAG_ELU) {
        set_error("%s: act must be 0, BNN_FLAG_RELU or BNN_FLAG_ELU", who);
        return BNN_E_RANGE;
    }
    if (act == BNN_FLAG_ELU && (!(alpha >= 0.0f) || alpha > 3.0e38f)) {
        set_error("%s: alpha must be finite and >= 0", who);
        return BNN_E_RANGE;
    }
    return BNN_OK;
}

static unsigned dropout_blocks(int64_t n)
{
    const int64_t blocks = (n + 255) / 256;
    return (unsigned)(blocks > 4096 ? 4096 : blocks);
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_moments_dropout(const float *m, const float *v, float *out_m, float *out_v, int64_t n, float p, int act, float alpha,
                        void *stream)
{
    const char *who = "bnn_moments_dropout";
    if (!m || !out_m || !out_v) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    const int rc = dropout_check(who, n, p, act, alpha);
    if (rc) return rc;
    if (misaligned(m, 3) || misaligned(v, 3) || misaligned(out_m, 3) || misaligned(out_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (n == 0) return BNN_OK;
    const dim3 g(dropout_blocks(n)), b(256);
    hipStream_t st = (hipStream_t)stream;
    if (act == BNN_FLAG_ELU) hipLaunchKernelGGL((k_moments_dropout<BNN_FLAG_ELU>), g, b, 0, st, m, v, out_m, out_v, n, p, alpha);
    else if (act == BNN_FLAG_RELU) hipLaunchKernelGGL((k_moments_dropout<BNN_FLAG_RELU>), g, b, 0, st, m, v, out_m, out_v, n, p, alpha);
    else hipLaunchKernelGGL((k_moments_dropout<0>), g, b, 0, st, m, v, out_m, out_v, n, p, alpha);
    return check_launch(who);
}

int bnn_moments_dropout_backward(const float *m, const float *v, const float *g_out_m, const float *g_out_v, float *g_m, float *g_v,
                                 int64_t n, float p, int act, float alpha, void *stream)
{
    const char *who = "bnn_moments_dropout_backward";
    if (!m || !g_out_m || !g_out_v || !g_m || (v && !g_v)) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    const int rc = dropout_check(who, n, p, act, alpha);
    if (rc) return rc;
    if (misaligned(m, 3) || misaligned(v, 3) || misaligned(g_out_m, 3) || misaligned(g_out_v, 3) || misaligned(g_m, 3) ||
        misaligned(g_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    if (n == 0) return BNN_OK;
    const dim3 g(dropout_blocks(n)), b(256);
    hipStream_t st = (hipStream_t)stream;
    if (act == BNN_FLAG_ELU)
        hipLaunchKernelGGL((k_moments_dropout_bwd<BNN_FLAG_ELU>), g, b, 0, st, m, v, g_out_m, g_out_v, g_m, g_v, n, p, alpha);
    else if (act == BNN_FLAG_RELU)
        hipLaunchKernelGGL((k_moments_dropout_bwd<BNN_FLAG_RELU>), g, b, 0, st, m, v, g_out_m, g_out_v, g_m, g_v, n, p, alpha);
    else
        hipLaunchKernelGGL((k_moments_dropout_bwd<0>), g, b, 0, st, m, v, g_out_m, g_out_v, g_m, g_v, n, p, alpha);
    return check_launch(who);
}

}  // extern "C"
