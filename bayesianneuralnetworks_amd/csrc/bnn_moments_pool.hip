// bnn_moments_pool.hip -- K20: moments through pooling and eval-mode BatchNorm, so that the sampling-free pass (K16 .. K19) does
// not stop at the first pooling layer behind a Bayesian one.  Elements are independent Gaussians, as everywhere in the pass.
//
// k_moments_pool3d<MAX>: a window is folded pairwise with the moment-matched maximum of two Gaussians (moments_max_step,
//   bnn_moments_act.hpp; Clark 1961).  The running maximum is treated as a Gaussian again: exact for a window of two, moment
//   matching beyond.  The fold order is part of the contract: window offsets ascending in (depth, height, width), row-major;
//   padded positions are skipped (torch pads max pooling with -inf) and the first valid element starts the fold.  The running
//   (m, v) stays fp64 and is rounded to fp32 once per output.
// k_moments_pool3d<AVG>: mean' = sum m / n, var' = sum v / n^2 over the valid positions, n the window size or
//   (BNN_POOL_FLAG_VALID_DIVISOR) the valid count; fp64 sums in the fold's order, one rounding.  Exact for independent elements.
// One thread per output element, consecutive threads along the output's innermost axis; every load and store is one element
// wide, so operands need element alignment only.  1-d and 2-d pooling are unit depth / height.
//
// k_moments_pool3d_bwd<MAX | AVG>: one thread per output window.  MAX folds the window again and keeps the prefix states of the
//   fold -- fold index j -> (m, v) after j + 1 elements -- in LDS, [j][thread] as 16-byte pairs (a dynamically indexed private
//   array would live in scratch); then it walks the window backwards through moments_max_step_bwd.  Nothing is handed from the
//   forward launch to this one.  The LDS block is (n - 1) x 16 B x threads for a window of n elements: 256 threads up to n = 9,
//   64 threads up to kPoolWindowCap = 64 (63 x 16 x 64 = 64512 B, under the 64 KiB a launch may ask for), which is where the cap on
//   a window comes from.
//   The input gradients are zeroed on the stream first (inputs no window covers get 0) by a launch of the library's own,
//   k_pool_zero -- a memset node replayed from a captured graph left other values there on the MI355X --, unless the windows tile
//   the input exactly (kernel = stride, no padding, no dilation, no remainder), where every element is written once anyway.
//   Windows that do not overlap (stride >=
//   dilated extent on every axis) are written with plain stores: identical calls give identical bits.  Overlapping windows add
//   with fp32 vector atomics, whose order is the hardware's: such a gradient can differ between identical calls by the rounding
//   of an fp32 sum of at most prod ceil(extent / stride) addends.
//
// k_moments_batchnorm: eval-mode BatchNorm as the per-channel affine map a = gamma / sqrt(running_var + eps),
//   m' = a (m - running_mean) + beta, v' = a^2 v; a is formed per element in the kernel (fp32).
#include "bnn_device.hpp"
#include "bnn_moments_act.hpp"

namespace bnn {

constexpr int kPoolWindowCap = 64;

struct PoolArgs {
    const float *m, *v;           // (B C, D, H, W)
    float *om, *ov;               // forward: (B C, OD, OH, OW)
    const float *gom, *gov;       // backward: gradients of the outputs
    float *gm, *gv;               // backward: gradients of the inputs
    uint32_t total;               // B C OD OH OW
    int32_t D, H, W, OD, OH, OW;
    int32_t KD, KH, KW, sd, sh, sw, pd, ph, pw, dd, dh, dw;
    int32_t valid_div;            // AVG: divide by the valid count
    int32_t atomic;               // backward: windows overlap
    int32_t tiled;                // backward: the windows tile the input exactly (every input element is written once: no zeros first)
};

enum { POOL_MAX = BNN_POOL_MAX, POOL_AVG = BNN_POOL_AVG };

struct PoolWindow { int64_t base; int32_t d0, h0, w0; };     // the input plane of the output and the window's first position

__device__ __forceinline__ PoolWindow pool_window(const PoolArgs &A, uint32_t o)
{
    const uint32_t ow = o % (uint32_t)A.OW;
    uint32_t t = o / (uint32_t)A.OW;
    const uint32_t oh = t % (uint32_t)A.OH;
    t /= (uint32_t)A.OH;
    const uint32_t od = t % (uint32_t)A.OD;
    const uint32_t bc = t / (uint32_t)A.OD;
    PoolWindow w;
    w.base = (int64_t)bc * A.D * A.H * A.W;
    w.d0 = (int32_t)od * A.sd - A.pd;
    w.h0 = (int32_t)oh * A.sh - A.ph;
    w.w0 = (int32_t)ow * A.sw - A.pw;
    return w;
}

template <int OP>
__global__ __launch_bounds__(256) void k_moments_pool3d(const PoolArgs A)
{
    const uint32_t o = blockIdx.x * 256u + threadIdx.x;
    if (o >= A.total) return;
    const PoolWindow w = pool_window(A, o);
    double rm = 0.0, rv = 0.0;
    int cnt = 0;
    for (int kd = 0; kd < A.KD; ++kd) {
        const int id = w.d0 + kd * A.dd;
        if (id < 0 || id >= A.D) continue;
        for (int kh = 0; kh < A.KH; ++kh) {
            const int ih = w.h0 + kh * A.dh;
            if (ih < 0 || ih >= A.H) continue;
            const int64_t row = w.base + ((int64_t)id * A.H + ih) * A.W;
            for (int kw = 0; kw < A.KW; ++kw) {
                const int iw = w.w0 + kw * A.dw;
                if (iw < 0 || iw >= A.W) continue;
                const double xm = (double)A.m[row + iw], xv = (double)A.v[row + iw];
                if (OP == POOL_AVG) {
                    rm += xm;
                    rv += xv;
                } else if (cnt == 0) {
                    rm = xm;
                    rv = xv;
                } else {
                    moments_max_step(rm, rv, xm, xv);
                }
                ++cnt;
            }
        }
    }
    if (OP == POOL_AVG) {
        const double n = (double)(A.valid_div ? cnt : A.KD * A.KH * A.KW);
        rm /= n;
        rv /= n * n;
    }
    A.om[o] = (float)rm;
    A.ov[o] = (float)rv;
}

__device__ __forceinline__ void pool_grad_out(const PoolArgs &A, int64_t i, float a, float b)
{
    if (A.atomic) {
        unsafeAtomicAdd(A.gm + i, a);
        unsafeAtomicAdd(A.gv + i, b);
    } else {
        A.gm[i] = a;
        A.gv[i] = b;
    }
}

// the input gradients' zeros, as a launch of the library's own (element-wide stores; a captured graph replays it like any kernel)
__global__ __launch_bounds__(256) void k_pool_zero(float *a, float *b, int64_t n)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        a[t] = 0.0f;
        b[t] = 0.0f;
    }
}

// blockDim.x threads; MAX: (window - 1) * blockDim.x double2 of dynamic LDS
template <int OP>
__global__ __launch_bounds__(256) void k_moments_pool3d_bwd(const PoolArgs A)
{
    extern __shared__ double2 pool_states[];
    const uint32_t T = blockDim.x;
    const uint32_t o = blockIdx.x * T + threadIdx.x;
    if (o >= A.total) return;
    const PoolWindow w = pool_window(A, o);
    const int slots = A.KD * A.KH * A.KW - 1;
    double rm = 0.0, rv = 0.0;
    int cnt = 0;
    for (int kd = 0; kd < A.KD; ++kd) {
        const int id = w.d0 + kd * A.dd;
        if (id < 0 || id >= A.D) continue;
        for (int kh = 0; kh < A.KH; ++kh) {
            const int ih = w.h0 + kh * A.dh;
            if (ih < 0 || ih >= A.H) continue;
            const int64_t row = w.base + ((int64_t)id * A.H + ih) * A.W;
            for (int kw = 0; kw < A.KW; ++kw) {
                const int iw = w.w0 + kw * A.dw;
                if (iw < 0 || iw >= A.W) continue;
                if (OP == POOL_MAX) {
                    const double xm = (double)A.m[row + iw], xv = (double)A.v[row + iw];
                    if (cnt == 0) {
                        rm = xm;
                        rv = xv;
                    } else {
                        moments_max_step(rm, rv, xm, xv);
                    }
                    if (cnt < slots) pool_states[(uint32_t)cnt * T + threadIdx.x] = make_double2(rm, rv);
                }
                ++cnt;
            }
        }
    }
    double gm = (double)A.gom[o], gv = (double)A.gov[o];
    if (OP == POOL_AVG) {
        const double n = (double)(A.valid_div ? cnt : slots + 1);
        gm /= n;
        gv /= n * n;
    }
    int j = cnt - 1;                                      // the fold index of the element the walk stands on
    for (int kd = A.KD - 1; kd >= 0; --kd) {
        const int id = w.d0 + kd * A.dd;
        if (id < 0 || id >= A.D) continue;
        for (int kh = A.KH - 1; kh >= 0; --kh) {
            const int ih = w.h0 + kh * A.dh;
            if (ih < 0 || ih >= A.H) continue;
            const int64_t row = w.base + ((int64_t)id * A.H + ih) * A.W;
            for (int kw = A.KW - 1; kw >= 0; --kw) {
                const int iw = w.w0 + kw * A.dw;
                if (iw < 0 || iw >= A.W) continue;
                double g2m = gm, g2v = gv;
                if (OP == POOL_MAX && j > 0) {
                    const double2 prev = pool_states[(uint32_t)(j - 1) * T + threadIdx.x];
                    moments_max_step_bwd(prev.x, prev.y, (double)A.m[row + iw], (double)A.v[row + iw], gm, gv, g2m, g2v);
                }
                pool_grad_out(A, row + iw, (float)g2m, (float)g2v);
                --j;
            }
        }
    }
}

// in place allowed: every element is read before it is written, by its own thread
__global__ __launch_bounds__(256) void k_moments_batchnorm(const float *m, const float *v, const float *gamma, const float *beta,
                                                           const float *rmean, const float *rvar, float eps, float *om, float *ov,
                                                           int64_t n, uint32_t C, uint32_t inner)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        const uint32_t c = ((uint32_t)t / inner) % C;
        const float a = (gamma ? gamma[c] : 1.0f) / sqrtf(rvar[c] + eps);
        om[t] = fmaf(a, m[t] - rmean[c], beta ? beta[c] : 0.0f);
        ov[t] = a * a * v[t];
    }
}

// one axis of the output by torch's floor rule, or -1
static int64_t pool_out_extent(int64_t I, int64_t k, int64_t s, int64_t p, int64_t d)
{
    const int64_t span = I + 2 * p - d * (k - 1) - 1;
    return span < 0 ? -1 : span / s + 1;
}

// does a window of this axis lie in the padding alone?  Only windows that touch an edge can: at most p + 1 at either end.
static bool pool_axis_has_empty_window(int64_t I, int64_t O, int64_t k, int64_t s, int64_t p, int64_t d)
{
    for (int pass = 0; pass < 2; ++pass) {
        const int64_t lo = pass == 0 ? 0 : (O - p - 1 > 0 ? O - p - 1 : 0), hi = pass == 0 ? (p + 1 < O ? p + 1 : O) : O;
        for (int64_t o = lo; o < hi; ++o) {
            bool any = false;
            for (int64_t j = 0; j < k && !any; ++j) {
                const int64_t i = o * s - p + j * d;
                any = i >= 0 && i < I;
            }
            if (!any) return true;
        }
    }
    return false;
}

// the checks both pooling entries share; fills A's geometry
static int pool_check(const char *who, const bnn_pool3d_shape_t *sh, int op, int flags, PoolArgs &A)
{
    const int64_t I[3] = {sh->D, sh->H, sh->W}, k[3] = {sh->KD, sh->KH, sh->KW}, s[3] = {sh->stride_d, sh->stride_h, sh->stride_w};
    const int64_t p[3] = {sh->pad_d, sh->pad_h, sh->pad_w}, d[3] = {sh->dil_d, sh->dil_h, sh->dil_w};
    const int64_t lim = (int64_t)1 << 31;
    if (sh->B < 1 || sh->C < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    int64_t O[3];
    for (int a = 0; a < 3; ++a) {
        if (I[a] < 1 || k[a] < 1 || s[a] < 1 || d[a] < 1 || p[a] < 0) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
        if (I[a] >= lim || k[a] >= lim || s[a] >= lim || d[a] >= lim || p[a] >= lim) {
            set_error("%s: an extent of 2^31 or more", who);
            return BNN_E_RANGE;
        }
        O[a] = pool_out_extent(I[a], k[a], s[a], p[a], d[a]);
        if (O[a] < 1) { set_error("%s: empty output (the window is larger than the padded input)", who); return BNN_E_SHAPE; }
    }
    for (int a = 0; a < 3; ++a)
        if (2 * p[a] > k[a]) { set_error("%s: padding above half the kernel", who); return BNN_E_RANGE; }
    if (k[0] > kPoolWindowCap || k[1] > kPoolWindowCap || k[2] > kPoolWindowCap || k[0] * k[1] * k[2] > kPoolWindowCap) {
        set_error("%s: a window of more than %d elements", who, kPoolWindowCap);
        return BNN_E_RANGE;
    }
    if (sh->B >= 2 * lim || sh->C >= 2 * lim) { set_error("%s: 2^32 elements or more", who); return BNN_E_RANGE; }
    uint64_t n_in = (uint64_t)sh->B, n_out = (uint64_t)sh->B;
    const uint64_t top = (uint64_t)1 << 32;
    const uint64_t fin[4] = {(uint64_t)sh->C, (uint64_t)I[0], (uint64_t)I[1], (uint64_t)I[2]};
    const uint64_t fout[4] = {(uint64_t)sh->C, (uint64_t)O[0], (uint64_t)O[1], (uint64_t)O[2]};
    for (int a = 0; a < 4; ++a) {
        n_in *= fin[a];
        n_out *= fout[a];
        if (n_in >= top || n_out >= top) { set_error("%s: 2^32 elements or more", who); return BNN_E_RANGE; }
    }
    for (int a = 0; a < 3; ++a)
        if (pool_axis_has_empty_window(I[a], O[a], k[a], s[a], p[a], d[a])) {
            set_error("%s: a window lies in the padding alone", who);
            return BNN_E_RANGE;
        }
    if (op != BNN_POOL_MAX && op != BNN_POOL_AVG) { set_error("%s: unknown op", who); return BNN_E_UNSUPPORTED; }
    if (flags & ~BNN_POOL_FLAG_VALID_DIVISOR) { set_error("%s: unknown flag", who); return BNN_E_UNSUPPORTED; }
    A.total = (uint32_t)n_out;
    A.D = (int32_t)I[0]; A.H = (int32_t)I[1]; A.W = (int32_t)I[2];
    A.OD = (int32_t)O[0]; A.OH = (int32_t)O[1]; A.OW = (int32_t)O[2];
    A.KD = (int32_t)k[0]; A.KH = (int32_t)k[1]; A.KW = (int32_t)k[2];
    A.sd = (int32_t)s[0]; A.sh = (int32_t)s[1]; A.sw = (int32_t)s[2];
    A.pd = (int32_t)p[0]; A.ph = (int32_t)p[1]; A.pw = (int32_t)p[2];
    A.dd = (int32_t)d[0]; A.dh = (int32_t)d[1]; A.dw = (int32_t)d[2];
    A.valid_div = (flags & BNN_POOL_FLAG_VALID_DIVISOR) ? 1 : 0;
    A.atomic = 0;
    A.tiled = 1;
    for (int a = 0; a < 3; ++a) {
        const int64_t ext = d[a] * (k[a] - 1) + 1;
        if (s[a] < ext) A.atomic = 1;
        if (s[a] != ext || ext != k[a] || p[a] != 0 || O[a] * s[a] != I[a]) A.tiled = 0;
    }
    return BNN_OK;
}

}  // namespace bnn

using namespace bnn;

extern "C" {

int bnn_moments_pool3d_forward(const float *m, const float *v, float *out_m, float *out_v, const bnn_pool3d_shape_t *shape, int op,
                               int flags, void *stream)
{
    const char *who = "bnn_moments_pool3d_forward";
    if (!m || !v || !out_m || !out_v || !shape) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    PoolArgs A{};
    const int rc = pool_check(who, shape, op, flags, A);
    if (rc) return rc;
    if (misaligned(m, 3) || misaligned(v, 3) || misaligned(out_m, 3) || misaligned(out_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    A.m = m; A.v = v; A.om = out_m; A.ov = out_v;
    const dim3 g((A.total + 255u) / 256u), b(256);
    if (op == BNN_POOL_MAX) hipLaunchKernelGGL(k_moments_pool3d<POOL_MAX>, g, b, 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(k_moments_pool3d<POOL_AVG>, g, b, 0, (hipStream_t)stream, A);
    return check_launch(who);
}

int bnn_moments_pool3d_backward(const float *m, const float *v, const float *g_out_m, const float *g_out_v, float *g_m, float *g_v,
                                const bnn_pool3d_shape_t *shape, int op, int flags, void *stream)
{
    const char *who = "bnn_moments_pool3d_backward";
    if (!m || !v || !g_out_m || !g_out_v || !g_m || !g_v || !shape) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    PoolArgs A{};
    const int rc = pool_check(who, shape, op, flags, A);
    if (rc) return rc;
    if (misaligned(m, 3) || misaligned(v, 3) || misaligned(g_out_m, 3) || misaligned(g_out_v, 3) || misaligned(g_m, 3) ||
        misaligned(g_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    A.m = m; A.v = v; A.gom = g_out_m; A.gov = g_out_v; A.gm = g_m; A.gv = g_v;
    hipStream_t st = (hipStream_t)stream;
    if (!A.tiled) {
        const int64_t n_in = shape->B * shape->C * (int64_t)A.D * A.H * A.W;
        int64_t zb = (n_in + 255) / 256;
        if (zb > 4096) zb = 4096;
        hipLaunchKernelGGL(k_pool_zero, dim3((unsigned)zb), dim3(256), 0, st, g_m, g_v, n_in);
        const int rz = check_launch(who);
        if (rz) return rz;
    }
    const int window = A.KD * A.KH * A.KW;
    const unsigned threads = (op == BNN_POOL_AVG || window <= 9) ? 256u : 64u;
    const size_t lds = op == BNN_POOL_MAX ? (size_t)(window - 1) * threads * sizeof(double2) : 0;
    const dim3 g((A.total + threads - 1u) / threads), b(threads);
    if (op == BNN_POOL_MAX) hipLaunchKernelGGL(k_moments_pool3d_bwd<POOL_MAX>, g, b, lds, st, A);
    else hipLaunchKernelGGL(k_moments_pool3d_bwd<POOL_AVG>, g, b, lds, st, A);
    return check_launch(who);
}

int bnn_moments_batchnorm(const float *m, const float *v, const float *gamma, const float *beta, const float *running_mean,
                          const float *running_var, float eps, float *out_m, float *out_v, int64_t B, int64_t C, int64_t inner,
                          void *stream)
{
    const char *who = "bnn_moments_batchnorm";
    if (!m || !v || !running_mean || !running_var || !out_m || !out_v) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if (B < 1 || C < 1 || inner < 1) { set_error("%s: bad extent", who); return BNN_E_SHAPE; }
    const uint64_t top = (uint64_t)1 << 32;
    if ((uint64_t)B >= top || (uint64_t)C >= top || (uint64_t)inner >= top || (uint64_t)B * (uint64_t)C >= top ||
        (uint64_t)B * (uint64_t)C * (uint64_t)inner >= top) {
        set_error("%s: 2^32 elements or more", who);
        return BNN_E_RANGE;
    }
    if (!(eps >= 0.0f) || eps > 3.0e38f) { set_error("%s: eps must be finite and >= 0", who); return BNN_E_RANGE; }
    if (misaligned(m, 3) || misaligned(v, 3) || misaligned(gamma, 3) || misaligned(beta, 3) || misaligned(running_mean, 3) ||
        misaligned(running_var, 3) || misaligned(out_m, 3) || misaligned(out_v, 3)) {
        set_error("%s: misaligned pointer", who);
        return BNN_E_ALIGN;
    }
    const int64_t n = B * C * inner;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_moments_batchnorm, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m, v, gamma, beta, running_mean,
                       running_var, eps, out_m, out_v, n, (uint32_t)C, (uint32_t)inner);
    return check_launch(who);
}

}  // extern "C"
