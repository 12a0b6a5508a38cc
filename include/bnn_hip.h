/*
 * bnn_hip.h -- C-ABI of libbnn_hip.so, the MI355X (gfx950) variational-layer engine.
 *
 * The reference (Mirko-Nava/BayesianNeuralNetworks, pytorch_bayesian 0.0.4) is
 * pure Python and has NO FFI: its hot path is a sequence of stock torch calls.
 * Each entry point below therefore replaces a reference *Python call site*; the
 * citation after "replaces" is that site, relative to /root/reference/.
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless the
 *     parameter is documented "host"; no allocation and no synchronisation inside
 *     (every call is legal during hipGraph / torch.cuda.graph capture);
 *   - `stream` is a hipStream_t passed as void*;
 *   - return value: 0 = success, <0 = BNN_E_* argument error (nothing launched),
 *     >0 = the hipError_t of a failed launch; bnn_last_error() gives the text;
 *   - tensors are dense row-major fp32 unless a dtype argument says otherwise.
 *
 * RNG contract (production eps source; its CPU twin is oracle/bnn_oracle.c, orc_eps4)
 *   eps for element e of tensor-stream `stream`, MC sample `sample`:
 *     (x0..x3) = Philox4x32-10(counter = (e / 4, (stream << 16) | sample,
 *                                         epoch_host, epoch_dev),
 *                              key     = (seed & 0xffffffff, seed >> 32))
 *     u  = ((x >> 8) + 0.5) * 2^-24
 *     z0 = r(u0) cos(2 pi u1), z1 = r(u0) sin(2 pi u1), z2, z3 likewise from x2, x3,
 *     r(u) = sqrt(-2 ln u);   eps[e] = z[e % 4].
 *   epoch_dev is read from device memory (*rng->epoch_dev + rng->epoch_dev_delta) so
 *   that a replayed graph draws fresh noise: bnn_rng_advance bumps it in-stream.
 *   The draw depends only on (seed, stream, sample, epochs, e): not on tiling,
 *   grid size, or the number of GPUs the MC samples are sharded over.
 *
 *   rng->generator selects the eps source (part of the key: every kernel that re-creates a draw -- the draw launch, the
 *   fused GEMM, the standalone sampler, the backward -- reads it from the same struct, so a draw is the same everywhere):
 *     BNN_GEN_PHILOX10_U24 (0, default): the stream above -- 24-bit uniforms, four eps per Philox4x32-10 block.
 *     BNN_GEN_PHILOX7_U16  (1): EIGHT eps per Philox4x32-7 block, from 16-bit uniforms -- for weights that are rounded to
 *       bf16 (8 significand bits) anyway; 0.4 x the integer work per eps (the draw launch of the BASELINE net: 16.5 -> 13.3 us):
 *         (x0..x3) = Philox4x32-7(counter = (e / 8, (stream << 16) | sample, epoch_host, epoch_dev), key as above)
 *         word x_k feeds elements 8 (e / 8) + 2 k and + 2 k + 1:  ua = ((x_k & 0xffff) + 0.5) 2^-16,  ub = ((x_k >> 16) + 0.5) 2^-16,
 *         z_even = r(ua) cos(2 pi ub), z_odd = r(ua) sin(2 pi ub);  |eps| <= r(2^-17) = 4.86.
 *       Philox4x32-7 is the 7-round member of the same family (Random123's kat_vectors hold its known answers, checked in
 *       tests/test_oracle_golden.py); CPU twin: orc_eps_fill_gen.
 *
 * Dropout-mask contract (MC dropout on the MC-batched path: bnn_mc_dropout, bnn_dense_forward_dropout, their backward)
 *   A mask is a keyed draw like eps, on the same bnn_rng_t fields -- seed, stream, sample, epoch_host, epoch_dev, generator -- from the
 *   UNIFORMS above, before Box-Muller.  Element index e = r * F + f: row r within the sample, F features per row (N of a
 *   linear, C * H * W of a conv).
 *     BNN_GEN_PHILOX10_U24: u = word e % 4 of block e / 4 (the counter above, block = e / 4), u = ((x >> 8) + 0.5) * 2^-24
 *                           rounded once to fp32 (it can round up to 1.0);
 *     BNN_GEN_PHILOX7_U16:  word k of block e / 8: its low half for element 8 (e / 8) + 2 k, its high half for + 2 k + 1,
 *                           u = (h + 0.5) * 2^-16.
 *   The element is DROPPED iff u < p (p as fp32), or p == 1 (every element).  A kept element is multiplied by
 *   scale = 1 / (1 - p), computed in fp32: y = x * scale, one rounding.  p = 0 is the identity.
 *   The mask depends only on the key and (sample, r, f): not on tiling, grid, fusion or dtype -- every kernel that applies or
 *   re-creates it uses one device function (drop_u4), so the fused and the standalone mask are the same bit for bit.
 *   rows * F < 2^32 per sample.  CPU twin: tests/test_mc_dropout.py (mask_twin), on the oracle's Philox.
 *
 * Flipout-sign contract (Flipout layers on the MC-batched path: bnn_flipout_signs, bnn_conv2d_flipout_forward_mc, bnn_draw_multi
 * BNN_DRAW_FLIPOUT, bnn_flipout_weight_backward)
 *   A Flipout sign is a keyed draw on the same UNIFORMS as the dropout mask above (same fields, both generators, before
 *   Box-Muller), one stream per layer, sample sample0 + s.  The sign of uniform u is -1 iff u < 0.5, +1 otherwise: the
 *   reference's (rand - .5).sign().  A 16-bit uniform is never 0.5; a 24-bit one is 0.5 when ((x >> 8) + 0.5) 2^-24 rounds to it
 *   (x >> 8 = 2^23), and that gives +1 -- so no sign is ever 0.  Element layout within one sample:
 *     conv (B images, O output and C input channels): e = b (O + C) + j; j < O is R[b][j], the rest is S[b][j - O];
 *     linear (O x K weight): one row of O + K elements, R = v[0 : O], S = v[O : O + K], eps[o][k] = R[o] S[k].
 *   rows (O + C) < 2^32 per sample.  Every kernel computes a sign with one device function (flip_sign on drop_u4).
 *   CPU twin: tests/test_flipout_mc.py (sign_twin), on the oracle's Philox.
 *
 * MVN-noise contract (the full-covariance posterior on the MC-batched path: bnn_mvn_draw, bnn_mvn_draw_backward)
 *   The reference draws UNIFORM noise for WeightMultivariateNormal (torch.rand_like, pytorch_bayesian/nn/core.py:89-92), and so
 *   does this contract: u_s[o][j] is the dropout mask's uniform above (same bnn_rng_t fields, both generators, before Box-Muller,
 *   one device function: drop_u4) at element e = o K + j of the (O, K) mean, sample sample0 + s.  A bias (O,) with its (O, O)
 *   scale is one row: K = O, e = j.  Under BNN_GEN_PHILOX10_U24 a uniform can round up to 1.0, as the mask's can.
 *   The draw, all fp32:
 *     L[o][i][j] = sqrt(softplus(scale[o][i][j]) + (i == j ? 1e-10 : 0))   for j <= i   (softplus: torch's, threshold 20)
 *     w_s[o][i]  = mu[o][i] + sum_{j <= i} L[o][i][j] u_s[o][j]
 *   (WeightMultivariateNormal.stddev / sample()).  Only the lower triangle of scale is read: the upper one has no effect.  The
 *   summation order over j is fixed by K alone, so w_s is the same bit for bit for any nsamples, sample0 or grid, and where
 *   the backward or a shard re-creates it.  O K < 2^32 per tensor.
 *   CPU twin: tests/test_mvn_device.py (mvn_twin), on the oracle's Philox.
 *
 * LRT-noise contract (the local-reparameterization dense layer: bnn_lrt_forward, bnn_lrt_backward_epilogue)
 *   The noise of LocalReparamLinear is one eps per OUTPUT element and MC sample, on the eps stream above (same bnn_rng_t fields,
 *   both generators, one device function: eps4), one stream per layer: element e = b N + n of a sample's (B, N) output -- row b
 *   within the sample, N outputs per row -- uses eps[e] of sample sample0 + s.  The value depends only on the key and
 *   (s, b, n): not on the tile shape, not on whether the input is shared by the samples or given per sample, not on which GPU
 *   of a sharded run computes the sample.  The backward re-creates it from the key; it is never stored.  B N < 2^32 per sample.
 *   CPU twin: oracle.eps_fill on the key (tests/test_lrt_device.py).
 *
 * LRT-conv noise contract (the local-reparameterization conv layers, K11: the forward entry of the bnn_conv3d_lrt_ family and
 * the backward epilogue of K10, which re-creates the noise)
 *   The noise of LocalReparamConv{1,2,3}d is one eps per OUTPUT element and MC sample, on the same eps stream and the same
 *   device function (eps4 / eps1) as the LRT-noise contract above, one stream per layer.  Element e of ONE sample's
 *   (B, O, *out_spatial) output, in that contiguous order -- e = (b O + o) P + p, P = the number of output positions, p the flat
 *   position -- takes eps[e] of sample sample0 + s of the key.  The value depends only on the key and (s, b, o, p): not on the
 *   tile, not on whether the input is shared by the samples or given per sample, not on groups, not on which GPU of a sharded
 *   run computes the sample.  It is never stored: the backward re-creates it from the key.  B O P < 2^32 per sample (the conv
 *   entries refuse a per-sample tensor of 2^31 elements already).  A lane's four accumulator registers run along p; when P is a
 *   multiple of 4 they are one aligned eps quad (one Philox block per four outputs), otherwise every output takes its own block.
 *   CPU twin: oracle.eps_fill on the key (tests/test_lrt_conv_device.py).
 */
#ifndef BNN_HIP_H
#define BNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BNN_ABI_VERSION 2

enum {
    BNN_OK = 0,
    BNN_E_NULL = -1,      /* required pointer is NULL */
    BNN_E_SHAPE = -2,     /* negative / zero / inconsistent extent */
    BNN_E_DTYPE = -3,     /* unknown dtype code */
    BNN_E_ALIGN = -4,     /* pointer not aligned: to its element, or to the 16 bytes the entry documents for it */
    BNN_E_RANGE = -5,     /* value outside the supported range (e.g. >65535 samples) */
    BNN_E_UNSUPPORTED = -6,
    BNN_E_DEVICE = -7     /* a kernel reported an internal error through the device error word (bnn_check_device) */
};

enum { BNN_F32 = 0, BNN_BF16 = 1,
       BNN_BF16X3 = 2 /* an fp32 value as THREE bf16 planes h, m, l: h = bf16(v), m = bf16(v - h), l = bf16(v - h - m), v = h + m + l
                       * to 2^-24 |v| -- the operand format of the fp32 parity mode's dense contraction (bnn_dense_forward_x3) */ };

/* Compute mode of the contraction kernels. */
enum {
    BNN_COMPUTE_F32 = 0,  /* fp32 operands, fp32 accumulate; the 1e-5 parity mode.  Wide forward layers on the fast path run
                           * it as three-way bf16 splits on v_mfma_f32_16x16x32_bf16 (a = ah + am + al exactly; the six
                           * largest partial products, dropped terms <= 2^-25 |a b|, i.e. below one fp32 rounding) --
                           * 1.4 x faster than v_mfma_f32_16x16x4_f32, which everything else in this mode uses */
    BNN_COMPUTE_BF16 = 1  /* operands rounded to bf16 (RNE), v_mfma_f32_16x16x32_bf16, fp32 accumulate */
};

enum { BNN_GEN_PHILOX10_U24 = 0, BNN_GEN_PHILOX7_U16 = 1 };

/* One eps stream (host struct, read at call time). */
typedef struct bnn_rng {
    uint64_t seed;
    uint32_t stream;            /* tensor-stream id, < 65536 */
    uint32_t sample0;           /* id of the first MC sample of this call; sample s uses sample0 + s */
    uint32_t epoch_host;        /* host-side draw counter */
    int32_t epoch_dev_delta;    /* added to *epoch_dev (e.g. -1 to re-create the previous replay's draw) */
    const uint32_t *epoch_dev;  /* device word bumped by bnn_rng_advance; NULL = 0 */
    uint32_t generator;         /* BNN_GEN_* (RNG contract above) */
    uint32_t reserved;          /* 0 */
} bnn_rng_t;

/* One Gaussian posterior tensor with its Gaussian prior (host struct). */
typedef struct bnn_kl_tensor {
    const float *mu;
    const float *rho;
    int64_t n;
    float prior_mu;
    float prior_sigma;
} bnn_kl_tensor_t;

/* ---- library / device queries ------------------------------------------- */
int bnn_abi_version(void);
const char *bnn_arch(void);          /* "gfx950" */
const char *bnn_last_error(void);    /* text of the last non-zero return on this thread */
/* Number of kernel launches issued through this library so far (tests use it to
 * prove the HIP path ran). */
uint64_t bnn_launch_count(void);

/* Optional per-device scratch: `bytes` >= 128 KiB of ZEROED device memory that stays valid until replaced
 * (ptr = NULL unregisters).  Layout: word 0 = the sticky DEVICE ERROR WORD, 64 KiB reserved, then slabs for
 * the fixed-order partial sums of the backward kernels that split samples / rows over workgroups (without the
 * workspace those entry points return BNN_E_UNSUPPORTED).  Host call, not stream-ordered: register before
 * launching.  Launches use the workspace of the CURRENT device: make the operands' device current. */
int bnn_set_workspace(int device, void *ptr, int64_t bytes);
/* Reads (and clears) the device error word of `device` after synchronising `stream`: BNN_OK, or BNN_E_DEVICE
 * when a kernel gave up on an internal protocol since the last check -- today only the bounded LDS hand-off
 * waits of the fused linear kernel, which then skip their tile's store instead of storing numbers computed on
 * an undrawn buffer.  A SYNCHRONISING host call (not graph-capturable): call it at a sync / check point. */
int bnn_check_device(int device, void *stream);

/* ---- K1: posterior draw --------------------------------------------------
 * replaces  WeightNormal.stddev / WeightNormal.sample
 *           pytorch_bayesian/nn/core.py:25-27, 44-45
 *   out = mu + (1e-10 + softplus(rho)) * eps        (softplus: beta 1, threshold 20)
 */
/* eps supplied by the caller (parity mode: eps from torch's CPU generator). */
int bnn_sample_affine_eps(const float *mu, const float *rho, const float *eps,
                          void *out, int64_t n, int out_dtype, void *stream);
/* eps drawn in-kernel; writes `nsamples` draws, draw s at out + s * out_sample_stride
 * elements. */
int bnn_sample_affine_philox(const float *mu, const float *rho, void *out, int64_t n,
                             int nsamples, int64_t out_sample_stride, int out_dtype,
                             const bnn_rng_t *rng, void *stream);
/* The raw eps stream (fp32), same layout as above. */
int bnn_eps_philox(float *out, int64_t n, int nsamples, int64_t out_sample_stride,
                   const bnn_rng_t *rng, void *stream);
/* sigma = 1e-10 + softplus(rho)   (WeightNormal.stddev, core.py:25-27) */
int bnn_sigma(const float *rho, float *out, int64_t n, void *stream);

/* Backward of K1 (what autograd derives from core.py:44-45), summed over samples:
 *   g_mu[e]  (+)= sum_s g_w[s][e]
 *   g_rho[e] (+)= sum_s g_w[s][e] * eps_s[e] * sigmoid(rho[e])
 * eps: external (eps != NULL, sample stride eps_sample_stride) or Philox (rng != NULL).
 * accumulate != 0 adds into g_mu / g_rho instead of overwriting. */
int bnn_sample_affine_bwd(const float *g_w, int64_t g_w_sample_stride, const float *rho,
                          const float *eps, int64_t eps_sample_stride, const bnn_rng_t *rng,
                          int64_t n, int nsamples, float *g_mu, float *g_rho, int accumulate,
                          void *stream);

/* epoch_dev[0] += inc, in stream order (a 1-thread kernel; graph-capturable). */
int bnn_rng_advance(uint32_t *epoch_dev, uint32_t inc, void *stream);

/* ---- K3: closed-form Gaussian KL ------------------------------------------
 * replaces  KLDivergence.compute_kl / KLDivergence.forward
 *           pytorch_bayesian/nn/loss.py:16-28, 30-38
 *           (torch.distributions.kl._kl_normal_normal)
 *   kl_e = 0.5 * (r + t - 1 - ln r),  r = (sigma/sigma_p)^2,  t = ((mu - mu_p)/sigma_p)^2
 * out[0..ntensors-1] = per-tensor SUMS (the reference's .mean() = sum / n);
 * out[ntensors]      = mean_t(sum_t / n_t) / n_batches   (loss.py:38).
 * `tensors` is a host array; `workspace` needs bnn_kl_workspace_bytes(ntensors) bytes; calls
 * sharing a workspace must be stream-ordered.
 * Deterministic: fixed-order two-pass reduction, no float atomics.  (Folding the second pass
 * into the first behind a last-workgroup ticket was measured SLOWER on MI355X: 23 us against
 * 6 + 7 us -- 1190 same-address atomics across 8 XCDs serialise.) */
int64_t bnn_kl_workspace_bytes(int ntensors);
int bnn_kl_forward(const bnn_kl_tensor_t *tensors, int ntensors, float n_batches,
                   float *out, void *workspace, void *stream);
/* The same result in two calls, for a step that ends in the MC reduction (examples/MNIST/uncertainty.py:50 after
 * nn/loss.py:30-38): bnn_kl_forward_partial launches only the first pass; bnn_mc_sum_kl (below) runs the second pass
 * as one extra workgroup of the reduction's launch.  Every launch costs >= 4 us on MI355X; this removes one from
 * each forward.  Same tensors / workspace in both calls, stream-ordered; values bit-identical to bnn_kl_forward. */
int bnn_kl_forward_partial(const bnn_kl_tensor_t *tensors, int ntensors, void *workspace, void *stream);
/* Backward: for tensor t,  g_mu (+)= scale_t * (mu - mu_p)/sigma_p^2,
 *   g_rho (+)= scale_t * (sigma/sigma_p^2 - 1/sigma) * sigmoid(rho),
 * scale_t = *upstream (device scalar, may be NULL = 1) / (n_t * ntensors * n_batches). */
int bnn_kl_backward(const bnn_kl_tensor_t *tensors, int ntensors, float n_batches,
                    const float *upstream, float *const *g_mu, float *const *g_rho,
                    int accumulate, void *stream);

/* ---- K2: sampled linear ----------------------------------------------------
 * replaces  NormalLinear.forward   pytorch_bayesian/nn/dense.py:56-60
 *           (sample(): dense.py:46-54 -> core.py:44-45, then F.linear)
 * and, with nsamples > 1, the MC loop of BayesianNetworkModule.forward
 *           pytorch_bayesian/nn/container.py:32-37  for this layer.
 *
 *   for s in [0, nsamples):
 *     w_s = mu_w + sigma(rho_w) * eps(rng_w, s)      (N, K)   never written to memory
 *     b_s = mu_b + sigma(rho_b) * eps(rng_b, s)      (N)      (mu_b == NULL: no bias)
 *     y[s] = x[s] @ w_s^T + b_s                      (M, N)
 *   x[s] = x + s * x_sample_stride (0 = every sample reads the same input),
 *   y[s] = y + s * y_sample_stride;  ldx / ldy = row strides in elements.
 * flags: BNN_FLAG_RELU applies max(.,0) in the epilogue. */
enum {
    BNN_FLAG_RELU = 1,
    /* bf16 compute mode only: x is bf16 in memory (ldx, strides in elements; K % 8 == 0,
     * 16-B aligned) / y is written as bf16.  Lets a chain of layers keep its hidden
     * activations in bf16: half the activation stream of the next layer.  With either flag x AND the weights (mu_w and
     * rho_w, or w) must be 16-B aligned: BNN_E_UNSUPPORTED otherwise.  Without them every operand may lie on its element
     * (BNN_E_ALIGN below that); 16-B aligned x, weights and K % 4 == 0 buy the sampler-paced kernel. */
    BNN_FLAG_X_BF16 = 2,
    BNN_FLAG_Y_BF16 = 4,
    /* bnn_conv3d_moments_forward only: the moment-matched ELU (bnn_moments_elu's function, its alpha an argument) in the epilogue */
    BNN_FLAG_ELU = 8
};
int bnn_linear_forward_sampled(const void *x, int64_t x_sample_stride, int64_t ldx,
                               const float *mu_w, const float *rho_w,
                               const float *mu_b, const float *rho_b,
                               void *y, int64_t y_sample_stride, int64_t ldy,
                               int64_t M, int64_t N, int64_t K, int nsamples,
                               const bnn_rng_t *rng_w, const bnn_rng_t *rng_b,
                               int compute, int flags, void *stream);
/* The same layer, and in the same launch the FIRST pass of the model's KL (bnn_kl_forward_partial): a narrow layer's
 * launch (N <= 16: a classifier head, 32 workgroups at the BASELINE shape) leaves most of MI355X's 256 CUs idle and a
 * launch of its own costs >= 4 us, so the KL partial sums ride along as extra workgroups.  When the layer is not a
 * narrow one on the fast path, or the model is large (>= 8 Mi scalars, > 8 tensors), the first pass is launched
 * separately by this call -- the result is the same either way; finish with bnn_mc_sum_kl (or run bnn_kl_forward).
 * replaces  nn/dense.py:56-60 + the first half of nn/loss.py:16-28. */
int bnn_linear_forward_sampled_kl(const void *x, int64_t x_sample_stride, int64_t ldx,
                                  const float *mu_w, const float *rho_w, const float *mu_b,
                                  const float *rho_b, void *y, int64_t y_sample_stride, int64_t ldy,
                                  int64_t M, int64_t N, int64_t K, int nsamples, const bnn_rng_t *rng_w,
                                  const bnn_rng_t *rng_b, int compute, int flags,
                                  const bnn_kl_tensor_t *tensors, int ntensors, void *kl_workspace, void *stream);
/* ---- draw-once path of the sampled linear layer (bf16 compute mode) ---------------------------------------
 * The same layer in two launches instead of one fused one: every posterior tensor of a forward is drawn ONCE
 * (all S MC samples, sigma computed once per weight) by bnn_draw_multi, then bnn_dense_forward contracts on the
 * drawn weights -- a dense MFMA GEMM with both operands arriving by LDS-DMA.  Same DrawKey -> the same draws as
 * the fused kernel and as bnn_sample_affine_philox, bit for bit (one device function).  On MI355X this is the
 * faster form at the BASELINE shapes: inside the GEMM the draw's ~150 VALU issue slots per 4 weights share each
 * SIMD's issue port with the MFMAs and pace the kernel through an LDS hand-off.
 *
 * One posterior tensor to draw (host struct, read at call time).
 * replaces  WeightNormal.sample  pytorch_bayesian/nn/core.py:44-45, called weight-then-bias by
 *           NormalLinear.sample  pytorch_bayesian/nn/dense.py:46-54, once per MC sample by the loop at
 *           pytorch_bayesian/nn/container.py:36-37 */
enum { BNN_DRAW_SAMPLE = 0, BNN_DRAW_MEAN = 1, BNN_DRAW_SIGMA = 2, BNN_DRAW_COPY = 3,   /* bnn_draw_tensor_t.kind (below) */
       BNN_DRAW_FLIPOUT = 16 };  /* ... of a Flipout draw (sign contract below) */
typedef struct bnn_draw_tensor {
    const float *mu;
    const float *rho;
    int64_t rows, cols;         /* posterior shape (N, K); a bias is (1, N).  rows > 1 needs cols % 4 == 0 */
    void *out;                  /* draw s at out + s * out_sample_stride elements: `rows` rows of `ld` elements */
    int64_t ld;                 /* >= cols (% 8 == 0 when rows > 1); columns cols .. ld - 1 are written as ZEROS */
    int64_t out_sample_stride;  /* elements */
    int out_dtype;              /* BNN_F32, BNN_BF16, or BNN_BF16X3: three planes, plane p of draw s at
                                 * out + (p * nsamples + s) * out_sample_stride (kinds 0, 1, 2) */
    int kind;                   /* BNN_DRAW_SAMPLE 0: draw mu + sigma(rho) eps (rng used); BNN_DRAW_FLIPOUT: the same with eps[r][c] = R[r] S[c], the
                                 * Flipout signs of rng (sign contract above, linear layout with O = rows, K = cols; no taps);
                                 * BNN_DRAW_MEAN 1: mu itself; BNN_DRAW_SIGMA 2: sigma(rho) itself (no eps: Flipout's
                                 * two operands, nsamples = 1); BNN_DRAW_COPY 3: `mu` as it is, written ONCE whatever nsamples is (rho ignored,
                                 * pass mu) -- with BNN_BF16X3 (planes out_sample_stride apart) this is bnn_split_bf16x3 of an
                                 * activation riding in the draw launch: the fp32 parity mode's input planes */
    int taps;                   /* 0 / 1: rows are written as they are.  KH * KW of a conv weight (O, C, KH, KW) viewed as
                                 * (O, C * KH * KW): element (o, c, t) is written to column t * C + c (tap-major, what
                                 * bnn_conv2d_dense_forward reads); the eps stream keeps the original element order */
    bnn_rng_t rng;
} bnn_draw_tensor_t;
/* Draws <= 8 tensors x nsamples MC samples in ONE launch.  kl_tensors != NULL: the launch also carries the first
 * pass of that model's KL (as bnn_linear_forward_sampled_kl does; same eligibility, same values) -- finish it with
 * bnn_mc_sum_kl; BNN_E_UNSUPPORTED (nothing launched) when the KL is not eligible. */
int bnn_draw_multi(const bnn_draw_tensor_t *tensors, int ntensors, int nsamples,
                   const bnn_kl_tensor_t *kl_tensors, int kl_ntensors, void *kl_workspace, void *stream);
/* y[s] = act(x[s] . w[s]^T + b[s]) on drawn weights: x (S or shared: x_sample_stride = 0) x M x ldx bf16,
 * w S x N x ldw bf16 with every row ZERO beyond K up to ldw >= roundup(K, 64) (what bnn_draw_multi writes),
 * b S x N fp32 or NULL, y fp32 or (BNN_FLAG_Y_BF16) bf16; BNN_FLAG_RELU.  K % 8 == 0, 16-B aligned rows.
 * N <= 16 (a classifier head) runs a K-split kernel without LDS staging.  fp32 accumulate (bf16 MFMA).
 * replaces  F.linear(x, *self.sampled)  pytorch_bayesian/nn/dense.py:60 */
int bnn_dense_forward(const void *x, int64_t x_sample_stride, int64_t ldx,
                      const void *w, int64_t w_sample_stride, int64_t ldw,
                      const float *b, int64_t b_sample_stride,
                      void *y, int64_t y_sample_stride, int64_t ldy,
                      int64_t M, int64_t N, int64_t K, int nsamples, int flags, void *stream);
/* bnn_dense_forward with MC dropout in the epilogue: y[s] = mask_s (.) act(x[s] . w[s]^T + b[s]) * 1 / (1 - p) -- bias, activation,
 * then mask and scale, then the store (dropout-mask contract above, F = N, sample rng->sample0 + s).  Same operands, strides and
 * flags as bnn_dense_forward.
 *   FAN-OUT: x, w and b all shared (x_sample_stride = w_sample_stride = 0, b_sample_stride = 0 or b NULL) -- every output tile is
 *   computed ONCE and its epilogue stores the nsamples masked copies (the first MC-dropout layer of a net: until the first mask
 *   every sample computes the same thing).  Otherwise one launch over the samples (w_sample_stride = 0 for shared weights).
 *   Fused (one launch) when N % 4 == 0 and N > 16, on the 256 x 80, 128 x 160, 64 x 160 and 32 x 160 tiles, fp32 or bf16 output
 *   (a layer the plain launch would give the 256 x 128 tile takes 128 x 160).  Otherwise -- the narrow N <= 16 kernel, or N % 4 != 0
 *   -- the plain kernel stores and the mask launch of bnn_mc_dropout runs after it, in place (two launches, the same values).
 *   nsamples <= 65535, 0 <= p <= 1 (BNN_E_RANGE), M * N < 2^32.
 * replaces  F.dropout(self.linear(x), self.drop_prob, sample, False)  pytorch_bayesian/nn/dense.py:174-179 */
int bnn_dense_forward_dropout(const void *x, int64_t x_sample_stride, int64_t ldx,
                              const void *w, int64_t w_sample_stride, int64_t ldw,
                              const float *b, int64_t b_sample_stride,
                              void *y, int64_t y_sample_stride, int64_t ldy,
                              int64_t M, int64_t N, int64_t K, int nsamples, int flags, float p, const bnn_rng_t *rng, void *stream);
/* A hidden layer AND the classifier head behind it in ONE launch (bf16 compute mode, inference): the hidden layer's output
 * act(x[s] w[s]^T + b[s]) is never stored -- every wave of the GEMM rounds its tile to bf16 (exactly what a stored bf16 hidden
 * activation holds) and contracts it with the matching columns of the head's drawn weights w_head (S x n_head x ldwh bf16, rows
 * zero beyond N up to ldwh, n_head <= 16), leaving PARTIAL logits
 *     partials[part][s][m][j],  part < bnn_dense_head_parts(M, N, nsamples),  fp32, M x n_head per (part, s);
 * partial 0 also carries the head's bias b_head (S x n_head fp32 or NULL).  The logits of sample s are the sum over `part`
 * (bnn_mc_sum with nsamples = parts, y_sample_stride = S * M * n_head, n = S * M * n_head), the predictive mean the sum over
 * (part, s) scaled by 1 / S (bnn_mc_sum / bnn_mc_sum_kl with nsamples = parts * S, y_sample_stride = M * n_head; parts * S
 * is not bounded -- it passes 256 from S = 17 at the BASELINE widths): one launch (the head's own, >= 4 us) and the hidden
 * activation's S * M * N * 2 bytes of stores fewer per forward.  Same bf16 products as bnn_dense_forward twice; fp32 sums in
 * another (fixed) order.
 * replaces  two consecutive F.linear(x, *self.sampled)  pytorch_bayesian/nn/dense.py:60 (+ the ReLU between them) */
int bnn_dense_head_parts(int64_t M, int64_t N, int nsamples);
int bnn_dense_forward_head(const void *x, int64_t x_sample_stride, int64_t ldx,
                           const void *w, int64_t w_sample_stride, int64_t ldw,
                           const float *b, int64_t b_sample_stride,
                           const void *w_head, int64_t wh_sample_stride, int64_t ldwh,
                           const float *b_head, int64_t bh_sample_stride, int64_t n_head,
                           float *partials, int64_t M, int64_t N, int64_t K, int nsamples, int flags, void *stream);
/* bnn_dense_forward_head in the fp32 PARITY mode: x, w and w_head are BNN_BF16X3 operands (plane strides in elements); the fp32
 * tile of the hidden layer is split into its three bf16 planes in the epilogue and contracted with the head's planes on the six
 * plane pairs of bnn_dense_forward_x3 (small pairs summed apart from (h, h)).  Partial logits as above, fp32. */
int bnn_dense_forward_x3_head(const void *x, int64_t x_plane_stride, int64_t x_sample_stride, int64_t ldx,
                              const void *w, int64_t w_plane_stride, int64_t w_sample_stride, int64_t ldw,
                              const float *b, int64_t b_sample_stride,
                              const void *w_head, int64_t wh_plane_stride, int64_t wh_sample_stride, int64_t ldwh,
                              const float *b_head, int64_t bh_sample_stride, int64_t n_head,
                              float *partials, int64_t M, int64_t N, int64_t K, int nsamples, int flags, void *stream);
/* The same layer in the fp32 PARITY mode (1e-5 against the reference) on the same kernel: x and w are BNN_BF16X3 operands
 * (plane p at + p * plane_stride elements; x from bnn_split_bf16x3 or a previous layer's BNN_FLAG_Y_BF16 output, w from
 * bnn_draw_multi with out_dtype BNN_BF16X3) and the contraction runs the six largest partial products of
 * (xh + xm + xl)(wh + wm + wl) on the bf16 MFMA with fp32 accumulation -- dropped terms <= 2^-25 |x w|, below one fp32
 * rounding; what BNN_COMPUTE_F32 does inside bnn_linear_forward_sampled.  y: fp32, or (BNN_FLAG_Y_BF16) three bf16
 * planes of the fp32 result, y_plane_stride apart, for the next layer.  N <= 16 (a classifier head: K <= 2048, fp32
 * outputs) runs the K-split kernel, the six plane pairs as six passes.
 * replaces  F.linear(x, *self.sampled)  pytorch_bayesian/nn/dense.py:60 */
int bnn_dense_forward_x3(const void *x, int64_t x_plane_stride, int64_t x_sample_stride, int64_t ldx,
                         const void *w, int64_t w_plane_stride, int64_t w_sample_stride, int64_t ldw,
                         const float *b, int64_t b_sample_stride,
                         void *y, int64_t y_plane_stride, int64_t y_sample_stride, int64_t ldy,
                         int64_t M, int64_t N, int64_t K, int nsamples, int flags, void *stream);
/* fp32 (rows x cols, row pitch ldx) -> BNN_BF16X3 planes (row pitch ld_out, planes plane_stride elements apart): the
 * input of the first bnn_dense_forward_x3 of a network.  cols % 8 == 0, 16-B aligned rows. */
int bnn_split_bf16x3(const float *x, int64_t rows, int64_t cols, int64_t ldx, void *out, int64_t ld_out, int64_t plane_stride,
                     void *stream);
/* bf16 (batch x rows x cols, row pitch ld_in) -> the transposes (batch x cols x ld_out), columns rows .. ld_out - 1 written as ZEROS:
 * drawn weights (S x N x ldw, from bnn_draw_multi) as the operand of the input gradient of a training step,
 *   gx[s] = gy[s] . w_s  =  bnn_dense_forward(x = gy, w = w_s^T (K rows of ld_out >= roundup(N, 64)), M, N' = K, K' = N)
 * -- the backward of F.linear (pytorch_bayesian/nn/dense.py:60, examples/MNIST/train.py:63-65) on the weights the forward drew,
 * with no second draw.  cols % 8 == 0, 16-B aligned rows on both sides. */
int bnn_transpose_bf16(const void *in, int64_t in_batch_stride, int64_t ld_in, void *out, int64_t out_batch_stride, int64_t ld_out,
                       int64_t rows, int64_t cols, int batch, void *stream);

/* Same contraction with the weights given (F.linear(x, w, b), dense.py:60):
 * w[s] = w + s * w_sample_stride, b[s] = b + s * b_sample_stride (b may be NULL). */
int bnn_linear_forward(const float *x, int64_t x_sample_stride, int64_t ldx,
                       const float *w, int64_t w_sample_stride,
                       const float *b, int64_t b_sample_stride,
                       float *y, int64_t y_sample_stride, int64_t ldy,
                       int64_t M, int64_t N, int64_t K, int nsamples,
                       int compute, int flags, void *stream);

/* ---- backward of K2 linear -----------------------------------
 * replaces  what autograd derives from F.linear(x, w, b) (dense.py:60) and
 *           w = mu + sigma(rho) * eps (core.py:44-45) in loss.backward()
 *           (examples/MNIST/train.py:63-65).  W is (N, K) row-major, as in the forward.
 *
 * Input gradient, fused with the re-creation of the forward's draw (same rng_w key):
 *     gx[s][m][k] = sum_n gy[s][m][n] * W_s[n][k],   W_s = mu_w + sigma(rho_w) * eps_s
 * flags: BNN_FLAG_X_BF16 = gy is bf16, BNN_FLAG_Y_BF16 = gx is written as bf16 (bf16 compute only).
 * Needs K % 4 == 0, N % 4 == 0 (fp32 gy) / N % 8 == 0 (bf16 gy), 16-B aligned operands;
 * returns BNN_E_UNSUPPORTED otherwise (callers then draw W_s with bnn_sample_affine_philox and
 * use bnn_linear_backward_input). */
int bnn_linear_backward_input_sampled(const void *gy, int64_t gy_sample_stride, int64_t ldgy,
                                      const float *mu_w, const float *rho_w,
                                      void *gx, int64_t gx_sample_stride, int64_t ldgx,
                                      int64_t M, int64_t N, int64_t K, int nsamples,
                                      const bnn_rng_t *rng_w, int compute, int flags, void *stream);
/* Same with the weights given: w[s] = w + s * w_sample_stride, fp32 (any shape). */
int bnn_linear_backward_input(const void *gy, int64_t gy_sample_stride, int64_t ldgy,
                              const float *w, int64_t w_sample_stride,
                              void *gx, int64_t gx_sample_stride, int64_t ldgx,
                              int64_t M, int64_t N, int64_t K, int nsamples, int flags, void *stream);
/* Weight gradient fused with the backward of the draw (dW_s = gy_s^T x_s is never stored):
 *     g_mu [n][k] (+)= sum_s dW_s[n][k]
 *     g_rho[n][k] (+)= sum_s dW_s[n][k] * eps_s[n][k] * sigmoid(rho_w[n][k])
 * x: (S, M, K) or shared (x_sample_stride = 0).  flags: BNN_FLAG_X_BF16 = x is bf16,
 * BNN_FLAG_Y_BF16 = gy is bf16 (bf16 compute only).  With few output tiles
 * the MC samples are split over workgroups through the registered workspace and added in a fixed
 * order: bitwise reproducible.
 * Bias (rho_b, g_mu_b, g_rho_b, rng_b all given, or all NULL): g_mu_b[n] (+)= sum_s c_s[n],
 * g_rho_b[n] (+)= sum_s c_s[n] * eps_b,s[n] * sigmoid(rho_b[n]), c_s = column sums of gy[s] -- taken
 * inside the same launch by the workgroups of k-tile 0 (one extra MFMA against a fragment of ones per
 * step), or by bnn_colsum + bnn_sample_affine_bwd when the samples are split.
 * KL (kl != NULL): the gradient of the layer's share of KLDivergence (loss.py:16-38) is added in the
 * same final store -- g_mu += c (mu - mu_p) / sigma_p^2, g_rho += c (sigma / sigma_p^2 - 1 / sigma)
 * sigmoid(rho), c = *upstream * scale -- instead of a separate bnn_kl_backward pass plus autograd's
 * accumulation adds.  scale_x = 1 / (n_x * ntensors * n_batches), n_x = elements of that tensor.
 * Alignment: x, gy, rho_w and the bias tensors on their element (16 bytes buy the 16-B loads and the LDS-DMA kernel); with
 * K % 4 == 0 g_mu and g_rho are stored four columns at a time and must be 16-B aligned, BNN_E_ALIGN otherwise. */
typedef struct bnn_kl_fuse {
    const float *upstream;      /* device scalar: d loss / d KL */
    const float *mu_w;          /* (N, K) */
    const float *mu_b;          /* (N) or NULL */
    float scale_w, prior_mu_w, prior_sigma_w;
    float scale_b, prior_mu_b, prior_sigma_b;
} bnn_kl_fuse_t;
int bnn_linear_backward_weight_sampled(const void *x, int64_t x_sample_stride, int64_t ldx,
                                       const void *gy, int64_t gy_sample_stride, int64_t ldgy,
                                       const float *rho_w, float *g_mu, float *g_rho,
                                       const float *rho_b, float *g_mu_b, float *g_rho_b,
                                       int64_t M, int64_t N, int64_t K, int nsamples,
                                       const bnn_rng_t *rng_w, const bnn_rng_t *rng_b,
                                       const bnn_kl_fuse_t *kl,
                                       int compute, int flags, int accumulate, void *stream);
/* Whole backward of a NARROW layer (N <= 16, K % 4 == 0: a classifier head) in one pass over the
 * activations: gx (may be NULL), g_mu / g_rho of the weight, and the bias gradients -- same definitions
 * as the three entry points above.  gy fp32; flags: BNN_FLAG_X_BF16 = x is bf16, BNN_FLAG_Y_BF16 = gx
 * is written as bf16.  Needs the registered workspace (S * (2 N K + N) floats); BNN_E_UNSUPPORTED
 * otherwise (callers then use the general entry points).  Rows of x and gx are read / written four
 * elements at a time: bases, sample strides and the pitches ldx, ldgx must be multiples of 4 elements;
 * mu_w, rho_w, g_mu and g_rho are read / written 16 bytes at a time and must be 16-B aligned: BNN_E_ALIGN
 * otherwise (callers use the general entry points then, too).  gy: element alignment.  Every argument check, both
 * keys included, comes before the first launch. */
int bnn_linear_backward_narrow_sampled(const void *x, int64_t x_sample_stride, int64_t ldx,
                                       const float *gy, int64_t gy_sample_stride, int64_t ldgy,
                                       const float *mu_w, const float *rho_w,
                                       void *gx, int64_t gx_sample_stride, int64_t ldgx,
                                       float *g_mu, float *g_rho,
                                       const float *rho_b, float *g_mu_b, float *g_rho_b,
                                       int64_t M, int64_t N, int64_t K, int nsamples,
                                       const bnn_rng_t *rng_w, const bnn_rng_t *rng_b,
                                       const bnn_kl_fuse_t *kl, int flags, int accumulate, void *stream);
/* F.linear's own weight gradient, per sample: gw[s][n][k] (+)= sum_m gy[s][m][n] * x[s][m][k],
 * gw[s] = gw + s * gw_sample_stride (parity mode, where the draw is a separate op).  With K % 4 == 0 gw must be 16-B aligned
 * and gw_sample_stride a multiple of 4 (BNN_E_ALIGN otherwise); x and gy: element alignment. */
int bnn_linear_backward_weight(const void *x, int64_t x_sample_stride, int64_t ldx,
                               const void *gy, int64_t gy_sample_stride, int64_t ldgy,
                               float *gw, int64_t gw_sample_stride,
                               int64_t M, int64_t N, int64_t K, int nsamples,
                               int compute, int flags, int accumulate, void *stream);
/* Bias: out[s][n] = sum_m gy[s][m][n]  (feed out to bnn_sample_affine_bwd with the bias key).
 * flags: BNN_FLAG_X_BF16 = gy is bf16. */
int bnn_colsum(const void *gy, int64_t gy_sample_stride, int64_t ldgy, float *out,
               int64_t M, int64_t N, int nsamples, int flags, void *stream);
/* Fused-ReLU layers: out[i] = y[i] > 0 ? g[i] : 0.  flags: BNN_FLAG_X_BF16 = g and out are bf16,
 * BNN_FLAG_Y_BF16 = y is bf16. */
int bnn_relu_backward(const void *g, const void *y, void *out, int64_t n, int flags, void *stream);

/* ---- K2: sampled conv2d (implicit GEMM) --------------------------------------
 * replaces  NormalConv2d.forward   pytorch_bayesian/nn/conv.py:112-119
 *   y[s] = conv2d(x[s], w_s, b_s, stride, padding, dilation, groups), NCHW / OIHW.
 * Implicit GEMM: M = B*OH*OW, N = O/groups, K = (C/groups)*KH*KW. */
typedef struct bnn_conv2d_shape {
    int32_t B, C, H, W;          /* input  (B, C, H, W) */
    int32_t O, KH, KW;           /* weight (O, C/groups, KH, KW) */
    int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, groups;
} bnn_conv2d_shape_t;
/* Two kernels behind these entry points.  FAST (groups == 1, K % 8 == 0, O >= 16, 16-B aligned
 * weights, a workspace of bnn_conv2d_workspace_bytes(shape, x_samples, compute) bytes, 16-B aligned):
 * an explicit im2col panel (bf16 in bf16 compute) written to the workspace, then the draw-paced
 * linear kernel (LDS-DMA activation rings, weights drawn once per 512 rows) with an NCHW-storing
 * epilogue.  GENERIC (workspace NULL / too small, or any other shape): one implicit-GEMM kernel with
 * scalar im2col loaders.  x_samples = 1 when x_sample_stride == 0 (a shared input is expanded once),
 * else nsamples.  bnn_conv2d_workspace_bytes returns 0 when only the generic kernel applies. */
int64_t bnn_conv2d_workspace_bytes(const bnn_conv2d_shape_t *shape, int x_samples, int compute);
int bnn_conv2d_forward_sampled(const float *x, int64_t x_sample_stride,
                               const float *mu_w, const float *rho_w,
                               const float *mu_b, const float *rho_b,
                               float *y, int64_t y_sample_stride,
                               const bnn_conv2d_shape_t *shape, int nsamples,
                               const bnn_rng_t *rng_w, const bnn_rng_t *rng_b,
                               int compute, int flags,
                               void *workspace, int64_t workspace_bytes, void *stream);
int bnn_conv2d_forward(const float *x, int64_t x_sample_stride,
                       const float *w, int64_t w_sample_stride,
                       const float *b, int64_t b_sample_stride,
                       float *y, int64_t y_sample_stride,
                       const bnn_conv2d_shape_t *shape, int nsamples,
                       int compute, int flags,
                       void *workspace, int64_t workspace_bytes, void *stream);

/* The conv on DRAWN weights as a true implicit GEMM (bf16 compute mode; no im2col panel, no workspace): w is what
 * bnn_draw_multi writes for the (O, C * KH * KW) posterior with taps = KH * KW -- S x O x ldw bf16, tap-major columns
 * (t * C + c), rows zero-padded to ldw >= roundup(C * KH * KW, 64).  A workgroup keeps its images in LDS (bf16, padded,
 * channel-last) and gathers the im2col rows in the address of its MFMA fragment reads; the weight tile streams by
 * LDS-DMA.  x fp32 NCHW (x_sample_stride = 0: shared), b S x O fp32 or NULL, y fp32 NCHW.  Built for groups = 1,
 * C = 64 or a multiple of 128, O = 64 or 128, <= 128 output pixels per image, one padded image + weight ring within
 * LDS (both BASELINE conv shapes); BNN_E_UNSUPPORTED otherwise (use bnn_conv2d_forward_sampled).
 * replaces  F.conv2d(x, *self.sampled, ...)  pytorch_bayesian/nn/conv.py:116-119 */
int bnn_conv2d_dense_forward(const float *x, int64_t x_sample_stride,
                             const void *w, int64_t w_sample_stride, int64_t ldw,
                             const float *b, int64_t b_sample_stride,
                             float *y, int64_t y_sample_stride,
                             const bnn_conv2d_shape_t *shape, int nsamples, int flags, void *stream);

/* The same convolution in the fp32 PARITY mode (1e-5 against the reference): w is a BNN_BF16X3 operand (three bf16 planes,
 * w_plane_stride elements apart: bnn_draw_multi with out_dtype BNN_BF16X3 and taps = KH * KW), the images are split into
 * three bf16 planes as they become resident in LDS, and every 64-k block is contracted on the six largest plane pairs of
 * (xh + xm + xl)(wh + wm + wl) with fp32 accumulation -- the five small pairs of every block first, then (h, h) over all of K,
 * as bnn_dense_forward_x3 does.  No im2col panel, no workspace.  Same shapes as bnn_conv2d_dense_forward.
 * replaces  F.conv2d(x, *self.sampled, ...)  pytorch_bayesian/nn/conv.py:116 */
int bnn_conv2d_dense_forward_x3(const float *x, int64_t x_sample_stride,
                                const void *w, int64_t w_plane_stride, int64_t w_sample_stride, int64_t ldw,
                                const float *b, int64_t b_sample_stride,
                                float *y, int64_t y_sample_stride,
                                const bnn_conv2d_shape_t *sh, int nsamples, int flags, void *stream);
/* Flipout conv2d in ONE launch: y[b] = conv(x[b], mean) + R[b] * conv(x[b] * S[b], stddev) with per-example
 * sign tensors S (B x C) and R (B x O) of +-1 (conv.py:154-161).  w = [O rows of the mean | O rows of the stddev], bf16
 * tap-major (bnn_draw_multi with kind = 1 / 2 and taps = KH * KW), ldw >= roundup(C KH KW, 64).  Both contractions share
 * the A fragment of the implicit GEMM above: S is XOR-ed into its sign bits for the second one, R scales that
 * accumulator in the epilogue.  No bias (the reference's Flipout conv has none).  Built for 2 O = 64 or 128.
 * replaces  FlipOutNormalConv2d.forward  pytorch_bayesian/nn/conv.py:207-221 */
int bnn_conv2d_flipout_forward(const float *x, const void *w, int64_t ldw, const float *sign_in, const float *sign_out,
                               float *y, const bnn_conv2d_shape_t *shape, int flags, void *stream);
/* The same launch in the fp32 PARITY mode: w = [O mean rows | O stddev rows] as BNN_BF16X3 planes (w_plane_stride elements apart,
 * >= 2 O ldw; bnn_draw_multi with kind = 1 / 2, taps, out_dtype = BNN_BF16X3 and out_sample_stride = the plane stride), the images
 * split into three planes in LDS, six plane pairs per 64-k block; S flips the sign bits of every plane of the A fragment alike.
 * 1e-5 of the output scale against float64.  replaces  FlipOutNormalConv2d.forward  pytorch_bayesian/nn/conv.py:207-221 */
int bnn_conv2d_flipout_forward_x3(const float *x, const void *w, int64_t w_plane_stride, int64_t ldw, const float *sign_in,
                                  const float *sign_out, float *y, const bnn_conv2d_shape_t *sh, int flags, void *stream);

/* Flipout conv2d of the MC-batched path in ONE launch for nsamples samples, the signs keyed (Flipout-sign contract above, conv
 * layout, sample rng->sample0 + s) and made inside the kernel -- no sign tensor in memory:
 *   y[s][b] = conv(x[s | 0][b], mean) + R_s[b] * conv(x[s | 0][b] * S_s[b], stddev)           (conv.py:207-221 per MC sample)
 * x fp32 NCHW: SHARED (x_sample_stride = 0: the first Bayesian layer of a net sees the un-replicated batch) -- the mean contraction
 * of a tile runs ONCE and is reused by every sample of the workgroup; only the stddev contraction, S_s XOR-ed into the A
 * fragment's sign bits, runs per sample -- or per sample (x_sample_stride = B C H W: a Bayesian layer earlier in the net).
 * y: nsamples x B x O x OH x OW fp32 (y_sample_stride elements).  w, ldw, shapes: as bnn_conv2d_flipout_forward.
 * nsamples <= 65535, B (O + C) < 2^32.  BNN_E_UNSUPPORTED (nothing launched) where bnn_conv2d_flipout_forward would refuse. */
int bnn_conv2d_flipout_forward_mc(const float *x, int64_t x_sample_stride, const void *w, int64_t ldw, float *y,
                                  int64_t y_sample_stride, const bnn_conv2d_shape_t *shape, int nsamples, const bnn_rng_t *rng,
                                  int flags, void *stream);
/* Does the LDS-resident kernel behind the five launches above take this shape?  A pure host query (no GPU call), the launches'
 * own fit computation: -> the images one workgroup keeps resident (>= 1, at most shape->B), 0 where the launch would answer
 * BNN_E_UNSUPPORTED for the shape (groups, C, O, > 128 output pixels per image, an image + the weight ring past the LDS block),
 * BNN_E_NULL / BNN_E_SHAPE / BNN_E_RANGE for a bad argument.  It assumes tap-major weights with ldw = roundup(C KH KW, 64) and
 * aligned pointers (what bnn_draw_multi writes); nsamples and shared_x (x_sample_stride = 0) matter to BNN_CONV_FLIPOUT_MC only. */
enum { BNN_CONV_DENSE = 0,        /* bnn_conv2d_dense_forward */
       BNN_CONV_DENSE_X3 = 1,     /* bnn_conv2d_dense_forward_x3 */
       BNN_CONV_FLIPOUT = 2,      /* bnn_conv2d_flipout_forward */
       BNN_CONV_FLIPOUT_X3 = 3,   /* bnn_conv2d_flipout_forward_x3 */
       BNN_CONV_FLIPOUT_MC = 4 }; /* bnn_conv2d_flipout_forward_mc */
int bnn_conv2d_dense_images(const bnn_conv2d_shape_t *shape, int variant, int nsamples, int shared_x);

/* ---- backward of K2 conv2d through the panel ------------------
 * replaces  autograd through F.conv2d (conv.py:116) for groups == 1, C*KH*KW % 8 == 0.  With
 * M = B*OH*OW rows, K = C*KH*KW, N = O:
 *   rows  = bnn_nchw_to_rows(gy)                 gy (S*B, O, OH*OW) -> (S*B*OH*OW, O), fp32 or bf16
 *   panel = bnn_conv2d_im2col(x)                 (x_samples*M, K), fp32 or bf16 (the forward's panel)
 *   bnn_linear_backward_weight_sampled(panel, rows, ...)   -> g_mu, g_rho of the (O, K) weight
 *   bnn_linear_backward_input_sampled(rows, ...) -> gpanel (S*M, K) fp32
 *   bnn_conv2d_col2im(gpanel)                    -> gx (S | 1, B, C, H, W), gather (no atomics);
 *                                                   shared_x != 0 also sums over the samples.
 * bnn_conv2d_im2col: the panel must be 16-B aligned (BNN_E_UNSUPPORTED otherwise); x on its element (16 bytes and
 * C H W % 4 == 0 buy 16-B image loads). */
int bnn_conv2d_im2col(const float *x, int64_t x_sample_stride, const bnn_conv2d_shape_t *shape,
                      int x_samples, void *panel, int out_bf16, void *stream);
int bnn_conv2d_col2im(const float *gpanel, const bnn_conv2d_shape_t *shape, int nsamples,
                      int shared_x, float *gx, void *stream);
int bnn_nchw_to_rows(const float *y, int64_t images, int channels, int pixels, void *rows,
                     int out_bf16, void *stream);

/* ---- conv3d on drawn weights (NormalConv3d on the device) -------------------------------------------------------------
 *   y[s] = conv3d(x[s | 0], w_s, b_s, stride, padding, dilation, groups), NCDHW activations, OIDHW weights.
 * Implicit GEMMs per (sample, group) with the im2col gather in the loaders' address arithmetic (no panel in memory):
 * forward M = B*OD*OH*OW, N = O/groups, K = (C/groups)*KD*KH*KW.  Every extent is accepted; the refusals are index ranges:
 * a per-sample tensor (x, y, one sample's weights) of 2^31 elements or more, or nsamples * groups > 65535 (BNN_E_RANGE). */
typedef struct bnn_conv3d_shape {
    int64_t B, C, D, H, W;               /* input  (B, C, D, H, W) */
    int64_t O, KD, KH, KW;               /* weight (O, C/groups, KD, KH, KW) */
    int64_t stride_d, stride_h, stride_w, pad_d, pad_h, pad_w, dil_d, dil_h, dil_w, groups;
} bnn_conv3d_shape_t;
/* Forward on the S drawn weights: w sample s at w + s * w_sample_stride elements, O rows of K = (C/groups) KD KH KW
 * (OIDHW order, row pitch K; w_sample_stride 0: one weight for every sample) -- bnn_draw_multi of the posterior as ONE flat row
 * (rows = 1, cols = O K, kind 0, ld = out_sample_stride = roundup(O K, 8) for bf16), so the eps order and the values are
 * K1's and the draw's cols % 4 rule does not apply.  compute BNN_COMPUTE_BF16: w bf16, x rounded to bf16 in the loader,
 * v_mfma_f32_16x16x32_bf16; BNN_COMPUTE_F32: w fp32, v_mfma_f32_16x16x4_f32 (a k-ordered fp32 fma chain).  fp32
 * accumulation.  x fp32 (x_sample_stride = 0: shared by the samples, the first Bayesian layer of a net), b S x O fp32
 * (b_sample_stride) or NULL, y nsamples x B x O x OD x OH x OW fp32.  One launch.
 * replaces  F.conv3d(x, *self.sampled, ...)  pytorch_bayesian/nn/conv.py:138-142 */
int bnn_conv3d_forward_drawn(const float *x, int64_t x_sample_stride, const void *w, int64_t w_sample_stride,
                             const float *b, int64_t b_sample_stride, float *y, const bnn_conv3d_shape_t *shape,
                             int nsamples, int compute, void *stream);
/* Input gradient: gx = the implicit GEMM of gy (nsamples x B x O x OD x OH x OW fp32) with the same weights over the input
 * positions; taps that no stride step reaches contribute zero.  shared_x != 0: gx is B x C x D x H x W, the sum over the
 * samples taken inside the reduction loop in sample order; else nsamples x B x C x D x H x W.  No atomics.  One launch.
 * replaces  autograd through F.conv3d (input)  pytorch_bayesian/nn/conv.py:138-142 */
int bnn_conv3d_backward_input(const float *gy, const void *w, int64_t w_sample_stride, float *gx, int shared_x,
                              const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *stream);
/* Weight and bias gradients: gw[s] = gy[s]^T . gathered x[s | 0], nsamples x O x K fp32 (NULL: bias only), gb[s][o] = the sum of
 * gy[s][.][o] over the positions, nsamples x O fp32 (NULL: none).  The reduction over B*OD*OH*OW is split into slabs taken from
 * the CALLER's workspace (bnn_conv3d_backward_weight_workspace_bytes(shape, nsamples) bytes, 4-B aligned; 0: none needed --
 * a per-call buffer, never the registered one) and summed in slab order.  Bitwise reproducible.  One launch for gw (two with
 * slabs), one for gb.  The posterior gradients follow from bnn_sample_affine_bwd on the recorded keys.
 * replaces  autograd through F.conv3d (weight, bias)  pytorch_bayesian/nn/conv.py:138-142 */
int64_t bnn_conv3d_backward_weight_workspace_bytes(const bnn_conv3d_shape_t *shape, int nsamples);
int bnn_conv3d_backward_weight(const float *x, int64_t x_sample_stride, const float *gy, float *gw, float *gb,
                               const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *workspace,
                               int64_t workspace_bytes, void *stream);

/* ---- Flipout conv3d (FlipOutNormalConv3d on the device), groups == 1 -------------------------------------------------------
 *   y[s][b] = conv3d(x[s | 0][b], mean) + R_s[b] (.) conv3d(x[s | 0][b] (.) S_s[b], stddev),   stddev = 1e-10 + softplus(scale)
 * The K7 tile skeleton with two contractions per tile on one pass over the gathers.  w = [O K mean | O K stddev], OIDHW order,
 * K = C KD KH KW: bf16 rows padded to roundup(O K, 8) (BNN_COMPUTE_BF16) or fp32 rows of O K (BNN_COMPUTE_F32) -- ONE
 * bnn_draw_multi with kinds 1 / 2, rows = 1, nsamples = 1.  signs: the conv layout of the Flipout-sign contract, per sample B rows
 * of O + C fp32 +-1 (R first, then S) -- what bnn_flipout_signs writes -- at sign_sample_stride elements (0: one set for every
 * sample).  Refusals (nothing launched): K7's index ranges and B (O + C) >= 2^31 (BNN_E_RANGE), groups != 1 (BNN_E_UNSUPPORTED).
 * Fixed summation orders, no atomics: identical calls give identical bits.
 * Forward, ONE launch for all samples: x fp32 (x_sample_stride 0: shared), y nsamples x B x O x OD x OH x OW fp32.
 * replaces  FlipOutNormalConv3d.forward  pytorch_bayesian/nn/conv.py:237-251 */
int bnn_conv3d_flipout_forward(const float *x, int64_t x_sample_stride, const void *w, const float *signs, int64_t sign_sample_stride,
                               float *y, const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *stream);
/* Input gradient, ONE launch: gx = dgrad(gy, mean) + S (.) dgrad(gy (.) R, stddev), gy nsamples x B x O x OD x OH x OW fp32.
 * shared_x != 0: gx is B x C x D x H x W, the samples summed inside the kernel in sample order (each sample's S_s fold at its
 * end); else nsamples x B x C x D x H x W.
 * replaces  autograd through FlipOutNormalConv3d.forward (input)  pytorch_bayesian/nn/conv.py:237-251 */
int bnn_conv3d_flipout_backward_input(const float *gy, const void *w, const float *signs, int64_t sign_sample_stride, float *gx,
                                      int shared_x, const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *stream);
/* Posterior gradients, TWO launches: one slab launch computes g_mean_s = wgrad(x, gy_s) and g_stddev_s = wgrad(x (.) S_s, gy_s (.) R_s)
 * from one pass over the gathers into the CALLER's workspace (bnn_conv3d_flipout_backward_weight_workspace_bytes(shape, nsamples)
 * bytes, 4-B aligned, always needed; -1 where the entries refuse the shape); one reduce launch writes
 *   g_mean = sum_s g_mean_s,   g_scale = (sum_s g_stddev_s) (.) softplus'(rho)   (torch's softplus backward, threshold 20),
 * samples in order, each sample's slabs in slab order.  rho, g_mean, g_scale: O x K fp32.
 * replaces  autograd through FlipOutNormalConv3d.forward (weight.mean, weight.scale)  pytorch_bayesian/nn/conv.py:237-251 */
int64_t bnn_conv3d_flipout_backward_weight_workspace_bytes(const bnn_conv3d_shape_t *shape, int nsamples);
int bnn_conv3d_flipout_backward_weight(const float *x, int64_t x_sample_stride, const float *gy, const float *signs,
                                       int64_t sign_sample_stride, const float *rho, float *g_mean, float *g_scale,
                                       const bnn_conv3d_shape_t *shape, int nsamples, int compute, void *workspace,
                                       int64_t workspace_bytes, void *stream);

/* ---- diagnostics ------------------------------------------------------------
 * VALU cost of the draw, no memory traffic: `blocks` workgroups of 256 threads each run
 * `iters` Philox blocks (4 draws) of stage 0 (Philox4x32-10 only), 1 (+ Box-Muller),
 * 2 (+ softplus sigma), 3 (+ fma = full draw); out needs blocks * 256 floats. */
int bnn_diag_sampler(float *out, int blocks, int iters, int stage, void *stream);
/* L2 -> CU activation stream in the access shapes of the fused linear kernel: S * (M / rows_per_wg)
 * * ntn workgroups of nwaves waves each read their (rows_per_wg x K) block of x (S, M, K) once.
 * pattern 0: MFMA-fragment shaped loads; 1: row-contiguous loads; 2: row-contiguous LDS-DMA.
 * out needs grid * nwaves * 64 floats. */
int bnn_diag_astream(const float *x, int S, int M, int K, int rows_per_wg, int ntn, int pattern,
                     int nwaves, float *out, void *stream);

/* ---- training-loop callers (either side of the backward path) ----------------
 * replaces  torch.optim.Adam(model.parameters(), lr).step()   examples/MNIST/train.py:41,65
 *   g += wd p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),   t = *step + 1; then *step += 1.
 * All tensors of the model in ONE launch (+ the 1-thread counter bump); `step` is a device float so
 * that a captured graph advances it. */
typedef struct bnn_adam_tensor {
    float *p;
    const float *g;
    float *m;
    float *v;
    int64_t n;
} bnn_adam_tensor_t;
int bnn_adam_step(const bnn_adam_tensor_t *tensors, int ntensors, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float *step, void *stream);
/* The same step, and advance_epoch[0] += advance_inc (may be NULL) in its last launch: the optimizer step is the end of
 * a training step (every draw of the step, forward and backward, has been consumed by then), so the fresh-noise bump of a
 * captured step needs no launch of its own (bnn_rng_advance). */
int bnn_adam_step_advance(const bnn_adam_tensor_t *tensors, int ntensors, float lr, float beta1, float beta2,
                          float eps, float weight_decay, float *step, uint32_t *advance_epoch,
                          uint32_t advance_inc, void *stream);
/* replaces  torch.nn.CrossEntropyLoss()(pred, y)   examples/MNIST/train.py:39,59-61  (reduction 'mean'):
 *   loss[0] = mean_r (logsumexp(x_r) - x_r[y_r]);  g_logits (may be NULL) = (softmax(x_r) - onehot(y_r)) / rows.
 * logits (rows, classes) fp32 row-major, target int64; workspace: bnn_xent_workspace_bytes(rows).
 * The row loss is formed as ln(sum_c exp(x_c - max)) - (x_y - max): it rounds at the magnitude of the loss, not of the logits.
 * A target outside [0, classes) -- compared as int64, before any narrowing; ignore_index is NOT supported -- makes that
 * row's loss NaN, hence loss[0], and its row of g_logits NaN; nothing outside the row is read, every other gradient row is
 * what it would be without it.  Checked on the device: no host synchronisation, the call stays graph-capturable. */
int64_t bnn_xent_workspace_bytes(int64_t rows);
int bnn_softmax_xent(const float *logits, const int64_t *target, int64_t rows, int classes,
                     float *loss, float *g_logits, void *workspace, void *stream);

/* ---- pruning score --------------------------------------------
 * replaces  param.dist.log_prob(0)   pytorch_bayesian/prune/prune.py:11
 *   out[i] = log N(0; mu[i], sigma(rho[i])) = -mu^2 / (2 sigma^2) - ln sigma - ln sqrt(2 pi)
 * (the top-k selection and the masked assignment of prune.py:12-17 stay torch ops on the device). */
int bnn_prune_score(const float *mu, const float *rho, float *out, int64_t n, void *stream);

/* ---- MC dropout (dropout-mask contract above) -------------------------------------
 * replaces  F.dropout(self.linear(x), p, sample, False)  pytorch_bayesian/nn/dense.py:174-179
 *           F.dropout(self.conv(x), p, sample, False)    pytorch_bayesian/nn/conv.py:277-326 (MCDropoutConv{1,2,3}d)
 *   y[s][r][f] = keep(s, r, f) ? x[s | 0][r][f] * 1 / (1 - p) : 0,   s < nsamples
 * x: (S, rows, F) at x_sample_stride elements, or SHARED (x_sample_stride = 0: the fan-out of a layer that ran once on the
 * un-replicated batch); y: (S, rows, F) at y_sample_stride.  Contiguous rows.  dtype BNN_F32 or BNN_BF16 (x and y alike; the
 * scaling is fp32).  y may alias x (in place; with x shared, y[0] may be x).  Graph-capturable, no allocation. */
int bnn_mc_dropout(const void *x, int64_t x_sample_stride, void *y, int64_t y_sample_stride, int64_t rows, int64_t features,
                   int nsamples, float p, int dtype, const bnn_rng_t *rng, void *stream);
/* Backward, the mask re-created from the key (never stored): gx[s] = mask_s (.) gy[s] * 1 / (1 - p), fp32.
 * sum_samples != 0 (the input was shared): gx (rows, F) = sum over s = 0 .. nsamples - 1 in that order, fp32 -- bitwise
 * reproducible. */
int bnn_mc_dropout_backward(const float *gy, int64_t gy_sample_stride, float *gx, int64_t gx_sample_stride, int64_t rows,
                            int64_t features, int nsamples, float p, int sum_samples, const bnn_rng_t *rng, void *stream);

/* ---- Flipout signs (Flipout-sign contract above) ---------------------------------
 * out[s][r][j] = sign of element r * width + j of sample rng->sample0 + s, as +-1 fp32, s < nsamples, r < rows, j < width
 * (conv: rows = B, width = O + C; linear: rows = 1, width = O + K); out_sample_stride >= rows * width elements.
 * replaces  (torch.rand(B, O / C, ...) - .5).sign()  pytorch_bayesian/nn/conv.py:154-161, dense.py:70-75, one draw per MC sample */
int bnn_flipout_signs(float *out, int64_t out_sample_stride, int64_t rows, int64_t width, int nsamples, const bnn_rng_t *rng,
                      void *stream);
/* Backward of bnn_draw_multi's BNN_DRAW_FLIPOUT draw (w_s = mu + sigma(rho) (.) R_s S_s^T, O x K), the signs re-created from the key (never stored):
 *   g_mu = sum_s g_w[s],  g_rho = sum_s g_w[s] (.) R_s S_s^T (.) sigmoid(rho),  s = 0 .. nsamples - 1 in that order, fp32.
 * g_w: nsamples x O x K fp32 at g_w_sample_stride elements. */
int bnn_flipout_weight_backward(const float *g_w, int64_t g_w_sample_stride, const float *rho, float *g_mu, float *g_rho,
                                int64_t O, int64_t K, int nsamples, const bnn_rng_t *rng, void *stream);

/* ---- MultivariateNormalLinear (MVN-noise contract above) --------------------------------
 * One full-covariance posterior tensor: mean rows x cols (a weight O x K, or a bias as ONE row of O), scale rows x cols x cols
 * (its lower triangle is read; the upper one never is).  Host struct. */
typedef struct bnn_mvn_tensor {
    const float *mu;            /* rows x cols */
    const float *scale;         /* rows x cols x cols */
    float *out;                 /* bnn_mvn_draw: nsamples x rows x cols at sample_stride elements (written) */
    const float *g_w;           /* bnn_mvn_draw_backward: the gradient of out, same layout (read) */
    float *g_mu;                /* bnn_mvn_draw_backward: rows x cols */
    float *g_scale;             /* bnn_mvn_draw_backward: rows x cols x cols, every element (0 above the diagonal) */
    int64_t sample_stride;
    int64_t rows, cols;
    bnn_rng_t rng;              /* the tensor's key: stream, sample0, epochs, generator */
} bnn_mvn_tensor_t;
/* w_s for s < nsamples of up to 8 tensors (a layer's weight and bias) in ONE launch.  A workgroup owns (tensor, row o, part of
 * the triangle rows): it makes the row's cols x nsamples uniforms once into LDS and streams the lower triangle once, every L
 * computed once and applied to all samples (beyond 16 samples, or cols x samples over 16 K floats, the triangle is streamed
 * once per group of samples).  cols <= 16384.
 * replaces  MultivariateNormalLinear.sample() -> WeightMultivariateNormal.sample()  pytorch_bayesian/nn/dense.py:123-130,
 *           nn/core.py:89-92, once per MC sample */
int bnn_mvn_draw(const bnn_mvn_tensor_t *tensors, int ntensors, int nsamples, void *stream);
/* Backward of bnn_mvn_draw, the uniforms re-created from the keys (never stored):
 *   g_mu = sum_s g_w[s];  g_scale[o][i][j] = (sum_s g_w[s][o][i] u_s[o][j]) sigmoid(scale[o][i][j]) / (2 L[o][i][j]) for j <= i,
 *   exactly 0 for j > i (autograd of the reference expression, where tril masks the gradient).  Sums over s in sample order,
 *   no atomics: bitwise reproducible.  Reads the lower triangle once.  ONE launch.  cols <= 8192. */
int bnn_mvn_draw_backward(const bnn_mvn_tensor_t *tensors, int ntensors, int nsamples, void *stream);

/* One full-covariance posterior against an ISOTROPIC prior MultivariateNormal(loc = prior_mu everywhere, scale_tril =
 * prior_sigma I) -- the default prior of MultivariateNormalLinear is (0, 1).  Host struct. */
typedef struct bnn_mvn_kl_tensor {
    const float *mu;            /* rows x cols */
    const float *scale;         /* rows x cols x cols, lower triangle read */
    float *g_mu;                /* bnn_mvn_kl_backward: rows x cols */
    float *g_scale;             /* bnn_mvn_kl_backward: rows x cols x cols, every element (0 above the diagonal) */
    int64_t rows, cols;
    float prior_mu, prior_sigma;
} bnn_mvn_kl_tensor_t;
/* KL(MVN(mu, scale_tril = V) || prior) in closed form, V = tril(softplus(scale)) + 1e-10 I (the reference's scale_tril is V
 * itself, not its element-wise root), per row o with s0 = prior_sigma, m0 = prior_mu, K = cols:
 *   KL_o = 0.5 (sum_{j <= i} V_ij^2 / s0^2 + sum_i (mu_i - m0)^2 / s0^2 - K) + K ln s0 - sum_i ln V_ii
 * out[t] = the mean of KL_o over the rows of tensor t (what KLDivergence.compute_kl returns for it).  Partial sums per workgroup
 * into the CALLER's workspace (bnn_mvn_kl_workspace_bytes, 8-B aligned; a per-call buffer), summed in fp64 in slot order: no
 * atomics, bitwise reproducible.  Two launches whatever the shapes.
 * replaces  kl_divergence(param.dist, MultivariateNormal(prior...)).mean()  pytorch_bayesian/nn/loss.py:16-28 */
int64_t bnn_mvn_kl_workspace_bytes(const bnn_mvn_kl_tensor_t *tensors, int ntensors);
int bnn_mvn_kl(const bnn_mvn_kl_tensor_t *tensors, int ntensors, float *out, void *workspace, int64_t workspace_bytes,
               void *stream);
/* Backward, g = upstream[t] / rows (upstream: ntensors device floats, NULL = 1):
 *   g_mu = g (mu - m0) / s0^2;   g_scale = g (V_ij / s0^2 - [i == j] / V_ii) sigmoid(scale_ij) for j <= i, 0 above.  ONE launch. */
int bnn_mvn_kl_backward(const bnn_mvn_kl_tensor_t *tensors, int ntensors, const float *upstream, void *stream);

/* ---- MC reduction ----------------------------------------------------------
 * replaces  torch.stack(preds).mean(0)   examples/MNIST/uncertainty.py:50
 *   out[i] (+)= scale * sum_s y[s * y_sample_stride + i],  i < n,  any nsamples >= 1, in a fixed order (bitwise reproducible):
 *     nsamples <= 32: one fp32 sum from +0 in sample order;
 *     nsamples > 32 (e.g. the partial logits of bnn_dense_forward_head): four quarters of ceil(nsamples / 4) consecutive
 *     samples, each summed from +0 in sample order (a quarter may be empty: +0), then ((q0 + q1) + q2) + q3;
 *   then times scale, and (accumulate) added to out[i] -- that add may be fused with the product (one rounding fewer).
 * advance_epoch (may be NULL): advance_epoch[0] += advance_inc in the same launch -- the
 * reduction is the tail of an MC step (every draw of the step has been consumed by the
 * kernels stream-ordered before it), so this saves the separate bnn_rng_advance launch. */
int bnn_mc_sum(const float *y, int64_t y_sample_stride, int nsamples, int64_t n,
               float scale, float *out, int accumulate, uint32_t *advance_epoch,
               uint32_t advance_inc, void *stream);

/* bnn_mc_sum + the second pass of a KL begun by bnn_kl_forward_partial(tensors, ntensors, workspace): kl_out as `out`
 * of bnn_kl_forward (ntensors + 1 floats). */
int bnn_mc_sum_kl(const float *y, int64_t y_sample_stride, int nsamples, int64_t n,
                  float scale, float *out, int accumulate, uint32_t *advance_epoch,
                  uint32_t advance_inc, const bnn_kl_tensor_t *tensors, int ntensors,
                  float n_batches, float *kl_out, const void *workspace, void *stream);

/* Predictive uncertainty of an MC forward in ONE launch: the predictive mean and the split of its entropy into an aleatoric
 * (expected per-sample entropy) and an epistemic part (mutual information, the BALD score).
 * replaces  agg = torch.stack(preds).mean(0); Entropy(dim=-1)(agg)   examples/MNIST/uncertainty.py:47-52
 *   y: nparts * nsamples addends of rows x classes fp32 (row-major, contiguous); addend v = part * nsamples + s starts at
 *   y + v * addend_stride.  A stacked output (S, rows, classes) has nparts = 1; a fused head's partial logits
 *   (bnn_dense_forward_head: parts, S, rows, classes) are first summed over the parts in the order bnn_mc_sum adds `parts`
 *   addends, so the values are bit-identical to bnn_mc_sum over the parts followed by this call.
 *   p_s = softmax(z_s) (kind BNN_UNC_LOGITS, max subtracted first) or z_s as given (BNN_UNC_PROBS, not renormalised);
 *   mean[r, c]   = (1/S) sum_s p_s[c]                 (rows x classes)
 *   aleatoric[r] = (1/S) sum_s H(p_s)                 (rows)
 *   total[r]     = H(mean[r, :])                      (rows)
 *   epistemic[r] = total - aleatoric, taken before the outputs are rounded to fp32
 *   H: BNN_UNC_PROBS  -sum_c p log(p + 1e-10), the convention of Entropy (nn/loss.py), so that total.mean() is
 *                     Entropy(-1)(mean);
 *      BNN_UNC_LOGITS exact Shannon entropy: H(p_s) = lse(z_s) - sum_c p_s[c] z_s[c] (one log per sample and row), and
 *                     0 log 0 = 0 in total.  The two conventions differ by at most classes * 1e-10.
 *   The sums over samples are fp64, in a fixed sample order, without float atomics: bitwise reproducible run to run, and
 *   their error does not grow with S.  1 <= nsamples <= 65536, 1 <= classes <= 4096, 1 <= nparts,
 *   1 <= rows <= 2^31 - 1 (BNN_E_SHAPE / BNN_E_RANGE otherwise).
 * Tails, as in bnn_mc_sum_kl: advance_epoch (may be NULL) += advance_inc in the same launch; kl_tensors != NULL: the second
 * pass of a KL begun by bnn_kl_forward_partial(kl_tensors, kl_ntensors, kl_workspace) runs as one extra workgroup, kl_out
 * as `out` of bnn_kl_forward (kl_ntensors + 1 floats, bit-identical). */
enum { BNN_UNC_LOGITS = 0, BNN_UNC_PROBS = 1 };
int bnn_mc_uncertainty(const float *y, int64_t addend_stride, int nparts, int nsamples, int64_t rows, int classes,
                       int kind /* BNN_UNC_LOGITS 0 | BNN_UNC_PROBS 1 */,
                       float *mean, float *total, float *aleatoric, float *epistemic,
                       uint32_t *advance_epoch, uint32_t advance_inc,
                       const bnn_kl_tensor_t *kl_tensors, int kl_ntensors, float kl_n_batches,
                       float *kl_out, const void *kl_workspace, void *stream);

/* ---- K14: an MC forward scored against its labels ----------------------------------
 * Per row, in ONE launch: the predictive mean, the negative log-likelihood of the MC predictive, the expected per-sample NLL,
 * the Brier score, the confidence, the prediction and the entropy; with a `state`, a second one-workgroup launch adds the
 * batch to a device accumulator that carries a whole test set (sums, reliability and rejection histograms).
 * replaces  the per-batch stack / mean / argmax / compare / host sum of examples/MNIST/prune.py:52-65
 *   y, addend_stride, nparts, nsamples, rows, classes, kind: as bnn_mc_uncertainty (a fused head's partials are first summed
 *   over the parts in bnn_mc_sum's order), but classes >= 2.  target: rows int64 labels.  With p_s the per-sample
 *   probabilities and m = (1/S) sum_s p_s, every output may be NULL and is then not written; fp32 except `prediction`:
 *   mean (rows x classes)  m: the bits bnn_mc_uncertainty writes as `mean`
 *   nll[r]           -ln m[y_r].  LOGITS: -(logsumexp_s(z_s[y] - lse(z_s)) - ln S), formed in the log domain: finite and
 *                    accurate where p_s[y] underflows fp32 (+inf only where no sample gives the label any mass).
 *                    PROBS: -ln(m[y] + 1e-10), the convention of Entropy (nn/loss.py).
 *   expected_nll[r]  -(1/S) sum_s ln p_s[y_r], the data term of the ELBO.  LOGITS: exact, each term ln(sum e) - (z[y] - max) as
 *                    bnn_softmax_xent forms its row loss.  PROBS: ln(p + 1e-10).
 *   brier[r]         sum_c (m[c] - [c = y_r])^2
 *   confidence[r]    max_c mean[r, c] (of the fp32 values written);  prediction[r] (int64): the lowest c attaining it.  The
 *                    row is correct where prediction == target.
 *   entropy[r]       H(m): the bits bnn_mc_uncertainty writes as `total` for the same kind.
 *   A target outside [0, classes) -- compared as int64 before any narrowing; there is no ignore_index -- makes that row's
 *   nll, expected_nll and brier NaN and the row not correct; nothing outside the row is read or changed, every other row keeps
 *   its bits, and no host synchronisation is involved.
 *   Per-sample terms fp32, sums over samples fp64 in a fixed order, no float atomics: bitwise reproducible.
 * state (may be NULL; bnn_mc_score_state_doubles(conf_bins, ent_bins) = 5 + 3 conf_bins + 2 ent_bins doubles, zeroed by the
 * caller once): the launch ADDS this batch --
 *   [n, sum nll, sum expected_nll, sum brier, sum correct], then per confidence bin (count, sum confidence, sum correct), then
 *   per entropy bin (count, sum correct).  Equal-width bins of the fp32 values written: confidence bin = min(conf_bins - 1,
 *   floor(confidence conf_bins)), entropy bin = clamp(floor(entropy / ln(classes) ent_bins), 0, ent_bins - 1);
 *   1 <= conf_bins, ent_bins <= 128.  An invalid target makes the three sums NaN; the row still counts in n and in its bins.
 *   The main launch leaves five words per row in `workspace` (bnn_mc_score_workspace_bytes(rows) = 20 rows bytes, 4-B aligned;
 *   required with a state) and one workgroup adds them in a fixed order: the counts are integers, the confidence sums 2^-31
 *   fixed point (confidences clamped to [0, 2] for the sum; within 2^-32 per row), the three other sums fp64.  Bitwise
 *   reproducible.  That pass reads 20 bytes per row through one workgroup: sized for evaluation batches.
 * advance_epoch (may be NULL) += advance_inc in the main launch, as in bnn_mc_uncertainty; there is no KL tail.
 * Launches: one without a state, two with it.  Errors (nothing launched): BNN_E_NULL (y, target; workspace with a state),
 * BNN_E_SHAPE / BNN_E_RANGE (extents as bnn_mc_uncertainty, classes < 2, bins outside 1 .. 128), BNN_E_ALIGN. */
int64_t bnn_mc_score_state_doubles(int conf_bins, int ent_bins);       /* 0 for bins outside 1 .. 128 */
int64_t bnn_mc_score_workspace_bytes(int64_t rows);                    /* 0 for rows outside 1 .. 2^31 - 1 */
int bnn_mc_score(const float *y, int64_t addend_stride, int nparts, int nsamples, int64_t rows, int classes,
                 int kind /* BNN_UNC_LOGITS 0 | BNN_UNC_PROBS 1 */, const int64_t *target,
                 float *mean, float *nll, float *expected_nll, float *brier, float *confidence, int64_t *prediction,
                 float *entropy, double *state /* may be NULL */, int conf_bins, int ent_bins, void *workspace,
                 uint32_t *advance_epoch, uint32_t advance_inc, void *stream);

/* ---- K12: the regression tail of an MC forward -------------------------------------
 * Predictive mean and variance decomposition of S stacked regression outputs in ONE launch: the moments of the equal-weight
 * mixture of the S per-sample predictives (law of total variance).
 * replaces  the mean / aleatoric / epistemic bands of examples/Simple/uncertainty.py over torch.stack(preds)
 *   y, addend_stride, nparts, nsamples, rows: as bnn_mc_uncertainty (a fused head's partials are first summed over the parts in
 *   bnn_mc_sum's order, bit-identical to bnn_mc_sum over the parts followed by this call); width: floats per row.
 *   kind BNN_REG_VALUES       D = width      m_s = y_s                    v_s = 0
 *        BNN_REG_MEAN_LOGVAR  D = width / 2  m_s = y_s[:D]                v_s = exp(y_s[D:])   (one v_exp_f32 per element)
 *        BNN_REG_MEAN_VAR     D = width / 2  m_s = y_s[:D]                v_s = y_s[D:] as given
 *   mean      = (1/S) sum_s m_s                  aleatoric = (1/S) sum_s v_s
 *   epistemic = (1/S) sum_s (m_s - mean)^2  (population variance: exactly 0 for S = 1; never negative)
 *   total     = aleatoric + epistemic, added before the outputs are rounded to fp32.       All four: rows x D fp32.
 *   The sums over samples are fp64 in a fixed order, without float atomics: bitwise reproducible.  The variance of the means is
 *   taken on m_s - m_0 (sample 0's value), so it keeps its relative accuracy when |mean| is large against the spread.
 *   1 <= nsamples <= 65536, 1 <= width <= 4096 (even for the two (mean, variance) kinds), 1 <= nparts, 1 <= rows <= 2^31 - 1
 *   (BNN_E_SHAPE / BNN_E_RANGE otherwise, nothing launched).  Tails: as bnn_mc_uncertainty. */
enum { BNN_REG_VALUES = 0, BNN_REG_MEAN_LOGVAR = 1, BNN_REG_MEAN_VAR = 2 };
int bnn_mc_regression(const float *y, int64_t addend_stride, int nparts, int nsamples, int64_t rows, int width,
                      int kind /* BNN_REG_VALUES 0 | BNN_REG_MEAN_LOGVAR 1 | BNN_REG_MEAN_VAR 2 */,
                      float *mean, float *total, float *aleatoric, float *epistemic,
                      uint32_t *advance_epoch, uint32_t advance_inc,
                      const bnn_kl_tensor_t *kl_tensors, int kl_ntensors, float kl_n_batches,
                      float *kl_out, const void *kl_workspace, void *stream);

/* The heteroscedastic Gaussian likelihood of a (mean, log-variance) head over the stacked MC samples, loss and gradient in one
 * pass (no constant term).
 * replaces  torch.nn.functional.gaussian_nll_loss(m, t, exp(s), full=False, reduction='mean') and its autograd
 *   y (nsamples, rows, width = 2 D) fp32 contiguous: D means then D log-variances s; target (rows, D) fp32, read once per
 *   sample, never expanded.  With r = target - m and N = nsamples rows D:
 *   loss[0] = (1/N) sum 0.5 (s + r^2 exp(-s));   g_y (may be NULL; y's layout): -r exp(-s) / N | 0.5 (1 - r^2 exp(-s)) / N.
 * Terms in fp32; the sum as per-workgroup fp64 partials into `workspace` (the workspace-bytes query below, 8-B aligned), added
 * in index order by a second one-workgroup launch: no float atomics, bitwise reproducible.  Errors as above (odd width: BNN_E_SHAPE). */
int64_t bnn_gaussian_nll_workspace_bytes(int64_t nsamples, int64_t rows, int width);
int bnn_gaussian_nll(const float *y, int nsamples, int64_t rows, int width, const float *target,
                     float *loss, float *g_y /* may be NULL */, void *workspace, void *stream);

/* ---- K15: a regression MC forward scored against its targets -------------------------
 * Per row and predicted quantity, in ONE launch: the predictive mean and variance, the squared error, the negative
 * log-likelihood of the MC predictive -- the equal-weight mixture of the S per-sample Gaussians --, that of the moment-matched
 * Gaussian, the mixture's CRPS and its probability integral transform (PIT); with a `state`, a second launch adds the batch to
 * a device accumulator that carries a whole test set (sums and the PIT histogram per predicted quantity).
 * replaces  pulling the stacked outputs back and a dozen small torch launches per batch, the O(S^2) pair term among them
 *   y, addend_stride, nparts, nsamples, rows, width, kind, D and the per-sample (m_s, v_s): as bnn_mc_regression (a fused head's
 *   partials are first summed over the parts in bnn_mc_sum's order), but 1 <= nsamples <= 1024 (BNN_E_RANGE above: the pair sum
 *   is quadratic in S).  target: rows x D fp32.  Every output is rows x D fp32, may be NULL and is then not written.  With
 *   t = target[r, d], Phi / phi the standard normal cdf / pdf, sg_s = sqrt(v_s):
 *   mean, variance   the bits bnn_mc_regression writes as `mean` and `total`
 *   sq_err           (mean - t)^2, of the fp64 mean before it is rounded
 *   gaussian_nll     (ln(2 pi V) + (t - mean)^2 / V) / 2 with V the fp64 total variance; NaN where V == 0
 *   nll              -(logsumexp_s l_s - ln S), l_s = -(ln 2 pi + ln v_s + (t - m_s)^2 / v_s) / 2, formed in the log domain.
 *                    MEAN_LOGVAR: ln v_s is the input s itself and (t - m_s)^2 / v_s = ((t - m_s) e^(-s / 2))^2, finite for a
 *                    log-variance far below fp32's exp range (down to -176).  MEAN_VAR: v_s <= 0 or NaN gives NaN.  VALUES has
 *                    no mixture density: written with gaussian_nll's bits.
 *   crps             (1/S) sum_s A(t - m_s, v_s) - (1 / 2 S^2) sum_i sum_j A(m_i - m_j, v_i + v_j)   (Grimit et al. 2006) with
 *                    A(mu, sg^2) = mu (2 Phi(mu / sg) - 1) + 2 sg phi(mu / sg), A(mu, 0) = |mu|: the ensemble CRPS for VALUES.
 *                    A negative or NaN v_s gives NaN.
 *   pit              (1/S) sum_s Phi((t - m_s) / sg_s); a zero-variance sample adds [t > m_s] + [t == m_s] / 2 (VALUES: the
 *                    ensemble's empirical cdf with mid-point ties).  A negative or NaN v_s gives NaN.
 *   A NaN target makes that element's sq_err, nll, gaussian_nll, crps and pit NaN; nothing outside the element changes, every
 *   other element keeps its bits, and no host synchronisation is involved.  Infinite targets follow IEEE.
 *   Per-term arithmetic fp32 (erf, exp, log, sqrt); every sum over samples and over pairs fp64 in a fixed order, no float
 *   atomics: bitwise reproducible.  The pair sum takes every unordered pair once and costs O(S^2 rows D).
 * state (may be NULL; bnn_mc_regression_score_state_doubles(D, pit_bins) = D (6 + pit_bins) doubles, zeroed by the caller
 * once): per predicted quantity d the launch ADDS [n, sum sq_err, sum nll, sum gaussian_nll, sum crps, sum variance], then
 *   pit_bins counts: bin = min(pit_bins - 1, floor(pit pit_bins)) of the fp32 pit written, 1 <= pit_bins <= 128.  The sums are
 *   of the fp32 values written; a NaN pit counts in n and in no bin; a NaN element makes its d's affected sums NaN.  Counts are
 *   exact integers, the sums fp64 in a fixed order.
 * workspace: bnn_mc_regression_score_workspace_bytes(...) bytes, 4-B aligned (16-B for 16-B loads), required whenever that
 *   query is non-zero (BNN_E_NULL otherwise): nsamples rows width floats where nparts > 1 -- the parts are added once, not once
 *   per pair --, then 6 rows D floats with a state, which a second launch of D workgroups adds to `state`.
 * advance_epoch (may be NULL) += advance_inc in the main launch, as in bnn_mc_score; there is no KL tail.
 * Launches: one without a state, two with it.  Errors (nothing launched): BNN_E_NULL (y, target, a needed workspace),
 * BNN_E_SHAPE / BNN_E_RANGE (extents as bnn_mc_regression, nsamples > 1024, unknown kind, odd width for a (mean, variance) kind,
 * bins outside 1 .. 128 with a state), BNN_E_ALIGN (state 8 B, workspace 4 B).
 * Not covered: the evidential head's Student-t predictive, a KL tail, S above 1024. */
int64_t bnn_mc_regression_score_state_doubles(int D, int pit_bins);    /* D * (6 + pit_bins); 0 for D outside 1 .. 4096 or bins outside 1 .. 128 */
int64_t bnn_mc_regression_score_workspace_bytes(int nparts, int nsamples, int64_t rows, int width, int kind, int with_state);
                                                                       /* may be 0 without a state; 0 for bad extents */
int bnn_mc_regression_score(const float *y, int64_t addend_stride, int nparts, int nsamples, int64_t rows, int width,
                            int kind /* BNN_REG_VALUES 0 | BNN_REG_MEAN_LOGVAR 1 | BNN_REG_MEAN_VAR 2 */,
                            const float *target /* rows x D */,
                            float *mean, float *variance, float *sq_err, float *nll, float *gaussian_nll, float *crps, float *pit,
                            double *state /* may be NULL */, int pit_bins, void *workspace,
                            uint32_t *advance_epoch, uint32_t advance_inc, void *stream);

/* ---- K13: evidential regression (the Normal-Inverse-Gamma head of examples/Simple) ----------------------------------
 * The head's activation.  replaces  the split / softplus / offsets of NormalInverseGaussianLinear.forward (nn/dense.py:141-162)
 *   z (rows, 4 D) fp32 contiguous, the output of the head's Linear.  One launch writes four contiguous (rows, D) tensors:
 *   gamma = z[:, 0:D];  upsilon = 1e-10 + softplus(z[:, D:2D]);  alpha = 1 + 1e-10 + softplus(z[:, 2D:3D]);
 *   beta = 1e-10 + softplus(z[:, 3D:4D]).  Softplus: torch's (beta 1, threshold 20: z > 20 gives z), log1pf(expf(z)) below.
 *   1 <= rows <= 2^31 - 1, 1 <= D <= 4096 (BNN_E_SHAPE / BNN_E_RANGE otherwise, nothing launched). */
int bnn_nig_head_forward(const float *z, int64_t rows, int D, float *gamma, float *upsilon, float *alpha, float *beta,
                         void *stream);
/* g_z (rows, 4 D) = [g_gamma | g_upsilon sigmoid(z_u) | g_alpha sigmoid(z_a) | g_beta sigmoid(z_b)] in one launch; the derivative
 * of the softplus is 1 above the threshold.  Each incoming gradient ((rows, D) contiguous) may be NULL = zero. */
int bnn_nig_head_backward(const float *z, const float *g_gamma, const float *g_upsilon, const float *g_alpha,
                          const float *g_beta, int64_t rows, int D, float *g_z, void *stream);

/* The evidential loss and its four gradients in one pass.
 * replaces  NormalInverseGaussianLoss.forward (nn/loss.py:54-69) and its autograd
 *   loss[0] = mean(nll) + reg_lambda mean(|y - gamma| (2 upsilon + alpha)) over n elements (five fp32 arrays of n), with
 *   nll = 0.5 ln(pi / upsilon) - alpha ln omega + (alpha + 0.5) ln(upsilon (y - gamma)^2 + omega) + lgamma(alpha) - lgamma(alpha + 0.5),
 *   omega = 2 beta (1 + upsilon).  g_gamma, g_upsilon, g_alpha, g_beta (n fp32 each): d loss / d input; each may be NULL and is
 *   then neither computed nor written.  y carries no gradient; d|y - gamma| at 0 is 0 (torch.abs).
 * Every element is evaluated in fp64 (the differences of lgamma and of digamma cancel for large alpha); the sum as
 * per-workgroup fp64 partials into `workspace` (bnn_nig_loss_workspace_bytes(n) bytes, 8-B aligned), added in a fixed order by a
 * second one-workgroup launch: no float atomics, bitwise reproducible.  n >= 1 (BNN_E_SHAPE otherwise; the query returns 0). */
int64_t bnn_nig_loss_workspace_bytes(int64_t n);
int bnn_nig_loss(const float *gamma, const float *upsilon, const float *alpha, const float *beta, const float *y, int64_t n,
                 double reg_lambda /* a double: the reference multiplies by the Python float */, float *loss,
                 float *g_gamma /* may be NULL */, float *g_upsilon /* may be NULL */,
                 float *g_alpha /* may be NULL */, float *g_beta /* may be NULL */, void *workspace, void *stream);

/* The moments of the equal-weight mixture of S NIG heads over a leading MC axis in ONE launch (law of total variance).
 *   gamma, upsilon, alpha, beta: (nsamples, rows, D) fp32, sample s at + s * sample_stride elements (>= rows * D).
 *   a_s = beta / (alpha - 1), e_s = a_s / upsilon: NormalInverseGaussianUncertainty (nn/loss.py:72-79) per sample, in fp32.
 *   mean = (1/S) sum gamma_s;  aleatoric = (1/S) sum a_s;  epistemic = (1/S) sum e_s + Var_s(gamma_s);  total = aleatoric +
 *   epistemic, added before the outputs are rounded to fp32.  All four: rows x D fp32.  Var_s as in bnn_mc_regression: on
 *   gamma_s - gamma_0, fp64, clamped at 0.  nsamples = 1 gives gamma and that module's two outputs exactly.
 *   Sums over samples fp64 in a fixed order, no float atomics: bitwise reproducible.
 *   1 <= nsamples <= 65536, 1 <= D <= 4096, 1 <= rows <= 2^31 - 1 (BNN_E_SHAPE / BNN_E_RANGE otherwise, nothing launched). */
int bnn_mc_evidential(const float *gamma, const float *upsilon, const float *alpha, const float *beta, int64_t sample_stride,
                      int nsamples, int64_t rows, int D, float *mean, float *total, float *aleatoric, float *epistemic,
                      void *stream);

/* ---- K10: local reparameterization (LocalReparamLinear, bayesianneuralnetworks_amd/nn/dense.py; Kingma, Salimans, Welling 2015,
 * "Variational Dropout and the Local Reparameterization Trick").  The layer has no call site in the reference: it is the other
 * estimator of NormalLinear's posterior (pytorch_bayesian/nn/dense.py:27-60).  With w ~ N(mu_w, sigma_w^2), b ~ N(mu_b, sigma_b^2)
 * independent, y = x w^T + b is Gaussian per output element:
 *     m = x mu_w^T + mu_b                      (mean contraction)
 *     v = x^2 (sigma_w^2)^T + sigma_b^2        (variance contraction, x^2 element-wise)
 *     y_s = m + sqrt(v + 1e-16) eps_s          eps_s ~ N(0, 1): the LRT-noise contract above
 * Both contractions of a pair run in one tile from one pass over the shared operand (x is squared in fp32 before any rounding).
 * compute: BNN_COMPUTE_F32 = fp32 operands on v_mfma_f32_16x16x4_f32, an ordered fp32 fma chain per output element;
 * BNN_COMPUTE_BF16 = every operand rounded to bf16 (RNE) as it is staged, v_mfma_f32_16x16x32_bf16, fp32 accumulate.  No
 * atomics and no split contraction: identical calls give identical bits.  Errors (nothing launched): BNN_E_NULL, BNN_E_SHAPE
 * (extent < 1, ldx < K), BNN_E_RANGE (more than 65535 samples, B N >= 2^32, rows > 64 * 65535, bad rng), BNN_E_DTYPE (compute),
 * BNN_E_UNSUPPORTED (bf16 activations in the fp32 mode), BNN_E_ALIGN (element alignment; 16 bytes for every output).
 *
 * bnn_lrt_prepare: s2_w[i] = sigma(rho_w[i])^2 for i < n_w and s2_b likewise (n_b may be 0), sigma = 1e-10 + softplus(rho):
 * the variance operands of one forward and its backward, one launch. */
int bnn_lrt_prepare(const float *rho_w, float *s2_w, int64_t n_w, const float *rho_b, float *s2_b, int64_t n_b, void *stream);
/* y_s = m + sqrt(v + 1e-16) eps_s for s = 0 .. nsamples - 1, ONE launch.  mu_w, s2_w: (N, K) fp32; mu_b, s2_b: (N) fp32, both
 * or neither.  shared_x != 0: x is (B, K) (row pitch ldx) and serves every sample -- m and v are contracted once and the
 * workgroup loops over the samples in its epilogue only; otherwise x is (nsamples B, K), rows [s B, (s + 1) B) belong to
 * sample s, and the sample is a grid dimension.  y: (nsamples B, N), rows [s B, (s + 1) B) sample s.  v_out (may be NULL):
 * v, (B, N) for a shared x, (nsamples B, N) otherwise -- what bnn_lrt_backward_epilogue reads.
 * flags: BNN_FLAG_X_BF16 = x is bf16, BNN_FLAG_Y_BF16 = y is written as bf16 (bf16 compute only). */
int bnn_lrt_forward(const void *x, int64_t ldx, const float *mu_w, const float *s2_w, const float *mu_b, const float *s2_b,
                    void *y, float *v_out, int64_t B, int64_t N, int64_t K, int nsamples, int shared_x,
                    const bnn_rng_t *rng, int compute, int flags, void *stream);
/* The elementwise part of the backward, eps re-created from the key:
 *     g_m = sum_s gy_s,   g_v = sum_s gy_s eps_s / (2 sqrt(v + 1e-16))     shared_x: (B, N), the sum in sample order
 *     g_m[s] = gy_s,      g_v[s] = gy_s eps_s / (2 sqrt(v_s + 1e-16))      otherwise: (nsamples B, N)
 * gy: (nsamples B, N), fp32 or (BNN_FLAG_X_BF16) bf16; v as bnn_lrt_forward stored it; g_m, g_v fp32. */
int bnn_lrt_backward_epilogue(const void *gy, const float *v, float *g_m, float *g_v, int64_t B, int64_t N, int nsamples,
                              int shared_x, const bnn_rng_t *rng, int flags, void *stream);
/* g_x = g_m mu_w + 2 x (.) (g_v sigma_w^2): both contractions (over n) in one tile, the product with 2 x in the epilogue.
 * g_m, g_v: (M, N) fp32; x: (M, K) fp32 or (BNN_FLAG_X_BF16) bf16, row pitch ldx; gx: (M, K) fp32 or (BNN_FLAG_Y_BF16) bf16.
 * M = B for a shared input (one sample's size), nsamples B otherwise (per row). */
int bnn_lrt_backward_input(const float *g_m, const float *g_v, const float *mu_w, const float *s2_w, const void *x, int64_t ldx,
                           void *gx, int64_t M, int64_t N, int64_t K, int compute, int flags, void *stream);
/* g_mu_w = g_m^T x and g(sigma_w^2) = g_v^T x^2 in one tile (the contraction runs over all M rows in row order), then
 * g_rho_w = g(sigma_w^2) 2 sigma_w sigmoid(rho_w) in the epilogue.  Bias (rho_b, g_mu_b, g_rho_b all given, or all NULL), a second
 * launch: g_mu_b = sum_rows g_m, g_rho_b = (sum_rows g_v) 2 sigma_b sigmoid(rho_b), rows added in a fixed order.
 * flags: BNN_FLAG_X_BF16 = x is bf16. */
int bnn_lrt_backward_weight(const void *x, int64_t ldx, const float *g_m, const float *g_v, const float *rho_w, float *g_mu_w,
                            float *g_rho_w, const float *rho_b, float *g_mu_b, float *g_rho_b, int64_t M, int64_t N, int64_t K,
                            int compute, int flags, void *stream);

/* ---- K11: local reparameterization for convolutions (LocalReparamConv1d / 2d / 3d, bayesianneuralnetworks_amd/nn/conv.py).
 * Like K10 the layer has no call site in the reference: it is the other estimator of NormalConvNd's posterior
 * (pytorch_bayesian/nn/conv.py:43-142).  Per output element the pre-activation of a conv with independent Gaussian weights is
 * Gaussian with
 *     m = convNd(x,   mu_w,      mu_b)
 *     v = convNd(x^2, sigma_w^2, sigma_b^2)
 *     y_s = m + sqrt(v + 1e-16) eps_s          eps_s ~ N(0, 1): the LRT-conv noise contract above
 * (the noise of different output positions is independent, which weight sampling's is not: the usual LRT-for-conv
 * approximation).  One paired-contraction implicit-GEMM tile on K7's skeleton (128 x 64 x 32, im2col in the loader's address
 * arithmetic, no panel): both contractions from one pass over the gathers, the second operand copy squared in fp32 before any
 * rounding.  sigma_w^2 / sigma_b^2 are bnn_lrt_prepare's fp32 values.  compute: BNN_COMPUTE_F32 = v_mfma_f32_16x16x4_f32;
 * BNN_COMPUTE_BF16 = every operand (x, x^2, g_m, g_v, mu_w, the fp32 sigma_w^2) rounded to bf16 (RNE) as it is written to LDS,
 * v_mfma_f32_16x16x32_bf16, fp32 accumulate.  Fixed summation orders, no atomics: identical calls give identical bits, and a
 * shared input gives the bits of the same images given per sample.  1-d and 2-d layers: unit depth / height.
 * Errors (nothing launched): K7's -- BNN_E_NULL, BNN_E_SHAPE (extents, groups not dividing the channels), BNN_E_DTYPE (compute),
 * BNN_E_RANGE (a per-sample tensor of 2^31 elements or more, so B O P < 2^32; nsamples * groups > 65535; bad rng), BNN_E_ALIGN
 * (4 bytes; 16 bytes for y and v_out), BNN_E_UNSUPPORTED (workspace too small).
 *
 * Forward, ONE launch for all nsamples samples.  x: fp32 NCDHW, x_sample_stride == 0: (B, C, D, H, W) serves every sample -- m
 * and v are contracted ONCE and the workgroup loops over the samples in its epilogue only; otherwise sample s starts at
 * x + s * x_sample_stride and the sample is a grid dimension.  mu_w, s2_w: (O, C / groups, KD, KH, KW) fp32; mu_b, s2_b: (O) fp32,
 * both or neither.  y: (nsamples, B, O, OD, OH, OW) fp32.  v_out (may be NULL): v, (B, O, OD, OH, OW) for a shared x, one per
 * sample otherwise -- what the backward epilogue of K10 reads with N = O P. */
int bnn_conv3d_lrt_forward(const float *x, int64_t x_sample_stride, const float *mu_w, const float *s2_w, const float *mu_b,
                           const float *s2_b, float *y, float *v_out, const bnn_conv3d_shape_t *shape, int nsamples,
                           const bnn_rng_t *rng, int compute, void *stream);
/* g_x = convNd^T(g_m, mu_w) + 2 x (.) convNd^T(g_v, sigma_w^2): both transposed contractions in one tile, the product with 2 x
 * in the epilogue.  nsets image sets, each of the shape's B images: 1 for a shared input (g_m, g_v are sums over the samples),
 * the sample count for a per-sample input.  g_m, g_v: (nsets, B, O, OD, OH, OW); x, gx: (nsets, B, C, D, H, W), contiguous. */
int bnn_conv3d_lrt_backward_input(const float *g_m, const float *g_v, const float *mu_w, const float *s2_w, const float *x,
                                  float *gx, const bnn_conv3d_shape_t *shape, int nsets, int compute, void *stream);
/* g_mu_w = sum over (set, b, position) of gather(x) g_m and g(sigma_w^2) likewise of gather(x)^2 g_v, in one tile; the
 * reduction over the B P positions of a set is split into slabs (caller's workspace, a per-call buffer), every slab adds its
 * share of every set in set order, and a second launch adds the slabs in slab order and writes g_mu_w and
 * g_rho_w = g(sigma_w^2) 2 sigma_w sigmoid(rho_w).  Bias (rho_b, g_mu_b, g_rho_b all given, or all NULL), a third launch:
 * g_mu_b[o] = sum g_m, g_rho_b[o] = (sum g_v) 2 sigma_b sigmoid(rho_b), in a fixed order. */
int64_t bnn_conv3d_lrt_backward_weight_workspace_bytes(const bnn_conv3d_shape_t *shape, int nsets);
int bnn_conv3d_lrt_backward_weight(const float *x, const float *g_m, const float *g_v, const float *rho_w, float *g_mu_w,
                                   float *g_rho_w, const float *rho_b, float *g_mu_b, float *g_rho_b,
                                   const bnn_conv3d_shape_t *shape, int nsets, int compute, void *workspace,
                                   int64_t workspace_bytes, void *stream);

/* ---- K16: sampling-free inference, moment propagation through dense layers (csrc/bnn_moments.hip; ops.moments_linear,
 * BayesianNetworkModule.predictive_moments).  No call site in the reference: one pass carries a mean and a variance per
 * activation (independent across elements) through NormalLinear / LocalReparamLinear's posterior, w ~ N(mu_w, sigma_w^2),
 * b ~ N(mu_b, sigma_b^2), sigma^2 = bnn_lrt_prepare's fp32 values:
 *     m = a_m mu_w^T + mu_b
 *     v = a_m^2 (sigma_w^2)^T + a_v (mu_w^2 + sigma_w^2)^T + sigma_b^2      (second term absent when a_v is NULL)
 * Three contractions in one 64 x 64 tile from one pass over the operands; a_m^2 and mu_w^2 + sigma_w^2 (one fma) are formed in fp32
 * by the loader before any rounding; both variance contractions add into one accumulator set; every addend of v is >= 0.
 * compute: BNN_COMPUTE_F32 = v_mfma_f32_16x16x4_f32 (an ordered fp32 fma chain per output element); BNN_COMPUTE_BF16 = all six
 * planes rounded to bf16 (RNE) as they are staged, v_mfma_f32_16x16x32_bf16, fp32 accumulate.  No atomics and no split
 * contraction: identical calls give identical bits.  Every entry is graph-capturable and returns its errors before launching.
 *
 * a_m: (B, K) fp32, or bf16 with BNN_FLAG_X_BF16 (bf16 compute and a_v == NULL only); a_v: (B, K) fp32 or NULL (a deterministic
 * input); both with row pitch lda.  mu_w, s2_w: (N, K) fp32; mu_b, s2_b: (N) fp32, both or neither.  out_m, out_v: (B, N) fp32.
 * BNN_FLAG_RELU: the moment-matched ReLU below in the epilogue.
 * Errors: BNN_E_NULL, BNN_E_SHAPE (extent < 1, lda < K), BNN_E_RANGE (rows > 64 * 65535), BNN_E_DTYPE (compute),
 * BNN_E_UNSUPPORTED (unknown flag; a bf16 a_m in the fp32 mode or beside a_v), BNN_E_ALIGN (element; 16 bytes for the outputs). */
int bnn_moments_forward(const void *a_m, const float *a_v, int64_t lda, const float *mu_w, const float *s2_w, const float *mu_b,
                        const float *s2_b, float *out_m, float *out_v, int64_t B, int64_t N, int64_t K, int compute, int flags,
                        void *stream);
/* ReLU of a Gaussian N(m, v) by moment matching, s = sqrt(v), alpha = m / s, Phi / phi the standard normal cdf / pdf:
 *     mean' = s (alpha Phi + phi)      var' = v (Phi + alpha^2 Phi Phi(-alpha) + alpha phi (Phi(-alpha) - Phi) - phi^2), clamped at 0
 * v == 0 gives (max(m, 0), 0).  n elements, in place allowed.  The device function is the forward's epilogue's: same bits. */
int bnn_moments_relu(const float *m, const float *v, float *out_m, float *out_v, int64_t n, void *stream);
/* y_s[e] = m[e] + sqrt(v[e] + 1e-16) eps_s[e], e = b N + n, s = 0 .. nsamples - 1, ONE launch: the LRT-noise contract above
 * (eps4 / eps1 on the key, sample sample0 + s).  m, v: (rows, N) fp32; y: (nsamples, rows, N) fp32; all 16-byte aligned.
 * flags: 0.  Errors: BNN_E_NULL, BNN_E_SHAPE, BNN_E_RANGE (more than 65535 samples, rows N >= 2^32, bad rng),
 * BNN_E_UNSUPPORTED (flags), BNN_E_ALIGN. */
int bnn_moments_sample(const float *m, const float *v, float *y, int64_t rows, int64_t N, int nsamples, const bnn_rng_t *rng,
                       int flags, void *stream);

/* ---- K17: moment propagation through convolutions and ELU (csrc/bnn_conv3d.hip, csrc/bnn_moments_act.hpp; ops.moments_convNd,
 * ops.moments_elu).  K16's recursion for NormalConv / LocalReparamConv 1d / 2d / 3d, elements independent:
 *     m = convNd(a_m, mu_w) + mu_b
 *     v = convNd(a_m^2, sigma_w^2) + convNd(a_v, mu_w^2 + sigma_w^2) + sigma_b^2      (second term absent when a_v is NULL)
 * One implicit-GEMM tile on K7 / K11's forward skeleton (128 x 64 x 32, im2col in the loader's address arithmetic, padding reads
 * zero, groups in the grid; 1-d and 2-d layers: unit depth / height) with K16's planes: a_m^2 and fma(mu_w, mu_w, sigma_w^2) are
 * formed in fp32 as they are staged, both variance contractions add into one accumulator set, every addend of v is >= 0.
 * compute: BNN_COMPUTE_F32 = v_mfma_f32_16x16x4_f32; BNN_COMPUTE_BF16 = every plane rounded to bf16 (RNE) into LDS,
 * v_mfma_f32_16x16x32_bf16, fp32 accumulate.  No sample axis, no rng, no atomics, no split reduction: identical calls give
 * identical bits.  Graph-capturable; every error is returned before anything is launched.
 *
 * a_m: (B, C, D, H, W) fp32; a_v: the same shape or NULL (a deterministic input).  mu_w, s2_w: (O, C / groups, KD, KH, KW) fp32
 * (s2 = bnn_lrt_prepare's sigma^2); mu_b, s2_b: (O) fp32, both or neither.  out_m, out_v: (B, O, OD, OH, OW) fp32, 16-byte aligned.
 * flags: 0, BNN_FLAG_RELU (bnn_moments_relu's function in the epilogue) or BNN_FLAG_ELU (bnn_moments_elu's, with elu_alpha;
 * elu_alpha is not read otherwise).  shape->B == 0 returns BNN_OK after the checks.
 * Errors: BNN_E_NULL (a pointer, the shape, one bias tensor without the other), BNN_E_SHAPE (extents, groups not dividing the
 * channels), BNN_E_DTYPE (compute), BNN_E_RANGE (K7's index ranges: a tensor of 2^31 elements or more, so B O P < 2^32;
 * groups > 65535; elu_alpha negative or not finite), BNN_E_UNSUPPORTED (an unknown flag; RELU and ELU together), BNN_E_ALIGN
 * (4 bytes; 16 bytes for out_m and out_v). */
int bnn_conv3d_moments_forward(const float *a_m, const float *a_v, const float *mu_w, const float *s2_w, const float *mu_b,
                               const float *s2_b, float *out_m, float *out_v, const bnn_conv3d_shape_t *shape, int compute,
                               int flags, float elu_alpha, void *stream);
/* ELU (x > 0: x; else alpha (exp(x) - 1)) of a Gaussian N(m, v) by moment matching.  With s = sqrt(v), al = m / s, Phi / phi the
 * standard normal cdf / pdf, Phi_c = Phi(-al), E_k = exp(k m + k^2 v / 2) Phi(-al - k s), P1 = s (al Phi + phi),
 * N1 = E_1 - Phi_c, N2 = E_2 - 2 E_1 + Phi_c:
 *     mean' = P1 + alpha N1
 *     var'  = v (Phi + al^2 Phi Phi_c + al phi (Phi_c - Phi) - phi^2) + alpha^2 (N2 - N1^2) - 2 alpha P1 N1,   clamped at 0
 * (the ReLU's variance, the negative part's, and their cross term: m^2 is never subtracted from m^2 + v), evaluated in fp64 on
 * fp32 inputs and rounded to fp32 at the end.  v == 0 gives (elu(m), 0).  n elements, in place allowed.  The device function is
 * bnn_conv3d_moments_forward's epilogue's: same bits.  Errors: BNN_E_NULL, BNN_E_SHAPE (n < 0), BNN_E_RANGE (alpha negative or
 * not finite), BNN_E_ALIGN. */
int bnn_moments_elu(const float *m, const float *v, float *out_m, float *out_v, int64_t n, float alpha, void *stream);

/* ---- K18: training without sampling, the backward of K16's dense layer and of the moment-matched ReLU
 * (csrc/bnn_moments_bwd.hip; ops.moments_linear(track=True), BayesianNetworkModule.forward_moments).  With G_m, G_v the (B, N)
 * gradients with respect to m and v of bnn_moments_forward, for an input that carries a variance:
 *     g_a_m  = G_m mu_w + 2 a_m (.) (G_v sigma_w^2)          g_a_v  = G_v (mu_w^2 + sigma_w^2)           contraction over n
 *     g_mu_w = G_m^T a_m + 2 mu_w (.) (G_v^T a_v)            g_s2_w = G_v^T (a_m^2 + a_v)                over the rows, in row order
 *     g_rho_w = g_s2_w 2 sigma_w sigmoid(rho_w)              g_mu_b = sum_rows G_m,  g_rho_b = (sum_rows G_v) 2 sigma_b sigmoid(rho_b)
 * One 64 x 64 x 32 tile of K10's skeleton for both: P planes (p1, p2, fma(p1, p1, p2) -- formed in fp32 by the loader), Q planes
 * (G_m, G_v) with G_v serving twice, three accumulator sets, out1 = acc1 + 2 x (.) acc2 and out2 = acc3 in the epilogue.
 * compute: BNN_COMPUTE_F32 = v_mfma_f32_16x16x4_f32 (an ordered fp32 fma chain); BNN_COMPUTE_BF16 = the five planes rounded to
 * bf16 (RNE) as they are staged, fp32 accumulate.  No atomics, no split contraction: identical calls give identical bits.
 * A deterministic input (no a_v) has K10's backward: call bnn_lrt_backward_input / bnn_lrt_backward_weight with x = a_m.
 * Every operand and gradient is fp32; a_m, a_v have row pitch lda; flags: 0.  Graph-capturable; errors are returned before
 * anything is launched: BNN_E_NULL, BNN_E_SHAPE (extent < 1, lda < K), BNN_E_RANGE (rows > 64 * 65535; the weight gradient:
 * N > 64 * 65535), BNN_E_DTYPE (compute), BNN_E_UNSUPPORTED (any flag), BNN_E_ALIGN (element; 16 bytes for the contraction
 * outputs g_a_m, g_a_v, g_mu_w, g_rho_w).  B == 0: bnn_moments_backward_input returns BNN_OK at once, the weight gradients are
 * stored as zeros. */
int bnn_moments_backward_input(const float *g_m, const float *g_v, const float *mu_w, const float *s2_w, const float *a_m, int64_t lda,
                               float *g_a_m, float *g_a_v, int64_t B, int64_t N, int64_t K, int compute, int flags, void *stream);
/* Bias (rho_b, g_mu_b, g_rho_b all given, or all NULL): K10's second launch. */
int bnn_moments_backward_weight(const float *a_m, const float *a_v, int64_t lda, const float *g_m, const float *g_v, const float *mu_w,
                                const float *rho_w, float *g_mu_w, float *g_rho_w, const float *rho_b, float *g_mu_b, float *g_rho_b,
                                int64_t B, int64_t N, int64_t K, int compute, int flags, void *stream);
/* Backward of bnn_moments_relu at the pre-activation (m, v), on the forward's own Phi, phi and mean':
 *     g_m = g_out_m Phi + g_out_v 2 mean' Phi(-alpha)        g_v = g_out_m phi / (2 s) + g_out_v (Phi - mean' phi / s)
 * Where the forward clamped var' to 0 the g_out_v terms are absent; v == 0 (and |alpha| >= 40) gives g_m = g_out_m [m > 0],
 * g_v = g_out_v [m > 0].  n elements; g_m / g_v may be g_out_m / g_out_v. */
int bnn_moments_relu_backward(const float *m, const float *v, const float *g_out_m, const float *g_out_v, float *g_m, float *g_v,
                              int64_t n, void *stream);

/* ---- K19: training conv nets without sampling, the backward of K17's contraction and of the moment-matched ELU
 * (csrc/bnn_conv3d.hip, csrc/bnn_moments_bwd.hip; ops.moments_convNd(track=True), ops.moments_elu(track=True)).  With G_m, G_v the
 * (B, O, OD, OH, OW) gradients with respect to m and v of bnn_conv3d_moments_forward, convT the transposed contraction and the
 * sums over (image, position) in that order, for an input that carries a variance:
 *     g_a_m  = convT(G_m, mu_w) + 2 a_m (.) convT(G_v, sigma_w^2)        g_a_v  = convT(G_v, mu_w^2 + sigma_w^2)
 *     g_mu_w = sum gather(a_m) G_m + 2 mu_w (.) sum gather(a_v) G_v       g_s2_w = sum gather(a_m^2 + a_v) G_v
 *     g_rho_w = g_s2_w 2 sigma_w sigmoid(rho_w)              g_mu_b = sum G_m,  g_rho_b = (sum G_v) 2 sigma_b sigmoid(rho_b)
 * K18's planes and three accumulator sets on K11's backward tile (128 x 64 x 32, gather and transposed-weight address
 * arithmetic, groups in the grid, 1-d / 2-d layers as unit axes); the derived plane fma(p1, p1, p2) is formed in fp32 before any
 * rounding.  compute: BNN_COMPUTE_F32 = v_mfma_f32_16x16x4_f32; BNN_COMPUTE_BF16 = the planes rounded to bf16 (RNE) into LDS,
 * v_mfma_f32_16x16x32_bf16, fp32 accumulate.  The weight gradient splits (image, position) into slabs [slab][3][O][K] in the
 * workspace (bnn_conv3d_moments_wgrad_workspace bytes, the call's own) and a second launch adds them in slab order; the bias sums
 * are K11's launch.  No atomics, fixed order: identical calls give identical bits.  A deterministic input (no a_v) has K11's
 * backward: call bnn_conv3d_lrt_backward_input / bnn_conv3d_lrt_backward_weight with nsets = 1 and x = a_m.
 * Every operand and gradient is fp32 and dense: a_m, a_v, g_a_m, g_a_v (B, C, D, H, W); mu_w, s2_w, rho_w, g_mu_w, g_rho_w
 * (O, C / groups, KD, KH, KW); rho_b, g_mu_b, g_rho_b (O), all given or all NULL.  Graph-capturable; errors are returned before
 * anything is launched: BNN_E_NULL (a pointer, the shape, part of a bias; a NULL a_v / g_a_v names K11's entry), BNN_E_SHAPE,
 * BNN_E_DTYPE (compute), BNN_E_RANGE (bnn_conv3d_moments_forward's ranges; more than 64 * 65535 channels per group),
 * BNN_E_UNSUPPORTED (a workspace that is NULL or too small), BNN_E_ALIGN (element; 16 bytes for the contraction outputs g_a_m,
 * g_a_v, g_mu_w, g_rho_w).  shape->B == 0: bnn_conv3d_moments_backward_input returns BNN_OK after the checks, the weight and
 * bias gradients are stored as zeros. */
int bnn_conv3d_moments_backward_input(const float *g_m, const float *g_v, const float *mu_w, const float *s2_w, const float *a_m,
                                      float *g_a_m, float *g_a_v, const bnn_conv3d_shape_t *shape, int compute, void *stream);
/* Bytes of workspace bnn_conv3d_moments_backward_weight needs for this shape, or -1 for a shape it refuses. */
int64_t bnn_conv3d_moments_wgrad_workspace(const bnn_conv3d_shape_t *shape);
int bnn_conv3d_moments_backward_weight(const float *a_m, const float *a_v, const float *g_m, const float *g_v, const float *mu_w,
                                       const float *rho_w, float *g_mu_w, float *g_rho_w, const float *rho_b, float *g_mu_b,
                                       float *g_rho_b, const bnn_conv3d_shape_t *shape, int compute, void *workspace,
                                       int64_t workspace_bytes, void *stream);
/* Backward of bnn_moments_elu at the pre-activation (m, v), v > 0, in that entry's symbols (mean' its first result):
 *     d mean'/d m = Phi + alpha E_1                    d mean'/d v = (alpha E_1 + (1 - alpha) phi / s) / 2
 *     d var'/d m  = 2 P1 + 2 alpha^2 (E_2 - E_1) - 2 mean' (Phi + alpha E_1)
 *     d var'/d v  = Phi + alpha^2 (2 E_2 - E_1) - mean' (alpha E_1 + (1 - alpha) phi / s)
 * (g_m, g_v) = the two columns applied to (g_out_m, g_out_v); fp64 on fp32 inputs, rounded to fp32 at the end.  Where the forward
 * clamped var' to 0 the g_out_v terms are absent.  v == 0: g_m = g_out_m elu'(m), g_v = g_out_v elu'(m)^2 + g_out_m alpha exp(m)
 * [m < 0] / 2, with elu'(0) = 1.  n elements; g_m / g_v may be g_out_m / g_out_v.  Errors: BNN_E_NULL, BNN_E_SHAPE (n < 0),
 * BNN_E_RANGE (alpha negative or not finite), BNN_E_ALIGN. */
int bnn_moments_elu_backward(const float *m, const float *v, const float *g_out_m, const float *g_out_v, float *g_m, float *g_v,
                             int64_t n, float alpha, void *stream);

/* ---- K20: moments through pooling and eval-mode BatchNorm (csrc/bnn_moments_pool.hip, csrc/bnn_moments_act.hpp;
 * ops.moments_pool, ops.moments_batchnorm).  Elements are independent Gaussians.
 * Max pooling folds a window pairwise with the moment-matched maximum of two Gaussians (Clark 1961): with theta^2 = v1 + v2,
 * d = m1 - m2, alpha = d / theta, Phi = Phi at alpha, Phi_c = Phi at -alpha, phi the density at alpha,
 *     mean' = m1 Phi + m2 Phi_c + theta phi
 *     var'  = v1 Phi + v2 Phi_c + d^2 Phi Phi_c + d theta phi [Phi_c - Phi] - theta^2 phi^2,   clamped at 0
 * (the pair ((m, v), (0, 0)) is the function of bnn_moments_relu); exact for two elements, moment matching of the running
 * maximum beyond.  The fold order is part of the contract: window offsets ascending in depth, height, width (row-major); padded
 * positions are skipped and the first valid element starts the fold.  theta^2 == 0 is the plain maximum: the larger element's
 * mean and variance, the running value on a tie; the backward sends both gradients to that element.  fp64 on fp32 inputs, one
 * rounding to fp32 per output.  Average pooling: mean' = sum m / n, var' = sum v / n^2 over the valid positions, n the window
 * size, or the valid count with BNN_POOL_FLAG_VALID_DIVISOR.
 * Tensors are fp32 and dense: m, v, g_m, g_v [B, C, D, H, W]; out_m, out_v, g_out_m, g_out_v [B, C, OD, OH, OW] with the output
 * extents floor((I + 2 pad - dil (K - 1) - 1) / stride) + 1 per axis; 1-d and 2-d pooling are unit depth / height.  Every operand
 * may lie on its element (all loads and stores are one element wide).  A window holds at most 64 elements (the backward keeps
 * the fold's prefix states in LDS).  The backward folds the window again from m, v (nothing is kept from the forward call),
 * zeroes g_m and g_v on the stream with a launch of its own (skipped where the windows tile the input exactly), and writes windows that do not overlap (stride >= dil (K - 1) + 1 on every axis) with plain
 * stores: identical calls give identical bits.  Overlapping windows are accumulated with fp32 atomics, whose order is not fixed:
 * there a gradient may differ between identical calls by the rounding of an fp32 sum of at most prod ceil(extent / stride) terms.
 * Graph-capturable; errors are returned before anything is launched: BNN_E_NULL, BNN_E_SHAPE (an extent < 1, a negative padding,
 * an empty output), BNN_E_RANGE (padding above half the kernel; a window of more than 64 elements or one that lies in the padding
 * alone; 2^32 elements or more, an extent of 2^31 or more), BNN_E_UNSUPPORTED (an unknown op or flag), BNN_E_ALIGN. */
typedef struct {
    int64_t B, C, D, H, W;
    int64_t KD, KH, KW;
    int64_t stride_d, stride_h, stride_w;
    int64_t pad_d, pad_h, pad_w;
    int64_t dil_d, dil_h, dil_w;
} bnn_pool3d_shape_t;
enum { BNN_POOL_MAX = 0, BNN_POOL_AVG = 1 };
enum { BNN_POOL_FLAG_VALID_DIVISOR = 1 };     /* average pooling: divide by the number of valid positions (count_include_pad=False) */
int bnn_moments_pool3d_forward(const float *m, const float *v, float *out_m, float *out_v, const bnn_pool3d_shape_t *shape, int op,
                               int flags, void *stream);
int bnn_moments_pool3d_backward(const float *m, const float *v, const float *g_out_m, const float *g_out_v, float *g_m, float *g_v,
                                const bnn_pool3d_shape_t *shape, int op, int flags, void *stream);
/* Eval-mode BatchNorm as a per-channel affine map of the moments: a = gamma / sqrt[running_var + eps],
 * m' = a [m - running_mean] + beta, v' = a^2 v, a formed per element in the launch (fp32).  m, v, out_m, out_v: B x C x inner
 * elements, channel c = [e / inner] mod C; gamma, beta, running_mean, running_var: C; gamma / beta NULL mean 1 / 0.  In place
 * allowed.  Errors: BNN_E_NULL, BNN_E_SHAPE (an extent < 1), BNN_E_RANGE (2^32 elements or more; eps negative or not finite),
 * BNN_E_ALIGN. */
int bnn_moments_batchnorm(const float *m, const float *v, const float *gamma, const float *beta, const float *running_mean,
                          const float *running_var, float eps, float *out_m, float *out_v, int64_t B, int64_t C, int64_t inner,
                          void *stream);

/* ---- K21: the head of a sampling-free pass (csrc/bnn_moments_head.hip; ops.moments_mvn_linear, ops.moments_head_cov,
 * ops.moments_sample on moments that carry a covariance).  Inference only, fp32 in both compute modes, no atomics and no split
 * reductions: every sum is one ascending fp32 fma chain and identical calls give identical bits.  Graph-capturable; every error is
 * returned before anything is launched.  Every operand may lie on its element (all loads and stores are one element wide).
 *
 * MultivariateNormalLinear draws w_o = mu_o + L_o u with UNIFORM u ~ U[0, 1)^K and L = sqrt[tril[softplus[scale]] + 1e-10 I] taken
 * element by element (L is lower-triangular; the bits of L are bnn_mvn_draw's, one device function); its bias is one row of O
 * elements with an O x O factor L_b.  So per weight row o
 *     E_w[o,k] = mu[o,k] + 1/2 sum_{j<=k} L[o,k,j]      D[o,k] = 1/12 sum_{j<=k} L[o,k,j]^2      G_w = E_w^2 + D
 *     E_b      = mu_b + 1/2 L_b 1                        C_b    = L_b L_b^T / 12   [O x O]
 * and for an input with independent elements of mean a_m and variance a_v (a_v NULL: a deterministic input)
 *     m[b,o] = sum_k a_m[b,k] E_w[o,k] + E_b[o]
 *     v[b,o] = 1/12 sum_j [sum_{k>=j} a_m[b,k] L[o,k,j]]^2 + sum_k a_v[b,k] G_w[o,k] + C_b[o,o]
 * the exact mean and variance of the layer's output (no Gaussian assumption).
 *
 * bnn_mvn_moments_prepare: ONE launch, independent of the input.  mu_w [O, K], scale_w [O, K, K] (its upper triangles are never
 * read), mu_b [O], scale_b [O, O] -> E_w, G_w [O, K], E_b [O], C_b [O, O] (both triangles, from one computed value).  mu_b, scale_b,
 * E_b, C_b: all given or all NULL.  Row sums run in ascending j.  K <= 4096, O < 2^15 (with a bias O <= 4096), O K < 2^31.
 * bnn_mvn_moments_forward: ONE launch.  a_m, a_v [B, K] with row pitch lda; out_m, out_v [B, O].  L is formed from scale_w on the
 * fly; E_b, C_b both or neither.  K <= 4096, B <= 64 * 65535 (BNN_E_RANGE beyond). */
int bnn_mvn_moments_prepare(const float *mu_w, const float *scale_w, const float *mu_b, const float *scale_b, float *E_w, float *G_w,
                            float *E_b, float *C_b, int64_t O, int64_t K, void *stream);
int bnn_mvn_moments_forward(const float *a_m, const float *a_v, int64_t lda, const float *scale_w, const float *E_w, const float *G_w,
                            const float *E_b, const float *C_b, float *out_m, float *out_v, int64_t B, int64_t O, int64_t K,
                            void *stream);
/* The N x N covariance of a dense head's outputs per batch row, for inputs with independent elements of variance a_v:
 *     cov[b,o,p] = sum_k [E[o,k] E[p,k]] a_v[b,k] + C_b[o,p]   (o != p)        cov[b,o,o] = var[b,o]
 * E [N, K] the weights' means (an MVN head: E_w; a Gaussian head: mu_w; a deterministic one: w), C_b [N, N] the bias covariance or
 * NULL (no bias term), var [B, N] the head's output variance, cov [B, N, N].  Both triangles are written from one computed value and
 * the diagonal is var's bits.  a_v NULL (a deterministic input): the off-diagonal is C_b's (E may be NULL).  N <= 32, B < 2^31. */
int bnn_moments_head_cov(const float *a_v, int64_t lda, const float *E, const float *C_b, const float *var, float *cov, int64_t B,
                         int64_t N, int64_t K, void *stream);
/* y_s[b,:] = m[b,:] + Lc_b eps_s[b,:], s = 0 .. nsamples - 1, ONE launch: Lc_b the lower Cholesky factor of cov[b] (its lower
 * triangle is read), computed in fp64 from the fp32 cov; a pivot <= 0 gives a zero column (a direction without variance: a
 * semi-definite covariance, or one made so by rounding).  The product is accumulated in fp64 and m + Lc eps is rounded once to fp32.
 * eps_s[b,n] is element e = b N + n of the key's sample sample0 + s (the LRT-noise contract above): bnn_moments_sample's values on
 * the same key.  m [rows, N], cov [rows, N, N], y [nsamples, rows, N].  N <= 32, rows N < 2^32, nsamples <= 65535; flags is 0. */
int bnn_moments_sample_cov(const float *m, const float *cov, float *y, int64_t rows, int64_t N, int nsamples, const bnn_rng_t *rng,
                           int flags, void *stream);

/* ---- K22: MC dropout in a sampling-free pass, folded through the activation behind it (csrc/bnn_moments_dropout.hip,
 * csrc/bnn_moments_act.hpp; ops.moments_dropout).  An MC-dropout layer hands on y = f(b z / q): z ~ N(m, v) its pre-dropout output,
 * b ~ Bernoulli(q) an independent mask, q = 1 - p, f the activation behind it with f(0) = 0 (act: 0 = identity, BNN_FLAG_RELU,
 * BNN_FLAG_ELU with alpha; alpha is not read otherwise).  Since f(b z / q) = b f(z / q), with (M, V) the moments of f at the Gaussian
 * N(m / q, v / q^2) -- bnn_moments_relu's / bnn_moments_elu's functions there, the identity's are the input --
 *     mean' = q M        var' = q V + q p M^2
 * exact for a Gaussian z and for a deterministic one (v == 0; a NaN v takes the same limit branches): a dropped unit is a spike at
 * zero, not a Gaussian, and the activation is applied to the spike.  Identity and ReLU in fp32; the ELU scales its input and
 * recombines its results in fp64 around bnn_moments_elu's fp64 evaluation.  p == 0 gives the activation's own bits, p == 1 gives
 * (0, 0) and divides nothing by q.  v NULL: a deterministic input, every variance zero (out_v is still written: q p f(m / q)^2).
 * n elements, one element per load and store (every operand may lie on its element), in place allowed (out_m == m, out_v == v).
 * No scratch, no atomics: identical calls give identical bits.  Graph-capturable; errors are returned before anything is launched:
 * BNN_E_NULL, BNN_E_RANGE (n < 0; p outside [0, 1] or NaN; an unknown act; alpha negative or not finite with BNN_FLAG_ELU),
 * BNN_E_ALIGN. */
int bnn_moments_dropout(const float *m, const float *v, float *out_m, float *out_v, int64_t n, float p, int act, float alpha,
                        void *stream);
/* Backward of bnn_moments_dropout at the pre-dropout (m, v): with M as above (evaluated again),
 *     gM = q g_out_m + 2 q p M g_out_v        gV = q g_out_v
 * go through the activation's backward at (m / q, v / q^2) (bnn_moments_relu_backward's / bnn_moments_elu_backward's functions,
 * their clamp and v == 0 conventions; the identity passes them) to (g_mi, g_vi), and g_m = g_mi / q, g_v = g_vi / q^2.  p == 0: the
 * activation's backward, its bits; p == 1: zeros.  v NULL: a deterministic input, and g_v may then be NULL (it is written when
 * given).  g_m / g_v may be g_out_m / g_out_v.  Errors: as bnn_moments_dropout. */
int bnn_moments_dropout_backward(const float *m, const float *v, const float *g_out_m, const float *g_out_v, float *g_m, float *g_v,
                                 int64_t n, float p, int act, float alpha, void *stream);

/* ---- K23: sparse variational dropout (VariationalDropoutLinear, bayesianneuralnetworks_amd/nn/dense.py; csrc/bnn_vd.hip;
 * Molchanov, Ashukha, Vetrov 2017, "Variational Dropout Sparsifies Deep Neural Networks").  No call site in the reference.  Every
 * weight has the posterior N(theta, sigma^2), parametrised by theta and log_sigma2 = ln sigma^2, and a log-uniform prior:
 *     s2 = exp(log_sigma2)        log_alpha = clamp(log_sigma2 - ln(theta^2), -8, 8)        (theta = 0: +8)
 *     KL_e = k1 sigmoid(-(k2 + k3 log_alpha)) + 0.5 log1p(exp(-log_alpha)),   k1 = 0.63576, k2 = 1.87320, k3 = 1.48695
 *     dKL_e / dlog_alpha = -k1 k3 s (1 - s) - 0.5 sigmoid(-log_alpha),  s = sigmoid(k2 + k3 log_alpha)
 *     dlog_alpha / dlog_sigma2 = 1,  dlog_alpha / dtheta = -2 / theta inside the clamp; both exactly 0 where it is active
 * The layer itself is K10's on the variance plane s2: bnn_lrt_forward (the LRT-noise contract), bnn_lrt_backward_epilogue,
 * bnn_lrt_backward_input and bnn_moments_forward take (theta, s2) for (mu_w, s2_w) unchanged; the optional Gaussian bias
 * (mu_b, rho_b) is K10's.  log_alpha, KL_e and its derivative are evaluated in fp64 on the device and rounded to fp32 once.
 *
 * bnn_vd_prepare: s2_out[i] = exp(log_sigma2[i]) for i < n_w, and s2_b = sigma(rho_b)^2 as bnn_lrt_prepare writes it (n_b may
 * be 0), one launch.  A threshold below +inf (the pruning mask of an inference pass): elements with log_alpha > threshold get
 * theta_out = 0 and s2_out = 0, every other one theta_out = theta, and *count_out (8-byte aligned) receives the number of masked
 * elements -- an integer sum, zeroed in-stream by the entry, the same for every grid.  threshold = +inf: nothing is masked,
 * theta_out (a copy when given) and count_out may be NULL, and theta may be NULL with theta_out.  Element alignment throughout.
 * Errors: BNN_E_NULL, BNN_E_SHAPE (n_w < 1, n_b < 0), BNN_E_RANGE (a NaN threshold), BNN_E_ALIGN. */
int bnn_vd_prepare(const float *theta, const float *log_sigma2, int64_t n_w, const float *rho_b, float *s2_b, int64_t n_b,
                   float threshold, float *theta_out, float *s2_out, int64_t *count_out, void *stream);
/* bnn_lrt_backward_weight for this posterior: g_theta = g_m^T x and g(s2) = g_v^T x^2 on the same paired tile (both compute modes,
 * BNN_FLAG_X_BF16 = x is bf16; the contraction runs over all M rows in row order), then g_log_sigma2 = g(s2) exp(log_sigma2) in
 * the epilogue.  Bias (rho_b, g_mu_b, g_rho_b all given, or all NULL): bnn_lrt_backward_weight's second launch.  Errors as there. */
int bnn_vd_backward_weight(const void *x, int64_t ldx, const float *g_m, const float *g_v, const float *log_sigma2, float *g_theta,
                           float *g_log_sigma2, const float *rho_b, float *g_mu_b, float *g_rho_b, int64_t M, int64_t N, int64_t K,
                           int compute, int flags, void *stream);
/* One posterior tensor of the log-uniform KL (host struct). */
typedef struct bnn_vd_tensor {
    const float *theta;
    const float *log_sigma2;
    int64_t n;
} bnn_vd_tensor_t;
/* out[t] = sum_e KL_e of tensor t, t < ntensors <= 128: a launch per 64 tensors that leaves one double per 2048-element workgroup
 * in `workspace` (bnn_vd_kl_workspace_bytes(tensors, ntensors) bytes, 8-byte aligned; -1 for a bad list), then one workgroup
 * that adds each tensor's partials in a fixed order.  No float atomics: identical calls give identical bits.  16-byte loads
 * where both operands of a tensor lie on 16 bytes, element loads otherwise; any n >= 1.
 * Errors: BNN_E_NULL, BNN_E_SHAPE (ntensors < 1, n < 1), BNN_E_UNSUPPORTED (more than 128 tensors), BNN_E_RANGE, BNN_E_ALIGN. */
int64_t bnn_vd_kl_workspace_bytes(const bnn_vd_tensor_t *tensors, int ntensors);
int bnn_vd_kl_forward(const bnn_vd_tensor_t *tensors, int ntensors, float *out, void *workspace, void *stream);
/* g_theta[t][e] (+)= upstream[t] / n_t * dKL_e / dtheta, g_log_sigma2[t][e] likewise: upstream a device array of ntensors floats
 * (the gradient of each tensor's MEAN KL), g_theta / g_log_sigma2 host arrays of ntensors device pointers; accumulate != 0 adds. */
int bnn_vd_kl_backward(const bnn_vd_tensor_t *tensors, int ntensors, const float *upstream, float *const *g_theta,
                       float *const *g_log_sigma2, int accumulate, void *stream);

/* ---- K24: sparse variational dropout for convolutions (VariationalDropoutConv1d / 2d / 3d, bayesianneuralnetworks_amd/nn/conv.py;
 * csrc/bnn_conv3d.hip).  No call site in the reference.  K23's posterior N(theta, exp(log_sigma2)) on K11's layer: the weight is
 * (O, C / groups, KD, KH, KW), bnn_vd_prepare writes its planes (a flat tensor of any shape), and bnn_conv3d_lrt_forward (the
 * LRT-conv noise contract, as written), bnn_lrt_backward_epilogue, bnn_conv3d_lrt_backward_input and bnn_conv3d_moments_forward
 * take (theta, s2) for (mu_w, s2_w) unchanged; the optional Gaussian bias (mu_b, rho_b) is K11's; the KL is K23's.
 *
 * bnn_conv3d_lrt_backward_weight for this posterior.  The slab launch is K11's own (the same kernel, grid and workspace:
 * bnn_conv3d_lrt_backward_weight_workspace_bytes), so the slabs hold the same bits; the reduce launch adds them in slab order
 * and writes g_theta = sum of the mean slabs -- bit for bit K11's g_mu_w on the same x, g_m, g_v -- and
 * g_log_sigma2 = (sum of the variance slabs) expf(log_sigma2), d exp(l) / dl = exp(l): within 3 u + 2 u^2 of the product in exact
 * arithmetic, and below log_sigma2 = -87, where expf returns a denormal, the fp64 product rounded once (one quantum, 2^-149, of
 * a denormal result; u of a normal one).  Bias (rho_b, g_mu_b, g_rho_b all given,
 * or all NULL): K11's third launch.  Two launches without a bias, three with one.  Fixed orders, no atomics: identical calls
 * give identical bits.  Errors (nothing launched) as bnn_conv3d_lrt_backward_weight: BNN_E_NULL, BNN_E_SHAPE, BNN_E_DTYPE (an
 * unknown compute), BNN_E_RANGE (K7's ranges), BNN_E_ALIGN (4 bytes), BNN_E_UNSUPPORTED (workspace NULL or too small). */
int bnn_conv3d_vd_backward_weight(const float *x, const float *g_m, const float *g_v, const float *log_sigma2, float *g_theta,
                                  float *g_log_sigma2, const float *rho_b, float *g_mu_b, float *g_rho_b,
                                  const bnn_conv3d_shape_t *shape, int nsets, int compute, void *workspace,
                                  int64_t workspace_bytes, void *stream);

/* ---- K25: the Bayesian LSTM cell, one time step per launch (nn.NormalLSTM, bayesianneuralnetworks_amd/nn/recurrent.py;
 * csrc/bnn_lstm.hip).  No call site in the reference: it has no recurrent layer (Fortunato et al. 2017, "Bayesian Recurrent
 * Neural Networks").  One weight draw per MC sample serves every step of that sample; the draw is K1's
 * (bnn_sample_affine_philox on a (4 H, I + H) tensor) and neither entry reads rho.  For sample s, row r, hidden unit j:
 *     G[q]  = gx[s][r][q H + j] + sum_k h_prev[s][r][k] w_h[s][q H + j][k]        q = 0 .. 3: the gates i, f, g, o (torch's order)
 *     c     = sigmoid(G[1]) c_prev + sigmoid(G[0]) tanh(G[2]),     h = sigmoid(G[3]) tanh(c)
 * gx is the input projection x_t W_x^T + b of the step, computed for all steps beforehand (bnn_linear_forward).
 * Every (S, rows, .) operand with a pitch argument has row r of sample s at base + (s * rows + r) * pitch: a step is read from
 * and written into a (S, rows, T, .) buffer in place with base + t * width and pitch T * width.  w_h: (4 H, H) row-major per
 * sample, sample s at w_h + s * w_sample_stride.  Operands without a pitch are contiguous (S, rows, H).
 * Numerics: fp32 operands and fp32 accumulation (v_mfma_f32_16x16x4_f32), whatever the compute mode of the caller.  The
 * accumulation order of an output element depends on H alone -- not on nsamples, rows or the grid -- and there are no atomics:
 * identical calls give identical bits, and sample s of a batched call has the bits of a one-sample call on that sample's
 * operands.  With u = 2^-24 the device sigmoid has relative error <= 4 u and tanh absolute error <= 5 u (csrc/bnn_lstm.hip);
 * neither overflows for |G| <= 88.
 * Alignment: every pointer on its element (BNN_E_ALIGN otherwise).  16-byte loads of h_prev and w_h (forward), of the pointwise
 * operands and stores of dg and g_c_prev (backward), when H % 4 == 0 and those pointers and pitches are multiples of 16 bytes;
 * element accesses otherwise -- the same bits.
 * Errors (nothing launched): BNN_E_NULL; BNN_E_SHAPE: rows, H or nsamples < 1, a pitch below its row length (4 H for gx, gates
 * and dg, H for the states), w_sample_stride < 4 H H; BNN_E_RANGE: rows >= 2^31, H > 16 * 65535, nsamples > 65535, a pitch
 * >= 2^31 or nsamples * rows * pitch (nsamples * w_sample_stride) > 2^62; BNN_E_ALIGN.
 *
 * bnn_lstm_step_forward: writes h and c, and -- gates != NULL, when a backward will follow -- the four gate ACTIVATIONS
 * sigmoid(G[0]), sigmoid(G[1]), tanh(G[2]), sigmoid(G[3]) at gates[s][r][q H + j].  h_prev = c_prev = NULL (together): zeros, the
 * first step.  No output may overlap an input.  One launch: a workgroup (one wave) owns 16 rows x 16 units of a sample. */
int bnn_lstm_step_forward(const float *gx, int64_t ldgx, const float *w_h, int64_t w_sample_stride,
                          const float *h_prev, int64_t ldh_prev, const float *c_prev, int64_t ldc_prev,
                          float *h, int64_t ldh, float *c, int64_t ldc, float *gates, int64_t ldgates,
                          int64_t rows, int64_t H, int nsamples, void *stream);
/* bnn_lstm_step_backward: the backward of that step.  With gh = g_h_out + g_h_in (the gradient reaching h_t from the layer's
 * output at step t and from step t + 1; either may be NULL = zeros, g_h_in and g_c_in together), the saved activations i, f, g, o
 * of gates, and tc = tanh(c):
 *     dc       = g_c_in + gh o (1 - tc^2)
 *     dg[0..3] = dc g i (1 - i),  dc c_prev f (1 - f),  dc i (1 - g^2),  gh tc o (1 - o)           at dg[s][r][q H + j]
 *     g_c_prev = dc f,      g_h_prev[s][r][k] = sum_n dg[s][r][n] w_h[s][n][k]                      n over all 4 H gate rows
 * c_prev = NULL: zeros (the first step).  g_h_in, g_c_in, g_h_prev, g_c_prev: contiguous (S, rows, H); no output may overlap an
 * input (carry the two gradients in two buffers each).  One launch: a workgroup owns 16 rows x 16 output units, forms dg for
 * its rows itself (pointwise), and the workgroup of unit block 0 stores dg and g_c_prev. */
int bnn_lstm_step_backward(const float *gates, int64_t ldgates, const float *c_prev, int64_t ldc_prev,
                           const float *c, int64_t ldc, const float *g_h_out, int64_t ldg_h_out,
                           const float *g_h_in, const float *g_c_in, const float *w_h, int64_t w_sample_stride,
                           float *dg, int64_t lddg, float *g_h_prev, float *g_c_prev,
                           int64_t rows, int64_t H, int nsamples, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BNN_HIP_H */
