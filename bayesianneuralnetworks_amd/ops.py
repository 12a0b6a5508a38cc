"""Tensor-level front-end of the C-ABI (include/bnn_hip.h) with autograd.

Forward passes are hand-written HIP (libbnn_hip.so).  Backward: the eps-dependent
elementwise parts are HIP too (bnn_sample_affine_bwd, bnn_kl_backward; eps is regenerated
from the draw key, never stored); the two plain GEMMs of a linear/conv backward go through
torch.bmm / torch's conv backward on the GPU (library GEMMs on already-drawn weights).

Every function here requires CUDA (HIP) tensors and raises BnnHipError otherwise.
"""
import collections
import contextlib
import ctypes
import functools
import itertools
import math
import os
import threading

import torch

from . import _lib
from ._lib import (BnnHipError, Rng, KlTensor, Conv2dShape, ptr, stream_ptr, check, require_cuda_f32,
                   require_cuda_act)
from ._rng import default_generator, DrawKey


def _rng_struct(key, device):
    r = Rng()
    r.seed = key.seed
    r.stream = key.stream
    r.sample0 = key.sample0
    r.epoch_host = key.epoch_host
    r.epoch_dev_delta = key.epoch_dev_delta
    r.epoch_dev = default_generator.epoch_dev(device).data_ptr()
    r.generator = key.gen
    return r


def _compute_code(compute):
    if compute in ("f32", "fp32", _lib.COMPUTE_F32):
        return _lib.COMPUTE_F32
    if compute in ("bf16", _lib.COMPUTE_BF16):
        return _lib.COMPUTE_BF16
    raise ValueError("compute must be 'f32' or 'bf16', got %r" % (compute,))


# --------------------------------------------------------------------------- K1
def sigma(rho):
    """1e-10 + softplus(rho)  (WeightNormal.stddev, core.py:25-27) -- no autograd."""
    rho = rho.detach()
    require_cuda_f32(rho, "rho")
    out = torch.empty_like(rho)
    check(_lib.load().bnn_sigma(ptr(rho), ptr(out), rho.numel(), stream_ptr(rho.device)), "bnn_sigma")
    return out


def eps_philox(shape, key, device):
    """The raw eps stream for `key` -> (nsamples, *shape) fp32."""
    n = 1
    for d in shape:
        n *= d
    out = torch.empty((key.nsamples,) + tuple(shape), dtype=torch.float32, device=device)
    r = _rng_struct(key, out.device)
    check(_lib.load().bnn_eps_philox(ptr(out), n, key.nsamples, n, ctypes.byref(r), stream_ptr(out.device)),
          "bnn_eps_philox")
    return out


def _sample_affine_philox_raw(mu, rho, key, out_dtype=torch.float32):
    require_cuda_f32(mu, "mu")
    require_cuda_f32(rho, "rho")
    n = mu.numel()
    out = torch.empty((key.nsamples,) + tuple(mu.shape), dtype=out_dtype, device=mu.device)
    r = _rng_struct(key, mu.device)
    code = _lib.F32 if out_dtype == torch.float32 else _lib.BF16
    check(_lib.load().bnn_sample_affine_philox(ptr(mu), ptr(rho), ptr(out), n, key.nsamples, n, code,
                                                ctypes.byref(r), stream_ptr(mu.device)),
          "bnn_sample_affine_philox")
    return out


def _sample_affine_bwd_raw(g_w, rho, n, nsamples, eps=None, key=None):
    g_w = g_w.contiguous()
    g_mu = torch.empty_like(rho)
    g_rho = torch.empty_like(rho)
    r = _rng_struct(key, rho.device) if key is not None else None
    check(_lib.load().bnn_sample_affine_bwd(ptr(g_w), n, ptr(rho), ptr(eps), n,
                                             ctypes.byref(r) if r is not None else None,
                                             n, nsamples, ptr(g_mu), ptr(g_rho), 0, stream_ptr(rho.device)),
          "bnn_sample_affine_bwd")
    return g_mu, g_rho


class _SampleAffineEps(torch.autograd.Function):
    """w = mu + sigma(rho) * eps with eps supplied (parity mode)."""

    @staticmethod
    def forward(ctx, mu, rho, eps):
        require_cuda_f32(mu, "mu")
        require_cuda_f32(rho, "rho")
        require_cuda_f32(eps, "eps")
        out = torch.empty_like(mu)
        check(_lib.load().bnn_sample_affine_eps(ptr(mu), ptr(rho), ptr(eps), ptr(out), mu.numel(), _lib.F32,
                                                 stream_ptr(mu.device)), "bnn_sample_affine_eps")
        ctx.save_for_backward(rho, eps)
        return out

    @staticmethod
    def backward(ctx, g):
        rho, eps = ctx.saved_tensors
        g_mu, g_rho = _sample_affine_bwd_raw(g, rho, rho.numel(), 1, eps=eps)
        return g_mu, g_rho, None


class _SampleAffinePhilox(torch.autograd.Function):
    """(S, *shape) draws of w = mu + sigma(rho) * eps(key)."""

    @staticmethod
    def forward(ctx, mu, rho, key):
        out = _sample_affine_philox_raw(mu.detach(), rho.detach(), key)
        ctx.save_for_backward(rho)
        ctx.key = key
        return out

    @staticmethod
    def backward(ctx, g):
        (rho,) = ctx.saved_tensors
        g_mu, g_rho = _sample_affine_bwd_raw(g, rho, rho.numel(), ctx.key.nsamples, key=ctx.key)
        return g_mu, g_rho, None


def sample_affine_eps(mu, rho, eps):
    return _SampleAffineEps.apply(mu.contiguous(), rho.contiguous(), eps.contiguous())


def sample_affine_philox(mu, rho, key):
    return _SampleAffinePhilox.apply(mu.contiguous(), rho.contiguous(), key)


# --------------------------------------------------------------------------- draw-once path (bf16 compute mode)
def _pad64(k):
    return (k + 63) // 64 * 64


def dense_eligible(mu_w):
    """The draw-once path takes a (N, K) posterior whose rows are whole 8-column groups and 16-B aligned."""
    return mu_w.dim() == 2 and mu_w.shape[1] % 8 == 0 and mu_w.data_ptr() % 16 == 0


class Predrawn:
    """The drawn weights of one layer for one forward: w (S, N, Kp) bf16 zero-padded to Kp = roundup(K, 64) -- or, drawn
    for the fp32 parity mode, (3, S, N, Kp): the three bf16 planes of the fp32 draw -- b (S, N) fp32 or None, and the
    DrawKeys they were drawn with."""
    __slots__ = ("w", "b", "key_w", "key_b")

    def __init__(self, w, b, key_w, key_b):
        self.w, self.b, self.key_w, self.key_b = w, b, key_w, key_b


def _draw_slot(t, mu, rho, rows, cols, out, ld, sample_stride, dtype, kind=_lib.DRAW_SAMPLE, taps=0, key=None):
    """Fills one bnn_draw_tensor_t (include/bnn_hip.h): the (rows, cols) source tensors mu / rho (rho None: a kind that reads mu
    alone), `out` the address of draw 0 -- rows of ld elements of `dtype`, the draws sample_stride elements apart -- the kind
    (_lib.DRAW_*), taps = KH * KW of a conv weight written tap-major, and the DrawKey of a kind that draws."""
    t.mu, t.rho, t.rows, t.cols = mu.data_ptr(), (mu if rho is None else rho).data_ptr(), rows, cols
    t.out, t.ld, t.out_sample_stride, t.out_dtype = out, ld, sample_stride, dtype
    t.kind, t.taps = kind, taps
    if key is not None:
        t.rng = _rng_struct(key, mu.device)


def _draw_launch(arr, n, nsamples, device):
    """ONE bnn_draw_multi launch of the first n slots of arr (no KL riding along)."""
    check(_lib.load().bnn_draw_multi(arr, n, nsamples, None, 0, None, stream_ptr(device)), "bnn_draw_multi")


def draw_layers(layers, nsamples, kl=None, x3=False, split=None):
    """ONE launch (bnn_draw_multi) draws the weights and biases of every (mu_w, rho_w, mu_b, rho_b, key_w, key_b) in
    `layers` for `nsamples` MC samples -> list of Predrawn.  kl (a KlDeferred from kl_normal_begin(carry=True)): the
    launch also carries that KL's first pass.  At most 4 layers (8 tensors) per launch; more are split.
    x3: weights as three bf16 planes of the fp32 draw (BNN_BF16X3; the fp32 parity mode's dense path).
    split (x3 only): an fp32 (M, K) activation whose three-plane split (what split_x3 returns) rides in the FIRST launch as one more
    tensor (kind BNN_DRAW_COPY) instead of a launch of its own; the planes come back as `_tls.last_split`."""
    _tls.last_split = None
    out = []
    lib = _lib.load()
    dev = layers[0][0].device
    step = 4 if split is None else 3                # (8 tensors per launch: the split takes one)
    for i0 in range(0, len(layers), step):
        group = layers[i0:i0 + step]
        arr = (_lib.DrawTensor * (2 * len(group) + 1))()
        n = 0
        keep = []
        if split is not None and i0 == 0 and x3:
            require_cuda_f32(split, "x")
            Ms, Ks = split.shape
            lds_ = _pad64(Ks)
            planes = torch.empty((3, 1, Ms, lds_), dtype=torch.bfloat16, device=dev)
            _draw_slot(arr[n], split, None, Ms, Ks, planes.data_ptr(), lds_, Ms * lds_, _lib.BF16X3, _lib.DRAW_COPY)
            n += 1
            _tls.last_split = planes
            keep.append(split)
        for spec in group:
            mu_w, rho_w, mu_b, rho_b, key_w, key_b = spec[:6]
            taps = spec[6] if len(spec) > 6 else 0      # KH * KW: a conv weight, written tap-major
            kind = spec[7] if len(spec) > 7 else _lib.DRAW_SAMPLE      # _lib.DRAW_FLIPOUT: a Flipout draw (eps = the key's sign outer product)
            require_cuda_f32(mu_w, "weight.mean")
            require_cuda_f32(rho_w, "weight.scale")
            N, K = mu_w.shape
            kp = _pad64(K)
            w = torch.empty(((3, nsamples, N, kp) if x3 else (nsamples, N, kp)), dtype=torch.bfloat16, device=dev)
            _draw_slot(arr[n], mu_w, rho_w, N, K, w.data_ptr(), kp, N * kp, _lib.BF16X3 if x3 else _lib.BF16, kind, taps, key_w)
            n += 1
            b = None
            if mu_b is not None:
                require_cuda_f32(mu_b, "bias.mean")
                require_cuda_f32(rho_b, "bias.scale")
                b = torch.empty((nsamples, N), dtype=torch.float32, device=dev)
                _draw_slot(arr[n], mu_b, rho_b, 1, N, b.data_ptr(), N, N, _lib.F32, key=key_b)
                n += 1
            keep.append((mu_w, rho_w, mu_b, rho_b))
            out.append(Predrawn(w, b, key_w, key_b))
        carried = False
        if kl is not None and not kl.launched and i0 == 0 and kl.out.device == dev:
            rc = lib.bnn_draw_multi(arr, n, nsamples, kl.arr, kl.T, ptr(kl.ws), stream_ptr(dev))
            if rc == 0:
                kl.launched = carried = True
            elif rc != _lib.E_UNSUPPORTED:
                check(rc, "bnn_draw_multi")
        if not carried:
            _draw_launch(arr, n, nsamples, dev)
    return out


def rows_pitch(t, K):
    """A (M, K) or (S, M, K) bf16 activation whose rows the dense kernel can read in place -- unit element stride, one row
    pitch (>= K, whole 16-B chunks), samples a whole number of 16-B chunks apart, e.g. the 128-B-aligned rows _dense_raw
    itself writes -> (row pitch, sample stride) in elements, the values to LAUNCH with; None if the view is not of that kind.
    The strides are read off the view, never re-derived from M and K: with one row per sample the row stride of the view says
    nothing (torch may report anything for a size-1 dimension) and the samples of a padded (S, 1, K) view sit stride(0)
    apart, not K."""
    if t.dtype != torch.bfloat16 or t.dim() not in (2, 3) or t.shape[-1] != K or t.stride(-1) != 1 or t.data_ptr() % 16 != 0:
        return None
    M = t.shape[-2]
    ld = t.stride(-2) if M > 1 else K               # a single row: its pitch is never used to step to another row
    if ld < K or ld % 8 != 0:
        return None
    if t.dim() == 2 or t.shape[0] == 1:
        return ld, M * ld
    xs = t.stride(0)
    if xs % 8 != 0 or xs < (M - 1) * ld + K:        # samples overlap, or are not 16-B aligned
        return None
    return ld, xs


def rows_regular(t, K):
    return rows_pitch(t, K) is not None


def _dense_raw(x2, x_sample_stride, M, pre, K, relu, out_dtype, ldx=None, pad_rows=False):
    """y (S, M, N) = act(x . w_s^T + b_s) on Predrawn weights (bnn_dense_forward); x bf16 with row pitch ldx.
    pad_rows (bf16 hidden activations): the rows of y are written 128 B apart-aligned (pitch roundup(N, 64)) and y is
    returned as a view of that buffer -- the next layer's LDS-DMA then reads whole cache lines (layer 2 of the BASELINE
    net: 19.6 -> 17.0 us)."""
    S, N, kp = pre.w.shape
    ldx = K if ldx is None else ldx
    ldy = _pad64(N) if (pad_rows and out_dtype == torch.bfloat16) else N
    ybuf = torch.empty((S, M, ldy), dtype=out_dtype, device=x2.device)
    flags = (_lib.FLAG_RELU if relu else 0) | (_lib.FLAG_Y_BF16 if out_dtype == torch.bfloat16 else 0)
    check(_lib.load().bnn_dense_forward(ptr(x2), x_sample_stride, ldx, ptr(pre.w), N * kp, kp,
                                         ptr(pre.b), N if pre.b is not None else 0, ptr(ybuf), M * ldy, ldy, M, N, K, S, flags,
                                         stream_ptr(x2.device)), "bnn_dense_forward")
    return ybuf if ldy == N else ybuf[:, :, :N]


class HeadPartials:
    """What a hidden layer fused with the classifier head behind it leaves (bnn_dense_forward_head): PARTIAL logits
    (parts, S, M, Nh) fp32 -- the head's contraction cut along the hidden units, partial 0 carrying the head's bias.  Not a
    tensor: the head layer passes it through, `BayesianNetworkModule.predictive_mean` / `ops.mc_mean` reduce it over
    (part, sample) in the step's ONE tail launch, `.logits()` over `part` for callers that want every sample."""
    __slots__ = ("p", "head")

    def __init__(self, p, head=None):
        self.p, self.head = p, head

    @property
    def shape(self):
        return torch.Size((self.p.shape[1] * self.p.shape[2], self.p.shape[3]))

    @property
    def is_cuda(self):
        return True

    @property
    def device(self):
        return self.p.device

    def dim(self):
        return 2

    def logits(self):
        """(S, M, Nh): the sum over the partials (one bnn_mc_sum launch)."""
        parts, S, M, Nh = self.p.shape
        out = torch.empty((S, M, Nh), dtype=torch.float32, device=self.p.device)
        n = S * M * Nh
        check(_lib.load().bnn_mc_sum(ptr(self.p), n, parts, n, 1.0, ptr(out), 0, None, 0, stream_ptr(self.p.device)), "bnn_mc_sum")
        return out


def dense_head_eligible(M, N, pre, pre_head):
    """Hidden layer (drawn weights `pre`, N > 16 outputs) + head (`pre_head`, <= 16 outputs) in one launch?"""
    return (pre is not None and pre_head is not None and pre.w.dim() == 3 and pre_head.w.dim() == 3 and N > 16 and N % 8 == 0 and
            pre_head.w.shape[1] <= 16 and pre_head.w.shape[2] >= N and pre.w.shape[0] == pre_head.w.shape[0] and M > 0)


def _dense_head_raw(x2, x_sample_stride, M, pre, K, relu, pre_head, ldx=None):
    """bnn_dense_forward_head: act(x . w_s^T + b_s) rounded to bf16 and contracted with the head's drawn weights in the same
    launch -> HeadPartials (the hidden activation is never stored)."""
    S, N, kp = pre.w.shape
    _, Nh, kph = pre_head.w.shape
    lib = _lib.load()
    parts = lib.bnn_dense_head_parts(M, N, S)
    P = torch.empty((parts, S, M, Nh), dtype=torch.float32, device=x2.device)
    ldx = K if ldx is None else ldx
    check(lib.bnn_dense_forward_head(ptr(x2), x_sample_stride, ldx, ptr(pre.w), N * kp, kp, ptr(pre.b), N if pre.b is not None else 0,
                                     ptr(pre_head.w), Nh * kph, kph, ptr(pre_head.b), Nh if pre_head.b is not None else 0, Nh,
                                     ptr(P), M, N, K, S, _lib.FLAG_RELU if relu else 0, stream_ptr(x2.device)), "bnn_dense_forward_head")
    return HeadPartials(P)


def dense_head_x3_eligible(M, N, pre, pre_head):
    """The same pair in the fp32 parity mode (three-plane operands): the 160-column tiles only (N % 80 == 0 or N < 128, N > 80)."""
    return (pre is not None and pre_head is not None and pre.w.dim() == 4 and pre_head.w.dim() == 4 and N > 80 and N % 8 == 0 and
            (N % 80 == 0 or N < 128) and pre_head.w.shape[2] <= 16 and pre_head.w.shape[3] >= N and pre.w.shape[1] == pre_head.w.shape[1] and M > 0)


def _dense_head_raw_x3(xp, shared, M, pre, K, relu, pre_head):
    """bnn_dense_forward_x3_head: xp (3, S or 1, M, ldx) planes, pre.w (3, S, N, kp), pre_head.w (3, S, Nh, kph) -> HeadPartials."""
    _, S, N, kp = pre.w.shape
    _, _, Nh, kph = pre_head.w.shape
    ldx = xp.shape[3]
    lib = _lib.load()
    parts = lib.bnn_dense_head_parts(M, N, S)
    P = torch.empty((parts, S, M, Nh), dtype=torch.float32, device=xp.device)
    check(lib.bnn_dense_forward_x3_head(ptr(xp), xp.shape[1] * M * ldx, 0 if shared else M * ldx, ldx,
                                        ptr(pre.w), S * N * kp, N * kp, kp, ptr(pre.b), N if pre.b is not None else 0,
                                        ptr(pre_head.w), S * Nh * kph, Nh * kph, kph, ptr(pre_head.b), Nh if pre_head.b is not None else 0, Nh,
                                        ptr(P), M, N, K, S, _lib.FLAG_RELU if relu else 0, stream_ptr(xp.device)), "bnn_dense_forward_x3_head")
    return HeadPartials(P)


class X3Activation:
    """A hidden activation of the fp32 parity mode as it travels between two dense layers: the fp32 values as three bf16
    planes (3, S, M, ld) (h, m, l: v = h + m + l to 2^-24 |v|), `cols` valid columns.  Not a tensor: only NormalLinear
    consumes it (nn.fuse_activations arranges that); .float() gives the fp32 tensor back."""
    __slots__ = ("planes", "cols")

    def __init__(self, planes, cols):
        self.planes, self.cols = planes, cols

    @property
    def shape(self):
        return torch.Size((self.planes.shape[1] * self.planes.shape[2], self.cols))

    @property
    def is_cuda(self):
        return self.planes.is_cuda

    @property
    def device(self):
        return self.planes.device

    def dim(self):
        return 2

    def float(self):
        p = self.planes[..., :self.cols].float()
        return (p[0] + p[1] + p[2]).reshape(-1, self.cols)


def split_x3(x2):
    """fp32 (M, K) -> (3, 1, M, roundup(K, 64)) bf16 planes (bnn_split_bf16x3)."""
    require_cuda_f32(x2, "x")
    M, K = x2.shape
    ld = _pad64(K)
    out = torch.empty((3, 1, M, ld), dtype=torch.bfloat16, device=x2.device)
    check(_lib.load().bnn_split_bf16x3(ptr(x2), M, K, x2.stride(0) if M > 1 else K, ptr(out), ld, M * ld, stream_ptr(x2.device)),
          "bnn_split_bf16x3")
    return out


def x3_eligible(x2, mu_w, M):
    """fp32 parity mode on the dense kernels: whole 8-column groups, a batch worth the draw-once path, an fp32 (M, K) input
    or an X3Activation; a narrow layer (N <= 16: the K-split head kernel) up to K = 2048."""
    N, K = mu_w.shape
    if not (dense_eligible(mu_w) and M >= 64 and (N > 16 or K <= 2048)):
        return False
    if isinstance(x2, X3Activation):
        return True
    return x2.dtype == torch.float32 and x2.dim() == 2 and x2.stride(-1) == 1 and x2.stride(0) % 4 == 0 and x2.data_ptr() % 16 == 0


def _dense_raw_x3(xp, shared, M, pre, K, relu, planes_out):
    """y = act(x . w_s^T + b_s) in the fp32 parity mode on three-plane operands (bnn_dense_forward_x3).
    xp: (3, S or 1, M, ldx) planes; pre.w (3, S, N, kp).  planes_out: the result as an X3Activation (for the next dense
    layer) instead of an fp32 (S, M, N) tensor."""
    _, S, N, kp = pre.w.shape
    ldx = xp.shape[3]
    xs = 0 if shared else M * ldx
    if planes_out:
        ldy = _pad64(N)
        y = torch.empty((3, S, M, ldy), dtype=torch.bfloat16, device=xp.device)
        yps = S * M * ldy
    else:
        ldy = N
        y = torch.empty((S, M, N), dtype=torch.float32, device=xp.device)
        yps = 0
    flags = (_lib.FLAG_RELU if relu else 0) | (_lib.FLAG_Y_BF16 if planes_out else 0)
    check(_lib.load().bnn_dense_forward_x3(ptr(xp), xp.shape[1] * M * ldx, xs, ldx, ptr(pre.w), S * N * kp, N * kp, kp,
                                            ptr(pre.b), N if pre.b is not None else 0, ptr(y), yps, M * ldy, ldy, M, N, K, S, flags,
                                            stream_ptr(xp.device)), "bnn_dense_forward_x3")
    return X3Activation(y, N) if planes_out else y


def linear_sampled_x3(x2, shared, M, mu_w, rho_w, mu_b, rho_b, key_w, key_b, relu=False, planes_out=False, predrawn=None, head_pre=None):
    """Inference call of NormalLinear in the fp32 parity mode (no autograd: the caller checked that no gradient is wanted):
    draw once as three bf16 planes (or `predrawn` by the network's draw plan), contract on the dense kernel.
    head_pre (the drawn planes of the classifier head behind this layer): the pair as ONE launch -> HeadPartials."""
    S = key_w.nsamples
    N, K = mu_w.shape
    pre = predrawn
    if pre is None:
        pre = draw_layers([(mu_w, rho_w, mu_b, rho_b, key_w, key_b)], S, kl=_tls.kl_carry, x3=True)[0]
        if _tls.kl_carry is not None and _tls.kl_carry.launched:
            _tls.kl_carry = None
    if isinstance(x2, X3Activation):
        xp = x2.planes
        if xp.shape[1] not in (1, S) or xp.shape[2] != M or x2.cols != K:
            raise BnnHipError("linear: three-plane activation of shape %s does not fit (S = %d, M = %d, K = %d)" % (tuple(xp.shape), S, M, K))
        shared = xp.shape[1] == 1
    else:
        xp = split_x3(x2.reshape(-1, K))            # (3, 1, rows, ld); rows = M (shared) or S * M
        if not shared:
            xp = xp.view(3, S, M, xp.shape[3])
    if head_pre is not None:
        return _dense_head_raw_x3(xp, shared, M, pre, K, relu, head_pre)
    return _dense_raw_x3(xp, shared, M, pre, K, relu, planes_out)


# --------------------------------------------------------------------------- K2 linear
def _linear_sampled_raw(x2, x_sample_stride, M, mu_w, rho_w, mu_b, rho_b, key_w, key_b, compute, relu=False,
                        out_dtype=torch.float32, predrawn=None, pad_rows=False):
    N, K = mu_w.shape
    S = key_w.nsamples
    _lib.ensure_workspace(x2.device)
    if compute == _lib.COMPUTE_BF16 and DRAW_ONCE_BF16 and dense_eligible(mu_w) and M > 0:
        # bf16 compute mode: the layer's weights are drawn ONCE for the S samples (K1, one launch -- or already drawn
        # for this forward by the network's draw plan, `predrawn`) and contracted by the dense MFMA GEMM (csrc/bnn_dense.hip).
        # Same DrawKeys -> the same weights as the fused kernel, bit for bit; the backward re-creates them as always.
        pre = predrawn
        if pre is None:
            pre = draw_layers([(mu_w, rho_w, mu_b, rho_b, key_w, key_b)], S, kl=_tls.kl_carry)[0]
            if _tls.kl_carry is not None and _tls.kl_carry.launched:
                _tls.kl_carry = None
        pitch = rows_pitch(x2, K) if x2.dtype == torch.bfloat16 else None
        if pitch is not None:
            ldx, xs = pitch
            return _dense_raw(x2, 0 if x_sample_stride == 0 else xs, M, pre, K, relu, out_dtype, ldx=ldx, pad_rows=pad_rows)
        xb = x2.contiguous().to(torch.bfloat16)        # (the fused kernel rounds its A operand the same way)
        if not _aligned16(xb):                         # (already bf16 and contiguous, at an odd offset: nothing above copied it)
            xb = xb.clone()
        return _dense_raw(xb, x_sample_stride, M, pre, K, relu, out_dtype, pad_rows=pad_rows)
    x2 = x2.contiguous()
    y = torch.empty((S, M, N), dtype=out_dtype, device=x2.device)
    rw = _rng_struct(key_w, x2.device)
    rb = _rng_struct(key_b, x2.device) if mu_b is not None else None
    flags = (_lib.FLAG_RELU if relu else 0) | (_lib.FLAG_X_BF16 if x2.dtype == torch.bfloat16 else 0) | \
            (_lib.FLAG_Y_BF16 if out_dtype == torch.bfloat16 else 0)
    if flags & (_lib.FLAG_X_BF16 | _lib.FLAG_Y_BF16) and not _aligned16(x2, mu_w, rho_w):
        # bf16 activations exist only on the kernels' 16-B path, which refuses an operand at an odd offset (a view into a flat
        # parameter buffer, a row slice): such an operand is copied -- the draw is addressed by position, so the bits are the same
        x2, mu_w, rho_w = (t if _aligned16(t) else t.clone() for t in (x2, mu_w, rho_w))
    if (M >= DRAW_ONCE_MIN_ROWS and N > 16 and K % 8 == 0 and mu_w.data_ptr() % 16 == 0 and rho_w.data_ptr() % 16 == 0):
        # Large batch: the fused kernel's 256- / 512-row tiles would re-draw every weight M / 256 (M / 512) times, and at
        # that size the draw is what the launch is made of -- so the weights of the S samples are drawn ONCE by K1 (same
        # DrawKey -> the same values, bit for bit) and the same kernel runs on explicit weights (configs[4] layer, 4096 x
        # 4096 at batch 4096: fp32 mode 111 -> 144 TFLOP/s, bf16 mode 310 -> 369).  S * N * K * 4 bytes of scratch; the
        # backward re-creates the draws from the keys as always.
        w = _sample_affine_philox_raw(mu_w.reshape(-1), rho_w.reshape(-1), key_w)
        b = _sample_affine_philox_raw(mu_b, rho_b, key_b) if mu_b is not None else None
        check(_lib.load().bnn_linear_forward(ptr(x2), x_sample_stride, K, ptr(w), N * K, ptr(b), N, ptr(y), M * N, N, M, N, K, S,
                                              compute, flags, stream_ptr(x2.device)), "bnn_linear_forward")
        return y
    h = _tls.kl_carry
    if h is not None and N <= 16 and not h.launched and h.out.device == x2.device:
        # a narrow layer: its launch carries the first pass of the KL begun with kl_normal_begin(carry=True)
        check(_lib.load().bnn_linear_forward_sampled_kl(
            ptr(x2), x_sample_stride, K, ptr(mu_w), ptr(rho_w), ptr(mu_b), ptr(rho_b),
            ptr(y), M * N, N, M, N, K, S, ctypes.byref(rw), ctypes.byref(rb) if rb is not None else None,
            compute, flags, h.arr, h.T, ptr(h.ws), stream_ptr(x2.device)), "bnn_linear_forward_sampled_kl")
        h.launched = True
        _tls.kl_carry = None
        return y
    check(_lib.load().bnn_linear_forward_sampled(
        ptr(x2), x_sample_stride, K, ptr(mu_w), ptr(rho_w), ptr(mu_b), ptr(rho_b),
        ptr(y), M * N, N, M, N, K, S, ctypes.byref(rw), ctypes.byref(rb) if rb is not None else None,
        compute, flags, stream_ptr(x2.device)), "bnn_linear_forward_sampled")
    return y


class _ThreadState(threading.local):
    """Per-thread hand-over state of the forward (two threads driving two models must not see each other's):
    kl_carry   -- a KlDeferred whose first pass waits for a narrow layer's launch to carry it (kl_normal_begin(carry=True));
    last_split -- draw_layers(split=...): the three planes of the activation that rode in the last launch.
    kl_pending is NOT per thread: a backward pass runs a device's nodes on the autograd engine's thread for that device, not on
    the thread that called backward(), so one dict serves every thread (what a caller reads after backward() is what the pass
    used) and every entry names its pass instead (see _KlPending)."""

    kl_pending = {}     # KL gradients parked for the layers' weight-gradient launches (FUSE_KL_GRADIENT), keyed by the mean's storage

    def __init__(self):
        self.kl_carry = None
        self.last_split = None


_tls = _ThreadState()
# from this many rows per sample on, a sampled linear layer draws its weights once (K1) instead of in the GEMM
DRAW_ONCE_MIN_ROWS = 2048
# bf16 compute mode: draw once + dense GEMM at every batch size (False: the round-1 fused kernel, kept for A/B runs)
DRAW_ONCE_BF16 = True
DENSE_X3_F32 = os.environ.get("BNN_DENSE_X3", "1") != "0"    # fp32 parity mode of wide inference layers on the dense kernel


def _bf(t):
    return t.dtype == torch.bfloat16


def _aligned16(*ts):
    """Every tensor starts on a 16-byte boundary (what the kernels' 16-B loads and the LDS-DMA ask of an operand)."""
    return all(t.data_ptr() % 16 == 0 for t in ts)


# --- KL gradient fused into the weight-gradient launch ------------------------------------------------
# KLDivergence's backward does not compute its gradient when the parameter's layer can do it for free: it
# PARKS (upstream, scale, prior) per posterior tensor here, keyed by the mean's storage; the sampled linear /
# conv backward of that layer -- which runs later in the same backward pass -- picks the entry up and the
# weight-gradient kernel adds the closed-form KL gradient in its final store (no bnn_kl_backward pass, no
# autograd accumulation add per parameter).  Entries nobody picked up (parity-mode layers, unused layers, a
# KL node that happened to run after the layers) are flushed at the end of the pass by an engine callback.
# Every entry carries the id of its backward pass (autograd's graph task): the engine runs no queued callback of
# a pass that raised, so such a pass leaves its entries behind -- a later pass does not take them (_kl_take), does
# not flush them (_kl_flush) and overwrites them when its own KL node parks for the same tensor.
# OPT-IN (nn.fuse_kl_gradient(True)): parking returns no gradient from the KL node itself, which is only right when
# the pass accumulates into .grad (loss.backward()); torch.autograd.grad(kl, params) needs the default path.
FUSE_KL_GRADIENT = False


class _KlPending:
    __slots__ = ("up", "scale", "prior", "mu", "rho", "task")

    def __init__(self, up, scale, prior, mu, rho, task):
        self.up, self.scale, self.prior, self.mu, self.rho, self.task = up, scale, prior, mu, rho, task


def _kl_take(mu):
    """The entry parked for `mu` by the KL node of the backward pass that is running, or None."""
    pend = _tls.kl_pending
    if not pend:
        return None
    key = (mu.device.index, mu.data_ptr())
    e = pend.get(key)
    if e is None or e.task != torch._C._current_graph_task_id():
        return None
    del pend[key]
    return e


def _kl_fuse_struct(ent_w, ent_b):
    """bnn_kl_fuse_t for a layer whose weight entry (and optionally bias entry) were parked by the same KL node."""
    k = _lib.KlFuse()
    k.upstream = ent_w.up.data_ptr()
    k.mu_w = ent_w.mu.data_ptr()
    k.scale_w, k.prior_mu_w, k.prior_sigma_w = ent_w.scale, ent_w.prior[0], ent_w.prior[1]
    if ent_b is not None:
        k.mu_b = ent_b.mu.data_ptr()
        k.scale_b, k.prior_mu_b, k.prior_sigma_b = ent_b.scale, ent_b.prior[0], ent_b.prior[1]
    else:
        k.mu_b, k.scale_b, k.prior_mu_b, k.prior_sigma_b = None, 0.0, 0.0, 1.0
    return k


def _kl_flush(task):
    """Engine callback at the end of backward pass `task`: KL gradients of the tensors no layer picked up."""
    pend = _tls.kl_pending
    ents = [(k, e) for k, e in list(pend.items()) if e.task == task]
    if not ents:
        return
    for k, _ in ents:
        del pend[k]
    ents = [e for _, e in ents]
    lib = _lib.load()
    for e in ents:
        g_mu, g_rho = torch.empty_like(e.mu), torch.empty_like(e.rho)
        arr = _kl_descs([e.mu], [e.rho], [e.prior])
        gm = (ctypes.c_void_p * 1)(g_mu.data_ptr())
        gr = (ctypes.c_void_p * 1)(g_rho.data_ptr())
        # scale = 1 / (n * T * n_batches): hand bnn_kl_backward an n_batches that reproduces it for one tensor
        check(lib.bnn_kl_backward(arr, 1, 1.0 / (e.scale * e.mu.numel()), ptr(e.up), gm, gr, 0, stream_ptr(e.mu.device)),
              "bnn_kl_backward")
        for p_, g_ in ((e.mu, g_mu), (e.rho, g_rho)):
            if p_.grad is None:
                p_.grad = g_
            else:
                p_.grad.add_(g_)


def _relu_backward_raw(g, y):
    """g * (y > 0) (the fused ReLU epilogue's backward)."""
    out = torch.empty_like(g)
    flags = (_lib.FLAG_X_BF16 if _bf(g) else 0) | (_lib.FLAG_Y_BF16 if _bf(y) else 0)
    check(_lib.load().bnn_relu_backward(ptr(g), ptr(y), ptr(out), g.numel(), flags, stream_ptr(g.device)),
          "bnn_relu_backward")
    return out


def _colsum_raw(gy):
    """(S, M, N) -> (S, N) fp32 column sums (the bias gradient of F.linear)."""
    S, M, N = gy.shape
    out = torch.empty((S, N), dtype=torch.float32, device=gy.device)
    check(_lib.load().bnn_colsum(ptr(gy), M * N, N, ptr(out), M, N, S, _lib.FLAG_X_BF16 if _bf(gy) else 0,
                                 stream_ptr(gy.device)), "bnn_colsum")
    return out


def _dgrad_plain_raw(gy, w, x_dtype):
    """gx[s] = gy[s] @ w[s] with explicit fp32 weights (S, N, K)."""
    S, M, N = gy.shape
    K = w.shape[2]
    gx = torch.empty((S, M, K), dtype=x_dtype, device=gy.device)
    flags = (_lib.FLAG_X_BF16 if _bf(gy) else 0) | (_lib.FLAG_Y_BF16 if x_dtype == torch.bfloat16 else 0)
    check(_lib.load().bnn_linear_backward_input(ptr(gy), M * N, N, ptr(w), N * K, ptr(gx), M * K, K, M, N, K, S,
                                                flags, stream_ptr(gy.device)), "bnn_linear_backward_input")
    return gx


DGRAD_ON_DRAWN = True      # bf16 mode: the input gradient contracts on the weights the forward drew (A/B switch)


def _transpose_drawn_raw(w, K):
    """Drawn weights (S, N, ldw) bf16 -> (S, K, roundup(N, 64)) with zeros beyond column N (bnn_transpose_bf16)."""
    S, N, ldw = w.shape
    ldn = _pad64(N)
    out = torch.empty((S, K, ldn), dtype=torch.bfloat16, device=w.device)
    check(_lib.load().bnn_transpose_bf16(ptr(w), N * ldw, ldw, ptr(out), K * ldn, ldn, N, K, S, stream_ptr(w.device)),
          "bnn_transpose_bf16")
    return out


def _dgrad_drawn_raw(gy, w, K):
    """gx[s] = gy[s] @ w_s on the weights the forward drew (bf16 (S, N, ldw)): transpose once, then the dense kernel
    (contraction over n) -- the backward on the draw-once path, no second draw.  gy (S, M, N) bf16 -> gx (S, M, K) bf16."""
    S, M, N = gy.shape
    if gy.data_ptr() % 16 != 0:                      # (a contiguous view at an odd offset: the LDS-DMA wants 16-B aligned rows)
        gy = gy.clone()
    wt = _transpose_drawn_raw(w, K)
    gx = torch.empty((S, M, K), dtype=torch.bfloat16, device=gy.device)
    check(_lib.load().bnn_dense_forward(ptr(gy), M * N, N, ptr(wt), K * wt.shape[2], wt.shape[2], None, 0, ptr(gx), M * K, K,
                                         M, K, N, S, _lib.FLAG_Y_BF16, stream_ptr(gy.device)), "bnn_dense_forward")
    return gx


def _sum_samples(t):
    """(S, ...) fp32 -> sum over S (bnn_mc_sum, scale 1)."""
    out = torch.empty(t.shape[1:], dtype=torch.float32, device=t.device)
    n = out.numel()
    check(_lib.load().bnn_mc_sum(ptr(t), n, t.shape[0], n, 1.0, ptr(out), 0, None, 0, stream_ptr(t.device)),
          "bnn_mc_sum")
    return out


def _wgrad_sampled_raw(x, x_sample_stride, gy, mu_w, rho_w, mu_b, rho_b, rw, key_b, M, N, K, S, need_b, compute, flags, *,
                       kl_weight, kl_bias, narrow_gx=None):
    """The sampled layer's weight-gradient launch (bnn_linear_backward_weight_sampled: x (., M, K), gy (S, M, N)) with the bias
    gradient (need_b) and the KL gradient KLDivergence's backward parked for this layer riding along -> (g_mu_w, g_rho_w,
    g_mu_b, g_rho_b).  What differs between its three callers is spelled out by them:
      kl_weight  take the weight's parked KL entry (the general linear site: M > 0 -- an empty batch zero-fills, the flush adds KL);
      kl_bias    ... and with it the bias's (False at the conv site: a conv bias entry is left to the flush);
      narrow_gx  (gx,), gx (S, M, K) or None: the narrow layer's one-pass kernel (bnn_linear_backward_narrow_sampled), which
                 writes the input gradient too.  Where it does not apply (workspace, alignment) the KL entries go back to
                 _tls.kl_pending and the answer is None: the caller falls through to the general kernels."""
    dev = gy.device
    g_mu_w, g_rho_w = torch.empty_like(mu_w), torch.empty_like(rho_w)
    g_mu_b = g_rho_b = rb = None
    if need_b:                                                         # bias gradient rides in the same launch
        g_mu_b, g_rho_b = torch.empty_like(rho_b), torch.empty_like(rho_b)
        rb = _rng_struct(key_b, dev)
    ent_w = _kl_take(mu_w) if kl_weight else None
    ent_b = _kl_take(mu_b) if (kl_bias and ent_w is not None and need_b and mu_b is not None) else None
    kl = _kl_fuse_struct(ent_w, ent_b) if ent_w is not None else None
    grads = (ptr(g_mu_w), ptr(g_rho_w), ptr(rho_b) if need_b else None, ptr(g_mu_b), ptr(g_rho_b), M, N, K, S, ctypes.byref(rw),
             ctypes.byref(rb) if rb is not None else None, ctypes.byref(kl) if kl is not None else None)
    lib = _lib.load()
    if narrow_gx is None:
        check(lib.bnn_linear_backward_weight_sampled(ptr(x), x_sample_stride, K, ptr(gy), M * N, N, ptr(rho_w), *grads,
                                                     compute, flags, 0, stream_ptr(dev)), "bnn_linear_backward_weight_sampled")
        return g_mu_w, g_rho_w, g_mu_b, g_rho_b
    rc = lib.bnn_linear_backward_narrow_sampled(ptr(x), x_sample_stride, K, ptr(gy), M * N, N, ptr(mu_w), ptr(rho_w),
                                                ptr(narrow_gx[0]), M * K, K, *grads, flags, 0, stream_ptr(dev))
    if rc == 0:
        return g_mu_w, g_rho_w, g_mu_b, g_rho_b
    if rc not in (_lib.E_UNSUPPORTED, _lib.E_ALIGN):
        check(rc, "bnn_linear_backward_narrow_sampled")
    for e in (ent_w, ent_b):
        if e is not None:
            _tls.kl_pending[(e.mu.device.index, e.mu.data_ptr())] = e
    return None


def _wgrad_plain_raw(x, x_sample_stride, gy, M, N, K, S, compute=_lib.COMPUTE_F32):
    """gw[s] = gy[s]^T x[s] for explicit weights (bnn_linear_backward_weight): x (., M, K), gy (S, M, N) fp32 -> (S, N, K) fp32."""
    gw = torch.empty((S, N, K), dtype=torch.float32, device=gy.device)
    check(_lib.load().bnn_linear_backward_weight(ptr(x), x_sample_stride, K, ptr(gy), M * N, N, ptr(gw), N * K, M, N, K, S,
                                                 compute, 0, 0, stream_ptr(gy.device)), "bnn_linear_backward_weight")
    return gw


class _SampledLinear(torch.autograd.Function):
    """y[s] = x[s] @ w_s^T + b_s, w_s / b_s drawn in-kernel (NormalLinear.forward, dense.py:56-60).
    Backward (what autograd derives in the reference, train.py:63-65) is HIP as well: the input
    gradient re-draws w_s inside the contraction, the weight gradient folds the draw's backward
    into its epilogue (csrc/bnn_linear_bwd.hip)."""

    @staticmethod
    def forward(ctx, x, mu_w, rho_w, mu_b, rho_b, key_w, key_b, shared_x, compute, relu, out_dtype, predrawn=None, track=True):
        # x: (M, K) shared by all samples, or (S, M, K), fp32 or (bf16 compute mode) bf16;
        # relu: max(., 0) fused in the epilogue; out_dtype: fp32, or bf16 for a hidden activation
        # x may be a row-padded view (rows_regular) on the inference path; whatever the backward saves is contiguous
        # track: grad mode at the call (inside forward it is always off, and needs_input_grad only mirrors requires_grad)
        needs_grad = track and any(ctx.needs_input_grad[:5])
        if needs_grad or not (x.dtype == torch.bfloat16 and rows_regular(x, x.shape[-1])):
            x = x.contiguous()
        require_cuda_act(x, "x", contiguous=False)
        if (x.dtype == torch.bfloat16 or out_dtype == torch.bfloat16) and compute != _lib.COMPUTE_BF16:
            raise BnnHipError("bf16 activations need compute mode 'bf16'")
        for t, n in ((mu_w, "weight.mean"), (rho_w, "weight.scale")):
            require_cuda_f32(t, n)
        if mu_b is not None:
            require_cuda_f32(mu_b, "bias.mean")
            require_cuda_f32(rho_b, "bias.scale")
        M = x.shape[-2]
        K = x.shape[-1]
        if K != mu_w.shape[1]:
            raise BnnHipError("linear: input has %d features, weight expects %d" % (K, mu_w.shape[1]))
        ctx.drawn_w = None
        if (track and ctx.needs_input_grad[0] and not shared_x and compute == _lib.COMPUTE_BF16 and DRAW_ONCE_BF16 and DGRAD_ON_DRAWN
                and dense_eligible(mu_w) and M > 0 and x.dtype == torch.bfloat16 and mu_w.shape[0] > 16 and mu_w.shape[0] % 8 == 0):
            # training, bf16 mode: the input gradient will contract on THESE drawn weights (kept alive by the graph node)
            if predrawn is None:
                predrawn = draw_layers([(mu_w, rho_w, mu_b, rho_b, key_w, key_b)], key_w.nsamples, kl=_tls.kl_carry)[0]
                if _tls.kl_carry is not None and _tls.kl_carry.launched:
                    _tls.kl_carry = None
            if predrawn.w.dim() == 3:
                ctx.drawn_w = predrawn.w
        y = _linear_sampled_raw(x, 0 if shared_x else M * K, M, mu_w, rho_w, mu_b, rho_b, key_w, key_b,
                                compute, relu, out_dtype, predrawn, pad_rows=not needs_grad)
        ctx.save_for_backward(x, mu_w, rho_w, rho_b if mu_b is not None else None, y if relu else None, mu_b)
        ctx.key_w, ctx.key_b, ctx.shared_x, ctx.compute = key_w, key_b, shared_x, compute
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mu_w, rho_w, rho_b, y_relu, mu_b = ctx.saved_tensors
        S, compute = ctx.key_w.nsamples, ctx.compute
        N, K = mu_w.shape
        M = x.shape[-2]
        dev = gy.device
        lib = _lib.load()
        _lib.ensure_workspace(dev)
        gy = gy.contiguous()
        if compute != _lib.COMPUTE_BF16 and gy.dtype != torch.float32:
            gy = gy.float()
        if y_relu is not None:
            gy = _relu_backward_raw(gy, y_relu)                            # fused ReLU
        gflag = _lib.FLAG_X_BF16 if _bf(gy) else 0
        rw = _rng_struct(ctx.key_w, dev)
        gx = g_mu_w = g_rho_w = g_mu_b = g_rho_b = None
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if N <= 16 and K % 4 == 0 and M > 0 and need_w and not _bf(gy) and not (ctx.shared_x and ctx.needs_input_grad[0]):
            # narrow layer (classifier head): the whole backward in one pass over the activations
            need_b = rho_b is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
            if ctx.needs_input_grad[0]:
                gx = torch.empty((S, M, K), dtype=x.dtype, device=dev)
            flags = (_lib.FLAG_X_BF16 if _bf(x) else 0) | (_lib.FLAG_Y_BF16 if (gx is not None and _bf(gx)) else 0)
            grads = _wgrad_sampled_raw(x, 0 if ctx.shared_x else M * K, gy, mu_w, rho_w, mu_b, rho_b, rw, ctx.key_b, M, N, K, S, need_b,
                                       compute, flags, kl_weight=True, kl_bias=True, narrow_gx=(gx,))
            if grads is not None:
                return (gx,) + grads + (None,) * 8
            gx = None               # not applicable here (workspace, alignment): the general kernels below
        if ctx.needs_input_grad[0]:
            # a shared input sums its gradient over the samples: fp32 partials, then one reduction
            gx_dtype = torch.float32 if ctx.shared_x else x.dtype
            # (bnn_linear_backward_input_sampled reads mu_w, rho_w and gy in 16-B pieces and refuses them elsewhere: a posterior that
            # is a view into a flat buffer, a gy that is a slice of a larger gradient -> the explicit-weight kernel below)
            fused = K % 4 == 0 and N % (8 if _bf(gy) else 4) == 0 and \
                (compute == _lib.COMPUTE_BF16 or (not _bf(gy) and gx_dtype == torch.float32)) and _aligned16(mu_w, rho_w, gy)
            if ctx.drawn_w is not None and _bf(gy) and gx_dtype == torch.bfloat16:
                gx = _dgrad_drawn_raw(gy, ctx.drawn_w, K)
            elif fused:
                gx = torch.empty((S, M, K), dtype=gx_dtype, device=dev)
                flags = gflag | (_lib.FLAG_Y_BF16 if gx_dtype == torch.bfloat16 else 0)
                check(lib.bnn_linear_backward_input_sampled(ptr(gy), M * N, N, ptr(mu_w), ptr(rho_w), ptr(gx),
                                                            M * K, K, M, N, K, S, ctypes.byref(rw), compute, flags,
                                                            stream_ptr(dev)), "bnn_linear_backward_input_sampled")
            else:
                w = _sample_affine_philox_raw(mu_w, rho_w, ctx.key_w)      # (S, N, K) fp32, the forward's draw
                gx = _dgrad_plain_raw(gy, w, gx_dtype)
            if ctx.shared_x:
                gx = _sum_samples(gx).to(x.dtype)
        need_b = rho_b is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            flags = (_lib.FLAG_X_BF16 if _bf(x) else 0) | (_lib.FLAG_Y_BF16 if _bf(gy) else 0)
            g_mu_w, g_rho_w, g_mu_b, g_rho_b = _wgrad_sampled_raw(
                x, 0 if ctx.shared_x else M * K, gy, mu_w, rho_w, mu_b, rho_b, rw, ctx.key_b, M, N, K, S, need_b, compute, flags,
                kl_weight=M > 0, kl_bias=True)
        elif need_b:
            gb = _colsum_raw(gy)                                           # (S, N)
            g_mu_b, g_rho_b = _sample_affine_bwd_raw(gb, rho_b, rho_b.numel(), S, key=ctx.key_b)
        return gx, g_mu_w, g_rho_w, g_mu_b, g_rho_b, None, None, None, None, None, None, None, None


def linear_sampled(x, mu_w, rho_w, mu_b, rho_b, key_w, key_b, shared_x, compute="f32", relu=False,
                   out_dtype=torch.float32, predrawn=None):
    return _SampledLinear.apply(x, mu_w.contiguous(), rho_w.contiguous(),
                                None if mu_b is None else mu_b.contiguous(),
                                None if rho_b is None else rho_b.contiguous(),
                                key_w, key_b, shared_x, _compute_code(compute), bool(relu), out_dtype, predrawn,
                                torch.is_grad_enabled())


# --------------------------------------------------------------------------- K10: local reparameterization
def lrt_eligible(x, mu_w, rows, nsamples):
    """None when bnn_lrt_forward takes the call, else the reason it refuses (index range, alignment, layout).  x: (rows, K) for a
    shared input or (S, rows, K); there is no torch fallback on device tensors -- linear_lrt raises with this reason."""
    N, K = mu_w.shape
    if x.shape[-1] != K:
        return "input has %d features, weight expects %d" % (x.shape[-1], K)
    if nsamples < 1 or nsamples > 0xFFFF:
        return "%d MC samples (1 .. 65535)" % nsamples
    if rows * N >= 2 ** 32:
        return "one sample has %d x %d output elements: the noise index b N + n is 32 bits wide" % (rows, N)
    if rows > 64 * 65535 or nsamples * rows > 64 * 65535:
        return "%d rows (at most %d)" % (nsamples * rows, 64 * 65535)
    if x.dtype not in (torch.float32, torch.bfloat16):
        return "input dtype %s (float32 or bfloat16)" % x.dtype
    if x.data_ptr() % x.element_size():
        return "input pointer is not aligned to its element size"
    return None


def _lrt_prepare_raw(rho_w, rho_b):
    """sigma^2 of weight and bias, fp32, one launch (bnn_lrt_prepare)."""
    s2_w = torch.empty_like(rho_w)
    s2_b = torch.empty_like(rho_b) if rho_b is not None else None
    check(_lib.load().bnn_lrt_prepare(ptr(rho_w), ptr(s2_w), rho_w.numel(), ptr(rho_b), ptr(s2_b),
                                      rho_b.numel() if rho_b is not None else 0, stream_ptr(rho_w.device)), "bnn_lrt_prepare")
    return s2_w, s2_b


def _lrt_check_posterior(mu_w, rho_w, mu_b, rho_b, conv=False):
    """The four posterior tensors of a K10 / K11 / K16 call: fp32, contiguous, on the device (conv: the weight's shape is the
    geometry's to check)."""
    require_cuda_f32(mu_w, "weight.mean")
    require_cuda_f32(rho_w, "weight.scale")
    if mu_b is not None:
        require_cuda_f32(mu_b, "bias.mean")
        require_cuda_f32(rho_b, "bias.scale")


# What a local-reparameterization call needs to know of its weight posterior (the bias is Gaussian in both): two instances,
# _GAUSSIAN here (N(mu, sigma(rho)^2): LocalReparamLinear / ConvNd) and _LOG_SIGMA2 at K23 (N(theta, exp(log_sigma2)):
# VariationalDropoutLinear / ConvNd).
#   name                 the error prefix: linear_<name>, conv_<name>
#   prepare              (mean, par, rho_b, threshold) -> (mean plane, s2_w, s2_b): the operand launch
#   check                (mean, par, mu_b, rho_b, conv): dtype, layout and shape of the posterior tensors
#   wgrad, conv_wgrad    the weight-gradient entries of the dense and the conv layer, (x, g_m, g_v, par) -> (g_mean, g_par, bias)
_LrtPosterior = collections.namedtuple("_LrtPosterior", ("name", "prepare", "check", "wgrad", "conv_wgrad"))

_GAUSSIAN = _LrtPosterior("lrt", lambda mu_w, rho_w, rho_b, threshold: (mu_w,) + _lrt_prepare_raw(rho_w, rho_b), _lrt_check_posterior,
                          "bnn_lrt_backward_weight", "bnn_conv3d_lrt_backward_weight")


def _lrt_refuse_masked_grad(who, ctx, track, threshold):
    if track and threshold is not None and any(ctx.needs_input_grad[1:5]):
        raise BnnHipError("%s: a threshold is set (%r) and a posterior tensor requires a gradient: the mask is for "
                          "inference" % (who, threshold))


class _LrtLinear(torch.autograd.Function):
    """y_s = m + sqrt(v + 1e-16) eps_s, m = x mean_w^T + mu_b, v = x^2 (s2_w)^T + sigma_b^2 (LocalReparamLinear,
    VariationalDropoutLinear): the posterior's operand launch (post.prepare: s2_w, sigma_b^2, with a threshold the masked planes)
    + one contraction launch for all S samples.  Backward: eps re-created from the key in one elementwise launch (g_m, g_v from
    the saved v), then the paired input- and weight-gradient contractions (csrc/bnn_lrt.hip; post.wgrad) -- no torch matmul."""

    @staticmethod
    def forward(ctx, x, mean_w, par_w, mu_b, rho_b, key, shared_x, compute, out_dtype, track, post, threshold):
        # x: (B, K) shared by all samples, or (S, B, K); fp32 or (bf16 compute mode) bf16
        who = "linear_" + post.name
        x = x.contiguous()
        require_cuda_act(x, "x")
        if (x.dtype == torch.bfloat16 or out_dtype == torch.bfloat16) and compute != _lib.COMPUTE_BF16:
            raise BnnHipError("bf16 activations need compute mode 'bf16'")
        post.check(mean_w, par_w, mu_b, rho_b)
        S = key.nsamples
        B, K = x.shape[-2], x.shape[-1]
        N = mean_w.shape[0]
        if not shared_x and (x.dim() != 3 or x.shape[0] != S):
            raise BnnHipError("%s: a per-sample input must be (S, B, K) with S = %d, got %s" % (who, S, tuple(x.shape)))
        why = lrt_eligible(x, mean_w, B, S)
        if why is not None:
            raise BnnHipError(who + ": " + why)
        dev = x.device
        needs_grad = track and any(ctx.needs_input_grad[:5])
        _lrt_refuse_masked_grad(who, ctx, track, threshold)
        mean, s2_w, s2_b = post.prepare(mean_w, par_w, rho_b if mu_b is not None else None, threshold)
        y = torch.empty((S, B, N), dtype=out_dtype, device=dev)
        v = torch.empty((B, N) if shared_x else (S, B, N), dtype=torch.float32, device=dev) if needs_grad else None
        flags = (_lib.FLAG_X_BF16 if _bf(x) else 0) | (_lib.FLAG_Y_BF16 if out_dtype == torch.bfloat16 else 0)
        r = _rng_struct(key, dev)
        check(_lib.load().bnn_lrt_forward(ptr(x), K, ptr(mean), ptr(s2_w), ptr(mu_b), ptr(s2_b), ptr(y), ptr(v), B, N, K, S,
                                          1 if shared_x else 0, ctypes.byref(r), compute, flags, stream_ptr(dev)), "bnn_lrt_forward")
        if needs_grad:
            # (mean: with a threshold the masked plane -- then only the input's gradient is ever asked for, through the masked layer)
            ctx.save_for_backward(x, mean, par_w, rho_b if mu_b is not None else None, s2_w, v)
        ctx.post, ctx.key, ctx.shared_x, ctx.compute = post, key, shared_x, compute
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mean_w, par_w, rho_b, s2_w, v = ctx.saved_tensors
        S, compute, shared = ctx.key.nsamples, ctx.compute, ctx.shared_x
        need = ctx.needs_input_grad
        N, K = mean_w.shape
        B = x.shape[-2]
        M = B if shared else S * B
        dev = gy.device
        lib = _lib.load()
        gy = gy.contiguous()
        if compute != _lib.COMPUTE_BF16 and gy.dtype != torch.float32:
            gy = gy.float()
        g_m = torch.empty((M, N), dtype=torch.float32, device=dev)
        g_v = torch.empty((M, N), dtype=torch.float32, device=dev)
        r = _rng_struct(ctx.key, dev)
        check(lib.bnn_lrt_backward_epilogue(ptr(gy), ptr(v), ptr(g_m), ptr(g_v), B, N, S, 1 if shared else 0, ctypes.byref(r),
                                            _lib.FLAG_X_BF16 if _bf(gy) else 0, stream_ptr(dev)), "bnn_lrt_backward_epilogue")
        xflag = _lib.FLAG_X_BF16 if _bf(x) else 0
        gx = g_mean_w = g_par_w = g_mu_b = g_rho_b = None
        if need[0]:
            gx = torch.empty_like(x)
            check(lib.bnn_lrt_backward_input(ptr(g_m), ptr(g_v), ptr(mean_w), ptr(s2_w), ptr(x), K, ptr(gx), M, N, K, compute,
                                             xflag | (_lib.FLAG_Y_BF16 if _bf(x) else 0), stream_ptr(dev)), "bnn_lrt_backward_input")
        need_b = rho_b is not None and (need[3] or need[4])
        if need[1] or need[2] or need_b:
            g_mean_w, g_par_w = torch.empty_like(mean_w), torch.empty_like(par_w)
            if need_b:
                g_mu_b, g_rho_b = torch.empty_like(rho_b), torch.empty_like(rho_b)
            check(getattr(lib, ctx.post.wgrad)(ptr(x), K, ptr(g_m), ptr(g_v), ptr(par_w), ptr(g_mean_w), ptr(g_par_w),
                                               ptr(rho_b) if need_b else None, ptr(g_mu_b), ptr(g_rho_b), M, N, K, compute, xflag,
                                               stream_ptr(dev)), ctx.post.wgrad)
        return gx, g_mean_w, g_par_w, g_mu_b, g_rho_b, None, None, None, None, None, None, None


def _linear_lrt(post, x, mean_w, par_w, mu_b, rho_b, key, shared_x, compute, out_dtype, threshold=None):
    return _LrtLinear.apply(x, mean_w.contiguous(), par_w.contiguous(),
                            None if mu_b is None else mu_b.contiguous(), None if rho_b is None else rho_b.contiguous(),
                            key, shared_x, _compute_code(compute), out_dtype, torch.is_grad_enabled(), post,
                            None if threshold is None else float(threshold))


def linear_lrt(x, mu_w, rho_w, mu_b, rho_b, key, shared_x, compute="f32", out_dtype=torch.float32):
    """LocalReparamLinear on the device: -> (S, B, N), S = key.nsamples; sample s uses eps[b N + n] of the key's sample
    sample0 + s.  Raises BnnHipError (with lrt_eligible's reason) for a call the kernel refuses: no torch fallback."""
    return _linear_lrt(_GAUSSIAN, x, mu_w, rho_w, mu_b, rho_b, key, shared_x, compute, out_dtype)


# --------------------------------------------------------------------------- K16: moment propagation (sampling-free inference)
class Moments:
    """A mean and a variance per activation, independent across elements (the mean-field assumption): what a dense layer takes
    and hands on inside a BayesianNetworkModule.predictive_moments pass.  A plain holder, not a Tensor; var None = a
    deterministic input (every variance zero), as the first Bayesian layer of a network sees.  It reshapes like a tensor (shape,
    size, dim, view, reshape, flatten -- each applied to mean and var alike), so torch.nn.Flatten and `x.view(x.size(0), -1)`
    work on it unchanged.  link: None, or 'softmax' when the moments are those of logits whose softmax ends the network
    (nn.MomentSoftmax): the predictive_* tails apply it to the sampled logits, and no layer takes such moments.  cov: None, or
    the (*rows, N, N) covariance of the N outputs of a row (K21: predictive_moments(covariance=True) at a dense head; its diagonal
    is var).  Nothing propagates a covariance: every reshape, layer and activation hands on moments without one; only
    nn.MomentSoftmax keeps it, and moments_sample draws correlated outputs from it.  dropout: None, or the p of an MC-dropout mask
    that is still to be applied to SAMPLES of these moments (K22: an MC-dropout head in front of a softmax, whose mask cannot be
    folded into the moments because softmax(0) != 0); the moments are then the pre-dropout ones, and it is only ever set together
    with link='softmax'.  Reshapes keep it; the predictive_* tails mask the drawn logits."""
    # _act: the activation the producing launch applied (a conv launch's epilogue, or an MC-dropout layer's moments_dropout; the
    # twin behind it passes; 'identity': an MC-dropout layer's mask with no activation, which the activation twins refuse); _head: a dense layer's HeadOperands while a covariance pass runs (dropped and kept as cov is);
    # _pending: the p of an MC-dropout layer's mask on its way to the nn.MomentSoftmax directly behind it
    __slots__ = ("mean", "var", "link", "_act", "cov", "_head", "dropout", "_pending")

    def __init__(self, mean, var=None, link=None, cov=None, dropout=None):
        if var is not None and var.shape != mean.shape:
            raise ValueError("Moments: mean %s and var %s differ in shape" % (tuple(mean.shape), tuple(var.shape)))
        if link not in (None, 'softmax'):
            raise ValueError("Moments: link must be None or 'softmax', got %r" % (link,))
        if cov is not None and (mean.dim() < 1 or tuple(cov.shape) != tuple(mean.shape) + (mean.shape[-1],)):
            raise ValueError("Moments: cov %s is not mean's shape %s with its last axis repeated" % (tuple(cov.shape), tuple(mean.shape)))
        if dropout is not None:
            if link != 'softmax':
                raise ValueError("Moments: dropout is the mask of an MC-dropout head in front of a softmax: it needs link='softmax'")
            check_drop_prob(dropout)
        self.mean, self.var, self.link, self._act, self.cov, self._head = mean, var, link, None, cov, None
        self.dropout, self._pending = dropout, None

    def __repr__(self):
        return "Moments(mean=%r, var=%r%s%s%s)" % (self.mean, self.var, "" if self.link is None else ", link=%r" % self.link,
                                                   "" if self.cov is None else ", cov=%r" % (self.cov,),
                                                   "" if self.dropout is None else ", dropout=%r" % (self.dropout,))

    def _both(self, fn):
        out = Moments(fn(self.mean), None if self.var is None else fn(self.var), self.link, dropout=self.dropout)
        out._pending = self._pending
        if self._act == 'identity':                  # (K22) a reshape does not make a masked output Gaussian
            out._act = self._act
        return out

    @property
    def shape(self):
        return self.mean.shape

    def size(self, dim=None):
        return self.mean.size() if dim is None else self.mean.size(dim)

    def dim(self):
        return self.mean.dim()

    def view(self, *shape):
        return self._both(lambda t: t.view(*shape))

    def reshape(self, *shape):
        return self._both(lambda t: t.reshape(*shape))

    def flatten(self, start_dim=0, end_dim=-1):
        return self._both(lambda t: t.flatten(start_dim, end_dim))


def _as_moments(a, who):
    if isinstance(a, Moments):
        return a
    if torch.is_tensor(a):
        return Moments(a, None)
    raise TypeError("%s: expected a tensor or ops.Moments, got %s" % (who, type(a).__name__))


def _tracking(track):
    """track=True asks a moment call for its autograd graph; it has one when grad mode is on."""
    return bool(track) and torch.is_grad_enabled()


class _MomentsLinear(torch.autograd.Function):
    """(m, v) of ops.moments_linear's pre-activation with a backward (K18): a deterministic input (av None) takes K10's two
    backward launches (bnn_lrt_backward_input / _weight with x = a_m), an input that carries a variance the three-contraction
    ones of csrc/bnn_moments_bwd.hip.  am, av: (B, K) fp32, contiguous; the posterior tensors contiguous."""

    @staticmethod
    def forward(ctx, am, av, mu_w, rho_w, mu_b, rho_b, code):
        B, K = am.shape
        N = mu_w.shape[0]
        dev = am.device
        s2_w, s2_b = _lrt_prepare_raw(rho_w, rho_b if mu_b is not None else None)
        out_m = torch.empty((B, N), dtype=torch.float32, device=dev)
        out_v = torch.empty((B, N), dtype=torch.float32, device=dev)
        check(_lib.load().bnn_moments_forward(ptr(am), ptr(av), K, ptr(mu_w), ptr(s2_w), ptr(mu_b), ptr(s2_b), ptr(out_m), ptr(out_v),
                                              B, N, K, code, 0, stream_ptr(dev)), "bnn_moments_forward")
        ctx.save_for_backward(am, av, mu_w, rho_w, rho_b if mu_b is not None else None, s2_w)
        ctx.code = code
        return out_m, out_v

    @staticmethod
    def backward(ctx, g_m, g_v):
        am, av, mu_w, rho_w, rho_b, s2_w = ctx.saved_tensors
        code = ctx.code
        B, K = am.shape
        N = mu_w.shape[0]
        dev = am.device
        lib = _lib.load()
        g_m, g_v = g_m.contiguous(), g_v.contiguous()
        g_am = g_av = g_mu_w = g_rho_w = g_mu_b = g_rho_b = None
        if ctx.needs_input_grad[0] or (av is not None and ctx.needs_input_grad[1]):
            g_am = torch.empty_like(am)
            if av is None:
                check(lib.bnn_lrt_backward_input(ptr(g_m), ptr(g_v), ptr(mu_w), ptr(s2_w), ptr(am), K, ptr(g_am), B, N, K, code, 0,
                                                 stream_ptr(dev)), "bnn_lrt_backward_input")
            else:
                g_av = torch.empty_like(av)
                check(lib.bnn_moments_backward_input(ptr(g_m), ptr(g_v), ptr(mu_w), ptr(s2_w), ptr(am), K, ptr(g_am), ptr(g_av),
                                                     B, N, K, code, 0, stream_ptr(dev)), "bnn_moments_backward_input")
        need_b = rho_b is not None and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5])
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3] or need_b:
            g_mu_w, g_rho_w = torch.empty_like(mu_w), torch.empty_like(rho_w)
            if need_b:
                g_mu_b, g_rho_b = torch.empty_like(rho_b), torch.empty_like(rho_b)
            pb = ptr(rho_b) if need_b else None
            if av is None:
                check(lib.bnn_lrt_backward_weight(ptr(am), K, ptr(g_m), ptr(g_v), ptr(rho_w), ptr(g_mu_w), ptr(g_rho_w), pb,
                                                  ptr(g_mu_b), ptr(g_rho_b), B, N, K, code, 0, stream_ptr(dev)),
                      "bnn_lrt_backward_weight")
            else:
                check(lib.bnn_moments_backward_weight(ptr(am), ptr(av), K, ptr(g_m), ptr(g_v), ptr(mu_w), ptr(rho_w), ptr(g_mu_w),
                                                      ptr(g_rho_w), pb, ptr(g_mu_b), ptr(g_rho_b), B, N, K, code, 0, stream_ptr(dev)),
                      "bnn_moments_backward_weight")
        return g_am, g_av, g_mu_w, g_rho_w, g_mu_b, g_rho_b, None


class _MomentsRelu(torch.autograd.Function):
    """bnn_moments_relu out of place with bnn_moments_relu_backward behind it; m, v fp32, contiguous."""

    @staticmethod
    def forward(ctx, m, v):
        om, ov = torch.empty_like(m), torch.empty_like(v)
        check(_lib.load().bnn_moments_relu(ptr(m), ptr(v), ptr(om), ptr(ov), m.numel(), stream_ptr(m.device)), "bnn_moments_relu")
        ctx.save_for_backward(m, v)
        return om, ov

    @staticmethod
    def backward(ctx, g_om, g_ov):
        m, v = ctx.saved_tensors
        g_om, g_ov = g_om.contiguous(), g_ov.contiguous()
        g_m, g_v = torch.empty_like(m), torch.empty_like(v)
        check(_lib.load().bnn_moments_relu_backward(ptr(m), ptr(v), ptr(g_om), ptr(g_ov), ptr(g_m), ptr(g_v), m.numel(),
                                                    stream_ptr(m.device)), "bnn_moments_relu_backward")
        return g_m, g_v


class _MomentsSample(torch.autograd.Function):
    """bnn_moments_sample with K10's noise launch as its backward: g_m = sum_s gy_s, g_v = sum_s gy_s eps_s / (2 sqrt(v + 1e-16)),
    eps re-created from the key (bnn_lrt_backward_epilogue on a shared input -- index for index the forward's eps)."""

    @staticmethod
    def forward(ctx, m, v, key, S):
        N = m.shape[-1]
        rows = m.numel() // N
        y = torch.empty((S,) + tuple(m.shape), dtype=torch.float32, device=m.device)
        r = _rng_struct(key, m.device)
        check(_lib.load().bnn_moments_sample(ptr(m), ptr(v), ptr(y), rows, N, S, ctypes.byref(r), 0, stream_ptr(m.device)),
              "bnn_moments_sample")
        ctx.save_for_backward(v)
        ctx.key, ctx.S, ctx.rows = key, S, rows
        return y

    @staticmethod
    def backward(ctx, gy):
        v, = ctx.saved_tensors
        gy = gy.contiguous()
        g_m, g_v = torch.empty_like(v), torch.empty_like(v)
        r = _rng_struct(ctx.key, v.device)
        check(_lib.load().bnn_lrt_backward_epilogue(ptr(gy), ptr(v), ptr(g_m), ptr(g_v), ctx.rows, v.shape[-1], ctx.S, 1,
                                                    ctypes.byref(r), 0, stream_ptr(v.device)), "bnn_lrt_backward_epilogue")
        return g_m, g_v, None, None


def moments_linear(a, mu_w, rho_w, mu_b, rho_b, relu=False, compute="f32", track=False):
    """Mean and variance of a dense layer's pre-activation for independent Gaussian weights, from the mean and variance of its
    input (bnn_lrt_prepare + bnn_moments_forward, csrc/bnn_moments.hip) -> Moments, fp32 (*rows, N):

        m = a_m mu_w^T + mu_b,    v = a_m^2 (sigma_w^2)^T + a_v (mu_w^2 + sigma_w^2)^T + sigma_b^2

    a: a device tensor (a deterministic input: the second term is absent) or a Moments.  relu: the moment-matched ReLU of
    moments_relu in the launch's epilogue (the same bits).  A bf16 `a` is read as it is in the 'bf16' mode (deterministic input
    only).  Nothing is drawn, no key is touched.  track=False (inference): the result is detached whatever the grad mode.
    track=True with grad mode on (training without sampling, K18): the result is attached to the graph of `a` and the four
    posterior tensors; the backward is HIP (csrc/bnn_moments_bwd.hip; K10's launches for a deterministic input); `a` is fp32."""
    return _moments_linear("moments_linear", _GAUSSIAN, a, mu_w, rho_w, mu_b, rho_b, relu, compute, track)


def _moments_linear(who, post, a, mu_w, par_w, mu_b, rho_b, relu, compute, track, threshold=None):
    """moments_linear / moments_linear_vd: the input's preparation, the checks and the untracked launch on the planes of
    post.prepare; track (the Gaussian posterior only) hands over to _MomentsLinear."""
    mom = _as_moments(a, who)
    code = _compute_code(compute)
    tracked = _tracking(track)
    keep = (lambda t: t) if tracked else (lambda t: t.detach())
    am = keep(mom.mean)
    av = None if mom.var is None else keep(mom.var)
    mu_w, par_w = keep(mu_w).contiguous(), keep(par_w).contiguous()
    if mu_b is not None:
        mu_b, rho_b = keep(mu_b).contiguous(), keep(rho_b).contiguous()
    post.check(mu_w, par_w, mu_b, rho_b)
    N, K = mu_w.shape
    if am.dim() < 1 or am.shape[-1] != K:
        raise BnnHipError("%s: input has %s features, weight expects %d" % (who, am.shape[-1] if am.dim() else "no", K))
    lead = tuple(am.shape[:-1])
    am = am.reshape(-1, K).contiguous()
    require_cuda_act(am, "a.mean")
    if am.dtype == torch.bfloat16 and (code != _lib.COMPUTE_BF16 or av is not None):
        raise BnnHipError("%s: a bf16 input needs compute mode 'bf16' and no variance (hidden moments are fp32)" % who)
    if av is not None:
        av = av.reshape(-1, K).contiguous()
        require_cuda_f32(av, "a.var")
    B = am.shape[0]
    if B > 64 * 65535:
        raise BnnHipError("%s: %d rows (at most %d)" % (who, B, 64 * 65535))
    if tracked:
        # the same launches' bits, the ReLU as bnn_moments_relu behind the contraction instead of in its epilogue (one device
        # function): the backward needs the pre-activation
        if _bf(am):
            raise BnnHipError("%s: track=True takes an fp32 input" % who)
        m, v = _MomentsLinear.apply(am, av, mu_w, par_w, mu_b, rho_b, code)
        if relu:
            m, v = _MomentsRelu.apply(m, v)
        return Moments(m.reshape(lead + (N,)), v.reshape(lead + (N,)))
    dev = am.device
    mu_w, s2_w, s2_b = post.prepare(mu_w, par_w, rho_b if mu_b is not None else None, threshold)
    out_m = torch.empty((B, N), dtype=torch.float32, device=dev)
    out_v = torch.empty((B, N), dtype=torch.float32, device=dev)
    flags = (_lib.FLAG_RELU if relu else 0) | (_lib.FLAG_X_BF16 if _bf(am) else 0)
    check(_lib.load().bnn_moments_forward(ptr(am), ptr(av), K, ptr(mu_w), ptr(s2_w), ptr(mu_b), ptr(s2_b), ptr(out_m), ptr(out_v),
                                          B, N, K, code, flags, stream_ptr(dev)), "bnn_moments_forward")
    return Moments(out_m.reshape(lead + (N,)), out_v.reshape(lead + (N,)))


def moments_relu(mom, track=False):
    """ReLU of Gaussian activations by moment matching (bnn_moments_relu) -> Moments: with s = sqrt(v), alpha = m / s,
    mean' = s (alpha Phi + phi), var' = v (Phi + alpha^2 Phi Phi(-alpha) + alpha phi (Phi(-alpha) - Phi) - phi^2) clamped at 0;
    v == 0 gives (max(m, 0), 0).  A deterministic input (var None) stays one.  track=True with grad mode on: attached to the
    graph, the backward is bnn_moments_relu_backward (a deterministic input: torch.relu's)."""
    mom = _as_moments(mom, "moments_relu")
    if _tracking(track):
        if mom.var is None:
            return Moments(torch.relu(mom.mean), None)
        m, v = mom.mean.contiguous(), mom.var.contiguous()
        require_cuda_f32(m, "mean")
        require_cuda_f32(v, "var")
        return Moments(*_MomentsRelu.apply(m, v))
    if mom.var is None:
        return Moments(torch.relu(mom.mean.detach()), None)
    m, v = mom.mean.detach().contiguous(), mom.var.detach().contiguous()
    require_cuda_f32(m, "mean")
    require_cuda_f32(v, "var")
    om, ov = torch.empty_like(m), torch.empty_like(v)
    check(_lib.load().bnn_moments_relu(ptr(m), ptr(v), ptr(om), ptr(ov), m.numel(), stream_ptr(m.device)), "bnn_moments_relu")
    return Moments(om, ov)


def moments_sample(mom, key, nsamples, track=False):
    """nsamples draws of independent Gaussians with the given moments in ONE launch (bnn_moments_sample) -> (S, *shape) fp32:
    y_s[e] = m[e] + sqrt(v[e] + 1e-16) eps_s[e], e the flat index within one sample, eps_s[e] element e of the key's sample
    sample0 + s (the LRT-noise contract).  The result is what the mc_* tails read.  CPU moments: torch.randn (the key is not
    used and may be None).  track=True with grad mode on: differentiable in the moments -- the backward re-creates eps from the
    key (bnn_lrt_backward_epilogue: g_m = sum_s gy_s, g_v = sum_s gy_s eps_s / (2 sqrt(v + 1e-16))).
    Moments that carry a covariance (mom.cov, K21) are drawn correlated: y_s[b, :] = m[b, :] + Lc_b eps_s[b, :] with Lc_b the
    lower Cholesky factor of cov[b] in float64 (bnn_moments_sample_cov; the same eps on the same key; CPU: cholesky_pivot_f64 and
    torch.randn).  Inference only: track=True with grad mode on raises BnnHipError."""
    mom = _as_moments(mom, "moments_sample")
    S = int(nsamples)
    if mom.cov is not None:
        return _moments_sample_cov(mom, key, S, track)
    tracked = _tracking(track)
    keep = (lambda t: t) if tracked else (lambda t: t.detach())
    m = keep(mom.mean)
    v = torch.zeros_like(m) if mom.var is None else keep(mom.var)
    if not m.is_cuda:
        m64, v64 = m.double(), v.double()
        return (m64 + torch.sqrt(v64 + 1e-16) * torch.randn((S,) + tuple(m.shape), dtype=torch.float64)).to(torch.float32)
    m, v = m.contiguous(), v.contiguous()
    require_cuda_f32(m, "mean")
    require_cuda_f32(v, "var")
    if m.dim() < 1:
        raise BnnHipError("moments_sample: the moments must have at least one axis")
    N = m.shape[-1]
    rows = m.numel() // N if N else 0
    if S < 1 or S > 0xFFFF:
        raise BnnHipError("moments_sample: %d MC samples (1 .. 65535)" % S)
    if m.numel() >= 2 ** 32:
        raise BnnHipError("moments_sample: one sample has %d elements: the noise index is 32 bits wide" % m.numel())
    m, v = (t if _aligned16(t) else t.clone() for t in (m, v))     # (bnn_moments_sample refuses moments off a 16-B boundary)
    if tracked:
        return _MomentsSample.apply(m, v, key, S)
    y = torch.empty((S,) + tuple(m.shape), dtype=torch.float32, device=m.device)
    r = _rng_struct(key, m.device)
    check(_lib.load().bnn_moments_sample(ptr(m), ptr(v), ptr(y), rows, N, S, ctypes.byref(r), 0, stream_ptr(m.device)),
          "bnn_moments_sample")
    return y


def _f64(track):
    """t -> float64, detached unless track=True with grad mode on."""
    if _tracking(track):
        return lambda t: t.to(torch.float64)
    return lambda t: t.detach().to(torch.float64)


def moments_relu_f64(mom, track=False):
    """moments_relu in float64 torch.  track=True: not detached (plain torch autograd; at v == 0 the gradient is the stated
    convention of moments_relu_backward_f64)."""
    mom = _as_moments(mom, "moments_relu_f64")
    f64 = _f64(track)
    m = f64(mom.mean)
    if mom.var is None:
        return Moments(torch.relu(m) if _tracking(track) else m.clamp_min(0), None)
    v = f64(mom.var)
    pos = v > 0
    s = torch.sqrt(torch.where(pos, v, torch.ones_like(v)))
    al = m / s
    cdf, cdc = 0.5 * torch.special.erfc(-al / math.sqrt(2.0)), 0.5 * torch.special.erfc(al / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * al * al) / math.sqrt(2.0 * math.pi)
    mean = s * (al * cdf + pdf)
    var = (v * (cdf + al * al * cdf * cdc + al * pdf * (cdc - cdf) - pdf * pdf)).clamp_min(0)
    if _tracking(track):        # the same values; v == 0 passes both gradients where m > 0
        return Moments(torch.where(pos, mean, torch.relu(m)), torch.where(pos, var, torch.where(m > 0, v, torch.zeros_like(v))))
    return Moments(torch.where(pos, mean, m.clamp_min(0)), torch.where(pos, var, torch.zeros_like(v)))


def moments_relu_backward_f64(mom, g_mean, g_var):
    """The backward of moments_relu in float64 torch, as a formula: (g_m, g_v) at the pre-activation `mom` from the gradients
    of the two outputs.  With s = sqrt(v), alpha = m / s, Phi / phi the normal cdf / pdf and mean' the forward's mean:

        g_m = g_mean Phi + g_var 2 mean' Phi(-alpha),    g_v = g_mean phi / (2 s) + g_var (Phi - mean' phi / s)

    Where the forward clamped var' to 0 the g_var terms are 0; v == 0 gives g_m = g_mean [m > 0], g_v = g_var [m > 0]; a
    deterministic input (var None) is plain ReLU: (g_mean [m > 0], None)."""
    mom = _as_moments(mom, "moments_relu_backward_f64")
    f64 = lambda t: t.detach().to(torch.float64)         # noqa: E731
    m, g_mean = f64(mom.mean), f64(g_mean)
    on = (m > 0).to(torch.float64)
    if mom.var is None:
        return g_mean * on, None
    v, g_var = f64(mom.var), f64(g_var)
    pos = v > 0
    s = torch.sqrt(torch.where(pos, v, torch.ones_like(v)))
    al = m / s
    cdf, cdc = 0.5 * torch.special.erfc(-al / math.sqrt(2.0)), 0.5 * torch.special.erfc(al / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * al * al) / math.sqrt(2.0 * math.pi)
    mean = s * (al * cdf + pdf)
    r = cdf + al * al * cdf * cdc + al * pdf * (cdc - cdf) - pdf * pdf
    gv = torch.where(v * r < 0, torch.zeros_like(g_var), g_var)
    g_m = g_mean * cdf + gv * (2.0 * mean * cdc)
    g_v = g_mean * (0.5 * pdf / s) + gv * (cdf - mean * pdf / s)
    return torch.where(pos, g_m, g_mean * on), torch.where(pos, g_v, g_var * on)


def moments_linear_f64(a, mu_w, rho_w, mu_b, rho_b, relu=False, track=False):
    """moments_linear in float64 torch (sigma = 1e-10 + softplus(rho)) -> Moments of float64 tensors.  track=True: not detached."""
    f64 = _f64(track)
    return _moments_linear_planes_f64(_as_moments(a, "moments_linear_f64"), f64(mu_w), _sigma2_f64(f64(rho_w)), mu_b, rho_b, relu, track)


def _sigma2_f64(rho):
    return (1e-10 + torch.nn.functional.softplus(rho)) ** 2


def _moments_linear_planes_f64(mom, mu, s2, mu_b, rho_b, relu, track):
    """The dense moment layer in float64 on the weight's mean and variance planes (float64 already); the bias is Gaussian."""
    f64 = _f64(track)
    am = f64(mom.mean)
    m = am @ mu.t()
    v = (am * am) @ s2.t()
    if mom.var is not None:
        v = v + f64(mom.var) @ (mu * mu + s2).t()
    if mu_b is not None:
        m, v = m + f64(mu_b), v + _sigma2_f64(f64(rho_b))
    out = Moments(m, v)
    return moments_relu_f64(out, track) if relu else out


def moments_f64(a, layers, track=False):
    """The moment recursion of a chain of dense layers in float64 torch -- the CPU path of predictive_moments and the tests'
    reference: a, a tensor or Moments; layers, a sequence of (mu_w, rho_w, mu_b, rho_b, relu).  -> Moments of float64 tensors.
    track=True: not detached (torch autograd through the whole recursion)."""
    mom = _as_moments(a, "moments_f64")
    for mu_w, rho_w, mu_b, rho_b, relu in layers:
        mom = moments_linear_f64(mom, mu_w, rho_w, mu_b, rho_b, relu, track)
    return mom


# --------------------------------------------------------------------------- K23: sparse variational dropout
VD_K1, VD_K2, VD_K3 = 0.63576, 1.87320, 1.48695         # Molchanov et al. 2017, eq. 14
VD_CLAMP = 8.0


def vd_log_alpha(theta, log_sigma2):
    """clamp(log_sigma2 - ln(theta^2), -8, 8) in torch, in the dtype given (theta = 0: +8) -- the CPU path and the references.
    Differentiable: 0 where the clamp is active, and theta = 0 is taken out of the logarithm so that it gets 0 there, not 0 / 0."""
    zero = theta == 0
    la = torch.clamp(log_sigma2 - 2.0 * torch.log(torch.abs(torch.where(zero, torch.ones_like(theta), theta))), -VD_CLAMP, VD_CLAMP)
    return torch.where(zero, torch.full_like(la, VD_CLAMP), la)


def vd_kl_elements(theta, log_sigma2):
    """The element-wise KL to the log-uniform prior in torch (differentiable): k1 sigmoid(-(k2 + k3 log_alpha)) + 0.5
    log1p(exp(-log_alpha)).  The clamp's gradient is 0 where it is active; theta = 0 lies there and gets exactly 0."""
    la = vd_log_alpha(theta, log_sigma2)
    return VD_K1 * torch.sigmoid(-(VD_K2 + VD_K3 * la)) + 0.5 * torch.log1p(torch.exp(-la))


def _vd_prepare_raw(theta, log_sigma2, rho_b, threshold=None):
    """-> (theta plane, s2 plane, s2_b, count): one bnn_vd_prepare launch.  threshold None: theta itself, s2 = exp(log_sigma2),
    count None.  A float: the masked planes (elements with log_alpha > threshold zeroed) and their number, a 0-d int64 tensor."""
    s2_w = torch.empty_like(log_sigma2)
    s2_b = torch.empty_like(rho_b) if rho_b is not None else None
    masked = threshold is not None
    th_out = torch.empty_like(theta) if masked else None
    count = torch.empty((), dtype=torch.int64, device=theta.device) if masked else None
    check(_lib.load().bnn_vd_prepare(ptr(theta), ptr(log_sigma2), theta.numel(), ptr(rho_b), ptr(s2_b),
                                     rho_b.numel() if rho_b is not None else 0, float(threshold) if masked else math.inf,
                                     ptr(th_out), ptr(s2_w), ptr(count), stream_ptr(theta.device)), "bnn_vd_prepare")
    return (th_out if masked else theta), s2_w, s2_b, count


def _vd_check_posterior(theta, log_sigma2, mu_b, rho_b, conv=False):
    """conv: the weight of a VariationalDropoutConvNd, (O, C / groups, *kernel) with 1, 2 or 3 kernel axes, in place of (N, K)."""
    require_cuda_f32(theta, "weight.mean")
    require_cuda_f32(log_sigma2, "weight.log_sigma2")
    if conv:
        if theta.shape != log_sigma2.shape or theta.dim() not in (3, 4, 5):
            raise BnnHipError("conv_vd: weight.mean %s and weight.log_sigma2 %s must be one (O, C / groups, *kernel) shape with "
                              "1, 2 or 3 kernel axes" % (tuple(theta.shape), tuple(log_sigma2.shape)))
    elif theta.shape != log_sigma2.shape or theta.dim() != 2:
        raise BnnHipError("linear_vd: weight.mean %s and weight.log_sigma2 %s must be one (N, K) shape"
                          % (tuple(theta.shape), tuple(log_sigma2.shape)))
    if mu_b is not None:
        require_cuda_f32(mu_b, "bias.mean")
        require_cuda_f32(rho_b, "bias.scale")


def _vd_refuse_masked_grad(who, threshold, *posterior):
    if threshold is not None and torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in posterior):
        raise BnnHipError("%s: a threshold is set (%r) and a posterior tensor requires a gradient: the mask is for inference -- "
                          "run under torch.no_grad(), or set layer.threshold = None to train" % (who, threshold))


_LOG_SIGMA2 = _LrtPosterior("vd", lambda theta, ls2, rho_b, threshold: _vd_prepare_raw(theta, ls2, rho_b, threshold)[:3],
                            _vd_check_posterior, "bnn_vd_backward_weight", "bnn_conv3d_vd_backward_weight")


def linear_vd(x, theta, log_sigma2, mu_b, rho_b, key, shared_x, compute="f32", out_dtype=torch.float32, threshold=None):
    """VariationalDropoutLinear on the device: -> (S, B, N), S = key.nsamples; y_s = m + sqrt(v + 1e-16) eps_s with m = x theta^T +
    mu_b, v = x^2 exp(log_sigma2)^T + sigma_b^2; sample s uses eps[b N + n] of the key's sample sample0 + s (the LRT-noise
    contract).  threshold: a float drops the weights with log_alpha > threshold (theta = 0, variance 0: bnn_vd_prepare's masked
    planes) -- inference only: a call that would need a gradient of a posterior tensor raises BnnHipError.  Calls the kernel
    refuses raise BnnHipError (lrt_eligible's reason): no torch fallback."""
    _vd_refuse_masked_grad("linear_vd", threshold, theta, log_sigma2, mu_b, rho_b)
    return _linear_lrt(_LOG_SIGMA2, x, theta, log_sigma2, mu_b, rho_b, key, shared_x, compute, out_dtype, threshold)


def vd_dropped(theta, log_sigma2, threshold):
    """The number of elements with log_alpha > threshold, a 0-d int64 device tensor (bnn_vd_prepare's count)."""
    theta, log_sigma2 = theta.detach().contiguous(), log_sigma2.detach().contiguous()
    require_cuda_f32(theta, "theta")
    require_cuda_f32(log_sigma2, "log_sigma2")
    return _vd_prepare_raw(theta, log_sigma2, None, float(threshold))[3]


def vd_dropped_mask(theta, log_sigma2, threshold):
    """The elements with log_alpha > threshold as a bool device tensor of theta's shape, read off bnn_vd_prepare's masked theta
    plane (one launch; a host-side report, not hot-path work).  Below the clamp's +8 a masked element is exactly a zero of that
    plane: theta = 0 has log_alpha = +8 and is masked, every kept element keeps its non-zero theta.  From +8 on nothing exceeds
    the threshold."""
    theta, log_sigma2 = theta.detach().contiguous(), log_sigma2.detach().contiguous()
    require_cuda_f32(theta, "theta")
    require_cuda_f32(log_sigma2, "log_sigma2")
    if float(threshold) >= VD_CLAMP:
        return torch.zeros_like(theta, dtype=torch.bool)
    return _vd_prepare_raw(theta, log_sigma2, None, float(threshold))[0] == 0


def moments_linear_vd(a, theta, log_sigma2, mu_b, rho_b, relu=False, compute="f32", threshold=None):
    """moments_linear for a VariationalDropoutLinear: the same launch (bnn_moments_forward) on the variance plane
    exp(log_sigma2), masked by `threshold` as linear_vd masks it (bnn_vd_prepare) -> Moments, fp32, detached.  Inference only."""
    return _moments_linear("moments_linear_vd", _LOG_SIGMA2, a, theta, log_sigma2, mu_b, rho_b, relu, compute, False, threshold)


def moments_linear_vd_f64(a, theta, log_sigma2, mu_b, rho_b, relu=False, threshold=None):
    """moments_linear_vd in float64 torch (the CPU path and the tests' reference) -> Moments of float64 tensors, detached."""
    th, s2 = _vd_planes_f64(theta, log_sigma2, threshold)
    return _moments_linear_planes_f64(_as_moments(a, "moments_linear_vd_f64"), th, s2, mu_b, rho_b, relu, False)


def _vd_planes_f64(theta, log_sigma2, threshold):
    """theta and exp(log_sigma2) in float64, detached, the elements with log_alpha > threshold zeroed in both."""
    th, ls2 = theta.detach().to(torch.float64), log_sigma2.detach().to(torch.float64)
    s2 = torch.exp(ls2)
    if threshold is not None:
        keep = ~(vd_log_alpha(th, ls2) > float(threshold))
        th, s2 = th * keep, s2 * keep
    return th, s2


def _vd_descs(thetas, ls2s):
    arr = (_lib.VdTensor * len(thetas))()
    for i, (t, l) in enumerate(zip(thetas, ls2s)):
        arr[i].theta, arr[i].log_sigma2, arr[i].n = t.data_ptr(), l.data_ptr(), t.numel()
    return arr


_vd_count_cache = {}


def _vd_counts(ns, device):
    """The element counts of a vd_kl call as an fp32 device tensor, uploaded once per (sizes, device)."""
    key = (ns, device.type, device.index)
    c = _vd_count_cache.get(key)
    if c is None:
        c = _vd_count_cache[key] = torch.tensor([float(n) for n in ns], dtype=torch.float32, device=device)
    return c


class _VdKL(torch.autograd.Function):
    """out[t] = mean over the elements of tensor t of the log-uniform KL: bnn_vd_kl_forward (per-tensor sums, two launches), / n_t;
    bnn_vd_kl_backward.  The gradient is returned, never parked (FUSE_KL_GRADIENT covers WeightNormal only)."""

    @staticmethod
    def forward(ctx, T, *params):
        thetas, ls2s = [p.detach() for p in params[:T]], [p.detach() for p in params[T:]]
        for t, l in zip(thetas, ls2s):
            require_cuda_f32(t, "theta")
            require_cuda_f32(l, "log_sigma2")
            if t.numel() != l.numel() or t.numel() < 1:
                raise BnnHipError("vd_kl: theta and log_sigma2 must have the same, non-zero number of elements")
        dev = thetas[0].device
        arr = _vd_descs(thetas, ls2s)
        nbytes = _lib.load().bnn_vd_kl_workspace_bytes(arr, T)
        if nbytes < 0:
            raise BnnHipError("bnn_vd_kl_workspace_bytes: bad tensors (1 .. 128 non-empty tensors)")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)            # per call: concurrent KLs never share it
        sums = torch.empty(T, dtype=torch.float32, device=dev)
        check(_lib.load().bnn_vd_kl_forward(arr, T, ptr(sums), ptr(ws), stream_ptr(dev)), "bnn_vd_kl_forward")
        ctx.save_for_backward(*params)
        ctx.T = T
        return sums / _vd_counts(tuple(t.numel() for t in thetas), dev)

    @staticmethod
    def backward(ctx, g):
        params = ctx.saved_tensors
        T = ctx.T
        thetas, ls2s = params[:T], params[T:]
        g_th = [torch.empty_like(t) for t in thetas]
        g_ls = [torch.empty_like(l) for l in ls2s]
        arr = _vd_descs(thetas, ls2s)
        up = g.contiguous().float()
        gt = (ctypes.c_void_p * T)(*[t.data_ptr() for t in g_th])
        gl = (ctypes.c_void_p * T)(*[t.data_ptr() for t in g_ls])
        check(_lib.load().bnn_vd_kl_backward(arr, T, ptr(up), gt, gl, 0, stream_ptr(up.device)), "bnn_vd_kl_backward")
        return (None,) + tuple(g_th) + tuple(g_ls)


def vd_kl(thetas, log_sigma2s):
    """-> (T,) fp32: each tensor's mean KL to the log-uniform prior (Molchanov et al. 2017's approximation on the clamped
    log_alpha), differentiable -- KLDivergence.compute_kl of a WeightVariationalDropout.  At most 128 tensors per call."""
    if len(thetas) != len(log_sigma2s) or not thetas:
        raise BnnHipError("vd_kl: one log_sigma2 per theta, at least one tensor")
    return _VdKL.apply(len(thetas), *[t.contiguous() for t in thetas], *[l.contiguous() for l in log_sigma2s])


# --------------------------------------------------------------------------- K17: moment propagation through convolutions and ELU
def _refuse_link(mom, who):
    """Moments that carry a link are the network's output: a softmax must end the network."""
    if mom.link is not None:
        raise BnnHipError("%s: the input carries link=%r: nn.MomentSoftmax must end the network (nothing propagates moments "
                          "through a softmax)" % (who, mom.link))
    if mom._pending is not None:
        raise BnnHipError("%s: the input carries the pending mask (dropout=%r) of an MC-dropout layer that nn.moment_activations "
                          "found directly in front of an nn.MomentSoftmax, and this module is not that softmax: call "
                          "nn.moment_activations again after changing a Sequential" % (who, mom._pending))


def _moment_activation(activation, who):
    """None | 'relu' | ('elu', alpha) -> (name or None, alpha)."""
    if activation is None:
        return None, 0.0
    if activation == 'relu':
        return 'relu', 0.0
    if isinstance(activation, (tuple, list)) and len(activation) == 2 and activation[0] == 'elu':
        alpha = float(activation[1])
        if not (0.0 <= alpha < float("inf")):
            raise BnnHipError("%s: ELU alpha must be finite and >= 0, got %r" % (who, alpha))
        return 'elu', alpha
    raise ValueError("%s: activation must be None, 'relu' or ('elu', alpha), got %r" % (who, activation))


class _MomentsConv(torch.autograd.Function):
    """(m, v) of ops.moments_convNd's pre-activation with a backward (K19): a deterministic input (av None) takes K11's backward
    launches (bnn_conv3d_lrt_backward_input / _weight with one image set and x = a_m), an input that carries a variance the
    three-contraction ones of csrc/bnn_conv3d.hip (k_moments_conv3d_bwd).  am, av: (B, C, *spatial) fp32, contiguous; the
    posterior tensors contiguous; sh: the bnn_conv3d_shape_t of the call, out_shape the output's."""

    @staticmethod
    def forward(ctx, am, av, mu_w, rho_w, mu_b, rho_b, sh, out_shape, code):
        dev = am.device
        s2_w, s2_b = _lrt_prepare_raw(rho_w, rho_b if mu_b is not None else None)
        out_m = torch.empty(out_shape, dtype=torch.float32, device=dev)
        out_v = torch.empty_like(out_m)
        check(_lib.load().bnn_conv3d_moments_forward(ptr(am), ptr(av), ptr(mu_w), ptr(s2_w), ptr(mu_b), ptr(s2_b), ptr(out_m),
                                                     ptr(out_v), ctypes.byref(sh), code, 0, 0.0, stream_ptr(dev)),
              "bnn_conv3d_moments_forward")
        ctx.save_for_backward(am, av, mu_w, rho_w, rho_b if mu_b is not None else None, s2_w)
        ctx.code, ctx.sh = code, sh
        return out_m, out_v

    @staticmethod
    def backward(ctx, g_m, g_v):
        am, av, mu_w, rho_w, rho_b, s2_w = ctx.saved_tensors
        code, sh = ctx.code, ctx.sh
        dev = am.device
        lib, st = _lib.load(), stream_ptr(dev)
        g_m, g_v = g_m.contiguous(), g_v.contiguous()
        g_am = g_av = g_mu_w = g_rho_w = g_mu_b = g_rho_b = None
        if ctx.needs_input_grad[0] or (av is not None and ctx.needs_input_grad[1]):
            g_am = torch.empty_like(am)
            if av is None:
                check(lib.bnn_conv3d_lrt_backward_input(ptr(g_m), ptr(g_v), ptr(mu_w), ptr(s2_w), ptr(am), ptr(g_am), ctypes.byref(sh),
                                                        1, code, st), "bnn_conv3d_lrt_backward_input")
            else:
                g_av = torch.empty_like(av)
                check(lib.bnn_conv3d_moments_backward_input(ptr(g_m), ptr(g_v), ptr(mu_w), ptr(s2_w), ptr(am), ptr(g_am), ptr(g_av),
                                                            ctypes.byref(sh), code, st), "bnn_conv3d_moments_backward_input")
        need_b = rho_b is not None and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5])
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3] or need_b:
            g_mu_w, g_rho_w = torch.empty_like(mu_w), torch.empty_like(rho_w)
            if need_b:
                g_mu_b, g_rho_b = torch.empty_like(rho_b), torch.empty_like(rho_b)
            pb = ptr(rho_b) if need_b else None
            if av is None:
                nb = lib.bnn_conv3d_lrt_backward_weight_workspace_bytes(ctypes.byref(sh), 1)
                ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)          # this call's own slabs
                check(lib.bnn_conv3d_lrt_backward_weight(ptr(am), ptr(g_m), ptr(g_v), ptr(rho_w), ptr(g_mu_w), ptr(g_rho_w), pb,
                                                         ptr(g_mu_b), ptr(g_rho_b), ctypes.byref(sh), 1, code, ptr(ws), nb, st),
                      "bnn_conv3d_lrt_backward_weight")
            else:
                nb = lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(sh))
                ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
                check(lib.bnn_conv3d_moments_backward_weight(ptr(am), ptr(av), ptr(g_m), ptr(g_v), ptr(mu_w), ptr(rho_w), ptr(g_mu_w),
                                                             ptr(g_rho_w), pb, ptr(g_mu_b), ptr(g_rho_b), ctypes.byref(sh), code,
                                                             ptr(ws), nb, st), "bnn_conv3d_moments_backward_weight")
        return g_am, g_av, g_mu_w, g_rho_w, g_mu_b, g_rho_b, None, None, None


class _MomentsElu(torch.autograd.Function):
    """bnn_moments_elu out of place with bnn_moments_elu_backward behind it; m, v fp32, contiguous."""

    @staticmethod
    def forward(ctx, m, v, alpha):
        om, ov = torch.empty_like(m), torch.empty_like(v)
        check(_lib.load().bnn_moments_elu(ptr(m), ptr(v), ptr(om), ptr(ov), m.numel(), alpha, stream_ptr(m.device)), "bnn_moments_elu")
        ctx.save_for_backward(m, v)
        ctx.alpha = alpha
        return om, ov

    @staticmethod
    def backward(ctx, g_om, g_ov):
        m, v = ctx.saved_tensors
        g_om, g_ov = g_om.contiguous(), g_ov.contiguous()
        g_m, g_v = torch.empty_like(m), torch.empty_like(v)
        check(_lib.load().bnn_moments_elu_backward(ptr(m), ptr(v), ptr(g_om), ptr(g_ov), ptr(g_m), ptr(g_v), m.numel(), ctx.alpha,
                                                   stream_ptr(m.device)), "bnn_moments_elu_backward")
        return g_m, g_v, None


class _MomentsAffine(torch.autograd.Function):
    """ops.moments_affine on moments that carry a variance, with K18's two backward launches behind it: the input gradient with
    the zero sigma^2 plane (g_a_m = G_m w, g_a_v = G_v w^2), the weight gradient with a zero rho whose g_rho_w is discarded
    (g_w = G_m^T a_m + 2 w (.) G_v^T a_v; the bias sums ride along: g_b = sum G_m).  am, av (B, K), w (N, K), b (N) or None."""

    @staticmethod
    def forward(ctx, am, av, w, b, code):
        B, K = am.shape
        N = w.shape[0]
        dev = am.device
        z_w = torch.zeros_like(w)
        z_b = None if b is None else torch.zeros_like(b)
        out_m = torch.empty((B, N), dtype=torch.float32, device=dev)
        out_v = torch.empty((B, N), dtype=torch.float32, device=dev)
        check(_lib.load().bnn_moments_forward(ptr(am), ptr(av), K, ptr(w), ptr(z_w), ptr(b), ptr(z_b), ptr(out_m), ptr(out_v),
                                              B, N, K, code, 0, stream_ptr(dev)), "bnn_moments_forward")
        ctx.save_for_backward(am, av, w)
        ctx.code, ctx.bias = code, b is not None
        return out_m, out_v

    @staticmethod
    def backward(ctx, g_m, g_v):
        am, av, w = ctx.saved_tensors
        code = ctx.code
        B, K = am.shape
        N = w.shape[0]
        dev = am.device
        lib, st = _lib.load(), stream_ptr(dev)
        g_m, g_v = g_m.contiguous(), g_v.contiguous()
        g_am = g_av = g_w = g_b = None
        zero = torch.zeros_like(w)                  # sigma^2 = 0 for the input gradient, rho = 0 for the weight gradient's chain
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g_am, g_av = torch.empty_like(am), torch.empty_like(av)
            check(lib.bnn_moments_backward_input(ptr(g_m), ptr(g_v), ptr(w), ptr(zero), ptr(am), K, ptr(g_am), ptr(g_av), B, N, K,
                                                 code, 0, st), "bnn_moments_backward_input")
        need_b = ctx.bias and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[2] or need_b:
            g_w, scrap = torch.empty_like(w), torch.empty_like(w)
            zb = sb = None
            if need_b:
                g_b = torch.empty(N, dtype=torch.float32, device=dev)
                zb, sb = torch.zeros_like(g_b), torch.empty_like(g_b)
            check(lib.bnn_moments_backward_weight(ptr(am), ptr(av), K, ptr(g_m), ptr(g_v), ptr(w), ptr(zero), ptr(g_w), ptr(scrap),
                                                  ptr(zb), ptr(g_b), ptr(sb), B, N, K, code, 0, st), "bnn_moments_backward_weight")
        return g_am, g_av, g_w, g_b, None


def moments_convNd(a, mu_w, rho_w, mu_b, rho_b, stride, padding, dilation, groups=1, activation=None, compute="f32", track=False):
    """Mean and variance of a convolution's pre-activation for independent Gaussian weights, from the mean and variance of its
    input, elements independent (bnn_lrt_prepare + bnn_conv3d_moments_forward, csrc/bnn_conv3d.hip; the dimension is the
    weight's, 1-d and 2-d as unit depth / height) -> Moments, fp32 (B, O, *out_spatial):

        m = convNd(a_m, mu_w) + mu_b,    v = convNd(a_m^2, sigma_w^2) + convNd(a_v, mu_w^2 + sigma_w^2) + sigma_b^2

    a: a device tensor (B, C, *spatial) (a deterministic input: the second term is absent) or a Moments.  activation: None,
    'relu' or ('elu', alpha) -- moments_relu / moments_elu in the launch's epilogue (the same bits).  Nothing is drawn, no key is
    touched.  track=False (inference): the result is detached whatever the grad mode.  track=True with grad mode on (training
    without sampling, K19): the result is attached to the graph of `a` and the four posterior tensors; the backward is HIP
    (k_moments_conv3d_bwd; K11's launches for a deterministic input), and an activation runs as its standalone launch behind the
    contraction (one device function: the same bits), because its backward needs the pre-activation.  Raises BnnHipError for a
    call the kernel refuses: no torch fallback."""
    return _moments_convNd("moments_convNd", _GAUSSIAN, a, mu_w, rho_w, mu_b, rho_b, stride, padding, dilation, groups, activation,
                           compute, track)


def _moments_convNd(who, post, a, mu_w, par_w, mu_b, rho_b, stride, padding, dilation, groups, activation, compute, track,
                    threshold=None):
    """moments_convNd / moments_convNd_vd: the input's preparation, the checks and the untracked launch on the planes of
    post.prepare; track (the Gaussian posterior only) hands over to _MomentsConv."""
    mom = _as_moments(a, who)
    _refuse_link(mom, who)
    act, alpha = _moment_activation(activation, who)
    code = _compute_code(compute)
    tracked = _tracking(track)
    keep = (lambda t: t) if tracked else (lambda t: t.detach())
    am = keep(mom.mean).contiguous()
    av = None if mom.var is None else keep(mom.var).contiguous()
    mu_w, par_w = keep(mu_w).contiguous(), keep(par_w).contiguous()
    if mu_b is not None:
        mu_b, rho_b = keep(mu_b).contiguous(), keep(rho_b).contiguous()
    post.check(mu_w, par_w, mu_b, rho_b, conv=True)
    require_cuda_f32(am, "a.mean")
    if av is not None:
        require_cuda_f32(av, "a.var")
    nd = mu_w.dim() - 2
    if nd not in (1, 2, 3) or am.dim() != nd + 2:
        raise BnnHipError("%s: input must be (B, C, ...) with %d spatial axes for a weight of shape %s, got %s"
                          % (who, nd, tuple(mu_w.shape), tuple(am.shape)))
    img, w5, st, pd, dl = _lrt_conv_views(am.shape, mu_w.shape, stride, padding, dilation)
    B = int(am.shape[0])
    sh, out3 = _conv3d_shape((B,) + img, w5, st, pd, dl, groups)
    out_sp = out3[3 - nd:]
    dev = am.device
    if tracked:
        m, v = _MomentsConv.apply(am, av, mu_w, par_w, mu_b, rho_b, sh, (B, sh.O) + out_sp, code)
        if act == 'relu':
            m, v = _MomentsRelu.apply(m, v)
        elif act == 'elu':
            m, v = _MomentsElu.apply(m, v, alpha)
        return Moments(m, v)
    mu_w, s2_w, s2_b = post.prepare(mu_w, par_w, rho_b if mu_b is not None else None, threshold)
    out_m = torch.empty((B, sh.O) + out_sp, dtype=torch.float32, device=dev)
    out_v = torch.empty_like(out_m)
    check(_lib.load().bnn_conv3d_moments_forward(ptr(am), ptr(av), ptr(mu_w), ptr(s2_w), ptr(mu_b), ptr(s2_b), ptr(out_m),
                                                 ptr(out_v), ctypes.byref(sh), code, _ACT_FLAGS[act], alpha, stream_ptr(dev)),
          "bnn_conv3d_moments_forward")
    return Moments(out_m, out_v)


def moments_affine(a, w, b, compute="f32", track=False):
    """A DETERMINISTIC dense layer (torch.nn.Linear behind a Bayesian layer, as in the CIFAR10 example) in a moment pass:
    m = a_m w^T + b, v = a_v (w^2)^T -- exact for independent inputs.  It is bnn_moments_forward with sigma_w^2 = 0 (the planes
    w, 0, fma(w, w, 0)), so K16's tile, bounds and both compute modes apply; no operand launch.  a: a tensor or a Moments
    (*rows, K); w (N, K); b (N) or None -> Moments, fp32 (*rows, N); a deterministic input stays one (var None).  track=False:
    detached.  track=True with grad mode on: attached to `a`, w and b; the backward is K18's two launches (a zero sigma^2 plane
    for the input gradient, a zero rho and a discarded g_rho for the weight gradient); a deterministic input is plain torch."""
    who = "moments_affine"
    mom = _as_moments(a, who)
    _refuse_link(mom, who)
    tracked = _tracking(track)
    keep = (lambda t: t) if tracked else (lambda t: t.detach())
    w = keep(w).contiguous()
    b = None if b is None else keep(b).contiguous()
    if mom.var is None:
        return Moments(torch.nn.functional.linear(keep(mom.mean), w, b), None)
    code = _compute_code(compute)
    N, K = w.shape
    am, av = keep(mom.mean), keep(mom.var)
    if am.dim() < 1 or am.shape[-1] != K:
        raise BnnHipError("%s: input has %s features, weight expects %d" % (who, am.shape[-1] if am.dim() else "no", K))
    lead = tuple(am.shape[:-1])
    am, av = am.reshape(-1, K).contiguous(), av.reshape(-1, K).contiguous()
    for t, n in ((am, "a.mean"), (av, "a.var"), (w, "weight")) + (((b, "bias"),) if b is not None else ()):
        require_cuda_f32(t, n)
    B = am.shape[0]
    if B > 64 * 65535:
        raise BnnHipError("%s: %d rows (at most %d)" % (who, B, 64 * 65535))
    if tracked:
        m, v = _MomentsAffine.apply(am, av, w, b, code)
        return Moments(m.reshape(lead + (N,)), v.reshape(lead + (N,)))
    dev = am.device
    z_w = torch.zeros_like(w)
    z_b = None if b is None else torch.zeros_like(b)
    out_m = torch.empty((B, N), dtype=torch.float32, device=dev)
    out_v = torch.empty((B, N), dtype=torch.float32, device=dev)
    check(_lib.load().bnn_moments_forward(ptr(am), ptr(av), K, ptr(w), ptr(z_w), ptr(b), ptr(z_b), ptr(out_m), ptr(out_v),
                                          B, N, K, code, 0, stream_ptr(dev)), "bnn_moments_forward")
    return Moments(out_m.reshape(lead + (N,)), out_v.reshape(lead + (N,)))


def moments_affine_f64(a, w, b, track=False):
    """moments_affine in float64 torch.  track=True: not detached."""
    mom = _as_moments(a, "moments_affine_f64")
    _refuse_link(mom, "moments_affine_f64")
    f64 = _f64(track)
    m = torch.nn.functional.linear(f64(mom.mean), f64(w), None if b is None else f64(b))
    return Moments(m, None if mom.var is None else f64(mom.var) @ (f64(w) * f64(w)).t())


def moments_elu(mom, alpha=1.0, track=False):
    """ELU of Gaussian activations by moment matching (bnn_moments_elu; the formulas are include/bnn_hip.h's, evaluated in fp64
    on the device and rounded to fp32) -> Moments.  v == 0 gives (elu(m), 0).  A deterministic input (var None) stays one.
    track=True with grad mode on: attached to the graph, the backward is bnn_moments_elu_backward (a deterministic input:
    torch's elu)."""
    mom = _as_moments(mom, "moments_elu")
    _refuse_link(mom, "moments_elu")
    _, alpha = _moment_activation(('elu', alpha), "moments_elu")
    tracked = _tracking(track)
    keep = (lambda t: t) if tracked else (lambda t: t.detach())
    if mom.var is None:
        return Moments(torch.nn.functional.elu(keep(mom.mean), alpha), None)
    m, v = keep(mom.mean).contiguous(), keep(mom.var).contiguous()
    require_cuda_f32(m, "mean")
    require_cuda_f32(v, "var")
    if tracked:
        return Moments(*_MomentsElu.apply(m, v, alpha))
    om, ov = torch.empty_like(m), torch.empty_like(v)
    check(_lib.load().bnn_moments_elu(ptr(m), ptr(v), ptr(om), ptr(ov), m.numel(), alpha, stream_ptr(m.device)), "bnn_moments_elu")
    return Moments(om, ov)


def _elu_terms_f64(m, vs):
    """The terms of the moment-matched ELU's closed form at float64 (m, vs), vs > 0: -> (s, alpha, Phi, Phi_c, phi, E_1, E_2, P1,
    r), r the ReLU's variance bracket; E_k through erfcx where alpha + k s >= 0, so that nothing overflows."""
    s = torch.sqrt(vs)
    al = m / s
    r2 = math.sqrt(2.0)
    cdf, cdc = 0.5 * torch.special.erfc(-al / r2), 0.5 * torch.special.erfc(al / r2)
    pdf = torch.exp(-0.5 * al * al) / math.sqrt(2.0 * math.pi)

    def e_k(k):
        t = al + k * s
        up = 0.5 * torch.exp(-0.5 * al * al) * torch.special.erfcx(t.clamp_min(0) / r2)
        lo = torch.exp((k * m + 0.5 * k * k * vs).clamp_max(0)) * 0.5 * torch.special.erfc(t.clamp_max(0) / r2)
        return torch.where(t >= 0, up, lo)

    e1, e2 = e_k(1.0), e_k(2.0)
    p1 = s * (al * cdf + pdf)
    return s, al, cdf, cdc, pdf, e1, e2, p1, cdf + al * al * cdf * cdc + al * pdf * (cdc - cdf) - pdf * pdf


def moments_elu_f64(mom, alpha=1.0, track=False):
    """moments_elu in float64 torch: the closed form of include/bnn_hip.h (the variance as the ReLU part's, the negative part's
    and their cross term; E_k through erfcx where alpha + k s >= 0, so that nothing overflows).  track=True: not detached (plain
    torch autograd; at v == 0 the gradient is the stated convention of moments_elu_backward_f64)."""
    mom = _as_moments(mom, "moments_elu_f64")
    a = float(alpha)
    f64 = _f64(track)
    m = f64(mom.mean)
    if mom.var is None:
        return Moments(torch.nn.functional.elu(m, a), None)
    v = f64(mom.var)
    pos = v > 0
    vs = torch.where(pos, v, torch.ones_like(v))
    s, al, cdf, cdc, pdf, e1, e2, p1, r = _elu_terms_f64(m, vs)
    n1, n2 = e1 - cdc, e2 - 2.0 * e1 + cdc
    mean = p1 + a * n1
    var = (vs * r + a * a * (n2 - n1 * n1) - 2.0 * a * p1 * n1).clamp_min(0)
    if _tracking(track):
        # the same values; v == 0 takes the limits: d mean'/d v = a exp(m) [m < 0] / 2, d var'/d v = elu'(m)^2, elu'(0) = 1
        md = m.detach()
        d = torch.where(md < 0, a * torch.exp(md.clamp_max(0)), torch.ones_like(md))
        elu = torch.where(m < 0, a * torch.expm1(m.clamp_max(0)), m)
        return Moments(torch.where(pos, mean, elu + v * torch.where(md < 0, 0.5 * d, torch.zeros_like(d))),
                       torch.where(pos, var, v * d * d))
    return Moments(torch.where(pos, mean, torch.nn.functional.elu(m, a)), torch.where(pos, var, torch.zeros_like(v)))


def moments_elu_backward_f64(mom, g_mean, g_var, alpha=1.0):
    """The backward of moments_elu in float64 torch, as a formula: (g_m, g_v) at the pre-activation `mom` from the gradients of
    the two outputs.  In include/bnn_hip.h's symbols (a = alpha of the ELU, al = m / s, mean' the forward's mean):

        d mean'/d m = Phi + a E_1                        d mean'/d v = (a E_1 + (1 - a) phi / s) / 2
        d var'/d m  = 2 P1 + 2 a^2 (E_2 - E_1) - 2 mean' (Phi + a E_1)
        d var'/d v  = Phi + a^2 (2 E_2 - E_1) - mean' (a E_1 + (1 - a) phi / s)

    (d_m E f = E f', d_v E f = E f'' / 2; a = 0: moments_relu_backward_f64's).  Where the forward clamped var' to 0 the g_var
    terms are 0; v == 0 takes the limits, g_m = g_mean elu'(m), g_v = g_var elu'(m)^2 + g_mean a exp(m) [m < 0] / 2 with
    elu'(0) = 1; a deterministic input (var None) is plain ELU: (g_mean elu'(m), None)."""
    mom = _as_moments(mom, "moments_elu_backward_f64")
    a = float(alpha)
    f64 = lambda t: t.detach().to(torch.float64)         # noqa: E731
    m, g_mean = f64(mom.mean), f64(g_mean)
    neg = m < 0
    d = torch.where(neg, a * torch.exp(m.clamp_max(0)), torch.ones_like(m))
    if mom.var is None:
        return g_mean * d, None
    v, g_var = f64(mom.var), f64(g_var)
    pos = v > 0
    vs = torch.where(pos, v, torch.ones_like(v))
    s, al, cdf, cdc, pdf, e1, e2, p1, r = _elu_terms_f64(m, vs)
    n1, n2 = e1 - cdc, e2 - 2.0 * e1 + cdc
    mean = p1 + a * n1
    gv = torch.where(vs * r + a * a * (n2 - n1 * n1) - 2.0 * a * p1 * n1 < 0, torch.zeros_like(g_var), g_var)
    dm, dv = cdf + a * e1, a * e1 + (1.0 - a) * pdf / s
    g_m = g_mean * dm + gv * (2.0 * p1 + 2.0 * a * a * (e2 - e1) - 2.0 * mean * dm)
    g_v = g_mean * (0.5 * dv) + gv * (cdf + a * a * (2.0 * e2 - e1) - mean * dv)
    zero = torch.zeros_like(m)
    return torch.where(pos, g_m, g_mean * d), torch.where(pos, g_v, g_var * d * d + g_mean * torch.where(neg, 0.5 * d, zero))


def moments_convNd_f64(a, mu_w, rho_w, mu_b, rho_b, stride, padding, dilation, groups=1, activation=None, track=False):
    """moments_convNd in float64 torch (two / three torch.nn.functional.convNd calls on the CPU; sigma = 1e-10 + softplus(rho))
    -> Moments of float64 tensors.  track=True: not detached (torch autograd through the convolutions and the activation)."""
    f64 = _f64(track)
    return _moments_convNd_planes_f64("moments_convNd_f64", a, f64(mu_w), _sigma2_f64(f64(rho_w)), mu_b, rho_b, stride, padding,
                                      dilation, groups, activation, track)


def _moments_convNd_planes_f64(who, a, mu, s2, mu_b, rho_b, stride, padding, dilation, groups, activation, track):
    """The conv moment layer in float64 on the weight's mean and variance planes (float64 already); the bias is Gaussian."""
    mom = _as_moments(a, who)
    _refuse_link(mom, who)
    act, alpha = _moment_activation(activation, who)
    f64 = _f64(track)
    nd = mu.dim() - 2
    if nd not in (1, 2, 3):
        raise BnnHipError("%s: weight must be (O, C / groups, *kernel) with 1, 2 or 3 kernel axes, got %s" % (who, tuple(mu.shape)))
    conv = (torch.nn.functional.conv1d, torch.nn.functional.conv2d, torch.nn.functional.conv3d)[nd - 1]
    geo = (tuple(stride), tuple(padding), tuple(dilation), int(groups))
    am = f64(mom.mean)
    m = conv(am, mu, None if mu_b is None else f64(mu_b), *geo)
    v = conv(am * am, s2, None if mu_b is None else _sigma2_f64(f64(rho_b)), *geo)
    if mom.var is not None:
        v = v + conv(f64(mom.var), mu * mu + s2, None, *geo)
    out = Moments(m, v)
    if act == 'relu':
        return moments_relu_f64(out, track)
    return moments_elu_f64(out, alpha, track) if act == 'elu' else out


def moments_convNd_vd(a, theta, log_sigma2, mu_b, rho_b, stride, padding, dilation, groups=1, activation=None, compute="f32",
                      threshold=None):
    """moments_convNd for a VariationalDropoutConvNd (K24): the same launch (bnn_conv3d_moments_forward, the activation in its
    epilogue) on the planes of bnn_vd_prepare -- theta and exp(log_sigma2), masked by `threshold` as convNd_vd masks them ->
    Moments, fp32 (B, O, *out_spatial), detached.  Inference only: there is no moment backward for this posterior."""
    return _moments_convNd("moments_convNd_vd", _LOG_SIGMA2, a, theta, log_sigma2, mu_b, rho_b, stride, padding, dilation, groups,
                           activation, compute, False, threshold)


def moments_convNd_vd_f64(a, theta, log_sigma2, mu_b, rho_b, stride, padding, dilation, groups=1, activation=None, threshold=None):
    """moments_convNd_vd in float64 torch (the CPU path and the tests' reference) -> Moments of float64 tensors, detached."""
    th, s2 = _vd_planes_f64(theta, log_sigma2, threshold)
    return _moments_convNd_planes_f64("moments_convNd_vd_f64", a, th, s2, mu_b, rho_b, stride, padding, dilation, groups, activation,
                                      False)


# --------------------------------------------------------------------------- K22: MC dropout (and deterministic convs) in a moment pass
_ACT_FLAGS = {None: 0, 'relu': _lib.FLAG_RELU, 'elu': _lib.FLAG_ELU}


class _MomentsDropout(torch.autograd.Function):
    """bnn_moments_dropout out of place with bnn_moments_dropout_backward behind it; m fp32, contiguous; v the same or None (a
    deterministic input: no gradient of a variance)."""

    @staticmethod
    def forward(ctx, m, v, p, flag, alpha):
        om, ov = torch.empty_like(m), torch.empty_like(m)
        check(_lib.load().bnn_moments_dropout(ptr(m), ptr(v), ptr(om), ptr(ov), m.numel(), p, flag, alpha, stream_ptr(m.device)),
              "bnn_moments_dropout")
        ctx.save_for_backward(m, v)
        ctx.p, ctx.flag, ctx.alpha = p, flag, alpha
        return om, ov

    @staticmethod
    def backward(ctx, g_om, g_ov):
        m, v = ctx.saved_tensors
        g_om, g_ov = g_om.contiguous(), g_ov.contiguous()
        g_m = torch.empty_like(m)
        g_v = None if v is None else torch.empty_like(v)
        check(_lib.load().bnn_moments_dropout_backward(ptr(m), ptr(v), ptr(g_om), ptr(g_ov), ptr(g_m), ptr(g_v), m.numel(), ctx.p,
                                                       ctx.flag, ctx.alpha, stream_ptr(m.device)), "bnn_moments_dropout_backward")
        return g_m, g_v, None, None, None


def moments_dropout(mom, p, activation=None, track=False):
    """An MC-dropout mask behind Gaussian activations, pushed through the activation that follows in ONE step
    (bnn_moments_dropout) -> Moments.  For z ~ N(m, v), an independent mask b ~ Bernoulli(q), q = 1 - p, and an activation f with
    f(0) = 0 (activation: None, 'relu' or ('elu', alpha)) the layer hands on f(b z / q) = b f(z / q); with (M, V) the moments of f at
    N(m / q, v / q^2) (moments_relu / moments_elu there):

        mean' = q M,    var' = q V + q p M^2

    exact for a Gaussian z and for a deterministic one: a dropped unit is a spike at zero, not a Gaussian, so the mask is NOT
    moment-matched in front of the activation.  A deterministic input (var None) comes out with the variance q p f(m / q)^2.
    p == 0 is the activation alone (its bits), p == 1 gives zeros.  track=True with grad mode on: attached to the graph, the
    backward is bnn_moments_dropout_backward."""
    who = "moments_dropout"
    mom = _as_moments(mom, who)
    _refuse_link(mom, who)
    act, alpha = _moment_activation(activation, who)
    check_drop_prob(p)
    p = float(p)
    tracked = _tracking(track)
    keep = (lambda t: t) if tracked else (lambda t: t.detach())
    m = keep(mom.mean).contiguous()
    v = None if mom.var is None else keep(mom.var).contiguous()
    require_cuda_f32(m, "mean")
    if v is not None:
        require_cuda_f32(v, "var")
    if tracked:
        return Moments(*_MomentsDropout.apply(m, v, p, _ACT_FLAGS[act], alpha))
    om, ov = torch.empty_like(m), torch.empty_like(m)
    check(_lib.load().bnn_moments_dropout(ptr(m), ptr(v), ptr(om), ptr(ov), m.numel(), p, _ACT_FLAGS[act], alpha, stream_ptr(m.device)),
          "bnn_moments_dropout")
    return Moments(om, ov)


def _act_f64(mom, act, alpha, track):
    if act == 'relu':
        return moments_relu_f64(mom, track)
    return moments_elu_f64(mom, alpha, track) if act == 'elu' else mom


def moments_dropout_f64(mom, p, activation=None, track=False):
    """moments_dropout in float64 torch: moments_relu_f64 / moments_elu_f64 at (m / q, v / q^2), then mean' = q M,
    var' = q V + q p M^2 -> Moments of float64 tensors; the result always carries a variance.  track=True: not detached (plain torch
    autograd through the activation's closed form, with its conventions at v == 0)."""
    who = "moments_dropout_f64"
    mom = _as_moments(mom, who)
    _refuse_link(mom, who)
    act, alpha = _moment_activation(activation, who)
    check_drop_prob(p)
    p = float(p)
    q = 1.0 - p
    f64 = _f64(track)
    m = f64(mom.mean)
    v = None if mom.var is None else f64(mom.var)
    never = torch.zeros_like(m, dtype=torch.bool)            # torch.where(never, t, 0): zeros that stay in t's graph, zero gradients
    if p == 0.0:
        out = _act_f64(Moments(m, v), act, alpha, track)
        return Moments(out.mean, torch.where(never, out.mean, torch.zeros_like(m)) if out.var is None else out.var)
    if p == 1.0:
        return Moments(torch.where(never, m, torch.zeros_like(m)), torch.where(never, m if v is None else v, torch.zeros_like(m)))
    inner = _act_f64(Moments(m / q, None if v is None else v / (q * q)), act, alpha, track)
    M = inner.mean
    var = q * p * M * M
    return Moments(q * M, var if inner.var is None else q * inner.var + var)


def moments_dropout_backward_f64(mom, g_mean, g_var, p, activation=None):
    """The backward of moments_dropout in float64 torch, as a formula: (g_m, g_v) at the pre-dropout `mom` from the gradients of the
    two outputs.  With M the activation's mean at (m / q, v / q^2):

        gM = q g_mean + 2 q p M g_var,    gV = q g_var

    through moments_relu_backward_f64 / moments_elu_backward_f64 there (the identity passes them) to (g_mi, g_vi);
    g_m = g_mi / q, g_v = g_vi / q^2.  p == 1 gives zeros; a deterministic input (var None) gives (g_m, None)."""
    who = "moments_dropout_backward_f64"
    mom = _as_moments(mom, who)
    act, alpha = _moment_activation(activation, who)
    check_drop_prob(p)
    p = float(p)
    q = 1.0 - p
    f64 = lambda t: t.detach().to(torch.float64)         # noqa: E731
    m, g_mean, g_var = f64(mom.mean), f64(g_mean), f64(g_var)
    v = None if mom.var is None else f64(mom.var)
    if p == 1.0:
        return torch.zeros_like(m), None if v is None else torch.zeros_like(m)
    inner = Moments(m / q, None if v is None else v / (q * q))
    M = _act_f64(inner, act, alpha, False).mean
    gM, gV = q * g_mean + 2.0 * q * p * M * g_var, q * g_var
    if act == 'relu':
        g_mi, g_vi = moments_relu_backward_f64(inner, gM, gV)
    elif act == 'elu':
        g_mi, g_vi = moments_elu_backward_f64(inner, gM, gV, alpha)
    else:
        g_mi, g_vi = gM, gV
    return g_mi / q, None if v is None else g_vi / (q * q)


class _MomentsConvAffine(torch.autograd.Function):
    """ops.moments_conv_affine on moments that carry a variance, with K19's backward launches behind it, as _MomentsAffine has
    K18's: the input gradient with the zero sigma^2 plane, the weight gradient with a zero rho whose g_rho_w is discarded (the bias
    sum rides along).  am, av (B, C, *spatial), w (O, C / groups, *kernel), b (O) or None, all fp32 and contiguous."""

    @staticmethod
    def forward(ctx, am, av, w, b, sh, out_shape, code):
        dev = am.device
        z_w = torch.zeros_like(w)
        z_b = None if b is None else torch.zeros_like(b)
        out_m = torch.empty(out_shape, dtype=torch.float32, device=dev)
        out_v = torch.empty_like(out_m)
        check(_lib.load().bnn_conv3d_moments_forward(ptr(am), ptr(av), ptr(w), ptr(z_w), ptr(b), ptr(z_b), ptr(out_m), ptr(out_v),
                                                     ctypes.byref(sh), code, 0, 0.0, stream_ptr(dev)), "bnn_conv3d_moments_forward")
        ctx.save_for_backward(am, av, w)
        ctx.code, ctx.sh, ctx.bias = code, sh, b is not None
        return out_m, out_v

    @staticmethod
    def backward(ctx, g_m, g_v):
        am, av, w = ctx.saved_tensors
        code, sh = ctx.code, ctx.sh
        dev = am.device
        lib, st = _lib.load(), stream_ptr(dev)
        g_m, g_v = g_m.contiguous(), g_v.contiguous()
        g_am = g_av = g_w = g_b = None
        zero = torch.zeros_like(w)                  # sigma^2 = 0 for the input gradient, rho = 0 for the weight gradient's chain
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g_am, g_av = torch.empty_like(am), torch.empty_like(av)
            check(lib.bnn_conv3d_moments_backward_input(ptr(g_m), ptr(g_v), ptr(w), ptr(zero), ptr(am), ptr(g_am), ptr(g_av),
                                                        ctypes.byref(sh), code, st), "bnn_conv3d_moments_backward_input")
        need_b = ctx.bias and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[2] or need_b:
            g_w, scrap = torch.empty_like(w), torch.empty_like(w)
            zb = sb = None
            if need_b:
                g_b = torch.empty(w.shape[0], dtype=torch.float32, device=dev)
                zb, sb = torch.zeros_like(g_b), torch.empty_like(g_b)
            nb = lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(sh))
            ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
            check(lib.bnn_conv3d_moments_backward_weight(ptr(am), ptr(av), ptr(g_m), ptr(g_v), ptr(w), ptr(zero), ptr(g_w), ptr(scrap),
                                                         ptr(zb), ptr(g_b), ptr(sb), ctypes.byref(sh), code, ptr(ws), nb, st),
                  "bnn_conv3d_moments_backward_weight")
        return g_am, g_av, g_w, g_b, None, None, None


def _plain_conv(nd):
    return (torch.nn.functional.conv1d, torch.nn.functional.conv2d, torch.nn.functional.conv3d)[nd - 1]


def moments_conv_affine(a, w, b, stride, padding, dilation, groups=1, compute="f32", track=False):
    """A DETERMINISTIC convolution (the torch conv inside an MCDropoutConv layer) in a moment pass: m = convNd(a_m, w) + b,
    v = convNd(a_v, w^2) -- exact for independent inputs.  It is bnn_conv3d_moments_forward with sigma_w^2 = 0, exactly as
    moments_affine is bnn_moments_forward with it, so K17's tile, bounds and both compute modes apply.  a: a tensor or a Moments
    (B, C, *spatial); w (O, C / groups, *kernel); b (O) or None -> Moments, fp32; a deterministic input stays one (var None, the
    torch convolution).  track=False: detached.  track=True with grad mode on: attached to `a`, w and b; the backward is K19's
    launches (a zero sigma^2 plane for the input gradient, a zero rho and a discarded g_rho for the weight gradient)."""
    who = "moments_conv_affine"
    mom = _as_moments(a, who)
    _refuse_link(mom, who)
    tracked = _tracking(track)
    keep = (lambda t: t) if tracked else (lambda t: t.detach())
    w = keep(w).contiguous()
    b = None if b is None else keep(b).contiguous()
    nd = w.dim() - 2
    if nd not in (1, 2, 3) or mom.mean.dim() != nd + 2:
        raise BnnHipError("%s: input must be (B, C, ...) with %d spatial axes for a weight of shape %s, got %s"
                          % (who, nd, tuple(w.shape), tuple(mom.mean.shape)))
    if mom.var is None:
        return Moments(_plain_conv(nd)(keep(mom.mean), w, b, tuple(stride), tuple(padding), tuple(dilation), int(groups)), None)
    code = _compute_code(compute)
    am, av = keep(mom.mean).contiguous(), keep(mom.var).contiguous()
    for t, n in ((am, "a.mean"), (av, "a.var"), (w, "weight")) + (((b, "bias"),) if b is not None else ()):
        require_cuda_f32(t, n)
    img, w5, st, pd, dl = _lrt_conv_views(am.shape, w.shape, stride, padding, dilation)
    B = int(am.shape[0])
    sh, out3 = _conv3d_shape((B,) + img, w5, st, pd, dl, groups)
    out_shape = (B, sh.O) + out3[3 - nd:]
    if tracked:
        return Moments(*_MomentsConvAffine.apply(am, av, w, b, sh, out_shape, code))
    dev = am.device
    z_w = torch.zeros_like(w)
    z_b = None if b is None else torch.zeros_like(b)
    out_m = torch.empty(out_shape, dtype=torch.float32, device=dev)
    out_v = torch.empty_like(out_m)
    check(_lib.load().bnn_conv3d_moments_forward(ptr(am), ptr(av), ptr(w), ptr(z_w), ptr(b), ptr(z_b), ptr(out_m), ptr(out_v),
                                                 ctypes.byref(sh), code, 0, 0.0, stream_ptr(dev)), "bnn_conv3d_moments_forward")
    return Moments(out_m, out_v)


def moments_conv_affine_f64(a, w, b, stride, padding, dilation, groups=1, track=False):
    """moments_conv_affine in float64 torch.  track=True: not detached."""
    who = "moments_conv_affine_f64"
    mom = _as_moments(a, who)
    _refuse_link(mom, who)
    f64 = _f64(track)
    nd = w.dim() - 2
    if nd not in (1, 2, 3):
        raise BnnHipError("%s: weight must be (O, C / groups, *kernel) with 1, 2 or 3 kernel axes, got %s" % (who, tuple(w.shape)))
    geo = (tuple(stride), tuple(padding), tuple(dilation), int(groups))
    w64 = f64(w)
    m = _plain_conv(nd)(f64(mom.mean), w64, None if b is None else f64(b), *geo)
    return Moments(m, None if mom.var is None else _plain_conv(nd)(f64(mom.var), w64 * w64, None, *geo))


# --------------------------------------------------------------------------- K20: moments through pooling and eval-mode BatchNorm
def _pool_geometry(who, mom, op, kernel_size, stride, padding, dilation):
    """The per-axis geometry of one pooling call on (B, C, *spatial) moments, 1 to 3 spatial axes -> (nd, kernel, stride,
    padding, dilation, out_spatial); stride None = the kernel (torch's default); the output extents by torch's floor rule.
    BnnHipError for what bnn_moments_pool3d_forward refuses (the same conditions, checked here so that the CPU route refuses
    them too)."""
    if op not in ('max', 'avg'):
        raise ValueError("%s: op must be 'max' or 'avg', got %r" % (who, op))
    nd = mom.dim() - 2
    if nd not in (1, 2, 3):
        raise BnnHipError("%s: the moments must be (B, C, *spatial) with 1, 2 or 3 spatial axes, got %s" % (who, tuple(mom.shape)))

    def axes(val, name):
        t = tuple(int(x) for x in val) if isinstance(val, (tuple, list)) else (int(val),) * nd
        if len(t) == 1 and nd > 1:
            t = t * nd
        if len(t) != nd:
            raise BnnHipError("%s: %s has %d entries for %d spatial axes" % (who, name, len(t), nd))
        return t

    k = axes(kernel_size, "kernel_size")
    s = k if stride is None else axes(stride, "stride")
    p, d = axes(padding, "padding"), axes(dilation, "dilation")
    if min(mom.shape) < 1 or min(k) < 1 or min(s) < 1 or min(d) < 1 or min(p) < 0:
        raise BnnHipError("%s: an extent below 1 (shape %s, kernel %s, stride %s, padding %s, dilation %s)"
                          % (who, tuple(mom.shape), k, s, p, d))
    if any(2 * pi > ki for pi, ki in zip(p, k)):
        raise BnnHipError("%s: padding %s above half the kernel %s" % (who, p, k))
    if math.prod(k) > _lib.POOL_WINDOW_CAP:
        raise BnnHipError("%s: a window of %d elements (at most %d)" % (who, math.prod(k), _lib.POOL_WINDOW_CAP))
    out = tuple((n + 2 * pi - di * (ki - 1) - 1) // si + 1 for n, ki, si, pi, di in zip(mom.shape[2:], k, s, p, d))
    if min(out) < 1:
        raise BnnHipError("%s: the window %s (dilation %s) is larger than the padded input %s" % (who, k, d, tuple(mom.shape[2:])))
    for n, o, ki, si, pi, di in zip(mom.shape[2:], out, k, s, p, d):
        for oi in set(range(min(o, pi + 1))) | set(range(max(0, o - pi - 1), o)):
            if not any(0 <= oi * si - pi + j * di < n for j in range(ki)):
                raise BnnHipError("%s: a window lies in the padding alone (kernel %s, padding %s, dilation %s)" % (who, k, p, d))
    return nd, k, s, p, d, out


def _pool3d_shape(shape, k, s, p, d):
    """bnn_pool3d_shape_t of a (B, C, *spatial) call: 1-d and 2-d pooling as unit depth / height."""
    pad3 = lambda t, one: (one,) * (3 - len(t)) + tuple(t)          # noqa: E731
    D, H, W = pad3(tuple(shape[2:]), 1)
    (KD, KH, KW), (sd, sh, sw), (pd, ph, pw), (dd, dh, dw) = pad3(k, 1), pad3(s, 1), pad3(p, 0), pad3(d, 1)
    return _lib.Pool3dShape(B=int(shape[0]), C=int(shape[1]), D=D, H=H, W=W, KD=KD, KH=KH, KW=KW, stride_d=sd, stride_h=sh,
                            stride_w=sw, pad_d=pd, pad_h=ph, pad_w=pw, dil_d=dd, dil_h=dh, dil_w=dw)


class _MomentsPool(torch.autograd.Function):
    """bnn_moments_pool3d_forward with bnn_moments_pool3d_backward behind it (the backward folds the windows again from the
    saved inputs); m, v fp32, contiguous, (B, C, *spatial)."""

    @staticmethod
    def forward(ctx, m, v, sh, out_shape, code, flags):
        om = torch.empty(out_shape, dtype=torch.float32, device=m.device)
        ov = torch.empty_like(om)
        check(_lib.load().bnn_moments_pool3d_forward(ptr(m), ptr(v), ptr(om), ptr(ov), ctypes.byref(sh), code, flags,
                                                     stream_ptr(m.device)), "bnn_moments_pool3d_forward")
        ctx.save_for_backward(m, v)
        ctx.sh, ctx.code, ctx.flags = sh, code, flags
        return om, ov

    @staticmethod
    def backward(ctx, g_om, g_ov):
        m, v = ctx.saved_tensors
        g_om, g_ov = g_om.contiguous(), g_ov.contiguous()
        g_m, g_v = torch.empty_like(m), torch.empty_like(v)
        check(_lib.load().bnn_moments_pool3d_backward(ptr(m), ptr(v), ptr(g_om), ptr(g_ov), ptr(g_m), ptr(g_v), ctypes.byref(ctx.sh),
                                                      ctx.code, ctx.flags, stream_ptr(m.device)), "bnn_moments_pool3d_backward")
        return g_m, g_v, None, None, None, None


def _plain_pool(mean, op, nd, k, s, p, d, count_include_pad):
    """A deterministic input (var None) stays one: torch's own pooling of the mean."""
    if op == 'max':
        return (torch.nn.functional.max_pool1d, torch.nn.functional.max_pool2d, torch.nn.functional.max_pool3d)[nd - 1](mean, k, s, p, d)
    if any(di != 1 for di in d):
        raise BnnHipError("moments_pool: torch's average pooling has no dilation (deterministic input)")
    return (torch.nn.functional.avg_pool1d, torch.nn.functional.avg_pool2d, torch.nn.functional.avg_pool3d)[nd - 1](
        mean, k, s, p, False, count_include_pad)


def moments_pool(mom, op, kernel_size, stride=None, padding=0, dilation=1, count_include_pad=True, track=False):
    """Max or average pooling of Gaussian activations (bnn_moments_pool3d_forward, csrc/bnn_moments_pool.hip) -> Moments, fp32
    (B, C, *out_spatial); mom (B, C, *spatial) with 1 to 3 spatial axes; op 'max' or 'avg'; kernel_size, stride (None: the
    kernel), padding, dilation per axis or one number.
      'max': the window is folded pairwise with the moment-matched maximum of two Gaussians (Clark 1961; include/bnn_hip.h has the
        formulas), offsets ascending in (depth, height, width), padded positions skipped: exact for a window of two, moment
        matching of the running maximum beyond.  theta^2 == 0 is the plain maximum.
      'avg': mean' = sum m / n, var' = sum v / n^2 over the valid positions, n the window size (count_include_pad) or the valid
        count: exact for independent elements.
    A deterministic input (var None) stays one (torch's pooling of the mean).  track=True with grad mode on: attached to the
    graph, the backward is bnn_moments_pool3d_backward -- bit-reproducible for windows that do not overlap, fp32 atomics (an
    order-dependent sum) for overlapping ones."""
    who = "moments_pool"
    mom = _as_moments(mom, who)
    _refuse_link(mom, who)
    nd, k, s, p, d, out_sp = _pool_geometry(who, mom, op, kernel_size, stride, padding, dilation)
    tracked = _tracking(track)
    keep = (lambda t: t) if tracked else (lambda t: t.detach())
    if mom.var is None:
        return Moments(_plain_pool(keep(mom.mean), op, nd, k, s, p, d, bool(count_include_pad)), None)
    m, v = keep(mom.mean).contiguous(), keep(mom.var).contiguous()
    require_cuda_f32(m, "mean")
    require_cuda_f32(v, "var")
    out_shape = tuple(m.shape[:2]) + out_sp
    if max(m.numel(), math.prod(out_shape)) >= 1 << 32:
        raise BnnHipError("%s: %d elements: the element index is 32 bits wide" % (who, m.numel()))
    sh = _pool3d_shape(m.shape, k, s, p, d)
    code = _lib.POOL_MAX if op == 'max' else _lib.POOL_AVG
    flags = 0 if (op == 'max' or count_include_pad) else _lib.POOL_FLAG_VALID_DIVISOR
    if tracked:
        return Moments(*_MomentsPool.apply(m, v, sh, out_shape, code, flags))
    om = torch.empty(out_shape, dtype=torch.float32, device=m.device)
    ov = torch.empty_like(om)
    check(_lib.load().bnn_moments_pool3d_forward(ptr(m), ptr(v), ptr(om), ptr(ov), ctypes.byref(sh), code, flags, stream_ptr(m.device)),
          "bnn_moments_pool3d_forward")
    return Moments(om, ov)


def _max_pair_f64(m1, v1, m2, v2):
    """The moment-matched maximum of two independent Gaussians in float64 torch (include/bnn_hip.h, K20); theta^2 == 0: the
    plain maximum, the first operand on a tie (torch.where, so that autograd sends both gradients to the element taken)."""
    th2 = v1 + v2
    plain = ~(th2 > 0)
    ths = torch.where(plain, torch.ones_like(th2), th2)
    th = torch.sqrt(ths)
    d = m1 - m2
    al = d / th
    r2 = math.sqrt(2.0)
    cdf, cdc = 0.5 * torch.special.erfc(-al / r2), 0.5 * torch.special.erfc(al / r2)
    pdf = torch.exp(-0.5 * al * al) / math.sqrt(2.0 * math.pi)
    mean = m1 * cdf + m2 * cdc + th * pdf
    var = (v1 * cdf + v2 * cdc + d * d * cdf * cdc + d * th * pdf * (cdc - cdf) - ths * pdf * pdf).clamp_min(0)
    second = m2 > m1
    return torch.where(plain, torch.where(second, m2, m1), mean), torch.where(plain, torch.where(second, v2, v1), var)


def moments_pool_f64(mom, op, kernel_size, stride=None, padding=0, dilation=1, count_include_pad=True, track=False):
    """moments_pool in float64 torch -- the CPU route and the tests' reference: the same fold in the same order, one strided view
    of the padded planes per window offset.  track=True: not detached (plain torch autograd)."""
    who = "moments_pool_f64"
    mom = _as_moments(mom, who)
    _refuse_link(mom, who)
    nd, k, s, p, d, out_sp = _pool_geometry(who, mom, op, kernel_size, stride, padding, dilation)
    f64 = _f64(track)
    if mom.var is None:
        return Moments(_plain_pool(f64(mom.mean), op, nd, k, s, p, d, bool(count_include_pad)), None)
    ok = torch.ones(tuple(mom.shape[2:]), dtype=torch.bool, device=mom.mean.device)
    geo = (k, s, p, d, out_sp)
    return _pool_fold_f64(_pool_windows(f64(mom.mean), *geo), _pool_windows(f64(mom.var), *geo), _pool_windows(ok, *geo), op,
                          float(math.prod(k)) if count_include_pad else None)


def _pool_windows(t, k, s, p, d, out_sp):
    """The windows of a pooling call, one strided view of the zero-padded t (..., *spatial) per window offset, offsets ascending
    in row-major order: entry j holds, for every output position, the element its window has at offset j."""
    return _pool_windows_of_padded(torch.nn.functional.pad(t, [q for pi in reversed(p) for q in (pi, pi)]), k, s, p, d, out_sp)


def _pool_windows_of_padded(pt, k, s, p, d, out_sp):
    """_pool_windows of a tensor that is padded already."""
    return [pt[(Ellipsis,) + tuple(slice(o * di, o * di + si * (n - 1) + 1, si) for o, di, si, n in zip(off, d, s, out_sp))]
            for off in itertools.product(*[range(ki) for ki in k])]


def _pool_fold_f64(ms, vs, valids, op, divisor):
    """The fold of moments_pool_f64 over the per-offset views of _pool_windows (means, variances, validity masks) -> Moments;
    divisor: the average's n, None = the valid count."""
    rm = rv = started = None
    count = 0.0
    for xm, xv, valid in zip(ms, vs, valids):
        if op == 'avg':
            rm, rv = (xm, xv) if rm is None else (rm + xm, rv + xv)            # (the padding holds zeros)
            count = count + valid
        elif rm is None:
            rm, rv, started = xm, xv, valid
        else:
            nm, nv = _max_pair_f64(rm, rv, xm, xv)
            rm = torch.where(valid, torch.where(started, nm, xm), rm)
            rv = torch.where(valid, torch.where(started, nv, xv), rv)
            started = started | valid
    if op == 'avg':
        n = count if divisor is None else divisor
        return Moments(rm / n, rv / (n * n))
    return Moments(rm, rv)


def _batchnorm_operands(bn, who):
    """(gamma, beta, running_mean, running_var, eps) of an eval-mode BatchNorm module, or the five given as a tuple."""
    if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
        if bn.training:
            raise BnnHipError("%s: %s is in training mode: the batch statistics of a random activation are not part of the "
                              "moment recursion (call .eval())" % (who, type(bn).__name__))
        if bn.running_mean is None or bn.running_var is None:
            raise BnnHipError("%s: %s has no running statistics (track_running_stats=False)" % (who, type(bn).__name__))
        return bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps)
    if isinstance(bn, (tuple, list)) and len(bn) == 5:
        return tuple(bn[:4]) + (float(bn[4]),)
    raise TypeError("%s: expected a BatchNorm module or (gamma, beta, running_mean, running_var, eps), got %s" % (who, type(bn).__name__))


def moments_batchnorm(mom, bn):
    """Eval-mode BatchNorm of Gaussian activations (bnn_moments_batchnorm) -> Moments, fp32: per channel (axis 1)
    a = gamma / sqrt(running_var + eps), m' = a (m - running_mean) + beta, v' = a^2 v.  bn: a torch BatchNorm module in eval mode
    with running statistics, or (gamma, beta, running_mean, running_var, eps) with gamma / beta None for affine=False.  Forward
    only (detached).  A deterministic input (var None) stays one."""
    who = "moments_batchnorm"
    mom = _as_moments(mom, who)
    _refuse_link(mom, who)
    gamma, beta, rmean, rvar, eps = _batchnorm_operands(bn, who)
    if mom.dim() < 2 or mom.shape[1] != rmean.numel():
        raise BnnHipError("%s: moments %s for %d channels" % (who, tuple(mom.shape), rmean.numel()))
    if not (0.0 <= eps < float("inf")):
        raise BnnHipError("%s: eps must be finite and >= 0, got %r" % (who, eps))
    if mom.var is None:
        return Moments(torch.nn.functional.batch_norm(mom.mean.detach(), rmean, rvar, gamma, beta, False, 0.0, eps).detach(), None)
    m, v = mom.mean.detach().contiguous(), mom.var.detach().contiguous()
    require_cuda_f32(m, "mean")
    require_cuda_f32(v, "var")
    par = [None if t is None else t.detach().contiguous() for t in (gamma, beta, rmean, rvar)]
    for t, name in zip(par, ("gamma", "beta", "running_mean", "running_var")):
        if t is not None:
            require_cuda_f32(t, name)
    if m.numel() >= 1 << 32:
        raise BnnHipError("%s: %d elements: the element index is 32 bits wide" % (who, m.numel()))
    om, ov = torch.empty_like(m), torch.empty_like(v)
    B, C = m.shape[0], m.shape[1]
    if m.numel():
        check(_lib.load().bnn_moments_batchnorm(ptr(m), ptr(v), ptr(par[0]), ptr(par[1]), ptr(par[2]), ptr(par[3]), eps, ptr(om), ptr(ov),
                                                B, C, m.numel() // (B * C), stream_ptr(m.device)), "bnn_moments_batchnorm")
    return Moments(om, ov)


def moments_batchnorm_f64(mom, bn):
    """moments_batchnorm in float64 torch (detached)."""
    who = "moments_batchnorm_f64"
    mom = _as_moments(mom, who)
    _refuse_link(mom, who)
    gamma, beta, rmean, rvar, eps = _batchnorm_operands(bn, who)
    if mom.dim() < 2 or mom.shape[1] != rmean.numel():
        raise BnnHipError("%s: moments %s for %d channels" % (who, tuple(mom.shape), rmean.numel()))
    f64 = lambda t: t.detach().to(torch.float64)          # noqa: E731
    shp = (1, -1) + (1,) * (mom.dim() - 2)
    a = 1.0 / torch.sqrt(f64(rvar) + eps)
    if gamma is not None:
        a = a * f64(gamma)
    a = a.reshape(shp)
    m = a * (f64(mom.mean) - f64(rmean).reshape(shp))
    if beta is not None:
        m = m + f64(beta).reshape(shp)
    return Moments(m, None if mom.var is None else a * a * f64(mom.var))


# --------------------------------------------------------------------------- K21: the head of a moment pass (MVN layer, covariance)
HEAD_COV_MAX_N = 32                     # outputs of a head whose covariance is carried (csrc/bnn_moments_head.hip: kCovMaxN)
MVN_MOMENTS_MAX_K = 4096                # input features of a MultivariateNormalLinear in a moment pass (kHeadMaxK)

# What the covariance of a dense layer's outputs needs beside their variance (include/bnn_hip.h, K21): the input's variance
# a_v (rows, K) or None (a deterministic input), the weights' means E (N, K) and the bias covariance C_b (N, N) or None.
HeadOperands = collections.namedtuple("HeadOperands", ("a_v", "E", "C_b"))


def head_operands(mom_in, E, C_b=None):
    """HeadOperands of a dense layer with weight means E whose input was `mom_in` (a Moments), detached."""
    K = E.shape[-1]
    a_v = None if mom_in.var is None else mom_in.var.detach().reshape(-1, K)
    return HeadOperands(a_v, E.detach(), None if C_b is None else C_b.detach())


def _mvn_check(mu_w, scale_w, mu_b, scale_b, who):
    if mu_w.dim() != 2 or tuple(scale_w.shape) != tuple(mu_w.shape) + (mu_w.shape[1],):
        raise BnnHipError("%s: weight mean %s with scale %s (expected (O, K) and (O, K, K))" % (who, tuple(mu_w.shape), tuple(scale_w.shape)))
    O, K = mu_w.shape
    if (mu_b is None) != (scale_b is None):
        raise BnnHipError("%s: the bias mean and scale come together" % who)
    if mu_b is not None and (tuple(mu_b.shape) != (O,) or tuple(scale_b.shape) != (O, O)):
        raise BnnHipError("%s: bias mean %s with scale %s (expected (%d,) and (%d, %d))" % (who, tuple(mu_b.shape), tuple(scale_b.shape), O, O, O))
    if K > MVN_MOMENTS_MAX_K or (mu_b is not None and O > MVN_MOMENTS_MAX_K):
        raise BnnHipError("%s: %d input features / %d outputs with a bias (at most %d)" % (who, K, O, MVN_MOMENTS_MAX_K))
    return O, K


def mvn_moments_prepare(mu_w, scale_w, mu_b, scale_b):
    """The input-independent part of MultivariateNormalLinear's moments in ONE launch (bnn_mvn_moments_prepare) -> (E_w, G_w, E_b,
    C_b): the weights' means under the layer's uniform-noise sampler, E_w^2 + their variances, the bias mean and the bias
    covariance (None, None without a bias).  Detached; the formulas are moments_mvn_linear's."""
    who = "mvn_moments_prepare"
    O, K = _mvn_check(mu_w, scale_w, mu_b, scale_b, who)
    ts = [t.detach().contiguous() for t in (mu_w, scale_w)] + ([t.detach().contiguous() for t in (mu_b, scale_b)] if mu_b is not None else [])
    for t in ts:
        require_cuda_f32(t, "posterior")
    dev = ts[0].device
    E_w, G_w = torch.empty((O, K), dtype=torch.float32, device=dev), torch.empty((O, K), dtype=torch.float32, device=dev)
    E_b = C_b = None
    if mu_b is not None:
        E_b, C_b = torch.empty((O,), dtype=torch.float32, device=dev), torch.empty((O, O), dtype=torch.float32, device=dev)
    check(_lib.load().bnn_mvn_moments_prepare(ptr(ts[0]), ptr(ts[1]), ptr(ts[2]) if mu_b is not None else None,
                                              ptr(ts[3]) if mu_b is not None else None, ptr(E_w), ptr(G_w), ptr(E_b), ptr(C_b), O, K,
                                              stream_ptr(dev)), "bnn_mvn_moments_prepare")
    return E_w, G_w, E_b, C_b


def moments_mvn_linear(a, mu_w, scale_w, mu_b, scale_b, track=False, prepared=None):
    """Mean and variance of MultivariateNormalLinear's output from the mean and variance of its input -> Moments, fp32 (*rows, O)
    (bnn_mvn_moments_prepare + bnn_mvn_moments_forward, csrc/bnn_moments_head.hip).  The layer draws w_o = mu_o + L_o u with
    uniform u ~ U[0, 1)^K and L = sqrt(tril(softplus(scale)) + 1e-10 I) element by element, so

        E_w[o,k] = mu[o,k] + 1/2 sum_{j<=k} L[o,k,j],  D[o,k] = 1/12 sum_{j<=k} L[o,k,j]^2,  E_b = mu_b + 1/2 L_b 1,  C_b = L_b L_b^T / 12
        m[b,o] = sum_k a_m[b,k] E_w[o,k] + E_b[o]
        v[b,o] = 1/12 sum_j (sum_{k>=j} a_m[b,k] L[o,k,j])^2 + sum_k a_v[b,k] (E_w[o,k]^2 + D[o,k]) + C_b[o,o]

    -- exact for independent input elements.  a: a device tensor (a deterministic input) or a Moments; prepared: the result of
    mvn_moments_prepare on the same posterior (a layer caches it).  Inference only: track=True raises BnnHipError."""
    who = "moments_mvn_linear"
    if track:
        raise BnnHipError("%s: MultivariateNormalLinear has no moment backward (inference only)" % who)
    mom = _as_moments(a, who)
    _refuse_link(mom, who)
    O, K = _mvn_check(mu_w, scale_w, mu_b, scale_b, who)
    am = mom.mean.detach()
    if am.dim() < 1 or am.shape[-1] != K:
        raise BnnHipError("%s: input has %s features, weight expects %d" % (who, am.shape[-1] if am.dim() else "no", K))
    lead = tuple(am.shape[:-1])
    am = am.reshape(-1, K).float().contiguous()
    require_cuda_f32(am, "a.mean")
    av = None
    if mom.var is not None:
        av = mom.var.detach().reshape(-1, K).contiguous()
        require_cuda_f32(av, "a.var")
    B = am.shape[0]
    if B > 64 * 65535:
        raise BnnHipError("%s: %d rows (at most %d)" % (who, B, 64 * 65535))
    E_w, G_w, E_b, C_b = prepared if prepared is not None else mvn_moments_prepare(mu_w, scale_w, mu_b, scale_b)
    scale_w = scale_w.detach().contiguous()
    dev = am.device
    out_m = torch.empty((B, O), dtype=torch.float32, device=dev)
    out_v = torch.empty((B, O), dtype=torch.float32, device=dev)
    check(_lib.load().bnn_mvn_moments_forward(ptr(am), ptr(av), K, ptr(scale_w), ptr(E_w), ptr(G_w), ptr(E_b), ptr(C_b), ptr(out_m),
                                              ptr(out_v), B, O, K, stream_ptr(dev)), "bnn_mvn_moments_forward")
    return Moments(out_m.reshape(lead + (O,)), out_v.reshape(lead + (O,)))


def mvn_factor_f64(scale):
    """L = sqrt(tril(softplus(scale)) + 1e-10 I) element by element, in float64 (WeightMultivariateNormal.stddev); zero above the
    diagonal."""
    s = scale.detach().to(torch.float64)
    return torch.sqrt(torch.tril(torch.nn.functional.softplus(s)) + 1e-10 * torch.eye(s.shape[-1], dtype=torch.float64, device=s.device))


def mvn_moments_prepare_f64(mu_w, scale_w, mu_b, scale_b):
    """mvn_moments_prepare in float64 torch -> (E_w, G_w, E_b, C_b)."""
    _mvn_check(mu_w, scale_w, mu_b, scale_b, "mvn_moments_prepare_f64")
    L = mvn_factor_f64(scale_w)
    E_w = mu_w.detach().to(torch.float64) + 0.5 * L.sum(-1)
    G_w = E_w * E_w + (L * L).sum(-1) / 12.0
    if mu_b is None:
        return E_w, G_w, None, None
    Lb = mvn_factor_f64(scale_b)
    return E_w, G_w, mu_b.detach().to(torch.float64) + 0.5 * Lb.sum(-1), Lb @ Lb.t() / 12.0


def moments_mvn_linear_f64(a, mu_w, scale_w, mu_b, scale_b, track=False, prepared=None):
    """moments_mvn_linear in float64 torch -> Moments of float64 tensors (detached).  prepared: (E_w, G_w, E_b, C_b) to use in place
    of mvn_moments_prepare_f64's (the tests hand in the device's own, so that the forward is compared on its own)."""
    who = "moments_mvn_linear_f64"
    if track:
        raise BnnHipError("%s: MultivariateNormalLinear has no moment backward (inference only)" % who)
    mom = _as_moments(a, who)
    _refuse_link(mom, who)
    f64 = lambda t: None if t is None else t.detach().to(torch.float64)          # noqa: E731
    E_w, G_w, E_b, C_b = [f64(t) for t in prepared] if prepared is not None else mvn_moments_prepare_f64(mu_w, scale_w, mu_b, scale_b)
    L = mvn_factor_f64(scale_w)
    am = f64(mom.mean)
    m = am @ E_w.t()
    t = torch.einsum('...k,okj->...oj', am, L)
    v = (t * t).sum(-1) / 12.0
    if mom.var is not None:
        v = v + f64(mom.var) @ G_w.t()
    if E_b is not None:
        m, v = m + E_b, v + torch.diagonal(C_b)
    return Moments(m, v)


def moments_head_cov(head, var):
    """The covariance of a dense head's outputs per row (ONE bnn_moments_head_cov launch) -> (rows, N, N) fp32:

        cov[b,o,p] = sum_k E[o,k] E[p,k] a_v[b,k] + C_b[o,p]   (o != p),        cov[b,o,o] = var[b,o]

    head: a HeadOperands (a_v (rows, K) or None, E (N, K), C_b (N, N) or None); var (rows, N), the head's output variance.  Both
    triangles hold the same bits and the diagonal holds var's.  N <= 32."""
    who = "moments_head_cov"
    a_v, E, C_b = head
    var = var.detach().contiguous()
    require_cuda_f32(var, "var")
    if var.dim() != 2:
        raise BnnHipError("%s: var must be (rows, N), got %s" % (who, tuple(var.shape)))
    B, N = var.shape
    if N > HEAD_COV_MAX_N:
        raise BnnHipError("%s: %d outputs (at most %d)" % (who, N, HEAD_COV_MAX_N))
    E = E.detach().float().contiguous()
    require_cuda_f32(E, "E")
    K = E.shape[1]
    if E.shape[0] != N:
        raise BnnHipError("%s: E %s for %d outputs" % (who, tuple(E.shape), N))
    if a_v is not None:
        a_v = a_v.detach().contiguous()
        require_cuda_f32(a_v, "a_v")
        if tuple(a_v.shape) != (B, K):
            raise BnnHipError("%s: a_v %s, expected %s" % (who, tuple(a_v.shape), (B, K)))
    if C_b is not None:
        C_b = C_b.detach().contiguous()
        require_cuda_f32(C_b, "C_b")
        if tuple(C_b.shape) != (N, N):
            raise BnnHipError("%s: C_b %s, expected %s" % (who, tuple(C_b.shape), (N, N)))
    cov = torch.empty((B, N, N), dtype=torch.float32, device=var.device)
    check(_lib.load().bnn_moments_head_cov(ptr(a_v), K, ptr(E), ptr(C_b), ptr(var), ptr(cov), B, N, K, stream_ptr(var.device)),
          "bnn_moments_head_cov")
    return cov


def moments_head_cov_f64(head, var):
    """moments_head_cov in float64 torch -> (rows, N, N) float64."""
    a_v, E, C_b = head
    f64 = lambda t: t.detach().to(torch.float64)          # noqa: E731
    var = f64(var)
    B, N = var.shape
    if N > HEAD_COV_MAX_N:
        raise BnnHipError("moments_head_cov_f64: %d outputs (at most %d)" % (N, HEAD_COV_MAX_N))
    cov = torch.zeros((B, N, N), dtype=torch.float64, device=var.device)
    if a_v is not None:
        E = f64(E)
        cov = cov + torch.einsum('ok,pk,bk->bop', E, E, f64(a_v))
    if C_b is not None:
        cov = cov + f64(C_b)
    # symmetric bit for bit, whatever order the BLAS behind einsum multiplies E[o] a_v E[p] in (x + y == y + x exactly)
    cov = 0.5 * (cov + cov.transpose(-1, -2))
    idx = torch.arange(N, device=var.device)
    cov[:, idx, idx] = var
    return cov


def moments_resolve_cov(mom, who="predictive_moments"):
    """Moments whose producing dense layer left its HeadOperands (a covariance pass) -> the same moments with cov (*rows, N, N):
    ONE bnn_moments_head_cov launch on the device, moments_head_cov_f64 on the CPU."""
    head = mom._head
    if head is None:
        raise BnnHipError("%s: these moments carry no head operands" % who)
    N = mom.shape[-1]
    lead = tuple(mom.shape[:-1])
    var = (torch.zeros_like(mom.mean) if mom.var is None else mom.var).reshape(-1, N)
    cov = moments_head_cov(head, var) if mom.mean.is_cuda else moments_head_cov_f64(head, var)
    return Moments(mom.mean, mom.var, mom.link, cov=cov.reshape(lead + (N, N)))


def cholesky_pivot_f64(cov):
    """The lower Cholesky factor of (..., N, N) covariances in float64, column by column in a plain loop, with
    bnn_moments_sample_cov's pivot rule: a pivot <= 0 gives a zero column (a direction without variance -- a semi-definite
    covariance, or one made so by rounding).  Only the lower triangle is read."""
    A = cov.detach().to(torch.float64)
    N = A.shape[-1]
    L = torch.zeros_like(A)
    for j in range(N):
        s = A[..., j:, j] - (L[..., j:, :j] * L[..., j:j + 1, :j]).sum(-1)
        pos = s[..., 0] > 0
        d = torch.sqrt(torch.where(pos, s[..., 0], torch.ones_like(s[..., 0])))
        L[..., j, j] = torch.where(pos, d, torch.zeros_like(d))
        if j + 1 < N:
            L[..., j + 1:, j] = torch.where(pos.unsqueeze(-1), s[..., 1:] / d.unsqueeze(-1), torch.zeros_like(s[..., 1:]))
    return L


def _moments_sample_cov(mom, key, S, track):
    """moments_sample for moments that carry a covariance."""
    who = "moments_sample"
    if _tracking(track):
        raise BnnHipError("%s: moments that carry a covariance have no backward (sample_moments / track=True)" % who)
    m, cov = mom.mean.detach(), mom.cov.detach()
    N = m.shape[-1]
    if not m.is_cuda:
        Lc = cholesky_pivot_f64(cov)
        eps = torch.randn((S,) + tuple(m.shape), dtype=torch.float64)
        return (m.to(torch.float64) + torch.einsum('...ik,s...k->s...i', Lc, eps)).to(torch.float32)
    m, cov = m.contiguous(), cov.contiguous()
    require_cuda_f32(m, "mean")
    require_cuda_f32(cov, "cov")
    if N > HEAD_COV_MAX_N:
        raise BnnHipError("%s: a covariance over %d outputs (at most %d)" % (who, N, HEAD_COV_MAX_N))
    if S < 1 or S > 0xFFFF:
        raise BnnHipError("%s: %d MC samples (1 .. 65535)" % (who, S))
    if m.numel() >= 2 ** 32:
        raise BnnHipError("%s: one sample has %d elements: the noise index is 32 bits wide" % (who, m.numel()))
    rows = m.numel() // N
    y = torch.empty((S,) + tuple(m.shape), dtype=torch.float32, device=m.device)
    r = _rng_struct(key, m.device)
    check(_lib.load().bnn_moments_sample_cov(ptr(m), ptr(cov), ptr(y), rows, N, S, ctypes.byref(r), 0, stream_ptr(m.device)),
          "bnn_moments_sample_cov")
    return y


class _PlainLinear(torch.autograd.Function):
    """y[s] = x[s] @ w[s]^T + b[s] with given weights (F.linear, dense.py:60)."""

    @staticmethod
    def forward(ctx, x, w, b, shared_x, compute):
        require_cuda_f32(x, "x")
        require_cuda_f32(w, "w")
        S, N, K = w.shape
        M = x.shape[-2]
        if x.shape[-1] != K:
            raise BnnHipError("linear: input has %d features, weight expects %d" % (x.shape[-1], K))
        y = torch.empty((S, M, N), dtype=torch.float32, device=x.device)
        if b is not None:
            require_cuda_f32(b, "b")
        check(_lib.load().bnn_linear_forward(ptr(x), 0 if shared_x else M * K, K, ptr(w), N * K, ptr(b), N,
                                              ptr(y), M * N, N, M, N, K, S, compute, 0, stream_ptr(x.device)),
              "bnn_linear_forward")
        ctx.save_for_backward(x, w)
        ctx.shared_x, ctx.has_b, ctx.compute = shared_x, b is not None, compute
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        S, N, K = w.shape
        M = x.shape[-2]
        gy = gy.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _dgrad_plain_raw(gy, w, torch.float32)
            if ctx.shared_x:
                gx = _sum_samples(gx)
        if ctx.needs_input_grad[1]:
            gw = _wgrad_plain_raw(x, 0 if ctx.shared_x else M * K, gy, M, N, K, S, ctx.compute)
        if ctx.has_b and ctx.needs_input_grad[2]:
            gb = _colsum_raw(gy)
        return gx, gw, gb, None, None


def linear_plain(x, w, b, shared_x, compute="f32"):
    return _PlainLinear.apply(x.contiguous(), w.contiguous(), None if b is None else b.contiguous(),
                              shared_x, _compute_code(compute))


# --------------------------------------------------------------------------- K25: the Bayesian LSTM cell (nn.NormalLSTM)
LSTM_TILE_ROWS, LSTM_TILE_UNITS = 16, 16        # csrc/bnn_lstm.hip: L_TR rows of a sample x L_TU hidden units per workgroup


def _at(t, elements):
    """Device pointer `elements` fp32 elements into t (a step of a (S, rows, T, .) buffer, addressed with a row pitch)."""
    return ctypes.c_void_p(t.data_ptr() + 4 * elements)


class _LstmSaved:
    """What the backward of one LSTM forward needs: the input, the two column blocks of the drawn weights, every step's hidden
    and cell state and gate activations (the tensors travel through ctx.save_for_backward, in this order)."""
    __slots__ = ("x", "wx", "wh", "hs", "cs", "gates", "shared_x")

    def __init__(self, x, wx, wh, hs, cs, gates, shared_x):
        self.x, self.wx, self.wh, self.hs, self.cs, self.gates, self.shared_x = x, wx, wh, hs, cs, gates, shared_x


def _lstm_forward_raw(x, w, b, shared_x, want_grad):
    """The recurrence on given weights.  x: (rows, T, I) shared by the samples or (S, rows, T, I); w: (S, 4 H, I + H), columns
    [0, I) on x_t and [I, I + H) on h_{t-1}, rows in gate order i, f, g, o; b: (S, 4 H) or None -- fp32, contiguous.
    -> hs (S, rows, T, H), and (wx, wh, cs, gates) when a backward will follow (None otherwise).  One bnn_linear_forward for the input projection of all
    steps, then T bnn_lstm_step_forward launches; nothing in the loop allocates or synchronises."""
    S, H4, IH = w.shape
    H = H4 // 4
    I = IH - H
    rows, T = x.shape[-3], x.shape[-2]
    if H4 != 4 * H or I < 1 or x.shape[-1] != I:
        raise BnnHipError("lstm: input has %d features, weight (%d, %d) expects %d" % (x.shape[-1], H4, IH, I))
    if rows < 1 or T < 1:
        raise BnnHipError("lstm: needs at least one row and one time step, got rows = %d, T = %d" % (rows, T))
    dev = x.device
    lib = _lib.load()
    st = stream_ptr(dev)
    wx, wh = w[:, :, :I].contiguous(), w[:, :, I:].contiguous()         # the existing contractions take a weight row pitch of K
    M = rows * T
    gx = torch.empty((S, rows, T, H4), dtype=torch.float32, device=dev)
    check(lib.bnn_linear_forward(ptr(x), 0 if shared_x else M * I, I, ptr(wx), H4 * I, ptr(b), H4, ptr(gx), M * H4, H4,
                                 M, H4, I, S, _lib.COMPUTE_F32, 0, st), "bnn_linear_forward")
    hs = torch.empty((S, rows, T, H), dtype=torch.float32, device=dev)
    if want_grad:
        cs = torch.empty((S, rows, T, H), dtype=torch.float32, device=dev)
        gates = torch.empty((S, rows, T, H4), dtype=torch.float32, device=dev)
    else:
        cs, gates = torch.empty((2, S, rows, H), dtype=torch.float32, device=dev), None
    for t in range(T):
        if want_grad:
            c_prev, c, ldc = (_at(cs, (t - 1) * H) if t else None), _at(cs, t * H), T * H
        else:                                                               # inference: two cell-state buffers take turns
            c_prev, c, ldc = (_at(cs, ((t - 1) % 2) * S * rows * H) if t else None), _at(cs, (t % 2) * S * rows * H), H
        check(lib.bnn_lstm_step_forward(_at(gx, t * H4), T * H4, ptr(wh), H4 * H, _at(hs, (t - 1) * H) if t else None, T * H,
                                        c_prev, ldc, _at(hs, t * H), T * H, c, ldc,
                                        _at(gates, t * H4) if want_grad else None, T * H4, rows, H, S, st), "bnn_lstm_step_forward")
    return hs, ((wx, wh, cs, gates) if want_grad else None)


def _lstm_backward_raw(sv, gy, need_x, need_w, need_b):
    """gy: (S, rows, T, H), or (S, rows, H) when only the last hidden state left the layer -> (g_x, g_w (S, 4 H, I + H), g_b (S, 4 H)),
    None where not needed.  T bnn_lstm_step_backward launches from t = T - 1 down leave dG (S, rows, T, 4 H); every sum over time
    then runs once over T * rows rows on the linear layer's entries."""
    S, rows, T, H = sv.hs.shape
    H4, I = 4 * H, sv.wx.shape[2]
    M = rows * T
    dev = gy.device
    lib = _lib.load()
    st = stream_ptr(dev)
    dg = torch.empty((S, rows, T, H4), dtype=torch.float32, device=dev)
    carry = torch.empty((2, 2, S, rows, H), dtype=torch.float32, device=dev)        # [g_h | g_c][t % 2]
    n = S * rows * H
    g_h, g_c = (_at(carry, 0), _at(carry, n)), (_at(carry, 2 * n), _at(carry, 3 * n))
    seq = gy.dim() == 4
    for t in range(T - 1, -1, -1):
        last = t == T - 1
        g_h_out = _at(gy, t * H) if seq else (ptr(gy) if last else None)
        check(lib.bnn_lstm_step_backward(_at(sv.gates, t * H4), T * H4, _at(sv.cs, (t - 1) * H) if t else None, T * H,
                                         _at(sv.cs, t * H), T * H, g_h_out, T * H if seq else H,
                                         None if last else g_h[(t + 1) % 2], None if last else g_c[(t + 1) % 2],
                                         ptr(sv.wh), H4 * H, _at(dg, t * H4), T * H4, g_h[t % 2], g_c[t % 2],
                                         rows, H, S, st), "bnn_lstm_step_backward")
    dg = dg.view(S, M, H4)
    g_x = g_w = g_b = None
    if need_w:
        g_wx = _wgrad_plain_raw(sv.x, 0 if sv.shared_x else M * I, dg, M, H4, I, S)
        h_prev = torch.zeros_like(sv.hs)                                            # h_{t-1} per (row, step): h_{-1} = 0
        h_prev[:, :, 1:] = sv.hs[:, :, :-1]
        g_wh = _wgrad_plain_raw(h_prev, M * H, dg, M, H4, H, S)
        g_w = torch.cat((g_wx, g_wh), dim=2)
    if need_b:
        g_b = _colsum_raw(dg)
    if need_x:
        g_x = _dgrad_plain_raw(dg, sv.wx, torch.float32)                            # (S, M, I)
        g_x = _sum_samples(g_x).view(rows, T, I) if sv.shared_x else g_x.view(S, rows, T, I)
    return g_x, g_w, g_b


def _lstm_check_input(x, shared_x, S):
    require_cuda_f32(x, "x")
    if x.dim() != (3 if shared_x else 4) or (not shared_x and x.shape[0] != S):
        raise BnnHipError("lstm: x must be (rows, T, I) for a shared input or (S, rows, T, I), got %s for S = %d" % (tuple(x.shape), S))


def _lstm_output(hs, return_sequences):
    return hs if return_sequences else hs[:, :, -1].contiguous()


class _LstmSampled(torch.autograd.Function):
    """NormalLSTM on its posterior: w (S, 4 H, I + H) and b (S, 4 H) drawn by bnn_sample_affine_philox on the keys -- ONE draw per
    MC sample for all T steps -- then _lstm_forward_raw.  Backward: _lstm_backward_raw, then bnn_sample_affine_bwd on the keys."""

    @staticmethod
    def forward(ctx, x, mu_w, rho_w, mu_b, rho_b, key_w, key_b, shared_x, return_sequences, track):
        S = key_w.nsamples
        _lstm_check_input(x, shared_x, S)
        w = _sample_affine_philox_raw(mu_w, rho_w, key_w)
        b = _sample_affine_philox_raw(mu_b, rho_b, key_b) if mu_b is not None else None
        want_grad = track and any(ctx.needs_input_grad[:5])
        hs, kept = _lstm_forward_raw(x, w, b, shared_x, want_grad)
        ctx.key_w, ctx.key_b, ctx.shared_x = key_w, key_b, shared_x
        if kept is not None:
            ctx.save_for_backward(x, kept[0], kept[1], hs, kept[2], kept[3], rho_w, rho_b)
        return _lstm_output(hs, return_sequences)

    @staticmethod
    def backward(ctx, gy):
        rho_w, rho_b = ctx.saved_tensors[6:]
        sv, S = _LstmSaved(*ctx.saved_tensors[:6], ctx.shared_x), ctx.key_w.nsamples
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        need_b = rho_b is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        g_x, g_w, g_b = _lstm_backward_raw(sv, gy.contiguous().float(), ctx.needs_input_grad[0], need_w, need_b)
        g_mu_w = g_rho_w = g_mu_b = g_rho_b = None
        if need_w:
            g_mu_w, g_rho_w = _sample_affine_bwd_raw(g_w, rho_w, rho_w.numel(), S, key=ctx.key_w)
        if need_b:
            g_mu_b, g_rho_b = _sample_affine_bwd_raw(g_b, rho_b, rho_b.numel(), S, key=ctx.key_b)
        return g_x, g_mu_w, g_rho_w, g_mu_b, g_rho_b, None, None, None, None, None


class _LstmPlain(torch.autograd.Function):
    """The same recurrence and the same kernels on given weights w (S, 4 H, I + H), b (S, 4 H) or None."""

    @staticmethod
    def forward(ctx, x, w, b, shared_x, return_sequences, track):
        require_cuda_f32(w, "w")
        if b is not None:
            require_cuda_f32(b, "b")
        _lstm_check_input(x, shared_x, w.shape[0])
        want_grad = track and any(ctx.needs_input_grad[:3])
        hs, kept = _lstm_forward_raw(x, w, b, shared_x, want_grad)
        ctx.has_b, ctx.shared_x = b is not None, shared_x
        if kept is not None:
            ctx.save_for_backward(x, kept[0], kept[1], hs, kept[2], kept[3])
        return _lstm_output(hs, return_sequences)

    @staticmethod
    def backward(ctx, gy):
        sv = _LstmSaved(*ctx.saved_tensors, ctx.shared_x)
        g_x, g_w, g_b = _lstm_backward_raw(sv, gy.contiguous().float(), ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                           ctx.has_b and ctx.needs_input_grad[2])
        return g_x, g_w, g_b, None, None, None


def lstm_sampled(x, mu_w, rho_w, mu_b, rho_b, key_w, key_b, shared_x, return_sequences=True):
    """The Bayesian LSTM layer (K25) on a device input: x (rows, T, I) shared by the key's S samples, or (S, rows, T, I) -> the hidden
    states (S, rows, T, H), or the last one (S, rows, H).  fp32 operands and accumulation in both compute modes."""
    for t, n in ((mu_w, "weight.mean"), (rho_w, "weight.scale")):
        if not t.is_cuda:
            raise BnnHipError("%s must be a CUDA/HIP tensor" % n)
    return _LstmSampled.apply(x.contiguous(), mu_w.contiguous(), rho_w.contiguous(),
                              None if mu_b is None else mu_b.contiguous(), None if rho_b is None else rho_b.contiguous(),
                              key_w, key_b, bool(shared_x), bool(return_sequences), torch.is_grad_enabled())


def lstm_plain(x, w, b, shared_x, return_sequences=True):
    """lstm_sampled's recurrence on explicit weights w (S, 4 H, I + H), b (S, 4 H) or None (weights assigned through .sampled)."""
    return _LstmPlain.apply(x.contiguous(), w.contiguous(), None if b is None else b.contiguous(), bool(shared_x),
                            bool(return_sequences), torch.is_grad_enabled())


# --------------------------------------------------------------------------- MC dropout
def check_drop_prob(p):
    """F.dropout's argument check (same ValueError)."""
    if not (0.0 <= p <= 1.0):
        raise ValueError("dropout probability has to be between 0 and 1, but got {}".format(p))


def _drop_rows(y, S, shared):
    """(rows per sample, features per row) of an MC-dropout operand: y (B, ...) shared, or (S * B, ...) stacked."""
    if y.dim() < 2:
        raise BnnHipError("mc_dropout: the input needs a batch dimension and features")
    R = y.shape[0] if shared else y.shape[0] // S
    if not shared and R * S != y.shape[0]:
        raise BnnHipError("mc_dropout: %d rows are not %d samples of equal batches" % (y.shape[0], S))
    F = 1
    for d in y.shape[1:]:
        F *= d
    return R, F


def _mc_dropout_bwd_raw(gy, R, F, p, key, shared):
    """mask (.) gy / (1 - p) for gy (S * R, ...) fp32 -> same shape, or (R, ...) summed over the samples (shared)."""
    S = key.nsamples
    gy = gy.contiguous().float()
    gx = torch.empty(((R,) if shared else (S * R,)) + tuple(gy.shape[1:]), dtype=torch.float32, device=gy.device)
    r = _rng_struct(key, gy.device)
    check(_lib.load().bnn_mc_dropout_backward(ptr(gy), R * F, ptr(gx), R * F, R, F, S, float(p), 1 if shared else 0,
                                              ctypes.byref(r), stream_ptr(gy.device)), "bnn_mc_dropout_backward")
    return gx


class _McDropout(torch.autograd.Function):
    """MC dropout under the mask contract (include/bnn_hip.h), F.dropout(y, p, True) of pytorch_bayesian/nn/dense.py:174-179 and
    nn/conv.py:277-326 with the keyed mask of every MC sample: bnn_mc_dropout forward, bnn_mc_dropout_backward backward."""

    @staticmethod
    def forward(ctx, y, p, key, shared):
        require_cuda_act(y, "y")
        S = key.nsamples
        R, F = _drop_rows(y, S, shared)
        out = torch.empty((S * R,) + tuple(y.shape[1:]), dtype=y.dtype, device=y.device)
        r = _rng_struct(key, y.device)
        dt = _lib.BF16 if y.dtype == torch.bfloat16 else _lib.F32
        check(_lib.load().bnn_mc_dropout(ptr(y), 0 if shared else R * F, ptr(out), R * F, R, F, S, float(p), dt,
                                         ctypes.byref(r), stream_ptr(y.device)), "bnn_mc_dropout")
        ctx.p, ctx.key, ctx.shared, ctx.R, ctx.F, ctx.dtype = p, key, shared, R, F, y.dtype
        return out

    @staticmethod
    def backward(ctx, gy):
        g = _mc_dropout_bwd_raw(gy, ctx.R, ctx.F, ctx.p, ctx.key, ctx.shared)
        return g.to(ctx.dtype), None, None, None


def mc_dropout(y, p, key, shared):
    """Masks of the key's `nsamples` MC samples (key.sample0 + s) on y: shared -- y (B, ...) computed once for every sample
    -> (S * B, ...) fanned out; else y (S * B, ...), sample s = row // B -> (S * B, ...).  fp32 or bf16.  The mask depends on
    (sample, row within the sample, flattened feature) only."""
    check_drop_prob(p)
    return _McDropout.apply(y.contiguous(), float(p), key, bool(shared))


def mean_bf16(w):
    """The fp32 weight (N, K) as the dense kernel's operand: (1, N, roundup(K, 64)) bf16 zero-padded (bnn_draw_multi kind BNN_DRAW_MEAN)."""
    require_cuda_f32(w, "weight")
    N, K = w.shape
    kp = _pad64(K)
    out = torch.empty((1, N, kp), dtype=torch.bfloat16, device=w.device)
    arr = (_lib.DrawTensor * 1)()
    _draw_slot(arr[0], w, None, N, K, out.data_ptr(), kp, N * kp, _lib.BF16, _lib.DRAW_MEAN)
    _draw_launch(arr, 1, 1, w.device)
    return out


def linear_mc_dropout_fusable(x, w, compute):
    """bf16 mode, and a shape the dense kernel takes (K % 8 == 0: whole 16-B rows of bf16)."""
    return _compute_code(compute) == _lib.COMPUTE_BF16 and w.dim() == 2 and w.shape[1] % 8 == 0 and x.dim() == 2


class _LinearMcDropout(torch.autograd.Function):
    """F.dropout(F.linear(x, w, b), p, True) for every MC sample in ONE bnn_dense_forward_dropout launch (bf16 operands, fp32
    accumulate and output): the mask is applied in the GEMM's epilogue.  (x arrives fp32 and is cast to bf16 by a torch op first:
    one pass over the layer's input that bnn_launch_count does not see.)  shared: x (B, K) is the same for every sample -- the
    GEMM runs once and the epilogue stores S masked copies.  Backward: the masked gradient (summed over the samples first when
    shared), then ONE contraction over the rows (bnn_linear_backward_input / _weight, bnn_colsum) in fp32."""

    @staticmethod
    def forward(ctx, x, w, b, p, key, shared, w_bf16):
        require_cuda_f32(x, "x")
        require_cuda_f32(w, "weight")
        S = key.nsamples
        N, K = w.shape
        if x.shape[-1] != K:
            raise BnnHipError("linear: input has %d features, weight expects %d" % (x.shape[-1], K))
        B = x.shape[0] if shared else x.shape[0] // S
        if w_bf16 is None:
            w_bf16 = mean_bf16(w)
        kp = w_bf16.shape[-1]
        xb = x.to(torch.bfloat16).contiguous()
        if b is not None:
            require_cuda_f32(b, "bias")
        y = torch.empty((S * B, N), dtype=torch.float32, device=x.device)
        r = _rng_struct(key, x.device)
        check(_lib.load().bnn_dense_forward_dropout(ptr(xb), 0 if shared else B * K, K, ptr(w_bf16), 0, kp, ptr(b), 0,
                                                    ptr(y), B * N, N, B, N, K, S, 0, float(p), ctypes.byref(r),
                                                    stream_ptr(x.device)), "bnn_dense_forward_dropout")
        ctx.save_for_backward(x, w)
        ctx.p, ctx.key, ctx.shared, ctx.B, ctx.has_b = p, key, shared, B, b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        N, K = w.shape
        g = _mc_dropout_bwd_raw(gy, ctx.B, N, ctx.p, ctx.key, ctx.shared)       # (B or S * B, N): one contraction below
        return _plain_linear_bwd(ctx, x, w, g) + (None, None, None, None)


def _plain_linear_bwd(ctx, x, w, g):
    """(gx, gw, gb) of y = x w^T + b for ONE weight over all rows of x (M, K) / g (M, N), fp32."""
    N, K = w.shape
    M = x.shape[0]
    gx = gw = gb = None
    g3 = g.view(1, M, N)
    if ctx.needs_input_grad[0]:
        gx = _dgrad_plain_raw(g3, w.view(1, N, K), torch.float32).view(M, K)
    if ctx.needs_input_grad[1]:
        gw = _wgrad_plain_raw(x, M * K, g, M, N, K, 1).view(N, K)
    if ctx.has_b and ctx.needs_input_grad[2]:
        gb = _colsum_raw(g3).view(N)
    return gx, gw, gb


def linear_mc_dropout(x, w, b, p, key, shared, compute="f32", w_bf16=None):
    """MCDropoutLinear on the MC-batched path: F.dropout(F.linear(x, w, b), p, True) with the keyed mask of each of the key's
    nsamples samples.  shared: x (B, K) -> (S * B, N) fanned out; else x (S * B, K), sample s = row // B -> (S * B, N).
      bf16 mode, K % 8 == 0: ONE fused launch (bnn_dense_forward_dropout; w_bf16: the weight as mean_bf16 returns it, drawn
                             here when None);
      otherwise (the fp32 parity mode, K % 8 != 0): the HIP linear (bnn_linear_forward) once over all rows, then bnn_mc_dropout."""
    check_drop_prob(p)
    x = x.contiguous()
    w = w.contiguous()
    b = None if b is None else b.contiguous()
    S = key.nsamples
    if linear_mc_dropout_fusable(x, w, compute):
        return _LinearMcDropout.apply(x.float() if x.dtype != torch.float32 else x, w, b, float(p), key, bool(shared), w_bf16)
    if x.dim() != 2:
        raise BnnHipError("linear_mc_dropout: x must be (rows, features)")
    M = x.shape[0]
    h = linear_plain(x.float(), w.unsqueeze(0), None if b is None else b.unsqueeze(0), True, compute)     # (1, M, N)
    return mc_dropout(h.view(M, -1), p, key, shared)


# --------------------------------------------------------------------------- Flipout, MC-batched
def flipout_signs(key, rows, width, device):
    """The keyed Flipout signs of the key's nsamples MC samples (sign contract, include/bnn_hip.h) -> (S, rows, width) fp32 +-1:
    conv rows = B, width = O + C (R = [..., :O], S = [..., O:]); linear rows = 1, width = O + K (bnn_flipout_signs)."""
    out = torch.empty((key.nsamples, rows, width), dtype=torch.float32, device=device)
    r = _rng_struct(key, device)
    check(_lib.load().bnn_flipout_signs(ptr(out), rows * width, rows, width, key.nsamples, ctypes.byref(r), stream_ptr(device)),
          "bnn_flipout_signs")
    return out


def flipout_draw(mu, rho, key, out_dtype=torch.float32, pad=False):
    """w_s = mu + sigma(rho) (.) R_s S_s^T for the key's samples (bnn_draw_multi kind BNN_DRAW_FLIPOUT) -> (S, O, K) fp32, or with pad (S, O,
    roundup(K, 64)) zero-padded -- the dense kernel's operand in bf16.  Needs K % 4 == 0 (K % 8 == 0 for an unpadded fp32 draw)."""
    require_cuda_f32(mu, "weight.mean")
    require_cuda_f32(rho, "weight.scale")
    O, K = mu.shape
    ld = _pad64(K) if pad else K
    S = key.nsamples
    w = torch.empty((S, O, ld), dtype=out_dtype, device=mu.device)
    arr = (_lib.DrawTensor * 1)()
    _draw_slot(arr[0], mu, rho, O, K, w.data_ptr(), ld, O * ld, _lib.F32 if out_dtype == torch.float32 else _lib.BF16,
               _lib.DRAW_FLIPOUT, key=key)
    _draw_launch(arr, 1, S, mu.device)
    return w


def flipout_drawable(mu):
    """The sign-outer-product draw takes this (O, K) posterior (whole rows of 8 columns, 16-B aligned)."""
    return mu.dim() == 2 and mu.shape[1] % 8 == 0 and mu.data_ptr() % 16 == 0


class _FlipoutLinear(torch.autograd.Function):
    """FlipoutNormalLinear on the MC-batched path: y[s] = x[s] (mu + sigma (.) R_s S_s^T)^T -- exactly x mu^T + ((x * S_s) sigma^T)
    * R_s of dense.py:70-83 -- with the keyed signs of every sample (bnn_draw_multi kind BNN_DRAW_FLIPOUT).  bf16 mode: the dense kernel on the
    bf16 draw (`predrawn`: drawn by the network's plan); fp32 mode: bnn_linear_forward on the fp32 draw.  Backward: the fp32 draw
    again (never stored), bnn_linear_backward_input / _weight, and bnn_flipout_weight_backward for d/d mu and d/d rho."""

    @staticmethod
    def forward(ctx, x, mu, rho, key, shared, compute, predrawn):
        require_cuda_f32(x, "x")
        S = key.nsamples
        O, K = mu.shape
        B = x.shape[0] if shared else x.shape[0] // S
        if x.shape[-1] != K:
            raise BnnHipError("linear: input has %d features, weight expects %d" % (x.shape[-1], K))
        if compute == _lib.COMPUTE_BF16:
            pre = predrawn
            if pre is None:
                pre = Predrawn(flipout_draw(mu, rho, key, torch.bfloat16, pad=True), None, key, None)
            xb = x.to(torch.bfloat16).contiguous()
            y = _dense_raw(xb, 0 if shared else B * K, B, pre, K, False, torch.float32)
        else:
            w = flipout_draw(mu, rho, key)
            y = torch.empty((S, B, O), dtype=torch.float32, device=x.device)
            check(_lib.load().bnn_linear_forward(ptr(x), 0 if shared else B * K, K, ptr(w), O * K, None, 0, ptr(y), B * O, O,
                                                  B, O, K, S, compute, 0, stream_ptr(x.device)), "bnn_linear_forward")
        ctx.save_for_backward(x, mu, rho)
        ctx.key, ctx.shared, ctx.B = key, shared, B
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mu, rho = ctx.saved_tensors
        key, B = ctx.key, ctx.B
        S = key.nsamples
        O, K = mu.shape
        dev = gy.device
        lib = _lib.load()
        gy = gy.contiguous().float()
        gx = g_mu = g_rho = None
        if ctx.needs_input_grad[0]:
            gx = _dgrad_plain_raw(gy, flipout_draw(mu, rho, key), torch.float32)       # (S, B, K)
            gx = _sum_samples(gx) if ctx.shared else gx.reshape(S * B, K)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw = _wgrad_plain_raw(x, 0 if ctx.shared else B * K, gy, B, O, K, S)
            g_mu, g_rho = torch.empty_like(mu), torch.empty_like(rho)
            r = _rng_struct(key, dev)
            check(lib.bnn_flipout_weight_backward(ptr(gw), O * K, ptr(rho), ptr(g_mu), ptr(g_rho), O, K, S, ctypes.byref(r),
                                                  stream_ptr(dev)), "bnn_flipout_weight_backward")
        return gx, g_mu, g_rho, None, None, None, None


def linear_flipout_mc(x, mu, rho, key, shared, compute="f32", predrawn=None):
    """FlipoutNormalLinear on the MC-batched path -> (S, B, O).  x (B, K) shared by the samples or (S * B, K), fp32; the
    caller checked flipout_drawable(mu)."""
    return _FlipoutLinear.apply(x.contiguous().float(), mu.contiguous(), rho.contiguous(), key, bool(shared),
                                _compute_code(compute), predrawn)


def conv2d_flipout_mc_eligible(x, mean, stride, padding, dilation, groups, S, shared):
    """bf16 compute, inference: the keyed one-launch Flipout conv (bnn_conv2d_flipout_forward_mc) takes this layer -- the shapes
    of bnn_conv2d_flipout_forward, with the samples' masks and R signs in the LDS block too."""
    if not (DRAW_ONCE_BF16 and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and mean.data_ptr() % 16 == 0):
        return False
    O, C, KH, KW = mean.shape
    B = x.shape[0] if shared else x.shape[0] // S
    if B * (O + C) >= 2 ** 32 or S > 0xFFFF:
        return False
    sh = _conv_shape((B,) + tuple(x.shape[1:]), mean.shape, stride, padding, dilation, groups)[0]
    return _conv_lds_images(sh, _lib.CONV_FLIPOUT_MC, S, shared) > 0


def conv2d_flipout_mc(x, mean, scale, key, shared, stride, padding, dilation):
    """FlipOutNormalConv2d on the MC-batched path (conv.py:207-221 with the keyed signs of every sample) in two launches: mean and
    stddev written tap-major as bf16 (bnn_draw_multi, kinds 1 / 2), then ONE keyed implicit GEMM for all S samples
    (bnn_conv2d_flipout_forward_mc; no sign tensor, no fanned-out x).  x (B, C, H, W) shared or (S * B, ...) -> (S * B, O, OH, OW).
    No autograd (inference path)."""
    x = x.contiguous()
    require_cuda_f32(x, "x")
    S = key.nsamples
    O = mean.shape[0]
    B = x.shape[0] if shared else x.shape[0] // S
    dev = x.device
    w2 = flipout_conv_weights(mean, scale)
    kp = w2.shape[1]
    sh, OH, OW = _conv_shape((B,) + tuple(x.shape[1:]), mean.shape, stride, padding, dilation, 1)
    y = torch.empty((S * B, O, OH, OW), dtype=torch.float32, device=dev)
    r = _rng_struct(key, dev)
    check(_lib.load().bnn_conv2d_flipout_forward_mc(ptr(x), 0 if shared else B * x[0].numel(), ptr(w2), kp, ptr(y),
                                                    B * O * OH * OW, ctypes.byref(sh), S, ctypes.byref(r), 0, stream_ptr(dev)),
          "bnn_conv2d_flipout_forward_mc")
    return y


# --------------------------------------------------------------------------- K2 conv2d
def _conv_shape(x_shape, w_shape, stride, padding, dilation, groups):
    sh = Conv2dShape()
    sh.B, sh.C, sh.H, sh.W = x_shape
    sh.O, _, sh.KH, sh.KW = w_shape
    sh.stride_h, sh.stride_w = stride
    sh.pad_h, sh.pad_w = padding
    sh.dil_h, sh.dil_w = dilation
    sh.groups = groups
    OH = (sh.H + 2 * sh.pad_h - sh.dil_h * (sh.KH - 1) - 1) // sh.stride_h + 1
    OW = (sh.W + 2 * sh.pad_w - sh.dil_w * (sh.KW - 1) - 1) // sh.stride_w + 1
    return sh, OH, OW


def _conv_workspace(sh, x_samples, compute, device):
    """im2col panel for the fast conv path (None: the generic kernel runs)."""
    nbytes = _lib.load().bnn_conv2d_workspace_bytes(ctypes.byref(sh), x_samples, compute)
    if nbytes <= 0:
        return None, 0
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _conv_lds_images(sh, variant, nsamples=1, shared_x=True):
    """Images a workgroup of the LDS-resident conv launch `variant` (_lib.CONV_*) keeps, 0 where that launch does not take the
    shape: the library's own fit computation (bnn_conv2d_dense_images, a host query), so the predicates below cannot drift from
    the kernel's ring depths and LDS blocks.  (A kernel larger than the padded input is a negative code: not taken either.)"""
    return _lib.load().bnn_conv2d_dense_images(ctypes.byref(sh), variant, nsamples, int(shared_x))


def conv_dense_eligible(sh, OH, OW):
    """Shapes bnn_conv2d_dense_forward is built for (include/bnn_hip.h): both BASELINE conv layers."""
    return _conv_lds_images(sh, _lib.CONV_DENSE) > 0


CONV_X3_F32 = os.environ.get("BNN_CONV_X3", "1") != "0"      # fp32 parity mode of eligible inference convolutions without the im2col panel


def conv_dense_x3_eligible(sh, OH, OW):
    """Shapes bnn_conv2d_dense_forward_x3 takes: as conv_dense_eligible with three bf16 planes of an image resident."""
    return _conv_lds_images(sh, _lib.CONV_DENSE_X3) > 0


def _conv_rows_raw(gy, sh, P, S, bf):
    """gy (S, B, O, OH, OW) fp32 -> the rows (S, B P, O) of the conv seen as a linear layer, fp32 or bf16 (bnn_nchw_to_rows)."""
    rows = torch.empty((S, sh.B * P, sh.O), dtype=torch.bfloat16 if bf else torch.float32, device=gy.device)
    check(_lib.load().bnn_nchw_to_rows(ptr(gy), S * sh.B, sh.O, P, ptr(rows), int(bf), stream_ptr(gy.device)), "bnn_nchw_to_rows")
    return rows


def _conv_panel_raw(x, sh, M, K, S, shared_x, bf):
    """x -> its im2col panel (1 or S, M, K), fp32 or bf16 (bnn_conv2d_im2col) -> (panel, its sample stride)."""
    nsx = 1 if shared_x else S
    panel = torch.empty((nsx, M, K), dtype=torch.bfloat16 if bf else torch.float32, device=x.device)
    per = sh.B * sh.C * sh.H * sh.W
    check(_lib.load().bnn_conv2d_im2col(ptr(x), 0 if shared_x else per, ctypes.byref(sh), nsx, ptr(panel), int(bf), stream_ptr(x.device)),
          "bnn_conv2d_im2col")
    return panel, 0 if shared_x else M * K


def _conv_col2im_raw(gpanel, sh, S, shared_x):
    """The panel's gradient (S, M, K) fp32 -> gx (B, C, H, W) summed over the samples (shared x) or (S, B, C, H, W) (bnn_conv2d_col2im)."""
    gx = torch.empty((sh.B, sh.C, sh.H, sh.W) if shared_x else (S, sh.B, sh.C, sh.H, sh.W), dtype=torch.float32, device=gpanel.device)
    check(_lib.load().bnn_conv2d_col2im(ptr(gpanel), ctypes.byref(sh), S, int(shared_x), ptr(gx), stream_ptr(gpanel.device)), "bnn_conv2d_col2im")
    return gx


def _conv2d_torch_bwd(x, w, gy, shared_x, conv_args, need_x, need_w):
    """Where the panel does not apply (groups > 1, K % 8 != 0): torch's conv gradients per sample on explicit weights w (S, O, Cg,
    KH, KW) -> (gx, gw), None where not wanted; gx summed over the samples for a shared x."""
    gxs, gws = [], []
    for s in range(w.shape[0]):
        xs_ = x if shared_x else x[s]
        if need_x:
            gxs.append(torch.nn.grad.conv2d_input(xs_.shape, w[s], gy[s], *conv_args))
        if need_w:
            gws.append(torch.nn.grad.conv2d_weight(xs_, w[s].shape, gy[s], *conv_args))
    gx = (torch.stack(gxs).sum(0) if shared_x else torch.stack(gxs)) if need_x else None
    return gx, (torch.stack(gws) if need_w else None)


class _SampledConv2d(torch.autograd.Function):
    """y[s] = conv2d(x[s], w_s, b_s, ...) as an implicit GEMM with in-kernel draws
    (NormalConv2d.forward, conv.py:112-119)."""

    @staticmethod
    def forward(ctx, x, mu_w, rho_w, mu_b, rho_b, key_w, key_b, shared_x, conv_args, compute, track=True):
        # track: grad mode at the call (inside forward it is always off, and needs_input_grad only mirrors requires_grad)
        require_cuda_f32(x, "x")
        require_cuda_f32(mu_w, "weight.mean")
        require_cuda_f32(rho_w, "weight.scale")
        stride, padding, dilation, groups = conv_args
        S = key_w.nsamples
        xs = x.shape[-4:]
        if xs[1] != mu_w.shape[1] * groups:
            raise BnnHipError("conv2d: input has %d channels, weight expects %d" % (xs[1], mu_w.shape[1] * groups))
        sh, OH, OW = _conv_shape(xs, mu_w.shape, stride, padding, dilation, groups)
        if OH < 1 or OW < 1:
            raise BnnHipError("conv2d: kernel larger than padded input")
        y = torch.empty((S, sh.B, sh.O, OH, OW), dtype=torch.float32, device=x.device)
        per = sh.B * sh.C * sh.H * sh.W
        _lib.ensure_workspace(x.device)
        ctx.save_for_backward(x, mu_w, rho_w, rho_b if mu_b is not None else None)
        ctx.key_w, ctx.key_b, ctx.shared_x, ctx.conv_args, ctx.compute = key_w, key_b, shared_x, conv_args, compute
        if compute == _lib.COMPUTE_BF16 and DRAW_ONCE_BF16 and conv_dense_eligible(sh, OH, OW) and mu_w.data_ptr() % 16 == 0:
            # bf16 mode: weights drawn once (tap-major) for the S samples, then the implicit GEMM on them -- images resident
            # in LDS, im2col in the fragment addresses, no panel (csrc/bnn_dense.hip, k_conv_bf16)
            K = mu_w[0].numel()
            pre = draw_layers([(mu_w.reshape(sh.O, K), rho_w.reshape(sh.O, K), mu_b, rho_b, key_w, key_b, sh.KH * sh.KW)], S)[0]
            kp = pre.w.shape[2]
            check(_lib.load().bnn_conv2d_dense_forward(ptr(x), 0 if shared_x else per, ptr(pre.w), sh.O * kp, kp,
                                                        ptr(pre.b), sh.O if pre.b is not None else 0, ptr(y),
                                                        sh.B * sh.O * OH * OW, ctypes.byref(sh), S, 0, stream_ptr(x.device)),
                  "bnn_conv2d_dense_forward")
            return y
        needs_grad = track and any(ctx.needs_input_grad[:5])
        if (compute == _lib.COMPUTE_F32 and CONV_X3_F32 and not needs_grad and conv_dense_x3_eligible(sh, OH, OW) and
                mu_w.data_ptr() % 16 == 0):
            # fp32 parity mode, inference: the same implicit GEMM on three bf16 planes per operand -- weights drawn once as
            # planes (tap-major), images split into planes as they become resident in LDS, six plane pairs per 64-k block; no
            # im2col panel (the backward still takes the panel kernels, so training-time forwards stay on them)
            K = mu_w[0].numel()
            pre = draw_layers([(mu_w.reshape(sh.O, K), rho_w.reshape(sh.O, K), mu_b, rho_b, key_w, key_b, sh.KH * sh.KW)], S, x3=True)[0]
            kp = pre.w.shape[3]
            check(_lib.load().bnn_conv2d_dense_forward_x3(ptr(x), 0 if shared_x else per, ptr(pre.w), S * sh.O * kp, sh.O * kp, kp,
                                                           ptr(pre.b), sh.O if pre.b is not None else 0, ptr(y),
                                                           sh.B * sh.O * OH * OW, ctypes.byref(sh), S, 0, stream_ptr(x.device)),
                  "bnn_conv2d_dense_forward_x3")
            return y
        rw = _rng_struct(key_w, x.device)
        rb = _rng_struct(key_b, x.device) if mu_b is not None else None
        ws, wsb = _conv_workspace(sh, 1 if shared_x else S, compute, x.device)
        check(_lib.load().bnn_conv2d_forward_sampled(
            ptr(x), 0 if shared_x else per, ptr(mu_w), ptr(rho_w), ptr(mu_b), ptr(rho_b), ptr(y),
            sh.B * sh.O * OH * OW, ctypes.byref(sh), S, ctypes.byref(rw),
            ctypes.byref(rb) if rb is not None else None, compute, 0, ptr(ws), wsb, stream_ptr(x.device)),
            "bnn_conv2d_forward_sampled")
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mu_w, rho_w, rho_b = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.conv_args
        S = ctx.key_w.nsamples
        gy = gy.contiguous()
        need_x = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        need_b = rho_b is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        sh, OH, OW = _conv_shape(x.shape[-4:], mu_w.shape, stride, padding, dilation, groups)
        K = mu_w[0].numel()
        if groups == 1 and K % 8 == 0 and sh.O % 8 == 0:
            return _SampledConv2d._backward_panel(ctx, gy, sh, OH, OW, need_x, need_w, need_b)
        gx = g_mu_w = g_rho_w = g_mu_b = g_rho_b = None
        if need_x or need_w:
            w = _sample_affine_philox_raw(mu_w, rho_w, ctx.key_w)          # (S, O, Cg, KH, KW)
            gx, gw = _conv2d_torch_bwd(x, w, gy, ctx.shared_x, ctx.conv_args, need_x, need_w)
            if need_w:
                g_mu_w, g_rho_w = _sample_affine_bwd_raw(gw, rho_w, rho_w.numel(), S, key=ctx.key_w)
        if need_b:
            gb = gy.sum((1, 3, 4))
            g_mu_b, g_rho_b = _sample_affine_bwd_raw(gb, rho_b, rho_b.numel(), S, key=ctx.key_b)
        return gx, g_mu_w, g_rho_w, g_mu_b, g_rho_b, None, None, None, None, None, None

    @staticmethod
    def _backward_panel(ctx, gy, sh, OH, OW, need_x, need_w, need_b):
        """All-HIP backward through the im2col panel (include/bnn_hip.h, 'backward of K2 conv2d'): the conv is
        the linear layer rows = (image, pixel), so the linear backward kernels (re-drawn weights, fused
        draw-backward) do the work; only the layout changes (NCHW -> rows, col2im) are conv-specific."""
        x, mu_w, rho_w, rho_b = ctx.saved_tensors
        S, compute, dev = ctx.key_w.nsamples, ctx.compute, gy.device
        _lib.ensure_workspace(dev)
        P, O = OH * OW, sh.O
        M, K = sh.B * P, mu_w[0].numel()
        bf = compute == _lib.COMPUTE_BF16
        rows = _conv_rows_raw(gy, sh, P, S, bf)
        rw = _rng_struct(ctx.key_w, dev)
        gx = g_mu_w = g_rho_w = g_mu_b = g_rho_b = None
        aflag = _lib.FLAG_X_BF16 if bf else 0
        if need_w:
            panel, pstride = _conv_panel_raw(x, sh, M, K, S, ctx.shared_x, bf)
            g_mu_w, g_rho_w, g_mu_b, g_rho_b = _wgrad_sampled_raw(
                panel, pstride, rows, mu_w, rho_w, None, rho_b, rw, ctx.key_b, M, O, K, S, need_b, compute,
                aflag | (_lib.FLAG_Y_BF16 if bf else 0), kl_weight=True, kl_bias=False)
            need_b = False
        if need_x:
            gpanel = torch.empty((S, M, K), dtype=torch.float32, device=dev)
            if not _aligned16(mu_w, rho_w):     # the re-draw reads the posterior in 16-B pieces: a view at an odd offset is copied
                mu_w, rho_w = mu_w.clone(), rho_w.clone()
            check(_lib.load().bnn_linear_backward_input_sampled(ptr(rows), M * O, O, ptr(mu_w), ptr(rho_w), ptr(gpanel), M * K, K,
                                                                M, O, K, S, ctypes.byref(rw), compute, aflag, stream_ptr(dev)),
                  "bnn_linear_backward_input_sampled")
            gx = _conv_col2im_raw(gpanel, sh, S, ctx.shared_x)
        if need_b:
            gb = _colsum_raw(rows)                                          # (S, O)
            g_mu_b, g_rho_b = _sample_affine_bwd_raw(gb, rho_b, rho_b.numel(), S, key=ctx.key_b)
        return gx, g_mu_w, g_rho_w, g_mu_b, g_rho_b, None, None, None, None, None, None


def conv2d_flipout_eligible(x, mean, stride, padding, dilation, groups):
    """bf16 compute, inference: the one-launch Flipout conv (bnn_conv2d_flipout_forward) takes this layer."""
    if not (DRAW_ONCE_BF16 and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and mean.data_ptr() % 16 == 0):
        return False
    sh = _conv_shape(x.shape, mean.shape, stride, padding, dilation, groups)[0]
    return _conv_lds_images(sh, _lib.CONV_FLIPOUT) > 0


def conv2d_flipout(x, mean, scale, R, S, stride, padding, dilation):
    """FlipOutNormalConv2d.forward (conv.py:207-221) in two launches: the mean and the stddev written tap-major as bf16
    (bnn_draw_multi, kinds 1 / 2 -- no eps), then ONE implicit GEMM that shares the A fragment between the two
    contractions, with S flipped into its sign bits and R applied in the epilogue (no autograd: inference path)."""
    x = x.contiguous()
    require_cuda_f32(x, "x")
    O, C, KH, KW = mean.shape
    dev = x.device
    lib = _lib.load()
    w2 = flipout_conv_weights(mean, scale)
    kp = w2.shape[1]
    sh, OH, OW = _conv_shape(x.shape, mean.shape, stride, padding, dilation, 1)
    y = torch.empty((sh.B, O, OH, OW), dtype=torch.float32, device=dev)
    # the sign tensors broadcast over the batch like the reference's expand_as (conv.py:207-221): drawn for another batch size
    # (sample=False after the constructor's sample(1)) a (1, C, 1, 1) tensor serves every image
    Sf = S.to(torch.float32).expand(sh.B, C, 1, 1).reshape(sh.B, C).contiguous()
    Rf = R.to(torch.float32).expand(sh.B, O, 1, 1).reshape(sh.B, O).contiguous()
    check(lib.bnn_conv2d_flipout_forward(ptr(x), ptr(w2), kp, ptr(Sf), ptr(Rf), ptr(y), ctypes.byref(sh), 0, stream_ptr(dev)),
          "bnn_conv2d_flipout_forward")
    return y


def conv2d_flipout_x3_fused_eligible(x, mean, stride, padding, dilation):
    """ONE contraction launch for both of Flipout's convolutions in the fp32 parity mode (bnn_conv2d_flipout_forward_x3): the tile's
    columns are [O means | O stddevs], so 2 O = 64 or 128, and three planes of an image + the ring fit the LDS block."""
    if not (CONV_X3_F32 and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and mean.data_ptr() % 16 == 0):
        return False
    sh = _conv_shape(x.shape, mean.shape, stride, padding, dilation, 1)[0]
    return _conv_lds_images(sh, _lib.CONV_FLIPOUT_X3) > 0


def conv2d_flipout_x3_fused(x, mean, stddev, R, S, stride, padding, dilation):
    """FlipOutNormalConv2d.forward (conv.py:207-221) in the fp32 parity mode in TWO launches: mean and stddev as three bf16 planes,
    tap-major, stacked [O means | O stddevs] (bnn_draw_multi, kind 1), then ONE implicit GEMM on three-plane operands that shares the
    A fragment between the two contractions -- S in its sign bits, R in the epilogue (no autograd: inference path)."""
    x = x.contiguous()
    O, C, KH, KW = mean.shape
    K = C * KH * KW
    kp = _pad64(K)
    dev = x.device
    lib = _lib.load()
    w2 = torch.empty((3, 2 * O, kp), dtype=torch.bfloat16, device=dev)
    arr = (_lib.DrawTensor * 2)()
    srcs = (mean.detach().contiguous(), stddev.detach().contiguous())
    for i, src in enumerate(srcs):
        require_cuda_f32(src, "weight")
        _draw_slot(arr[i], src, None, O, K, w2.data_ptr() + i * O * kp * 2, kp, 2 * O * kp, _lib.BF16X3, _lib.DRAW_MEAN, KH * KW)
    _draw_launch(arr, 2, 1, dev)
    sh, OH, OW = _conv_shape(x.shape, mean.shape, stride, padding, dilation, 1)
    y = torch.empty((sh.B, O, OH, OW), dtype=torch.float32, device=dev)
    Sf = S.to(torch.float32).expand(sh.B, C, 1, 1).reshape(sh.B, C).contiguous()
    Rf = R.to(torch.float32).expand(sh.B, O, 1, 1).reshape(sh.B, O).contiguous()
    check(lib.bnn_conv2d_flipout_forward_x3(ptr(x), ptr(w2), 2 * O * kp, kp, ptr(Sf), ptr(Rf), ptr(y), ctypes.byref(sh), 0, stream_ptr(dev)),
          "bnn_conv2d_flipout_forward_x3")
    return y


def conv2d_flipout_x3(x, mean, stddev, R, S, stride, padding, dilation):
    """FlipOutNormalConv2d.forward (conv.py:207-221) in the fp32 parity mode without the im2col panel: mean and stddev as three
    bf16 planes each (ONE bnn_draw_multi launch, kind 1), two implicit-GEMM contractions (bnn_conv2d_dense_forward_x3), the sign
    tensors by torch (no autograd: inference path; the caller checked conv2d_plain_x3_eligible).  Shapes the one-launch form does not
    take (O = 128)."""
    x = x.contiguous()
    sh, OH, OW = _conv_shape(x.shape, mean.shape, stride, padding, dilation, 1)
    pm, ps = plain_conv_planes([mean.detach().contiguous(), stddev.detach().contiguous()])
    out = _conv_planes_raw(x, pm, None, sh, OH, OW)[0]
    noise = _conv_planes_raw((x * S.expand_as(x)).contiguous(), ps, None, sh, OH, OW)[0]
    return out + noise * R.expand_as(out)


def flipout_conv_weights(mean, scale):
    """[O rows of the mean | O rows of the stddev] as bf16, tap-major, rows zero-padded to a multiple of 64 columns: the
    weight operand of bnn_conv2d_flipout_forward (one bnn_draw_multi launch with kinds 1 / 2 -- no eps)."""
    mean, scale = mean.detach().contiguous(), scale.detach().contiguous()
    require_cuda_f32(mean, "weight.mean")
    require_cuda_f32(scale, "weight.scale")
    O, C, KH, KW = mean.shape
    K = C * KH * KW
    kp = _pad64(K)
    dev = mean.device
    w2 = torch.empty((2 * O, kp), dtype=torch.bfloat16, device=dev)
    arr = (_lib.DrawTensor * 2)()
    for i, kind in enumerate((_lib.DRAW_MEAN, _lib.DRAW_SIGMA)):
        _draw_slot(arr[i], mean, scale, O, K, w2.data_ptr() + i * O * kp * 2, kp, O * kp, _lib.BF16, kind, KH * KW)
    _draw_launch(arr, 2, 1, dev)
    return w2


def conv2d_sampled(x, mu_w, rho_w, mu_b, rho_b, key_w, key_b, shared_x, stride, padding, dilation, groups,
                   compute="f32"):
    return _SampledConv2d.apply(x.contiguous(), mu_w.contiguous(), rho_w.contiguous(),
                                None if mu_b is None else mu_b.contiguous(),
                                None if rho_b is None else rho_b.contiguous(),
                                key_w, key_b, shared_x,
                                (tuple(stride), tuple(padding), tuple(dilation), int(groups)),
                                _compute_code(compute), torch.is_grad_enabled())


class _PlainConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, shared_x, conv_args, compute):
        require_cuda_f32(x, "x")
        require_cuda_f32(w, "w")
        stride, padding, dilation, groups = conv_args
        S = w.shape[0]
        xs = x.shape[-4:]
        if xs[1] != w.shape[2] * groups:
            raise BnnHipError("conv2d: input has %d channels, weight expects %d" % (xs[1], w.shape[2] * groups))
        sh, OH, OW = _conv_shape(xs, w.shape[1:], stride, padding, dilation, groups)
        if OH < 1 or OW < 1:
            raise BnnHipError("conv2d: kernel larger than padded input")
        y = torch.empty((S, sh.B, sh.O, OH, OW), dtype=torch.float32, device=x.device)
        per = sh.B * sh.C * sh.H * sh.W
        wper = w[0].numel()
        _lib.ensure_workspace(x.device)
        ws, wsb = _conv_workspace(sh, 1 if shared_x else S, compute, x.device)
        check(_lib.load().bnn_conv2d_forward(ptr(x), 0 if shared_x else per, ptr(w), wper, ptr(b), sh.O, ptr(y),
                                              sh.B * sh.O * OH * OW, ctypes.byref(sh), S, compute, 0, ptr(ws), wsb,
                                              stream_ptr(x.device)), "bnn_conv2d_forward")
        ctx.save_for_backward(x, w)
        ctx.shared_x, ctx.conv_args, ctx.has_b = shared_x, conv_args, b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.conv_args
        S = w.shape[0]
        gy = gy.contiguous()
        gx = gw = gb = None
        sh, OH, OW = _conv_shape(x.shape[-4:], w.shape[1:], stride, padding, dilation, groups)
        K = w[0, 0].numel()
        if groups == 1 and K % 8 == 0:
            # all-HIP backward through the im2col panel (exact fp32 here: parity mode / Flipout): the conv is
            # F.linear on rows = (image, pixel), see include/bnn_hip.h 'backward of K2 conv2d'
            _lib.ensure_workspace(gy.device)
            P, O = OH * OW, sh.O
            M = sh.B * P
            rows = _conv_rows_raw(gy, sh, P, S, False)
            if ctx.needs_input_grad[1]:
                panel, pstride = _conv_panel_raw(x, sh, M, K, S, ctx.shared_x, False)
                gw = _wgrad_plain_raw(panel, pstride, rows, M, O, K, S).view_as(w)
            if ctx.needs_input_grad[0]:
                gpanel = _dgrad_plain_raw(rows, w.reshape(S, O, K), torch.float32)          # (S, M, K)
                gx = _conv_col2im_raw(gpanel, sh, S, ctx.shared_x)
            if ctx.has_b and ctx.needs_input_grad[2]:
                gb = _colsum_raw(rows)
            return gx, gw, gb, None, None, None
        gx, gw = _conv2d_torch_bwd(x, w, gy, ctx.shared_x, ctx.conv_args, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        if ctx.has_b and ctx.needs_input_grad[2]:
            gb = gy.sum((1, 3, 4))
        return gx, gw, gb, None, None, None


def plain_conv_planes(ws):
    """Explicit conv weights, each (O, C, KH, KW) fp32, as the three-plane tap-major operands of bnn_conv2d_dense_forward_x3:
    (3, 1, O, kp) bf16 each -- ONE bnn_draw_multi launch (kind 1: the tensor as it is, no draw)."""
    dev = ws[0].device
    arr = (_lib.DrawTensor * len(ws))()
    outs = []
    for i, w in enumerate(ws):
        require_cuda_f32(w, "w")
        O, C, KH, KW = w.shape
        K = C * KH * KW
        kp = _pad64(K)
        out = torch.empty((3, 1, O, kp), dtype=torch.bfloat16, device=dev)
        _draw_slot(arr[i], w, None, O, K, out.data_ptr(), kp, O * kp, _lib.BF16X3, _lib.DRAW_MEAN, KH * KW)
        outs.append(out)
    _draw_launch(arr, len(ws), 1, dev)
    return outs


def _conv_planes_raw(x, planes, b, sh, OH, OW):
    """conv2d of x (B, C, H, W) fp32 with ONE explicit weight given as planes (plain_conv_planes) in the fp32 parity mode:
    the implicit GEMM on three bf16 planes per operand, no im2col panel -> (1, B, O, OH, OW)."""
    kp = planes.shape[3]
    y = torch.empty((1, sh.B, sh.O, OH, OW), dtype=torch.float32, device=x.device)
    check(_lib.load().bnn_conv2d_dense_forward_x3(ptr(x), 0, ptr(planes), sh.O * kp, sh.O * kp, kp, ptr(b), sh.O if b is not None else 0,
                                                   ptr(y), sh.B * sh.O * OH * OW, ctypes.byref(sh), 1, 0, stream_ptr(x.device)),
          "bnn_conv2d_dense_forward_x3")
    return y


def conv2d_plain_x3_eligible(x, w, stride, padding, dilation, groups, compute):
    """fp32 parity mode, no gradient wanted, one explicit weight (S = 1) of a shape the three-plane implicit GEMM takes."""
    if not (CONV_X3_F32 and _compute_code(compute) == _lib.COMPUTE_F32 and x.is_cuda and x.dim() == 4 and w.dim() == 5 and w.shape[0] == 1):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        return False
    if x.dtype != torch.float32 or w.dtype != torch.float32 or x.shape[1] != w.shape[2] * groups:
        return False
    sh, OH, OW = _conv_shape(x.shape, w.shape[1:], stride, padding, dilation, groups)
    return OH >= 1 and OW >= 1 and conv_dense_x3_eligible(sh, OH, OW)


def conv2d_plain(x, w, b, shared_x, stride, padding, dilation, groups, compute="f32"):
    bias_grad = torch.is_grad_enabled() and b is not None and b.requires_grad        # (then autograd must see the call)
    if shared_x and not bias_grad and conv2d_plain_x3_eligible(x, w, stride, padding, dilation, groups, compute):
        # inference in the fp32 parity mode: no panel (FlipOutNormalConv2d's two contractions, MC-dropout-free plain layers)
        x, w0 = x.contiguous(), w[0].detach().contiguous()
        if w0.data_ptr() % 16 == 0 and (b is None or b.is_cuda):
            sh, OH, OW = _conv_shape(x.shape, w0.shape, stride, padding, dilation, groups)
            return _conv_planes_raw(x, plain_conv_planes([w0])[0], None if b is None else b.detach().contiguous().float(), sh, OH, OW)
    return _PlainConv2d.apply(x.contiguous(), w.contiguous(), None if b is None else b.contiguous(), shared_x,
                              (tuple(stride), tuple(padding), tuple(dilation), int(groups)),
                              _compute_code(compute))


# --------------------------------------------------------------------------- conv3d (NormalConv3d on the device)
def _conv3d_shape(x_shape, w_shape, stride, padding, dilation, groups):
    """-> (bnn_conv3d_shape_t, (OD, OH, OW)) of conv3d(x (B, C, D, H, W), w (O, C/groups, KD, KH, KW)).  BnnHipError where torch's
    conv3d refuses too: a channel count that does not match, a kernel larger than the padded input.  Host arithmetic only."""
    B, C, D, H, W = (int(v) for v in x_shape)
    O, Cg, KD, KH, KW = (int(v) for v in w_shape)
    groups = int(groups)
    if groups < 1 or C != Cg * groups or O % groups != 0:
        raise BnnHipError("conv3d: input has %d channels, weight (%d, %d, ...) with groups=%d expects %d" % (C, O, Cg, groups, Cg * groups))
    out = []
    for n, k, s, p, d in zip((D, H, W), (KD, KH, KW), stride, padding, dilation):
        span = int(d) * (k - 1) + 1
        if n + 2 * int(p) < span:
            raise BnnHipError("conv3d: kernel larger than padded input")
        out.append((n + 2 * int(p) - span) // int(s) + 1)
    sh = _lib.Conv3dShape(B, C, D, H, W, O, KD, KH, KW, *(int(v) for v in stride), *(int(v) for v in padding),
                          *(int(v) for v in dilation), groups)
    return sh, tuple(out)


def _conv3d_operands(mu_w, rho_w, mu_b, rho_b, key_w, key_b, compute):
    """The contraction's weight (and bias) operands -> (w, w_sample_stride, b, b_sample_stride).
    Keyed: the S draws of the posterior in ONE bnn_draw_multi launch -- the weight as one flat row per sample (rows = 1: the eps
    order is K1's and the draw's cols % 4 rule does not apply), bf16 with the row padded to a multiple of 8 or fp32, the bias fp32.
    Explicit (key_w None): mu_w / mu_b are the weight and bias of every sample (sample stride 0); bf16 mode rounds the weight with
    a kind-1 draw (the tensor as it is)."""
    dev = mu_w.device
    n = mu_w.numel()
    bf = compute == _lib.COMPUTE_BF16
    if key_w is None and not bf:
        return mu_w, 0, mu_b, 0
    ld = (n + 7) // 8 * 8 if bf else n
    S = key_w.nsamples if key_w is not None else 1
    w = torch.empty((S, ld), dtype=torch.bfloat16 if bf else torch.float32, device=dev)
    arr = (_lib.DrawTensor * 2)()
    if key_w is not None:
        _draw_slot(arr[0], mu_w, rho_w, 1, n, w.data_ptr(), ld, ld, _lib.BF16 if bf else _lib.F32, key=key_w)
    else:
        _draw_slot(arr[0], mu_w, None, 1, n, w.data_ptr(), ld, ld, _lib.BF16, _lib.DRAW_MEAN)
    cnt, b = 1, (mu_b if key_w is None else None)
    if key_w is not None and mu_b is not None:
        nb = mu_b.numel()
        b = torch.empty((S, nb), dtype=torch.float32, device=dev)
        _draw_slot(arr[1], mu_b, rho_b, 1, nb, b.data_ptr(), nb, nb, _lib.F32, key=key_b)
        cnt = 2
    _draw_launch(arr, cnt, S, dev)
    return w, (ld if key_w is not None else 0), b, (0 if key_w is None or b is None else b.shape[1])


class _Conv3d(torch.autograd.Function):
    """y[s] = conv3d(x[s | 0], w_s, b_s, ...) for S samples on the implicit GEMMs of csrc/bnn_conv3d.hip (NormalConv3d.forward,
    conv.py:138-142): one draw launch + one contraction launch.  Keyed (key_w given): w_s, b_s are the draws of the posterior on
    the keys; the backward re-draws them from the keys (nothing drawn is saved) and takes g_mu / g_rho from bnn_sample_affine_bwd.
    Explicit (key_w None): mu_w / mu_b are the weight and bias of every sample."""

    @staticmethod
    def forward(ctx, x, mu_w, rho_w, mu_b, rho_b, key_w, key_b, S, shared_x, conv_args, compute):
        require_cuda_f32(x, "x")
        require_cuda_f32(mu_w, "weight")
        for t, name in ((rho_w, "weight.scale"), (mu_b, "bias"), (rho_b, "bias.scale")):
            if t is not None:
                require_cuda_f32(t, name)
        stride, padding, dilation, groups = conv_args
        if x.dim() != (5 if shared_x else 6) or (not shared_x and x.shape[0] != S):
            raise BnnHipError("conv3d: x must be (B, C, D, H, W) shared by the samples or (S, B, C, D, H, W), got %s" % (tuple(x.shape),))
        sh, (OD, OH, OW) = _conv3d_shape(x.shape[-5:], mu_w.shape, stride, padding, dilation, groups)
        dev = x.device
        w, w_ss, b, b_ss = _conv3d_operands(mu_w, rho_w, mu_b, rho_b, key_w, key_b, compute)
        y = torch.empty((S, sh.B, sh.O, OD, OH, OW), dtype=torch.float32, device=dev)
        check(_lib.load().bnn_conv3d_forward_drawn(ptr(x), 0 if shared_x else x[0].numel(), ptr(w), w_ss, ptr(b), b_ss, ptr(y),
                                                   ctypes.byref(sh), S, compute, stream_ptr(dev)), "bnn_conv3d_forward_drawn")
        ctx.save_for_backward(x, mu_w, rho_w, mu_b, rho_b)
        ctx.key_w, ctx.key_b, ctx.S, ctx.shared_x, ctx.sh, ctx.compute = key_w, key_b, S, shared_x, sh, compute
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mu_w, rho_w, mu_b, rho_b = ctx.saved_tensors
        S, sh, compute, dev = ctx.S, ctx.sh, ctx.compute, gy.device
        lib, st = _lib.load(), stream_ptr(dev)
        keyed = ctx.key_w is not None
        need_x = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        need_b = mu_b is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        gy = gy.contiguous()
        gx = g_mu_w = g_rho_w = g_mu_b = g_rho_b = None
        if need_x:
            w, w_ss, _, _ = _conv3d_operands(mu_w, rho_w, None, None, ctx.key_w, None, compute)
            gx = torch.empty(x.shape, dtype=torch.float32, device=dev)
            check(lib.bnn_conv3d_backward_input(ptr(gy), ptr(w), w_ss, ptr(gx), int(ctx.shared_x), ctypes.byref(sh), S, compute, st),
                  "bnn_conv3d_backward_input")
        if need_w or need_b:
            O, K = sh.O, mu_w[0].numel()
            gw = torch.empty((S, O, K), dtype=torch.float32, device=dev) if need_w else None
            gb = torch.empty((S, O), dtype=torch.float32, device=dev) if need_b else None
            nb = lib.bnn_conv3d_backward_weight_workspace_bytes(ctypes.byref(sh), S) if need_w else 0
            ws = torch.empty(nb, dtype=torch.uint8, device=dev) if nb > 0 else None     # this call's own slabs
            check(lib.bnn_conv3d_backward_weight(ptr(x), 0 if ctx.shared_x else x[0].numel(), ptr(gy), ptr(gw), ptr(gb),
                                                 ctypes.byref(sh), S, compute, ptr(ws), nb, st), "bnn_conv3d_backward_weight")
            if need_w:
                if keyed:
                    g_mu_w, g_rho_w = _sample_affine_bwd_raw(gw, rho_w, rho_w.numel(), S, key=ctx.key_w)
                else:
                    g_mu_w = gw.sum(0).reshape(mu_w.shape)
            if need_b:
                if keyed:
                    g_mu_b, g_rho_b = _sample_affine_bwd_raw(gb, rho_b, rho_b.numel(), S, key=ctx.key_b)
                else:
                    g_mu_b = gb.sum(0)
        return gx, g_mu_w, g_rho_w, g_mu_b, g_rho_b, None, None, None, None, None, None


def conv3d_sampled(x, mu_w, rho_w, mu_b, rho_b, key_w, key_b, shared_x, stride, padding, dilation, groups, compute="f32"):
    """NormalConv3d on the device for the key's S MC samples: x (B, C, D, H, W) shared by them (shared_x) or (S, B, C, D, H, W)
    -> (S, B, O, OD, OH, OW) fp32.  Draw + contraction: two launches; autograd to x and the four posterior tensors."""
    return _Conv3d.apply(x.contiguous(), mu_w.contiguous(), rho_w.contiguous(),
                         None if mu_b is None else mu_b.contiguous(), None if rho_b is None else rho_b.contiguous(),
                         key_w, key_b, key_w.nsamples, bool(shared_x),
                         (tuple(stride), tuple(padding), tuple(dilation), int(groups)), _compute_code(compute))


def conv3d_plain(x, w, b, nsamples, shared_x, stride, padding, dilation, groups, compute="f32"):
    """conv3d_sampled on ONE explicit weight (O, C/groups, KD, KH, KW) and bias (O,) or None for all `nsamples` samples (a layer
    whose weights were set rather than keyed, e.g. WeightNormal.sample_with_eps); autograd to x, w and b."""
    return _Conv3d.apply(x.contiguous(), w.contiguous(), None, None if b is None else b.contiguous(), None, None, None,
                         int(nsamples), bool(shared_x), (tuple(stride), tuple(padding), tuple(dilation), int(groups)),
                         _compute_code(compute))


# --------------------------------------------------------------------------- K11: local reparameterization, convolutions
def _lrt_conv_views(x_shape, w_shape, stride, padding, dilation):
    """A 1-d / 2-d / 3-d conv as the 3-d one on unit depth / height: -> (image shape (C, D, H, W), weight shape
    (O, C / groups, KD, KH, KW), stride, padding, dilation) with x_shape = (..., C, *spatial)."""
    nd = len(w_shape) - 2
    if nd not in (1, 2, 3):
        raise BnnHipError("conv_lrt: weight must be (O, C / groups, *kernel) with 1, 2 or 3 kernel axes, got %s" % (tuple(w_shape),))
    if len(stride) != nd or len(padding) != nd or len(dilation) != nd:
        raise BnnHipError("conv_lrt: stride, padding and dilation must have %d entries" % nd)
    one = (1,) * (3 - nd)
    img = (int(x_shape[-nd - 1]),) + one + tuple(int(v) for v in x_shape[-nd:])
    w5 = tuple(int(v) for v in w_shape[:2]) + one + tuple(int(v) for v in w_shape[2:])
    return (img, w5, one + tuple(int(v) for v in stride), (0,) * (3 - nd) + tuple(int(v) for v in padding),
            one + tuple(int(v) for v in dilation))


def conv_lrt_eligible(x, mu_w, nsamples, shared_x, stride, padding, dilation, groups):
    """None when the K11 entries take the call, else the reason they refuse (layout, K7's index ranges).  x: (B, C, *spatial) for
    a shared input or (S, B, C, *spatial); there is no torch fallback on device tensors -- convNd_lrt raises with this reason."""
    nd = mu_w.dim() - 2
    if nd not in (1, 2, 3):
        return "weight has %d kernel axes (1, 2 or 3)" % nd
    if x.dim() != nd + (2 if shared_x else 3) or (not shared_x and x.shape[0] != nsamples):
        return "input must be (B, C, ...) shared by the samples or (S = %d, B, C, ...) with %d spatial axes, got %s" % (
            nsamples, nd, tuple(x.shape))
    if x.dtype != torch.float32:
        return "input dtype %s (float32)" % x.dtype
    if x.data_ptr() % 4:
        return "input pointer is not aligned to its element size"
    if nsamples < 1 or nsamples > 0xFFFF:
        return "%d MC samples (1 .. 65535)" % nsamples
    try:
        img, w5, st, pd, dl = _lrt_conv_views(x.shape, mu_w.shape, stride, padding, dilation)
        sh, _ = _conv3d_shape((int(x.shape[-nd - 2]),) + img, w5, st, pd, dl, groups)
    except BnnHipError as e:
        return str(e)
    lib = _lib.load()
    if lib.bnn_conv3d_lrt_backward_weight_workspace_bytes(ctypes.byref(sh), int(nsamples)) < 0:
        return lib.bnn_last_error().decode()
    return None


class _LrtConv(torch.autograd.Function):
    """y_s = m + sqrt(v + 1e-16) eps_s, m = convNd(x, mean_w, mu_b), v = convNd(x^2, s2_w, sigma_b^2) (LocalReparamConvNd,
    VariationalDropoutConvNd): the posterior's operand launch (post.prepare: s2_w, sigma_b^2, with a threshold the masked planes) +
    one paired-contraction launch for all S samples (csrc/bnn_conv3d.hip, k_lrt_conv3d).  Backward: eps re-created from the key in
    one elementwise launch (g_m, g_v from the saved v; K10's, with N = O P), the paired input-gradient launch, the paired
    weight-gradient slabs + their reduce, the bias sums (post.conv_wgrad) -- 5 launches with a bias, 4 without, no torch conv."""

    @staticmethod
    def forward(ctx, x, mean_w, par_w, mu_b, rho_b, key, shared_x, conv_args, compute, track, post, threshold):
        who = "conv_" + post.name
        require_cuda_f32(x, "x")
        post.check(mean_w, par_w, mu_b, rho_b, conv=True)
        stride, padding, dilation, groups = conv_args
        S = key.nsamples
        why = conv_lrt_eligible(x, mean_w, S, shared_x, stride, padding, dilation, groups)
        if why is not None:
            raise BnnHipError(who + ": " + why)
        _lrt_refuse_masked_grad(who, ctx, track, threshold)
        nd = mean_w.dim() - 2
        img, w5, st, pd, dl = _lrt_conv_views(x.shape, mean_w.shape, stride, padding, dilation)
        B = int(x.shape[-nd - 2])
        sh, out3 = _conv3d_shape((B,) + img, w5, st, pd, dl, groups)
        out_sp = out3[3 - nd:]
        dev = x.device
        needs_grad = track and any(ctx.needs_input_grad[:5])
        mean, s2_w, s2_b = post.prepare(mean_w, par_w, rho_b if mu_b is not None else None, threshold)
        y = torch.empty((S, B, sh.O) + out_sp, dtype=torch.float32, device=dev)
        v = torch.empty(((B, sh.O) if shared_x else (S, B, sh.O)) + out_sp, dtype=torch.float32, device=dev) if needs_grad else None
        r = _rng_struct(key, dev)
        check(_lib.load().bnn_conv3d_lrt_forward(ptr(x), 0 if shared_x else x[0].numel(), ptr(mean), ptr(s2_w), ptr(mu_b), ptr(s2_b),
                                                 ptr(y), ptr(v), ctypes.byref(sh), S, ctypes.byref(r), compute, stream_ptr(dev)),
              "bnn_conv3d_lrt_forward")
        if needs_grad:
            # (mean: with a threshold the masked plane -- then only the input's gradient is ever asked for, through the masked layer)
            ctx.save_for_backward(x, mean, par_w, rho_b if mu_b is not None else None, s2_w, v)
        ctx.post, ctx.key, ctx.shared_x, ctx.compute, ctx.sh = post, key, shared_x, compute, sh
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mean_w, par_w, rho_b, s2_w, v = ctx.saved_tensors
        S, compute, shared, sh = ctx.key.nsamples, ctx.compute, ctx.shared_x, ctx.sh
        dev = gy.device
        lib, st = _lib.load(), stream_ptr(dev)
        gy = gy.contiguous().float()
        nsets = 1 if shared else S
        g_m, g_v = torch.empty_like(v), torch.empty_like(v)
        r = _rng_struct(ctx.key, dev)
        check(lib.bnn_lrt_backward_epilogue(ptr(gy), ptr(v), ptr(g_m), ptr(g_v), sh.B, v[0].numel() if shared else v[0][0].numel(),
                                            S, 1 if shared else 0, ctypes.byref(r), 0, st), "bnn_lrt_backward_epilogue")
        gx = g_mean_w = g_par_w = g_mu_b = g_rho_b = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            check(lib.bnn_conv3d_lrt_backward_input(ptr(g_m), ptr(g_v), ptr(mean_w), ptr(s2_w), ptr(x), ptr(gx), ctypes.byref(sh),
                                                    nsets, compute, st), "bnn_conv3d_lrt_backward_input")
        need_b = rho_b is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or need_b:
            g_mean_w, g_par_w = torch.empty_like(mean_w), torch.empty_like(par_w)
            if need_b:
                g_mu_b, g_rho_b = torch.empty_like(rho_b), torch.empty_like(rho_b)
            nb = lib.bnn_conv3d_lrt_backward_weight_workspace_bytes(ctypes.byref(sh), nsets)
            ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)          # this call's own slabs
            check(getattr(lib, ctx.post.conv_wgrad)(ptr(x), ptr(g_m), ptr(g_v), ptr(par_w), ptr(g_mean_w), ptr(g_par_w),
                                                    ptr(rho_b) if need_b else None, ptr(g_mu_b), ptr(g_rho_b), ctypes.byref(sh),
                                                    nsets, compute, ptr(ws), nb, st), ctx.post.conv_wgrad)
        return gx, g_mean_w, g_par_w, g_mu_b, g_rho_b, None, None, None, None, None, None, None


def _convNd_lrt(post, x, mean_w, par_w, mu_b, rho_b, key, shared_x, stride, padding, dilation, groups, compute, threshold=None):
    return _LrtConv.apply(x.contiguous(), mean_w.contiguous(), par_w.contiguous(),
                          None if mu_b is None else mu_b.contiguous(), None if rho_b is None else rho_b.contiguous(),
                          key, bool(shared_x), (tuple(stride), tuple(padding), tuple(dilation), int(groups)),
                          _compute_code(compute), torch.is_grad_enabled(), post, None if threshold is None else float(threshold))


def convNd_lrt(x, mu_w, rho_w, mu_b, rho_b, key, shared_x, stride, padding, dilation, groups=1, compute="f32"):
    """LocalReparamConv{1,2,3}d on the device (the dimension is the weight's): x (B, C, *spatial) shared by the key's S samples
    (shared_x) or (S, B, C, *spatial) -> (S, B, O, *out_spatial) fp32; sample s uses eps[(b O + o) P + p] of the key's sample
    sample0 + s.  Raises BnnHipError (with conv_lrt_eligible's reason) for a call the kernel refuses: no torch fallback."""
    return _convNd_lrt(_GAUSSIAN, x, mu_w, rho_w, mu_b, rho_b, key, shared_x, stride, padding, dilation, groups, compute)


# --------------------------------------------------------------------------- K24: sparse variational dropout, convolutions
def convNd_vd(x, theta, log_sigma2, mu_b, rho_b, key, shared_x, stride, padding, dilation, groups=1, compute="f32", threshold=None):
    """VariationalDropoutConv{1,2,3}d on the device (the dimension is the weight's): convNd_lrt on the posterior
    N(theta, exp(log_sigma2)) -- x (B, C, *spatial) shared by the key's S samples (shared_x) or (S, B, C, *spatial) ->
    (S, B, O, *out_spatial) fp32, y_s = m + sqrt(v + 1e-16) eps_s with m = convNd(x, theta, mu_b), v = convNd(x^2,
    exp(log_sigma2), sigma_b^2); sample s uses eps[(b O + o) P + p] of the key's sample sample0 + s (the LRT-conv noise contract).
    threshold: a float drops the weights with log_alpha > threshold (theta = 0, variance 0: bnn_vd_prepare's masked planes) --
    inference only: a call that would need a gradient of a posterior tensor raises BnnHipError.  Raises BnnHipError (with
    conv_lrt_eligible's reason) for a call the kernel refuses: no torch fallback."""
    _vd_refuse_masked_grad("convNd_vd", threshold, theta, log_sigma2, mu_b, rho_b)
    return _convNd_lrt(_LOG_SIGMA2, x, theta, log_sigma2, mu_b, rho_b, key, shared_x, stride, padding, dilation, groups, compute,
                       threshold)


# --------------------------------------------------------------------------- Flipout conv3d (FlipOutNormalConv3d on the device)
def _flip3d_operands(mean, scale, compute):
    """[O K mean | O K stddev] (OIDHW order, stddev = 1e-10 + softplus(scale)) in ONE bnn_draw_multi launch (kinds 1 / 2, one flat
    row each): bf16 rows padded to a multiple of 8, or fp32 rows -> (2, ld)."""
    dev = mean.device
    n = mean.numel()
    bf = compute == _lib.COMPUTE_BF16
    ld = (n + 7) // 8 * 8 if bf else n
    w = torch.empty((2, ld), dtype=torch.bfloat16 if bf else torch.float32, device=dev)
    arr = (_lib.DrawTensor * 2)()
    for i, kind in enumerate((_lib.DRAW_MEAN, _lib.DRAW_SIGMA)):
        _draw_slot(arr[i], mean, scale, 1, n, w.data_ptr() + i * ld * w.element_size(), ld, ld, _lib.BF16 if bf else _lib.F32, kind)
    _draw_launch(arr, 2, 1, dev)
    return w


def conv3d_flipout_eligible(x_shape, mean_shape, nsamples, stride, padding, dilation, groups):
    """The Flipout conv3d entries take this shape (groups == 1, K7's index ranges, B (O + C) < 2^31) -- host arithmetic only.
    False: the caller keeps the torch expression."""
    if int(groups) != 1 or len(x_shape) != 5 or len(mean_shape) != 5:
        return False
    try:
        sh, _ = _conv3d_shape(x_shape, mean_shape, stride, padding, dilation, groups)
    except BnnHipError:
        return False
    return _lib.load().bnn_conv3d_flipout_backward_weight_workspace_bytes(ctypes.byref(sh), int(nsamples)) >= 0


class _FlipoutConv3d(torch.autograd.Function):
    """y[s][b] = conv3d(x[s | 0][b], mean) + R_s[b] (.) conv3d(x[s | 0][b] (.) S_s[b], stddev) (FlipOutNormalConv3d.forward,
    conv.py:237-251, groups == 1) for S samples on csrc/bnn_conv3d.hip's Flipout tiles: one operand draw + one contraction launch.
    signs (S | 1, B, O + C): R then S per example (bnn_flipout_signs' conv layout), saved for the backward.  Backward: the operands
    again (one draw), one input-gradient launch, one slab launch + one reduce for d/d mean and d/d scale."""

    @staticmethod
    def forward(ctx, x, mean, scale, signs, S, shared_x, conv_args, compute):
        require_cuda_f32(x, "x")
        require_cuda_f32(mean, "weight.mean")
        require_cuda_f32(scale, "weight.scale")
        require_cuda_f32(signs, "signs")
        stride, padding, dilation = conv_args
        if x.dim() != (5 if shared_x else 6) or (not shared_x and x.shape[0] != S):
            raise BnnHipError("conv3d_flipout: x must be (B, C, D, H, W) shared by the samples or (S, B, C, D, H, W), got %s"
                              % (tuple(x.shape),))
        sh, (OD, OH, OW) = _conv3d_shape(x.shape[-5:], mean.shape, stride, padding, dilation, 1)
        OC = sh.O + sh.C
        if signs.numel() not in (sh.B * OC, S * sh.B * OC):
            raise BnnHipError("conv3d_flipout: signs must hold (1 or %d) x %d x %d values, got %s" % (S, sh.B, OC, tuple(signs.shape)))
        sg_ss = 0 if signs.numel() == sh.B * OC else sh.B * OC
        dev = x.device
        w = _flip3d_operands(mean, scale, compute)
        y = torch.empty((S, sh.B, sh.O, OD, OH, OW), dtype=torch.float32, device=dev)
        check(_lib.load().bnn_conv3d_flipout_forward(ptr(x), 0 if shared_x else x[0].numel(), ptr(w), ptr(signs), sg_ss, ptr(y),
                                                     ctypes.byref(sh), S, compute, stream_ptr(dev)), "bnn_conv3d_flipout_forward")
        ctx.save_for_backward(x, mean, scale, signs)
        ctx.S, ctx.shared_x, ctx.sh, ctx.compute, ctx.sg_ss = S, shared_x, sh, compute, sg_ss
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mean, scale, signs = ctx.saved_tensors
        S, sh, compute, sg_ss, dev = ctx.S, ctx.sh, ctx.compute, ctx.sg_ss, gy.device
        lib, st = _lib.load(), stream_ptr(dev)
        gy = gy.contiguous()
        gx = g_mean = g_scale = None
        if ctx.needs_input_grad[0]:
            w = _flip3d_operands(mean, scale, compute)
            gx = torch.empty(x.shape, dtype=torch.float32, device=dev)
            check(lib.bnn_conv3d_flipout_backward_input(ptr(gy), ptr(w), ptr(signs), sg_ss, ptr(gx), int(ctx.shared_x),
                                                        ctypes.byref(sh), S, compute, st), "bnn_conv3d_flipout_backward_input")
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            g_mean, g_scale = torch.empty_like(mean), torch.empty_like(scale)
            nb = lib.bnn_conv3d_flipout_backward_weight_workspace_bytes(ctypes.byref(sh), S)
            ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)          # this call's own slabs
            check(lib.bnn_conv3d_flipout_backward_weight(ptr(x), 0 if ctx.shared_x else x[0].numel(), ptr(gy), ptr(signs), sg_ss,
                                                         ptr(scale), ptr(g_mean), ptr(g_scale), ctypes.byref(sh), S, compute,
                                                         ptr(ws), nb, st), "bnn_conv3d_flipout_backward_weight")
        return gx, g_mean, g_scale, None, None, None, None, None


def conv3d_flipout(x, mean, scale, signs, nsamples, shared_x, stride, padding, dilation, compute="f32"):
    """FlipOutNormalConv3d on the device for `nsamples` MC samples: x (B, C, D, H, W) shared by them (shared_x) or
    (S, B, C, D, H, W), signs (S | 1, B, O + C) fp32 +-1 (R then S per example; one set is used by every sample) -> (S, B, O, OD,
    OH, OW) fp32.  Draw + contraction: two launches; autograd to x, mean and scale.  groups == 1 (conv3d_flipout_eligible)."""
    return _FlipoutConv3d.apply(x.contiguous(), mean.contiguous(), scale.contiguous(), signs.detach().contiguous(), int(nsamples),
                                bool(shared_x), (tuple(stride), tuple(padding), tuple(dilation)), _compute_code(compute))


# --------------------------------------------------------------------------- MultivariateNormalLinear (MVN-noise contract)
def _mvn_extent(mu, scale):
    """(rows, cols) of a full-covariance posterior: mean (..., K), scale (..., K, K)."""
    require_cuda_f32(mu, "mean")
    require_cuda_f32(scale, "scale")
    K = mu.shape[-1]
    if tuple(scale.shape) != tuple(mu.shape) + (K,):
        raise BnnHipError("mvn: scale has shape %s, the mean %s needs %s" % (tuple(scale.shape), tuple(mu.shape),
                                                                             tuple(mu.shape) + (K,)))
    return mu.numel() // K, K


def _mvn_descs(mus, scales, keys, S, outs=None, gws=None, g_mus=None, g_scales=None):
    arr = (_lib.MvnTensor * len(mus))()
    for i, (m, sc, k) in enumerate(zip(mus, scales, keys)):
        rows, K = _mvn_extent(m, sc)
        t = arr[i]
        t.mu, t.scale, t.rows, t.cols, t.sample_stride = m.data_ptr(), sc.data_ptr(), rows, K, rows * K
        if outs is not None:
            t.out = outs[i].data_ptr()
        if gws is not None:
            t.g_w, t.g_mu, t.g_scale = gws[i].data_ptr(), g_mus[i].data_ptr(), g_scales[i].data_ptr()
        if k.nsamples != S:
            raise BnnHipError("mvn: the keys of one draw must have the same number of samples")
        t.rng = _rng_struct(k, m.device)
    return arr


def _mvn_draw_raw(mus, scales, keys):
    S = keys[0].nsamples
    outs = [torch.empty((S,) + tuple(m.shape), dtype=torch.float32, device=m.device) for m in mus]
    arr = _mvn_descs(mus, scales, keys, S, outs=outs)
    check(_lib.load().bnn_mvn_draw(arr, len(mus), S, stream_ptr(mus[0].device)), "bnn_mvn_draw")
    return outs


def mvn_draw(mu, scale, key):
    """The keyed draws w_s = mu + L u_s of the key's nsamples MC samples (MVN-noise contract, include/bnn_hip.h): mu (O, K) with
    scale (O, K, K), or a bias (O,) with (O, O) -> (S, *mu.shape) fp32.  One bnn_mvn_draw launch, no autograd."""
    return _mvn_draw_raw([mu.detach().contiguous()], [scale.detach().contiguous()], [key])[0]


class _MvnDraw(torch.autograd.Function):
    """(w_s for each tensor) = mu + tril(sqrt(softplus(scale) + 1e-10 I)) u_s with keyed uniforms: bnn_mvn_draw forward (every
    tensor in one launch), bnn_mvn_draw_backward backward (the uniforms re-created from the keys)."""

    @staticmethod
    def forward(ctx, keys, *params):
        T = len(keys)
        mus, scales = [p.detach() for p in params[:T]], [p.detach() for p in params[T:]]
        outs = _mvn_draw_raw(mus, scales, keys)
        ctx.save_for_backward(*params)
        ctx.keys = keys
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        params = ctx.saved_tensors
        T = len(ctx.keys)
        mus, scales = params[:T], params[T:]
        S = ctx.keys[0].nsamples
        gws = [g.contiguous().float() if g is not None else torch.zeros((S,) + tuple(m.shape), device=m.device)
               for g, m in zip(gs, mus)]
        g_mus = [torch.empty_like(m) for m in mus]
        g_scales = [torch.empty_like(sc) for sc in scales]
        arr = _mvn_descs(mus, scales, ctx.keys, S, gws=gws, g_mus=g_mus, g_scales=g_scales)
        check(_lib.load().bnn_mvn_draw_backward(arr, T, S, stream_ptr(mus[0].device)), "bnn_mvn_draw_backward")
        return (None,) + tuple(g_mus) + tuple(g_scales)


def mvn_draw_layer(mu_w, scale_w, mu_b, scale_b, key_w, key_b):
    """A MultivariateNormalLinear's weight (S, O, K) and bias (S, O) (or None) for the keys' samples, in ONE launch, with autograd."""
    if mu_b is None:
        return _MvnDraw.apply((key_w,), mu_w.contiguous(), scale_w.contiguous())[0], None
    w, b = _MvnDraw.apply((key_w, key_b), mu_w.contiguous(), mu_b.contiguous(), scale_w.contiguous(), scale_b.contiguous())
    return w, b


def mvn_isotropic(prior):
    """(m0, sigma0) if `prior` is MultivariateNormal(loc = m0 everywhere, scale_tril = sigma0 I), else None.  Checked once per
    prior object (its tensors are (O, K, K) on the host) and cached on it."""
    cached = prior.__dict__.get("_bnn_isotropic", False)
    if cached is not False:
        return cached
    from torch.distributions import MultivariateNormal
    iso = None
    if isinstance(prior, MultivariateNormal):
        loc = prior.loc.detach().double().cpu()
        tril = prior.scale_tril.detach().double().cpu()
        K = loc.shape[-1]
        m0, s0 = float(loc.reshape(-1)[0]), float(tril.reshape(-1, K, K)[0, 0, 0])
        eye = torch.eye(K, dtype=torch.float64)
        if s0 > 0 and bool((loc == m0).all()) and bool((tril == s0 * eye).all()):
            iso = (m0, s0)
    prior.__dict__["_bnn_isotropic"] = iso
    return iso


def _mvn_kl_descs(mus, scales, priors, g_mus=None, g_scales=None):
    arr = (_lib.MvnKlTensor * len(mus))()
    for i, (m, sc, pr) in enumerate(zip(mus, scales, priors)):
        rows, K = _mvn_extent(m, sc)
        t = arr[i]
        t.mu, t.scale, t.rows, t.cols = m.data_ptr(), sc.data_ptr(), rows, K
        t.prior_mu, t.prior_sigma = pr
        if g_mus is not None:
            t.g_mu, t.g_scale = g_mus[i].data_ptr(), g_scales[i].data_ptr()
    return arr


class _MvnKL(torch.autograd.Function):
    """out[t] = mean over the rows of KL(MVN(mu_t, scale_tril = V_t) || isotropic prior t): bnn_mvn_kl (two launches) forward,
    bnn_mvn_kl_backward backward.  The gradient is returned, never parked (FUSE_KL_GRADIENT covers WeightNormal only)."""

    @staticmethod
    def forward(ctx, priors, *params):
        T = len(priors)
        mus, scales = [p.detach() for p in params[:T]], [p.detach() for p in params[T:]]
        dev = mus[0].device
        arr = _mvn_kl_descs(mus, scales, priors)
        nbytes = _lib.load().bnn_mvn_kl_workspace_bytes(arr, T)
        if nbytes < 0:
            raise BnnHipError("bnn_mvn_kl_workspace_bytes: bad tensors")
        ws = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=dev)        # per call: concurrent KLs never share it
        out = torch.empty(T, dtype=torch.float32, device=dev)
        check(_lib.load().bnn_mvn_kl(arr, T, ptr(out), ptr(ws), ws.numel() * 8, stream_ptr(dev)), "bnn_mvn_kl")
        ctx.save_for_backward(*params)
        ctx.priors = priors
        return out

    @staticmethod
    def backward(ctx, g):
        params = ctx.saved_tensors
        T = len(ctx.priors)
        mus, scales = params[:T], params[T:]
        g_mus = [torch.empty_like(m) for m in mus]
        g_scales = [torch.empty_like(sc) for sc in scales]
        arr = _mvn_kl_descs(mus, scales, ctx.priors, g_mus, g_scales)
        up = g.contiguous().float()
        check(_lib.load().bnn_mvn_kl_backward(arr, T, ptr(up), stream_ptr(up.device)), "bnn_mvn_kl_backward")
        return (None,) + tuple(g_mus) + tuple(g_scales)


def mvn_kl(mus, scales, priors):
    """priors: (m0, sigma0) per tensor (mvn_isotropic).  -> (T,) fp32: each tensor's mean KL over its rows, differentiable --
    KLDivergence.compute_kl of a WeightMultivariateNormal against its isotropic prior."""
    return _MvnKL.apply(tuple((float(a), float(b)) for a, b in priors), *[m.contiguous() for m in mus],
                        *[sc.contiguous() for sc in scales])


# --------------------------------------------------------------------------- K3
_kl_ws = {}


def _kl_workspace(device):
    key = (device.type, device.index)
    ws = _kl_ws.get(key)
    if ws is None:
        nbytes = _lib.load().bnn_kl_workspace_bytes(0)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        _kl_ws[key] = ws
    return ws


def _kl_descs(mus, rhos, priors):
    T = len(mus)
    arr = (KlTensor * T)()
    for i in range(T):
        arr[i].mu = mus[i].data_ptr()
        arr[i].rho = rhos[i].data_ptr()
        arr[i].n = mus[i].numel()
        arr[i].prior_mu = priors[i][0]
        arr[i].prior_sigma = priors[i][1]
    return arr


class _KLNormal(torch.autograd.Function):
    """Returns (out, scalar): out (T + 1) = per-tensor KL SUMS then the KLDivergence scalar (loss.py:16-38); scalar = the
    0-d view out[T] made inside forward, so that a loss built on it back-propagates straight into this node (selecting
    out[T] outside costs the backward a zero-fill and a copy launch)."""

    @staticmethod
    def forward(ctx, n_batches, priors, out, *params):
        T = len(params) // 2
        mus = [p.detach() for p in params[:T]]
        rhos = [p.detach() for p in params[T:]]
        for m, r in zip(mus, rhos):
            require_cuda_f32(m, "mean")
            require_cuda_f32(r, "scale")
        dev = mus[0].device
        if out is None:
            out = torch.empty(T + 1, dtype=torch.float32, device=dev)
        else:
            require_cuda_f32(out, "out")
            if out.numel() != T + 1:
                raise BnnHipError("kl_normal: out must hold %d floats" % (T + 1))
            ctx.mark_dirty(out)
        arr = _kl_descs(mus, rhos, priors)
        check(_lib.load().bnn_kl_forward(arr, T, float(n_batches), ptr(out), ptr(_kl_workspace(dev)),
                                          stream_ptr(dev)), "bnn_kl_forward")
        ctx.save_for_backward(*params)
        ctx.n_batches, ctx.priors, ctx.T = float(n_batches), priors, T
        ctx.set_materialize_grads(False)
        return out, out[T]

    @staticmethod
    def backward(ctx, g_out, g_scalar):
        # Only the scalar is differentiable here -- as the second output, or as out[T] of the first (the per-tensor sums
        # are reported for diagnostics / the sharded all-reduce and carry no gradient).
        params = ctx.saved_tensors
        T = ctx.T
        mus, rhos = params[:T], params[T:]
        if g_out is None and g_scalar is None:
            return (None, None, None) + (None,) * (2 * T)
        up = g_scalar.reshape(1) if g_scalar is not None else None
        if g_out is not None:
            up2 = g_out[T:T + 1].contiguous()
            up = up2 if up is None else up + up2
        up = up.contiguous()
        pend, task = _tls.kl_pending, torch._C._current_graph_task_id()
        keys = [(m.device.index, m.data_ptr()) for m in mus]
        if FUSE_KL_GRADIENT and all(m.is_leaf and r.is_leaf for m, r in zip(mus, rhos)) and \
                not any(k in pend and pend[k].task == task for k in keys):   # (two KL terms of THIS pass on one tensor: no parking)
            # park the gradient for the layers' weight-gradient launches (see _KlPending above); what an earlier pass that
            # raised left under the same key is overwritten
            for k, m, r, pr in zip(keys, mus, rhos, ctx.priors):
                pend[k] = _KlPending(up, 1.0 / (m.numel() * T * ctx.n_batches), pr, m, r, task)
            torch.autograd.Variable._execution_engine.queue_callback(functools.partial(_kl_flush, task))
            return (None, None, None) + (None,) * (2 * T)
        g_mu = [torch.empty_like(m) for m in mus]
        g_rho = [torch.empty_like(r) for r in rhos]
        arr = _kl_descs(mus, rhos, ctx.priors)
        gm = (ctypes.c_void_p * T)(*[t.data_ptr() for t in g_mu])
        gr = (ctypes.c_void_p * T)(*[t.data_ptr() for t in g_rho])
        check(_lib.load().bnn_kl_backward(arr, T, ctx.n_batches, ptr(up), gm, gr, 0, stream_ptr(up.device)),
              "bnn_kl_backward")
        return (None, None, None) + tuple(g_mu) + tuple(g_rho)


def kl_normal(mus, rhos, priors, n_batches=1.0, out=None):
    """priors: list of (prior_mu, prior_sigma) floats.  -> tensor (T + 1): per-tensor KL sums,
    then the KLDivergence scalar.  `out` (optional, T + 1 floats) receives the result in place."""
    mus = [m.contiguous() for m in mus]
    rhos = [r.contiguous() for r in rhos]
    return _KLNormal.apply(n_batches, tuple(priors), out, *mus, *rhos)[0]


def kl_normal_scalar(mus, rhos, priors, n_batches=1.0):
    """The KLDivergence scalar of kl_normal as a 0-d tensor (differentiable; what KLDivergence.forward returns)."""
    mus = [m.contiguous() for m in mus]
    rhos = [r.contiguous() for r in rhos]
    return _KLNormal.apply(n_batches, tuple(priors), None, *mus, *rhos)[1]


class KlDeferred:
    """A KL whose first pass has been launched (kl_normal_begin); mc_mean(..., kl=this) runs the second pass inside the
    MC reduction's launch and fills `out` (T + 1 floats: per-tensor sums, then the KLDivergence scalar)."""
    __slots__ = ("arr", "T", "n_batches", "out", "ws", "keep", "done", "launched")


def kl_normal_begin(mus, rhos, priors, n_batches=1.0, out=None, carry=False):
    """First half of kl_normal for an inference step that ends in mc_mean (no autograd): launches the partial sums
    only.  The result lands in the returned handle's `.out` when mc_mean(..., kl=handle) has run; values are
    bit-identical to kl_normal's.
    carry=True: nothing is launched here -- the next narrow sampled linear layer (N <= 16, a classifier head, whose
    launch leaves most CUs idle) carries the partial sums in ITS launch (bnn_linear_forward_sampled_kl); if no such
    layer runs before mc_mean(kl=handle), mc_mean launches them itself."""
    T = len(mus)
    mus = [m.detach().contiguous() for m in mus]
    rhos = [r.detach().contiguous() for r in rhos]
    for m, r in zip(mus, rhos):
        require_cuda_f32(m, "mean")
        require_cuda_f32(r, "scale")
    dev = mus[0].device
    if out is None:
        out = torch.empty(T + 1, dtype=torch.float32, device=dev)
    else:
        require_cuda_f32(out, "out")
        if out.numel() != T + 1:
            raise BnnHipError("kl_normal_begin: out must hold %d floats" % (T + 1))
    h = KlDeferred()
    h.arr, h.T, h.n_batches, h.out, h.ws = _kl_descs(mus, rhos, priors), T, float(n_batches), out, _kl_workspace(dev)
    h.keep, h.done, h.launched = (mus, rhos), False, False
    if carry:
        _tls.kl_carry = h
        return h
    check(_lib.load().bnn_kl_forward_partial(h.arr, T, ptr(h.ws), stream_ptr(dev)), "bnn_kl_forward_partial")
    h.launched = True
    return h


def _kl_uncarry(kl):
    """No later launch may carry `kl`'s first pass (a KlDeferred or None)."""
    if kl is not None and _tls.kl_carry is kl:
        _tls.kl_carry = None


def _kl_tail_args(kl, who, dev):
    """The five KL arguments of a launch whose extra workgroup runs the second pass of `kl` (a KlDeferred from kl_normal_begin;
    None: no such tail).  Refuses a finished one; launches the first pass now if no narrow layer took it along."""
    if kl is None:
        return None, 0, 1.0, None, None
    if kl.done:
        raise BnnHipError("%s: this KlDeferred has already been finished" % who)
    if not kl.launched:
        _kl_uncarry(kl)
        check(_lib.load().bnn_kl_forward_partial(kl.arr, kl.T, ptr(kl.ws), stream_ptr(dev)), "bnn_kl_forward_partial")
        kl.launched = True
    return kl.arr, kl.T, kl.n_batches, ptr(kl.out), ptr(kl.ws)


@contextlib.contextmanager
def _kl_finishing(kl):
    """Around the checks and the launch that finish `kl` (a KlDeferred or None): done once they succeeded; after a BnnHipError the
    launch that was to finish it has failed, and nothing may carry it later."""
    try:
        yield
    except BnnHipError:
        _kl_uncarry(kl)
        raise
    if kl is not None:
        kl.done = True


def _mc_input(y, who, noun):
    """The stacked MC outputs of a tail -> (yy, nparts, S, rows_shape, rows, width): y a CUDA fp32 (S, *rows, width) tensor (made
    contiguous if it is not), or a HeadPartials, whose (parts, S, M, width) partials the launch adds itself."""
    if isinstance(y, HeadPartials):
        yy = y.p
        require_cuda_f32(yy, "y")
        nparts, S, M, width = yy.shape
        rows_shape = (M,)
    else:
        if not y.is_cuda:
            raise BnnHipError("y must be a CUDA/HIP tensor")
        if y.dtype != torch.float32:
            raise BnnHipError("y must be float32, got %s" % y.dtype)
        if y.dim() < 2:
            raise BnnHipError("%s: y must be (S, *rows, %s), got %s" % (who, noun, tuple(y.shape)))
        yy = y.detach().contiguous()
        nparts, S, width = 1, yy.shape[0], yy.shape[-1]
        rows_shape = tuple(yy.shape[1:-1])
    rows = 1
    for d in rows_shape:
        rows *= d
    return yy, nparts, S, rows_shape, rows, width


# --------------------------------------------------------------------------- MC reduction
def mc_mean(y, out=None, scale=None, advance=None, kl=None):
    """scale * sum over the leading MC axis (default scale 1/S = torch.stack(preds).mean(0),
    examples/MNIST/uncertainty.py:50).  `out` (optional, y[0].numel() floats) is written in place.
    `advance` (optional, a device epoch cell of _rng.EpsGenerator.epoch_dev) is bumped by one in the
    same launch: the fresh-noise step of a captured MC forward without a launch of its own.
    `kl` (optional, a KlDeferred from kl_normal_begin): that KL's second pass runs in this launch too.
    y may be a HeadPartials (a hidden layer fused with its classifier head): the same launch then adds the partial logits over
    (part, sample) -- the default scale stays 1 / S."""
    if isinstance(y, HeadPartials):
        parts, S, M, Nh = y.p.shape
        y = y.p.view(parts * S, M, Nh)              # addend v = part * S + s, M * Nh floats apart
        nadd, out_shape = parts * S, (M, Nh)
    else:
        S = nadd = y.shape[0]
        out_shape = y.shape[1:]
    require_cuda_f32(y, "y")
    n = y[0].numel()
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=y.device)
    else:
        require_cuda_f32(out, "out")
        if out.numel() != n:
            raise BnnHipError("mc_mean: out must hold %d floats" % n)
    sc = (1.0 / S) if scale is None else float(scale)
    adv = ptr(advance) if advance is not None else None
    if kl is not None:
        # second pass of a KL begun by kl_normal_begin, as one extra workgroup of this launch (a failed launch leaves a
        # carried handle where it is: no _kl_finishing here)
        check(_lib.load().bnn_mc_sum_kl(ptr(y), n, nadd, n, sc, ptr(out), 0, adv, 1, *_kl_tail_args(kl, "mc_mean", y.device),
                                        stream_ptr(y.device)), "bnn_mc_sum_kl")
        kl.done = True
        return out
    check(_lib.load().bnn_mc_sum(ptr(y), n, nadd, n, sc, ptr(out), 0, adv, 1, stream_ptr(y.device)), "bnn_mc_sum")
    return out


# --------------------------------------------------------------------------- predictive uncertainty
PredictiveUncertainty = collections.namedtuple("PredictiveUncertainty", ("mean", "total", "aleatoric", "epistemic"))
PredictiveUncertainty.__doc__ = """What mc_uncertainty returns: mean (*rows, C), the predictive mean of the per-sample probabilities;
total (*rows), its entropy; aleatoric (*rows), the mean per-sample entropy; epistemic (*rows) = total - aleatoric, the mutual
information between the prediction and the weights (the BALD score)."""

_UNC_INPUTS = {"logits": _lib.UNC_LOGITS, "probs": _lib.UNC_PROBS}


def _unc_kind(inputs, who, kl=None):
    """BNN_UNC_* of `inputs`.  Raises ValueError for anything but 'logits' / 'probs' (whether the outputs are logits or
    probabilities cannot be told safely from their values) -- and then leaves no KL pending for a later launch to carry."""
    if isinstance(inputs, str) and inputs in _UNC_INPUTS:
        return _UNC_INPUTS[inputs]
    _kl_uncarry(kl)
    raise ValueError("%s: inputs must be 'logits' or 'probs', got %r" % (who, inputs))


def uncertainty_f64(ys, inputs):
    """The formulas of mc_uncertainty in float64 torch, rounded to float32 at the end (the CPU path of
    BayesianNetworkModule.predictive_uncertainty): ys (S, *rows, C), the stacked MC outputs.
    logits: p_s = softmax(z_s), H(p_s) = logsumexp(z_s) - sum p_s z_s, total = -sum mean log mean (0 log 0 = 0);
    probs:  p_s = ys[s] as given, H(p) = -sum p log(p + 1e-10) for both (nn.Entropy's convention)."""
    kind = _unc_kind(inputs, "uncertainty_f64")
    y = ys.detach().to(torch.float64)
    if kind == _lib.UNC_LOGITS:
        p = torch.softmax(y, -1)
        h = torch.logsumexp(y, -1) - (p * y).sum(-1)
        mean = p.mean(0)
        total = -torch.xlogy(mean, mean).sum(-1)
    else:
        h = -(y * torch.log(y + 1e-10)).sum(-1)
        mean = y.mean(0)
        total = -(mean * torch.log(mean + 1e-10)).sum(-1)
    ale = h.mean(0)
    f32 = lambda t: t.to(torch.float32)         # noqa: E731
    return PredictiveUncertainty(f32(mean), f32(total), f32(ale), f32(total - ale))


def mc_uncertainty(y, inputs=None, advance=None, kl=None):
    """Predictive uncertainty over the leading MC axis in ONE launch (bnn_mc_uncertainty) -> PredictiveUncertainty.
    y: CUDA fp32 (S, *rows, C), class axis last (made contiguous if it is not), or a HeadPartials (a hidden layer fused with
    its classifier head: the launch adds the partial logits itself, bit for bit as y.logits() would).
    inputs: 'logits' (p_s = softmax) or 'probs' (p_s as given, e.g. a net ending in torch.nn.Softmax) -- required.
    advance / kl: as mc_mean (the device epoch bumped, a KlDeferred's second pass run, in the same launch).
    The sums over samples are fp64 in a fixed order: bitwise reproducible."""
    kind = _unc_kind(inputs, "mc_uncertainty", kl)
    with _kl_finishing(kl):
        yy, nparts, S, rows_shape, rows, C = _mc_input(y, "mc_uncertainty", "classes")
        dev = yy.device
        mean = torch.empty(rows_shape + (C,), dtype=torch.float32, device=dev)
        total, ale, epi = (torch.empty(rows_shape, dtype=torch.float32, device=dev) for _ in range(3))
        adv = ptr(advance) if advance is not None else None
        check(_lib.load().bnn_mc_uncertainty(ptr(yy), rows * C, nparts, S, rows, C, kind, ptr(mean), ptr(total), ptr(ale),
                                             ptr(epi), adv, 1, *_kl_tail_args(kl, "mc_uncertainty", dev), stream_ptr(dev)),
              "bnn_mc_uncertainty")
    return PredictiveUncertainty(mean, total, ale, epi)


# --------------------------------------------------------------------------- predictive score (against labels)
PredictiveScore = collections.namedtuple("PredictiveScore", ("mean", "nll", "expected_nll", "brier", "confidence", "prediction",
                                                             "entropy"))
PredictiveScore.__doc__ = """What mc_score returns: mean (*rows, C), the predictive mean of the per-sample probabilities; and per row
(*rows) nll = -ln mean[y], expected_nll = -(1/S) sum_s ln p_s[y] (the ELBO's data term), brier = sum_c (mean[c] - [c = y])^2,
confidence = max_c mean[c], prediction (int64) = the lowest class attaining it, entropy = H(mean).  A target outside [0, C) makes
the row's nll, expected_nll and brier NaN."""

ScoreResult = collections.namedtuple("ScoreResult", ("n", "accuracy", "nll", "expected_nll", "brier", "ece", "mce", "reliability",
                                                     "rejection"))
ScoreResult.__doc__ = """What ScoreState.result() returns (Python floats): n rows; accuracy, nll, expected_nll, brier: their means;
ece = sum_b (n_b / n) |acc_b - conf_b| and mce = max_b |acc_b - conf_b| over the non-empty confidence bins; reliability: per
confidence bin (count, mean confidence, accuracy), NaN in an empty bin; rejection: per upper entropy-bin edge (coverage, accuracy)
of the rows kept when only those up to that edge are answered -- cumulative from the least uncertain bin upward."""


def score_state_size(conf_bins, ent_bins):
    """Doubles of a score state: [n, sum nll, sum expected_nll, sum brier, sum correct] + (count, sum confidence, sum correct) per
    confidence bin + (count, sum correct) per entropy bin (bnn_mc_score_state_doubles)."""
    if not (1 <= int(conf_bins) <= 128 and 1 <= int(ent_bins) <= 128):
        raise ValueError("score state: conf_bins and ent_bins must be in 1 .. 128, got %r, %r" % (conf_bins, ent_bins))
    return 5 + 3 * int(conf_bins) + 2 * int(ent_bins)


class ScoreState:
    """The accumulator of mc_score / BayesianNetworkModule.predictive_score over the batches of a test set: a zeroed float64
    buffer on `device` (layout: score_state_size) that every scored batch is added to on the device, and the launch's workspace.
    Nothing is copied to the host until result().  On a CPU device it accumulates what score_f64 returns."""

    def __init__(self, device, conf_bins=15, ent_bins=20):
        self.conf_bins, self.ent_bins = int(conf_bins), int(ent_bins)
        self.device = torch.device(device)
        self.state = torch.zeros(score_state_size(conf_bins, ent_bins), dtype=torch.float64, device=self.device)
        self._ws = None

    def workspace(self, rows):
        """The launch's per-row words (bnn_mc_score_workspace_bytes), grown when a larger batch comes."""
        need = _lib.load().bnn_mc_score_workspace_bytes(rows) // 4
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._ws

    def reset(self):
        self.state.zero_()
        return self

    def add_(self, vec):
        """Adds a state vector (what score_f64 returns) -- the CPU path."""
        self.state += vec.to(self.state.device, torch.float64)
        return self

    def result(self):
        """ScoreResult of everything added so far: ONE device-to-host copy, finished in Python float64.  n = 0: NaN ratios."""
        v = self.state.detach().cpu().tolist()
        nan = float("nan")
        div = lambda a, b: a / b if b > 0 else nan         # noqa: E731
        n = v[0]
        cb, eb = self.conf_bins, self.ent_bins
        rel, ece, gaps = [], 0.0, []
        for b in range(cb):
            cnt, sc, sk = v[5 + 3 * b:8 + 3 * b]
            conf, acc = div(sc, cnt), div(sk, cnt)
            rel.append((cnt, conf, acc))
            if cnt > 0:
                gaps.append(abs(acc - conf))
                ece += cnt / n * gaps[-1]
        ece, mce = (ece, max(gaps)) if gaps else (nan, nan)
        rej, cum_n, cum_k = [], 0.0, 0.0
        for b in range(eb):
            cnt, sk = v[5 + 3 * cb + 2 * b:7 + 3 * cb + 2 * b]
            cum_n += cnt
            cum_k += sk
            rej.append((div(cum_n, n), div(cum_k, cum_n)))
        return ScoreResult(n, div(v[4], n), div(v[1], n), div(v[2], n), div(v[3], n), ece, mce, rel, rej)


def _score_bins(conf, ent, C, conf_bins, ent_bins):
    """The launch's bins of fp32 confidences / entropies, in float64: min(conf_bins - 1, floor(confidence conf_bins)),
    clamp(floor(entropy / ln C ent_bins), 0, ent_bins - 1)."""
    cbin = torch.floor(conf.to(torch.float64) * conf_bins).clamp_(0, conf_bins - 1).to(torch.int64)
    ebin = torch.floor(ent.to(torch.float64) * (ent_bins / math.log(C))).clamp_(0, ent_bins - 1).to(torch.int64)
    return cbin, ebin


def score_f64(ys, target, inputs, conf_bins=15, ent_bins=20):
    """The formulas of mc_score in float64 torch (the CPU path of BayesianNetworkModule.predictive_score): ys (S, *rows, C), the
    stacked MC outputs; target (*rows) int64.  Returns (PredictiveScore, state vector): the per-row values rounded to float32 at
    the end, and the float64 vector a ScoreState adds (score_state_size), whose bins and sums are those of the rounded values.
    logits: log p_s = log_softmax(z_s), nll = -(logsumexp_s log p_s[y] - ln S);  probs: p_s = ys[s] as given, logs of p + 1e-10."""
    kind = _unc_kind(inputs, "score_f64")
    nstate = score_state_size(conf_bins, ent_bins)
    y = ys.detach().to(torch.float64)
    if y.dim() < 2 or y.shape[-1] < 2:
        raise ValueError("score_f64: ys must be (S, *rows, classes >= 2), got %s" % (tuple(ys.shape),))
    S, C = y.shape[0], y.shape[-1]
    if target.dtype != torch.int64 or tuple(target.shape) != tuple(y.shape[1:-1]):
        raise ValueError("score_f64: target must be int64 of shape %s, got %s %s" % (tuple(y.shape[1:-1]), target.dtype, tuple(target.shape)))
    y = y.reshape(S, -1, C)
    t = target.detach().reshape(-1).to(y.device)
    ok = (t >= 0) & (t < C)
    idx = torch.where(ok, t, torch.zeros_like(t)).view(1, -1, 1).expand(S, -1, 1)
    if kind == _lib.UNC_LOGITS:
        lp = torch.log_softmax(y, -1)
        mean = lp.exp().mean(0)
        lpy = lp.gather(-1, idx).squeeze(-1)                        # (S, rows)
        nll = -(torch.logsumexp(lpy, 0) - math.log(S))
        enll = -lpy.mean(0)
        ent = -torch.xlogy(mean, mean).sum(-1)
    else:
        mean = y.mean(0)
        py = y.gather(-1, idx).squeeze(-1)
        nll = -torch.log(mean.gather(-1, idx[0]).squeeze(-1) + 1e-10)
        enll = -torch.log(py + 1e-10).mean(0)
        ent = -(mean * torch.log(mean + 1e-10)).sum(-1)
    onehot = torch.zeros_like(mean).scatter_(-1, idx[0], 1.0)
    brier = ((mean - onehot) ** 2).sum(-1)
    nan = torch.full_like(nll, float("nan"))
    nll, enll, brier = (torch.where(ok, v, nan) for v in (nll, enll, brier))
    mean32 = mean.to(torch.float32)
    conf = mean32.max(-1).values
    pred = (mean32 == conf.unsqueeze(-1)).to(torch.int64).argmax(-1)      # the lowest class attaining the maximum
    f32 = lambda v: v.to(torch.float32)         # noqa: E731
    rows_shape = tuple(ys.shape[1:-1])
    out = PredictiveScore(mean32.reshape(rows_shape + (C,)), *(v.reshape(rows_shape) for v in
                          (f32(nll), f32(enll), f32(brier), conf, pred, f32(ent))))
    correct = (ok & (pred == t)).to(torch.float64)
    cbin, ebin = _score_bins(conf, f32(ent), C, conf_bins, ent_bins)
    vec = torch.zeros(nstate, dtype=torch.float64, device=y.device)
    vec[0] = t.numel()
    vec[1], vec[2], vec[3] = (f32(v).to(torch.float64).sum() for v in (nll, enll, brier))
    vec[4] = correct.sum()
    one = torch.ones_like(correct)
    cpart = vec[5:5 + 3 * conf_bins].view(conf_bins, 3)
    cpart[:, 0].index_add_(0, cbin, one)
    cpart[:, 1].index_add_(0, cbin, conf.to(torch.float64))
    cpart[:, 2].index_add_(0, cbin, correct)
    epart = vec[5 + 3 * conf_bins:].view(ent_bins, 2)
    epart[:, 0].index_add_(0, ebin, one)
    epart[:, 1].index_add_(0, ebin, correct)
    return out, vec


def mc_score(y, target, inputs=None, state=None, advance=None):
    """An MC forward scored against its labels over the leading MC axis in ONE launch (bnn_mc_score) -> PredictiveScore.
    y: CUDA fp32 (S, *rows, C >= 2), class axis last (made contiguous if it is not), or a HeadPartials (the launch adds the partial
    logits itself, bit for bit as y.logits() would).  target: CUDA int64 (*rows); a value outside [0, C) makes its row's nll,
    expected_nll and brier NaN (checked on the device: no host synchronisation, no ignore_index).
    inputs: 'logits' (p_s = softmax) or 'probs' (p_s as given) -- required.
    state: a ScoreState on y's device; a second one-workgroup launch adds this batch to it (sums, reliability and rejection
    histograms), so one state carries a whole test set and ScoreState.result() is the only host copy.
    advance: as mc_mean (the device epoch bumped in the same launch).  Bitwise reproducible; graph-capturable."""
    kind = _unc_kind(inputs, "mc_score")
    yy, nparts, S, rows_shape, rows, C = _mc_input(y, "mc_score", "classes")
    dev = yy.device
    if not isinstance(target, torch.Tensor) or not target.is_cuda or target.device != dev:
        raise BnnHipError("mc_score: target must be a CUDA/HIP tensor on y's device")
    if target.dtype != torch.int64 or tuple(target.shape) != rows_shape:
        raise BnnHipError("mc_score: target must be int64 of shape %s, got %s %s" % (rows_shape, target.dtype, tuple(target.shape)))
    tt = target.detach().contiguous()
    sp, cb, eb, ws = None, 0, 0, None
    if state is not None:
        if not isinstance(state, ScoreState) or state.device.type != "cuda" or state.state.device != dev:
            raise BnnHipError("mc_score: state must be a ScoreState on y's device")
        if rows > 0:
            sp, cb, eb, ws = ptr(state.state), state.conf_bins, state.ent_bins, ptr(state.workspace(rows))
    mean = torch.empty(rows_shape + (C,), dtype=torch.float32, device=dev)
    nll, enll, brier, conf, ent = (torch.empty(rows_shape, dtype=torch.float32, device=dev) for _ in range(5))
    pred = torch.empty(rows_shape, dtype=torch.int64, device=dev)
    adv = ptr(advance) if advance is not None else None
    check(_lib.load().bnn_mc_score(ptr(yy), rows * C, nparts, S, rows, C, kind, ptr(tt), ptr(mean), ptr(nll), ptr(enll), ptr(brier),
                                   ptr(conf), ptr(pred), ptr(ent), sp, cb, eb, ws, adv, 1, stream_ptr(dev)), "bnn_mc_score")
    return PredictiveScore(mean, nll, enll, brier, conf, pred, ent)


# --------------------------------------------------------------------------- predictive regression
PredictiveRegression =collections.namedtuple("PredictiveRegression", ("mean", "total", "aleatoric", "epistemic"))
PredictiveRegression.__doc__ = """What mc_regression returns, all (*rows, D): mean, the mean of the per-sample means; aleatoric, the
mean of the per-sample variances; epistemic, the (population) variance of the per-sample means; total = aleatoric + epistemic, the
variance of the equal-weight mixture of the per-sample predictives (law of total variance)."""

_REG_OUTPUTS = {"values": _lib.REG_VALUES, "mean_logvar": _lib.REG_MEAN_LOGVAR, "mean_var": _lib.REG_MEAN_VAR}


def _reg_kind(outputs, who, kl=None):
    """BNN_REG_* of `outputs`.  Raises ValueError for anything but 'values' / 'mean_logvar' / 'mean_var' (what the last axis
    holds cannot be told from its values) -- and then leaves no KL pending for a later launch to carry."""
    if isinstance(outputs, str) and outputs in _REG_OUTPUTS:
        return _REG_OUTPUTS[outputs]
    _kl_uncarry(kl)
    raise ValueError("%s: outputs must be 'values', 'mean_logvar' or 'mean_var', got %r" % (who, outputs))


def _reg_split(y, kind, who):
    """(means, variances or None) of stacked outputs y (..., width) in float64."""
    if kind == _lib.REG_VALUES:
        return y, None
    if y.shape[-1] % 2:
        raise ValueError("%s: a (mean, variance) layout needs an even last axis, got %d" % (who, y.shape[-1]))
    D = y.shape[-1] // 2
    m, v = y[..., :D], y[..., D:]
    return m, (torch.exp(v) if kind == _lib.REG_MEAN_LOGVAR else v)


def regression_f64(ys, outputs):
    """The formulas of mc_regression in float64 torch, rounded to float32 at the end (the CPU path of
    BayesianNetworkModule.predictive_regression): ys (S, *rows, width), the stacked MC outputs.  The variance of the means is
    the two-pass population variance."""
    kind = _reg_kind(outputs, "regression_f64")
    m, v = _reg_split(ys.detach().to(torch.float64), kind, "regression_f64")
    mean = m.mean(0)
    epi = ((m - mean) ** 2).mean(0)
    ale = torch.zeros_like(mean) if v is None else v.mean(0)
    f32 = lambda t: t.to(torch.float32)         # noqa: E731
    return PredictiveRegression(f32(mean), f32(ale + epi), f32(ale), f32(epi))


def mc_regression(y, outputs=None, advance=None, kl=None):
    """Predictive mean and variance decomposition over the leading MC axis in ONE launch (bnn_mc_regression) ->
    PredictiveRegression.
    y: CUDA fp32 (S, *rows, width) (made contiguous if it is not), or a HeadPartials (a hidden layer fused with its <= 16-wide
    head: the launch adds the partials itself, bit for bit as y.logits() would).
    outputs: 'values' (point predictions, D = width), 'mean_logvar' (D means then D log-variances) or 'mean_var' (D means then
    D variances as given) -- required.
    advance / kl: as mc_mean (the device epoch bumped, a KlDeferred's second pass run, in the same launch).
    The sums over samples are fp64 in a fixed order: bitwise reproducible."""
    kind = _reg_kind(outputs, "mc_regression", kl)
    with _kl_finishing(kl):
        yy, nparts, S, rows_shape, rows, W = _mc_input(y, "mc_regression", "width")
        if kind != _lib.REG_VALUES and W % 2:
            raise BnnHipError("mc_regression: outputs=%r needs an even last axis, got %d" % (outputs, W))
        D = W if kind == _lib.REG_VALUES else W // 2
        dev = yy.device
        mean, total, ale, epi = (torch.empty(rows_shape + (D,), dtype=torch.float32, device=dev) for _ in range(4))
        adv = ptr(advance) if advance is not None else None
        check(_lib.load().bnn_mc_regression(ptr(yy), rows * W, nparts, S, rows, W, kind, ptr(mean), ptr(total), ptr(ale),
                                            ptr(epi), adv, 1, *_kl_tail_args(kl, "mc_regression", dev), stream_ptr(dev)),
              "bnn_mc_regression")
    return PredictiveRegression(mean, total, ale, epi)


# --------------------------------------------------------------------------- predictive regression score (against targets)
RegressionScore = collections.namedtuple("RegressionScore", ("mean", "variance", "sq_err", "nll", "gaussian_nll", "crps", "pit"))
RegressionScore.__doc__ = """What mc_regression_score returns, all (*rows, D): mean and variance, mc_regression's mean and total;
sq_err = (mean - t)^2; nll, the negative log-density of the MC predictive -- the equal-weight mixture of the S per-sample Gaussians
-- at the target t ('values' has no density: gaussian_nll's bits); gaussian_nll, that of the moment-matched Gaussian
N(mean, variance) (NaN where variance == 0); crps, the mixture's continuous ranked probability score (the ensemble CRPS for
'values'); pit, the mixture's cdf at t.  A NaN target makes its element's last five NaN; a negative or NaN per-sample variance
('mean_var') makes its element's nll, crps and pit NaN."""

REG_SCORE_MAX_SAMPLES = 1024            # the CRPS's pair sum is quadratic in S


def regression_score_state_size(D, pit_bins):
    """Doubles of a regression score state: per predicted quantity [n, sum sq_err, sum nll, sum gaussian_nll, sum crps,
    sum variance] + pit_bins counts (bnn_mc_regression_score_state_doubles)."""
    if not (1 <= int(D) <= 4096 and 1 <= int(pit_bins) <= 128):
        raise ValueError("regression score state: D must be in 1 .. 4096 and pit_bins in 1 .. 128, got %r, %r" % (D, pit_bins))
    return int(D) * (6 + int(pit_bins))


class RegressionScoreResult(collections.namedtuple("RegressionScoreResult", ("n", "rmse", "nll", "gaussian_nll", "crps", "sharpness",
                                                                             "pit_hist", "calibration", "calibration_error"))):
    """What RegressionScoreState.result() returns: per predicted quantity d (lists of length D, Python floats) n targets; rmse;
    the means of nll, gaussian_nll and crps; sharpness = sqrt(mean predictive variance); pit_hist, the counts of the PIT in
    equal-width bins (a NaN pit is in none); calibration, the list of (k / bins, observed share of the binned pit below that
    edge) for k = 1 .. bins -- a calibrated predictive lies on the diagonal --; calibration_error = mean_k |observed - k / bins|.
    n = 0 (or nothing binned): NaN ratios."""
    __slots__ = ()

    def coverage(self, level):
        """Per d, the share of the binned targets inside the central `level` interval of the predictive: pit in
        [(1 - level) / 2, (1 + level) / 2].  The interval must end on bin edges: ValueError unless (1 - level) / 2 * bins is an
        integer to 1e-9."""
        out = []
        for hist in self.pit_hist:
            bins = len(hist)
            lo = (1.0 - float(level)) / 2.0 * bins
            k = int(round(lo))
            if not (0.0 < float(level) <= 1.0) or abs(lo - k) > 1e-9:
                raise ValueError("coverage: the central %r interval does not end on the edges of %d bins" % (level, bins))
            tot = sum(hist)
            out.append(sum(hist[k:bins - k]) / tot if tot > 0 else float("nan"))
        return out


class RegressionScoreState:
    """The accumulator of mc_regression_score / BayesianNetworkModule.predictive_regression_score over the batches of a test set:
    a zeroed float64 (D, 6 + pit_bins) buffer on `device` (layout: regression_score_state_size) that every scored batch is added
    to on the device, and the launch's workspace.  Nothing is copied to the host until result().  On a CPU device it accumulates
    what regression_score_f64 returns."""

    def __init__(self, device, D, pit_bins=20):
        self.D, self.pit_bins = int(D), int(pit_bins)
        self.device = torch.device(device)
        regression_score_state_size(D, pit_bins)
        self.state = torch.zeros(self.D, 6 + self.pit_bins, dtype=torch.float64, device=self.device)
        self._ws = None

    def workspace(self, nparts, nsamples, rows, width, kind):
        """The launch's workspace with this state (bnn_mc_regression_score_workspace_bytes), grown when a larger batch comes."""
        need = _lib.load().bnn_mc_regression_score_workspace_bytes(nparts, nsamples, rows, width, kind, 1) // 4
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._ws

    def reset(self):
        self.state.zero_()
        return self

    def add_(self, mat):
        """Adds a state matrix (what regression_score_f64 returns) -- the CPU path."""
        self.state += mat.to(self.state.device, torch.float64).reshape(self.state.shape)
        return self

    def result(self):
        """RegressionScoreResult of everything added so far: ONE device-to-host copy, finished in Python float64."""
        rows = self.state.detach().cpu().tolist()
        nan = float("nan")
        div = lambda a, b: a / b if b > 0 else nan         # noqa: E731
        root = lambda a: math.sqrt(a) if a >= 0 else nan   # noqa: E731      (NaN: NaN)
        bins = self.pit_bins
        out = [[] for _ in range(9)]
        for v in rows:
            n = v[0]
            hist = v[6:6 + bins]
            tot, cum, cal = sum(hist), 0.0, []
            for k in range(1, bins + 1):
                cum += hist[k - 1]
                cal.append((k / bins, div(cum, tot)))
            err = sum(abs(obs - edge) for edge, obs in cal) / bins if tot > 0 else nan
            for o, x in zip(out, (n, root(div(v[1], n)), div(v[2], n), div(v[3], n), div(v[4], n), root(div(v[5], n)), hist, cal, err)):
                o.append(x)
        return RegressionScoreResult(*out)


def _crps_a(mu, var):
    """A(mu, sigma^2) = mu (2 Phi(mu / sigma) - 1) + 2 sigma phi(mu / sigma), A(mu, 0) = |mu|; a negative or NaN variance: NaN."""
    sg = torch.sqrt(var.clamp_min(0.0))
    safe = torch.where(sg > 0, sg, torch.ones_like(sg))
    z = mu / safe
    a = mu * torch.erf(z / math.sqrt(2.0)) + safe * math.sqrt(2.0 / math.pi) * torch.exp(-0.5 * z * z)
    a = torch.where(var == 0, mu.abs(), a)
    return torch.where(var >= 0, a, torch.full_like(a, float("nan")))


def regression_score_f64(ys, target, outputs, pit_bins=20):
    """The formulas of mc_regression_score in float64 torch (the CPU path of BayesianNetworkModule.predictive_regression_score):
    ys (S, *rows, width), the stacked MC outputs; target (*rows, D).  Returns (RegressionScore, state matrix): the per-element
    values rounded to float32 at the end, and the float64 (D, 6 + pit_bins) matrix a RegressionScoreState adds, whose bins and
    sums are those of the rounded values.  The pair term of the CRPS is summed one sample at a time: O(S) memory."""
    kind = _reg_kind(outputs, "regression_score_f64")
    y = ys.detach().to(torch.float64)
    if y.dim() < 2:
        raise ValueError("regression_score_f64: ys must be (S, *rows, width), got %s" % (tuple(ys.shape),))
    raw = None if kind == _lib.REG_VALUES else y[..., y.shape[-1] // 2:]
    m, v = _reg_split(y, kind, "regression_score_f64")
    S, D = m.shape[0], m.shape[-1]
    regression_score_state_size(D, pit_bins)
    rows_shape = tuple(m.shape[1:-1])
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != rows_shape + (D,):
        raise ValueError("regression_score_f64: target must be a tensor of shape %s" % (rows_shape + (D,),))
    m = m.reshape(S, -1, D)
    v = torch.zeros_like(m) if v is None else v.reshape(S, -1, D)
    t = target.detach().to(y.device, torch.float64).reshape(-1, D)
    nan = torch.full_like(t, float("nan"))
    mean = m.mean(0)
    V = v.mean(0) + ((m - mean) ** 2).mean(0)
    e = mean - t
    Vs = torch.where(V == 0, torch.ones_like(V), V)
    gnll = torch.where(V == 0, nan, 0.5 * (torch.log(2.0 * math.pi * Vs) + e * e / Vs))
    r = t - m                                                       # (S, rows, D)
    if kind == _lib.REG_VALUES:
        nll = gnll
    else:
        raw = raw.reshape(S, -1, D)
        if kind == _lib.REG_MEAN_LOGVAR:
            lnv, inv = raw, torch.exp(-raw)
        else:
            pos = v > 0
            vs = torch.where(pos, v, torch.ones_like(v))
            lnv, inv = torch.where(pos, torch.log(vs), torch.full_like(v, float("nan"))), 1.0 / vs
        ell = -0.5 * (math.log(2.0 * math.pi) + lnv + r * r * inv)
        nll = -(torch.logsumexp(ell, 0) - math.log(S))
    sg = torch.sqrt(v.clamp_min(0.0))
    safe = torch.where(sg > 0, sg, torch.ones_like(sg))
    step = (r > 0).to(torch.float64) + 0.5 * (r == 0).to(torch.float64)
    cdf = torch.where(sg > 0, 0.5 * torch.erfc(-(r / safe) / math.sqrt(2.0)), step)
    cdf = torch.where(v >= 0, cdf, torch.full_like(cdf, float("nan")))
    pit = cdf.mean(0)
    pair = torch.zeros_like(mean)
    for i in range(S):
        pair += _crps_a(m[i] - m, v[i] + v).sum(0)
    bad = (v >= 0).logical_not().any(0)                             # a pair's variances may add up to a valid one
    crps = _crps_a(r, v).mean(0) - pair / (2.0 * S * S)
    crps = torch.where(bad, nan, crps)
    tnan = torch.isnan(t)
    sq, nll, gnll, crps, pit = (torch.where(tnan, nan, x) for x in (e * e, nll, gnll, crps, pit))
    f32 = lambda x: x.to(torch.float32)         # noqa: E731
    vals = [f32(x) for x in (mean, V, sq, nll, gnll, crps, pit)]
    out = RegressionScore(*(x.reshape(rows_shape + (D,)) for x in vals))
    mat = torch.zeros(D, 6 + pit_bins, dtype=torch.float64, device=y.device)
    mat[:, 0] = t.shape[0]
    for k, x in enumerate((vals[2], vals[3], vals[4], vals[5], vals[1])):
        mat[:, 1 + k] = x.to(torch.float64).sum(0)
    p64 = vals[6].to(torch.float64)
    bins = torch.floor(p64 * pit_bins).clamp(0, pit_bins - 1)
    for d in range(D):
        ok = ~torch.isnan(p64[:, d])
        mat[d, 6:] = torch.bincount(bins[ok, d].to(torch.int64), minlength=pit_bins).to(torch.float64)
    return out, mat


def mc_regression_score(y, target, outputs=None, state=None, advance=None):
    """A regression MC forward scored against its targets over the leading MC axis in ONE launch (bnn_mc_regression_score) ->
    RegressionScore.
    y: CUDA fp32 (S, *rows, width) (made contiguous if it is not), S <= 1024, or a HeadPartials (the launch adds the partials
    itself, once, bit for bit as y.logits() would).  target: CUDA fp32 (*rows, D); a NaN target makes its element's scores NaN
    (on the device: no host synchronisation).
    outputs: 'values', 'mean_logvar' or 'mean_var' as mc_regression -- required.
    state: a RegressionScoreState on y's device with the same D; a second launch adds this batch to it (sums and the PIT
    histogram per predicted quantity), so one state carries a whole test set and RegressionScoreState.result() is the only host
    copy.  advance: as mc_mean (the device epoch bumped in the same launch).  Bitwise reproducible; graph-capturable.
    Not covered: the evidential head's Student-t predictive, a KL tail, S above 1024 (the pair sum is O(S^2 rows D))."""
    kind = _reg_kind(outputs, "mc_regression_score")
    yy, nparts, S, rows_shape, rows, W = _mc_input(y, "mc_regression_score", "width")
    if kind != _lib.REG_VALUES and W % 2:
        raise BnnHipError("mc_regression_score: outputs=%r needs an even last axis, got %d" % (outputs, W))
    if S > REG_SCORE_MAX_SAMPLES:
        raise BnnHipError("mc_regression_score: %d samples; the pair sum of the CRPS takes at most %d" % (S, REG_SCORE_MAX_SAMPLES))
    D = W if kind == _lib.REG_VALUES else W // 2
    dev = yy.device
    if not isinstance(target, torch.Tensor) or not target.is_cuda or target.device != dev:
        raise BnnHipError("mc_regression_score: target must be a CUDA/HIP tensor on y's device")
    if target.dtype != torch.float32 or tuple(target.shape) != rows_shape + (D,):
        raise BnnHipError("mc_regression_score: target must be float32 of shape %s, got %s %s"
                          % (rows_shape + (D,), target.dtype, tuple(target.shape)))
    tt = target.detach().contiguous()
    lib = _lib.load()
    sp, bins, ws = None, 0, None
    if state is not None:
        if not isinstance(state, RegressionScoreState) or state.device.type != "cuda" or state.state.device != dev:
            raise BnnHipError("mc_regression_score: state must be a RegressionScoreState on y's device")
        if state.D != D:
            raise BnnHipError("mc_regression_score: the state holds %d predicted quantities, y has %d" % (state.D, D))
        sp, bins, ws = ptr(state.state), state.pit_bins, state.workspace(nparts, S, rows, W, kind)
    else:
        need = lib.bnn_mc_regression_score_workspace_bytes(nparts, S, rows, W, kind, 0) // 4
        if need:
            ws = torch.empty(need, dtype=torch.float32, device=dev)         # a fused head's rows, the parts added once
    outs = [torch.empty(rows_shape + (D,), dtype=torch.float32, device=dev) for _ in range(7)]
    adv = ptr(advance) if advance is not None else None
    check(lib.bnn_mc_regression_score(ptr(yy), rows * W, nparts, S, rows, W, kind, ptr(tt), *(ptr(o) for o in outs), sp, bins,
                                      ptr(ws) if ws is not None and ws.numel() else None, adv, 1, stream_ptr(dev)),
          "bnn_mc_regression_score")
    return RegressionScore(*outs)


class _GaussianNLL(torch.autograd.Function):
    """gaussian_nll_loss(m, t, exp(s), full=False, reduction='mean') over the stacked samples: the loss and d loss / d ys in
    one HIP pass (bnn_gaussian_nll).  ys (S, rows, 2 D), target (rows, D); the target carries no gradient."""

    @staticmethod
    def forward(ctx, ys, target):
        require_cuda_f32(ys, "ys")
        require_cuda_f32(target, "target")
        S, R, W = ys.shape
        lib = _lib.load()
        loss = torch.empty((), dtype=torch.float32, device=ys.device)
        g = torch.empty_like(ys) if ys.requires_grad else None
        ws = torch.empty(max(1, lib.bnn_gaussian_nll_workspace_bytes(S, R, W) // 8), dtype=torch.float64, device=ys.device)
        check(lib.bnn_gaussian_nll(ptr(ys), S, R, W, ptr(target), ptr(loss), ptr(g), ptr(ws), stream_ptr(ys.device)),
              "bnn_gaussian_nll")
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, up):
        (g,) = ctx.saved_tensors
        return (g * up if g is not None else None), None


def gaussian_nll(ys, target):
    """Mean heteroscedastic Gaussian negative log-likelihood (no constant term) of MC outputs in 'mean_logvar' layout:
    ys (S, *rows, 2 D) -- or (*rows, 2 D), one sample -- holding D means then D log-variances s; target (*rows, D), shared by
    the samples (never expanded).  mean over samples, rows and D of 0.5 (s + (target - m)^2 exp(-s)) =
    torch.nn.functional.gaussian_nll_loss(m, target, exp(s)).  Differentiable in ys (the gradient comes out of the same launch);
    the target carries no gradient.  CPU tensors: the same expression in torch (float64 inside)."""
    if ys.dim() == target.dim():
        ys = ys.unsqueeze(0)
    if ys.dim() != target.dim() + 1 or ys.dim() < 3 or ys.shape[-1] != 2 * target.shape[-1] or ys.shape[1:-1] != target.shape[:-1]:
        raise ValueError("gaussian_nll: ys must be (S, *rows, 2 D) or (*rows, 2 D) for a target (*rows, D), got %s and %s"
                         % (tuple(ys.shape), tuple(target.shape)))
    if not ys.is_cuda:
        D = target.shape[-1]
        y64 = ys.to(torch.float64)
        m, s = y64[..., :D], y64[..., D:]
        r = target.to(torch.float64) - m
        return (0.5 * (s + r * r * torch.exp(-s))).mean().to(ys.dtype)
    if target.requires_grad:
        raise BnnHipError("gaussian_nll: the target carries no gradient on the device path")
    S, W = ys.shape[0], ys.shape[-1]
    return _GaussianNLL.apply(ys.contiguous().view(S, -1, W), target.contiguous().view(-1, W // 2))


# --------------------------------------------------------------------------- K13: evidential regression
# The device path of NormalInverseGaussianLinear / NormalInverseGaussianLoss (A/B switch: off = the torch-op chain of the
# reference on the device, what the layers did before K13).
EVIDENTIAL_HIP = True


def _is_dev_f32(*ts):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in ts)


class _NigHead(torch.autograd.Function):
    """z (rows, 4 D) -> gamma, upsilon, alpha, beta (rows, D) in one launch (bnn_nig_head_forward); the backward is one launch
    too (bnn_nig_head_backward), an absent incoming gradient is passed as NULL."""

    @staticmethod
    def forward(ctx, z, D):
        require_cuda_f32(z, "z")
        rows = z.shape[0]
        outs = tuple(torch.empty((rows, D), dtype=torch.float32, device=z.device) for _ in range(4))
        check(_lib.load().bnn_nig_head_forward(ptr(z), rows, D, *[ptr(t) for t in outs], stream_ptr(z.device)),
              "bnn_nig_head_forward")
        ctx.save_for_backward(z)
        ctx.D = D
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *gs):
        (z,) = ctx.saved_tensors
        gs = [None if g is None else g.contiguous() for g in gs]
        for g in gs:
            if g is not None:
                require_cuda_f32(g, "gradient")
        gz = torch.empty_like(z)
        check(_lib.load().bnn_nig_head_backward(ptr(z), *[ptr(g) for g in gs], z.shape[0], ctx.D, ptr(gz), stream_ptr(z.device)),
              "bnn_nig_head_backward")
        return gz, None


def nig_head(z, D):
    """The evidential head's activation on the output z (*rows, 4 D) of its Linear (CUDA fp32) -> (gamma, upsilon, alpha, beta),
    each (*rows, D) and contiguous: gamma = z[..., :D], upsilon = 1e-10 + softplus(z[..., D:2D]), alpha = 1 + 1e-10 +
    softplus(z[..., 2D:3D]), beta = 1e-10 + softplus(z[..., 3D:]) (NormalInverseGaussianLinear, dense.py:141-162).
    Differentiable in z; one launch forward, one backward."""
    if not _is_dev_f32(z):
        raise BnnHipError("nig_head: z must be a CUDA/HIP float32 tensor")
    if z.dim() < 1 or D < 1 or z.shape[-1] != 4 * D:
        raise BnnHipError("nig_head: z must be (*rows, 4 D) with D = %d, got %s" % (D, tuple(z.shape)))
    lead = tuple(z.shape[:-1])
    outs = _NigHead.apply(z.contiguous().view(-1, 4 * D), D)
    return tuple(t.view(lead + (D,)) for t in outs)


class _NigLoss(torch.autograd.Function):
    """NormalInverseGaussianLoss.forward (loss.py:54-69) and the gradients of the inputs that require one, in one HIP pass
    (bnn_nig_loss: two launches).  Flat contiguous fp32 inputs of one length; y carries no gradient."""

    @staticmethod
    def forward(ctx, gamma, upsilon, alpha, beta, y, reg_lambda):
        for t, name in ((gamma, "gamma"), (upsilon, "upsilon"), (alpha, "alpha"), (beta, "beta"), (y, "y")):
            require_cuda_f32(t, name)
        n = gamma.numel()
        lib = _lib.load()
        dev = gamma.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        gs = [torch.empty_like(t) if need else None for t, need in zip((gamma, upsilon, alpha, beta), ctx.needs_input_grad[:4])]
        ws = torch.empty(max(1, lib.bnn_nig_loss_workspace_bytes(n) // 8), dtype=torch.float64, device=dev)
        check(lib.bnn_nig_loss(ptr(gamma), ptr(upsilon), ptr(alpha), ptr(beta), ptr(y), n, float(reg_lambda), ptr(loss),
                               *[ptr(g) for g in gs], ptr(ws), stream_ptr(dev)), "bnn_nig_loss")
        ctx.save_for_backward(*gs)
        return loss

    @staticmethod
    def backward(ctx, up):
        return tuple(None if g is None else g * up for g in ctx.saved_tensors) + (None, None)


def nig_loss(gamma, upsilon, alpha, beta, y, reg_lambda=1e-2):
    """mean(nll) + reg_lambda * mean(|y - gamma| (2 upsilon + alpha)) of an evidential head's outputs against y
    (NormalInverseGaussianLoss, loss.py:54-69): five CUDA fp32 tensors of one shape (strided views are made contiguous).  The
    gradients of the inputs that require one come out of the same pass; y carries no gradient.  Every element is evaluated in
    float64 on the device and the sum is taken in a fixed order: bitwise reproducible."""
    ts = (gamma, upsilon, alpha, beta, y)
    if not _is_dev_f32(*ts):
        raise BnnHipError("nig_loss: gamma, upsilon, alpha, beta and y must be CUDA/HIP float32 tensors")
    if any(t.shape != gamma.shape for t in ts) or gamma.numel() < 1:
        raise BnnHipError("nig_loss: the five tensors must have one non-empty shape, got %s" % ([tuple(t.shape) for t in ts],))
    if y.requires_grad and torch.is_grad_enabled():
        raise BnnHipError("nig_loss: y carries no gradient on the device path")
    return _NigLoss.apply(*[t.contiguous().view(-1) for t in ts], float(reg_lambda))


def _evidential_shapes(ts, who):
    if any(not isinstance(t, torch.Tensor) or t.shape != ts[0].shape for t in ts) or ts[0].dim() < 2 or ts[0].numel() < 1:
        raise ValueError("%s: gamma, upsilon, alpha, beta must be four (S, *rows, D) tensors of one shape" % who)


def evidential_f64(gamma, upsilon, alpha, beta):
    """The formulas of mc_evidential in float64 torch, rounded to float32 at the end (the CPU path of
    BayesianNetworkModule.predictive_evidential): four (S, *rows, D) tensors, the stacked per-sample head outputs.  The variance
    of gamma is the two-pass population variance."""
    _evidential_shapes((gamma, upsilon, alpha, beta), "evidential_f64")
    g, u, a, b = (t.detach().to(torch.float64) for t in (gamma, upsilon, alpha, beta))
    ale_s = b / (a - 1)
    mean = g.mean(0)
    ale = ale_s.mean(0)
    epi = (ale_s / u).mean(0) + ((g - mean) ** 2).mean(0)
    f32 = lambda t: t.to(torch.float32)         # noqa: E731
    return PredictiveRegression(f32(mean), f32(ale + epi), f32(ale), f32(epi))


def mc_evidential(gamma, upsilon, alpha, beta):
    """Predictive moments of the equal-weight mixture of S evidential heads over the leading MC axis in ONE launch
    (bnn_mc_evidential) -> PredictiveRegression: mean = mean_s gamma_s, aleatoric = mean_s beta / (alpha - 1), epistemic =
    mean_s beta / (upsilon (alpha - 1)) + Var_s(gamma_s), total = aleatoric + epistemic.  Four CUDA fp32 (S, *rows, D) tensors
    (made contiguous if they are not).  S = 1: gamma and NormalInverseGaussianUncertainty's two outputs, bit for bit.  The
    sums over samples are fp64 in a fixed order: bitwise reproducible."""
    ts = (gamma, upsilon, alpha, beta)
    _evidential_shapes(ts, "mc_evidential")
    if not _is_dev_f32(*ts):
        raise BnnHipError("mc_evidential: gamma, upsilon, alpha, beta must be CUDA/HIP float32 tensors")
    g, u, a, b = (t.detach().contiguous() for t in ts)
    S, D = g.shape[0], g.shape[-1]
    rows_shape = tuple(g.shape[1:-1])
    rows = 1
    for d in rows_shape:
        rows *= d
    mean, total, ale, epi = (torch.empty(rows_shape + (D,), dtype=torch.float32, device=g.device) for _ in range(4))
    check(_lib.load().bnn_mc_evidential(ptr(g), ptr(u), ptr(a), ptr(b), rows * D, S, rows, D, ptr(mean), ptr(total), ptr(ale),
                                        ptr(epi), stream_ptr(g.device)), "bnn_mc_evidential")
    return PredictiveRegression(mean, total, ale, epi)


# --------------------------------------------------------------------------- training-loop callers
class _SoftmaxXent(torch.autograd.Function):
    """CrossEntropyLoss()(logits, target), reduction 'mean' (examples/MNIST/train.py:39,59-61): the loss
    and d loss / d logits in one HIP pass."""

    @staticmethod
    def forward(ctx, logits, target):
        require_cuda_f32(logits, "logits")
        if target.dtype != torch.int64 or not target.is_cuda:
            raise BnnHipError("cross_entropy: target must be a CUDA int64 tensor")
        R, C = logits.shape
        if target.numel() != R:
            raise BnnHipError("cross_entropy: %d targets for %d rows" % (target.numel(), R))
        lib = _lib.load()
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        g = torch.empty_like(logits) if logits.requires_grad else None
        ws = torch.empty(lib.bnn_xent_workspace_bytes(R) // 8, dtype=torch.float64, device=logits.device)
        check(lib.bnn_softmax_xent(ptr(logits), ptr(target), R, C, ptr(loss), ptr(g), ptr(ws),
                                   stream_ptr(logits.device)), "bnn_softmax_xent")
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, up):
        (g,) = ctx.saved_tensors
        return (g * up if g is not None else None), None


def cross_entropy(logits, target):
    """Mean cross-entropy of (rows, classes) fp32 logits against int64 class indices.

    A target outside [0, classes) (compared as int64; there is no ignore_index) makes the loss NaN and that row of the
    gradient NaN; the other gradient rows are unaffected and nothing outside the row is read.  The check runs on the device:
    no host synchronisation, the call stays graph-capturable."""
    return _SoftmaxXent.apply(logits.contiguous(), target.contiguous())


def prune_score(mu, rho):
    """log N(0; mu, sigma(rho)) element-wise (PruneNormal's ranking score, prune/prune.py:11)."""
    require_cuda_f32(mu, "mean")
    require_cuda_f32(rho, "scale")
    mu_c, rho_c = mu.detach().contiguous(), rho.detach().contiguous()
    out = torch.empty_like(mu_c)
    check(_lib.load().bnn_prune_score(ptr(mu_c), ptr(rho_c), ptr(out), mu_c.numel(), stream_ptr(mu_c.device)),
          "bnn_prune_score")
    return out
