"""Flipout layers on the MC-batched device path (bnn_flipout_signs, bnn_conv2d_flipout_forward_mc, bnn_draw_multi kind BNN_DRAW_FLIPOUT,
bnn_flipout_weight_backward; ops.flipout_signs, ops.conv2d_flipout_mc, ops.linear_flipout_mc; FlipOutNormalConv{1,2,3}d and
FlipoutNormalLinear inside an McContext) -- the reference's FashionMNIST example (examples/FashionMNIST/model.py) with signs
of their own for every MC sample.

CPU: a NumPy twin of the Flipout-sign contract (include/bnn_hip.h) on the oracle's Philox core, its layout and statistics, the
argument errors of every new C-ABI entry, and the unchanged serial CPU path.
GPU: the FashionMNIST-shaped net against float64 on the twin's signs (forward, uncertainty, training), the fused kernel's signs
bit for bit, the 1-d and 3-d layers, launch counts, graph replay, and a spill check of the keyed kernel."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import seeded
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, _rng, ops
from bayesianneuralnetworks_amd._rng import DrawKey
from bayesianneuralnetworks_amd.nn import (BayesianNetworkModule, FlipOutNormalConv1d, FlipOutNormalConv2d, FlipOutNormalConv3d,
                                           FlipoutNormalLinear)
from oracle import oracle as orc

gpu = pytest.mark.gpu
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN, E_RANGE, E_UNSUPPORTED = -1, -2, -3, -4, -5, -6     # BNN_E_* (include/bnn_hip.h)
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the twin
def philox_np(c, k0, k1, rounds):
    """Philox4x32-`rounds` on arrays of counters: c = (c0, c1, c2, c3) uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & M32 for v in c)
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(rounds):
        p0 = c0 * np.uint64(0xD2511F53)
        p1 = c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def sign_uniforms(seed, stream, sample, epoch_host, epoch_dev, n, gen):
    """The contract's uniform u of elements 0 .. n - 1 of one sample, fp32 (the dropout mask's uniforms)."""
    e = np.arange(n, dtype=np.uint64)
    ctr1 = np.uint64(((stream << 16) | (sample & 0xFFFF)) & 0xFFFFFFFF)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    if gen == _rng.GEN_PHILOX10_U24:
        nb = (n + 3) // 4
        b = np.arange(nb, dtype=np.uint64)
        w = np.stack(philox_np((b, np.full(nb, ctr1), np.full(nb, epoch_host), np.full(nb, epoch_dev)), k0, k1, 10), 1)
        x = w.reshape(-1)[:n]
        return (((x >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)
    nb = (n + 7) // 8
    b = np.arange(nb, dtype=np.uint64)
    w = np.stack(philox_np((b, np.full(nb, ctr1), np.full(nb, epoch_host), np.full(nb, epoch_dev)), k0, k1, 7), 1)
    word = w[(e >> np.uint64(3)).astype(np.int64), ((e & np.uint64(7)) >> np.uint64(1)).astype(np.int64)]
    h = np.where((e & np.uint64(1)) == 0, word & np.uint64(0xFFFF), word >> np.uint64(16))
    return ((h.astype(np.float64) + 0.5) * 2.0 ** -16).astype(np.float32)


def sign_twin(key, s, epoch_dev, rows, width):
    """(rows, width) float64 +-1 signs of sample key.sample0 + s: -1 iff u < 0.5."""
    u = sign_uniforms(key.seed, key.stream, key.sample0 + s, key.epoch_host, (epoch_dev + key.epoch_dev_delta) & 0xFFFFFFFF,
                      rows * width, key.gen)
    return np.where(u < np.float32(0.5), -1.0, 1.0).reshape(rows, width)


def conv_signs(key, s, epoch_dev, B, O, C):
    """-> R (B, O), S (B, C) of the conv layout e = b (O + C) + j."""
    v = sign_twin(key, s, epoch_dev, B, O + C)
    return v[:, :O], v[:, O:]


def linear_signs(key, s, epoch_dev, O, K):
    """-> R (O,), S (K,) of the linear layout v[0:O] | v[O:O+K]."""
    v = sign_twin(key, s, epoch_dev, 1, O + K)[0]
    return v[:O], v[O:]


# ------------------------------------------------------------------------------------------------ CPU
def test_twin_philox_is_the_oracle_core():
    rng = np.random.default_rng(5)
    for rounds, fn in ((10, lambda c, k: orc.philox4x32_10(c, k)), (7, lambda c, k: orc.philox4x32_r(c, k, 7))):
        for _ in range(16):
            c = rng.integers(0, 2 ** 32, 4, dtype=np.uint64)
            k = rng.integers(0, 2 ** 32, 2, dtype=np.uint64)
            got = philox_np(tuple(np.array([v]) for v in c), int(k[0]), int(k[1]), rounds)
            want = fn(c.astype(np.uint32), k.astype(np.uint32))
            assert [int(g[0]) for g in got] == [int(v) for v in want]


@pytest.mark.parametrize("gen", [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16])
def test_twin_sign_layout(gen):
    # conv: element b (O + C) + j is R[b][j] (j < O) or S[b][j - O]; linear: one row R | S -- spelled out with the oracle's blocks
    seed, stream, sample, eh, ed = 0x0123_4567_89AB_CDEF, 9, 2, 5, 3
    key = DrawKey(seed, stream, sample, 1, eh, gen=gen)
    B, O, C = 3, 5, 7
    R, S = conv_signs(key, 0, ed, B, O, C)
    kk = [seed & 0xFFFFFFFF, seed >> 32]
    for b in range(B):
        for j in range(O + C):
            e = b * (O + C) + j
            if gen == _rng.GEN_PHILOX10_U24:
                x = int(orc.philox4x32_10([e // 4, (stream << 16) | sample, eh, ed], kk)[e % 4])
                u = np.float32(((x >> 8) + 0.5) * 2.0 ** -24)
            else:
                w = int(orc.philox4x32_r([e // 8, (stream << 16) | sample, eh, ed], kk, 7)[(e % 8) // 2])
                u = np.float32((((w & 0xFFFF) if e % 2 == 0 else (w >> 16)) + 0.5) * 2.0 ** -16)
            want = -1.0 if u < np.float32(0.5) else 1.0
            assert (R[b, j] if j < O else S[b, j - O]) == want
    r, s = linear_signs(key, 0, ed, O, C)
    v = sign_twin(key, 0, ed, 1, O + C)[0]
    assert np.array_equal(r, v[:O]) and np.array_equal(s, v[O:])


@pytest.mark.parametrize("gen", [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16])
def test_twin_sign_fraction(gen):
    v = sign_twin(DrawKey(424242, 17, 0, 1, 3, gen=gen), 0, 0, 300, 400)
    assert set(np.unique(v)) == {-1.0, 1.0}
    assert abs((v > 0).mean() - 0.5) < 1e-2


def _rng_arg(gen=0, stream=3):
    r = _lib.Rng()
    r.seed, r.stream, r.sample0, r.epoch_host, r.epoch_dev_delta, r.epoch_dev, r.generator = 1, stream, 0, 0, 0, None, gen
    return r


FAKE = ctypes.c_void_p(1 << 20)           # never dereferenced: every call below is refused before a launch
FAKE2 = ctypes.c_void_p((1 << 20) + 2)    # 2-B aligned only


def test_flipout_signs_entry_refuses_bad_arguments():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    r = ctypes.byref(_rng_arg())
    call = lambda o=FAKE, os_=64, rows=4, w=16, s=2, rng=r: lib.bnn_flipout_signs(o, os_, rows, w, s, rng, None)
    assert call(o=None) == E_NULL
    assert call(rng=None) == E_NULL
    assert call(w=0) == E_SHAPE
    assert call(s=0) == E_SHAPE
    assert call(s=65536) == E_RANGE
    assert call(rows=1 << 20, w=1 << 12, os_=1 << 32) == E_RANGE
    assert call(os_=10) == E_SHAPE
    assert call(o=FAKE2) == E_ALIGN
    assert call(rng=ctypes.byref(_rng_arg(stream=1 << 16))) == E_RANGE
    assert call(rng=ctypes.byref(_rng_arg(gen=9))) == E_RANGE
    assert lib.bnn_launch_count() == n0


def test_flipout_weight_backward_entry_refuses_bad_arguments():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    r = ctypes.byref(_rng_arg())
    call = lambda g=FAKE, gs=80, rho=FAKE, gm=FAKE, gr=FAKE, O=8, K=10, s=2, rng=r: \
        lib.bnn_flipout_weight_backward(g, gs, rho, gm, gr, O, K, s, rng, None)
    for kw in ("g", "rho", "gm", "gr"):
        assert call(**{kw: None}) == E_NULL
    assert call(rng=None) == E_NULL
    assert call(O=0) == E_SHAPE
    assert call(K=0) == E_SHAPE
    assert call(gs=79) == E_SHAPE
    assert call(s=65536) == E_RANGE
    assert call(gm=FAKE2) == E_ALIGN
    assert lib.bnn_launch_count() == n0


def test_conv2d_flipout_mc_entry_refuses_bad_arguments():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    r = ctypes.byref(_rng_arg())

    def shape(B=3, C=64, H=6, W=6, O=64, groups=1):
        sh = _lib.Conv2dShape()
        sh.B, sh.C, sh.H, sh.W, sh.O, sh.KH, sh.KW = B, C, H, W, O, 3, 3
        sh.stride_h = sh.stride_w = 2
        sh.pad_h = sh.pad_w = 1
        sh.dil_h = sh.dil_w = 1
        sh.groups = groups
        return sh

    def call(x=FAKE, xs=0, w=FAKE, ldw=576, y=FAKE, ys=3 * 64 * 9, sh=None, s=4, rng=r, flags=0):
        return lib.bnn_conv2d_flipout_forward_mc(x, xs, w, ldw, y, ys, ctypes.byref(sh or shape()), s, rng, flags, None)
    assert call(x=None) == E_NULL
    assert call(w=None) == E_NULL
    assert call(y=None) == E_NULL
    assert call(rng=None) == E_NULL
    assert call(xs=7) == E_SHAPE                    # neither shared (0) nor a whole sample apart
    assert call(ys=-1) == E_SHAPE
    assert call(s=0) == E_SHAPE
    assert call(s=65536) == E_RANGE
    assert call(rng=ctypes.byref(_rng_arg(gen=5))) == E_RANGE
    assert call(flags=1) == E_UNSUPPORTED
    assert call(sh=shape(O=128)) == E_UNSUPPORTED   # 2 O = 256: not a tile of the kernel
    assert call(sh=shape(C=96)) == E_UNSUPPORTED
    assert call(w=FAKE2) == E_UNSUPPORTED
    assert lib.bnn_launch_count() == n0


def test_draw_multi_refuses_a_flipout_draw_with_taps():
    lib = _lib.load()
    arr = (_lib.DrawTensor * 1)()
    t = arr[0]
    t.mu = t.rho = t.out = 1 << 20
    t.rows, t.cols, t.ld, t.out_sample_stride, t.out_dtype = 8, 72, 128, 1024, _lib.BF16
    t.kind, t.taps = _lib.DRAW_FLIPOUT, 9
    assert lib.bnn_draw_multi(arr, 1, 2, None, 0, None, None) == E_SHAPE
    t.kind, t.taps = 5, 0
    assert lib.bnn_draw_multi(arr, 1, 2, None, 0, None, None) == E_RANGE


class FashionNet(BayesianNetworkModule):
    """examples/FashionMNIST/model.py"""

    def __init__(self, in_channels=1, out_channels=10, samples=10):
        super().__init__(in_channels, out_channels, samples)
        self.layers = torch.nn.Sequential(
            torch.nn.Conv2d(in_channels, 32, 5, padding=2, stride=2), torch.nn.BatchNorm2d(32), torch.nn.ELU(),
            torch.nn.Conv2d(32, 32, 3, padding=1, stride=1), torch.nn.ELU(),
            torch.nn.Conv2d(32, 64, 3, padding=0, stride=2), torch.nn.ELU(),
            FlipOutNormalConv2d(64, 64, 3, padding=1, stride=2), torch.nn.ELU(),
            torch.nn.Flatten(),
            FlipoutNormalLinear(576, out_channels),
            torch.nn.Softmax(dim=-1))

    def _forward(self, x):
        return self.layers(x)


def test_serial_cpu_path_is_the_reference():
    torch.manual_seed(0)
    first = _rng.new_stream_id()
    net = FashionNet(samples=3).eval()
    after = _rng.new_stream_id()
    net.mc_batched = True                                 # (a CPU input runs the serial loop anyway)
    x = torch.randn(4, 1, 28, 28)
    torch.manual_seed(21)
    ys = net(x)
    torch.manual_seed(21)
    conv, lin = net.layers[7], net.layers[10]
    with torch.no_grad():
        for y in ys:
            h = net.layers[:7](x)
            R = (torch.rand(4, 64, 1, 1) - .5).sign()
            S = (torch.rand(4, 64, 1, 1) - .5).sign()
            out = F.conv2d(h, conv.weight.mean, None, 2, 1) + F.conv2d(h * S, conv.weight.stddev, None, 2, 1) * R
            h = F.elu(out).flatten(1)
            r = (torch.rand(10) - .5).sign()
            s = (torch.rand(576) - .5).sign()
            want = torch.softmax(F.linear(h, lin.weight.mean, torch.matmul(h * s, lin.weight.stddev.t()) * r), -1)
            assert torch.equal(y, want)
    assert conv.flip_key is None and lin.flip_key is None and conv._flip_stream is None and lin._flip_stream is None
    assert _rng.new_stream_id() == after + 1 and after > first


# ------------------------------------------------------------------------------------------------ GPU helpers
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


def _epoch_dev(dev):
    return int(_rng.default_generator.epoch_dev(dev)[0].item())


def _scaled_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / max(1.0, float(want.abs().max())))


def _flip_conv64(h, mean, std, key, s, ed, stride, padding, dilation=1, conv=F.conv2d):
    """conv.py:207-221 in float64 on the twin's signs of sample s."""
    B, C = h.shape[:2]
    O = mean.shape[0]
    R, S = conv_signs(key, s, ed, B, O, C)
    nd = h.dim() - 2
    R = torch.from_numpy(R).reshape(B, O, *([1] * nd))
    S = torch.from_numpy(S).reshape(B, C, *([1] * nd))
    return conv(h, mean, None, stride, padding, dilation) + conv(h * S, std, None, stride, padding, dilation) * R


def _flip_linear64(h, mean, std, key, s, ed):
    """dense.py:70-83 in float64 on the twin's signs of sample s."""
    O, K = mean.shape
    r, sg = linear_signs(key, s, ed, O, K)
    return F.linear(h, mean) + F.linear(h * torch.from_numpy(sg), std) * torch.from_numpy(r)


def _fashion_ref(net, h_in, S, ed, params=None):
    """float64 of the net behind the prefix for every sample on the recorded keys: h_in (B, 64, 6, 6) -> (S, B, 10)."""
    conv, lin = net.layers[7], net.layers[10]
    cm, cs, lm, ls = params or [t.detach().cpu().double() for t in (conv.weight.mean, conv.weight.stddev, lin.weight.mean,
                                                                     lin.weight.stddev)]
    outs = []
    for s in range(S):
        h = F.elu(_flip_conv64(h_in, cm, cs, conv.flip_key, s, ed, 2, 1)).flatten(1)
        outs.append(torch.softmax(_flip_linear64(h, lm, ls, lin.flip_key, s, ed), -1))
    return torch.stack(outs)


def _capture_input(layer):
    box = []
    hnd = layer.register_forward_pre_hook(lambda m, a: box.append(a[0].detach()))
    return box, hnd


# ------------------------------------------------------------------------------------------------ GPU: the bug
@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_fashion_batched_samples_differ_and_match_the_twin(dev, mode):
    bnn.set_compute(mode)
    S, B = 8, 32
    torch.manual_seed(1)
    net = FashionNet(samples=S).to(dev).eval()
    seeded.pin_streams(net, 1000)
    net.mc_batched = True
    bnn.manual_seed(77)
    x = torch.randn(B, 1, 28, 28, device=dev)
    box, hnd = _capture_input(net.layers[7])
    with torch.no_grad():
        ys = torch.stack(net(x))
    hnd.remove()
    assert ys.shape == (S, B, 10)
    flat = ys.reshape(S, -1)
    for a in range(S):
        for b in range(a + 1, S):
            assert not torch.equal(flat[a], flat[b]), (a, b)
    kc, kl = net.layers[7].flip_key, net.layers[10].flip_key
    assert kc is not None and kl is not None and kc.stream != kl.stream and kc.nsamples == kl.nsamples == S
    assert kc.gen == _rng.generator_for(mode)
    assert len(box) == 1 and box[0].shape == (B, 64, 6, 6)          # the prefix ran once, on the un-replicated batch
    want = _fashion_ref(net, box[0].cpu().double(), S, _epoch_dev(dev))
    err = _scaled_err(ys, want)
    assert err <= (2e-5 if mode == "f32" else 2e-2), err


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_fashion_predictive_uncertainty_has_epistemic_part(dev, mode):
    bnn.set_compute(mode)
    S, B = 8, 48
    torch.manual_seed(2)
    net = FashionNet(samples=S).to(dev).eval()
    seeded.pin_streams(net, 1010)
    net.mc_batched = True
    bnn.manual_seed(5)
    x = torch.randn(B, 1, 28, 28, device=dev)
    box, hnd = _capture_input(net.layers[7])
    with torch.no_grad():
        u = net.predictive_uncertainty(x, inputs="probs")
    hnd.remove()
    assert float(u.epistemic.min()) > 0.0
    want = ops.uncertainty_f64(_fashion_ref(net, box[0].cpu().double(), S, _epoch_dev(dev)).float(), "probs")
    tol = 1e-4 if mode == "f32" else 3e-2
    for name in ("mean", "total", "aleatoric", "epistemic"):
        err = _scaled_err(getattr(u, name), getattr(want, name))
        assert err <= tol, (name, err)


@gpu
def test_sample_false_reuses_the_recorded_signs(dev):
    torch.manual_seed(4)
    net = FashionNet(samples=4).to(dev).eval()
    net.mc_batched = True
    x = torch.randn(8, 1, 28, 28, device=dev)
    with torch.no_grad():
        a = net.forward_stacked(x)
        conv, lin = net.layers[7], net.layers[10]
        key = conv.flip_key
        with _mc.McContext(4, 8):
            h = net.layers[:7](x)
            y1 = conv(h, sample=False)
        assert conv.flip_key is key
        with _mc.McContext(3, 8):
            with pytest.raises(RuntimeError, match="sample=False"):
                conv(h, sample=False)
            with pytest.raises(RuntimeError, match="mc_batched"):
                lin(torch.randn(5, 576, device=dev))
    assert y1.shape == (32, 64, 3, 3)
    assert a.shape == (4, 8, 10)


# ------------------------------------------------------------------------------------------------ GPU: kernel parity
def _key(S, gen, stream=1234, epoch=29, sample0=0):
    return DrawKey(0xFEEDFACE87654321, stream, sample0, S, epoch, gen=gen)


def _int_weights(O, C, dev, seed):
    """Small-integer mean / stddev (O, C, 3, 3) and their bf16 [mean | stddev] tap-major operand: every MFMA sum is exact."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randint(-2, 3, (O, C, 3, 3), generator=g).double()
    std = torch.randint(-2, 3, (O, C, 3, 3), generator=g).double()
    K = C * 9
    kp = (K + 63) // 64 * 64
    w2 = torch.zeros(2 * O, kp, dtype=torch.bfloat16)
    for i, t in enumerate((mean, std)):
        w2[i * O:(i + 1) * O, :K] = t.permute(0, 2, 3, 1).reshape(O, K).to(torch.bfloat16)       # column tap * C + c
    return mean, std, w2.to(dev), kp


@gpu
@pytest.mark.parametrize("O", [32, 64])
@pytest.mark.parametrize("S", [1, 3, 8, 100])
@pytest.mark.parametrize("gen", [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16])
@pytest.mark.parametrize("shared", [True, False])
def test_fused_kernel_signs_are_the_twin(dev, O, S, gen, shared):
    B, C = 7, 64                                          # odd B: a ragged image tile
    mean, std, w2, kp = _int_weights(O, C, dev, O + S)
    key = _key(S, gen, sample0=3)
    g = torch.Generator().manual_seed(S)
    x = torch.randint(-2, 3, ((B if shared else S * B), C, 6, 6), generator=g).float()
    sh = _lib.Conv2dShape()
    sh.B, sh.C, sh.H, sh.W, sh.O, sh.KH, sh.KW = B, C, 6, 6, O, 3, 3
    sh.stride_h = sh.stride_w = 2
    sh.pad_h = sh.pad_w = 1
    sh.dil_h = sh.dil_w = 1
    sh.groups = 1
    xd = x.to(dev)
    y = torch.full((S * B, O, 3, 3), float("nan"), device=dev)
    r = ops._rng_struct(key, dev)
    _lib.check(_lib.load().bnn_conv2d_flipout_forward_mc(_lib.ptr(xd), 0 if shared else B * C * 36, _lib.ptr(w2), kp, _lib.ptr(y),
                                                         B * O * 9, ctypes.byref(sh), S, ctypes.byref(r), 0, _lib.stream_ptr(dev)),
               "bnn_conv2d_flipout_forward_mc")
    got = y.cpu().double()
    ed = _epoch_dev(dev)
    xs = x.double()
    for s in range(S):
        h = xs if shared else xs[s * B:(s + 1) * B]
        want = _flip_conv64(h, mean, std, key, s, ed, 2, 1)
        assert torch.equal(got[s * B:(s + 1) * B], want), s


@gpu
@pytest.mark.parametrize("gen", [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16])
def test_flipout_signs_kernel_is_the_twin(dev, gen):
    S, rows, width = 5, 9, 77
    key = _key(S, gen, sample0=2)
    got = ops.flipout_signs(key, rows, width, dev).cpu().double().numpy()
    for s in range(S):
        assert np.array_equal(got[s], sign_twin(key, s, _epoch_dev(dev), rows, width)), s


@gpu
@pytest.mark.parametrize("gen", [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16])
def test_flipout_draw_is_mean_plus_sigma_sign_outer_product(dev, gen):
    S, O, K = 4, 10, 72
    key = _key(S, gen)
    mu = torch.randn(O, K, device=dev)
    rho = torch.randn(O, K, device=dev) - 2
    w = ops.flipout_draw(mu, rho, key).cpu().double()
    sig = F.softplus(rho.cpu().double()) + 1e-10
    for s in range(S):
        r, sg = linear_signs(key, s, _epoch_dev(dev), O, K)
        want = mu.cpu().double() + sig * torch.from_numpy(np.outer(r, sg))
        assert (w[s] - want).abs().max() <= 2e-6, s


# ------------------------------------------------------------------------------------------------ GPU: launches, graphs
@gpu
def test_bf16_inference_pass_launches(dev):
    """Flipout conv: the bf16 [mean | stddev] operand (one draw launch) and ONE contraction launch for all S samples.  Flipout
    linear: its draw rides in the network's one draw launch; then one dense launch.  Four HIP launches in all."""
    bnn.set_compute("bf16")
    lib = _lib.load()
    torch.manual_seed(6)
    net = FashionNet(samples=8).to(dev).eval()
    seeded.pin_streams(net, 1020)
    net.mc_batched = True
    x = torch.randn(64, 1, 28, 28, device=dev)
    with torch.no_grad():
        net.forward_stacked(x)
        torch.cuda.synchronize()
        n0 = lib.bnn_launch_count()
        y = net.forward_stacked(x)
        torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 4, lib.bnn_launch_count() - n0
    assert y.shape == (8, 64, 10)
    _lib.check_device(dev)


@gpu
def test_captured_graph_replays_fresh_signs(dev):
    bnn.set_compute("bf16")
    torch.manual_seed(7)
    net = FashionNet(samples=4).to(dev).eval()
    seeded.pin_streams(net, 1030)
    net.mc_batched = True
    x = torch.randn(16, 1, 28, 28, device=dev)
    cell = _rng.default_generator.epoch_dev(dev)
    lib = _lib.load()
    with torch.no_grad():
        net.forward_stacked(x)                            # warm up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = net.forward_stacked(x)
            _lib.check(lib.bnn_rng_advance(ctypes.c_void_p(cell.data_ptr()), 1, _lib.stream_ptr(dev)), "bnn_rng_advance")
        g.replay()
        torch.cuda.synchronize()
        a = y.clone()
        g.replay()
        torch.cuda.synchronize()
    assert not torch.equal(a, y)
    flat = y.reshape(4, -1)
    assert not torch.equal(flat[0], flat[1])
    _lib.check_device(dev)


# ------------------------------------------------------------------------------------------------ GPU: training
@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_fashion_training_gradients(dev, mode):
    bnn.set_compute(mode)
    S, B = 4, 16
    torch.manual_seed(3)
    net = FashionNet(samples=S).to(dev).train()
    seeded.pin_streams(net, 1040)
    net.mc_batched = True
    ref_net = FashionNet(samples=S).double().train()
    ref_net.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.cpu() for k, v in net.state_dict().items()})
    bnn.manual_seed(9)
    x = torch.randn(B, 1, 28, 28, device=dev)
    t = torch.randint(0, 10, (B,), device=dev)
    preds = net(x)
    kl = net.kl_divergence(100)
    loss = torch.stack([F.cross_entropy(p, t) for p in preds]).mean() + kl
    loss.backward()
    # float64 autograd on the twin signs of the recorded keys; the prefix in float64 too
    conv, lin = net.layers[7], net.layers[10]
    rconv, rlin = ref_net.layers[7], ref_net.layers[10]
    ed = _epoch_dev(dev)
    h = ref_net.layers[:7](x.cpu().double())
    cm, cs = rconv.weight.mean, F.softplus(rconv.weight.scale) + 1e-10
    lm, ls = rlin.weight.mean, F.softplus(rlin.weight.scale) + 1e-10
    outs = []
    for s in range(S):
        hh = F.elu(_flip_conv64(h, cm, cs, conv.flip_key, s, ed, 2, 1)).flatten(1)
        outs.append(F.cross_entropy(torch.softmax(_flip_linear64(hh, lm, ls, lin.flip_key, s, ed), -1), t.cpu()))
    (torch.stack(outs).mean() + ref_net.kl_divergence(100)).backward()
    pairs = [(conv.weight.mean, rconv.weight.mean), (conv.weight.scale, rconv.weight.scale),
             (lin.weight.mean, rlin.weight.mean), (lin.weight.scale, rlin.weight.scale),
             (net.layers[5].weight, ref_net.layers[5].weight), (net.layers[0].weight, ref_net.layers[0].weight)]
    tol = 1e-4 if mode == "f32" else 3e-2
    for i, (q, r) in enumerate(pairs):
        err = _scaled_err(q.grad, r.grad)
        assert err <= tol, (i, err)


# ------------------------------------------------------------------------------------------------ GPU: 1-d and 3-d
class OneLayer(BayesianNetworkModule):
    def __init__(self, layer, samples):
        super().__init__(1, 1, samples)
        self.layer = layer

    def _forward(self, x):
        return self.layer(x)


@gpu
@pytest.mark.parametrize("kind,mode", [("1d", "f32"), ("1d", "bf16"), ("3d", "f32")])
def test_flipout_conv_1d_3d_batched(dev, kind, mode):
    bnn.set_compute(mode)
    S, B, C, O = 4, 5, 64, 32
    torch.manual_seed(8)
    if kind == "1d":
        layer = FlipOutNormalConv1d(C, O, 3, stride=2, padding=1)
        x = torch.randn(B, C, 11, device=dev)
        conv = F.conv1d
    else:
        layer = FlipOutNormalConv3d(C, O, 3, stride=1, padding=1)
        x = torch.randn(B, C, 3, 4, 4, device=dev)
        conv = F.conv3d
    net = OneLayer(layer.to(dev), S)
    net.mc_batched = True
    with torch.no_grad():
        y = net.forward_stacked(x)
    key = layer.flip_key
    assert key is not None and key.nsamples == S
    mean, std = layer.weight.mean.detach().cpu().double(), layer.weight.stddev.detach().cpu().double()
    want = torch.stack([_flip_conv64(x.cpu().double(), mean, std, key, s, _epoch_dev(dev), layer.stride, layer.padding,
                                     layer.dilation, conv) for s in range(S)])
    err = _scaled_err(y, want)
    assert err <= (2e-5 if mode == "f32" else 2e-2), err
    assert not torch.equal(y[0], y[1])


# ------------------------------------------------------------------------------------------------ code object
def _code_object_notes():
    tools = ["/opt/rocm/llvm/bin/llvm-objcopy", "/opt/rocm/llvm/bin/clang-offload-bundler", "/opt/rocm/llvm/bin/llvm-readelf"]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not found")
    notes = ""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([tools[0], "--dump-section=.hip_fatbin=" + fat, _lib.LIB_PATH, os.path.join(d, "lib.so")])
        blob = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        for i, a in enumerate(starts):
            part, co = os.path.join(d, "b%d.bin" % i), os.path.join(d, "b%d.co" % i)
            open(part, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.check_call([tools[1], "--unbundle", "--type=o", "--input=" + part,
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
            notes += subprocess.check_output([tools[2], "--notes", co]).decode()
    return notes


def test_keyed_flipout_conv_does_not_spill():
    """The keyed instantiations (NS samples per workgroup: 1, 2, 4 at 2 O = 64; 1, 2 at 2 O = 128) keep their accumulators --
    the mean block and one stddev block per sample -- and the samples' sign masks in registers."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    keyed = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn11k_conv_bf16I.*Lb1ELb0ELi[1-9]EEEvNS_10ConvParamsE$", n)}
    assert len(keyed) == 5, sorted(keyed)
    for n, f in keyed.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("private_segment_fixed_size", 0)) == 0, (n, f)


def test_flipout_draw_keeps_the_draw_kernel_registers():
    """The Flipout draw's sign blocks live in a block of their own with a sample loop that is not unrolled: k_draw_multi (one
    instantiation: the unrolled ones left with their A/B knob) keeps the occupancy of the plain draw (4 waves per SIMD, <= 128
    VGPRs) -- inside an unrolled loop they had doubled the register count of every draw, Flipout or not."""
    notes = _code_object_notes()
    seen = 0
    for block in notes.split("- .agpr_count")[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|vgpr_spill_count):\s+(\S+)", block))
        if re.match(r"_ZN3bnn12k_draw_multi(ILi\d+EEEv|E)NS_10DrawLaunchE$", f.get("name", "")):
            seen += 1
            assert int(f["vgpr_count"]) <= 128 and int(f.get("vgpr_spill_count", 0)) == 0, f
    assert seen == 1
