"""FlipOutNormalConv3d on the device: one keyed sign launch + the Flipout implicit GEMM of csrc/bnn_conv3d.hip for all S MC samples,
forward and backward, against float64 torch conv3d of the reference expression (conv.py:237-251) on the twin's signs.

bf16 bounds are derived, not blanket: the reference is float64 on the operands the kernel contracts -- x and gy rounded to bf16,
the mean and stddev rows the operand draw wrote -- so what is left is fp32 accumulation: at most (L + c) 2^-24 sum |a b| for a
reduction of L products, c covering the epilogue / fold / slab / sample additions, and a few 2^-24 for softplus'."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_scaled
import seeded

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, _rng, ops
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, FlipOutNormalConv3d, NormalConv3d, NormalLinear
from test_flipout_mc import conv_signs, _flip_conv64, _epoch_dev, _key, _code_object_notes

U = 2.0 ** -24
gpu = pytest.mark.gpu


def N(t):
    return t.detach().double().cpu().numpy()


def bf(t):
    return t.float().to(torch.bfloat16).double()


def assert_within(got, ref, bound, what):
    got, ref, bound = (np.asarray(v, dtype=np.float64) for v in (got, ref, bound))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    ex = err - bound
    i = int(np.argmax(ex))
    assert (ex <= 0).all(), "%s: |err| %.3e > derived bound %.3e (%d of %d out)" % (
        what, err.reshape(-1)[i], bound.reshape(-1)[i], int((ex > 0).sum()), ex.size)


# ------------------------------------------------------------------------------------------------ CPU
ENTRIES = ("bnn_conv3d_flipout_forward", "bnn_conv3d_flipout_backward_input", "bnn_conv3d_flipout_backward_weight_workspace_bytes",
           "bnn_conv3d_flipout_backward_weight")


def test_flipout_conv3d_entries_resolve():
    import ctypes
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name


def test_flipout_conv3d_workspace_query_refuses_what_the_entries_refuse():
    lib = _lib.load()
    sh, _ = ops._conv3d_shape((2, 4, 5, 5, 5), (6, 4, 3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 1)
    assert lib.bnn_conv3d_flipout_backward_weight_workspace_bytes(ctypes_ref(sh), 3) > 0
    sh2, _ = ops._conv3d_shape((2, 4, 5, 5, 5), (6, 2, 3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 2)
    assert lib.bnn_conv3d_flipout_backward_weight_workspace_bytes(ctypes_ref(sh2), 3) == -1           # groups != 1
    assert not ops.conv3d_flipout_eligible((2, 4, 5, 5, 5), (6, 2, 3, 3, 3), 3, (1, 1, 1), (1, 1, 1), (1, 1, 1), 2)
    assert ops.conv3d_flipout_eligible((2, 4, 5, 5, 5), (6, 4, 3, 3, 3), 3, (1, 1, 1), (1, 1, 1), (1, 1, 1), 1)
    big = (1, 2048, 1024, 1024, 2)                                                                     # 2^32 input elements
    assert not ops.conv3d_flipout_eligible(big, (4, 2048, 1, 1, 1), 1, (1, 1, 1), (0, 0, 0), (1, 1, 1), 1)


def ctypes_ref(sh):
    import ctypes
    return ctypes.byref(sh)


def test_flipout_conv3d_tiles_do_not_spill():
    """Every Flipout instantiation of k_conv3d (FWD, DGRAD, WGRAD x bf16, fp32) keeps both accumulator sets in registers."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    flip = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn8k_conv3dI[tf]Li[012]ELb1EEEvNS_9Conv3dGeoENS_10Conv3dArgsE$", n)}
    assert len(flip) == 6, sorted(kernels)
    for n, f in flip.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("private_segment_fixed_size", 0)) == 0, (n, f)


# ------------------------------------------------------------------------------------------------ GPU helpers
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


def _operands(layer, mode):
    """(mean, stddev) float64 as the kernel contracts them: the rows of the operand draw (bf16 mode), or float64 softplus."""
    mean, scale = layer.weight.mean.detach(), layer.weight.scale.detach()
    if mode == "f32":
        return mean.double().cpu(), (F.softplus(scale.double()) + 1e-10).cpu()
    w = ops._flip3d_operands(mean.contiguous(), scale.contiguous(), _lib.COMPUTE_BF16).double().cpu()
    n = mean.numel()
    m, sd = w[0, :n].reshape(mean.shape), w[1, :n].reshape(mean.shape)
    want = (F.softplus(scale.double()) + 1e-10).cpu()
    assert torch.equal(m, bf(mean.cpu()))
    assert ((sd - want).abs() <= 2.0 ** -7 * want.abs() + 1e-30).all()            # within one bf16 step of softplus + 1e-10
    return m, sd


def _signs(layer, s, ed, B):
    O, C = layer.weight.shape[:2]
    R, Sg = conv_signs(layer.flip_key, s, ed, B, O, C)
    return torch.from_numpy(R).reshape(B, O, 1, 1, 1), torch.from_numpy(Sg).reshape(B, C, 1, 1, 1)


def _geo(layer):
    return layer.stride, layer.padding, layer.dilation


def _check_forward(y, xs, layer, mean, std, R, Sg, mode, what):
    """y (B, O, ...) of one sample vs float64 of the reference expression on x_s (float64 CPU) and signs R, Sg."""
    geo = _geo(layer)
    xr = bf(xs) if mode == "bf16" else xs
    want = F.conv3d(xr, mean, None, *geo) + F.conv3d(xr * Sg, std, None, *geo) * R
    if mode == "f32":
        scale = max(1.0, float(want.abs().max()))
        err = float((torch.from_numpy(N(y)) - want).abs().max())
        assert err <= 2e-5 * scale, (what, err, scale)
    else:
        K = mean[0].numel()
        mag = F.conv3d(xr.abs(), mean.abs(), None, *geo) + F.conv3d(xr.abs(), std.abs(), None, *geo)
        assert_within(N(y), want.numpy(), ((K + 3) * U * mag).numpy() + 1e-30, what)


# ------------------------------------------------------------------------------------------------ GPU: MC forward in a network
class Vol(BayesianNetworkModule):
    """[optional leading NormalConv3d] -> FlipOutNormalConv3d -> flatten."""

    def __init__(self, C, O, S, front=False):
        super().__init__(C, O, samples=S)
        self.front = NormalConv3d(C, C, 1) if front else None
        self.flip = FlipOutNormalConv3d(C, O, 3, padding=1)

    def _forward(self, x):
        if self.front is not None:
            x = self.front(x)
        return self.flip(x).flatten(1)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("front", [False, True])
def test_mc_batched_flipout_conv3d_forward(dev, mode, S, front):
    B, C, O = 3, 5, 7
    torch.manual_seed(31 + S)
    net = Vol(C, O, S, front=front).to(dev)
    seeded.pin_streams(net, 3000)
    net.mc_batched = True
    x = torch.randn(B, C, 5, 6, 7, generator=torch.Generator().manual_seed(4))
    bnn.set_compute(mode)
    bnn.manual_seed(22)
    box = []
    hnd = net.flip.register_forward_pre_hook(lambda m, a: box.append(a[0].detach().clone()))
    with torch.no_grad():
        ys = net(x.to(dev))
    hnd.remove()
    ys = ys if isinstance(ys, list) else [ys]
    assert len(ys) == S
    for a in range(S):
        for c in range(a + 1, S):
            assert not torch.equal(ys[a], ys[c]), (a, c)
    xin = box[0].double().cpu()
    assert xin.shape[0] == (B * S if front and S > 1 else B)
    mean, std = _operands(net.flip, mode)
    ed = _epoch_dev(dev)
    for s in range(S):
        xs = xin[s * B:(s + 1) * B] if xin.shape[0] == B * S else xin
        if net.flip.flip_key is None:                           # S = 1: the serial device path on the recorded R and S
            R, Sg = net.flip.R.double().cpu(), net.flip.S.double().cpu()
        else:
            R, Sg = _signs(net.flip, s, ed, B)
        _check_forward(ys[s].reshape(B, O, 5, 6, 7), xs, net.flip, mean, std, R, Sg, mode, "%s S=%d sample %d" % (mode, S, s))


# ------------------------------------------------------------------------------------------------ GPU: forward + backward sweep
SWEEP = [
    # C, O, vol, k, stride, pad, dil, S, shared
    (3, 5, (7, 9, 11), 3, 1, 1, 1, 1, True),
    (3, 5, (7, 9, 11), 3, 1, 1, 1, 3, False),
    (16, 32, (5, 6, 7), (3, 1, 2), (2, 1, 1), 1, 1, 3, False),
    (5, 7, (6, 5, 9), 3, 2, 0, 2, 8, True),
    (8, 64, (5, 5, 5), 3, 1, 1, 1, 8, True),
    (4, 70, (4, 6, 5), (1, 3, 3), 1, (0, 1, 1), 1, 3, False),
    (33, 6, (3, 4, 5), 2, 1, 1, (1, 2, 1), 1, False),
    (1, 1, (7, 9, 11), 1, 1, 0, 1, 8, True),
]


def _layer_backward(layer, x, S, shared, dev, gseed):
    """y = layer(x) in an MC context of S samples, loss = <y, G> -> (y, G, grads of x, weight.mean, weight.scale)."""
    xd = x.to(dev).requires_grad_(True)
    B = x.shape[0] if shared else x.shape[0] // S
    with _mc.McContext(S, B, 0):
        y = layer(xd)
    G = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
    grads = torch.autograd.grad(y, [xd, layer.weight.mean, layer.weight.scale], G.to(dev))
    return y, G, grads


def _ref_backward(layer, x, S, shared, mode, G, ed):
    """float64 gradients of <reference expression, G> over the samples, and their derived bf16 bounds."""
    geo = _geo(layer)
    mean, std = _operands(layer, mode)
    sig = torch.sigmoid(layer.weight.scale.detach().double().cpu())
    B = x.shape[0] if shared else x.shape[0] // S
    bfm = mode == "bf16"
    xr = bf(x.double()) if bfm else x.double()
    Gr = bf(G.double()) if bfm else G.double()
    gx, gxb = torch.zeros_like(xr), torch.zeros_like(xr)
    gm, gmb, gs, gsb = (torch.zeros_like(mean) for _ in range(4))
    T = mean[0, 0].numel()
    O, C = mean.shape[:2]
    for s in range(S):
        sl = slice(None) if shared else slice(s * B, (s + 1) * B)
        R, Sg = _signs(layer, s, ed, B)
        xs = xr[sl].clone().requires_grad_(True)
        m = mean.clone().requires_grad_(True)
        sd = std.clone().requires_grad_(True)
        gys = Gr[s * B:(s + 1) * B]
        ys = F.conv3d(xs, m, None, *geo) + F.conv3d(xs * Sg, sd, None, *geo) * R
        g_x, g_m, g_s = torch.autograd.grad(ys, (xs, m, sd), gys)
        xa, ma, sa = (t.detach().abs().requires_grad_(True) for t in (xs, m, sd))
        ya = F.conv3d(xa, ma, None, *geo) + F.conv3d(xa, sa, None, *geo)
        a_x, a_m, a_s = torch.autograd.grad(ya, (xa, ma, sa), gys.abs())
        P = ys[0, 0].numel()
        gx[sl] += g_x
        gxb[sl] += ((S if shared else 1) * (O * T + 2) + 2) * U * a_x
        gm += g_m
        gs += g_s
        gmb += (B * P + 16 + S) * U * a_m
        gsb += (B * P + 16 + S) * U * a_s
    return [gx, gm, gs * sig], [gxb, gmb + 2 * U * gm.abs(), (gsb + 8 * U * gs.abs()) * sig]


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", SWEEP)
def test_flipout_conv3d_sweep_forward_and_backward(dev, mode, case):
    C, O, vol, k, st, pad, dil, S, shared = case
    torch.manual_seed(C * 37 + O)
    layer = FlipOutNormalConv3d(C, O, k, stride=st, padding=pad, dilation=dil).to(dev)
    seeded.pin_streams(layer, 3100)
    B = 3
    x = torch.randn((B if shared else S * B, C) + vol, generator=torch.Generator().manual_seed(9))
    bnn.set_compute(mode)
    bnn.manual_seed(14)
    y, G, grads = _layer_backward(layer, x, S, shared, dev, 17)
    ed = _epoch_dev(dev)
    mean, std = _operands(layer, mode)
    for s in range(S):
        xs = x.double() if shared else x[s * B:(s + 1) * B].double()
        R, Sg = _signs(layer, s, ed, B)
        _check_forward(y[s * B:(s + 1) * B], xs, layer, mean, std, R, Sg, mode, "%s %s y[%d]" % (mode, case, s))
    refs, bounds = _ref_backward(layer, x, S, shared, mode, G, ed)
    for got, ref, bd, name in zip(grads, refs, bounds, ["x", "weight.mean", "weight.scale"]):
        if mode == "f32":
            assert_close_scaled(N(got), ref.numpy(), 1e-4, "%s grad %s" % (case, name))
        else:
            assert_within(N(got), ref.numpy(), bd.numpy() + 1e-30, "%s grad %s" % (case, name))


# ------------------------------------------------------------------------------------------------ GPU: serial device path
@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_serial_device_path_on_recorded_signs(dev, mode, monkeypatch):
    torch.manual_seed(6)
    layer = FlipOutNormalConv3d(6, 10, 3, stride=(1, 2, 1), padding=1).to(dev)
    x = torch.randn(4, 6, 5, 7, 6, generator=torch.Generator().manual_seed(2))
    bnn.set_compute(mode)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    xd = x.to(dev).requires_grad_(True)
    y = layer(xd)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() - n0 == 2                     # the operand draw + the contraction
    assert layer.R.shape == (4, 10, 1, 1, 1) and layer.S.shape == (4, 6, 1, 1, 1)
    R, Sg = layer.R.double().cpu(), layer.S.double().cpu()
    mean, std = _operands(layer, mode)
    _check_forward(y, x.double(), layer, mean, std, R, Sg, mode, "serial %s" % mode)
    G = torch.randn(y.shape, generator=torch.Generator().manual_seed(8))
    grads = torch.autograd.grad(y, [xd, layer.weight.mean, layer.weight.scale], G.to(dev))

    # float64 autograd of the reference expression on the recorded signs
    geo = _geo(layer)
    bfm = mode == "bf16"
    xr = bf(x.double()) if bfm else x.double()
    Gr = bf(G.double()) if bfm else G.double()
    xs, m, sd = (t.clone().requires_grad_(True) for t in (xr, mean, std))
    ys = F.conv3d(xs, m, None, *geo) + F.conv3d(xs * Sg, sd, None, *geo) * R
    refs = list(torch.autograd.grad(ys, (xs, m, sd), Gr))
    refs[2] = refs[2] * torch.sigmoid(layer.weight.scale.detach().double().cpu())
    for got, ref, name in zip(grads, refs, ["x", "weight.mean", "weight.scale"]):
        assert_close_scaled(N(got), ref.numpy(), 1e-4 if mode == "f32" else 2e-3, "serial %s grad %s" % (mode, name))

    # sample=False: the recorded R and S again, bit for bit
    with torch.no_grad():
        y2 = layer(x.to(dev), sample=False)
        y3 = layer(x.to(dev))
    assert torch.equal(y2, y.detach())
    assert not torch.equal(y3, y.detach())


@gpu
def test_mc_sample_false_reuses_the_key(dev):
    torch.manual_seed(3)
    net = Vol(4, 6, 3).to(dev)
    seeded.pin_streams(net, 3200)
    net.mc_batched = True
    x = torch.randn(2, 4, 4, 5, 6, device=dev)
    bnn.manual_seed(9)
    with torch.no_grad():
        y1 = torch.stack(net(x))
        key = net.flip.flip_key
        with _mc.McContext(3, 2, 0):
            y2 = net.flip(x, sample=False)
    assert net.flip.flip_key is key
    assert torch.equal(y2.reshape(3, 2, -1), y1.reshape(3, 2, -1))


# ------------------------------------------------------------------------------------------------ GPU: no torch convolution
@gpu
@pytest.mark.parametrize("S", [1, 8])
def test_mc_flipout_conv3d_runs_no_torch_conv(dev, monkeypatch, S):
    def refuse(*a, **k):
        raise AssertionError("torch conv3d called on the device path")

    monkeypatch.setattr(torch.nn.functional, "conv3d", refuse)
    monkeypatch.setattr(torch, "conv3d", refuse)
    monkeypatch.setattr(FlipOutNormalConv3d, "_op", staticmethod(refuse))
    lib = _lib.load()
    torch.manual_seed(5)
    layer = FlipOutNormalConv3d(3, 5, 3, padding=1).to(dev)
    seeded.pin_streams(layer, 3300)
    x = torch.randn(4, 3, 6, 6, 6, device=dev)
    for mode in ("f32", "bf16"):
        bnn.set_compute(mode)
        xd = x.clone().requires_grad_(True)
        with _mc.McContext(S, 4, 0):
            layer(xd)                                           # warm
        torch.cuda.synchronize()
        n0 = lib.bnn_launch_count()
        with _mc.McContext(S, 4, 0):
            y = layer(xd)
        torch.cuda.synchronize()
        assert lib.bnn_launch_count() - n0 == 3                 # the operand draw, the sign launch, the contraction
        n0 = lib.bnn_launch_count()
        g = torch.autograd.grad(y.sum(), [xd, layer.weight.mean, layer.weight.scale])
        torch.cuda.synchronize()
        assert lib.bnn_launch_count() - n0 == 4                 # the operand draw, the input gradient, the slabs, the reduce
        assert all(bool(torch.isfinite(t).all()) for t in g)


# ------------------------------------------------------------------------------------------------ GPU: keys and bits
@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_sample_s_of_a_batched_pass_is_the_single_sample_pass(dev, mode):
    torch.manual_seed(12)
    mean = torch.randn(9, 5, 3, 3, 3, device=dev) * 0.2
    scale = torch.randn(9, 5, 3, 3, 3, device=dev) - 3
    x = torch.randn(3, 5, 6, 7, 5, device=dev)
    geo = ((1, 1, 1), (1, 1, 1), (1, 1, 1))
    gen = _rng.GEN_PHILOX10_U24 if mode == "f32" else _rng.GEN_PHILOX7_U16
    key8 = _key(8, gen, stream=77)
    y8 = ops.conv3d_flipout(x, mean, scale, ops.flipout_signs(key8, 3, 14, dev), 8, True, *geo, mode)
    for s in range(8):
        key1 = _key(1, gen, stream=77, sample0=s)
        y1 = ops.conv3d_flipout(x, mean, scale, ops.flipout_signs(key1, 3, 14, dev), 1, True, *geo, mode)
        assert torch.equal(y8[s], y1[0]), s


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shared", [True, False])
def test_forward_and_backward_are_bitwise_reproducible(dev, mode, shared):
    torch.manual_seed(2)
    layer = FlipOutNormalConv3d(8, 16, 3, padding=1).to(dev)
    seeded.pin_streams(layer, 3400)
    S, B = 8, 4
    x = torch.randn((B if shared else S * B, 8, 12, 12, 12), generator=torch.Generator().manual_seed(1))
    bnn.set_compute(mode)
    bnn.manual_seed(5)
    y1, _, g1 = _layer_backward(layer, x, S, shared, dev, 3)
    xd = x.to(dev).requires_grad_(True)
    with _mc.McContext(S, B, 0):
        y2 = layer(xd, sample=False)                            # the same key
    G = torch.randn(y2.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    g2 = torch.autograd.grad(y2, [xd, layer.weight.mean, layer.weight.scale], G)
    assert torch.equal(y1, y2)
    for a, c in zip(g1, g2):
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ GPU: a small training step
class Small(BayesianNetworkModule):
    """NormalConv3d -> ReLU -> FlipOutNormalConv3d -> pool -> NormalLinear."""

    def __init__(self, S):
        super().__init__(3, 4, samples=S)
        self.c1 = NormalConv3d(3, 6, 3, padding=1)
        self.c2 = FlipOutNormalConv3d(6, 8, 3, stride=2, padding=1)
        self.fc = NormalLinear(8, 4)

    def _forward(self, x):
        h = self.c2(torch.relu(self.c1(x)))
        return self.fc(F.adaptive_avg_pool3d(h, 1).flatten(1))


@gpu
def test_small_training_step_gradients(dev):
    S, B = 3, 2
    torch.manual_seed(17)
    net = Small(S).to(dev)
    seeded.pin_streams(net, 3500)
    net.mc_batched = True
    bnn.set_compute("f32")
    bnn.manual_seed(40)
    x = torch.randn(B, 3, 6, 6, 6, generator=torch.Generator().manual_seed(3))
    t = torch.tensor([1, 3])
    ys = net(x.to(dev))
    loss = sum(F.cross_entropy(y, t.to(dev)) for y in ys) / S
    loss.backward()

    # float64 on the recorded draws and signs
    ed = _epoch_dev(dev)
    w1 = ops._sample_affine_philox_raw(net.c1.weight.mean.detach(), net.c1.weight.scale.detach(), net.c1.weight.draw_key).double().cpu()
    b1 = ops._sample_affine_philox_raw(net.c1.bias.mean.detach(), net.c1.bias.scale.detach(), net.c1.bias.draw_key).double().cpu()
    wf = ops._sample_affine_philox_raw(net.fc.weight.mean.detach(), net.fc.weight.scale.detach(), net.fc.weight.draw_key).double().cpu()
    bfc = ops._sample_affine_philox_raw(net.fc.bias.mean.detach(), net.fc.bias.scale.detach(), net.fc.bias.draw_key).double().cpu()
    m2 = net.c2.weight.mean.detach().double().cpu().requires_grad_(True)
    r2 = net.c2.weight.scale.detach().double().cpu().requires_grad_(True)
    x64 = x.double()
    outs = []
    for s in range(S):
        h = torch.relu(F.conv3d(x64, w1[s], b1[s], 1, 1))
        hh = _flip_conv64(h, m2, F.softplus(r2) + 1e-10, net.c2.flip_key, s, ed, net.c2.stride, net.c2.padding, net.c2.dilation,
                          F.conv3d)
        outs.append(F.cross_entropy(F.linear(F.adaptive_avg_pool3d(hh, 1).flatten(1), wf[s], bfc[s]), t))
    (sum(outs) / S).backward()
    assert_close_scaled(N(net.c2.weight.mean.grad), m2.grad.numpy(), 1e-4, "c2 mean grad")
    assert_close_scaled(N(net.c2.weight.scale.grad), r2.grad.numpy(), 1e-4, "c2 scale grad")
    assert float(net.c1.weight.mean.grad.abs().max()) > 0
