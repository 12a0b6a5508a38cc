"""Every contraction that runs through the shared conv3d tile (csrc/bnn_conv3d_tile.hpp), at the tile's own edges.

Thirteen contractions use the 128 x 64 x 32 implicit-GEMM tile: FWD / DGRAD / WGRAD of K7 (NormalConv3d), K9
(FlipOutNormalConv3d) and K11 (LocalReparamConv{1,2,3}d), K17's forward (conv moments) and K19's DGRAD / WGRAD (their backward).
The families' own case tables were written before the tile was shared, and each reaches other edges of the row decode, the gather
and B walkers, FastDiv, the slab split and the epilogue's lane map.  Here ONE table (conv3d_tile_cases.TABLE) goes through all of
them: a partial second column block and a partial second row block, with and without a group offset; per-axis geometry; output
positions that read only padding; input positions no tap reaches (exact zeros in every input gradient); one output position per
image (FastDiv by 1, tiles and quads that span many images); a weight gradient of one k-tile (K7 writes it with no slab) and one of
24 k-tiles in 12 slabs with a short last slab.

References and bounds are the families' own, imported: float64 conv3d and its autograd on the device's own draws, signs and eps;
the derived bf16 bounds and the fp32 constants of test_conv3d_device, test_flipout_conv3d_device, test_lrt_conv_device,
test_moment_conv and test_moment_conv_backward.  No tolerance is defined here.

What the file is for, measured on the MI355X with two deliberately wrong builds (both stay inside every tensor): with FastDiv of
P == 1 dividing by 2, and with K7 / K9 reading the bias of, and storing zeros to the input and weight gradients of, columns
n >= 64, every test of the five family files passed; here 46 and 20 tests failed (one-output and point; wide and wide-groups).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_scaled
import seeded

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd import nn as bnn_nn
from bayesianneuralnetworks_amd.nn import FlipOutNormalConv3d, NormalConv3d

import test_conv3d_device as k7
import test_flipout_conv3d_device as k9
import test_lrt_conv_device as k11
import test_moment_conv as k17
import test_moment_conv_backward as k19
from conv3d_tile_cases import BK, BM, BN, CASES, EXACT_ZERO, MULTI_SAMPLE, TABLE, geometry
from test_flipout_mc import _epoch_dev
from test_lrt_device import assert_within, sigma64

gpu = pytest.mark.gpu
MODES = ["f32", "bf16"]

_structure = {}


def structure(name):
    """(padding_only, unreached) of a case: bool masks over the output positions (OD, OH, OW) that read nothing but padding --
    the zeros of conv3d(ones, ones) -- and over the input positions (D, H, W) that no tap reaches -- the zeros of that
    convolution's input gradient.  Neither depends on the image or the channel."""
    if name not in _structure:
        g = geometry(name)
        x = torch.ones((1, g.C) + g.vol, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(x, torch.ones(g.w_shape, dtype=torch.float64), None, *g.geo)
        gx, = torch.autograd.grad(y.sum(), x)
        assert all(torch.equal(y[0, o], y[0, 0]) for o in range(g.O)) and all(torch.equal(gx[0, c] == 0, gx[0, 0] == 0) for c in range(g.C))
        _structure[name] = (y[0, 0] == 0, gx[0, 0] == 0)
    return _structure[name]


def shape_of(name):
    g = geometry(name)
    return ops._conv3d_shape(g.x_shape, g.w_shape, g.stride, g.padding, g.dilation, g.groups)[0]


def assert_unreached_are_zero(name, grad, what):
    """`grad` (..., D, H, W): exactly zero at every input position the reference marks unreached."""
    if name not in EXACT_ZERO:
        return
    unreached = structure(name)[1]
    assert unreached.any()
    at = grad.detach().cpu()[..., unreached]
    assert at.numel() > 0 and bool((at == 0).all()), "%s %s: %d of %d unreached positions are not zero" % (
        what, name, int((at != 0).sum()), at.numel())


# ================================================================================================ CPU: the table's claims
@pytest.mark.parametrize("name", CASES)
def test_table_claims(name):
    g, claims = TABLE[name]
    for key in ("Cg", "Ng", "K", "P", "Pin", "T", "out"):
        if key in claims:
            assert getattr(g, key) == claims[key], key
    assert g.P % 4 == claims["P4"]
    if "BP" in claims:
        assert g.B * g.P == claims["BP"]
    want = F.conv3d(torch.zeros(g.x_shape), torch.zeros(g.w_shape), None, *g.geo).shape
    assert tuple(want) == (g.B, g.O) + g.out                      # torch accepts the geometry, and ops._conv3d_shape agrees
    assert ops._conv3d_shape(g.x_shape, g.w_shape, g.stride, g.padding, g.dilation, g.groups)[1] == g.out
    padding_only, unreached = structure(name)
    assert int(padding_only.sum()) == claims["padding_only"] and int(unreached.sum()) == claims["unreached"]
    assert padding_only.numel() == g.P and unreached.numel() == g.Pin


def test_table_reaches_every_edge():
    span = lambda g, i: g.dilation[i] * (g.kernel[i] - 1) + 1         # noqa: E731
    for name in ("wide", "wide-groups"):
        g = geometry(name)
        assert BN < g.Cg < 2 * BN and BN < g.Ng < 2 * BN            # a partial second column block: DGRAD; FWD and WGRAD
        assert BM < g.K < 2 * BM                                    # a partial second row block in WGRAD
        assert g.P % 2 == 1
    assert geometry("wide").groups == 1 and geometry("wide-groups").groups == 2
    assert geometry("wide-groups").B * geometry("wide-groups").P <= BK                    # one k-tile
    g = geometry("peraxis")
    for triple in (g.vol, g.out, g.kernel, g.stride, g.padding, g.dilation):
        assert len(set(triple)) == 3, triple
    assert structure("peraxis")[0].any() and structure("peraxis")[1].any()
    g = geometry("peraxis-odd")
    for triple in (g.vol, g.out, g.kernel, g.stride, g.padding, g.dilation):
        assert len(set(triple)) == 3, triple
    assert g.groups == 2 and all(getattr(g, k) != getattr(geometry("peraxis"), k) for k in ("kernel", "stride", "padding", "dilation"))
    g = geometry("padding-only")
    assert any(g.padding[i] >= span(g, i) for i in range(3))          # padding at least as large as the window
    assert 2 * int(structure("padding-only")[0].sum()) > g.P and g.B * g.P > BM > g.B * g.Pin
    g = geometry("unreached")
    assert any(g.stride[i] > span(g, i) for i in range(3))            # stride larger than the window
    assert any((g.vol[i] + 2 * g.padding[i] - span(g, i)) % g.stride[i] for i in range(3))         # and a tail the forward never reads
    assert 2 * int(structure("unreached")[1].sum()) > g.Pin
    g = geometry("stride-eq-dil")
    assert g.stride == g.dilation and min(g.stride) > 1 and structure("stride-eq-dil")[1].any()
    g = geometry("one-output")
    assert g.P == 1 and g.out == (1, 1, 1) and BM < g.B < 2 * BM       # two row blocks, every row its own image
    g = geometry("point")
    assert g.P == g.Pin == g.T == 1 and g.K == 2 and g.B * g.P == 5
    g = geometry("one-ktile")
    assert g.B * g.P <= BK and g.P % 4 == 0
    g = geometry("long-reduction")
    assert -(-g.B * g.P // BK) == 24 and g.P % BK != 0                 # 24 k-tiles, image boundaries off the k-tile grid
    # K9 takes groups == 1 only: it runs every case but these two
    assert [n for n in CASES if geometry(n).groups != 1] == ["wide-groups", "peraxis-odd"]
    assert set(MULTI_SAMPLE) <= set(CASES) and set(EXACT_ZERO) <= set(CASES)
    assert all(structure(n)[1].any() for n in EXACT_ZERO)
    assert [n for n in CASES if structure(n)[1].any()] == [n for n in CASES if n in EXACT_ZERO]


def test_slab_counts_are_the_librarys():
    """The slab split is read from the library's own workspace queries (nslab x the entry's planes x O K floats)."""
    lib = _lib.load()
    one, many = shape_of("one-ktile"), shape_of("long-reduction")
    for S in (1, 3):
        assert lib.bnn_conv3d_backward_weight_workspace_bytes(ctypes.byref(one), S) == 0          # K7: gw written with no slab
        assert lib.bnn_conv3d_backward_weight_workspace_bytes(ctypes.byref(many), S) > 0
    g = geometry("long-reduction")
    n = g.O * g.K * 4
    nslab = lib.bnn_conv3d_backward_weight_workspace_bytes(ctypes.byref(many), 1) // n
    assert nslab == 12
    assert lib.bnn_conv3d_flipout_backward_weight_workspace_bytes(ctypes.byref(many), 1) == nslab * 2 * n
    assert lib.bnn_conv3d_lrt_backward_weight_workspace_bytes(ctypes.byref(many), 1) == nslab * 2 * n
    assert lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(many)) == nslab * 3 * n
    # 24 k-tiles in 12 slabs: two k-tiles each; the last slab is short and its last k-tile partial
    chunk = 24 // nslab * BK
    R = g.B * g.P
    assert (nslab - 1) * chunk < R < nslab * chunk and (R - (nslab - 1) * chunk) % BK != 0
    # one k-tile: every family has one slab
    g = geometry("one-ktile")
    n = g.O * g.K * 4
    assert lib.bnn_conv3d_flipout_backward_weight_workspace_bytes(ctypes.byref(one), 1) == 2 * n
    assert lib.bnn_conv3d_lrt_backward_weight_workspace_bytes(ctypes.byref(one), 1) == 2 * n
    assert lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(one)) == 3 * n
    # no case is refused by a workspace query (they run every range check of the entries)
    for name in CASES:
        sh = shape_of(name)
        assert lib.bnn_conv3d_backward_weight_workspace_bytes(ctypes.byref(sh), 4) >= 0, name
        assert lib.bnn_conv3d_lrt_backward_weight_workspace_bytes(ctypes.byref(sh), 4) > 0, name
        assert lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(sh)) > 0, name
        if geometry(name).groups == 1:
            assert lib.bnn_conv3d_flipout_backward_weight_workspace_bytes(ctypes.byref(sh), 4) > 0, name


# ================================================================================================ GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


@pytest.fixture
def switch():
    """nn.conv_moment_training on for one test, restored afterwards."""
    was = bnn_nn.conv_moment_training_enabled()
    bnn_nn.conv_moment_training(True)
    yield
    bnn_nn.conv_moment_training(was)


def plans(names):
    """(case, S, shared input): S = 3 shared and per sample on MULTI_SAMPLE, S = 1 elsewhere."""
    return [(n, S, shared) for n in names for S, shared in ([(3, True), (3, False)] if n in MULTI_SAMPLE else [(1, True)])]


def plan_id(plan):
    return "%s-S%d-%s" % (plan[0], plan[1], "shared" if plan[2] else "persample")


K7_PLANS = plans(CASES)
K9_PLANS = plans([n for n in CASES if geometry(n).groups == 1])


# ------------------------------------------------------------------------------------------------ K7: NormalConv3d
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("plan", K7_PLANS, ids=plan_id)
def test_normal_conv3d_forward_and_backward(dev, plan, bias, mode):
    """FWD, DGRAD and WGRAD of K7 through the layer: y of every sample and all five gradients, every element."""
    name, S, shared = plan
    g = geometry(name)
    lib = _lib.load()
    nb = lib.bnn_conv3d_backward_weight_workspace_bytes(ctypes.byref(shape_of(name)), S)
    if name == "one-ktile":
        assert nb == 0                                          # the weight gradient is written directly
    if name == "long-reduction":
        assert nb > 0
    torch.manual_seed(g.C * 31 + g.O)
    layer = NormalConv3d(g.C, g.O, g.kernel, stride=g.stride, padding=g.padding, dilation=g.dilation, groups=g.groups, bias=bias).to(dev)
    seeded.pin_streams(layer, 5000)
    B = g.B
    x = torch.randn((B if shared else S * B, g.C) + g.vol, generator=torch.Generator().manual_seed(9))
    bnn.set_compute(mode)
    bnn.manual_seed(13)
    n0 = lib.bnn_launch_count()
    y, R, grads = k7._layer_backward(layer, x, S, shared, mode, dev, 17)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() > n0
    assert y.shape == (S * B, g.O) + g.out
    w, b = k7._draws(layer, mode)
    what = "%s %s" % (plan_id(plan), mode)
    for s in range(S):
        xs = x.double() if shared else x[s * B:(s + 1) * B].double()
        k7._check_forward(y[s * B:(s + 1) * B], xs, layer, w[s], None if b is None else b[s], mode, "%s y[%d]" % (what, s))
    refs, bounds = k7._ref_backward(layer, x, S, shared, mode, R)
    assert len(grads) == len(refs) == (5 if bias else 3)
    for got, ref, bd, gname in zip(grads, refs, bounds, ["x", "weight.mean", "weight.scale", "bias.mean", "bias.scale"]):
        if mode == "f32":
            assert_close_scaled(k7.N(got), ref.numpy(), 1e-4, "%s grad %s" % (what, gname))
        else:
            k7.assert_within(k7.N(got), ref.numpy(), bd.numpy() + 1e-30, "%s grad %s" % (what, gname))
    assert_unreached_are_zero(name, grads[0], "K7 gx " + what)
    _lib.check_device(dev)


# ------------------------------------------------------------------------------------------------ K9: FlipOutNormalConv3d
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("plan", K9_PLANS, ids=plan_id)
def test_flipout_conv3d_forward_and_backward(dev, monkeypatch, plan, mode):
    """FWD, DGRAD and WGRAD of K9 through the layer, on the twin's signs; the layer's torch expression is out of reach."""
    name, S, shared = plan
    g = geometry(name)
    assert ops.conv3d_flipout_eligible(g.x_shape, g.w_shape, S, g.stride, g.padding, g.dilation, g.groups)

    def refuse(*a, **k):
        raise AssertionError("the torch expression ran in place of the HIP entries")

    monkeypatch.setattr(FlipOutNormalConv3d, "_op", staticmethod(refuse))
    torch.manual_seed(g.C * 37 + g.O)
    layer = FlipOutNormalConv3d(g.C, g.O, g.kernel, stride=g.stride, padding=g.padding, dilation=g.dilation).to(dev)
    seeded.pin_streams(layer, 5100)
    B = g.B
    x = torch.randn((B if shared else S * B, g.C) + g.vol, generator=torch.Generator().manual_seed(9))
    bnn.set_compute(mode)
    bnn.manual_seed(14)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    y, G, grads = k9._layer_backward(layer, x, S, shared, dev, 17)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() > n0
    assert y.shape == (S * B, g.O) + g.out
    ed = _epoch_dev(dev)
    mean, std = k9._operands(layer, mode)
    what = "%s %s" % (plan_id(plan), mode)
    for s in range(S):
        xs = x.double() if shared else x[s * B:(s + 1) * B].double()
        Rs, Sg = k9._signs(layer, s, ed, B)
        k9._check_forward(y[s * B:(s + 1) * B], xs, layer, mean, std, Rs, Sg, mode, "%s y[%d]" % (what, s))
    refs, bounds = k9._ref_backward(layer, x, S, shared, mode, G, ed)
    for got, ref, bd, gname in zip(grads, refs, bounds, ["x", "weight.mean", "weight.scale"]):
        if mode == "f32":
            assert_close_scaled(k9.N(got), ref.numpy(), 1e-4, "%s grad %s" % (what, gname))
        else:
            k9.assert_within(k9.N(got), ref.numpy(), bd.numpy() + 1e-30, "%s grad %s" % (what, gname))
    assert_unreached_are_zero(name, grads[0], "K9 gx " + what)
    _lib.check_device(dev)


# ------------------------------------------------------------------------------------------------ K11: LocalReparamConv3d
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "persample"])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("name", CASES)
def test_lrt_conv3d_forward_and_backward(dev, name, S, shared, mode):
    """ops.convNd_lrt on the key's eps: y of every sample (FWD) and all five gradients (DGRAD, WGRAD, the bias sums)."""
    case = k11.Case(*geometry(name).lrt_args)
    assert (case.out, case.P, case.K) == (geometry(name).out, geometry(name).P, geometry(name).K)
    k11.check_forward(dev, case, name, S, shared, True, mode)
    got = k11.check_backward(dev, case, name, S, shared, True, mode)
    assert len(got) == 5
    assert_unreached_are_zero(name, got[0], "K11 gx S=%d shared=%s %s" % (S, shared, mode))
    _lib.check_device(dev)


# ------------------------------------------------------------------------------------------------ K17: conv moments forward
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("with_var", [False, True], ids=["det", "var"])
@pytest.mark.parametrize("name", CASES)
def test_conv_moments_forward(dev, name, with_var, mode):
    g = geometry(name)
    p = k17.conv_params(g.O, g.Cg, g.kernel, True, 11)
    mom = k17.conv_input(g.x_shape, with_var, 12)
    a = k17.on(dev, mom) if with_var else mom.mean.to(dev)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    out = ops.moments_convNd(a, *k17.to(dev, *p), *g.geo, compute=mode)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 2                      # the operand launch + ONE contraction launch
    m, v, bm, bv = k17.conv_ref(mom, *p, g.geo, mode, dev)
    assert out.mean.shape == m.shape == (g.B, g.O) + g.out and out.mean.dtype == out.var.dtype == torch.float32
    what = "%s var=%s %s" % (name, with_var, mode)
    assert_within(out.mean, m, bm, "m " + what)
    assert_within(out.var, v, bv, "v " + what)
    assert (out.var >= 0).all()
    padding_only = structure(name)[0]
    if padding_only.any():
        # the reference says it: a position that reads only padding has the bias' moments (so the device has, within the bounds)
        mu_b, s2_b = p[2].double(), sigma64(p[3]) ** 2
        assert torch.equal(m[..., padding_only], mu_b[None, :, None].expand(g.B, g.O, int(padding_only.sum())))
        assert ((v[..., padding_only] - s2_b[None, :, None]).abs() <= 1e-6 * s2_b[None, :, None]).all()
    _lib.check_device(dev)


# ------------------------------------------------------------------------------------------------ K19: conv moments backward
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_conv_moments_backward(dev, name, mode, switch):
    """DGRAD and WGRAD of K19 behind nn.conv_moment_training: forward_moments through a NormalConv3d on an input that carries a
    variance, all six gradients against test_conv_backward_matches_float64's reference."""
    g = geometry(name)
    ops_cpu = k19.backward_operands(g.moment_spec, True)
    a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b, geo = ops_cpu
    mu_b = k17.conv_params(g.O, g.Cg, g.kernel, True, 11)[2]
    assert geo == g.geo and tuple(a_m.shape) == g.x_shape
    bnn.set_compute(mode)
    layer = NormalConv3d(g.C, g.O, g.kernel, g.stride, g.padding, g.dilation, g.groups, True).to(dev)
    with torch.no_grad():
        for t, s in zip((layer.weight.mean, layer.weight.scale, layer.bias.mean, layer.bias.scale), (mu_w, rho_w, mu_b, rho_b)):
            t.copy_(s)
    net = k19.Wrap(layer)
    am, av = a_m.to(dev).requires_grad_(), a_v.to(dev).requires_grad_()
    out = net.forward_moments(ops.Moments(am, av))
    assert out.mean.requires_grad and out.var.requires_grad and out.mean.shape == (g.B, g.O) + g.out
    lib = _lib.load()
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    got = torch.autograd.grad([out.mean, out.var], [am, av, layer.weight.mean, layer.weight.scale, layer.bias.mean, layer.bias.scale],
                              k19.to(dev, G_m, G_v))
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1 + 3                  # the input gradient; slabs, reduce and bias sums
    s2_dev, _ = ops._lrt_prepare_raw(rho_w.to(dev), None)
    want = k19.backward_reference(mode, *ops_cpu, s2_dev.cpu())
    assert len(got) == len(want) == 6
    for a, (gname, ref, bound) in zip(got, want):
        assert_within(a, ref, bound, "%s %s %s" % (gname, name, mode))
    assert_unreached_are_zero(name, got[0], "K19 g_a_m " + mode)
    assert_unreached_are_zero(name, got[1], "K19 g_a_v " + mode)
    _lib.check_device(dev)
