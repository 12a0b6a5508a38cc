"""NormalConv3d on the device: one keyed draw launch + one implicit-GEMM launch for all S MC samples (csrc/bnn_conv3d.hip),
forward and backward, against float64 torch conv3d on the K1 draws of the layer's recorded keys.

bf16 bounds are derived, not blanket: the reference is float64 on the bf16-rounded operands, so what is left is fp32
accumulation -- at most (L + 2) 2^-24 sum |a b| for a reduction of L products (one rounding per addend, one for the bias) --
and the fp32 elementwise work of the draw backward (a few 2^-24 of each term)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_scaled
import seeded

from bayesianneuralnetworks_amd._lib import BnnHipError
from bayesianneuralnetworks_amd import ops
from bayesianneuralnetworks_amd.nn import NormalConv3d, BayesianNetworkModule

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
@pytest.mark.parametrize("seed", range(6))
def test_conv3d_shape_matches_torch(seed):
    g = torch.Generator().manual_seed(seed)
    for _ in range(40):
        r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
        groups = r(1, 3)
        C, O = groups * r(1, 3), groups * r(1, 3)
        k = (r(1, 4), r(1, 4), r(1, 4))
        st, pad, dil = (r(1, 3), r(1, 3), r(1, 3)), (r(0, 2), r(0, 2), r(0, 2)), (r(1, 2), r(1, 2), r(1, 2))
        x_shape = (r(1, 3), C, r(1, 9), r(1, 9), r(1, 9))
        w_shape = (O, C // groups) + k
        try:
            want = F.conv3d(torch.zeros(x_shape), torch.zeros(w_shape), None, st, pad, dil, groups).shape
        except RuntimeError:
            with pytest.raises(BnnHipError, match="kernel larger"):
                ops._conv3d_shape(x_shape, w_shape, st, pad, dil, groups)
            continue
        sh, out = ops._conv3d_shape(x_shape, w_shape, st, pad, dil, groups)
        assert (x_shape[0], O) + out == tuple(want)
        assert (sh.B, sh.C, sh.D, sh.H, sh.W, sh.O, sh.KD, sh.KH, sh.KW) == x_shape + w_shape[:1] + k
        assert (sh.stride_d, sh.pad_h, sh.dil_w, sh.groups) == (st[0], pad[1], dil[2], groups)


def test_conv3d_shape_refuses_a_kernel_larger_than_the_padded_input():
    with pytest.raises(BnnHipError, match="kernel larger"):
        ops._conv3d_shape((1, 2, 4, 9, 9), (3, 2, 5, 3, 3), (1, 1, 1), (0, 0, 0), (1, 1, 1), 1)
    with pytest.raises(BnnHipError, match="kernel larger"):
        ops._conv3d_shape((1, 2, 4, 9, 9), (3, 2, 3, 3, 3), (1, 1, 1), (0, 0, 0), (2, 1, 1), 1)
    ops._conv3d_shape((1, 2, 4, 9, 9), (3, 2, 5, 3, 3), (1, 1, 1), (1, 0, 0), (1, 1, 1), 1)      # padding makes it fit


def test_cpu_normal_conv3d_is_the_reference_expression():
    torch.manual_seed(3)
    layer = NormalConv3d(3, 4, (3, 1, 2), stride=(2, 1, 1), padding=1, groups=1)
    x = torch.randn(2, 3, 5, 6, 7)
    y = layer(x)
    w, b = layer.sampled
    assert torch.equal(y, F.conv3d(x, w, b, layer.stride, layer.padding, layer.dilation, layer.groups))
    y2 = layer(x, sample=False)
    assert torch.equal(y2, y)


# ------------------------------------------------------------------------------------------------ GPU helpers
def _draws(layer, mode):
    """The K1 draws (S, ...) of the layer's recorded keys, float64 (bf16-rounded in the bf16 mode)."""
    kw = layer.weight.draw_key
    w = ops._sample_affine_philox_raw(layer.weight.mean.detach(), layer.weight.scale.detach(), kw).double().cpu()
    b = None
    if layer.bias is not None:
        b = ops._sample_affine_philox_raw(layer.bias.mean.detach(), layer.bias.scale.detach(), layer.bias.draw_key).double().cpu()
    return (bf(w) if mode == "bf16" else w), b


def _geo(layer):
    return layer.stride, layer.padding, layer.dilation, layer.groups


def _check_forward(y, x_s, layer, w, b, mode, what):
    """y (B, O, ...) of one sample vs float64 conv3d of x_s (float64 CPU) on draws w, b."""
    geo = _geo(layer)
    xr = bf(x_s) if mode == "bf16" else x_s
    want = F.conv3d(xr, w, b, *geo)
    if mode == "f32":
        assert_close_scaled(N(y), want.numpy(), 1e-5, what)
    else:
        K = w[0].numel()
        mag = F.conv3d(xr.abs(), w.abs(), None if b is None else b.abs(), *geo)
        assert_within(N(y), want.numpy(), ((K + 2) * U * mag).numpy() + 1e-30, what)


class Vol(BayesianNetworkModule):
    """[optional leading NormalConv3d] -> NormalConv3d -> flatten logits."""

    def __init__(self, C, O, S, front=False, k=3, pad=1):
        super().__init__(C, O, samples=S)
        self.front = NormalConv3d(C, C, 1) if front else None
        self.conv = NormalConv3d(C, O, k, padding=pad)

    def _forward(self, x):
        if self.front is not None:
            x = self.front(x)
        return self.conv(x).flatten(1)


# ------------------------------------------------------------------------------------------------ GPU: MC-batched forward
@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("front", [False, True])
def test_mc_batched_conv3d_draws_every_sample(mode, S, front):
    import bayesianneuralnetworks_amd as bnn
    dev = torch.device("cuda:0")
    B, C, O = 3, 4, 6
    torch.manual_seed(11 + S)
    net = Vol(C, O, S, front=front).to(dev)
    seeded.pin_streams(net, 2000)
    net.mc_batched = True
    x = torch.randn(B, C, 5, 6, 7, generator=torch.Generator().manual_seed(4))
    bnn.set_compute(mode)
    try:
        bnn.manual_seed(21)
        box = []
        hnd = net.conv.register_forward_pre_hook(lambda m, a: box.append(a[0].detach().clone()))
        with torch.no_grad():
            ys = net(x.to(dev))
        hnd.remove()
        ys = ys if isinstance(ys, list) else [ys]
        assert len(ys) == S and all(t.shape == (B, O * 5 * 6 * 7) for t in ys)
        for a in range(S):
            for c in range(a + 1, S):
                assert not torch.equal(ys[a], ys[c]), (a, c)
        w, b = _draws(net.conv, mode)
        assert w.shape[0] == S
        xin = box[0].double().cpu()
        assert xin.shape[0] == (B * S if front and S > 1 else B)           # shared input unless a Bayesian layer is in front
        for s in range(S):
            xs = xin[s * B:(s + 1) * B] if xin.shape[0] == B * S else xin
            _check_forward(ys[s].reshape(B, O, 5, 6, 7), xs, net.conv, w[s], b[s], mode, "%s S=%d sample %d" % (mode, S, s))
    finally:
        bnn.set_compute("f32")


@gpu
@pytest.mark.parametrize("S", [1, 8])
def test_conv3d_forward_is_two_launches_and_no_torch_conv(monkeypatch, S):
    import bayesianneuralnetworks_amd as bnn
    from bayesianneuralnetworks_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def refuse(*a, **k):
        raise AssertionError("torch conv3d called on the device path")

    monkeypatch.setattr(torch.nn.functional, "conv3d", refuse)
    torch.manual_seed(5)
    net = Vol(3, 5, S).to(dev)
    seeded.pin_streams(net, 2100)
    net.mc_batched = True
    bnn.manual_seed(3)
    x = torch.randn(4, 3, 6, 6, 6, device=dev)
    with torch.no_grad():
        net(x)                                              # warm (workspace registration and the like)
        torch.cuda.synchronize()
        n0 = lib.bnn_launch_count()
        net(x)
        torch.cuda.synchronize()
        assert lib.bnn_launch_count() - n0 == 2              # the draw (weight + bias, all samples) + the contraction
    if S > 1:
        with torch.no_grad():
            u = net.predictive_uncertainty(x, inputs="logits")
        assert float(u.epistemic.min()) >= 0 and float(u.epistemic.mean()) > 0


# ------------------------------------------------------------------------------------------------ GPU: forward + backward sweep
def _sweep():
    g = np.random.RandomState(7)
    cases = [
        # C, O, vol, k, stride, pad, dil, groups, bias, S, shared
        (1, 1, (7, 9, 11), 1, 1, 0, 1, 1, True, 1, True),
        (3, 5, (7, 9, 11), 3, 1, 1, 1, 1, True, 3, True),
        (16, 32, (5, 6, 7), (3, 1, 2), (2, 1, 1), 1, 1, 2, False, 3, False),
        (3, 5, (7, 9, 11), 3, 2, 0, 2, 1, False, 1, False),
        (16, 32, (6, 5, 4), 3, 2, 1, 1, 2, True, 3, True),
        (16, 1, (5, 5, 6), (3, 1, 2), 1, 0, (2, 1, 1), 1, True, 3, False),
    ]
    for _ in range(6):
        groups = int(g.choice([1, 2]))
        C = int(g.choice([1, 3, 16])) * (groups if groups > 1 else 1)
        O = int(g.choice([1, 5, 32])) * groups
        k = [1, 3, (3, 1, 2)][g.randint(3)]
        st = [1, 2, (2, 1, 1)][g.randint(3)]
        cases.append((C, O, (7, 9, 11), k, st, int(g.randint(2)), int(g.choice([1, 2])), groups, bool(g.randint(2)),
                      int(g.choice([1, 3])), bool(g.randint(2))))
    return cases


def _layer_backward(layer, x, S, shared, mode, dev, gseed):
    """y = layer(x) in an MC context of S samples, loss = <y, R> -> (y, R, grads of x and the posterior tensors)."""
    from bayesianneuralnetworks_amd import _mc
    xd = x.to(dev).requires_grad_(True)
    B = x.shape[0] if shared else x.shape[0] // S
    with _mc.McContext(S, B, 0):
        y = layer(xd)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
    ps = [layer.weight.mean, layer.weight.scale] + ([layer.bias.mean, layer.bias.scale] if layer.bias is not None else [])
    grads = torch.autograd.grad(y, [xd] + ps, R.to(dev))
    return y, R, grads


def _ref_backward(layer, x, S, shared, mode, R):
    """float64 reference of y and of every gradient, with derived bounds for the bf16 mode (None in the fp32 mode)."""
    geo = _geo(layer)
    w, b = _draws(layer, mode)
    kw = layer.weight.draw_key
    eps = ops.eps_philox(tuple(layer.weight.mean.shape), kw, layer.weight.mean.device).double().cpu()
    sig = torch.sigmoid(layer.weight.scale.detach().double().cpu())
    B = x.shape[0] if shared else x.shape[0] // S
    bfm = mode == "bf16"
    xr = bf(x.double()) if bfm else x.double()
    Rr = bf(R.double()) if bfm else R.double()
    gx = torch.zeros_like(x, dtype=torch.float64)
    gxb = torch.zeros_like(gx)
    gmu = torch.zeros_like(w[0]); grho = torch.zeros_like(w[0]); gmub = torch.zeros_like(gmu); grhob = torch.zeros_like(gmu)
    gb, gbb = [], []
    T = w[0, 0].numel()
    Ng = w.shape[1] // layer.groups
    for s in range(S):
        sl = slice(None) if shared else slice(s * B, (s + 1) * B)
        xs = xr[sl].clone().requires_grad_(True)
        ws = w[s].clone().requires_grad_(True)
        rs = Rr[s * B:(s + 1) * B]
        ys = F.conv3d(xs, ws, None, *geo)
        g_x, g_w = torch.autograd.grad(ys, (xs, ws), rs)
        xa = xs.detach().abs().requires_grad_(True)
        wa = ws.detach().abs().requires_grad_(True)
        ya = F.conv3d(xa, wa, None, *geo)
        m_x, m_w = torch.autograd.grad(ya, (xa, wa), rs.abs())
        P = ys[0, 0].numel()
        gx[sl] += g_x
        Lx = (S if shared else 1) * Ng * T
        gxb[sl] += (Lx + 2) * U * m_x
        gw_b = (B * P + 2) * U * m_w
        gmu += g_w
        gmub += gw_b + 4 * U * g_w.abs()
        grho += g_w * eps[s].double() * sig
        grhob += (gw_b + 8 * U * g_w.abs()) * eps[s].abs() * sig
        if b is not None:
            gbs = R[s * B:(s + 1) * B].double().sum((0, 2, 3, 4))
            gb.append(gbs)
            gbb.append((B * P + 2) * U * R[s * B:(s + 1) * B].double().abs().sum((0, 2, 3, 4)))
    refs = [gx, gmu, grho]
    bounds = [gxb, gmub, grhob]
    if b is not None:
        ebs = ops.eps_philox(tuple(layer.bias.mean.shape), layer.bias.draw_key, layer.bias.mean.device).double().cpu()
        sgb = torch.sigmoid(layer.bias.scale.detach().double().cpu())
        refs += [sum(gb), sum(gb[s] * ebs[s] for s in range(S)) * sgb]
        bounds += [sum(gbb) + 4 * U * sum(g.abs() for g in gb),
                   sum((gbb[s] + 8 * U * gb[s].abs()) * ebs[s].abs() for s in range(S)) * sgb]
    return refs, bounds


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", _sweep())
def test_conv3d_sweep_forward_and_backward(mode, case):
    import bayesianneuralnetworks_amd as bnn
    C, O, vol, k, st, pad, dil, groups, bias, S, shared = case
    dev = torch.device("cuda:0")
    torch.manual_seed(C * 31 + O)
    layer = NormalConv3d(C, O, k, stride=st, padding=pad, dilation=dil, groups=groups, bias=bias).to(dev)
    seeded.pin_streams(layer, 2200)
    B = 2
    x = torch.randn((B if shared else S * B, C) + vol, generator=torch.Generator().manual_seed(9))
    bnn.set_compute(mode)
    try:
        bnn.manual_seed(13)
        y, R, grads = _layer_backward(layer, x, S, shared, mode, dev, 17)
        w, b = _draws(layer, mode)
        for s in range(S):
            xs = x.double() if shared else x[s * B:(s + 1) * B].double()
            _check_forward(y[s * B:(s + 1) * B], xs, layer, w[s], None if b is None else b[s], mode, "%s %s y[%d]" % (mode, case, s))
        refs, bounds = _ref_backward(layer, x, S, shared, mode, R)
        names = ["x", "weight.mean", "weight.scale", "bias.mean", "bias.scale"]
        for got, ref, bd, name in zip(grads, refs, bounds, names):
            if mode == "f32":
                assert_close_scaled(N(got), ref.numpy(), 1e-4, "%s grad %s" % (case, name))
            else:
                assert_within(N(got), ref.numpy(), bd.numpy() + 1e-30, "%s grad %s" % (case, name))
    finally:
        bnn.set_compute("f32")


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_conv3d_backward_is_bitwise_reproducible(mode):
    import bayesianneuralnetworks_amd as bnn
    dev = torch.device("cuda:0")
    torch.manual_seed(2)
    layer = NormalConv3d(8, 16, 3, padding=1).to(dev)
    seeded.pin_streams(layer, 2300)
    x = torch.randn(4, 8, 12, 12, 12, generator=torch.Generator().manual_seed(1))
    bnn.set_compute(mode)
    try:
        bnn.manual_seed(5)
        _, _, g1 = _layer_backward(layer, x, 3, True, mode, dev, 3)
        from bayesianneuralnetworks_amd import _mc
        xd = x.to(dev).requires_grad_(True)
        with _mc.McContext(3, 4, 0):
            y = layer(xd, sample=False)                  # the same keys
        R = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        g2 = torch.autograd.grad(y, [xd, layer.weight.mean, layer.weight.scale, layer.bias.mean, layer.bias.scale], R)
        for a, c in zip(g1, g2):
            assert torch.equal(a, c)
    finally:
        bnn.set_compute("f32")


@gpu
def test_two_conv3d_layers_in_a_row_each_get_their_own_slabs():
    """Two layers, one backward: the second layer's weight gradient runs while the first's slabs would still be live if they
    shared a buffer; both match float64."""
    import bayesianneuralnetworks_amd as bnn
    from bayesianneuralnetworks_amd import _mc
    dev = torch.device("cuda:0")
    torch.manual_seed(8)
    l1 = NormalConv3d(4, 8, 3, padding=1).to(dev)
    l2 = NormalConv3d(8, 6, 3, padding=1).to(dev)
    seeded.pin_streams(torch.nn.ModuleList([l1, l2]), 2400)
    S, B = 3, 2
    x = torch.randn(B, 4, 16, 16, 16, generator=torch.Generator().manual_seed(2))
    bnn.manual_seed(9)
    with _mc.McContext(S, B, 0):
        h = l1(x.to(dev))
        y = l2(h)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
    g = torch.autograd.grad(y, [l1.weight.mean, l2.weight.mean], R.to(dev))
    w1, b1 = _draws(l1, "f32")
    w2, b2 = _draws(l2, "f32")
    x64 = x.double()
    want1 = torch.zeros_like(w1[0])
    want2 = torch.zeros_like(w2[0])
    for s in range(S):
        a = w1[s].clone().requires_grad_(True)
        c = w2[s].clone().requires_grad_(True)
        ys = F.conv3d(F.conv3d(x64, a, b1[s], 1, 1), c, b2[s], 1, 1)
        ga, gc = torch.autograd.grad(ys, (a, c), R[s * B:(s + 1) * B].double())
        want1 += ga
        want2 += gc
    assert_close_scaled(N(g[0]), want1.numpy(), 1e-4, "layer 1 g_mu")
    assert_close_scaled(N(g[1]), want2.numpy(), 1e-4, "layer 2 g_mu")


@gpu
@pytest.mark.parametrize("example", [(1, 1, 1, 1, 1, 1, 1, False), (1, 1, 1, 1, 1, 1, 1, True),
                                     (3, 4, 3, 1, 1, 1, 1, False), (3, 4, 3, 1, 1, 1, 1, True)])
def test_reference_normal_conv3d_setup_on_the_device(example):
    """The reference's test_NormalConv3d (mean 1, scale -100, ones input 10^3) on a CUDA layer."""
    dev = torch.device("cuda:0")
    i, o, k, s, pad, d, g, b = example
    layer = NormalConv3d(i, o, k, s, pad, d, g, b).to(dev)
    with torch.no_grad():
        layer.weight.mean.fill_(1)
        layer.weight.scale.fill_(-100)
        if b:
            layer.bias.mean.fill_(3)
            layer.bias.scale.fill_(-100)
    layer.sample()
    x = torch.ones(1, i, 10, 10, 10, device=dev)
    with torch.no_grad():
        result = layer(x)
    expected = F.conv3d(torch.ones(1, i, 10, 10, 10), torch.ones(o, i // g, k, k, k), None, s, pad, d, g)
    if b:
        expected = expected + 3
    assert result.shape == expected.shape
    assert torch.allclose(result.cpu(), expected, atol=1e-5, rtol=1e-5)
