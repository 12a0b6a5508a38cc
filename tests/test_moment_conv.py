"""Sampling-free inference for conv nets (K17): moments through NormalConv / LocalReparamConv 1d / 2d / 3d and ELU,

    m = convNd(a_m, mu_w) + mu_b,   v = convNd(a_m^2, sigma_w^2) + convNd(a_v, mu_w^2 + sigma_w^2) + sigma_b^2,

the moment-matched ELU, the nn.moment_activations rewrite and the softmax link.  CPU tests: the conv marginals against weight
sampling, the ELU closed form against quadrature, the host surface, the argument checks, the built code object.  GPU tests: the
kernel against float64, the fused epilogue, the ELU grid, the example network's Bayesian tail, alignment, graph capture.

Bounds.  fp32 mode: 1e-5 of the output scale (test_lrt_device.scaled_bound).  bf16 mode: float64 on the planes as the kernel rounds
them (a_m, a_m^2 -- squared in fp32 first --, a_v, mu_w, sigma_w^2, fma(mu_w, mu_w, sigma_w^2) in fp32 first, each to bf16, RNE);
the device differs by the fp32 accumulation alone: gamma_n sum |a| |b| with n = K + 1 for m and 2 K + 1 for v, K = C / groups x
taps (test_moment_propagation.py's rule).  ELU: ELU_MEAN_TOL / ELU_VAR_TOL below.
"""
import ctypes
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, _rng, ops
from bayesianneuralnetworks_amd import nn as bnn_nn
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, NormalConv2d, NormalLinear

from alignment import guards_intact, offset_view, output_view, same_bits
from bf16ref import gamma, rne_bf16
from test_flipout_mc import _code_object_notes
from test_lrt_device import assert_within, scaled_bound, sigma64
from test_moment_propagation import linear_ref, six_se

gpu = pytest.mark.gpu

# The moment-matched ELU against ops.moments_elu_f64, in units of s = sqrt(v) (mean) and of v (variance).  Measured on the MI355X
# over alpha in [-12, 12] (4801 points) at v = 1e-6, 0.3, 1, 47 for a = 1 and a = 0.5 (test_elu_matches_float64_on_a_grid prints
# them): worst mean deviation 4.655e-7 s (a = 1, v = 1e-6), worst variance deviation 5.684e-8 v (a = 1, v = 1e-6); per
# (a, v), mean / variance: a = 1: 4.66e-7 / 5.68e-8, 2.18e-7 / 4.97e-8, 2.38e-7 / 2.98e-8, 1.71e-7 / 4.06e-8; a = 0.5: 2.33e-7 /
# 5.68e-8, 2.17e-7 / 4.97e-8, 2.37e-7 / 2.98e-8, 2.34e-7 / 4.06e-8.  The device function works in fp64, so what is measured is
# the fp32 rounding of its two results (|mean'| <= 12 s on the grid: at most 12 x 2^-24 = 7.2e-7 s, and 2^-24 = 6e-8 v).  The
# constants are 4 x the measured worst: the margin covers inputs off the grid.  Both are
# below 1e-5, the project's parity rule.
ELU_MEAN_TOL = 1.87e-6
ELU_VAR_TOL = 2.28e-7

ELU_GRID_V = (1e-6, 0.3, 1.0, 47.0)
ELU_GRID_A = (1.0, 0.5)


def conv_params(O, Cg, kernel, bias, seed, rho0=-3.0):
    g = torch.Generator().manual_seed(seed)
    K = Cg * int(np.prod(kernel))
    mu_w = (torch.rand(O, Cg, *kernel, generator=g) * 2 - 1) / K ** 0.5
    rho_w = rho0 + 0.3 * torch.randn(O, Cg, *kernel, generator=g)
    mu_b = (torch.rand(O, generator=g) * 2 - 1) / K ** 0.5 if bias else None
    rho_b = rho0 + 0.3 * torch.randn(O, generator=g) if bias else None
    return mu_w, rho_w, mu_b, rho_b


def conv_input(shape, with_var, seed):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(*shape, generator=g)
    return ops.Moments(mean, 0.5 * torch.rand(*shape, generator=g) ** 2 if with_var else None)


def convnd(nd):
    return (F.conv1d, F.conv2d, F.conv3d)[nd - 1]


# ================================================================================================ CPU
def _unfold_outputs(x, w, b, kernel, stride, padding):
    """y[s] = conv2d(x or x[s], w[s]) + b[s] for S weight draws through one unfold: x (B, C, H, W) or (S, B, C, H, W)."""
    S, O = w.shape[:2]
    if x.dim() == 4:
        cols = F.unfold(x, kernel, padding=padding, stride=stride)                      # (B, K, P)
        return torch.einsum("sok,bkp->sbop", w.reshape(S, O, -1), cols) + b[:, None, :, None]
    Bn = x.shape[1]
    cols = F.unfold(x.reshape(S * Bn, *x.shape[2:]), kernel, padding=padding, stride=stride)
    cols = cols.reshape(S, Bn, *cols.shape[1:])
    return torch.einsum("sok,sbkp->sbop", w.reshape(S, O, -1), cols) + b[:, None, :, None]


@pytest.mark.parametrize("with_var", [False, True])
def test_conv_marginals_are_exact_against_weight_sampling(with_var):
    """2 images, 2 -> 3 channels, 5 x 4, kernel (2, 3), stride (1, 2), padding (1, 0), bias; 250 000 float64 weight draws (and,
    for a Moments input, as many independent draws of every input element): each output's marginal mean and variance are
    ops.moments_convNd_f64's, within 6 standard errors."""
    S, chunk = 250_000, 50_000
    g = torch.Generator().manual_seed(417)
    kernel, stride, padding = (2, 3), (1, 2), (1, 0)
    mu_w, rho_w, mu_b, rho_b = [t.double() for t in conv_params(3, 2, kernel, True, 3, rho0=-1.0)]
    am = torch.randn(2, 2, 5, 4, generator=g, dtype=torch.float64)
    av = 0.5 * torch.rand(2, 2, 5, 4, generator=g, dtype=torch.float64) ** 2 if with_var else None
    mom = ops.moments_convNd_f64(ops.Moments(am, av), mu_w, rho_w, mu_b, rho_b, stride, padding, (1, 1), 1)
    assert mom.mean.dtype == torch.float64 and mom.mean.shape == (2, 3, 6, 1) and (mom.var > 0).all()
    ys = []
    for _ in range(S // chunk):
        w = mu_w + sigma64(rho_w) * torch.randn((chunk,) + tuple(mu_w.shape), generator=g, dtype=torch.float64)
        b = mu_b + sigma64(rho_b) * torch.randn((chunk, 3), generator=g, dtype=torch.float64)
        x = am if av is None else am + av.sqrt() * torch.randn((chunk,) + tuple(am.shape), generator=g, dtype=torch.float64)
        ys.append(_unfold_outputs(x, w, b, kernel, stride, padding).reshape(chunk, 2, 3, 6, 1))
    six_se(torch.cat(ys), mom.mean, mom.var, "conv 2->3 (var=%s) against %d weight draws" % (with_var, S))


def elu_quadrature(m, v, a, nodes=200):
    """E[elu(x)] and Var[elu(x)] for x ~ N(m, v) by Gauss-Legendre on [m - 14 s, 0] and [0, m + 14 s] (the kink at 0 is a
    panel edge; beyond 14 s the Gaussian weighs 1e-43), float64, vectorised over m."""
    t, w = np.polynomial.legendre.leggauss(nodes)
    t, w = torch.from_numpy(t), torch.from_numpy(w)
    s = math.sqrt(v)
    lo, hi = m - 14 * s, m + 14 * s
    mid = torch.zeros_like(m).clamp(min=lo, max=hi)

    def panel(a0, b0, f):
        x = 0.5 * (a0 + b0)[:, None] + 0.5 * (b0 - a0)[:, None] * t
        pdf = torch.exp(-0.5 * ((x - m[:, None]) / s) ** 2) / (s * math.sqrt(2 * math.pi))
        return x, 0.5 * (b0 - a0)[:, None] * w * pdf, f(x)

    xn, wn, fn = panel(lo, mid, lambda x: a * torch.expm1(x))
    xp, wp, fp = panel(mid, hi, lambda x: x)
    mean = (wn * fn).sum(1) + (wp * fp).sum(1)
    var = (wn * (fn - mean[:, None]) ** 2).sum(1) + (wp * (fp - mean[:, None]) ** 2).sum(1)
    return mean, var


def test_elu_reference_against_quadrature():
    """ops.moments_elu_f64 against quadrature over alpha in [-12, 12] (4801 points) at v = 1e-6, 0.3, 1, 47 and a = 1, 0.5, to
    1e-8 of s and of v; the limits."""
    alpha = torch.linspace(-12, 12, 4801, dtype=torch.float64)
    for a in ELU_GRID_A:
        for v in ELU_GRID_V:
            s = math.sqrt(v)
            m = alpha * s
            out = ops.moments_elu_f64(ops.Moments(m, torch.full_like(m, v)), a)
            qm, qv = elu_quadrature(m, v, a)
            dm, dv = ((out.mean - qm).abs() / s).max().item(), ((out.var - qv).abs() / v).max().item()
            print("moments_elu_f64 a = %g v = %g: against quadrature %.2e s, %.2e v" % (a, v, dm, dv))
            assert dm <= 1e-8 and dv <= 1e-8, (a, v, dm, dv)
            assert (out.var >= 0).all() and (out.mean >= -a).all()
    f = ops.moments_elu_f64
    t64 = lambda x: torch.tensor([x], dtype=torch.float64)         # noqa: E731
    for a in ELU_GRID_A:
        for v in (1e-6, 0.3, 47.0):
            s = math.sqrt(v)
            hi, lo = f(ops.Moments(t64(12 * s), t64(v)), a), f(ops.Moments(t64(-12 * s), t64(v)), a)
            assert abs(hi.mean.item() - 12 * s) <= 1e-12 * s and abs(hi.var.item() - v) <= 1e-12 * v       # passes the input
            m = -12 * s                                                                                     # the lognormal limit
            assert abs(lo.mean.item() - a * math.expm1(m + v / 2)) <= 1e-12 * max(s, a)
            assert abs(lo.var.item() - a * a * math.exp(2 * m + v) * math.expm1(v)) <= 1e-12 * max(v, a * a) and lo.var.item() >= 0
        z = f(ops.Moments(torch.tensor([-2.0, 0.0, 3.0]), torch.zeros(3)), a)
        assert torch.equal(z.mean, F.elu(torch.tensor([-2.0, 0.0, 3.0], dtype=torch.float64), a)) and not z.var.any()
        n = f(ops.Moments(torch.tensor([-1.0, 2.0])), a)
        assert n.var is None and torch.equal(n.mean, F.elu(torch.tensor([-1.0, 2.0], dtype=torch.float64), a))
    big = f(ops.Moments(t64(-10.0), t64(2000.0)))                   # exp(m + v / 2) alone would overflow
    assert math.isfinite(big.mean.item()) and math.isfinite(big.var.item()) and big.var.item() >= 0


class Flatten(torch.nn.Module):
    """The examples' own Flatten."""

    def forward(self, x):
        return x.view(x.size(0), -1)


class Tail(BayesianNetworkModule):
    """The MNIST example's Bayesian tail behind a deterministic trunk: conv -> ELU -> NormalConv2d(k3 s2 p1) -> ELU -> Flatten ->
    NormalLinear -> Softmax."""

    def __init__(self, channels=64, side=6, classes=10, conv=NormalConv2d, trunk=True, flatten=Flatten):
        super().__init__(channels, classes, samples=4)
        out_side = (side + 2 - 3) // 2 + 1
        front = [torch.nn.Conv2d(channels, channels, 1), torch.nn.ELU()] if trunk else []
        self.layers = torch.nn.Sequential(*front, conv(channels, channels, 3, padding=1, stride=2), torch.nn.ELU(), flatten(),
                                          NormalLinear(channels * out_side * out_side, classes), torch.nn.Softmax(dim=-1))

    def _forward(self, x):
        return self.layers(x)


class Seq(BayesianNetworkModule):
    """A container around given layers (the sampling side of a comparison)."""

    def __init__(self, layers):
        super().__init__(0, 0, samples=1)
        self.layers = layers
        self.mc_batched = True

    def _forward(self, x):
        return self.layers(x)


def tail_recursion64(net, x):
    """The hand-written float64 recursion of a CPU Tail: -> the logit Moments."""
    mods = list(net.layers)
    i = 0
    h = x.detach()
    while not isinstance(mods[i], bnn_nn.BayesianModule):
        h = mods[i](h)
        i += 1
    conv, lin = mods[i], [m for m in mods if isinstance(m, NormalLinear)][0]
    c = lambda t: t.detach().cpu()         # noqa: E731
    mom = ops.moments_convNd_f64(h.detach(), c(conv.weight.mean), c(conv.weight.scale), c(conv.bias.mean), c(conv.bias.scale),
                                 conv.stride, conv.padding, conv.dilation, conv.groups)
    mom = ops.moments_elu_f64(mom, 1.0)
    mom = ops.Moments(mom.mean.reshape(x.shape[0], -1), mom.var.reshape(x.shape[0], -1))
    return ops.moments_linear_f64(mom, c(lin.weight.mean), c(lin.weight.scale), c(lin.bias.mean), c(lin.bias.scale))


def test_host_surface_on_the_cpu():
    torch.manual_seed(0)
    net = Tail(channels=4, side=6, classes=3)
    x = torch.randn(5, 4, 6, 6)
    keys0 = list(net.state_dict().keys())
    # un-rewritten torch activations stay refused
    with pytest.raises(ops.BnnHipError, match="NormalLinear / LocalReparamLinear"):
        net.predictive_moments(x)
    torch.manual_seed(3)
    before = net(x, samples=1)
    assert bnn_nn.moment_activations(net) == 3 + 0            # two ELUs and the softmax
    assert bnn_nn.moment_activations(net) == 0                # idempotent
    assert list(net.state_dict().keys()) == keys0
    assert [type(m).__name__ for m in net.layers] == ["Conv2d", "MomentELU", "NormalConv2d", "MomentELU", "Flatten", "NormalLinear",
                                                      "MomentSoftmax"]
    assert net.layers[2].__dict__["_moment_act"] == ("elu", 1.0) and "_moment_act" not in net.layers[2]._modules
    torch.manual_seed(3)
    assert torch.equal(net(x, samples=1), before)            # the sampling path is the parent's, bit for bit
    # the twins on tensors
    t = torch.randn(7, 5)
    assert torch.equal(bnn_nn.MomentReLU()(t), torch.nn.ReLU()(t))
    assert torch.equal(bnn_nn.MomentELU(alpha=0.5)(t), torch.nn.ELU(alpha=0.5)(t))
    assert torch.equal(bnn_nn.MomentSoftmax(dim=-1)(t), torch.nn.Softmax(dim=-1)(t))
    # the moment pass is the hand-written float64 recursion
    e0 = _rng.default_generator.epoch_host
    dk = (net.layers[2].weight.draw_key, net.layers[5].weight.draw_key)
    mom = net.predictive_moments(x)
    want = tail_recursion64(net, x)
    assert mom.link == "softmax" and mom.mean.dtype == torch.float32 and mom.mean.shape == (5, 3)
    assert torch.equal(mom.mean, want.mean.float()) and torch.equal(mom.var, want.var.float())
    assert _mc.moments_current() is None and _rng.default_generator.epoch_host == e0
    assert (net.layers[2].weight.draw_key, net.layers[5].weight.draw_key) == dk
    # the standalone twin behind the conv gives what the fused epilogue gives, and torch.nn.Flatten is the examples' Flatten
    del net.layers[2].__dict__["_moment_act"]
    alone = net.predictive_moments(x)
    assert torch.equal(alone.mean, mom.mean) and torch.equal(alone.var, mom.var)
    net.layers[4] = torch.nn.Flatten()
    assert bnn_nn.moment_activations(net) == 0 and net.layers[2].__dict__["_moment_act"] == ("elu", 1.0)
    again = net.predictive_moments(x)
    assert torch.equal(again.mean, mom.mean) and torch.equal(again.var, mom.var)
    # the link is applied by the tails
    torch.manual_seed(5)
    u = net.predictive_uncertainty(x, samples=8, inputs="probs", propagation="moments")
    torch.manual_seed(5)
    probs = torch.softmax(ops.moments_sample(mom, None, 8), -1)
    assert all(torch.equal(a, b) for a, b in zip(u, ops.uncertainty_f64(probs, "probs")))
    assert (u.mean.sum(-1) - 1).abs().max() <= 1e-6
    with pytest.raises(ops.BnnHipError, match="link"):
        net.predictive_regression(x, outputs="values", propagation="moments")
    # a layer fed linked moments raises
    linked = ops.Moments(torch.randn(5, 4, 6, 6), None, link="softmax")
    with _mc.MomentContext():
        for layer, inp in ((net.layers[2], linked), (net.layers[5], ops.Moments(torch.randn(5, 36), None, "softmax")),
                           (net.layers[3], linked), (net.layers[6], linked)):
            with pytest.raises(ops.BnnHipError, match="link"):
                layer(inp)
    with pytest.raises(ValueError):
        ops.Moments(torch.zeros(2), None, "sigmoid")
    assert ops.Moments(torch.zeros(2), torch.zeros(2)).link is None              # the two-argument constructor stays valid
    # what stays refused
    for bad in (bnn_nn.FlipOutNormalConv2d, bnn_nn.MCDropoutConv2d):
        kw = {"drop_prob": 0.1} if bad is bnn_nn.MCDropoutConv2d else {}
        other = Tail(channels=4, side=6, classes=3, conv=lambda *a, **k: bad(*a, **k, **kw))
        bnn_nn.moment_activations(other)
        with pytest.raises(ops.BnnHipError, match=bad.__name__):
            other.predictive_moments(x)
    # LocalReparamConv2d is NormalConv2d's moment layer
    lrt = Tail(channels=4, side=6, classes=3, conv=bnn_nn.LocalReparamConv2d)
    lrt.load_state_dict(net.state_dict())
    bnn_nn.moment_activations(lrt)
    got = lrt.predictive_moments(x)
    assert torch.equal(got.mean, mom.mean) and torch.equal(got.var, mom.var)
    # one image, 1-d and 3-d layers, ReLU fused behind a conv
    for nd, cls in ((1, bnn_nn.NormalConv1d), (3, bnn_nn.LocalReparamConv3d)):
        seq = torch.nn.Sequential(cls(2, 3, 2, stride=1, padding=1), torch.nn.ReLU())
        assert bnn_nn.moment_activations(seq) == 1 and seq[0].__dict__["_moment_act"] == "relu"
        xi = torch.randn(4, 2, *([5] * nd))
        with _mc.MomentContext():
            full, one = seq(xi), seq(xi[0])
        c = seq[0]
        ref = ops.moments_convNd_f64(xi, c.weight.mean, c.weight.scale, c.bias.mean, c.bias.scale, c.stride, c.padding, c.dilation,
                                     c.groups, activation="relu")
        assert torch.equal(full.mean, ref.mean) and torch.equal(full.var, ref.var)
        assert one.mean.shape == ref.mean.shape[1:] and torch.allclose(one.mean, ref.mean[0], rtol=1e-12, atol=1e-12)
        assert torch.allclose(one.var, ref.var[0], rtol=1e-12, atol=1e-12)


def test_moments_reshape_like_tensors():
    m, v = torch.arange(24.0).reshape(2, 3, 4), torch.arange(24.0).reshape(2, 3, 4) + 1
    mom = ops.Moments(m, v)
    assert mom.shape == (2, 3, 4) and mom.size() == m.size() and mom.size(0) == 2 and mom.size(-1) == 4 and mom.dim() == 3
    for got, fn in ((mom.view(2, -1), lambda t: t.view(2, -1)), (mom.view(mom.size(0), -1), lambda t: t.view(2, -1)),
                    (mom.reshape(6, 4), lambda t: t.reshape(6, 4)), (mom.flatten(1), lambda t: t.flatten(1)),
                    (mom.flatten(), lambda t: t.flatten()), (torch.nn.Flatten()(mom), lambda t: t.flatten(1))):
        assert isinstance(got, ops.Moments) and torch.equal(got.mean, fn(m)) and torch.equal(got.var, fn(v))
    det = ops.Moments(m).flatten(1)
    assert det.var is None and det.mean.shape == (2, 12)
    assert ops.Moments(m, v, "softmax").view(6, 4).link == "softmax"


def test_conv_and_elu_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one, odd, off8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(72)
    F32, BF16 = _lib.COMPUTE_F32, _lib.COMPUTE_BF16

    def shape(B=2, C=4, D=1, H=6, W=6, O=4, k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1), d=(1, 1, 1), groups=1):
        return _lib.Conv3dShape(B, C, D, H, W, O, *k, *s, *p, *d, groups)

    def fwd(a_m=one, a_v=None, mu_w=one, s2_w=one, mu_b=None, s2_b=None, out_m=one, out_v=one, sh=None, compute=F32, flags=0,
            alpha=1.0):
        sh = shape() if sh is None else sh
        rc = lib.bnn_conv3d_moments_forward(a_m, a_v, mu_w, s2_w, mu_b, s2_b, out_m, out_v,
                                            ctypes.byref(sh) if sh != "null" else None, compute, flags, alpha, None)
        if rc:
            assert lib.bnn_last_error().startswith(b"bnn_conv3d_moments_forward: "), lib.bnn_last_error()
        return rc

    assert fwd(a_m=None) == -1 and fwd(mu_w=None) == -1 and fwd(s2_w=None) == -1 and fwd(out_m=None) == -1 and fwd(out_v=None) == -1
    assert fwd(sh="null") == -1
    assert fwd(mu_b=one) == -1 and fwd(s2_b=one) == -1                       # a partial bias
    assert fwd(sh=shape(C=0)) == -2 and fwd(sh=shape(s=(1, 0, 1))) == -2 and fwd(sh=shape(p=(0, -1, 1))) == -2
    assert fwd(sh=shape(B=-1)) == -2
    assert fwd(sh=shape(H=2, W=2, k=(1, 5, 5), p=(0, 0, 0))) == -2            # kernel larger than the padded input
    assert fwd(sh=shape(C=4, O=4, groups=3)) == -2 and fwd(sh=shape(C=4, O=6, groups=4)) == -2
    assert fwd(sh=shape(B=1, C=1, H=65536, W=65536, O=1)) == -5                # a tensor of 2^31 elements or more
    assert b"2^31" in lib.bnn_last_error()
    assert fwd(sh=shape(B=1 << 20, C=1, H=64, W=64, O=1)) == -5                # B O P
    assert fwd(compute=7) == -3
    assert fwd(flags=_lib.FLAG_X_BF16) == -6 and fwd(flags=_lib.FLAG_Y_BF16) == -6 and fwd(flags=16) == -6
    assert fwd(flags=_lib.FLAG_RELU | _lib.FLAG_ELU) == -6
    assert b"together" in lib.bnn_last_error()
    assert fwd(flags=_lib.FLAG_ELU, alpha=-1.0) == -5 and fwd(flags=_lib.FLAG_ELU, alpha=float("nan")) == -5
    for name in ("a_m", "a_v", "mu_w", "s2_w"):
        assert fwd(**{name: odd}) == -4, name
    assert fwd(mu_b=odd, s2_b=one) == -4 and fwd(mu_b=one, s2_b=odd) == -4
    assert fwd(out_m=off8) == -4 and fwd(out_v=off8) == -4 and fwd(out_m=ctypes.c_void_p(68), compute=BF16) == -4
    assert b"16 bytes" in lib.bnn_last_error()
    assert fwd(a_m=off8, a_v=off8, mu_w=off8, s2_w=off8, mu_b=off8, s2_b=off8, sh=shape(B=0)) == 0       # inputs on the element
    assert fwd(sh=shape(B=0), compute=BF16, flags=_lib.FLAG_ELU) == 0          # no images: nothing to do
    assert fwd(sh=shape(B=0), out_m=off8) == -4 and fwd(sh=shape(B=0, C=0)) == -2       # ... after every check

    elu = lib.bnn_moments_elu
    assert elu(None, one, one, one, 4, 1.0, None) == -1 and elu(one, None, one, one, 4, 1.0, None) == -1
    assert elu(one, one, None, one, 4, 1.0, None) == -1 and elu(one, one, one, None, 4, 1.0, None) == -1
    assert elu(one, one, one, one, -1, 1.0, None) == -2
    assert elu(one, one, one, one, 4, -0.5, None) == -5 and elu(one, one, one, one, 4, float("inf"), None) == -5
    assert lib.bnn_last_error().startswith(b"bnn_moments_elu: ")
    assert elu(odd, one, one, one, 4, 1.0, None) == -4 and elu(one, one, one, odd, 4, 1.0, None) == -4
    assert elu(one, one, one, one, 0, 1.0, None) == 0
    assert lib.bnn_launch_count() == n0


def test_conv_moment_kernels_do_not_spill():
    """The four instantiations of the conv tile (bf16, fp32 x deterministic, Moments input) and the ELU launch use no scratch and
    spill nothing -- no vector register and no scalar one; k_moments' own figures are test_moment_propagation.py's."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    tiles = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn16k_moments_conv3dI[tf]Lb[01]EEEvNS_9Conv3dGeoENS_11MomConvArgsE$", n)}
    assert len(tiles) == 4, sorted(kernels)
    elu = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn13k_moments_eluE", n)}
    assert len(elu) == 1, sorted(kernels)
    for n, f in {**tiles, **elu}.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0 and \
            int(f.get("private_segment_fixed_size", 0)) == 0, (n, f)
    lds = sorted(int(f["group_segment_fixed_size"]) for f in tiles.values())
    assert lds == [30720, 46080, 55296, 82944], lds            # two / three planes of 192 rows: bf16 80-B rows, fp32 144-B rows
    # the names K7 and K11 are known by stay what they were
    assert any(re.match(r"_ZN3bnn8k_conv3dIfLi0ELb0EEEvNS_9Conv3dGeoENS_10Conv3dArgsE$", n) for n in kernels), sorted(kernels)
    assert any(re.match(r"_ZN3bnn12k_lrt_conv3dIfLi0EEEvNS_9Conv3dGeoENS_11LrtConvArgsE$", n) for n in kernels), sorted(kernels)


# ================================================================================================ GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


def to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def on(dev, mom):
    return ops.Moments(mom.mean.to(dev), None if mom.var is None else mom.var.to(dev))


def conv_ref(mom, mu_w, rho_w, mu_b, rho_b, geo, mode, dev):
    """float64 reference of ONE moments_convNd call (no activation) with the bound on the device's deviation
    -> (m, v, bound_m, bound_v).  mom: CPU Moments (fp32 values, the call's own input); geo = (stride, padding, dilation, groups)."""
    nd = mu_w.dim() - 2
    conv = convnd(nd)
    K = mu_w[0].numel()
    if mode == "f32":
        r = ops.moments_convNd_f64(mom, mu_w, rho_w, mu_b, rho_b, *geo)
        return r.mean, r.var, scaled_bound(r.mean), scaled_bound(r.var)
    # bf16: the six planes as the loader rounds them; sigma^2 is the device's fp32 value (checked against float64)
    s2_w, s2_b = ops._lrt_prepare_raw(rho_w.to(dev), None if rho_b is None else rho_b.to(dev))
    s2_w = s2_w.cpu()
    assert ((s2_w.double() - sigma64(rho_w) ** 2).abs() <= 1e-6 * sigma64(rho_w) ** 2).all()
    p_mu, p_s2 = rne_bf16(mu_w), rne_bf16(s2_w)
    p_e2 = rne_bf16((mu_w.double() ** 2 + s2_w.double()).float())           # one fp32 fma, then bf16
    q_m, q_sq = rne_bf16(mom.mean), rne_bf16(mom.mean.float() * mom.mean.float())
    m = conv(q_m, p_mu, None, *geo)
    a = conv(q_m.abs(), p_mu.abs(), None, *geo)
    v = conv(q_sq, p_s2, None, *geo)
    n_v = K
    if mom.var is not None:
        v = v + conv(rne_bf16(mom.var), p_e2, None, *geo)
        n_v = 2 * K
    if mu_b is not None:
        shp = (1, -1) + (1,) * nd
        mb, sb = mu_b.double().reshape(shp), s2_b.cpu().double().reshape(shp)
        m, a, v = m + mb, a + mb.abs(), v + sb
    return m, v, gamma(K + 1) * a + 1e-300, gamma(n_v + 1) * v + 1e-300       # v is its own sum |a| |b|: every term is >= 0


# (input shape, O, kernel, stride, padding, dilation, groups, bias): every edge of the 128 x 64 x 32 tile is crossed once --
#   B P over 128 and no multiple of it (2d-geo, 2d-wide, 3d); O / groups = 70 (2d-wide); C / groups x taps = 42, 36 (2d-wide, 3d)
#   and 576 (tail: 18 whole k-tiles); groups = 2; window, stride, padding, dilation and image all differ per axis (2d-geo, 3d);
#   P % 4: 25, 9, 63 odd, 24 and 16 multiples; one 1-d and one 3-d shape; no bias in 2d-wide.
CASES = {
    "2d-geo": ((6, 6, 9, 7), 10, (3, 2), (2, 1), (1, 0), (1, 2), 2, True),
    "tail": ((4, 64, 6, 6), 64, (3, 3), (2, 2), (1, 1), (1, 1), 1, True),
    "2d-wide": ((6, 14, 10, 6), 140, (2, 3), (1, 2), (0, 1), (2, 1), 2, False),
    "1d": ((7, 5, 50), 9, (5,), (3,), (2,), (2,), 1, True),
    "3d": ((3, 12, 5, 6, 7), 6, (1, 2, 3), (2, 1, 3), (0, 1, 2), (3, 1, 2), 2, True),
}


def case_operands(name, with_var):
    xs, O, kernel, stride, padding, dilation, groups, bias = CASES[name]
    p = conv_params(O, xs[1] // groups, kernel, bias, 11)
    return conv_input(xs, with_var, 12), p, (stride, padding, dilation, groups)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("with_var", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_conv_moments_match_float64(dev, case, with_var, mode):
    mom, p, geo = case_operands(case, with_var)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    a = on(dev, mom) if with_var else mom.mean.to(dev)
    out = ops.moments_convNd(a, *to(dev, *p), *geo, compute=mode)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 2                    # the operand launch + ONE contraction launch
    m, v, bm, bv = conv_ref(mom, *p, geo, mode, dev)
    assert out.mean.shape == m.shape and out.mean.dtype == out.var.dtype == torch.float32
    what = "%s var=%s %s" % (case, with_var, mode)
    assert_within(out.mean, m, bm, "m " + what)
    assert_within(out.var, v, bv, "v " + what)
    assert (out.var >= 0).all()
    again = ops.moments_convNd(a, *to(dev, *p), *geo, compute=mode)
    assert torch.equal(again.mean, out.mean) and torch.equal(again.var, out.var)
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("with_var", [False, True])
@pytest.mark.parametrize("act", ["relu", ("elu", 1.0), ("elu", 0.5)], ids=["relu", "elu1", "elu.5"])
@pytest.mark.parametrize("case", ["2d-geo", "2d-wide"])
def test_fused_activation_is_the_standalone_launch_bit_for_bit(dev, case, act, with_var, mode):
    mom, p, geo = case_operands(case, with_var)
    a = on(dev, mom) if with_var else mom.mean.to(dev)
    p = to(dev, *p)
    pre = ops.moments_convNd(a, *p, *geo, compute=mode)
    fused = ops.moments_convNd(a, *p, *geo, activation=act, compute=mode)
    alone = ops.moments_relu(pre) if act == "relu" else ops.moments_elu(pre, act[1])
    assert torch.equal(fused.mean, alone.mean) and torch.equal(fused.var, alone.var)
    assert not torch.equal(fused.mean, pre.mean)
    twice = ops.moments_convNd(a, *p, *geo, activation=act, compute=mode)
    assert torch.equal(twice.mean, fused.mean) and torch.equal(twice.var, fused.var)


def elu_deviation(got, m32, v32, a):
    """worst |device - float64| of moments_elu on fp32 inputs, in units of s (mean) and v (variance)"""
    ref = ops.moments_elu_f64(ops.Moments(m32, v32), a)
    s, v = v32.double().sqrt(), v32.double()
    return ((got.mean.double().cpu() - ref.mean).abs() / s).max().item(), ((got.var.double().cpu() - ref.var).abs() / v).max().item()


@gpu
def test_elu_matches_float64_on_a_grid(dev):
    """alpha in [-12, 12] (4801 points) at v = 1e-6, 0.3, 1, 47 for a = 1 and a = 0.5.  Measured on the MI355X: worst mean
    deviation 4.655e-7 s, worst variance deviation 5.684e-8 v (per (a, v) in the header comment); the bounds ELU_MEAN_TOL = 1.87e-6
    and ELU_VAR_TOL = 2.28e-7 are 4 x that (both <= 1e-5)."""
    alpha = torch.linspace(-12, 12, 4801, dtype=torch.float64)
    worst_m = worst_v = 0.0
    for a in ELU_GRID_A:
        for v in ELU_GRID_V:
            m32, v32 = (alpha * math.sqrt(v)).float(), torch.full_like(alpha, v).float()
            got = ops.moments_elu(ops.Moments(m32.to(dev), v32.to(dev)), a)
            assert (got.var >= 0).all() and torch.isfinite(got.mean).all() and torch.isfinite(got.var).all()
            dm, dv = elu_deviation(got, m32, v32, a)
            print("moments_elu a = %g v = %g: worst mean deviation %.3e s, worst variance deviation %.3e v" % (a, v, dm, dv))
            worst_m, worst_v = max(worst_m, dm), max(worst_v, dv)
    print("moments_elu: worst mean deviation %.3e s (bound %.2e), worst variance deviation %.3e v (bound %.2e)"
          % (worst_m, ELU_MEAN_TOL, worst_v, ELU_VAR_TOL))
    assert ELU_MEAN_TOL <= 1e-5 and ELU_VAR_TOL <= 1e-5
    assert worst_m <= ELU_MEAN_TOL and worst_v <= ELU_VAR_TOL
    # v == 0, the far tails, an exponent that would overflow on its own, in place
    m = torch.tensor([-2.0, 0.0, 3.0, 1e30, -1e30, -10.0], device=dev)
    v = torch.tensor([0.0, 0.0, 0.0, 1e-30, 1e-30, 2000.0], device=dev)
    z = ops.moments_elu(ops.Moments(m, v), 0.5)
    assert torch.equal(z.mean[:5].cpu(), torch.tensor([0.5 * math.expm1(-2.0), 0.0, 3.0, 1e30, -0.5]))
    assert torch.equal(z.var[:5].cpu(), torch.tensor([0.0, 0.0, 0.0, 1e-30, 0.0]))
    assert torch.isfinite(z.mean[5]) and torch.isfinite(z.var[5]) and z.var[5] >= 0
    m2, v2 = m.clone(), v.clone()
    lib = _lib.load()
    assert lib.bnn_moments_elu(m2.data_ptr(), v2.data_ptr(), m2.data_ptr(), v2.data_ptr(), m2.numel(), 0.5, ops.stream_ptr(dev)) == 0
    assert torch.equal(m2, z.mean) and torch.equal(v2, z.var)
    assert ops.moments_elu(ops.Moments(m), 0.5).var is None


def device_tail(dev, conv=NormalConv2d, seed=6):
    """The tail alone (no torch trunk in front: the vendor's convs need not repeat their bits from call to call, and these tests
    compare bits across calls; test_example_model_shapes_run_the_moment_route has the trunks)."""
    torch.manual_seed(seed)
    net = Tail(conv=NormalConv2d, trunk=False)
    with torch.no_grad():
        net.layers[0].weight.scale.add_(1.0)                   # sigma ~ 0.13: a variance worth testing
    if conv is not NormalConv2d:
        other = Tail(conv=conv, trunk=False)
        other.load_state_dict(net.state_dict())
        net = other
    assert bnn_nn.moment_activations(net) == 2
    return net.to(dev).eval()


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_network_pass(dev, mode):
    """The MNIST example's tail at B = 4: (4, 64, 6, 6) -> NormalConv2d(64, 64, 3, stride 2, padding 1) -> ELU -> Flatten ->
    NormalLinear(576, 10) -> Softmax.  predictive_moments is the chain of ops calls bit for bit; every
    step is within its bound of float64 applied to the DEVICE's own input of that step (the conv pre-activation against the
    contraction bound, the fused ELU equal to moments_elu of it and that within the ELU bound, the head against K16's bound)."""
    bnn.set_compute(mode)
    net = device_tail(dev)
    x = torch.randn(4, 64, 6, 6, device=dev)
    conv, lin = net.layers[0], net.layers[3]
    keys = [(m.weight.draw_key, m.bias.draw_key) for m in (conv, lin)]
    e0 = _rng.default_generator.epoch_host
    lib = _lib.load()
    h = x
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    mom = net.predictive_moments(x)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 4                    # per Bayesian layer the operand launch + ONE contraction: ELU is fused
    assert _rng.default_generator.epoch_host == e0 and [(m.weight.draw_key, m.bias.draw_key) for m in (conv, lin)] == keys
    assert mom.link == "softmax" and mom.mean.shape == (4, 10) and not mom.mean.requires_grad
    cp = [t.detach() for t in (conv.weight.mean, conv.weight.scale, conv.bias.mean, conv.bias.scale)]
    geo = (conv.stride, conv.padding, conv.dilation, conv.groups)
    pre = ops.moments_convNd(h, *cp, *geo, compute=mode)
    m, v, bm, bv = conv_ref(ops.Moments(h.cpu()), *[t.cpu() for t in cp], geo, mode, dev)
    assert_within(pre.mean, m, bm, "conv m " + mode)
    assert_within(pre.var, v, bv, "conv v " + mode)
    act = ops.moments_convNd(h, *cp, *geo, activation=("elu", 1.0), compute=mode)
    alone = ops.moments_elu(pre, 1.0)
    assert torch.equal(act.mean, alone.mean) and torch.equal(act.var, alone.var)
    dm, dv = elu_deviation(act, pre.mean.cpu(), pre.var.cpu(), 1.0)
    print("network ELU %s: %.3e s, %.3e v" % (mode, dm, dv))
    assert dm <= ELU_MEAN_TOL and dv <= ELU_VAR_TOL, (dm, dv)
    flat = act.view(act.size(0), -1)
    lp = [t.detach() for t in (lin.weight.mean, lin.weight.scale, lin.bias.mean, lin.bias.scale)]
    logits = ops.moments_linear(flat, *lp, compute=mode)
    m, v, bm, bv = linear_ref(ops.Moments(flat.mean.cpu(), flat.var.cpu()), *[t.cpu() for t in lp], mode, dev)
    assert_within(logits.mean, m, bm, "head m " + mode)
    assert_within(logits.var, v, bv, "head v " + mode)
    assert torch.equal(logits.mean, mom.mean) and torch.equal(logits.var, mom.var)
    # LocalReparamConv2d is the same moment layer and records no noise
    lrt = device_tail(dev, bnn_nn.LocalReparamConv2d)
    got = lrt.predictive_moments(x)
    assert torch.equal(got.mean, mom.mean) and torch.equal(got.var, mom.var) and lrt.layers[0].noise_key is None
    _lib.check_device(dev)


@gpu
def test_tails_apply_the_softmax_link(dev):
    net = device_tail(dev)
    x = torch.randn(4, 64, 6, 6, device=dev)
    lib = _lib.load()
    net.predictive_uncertainty(x, samples=2, inputs="probs", propagation="moments")        # takes the model's stream id
    e0 = _rng.default_generator.epoch_host
    mom = net.predictive_moments(x)
    assert _rng.default_generator.epoch_host == e0             # the layers consume no draw epoch
    for S in (2, 16):
        bnn.manual_seed(100)
        u = net.predictive_uncertainty(x, samples=S, sample0=1, inputs="probs", propagation="moments")
        key = net.moment_key
        assert (key.stream, key.sample0, key.nsamples) == (net._moment_stream, 1, S)
        want = ops.mc_uncertainty(torch.softmax(ops.moments_sample(mom, key, S), -1), "probs")
        assert all(torch.equal(a, b) for a, b in zip(u, want))
        assert (u.mean.sum(-1) - 1).abs().max() <= 1e-5 and torch.isfinite(u.total).all()
    _lib.check_device(dev)


@gpu
def test_agreement_with_weight_sampling_is_reported(dev):
    """What the pass keeps and what it drops.  Per conv output element the marginal mean and variance are exact for a
    deterministic input: 2048 device weight draws of the conv layer agree within 6 standard errors.  The positions of an output
    map share weights and the pass drops that correlation, so the LOGIT variance is approximate: its ratio to the sampled one is
    printed, not asserted."""
    torch.manual_seed(8)
    net = device_tail(dev)
    x = torch.randn(2, 64, 6, 6, device=dev)
    h, S = x, 2048
    conv = net.layers[0]
    only_conv, to_logits = Seq(torch.nn.Sequential(conv)), Seq(torch.nn.Sequential(*list(net.layers)[:-1]))
    bnn.manual_seed(77)
    with torch.no_grad():
        ys = only_conv.forward_stacked(h, S)
    assert ys.shape == (S, 2, 64, 3, 3)
    pre = ops.moments_convNd(h, *[t.detach() for t in (conv.weight.mean, conv.weight.scale, conv.bias.mean, conv.bias.scale)],
                             conv.stride, conv.padding, conv.dilation, conv.groups)          # (the layer itself would fuse its ELU)
    six_se(ys[:, :, :8].double().cpu(), pre.mean[:, :8].double().cpu(), pre.var[:, :8].double().cpu(),
           "conv output against %d device weight draws" % S)
    bnn.manual_seed(78)
    with torch.no_grad():
        logits = to_logits.forward_stacked(x, S)
    sv = logits.double().var(0).cpu()
    mom = net.predictive_moments(x)
    ratio = mom.var.double().cpu() / sv
    print("logit variance, moments / %d weight draws: ratio %.3f .. %.3f, median %.3f" % (S, ratio.min(), ratio.max(), ratio.median()))


@gpu
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("moved", ["posterior", "input", "all"])
def test_operands_off_16_bytes_give_the_same_bits(dev, moved, which):
    """Every input of bnn_conv3d_moments_forward and bnn_moments_elu is fetched one element per load: moved to an address that is
    aligned to the element only (NaN guards around it), the results are bit-equal to the aligned run."""
    mom, p, geo = case_operands("2d-geo", True)
    mom, p = on(dev, mom), to(dev, *p)
    n = [0]

    def mv(t, role):
        if moved not in (role, "all"):
            return t
        n[0] += 1
        return offset_view(t, (4, 8)[(which + n[0]) % 2])

    def run(put):
        a = ops.Moments(put(mom.mean, "input"), put(mom.var, "input"))
        pre = ops.moments_convNd(a, *[put(t, "posterior") for t in p], *geo)
        act = ops.moments_convNd(a, *[put(t, "posterior") for t in p], *geo, activation=("elu", 1.0), compute="bf16")
        elu = ops.moments_elu(ops.Moments(put(pre.mean, "input"), put(pre.var, "input")), 0.5)
        return [pre.mean, pre.var, act.mean, act.var, elu.mean, elu.var]

    want, got = run(lambda t, role: t), run(mv)
    assert n[0] > 0
    for a, b in zip(got, want):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b)


@gpu
def test_outputs_off_16_bytes_are_refused_by_the_entry(dev):
    """out_m / out_v off the 16-byte boundary: BNN_E_ALIGN from the C entry, nothing written (the ops wrapper allocates its own)."""
    mom, p, geo = case_operands("2d-geo", False)
    a, p = mom.mean.to(dev), to(dev, *p)
    good = ops.moments_convNd(a, *p, *geo)
    s2_w, s2_b = ops._lrt_prepare_raw(p[1], p[3])
    sh, _ = ops._conv3d_shape((6, 6, 1, 9, 7), (10, 3, 1, 3, 2), (1, 2, 1), (0, 1, 0), (1, 1, 2), 2)
    lib = _lib.load()
    for off in (4, 8):
        om, ov = output_view(good.mean.shape, torch.float32, dev, off), output_view(good.mean.shape, torch.float32, dev, 0)
        for first, second in ((om, ov), (ov, om)):
            rc = lib.bnn_conv3d_moments_forward(a.data_ptr(), None, p[0].data_ptr(), s2_w.data_ptr(), p[2].data_ptr(), s2_b.data_ptr(),
                                                first.data_ptr(), second.data_ptr(), ctypes.byref(sh), 0, 0, 1.0, ops.stream_ptr(dev))
            assert rc == _lib.E_ALIGN
        torch.cuda.synchronize()
        assert guards_intact(om) and guards_intact(ov) and bool((om == -12345.0).all()) and bool((ov == -12345.0).all())
    om, ov = output_view(good.mean.shape, torch.float32, dev, 0), output_view(good.mean.shape, torch.float32, dev, 0)
    assert lib.bnn_conv3d_moments_forward(a.data_ptr(), None, p[0].data_ptr(), s2_w.data_ptr(), p[2].data_ptr(), s2_b.data_ptr(),
                                          om.data_ptr(), ov.data_ptr(), ctypes.byref(sh), 0, 0, 1.0, ops.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert guards_intact(om) and guards_intact(ov) and same_bits(om, good.mean) and same_bits(ov, good.var)


@gpu
def test_graph_capture(dev):
    net = device_tail(dev)
    x = torch.randn(4, 64, 6, 6, device=dev)
    bnn.manual_seed(3)
    net.predictive_uncertainty(x, samples=8, inputs="probs", propagation="moments")        # warm up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        u = net.predictive_uncertainty(x, samples=8, inputs="probs", propagation="moments")
    key = net.moment_key
    g.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in u]
    for t in u:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, u))
    want = ops.mc_uncertainty(torch.softmax(ops.moments_sample(net.predictive_moments(x), key, 8), -1), "probs")
    assert all(torch.equal(a, b) for a, b in zip(first, want))
    assert torch.isfinite(u.total).all() and (u.mean.sum(-1) - 1).abs().max() <= 1e-5
    _lib.check_device(dev)


# ================================================================================================ the example models' shapes
def example_model(name):
    """The layer shapes of the MNIST and CIFAR10 example models (CIFAR10 with a NormalLinear head: its MultivariateNormalLinear
    head stays refused): a deterministic trunk, one Bayesian conv, ELU, flatten, the dense tail, softmax."""
    c2, bn, elu = torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.ELU
    if name == "mnist":
        mods = [c2(1, 32, 5, padding=2, stride=2), bn(32), elu(), c2(32, 32, 3, padding=1), elu(), c2(32, 64, 3, stride=2), elu(),
                NormalConv2d(64, 64, 3, padding=1, stride=2), elu(), Flatten(), NormalLinear(576, 10), torch.nn.Softmax(dim=-1)]
        shape = (1, 28, 28)
    else:
        mods = [c2(3, 64, 5, padding=2, stride=2), bn(64), elu(), c2(64, 128, 5, padding=2, stride=2), elu(),
                c2(128, 128, 5, padding=2, stride=2), elu(), c2(128, 128, 3, padding=1), elu(), c2(128, 128, 3, padding=1), elu(),
                NormalConv2d(128, 128, 3, padding=1), elu(), Flatten(), torch.nn.Linear(2048, 128), elu(), NormalLinear(128, 10),
                torch.nn.Softmax(dim=-1)]
        shape = (3, 32, 32)
    return Seq(torch.nn.Sequential(*mods)), shape


def test_rewrite_of_the_cifar10_shape_on_the_cpu():
    """A torch.nn.Linear BEHIND a Bayesian layer is re-classed in place (the trunk's modules keep their types but the ELUs), the
    sampling path keeps its bits, and the moment pass is the hand-written float64 recursion."""
    torch.manual_seed(1)
    seq = torch.nn.Sequential(torch.nn.Linear(6, 6), torch.nn.ELU(), bnn_nn.NormalConv1d(2, 3, 2), torch.nn.ELU(alpha=0.5), torch.nn.Flatten(),
                              torch.nn.Linear(15, 5), torch.nn.ELU(), NormalLinear(5, 4), torch.nn.Softmax(dim=-1))
    net = Seq(seq).eval()
    net.mc_batched = False
    x = torch.randn(3, 2, 6)
    keys0, lin = list(net.state_dict().keys()), seq[5]
    torch.manual_seed(2)
    before = net(x, samples=1)
    assert bnn_nn.moment_activations(net) == 5 and bnn_nn.moment_activations(net) == 0
    assert type(seq[0]) is torch.nn.Linear and type(seq[5]) is bnn_nn.MomentLinear and seq[5] is lin
    assert list(net.state_dict().keys()) == keys0
    torch.manual_seed(2)
    assert torch.equal(net(x, samples=1), before)
    mom = net.predictive_moments(x)
    c, head = seq[2], seq[7]
    h = seq[1](seq[0](x))
    r = ops.moments_convNd_f64(h.detach(), c.weight.mean, c.weight.scale, c.bias.mean, c.bias.scale, c.stride, c.padding, c.dilation, 1)
    r = ops.moments_elu_f64(r, 0.5).flatten(1)
    w, b = lin.weight.detach().double(), lin.bias.detach().double()
    r = ops.moments_elu_f64(ops.Moments(r.mean @ w.t() + b, r.var @ (w * w).t()), 1.0)
    r = ops.moments_linear_f64(r, head.weight.mean, head.weight.scale, head.bias.mean, head.bias.scale)
    assert mom.link == "softmax" and torch.equal(mom.mean, r.mean.float()) and torch.equal(mom.var, r.var.float())
    det = ops.moments_affine_f64(torch.randn(3, 15), lin.weight, lin.bias)
    assert det.var is None
    with pytest.raises(ops.BnnHipError, match="link"):
        lin(ops.Moments(torch.randn(3, 15), torch.rand(3, 15), "softmax"))


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
def test_affine_matches_float64(dev, bias, mode):
    """ops.moments_affine (a deterministic Linear behind a Bayesian layer) is bnn_moments_forward with a zero sigma^2 plane: the
    fp32 scaled bound, or in the bf16 mode float64 on the planes a_m, a_v, w, fma(w, w, 0) as rounded, gamma_n sum |a| |b| with
    n = K + 1 for m and 2 K + 1 for v (the zero plane's addends pass through the accumulator too)."""
    g = torch.Generator().manual_seed(5)
    B, N, K = 65, 68, 130
    w, b = (torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5, (torch.rand(N, generator=g) - 0.5 if bias else None)
    am, av = torch.randn(B, K, generator=g), 0.5 * torch.rand(B, K, generator=g) ** 2
    out = ops.moments_affine(ops.Moments(am.to(dev), av.to(dev)), w.to(dev), None if b is None else b.to(dev), compute=mode)
    if mode == "f32":
        ref = ops.moments_affine_f64(ops.Moments(am, av), w, b)
        m, v, bm, bv = ref.mean, ref.var, scaled_bound(ref.mean), scaled_bound(ref.var)
    else:
        p_w, p_e2, q_m, q_v = rne_bf16(w), rne_bf16((w.double() ** 2).float()), rne_bf16(am), rne_bf16(av)
        m, a, v = q_m @ p_w.t(), q_m.abs() @ p_w.abs().t(), q_v @ p_e2.t()
        if bias:
            m, a = m + b.double(), a + b.double().abs()
        bm, bv = gamma(K + 1) * a + 1e-300, gamma(2 * K + 1) * v + 1e-300
    assert_within(out.mean, m, bm, "affine m bias=%s %s" % (bias, mode))
    assert_within(out.var, v, bv, "affine v bias=%s %s" % (bias, mode))
    det = ops.moments_affine(am.to(dev), w.to(dev), None if b is None else b.to(dev), compute=mode)
    assert det.var is None and det.mean.shape == (B, N)


@gpu
@pytest.mark.parametrize("name", ["mnist", "cifar10"])
def test_example_model_shapes_run_the_moment_route(dev, name):
    """The example models' shapes after nn.moment_activations: predictive_uncertainty(inputs='probs', propagation='moments') runs on
    the device, and predictive_moments is the chain of ops calls on the trunk's output, bit for bit."""
    torch.manual_seed(4)
    net, shape = example_model(name)
    assert bnn_nn.moment_activations(net) > 0
    net = net.to(dev).eval()
    seq = net.layers
    x = torch.randn(5, *shape, device=dev)
    bnn.manual_seed(9)
    u = net.predictive_uncertainty(x, samples=16, inputs="probs", propagation="moments")
    assert u.mean.shape == (5, 10) and (u.mean.sum(-1) - 1).abs().max() <= 1e-5
    assert all(torch.isfinite(t).all() for t in u) and (u.total >= 0).all()
    i = [k for k, m in enumerate(seq) if isinstance(m, NormalConv2d)][0]
    c, seen = seq[i], []
    hook = c.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))         # the trunk's output of THIS pass (the
    mom = net.predictive_moments(x)                                                    # vendor convs need not repeat their bits)
    hook.remove()
    h = seen[0]
    post = lambda l: [t.detach() for t in (l.weight.mean, l.weight.scale, l.bias.mean, l.bias.scale)]         # noqa: E731
    r = ops.moments_convNd(h, *post(c), c.stride, c.padding, c.dilation, c.groups, activation=("elu", 1.0)).flatten(1)
    if name == "cifar10":
        r = ops.moments_elu(ops.moments_affine(r, seq[i + 3].weight, seq[i + 3].bias), 1.0)
    r = ops.moments_linear(r, *post(seq[-2]))
    assert mom.link == "softmax" and torch.equal(mom.mean, r.mean) and torch.equal(mom.var, r.var)
    assert (mom.var > 0).all()
    _lib.check_device(dev)
