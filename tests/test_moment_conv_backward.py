"""Training conv nets without sampling (K19): the backward of K17's contraction (csrc/bnn_conv3d.hip, k_moments_conv3d_bwd)

    g_a_m  = convT(G_m, mu_w) + 2 a_m (.) convT(G_v, sigma_w^2)          g_a_v  = convT(G_v, mu_w^2 + sigma_w^2)
    g_mu_w = sum gather(a_m) G_m + 2 mu_w (.) sum gather(a_v) G_v         g_s2_w = sum gather(a_m^2 + a_v) G_v,
    g_rho_w = g_s2_w 2 sigma_w sigmoid(rho_w)

of the moment-matched ELU (bnn_moments_elu_backward) and of ops.moments_affine, and BayesianNetworkModule.forward_moments through
conv layers behind the nn.conv_moment_training switch.  CPU tests: the ELU's analytic backward against float64 autograd, gradcheck
of the float64 recursion, the gate, the argument checks, the built code object, a training run.  GPU tests: every kernel against
float64, K11's bits for a deterministic input, the networks end to end, alignment, graph capture, training.

Bounds.  Contractions, fp32 mode: 1e-5 of the output scale (test_lrt_device.scaled_bound) against float64 autograd of
ops.moments_convNd_f64(track=True).  bf16 mode: float64 on the planes as the kernel rounds them (RNE; the derived plane
fma(p1, p1, p2) in fp32 first), so the device differs by its fp32 accumulation alone: gamma_n sum |a| |b| per element with n the
addends the element's accumulators see plus the epilogue fma -- 2 R + 2 for g_a_m, R + 1 for g_a_v with R = (O / groups) x taps;
2 R' + 2 for g_mu_w, R' + 1 for g_s2_w with R' = B x P (the slab sums are part of the same chain) -- and 16 U for the rho chain
factor, as in test_moment_backward.py.  The bias sums read the fp32 G_m / G_v: gamma_R' sum |G|.
ELU backward: ELU_BWD_M_TOL / ELU_BWD_V_TOL below.
"""
import ctypes
import math
import re

import pytest
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _rng, ops
from bayesianneuralnetworks_amd import nn as bnn_nn
from bayesianneuralnetworks_amd.nn import (BayesianNetworkModule, KLDivergence, MultivariateNormalLinear, NormalConv1d, NormalConv2d,
                                           NormalLinear)
from bayesianneuralnetworks_amd._rng import DrawKey

from alignment import guards_intact, offset_view, output_view, same_bits
from bf16ref import gamma, rne_bf16
from test_flipout_mc import _code_object_notes
from test_lrt_device import U, assert_within, scaled_bound, sigma64
from test_moment_backward import recovered_eps
from test_moment_conv import CASES, conv_input, conv_params, convnd

gpu = pytest.mark.gpu

# The backward of the moment-matched ELU against float64 (ops.moments_elu_backward_f64 on the fp32 inputs), g_m in units of
# |g_mean'| + s |g_var'| and g_v in units of |g_mean'| / s + |g_var'| (s = sqrt(v); K18's units).  Measured on the MI355X over
# alpha in [-12, 12] (4801 points) at v = 1e-6, 0.3, 1, 47 for a = 1 and a = 0.5 (test_elu_backward_matches_float64_on_a_grid
# prints them): worst g_m deviation 5.784e-8 (a = 1, v = 1e-6), worst g_v deviation 5.376e-8 (a = 0.5, v = 47); per (a, v),
# g_m / g_v: a = 1: 5.78e-8 / 1.73e-8, 5.08e-8 / 5.26e-8, 4.68e-8 / 4.92e-8, 4.62e-8 / 5.10e-8; a = 0.5: 5.61e-8 / 5.99e-9,
# 4.94e-8 / 4.84e-8, 4.59e-8 / 4.81e-8, 4.54e-8 / 5.38e-8.  The device function works in fp64, so what is measured is the fp32
# rounding of its two results (2^-24 = 6e-8 of a result that the unit bounds).  The constants are 4 x the measured worst, the
# margin of ELU_*_TOL; both are below 1e-5.
ELU_BWD_M_TOL = 2.32e-7
ELU_BWD_V_TOL = 2.16e-7

GRID_V = (1e-6, 0.3, 1.0, 47.0)
GRID_A = (1.0, 0.5)

ALL_CASES = dict(CASES)
ALL_CASES["c70"] = ((2, 70, 5, 5), 8, (3, 3), (1, 1), (1, 1), (1, 1), 1, True)        # C / groups = 70: the input gradient's N edge


@pytest.fixture
def switch():
    """nn.conv_moment_training on for one test, restored afterwards."""
    was = bnn_nn.conv_moment_training_enabled()
    bnn_nn.conv_moment_training(True)
    yield
    bnn_nn.conv_moment_training(was)


def elu_grid(v, a, n=4801):
    alpha = torch.linspace(-12, 12, n, dtype=torch.float64)
    m32, v32 = (alpha * math.sqrt(v)).float(), torch.full_like(alpha, v).float()
    g = torch.Generator().manual_seed(int(v * 1000) + int(a * 10) + 5)
    return m32, v32, torch.randn(n, generator=g), torch.randn(n, generator=g)


# ================================================================================================ CPU
def test_elu_backward_formula_is_the_autograd_of_the_forward():
    worst = 0.0
    for a in GRID_A:
        for v in GRID_V:
            m32, v32, gm, gv = elu_grid(v, a)
            m, vv = m32.double().requires_grad_(), v32.double().requires_grad_()
            out = ops.moments_elu_f64(ops.Moments(m, vv), a, track=True)
            assert out.mean.requires_grad and out.var.requires_grad
            plain = ops.moments_elu_f64(ops.Moments(m, vv), a)
            assert not plain.mean.requires_grad and torch.equal(plain.mean, out.mean.detach()) and torch.equal(plain.var, out.var.detach())
            want = torch.autograd.grad([out.mean, out.var], [m, vv], [gm.double(), gv.double()])
            got = ops.moments_elu_backward_f64(ops.Moments(m32, v32), gm, gv, a)
            s = math.sqrt(v)
            dm = ((got[0] - want[0]).abs() / (gm.abs() + s * gv.abs())).max().item()
            dv = ((got[1] - want[1]).abs() / (gm.abs() / s + gv.abs())).max().item()
            print("moments_elu_backward_f64 a = %g v = %g: against autograd %.2e, %.2e" % (a, v, dm, dv))
            worst = max(worst, dm, dv)
            assert dm <= 1e-8 and dv <= 1e-8, (a, v, dm, dv)
            assert not got[0].requires_grad
    print("moments_elu_backward_f64: worst deviation from autograd %.2e" % worst)
    # a = 0 is the ReLU's backward
    m32, v32, gm, gv = elu_grid(0.3, 1.0)
    r = ops.moments_relu_backward_f64(ops.Moments(m32, v32), gm, gv)
    e = ops.moments_elu_backward_f64(ops.Moments(m32, v32), gm, gv, 0.0)
    assert (r[0] - e[0]).abs().max() <= 1e-13 and (r[1] - e[1]).abs().max() <= 1e-12
    # v == 0: the limits, m == 0 on the positive side (the formula, and the tracked forward's autograd)
    for a in GRID_A:
        m0, v0 = torch.tensor([-2.0, 0.0, 3.0], dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
        gm, gv = torch.tensor([1.5, -2.0, 0.5], dtype=torch.float64), torch.tensor([4.0, 3.0, -7.0], dtype=torch.float64)
        d = a * math.exp(-2.0)
        g_m, g_v = ops.moments_elu_backward_f64(ops.Moments(m0, v0), gm, gv, a)
        assert torch.allclose(g_m, torch.tensor([1.5 * d, -2.0, 0.5], dtype=torch.float64), rtol=1e-15, atol=0)
        assert torch.allclose(g_v, torch.tensor([4.0 * d * d + 1.5 * 0.5 * d, 3.0, -7.0], dtype=torch.float64), rtol=1e-15, atol=0)
        m, vv = m0.clone().requires_grad_(), v0.clone().requires_grad_()
        out = ops.moments_elu_f64(ops.Moments(m, vv), a, track=True)
        assert torch.allclose(out.mean.detach(), F.elu(m0, a), rtol=1e-15, atol=0) and not out.var.detach().any()
        a_m, a_v = torch.autograd.grad([out.mean, out.var], [m, vv], [gm, gv])
        assert torch.allclose(a_m, g_m, rtol=1e-15, atol=0) and torch.allclose(a_v, g_v, rtol=1e-15, atol=0)
    # where the forward clamped var' to 0 the g_var' terms are absent.  At a = 0 the forward's sum is the ReLU's v r, and far in the
    # lower tail (Phi and phi subnormal in float64) the bracket r rounds below 0 at thousands of these points
    al = torch.linspace(-38.8, -37.9, 9001, dtype=torch.float64)
    one = torch.ones_like(al)
    fwd = ops.moments_elu_f64(ops.Moments(al, one), 0.0)
    clamped = ops._elu_terms_f64(al, one)[-1] < 0
    assert clamped.any() and not fwd.var[clamped].any()
    g_m, g_v = ops.moments_elu_backward_f64(ops.Moments(al, one), torch.zeros_like(al), one, 0.0)
    assert not g_m[clamped].any() and not g_v[clamped].any()
    # a deterministic input is plain ELU
    g_m, g_v = ops.moments_elu_backward_f64(ops.Moments(torch.tensor([-1.0, 0.0, 2.0])), torch.tensor([3.0, 5.0, 4.0]), None, 0.5)
    assert g_v is None and torch.allclose(g_m, torch.tensor([3.0 * 0.5 * math.exp(-1.0), 5.0, 4.0], dtype=torch.float64), rtol=1e-15, atol=0)


GRADCHECK = [  # (input shape, O, kernel, stride, padding, dilation, groups)
    ((2, 4, 7), 4, (3,), (2,), (1,), (1,), 2),
    ((2, 2, 5, 4), 3, (2, 3), (1, 2), (1, 0), (2, 1), 1),
    ((2, 4, 4, 5), 6, (3, 2), (1, 1), (1, 1), (1, 1), 2),
]


@pytest.mark.parametrize("act", [None, "relu", ("elu", 1.0), ("elu", 0.5)], ids=["none", "relu", "elu1", "elu.5"])
@pytest.mark.parametrize("with_var", [False, True])
@pytest.mark.parametrize("case", range(len(GRADCHECK)))
def test_conv_recursion_gradcheck(case, with_var, act):
    xs, O, kernel, stride, padding, dilation, groups = GRADCHECK[case]
    g = torch.Generator().manual_seed(20 + case)
    p = [t.double().requires_grad_() for t in conv_params(O, xs[1] // groups, kernel, True, 21 + case, rho0=-1.5)]
    am = torch.randn(*xs, generator=g, dtype=torch.float64).requires_grad_()
    av = (0.05 + 0.5 * torch.rand(*xs, generator=g, dtype=torch.float64)).requires_grad_() if with_var else None
    probe = ops.moments_convNd_f64(ops.Moments(am, av), *p, stride, padding, dilation, groups, activation=act, track=True)
    c1, c2 = torch.randn(probe.mean.shape, generator=g, dtype=torch.float64), torch.randn(probe.mean.shape, generator=g, dtype=torch.float64)

    def f(am, *rest):
        av_, ps = (rest[0], rest[1:]) if with_var else (None, rest)
        out = ops.moments_convNd_f64(ops.Moments(am, av_), *ps, stride, padding, dilation, groups, activation=act, track=True)
        assert out.mean.requires_grad and out.var.requires_grad and out.mean.dtype == torch.float64
        return (c1 * out.mean + c2 * out.var).sum()

    inputs = (am,) + ((av,) if with_var else ()) + tuple(p)
    assert torch.autograd.gradcheck(f, inputs, eps=1e-6, atol=1e-7, rtol=1e-5)
    plain = ops.moments_convNd_f64(ops.Moments(am, av), *p, stride, padding, dilation, groups, activation=act)
    assert not plain.mean.requires_grad and torch.equal(plain.mean, probe.mean.detach()) and torch.equal(plain.var, probe.var.detach())


def test_affine_recursion_gradcheck():
    g = torch.Generator().manual_seed(30)
    am = torch.randn(4, 6, generator=g, dtype=torch.float64).requires_grad_()
    av = (0.1 + torch.rand(4, 6, generator=g, dtype=torch.float64)).requires_grad_()
    w = torch.randn(3, 6, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(3, generator=g, dtype=torch.float64).requires_grad_()
    c1, c2 = torch.randn(4, 3, generator=g, dtype=torch.float64), torch.randn(4, 3, generator=g, dtype=torch.float64)

    def f(am, av, w, b):
        out = ops.moments_affine_f64(ops.Moments(am, av), w, b, track=True)
        return (c1 * out.mean + c2 * out.var).sum()

    assert torch.autograd.gradcheck(f, (am, av, w, b), eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda am, w: ops.moments_affine_f64(am, w, None, track=True).mean.sum(), (am, w), eps=1e-6, atol=1e-7)
    assert not ops.moments_affine_f64(ops.Moments(am, av), w, b).var.requires_grad
    with torch.no_grad():
        assert not ops.moments_affine_f64(ops.Moments(am, av), w, b, track=True).var.requires_grad


class ConvNet(BayesianNetworkModule):
    """front -> ELU -> NormalConv2d(4, 6, 3, stride 2, padding 1) -> ELU -> flatten -> NormalLinear [-> Linear] -> softmax on
    (B, 1, 10, 10) images; front: a deterministic Conv2d(1, 4, 3) or a NormalConv2d of that shape."""

    def __init__(self, bayes_front, linear_tail=False, classes=5, conv=NormalConv2d):
        super().__init__(1, classes, samples=8)
        front = (conv if bayes_front else torch.nn.Conv2d)(1, 4, 3)
        tail = [NormalLinear(96, 7), torch.nn.Linear(7, classes)] if linear_tail else [NormalLinear(96, classes)]
        self.layers = torch.nn.Sequential(front, torch.nn.ELU(), conv(4, 6, 3, stride=2, padding=1), torch.nn.ELU(), torch.nn.Flatten(),
                                          *tail, torch.nn.Softmax(dim=-1))
        bnn_nn.moment_activations(self)

    def _forward(self, x):
        return self.layers(x)


def set_posteriors(net, seed, rho0=-2.5):
    """Posteriors with variances of a healthy size (every logit's standard deviation within a few orders of its mean)."""
    with torch.no_grad():
        for i, m in enumerate(net.modules()):
            if isinstance(m, bnn_nn.BayesianModule):
                g = torch.Generator().manual_seed(seed + i)
                K = m.weight.mean[0].numel()
                m.weight.mean.copy_((torch.rand(m.weight.mean.shape, generator=g) * 2 - 1) / K ** 0.5)
                m.weight.scale.copy_(rho0 + 0.3 * torch.randn(m.weight.scale.shape, generator=g))
                m.bias.mean.copy_((torch.rand(m.bias.mean.shape, generator=g) * 2 - 1) / K ** 0.5)
                m.bias.scale.copy_(rho0 + 0.3 * torch.randn(m.bias.scale.shape, generator=g))
    return net


class Wrap(BayesianNetworkModule):
    """A container around given modules."""

    def __init__(self, *mods):
        super().__init__(0, 0, samples=1)
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


def test_forward_moments_gate():
    torch.manual_seed(1)
    net = set_posteriors(ConvNet(False, linear_tail=True), 3)
    assert [type(m).__name__ for m in net.layers] == ["Conv2d", "MomentELU", "NormalConv2d", "MomentELU", "Flatten", "NormalLinear",
                                                      "MomentLinear", "MomentSoftmax"]
    x = torch.randn(3, 1, 10, 10)
    assert not bnn_nn.conv_moment_training_enabled()
    # off: today's refusals, with today's messages
    with pytest.raises(ops.BnnHipError, match="has no moment backward"):
        net.forward_moments(x)
    dense = Wrap(net.layers[2])
    with pytest.raises(ops.BnnHipError, match="forward_moments: NormalConv2d has no moment backward; training without sampling supports "
                                              "NormalLinear / LocalReparamLinear, ReLU \\(folded, or nn.MomentReLU\\), reshaping modules, "
                                              "torch.nn.Identity and a closing nn.MomentSoftmax$"):
        dense.forward_moments(torch.randn(3, 4, 8, 8))
    dense = Wrap(*list(net.layers)[4:])
    with pytest.raises(ops.BnnHipError, match="MomentLinear has no moment backward"):
        dense.forward_moments(torch.randn(3, 96))
    dense = Wrap(net.layers[5], bnn_nn.MomentELU())
    with pytest.raises(ops.BnnHipError, match="MomentELU has no moment backward"):
        dense.forward_moments(torch.randn(3, 96))
    bnn_nn.conv_moment_training(True)
    try:
        assert bnn_nn.conv_moment_training_enabled()
        mom = net.forward_moments(x)
        assert mom.link == 'softmax' and mom.mean.shape == (3, 5) and mom.mean.requires_grad and mom.var.requires_grad
        ref = net.predictive_moments(x)
        assert torch.equal(mom.mean.float(), ref.mean) and torch.equal(mom.var.float(), ref.var) and not ref.mean.requires_grad
        ps = net.sample_moments(mom)
        assert ps.shape == (8, 3, 5) and ps.requires_grad and not hasattr(net, "moment_key")
        t = torch.tensor([0, 2, 1]).repeat(8)
        params = list(net.parameters())
        grads = torch.autograd.grad(F.nll_loss(torch.log(ps.reshape(-1, 5)), t), params)
        assert len(grads) == 2 + 4 + 4 + 2 and all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads)
        with torch.no_grad():
            assert not net.forward_moments(x).mean.requires_grad
        # what stays refused
        for bad, kw in ((bnn_nn.FlipOutNormalConv2d, {}), (bnn_nn.MCDropoutConv2d, {"drop_prob": 0.1})):
            other = ConvNet(True, conv=lambda *a, **k: bad(*a, **k, **kw))
            with pytest.raises(ops.BnnHipError, match=bad.__name__ + " has no moment backward"):
                other.forward_moments(x)
        mvn = Wrap(*list(net.layers)[:5], MultivariateNormalLinear(96, 7))
        with pytest.raises(ops.BnnHipError, match="MultivariateNormalLinear"):
            mvn.forward_moments(x)
        # untracked calls stay detached under enable_grad
        c = net.layers[2]
        xr = torch.randn(3, 4, 8, 8, requires_grad=True)
        args = (c.weight.mean, c.weight.scale, c.bias.mean, c.bias.scale, c.stride, c.padding, c.dilation, c.groups)
        with torch.enable_grad():
            out = ops.moments_convNd_f64(xr, *args, activation=("elu", 1.0))
            assert not out.mean.requires_grad and not out.var.requires_grad
            act = ops.moments_elu_f64(ops.Moments(xr, xr * xr))
            assert not act.mean.requires_grad and not act.var.requires_grad
            aff = ops.moments_affine_f64(ops.Moments(xr.flatten(1)[:, :7], xr.flatten(1)[:, :7] ** 2), net.layers[6].weight, net.layers[6].bias)
            assert not aff.mean.requires_grad and not aff.var.requires_grad
            assert ops.moments_convNd_f64(xr, *args, activation=("elu", 1.0), track=True).var.requires_grad
        with torch.no_grad():
            assert not ops.moments_convNd_f64(xr, *args, track=True).mean.requires_grad
    finally:
        bnn_nn.conv_moment_training(False)
    assert not bnn_nn.conv_moment_training_enabled()
    with pytest.raises(ops.BnnHipError, match="has no moment backward"):
        net.forward_moments(x)


def conv3d_shape(xs, O, kernel, stride, padding, dilation, groups):
    img, w5, st, pd, dl = ops._lrt_conv_views(xs, (O, xs[1] // groups) + tuple(kernel), stride, padding, dilation)
    sh, _ = ops._conv3d_shape((xs[0],) + img, w5, st, pd, dl, groups)
    return sh


def test_conv_backward_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one, odd, off8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(72)
    F32, BF16 = _lib.COMPUTE_F32, _lib.COMPUTE_BF16
    big = 1 << 40

    def shape(B=2, C=4, D=1, H=6, W=6, O=4, k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1), d=(1, 1, 1), groups=1):
        return _lib.Conv3dShape(B, C, D, H, W, O, *k, *s, *p, *d, groups)

    def ref(sh):
        return None if isinstance(sh, str) else ctypes.byref(sh)

    def inp(g_m=one, g_v=one, mu_w=one, s2_w=one, a_m=one, g_a_m=one, g_a_v=one, sh=None, compute=F32):
        sh = shape() if sh is None else sh
        rc = lib.bnn_conv3d_moments_backward_input(g_m, g_v, mu_w, s2_w, a_m, g_a_m, g_a_v, ref(sh), compute, None)
        if rc:
            assert lib.bnn_last_error().startswith(b"bnn_conv3d_moments_backward_input: "), lib.bnn_last_error()
        return rc

    def wgt(a_m=one, a_v=one, g_m=one, g_v=one, mu_w=one, rho_w=one, g_mu_w=one, g_rho_w=one, rho_b=None, g_mu_b=None, g_rho_b=None,
            sh=None, compute=F32, ws=one, nbytes=big):
        sh = shape() if sh is None else sh
        rc = lib.bnn_conv3d_moments_backward_weight(a_m, a_v, g_m, g_v, mu_w, rho_w, g_mu_w, g_rho_w, rho_b, g_mu_b, g_rho_b, ref(sh),
                                                    compute, ws, nbytes, None)
        if rc:
            assert lib.bnn_last_error().startswith(b"bnn_conv3d_moments_backward_weight: "), lib.bnn_last_error()
        return rc

    # NULL operands; a missing variance side names K11's entry
    for name in ("g_m", "g_v", "mu_w", "s2_w", "a_m", "g_a_m"):
        assert inp(**{name: None}) == -1, name
    assert inp(g_a_v=None) == -1 and b"bnn_conv3d_lrt_backward_input" in lib.bnn_last_error()
    assert inp(sh="null") == -1
    for name in ("a_m", "g_m", "g_v", "mu_w", "rho_w", "g_mu_w", "g_rho_w"):
        assert wgt(**{name: None}) == -1, name
    assert wgt(a_v=None) == -1 and b"bnn_conv3d_lrt_backward_weight" in lib.bnn_last_error()
    assert wgt(sh="null") == -1
    # a partial bias
    assert wgt(rho_b=one) == -1 and wgt(rho_b=one, g_mu_b=one) == -1 and wgt(g_mu_b=one, g_rho_b=one) == -1
    # conv3d_geo's extents and ranges
    for f in (inp, wgt):
        assert f(sh=shape(C=0)) == -2 and f(sh=shape(s=(1, 0, 1))) == -2 and f(sh=shape(p=(0, -1, 1))) == -2 and f(sh=shape(B=-1)) == -2
        assert f(sh=shape(H=2, W=2, k=(1, 5, 5), p=(0, 0, 0))) == -2
        assert f(sh=shape(C=4, O=4, groups=3)) == -2
        assert f(sh=shape(B=1, C=1, H=65536, W=65536, O=1)) == -5 and b"2^31" in lib.bnn_last_error()
        assert f(sh=shape(B=1 << 20, C=1, H=64, W=64, O=1)) == -5
        assert f(sh=shape(B=1, C=64 * 65535 + 64, H=1, W=1, O=1, k=(1, 1, 1), p=(0, 0, 0))) == -5
        assert f(sh=shape(B=1, C=1, H=1, W=1, O=64 * 65535 + 64, k=(1, 1, 1), p=(0, 0, 0))) == -5
        # the compute mode
        assert f(compute=7) == -3 and f(compute=-1) == -3
    sh = shape()
    assert lib.bnn_conv3d_moments_wgrad_workspace(None) == -1 and lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(shape(C=0))) == -1
    need = lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(sh))
    assert need > 0 and need % (3 * 4 * 4 * 36) == 0           # whole [3][O][K] slabs
    # the workspace
    assert wgt(ws=None) == -6 and wgt(nbytes=need - 1) == -6 and b"bnn_conv3d_moments_wgrad_workspace" in lib.bnn_last_error()
    assert wgt(nbytes=0, sh=shape(B=0)) == -6
    # alignment: inputs on the element, 16 bytes for the contraction outputs
    for name in ("g_m", "g_v", "mu_w", "s2_w", "a_m"):
        assert inp(**{name: odd}) == -4, name
    assert inp(g_a_m=off8) == -4 and inp(g_a_v=off8) == -4 and inp(g_a_v=ctypes.c_void_p(68), compute=BF16) == -4
    assert b"16 bytes" in lib.bnn_last_error()
    for name in ("a_m", "a_v", "g_m", "g_v", "mu_w", "rho_w"):
        assert wgt(**{name: odd}) == -4, name
    assert wgt(g_mu_w=off8) == -4 and wgt(g_rho_w=off8) == -4 and b"16 bytes" in lib.bnn_last_error()
    assert wgt(rho_b=odd, g_mu_b=one, g_rho_b=one) == -4 and wgt(rho_b=one, g_mu_b=one, g_rho_b=odd) == -4 and wgt(ws=odd) == -4
    # no images: the input gradient has nothing to do -- after every check
    assert inp(sh=shape(B=0)) == 0 and inp(sh=shape(B=0), compute=BF16, g_m=off8, g_v=off8, mu_w=off8, s2_w=off8, a_m=off8) == 0
    assert inp(sh=shape(B=0), g_a_m=off8) == -4 and inp(sh=shape(B=0, C=0)) == -2 and inp(sh=shape(B=0), compute=9) == -3

    eb = lib.bnn_moments_elu_backward
    for i in range(6):
        a = [one] * 6
        a[i] = None
        assert eb(*a, 4, 1.0, None) == -1, i
    assert eb(one, one, one, one, one, one, -1, 1.0, None) == -2
    assert eb(one, one, one, one, one, one, 4, -0.5, None) == -5 and eb(one, one, one, one, one, one, 4, float("inf"), None) == -5
    assert eb(one, one, one, one, one, one, 4, float("nan"), None) == -5
    assert lib.bnn_last_error().startswith(b"bnn_moments_elu_backward: ")
    for i in range(6):
        a = [one] * 6
        a[i] = odd
        assert eb(*a, 4, 1.0, None) == -4, i
    assert eb(off8, off8, off8, off8, off8, off8, 0, 1.0, None) == 0
    assert lib.bnn_launch_count() == n0


def test_conv_moment_backward_kernels_do_not_spill():
    """The four instantiations of the three-accumulator conv tile (input, weight gradient x bf16, fp32) keep their 96 accumulator
    registers and the staged operands in registers; the ELU's backward and the slab reduce use no scratch either.  The names K11
    and K17 are known by stay what they were."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    tiles = {n: f for n, f in kernels.items()
             if re.match(r"_ZN3bnn20k_moments_conv3d_bwdI[tf]Li[12]EEEvNS_9Conv3dGeoENS_14MomConvBwdArgsE$", n)}
    assert len(tiles) == 4, sorted(kernels)
    elu = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn17k_moments_elu_bwdE", n)}
    wsum = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn19k_moments_conv_wsumE", n)}
    assert len(elu) == 1 and len(wsum) == 1, sorted(kernels)
    for n, f in {**tiles, **elu, **wsum}.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0 and \
            int(f.get("private_segment_fixed_size", 0)) == 0, (n, f)
    lds = sorted(int(f["group_segment_fixed_size"]) for f in tiles.values())
    # bf16 (80-B rows): 2 + 3 planes of 128 / 64 rows (input gradient), 3 + 2 (weight gradient); fp32 (144-B rows): K11's 2 + 2
    assert lds == [35840, 40960, 55296, 55296], lds
    assert len([n for n in kernels if re.match(r"_ZN3bnn12k_lrt_conv3dI[tf]Li[012]EEEvNS_9Conv3dGeoENS_11LrtConvArgsE$", n)]) == 6
    assert len([n for n in kernels if re.match(r"_ZN3bnn16k_moments_conv3dI[tf]Lb[01]EEEvNS_9Conv3dGeoENS_11MomConvArgsE$", n)]) == 4
    assert any(re.match(r"_ZN3bnn8k_conv3dIfLi0ELb0EEEvNS_9Conv3dGeoENS_10Conv3dArgsE$", n) for n in kernels), sorted(kernels)


class Conv1dNet(BayesianNetworkModule):
    """x (B, 1, 16) -> NormalConv1d(1, 8, 3, padding 1) -> ELU -> NormalConv1d(8, 4, 3, stride 2, padding 1) -> ELU -> flatten ->
    NormalLinear(32, 1): a fully Bayesian CNN."""

    def __init__(self):
        super().__init__(1, 1, samples=1)
        self.layers = torch.nn.Sequential(NormalConv1d(1, 8, 3, padding=1), torch.nn.ELU(), NormalConv1d(8, 4, 3, stride=2, padding=1),
                                          torch.nn.ELU(), torch.nn.Flatten(), NormalLinear(32, 1))
        bnn_nn.moment_activations(self)

    def _forward(self, x):
        return self.layers(x)


def toy_conv_regression(device, steps=200):
    """y = tanh(sum of the first half - sum of the second half) of x (64, 1, 16); Adam (lr 1e-2) on
    mean(((y - m)^2 + v) / (2 0.3^2)) + KL / B, the expected Gaussian negative log-likelihood under the propagated moments -- no
    sample anywhere.  -> (net, [loss per step])"""
    torch.manual_seed(14)
    net = Conv1dNet()
    g = torch.Generator().manual_seed(15)
    x = torch.randn(64, 1, 16, generator=g)
    y = torch.tanh(x[:, 0, :8].sum(1) - x[:, 0, 8:].sum(1)).unsqueeze(1)
    net, x, y = net.to(device), x.to(device), y.to(device)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    kl = KLDivergence(1)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        mom = net.forward_moments(x)
        loss = (((y - mom.mean) ** 2 + mom.var) / (2 * 0.3 ** 2)).mean() + kl(net) / 64
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return net, losses


def test_conv_training_without_sampling_cpu(switch):
    """The method's own curve (the float64 recursion under torch autograd).  Measured: 6.49 -> 0.495, a ratio of 0.076 -- below the
    quarter that lets the device test keep "one half" (the device: 0.076 in both modes)."""
    net, losses = toy_conv_regression("cpu")
    print("toy conv regression, CPU float64 path: loss %.4f -> %.4f (ratio %.3f)" % (losses[0], losses[-1], losses[-1] / losses[0]))
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < 0.25 * losses[0]
    assert losses[-1] < 0.5 * losses[0]
    assert not hasattr(net, "moment_key")


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


_case_cache = {}


def backward_case(name, bias):
    """CPU operands of one case: (a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b, geo); a_v with exact zeros, G of both signs."""
    key = (name, bias)
    if key not in _case_cache:
        _case_cache[key] = backward_operands(ALL_CASES[name], bias)
    return _case_cache[key]


def backward_operands(spec, bias):
    """backward_case's operands for a geometry given as CASES' tuple (input shape, O, kernel, stride, padding, dilation, groups,
    has a bias)."""
    xs, O, kernel, stride, padding, dilation, groups, has_bias = spec
    mu_w, rho_w, _, rho_b = conv_params(O, xs[1] // groups, kernel, bias and has_bias, 11)
    mom = conv_input(xs, True, 12)
    a_v = mom.var.clone()
    a_v[a_v < 0.02] = 0.0                                  # a fifth of the variances are exact zeros
    a_v[0, 0] = 0.0                                         # and one whole channel of one image
    geo = (stride, padding, dilation, groups)
    out = convnd(len(kernel))(mom.mean, mu_w, None, *geo)
    g = torch.Generator().manual_seed(13)
    G_m, G_v = torch.randn(out.shape, generator=g), torch.randn(out.shape, generator=g)
    return (mom.mean, a_v, G_m, G_v, mu_w, rho_w, rho_b, geo)


def backward_device(dev, mode, a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b, geo, ws_off=0):
    """The two entries called as they are -> [g_a_m, g_a_v, g_mu_w, g_rho_w (, g_mu_b, g_rho_b)] and the device's fp32 sigma_w^2."""
    lib, p, st = _lib.load(), ops.ptr, ops.stream_ptr(dev)
    code = ops._compute_code(mode)
    sh = conv3d_shape(tuple(a_m.shape), mu_w.shape[0], tuple(mu_w.shape[2:]), *geo)
    s2_w, _ = ops._lrt_prepare_raw(rho_w.contiguous(), None)
    g_am, g_av = torch.empty(a_m.shape, device=dev), torch.empty(a_m.shape, device=dev)
    g_mu, g_rho = torch.empty(mu_w.shape, device=dev), torch.empty(mu_w.shape, device=dev)
    g_mb = None if rho_b is None else torch.empty(rho_b.shape, device=dev)
    g_rb = None if rho_b is None else torch.empty(rho_b.shape, device=dev)
    nb = lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(sh))
    assert nb > 0
    ws = torch.empty(nb // 4 + 4, device=dev)[ws_off:]
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    ops.check(lib.bnn_conv3d_moments_backward_input(p(G_m), p(G_v), p(mu_w), p(s2_w), p(a_m), p(g_am), p(g_av), ctypes.byref(sh), code, st),
              "bnn_conv3d_moments_backward_input")
    assert lib.bnn_launch_count() == n0 + 1
    ops.check(lib.bnn_conv3d_moments_backward_weight(p(a_m), p(a_v), p(G_m), p(G_v), p(mu_w), p(rho_w), p(g_mu), p(g_rho), p(rho_b), p(g_mb),
                                                     p(g_rb), ctypes.byref(sh), code, p(ws), nb, st), "bnn_conv3d_moments_backward_weight")
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1 + (2 if rho_b is None else 3)       # slabs + reduce (+ the bias sums)
    return [g_am, g_av, g_mu, g_rho] + ([] if rho_b is None else [g_mb, g_rb]), s2_w


def conv_t(G, W, xshape, geo):
    """convT(G, W) in float64: the gradient of convNd(x, W) with respect to x with upstream G (linear in x)."""
    x = torch.zeros(xshape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(convnd(W.dim() - 2)(x, W.double(), None, *geo), x, G.double())[0]


def conv_w(a, G, wshape, geo):
    """sum gather(a) G in float64: the gradient of convNd(a, W) with respect to W with upstream G (linear in W)."""
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(convnd(len(wshape) - 2)(a.double(), w, None, *geo), w, G.double())[0]


def backward_reference(mode, a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b, geo, s2_dev):
    """-> [(name, float64 reference, bound)] in backward_device's order (CPU tensors; s2_dev the device's fp32 sigma_w^2)."""
    d = lambda t: t.double()         # noqa: E731
    groups = geo[3]
    taps = mu_w[0, 0].numel()
    R = (mu_w.shape[0] // groups) * taps
    R2 = G_m.shape[0] * G_m[0, 0].numel()
    c_w = 2 * sigma64(rho_w) * torch.sigmoid(d(rho_w))
    c_b = None if rho_b is None else 2 * sigma64(rho_b) * torch.sigmoid(d(rho_b))
    red = [0] + list(range(2, G_m.dim()))
    if mode == "f32":
        s2 = sigma64(rho_w) ** 2
        assert ((d(s2_dev) - s2).abs() <= 1e-6 * s2).all()
        leaves = [d(a_m).requires_grad_(), d(a_v).requires_grad_(), d(mu_w).requires_grad_(), d(rho_w).requires_grad_()]
        zb = None
        if rho_b is not None:
            zb = torch.zeros_like(rho_b, dtype=torch.float64).requires_grad_()
            leaves += [zb, d(rho_b).requires_grad_()]
        out = ops.moments_convNd_f64(ops.Moments(leaves[0], leaves[1]), leaves[2], leaves[3], zb, leaves[5] if zb is not None else None,
                                     *geo, track=True)
        grads = torch.autograd.grad([out.mean, out.var], leaves, [d(G_m), d(G_v)])
        names = ["g_a_m", "g_a_v", "g_mu_w", "g_rho_w", "g_mu_b", "g_rho_b"]
        return [(n, r, scaled_bound(r)) for n, r in zip(names, grads)]
    # bf16: the planes as the loaders round them; each derived plane is one fp32 fma first
    qm, qv = rne_bf16(G_m), rne_bf16(G_v)
    p0, p1, p2 = rne_bf16(mu_w), rne_bf16(s2_dev), rne_bf16((d(mu_w) ** 2 + d(s2_dev)).float())
    r0, r1, r2 = rne_bf16(a_m), rne_bf16(a_v), rne_bf16((d(a_m) ** 2 + d(a_v)).float())
    xs, ws = a_m.shape, mu_w.shape
    tiny = 1e-300
    T = lambda G, W: conv_t(G, W, xs, geo)          # noqa: E731
    W = lambda a, G: conv_w(a, G, ws, geo)          # noqa: E731
    out = [("g_a_m", T(qm, p0) + 2 * d(a_m) * T(qv, p1),
            gamma(2 * R + 2) * (T(qm.abs(), p0.abs()) + 2 * d(a_m).abs() * T(qv.abs(), p1.abs())) + tiny),
           ("g_a_v", T(qv, p2), gamma(R + 1) * T(qv.abs(), p2.abs()) + tiny),
           ("g_mu_w", W(r0, qm) + 2 * d(mu_w) * W(r1, qv),
            gamma(2 * R2 + 2) * (W(r0.abs(), qm.abs()) + 2 * d(mu_w).abs() * W(r1.abs(), qv.abs())) + tiny)]
    t = W(r2, qv)
    out.append(("g_rho_w", t * c_w, gamma(R2 + 1) * W(r2.abs(), qv.abs()) * c_w + 16 * U * (t * c_w).abs() + tiny))
    if rho_b is not None:
        out.append(("g_mu_b", d(G_m).sum(red), gamma(R2) * d(G_m).abs().sum(red) + tiny))
        tb = d(G_v).sum(red)
        out.append(("g_rho_b", tb * c_b, gamma(R2) * d(G_v).abs().sum(red) * c_b + 16 * U * (tb * c_b).abs() + tiny))
    return out


# every case with its bias where it has one, and every case without
CASE_BIAS = [(c, b) for c in ALL_CASES for b in ((True, False) if ALL_CASES[c][7] else (False,))]


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case,bias", CASE_BIAS, ids=["%s-%s" % (c, "bias" if b else "nobias") for c, b in CASE_BIAS])
def test_conv_backward_matches_float64(dev, case, bias, mode):
    """Both entries against float64 on every case, with its bias and without.  Measured on the MI355X, the worst |err| / bound
    over the cases (g_a_m, g_a_v, g_mu_w, g_rho_w, g_mu_b, g_rho_b): fp32 mode 0.087 (2d-wide), 0.027, 0.038, 0.010, 0.013, 0.002;
    bf16 mode 0.047 (3d), 0.058 (3d), 0.023, 0.060 (tail), 0.021, 0.020."""
    ops_cpu = backward_case(case, bias)
    on_dev = to(dev, *ops_cpu[:7]) + [ops_cpu[7]]
    got, s2_dev = backward_device(dev, mode, *on_dev)
    _lib.check_device(dev)
    want = backward_reference(mode, *ops_cpu, s2_dev.cpu())
    assert len(got) == len(want)
    for a, (name, ref, bound) in zip(got, want):
        assert_within(a, ref, bound, "%s %s bias=%s %s" % (name, case, bias, mode))
    again, _ = backward_device(dev, mode, *on_dev)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_no_images_store_zero_weight_gradients(dev, mode):
    a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b, geo = backward_case("2d-geo", True)
    lib, p, st = _lib.load(), ops.ptr, ops.stream_ptr(dev)
    sh = conv3d_shape((0,) + tuple(a_m.shape[1:]), mu_w.shape[0], tuple(mu_w.shape[2:]), *geo)
    mu_w, rho_w, rho_b = to(dev, mu_w, rho_w, rho_b)
    outs = [torch.full_like(mu_w, 7.0), torch.full_like(mu_w, 7.0), torch.full_like(rho_b, 7.0), torch.full_like(rho_b, 7.0)]
    e = torch.empty(4, device=dev)
    nb = lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(sh))
    ws = torch.empty(nb // 4 + 4, device=dev)
    ops.check(lib.bnn_conv3d_moments_backward_weight(p(e), p(e), p(e), p(e), p(mu_w), p(rho_w), p(outs[0]), p(outs[1]), p(rho_b), p(outs[2]),
                                                     p(outs[3]), ctypes.byref(sh), ops._compute_code(mode), p(ws), nb, st),
              "bnn_conv3d_moments_backward_weight")
    torch.cuda.synchronize()
    assert all(not t.any() for t in outs)
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_deterministic_input_takes_k11s_backward_bit_for_bit(dev, mode):
    """A tensor input: the tracked conv's five gradients are bnn_conv3d_lrt_backward_input / _weight (nsets = 1, x = a_m) called on
    the same G; neither new contraction entry is reached (K11's launch counts: 1 + 3)."""
    a_m, _, G_m, G_v, mu_w, rho_w, rho_b, geo = backward_case("2d-geo", True)
    mu_b = conv_params(mu_w.shape[0], mu_w.shape[1], tuple(mu_w.shape[2:]), True, 11)[2]
    x, mu_w, rho_w, mu_b, rho_b = [t.to(dev).requires_grad_() for t in (a_m, mu_w, rho_w, mu_b, rho_b)]
    G_m, G_v = to(dev, G_m, G_v)
    out = ops.moments_convNd(x, mu_w, rho_w, mu_b, rho_b, *geo, compute=mode, track=True)
    plain = ops.moments_convNd(x, mu_w, rho_w, mu_b, rho_b, *geo, compute=mode)
    assert torch.equal(out.mean, plain.mean) and torch.equal(out.var, plain.var) and not plain.var.requires_grad
    lib, p, st = _lib.load(), ops.ptr, ops.stream_ptr(dev)
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    got = torch.autograd.grad([out.mean, out.var], [x, mu_w, rho_w, mu_b, rho_b], [G_m, G_v])
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 4                     # K11's input gradient; slabs, reduce and bias sums
    code = ops._compute_code(mode)
    sh = conv3d_shape(tuple(a_m.shape), mu_w.shape[0], tuple(mu_w.shape[2:]), *geo)
    s2_w, _ = ops._lrt_prepare_raw(rho_w.detach(), None)
    want = [torch.empty_like(t) for t in got]
    xx = x.detach()
    ops.check(lib.bnn_conv3d_lrt_backward_input(p(G_m), p(G_v), p(mu_w.detach()), p(s2_w), p(xx), p(want[0]), ctypes.byref(sh), 1, code, st),
              "bnn_conv3d_lrt_backward_input")
    nb = lib.bnn_conv3d_lrt_backward_weight_workspace_bytes(ctypes.byref(sh), 1)
    ws = torch.empty(nb // 4 + 4, device=dev)
    ops.check(lib.bnn_conv3d_lrt_backward_weight(p(xx), p(G_m), p(G_v), p(rho_w.detach()), p(want[1]), p(want[2]), p(rho_b.detach()),
                                                 p(want[3]), p(want[4]), ctypes.byref(sh), 1, code, p(ws), nb, st),
              "bnn_conv3d_lrt_backward_weight")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    _lib.check_device(dev)


def elu_bwd_deviation(g_m, g_v, m32, v32, gm, gv, a):
    """worst |device - float64| of the ELU's backward on fp32 inputs, in the units stated at ELU_BWD_M_TOL"""
    want = ops.moments_elu_backward_f64(ops.Moments(m32, v32), gm, gv, a)
    s = v32.double().sqrt()
    dm = ((g_m.double().cpu() - want[0]).abs() / (gm.double().abs() + s * gv.double().abs())).max().item()
    dv = ((g_v.double().cpu() - want[1]).abs() / (gm.double().abs() / s + gv.double().abs())).max().item()
    return dm, dv


@gpu
def test_elu_backward_matches_float64_on_a_grid(dev):
    """alpha in [-12, 12] at v = 1e-6, 0.3, 1, 47 for a = 1 and 0.5, random output gradients.  Measured on the MI355X: worst g_m
    deviation 5.784e-8, worst g_v deviation 5.376e-8 in the stated units (per (a, v) in the header comment); ELU_BWD_M_TOL =
    2.32e-7 and ELU_BWD_V_TOL = 2.16e-7 are 4 x that (both <= 1e-5)."""
    worst_m = worst_v = 0.0
    for a in GRID_A:
        for v in GRID_V:
            m32, v32, gm, gv = elu_grid(v, a)
            m, vv = m32.to(dev).requires_grad_(), v32.to(dev).requires_grad_()
            out = ops.moments_elu(ops.Moments(m, vv), a, track=True)
            plain = ops.moments_elu(ops.Moments(m, vv), a)
            assert torch.equal(out.mean, plain.mean) and torch.equal(out.var, plain.var) and not plain.mean.requires_grad
            g_m, g_v = torch.autograd.grad([out.mean, out.var], [m, vv], [gm.to(dev), gv.to(dev)])
            assert torch.isfinite(g_m).all() and torch.isfinite(g_v).all()
            dm, dv = elu_bwd_deviation(g_m, g_v, m32, v32, gm, gv, a)
            print("moments_elu backward a = %g v = %g: worst g_m deviation %.3e, worst g_v deviation %.3e" % (a, v, dm, dv))
            worst_m, worst_v = max(worst_m, dm), max(worst_v, dv)
    print("moments_elu backward: worst g_m deviation %.3e (bound %.2e), worst g_v deviation %.3e (bound %.2e)"
          % (worst_m, ELU_BWD_M_TOL, worst_v, ELU_BWD_V_TOL))
    assert ELU_BWD_M_TOL <= 1e-5 and ELU_BWD_V_TOL <= 1e-5
    assert worst_m <= ELU_BWD_M_TOL and worst_v <= ELU_BWD_V_TOL
    # v == 0 and the far tails, in place on the gradients
    m = torch.tensor([-2.0, 0.0, 3.0, 1e30, -1e30], device=dev)
    vv = torch.tensor([0.0, 0.0, 0.0, 1e-30, 1e-30], device=dev)
    gm, gv = torch.tensor([1.5, -2.0, 0.5, 0.25, 8.0], device=dev), torch.tensor([4.0, 3.0, -7.0, 2.0, 9.0], device=dev)
    want = ops.moments_elu_backward_f64(ops.Moments(m.cpu(), vv.cpu()), gm.cpu(), gv.cpu(), 0.5)
    lib = _lib.load()
    assert lib.bnn_moments_elu_backward(m.data_ptr(), vv.data_ptr(), gm.data_ptr(), gv.data_ptr(), gm.data_ptr(), gv.data_ptr(), 5, 0.5,
                                        ops.stream_ptr(dev)) == 0
    assert torch.equal(gm.cpu(), want[0].float()) and torch.equal(gv.cpu(), want[1].float())
    assert torch.equal(gm.cpu()[1:], torch.tensor([-2.0, 0.5, 0.25, 0.0])) and torch.equal(gv.cpu()[1:], torch.tensor([3.0, -7.0, 2.0, 0.0]))
    det = ops.moments_elu(ops.Moments(m.clone().requires_grad_()), 0.5, track=True)
    assert det.var is None and det.mean.requires_grad
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("act", ["relu", ("elu", 1.0)], ids=["relu", "elu"])
def test_tracked_forward_is_the_fused_forward_bit_for_bit(dev, act, mode, switch):
    xs, O, kernel, stride, padding, dilation, groups, _ = CASES["2d-geo"]
    p = [t.to(dev).requires_grad_() for t in conv_params(O, xs[1] // groups, kernel, True, 11)]
    mom = conv_input(xs, True, 12)
    a = ops.Moments(mom.mean.to(dev).requires_grad_(), mom.var.to(dev).requires_grad_())
    geo = (stride, padding, dilation, groups)
    fused = ops.moments_convNd(a, *p, *geo, activation=act, compute=mode)
    tracked = ops.moments_convNd(a, *p, *geo, activation=act, compute=mode, track=True)
    assert not fused.mean.requires_grad and tracked.mean.requires_grad and tracked.var.requires_grad
    assert torch.equal(fused.mean, tracked.mean) and torch.equal(fused.var, tracked.var)
    with torch.no_grad():
        assert not ops.moments_convNd(a, *p, *geo, activation=act, compute=mode, track=True).mean.requires_grad
    # the layer: its result carries the activation and the twin passes it through
    bnn.set_compute(mode)
    seq = torch.nn.Sequential(NormalConv2d(xs[1], O, kernel, stride, padding, dilation, groups),
                              torch.nn.ReLU() if act == "relu" else torch.nn.ELU(alpha=act[1])).to(dev)
    assert bnn_nn.moment_activations(seq) == 1
    with torch.no_grad():
        for t, s in zip((seq[0].weight.mean, seq[0].weight.scale, seq[0].bias.mean, seq[0].bias.scale), p):
            t.copy_(s)
    net = BayesianNetworkModule(xs[1], O)
    net.layers = seq
    net._forward = lambda x: seq(x)
    got = net.forward_moments(a)
    assert got._act is None and torch.equal(got.mean, fused.mean) and torch.equal(got.var, fused.var) and got.var.requires_grad
    inf = net.predictive_moments(a)
    assert torch.equal(inf.mean, fused.mean) and torch.equal(inf.var, fused.var) and not inf.var.requires_grad


def dense_bounds(mode, a_m, a_v, G_m, G_v, w):
    """K18's dense bounds for ops.moments_affine's backward (sigma^2 = 0): -> [(name, reference, bound)] for g_a_m, g_a_v, g_w, g_b."""
    d = lambda t: t.double()         # noqa: E731
    B, N = G_m.shape
    if mode == "f32":
        leaves = [d(a_m).requires_grad_(), d(a_v).requires_grad_(), d(w).requires_grad_(), torch.zeros(N, dtype=torch.float64, requires_grad=True)]
        out = ops.moments_affine_f64(ops.Moments(leaves[0], leaves[1]), leaves[2], leaves[3], track=True)
        grads = torch.autograd.grad([out.mean, out.var], leaves, [d(G_m), d(G_v)])
        return [(n, r, scaled_bound(r)) for n, r in zip(("g_a_m", "g_a_v", "g_w", "g_b"), grads)]
    qm, qv = rne_bf16(G_m), rne_bf16(G_v)
    p0, p2 = rne_bf16(w), rne_bf16((d(w) ** 2).float())
    r0, r1 = rne_bf16(a_m), rne_bf16(a_v)
    tiny = 1e-300
    return [("g_a_m", qm @ p0, gamma(2 * N + 2) * (qm.abs() @ p0.abs()) + tiny),
            ("g_a_v", qv @ p2, gamma(N + 1) * (qv.abs() @ p2.abs()) + tiny),
            ("g_w", qm.t() @ r0 + 2 * d(w) * (qv.t() @ r1),
             gamma(2 * B + 2) * (qm.abs().t() @ r0.abs() + 2 * d(w).abs() * (qv.abs().t() @ r1.abs())) + tiny),
            ("g_b", d(G_m).sum(0), gamma(B) * d(G_m).abs().sum(0) + tiny)]


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(33, 100, 7), (70, 128, 10)], ids=lambda s: "x".join(map(str, s)))
def test_affine_backward_matches_float64(dev, shape, mode):
    B, K, N = shape
    g = torch.Generator().manual_seed(41)
    w, b = (torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5, torch.rand(N, generator=g) - 0.5
    a_m, a_v = torch.randn(B, K, generator=g), 0.5 * torch.rand(B, K, generator=g) ** 2
    a_v[a_v < 0.02] = 0.0
    G_m, G_v = torch.randn(B, N, generator=g), torch.randn(B, N, generator=g)
    leaves = [t.to(dev).requires_grad_() for t in (a_m, a_v, w, b)]
    out = ops.moments_affine(ops.Moments(leaves[0], leaves[1]), leaves[2], leaves[3], compute=mode, track=True)
    plain = ops.moments_affine(ops.Moments(leaves[0], leaves[1]), leaves[2], leaves[3], compute=mode)
    assert torch.equal(out.mean, plain.mean) and torch.equal(out.var, plain.var) and not plain.var.requires_grad
    lib = _lib.load()
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    got = torch.autograd.grad([out.mean, out.var], leaves, to(dev, G_m, G_v))
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 3                     # K18's input gradient, weight gradient and bias sums
    for a, (name, ref, bound) in zip(got, dense_bounds(mode, a_m, a_v, G_m, G_v, w)):
        assert_within(a, ref, bound, "affine %s %s %s" % (name, shape, mode))
    det = ops.moments_affine(leaves[0], leaves[2], leaves[3], compute=mode, track=True)
    assert det.var is None and det.mean.requires_grad           # a deterministic input stays plain torch, not detached
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_inputs_off_16_bytes_give_the_same_bits(dev, mode):
    """Every input of the three entries is fetched one element per load: moved to an address that is aligned to the element only
    (NaN guards around it), and the slab workspace moved by 8 bytes, the results are bit-equal to the aligned run."""
    case = backward_case("2d-geo", True)
    on_dev = to(dev, *case[:7])
    want, _ = backward_device(dev, mode, *on_dev, case[7])
    for k in (0, 1):
        moved = [offset_view(t, (4, 8)[(i + k) % 2]) for i, t in enumerate(on_dev)]
        got, _ = backward_device(dev, mode, *moved, case[7], ws_off=2 * k + 1)
        assert all(bool(torch.isfinite(a).all()) and same_bits(a, b) for a, b in zip(got, want))
    if mode == "f32":
        lib, p = _lib.load(), ops.ptr
        m32, v32, gm, gv = to(dev, *elu_grid(0.3, 0.5, 1001))
        outs = []
        for f in (lambda t, o: t, offset_view):
            g_m, g_v = output_view(m32.shape, torch.float32, dev, 4), output_view(m32.shape, torch.float32, dev, 8)
            a = [f(t, (4, 8)[i % 2]) for i, t in enumerate((m32, v32, gm, gv))]          # (held until the launch has run)
            ops.check(lib.bnn_moments_elu_backward(p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(g_m), p(g_v), m32.numel(), 0.5,
                                                   ops.stream_ptr(dev)), "bnn_moments_elu_backward")
            torch.cuda.synchronize()
            assert guards_intact(g_m) and guards_intact(g_v)
            outs.append((g_m.clone(), g_v.clone()))
        assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    _lib.check_device(dev)


@gpu
def test_outputs_off_16_bytes_are_refused_by_the_entries(dev):
    """g_a_m / g_a_v / g_mu_w / g_rho_w off the 16-byte boundary: BNN_E_ALIGN from the C entries, nothing launched or written."""
    a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b, geo = backward_case("2d-geo", True)
    sh = conv3d_shape(tuple(a_m.shape), mu_w.shape[0], tuple(mu_w.shape[2:]), *geo)
    a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b = to(dev, a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b)
    s2_w, _ = ops._lrt_prepare_raw(rho_w, None)
    lib, p, st = _lib.load(), ops.ptr, ops.stream_ptr(dev)
    nb = lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(sh))
    ws = torch.empty(nb // 4, device=dev)
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    for off in (4, 8):
        bad, good = output_view(a_m.shape, torch.float32, dev, off), output_view(a_m.shape, torch.float32, dev, 0)
        for first, second in ((bad, good), (good, bad)):
            assert lib.bnn_conv3d_moments_backward_input(p(G_m), p(G_v), p(mu_w), p(s2_w), p(a_m), p(first), p(second), ctypes.byref(sh), 0,
                                                         st) == _lib.E_ALIGN
        wbad, wgood = output_view(mu_w.shape, torch.float32, dev, off), output_view(mu_w.shape, torch.float32, dev, 0)
        for first, second in ((wbad, wgood), (wgood, wbad)):
            assert lib.bnn_conv3d_moments_backward_weight(p(a_m), p(a_v), p(G_m), p(G_v), p(mu_w), p(rho_w), p(first), p(second), None, None,
                                                          None, ctypes.byref(sh), 0, p(ws), nb, st) == _lib.E_ALIGN
        torch.cuda.synchronize()
        for t in (bad, good, wbad, wgood):
            assert guards_intact(t) and bool((t == -12345.0).all())
    assert lib.bnn_launch_count() == n0


# End to end against float64 autograd of the CPU recursion.  The device result passes through a chain of stages, each within its
# own bound of float64 on its own inputs.  Network (a): Conv2d, ELU (torch), the Bayesian conv's contraction, its ELU, the dense
# contraction, the sampling launch, softmax / nll (torch) -- 7 forward stages -- and the sampling backward, the dense backward, the
# ELU backward, the conv backward, torch's ELU and Conv2d backward -- 6: 13 stages.  Network (b) has a Bayesian conv and a moment ELU
# in place of the two torch stages, forward and backward: 13 too.
# fp32 mode: every stage is within 1e-5 of its output's scale (the project's parity rule; the ELU bounds are below it), so to
# first order the gradients are within 13 x 1e-5 of theirs.
# bf16 mode: each contraction reads operands rounded to bf16 (2^-8 per product), so against float64 on the UNROUNDED operands it
# is within 2^-8 sum |a| |b| <= 2^-8 sqrt(R) of the scale of its sum, R its reduction length (Cauchy-Schwarz on the rms).  Per layer:
#   the Bayesian conv 4 -> 6, 3 x 3, stride 2 on 8 x 8 (P = 16):  forward R = 36, input gradient R = 54, weight gradient R = 144
#   NormalLinear 96 -> 5 at B = 9:                               forward R = 96, input gradient R = 5,  weight gradient R = 9
#   (b) the front NormalConv2d 1 -> 4, 3 x 3 on 10 x 10 (P = 64): forward R = 9,  weight gradient R = 576 (x needs no gradient)
E2E_R = {"a": (36, 54, 144, 96, 5, 9), "b": (36, 54, 144, 96, 5, 9, 9, 576)}
E2E_TOL = {(n, "f32"): 13 * 1e-5 for n in "ab"}
E2E_TOL.update({(n, "bf16"): 13 * 1e-5 + 2.0 ** -8 * sum(math.sqrt(r) for r in E2E_R[n]) for n in "ab"})


def e2e_step(net, xd, t, S, key=None):
    """-> (logit moments, probabilities, parameter gradients); key None: net.sample_moments (the model's stream, a fresh key)."""
    mom = net.forward_moments(xd)
    if key is None:
        ps = net.sample_moments(mom, S)
    else:
        ps = torch.softmax(ops.moments_sample(ops.Moments(mom.mean, mom.var), key, S, track=True), -1)
    loss = F.nll_loss(torch.log(ps.reshape(-1, ps.shape[-1])), t.repeat(S), reduction="sum")
    return mom, ps, torch.autograd.grad(loss, list(net.parameters()))


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("which", ["a", "b"])
def test_network_gradients_end_to_end(dev, which, mode, switch):
    """(9, 1, 10, 10) through ConvNet (a: a deterministic Conv2d in front; b: a NormalConv2d, which reaches the VAR kernels):
    forward_moments is predictive_moments bit for bit; the gradients of nll_loss(log(sample_moments(mom, 8))) (summed over the 72
    rows) with respect to every parameter match float64 autograd of the CPU recursion fed the eps recovered from the device's
    samples, within E2E_TOL of each gradient's scale; a second run on the same key gives the same bits."""
    bnn.set_compute(mode)
    torch.manual_seed(8)
    cpu = set_posteriors(ConvNet(which == "b"), 80)
    net = ConvNet(which == "b")
    net.load_state_dict(cpu.state_dict())
    net = net.to(dev)
    g = torch.Generator().manual_seed(81)
    x, t = torch.randn(9, 1, 10, 10, generator=g), torch.randint(0, 5, (9,), generator=g)
    xd, td = x.to(dev), t.to(dev)
    S = 8
    mom, ps, got = e2e_step(net, xd, td, S)
    if which == "b":                                            # (a: torch's Conv2d need not repeat its bits from call to call)
        ref = net.predictive_moments(xd)
        assert torch.equal(mom.mean, ref.mean) and torch.equal(mom.var, ref.var)
    assert mom.link == "softmax" and mom.mean.requires_grad
    key = net.moment_key
    assert (key.nsamples, key.sample0, key.stream) == (S, 0, net._moment_stream)
    if which == "b":
        _, ps2, again = e2e_step(net, xd, td, S, key)
        assert torch.equal(ps, ps2) and all(torch.equal(a, b) for a, b in zip(got, again))
    # float64 autograd of the CPU recursion on the device's eps
    ys = ops.moments_sample(ops.Moments(mom.mean.detach(), mom.var.detach()), key, S)
    assert torch.equal(torch.softmax(ys, -1), ps.detach())
    eps = recovered_eps(ys, mom.mean, mom.var)
    assert eps.abs().max() < 7
    net64 = cpu.double()
    m64 = net64.forward_moments(x.double())
    assert m64.mean.dtype == torch.float64 and m64.link == "softmax"
    y64 = torch.softmax(m64.mean + torch.sqrt(m64.var + 1e-16) * eps, -1)
    want = torch.autograd.grad(F.nll_loss(torch.log(y64.reshape(-1, 5)), t.repeat(S), reduction="sum"), list(net64.parameters()))
    names = [n for n, _ in net.named_parameters()]
    assert len(names) == len(got) == len(want) == (10 if which == "a" else 12)
    for n, a, w in zip(names, got, want):
        assert_within(a, w, scaled_bound(w, E2E_TOL[(which, mode)]), "%s net %s %s" % (n, which, mode))
    _lib.check_device(dev)


@gpu
def test_forward_and_backward_are_graph_capturable(dev, switch):
    """forward_moments of network (b), the sampling launch on a fixed key, the loss and the whole backward in ONE captured graph on a
    side stream: two replays give the eager gradients' bits."""
    torch.manual_seed(8)
    net = set_posteriors(ConvNet(True), 80).to(dev)
    g = torch.Generator().manual_seed(82)
    xd = torch.randn(9, 1, 10, 10, generator=g).to(dev)
    t = torch.randint(0, 5, (9,), generator=g).to(dev)
    key = DrawKey(0x1234567890ABCDEF, 323, 0, 4, 19, gen=_rng.generator_for("f32"))

    def step():
        return e2e_step(net, xd, t, 4, key)[2]

    want = [a.clone() for a in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                  # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = step()
    for _ in range(2):
        for a in got:
            a.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_conv_training_without_sampling(dev, mode, switch):
    """200 Adam steps of the sampling-free regression loss through two Bayesian convs on the device: the loss falls below half its
    starting value (the CPU float64 path ends below a quarter, test_conv_training_without_sampling_cpu), and no key is ever drawn."""
    bnn.set_compute(mode)
    net, losses = toy_conv_regression(dev)
    print("toy conv regression, %s: loss %.4f -> %.4f (ratio %.3f)" % (mode, losses[0], losses[-1], losses[-1] / losses[0]))
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < 0.5 * losses[0]
    assert not hasattr(net, "moment_key")
