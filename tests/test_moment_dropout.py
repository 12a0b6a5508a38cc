"""Sampling-free passes through MC-dropout and Flipout layers (K22, csrc/bnn_moments_dropout.hip, nn.moment_estimator_layers).

An MC-dropout layer hands on f(b z / q) = b f(z / q): z ~ N(m, v) its pre-dropout output, b ~ Bernoulli(q), q = 1 - p, f the activation
behind it with f(0) = 0.  With (M, V) the moments of f at N(m / q, v / q^2)

    mean' = q M,    var' = q V + q p M^2

(ops.moments_dropout / bnn_moments_dropout; float64 twin ops.moments_dropout_f64).  CPU tests: the twin against quadrature, the
limits, the backward twin, the exactness on a Titanic-shaped net, the reference's own sampler, Flipout, the plumbing, the tail.
GPU tests: the kernels against the twin, sizes and addresses, the networks in both compute modes, launches, graph capture, the tail.

Bounds.  Forward kernel: with r = sqrt(m^2 + v) -- every term of mean' is bounded by r, every term of var' by r^2 (|M| <= r / q,
V <= v / q^2, times q and q p) -- DROPOUT_TOL r and DROPOUT_TOL r^2, DROPOUT_TOL = 1e-5, the project's parity bar.  Backward kernel:
in test_moment_pool.py's form, |got - ref| - TINY <= tol x magnitude with its TINY = 2^-126, the magnitude that of the gradient's own two terms,
|g_mean'| |d mean'/d x| + |g_var'| |d var'/d x| (x = m or v: in the tails both are of the size of the gradient itself, 1e-33 at
alpha = -12), and tol = DROPOUT_TOL + 4 alpha^2 U, U = 2^-24.  The second addend is what the number format costs: every tail term
carries phi(alpha) = exp(-alpha^2 / 2) or Phi(-|alpha|) of the same decay, and the kernel forms alpha = (m / q) / sqrt(v / q^2)
from fp32 values -- one rounding in m / q, two in v / q^2 halved by the square root, one each in the root and the quotient (q's own
rounding cancels in alpha): 3.5 U relative, 4 U taken, which exp(-alpha^2 / 2) turns into alpha^2 x 4 U relative, 3.4e-5 at
|alpha| = 12 (the ELU path rounds m / q and v / q^2 to fp32 before its fp64 evaluation: the same alpha).  A deterministic input has
no tail terms: DROPOUT_TOL alone.  The ReLU path is fp32 throughout, and its mean M = s (alpha Phi + phi) cancels for alpha < 0 (to
phi / alpha^2): the g_var' terms, which all carry M, are allowed kappa = (|alpha| Phi + phi) / (alpha Phi + phi) times their
magnitude (1 for alpha >= 0, about 2 alpha^2 in the far negative tail, where the terms are below 1e-20 of the gradients elsewhere).
So that a regression in the bulk cannot hide inside the tail allowance, on |alpha| <= 3 (4 alpha^2 U <= 2e-6 there) every gradient is
also held to DROPOUT_TOL alone of the plain magnitude, without kappa.
The twin is evaluated on the fp32 inputs and on the p the device receives (p rounded to fp32).
Measured on the MI355X (test_forward_kernel_matches_the_twin_on_the_grid / test_backward_kernel_matches_float64_autograd print
them), worst over the grid, identity / ReLU / ELU a = 1 / ELU a = 0.5: forward mean 7.4e-8 / 1.96e-7 / 1.47e-7 / 1.41e-7 r, variance
1.63e-6 / 3.16e-6 / 2.00e-6 / 2.13e-6 r^2 (all at p = 0.9, where v / q^2 carries q's rounding a hundredfold); backward, worst error
over its bound, g_m 0.019 / 0.492 / 0.376 / 0.379, g_v 0.015 / 0.334 / 0.891 / 0.383; on |alpha| <= 3 over 1e-5 of the plain magnitude,
g_m 0.018 / 0.860 / 0.112 / 0.102, g_v 0.015 / 0.153 / 0.219 / 0.151.
Networks: K16's dense bounds (test_moment_propagation.py) and K17's conv bounds (test_moment_conv.py) per contraction;
gradients in test_moment_pool.py's manner: 1e-5 per stage, and in the bf16 mode 2^-8 sqrt(R) per bf16 contraction of reduction
length R.
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
from bayesianneuralnetworks_amd.nn import (BayesianNetworkModule, FlipOutNormalConv2d, FlipoutNormalLinear, MCDropoutConv1d,
                                           MCDropoutConv2d, MCDropoutConv3d, MCDropoutLinear, NormalConv2d, NormalLinear)

from alignment import guards_intact, offset_view, output_view, same_bits
from bf16ref import gamma, rne_bf16
from test_flipout_mc import _code_object_notes
from test_lrt_device import assert_within, scaled_bound
from test_moment_backward import recovered_eps
from test_moment_conv import ELU_GRID_A, ELU_GRID_V

gpu = pytest.mark.gpu

DROPOUT_TOL = 1e-5
TINY = 2.0 ** -126                 # test_moment_pool.py's: the smallest normal fp32
U = 2.0 ** -24
GRID_P = (0.1, 0.2, 0.5, 0.9)
ACTS = (None, 'relu') + tuple(('elu', a) for a in ELU_GRID_A)
ALPHA = torch.linspace(-12, 12, 4801, dtype=torch.float64)
BULK = ALPHA.abs() <= 3


@pytest.fixture(autouse=True)
def switches_off():
    yield
    bnn_nn.moment_estimator_layers(False)
    bnn_nn.conv_moment_training(False)


def act_name(act):
    return "none" if act is None else act if isinstance(act, str) else "elu%g" % act[1]


def plain_act(act, x):
    if act is None:
        return x
    return torch.relu(x) if act == 'relu' else F.elu(x, act[1])


class Seq(BayesianNetworkModule):
    def __init__(self, *mods, samples=8):
        super().__init__(1, 1, samples=samples)
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


def titanic(hidden=24, p=0.2, softmax=True, seed=3, inputs=9):
    """The Titanic example's shape: MCDropoutLinear -> ELU -> MCDropoutLinear (-> Softmax), rewritten by nn.moment_activations."""
    torch.manual_seed(seed)
    mods = [MCDropoutLinear(inputs, hidden, drop_prob=p), torch.nn.ELU(), MCDropoutLinear(hidden, 2, drop_prob=p)]
    net = Seq(*(mods + ([torch.nn.Softmax(dim=-1)] if softmax else [])))
    bnn_nn.moment_activations(net)
    return net


def titanic_closed_form(net, x, p):
    """The logits' pre-dropout moments for a deterministic input, float64: the hidden masks are independent, so these are exact."""
    q = 1.0 - p
    l1, l2 = net.layers[0].linear, net.layers[2].linear
    z1 = x.double() @ l1.weight.double().t() + l1.bias.double()
    e = F.elu(z1 / q)
    hm, hv = q * e, q * p * e * e
    w2 = l2.weight.double()
    return hm @ w2.t() + l2.bias.double(), hv @ (w2 * w2).t()


# ================================================================================================ CPU
def act_quadrature(mi, vi, act, nodes=200):
    """E[f(x)] and E[f(x)^2] for x ~ N(mi, vi) by Gauss-Legendre on [mi - 14 s, 0] and [0, mi + 14 s] (the kink at 0 is a panel
    edge), float64, vectorised over mi."""
    t, w = np.polynomial.legendre.leggauss(nodes)
    t, w = torch.from_numpy(t), torch.from_numpy(w)
    s = math.sqrt(vi)
    lo, hi = mi - 14 * s, mi + 14 * s
    mid = torch.zeros_like(mi).clamp(min=lo, max=hi)
    e1, e2 = torch.zeros_like(mi), torch.zeros_like(mi)
    for a0, b0 in ((lo, mid), (mid, hi)):
        x = 0.5 * (a0 + b0)[:, None] + 0.5 * (b0 - a0)[:, None] * t
        wt = 0.5 * (b0 - a0)[:, None] * w * torch.exp(-0.5 * ((x - mi[:, None]) / s) ** 2) / (s * math.sqrt(2 * math.pi))
        fx = plain_act(act, x)
        e1, e2 = e1 + (wt * fx).sum(1), e2 + (wt * fx * fx).sum(1)
    return e1, e2


@pytest.mark.parametrize("act", ACTS, ids=act_name)
def test_twin_against_quadrature(act):
    """ops.moments_dropout_f64 against quadrature of E[f(z / q)] and E[f(z / q)^2] with the Bernoulli factor applied here
    (mean' = q E1, var' = q E2 - q^2 E1^2), on test_moment_conv.py's ELU grid x p x activation, to 1e-8 of s and of v: the bound of
    test_elu_reference_against_quadrature."""
    worst = 0.0
    for p in GRID_P:
        q = 1.0 - p
        for v in ELU_GRID_V:
            s = math.sqrt(v)
            m = ALPHA * s
            out = ops.moments_dropout_f64(ops.Moments(m, torch.full_like(m, v)), p, act)
            e1, e2 = act_quadrature(m / q, v / (q * q), act)
            dm = ((out.mean - q * e1).abs() / s).max().item()
            dv = ((out.var - (q * e2 - q * q * e1 * e1)).abs() / v).max().item()
            worst = max(worst, dm, dv)
            print("moments_dropout_f64 %s p = %g v = %g: against quadrature %.2e s, %.2e v" % (act_name(act), p, v, dm, dv))
            assert dm <= 1e-8 and dv <= 1e-8, (act, p, v, dm, dv)
            assert (out.var >= 0).all()
    print("moments_dropout_f64 %s: worst deviation from quadrature %.2e" % (act_name(act), worst))


def test_limits():
    g = torch.Generator().manual_seed(5)
    m, v = torch.randn(50, generator=g, dtype=torch.float64), torch.rand(50, generator=g, dtype=torch.float64)
    mom = ops.Moments(m, v)
    for act in ACTS:
        alone = mom if act is None else ops.moments_relu_f64(mom) if act == 'relu' else ops.moments_elu_f64(mom, act[1])
        out = ops.moments_dropout_f64(mom, 0.0, act)                                # p = 0: the activation alone
        assert torch.equal(out.mean, alone.mean) and torch.equal(out.var, alone.var)
        out = ops.moments_dropout_f64(mom, 1.0, act)                                # p = 1: everything is dropped
        assert not out.mean.any() and not out.var.any()
        for p in GRID_P:                                                            # a deterministic input, both ways of saying so
            q = 1.0 - p
            f = plain_act(act, m / q)
            for det in (ops.Moments(m, torch.zeros_like(m)), ops.Moments(m, None), m):
                out = ops.moments_dropout_f64(det, p, act)
                assert (out.mean - q * f).abs().max() <= 1e-15 * (1 + f.abs().max())
                assert (out.var - q * p * f * f).abs().max() <= 1e-15 * (1 + (f * f).max())
    with pytest.raises(ValueError, match="dropout probability"):
        ops.moments_dropout_f64(mom, 1.5)
    with pytest.raises(ValueError, match="activation must be"):
        ops.moments_dropout_f64(mom, 0.5, 'tanh')
    linked = ops.Moments(m, v, link='softmax')
    with pytest.raises(ops.BnnHipError, match="carries link"):
        ops.moments_dropout_f64(linked, 0.5)


@pytest.mark.parametrize("act", ACTS, ids=act_name)
def test_backward_twin_gradcheck(act):
    """The tracked twin against finite differences with test_moment_pool.py's gradcheck settings, and
    ops.moments_dropout_backward_f64 (the formula) against its autograd."""
    g = torch.Generator().manual_seed(31)
    for p in (0.0,) + GRID_P:
        m = torch.randn(12, generator=g, dtype=torch.float64, requires_grad=True)
        v = (0.2 + torch.rand(12, generator=g, dtype=torch.float64)).requires_grad_()

        def fn(m_, v_):
            o = ops.moments_dropout_f64(ops.Moments(m_, v_), p, act, track=True)
            return o.mean, o.var

        assert torch.autograd.gradcheck(fn, (m, v), eps=1e-6, atol=1e-7, rtol=1e-6)
        gm, gv = torch.randn(12, generator=g, dtype=torch.float64), torch.randn(12, generator=g, dtype=torch.float64)
        want = torch.autograd.grad(list(fn(m, v)), [m, v], [gm, gv])
        got = ops.moments_dropout_backward_f64(ops.Moments(m, v), gm, gv, p, act)
        for a, b in zip(got, want):
            assert (a - b).abs().max() <= 1e-13 * (1 + b.abs().max())
        det = ops.moments_dropout_backward_f64(ops.Moments(m), gm, gv, p, act)       # a deterministic input
        md = m.detach().clone().requires_grad_()
        o = ops.moments_dropout_f64(ops.Moments(md), p, act, track=True)
        wd, = torch.autograd.grad([o.mean, o.var], [md], [gm, gv])
        assert det[1] is None and (det[0] - wd).abs().max() <= 1e-13 * (1 + wd.abs().max())
    z = ops.moments_dropout_backward_f64(ops.Moments(m, v), gm, gv, 1.0, act)
    assert not z[0].any() and not z[1].any()
    # v == 0 given as a tensor: with x = m / q, M = f(x), d = f'(x) (elu'(0) = 1, relu'(0) = 0) and h = lim d M / d v = f''(x) / 2
    # (a exp(x) / 2 for the ELU at x < 0, else 0):  g_m = d (g_mean + 2 p M g_var),  g_v = (g_var d^2 + (g_mean + 2 p M g_var) h) / q
    m0 = torch.cat([torch.tensor([-2.0, -0.3, 0.0, 0.4, 3.0], dtype=torch.float64), m.detach()[:7]])
    for p in GRID_P:
        q = 1.0 - p
        x = m0 / q
        M = plain_act(act, x)
        if act is None:
            d, h = torch.ones_like(x), torch.zeros_like(x)
        elif act == 'relu':
            d, h = (x > 0).double(), torch.zeros_like(x)
        else:
            d = torch.where(x < 0, act[1] * torch.exp(x), torch.ones_like(x))
            h = torch.where(x < 0, 0.5 * act[1] * torch.exp(x), torch.zeros_like(x))
        t = gm + 2.0 * p * M * gv
        got = ops.moments_dropout_backward_f64(ops.Moments(m0, torch.zeros_like(m0)), gm, gv, p, act)
        assert (got[0] - d * t).abs().max() <= 1e-14 * (1 + t.abs().max())
        assert (got[1] - (gv * d * d + t * h) / q).abs().max() <= 1e-14 * (1 + t.abs().max()) / q
    with torch.enable_grad():
        assert not ops.moments_dropout_f64(ops.Moments(m, v), 0.3, act).mean.requires_grad           # untracked: detached


def test_titanic_shape_is_exact():
    """9 -> 24 -> 2, B = 5, p = 0.2: through nn.moment_activations and the switch the logits' PRE-dropout moments come out with
    link='softmax' and dropout = 0.2, equal to the closed form to the fp32 rounding of the result."""
    p = 0.2
    net = titanic(24, p)
    x = torch.randn(5, 9, generator=torch.Generator().manual_seed(4))
    bnn_nn.moment_estimator_layers()
    mom = net.predictive_moments(x)
    assert mom.link == 'softmax' and mom.dropout == p and "dropout=0.2" in repr(mom)
    assert mom.mean.dtype == torch.float32 and mom.mean.shape == (5, 2)
    m, v = titanic_closed_form(net, x, p)
    for got, ref, what in ((mom.mean, m, "mean"), (mom.var, v, "var")):
        d = ((got.double() - ref).abs() / ref.abs()).max().item()
        print("titanic closed form, %s: worst relative deviation %.2e" % (what, d))
        assert d <= 2.0 ** -24 * (1 + 1e-6)
    flat = mom.view(10)
    assert flat.dropout == p and flat.link == 'softmax' and flat.shape == (10,)
    with pytest.raises(ValueError, match="needs link='softmax'"):
        ops.Moments(mom.mean, mom.var, dropout=0.2)


def five_se(samples, mean, var, what):
    """samples (S, ...) float64 against the claimed moments: EVERY mean within 5 standard errors, every variance within 5 standard
    errors of the sample variance by the sample's own fourth central moment."""
    S = samples.shape[0]
    sm = samples.mean(0)
    d = samples - sm
    sv = (d * d).sum(0) / (S - 1)
    m4 = (d ** 4).mean(0)
    z_m = ((sm - mean).abs() / (sv / S).sqrt()).max().item()
    z_v = 0.0 if var is None else ((sv - var).abs() / ((m4 - sv * sv).clamp_min(0) / S).sqrt()).max().item()
    print("%s: worst mean %.2f standard errors, worst variance %.2f standard errors" % (what, z_m, z_v))
    assert z_m <= 5 and z_v <= 5, (what, z_m, z_v)
    return z_m, z_v


def test_against_the_reference_sampler():
    """The same net without the Softmax: predictive_regression(outputs='values', propagation='moments') -- the post-dropout moments
    of the outputs -- against 200 000 draws of the layers' own serial-loop forward (F.dropout, seeded), every element of every row.
    The draws of one input row are independent whichever call they come from, so they are taken 10 000 copies of the batch at a
    time."""
    p = 0.2
    net = titanic(24, p, softmax=False)
    x = torch.randn(5, 9, generator=torch.Generator().manual_seed(4))
    bnn_nn.moment_estimator_layers()
    out = net.predictive_regression(x, outputs='values', propagation='moments')
    assert not out.aleatoric.any() and torch.equal(out.total, out.epistemic)
    torch.manual_seed(1234)
    S, chunk = 200_000, 10_000
    with torch.no_grad():
        ys = torch.cat([net._forward(x.repeat(chunk, 1)).reshape(chunk, 5, 2).double() for _ in range(S // chunk)])
    assert ys.shape == (S, 5, 2)
    five_se(ys, out.mean.double(), out.total.double(), "titanic without softmax against %d sampler draws" % S)


def test_flipout():
    torch.manual_seed(9)
    x = torch.randn(4, 12)
    hidden = ops.Moments(torch.randn(4, 12), torch.rand(4, 12))
    flip, normal = FlipoutNormalLinear(12, 5), NormalLinear(12, 5, bias=False)
    normal.load_state_dict(flip.state_dict())
    nets = Seq(flip), Seq(normal)
    with pytest.raises(ops.BnnHipError, match="FlipoutNormalLinear is not supported"):
        nets[0].predictive_moments(x)
    bnn_nn.moment_estimator_layers()
    for inp in (x, hidden):
        a, b = nets[0].predictive_moments(inp), nets[1].predictive_moments(inp)
        assert torch.equal(a.mean, b.mean) and torch.equal(a.var, b.var) and (a.var > 0).all()
    mom = nets[0].predictive_moments(x)
    with torch.no_grad():                                                           # its own sign sampler, one sign draw per call
        ys = torch.stack([flip(x) for _ in range(4000)]).double()
    five_se(ys, mom.mean.double(), None, "FlipoutNormalLinear mean against its sign sampler")
    sv = ys.var(0)
    print("FlipoutNormalLinear: worst |sampled var / moment var - 1| %.3f" % (sv / mom.var.double() - 1).abs().max().item())
    torch.manual_seed(10)
    fc, nc = FlipOutNormalConv2d(3, 4, 3, padding=1), NormalConv2d(3, 4, 3, padding=1, bias=False)
    nc.load_state_dict(fc.state_dict())
    img = torch.randn(2, 3, 6, 5)
    a, b = Seq(fc).predictive_moments(img), Seq(nc).predictive_moments(img)
    assert torch.equal(a.mean, b.mean) and torch.equal(a.var, b.var) and a.mean.shape == (2, 4, 6, 5)
    ma, mb = Seq(fc).forward_moments, Seq(nc).forward_moments
    with pytest.raises(ops.BnnHipError, match="FlipOutNormalConv2d has no moment backward"):
        ma(img)                                                                     # the conv ones need nn.conv_moment_training too
    bnn_nn.conv_moment_training()
    a, b = ma(img), mb(img)
    assert torch.equal(a.mean, b.mean) and a.mean.requires_grad
    assert torch.equal(Seq(flip).forward_moments(x).var, Seq(normal).forward_moments(x).var)


def test_plumbing():
    x = torch.randn(5, 9, generator=torch.Generator().manual_seed(4))
    net = titanic()
    assert not bnn_nn.moment_estimator_layers_enabled()                             # off by default: the refusals as they were
    with pytest.raises(ops.BnnHipError, match="predictive_moments: MCDropoutLinear is not supported; moment propagation supports"):
        net.predictive_moments(x)
    with pytest.raises(ops.BnnHipError, match="forward_moments: MCDropoutLinear has no moment backward"):
        net.forward_moments(x)
    assert "MCDropoutLinear" not in bnn_nn.container._moments_supported()
    bnn_nn.moment_estimator_layers()
    assert bnn_nn.moment_estimator_layers_enabled() and "MCDropoutLinear" in bnn_nn.container._moments_supported()
    # the bookkeeping: set, idempotent, cleared
    l0, l2 = net.layers[0], net.layers[2]
    assert l0.__dict__["_moment_act"] == ('elu', 1.0) and l2.__dict__["_moment_act"] == 'softmax'
    assert bnn_nn.moment_activations(net) == 0 and l0.__dict__["_moment_act"] == ('elu', 1.0)
    want = net.predictive_moments(x)
    net.layers[1] = torch.nn.Identity()
    bnn_nn.moment_activations(net)
    assert "_moment_act" not in l0.__dict__
    assert not torch.equal(net.predictive_moments(x).mean, want.mean)               # the identity behind the first layer now
    # sample=False applies no dropout
    lone = Seq(MCDropoutLinear(9, 4, drop_prob=0.5))
    with _mc.MomentContext():
        off = lone.layers[0](x, sample=False)
    assert off.var is None and torch.allclose(off.mean.float(), lone.layers[0].linear(x), atol=1e-6)
    # a stale Sequential: the layer still believes a softmax is behind it
    stale = titanic()
    stale.layers[3] = bnn_nn.MomentReLU()
    with pytest.raises(ops.BnnHipError, match="call nn.moment_activations again"):
        stale.predictive_moments(x)
    del stale.layers[3]
    with pytest.raises(ops.BnnHipError, match="no such softmax followed"):
        stale.predictive_moments(x)
    # ... or an activation that is not the one behind it any more
    stale = titanic()
    stale.layers[1] = bnn_nn.MomentReLU()
    with pytest.raises(ops.BnnHipError, match="call nn.moment_activations again"):
        stale.predictive_moments(x)
    # a hand-placed twin the layer was never told about: the mask went through the identity, the twin must not moment-match that
    for twin in (bnn_nn.MomentReLU(), bnn_nn.MomentELU()):
        by_hand = Seq(MCDropoutLinear(9, 6, drop_prob=0.3), twin)
        with pytest.raises(ops.BnnHipError, match="'identity' into its launch.*call nn.moment_activations again"):
            by_hand.predictive_moments(x)
        by_hand = Seq(MCDropoutLinear(9, 6, drop_prob=0.3), torch.nn.Flatten(), twin)                 # ... nor behind a reshape
        with pytest.raises(ops.BnnHipError, match="call nn.moment_activations again"):
            by_hand.predictive_moments(x)
        bnn_nn.moment_activations(by_hand.layers)
        with pytest.raises(ops.BnnHipError, match="call nn.moment_activations again"):                # (not adjacent: not paired)
            by_hand.predictive_moments(x)
        paired = Seq(MCDropoutLinear(9, 6, drop_prob=0.3), twin)
        bnn_nn.moment_activations(paired)
        assert paired.predictive_moments(x).var is not None
    # refusals by name
    net = titanic()
    with pytest.raises(ops.BnnHipError, match="covariance=True is not covered at a MCDropoutLinear head"):
        net.predictive_moments(x, covariance=True)
    with pytest.raises(ops.BnnHipError, match="covariance=True is not covered at a FlipoutNormalLinear head"):
        Seq(NormalLinear(9, 6), FlipoutNormalLinear(6, 3)).predictive_moments(x, covariance=True)
    with pytest.raises(ops.BnnHipError, match="PRE-dropout moments of an MC-dropout head"):
        net.predictive_regression(x, outputs='values', propagation='moments')
    net.layers[0].drop_prob = 1.5
    with pytest.raises(ValueError, match="dropout probability"):
        net.predictive_moments(x)


def test_entry_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one = ctypes.c_void_p(16)
    fwd, bwd = lib.bnn_moments_dropout, lib.bnn_moments_dropout_backward
    assert fwd(None, one, one, one, 4, 0.5, 0, 0.0, None) == -1 and b"NULL" in lib.bnn_last_error()
    assert fwd(one, None, one, None, 4, 0.5, 0, 0.0, None) == -1
    assert bwd(one, one, one, one, one, None, 4, 0.5, 0, 0.0, None) == -1              # a variance without room for its gradient
    for p in (-0.1, 1.5, float("nan")):
        assert fwd(one, one, one, one, 4, p, 0, 0.0, None) == -5
        assert lib.bnn_last_error().startswith(b"bnn_moments_dropout: p must lie")
        assert bwd(one, one, one, one, one, one, 4, p, 0, 0.0, None) == -5
        assert lib.bnn_last_error().startswith(b"bnn_moments_dropout_backward: p must lie")
    for act in (2, 3, 9, -1):
        assert fwd(one, one, one, one, 4, 0.5, act, 1.0, None) == -5 and b"act must be" in lib.bnn_last_error()
        assert bwd(one, one, one, one, one, one, 4, 0.5, act, 1.0, None) == -5
    assert fwd(one, one, one, one, -1, 0.5, 0, 0.0, None) == -5 and b"n must be" in lib.bnn_last_error()
    assert bwd(one, one, one, one, one, one, -1, 0.5, 0, 0.0, None) == -5
    assert fwd(one, one, one, one, 4, 0.5, _lib.FLAG_ELU, -1.0, None) == -5 and b"alpha" in lib.bnn_last_error()
    two = ctypes.c_void_p(18)
    assert fwd(two, one, one, one, 4, 0.5, 0, 0.0, None) == -4 and bwd(one, one, one, two, one, one, 4, 0.5, 0, 0.0, None) == -4
    assert fwd(one, None, one, one, 0, 0.5, 0, 0.0, None) == 0 and bwd(one, None, one, one, one, None, 0, 0.5, 0, 0.0, None) == 0
    assert lib.bnn_launch_count() == n0
    m = torch.zeros(3)
    with pytest.raises(ops.BnnHipError):
        ops.moments_dropout(ops.Moments(m, m), 0.5)                                 # a CPU tensor: no fallback
    with pytest.raises(ops.BnnHipError):
        ops.moments_conv_affine(ops.Moments(torch.zeros(1, 1, 4), torch.zeros(1, 1, 4)), torch.zeros(1, 1, 3), None, (1,), (0,), (1,))


def test_dropout_kernels_use_no_scratch():
    """The three instantiations of each kernel (identity, ReLU, ELU) keep everything in registers: no spill, no private segment."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    mine = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn\d+k_moments_dropout(_bwd)?ILi\d+EEEv", n)}
    assert len(mine) == 6, sorted(mine)
    for n, f in sorted(mine.items()):
        print(n, f)
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0 and int(f["private_segment_fixed_size"]) == 0, (n, f)


def masked_share(pre, p, what):
    """The share of masked (exactly zero) drawn logits against p, within 5 binomial standard errors."""
    n = pre.numel()
    share = (pre == 0).double().mean().item()
    z = abs(share - p) / math.sqrt(p * (1 - p) / n)
    print("%s: %.4f of %d drawn logits masked (p = %g): %.2f binomial standard errors" % (what, share, n, p, z))
    assert z <= 5, (share, p, z)


def capture_logits(monkeypatch):
    """The drawn (and masked) logits on their way into the tail's softmax: every argument torch.softmax is called with from here on,
    in call order (the tail calls it once per pass)."""
    seen, softmax = [], torch.softmax

    def recording(ys, *args, **kwargs):
        seen.append(ys.detach().clone())
        return softmax(ys, *args, **kwargs)

    monkeypatch.setattr(torch, "softmax", recording)
    return seen


def test_tail_on_the_cpu(monkeypatch):
    p = 0.2
    net = titanic(24, p)
    x = torch.randn(5, 9, generator=torch.Generator().manual_seed(4))
    bnn_nn.moment_estimator_layers()
    seen = capture_logits(monkeypatch)
    torch.manual_seed(77)
    u = net.predictive_uncertainty(x, inputs='probs', propagation='moments', samples=4000)
    assert (u.mean.sum(-1) - 1).abs().max() <= 1e-6
    assert len(seen) == 1 and seen[0].shape == (4000, 5, 2)
    masked_share(seen[0], p, "CPU tail")
    torch.manual_seed(78)
    ref = net.predictive_uncertainty(x, inputs='probs', samples=1000)                   # the sampler it replaces (reported only)
    print("CPU tail (S = 4000) against the sampler at S = 1000: worst |total - total_s| %.4f, |epistemic - epistemic_s| %.4f, |mean - mean_s| %.4f"
          % ((u.total - ref.total).abs().max().item(), (u.epistemic - ref.epistemic).abs().max().item(),
             (u.mean - ref.mean).abs().max().item()))
    s = net.predictive_score(x, torch.tensor([0, 1, 1, 0, 1]), inputs='probs', propagation='moments', samples=16)
    assert torch.isfinite(s.nll).all()
    net.train()
    ys = net.sample_moments(net.forward_moments(x), 8)                                  # tracked on the CPU
    F.nll_loss(torch.log(ys.reshape(-1, 2) + 1e-30), torch.tensor([0, 1, 1, 0, 1]).repeat(8)).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in net.parameters())


# ================================================================================================ GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


def p32(p):
    """p as the device receives it"""
    return float(torch.tensor(p, dtype=torch.float32))


def grid_inputs(v):
    """fp32 (m, v) on the alpha grid; v None: a deterministic input, v == 0: zeros (m = alpha in both)"""
    s = math.sqrt(v) if v else 1.0
    m32 = (ALPHA * s).float()
    return m32, None if v is None else torch.full_like(m32, v)


@gpu
@pytest.mark.parametrize("act", ACTS, ids=act_name)
def test_forward_kernel_matches_the_twin_on_the_grid(dev, act):
    worst_m = worst_v = 0.0
    for p in (0.0,) + GRID_P + (1.0,):
        for v in ELU_GRID_V + (0.0, None):
            m32, v32 = grid_inputs(v)
            ref = ops.moments_dropout_f64(ops.Moments(m32, v32), p32(p), act)
            got = ops.moments_dropout(ops.Moments(m32.to(dev), None if v32 is None else v32.to(dev)), p, act)
            assert got.mean.dtype == got.var.dtype == torch.float32 and got.var.shape == m32.shape
            r2 = m32.double() ** 2 + (v or 0.0)
            dm = ((got.mean.double().cpu() - ref.mean).abs() / r2.sqrt().clamp_min(TINY)).max().item()
            dv = ((got.var.double().cpu() - ref.var).abs() / r2.clamp_min(TINY)).max().item()
            worst_m, worst_v = max(worst_m, dm), max(worst_v, dv)
            print("moments_dropout %s p = %g v = %s: worst mean deviation %.3e r, worst variance deviation %.3e r^2"
                  % (act_name(act), p, v, dm, dv))
            assert torch.isfinite(got.mean).all() and torch.isfinite(got.var).all() and (got.var >= 0).all()
            assert dm <= DROPOUT_TOL and dv <= DROPOUT_TOL, (act, p, v, dm, dv)
            if p == 0.0 and v:                                                       # the dropout-free limit: the activation's bits
                pre = ops.Moments(m32.to(dev), v32.to(dev))
                alone = pre if act is None else ops.moments_relu(pre) if act == 'relu' else ops.moments_elu(pre, act[1])
                assert same_bits(got.mean, alone.mean) and same_bits(got.var, alone.var)
            if p == 1.0:
                assert not got.mean.any() and not got.var.any()
    print("moments_dropout %s: worst mean deviation %.3e r, worst variance deviation %.3e r^2 (bound %.1e)"
          % (act_name(act), worst_m, worst_v, DROPOUT_TOL))
    nan = ops.moments_dropout(ops.Moments(torch.tensor([1.0, -1.0], device=dev), torch.tensor([float("nan")] * 2, device=dev)), 0.5, act)
    assert nan.mean.shape == (2,)                                                    # a NaN variance takes the limit branches
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("act", ACTS, ids=act_name)
def test_backward_kernel_matches_float64_autograd(dev, act):
    """Against float64 autograd of the tracked twin on the fp32 inputs; each gradient within DROPOUT_TOL + 4 alpha^2 U (the file's
    header derives it) of the magnitude of its own two terms (|g_mean'| |d mean'/d x| + |g_var'| |d var'/d x|, from the formula
    twin on unit gradients), beside TINY; and on |alpha| <= 3, where that allowance is nothing, within DROPOUT_TOL alone of the
    plain magnitudes.  The grid is the forward test's: v = 0 as a tensor, var None and p in {0, 1} included."""
    g = torch.Generator().manual_seed(41)
    worst, bulk = [0.0, 0.0], [0.0, 0.0]
    for p in (0.0,) + GRID_P + (1.0,):
        for v in ELU_GRID_V + (0.0, None):
            m32, v32 = grid_inputs(v)
            gm, gv = torch.randn(m32.shape, generator=g), torch.randn(m32.shape, generator=g)
            pp = p32(p)
            tol = DROPOUT_TOL + (4 * U * ALPHA ** 2 if v else 0.0)
            kappa = 1.0
            if v and act == 'relu':                                                  # the fp32 mean's own cancellation (header)
                cdf, pdf = 0.5 * torch.special.erfc(-ALPHA / math.sqrt(2.0)), torch.exp(-0.5 * ALPHA * ALPHA) / math.sqrt(2.0 * math.pi)
                kappa = (ALPHA.abs() * cdf + pdf) / (ALPHA * cdf + pdf)
            if v:
                m64, v64 = m32.double().requires_grad_(), v32.double().requires_grad_()
                out = ops.moments_dropout_f64(ops.Moments(m64, v64), pp, act, track=True)
                want = torch.autograd.grad([out.mean, out.var], [m64, v64], [gm.double(), gv.double()])
            else:
                # a deterministic input, as a zero variance (g_v through the v == 0 limit branches) or as None: the formula twin with
                # the stated conventions (autograd divides by sqrt(0) there, and torch's own elu backward takes the other side at 0;
                # test_backward_twin_gradcheck holds the twin's v == 0 branch to the closed form)
                want = ops.moments_dropout_backward_f64(ops.Moments(m32, v32), gm, gv, pp, act)[:2 if v32 is not None else 1]
            one, zero = torch.ones_like(gm), torch.zeros_like(gm)
            jm = ops.moments_dropout_backward_f64(ops.Moments(m32, v32), one, zero, pp, act)
            jv = ops.moments_dropout_backward_f64(ops.Moments(m32, v32), zero, one, pp, act)
            a = m32.to(dev).requires_grad_()
            b = None if v32 is None else v32.to(dev).requires_grad_()
            res = ops.moments_dropout(ops.Moments(a, b), p, act, track=True)
            assert res.mean.requires_grad
            got = torch.autograd.grad([res.mean, res.var], [a] + ([] if b is None else [b]), [gm.to(dev), gv.to(dev)])
            for i, (gt, ref) in enumerate(zip(got, want)):
                mag = gm.double().abs() * jm[i].abs() + kappa * gv.double().abs() * jv[i].abs()
                excess = ((gt.double().cpu() - ref).abs() - TINY).clamp_min(0)
                w = (excess / (tol * mag).clamp_min(1e-300))[mag > 0].max().item() if (mag > 0).any() else 0.0
                worst[i] = max(worst[i], w)
                # the bulk on its own: the project's 1e-5 of the plain term magnitudes, no tail allowance and no kappa
                plain = gm.double().abs() * jm[i].abs() + gv.double().abs() * jv[i].abs()
                sel = BULK & (plain > 0)
                wb = (excess / (DROPOUT_TOL * plain).clamp_min(1e-300))[sel].max().item() if sel.any() else 0.0
                bulk[i] = max(bulk[i], wb)
                print("moments_dropout backward %s p = %g v = %s %s: worst error / bound %.3f, |alpha| <= 3 against 1e-5 alone %.3f"
                      % (act_name(act), p, v, "g_m g_v".split()[i], w, wb))
                assert bool(torch.isfinite(gt).all()) and bool((excess <= tol * mag).all()), (act, p, v, i, w)
                assert bool((excess <= DROPOUT_TOL * plain)[BULK].all()), (act, p, v, i, wb)
            if p == 1.0:
                assert not any(t.any() for t in got)
    print("moments_dropout backward %s: worst error / bound: g_m %.3f, g_v %.3f; |alpha| <= 3 against 1e-5 alone: g_m %.3f, g_v %.3f"
          % (act_name(act), worst[0], worst[1], bulk[0], bulk[1]))
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 772])
def test_sizes_in_place_and_addresses(dev, n):
    """More than one block (772 = 3 x 256 + 4), the block edge, one element; in place; every operand 4 and 8 bytes off a 16-byte
    boundary (NaN guards around the inputs, sentinels around the outputs): the same bits."""
    g = torch.Generator().manual_seed(n)
    m, v = torch.randn(n, generator=g).to(dev), torch.rand(n, generator=g).to(dev)
    gm, gv = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    lib, st = _lib.load(), ops.stream_ptr(dev)
    P = lambda t: None if t is None else t.data_ptr()                                # noqa: E731
    for act, flag, alpha in ((None, 0, 0.0), ('relu', _lib.FLAG_RELU, 0.0), (('elu', 0.5), _lib.FLAG_ELU, 0.5)):
        for var in (v, None):
            want = ops.moments_dropout(ops.Moments(m, var), 0.3, act)
            ref = ops.moments_dropout_f64(ops.Moments(m.cpu(), None if var is None else var.cpu()), p32(0.3), act)
            r2 = m.double().cpu() ** 2 + (0 if var is None else var.double().cpu())
            assert ((want.mean.double().cpu() - ref.mean).abs() <= DROPOUT_TOL * r2.sqrt()).all()
            assert ((want.var.double().cpu() - ref.var).abs() <= DROPOUT_TOL * r2).all()
            m2, v2 = m.clone(), v.clone()                                            # in place (a deterministic input: out_v apart)
            assert lib.bnn_moments_dropout(P(m2), None if var is None else P(v2), P(m2), P(v2), n, 0.3, flag, alpha, st) == 0
            assert same_bits(m2, want.mean) and same_bits(v2, want.var)
            wg = torch.empty_like(m), torch.empty_like(m)
            assert lib.bnn_moments_dropout_backward(P(m), P(var), P(gm), P(gv), P(wg[0]), None if var is None else P(wg[1]), n, 0.3, flag,
                                                    alpha, st) == 0
            g2 = gm.clone(), gv.clone()                                              # in place on the gradients
            assert lib.bnn_moments_dropout_backward(P(m), P(var), P(g2[0]), P(g2[1]), P(g2[0]), None if var is None else P(g2[1]), n, 0.3,
                                                    flag, alpha, st) == 0
            assert same_bits(g2[0], wg[0]) and (var is None or same_bits(g2[1], wg[1]))
            for off in (4, 8):
                other = 12 - off
                a, b = offset_view(m, off), None if var is None else offset_view(var, other)
                om, ov = output_view((n,), torch.float32, dev, other), output_view((n,), torch.float32, dev, off)
                assert lib.bnn_moments_dropout(P(a), P(b), P(om), P(ov), n, 0.3, flag, alpha, st) == 0
                ga, gb = offset_view(gm, other), offset_view(gv, off)
                o1, o2 = output_view((n,), torch.float32, dev, off), output_view((n,), torch.float32, dev, other)
                assert lib.bnn_moments_dropout_backward(P(a), P(b), P(ga), P(gb), P(o1), None if var is None else P(o2), n, 0.3, flag,
                                                        alpha, st) == 0
                torch.cuda.synchronize()
                assert all(guards_intact(t) for t in (om, ov, o1, o2))
                assert same_bits(om, want.mean) and same_bits(ov, want.var) and same_bits(o1, wg[0])
                assert var is None or same_bits(o2, wg[1])
    _lib.check_device(dev)


def affine_ref(mom, w, b, mode):
    """float64 reference of ONE ops.moments_affine call on moments that carry a variance, with K16's bound (linear_ref's rule at
    sigma^2 = 0) -> (m, v, bound_m, bound_v).  mom: CPU Moments holding the call's own fp32 input."""
    K = w.shape[1]
    if mode == "f32":
        r = ops.moments_affine_f64(mom, w, b)
        return r.mean, r.var, scaled_bound(r.mean), scaled_bound(r.var)
    p_w, p_w2 = rne_bf16(w), rne_bf16((w.double() ** 2).float())
    q_m = rne_bf16(mom.mean)
    m, a = q_m @ p_w.t() + b.double(), q_m.abs() @ p_w.abs().t() + b.double().abs()
    v = rne_bf16(mom.var) @ p_w2.t()
    return m, v, gamma(K + 1) * a + 1e-300, gamma(2 * K + 1) * v + 1e-300


# forward: linear, dropout + ELU, affine; training adds the sampling launch, the masks, softmax / nll and the 5 backward stages.
# bf16 mode: only the second layer's contraction reads bf16 planes (the first layer's deterministic input takes the layer's own
# fp32 linear): forward R = 256, input gradient R = 2, weight gradient R = B = 8.
TITANIC_TOL = {"f32": 11e-5, "bf16": 11e-5 + 2.0 ** -8 * (math.sqrt(256) + math.sqrt(2) + math.sqrt(8))}


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_titanic_net_on_the_device(dev, mode, monkeypatch):
    """9 -> 256 -> 2, B = 8: predictive_moments is the chain of its ops calls bit for bit, every stage within its bound of float64 on
    the DEVICE's own input of that stage; forward_moments + sample_moments gradients of every parameter against CPU float64
    autograd on the recovered eps and the masks read back from the drawn samples."""
    p, B, S = 0.2, 8, 8
    bnn.set_compute(mode)
    bnn_nn.moment_estimator_layers()
    cpu = titanic(256, p, seed=12)
    net = titanic(256, p, seed=12).to(dev)
    g = torch.Generator().manual_seed(13)
    x, t = torch.randn(B, 9, generator=g), torch.randint(0, 2, (B,), generator=g)
    xd = x.to(dev)
    e0 = _rng.default_generator.epoch_host
    mom = net.predictive_moments(xd)
    assert _rng.default_generator.epoch_host == e0 and mom.link == 'softmax' and mom.dropout == p
    l1, l2 = net.layers[0].linear, net.layers[2].linear
    pre1 = l1(xd).detach()
    c1 = cpu.layers[0].linear
    z64 = (x.double() @ c1.weight.double().t() + c1.bias.double()).detach()
    assert_within(pre1, z64, scaled_bound(z64), "titanic layer 1 " + mode)
    h = ops.moments_dropout(ops.Moments(pre1), p, ('elu', 1.0))
    h64 = ops.moments_dropout_f64(ops.Moments(pre1.cpu()), p32(p), ('elu', 1.0))
    r2 = pre1.double().cpu() ** 2
    assert_within(h.mean, h64.mean, DROPOUT_TOL * r2.sqrt() + TINY, "titanic hidden mean " + mode)
    assert_within(h.var, h64.var, DROPOUT_TOL * r2 + TINY, "titanic hidden var " + mode)
    out = ops.moments_affine(h, l2.weight, l2.bias, compute=mode)
    m, v, bm, bv = affine_ref(ops.Moments(h.mean.cpu(), h.var.cpu()), l2.weight.detach().cpu(), l2.bias.detach().cpu(), mode)
    assert_within(out.mean, m, bm, "titanic logits m " + mode)
    assert_within(out.var, v, bv, "titanic logits v " + mode)
    assert torch.equal(out.mean, mom.mean) and torch.equal(out.var, mom.var)
    # training without sampling
    net.train()
    tr = net.forward_moments(xd)
    assert torch.equal(tr.mean, mom.mean) and torch.equal(tr.var, mom.var) and tr.mean.requires_grad and tr.dropout == p
    seen = capture_logits(monkeypatch)
    ps = net.sample_moments(tr, S)
    grads = torch.autograd.grad(F.nll_loss(torch.log(ps.reshape(-1, 2)), t.to(dev).repeat(S), reduction="sum"), list(net.parameters()))
    ys = ops.moments_sample(ops.Moments(tr.mean.detach(), tr.var.detach()), net.moment_key, S)
    eps = recovered_eps(ys, tr.mean, tr.var)
    keep = (seen[0] != 0).double().cpu()                                             # the masks, read back from the drawn logits
    assert torch.equal(seen[0] != 0, ops.mc_dropout(ys.reshape(S * B, 2), p, net.moment_mask_key, False).reshape(S, B, 2) != 0)
    net64 = cpu.double()
    m64 = net64.forward_moments(x.double())
    y64 = torch.softmax(keep * (m64.mean + torch.sqrt(m64.var + 1e-16) * eps) / (1.0 - p32(p)), -1)
    want = torch.autograd.grad(F.nll_loss(torch.log(y64.reshape(-1, 2)), t.repeat(S), reduction="sum"), list(net64.parameters()))
    assert len(grads) == len(want) == 4
    for (n, _), a, w in zip(net.named_parameters(), grads, want):
        assert_within(a, w, scaled_bound(w, TITANIC_TOL[mode]), "%s titanic %s" % (n, mode))
    _lib.check_device(dev)


def conv_net(nd, seed):
    torch.manual_seed(seed)
    if nd == 2:
        mods = [NormalConv2d(4, 4, 3, padding=1), MCDropoutConv2d(4, 4, 3, padding=1, drop_prob=.3), torch.nn.ELU(),
                torch.nn.MaxPool2d(2), torch.nn.Flatten(), MCDropoutLinear(36, 3, drop_prob=.3), torch.nn.Softmax(dim=-1)]
    else:
        norm, drop = (bnn_nn.NormalConv1d, MCDropoutConv1d) if nd == 1 else (bnn_nn.NormalConv3d, MCDropoutConv3d)
        mods = [norm(2, 2, 3, padding=1), drop(2, 3, 3, padding=1, drop_prob=.3), torch.nn.ReLU()]
    net = Seq(*mods)
    bnn_nn.moment_activations(net)
    return net


def conv_recursion64(net, x):
    """The float64 recursion of conv_net through the ops twins."""
    mods = list(net.layers)
    c0, c1 = mods[0], mods[1]
    mom = ops.moments_convNd_f64(ops.Moments(x), c0.weight.mean, c0.weight.scale, c0.bias.mean, c0.bias.scale, c0.stride, c0.padding,
                                 c0.dilation, c0.groups)
    mom = ops.moments_conv_affine_f64(mom, c1.conv.weight, c1.conv.bias, c1.conv.stride, c1.conv.padding, c1.conv.dilation, c1.conv.groups)
    if len(mods) == 3:
        return ops.moments_dropout_f64(mom, c1.drop_prob, 'relu')
    mom = ops.moments_dropout_f64(mom, c1.drop_prob, ('elu', 1.0))
    mom = ops.moments_pool_f64(mom, 'max', 2).flatten(1)
    return ops.moments_affine_f64(mom, mods[5].linear.weight, mods[5].linear.bias)


# conv, conv-affine, dropout + ELU, max pool, affine: 5 stages forward; the sampling launch, the masks, softmax / nll and 7 backward
# stages: 15.  bf16: NormalConv2d 4 -> 4, 3 x 3 on 6 x 6 (P = 36): forward R = 36, weight gradient 3 x 36; the dropout conv the same
# and its input gradient 36; the head 36 -> 3 at B = 3: 36, 3, 3.
CONV_R_FWD = (36, 36, 36)
CONV_R = CONV_R_FWD + (108, 108, 36, 3, 3)
CONV_FWD_TOL = {"f32": 5e-5, "bf16": 5e-5 + 2.0 ** -8 * sum(math.sqrt(r) for r in CONV_R_FWD)}
CONV_TOL = {"f32": 15e-5, "bf16": 15e-5 + 2.0 ** -8 * sum(math.sqrt(r) for r in CONV_R)}


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_conv_net_on_the_device(dev, mode, monkeypatch):
    """NormalConv2d -> MCDropoutConv2d(p = .3) -> ELU -> MaxPool2d(2) -> Flatten -> MCDropoutLinear(36, 3) -> Softmax on (3, 4, 6, 6):
    the dropout conv sees a variance.  predictive_moments against the float64 recursion; with nn.conv_moment_training the
    gradients of every parameter against CPU float64 autograd."""
    B, S, p = 3, 8, 0.3
    bnn.set_compute(mode)
    bnn_nn.moment_estimator_layers()
    cpu, net = conv_net(2, 21), conv_net(2, 21).to(dev)
    g = torch.Generator().manual_seed(22)
    x, t = torch.randn(B, 4, 6, 6, generator=g), torch.randint(0, 3, (B,), generator=g)
    xd = x.to(dev)
    ref = conv_recursion64(cpu, x)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    got = net.predictive_moments(xd)
    torch.cuda.synchronize()
    # operand + conv launch, the conv-affine launch, ONE dropout launch (none for the ELU twin), the pool, the head's affine launch
    assert lib.bnn_launch_count() == n0 + 6
    assert got.link == 'softmax' and got.dropout == p and got.mean.shape == (B, 3)
    assert_within(got.mean, ref.mean, scaled_bound(ref.mean, CONV_FWD_TOL[mode]), "conv net logits m " + mode)
    assert_within(got.var, ref.var, scaled_bound(ref.var, CONV_FWD_TOL[mode]), "conv net logits v " + mode)
    with pytest.raises(ops.BnnHipError, match="has no moment backward"):
        net.forward_moments(xd)
    bnn_nn.conv_moment_training()
    net.train()
    tr = net.forward_moments(xd)
    assert torch.equal(tr.mean, got.mean) and torch.equal(tr.var, got.var)
    seen = capture_logits(monkeypatch)
    ps = net.sample_moments(tr, S)
    grads = torch.autograd.grad(F.nll_loss(torch.log(ps.reshape(-1, 3)), t.to(dev).repeat(S), reduction="sum"), list(net.parameters()))
    ys = ops.moments_sample(ops.Moments(tr.mean.detach(), tr.var.detach()), net.moment_key, S)
    eps = recovered_eps(ys, tr.mean, tr.var)
    keep = (seen[0] != 0).double().cpu()
    net64 = cpu.double()
    m64 = net64.forward_moments(x.double())
    y64 = torch.softmax(keep * (m64.mean + torch.sqrt(m64.var + 1e-16) * eps) / (1.0 - p32(p)), -1)
    want = torch.autograd.grad(F.nll_loss(torch.log(y64.reshape(-1, 3)), t.repeat(S), reduction="sum"), list(net64.parameters()))
    assert len(grads) == len(want) == 8
    for (n, _), a, w in zip(net.named_parameters(), grads, want):
        assert_within(a, w, scaled_bound(w, CONV_TOL[mode]), "%s conv net %s" % (n, mode))
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("nd", [1, 3])
def test_conv_1d_and_3d_once(dev, nd):
    """NormalConvNd -> MCDropoutConvNd -> ReLU on (2, 2, 5[, 5, 5]): forward and (nn.conv_moment_training) gradients against float64;
    three forward stages, four backward ones."""
    bnn_nn.moment_estimator_layers()
    bnn_nn.conv_moment_training()
    cpu, net = conv_net(nd, 30 + nd), conv_net(nd, 30 + nd).to(dev)
    g = torch.Generator().manual_seed(33)
    x = torch.randn((2, 2) + (5,) * nd, generator=g)
    ref = conv_recursion64(cpu, x)
    got = net.predictive_moments(x.to(dev))
    assert got.link is None and got.dropout is None
    assert_within(got.mean, ref.mean, scaled_bound(ref.mean, 3e-5), "conv%dd m" % nd)
    assert_within(got.var, ref.var, scaled_bound(ref.var, 3e-5), "conv%dd v" % nd)
    G_m, G_v = torch.randn(ref.mean.shape, generator=g), torch.randn(ref.mean.shape, generator=g)
    tr = net.forward_moments(x.to(dev))
    grads = torch.autograd.grad([tr.mean, tr.var], list(net.parameters()), [G_m.to(dev), G_v.to(dev)])
    t64 = cpu.double().forward_moments(x.double())
    want = torch.autograd.grad([t64.mean, t64.var], list(cpu.parameters()), [G_m.double(), G_v.double()])
    for (n, _), a, w in zip(net.named_parameters(), grads, want):
        assert_within(a, w, scaled_bound(w, 7e-5), "%s conv%dd" % (n, nd))
    _lib.check_device(dev)


@gpu
def test_launches_and_graph_capture(dev):
    """One bnn_moments_dropout launch per MC-dropout layer and none for the twin behind it; the forward and the backward in a
    captured graph replay to the eager bits."""
    bnn_nn.moment_estimator_layers()
    lib = _lib.load()
    x = torch.randn(8, 9, device=dev)
    for softmax, launches in ((False, 3), (True, 2)):          # dropout + ELU, the second layer's affine launch (, its own dropout)
        net = titanic(64, 0.2, softmax=softmax).to(dev)
        net.predictive_moments(x)
        torch.cuda.synchronize()
        n0 = lib.bnn_launch_count()
        net.predictive_moments(x)
        torch.cuda.synchronize()
        assert lib.bnn_launch_count() == n0 + launches, (softmax, lib.bnn_launch_count() - n0)
    g = torch.Generator().manual_seed(51)
    m, v = torch.randn(772, generator=g).to(dev), torch.rand(772, generator=g).to(dev)
    G_m, G_v = torch.randn(772, generator=g).to(dev), torch.randn(772, generator=g).to(dev)
    a, b = m.clone().requires_grad_(), v.clone().requires_grad_()

    def step():
        out = ops.moments_dropout(ops.Moments(a, b), 0.3, ('elu', 1.0), track=True)
        return [out.mean, out.var] + list(torch.autograd.grad([out.mean, out.var], [a, b], [G_m, G_v]))

    want = [t.detach().clone() for t in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                  # warm up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = step()
    for _ in range(2):
        for t in got:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x_.detach(), y_) for x_, y_ in zip(got, want))
    _lib.check_device(dev)


@gpu
def test_tail_on_the_device(dev, monkeypatch):
    """predictive_uncertainty / predictive_score with propagation='moments' on an MC-dropout head: the same seed and epoch give the
    same bits, sample0 shifts the samples as the mask contract says, the masked share is p."""
    p, S = 0.2, 512
    bnn_nn.moment_estimator_layers()
    net = titanic(64, p).to(dev)
    x = torch.randn(16, 9, generator=torch.Generator().manual_seed(4)).to(dev)
    seen = capture_logits(monkeypatch)
    bnn.manual_seed(99)
    u = net.predictive_uncertainty(x, inputs='probs', propagation='moments', samples=S)
    k, mk = net.moment_key, net.moment_mask_key
    assert (u.mean.sum(-1) - 1).abs().max() <= 1e-5 and torch.isfinite(u.total).all()
    assert (mk.seed, mk.epoch_host, mk.sample0, mk.nsamples, mk.gen) == (k.seed, k.epoch_host, k.sample0, k.nsamples, k.gen)
    assert mk.stream != k.stream
    masked_share(seen[0], p, "device tail")
    bnn.manual_seed(99)
    u2 = net.predictive_uncertainty(x, inputs='probs', propagation='moments', samples=S)
    assert torch.equal(u.mean, u2.mean) and torch.equal(u.total, u2.total) and torch.equal(seen[0], seen[1])
    bnn.manual_seed(99)
    net.predictive_uncertainty(x, inputs='probs', propagation='moments', samples=S - 3, sample0=3)
    assert net.moment_mask_key.sample0 == 3 and torch.equal(seen[2], seen[0][3:])        # sample s of the key, wherever the call starts
    s = net.predictive_score(x, torch.randint(0, 2, (16,), device=dev), inputs='probs', propagation='moments', samples=32)
    assert torch.isfinite(s.nll).all()
    bnn.manual_seed(100)
    ref = net.predictive_uncertainty(x, inputs='probs', samples=S)
    print("device tail against the sampler at S = %d: worst |total - total_s| %.4f, |epistemic - epistemic_s| %.4f"
          % (S, (u.total - ref.total).abs().max().item(), (u.epistemic - ref.epistemic).abs().max().item()))
    _lib.check_device(dev)
