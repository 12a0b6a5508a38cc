"""Sampling-free passes through pooling and BatchNorm (K20): the moment-matched maximum of two Gaussians (Clark 1961)

    theta^2 = v1 + v2,  d = m1 - m2,  alpha = d / theta
    mean' = m1 Phi + m2 Phi_c + theta phi
    var'  = v1 Phi + v2 Phi_c + d^2 Phi Phi_c + d theta phi (Phi_c - Phi) - theta^2 phi^2

folded over a max-pooling window (offsets ascending, padded positions skipped), average pooling (sum m / n, sum v / n^2) and
eval-mode BatchNorm (a = gamma / sqrt(running_var + eps), m' = a (m - running_mean) + beta, v' = a^2 v); their nn twins and the
nn.moment_activations rewrite.  CPU tests: the pair step against quadrature, the ReLU identity, the limits, average pooling and
BatchNorm against torch, gradcheck, the modules, a LeNet-shaped net, the argument checks, the built code object, agreement with
sampling.  GPU tests: forward and backward against float64, BatchNorm, alignment, graph capture, the LeNet-shaped net.

Bounds of the pooling launches (bnn_moments_pool3d_forward / _backward against ops.moments_pool_f64 and its float64 autograd on the
fp32 inputs).  The device folds in fp64 and rounds once per result, so what is measured is that one fp32 rounding and the
difference between the host's and the device's erfc / exp.  Forward, in the ELU test's units: the mean in units of sqrt(var'_ref)
plus half an fp32 ulp of the result, the variance in units of var'_ref; an output whose var'_ref is 0 must be exact.  Below the
smallest normal fp32 number (2^-126) the format has no relative precision: that much is allowed absolutely.  Measured on the
MI355X over POOL_CASES x (max, avg) (test_pool_forward_matches_float64 prints them): the mean never left its half ulp (worst
deviation beyond it: 0 sqrt(var') on all twelve cases); worst variance deviation 5.930e-8 var' (blocks, avg; max: 5.773e-8) -- the
fp32 rounding, 2^-24 = 5.96e-8.  Backward (test_pool_backward_matches_float64_autograd), in units of |ref| per gradient element
after the TINY floor and, for overlapping windows, the atomics' term below: worst 5.892e-8 (blocks, max, g_m; g_v 5.851e-8;
the average pool and the overlapping cases: 0 beyond their terms).  The constants are 4 x the measured worst, the margin of the
ELU launch's constants, which covers libm differences between host and device: 2.38e-7 and 2.36e-7.  For the mean 4 x 0 would
leave nothing for an fp64 difference between two libms that moves a result across an fp32 rounding boundary (the allowance
2^-24 |mean| is exactly half an ulp for a mean just above a power of two), so its constant is 4 x 2^-24 = 2.39e-7 of sqrt(var'):
what one more fp32 rounding of a quantity of that size costs.  All are below 1e-5, the project's parity cap.  Overlapping windows
add their contributions with fp32 atomics: n contributions, each rounded to fp32 and added in any order, are within gamma_n
sum |contribution| of their exact sum, n <= prod ceil(extent / stride).
"""
import ctypes
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd import nn as bnn_nn
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, NormalConv2d, NormalLinear

from alignment import guards_intact, offset_view, output_view, same_bits
from bf16ref import gamma
from test_flipout_mc import _code_object_notes
from test_lrt_device import U, assert_within, scaled_bound
from test_moment_backward import recovered_eps
from test_moment_conv_backward import e2e_step, set_posteriors, switch       # noqa: F401  (switch: a fixture)

gpu = pytest.mark.gpu

POOL_FWD_M_TOL = 2.39e-7         # of sqrt(var'_ref), beside half an ulp of the mean
POOL_FWD_V_TOL = 2.38e-7         # of var'_ref
POOL_BWD_TOL = 2.36e-7           # of |ref|
TINY = 2.0 ** -126

# Agreement with sampling (test_agreement_with_sampling_is_reported), 2^20 float64 draws, seed 5.  Measured on the CPU: the
# 2 x 2 window's mean shift (mean' - max m) is 0.9423 of the sampled one and its variance 0.9116; the 3 x 3 window's 1.0084 and
# 0.8880.  The sampled estimates' own standard errors are at most 3.8e-3 of the shift and 1.6e-3 of the variance.  The fold is
# biased for more than two elements (the running maximum is not Gaussian), so no bound can be derived: the assertion is the
# measured worst deviation of a ratio from 1 (0.0577 for the shift, 0.1120 for the variance) with a factor 2 of margin.
SAMPLING_SHIFT_DEV = 2 * 0.0577
SAMPLING_VAR_DEV = 2 * 0.1120


# ================================================================================================ CPU
def max_quadrature(m1, v1, m2, v2, nodes=200):
    """E[max] and Var[max] of two independent Gaussians by Gauss-Legendre on the panels between m_i - 14 s_i, m_i, m_i + 14 s_i
    (beyond 14 s a Gaussian weighs 1e-43), the integrand (x - c)^p (f1 Phi2 + f2 Phi1); float64, vectorised over m1."""
    t, w = np.polynomial.legendre.leggauss(nodes)
    t, w = torch.from_numpy(t), torch.from_numpy(w)
    s1, s2 = math.sqrt(v1), math.sqrt(v2)
    m2 = torch.full_like(m1, m2)
    edges = torch.stack([m1 - 14 * s1, m1, m1 + 14 * s1, m2 - 14 * s2, m2, m2 + 14 * s2], 1).sort(1).values
    r2 = math.sqrt(2.0)

    def weight(x):
        z1, z2 = (x - m1[:, None, None]) / s1, (x - m2[:, None, None]) / s2
        f1, f2 = torch.exp(-0.5 * z1 * z1) / (s1 * math.sqrt(2 * math.pi)), torch.exp(-0.5 * z2 * z2) / (s2 * math.sqrt(2 * math.pi))
        return f1 * 0.5 * torch.special.erfc(-z2 / r2) + f2 * 0.5 * torch.special.erfc(-z1 / r2)

    a0, b0 = edges[:, :-1, None], edges[:, 1:, None]
    x = 0.5 * (a0 + b0) + 0.5 * (b0 - a0) * t
    wx = 0.5 * (b0 - a0) * w * weight(x)
    mean = m2 + (wx * (x - m2[:, None, None])).sum((1, 2))
    var = (wx * (x - mean[:, None, None]) ** 2).sum((1, 2))
    return mean, var


def pair(m1, v1, m2, v2, **kw):
    """ops.moments_pool_f64 on windows of two: element i of the result is the maximum of (m1[i], v1[i]) and (m2[i], v2[i])."""
    mean, var = torch.stack([m1, m2], -1).reshape(1, 1, -1), torch.stack([v1, v2], -1).reshape(1, 1, -1)
    out = ops.moments_pool_f64(ops.Moments(mean, var), 'max', 2, **kw)
    return out.mean.reshape(-1), out.var.reshape(-1)


def test_pair_step_against_quadrature():
    """A window of two against quadrature over alpha in [-12, 12] (1201 points), (v1, v2) in {1e-6, 0.3, 47}^2, the second mean
    at 100 (what the shifted form is for): the mean to 1e-8 theta, the variance to 1e-8 (v1 Phi + v2 Phi_c)."""
    alpha = torch.linspace(-12, 12, 1201, dtype=torch.float64)
    for v1 in (1e-6, 0.3, 47.0):
        for v2 in (1e-6, 0.3, 47.0):
            theta = math.sqrt(v1 + v2)
            m1 = 100.0 + alpha * theta
            gm, gv = pair(m1, torch.full_like(m1, v1), torch.full_like(m1, 100.0), torch.full_like(m1, v2))
            qm, qv = max_quadrature(m1, v1, 100.0, v2)
            cdf = 0.5 * torch.special.erfc(-alpha / math.sqrt(2.0))
            unit = v1 * cdf + v2 * (1 - cdf)
            dm, dv = ((gm - qm).abs() / theta).max().item(), ((gv - qv).abs() / unit).max().item()
            print("pair step v1 = %g v2 = %g: against quadrature %.2e theta, %.2e (v1 Phi + v2 Phi_c)" % (v1, v2, dm, dv))
            assert dm <= 1e-8 and dv <= 1e-8, (v1, v2, dm, dv)
            assert (gv >= 0).all() and (gm >= torch.maximum(m1, torch.full_like(m1, 100.0)) - 1e-12).all()


def test_pair_with_zero_is_the_relu():
    g = torch.Generator().manual_seed(2)
    m = 3 * torch.randn(4000, generator=g, dtype=torch.float64)
    v = torch.exp(torch.empty(4000, dtype=torch.float64).uniform_(math.log(1e-6), math.log(50.0), generator=g))
    v[:50] = 0.0
    z = torch.zeros_like(m)
    gm, gv = pair(m, v, z, z)
    r = ops.moments_relu_f64(ops.Moments(m, v))
    assert ((gm - r.mean).abs() <= 1e-12 * (1 + r.mean.abs())).all() and ((gv - r.var).abs() <= 1e-12 * (1 + r.var)).all()


def test_limits():
    t64 = lambda *x: torch.tensor(x, dtype=torch.float64)         # noqa: E731
    # theta^2 == 0: the plain maximum, the larger element's (m, v); a tie keeps the running value, and so does the gradient
    m1, m2 = t64(1.0, -2.0, 0.5, 0.5).requires_grad_(), t64(-1.0, 3.0, 0.5, 0.25).requires_grad_()
    v1, v2 = torch.zeros(4, dtype=torch.float64, requires_grad=True), torch.zeros(4, dtype=torch.float64, requires_grad=True)
    gm, gv = pair(m1, v1, m2, v2, track=True)
    assert torch.equal(gm.detach(), t64(1.0, 3.0, 0.5, 0.5)) and not gv.detach().any()
    g = torch.autograd.grad((gm * t64(1, 2, 3, 4) + gv * t64(5, 6, 7, 8)).sum(), [m1, v1, m2, v2])
    assert torch.equal(g[0], t64(1, 0, 3, 4)) and torch.equal(g[2], t64(0, 2, 0, 0))
    assert torch.equal(g[1], t64(5, 0, 7, 8)) and torch.equal(g[3], t64(0, 6, 0, 0))
    # a zero-variance window of four, with a tie for the maximum
    w = ops.moments_pool_f64(ops.Moments(t64(0.5, 2.0, 2.0, -1.0).reshape(1, 1, 2, 2), torch.zeros(1, 1, 2, 2, dtype=torch.float64)), 'max', 2)
    assert w.mean.item() == 2.0 and w.var.item() == 0.0
    # |alpha| = 40: the larger input passes through exactly
    for v1_, v2_ in ((1e-6, 0.3), (47.0, 1e-6), (0.3, 0.0)):
        th = math.sqrt(v1_ + v2_)
        for sign in (1.0, -1.0):
            gm, gv = pair(t64(100.0 + sign * 40 * th), t64(v1_), t64(100.0), t64(v2_))
            assert gm.item() == (100.0 + 40 * th if sign > 0 else 100.0) and gv.item() == (v1_ if sign > 0 else v2_)
    # var None stays deterministic
    x = torch.randn(2, 3, 6, 5)
    for op, fn in (('max', F.max_pool2d), ('avg', F.avg_pool2d)):
        o = ops.moments_pool_f64(ops.Moments(x), op, (2, 3), (2, 1), (1, 1))
        assert o.var is None and torch.equal(o.mean, fn(x.double(), (2, 3), (2, 1), (1, 1)))
    with pytest.raises(ops.BnnHipError, match="link"):
        ops.moments_pool_f64(ops.Moments(x, x * x, link='softmax'), 'max', 2)
    with pytest.raises(ops.BnnHipError, match="link"):
        ops.moments_pool(ops.Moments(x, x * x, link='softmax'), 'max', 2)
    # an all-padded window cannot occur: padding above half the kernel is refused, by the reference and by the entry
    with pytest.raises(ops.BnnHipError, match="half the kernel"):
        ops.moments_pool_f64(ops.Moments(x, x * x), 'max', 2, 2, 2)
    with pytest.raises(ops.BnnHipError, match="padding alone"):
        ops.moments_pool_f64(ops.Moments(x[..., :2], x[..., :2] ** 2), 'max', (1, 2), 1, (0, 1), (1, 3))
    lib, one = _lib.load(), ctypes.c_void_p(16)
    sh = pool_shape(p=(0, 2, 0), k=(1, 3, 2))
    assert lib.bnn_moments_pool3d_forward(one, one, one, one, ctypes.byref(sh), 0, 0, None) == -5
    assert b"half the kernel" in lib.bnn_last_error()


@pytest.mark.parametrize("cip", [True, False])
def test_avg_pool_against_torch(cip):
    g = torch.Generator().manual_seed(4)
    for shape, k, s, p, fn in (((2, 3, 9), 2, 2, 0, F.avg_pool1d), ((2, 3, 9), (3,), (2,), (1,), F.avg_pool1d),
                               ((2, 3, 9, 8), (3, 2), (2, 1), (1, 1), F.avg_pool2d), ((2, 2, 5, 6, 7), (2, 3, 2), (2, 2, 1), (1, 1, 0), F.avg_pool3d)):
        m, v = torch.randn(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64)
        o = ops.moments_pool_f64(ops.Moments(m, v), 'avg', k, s, p, 1, cip)
        size = float(np.prod(k))
        n = size if cip else fn(torch.ones(shape, dtype=torch.float64), k, s, p, False, True) * size          # the valid count
        assert ((o.mean - fn(m, k, s, p, False, cip)).abs() <= 1e-12).all()
        assert ((o.var - fn(v, k, s, p, False, cip) / n).abs() <= 1e-12).all()


@pytest.mark.parametrize("affine", [True, False])
def test_batchnorm_against_torch(affine):
    torch.manual_seed(6)
    for cls, shape in ((torch.nn.BatchNorm2d, (3, 5, 4, 3)), (torch.nn.BatchNorm1d, (4, 6)), (torch.nn.BatchNorm3d, (2, 3, 2, 3, 2))):
        bn = cls(shape[1], affine=affine).double()
        with torch.no_grad():
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
            if affine:
                bn.weight.normal_()
                bn.bias.normal_()
        bn.eval()
        m, v = torch.randn(shape, dtype=torch.float64), torch.rand(shape, dtype=torch.float64)
        o = ops.moments_batchnorm_f64(ops.Moments(m, v), bn)
        a = (bn.weight if affine else 1.0) / torch.sqrt(bn.running_var + bn.eps)
        a = (a * torch.ones(shape[1], dtype=torch.float64)).reshape((1, -1) + (1,) * (len(shape) - 2))
        assert ((o.mean - bn(m)).abs() <= 1e-12).all() and ((o.var - a * a * v).abs() <= 1e-12).all()
        assert not o.mean.requires_grad
        assert ops.moments_batchnorm_f64(ops.Moments(m), bn).var is None
        t = ops.moments_batchnorm_f64(ops.Moments(m, v), (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps))
        assert torch.equal(t.mean, o.mean) and torch.equal(t.var, o.var)


GRADCHECK = [  # (shape, op, kernel, stride, padding, dilation, count_include_pad)
    ((2, 2, 7), 'max', 2, 2, 0, 1, True),
    ((1, 2, 5, 4), 'max', (3, 2), (2, 1), (1, 0), 1, True),
    ((1, 1, 3, 4, 5), 'max', (2, 3, 2), (1, 2, 1), (0, 1, 1), (1, 1, 2), True),
    ((1, 2, 5, 4), 'avg', (3, 2), (2, 1), (1, 1), 1, True),
    ((1, 2, 5, 4), 'avg', (3, 2), (2, 1), (1, 1), 1, False),
]


@pytest.mark.parametrize("case", range(len(GRADCHECK)))
def test_tracked_recursion_gradcheck(case):
    """The tracked float64 route against finite differences, the inputs planted away from theta^2 == 0."""
    shape, op, k, s, p, d, cip = GRADCHECK[case]
    g = torch.Generator().manual_seed(20 + case)
    m = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
    v = (0.2 + torch.rand(shape, generator=g, dtype=torch.float64)).requires_grad_()

    def fn(m_, v_):
        o = ops.moments_pool_f64(ops.Moments(m_, v_), op, k, s, p, d, cip, track=True)
        return o.mean, o.var

    assert torch.autograd.gradcheck(fn, (m, v), eps=1e-6, atol=1e-7, rtol=1e-6)
    with torch.enable_grad():
        assert not ops.moments_pool_f64(ops.Moments(m, v), op, k, s, p, d, cip).mean.requires_grad         # untracked: detached


class Seq(BayesianNetworkModule):
    def __init__(self, *mods, samples=8):
        super().__init__(0, 0, samples=samples)
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


def test_rewrite_reclasses_only_behind_a_bayesian_layer():
    torch.manual_seed(3)
    tn = torch.nn
    net = Seq(tn.MaxPool2d(2), tn.BatchNorm2d(1), NormalConv2d(1, 2, 3), tn.MaxPool2d(2), tn.BatchNorm2d(2), tn.AvgPool2d(2, 1),
              tn.AdaptiveAvgPool2d(1), tn.Flatten(), NormalLinear(2, 3)).eval()
    mods = list(net.layers)
    x = torch.randn(3, 1, 20, 20)
    keys0 = list(net.state_dict().keys())
    torch.manual_seed(9)
    before = net(x, samples=1)
    assert bnn_nn.moment_activations(net) == 4 and bnn_nn.moment_activations(net) == 0
    assert [type(m).__name__ for m in net.layers] == ["MaxPool2d", "BatchNorm2d", "NormalConv2d", "MomentMaxPool2d", "MomentBatchNorm2d",
                                                      "MomentAvgPool2d", "MomentAdaptiveAvgPool2d", "Flatten", "NormalLinear"]
    assert all(a is b for a, b in zip(mods, net.layers)) and list(net.state_dict().keys()) == keys0
    torch.manual_seed(9)
    after = net(x, samples=1)
    assert torch.equal(before, after)
    for name in ("MaxPool", "AvgPool", "AdaptiveAvgPool", "BatchNorm"):
        for nd in "123":
            twin, parent = getattr(bnn_nn, "Moment%s%sd" % (name, nd)), getattr(tn, "%s%sd" % (name, nd))
            assert issubclass(twin, parent) and twin.__name__ not in bnn_nn.__all__
    # the whole pass is the hand-written recursion
    got = net.predictive_moments(x)
    c, lin = net.layers[2], net.layers[8]
    h = net.layers[1](net.layers[0](x))
    h = ops.moments_convNd_f64(h, *posterior(c), c.stride, c.padding, c.dilation, c.groups)
    h = ops.moments_batchnorm_f64(ops.moments_pool_f64(h, 'max', 2), net.layers[4])
    h = ops.moments_pool_f64(ops.moments_pool_f64(h, 'avg', 2, 1), 'avg', 3).flatten(1)
    want = ops.moments_linear_f64(h, *posterior(lin))
    assert torch.equal(got.mean, want.mean.float()) and torch.equal(got.var, want.var.float())
    one = net.layers[3](ops.Moments(x[0], x[0] ** 2))                            # one item (C, H, W), as the parent takes it
    assert one.mean.shape == (1, 10, 10)
    with pytest.raises(ops.BnnHipError, match="MomentBatchNorm2d has no moment backward"):
        net.forward_moments(x)


def posterior(layer):
    return [t.detach() for t in (layer.weight.mean, layer.weight.scale, layer.bias.mean, layer.bias.scale)]


def test_refusals():
    tn = torch.nn
    mom = ops.Moments(torch.randn(2, 2, 6, 6), torch.rand(2, 2, 6, 6))

    def twin(mod):
        seq = tn.Sequential(NormalConv2d(2, 2, 1), mod)
        assert bnn_nn.moment_activations(seq) == 1
        return seq[1]

    for mod, what in ((tn.MaxPool2d(2, ceil_mode=True), "ceil_mode"), (tn.AvgPool2d(2, ceil_mode=True), "ceil_mode"),
                      (tn.MaxPool2d(2, return_indices=True), "return_indices"), (tn.AvgPool2d(2, divisor_override=3), "divisor_override"),
                      (tn.AdaptiveAvgPool2d(4), "no multiple"), (tn.BatchNorm2d(2), "training mode"),
                      (tn.BatchNorm2d(2, track_running_stats=False).eval(), "no running statistics"),
                      (tn.MaxPool2d(7), "larger than the padded input")):
        with pytest.raises(ops.BnnHipError, match=what):
            twin(mod)(mom)
    assert twin(tn.AdaptiveAvgPool2d((3, None)))(mom).mean.shape == (2, 2, 3, 6)
    assert twin(tn.AdaptiveAvgPool2d(4))(mom.mean).shape == (2, 2, 4, 4)          # on tensors it is its parent
    with pytest.raises(ops.BnnHipError, match="at most 64"):
        ops.moments_pool_f64(ops.Moments(torch.zeros(1, 1, 9, 9), torch.zeros(1, 1, 9, 9)), 'max', 9)
    with pytest.raises(_lib.BnnHipError):
        ops.moments_pool(mom, 'max', 2)                                          # CPU moments: no device route
    with pytest.raises(_lib.BnnHipError):
        ops.moments_batchnorm(mom, tn.BatchNorm2d(2).eval())


class LeNet(BayesianNetworkModule):
    """NormalConv2d(1, 4, 3) -> ELU -> MaxPool2d(2) -> NormalConv2d(4, 6, 3) -> ELU -> AvgPool2d(2) -> Flatten -> NormalLinear ->
    Softmax on (B, 1, 14, 14)."""

    def __init__(self, classes=5):
        super().__init__(1, classes, samples=8)
        tn = torch.nn
        self.layers = tn.Sequential(NormalConv2d(1, 4, 3), tn.ELU(), tn.MaxPool2d(2), NormalConv2d(4, 6, 3), tn.ELU(), tn.AvgPool2d(2),
                                    tn.Flatten(), NormalLinear(24, classes), tn.Softmax(dim=-1))
        assert bnn_nn.moment_activations(self) == 5

    def _forward(self, x):
        return self.layers(x)


def lenet_recursion64(net, x, track=False):
    """The hand-written float64 recursion of a CPU LeNet -> the logit Moments."""
    c1, c2, lin = net.layers[0], net.layers[3], net.layers[7]
    par = (lambda l: (l.weight.mean, l.weight.scale, l.bias.mean, l.bias.scale)) if track else posterior
    h = ops.moments_convNd_f64(x, *par(c1), c1.stride, c1.padding, c1.dilation, c1.groups, activation=("elu", 1.0), track=track)
    h = ops.moments_pool_f64(h, 'max', 2, track=track)
    h = ops.moments_convNd_f64(h, *par(c2), c2.stride, c2.padding, c2.dilation, c2.groups, activation=("elu", 1.0), track=track)
    h = ops.moments_pool_f64(h, 'avg', 2, track=track)
    return ops.moments_linear_f64(h.flatten(1), *par(lin), track=track)


def test_lenet_on_the_cpu(switch):
    torch.manual_seed(1)
    net = set_posteriors(LeNet(), 40)
    assert [type(m).__name__ for m in net.layers][1:6] == ["MomentELU", "MomentMaxPool2d", "NormalConv2d", "MomentELU", "MomentAvgPool2d"]
    x = torch.randn(3, 1, 14, 14)
    got, want = net.predictive_moments(x), lenet_recursion64(net, x)
    assert got.link == "softmax" and got.mean.shape == (3, 5) and (got.var > 0).all()
    assert torch.equal(got.mean, want.mean.float()) and torch.equal(got.var, want.var.float())
    mom = net.forward_moments(x)
    ref = lenet_recursion64(net, x, track=True)
    assert mom.mean.dtype == torch.float64 and mom.mean.requires_grad and torch.equal(mom.mean, ref.mean) and torch.equal(mom.var, ref.var)
    params = list(net.parameters())
    loss = lambda o: (o.mean.sum() + o.var.sum())         # noqa: E731
    a, b = torch.autograd.grad(loss(mom), params), torch.autograd.grad(loss(ref), params)
    assert len(a) == 12 and all(torch.isfinite(p).all() and p.abs().sum() > 0 for p in a)
    assert all((p - q).abs().max() <= 1e-12 * (1 + q.abs().max()) for p, q in zip(a, b))


def pool_shape(B=2, C=3, sp=(1, 7, 6), k=(1, 2, 2), s=(1, 2, 2), p=(0, 0, 0), d=(1, 1, 1)):
    return _lib.Pool3dShape(B=B, C=C, D=sp[0], H=sp[1], W=sp[2], KD=k[0], KH=k[1], KW=k[2], stride_d=s[0], stride_h=s[1], stride_w=s[2],
                            pad_d=p[0], pad_h=p[1], pad_w=p[2], dil_d=d[0], dil_h=d[1], dil_w=d[2])


def test_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(18)

    def fwd(m=one, v=one, om=one, ov=one, sh=None, op=0, flags=0):
        sh = pool_shape() if sh is None else sh
        return lib.bnn_moments_pool3d_forward(m, v, om, ov, ctypes.byref(sh) if sh != "null" else None, op, flags, None)

    def bwd(m=one, v=one, gom=one, gov=one, gm=one, gv=one, sh=None, op=0, flags=0):
        sh = pool_shape() if sh is None else sh
        return lib.bnn_moments_pool3d_backward(m, v, gom, gov, gm, gv, ctypes.byref(sh) if sh != "null" else None, op, flags, None)

    for name in ("m", "v", "om", "ov"):
        assert fwd(**{name: None}) == -1, name
    for name in ("m", "v", "gom", "gov", "gm", "gv"):
        assert bwd(**{name: None}) == -1, name
    assert fwd(sh="null") == -1 and bwd(sh="null") == -1
    assert lib.bnn_last_error().startswith(b"bnn_moments_pool3d_backward: ")
    for call in (fwd, bwd):
        assert call(sh=pool_shape(B=0)) == -2 and call(sh=pool_shape(C=0)) == -2 and call(sh=pool_shape(sp=(1, 0, 6))) == -2
        assert call(sh=pool_shape(k=(1, 0, 2))) == -2 and call(sh=pool_shape(s=(1, 2, 0))) == -2 and call(sh=pool_shape(d=(0, 1, 1))) == -2
        assert call(sh=pool_shape(p=(0, -1, 0))) == -2
        assert call(sh=pool_shape(k=(1, 8, 2))) == -2                              # an empty output
        assert b"empty output" in lib.bnn_last_error()
        assert call(sh=pool_shape(k=(1, 3, 2), p=(0, 2, 0))) == -5                 # padding above half the kernel
        assert call(sh=pool_shape(sp=(9, 9, 9), k=(5, 5, 3))) == -5                # 75 elements: over the cap of 64
        assert b"64" in lib.bnn_last_error()
        assert call(sh=pool_shape(B=1 << 16, C=1 << 16, sp=(1, 2, 2))) == -5       # 2^32 elements or more
        assert b"2^32" in lib.bnn_last_error()
        assert call(sh=pool_shape(B=1, C=1, sp=(1, 1, 1 << 31), k=(1, 1, 1), s=(1, 1, 1))) == -5
        assert call(sh=pool_shape(sp=(1, 7, 2), k=(1, 2, 2), s=(1, 2, 1), p=(0, 0, 1), d=(1, 1, 3))) == -5       # a window in the padding alone
        assert b"padding alone" in lib.bnn_last_error()
        assert call(op=2) == -6 and call(op=-1) == -6 and call(flags=2) == -6 and call(op=1, flags=3) == -6
    for name in ("m", "v", "om", "ov"):
        assert fwd(**{name: odd}) == -4, name
    for name in ("m", "v", "gom", "gov", "gm", "gv"):
        assert bwd(**{name: odd}) == -4, name

    def norm(m=one, v=one, g=one, b=one, rm=one, rv=one, eps=1e-5, om=one, ov=one, B=2, C=3, inner=4):
        return lib.bnn_moments_batchnorm(m, v, g, b, rm, rv, eps, om, ov, B, C, inner, None)

    for name in ("m", "v", "rm", "rv", "om", "ov"):
        assert norm(**{name: None}) == -1, name
    assert norm(B=0) == -2 and norm(C=0) == -2 and norm(inner=0) == -2
    assert norm(B=1 << 20, C=1 << 10, inner=4) == -5 and norm(eps=-1.0) == -5 and norm(eps=float("nan")) == -5 and norm(eps=float("inf")) == -5
    assert lib.bnn_last_error().startswith(b"bnn_moments_batchnorm: ")
    for name in ("m", "v", "g", "b", "rm", "rv", "om", "ov"):
        assert norm(**{name: odd}) == -4, name
    assert lib.bnn_launch_count() == n0


def test_pool_kernels_do_not_spill():
    """The six new kernels use no scratch and spill nothing (the backward's prefix states live in dynamic LDS, so its static LDS
    block is empty too); read the way test_conv_moment_kernels_do_not_spill reads the notes."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    mine = {n: f for n, f in kernels.items()
            if re.match(r"_ZN3bnn(16k_moments_pool3dILi[01]EEEvNS_8PoolArgsE|20k_moments_pool3d_bwdILi[01]EEEvNS_8PoolArgsE|19k_moments_batchnormE|"
                        r"11k_pool_zeroE)", n)}
    assert len(mine) == 6, sorted(kernels)
    for n, f in mine.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0 and \
            int(f.get("private_segment_fixed_size", 0)) == 0 and int(f.get("group_segment_fixed_size", 0)) == 0, (n, f)


def test_agreement_with_sampling_is_reported():
    """A 2 x 2 and a 3 x 3 window of independent Gaussians with mixed means and variances against 2^20 draws: the moment / sampled
    ratios of the mean shift (mean' - max m) and of the variance, within twice the deviation measured (the header comment)."""
    g = torch.Generator().manual_seed(5)
    S = 1 << 20
    for side in (2, 3):
        n = side * side
        m = torch.randn(n, generator=g, dtype=torch.float64)
        v = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(math.log(0.05), math.log(2.0), generator=g))
        out = ops.moments_pool_f64(ops.Moments(m.reshape(1, 1, side, side), v.reshape(1, 1, side, side)), 'max', side)
        y = (m + v.sqrt() * torch.randn(S, n, generator=g, dtype=torch.float64)).max(1).values
        shift, var = y.mean() - m.max(), y.var()
        se_shift, se_var = (var / S).sqrt() / shift, ((y - y.mean()).pow(4).mean() - var ** 2).sqrt() / math.sqrt(S) / var
        r_shift, r_var = ((out.mean.item() - m.max()) / shift).item(), (out.var.item() / var).item()
        print("%d x %d window: moment / sampled mean shift %.4f (se %.1e), variance %.4f (se %.1e)" % (side, side, r_shift, se_shift, r_var, se_var))
        assert abs(r_shift - 1) <= SAMPLING_SHIFT_DEV and abs(r_var - 1) <= SAMPLING_VAR_DEV, (side, r_shift, r_var)


# ================================================================================================ GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


# (shape, kernel, stride, padding, dilation)
POOL_CASES = {
    "1d": ((3, 2, 9), 2, 2, 0, 1),                                             # the trailing element is unused
    "lenet": ((2, 3, 7, 6), 2, 2, 0, 1),
    "overlap": ((2, 3, 9, 8), (3, 2), (2, 1), (1, 0), 1),
    "3d": ((2, 2, 5, 6, 7), (2, 3, 2), (2, 2, 1), (0, 1, 1), (1, 1, 2)),
    "27": ((1, 1, 5, 5, 5), 3, 1, 1, 1),                                        # a 27-element window
    "blocks": ((5, 7, 13, 11), 2, 2, 0, 1),                                     # 1050 outputs: several workgroups, a ragged last one
}
OVERLAPPING = ("overlap", "3d", "27")


def pool_input(shape, seed):
    """Means ~ N(0, 1), variances log-uniform in [1e-6, 10]; planted: zero-variance neighbours, equal means, a zero-variance channel."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(shape, generator=g)
    v = torch.exp(torch.empty(shape).uniform_(math.log(1e-6), math.log(10.0), generator=g))
    fm, fv = m.view(-1), v.view(-1)
    idx = torch.randperm(fm.numel() - 1, generator=g)
    z, e = idx[:fm.numel() // 8], idx[fm.numel() // 8:fm.numel() // 4]
    fv[z] = 0.0
    fv[z + 1] = 0.0
    fm[e + 1] = fm[e]
    if shape[1] > 1:
        v[:, -1] = 0.0
        m[0, -1].view(-1)[:2] = 0.75                                           # a tie inside the zero-variance channel
    return m, v


_reference = {}


def pool_reference(case, op):
    """(m, v, G_m, G_v, the float64 forward, its float64 gradients (g_m, g_v), sum |contribution| per input element) -- computed
    once per (case, op) and left unchanged."""
    if (case, op) not in _reference:
        shape, k, s, p, d = POOL_CASES[case]
        m, v = pool_input(shape, 31)
        mom = ops.Moments(m, v)
        nd, kk, ss, pp, dd, out_sp = ops._pool_geometry("test", mom, op, k, s, p, d)
        geo = (kk, ss, pp, dd, out_sp)
        ms = [w.clone().requires_grad_() for w in ops._pool_windows(m.double(), *geo)]
        vs = [w.clone().requires_grad_() for w in ops._pool_windows(v.double(), *geo)]
        out = ops._pool_fold_f64(ms, vs, ops._pool_windows(torch.ones(shape[2:], dtype=torch.bool), *geo), op, float(np.prod(kk)))
        whole = ops.moments_pool_f64(mom, op, k, s, p, d)
        assert torch.equal(whole.mean, out.mean.detach()) and torch.equal(whole.var, out.var.detach())
        g = torch.Generator().manual_seed(32)
        G_m, G_v = torch.randn(out.mean.shape, generator=g), torch.randn(out.mean.shape, generator=g)
        parts = torch.autograd.grad((out.mean * G_m.double() + out.var * G_v.double()).sum(), ms + vs)
        sums = []
        for part in (parts[:len(ms)], parts[len(ms):]):
            total, mag = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
            pt, pa = F.pad(total, [q for pi in reversed(pp) for q in (pi, pi)]), F.pad(mag, [q for pi in reversed(pp) for q in (pi, pi)])
            for wt, wa, c in zip(ops._pool_windows_of_padded(pt, *geo), ops._pool_windows_of_padded(pa, *geo), part):
                wt += c
                wa += c.abs()
            crop = (Ellipsis,) + tuple(slice(pi, pi + n) for pi, n in zip(pp, shape[2:]))
            sums.append((pt[crop], pa[crop]))
        _reference[(case, op)] = (m, v, G_m, G_v, whole, sums[0][0], sums[1][0], sums[0][1], sums[1][1])
    return _reference[(case, op)]


def forward_deviation(got, ref):
    """-> (mean deviation beyond half an ulp in units of sqrt(var'_ref), variance deviation in units of var'_ref) over the outputs
    with var'_ref > 0 (TINY allowed absolutely); the outputs with var'_ref == 0 must be exact."""
    gm, gv = got.mean.double().cpu(), got.var.double().cpu()
    zero = ref.var == 0
    assert torch.equal(gm[zero], ref.mean[zero].float().double()) and not gv[zero].any()
    pos = ~zero
    if not pos.any():
        return 0.0, 0.0
    em = ((gm - ref.mean).abs() - 2.0 ** -24 * ref.mean.abs() - TINY).clamp_min(0)[pos] / ref.var[pos].sqrt()
    ev = ((gv - ref.var).abs() - TINY).clamp_min(0)[pos] / ref.var[pos]
    return em.max().item(), ev.max().item()


@gpu
@pytest.mark.parametrize("op", ["max", "avg"])
@pytest.mark.parametrize("case", list(POOL_CASES))
def test_pool_forward_matches_float64(dev, case, op):
    shape, k, s, p, d = POOL_CASES[case]
    m, v, _, _, ref = pool_reference(case, op)[:5]
    got = ops.moments_pool(ops.Moments(m.to(dev), v.to(dev)), op, k, s, p, d)
    assert got.mean.shape == ref.mean.shape and got.mean.dtype == torch.float32 and not got.mean.requires_grad
    assert torch.isfinite(got.mean).all() and (got.var >= 0).all()
    dm, dv = forward_deviation(got, ref)
    print("pool forward %s %s: %.3e sqrt(var') beyond half an ulp, %.3e var'" % (case, op, dm, dv))
    assert max(POOL_FWD_M_TOL, POOL_FWD_V_TOL) <= 1e-5
    assert dm <= POOL_FWD_M_TOL and dv <= POOL_FWD_V_TOL, (dm, dv)
    if op == "avg":                                                             # the divisor flag, on a padded shape
        a = ops.moments_pool(ops.Moments(m.to(dev), v.to(dev)), op, k, s, p, d, count_include_pad=False)
        dm, dv = forward_deviation(a, ops.moments_pool_f64(ops.Moments(m, v), op, k, s, p, d, count_include_pad=False))
        assert dm <= POOL_FWD_M_TOL and dv <= POOL_FWD_V_TOL, (dm, dv)
    z = ops.moments_pool(ops.Moments(m.to(dev)), op, k, s, p, 1 if op == "avg" else d)         # var None stays deterministic
    assert z.var is None
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("op", ["max", "avg"])
@pytest.mark.parametrize("case", list(POOL_CASES))
def test_pool_backward_matches_float64_autograd(dev, case, op):
    shape, k, s, p, d = POOL_CASES[case]
    m, v, G_m, G_v, _, rm, rv, am, av = pool_reference(case, op)

    def run():
        a, b = m.to(dev).requires_grad_(), v.to(dev).requires_grad_()
        out = ops.moments_pool(ops.Moments(a, b), op, k, s, p, d, track=True)
        assert out.mean.requires_grad and out.var.requires_grad
        return torch.autograd.grad([out.mean, out.var], [a, b], [G_m.to(dev), G_v.to(dev)])

    gm, gv = run()
    _, kk, ss, _, dd, _ = ops._pool_geometry("test", ops.Moments(m, v), op, k, s, p, d)
    n_add = int(np.prod([-(-(di * (ki - 1) + 1) // si) for ki, si, di in zip(kk, ss, dd)]))     # prod ceil(extent / stride)
    assert (n_add == 1) == (case not in OVERLAPPING) and POOL_BWD_TOL <= 1e-5
    for got, ref, mag, what in ((gm, rm, am, "g_m"), (gv, rv, av, "g_v")):
        excess = ((got.double().cpu() - ref).abs() - TINY).clamp_min(0)
        if case in OVERLAPPING:
            excess = (excess - gamma(n_add) * mag).clamp_min(0)                # the atomics' fp32 sum of at most n_add contributions
        worst = (excess / ref.abs().clamp_min(1e-300))[ref != 0].max().item() if (ref != 0).any() else 0.0
        print("pool backward %s %s %s: %.3e |ref| (%d addends at most)" % (case, op, what, worst, n_add))
        assert bool(torch.isfinite(got).all()) and bool((excess <= POOL_BWD_TOL * ref.abs()).all()), (what, worst)
    if case not in OVERLAPPING:                                                 # plain stores: identical calls, identical bits
        again = run()
        assert torch.equal(gm, again[0]) and torch.equal(gv, again[1])
    if case == "1d":                                                            # the input no window covers
        assert not gm[..., 8].any() and not gv[..., 8].any()
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("shape", [(3, 5, 4, 3), (4, 6)], ids=lambda s: "x".join(map(str, s)))
def test_batchnorm_matches_float64(dev, shape, affine):
    """The launch forms a = gamma / sqrt(rv + eps) in fp32 -- three roundings, the sqrt halving the first: 2.5 U --, m - rm (U)
    and one fma (U of the result): |dm| <= 3.5 U |a (m - rm)| + U |m'|, bounded here by 5 U (|a (m - rm)| + |beta|);
    v' = (a a) v: 5 U + U + U = 7 U, bounded by 8 U v'.  U = 2^-24.  eps is the module's, rounded to fp32 on both sides."""
    g = torch.Generator().manual_seed(7)
    C = shape[1]
    bn = (torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm1d)(C, affine=affine)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
        if affine:
            bn.weight.copy_(torch.randn(C, generator=g))
            bn.bias.copy_(torch.randn(C, generator=g))
    bn.eval()
    m, v = torch.randn(shape, generator=g), torch.rand(shape, generator=g)
    eps32 = float(torch.tensor(bn.eps, dtype=torch.float32))
    ref = ops.moments_batchnorm_f64(ops.Moments(m, v), (bn.weight, bn.bias, bn.running_mean, bn.running_var, eps32))
    beta = (bn.bias.detach().double() if affine else torch.zeros(C, dtype=torch.float64)).reshape((1, -1) + (1,) * (len(shape) - 2))
    twin = torch.nn.Sequential(NormalLinear(1, 1), bn)
    assert bnn_nn.moment_activations(twin) == 1
    got = twin[1].to(dev)(ops.Moments(m.to(dev), v.to(dev)))
    assert_within(got.mean, ref.mean, 5 * U * ((ref.mean - beta).abs() + beta.abs()) + TINY, "batchnorm mean")
    assert_within(got.var, ref.var, 8 * U * ref.var + TINY, "batchnorm var")
    assert torch.equal(twin[1](m.to(dev)), torch.nn.functional.batch_norm(m.to(dev), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                                                                          False, 0.0, bn.eps))
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("op", ["max", "avg"])
@pytest.mark.parametrize("off", [4, 8])
def test_operands_off_16_bytes_give_the_same_bits(dev, off, op):
    """Every operand of the three entries is read and written one element at a time: moved 4 and 8 bytes off a 16-byte boundary
    (NaN guards around the inputs, sentinels around the outputs) the results keep their bits."""
    shape, k, s, p, d = POOL_CASES["lenet"]
    m, v, G_m, G_v = [t.to(dev) for t in pool_reference("lenet", op)[:4]]
    lib, st = _lib.load(), ops.stream_ptr(dev)
    sh = ops._pool3d_shape(shape, (2, 2), (2, 2), (0, 0), (1, 1))
    code = _lib.POOL_MAX if op == "max" else _lib.POOL_AVG
    other = 12 - off
    g = torch.Generator().manual_seed(13)
    stats = [t.to(dev) for t in (torch.randn(3, generator=g), torch.rand(3, generator=g) + 0.5, torch.randn(3, generator=g), torch.randn(3, generator=g))]

    def run(o1, o2):
        mv = (lambda t, o: offset_view(t, o)) if o1 is not None else (lambda t, o: t)
        a, b, ga, gb = mv(m, o1), mv(v, o2), mv(G_m, o2), mv(G_v, o1)
        om, ov = output_view(G_m.shape, torch.float32, dev, o1 or 0), output_view(G_m.shape, torch.float32, dev, o2 or 0)
        gm, gv = output_view(shape, torch.float32, dev, o2 or 0), output_view(shape, torch.float32, dev, o1 or 0)
        assert lib.bnn_moments_pool3d_forward(a.data_ptr(), b.data_ptr(), om.data_ptr(), ov.data_ptr(), ctypes.byref(sh), code, 0, st) == 0
        assert lib.bnn_moments_pool3d_backward(a.data_ptr(), b.data_ptr(), ga.data_ptr(), gb.data_ptr(), gm.data_ptr(), gv.data_ptr(),
                                               ctypes.byref(sh), code, 0, st) == 0
        rm, rv, ga_, be_ = mv(stats[0], o1), mv(stats[1], o2), mv(stats[2], o2), mv(stats[3], o1)
        nm, nv = output_view(shape, torch.float32, dev, o1 or 0), output_view(shape, torch.float32, dev, o2 or 0)
        assert lib.bnn_moments_batchnorm(a.data_ptr(), b.data_ptr(), ga_.data_ptr(), be_.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5,
                                         nm.data_ptr(), nv.data_ptr(), shape[0], shape[1], shape[2] * shape[3], st) == 0
        torch.cuda.synchronize()
        outs = [om, ov, gm, gv, nm, nv]
        assert all(guards_intact(t) for t in outs)
        return outs

    want, got = run(None, None), run(off, other)
    for a, b in zip(got, want):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b)
    _lib.check_device(dev)


@gpu
def test_graph_capture(dev):
    """One forward and one backward of a max pool whose windows do not overlap in a captured graph: two replays give the eager
    bits."""
    shape, k, s, p, d = POOL_CASES["blocks"]
    m, v, G_m, G_v = [t.to(dev) for t in pool_reference("blocks", "max")[:4]]
    a, b = m.clone().requires_grad_(), v.clone().requires_grad_()

    def step():
        out = ops.moments_pool(ops.Moments(a, b), 'max', k, s, p, d, track=True)
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
        diffs = [(x.detach() - y).abs().max().item() for x, y in zip(got, want)]
        assert all(torch.equal(x.detach(), y) for x, y in zip(got, want)), diffs
    _lib.check_device(dev)


# The LeNet-shaped net end to end, in the manner of test_moment_conv_backward.py's network test.  Forward: conv, ELU, max pool, conv,
# ELU, average pool, dense -- 7 stages, each within 1e-5 of its output's scale in the fp32 mode (the pooling bounds above are far
# below that), so the logit moments are within 7 x 1e-5 of float64's.  The training step adds the sampling launch and softmax / nll
# and the 8 backward stages: 17.  bf16 mode: each contraction reads operands rounded to bf16, within 2^-8 sqrt(R) of the scale of
# its sum, R its reduction length: conv 1 -> 4, 3 x 3 on 14 x 14 (P = 144): forward R = 9, weight gradient R = 3 x 144; conv 4 -> 6,
# 3 x 3 on 6 x 6 (P = 16): forward 36, input gradient 54, weight gradient 3 x 16; NormalLinear 24 -> 5 at B = 3: 24, 5, 3.
LENET_R_FWD = (9, 36, 24)
LENET_R = LENET_R_FWD + (432, 54, 48, 5, 3)
LENET_FWD_TOL = {"f32": 7e-5, "bf16": 7e-5 + 2.0 ** -8 * sum(math.sqrt(r) for r in LENET_R_FWD)}
LENET_TOL = {"f32": 17e-5, "bf16": 17e-5 + 2.0 ** -8 * sum(math.sqrt(r) for r in LENET_R)}


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_lenet_on_the_device(dev, mode, switch):
    bnn.set_compute(mode)
    torch.manual_seed(8)
    cpu = set_posteriors(LeNet(), 80)
    net = LeNet()
    net.load_state_dict(cpu.state_dict())
    net = net.to(dev)
    g = torch.Generator().manual_seed(81)
    x, t = torch.randn(3, 1, 14, 14, generator=g), torch.randint(0, 5, (3,), generator=g)
    xd, td = x.to(dev), t.to(dev)
    ref = lenet_recursion64(cpu, x)
    got = net.predictive_moments(xd)
    assert got.link == "softmax" and got.mean.dtype == torch.float32
    assert_within(got.mean, ref.mean, scaled_bound(ref.mean, LENET_FWD_TOL[mode]), "lenet logits m " + mode)
    assert_within(got.var, ref.var, scaled_bound(ref.var, LENET_FWD_TOL[mode]), "lenet logits v " + mode)
    u = net.predictive_uncertainty(xd, samples=4, inputs="probs", propagation="moments")
    assert torch.isfinite(u.total).all() and (u.mean.sum(-1) - 1).abs().max() <= 1e-5
    S = 8
    mom, ps, grads = e2e_step(net, xd, td, S)
    assert torch.equal(mom.mean, got.mean) and torch.equal(mom.var, got.var)
    key = net.moment_key
    ys = ops.moments_sample(ops.Moments(mom.mean.detach(), mom.var.detach()), key, S)
    eps = recovered_eps(ys, mom.mean, mom.var)
    net64 = cpu.double()
    m64 = net64.forward_moments(x.double())
    y64 = torch.softmax(m64.mean + torch.sqrt(m64.var + 1e-16) * eps, -1)
    want = torch.autograd.grad(F.nll_loss(torch.log(y64.reshape(-1, 5)), t.repeat(S), reduction="sum"), list(net64.parameters()))
    names = [n for n, _ in net.named_parameters()]
    assert len(names) == len(grads) == len(want) == 12
    for n, a, w in zip(names, grads, want):
        assert torch.isfinite(a).all()
        assert_within(a, w, scaled_bound(w, LENET_TOL[mode]), "%s lenet %s" % (n, mode))
    _lib.check_device(dev)
