"""The head of a sampling-free pass (K21, csrc/bnn_moments_head.hip): the moments of MultivariateNormalLinear under its own
sampler (uniform noise through the element-wise square root of the triangle), the N x N covariance of a dense head's outputs
per row (predictive_moments(covariance=True)), and correlated draws from it (ops.moments_sample on moments that carry a cov).

CPU: the float64 twins against sampling (the formulas are exact for independent inputs, so everything lies within 5 standard
errors), the exactness of the head covariance behind one hidden layer, the plumbing of Moments.cov, the Cholesky pivot rule,
and the CIFAR10 example's layer sequence with its real head at reduced widths.  GPU: every entry against its float64 twin on the
same fp32 inputs with derived bounds, operands off the 16-byte boundary, graph capture, the reduced CIFAR10 net in both modes.

Bounds.  L = sqrt(softplus(scale) [+ 1e-10]) is formed on the device by mvn_l (native exp2 / log2 / rcp, a correctly rounded
sqrt) and by torch's float64 softplus on the host.  L_REL_TOL is 4 x the worst relative deviation measured on the MI355X by
test_factor_element_deviation (it prints it) over 4096 scales in [-87, 25]: measured 4.816e-7 (about 8 u, u = 2^-24), so
L_REL_TOL = 1.93e-6 -- the project's margin for libm differences, as in the ELU and pool tests.  Below softplus = 2^-126 (scale <
-87.3) the value is subnormal in fp32 and may lose all its bits or be flushed: there L is only known to 2^-63 absolutely
(L_ABS_TOL).  On top of that every sum of n fp32 terms adds gamma(n) sum |addends| (Higham eq. 3.5), evaluated from the twin's
terms; an output whose addends are all zero is exact.

End to end on the CPU (test_reduced_cifar10_on_the_cpu prints the figures): the reduced CIFAR10 net, 4 rows, 4096 draws from the
moment pass with covariance=True against 4096 stochastic forwards -- the logits are only approximately Gaussian, so no bound can be
derived.  Measured: worst |mean probability difference| 0.00094, worst |total - total'| 0.00181, |aleatoric| 0.00143, |epistemic|
0.00038 nats.  The epistemic part itself is 0.0097 nats, and the same pass WITHOUT the covariance (printed too, not asserted) is off
by 0.043 in the aleatoric and 0.039 in the epistemic part: an error of four times the mutual information.  The constants below
are 2 x the measured figures."""
import ctypes
import math
import re

import pytest
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _rng, ops
from bayesianneuralnetworks_amd import nn as bnn_nn
from bayesianneuralnetworks_amd._rng import DrawKey
from bayesianneuralnetworks_amd.nn import (BayesianNetworkModule, LocalReparamLinear, MultivariateNormalLinear, NormalConv2d,
                                           NormalLinear)

from alignment import guards_intact, offset_view, output_view, same_bits
from bf16ref import gamma
from conftest import load_golden
from test_flipout_mc import _code_object_notes
from test_lrt_device import U, assert_within, scaled_bound
from test_moment_backward import recovered_eps

gpu = pytest.mark.gpu

L_REL_TOL = 1.93e-6             # 4 x the measured 4.816e-7 (module docstring)
L_ABS_TOL = 2.0 ** -63          # sqrt of the smallest normal fp32
E2E_MEAN_DEV, E2E_TOTAL_DEV, E2E_ALEATORIC_DEV, E2E_EPISTEMIC_DEV = 2 * 0.00094, 2 * 0.00181, 2 * 0.00143, 2 * 0.00038
E_NULL, E_SHAPE, E_ALIGN, E_RANGE, E_UNSUPPORTED = -1, -2, -4, -5, -6


def f64(t):
    return t.detach().double().cpu()


def mvn_params(O, K, bias, seed, plant=True):
    """A posterior of MultivariateNormalLinear(K, O): means ~ U / sqrt(K), scales ~ N(-2, 0.5) on the lower triangles with -100 and
    +20 (and 25, past softplus' threshold) planted, NaN above the diagonals -- what is never to be read."""
    g = torch.Generator().manual_seed(seed)

    def tri(*shape):
        s = -2.0 + 0.5 * torch.randn(*shape, generator=g)
        n = shape[-1]
        low = torch.tril(torch.ones(n, n, dtype=torch.bool))
        if plant:
            flat = s.reshape(-1, n, n)
            flat[:, n - 1, 0] = -100.0
            flat[:, n // 2, n // 2] = 20.0
            flat[:, n - 1, n // 3] = 25.0
            flat[0, 0, 0] = -100.0 if n > 1 else 20.0
        return torch.where(low, s, torch.full_like(s, float("nan")))

    mu_w = (torch.rand(O, K, generator=g) * 2 - 1) / K ** 0.5
    scale_w = tri(O, K, K)
    if not bias:
        return mu_w, scale_w, None, None
    return mu_w, scale_w, (torch.rand(O, generator=g) * 2 - 1) / K ** 0.5, tri(O, O)


def chunked_moments(draw, S, chunk, center):
    """Sample mean, covariance and their standard errors of S draws y (chunk, rows, N) = draw(chunk), accumulated around `center`
    (rows, N): the error of a covariance element is estimated from the sample's own fourth moment."""
    rows, N = center.shape
    s1 = torch.zeros(rows, N, dtype=torch.float64)
    s2 = torch.zeros(rows, N, N, dtype=torch.float64)
    s4 = torch.zeros(rows, N, N, dtype=torch.float64)
    for _ in range(S // chunk):
        d = draw(chunk).double() - center
        p = d.unsqueeze(-1) * d.unsqueeze(-2)
        s1 += d.sum(0)
        s2 += p.sum(0)
        s4 += (p * p).sum(0)
    n = (S // chunk) * chunk
    m1 = s1 / n
    cov = s2 / n - m1.unsqueeze(-1) * m1.unsqueeze(-2)
    se_cov = ((s4 / n - (s2 / n) ** 2).clamp_min(0) / n).sqrt()
    se_mean = (torch.diagonal(cov, dim1=-2, dim2=-1) / n).sqrt()
    return center + m1, se_mean, cov, se_cov


# ================================================================================================ CPU
def test_twin_against_sampling():
    """The float64 twins on the reference's own CIFAR10-head posterior (tests/golden/mvn_linear_128x10.npz) with a_m its x and
    a_v = 0.1 a_m^2, against 2^17 draws of the layer's own torch expression (w = mu + sqrt(variance) u, u = torch.rand) on Gaussian
    inputs: m, v and every element of cov within 5 standard errors -- and some off-diagonal element of the sampled covariance more
    than 10 standard errors from zero, so the diagonal pass would fail here."""
    gold = load_golden("mvn_linear_128x10")
    mu_w, scale_w, mu_b, scale_b, a_m = (torch.from_numpy(gold[k]) for k in ("mu_w", "scale_w", "mu_b", "scale_b", "x"))
    a_v = 0.1 * a_m * a_m
    mom = ops.moments_mvn_linear_f64(ops.Moments(a_m, a_v), mu_w, scale_w, mu_b, scale_b)
    E_w, G_w, E_b, C_b = ops.mvn_moments_prepare_f64(mu_w, scale_w, mu_b, scale_b)
    cov = ops.moments_head_cov_f64(ops.HeadOperands(a_v, E_w, C_b), mom.var)
    assert mom.mean.dtype == torch.float64 and cov.shape == (16, 10, 10)
    assert torch.equal(torch.diagonal(cov, dim1=-2, dim2=-1), mom.var) and torch.equal(cov, cov.transpose(-1, -2))

    g = torch.Generator().manual_seed(1217)
    low_w = torch.tril(torch.nn.functional.softplus(scale_w)) + 1e-10 * torch.eye(128)        # WeightMultivariateNormal.variance
    low_b = torch.tril(torch.nn.functional.softplus(scale_b)) + 1e-10 * torch.eye(10)
    sd_w, sd_b = low_w.sqrt(), low_b.sqrt()                                                    # .stddev
    sd_a = a_v.sqrt()

    def draw(n):
        w = mu_w + torch.einsum("okj,soj->sok", sd_w, torch.rand(n, 10, 128, generator=g))     # .sample(), one per draw
        b = mu_b + torch.einsum("oj,sj->so", sd_b, torch.rand(n, 10, generator=g))
        a = a_m + sd_a * torch.randn(n, 16, 128, generator=g)
        return torch.einsum("sbk,sok->sbo", a.double(), w.double()) + b.double().unsqueeze(1)

    mean, se_mean, scov, se_cov = chunked_moments(draw, 1 << 17, 1 << 12, mom.mean)
    z_m = ((mom.mean - mean).abs() / se_mean).max().item()
    z_c = ((cov - scov).abs() / se_cov).max().item()
    off = ~torch.eye(10, dtype=torch.bool)
    z_off = (scov.abs() / se_cov)[:, off].max().item()
    print("mean: worst %.2f standard errors; covariance (the variance on its diagonal): worst %.2f; largest off-diagonal element of "
          "the sampled covariance: %.1f standard errors from zero" % (z_m, z_c, z_off))
    assert z_m <= 5 and z_c <= 5, (z_m, z_c)
    assert z_off > 10, z_off
    # the restatement above is the layer's: 4096 forwards of a MultivariateNormalLinear that holds this posterior (its own
    # sample() on torch's global generator) against the same moments, at 6 standard errors
    layer = MultivariateNormalLinear(128, 10)
    with torch.no_grad():
        for p, t in ((layer.weight.mean, mu_w), (layer.weight.scale, scale_w), (layer.bias.mean, mu_b), (layer.bias.scale, scale_b)):
            p.copy_(t)
    torch.manual_seed(77)

    def forwards(n):
        with torch.no_grad():
            return torch.stack([layer(a_m + sd_a * torch.randn(16, 128)) for _ in range(n)])

    mean, se_mean, scov, se_cov = chunked_moments(forwards, 1 << 12, 1 << 10, mom.mean)
    z_m, z_c = ((mom.mean - mean).abs() / se_mean).max().item(), ((cov - scov).abs() / se_cov).max().item()
    print("the layer's own forward, 4096 calls: mean worst %.2f standard errors, covariance worst %.2f" % (z_m, z_c))
    assert z_m <= 6 and z_c <= 6, (z_m, z_c)


class Mlp(BayesianNetworkModule):
    def __init__(self, *mods, samples=4):
        super().__init__(1, 1, samples=samples)
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


def test_head_covariance_is_exact_behind_one_hidden_layer():
    """NormalLinear(6, 16) -> folded ReLU -> NormalLinear(16, 4) on a deterministic input: the hidden activations are independent,
    so predictive_moments(covariance=True).cov is the covariance of the logits -- 2^18 sampled logits, 5 standard errors."""
    torch.manual_seed(3)
    net = Mlp(NormalLinear(6, 16), torch.nn.ReLU(), NormalLinear(16, 4))
    with torch.no_grad():
        for layer in (net.layers[0], net.layers[2]):
            layer.weight.scale.fill_(-1.0)
            layer.bias.scale.fill_(-1.5)
    assert bnn_nn.fuse_activations(net) == 1
    g = torch.Generator().manual_seed(31)
    x = torch.randn(3, 6, generator=g)
    mom = net.predictive_moments(x, covariance=True)
    plain = net.predictive_moments(x)
    assert plain.cov is None and torch.equal(plain.mean, mom.mean) and torch.equal(plain.var, mom.var)
    assert mom.cov.shape == (3, 4, 4) and mom.cov.dtype == torch.float32
    assert torch.equal(torch.diagonal(mom.cov, dim1=-2, dim2=-1), mom.var)
    l1, l2 = net.layers[0], net.layers[2]

    def normal(p, n):
        return p.mean.detach() + p.stddev.detach() * torch.randn((n,) + tuple(p.mean.shape), generator=g)

    def draw(n):
        h = (torch.einsum("bk,snk->sbn", x, normal(l1.weight, n)) + normal(l1.bias, n).unsqueeze(1)).clamp_min(0)
        return torch.einsum("sbk,snk->sbn", h, normal(l2.weight, n)) + normal(l2.bias, n).unsqueeze(1)

    mean, se_mean, scov, se_cov = chunked_moments(draw, 1 << 18, 1 << 14, mom.mean.double())
    z_m = ((mom.mean.double() - mean).abs() / se_mean).max().item()
    z_c = ((mom.cov.double() - scov).abs() / se_cov).max().item()
    off = ~torch.eye(4, dtype=torch.bool)
    print("6-16-4: mean worst %.2f standard errors, covariance worst %.2f; largest sampled off-diagonal %.1f standard errors from zero"
          % (z_m, z_c, (scov.abs() / se_cov)[:, off].max().item()))
    assert z_m <= 5 and z_c <= 5, (z_m, z_c)


class ConvEnded(BayesianNetworkModule):
    def __init__(self):
        super().__init__(1, 2)
        self.conv = NormalConv2d(1, 2, 3)

    def _forward(self, x):
        return self.conv(x)


def test_cov_plumbing():
    g = torch.Generator().manual_seed(7)
    m, v = torch.randn(2, 3, 4, generator=g), torch.rand(2, 3, 4, generator=g)
    c = torch.randn(2, 3, 4, 4, generator=g)
    two = ops.Moments(m, v)                                                     # the two-argument constructor still works
    assert two.cov is None and two.link is None and two._head is None
    assert repr(two) == "Moments(mean=%r, var=%r)" % (m, v)                     # repr is unchanged without a cov
    assert repr(ops.Moments(m, v, "softmax")) == "Moments(mean=%r, var=%r, link='softmax')" % (m, v)
    mom = ops.Moments(m, v, cov=c)
    assert mom.cov is c and "cov=" in repr(mom)
    with pytest.raises(ValueError, match="cov"):
        ops.Moments(m, v, cov=c[..., :3])
    # every reshape drops it
    for out in (mom.view(6, 4), mom.reshape(2, 12), mom.flatten(1), mom.flatten()):
        assert out.cov is None and out._head is None
    # every layer and activation drops it; the softmax twin keeps it
    flat = ops.Moments(m.reshape(6, 4), v.reshape(6, 4), cov=c.reshape(6, 4, 4))
    flat._head = ops.HeadOperands(None, torch.zeros(4, 4), None)
    lin, lrt, mvn, det = NormalLinear(4, 3), LocalReparamLinear(4, 3), MultivariateNormalLinear(4, 3), bnn_nn.MomentLinear(4, 3)
    from bayesianneuralnetworks_amd import _mc
    with _mc.MomentContext():
        outs = [lin(flat), lrt(flat), mvn(flat), det(flat), bnn_nn.MomentReLU()(flat), bnn_nn.MomentELU()(flat)]
        kept = bnn_nn.MomentSoftmax(dim=-1)(flat)
    for out in outs:
        assert isinstance(out, ops.Moments) and out.cov is None and out._head is None
    assert kept.cov is flat.cov and kept._head is flat._head and kept.link == "softmax"
    # and so do the conv layers, the pooling twins and an eval-mode BatchNorm, fed image moments that carry a cov and head operands
    img = ops.Moments(torch.randn(2, 2, 4, 4, generator=g), torch.rand(2, 2, 4, 4, generator=g), cov=torch.randn(2, 2, 4, 4, 4, generator=g))
    img._head = flat._head
    from bayesianneuralnetworks_amd.nn import LocalReparamConv2d
    with _mc.MomentContext(covariance=True):
        outs = [NormalConv2d(2, 3, 3)(img), LocalReparamConv2d(2, 3, 3)(img), bnn_nn.MomentMaxPool2d(2)(img), bnn_nn.MomentAvgPool2d(2)(img),
                bnn_nn.MomentAdaptiveAvgPool2d(2)(img), bnn_nn.MomentBatchNorm2d(2).eval()(img)]
    for out in outs:
        assert isinstance(out, ops.Moments) and out.var is not None and out.cov is None and out._head is None
    # in a covariance pass the dense layers leave their operands; a layer wider than 32 and an activation behind a layer do not
    with _mc.MomentContext(covariance=True):
        assert all(layer(flat)._head is not None for layer in (lin, lrt, mvn, det))
        assert NormalLinear(4, 33)(flat)._head is None and MultivariateNormalLinear(4, 33)(flat)._head is None
        assert bnn_nn.MomentReLU()(lin(flat))._head is None
        relu = NormalLinear(4, 3)
        relu.activation = 'relu'
        assert relu(flat)._head is None                                         # a folded ReLU stands behind the contraction
    x = torch.randn(5, 4, generator=g)
    # covariance=True: what raises
    with pytest.raises(ops.BnnHipError, match="its last layer is not dense"):
        ConvEnded().predictive_moments(torch.randn(2, 1, 5, 5, generator=g), covariance=True)
    with pytest.raises(ops.BnnHipError, match="its head NormalLinear has 33 outputs"):
        Mlp(NormalLinear(4, 33)).predictive_moments(x, covariance=True)
    with pytest.raises(ops.BnnHipError, match="behind its last dense layer NormalLinear"):
        Mlp(NormalLinear(4, 3), bnn_nn.MomentReLU()).predictive_moments(x, covariance=True)
    net = Mlp(NormalLinear(4, 8), bnn_nn.MomentReLU(), MultivariateNormalLinear(8, 3), bnn_nn.MomentSoftmax(dim=-1))
    for call in (lambda **k: net.predictive_mean(x, samples=2, **k),
                 lambda **k: net.predictive_uncertainty(x, samples=2, inputs="probs", **k),
                 lambda **k: net.predictive_score(x, torch.zeros(5, dtype=torch.int64), samples=2, inputs="probs", **k),
                 lambda **k: net.predictive_regression(x, samples=2, outputs="values", **k),
                 lambda **k: net.predictive_regression_score(x, torch.zeros(5, 3), samples=2, outputs="values", **k)):
        with pytest.raises(ValueError, match="covariance"):
            call(covariance=True)                                               # propagation='samples'
        with pytest.raises(ValueError):
            call(covariance=True, propagation="moment")
    mom = net.predictive_moments(x, covariance=True)
    assert mom.link == "softmax" and mom.cov.shape == (5, 3, 3) and mom.cov.dtype == torch.float32
    assert torch.equal(torch.diagonal(mom.cov, dim1=-2, dim2=-1), mom.var)
    # the tails with covariance=True read correlated draws of these moments
    torch.manual_seed(5)
    u = net.predictive_uncertainty(x, samples=8, inputs="probs", propagation="moments", covariance=True)
    torch.manual_seed(5)
    ys = torch.softmax(ops.moments_sample(mom, None, 8), -1)
    assert all(torch.equal(a, b) for a, b in zip(u, ops.uncertainty_f64(ys, "probs")))
    torch.manual_seed(5)
    assert not torch.equal(ys, torch.softmax(ops.moments_sample(ops.Moments(mom.mean, mom.var), None, 8), -1))
    # no backward: forward_moments keeps refusing the layer by name, sample_moments refuses a covariance
    with pytest.raises(ops.BnnHipError, match="MultivariateNormalLinear"):
        net.forward_moments(x)
    with pytest.raises(ops.BnnHipError, match="covariance"):
        net.sample_moments(mom, samples=2)
    with pytest.raises(ops.BnnHipError, match="covariance"):
        ops.moments_sample(ops.Moments(mom.mean.clone().requires_grad_(), mom.var, cov=mom.cov), None, 2, track=True)
    with pytest.raises(ops.BnnHipError, match="inference only"):
        ops.moments_mvn_linear_f64(x, *mvn._posterior(), track=True)
    with pytest.raises(ops.BnnHipError, match="inference only"):
        ops.moments_mvn_linear(x, *mvn._posterior(), track=True)


def test_cholesky_pivot_rule():
    """A pivot <= 0 gives a zero column: [[1, 1], [1, 1]] moves both outputs by the same amount, bit for bit; a zero covariance
    gives y == m; a diagonal covariance is moments_sample up to the rounding of sqrt(v) against sqrt(v + 1e-16)."""
    L = ops.cholesky_pivot_f64(torch.tensor([[1.0, 1.0], [1.0, 1.0]]))
    assert torch.equal(L, torch.tensor([[1.0, 0.0], [1.0, 0.0]], dtype=torch.float64))
    g = torch.Generator().manual_seed(11)
    A = torch.randn(5, 6, 6, generator=g, dtype=torch.float64)
    A = A @ A.transpose(-1, -2) + 0.1 * torch.eye(6, dtype=torch.float64)
    assert (ops.cholesky_pivot_f64(A) - torch.linalg.cholesky(A)).abs().max() <= 1e-12
    m = torch.full((3, 2), 0.25)
    ones = torch.ones(3, 2, 2)
    torch.manual_seed(2)
    y = ops.moments_sample(ops.Moments(m, torch.ones(3, 2), cov=ones), None, 4)
    assert y.shape == (4, 3, 2) and same_bits(y[..., 0] - m[..., 0], y[..., 1] - m[..., 1]) and (y[..., 0] != 0.25).all()
    mm = torch.randn(3, 4, generator=g)
    assert torch.equal(ops.moments_sample(ops.Moments(mm, torch.zeros(3, 4), cov=torch.zeros(3, 4, 4)), None, 3), mm.expand(3, 3, 4))
    v = 0.1 + torch.rand(3, 4, generator=g)
    torch.manual_seed(9)
    want = ops.moments_sample(ops.Moments(mm, v), None, 5)
    torch.manual_seed(9)
    got = ops.moments_sample(ops.Moments(mm, v, cov=torch.diag_embed(v)), None, 5)
    # both are one fp32 rounding of a float64 value; the values differ by |eps| (sqrt(v + 1e-16) - sqrt(v)) <= |eps| 5e-17 / sqrt(v)
    assert (got.double() - want.double()).abs().max() <= 2 * U * want.abs().max()


def test_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one = ctypes.c_void_p(16)
    odd = ctypes.c_void_p(18)
    r = ctypes.byref(_lib.Rng(seed=1, stream=8))
    prep = lambda **k: lib.bnn_mvn_moments_prepare(*[k.get(n, one) for n in ("mu_w", "scale_w", "mu_b", "scale_b", "E_w", "G_w", "E_b", "C_b")],  # noqa: E731
                                                   k.get("O", 3), k.get("K", 7), None)
    assert prep(mu_w=None) == E_NULL and prep(E_b=None) == E_NULL and prep(mu_b=None, scale_b=None, E_b=None) == E_NULL
    assert prep(K=0) == E_SHAPE and prep(K=4097) == E_RANGE and prep(O=4097) == E_RANGE and prep(G_w=odd) == E_ALIGN
    fwd = lambda **k: lib.bnn_mvn_moments_forward(k.get("a_m", one), k.get("a_v", one), k.get("lda", 7), one, one, one, k.get("E_b", one),  # noqa: E731
                                                  k.get("C_b", one), one, k.get("out_v", one), k.get("B", 5), 3, k.get("K", 7), None)
    assert fwd(a_m=None) == E_NULL and fwd(E_b=None) == E_NULL and fwd(lda=6) == E_SHAPE and fwd(K=4097, lda=4097) == E_RANGE
    assert fwd(B=64 * 65535 + 1) == E_RANGE and fwd(out_v=odd) == E_ALIGN and fwd(B=0) == 0
    cov = lambda **k: lib.bnn_moments_head_cov(k.get("a_v", one), k.get("lda", 7), k.get("E", one), one, k.get("var", one), k.get("cov", one),  # noqa: E731
                                               5, k.get("N", 3), 7, None)
    assert cov(var=None) == E_NULL and cov(E=None) == E_NULL and cov(lda=6) == E_SHAPE and cov(N=33) == E_RANGE and cov(cov=odd) == E_ALIGN
    smp = lambda **k: lib.bnn_moments_sample_cov(k.get("m", one), one, k.get("y", one), 5, k.get("N", 3), k.get("S", 2), k.get("rng", r),  # noqa: E731
                                                 k.get("flags", 0), None)
    assert smp(m=None) == E_NULL and smp(rng=None) == E_NULL and smp(S=0) == E_SHAPE and smp(N=33) == E_RANGE and smp(S=70000) == E_RANGE
    assert smp(flags=1) == E_UNSUPPORTED and smp(y=odd) == E_ALIGN
    assert lib.bnn_launch_count() == n0


def test_head_kernels_do_not_spill():
    """The four new kernels use no scratch and spill nothing; read the way test_pool_kernels_do_not_spill reads the notes."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    mine = {n: f for n, f in kernels.items()
            if re.match(r"_ZN3bnn(21k_moments_mvn_prepareE|21k_moments_mvn_forwardE|18k_moments_head_covE|20k_moments_sample_covE)", n)}
    assert len(mine) == 4, sorted(kernels)
    for n, f in mine.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0 and \
            int(f.get("private_segment_fixed_size", 0)) == 0, (n, f)


class Flatten(torch.nn.Module):
    def forward(self, x):
        return x.view(x.size(0), -1)


def reduced_cifar10(seed):
    """The CIFAR10 example's layer sequence with its real head at reduced widths: 8 / 16 channels, 16 x 16 images (2 x 2 behind the
    three stride-2 convolutions), Linear(64, 32), MultivariateNormalLinear(32, 10)."""
    c2, elu = torch.nn.Conv2d, torch.nn.ELU
    torch.manual_seed(seed)
    mods = [c2(3, 8, 5, padding=2, stride=2), torch.nn.BatchNorm2d(8), elu(), c2(8, 16, 5, padding=2, stride=2), elu(),
            c2(16, 16, 5, padding=2, stride=2), elu(), c2(16, 16, 3, padding=1), elu(), c2(16, 16, 3, padding=1), elu(),
            NormalConv2d(16, 16, 3, padding=1), elu(), Flatten(), torch.nn.Linear(64, 32), elu(), MultivariateNormalLinear(32, 10),
            torch.nn.Softmax(dim=-1)]
    net = Mlp(*mods).eval()
    with torch.no_grad():                               # a conv posterior wide enough for the uncertainty to show; a head whose
        net.layers[11].weight.scale.fill_(-2.0)         # factor's row sums (up to 32 elements of sqrt(softplus)) do not saturate the softmax
        head = net.layers[16]
        head.weight.scale.copy_(torch.where(torch.tril(torch.ones(32, 32)).bool(), torch.full((10, 32, 32), -6.0), head.weight.scale))
    assert bnn_nn.moment_activations(net) > 0
    return net


def test_reduced_cifar10_on_the_cpu():
    net = reduced_cifar10(4)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(4, 3, 16, 16, generator=g)
    S = 4096
    mom = net.predictive_moments(x, covariance=True)
    assert mom.link == "softmax" and mom.cov.shape == (4, 10, 10) and torch.isfinite(mom.cov).all()
    assert torch.equal(torch.diagonal(mom.cov, dim1=-2, dim2=-1), mom.var) and torch.equal(mom.cov, mom.cov.transpose(-1, -2))
    assert (torch.linalg.eigvalsh(mom.cov.double()) > -1e-9).all()
    torch.manual_seed(6)
    u = net.predictive_uncertainty(x, samples=S, inputs="probs", propagation="moments", covariance=True)
    torch.manual_seed(7)
    ref = net.predictive_uncertainty(x, samples=S, inputs="probs")
    for r in (u, ref):
        assert all(torch.isfinite(t).all() for t in r) and (r.mean.sum(-1) - 1).abs().max() <= 1e-5
        assert (r.total - r.aleatoric - r.epistemic).abs().max() <= 1e-5            # the parts sum as the sampled path's do
    devs = [(a - b).abs().max().item() for a, b in zip(u, ref)]
    torch.manual_seed(6)
    diag = net.predictive_uncertainty(x, samples=S, inputs="probs", propagation="moments")
    print("the same pass with independent logits: %.4f, %.4f, %.4f, %.4f; the sampler's epistemic part is %.4f nats at the most"
          % (*[(a - b).abs().max().item() for a, b in zip(diag, ref)], ref.epistemic.max().item()))
    print("reduced CIFAR10, 4 rows, S = %d: moments with covariance against the serial sampler: worst |mean probability difference| "
          "%.4f, |total| %.4f, |aleatoric| %.4f, |epistemic| %.4f nats" % (S, *devs))
    assert devs[0] <= E2E_MEAN_DEV and devs[1] <= E2E_TOTAL_DEV and devs[2] <= E2E_ALEATORIC_DEV and devs[3] <= E2E_EPISTEMIC_DEV, devs


# ================================================================================================ GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


def factor64(scale):
    return ops.mvn_factor_f64(torch.nan_to_num(scale, nan=0.0))


def factor_err(L):
    """What the device's L may differ from the float64 L by, element by element (zero above the diagonal: never formed)."""
    return torch.where(L > 0, L_REL_TOL * L + L_ABS_TOL, torch.zeros_like(L))


@gpu
def test_factor_element_deviation(dev):
    """mvn_l on the device against float64, read through a K = 1 layer with zero means (E_w = L / 2 exactly): the worst relative
    deviation over 4096 scales in [-87, 25] is printed -- L_REL_TOL is 4 x the figure measured -- and below the normal range the
    absolute bound holds."""
    scale = torch.cat([torch.linspace(-87.0, 25.0, 4096), torch.linspace(-104.0, -87.5, 256)])
    O = scale.numel()
    E_w, _, _, _ = ops.mvn_moments_prepare(torch.zeros(O, 1, device=dev), scale.reshape(O, 1, 1).to(dev), None, None)
    got = 2.0 * f64(E_w).reshape(-1)
    want = ops.mvn_factor_f64(scale.reshape(O, 1, 1)).reshape(-1)
    rel = ((got - want).abs() / want)[:4096].max().item()
    print("mvn_l against float64 over scale in [-87, 25]: worst relative deviation %.3e (L_REL_TOL = %.3e)" % (rel, L_REL_TOL))
    assert_within(got, want, factor_err(want), "L")


@gpu
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("OK", [(1, 1), (3, 7), (10, 128), (2, 257)], ids=lambda s: "x".join(map(str, s)))
def test_prepare_matches_float64(dev, OK, bias):
    O, K = OK
    mu_w, scale_w, mu_b, scale_b = mvn_params(O, K, bias, 100 + K)
    E_w, G_w, E_b, C_b = ops.mvn_moments_prepare(*[None if t is None else t.to(dev) for t in (mu_w, scale_w, mu_b, scale_b)])
    rE, rG, rEb, rCb = ops.mvn_moments_prepare_f64(mu_w, torch.nan_to_num(scale_w), mu_b, None if scale_b is None else torch.nan_to_num(scale_b))

    def mean_bound(L, mu, E):
        # the row sum: the error of every L and gamma(n) sum |addends|; then one fma
        n = L.shape[-1]
        return 0.5 * (factor_err(L).sum(-1) + gamma(n) * L.sum(-1)) + U * E.abs()

    L = factor64(scale_w)
    bE = mean_bound(L, mu_w.double(), rE)
    D = (L * L).sum(-1) / 12.0
    bD = ((2 * L * factor_err(L) + factor_err(L) ** 2).sum(-1) + gamma(K + 2) * (L * L).sum(-1)) / 12.0
    bG = 2 * rE.abs() * bE + bE * bE + bD + U * rG.abs()
    assert_within(E_w, rE, bE, "E_w")
    assert_within(G_w, rG, bG, "G_w")
    assert (f64(G_w) >= D * (1 - 1e-5)).all()
    if bias:
        Lb = factor64(scale_b)
        assert_within(E_b, rEb, mean_bound(Lb, mu_b.double(), rEb), "E_b")
        prod = Lb.unsqueeze(1) * Lb.unsqueeze(0)                                      # [o, p, j]
        eb = factor_err(Lb)
        bC = ((Lb.unsqueeze(1) * eb.unsqueeze(0) + eb.unsqueeze(1) * Lb.unsqueeze(0) + eb.unsqueeze(1) * eb.unsqueeze(0)).sum(-1)
              + gamma(O + 2) * prod.sum(-1)) / 12.0
        assert_within(C_b, rCb, bC, "C_b")
        assert same_bits(C_b, C_b.t().contiguous())
    else:
        assert E_b is None and C_b is None
    _lib.check_device(dev)


# K*: one past the forward kernel's panel (32 rows of L per LDS panel) and one past its slab (64 columns per sweep)
FWD_CASES = [(1, 1, 1), (5, 3, 7), (67, 10, 128), (3, 2, 33), (3, 2, 65)]


@gpu
@pytest.mark.parametrize("pitch", [0, 5], ids=["dense", "lda"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("var", [True, False])
@pytest.mark.parametrize("BOK", FWD_CASES, ids=lambda s: "x".join(map(str, s)))
def test_forward_matches_float64(dev, BOK, var, bias, pitch):
    """bnn_mvn_moments_forward against the twin fed the device's own prepare outputs: m within gamma(K + 1) sum |addends|; v within
    the error the factor's elements carry into the quadratic form plus gamma(n) sum |addends| of its chains.  One input row is
    all zero: its m and v are the bias terms, exactly."""
    B, O, K = BOK
    mu_w, scale_w, mu_b, scale_b = mvn_params(O, K, bias, 200 + K)
    g = torch.Generator().manual_seed(300 + B)
    lda = K + pitch
    am_full, av_full = torch.randn(B, lda, generator=g), 0.3 * torch.rand(B, lda, generator=g) ** 2
    am_full[B // 2, :K] = 0.0
    av_full[B // 2, :K] = 0.0
    am_full[:, K:] = float("nan")                                                # the pitch's padding is never read
    av_full[:, K:] = float("nan")
    am, av = am_full[:, :K], (av_full[:, :K] if var else None)
    d = lambda t: None if t is None else t.to(dev)                               # noqa: E731
    prepared = ops.mvn_moments_prepare(d(mu_w), d(scale_w), d(mu_b), d(scale_b))
    E_w, G_w, E_b, C_b = prepared
    amd, avd = am_full.to(dev), av_full.to(dev)
    out_m, out_v = torch.empty(B, O, device=dev), torch.empty(B, O, device=dev)
    sw = scale_w.to(dev)
    _lib.check(_lib.load().bnn_mvn_moments_forward(_lib.ptr(amd), _lib.ptr(avd) if var else None, lda, _lib.ptr(sw), _lib.ptr(E_w),
                                                   _lib.ptr(G_w), _lib.ptr(E_b), _lib.ptr(C_b), _lib.ptr(out_m), _lib.ptr(out_v), B, O, K,
                                                   _lib.stream_ptr(dev)), "bnn_mvn_moments_forward")
    ref = ops.moments_mvn_linear_f64(ops.Moments(am, av), mu_w, torch.nan_to_num(scale_w), mu_b, scale_b,
                                     prepared=[None if t is None else t.cpu() for t in prepared])
    if pitch == 0:                                                               # the host wrapper is the same launch
        got = ops.moments_mvn_linear(ops.Moments(d(am.contiguous()), d(av)), d(mu_w), sw, d(mu_b), d(scale_b), prepared=prepared)
        assert same_bits(got.mean, out_m) and same_bits(got.var, out_v)
    L = factor64(scale_w)
    a64, E64, G64 = am.double(), f64(E_w), f64(G_w)
    abs_m = a64.abs() @ E64.abs().t() + (f64(E_b).abs() if bias else 0.0)
    t = torch.einsum("bk,okj->boj", a64, L)
    dt = torch.einsum("bk,okj->boj", a64.abs(), factor_err(L)) + gamma(K) * torch.einsum("bk,okj->boj", a64.abs(), L)
    quad = (t * t).sum(-1) / 12.0
    lin = av.double() @ G64.t() if var else torch.zeros_like(quad)
    cbb = torch.diagonal(f64(C_b)) if bias else torch.zeros(O, dtype=torch.float64)
    bound_m = gamma(K + 1) * abs_m
    bound_v = (2 * t.abs() * dt + dt * dt).sum(-1) / 12.0 + gamma(K + 4) * (quad + lin + cbb)
    assert_within(out_m, ref.mean, bound_m, "m")
    assert_within(out_v, ref.var, bound_v, "v")
    z = B // 2                                                                   # the all-zero row: exact
    if bias:
        assert same_bits(out_m[z], E_b) and same_bits(out_v[z], torch.diagonal(C_b).contiguous())
    else:
        assert (out_m[z] == 0).all() and (out_v[z] == 0).all()
    assert_within(out_m, ref.mean, scaled_bound(ref.mean), "m, the 1e-5 scaled bound")
    assert_within(out_v, ref.var, scaled_bound(ref.var), "v, the 1e-5 scaled bound")
    _lib.check_device(dev)


COV_CASES = [(1, 1, 1), (5, 2, 3), (33, 10, 130), (7, 32, 65)]


def cov_inputs(B, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    E = (torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5
    a_v = 0.5 * torch.rand(B, K, generator=g) ** 2
    C = torch.randn(N, N, generator=g)
    C_b = (C @ C.t() / N).contiguous()
    var = 0.1 + torch.rand(B, N, generator=g)
    return E, a_v, C_b, var


@gpu
@pytest.mark.parametrize("with_cb", [True, False], ids=["C_b", "no-C_b"])
@pytest.mark.parametrize("with_av", [True, False], ids=["a_v", "deterministic"])
@pytest.mark.parametrize("BNK", COV_CASES, ids=lambda s: "x".join(map(str, s)))
def test_head_cov_matches_float64(dev, BNK, with_av, with_cb):
    B, N, K = BNK
    E, a_v, C_b, var = cov_inputs(B, N, K, 400 + K)
    head = ops.HeadOperands(a_v if with_av else None, E, C_b if with_cb else None)
    cov = ops.moments_head_cov(ops.HeadOperands(*[None if t is None else t.to(dev) for t in head]), var.to(dev))
    ref = ops.moments_head_cov_f64(head, var)
    # per element: the product E_o E_p is rounded, then K fmas and the bias term: gamma(K + 2) sum |addends|
    addends = torch.einsum("ok,pk,bk->bop", E.double().abs(), E.double().abs(), a_v.double()) if with_av else torch.zeros(B, N, N, dtype=torch.float64)
    if with_cb:
        addends = addends + C_b.double().abs()
    bound = gamma(K + 2) * addends
    bound[:, torch.arange(N), torch.arange(N)] = 0.0                                # the diagonal is var's bits
    assert_within(cov, ref, bound, "cov")
    assert same_bits(cov, cov.transpose(-1, -2).contiguous())
    assert same_bits(torch.diagonal(cov, dim1=-2, dim2=-1).contiguous(), var.to(dev))
    _lib.check_device(dev)


@gpu
def test_head_cov_refuses_33_outputs_before_any_launch(dev):
    lib = _lib.load()
    E, a_v, C_b, var = [t.to(dev) for t in cov_inputs(2, 33, 5, 1)]
    n0 = lib.bnn_launch_count()
    with pytest.raises(ops.BnnHipError, match="33"):
        ops.moments_head_cov(ops.HeadOperands(a_v, E, C_b), var)
    cov = torch.empty(2, 33, 33, device=dev)
    assert lib.bnn_moments_head_cov(_lib.ptr(a_v), 5, _lib.ptr(E), _lib.ptr(C_b), _lib.ptr(var), _lib.ptr(cov), 2, 33, 5,
                                    _lib.stream_ptr(dev)) == E_RANGE
    assert lib.bnn_launch_count() == n0


def spd(rows, N, seed):
    """Random symmetric positive definite fp32 matrices with eigenvalues log-uniform in [1.2e-3, 1e3], the two ends present in every
    matrix of more than one row: condition numbers up to 8.3e5 before the rounding to fp32, which moves the smallest eigenvalue by
    a few per cent (the test verifies cond <= 1e6 on the rounded matrices)."""
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.randn(rows, N, N, generator=g, dtype=torch.float64))
    lam = torch.exp(torch.empty(rows, N, dtype=torch.float64).uniform_(math.log(1.2e-3), math.log(1e3), generator=g))
    if N > 1:
        lam[:, 0], lam[:, -1] = 1.2e-3, 1e3
    A = (Q * lam.unsqueeze(-2)) @ Q.transpose(-1, -2)
    A = (0.5 * (A + A.transpose(-1, -2))).float()
    return A, torch.randn(rows, N, generator=g)


def sample_key(S, stream=77):
    return DrawKey(0x1234567890ABCDEF, stream, 3, S, 17, gen=_rng.generator_for("f32"))          # sample0 = 3


@gpu
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("N", [1, 2, 10, 32])
def test_sampler_matches_float64_on_the_recovered_eps(dev, N, rows, S):
    """y - m = Lc eps with eps recovered from a bnn_moments_sample launch on the same key at unit variance: within one fp32
    rounding of y plus the float64 factorization's backward error (N + 1) 2^-53 cond (in units of sum_k |Lc_ik| |eps_k|)."""
    cov, m = spd(rows, N, 500 + N)
    ev = torch.linalg.eigvalsh(cov.double())
    cond = (ev[:, -1] / ev[:, 0])
    assert (ev[:, 0] > 0).all() and cond.max() <= 1e6 and (N == 1 or cond.max() >= 5e5), cond.max()
    key = sample_key(S)
    md, cd = m.to(dev), cov.to(dev)
    zero, one = torch.zeros(rows, N, device=dev), torch.ones(rows, N, device=dev)
    eps = recovered_eps(ops.moments_sample(ops.Moments(zero, one), key, S), zero, one)
    y = ops.moments_sample(ops.Moments(md, one, cov=cd), key, S)
    assert y.shape == (S, rows, N) and y.dtype == torch.float32
    Lc = ops.cholesky_pivot_f64(cov)
    ref = m.double() + torch.einsum("bik,sbk->sbi", Lc, eps)
    mag = torch.einsum("bik,sbk->sbi", Lc.abs(), eps.abs())
    bound = U * ref.abs() + (N + 1) * 2.0 ** -53 * cond.reshape(1, rows, 1) * mag + 1e-300
    assert_within(y, ref, bound, "y")
    assert same_bits(y, ops.moments_sample(ops.Moments(md, None, cov=cd), key, S))              # identical calls, identical bits
    _lib.check_device(dev)


@gpu
def test_sampler_pivot_rule_on_the_device(dev):
    key = sample_key(4)
    m = torch.full((3, 2), 0.25, device=dev)
    y = ops.moments_sample(ops.Moments(m, None, cov=torch.ones(3, 2, 2, device=dev)), key, 4)
    assert same_bits(y[..., 0].contiguous(), y[..., 1].contiguous()) and (y[..., 0] != 0.25).all()
    unit = ops.moments_sample(ops.Moments(torch.zeros(3, 2, device=dev), torch.ones(3, 2, device=dev)), key, 4)
    assert (f64(y[..., 0]) - (0.25 + f64(unit[..., 0]))).abs().max() <= U * f64(y).abs().max()       # the first element's eps moves both
    g = torch.Generator().manual_seed(12)
    mm = torch.randn(5, 7, generator=g).to(dev)
    got = ops.moments_sample(ops.Moments(mm, None, cov=torch.zeros(5, 7, 7, device=dev)), key, 4)
    assert same_bits(got, mm.expand(4, 5, 7).contiguous())
    v = (0.1 + torch.rand(5, 7, generator=g)).to(dev)
    want = ops.moments_sample(ops.Moments(mm, v), key, 4)
    got = ops.moments_sample(ops.Moments(mm, v, cov=torch.diag_embed(v)), key, 4)
    assert (f64(got) - f64(want)).abs().max() <= 2 * U * f64(want).abs().max()
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("off", [4, 8])
def test_operands_off_16_bytes_give_the_same_bits(dev, off):
    """Every new entry reads and writes one element at a time, so operands one float off the 16-byte boundary are accepted: guards
    intact, the aligned call's bits."""
    lib = _lib.load()
    O, K, B, S = 3, 37, 9, 2
    mu_w, scale_w, mu_b, scale_b = [t.to(dev) for t in mvn_params(O, K, True, 600)]
    g = torch.Generator().manual_seed(601)
    am, av = torch.randn(B, K, generator=g).to(dev), (0.3 * torch.rand(B, K, generator=g)).to(dev)
    key = sample_key(S)
    r = ops._rng_struct(key, dev)
    st = _lib.stream_ptr(dev)
    p = _lib.ptr

    def run(o):
        inp = (lambda t: offset_view(t, o)) if o is not None else (lambda t: t)
        out = (lambda *shape: output_view(shape, torch.float32, dev, o)) if o is not None else (lambda *shape: torch.full(shape, -1.0, device=dev))
        a, b, c, d_, x, xv = [inp(t) for t in (mu_w, scale_w, mu_b, scale_b, am, av)]
        E_w, G_w, E_b, C_b = out(O, K), out(O, K), out(O), out(O, O)
        _lib.check(lib.bnn_mvn_moments_prepare(p(a), p(b), p(c), p(d_), p(E_w), p(G_w), p(E_b), p(C_b), O, K, st), "prepare")
        om, ov = out(B, O), out(B, O)
        _lib.check(lib.bnn_mvn_moments_forward(p(x), p(xv), K, p(b), p(E_w), p(G_w), p(E_b), p(C_b), p(om), p(ov), B, O, K, st), "forward")
        cov = out(B, O, O)
        _lib.check(lib.bnn_moments_head_cov(p(xv), K, p(E_w), p(C_b), p(ov), p(cov), B, O, K, st), "head_cov")
        y = out(S, B, O)
        _lib.check(lib.bnn_moments_sample_cov(p(om), p(cov), p(y), B, O, S, ctypes.byref(r), 0, st), "sample_cov")
        torch.cuda.synchronize()
        outs = [E_w, G_w, E_b, C_b, om, ov, cov, y]
        if o is not None:
            assert all(guards_intact(t) for t in outs)
        return outs

    for a, b in zip(run(off), run(None)):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b)
    _lib.check_device(dev)


@gpu
def test_graph_capture(dev):
    """The four launches on one stream in a captured graph: two replays give the eager bits."""
    O, K, B, S = 10, 70, 37, 3
    post = [t.to(dev) for t in mvn_params(O, K, True, 700)]
    g = torch.Generator().manual_seed(701)
    am, av = torch.randn(B, K, generator=g).to(dev), (0.3 * torch.rand(B, K, generator=g)).to(dev)
    key = sample_key(S)

    def step():
        prepared = ops.mvn_moments_prepare(*post)
        mom = ops.moments_mvn_linear(ops.Moments(am, av), *post, prepared=prepared)
        cov = ops.moments_head_cov(ops.HeadOperands(av, prepared[0], prepared[3]), mom.var)
        y = ops.moments_sample(ops.Moments(mom.mean, mom.var, cov=cov), key, S)
        return list(prepared) + [mom.mean, mom.var, cov, y]

    want = [t.clone() for t in step()]
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
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(x, y) for x, y in zip(got, want))
    _lib.check_device(dev)


# The reduced CIFAR10 net behind its deterministic trunk: conv (its ELU fused), the deterministic Linear, ELU, the MVN head, the head
# covariance -- 5 stages, each within 1e-5 of its output's scale in the fp32 mode (the bounds the conv and dense moment tests use), so
# the logit moments and covariances are within 5 x 1e-5 of float64's.  bf16 mode: the two contractions that read operands rounded to
# bf16 add 2^-8 sqrt(R) of the scale of their sums, R their reduction lengths: the 3 x 3 conv over 16 channels (144), Linear(64, 32)
# (64); the head's launches are fp32 in both modes.
CIFAR_R = (144, 64)
CIFAR_TOL = {"f32": 5e-5, "bf16": 5e-5 + 2.0 ** -8 * sum(math.sqrt(r) for r in CIFAR_R)}


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_reduced_cifar10_on_the_device(dev, mode):
    bnn.set_compute(mode)
    cpu = reduced_cifar10(4)
    net = reduced_cifar10(4)
    net.load_state_dict(cpu.state_dict())
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(41)
    x = torch.randn(5, 3, 16, 16, generator=g).to(dev)
    seen = []
    hook = net.layers[11].register_forward_pre_hook(lambda mod, args: seen.append(args[0]))     # the trunk's output of THIS pass
    lib = _lib.load()
    head = net.layers[16]
    got = net.predictive_moments(x, covariance=True)
    n0 = lib.bnn_launch_count()
    again = net.predictive_moments(x, covariance=True)
    n1 = lib.bnn_launch_count()
    hook.remove()
    plain = net.predictive_moments(x)
    assert lib.bnn_launch_count() - n1 == n1 - n0 - 1                           # the covariance is ONE more launch ...
    assert head.__dict__["_moments_cache"] is not None                          # ... and the prepare launch ran once, at the first pass
    assert all(same_bits(a, b) for a, b in zip((got.mean, got.var, got.cov), (again.mean, again.var, again.cov)))
    assert plain.cov is None and same_bits(plain.mean, got.mean) and same_bits(plain.var, got.var)
    tail = Mlp(*list(cpu.layers)[11:]).eval()
    ref = tail.predictive_moments(seen[0].detach().cpu(), covariance=True)
    assert got.link == "softmax" and got.cov.shape == (5, 10, 10)
    tol = CIFAR_TOL[mode]
    assert_within(got.mean, ref.mean, scaled_bound(ref.mean, tol), "logits m " + mode)
    assert_within(got.var, ref.var, scaled_bound(ref.var, tol), "logits v " + mode)
    assert_within(got.cov, ref.cov, scaled_bound(ref.cov, tol), "logits cov " + mode)
    assert same_bits(got.cov, got.cov.transpose(-1, -2).contiguous())
    bnn.manual_seed(9)
    u = net.predictive_uncertainty(x, samples=16, inputs="probs", propagation="moments", covariance=True)
    assert u.mean.shape == (5, 10) and (u.mean.sum(-1) - 1).abs().max() <= 1e-5
    assert all(torch.isfinite(t).all() for t in u) and (u.total >= 0).all()
    want = ops.mc_uncertainty(torch.softmax(ops.moments_sample(got, net.moment_key, 16), -1), "probs")
    assert all(torch.equal(a, b) for a, b in zip(u, want))
    _lib.check_device(dev)
