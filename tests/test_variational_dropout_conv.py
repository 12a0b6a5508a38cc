"""VariationalDropoutConv1d / 2d / 3d (K24, csrc/bnn_conv3d.hip): sparse variational dropout (Molchanov, Ashukha, Vetrov 2017) for
convolutions -- K23's posterior N(theta, exp(log_sigma2)) under the log-uniform prior on K11's layer,

    m = convNd(x, theta, mu_b),   v = convNd(x^2, exp(log_sigma2), sigma_b^2),   y_s = m + sqrt(v + 1e-16) eps_s,

eps[(b O + o) P + p] of the layer's noise key, sample sample0 + s (the LRT-conv noise contract).  CPU tests: the host surface, the
torch expression, the KL's dispatch, pruning and the two sparsity reports, the threshold, a seeded training run, the built code
object, the new entry's argument checks.  GPU tests: every path against float64 on the fp32 inputs as given, eps from the key's CPU
twin in oracle.

Bounds.  Forward: test_lrt_conv_device.check_forward's construction (the im2col panel against the dense weight: lrt64 and
forward_bound with K = (C / groups) taps), with the device's bnn_vd_prepare plane where that file takes bnn_lrt_prepare's; the plane
itself is held to float64 at test_variational_dropout.bound_s2 (3 u relative: ocml expf is a 1-ulp function, 2 u, and its result is
one fp32 number; one quantum 2^-149 where the result is denormal).  Backward: test_lrt_conv_device.check_backward's -- fp32 mode:
scaled_bound against float64 autograd of the formula; bf16 mode: g_m / g_v rounded as operands (bf16ref.round_hidden), the
contractions as bilinear maps in float64 with gamma_{R+1} of sum |a| |b|, the weight gradient with at most 16 slab sums on top
(gamma_{R+17}) -- with c_w = exp(log_sigma2) in float64 in place of 2 sigma sigmoid(rho).  The epilogue of k_lrt_conv_wsum<ChainLogSigma2> is
g_log_sigma2 = fl(t expf(l)) with t the fp32 slab sum: expf(l) = exp(l) (1 + d1), |d1| <= 2 u (1 ulp of the function), and the one
product rounds once, (1 + d2), |d2| <= u, so fl(t expf(l)) = t exp(l) (1 + d), |d| <= 3 u + 2 u^2 < 4 u.  With |t - t64| <= b_t:
|g - t64 exp(l)| <= b_t exp(l) (1 + 4 u) + 4 u |t64| exp(l), + 2^-149 where the product is denormal (EPI_U = 4 below; K11's own
epilogue, sigma, sigmoid and three products, allows 16 u).  That model of expf holds while its result is a normal number; below
l = ln 2^-126 = -87.3 it returns a denormal whose error is a quantum, which the product would multiply by |t|.  The kernel forms
the product in fp64 there (l < -87) and rounds once -- u relative or one quantum -- so the bound above, with its ONE quantum,
holds over the whole range; test_epilogue_over_the_parameters_range holds it to that.  g_theta is the slab sum itself: K11's
g_mu_w, bit for bit.

Launches.  Forward 2 (bnn_vd_prepare, ONE contraction for all S samples); backward 1 (g_m, g_v) + 1 (input gradient) + 2 (the
slabs, their reduce) + 1 with a bias = 5 with a bias, 4 without.  One training step of SmallNet (conv - ReLU - conv(groups 2) -
Flatten - dense; KLDivergence + cross-entropy + optim.Adam), DESIGN.md K24: forward 3 x 2 = 6; backward 4 (the first conv has no
input gradient) + 5 + 4 (the dense layer: K23) = 13; the log-uniform KL of the three weights 2 + 1; the Gaussian KL of the three
biases 2 + 1; optim.Adam 2 (k_adam on all twelve tensors, the device step counter's bump): 27.
"""
import ctypes
import math
import re

import pytest
import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, _rng, nn, ops, optim, prune
from bayesianneuralnetworks_amd.nn import (BayesianConvNd, BayesianNetworkModule, KLDivergence, NormalConvNd, LocalReparamConvNd,
                                           VariationalDropoutConvNd, VariationalDropoutConv1d, VariationalDropoutConv2d,
                                           VariationalDropoutConv3d, VariationalDropoutLinear, WeightNormal, WeightVariationalDropout)
from bayesianneuralnetworks_amd._rng import DrawKey
from bayesianneuralnetworks_amd.utils import apply_wb

from bf16ref import gamma, rne_bf16, round_hidden
from test_flipout_mc import _code_object_notes
from test_lrt_conv_device import BWD_CASES, CONV, FWD_CASES, Case, conv_eps
from test_lrt_device import EPS_TWIN, assert_within, forward_bound, lrt64, scaled_bound, sigma64
from test_moment_conv import ELU_MEAN_TOL, ELU_VAR_TOL, elu_deviation
from test_variational_dropout import bound_s2, kl64, log_alpha_raw64, wide_grid

U = 2.0 ** -24
EPI_U = 4                      # the epilogue's relative error in u: one 2-u expf and one product (the docstring's derivation)
STEP_LAUNCHES = 27             # one training step of SmallNet (the docstring's count)
gpu = pytest.mark.gpu
LAYER = {1: VariationalDropoutConv1d, 2: VariationalDropoutConv2d, 3: VariationalDropoutConv3d}


def vd_params(case, bias, seed):
    """(theta, log_sigma2, mu_b, rho_b): Case.params' means, log_sigma2 around -6 (sigma around e^-3, as that file's rho = -3)."""
    theta, rho_w, mu_b, rho_b = case.params(bias, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    return theta, -6 + 0.6 * torch.randn(theta.shape, generator=g), mu_b, rho_b


def formula64(case, x, theta, ls2, mu_b, rho_b, eps):
    """(y, m, v) of the formula in float64 with torch's conv; x (B, C, ...) or (S, B, C, ...), eps (S, B, O, ...)."""
    m = case.conv(x, theta, mu_b)
    v = case.conv(x * x, torch.exp(ls2), None if rho_b is None else sigma64(rho_b) ** 2)
    return m + torch.sqrt(v + 1e-16) * eps, m, v


class SmallNet(BayesianNetworkModule):
    """The issue's small net: (B, 3, 7, 7) -> 8 x 7 x 7 -> ReLU -> 6 x 3 x 3 (groups 2, stride 2) -> 54 -> 10."""

    def __init__(self, samples=4):
        super().__init__(3, 10, samples=samples)
        self.layers = torch.nn.Sequential(VariationalDropoutConv2d(3, 8, 3, padding=1), torch.nn.ReLU(),
                                          VariationalDropoutConv2d(8, 6, 3, stride=2, groups=2), torch.nn.Flatten(),
                                          VariationalDropoutLinear(6 * 3 * 3, 10))

    def _forward(self, x):
        return self.layers(x)


def vd_layers(net):
    return [m for m in net.modules() if isinstance(m, (VariationalDropoutConvNd, VariationalDropoutLinear))]


def spread_log_sigma2(net, seed):
    """log_sigma2 around the weights' own scale, so that log_alpha covers both sides of a threshold."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in vd_layers(net):
            w = m.weight
            w.log_sigma2.copy_((2 * torch.log(w.mean.abs().cpu() + 1e-3) + 3 * torch.randn(w.mean.shape, generator=g)).to(w.device))


def clear_of_cuts(net, thr):
    """Move every log_sigma2 whose float64 log_alpha lies within 5e-3 of thr or of +-8 by 0.02; assert none is within 1e-3."""
    with torch.no_grad():
        for m in vd_layers(net):
            w = m.weight
            raw = log_alpha_raw64(w.mean.cpu(), w.log_sigma2.cpu())
            near = ((raw - thr).abs() < 5e-3) | ((raw.abs() - 8).abs() < 5e-3)
            w.log_sigma2.add_(0.02 * near.to(w.mean.device))
            raw = log_alpha_raw64(w.mean.cpu(), w.log_sigma2.cpu())
            assert not (((raw - thr).abs() < 1e-3) | ((raw.abs() - 8).abs() < 1e-3)).any()


# ================================================================================================ CPU
def test_layer_surface():
    import pytorch_bayesian.nn as alias
    for nd in (1, 2, 3):
        cls = LAYER[nd]
        assert getattr(alias, cls.__name__) is cls and getattr(bnn.nn, cls.__name__) is cls
        assert cls.__name__ not in bnn.nn.__all__
        assert issubclass(cls, VariationalDropoutConvNd) and issubclass(cls, BayesianConvNd)
        # the draw plan and fuse_activations select by exact type; nothing may select these as Gaussian conv layers
        assert not issubclass(cls, (NormalConvNd, LocalReparamConvNd))
    assert alias.VariationalDropoutConvNd is VariationalDropoutConvNd and "VariationalDropoutConvNd" not in bnn.nn.__all__
    torch.manual_seed(0)
    a = VariationalDropoutConv2d(4, 6, (3, 2), stride=(2, 1), padding=(1, 0), dilation=(1, 2), groups=2)
    assert list(a.state_dict()) == ["weight.mean", "weight.log_sigma2", "bias.mean", "bias.scale"]
    assert (a.kernel_size, a.stride, a.padding, a.dilation, a.groups) == ((3, 2), (2, 1), (1, 0), (1, 2), 2)
    assert isinstance(a.weight, WeightVariationalDropout) and isinstance(a.bias, WeightNormal) and a.threshold is None
    assert a.weight.shape == (6, 2, 3, 2) and a.bias.mean.shape == (6,)
    nob = VariationalDropoutConv2d(4, 6, 3, bias=False)
    assert list(nob.state_dict()) == ["weight.mean", "weight.log_sigma2"] and nob.bias is None
    assert VariationalDropoutConv1d(4, 6, 3).weight.shape == (6, 4, 3) and VariationalDropoutConv3d(4, 6, 2, groups=2).weight.shape == (6, 2, 2, 2, 2)
    assert VariationalDropoutConv3d(4, 6, 2, threshold=2.5).threshold == 2.5
    with pytest.raises(ValueError):
        VariationalDropoutConv2d(4, 6, 3, groups=3)
    # initial values: the mean as NormalConvNd's (kaiming_uniform(a = sqrt 5): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))), log_sigma2 = -10
    assert torch.equal(a.weight.log_sigma2, torch.full((6, 2, 3, 2), -10.0))
    bound = 1 / math.sqrt(2 * 3 * 2)
    assert a.weight.mean.abs().max() <= bound and a.weight.mean.std() > 0.4 * bound
    assert a.bias.mean.abs().max() <= bound and (a.bias.scale + 2).abs().max() < 1.0
    la = a.weight.log_alpha
    assert la.shape == (6, 2, 3, 2) and la.min() >= -8 and la.max() <= 8
    # traverse / apply_wb see a Bayesian leaf with a weight and a bias
    net = SmallNet()
    seen = net.traverse(lambda m: apply_wb(m, lambda p, module, type: (type, p), pass_module=True, pass_type=True))
    assert [k for k, _ in seen] == ["w", "b"] * 3
    assert [type(p) for _, p in seen] == [WeightVariationalDropout, WeightNormal] * 3
    # nn.fuse_activations passes the layers by
    bnn.nn.fuse_activations(net)
    assert all(getattr(l, "activation", None) is None for l in net.layers)
    assert "VariationalDropoutConv1d / 2d / 3d" in nn.container._MOMENTS_SUPPORTED


CPU_CASES = {
    "bias": (Case(3, 4, (7, 8), 6, 3, 1, 1), True),
    "nobias": (Case(3, 4, (7, 8), 6, 3, 1, 1), False),
    "groups2": (Case(3, 4, (7, 8), 6, 3, 1, 1, 1, 2), True),
    "peraxis": (Case(2, 3, (9, 11), 5, (3, 2), (2, 1), (1, 2), (1, 2)), True),
    "1d": (Case(3, 4, (13,), 5, 4, 2, 1, 2), True),
    "3d": (Case(2, 3, (5, 6, 7), 4, (2, 3, 2), (1, 2, 1), (1, 0, 1), (2, 1, 1)), True),
}


def cpu_layer(case, bias, seed, threshold=None):
    torch.manual_seed(seed)
    layer = LAYER[case.nd](case.C, case.O, case.k, case.s, case.p, case.d, case.g, bias, threshold=threshold)
    with torch.no_grad():
        layer.weight.log_sigma2.copy_(-6 + torch.randn(layer.weight.shape))
    return layer


def panel_reference(case, layer, x, eps, keep=None):
    """float64 on the im2col panel (no torch conv in the reference); keep: the mask of a threshold."""
    theta, s2 = layer.weight.mean.detach().double(), torch.exp(layer.weight.log_sigma2.detach().double())
    if keep is not None:
        theta, s2 = theta * keep, s2 * keep
    bias = layer.bias is not None
    ref, _, _ = lrt64(case.im2col(x.double()), case.im2col(x.double() ** 2), case.dense_w(theta), case.dense_w(s2),
                      layer.bias.mean.detach().double() if bias else None, sigma64(layer.bias.scale.detach()) ** 2 if bias else None,
                      case.rows(eps.double()))
    return ref


@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_cpu_forward_is_the_formula(name):
    case, bias = CPU_CASES[name]
    layer = cpu_layer(case, bias, 1)
    x = torch.randn(case.B, case.C, *case.sp)
    torch.manual_seed(77)
    y = layer(x)
    assert y.shape == (case.B, case.O) + case.out
    torch.manual_seed(77)
    eps = torch.randn(y.shape)
    assert torch.allclose(case.rows(y.detach().double()), panel_reference(case, layer, x, eps), atol=1e-5, rtol=1e-5)
    assert torch.equal(layer(x, sample=False), y)                  # the same noise again
    torch.manual_seed(78)
    y1 = layer(x[0])                                               # unbatched: the one image
    assert y1.shape == (case.O,) + case.out
    torch.manual_seed(78)
    eps1 = torch.randn(y1.shape)
    assert torch.allclose(case.rows(y1.detach().double().unsqueeze(0)), panel_reference(case, layer, x[:1], eps1.unsqueeze(0)),
                          atol=1e-5, rtol=1e-5)
    assert torch.equal(layer(x[0], sample=False), y1)
    with pytest.raises(RuntimeError):
        layer(x, sample=False)                                     # the recorded noise has another shape now
    y1.sum().backward()
    assert layer.weight.mean.grad is not None and layer.weight.log_sigma2.grad.abs().sum() > 0


def test_cpu_sample_false_refusals():
    layer = cpu_layer(CPU_CASES["bias"][0], True, 2)
    x = torch.randn(3, 4, 7, 8)
    with pytest.raises(RuntimeError, match="sample=False"):
        layer(x, sample=False)                                     # nothing recorded yet
    y = layer(x)
    assert torch.equal(layer(x, sample=False), y) and not torch.equal(layer(x), y)
    with pytest.raises(RuntimeError, match="sample=False"):
        layer(x[:2], sample=False)


def test_cpu_expression_gradcheck():
    torch.manual_seed(2)
    layer = VariationalDropoutConv2d(2, 4, 3, stride=(2, 1), padding=(1, 0), groups=2).double()
    with torch.no_grad():
        layer.weight.log_sigma2.copy_(-3 + torch.randn(layer.weight.shape, dtype=torch.float64))
    x = torch.randn(2, 2, 5, 4, dtype=torch.float64, requires_grad=True)
    layer(x)                                                       # records the noise

    def f(x, th, ls, mb, rb):
        return torch.func.functional_call(layer, {"weight.mean": th, "weight.log_sigma2": ls, "bias.mean": mb, "bias.scale": rb},
                                          (x, False))

    assert torch.autograd.gradcheck(f, (x, layer.weight.mean, layer.weight.log_sigma2, layer.bias.mean, layer.bias.scale))


def test_kl_divergence_of_the_small_net(monkeypatch):
    """mean over the six tensors of their per-tensor means: vd_kl_elements(...).mean() per VD tensor (the formula itself, kl64, in
    float64), the Gaussian KL of the biases.  Every VD tensor, conv-shaped ones included, is handed to the log-uniform KL exactly
    once: on CPU tensors that is one ops.vd_kl_elements call per tensor (ops.vd_kl is the device's entry; the GPU network test
    counts ONE call of it for all three)."""
    torch.manual_seed(3)
    net = SmallNet()
    spread_log_sigma2(net, 4)
    terms, prior = [], torch.distributions.Normal(torch.tensor(0.0).double(), torch.tensor(0.1).double())
    for layer in vd_layers(net):
        terms.append(kl64(layer.weight.mean.detach(), layer.weight.log_sigma2.detach()).mean())
        assert abs(ops.vd_kl_elements(layer.weight.mean, layer.weight.log_sigma2).mean().item() - terms[-1].item()) <= 1e-5 * terms[-1].item()
        q = torch.distributions.Normal(layer.bias.mean.detach().double(), sigma64(layer.bias.scale.detach()))
        terms.append(torch.distributions.kl_divergence(q, prior).mean())
    want = torch.stack(terms).mean() / 4.0
    calls = []
    real = ops.vd_kl_elements
    monkeypatch.setattr(ops, "vd_kl_elements", lambda t, l: calls.append(tuple(t.shape)) or real(t, l))
    got = KLDivergence(4)(net)
    assert sorted(calls) == sorted(tuple(l.weight.shape) for l in vd_layers(net)) and len(calls) == 3
    assert abs(got.item() - want.item()) <= 1e-5 * (1 + abs(want.item())), (got.item(), want.item())
    assert abs(net.kl_divergence(4).item() - got.item()) <= 1e-7
    one = net.layers[2].kl_divergence()
    assert abs(one.item() - ((terms[2] + terms[3]) / 2).item()) <= 1e-5 * (1 + one.item())
    got.backward()
    for layer in vd_layers(net):
        assert layer.weight.mean.grad is not None and layer.weight.log_sigma2.grad is not None and layer.bias.scale.grad is not None


def explicit_filters(layer, thr=3.0):
    """Filter 0 wholly above the threshold, filter 1 wholly below, the others alternating: log_alpha = thr +- 2 exactly."""
    with torch.no_grad():
        w = layer.weight
        sign = torch.ones(w.shape)
        sign.reshape(w.shape[0], -1)[:, ::2] = -1                  # the other filters: every second weight kept
        sign[0], sign[1] = 1, -1
        mean = w.mean.cpu()
        mean = torch.where(mean.abs() < 1e-2, torch.full_like(mean, 0.05), mean)
        w.mean.copy_(mean)
        w.log_sigma2.copy_(2 * torch.log(mean.abs()) + thr + 2 * sign)
    return sign > 0


def test_pruning_sparsity_and_filter_sparsity():
    torch.manual_seed(5)
    net = SmallNet()
    spread_log_sigma2(net, 6)
    c0, c2, lin = net.layers[0], net.layers[2], net.layers[4]
    drop0 = explicit_filters(c0)
    count = lambda l, t: int((log_alpha_raw64(l.weight.mean.detach(), l.weight.log_sigma2.detach()).clamp(-8, 8) > t).sum())  # noqa: E731
    assert count(c0, 3.0) == int(drop0.sum()) and 0 < count(c0, 3.0) < drop0.numel()
    assert c0.sparsity() == count(c0, 3.0) / drop0.numel()
    assert c0.filter_sparsity() == 1 / 8                            # filter 0 alone is wholly dropped; filter 1 is wholly kept
    la2 = log_alpha_raw64(c2.weight.mean.detach(), c2.weight.log_sigma2.detach()).clamp(-8, 8)
    assert c2.filter_sparsity() == int((la2 > 3.0).reshape(6, -1).all(1).sum()) / 6
    total = sum(l.weight.mean.numel() for l in (c0, c2, lin))
    assert total == 8 * 27 + 6 * 36 + 540
    assert net.sparsity() == (count(c0, 3.0) + count(c2, 3.0) + count(lin, 3.0), total)
    c0.threshold = 2.0
    assert c0.sparsity() == count(c0, 2.0) / drop0.numel() and c0.filter_sparsity() == 1 / 8      # log_alpha is 1 or 5: the same split
    c0.threshold = 6.0
    assert c0.sparsity() == 0.0 and c0.filter_sparsity() == 0.0
    c0.threshold = 0.0
    assert c0.sparsity() == 1.0 and c0.filter_sparsity() == 1.0
    c0.threshold = None
    assert net.sparsity()[0] == count(c0, 3.0) + count(c2, 3.0) + count(lin, 3.0)
    # PruneLogAlpha on conv weights
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    prune.PruneLogAlpha()(net)
    assert torch.equal(c0.weight.mean.detach(), before["layers.0.weight.mean"] * ~drop0)
    assert torch.equal(c0.weight.log_sigma2.detach(), torch.where(drop0, torch.tensor(-30.0), before["layers.0.weight.log_sigma2"]))
    assert (c0.weight.mean[0] == 0).all() and (c0.weight.mean[1] != 0).all()
    assert torch.equal(c0.bias.mean.detach(), before["layers.0.bias.mean"]) and torch.equal(c0.bias.scale.detach(), before["layers.0.bias.scale"])
    assert int((c2.weight.mean == 0).sum()) == int((la2 > 3.0).sum())
    with pytest.raises(TypeError, match="PruneLogAlpha"):
        prune.PruneNormal()(net, 0.5)


def test_threshold_on_the_cpu():
    case, bias = CPU_CASES["groups2"]
    layer = cpu_layer(case, bias, 7, threshold=1.0)
    spread = torch.Generator().manual_seed(8)
    with torch.no_grad():
        layer.weight.log_sigma2.copy_(2 * torch.log(layer.weight.mean.abs() + 1e-3) + 3 * torch.randn(layer.weight.shape, generator=spread))
    keep = ~(log_alpha_raw64(layer.weight.mean.detach(), layer.weight.log_sigma2.detach()).clamp(-8, 8) > 1.0)
    assert keep.any() and (~keep).any()
    x = torch.randn(case.B, case.C, *case.sp)
    with pytest.raises(ops.BnnHipError, match="inference"):
        layer(x)                                                   # a posterior gradient with a threshold set
    torch.manual_seed(79)
    with torch.no_grad():
        y = layer(x)
    torch.manual_seed(79)
    eps = torch.randn(y.shape)
    assert torch.allclose(case.rows(y.double()), panel_reference(case, layer, x, eps, keep), atol=1e-5, rtol=1e-5)
    # the input's gradient alone flows through the masked layer
    for p in layer.parameters():
        p.requires_grad_(False)
    xg = x.clone().requires_grad_()
    layer(xg).sum().backward()
    assert torch.isfinite(xg.grad).all() and xg.grad.abs().sum() > 0
    # the moment pass honours the mask and refuses to be tracked
    net = BayesianNetworkModule(case.C, case.O)
    net.layers = torch.nn.Sequential(layer)
    net._forward = lambda x: net.layers(x)
    mom = net.predictive_moments(x)
    ref = ops.moments_convNd_vd_f64(x, *layer._posterior(), *case.geo, threshold=1.0)
    hand = ops.moments_convNd_vd_f64(x, layer.weight.mean * keep, torch.where(keep, layer.weight.log_sigma2, torch.tensor(-math.inf)),
                                     layer.bias.mean, layer.bias.scale, *case.geo)
    assert torch.equal(ref.mean, hand.mean) and torch.equal(ref.var, hand.var)
    assert torch.allclose(mom.mean.double(), ref.mean, rtol=1e-5, atol=1e-6) and torch.allclose(mom.var.double(), ref.var, rtol=1e-5, atol=1e-9)
    for p in layer.parameters():
        p.requires_grad_(True)
    layer.threshold = None
    with pytest.raises(ops.BnnHipError, match="no moment backward"):
        net.forward_moments(x)
    nn.conv_moment_training()
    try:
        with pytest.raises(ops.BnnHipError, match="no moment backward"):
            net.forward_moments(x)
    finally:
        nn.conv_moment_training(False)


def test_training_lowers_the_loss_and_raises_the_sparsity():
    """SmallNet on 64 seeded 3 x 7 x 7 images whose class (of 10) is a planted pattern, torch only, torch.manual_seed(1): 100 Adam
    steps (lr 0.02) on cross-entropy + 0.1 KL.  Observed: cross-entropy 2.2889 -> 0.0000, model.sparsity() (9, 972) -> (215, 972)
    (at initialisation the nine weights with |theta| < e^-6.5 already have log_alpha > 3: under 2 % by construction, asserted).  The
    assertions ask for half the loss and for 5 % of the weights more than at the start."""
    torch.manual_seed(1)
    net = SmallNet(samples=1)
    proto = torch.randn(10, 3, 7, 7)
    target = torch.arange(64) % 10
    X = proto[target] + 0.3 * torch.randn(64, 3, 7, 7)
    opt = torch.optim.Adam(net.parameters(), lr=0.02)
    start = net.sparsity()
    first = None
    for _ in range(100):
        opt.zero_grad()
        ce = F.cross_entropy(net(X), target)
        (ce + 0.1 * net.kl_divergence()).backward()
        opt.step()
        first = ce.item() if first is None else first
    end = net.sparsity()
    print("cross-entropy %.4f -> %.4f, sparsity %s -> %s, filter sparsity %s" % (first, ce.item(), start, end,
                                                                                 [net.layers[i].filter_sparsity() for i in (0, 2)]))
    assert ce.item() < 0.5 * first
    assert start[0] < 0.02 * start[1] and end[0] > start[0] + 0.05 * end[1] and end[1] == start[1] == 972


def test_code_object_holds_the_new_kernel():
    """The slab reduce with this posterior's chain factor is in the gfx950 code object, once, and uses no scratch; K11's
    instantiation is still there beside it."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    for pat in (r"_ZN3bnn15k_lrt_conv_wsumINS_14ChainLogSigma2EEEv", r"_ZN3bnn15k_lrt_conv_wsumINS_8ChainRhoEEEv"):
        found = [f for n, f in kernels.items() if re.match(pat, n)]
        assert len(found) == 1, (pat, sorted(n for n in kernels if "wsum" in n))
        assert int(found[0].get("vgpr_spill_count", 0)) == 0 and int(found[0].get("private_segment_fixed_size", 0)) == 0, (pat, found[0])


def test_argument_errors_are_reported_without_launching():
    """bnn_conv3d_vd_backward_weight refuses what bnn_conv3d_lrt_backward_weight refuses, with the same codes, before any launch;
    the pointers are plain integers that no refused call dereferences."""
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)

    def shape(B=2, C=4, D=1, H=5, W=5, O=6, k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1), d=(1, 1, 1), g=1):
        return ctypes.byref(_lib.Conv3dShape(B, C, D, H, W, O, *k, *s, *p, *d, g))

    ok = shape()
    wgr, wsb = lib.bnn_conv3d_vd_backward_weight, lib.bnn_conv3d_lrt_backward_weight_workspace_bytes
    big = 1 << 30
    need = wsb(ok, 1)
    assert need > 0

    def refused(rc, code, word):
        msg = lib.bnn_last_error().decode()
        assert rc == code and word in msg, (rc, code, msg)

    refused(wgr(None, one, one, one, one, one, None, None, None, ok, 1, 0, one, big, None), -1, "NULL")
    refused(wgr(one, one, one, None, one, one, None, None, None, ok, 1, 0, one, big, None), -1, "NULL")      # no log_sigma2
    refused(wgr(one, one, one, one, one, None, None, None, None, ok, 1, 0, one, big, None), -1, "NULL")      # no g_log_sigma2
    refused(wgr(one, one, one, one, one, one, one, one, None, ok, 1, 0, one, big, None), -1, "NULL")         # partial bias
    refused(wgr(one, one, one, one, one, one, None, None, None, None, 1, 0, one, big, None), -1, "")        # no shape
    refused(wgr(one, one, one, one, one, one, None, None, None, shape(g=3), 1, 0, one, big, None), -2, "")
    refused(wgr(one, one, one, one, one, one, None, None, None, ok, 0, 0, one, big, None), -2, "")           # no image set
    refused(wgr(one, one, one, odd, one, one, None, None, None, ok, 1, 0, one, big, None), -4, "misaligned")
    refused(wgr(one, one, one, one, odd, one, None, None, None, ok, 1, 0, one, big, None), -4, "misaligned")
    refused(wgr(one, one, one, one, one, one, None, None, None, ok, 1, 0, odd, big, None), -4, "misaligned")
    refused(wgr(one, one, one, one, one, one, None, None, None, ok, 1, 5, one, big, None), -3, "")           # BNN_E_DTYPE
    refused(wgr(one, one, one, one, one, one, None, None, None, shape(g=2), 40000, 0, one, big, None), -5, "")
    refused(wgr(one, one, one, one, one, one, None, None, None, shape(B=1 << 16, C=1 << 8, H=16, W=16), 1, 0, one, big, None), -5, "2^31")
    refused(wgr(one, one, one, one, one, one, None, None, None, ok, 1, 0, one, need - 4, None), -6, "workspace")
    refused(wgr(one, one, one, one, one, one, None, None, None, ok, 1, 0, None, 0, None), -6, "workspace")
    assert lib.bnn_launch_count() == n0
    # the host op reports its refusals before anything is launched too
    key = DrawKey(1, 2, 0, 1, 3)
    with pytest.raises(ops.BnnHipError):
        ops.convNd_vd(torch.zeros(2, 4, 5, 5), torch.zeros(6, 4, 3, 3), torch.zeros(6, 4, 3, 3), None, None, key, True, (1, 1), (1, 1), (1, 1))
    assert lib.bnn_launch_count() == n0


# ================================================================================================ GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


def put(dev, ts):
    return [None if t is None else t.to(dev) for t in ts]


def run_vd(case, x, params, key, shared, mode, threshold=None):
    theta, ls2, mu_b, rho_b = params
    return ops.convNd_vd(x, theta, ls2, mu_b, rho_b, key, shared, *case.geo, mode, threshold=threshold)


def vd_operands64(x, theta, ls2, mu_b, rho_b, mode, dev):
    """float64 operands as the kernel contracts them: (x, x^2, theta, s2, mu_b, sigma_b^2).  The device's bnn_vd_prepare plane is
    held to float64 at bound_s2 (3 u) in BOTH modes; the bf16 mode's reference rounds that plane, as the kernel does."""
    want_w = torch.exp(ls2.double())
    want_b = sigma64(rho_b) ** 2 if rho_b is not None else None
    _, s2_w, s2_b, _ = ops._vd_prepare_raw(theta.to(dev), ls2.to(dev), None if rho_b is None else rho_b.to(dev))
    s2_w = s2_w.cpu()
    assert ((s2_w.double() - want_w).abs() <= bound_s2(ls2)).all()
    if rho_b is not None:
        s2_b = s2_b.cpu()
        assert ((s2_b.double() - want_b).abs() <= 1e-6 * want_b).all()
    if mode == "f32":
        return x.double(), x.double() ** 2, theta.double(), want_w, None if mu_b is None else mu_b.double(), want_b
    return (rne_bf16(x), rne_bf16(x.float() * x.float()), rne_bf16(theta), rne_bf16(s2_w),
            None if mu_b is None else mu_b.double(), None if rho_b is None else s2_b.double())


VD_FWD = ["lenet", "peraxis2d", "groups2", "1d", "3d", "1x1"]


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("S", [1, 4, 33])
@pytest.mark.parametrize("name", VD_FWD)
def test_forward_matches_float64_on_the_keys_eps(dev, name, S, shared, bias, mode):
    case = FWD_CASES[name]
    params = vd_params(case, bias, 11)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(*((case.B,) if shared else (S, case.B)), case.C, *case.sp, generator=g)
    key = DrawKey(0x1234567890ABCDEF, 321, 3, S, 17, gen=_rng.generator_for(mode))          # sample0 = 3
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    y = run_vd(case, x.to(dev), put(dev, params), key, shared, mode)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 2            # bnn_vd_prepare + ONE contraction launch for all S samples
    assert y.shape == (S, case.B, case.O) + case.out and y.dtype == torch.float32
    x64, xsq, th64, s2, mb, s2b = vd_operands64(x, *params, mode, dev)
    eps = case.rows(conv_eps(key, S, case, dev))
    flat = (lambda t: t) if shared else (lambda t: t.reshape(-1, *t.shape[2:]))
    col, colsq = case.im2col(flat(x64)), case.im2col(flat(xsq))
    if not shared:
        col, colsq = col.reshape(S, -1, col.shape[-1]), colsq.reshape(S, -1, col.shape[-1])
    th2 = case.dense_w(th64)
    ref, _, v = lrt64(col, colsq, th2, case.dense_w(s2), mb, s2b, eps)
    assert_within(case.rows(y), ref, forward_bound(mode, col, th2, mb, ref, v, eps, case.K), "y %s S=%d %s" % (name, S, mode))


def shape_of(case, B=None):
    img, w5, st, pd, dl = ops._lrt_conv_views((case.B, case.C) + case.sp, (case.O, case.C // case.g) + case.k, case.s, case.p, case.d)
    return ops._conv3d_shape((case.B if B is None else B,) + img, w5, st, pd, dl, case.g)[0]


def slabs_of(case):
    nb = _lib.load().bnn_conv3d_lrt_backward_weight_workspace_bytes(ctypes.byref(shape_of(case)), 1)
    assert nb > 0 and nb % (2 * case.O * case.K * 4) == 0
    return nb // (2 * case.O * case.K * 4)


VD_BWD = dict(BWD_CASES, one=Case(1, 4, (5, 5), 6, 3), cap=Case(8, 3, (8, 8), 4, 3, 1, 1))
SLABS = {"strided": 2, "dilated": 7, "3d": 5, "groups2": 7, "one": 1, "cap": 16}


def test_backward_cases_pin_the_slab_counts():
    """B P = 9 is ONE slab, B P = 512 the 16-slab cap: a change of wgrad_split cannot silently move the cases."""
    assert VD_BWD["one"].B * VD_BWD["one"].P == 9 and VD_BWD["cap"].B * VD_BWD["cap"].P == 512
    assert {n: slabs_of(c) for n, c in VD_BWD.items()} == SLABS


def vd_backward64(case, x, xsq, x_epi, theta, s2, c_w, rho_b, v, eps, gy, shared, rnd, betas):
    """test_lrt_conv_device.backward64's bf16 branch with c_w = exp(log_sigma2) (float64) and the epilogue term of this file's
    docstring: -> [(gradient, bound), ...] for x, theta, log_sigma2 (, mu_b, rho_b)."""
    inv = 0.5 / torch.sqrt(v + 1e-16)
    if shared:
        g_m, g_v = gy.sum(0), (gy * eps).sum(0) * inv
    else:
        g_m, g_v = gy, gy * eps * inv
    c_b = None if rho_b is None else 2 * sigma64(rho_b) * torch.sigmoid(rho_b.double())
    red = [0] + list(range(2, g_m.dim()))
    h_m, d_m = rnd(g_m, betas[0])
    h_v, d_v = rnd(g_v, betas[1])

    def pair(fn, a, da, b, R):
        t, ab = fn(a, b), fn(a.abs(), b.abs())
        slack = fn(da, b.abs())
        return t, gamma(R) * (ab + slack) + gamma(R, 2.0 ** -53) * ab, slack

    Kd = case.O // case.g * case.T + 1
    t1, a1, s1 = pair(case.dgrad, h_m, d_m, theta, Kd)
    t2, a2, s2_ = pair(case.dgrad, h_v, d_v, s2, Kd)
    out = [(t1 + 2 * x_epi * t2, a1 + s1 + 2 * x_epi.abs() * (a2 + s2_) + 4 * U * (t1.abs() + 2 * x_epi.abs() * t2.abs()))]
    R = g_m.shape[0] * case.P + 17                                       # every position of every image, and at most 16 slab sums
    sw = lambda a, da, b, n: pair(lambda p, q: case.wgrad(q, p), a, da, b, n)    # noqa: E731  (the deviating operand first)
    t, a, s = sw(h_m, d_m, x, R)
    out.append((t, a + s))
    t, a, s = sw(h_v, d_v, xsq, R)
    out.append((t * c_w, (a + s) * c_w * (1 + EPI_U * U) + EPI_U * U * (t * c_w).abs() + 2.0 ** -149))
    if rho_b is not None:
        M = g_m.shape[0] * case.P
        out.append((g_m.sum(red), gamma(M) * g_m.abs().sum(red) + betas[0].sum(red)))     # the bias sums read the fp32 g_m / g_v
        tb = g_v.sum(red)
        out.append((tb * c_b, (gamma(M) * g_v.abs().sum(red) + betas[1].sum(red)) * c_b + 16 * U * (tb * c_b).abs()))
    return out


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("name", sorted(VD_BWD))
def test_backward_matches_float64_on_the_keys_eps(dev, name, S, shared, bias, mode):
    """All five gradients, every element; image 1 of the batch is all zero (the only image of `one` is image 0: it stays).  Worst
    err / bound the MI355X run printed, fp32 / bf16: g_x 0.034 / 0.981, g_theta 0.056 / 0.036, g_log_sigma2 0.021 / 0.990, g_mu_b
    0.025 / 0.067, g_rho_b 0.023 / 0.002.  The two bf16 figures near 1 are `strided` at S = 4 (36 rows): an element of g_m / g_v
    that bf16ref.round_hidden cannot decide enters the bound with its whole bf16 ulp, and with so few rows one such element is most
    of the bound -- which is nearly attained when the device rounds it the other way (the likely reading; not traced further)."""
    case = VD_BWD[name]
    assert slabs_of(case) == SLABS[name]
    params = vd_params(case, bias, 31)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(*((case.B,) if shared else (S, case.B)), case.C, *case.sp, generator=g)
    if case.B > 1:
        x[(Ellipsis, 1) + (slice(None),) * (case.nd + 1)] = 0
    gy = torch.randn(S, case.B, case.O, *case.out, generator=g)
    key = DrawKey(777, 45, 1, S, 9, gen=_rng.generator_for(mode))
    leaves = [None if t is None else t.to(dev).requires_grad_() for t in (x,) + params]
    lib = _lib.load()
    y = run_vd(case, leaves[0], leaves[1:], key, shared, mode)
    n0 = lib.bnn_launch_count()
    got = torch.autograd.grad(y, [t for t in leaves if t is not None], gy.to(dev))
    torch.cuda.synchronize()
    # g_m / g_v, the paired input gradient, the paired weight-gradient slabs and their reduce, the bias sums: nothing else ran
    assert lib.bnn_launch_count() == n0 + (5 if bias else 4)
    assert all(torch.isfinite(t).all() for t in got)
    theta, ls2, mu_b, rho_b = params
    eps = conv_eps(key, S, case, dev)
    names = ["x", "weight.mean", "weight.log_sigma2"] + (["bias.mean", "bias.scale"] if bias else [])
    if mode == "f32":
        ref = [t.double().requires_grad_() for t in (x,) + params if t is not None]
        p64 = ref[1:] + ([None, None] if not bias else [])
        yr, _, _ = formula64(case, ref[0], *p64, eps)
        want = torch.autograd.grad((yr * gy.double()).sum(), ref)
        for n, a, w in zip(names, got, want):
            assert_within(a, w, scaled_bound(w), "g %s %s S=%d f32" % (n, name, S))
        return
    x64, xsq, th64, s2, mb, s2b = vd_operands64(x, theta, ls2, mu_b, rho_b, mode, dev)
    v = case.conv(xsq, s2, s2b)                                          # every term >= 0: v is its own sum |a| |b|
    gy64 = gy.double()
    rel_inv = 1.01 * 0.5 * gamma(case.K + 1) * v / (v + 1e-16) + 4 * U
    inv = 0.5 / torch.sqrt(v + 1e-16)
    term = gy64.abs() * inv * (eps.abs() * (rel_inv + 3 * U) + EPS_TWIN)
    if shared:
        beta_m = gamma(S) * gy64.abs().sum(0)
        beta_v = 1.01 * (term.sum(0) + gamma(S) * (gy64 * eps).abs().sum(0) * inv)
    else:
        beta_m, beta_v = torch.zeros_like(gy64), 1.01 * term
    flat = (lambda t: t) if shared else (lambda t: t.reshape(-1, *t.shape[2:]))
    # the epilogue multiplies by expf(log_sigma2) in fp32 (not by the bf16-rounded plane): c_w = exp in float64
    want = vd_backward64(case, flat(x64), flat(xsq), flat(x.double()), th64, s2, torch.exp(ls2.double()), rho_b if bias else None,
                         v if shared else flat(v), eps if shared else flat(eps), gy64 if shared else flat(gy64), shared,
                         rnd=lambda t, beta: round_hidden(t, beta)[:2], betas=(flat(beta_m), flat(beta_v)))
    for n, a, (w, bound) in zip(names, got, want):
        assert_within(a.reshape(w.shape), w, bound + 1e-30, "g %s %s S=%d bf16" % (n, name, S))


@gpu
@pytest.mark.parametrize("bias", [True, False])
def test_epilogue_over_the_parameters_range(dev, bias):
    """bnn_conv3d_vd_backward_weight called directly, log_sigma2 from wide_grid's [-100, 20] (exp from 0 and denormals to 5e8):
    g_theta is bnn_conv3d_lrt_backward_weight's g_mu_w on the same x, g_m, g_v bit for bit (and the bias gradients are K11's);
    g_log_sigma2 within the docstring's bound of (float64 sum) exp(log_sigma2).  fp32 mode: the MFMA takes the operands as they
    are, so the slab sums differ from float64 by the accumulation alone, gamma_{R+17} sum |x^2| |g_v|, R = B P.  Worst err / bound
    the MI355X run printed: g_log_sigma2 0.427, g_theta 0.008 (before the kernel formed the product in fp64 below -87: 8.8, nine
    quanta at |sum| = 9)."""
    case = Case(3, 4, (6, 5), 6, 3, 1, 1)                                 # B P = 90: 3 slabs
    assert slabs_of(case) == 3
    n = case.O * case.K
    _, ls2 = wide_grid(n, seed=5)
    assert ls2.min() <= -99 and ls2.max() >= 19
    ls2 = ls2.reshape(case.O, case.C, *case.k)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(case.B, case.C, *case.sp, generator=g)
    g_m = torch.randn(case.B, case.O, *case.out, generator=g)
    g_v = torch.randn(case.B, case.O, *case.out, generator=g)
    rho_w = -3 + 0.3 * torch.randn(ls2.shape, generator=g)
    rho_b = -3 + 0.3 * torch.randn(case.O, generator=g)
    lib, st, sh = _lib.load(), _lib.stream_ptr(dev), shape_of(case)
    nb = lib.bnn_conv3d_lrt_backward_weight_workspace_bytes(ctypes.byref(sh), 1)
    xd, gmd, gvd, ld, rwd, rbd = put(dev, (x, g_m, g_v, ls2, rho_w, rho_b))
    outs = {}
    for which in ("lrt", "vd", "vd2"):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        gw, gs = torch.empty_like(ld), torch.empty_like(ld)
        gmb, grb = (torch.empty_like(rbd), torch.empty_like(rbd)) if bias else (None, None)
        fn = lib.bnn_conv3d_lrt_backward_weight if which == "lrt" else lib.bnn_conv3d_vd_backward_weight
        n0 = lib.bnn_launch_count()
        _lib.check(fn(_lib.ptr(xd), _lib.ptr(gmd), _lib.ptr(gvd), _lib.ptr(rwd if which == "lrt" else ld), _lib.ptr(gw), _lib.ptr(gs),
                      _lib.ptr(rbd) if bias else None, _lib.ptr(gmb), _lib.ptr(grb), ctypes.byref(sh), 1, _lib.COMPUTE_F32,
                      _lib.ptr(ws), nb, st), which)
        torch.cuda.synchronize()
        assert lib.bnn_launch_count() == n0 + (3 if bias else 2)
        outs[which] = (gw, gs, gmb, grb)
    assert torch.equal(outs["vd"][0], outs["lrt"][0])                     # g_theta: the same slabs added in the same order
    assert all(torch.equal(a, b) for a, b in zip(outs["vd"], outs["vd2"]) if a is not None)
    if bias:
        assert torch.equal(outs["vd"][2], outs["lrt"][2]) and torch.equal(outs["vd"][3], outs["lrt"][3])
    xsq = x.double() ** 2
    t = case.wgrad(xsq, g_v.double())
    b_t = gamma(case.B * case.P + 17) * case.wgrad(xsq, g_v.double().abs())
    c = torch.exp(ls2.double())
    want = t * c
    assert (want.abs()[ls2 <= -95] < 2.0 ** -126).all() and want.abs().max() > 1e8
    assert_within(outs["vd"][1], want, b_t * c * (1 + EPI_U * U) + EPI_U * U * want.abs() + 2.0 ** -149, "g_log_sigma2, wide grid")
    assert_within(outs["vd"][0], case.wgrad(x.double(), g_m.double()),
                  gamma(case.B * case.P + 17) * case.wgrad(x.double().abs(), g_m.double().abs()), "g_theta, wide grid")


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["lenet", "3d", "groups2"])
def test_shared_and_per_sample_inputs_and_repeated_calls_give_the_same_bits(dev, name, mode):
    case, S = FWD_CASES[name], 4
    params = [t.to(dev).requires_grad_() for t in vd_params(case, True, 21)]
    x = torch.randn(case.B, case.C, *case.sp, device=dev).requires_grad_()
    xs = x.detach().unsqueeze(0).repeat(S, *([1] * x.dim())).requires_grad_()
    key = DrawKey(99, 7, 2, S, 5, gen=_rng.generator_for(mode))
    a = run_vd(case, x, params, key, True, mode)
    b = run_vd(case, xs, params, key, False, mode)
    c = run_vd(case, x, params, key, True, mode)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(a[0], a[1])
    gy = torch.randn_like(a)
    for y, leaves in ((a, [x] + params), (b, [xs] + params)):
        g1 = torch.autograd.grad(y, leaves, gy, retain_graph=True)
        g2 = torch.autograd.grad(y, leaves, gy)
        assert all(torch.isfinite(t).all() for t in g1)
        assert all(torch.equal(p, q) for p, q in zip(g1, g2))          # identical backward calls, identical bits


@gpu
def test_sample_flag_noise_key_and_refusals(dev):
    torch.manual_seed(4)
    layer = VariationalDropoutConv2d(6, 8, 3, padding=1).to(dev)
    x = torch.randn(5, 6, 7, 7, device=dev)
    bnn.manual_seed(5)
    with pytest.raises(RuntimeError):
        layer(x, sample=False)                         # nothing recorded yet
    y0 = layer(x)
    k0 = layer.noise_key
    assert y0.shape == (5, 8, 7, 7) and y0.dtype == torch.float32 and torch.isfinite(y0).all()
    assert (k0.stream, k0.sample0, k0.nsamples, k0.gen) == (layer._noise_stream, 0, 1, _rng.GEN_PHILOX10_U24)
    assert torch.equal(layer(x, sample=False), y0) and layer.noise_key is k0
    y1 = layer(x)
    assert layer.noise_key.epoch_host != k0.epoch_host and not torch.equal(y1, y0)
    with pytest.raises(RuntimeError):
        layer(x[:3], sample=False)                     # another shape
    yu = layer(x[0])                                   # unbatched: the batch of one image, squeezed
    assert yu.shape == (8, 7, 7) and torch.isfinite(yu).all()
    assert torch.equal(layer(x[:1], sample=False)[0], yu) and torch.equal(layer(x[0], sample=False), yu)
    with _mc.McContext(4, 5, sample0=2):
        ys = layer(x)                                  # shared input: 5 rows in, 20 out
        assert ys.shape == (20, 8, 7, 7) and (layer.noise_key.sample0, layer.noise_key.nsamples) == (2, 4)
        assert torch.equal(layer(x.repeat(4, 1, 1, 1), sample=False), ys)
        with pytest.raises(RuntimeError):
            layer(x[:3])
    with pytest.raises(RuntimeError, match="MC samples"):
        with _mc.McContext(3, 5, sample0=0):
            layer(x, sample=False)                     # the recorded noise has 4 samples
    bnn.set_compute("bf16")
    layer(x)
    assert layer.noise_key.gen == _rng.generator_for("bf16")
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    p = [t.detach() for t in layer._posterior()]
    with pytest.raises(ops.BnnHipError):               # no torch fallback
        ops.convNd_vd(x.double(), p[0], p[1], None, None, k0, True, (1, 1), (1, 1), (1, 1), 1, "f32")
    with pytest.raises(ops.BnnHipError, match="channels"):
        ops.convNd_vd(x[:, :5], p[0], p[1], None, None, k0, True, (1, 1), (1, 1), (1, 1), 1, "f32")
    with pytest.raises(ops.BnnHipError, match="kernel axes"):
        ops.convNd_vd(x, p[0][:, :, 0, 0], p[1][:, :, 0, 0], None, None, k0, True, (1, 1), (1, 1), (1, 1), 1, "f32")
    assert lib.bnn_launch_count() == n0
    l1, l3 = VariationalDropoutConv1d(6, 4, 3).to(dev), VariationalDropoutConv3d(6, 4, 2).to(dev)
    for layer_n, xn, shape in ((l1, torch.randn(2, 6, 9, device=dev), (2, 4, 7)), (l3, torch.randn(2, 6, 4, 4, 4, device=dev), (2, 4, 3, 3, 3))):
        assert layer_n(xn).shape == shape
        yu = layer_n(xn[0])
        assert yu.shape == shape[1:] and torch.isfinite(yu).all()
        assert torch.equal(layer_n(xn[:1], sample=False)[0], yu)


def hand_masked(net, cls, thr, dev):
    """A copy of `net` whose dropped elements are overwritten by hand (theta = 0, log_sigma2 = -inf: s2 = 0); sets net's threshold
    -> (the copy, the number of dropped elements)."""
    hand = cls().to(dev)
    nn.moment_activations(hand)
    hand.load_state_dict(net.state_dict())
    dropped = 0
    with torch.no_grad():
        for a, b in zip(vd_layers(net), vd_layers(hand)):
            drop = (log_alpha_raw64(a.weight.mean.cpu(), a.weight.log_sigma2.cpu()).clamp(-8, 8) > thr).to(dev)
            assert drop.any() and (~drop).any()
            dropped += int(drop.sum())
            b.weight.mean[drop] = 0
            b.weight.log_sigma2[drop] = -math.inf
            a.threshold = thr
    return hand, dropped


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_threshold_is_the_hand_masked_layer(dev, mode):
    """With a threshold the sampling forward, the MC-batched pass and the moment pass give the bits of the unmasked network whose
    dropped elements were overwritten by hand, on the same keys; sparsity() and filter_sparsity() read bnn_vd_prepare's plane."""
    torch.manual_seed(10)
    bnn.set_compute(mode)
    thr, S, B = 1.0, 4, 8
    net = SmallNet(S).to(dev)
    spread_log_sigma2(net, 11)
    with torch.no_grad():
        explicit_filters(net.layers[0], thr)                        # filter 0 of the first conv is wholly dropped at this threshold
    clear_of_cuts(net, thr)
    nn.moment_activations(net)
    hand, dropped = hand_masked(net, SmallNet, thr, dev)
    net.mc_batched = hand.mc_batched = True
    assert net.sparsity() == (dropped, 972)
    c0 = net.layers[0]
    la0 = log_alpha_raw64(c0.weight.mean.cpu(), c0.weight.log_sigma2.cpu()).clamp(-8, 8)
    assert c0.sparsity() == int((la0 > thr).sum()) / la0.numel() and c0.filter_sparsity() == 1 / 8
    la2 = log_alpha_raw64(net.layers[2].weight.mean.cpu(), net.layers[2].weight.log_sigma2.cpu()).clamp(-8, 8)
    assert net.layers[2].filter_sparsity() == int((la2 > thr).reshape(6, -1).all(1).sum()) / 6
    x = torch.randn(B, 3, 7, 7, device=dev)
    pairs = list(zip(vd_layers(net), vd_layers(hand)))
    # the sampling forward of one layer, outside any pass
    with torch.no_grad():
        bnn.manual_seed(7)
        ya = c0(x)
        hand.layers[0].noise_key, hand.layers[0]._noise_shape = c0.noise_key, c0._noise_shape
        yb = hand.layers[0](x, sample=False)
    assert torch.equal(ya, yb)
    # the MC-batched pass: the two nets' noise streams differ, so the keys are handed over layer by layer
    with torch.no_grad():
        bnn.manual_seed(8)
        full = net.forward_stacked(x, S)
        for a, b in pairs:
            b.noise_key, b._noise_shape = a.noise_key, a._noise_shape
        with _mc.McContext(S, B, sample0=0):
            h = x
            for layer in hand.layers:
                h = layer(h, sample=False) if hasattr(layer, "noise_key") else layer(h)
    assert torch.equal(full.reshape(S * B, -1), h)
    # the moment pass
    ma, mb = net.predictive_moments(x), hand.predictive_moments(x)
    assert torch.equal(ma.mean, mb.mean) and torch.equal(ma.var, mb.var)
    # the mask is for inference
    with pytest.raises(ops.BnnHipError, match="inference"):
        c0(x)
    with pytest.raises(ops.BnnHipError, match="inference"):
        net(x)
    # ... a gradient of the INPUT alone is not a posterior gradient: it goes through the masked layer
    for p in list(net.parameters()) + list(hand.parameters()):
        p.requires_grad_(False)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    bnn.manual_seed(9)
    c0(xa).sum().backward()
    hand.layers[0].noise_key = c0.noise_key
    hand.layers[0](xb, sample=False).sum().backward()
    assert torch.isfinite(xa.grad).all() and xa.grad.abs().sum() > 0 and torch.equal(xa.grad, xb.grad)


class TwoConv(BayesianNetworkModule):
    """(B, 5, 9, 8) -> VariationalDropoutConv2d(5, 8, 3, p1) -> ELU -> VariationalDropoutConv2d(8, 6, (3, 2), s (2, 1), groups 2)."""

    def __init__(self, samples=1):
        super().__init__(5, 6, samples=samples)
        self.layers = torch.nn.Sequential(VariationalDropoutConv2d(5, 8, 3, padding=1), torch.nn.ELU(),
                                          VariationalDropoutConv2d(8, 6, (3, 2), stride=(2, 1), groups=2))

    def _forward(self, x):
        return self.layers(x)


def vd_conv_ref(mom, theta, ls2, mu_b, rho_b, geo, mode, dev, threshold=None):
    """test_moment_conv.conv_ref on bnn_vd_prepare's planes: float64 of ONE moments_convNd_vd call (no activation) with the bound
    on the device's deviation -> (m, v, bound_m, bound_v); mom: CPU Moments, the call's own input."""
    if mode == "f32":
        r = ops.moments_convNd_vd_f64(mom, theta, ls2, mu_b, rho_b, *geo, threshold=threshold)
        return r.mean, r.var, scaled_bound(r.mean), scaled_bound(r.var)
    conv = CONV[theta.dim() - 2]
    K = theta[0].numel()
    th, s2_w, s2_b, _ = ops._vd_prepare_raw(theta.to(dev), ls2.to(dev), rho_b.to(dev), threshold)
    th, s2_w = th.cpu(), s2_w.cpu()
    want = torch.exp(ls2.double())
    if threshold is not None:
        keep = ~(log_alpha_raw64(theta, ls2).clamp(-8, 8) > threshold)
        want = want * keep
        assert torch.equal(th, theta * keep)
    assert ((s2_w.double() - want).abs() <= bound_s2(ls2)).all()
    p_th, p_s2 = rne_bf16(th), rne_bf16(s2_w)
    p_e2 = rne_bf16((th.double() ** 2 + s2_w.double()).float())             # one fp32 fma, then bf16
    q_m, q_sq = rne_bf16(mom.mean), rne_bf16(mom.mean.float() * mom.mean.float())
    m = conv(q_m, p_th, None, *geo)
    a = conv(q_m.abs(), p_th.abs(), None, *geo)
    v = conv(q_sq, p_s2, None, *geo)
    n_v = K
    if mom.var is not None:
        v = v + conv(rne_bf16(mom.var), p_e2, None, *geo)
        n_v = 2 * K
    shp = (1, -1) + (1,) * (theta.dim() - 2)
    mb, sb = mu_b.double().reshape(shp), s2_b.cpu().double().reshape(shp)
    m, a, v = m + mb, a + mb.abs(), v + sb
    return m, v, gamma(K + 1) * a + 1e-300, gamma(n_v + 1) * v + 1e-300       # v is its own sum |a| |b|: every term is >= 0


@gpu
@pytest.mark.parametrize("thr", [None, 1.0], ids=["all", "masked"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_predictive_moments_is_the_float64_recursion(dev, mode, thr):
    """Layer by layer (test_moment_conv's scheme): each conv against moments_convNd_vd_f64 on the DEVICE's own input of that layer
    -- fp32 mode within 1e-5 of the output scale, bf16 mode within the accumulation bound on the planes as rounded -- the fused
    ELU equal to the standalone launch on the pre-activation bit for bit and that within the ELU's measured bound, and the pass
    through the network the chained calls' bits.  A tracking pass raises."""
    torch.manual_seed(8)
    bnn.set_compute(mode)
    net = TwoConv().to(dev)
    spread_log_sigma2(net, 9)
    with torch.no_grad():
        for m in vd_layers(net):
            m.weight.log_sigma2.sub_(2.0)
    if thr is not None:
        clear_of_cuts(net, thr)
    assert nn.moment_activations(net) == 1
    l0, l2 = net.layers[0], net.layers[2]
    l0.threshold = l2.threshold = thr
    x = torch.randn(3, 5, 9, 8, device=dev)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    mom = net.predictive_moments(x)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 4            # per layer bnn_vd_prepare + ONE contraction: the ELU is fused
    assert mom.mean.shape == (3, 6, 4, 7) and not mom.mean.requires_grad and l0.noise_key is None
    geo0, geo2 = [(l.stride, l.padding, l.dilation, l.groups) for l in (l0, l2)]
    p0, p2 = [[t.detach() for t in l._posterior()] for l in (l0, l2)]
    pre = ops.moments_convNd_vd(x, *p0, *geo0, compute=mode, threshold=thr)
    hid = ops.moments_convNd_vd(x, *p0, *geo0, activation=("elu", 1.0), compute=mode, threshold=thr)
    alone = ops.moments_elu(pre, 1.0)
    assert torch.equal(hid.mean, alone.mean) and torch.equal(hid.var, alone.var)
    dm, dv = elu_deviation(hid, pre.mean.cpu(), pre.var.cpu(), 1.0)
    assert dm <= ELU_MEAN_TOL and dv <= ELU_VAR_TOL, (dm, dv)
    out = ops.moments_convNd_vd(hid, *p2, *geo2, compute=mode, threshold=thr)
    assert torch.equal(out.mean, mom.mean) and torch.equal(out.var, mom.var)
    for p, geo, a, got, what in ((p0, geo0, ops.Moments(x.cpu(), None), pre, "conv 0"),
                                 (p2, geo2, ops.Moments(hid.mean.cpu(), hid.var.cpu()), out, "conv 2")):
        m, v, bm, bv = vd_conv_ref(a, *[t.cpu() for t in p], geo, mode, dev, thr)
        assert_within(got.mean, m, bm, "%s m %s thr=%s" % (what, mode, thr))
        assert_within(got.var, v, bv, "%s v %s thr=%s" % (what, mode, thr))
        assert (got.var >= 0).all()
    l0.threshold = l2.threshold = None
    with pytest.raises(ops.BnnHipError, match="no moment backward"):
        net.forward_moments(x)
    nn.conv_moment_training()
    try:
        with pytest.raises(ops.BnnHipError, match="no moment backward"):
            net.forward_moments(x)
    finally:
        nn.conv_moment_training(False)


def net64(net, x, S, dev):
    """The serial float64 restatement on the recorded noise keys, the noise read from the device stream of each key
    (test_lrt_conv_device.net64)."""
    outs = []
    for s in range(S):
        h = x.double().cpu()
        for layer in net.layers:
            if hasattr(layer, "noise_key"):
                conv = isinstance(layer, VariationalDropoutConvNd)
                args = (layer.stride, layer.padding, layer.dilation, layer.groups) if conv else ()
                op = F.conv2d if conv else F.linear
                th, s2 = layer.weight.mean.detach().double().cpu(), torch.exp(layer.weight.log_sigma2.detach().double().cpu())
                mb, s2b = layer.bias.mean.detach().double().cpu(), sigma64(layer.bias.scale.detach().cpu()) ** 2
                m, v = op(h, th, mb, *args), op(h * h, s2, s2b, *args)
                eps = ops.eps_philox((m.numel(),), layer.noise_key, dev)[s].reshape(m.shape).double().cpu()
                h = m + torch.sqrt(v + 1e-16) * eps
            elif isinstance(layer, torch.nn.Flatten):
                h = h.flatten(1)
            else:
                h = h.clamp_min(0)
        outs.append(h)
    return torch.stack(outs)


class _CountConvs(TorchDispatchMode):
    """aten convolution operators reaching the backend (below autograd: the backward's own too)."""

    def __init__(self):
        super().__init__()
        self.n = self.seen = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.seen += 1
        if "conv" in str(func):
            self.n += 1
        return func(*args, **(kwargs or {}))


@gpu
def test_network_forward_predictive_kl_and_training_step(dev, monkeypatch):
    torch.manual_seed(6)
    S, B = 4, 8
    net = SmallNet(S).to(dev)
    spread_log_sigma2(net, 7)
    with torch.no_grad():
        for m in vd_layers(net):
            m.weight.log_sigma2.sub_(4.0)                           # mostly signal: the outputs are not all noise
    net.mc_batched = True
    x = torch.randn(B, 3, 7, 7, device=dev)
    lib = _lib.load()
    bnn.manual_seed(100)
    counts, hooks = [], []
    for l in net.layers:
        hooks.append(l.register_forward_pre_hook(lambda *_: counts.append(lib.bnn_launch_count())))
    n0 = lib.bnn_launch_count()
    with torch.no_grad():
        ys = torch.stack(net(x))
    counts.append(lib.bnn_launch_count())
    for h in hooks:
        h.remove()
    # per layer bnn_vd_prepare + ONE contraction launch (the first sees the shared batch, the others S B rows)
    assert [b - a for a, b in zip(counts, counts[1:])] == [2, 0, 2, 0, 2] and lib.bnn_launch_count() == n0 + 6
    keys = [l.noise_key for l in vd_layers(net)]
    assert [k.nsamples for k in keys] == [S] * 3 and len({k.stream for k in keys}) == 3
    want = net64(net, x, S, dev)
    assert_within(ys, want, scaled_bound(want), "conv-conv-linear VD net")
    bnn.manual_seed(100)
    with torch.no_grad():
        u = net.predictive_uncertainty(x, inputs="logits")
    r = ops.uncertainty_f64(ys.cpu(), "logits")
    tol = 1e-5 * max(1.0, math.log(10))
    assert (u.mean.double().cpu() - r.mean.double()).abs().max() <= 1e-6
    for a, b in ((u.total, r.total), (u.aleatoric, r.aleatoric), (u.epistemic, r.epistemic)):
        assert (a.double().cpu() - b.double()).abs().max() <= tol
    # KL: ONE ops.vd_kl call for the three VD tensors (conv-shaped ones included), ONE bnn_kl_forward call for the three biases
    terms, prior = [], torch.distributions.Normal(torch.tensor(0.0).double(), torch.tensor(0.1).double())
    for layer in vd_layers(net):
        terms.append(kl64(layer.weight.mean.detach().cpu(), layer.weight.log_sigma2.detach().cpu()).mean())
        q = torch.distributions.Normal(layer.bias.mean.detach().double().cpu(), sigma64(layer.bias.scale.detach().cpu()))
        terms.append(torch.distributions.kl_divergence(q, prior).mean())
    wkl = torch.stack(terms).mean().item()
    vd_calls, g_calls = [], []
    real_vd, real_g = ops.vd_kl, ops.kl_normal_scalar
    monkeypatch.setattr(ops, "vd_kl", lambda t, l: vd_calls.append([tuple(a.shape) for a in t]) or real_vd(t, l))
    monkeypatch.setattr(ops, "kl_normal_scalar", lambda m, *a: g_calls.append(len(m)) or real_g(m, *a))
    n1 = lib.bnn_launch_count()
    kl = KLDivergence()(net)
    assert lib.bnn_launch_count() == n1 + 4                         # bnn_vd_kl_forward and bnn_kl_forward, two launches each
    assert vd_calls == [[(8, 3, 3, 3), (6, 4, 3, 3), (10, 54)]] and g_calls == [3]
    assert abs(kl.item() - wkl) <= 1e-5 * (1 + abs(wkl)), (kl.item(), wkl)
    monkeypatch.undo()
    # one training step: every parameter gets a finite gradient and moves; no aten convolution runs
    before = [p.detach().clone() for p in net.parameters()]
    assert len(before) == 12
    opt = optim.Adam(net.parameters(), lr=1e-2)
    target = torch.randint(0, 10, (B,), device=dev)
    torch.cuda.synchronize()
    n2 = lib.bnn_launch_count()
    with _CountConvs() as convs:
        loss = KLDivergence()(net) + sum(F.cross_entropy(y, target) for y in net(x)) / S
        loss.backward()
        grads = {name: p.grad.clone() for name, p in net.named_parameters()}
        opt.step()
    torch.cuda.synchronize()
    step = lib.bnn_launch_count() - n2
    print("training step: %d launches of this library, %d aten operators, %d of them convolutions" % (step, convs.seen, convs.n))
    assert convs.seen > 0 and convs.n == 0
    assert step == STEP_LAUNCHES
    assert len(grads) == 12 and all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads.values()), sorted(grads)
    for (name, p), b in zip(net.named_parameters(), before):
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), b), name
    assert net.sparsity()[1] == 972
    _lib.check_device(dev)
