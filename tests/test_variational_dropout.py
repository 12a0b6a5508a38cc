"""VariationalDropoutLinear (K23, csrc/bnn_vd.hip): sparse variational dropout (Molchanov, Ashukha, Vetrov 2017).  Every weight has
the posterior N(theta, exp(log_sigma2)) and a log-uniform prior; the layer samples its pre-activation,

    m = x theta^T + mu_b,   v = x^2 exp(log_sigma2)^T + sigma_b^2,   y_s = m + sqrt(v + 1e-16) eps_s,
    log_alpha = clamp(log_sigma2 - ln(theta^2), -8, 8)   (theta = 0: +8)
    KL_e = k1 sigmoid(-(k2 + k3 log_alpha)) + 0.5 log1p(exp(-log_alpha))

eps[b N + n] of the layer's noise key, sample sample0 + s.  CPU tests: the host surface, the torch expressions, the pruning rule, a
seeded training run, the built code object.  GPU tests: every kernel against float64 on the fp32 inputs as given, eps from the key's
CPU twin in oracle.

Bounds.  Forward and backward: test_lrt_device.py's, with exp(log_sigma2) where that file has sigma^2 and its derivative (fp32 mode:
1e-5 of the output scale + 2e-5 sqrt(v); bf16 mode: float64 on the operands as the kernel rounds them, tests/golden/bf16ref.py).
bnn_vd_prepare: ocml expf is a 1-ulp function (2 u, tests/posterior_range.py) and the result is one fp32 number: 3 u relative, and
one quantum of the denormal range (2^-149) where the result is denormal.  The log-uniform KL and its gradient are evaluated in
float64 on the device; what they are held to is derived at test_kl_forward_and_backward.
"""
import ctypes
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, _rng, nn, ops, prune
from bayesianneuralnetworks_amd.nn import (BayesianLinear, BayesianNetworkModule, KLDivergence, NormalLinear, VariationalDropoutLinear,
                                           WeightNormal, WeightVariationalDropout)
from bayesianneuralnetworks_amd._rng import DrawKey
from bayesianneuralnetworks_amd.utils import apply_wb

from bf16ref import chain_layer, gamma, rne_bf16, round_hidden
from test_flipout_mc import _code_object_notes
from test_lrt_device import BWD_SHAPES, EPS_TWIN, assert_within, forward_bound, lrt64, scaled_bound, sigma64, twin_eps

U = 2.0 ** -24
K1, K2, K3 = 0.63576, 1.87320, 1.48695
gpu = pytest.mark.gpu

THETA_GRID = [0.0, 1e-30, -1e-30, 1e-6, -1e-6, 1e-3, -1e-3, 1.0, -1.0, 1e4, -1e4]
LS2_FIXED = [-100.0, -95.0, -88.0, -87.5, -87.0, -50.0, -30.0, -20.0, -12.0, -10.0, -5.0, -1.0, 0.0, 1.0, 5.0, 8.0, 10.0, 20.0]


def log_alpha_raw64(theta, ls2):
    """log_sigma2 - ln(theta^2) in float64, not clamped; +inf at theta = 0."""
    return ls2.double() - 2.0 * torch.log(theta.double().abs())


def wide_grid(n=None, thresholds=(), seed=0):
    """(theta, log_sigma2), fp32: THETA_GRID crossed with LS2_FIXED and 48 seeded draws from [-100, 20], repeated (rolled by one per
    repeat, so that the pairs change) up to n elements.  No element's float64 log_alpha lies within 1e-3 of -8, 8 or a threshold:
    an offender's log_sigma2 is moved by 0.01 steps, and the condition is asserted on the result."""
    g = torch.Generator().manual_seed(seed)
    ls = torch.cat([torch.tensor(LS2_FIXED), torch.rand(48, generator=g) * 120 - 100]).float()
    th = torch.tensor(THETA_GRID).float()
    theta, ls2 = th.repeat_interleave(ls.numel()), ls.repeat(th.numel())
    if n is not None:
        reps = -(-n // theta.numel())
        theta = torch.cat([theta.roll(r) for r in range(reps)])[:n].clone()
        ls2 = torch.cat([ls2 for _ in range(reps)])[:n].clone()
    cuts = (-8.0, 8.0) + tuple(thresholds)
    near = lambda: torch.stack([(log_alpha_raw64(theta, ls2) - c).abs() < 1e-3 for c in cuts]).any(0)       # noqa: E731
    for _ in range(8):
        ls2 = torch.where(near(), ls2 + 0.01, ls2)
    assert not near().any()
    return theta, ls2


def kl64(theta, ls2):
    """The element-wise KL in float64 from the formula itself (numpy, no torch autograd involved)."""
    t, l = theta.double().numpy(), ls2.double().numpy()
    with np.errstate(divide="ignore"):
        la = np.clip(l - np.log(t * t), -8.0, 8.0)
    return torch.from_numpy(K1 / (1.0 + np.exp(K2 + K3 * la)) + 0.5 * np.log1p(np.exp(-la)))


def kl_grad64(theta, ls2):
    """(dKL_e / dtheta, dKL_e / dlog_sigma2) in float64 from the analytic formula: 0 where the clamp is active."""
    raw = log_alpha_raw64(theta, ls2)
    inside = (raw >= -8.0) & (raw <= 8.0)
    la = raw.clamp(-8.0, 8.0)
    s = torch.sigmoid(K2 + K3 * la)
    d = torch.where(inside, -K1 * K3 * s * (1 - s) - 0.5 * torch.sigmoid(-la), torch.zeros_like(la))
    safe = torch.where(theta == 0, torch.ones_like(theta), theta).double()
    return torch.where(inside, d * (-2.0 / safe), torch.zeros_like(d)), d


class VdNet(BayesianNetworkModule):
    def __init__(self, samples=4):
        super().__init__(40, 5, samples=samples)
        self.layers = torch.nn.Sequential(VariationalDropoutLinear(40, 24), torch.nn.ReLU(), VariationalDropoutLinear(24, 5))

    def _forward(self, x):
        return self.layers(x)


def spread_log_sigma2(net, seed):
    """log_sigma2 around the weights' own scale, so that log_alpha covers both sides of a threshold."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, VariationalDropoutLinear):
                w = m.weight
                w.log_sigma2.copy_((2 * torch.log(w.mean.abs().cpu() + 1e-3) + 3 * torch.randn(w.mean.shape, generator=g)).to(w.device))


# ================================================================================================ CPU
def test_layer_surface():
    import pytorch_bayesian.nn as alias
    assert alias.VariationalDropoutLinear is VariationalDropoutLinear and alias.WeightVariationalDropout is WeightVariationalDropout
    assert "VariationalDropoutLinear" not in bnn.nn.__all__ and "WeightVariationalDropout" not in bnn.nn.__all__
    assert issubclass(VariationalDropoutLinear, BayesianLinear) and not issubclass(VariationalDropoutLinear, NormalLinear)
    assert prune.PruneLogAlpha is not None and "PruneLogAlpha" not in prune.__all__
    torch.manual_seed(0)
    a, ref = VariationalDropoutLinear(40, 24), NormalLinear(40, 24)
    assert list(a.state_dict()) == ["weight.mean", "weight.log_sigma2", "bias.mean", "bias.scale"]
    assert list(VariationalDropoutLinear(40, 24, bias=False).state_dict()) == ["weight.mean", "weight.log_sigma2"]
    assert isinstance(a.weight, WeightVariationalDropout) and isinstance(a.bias, WeightNormal) and a.threshold is None
    assert VariationalDropoutLinear(40, 24, bias=False).bias is None
    assert torch.equal(a.weight.log_sigma2, torch.full((24, 40), -10.0))
    bound = 1 / math.sqrt(40)                                     # kaiming_uniform(a = sqrt 5): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
    assert a.weight.mean.abs().max() <= bound and a.weight.mean.std() > 0.4 * bound and ref.weight.mean.abs().max() <= bound
    assert a.bias.mean.abs().max() <= bound and (a.bias.scale + 2).abs().max() < 1.0
    w = a.weight
    assert w.shape == (24, 40) and w.size(1) == 40 and w.device == w.mean.device and w.requires_grad
    assert torch.allclose(w.variance, torch.exp(w.log_sigma2)) and torch.allclose(w.stddev ** 2, w.variance)
    assert torch.equal(w.dist.loc, w.mean) and torch.allclose(w.dist.scale, w.stddev)
    la = w.log_alpha
    assert la.shape == (24, 40) and la.min() >= -8 and la.max() <= 8
    t = WeightVariationalDropout(3)
    with torch.no_grad():
        t.mean.copy_(torch.tensor([0.0, 1.0, 1e-30]))
        t.log_sigma2.copy_(torch.tensor([-50.0, -50.0, 0.0]))
    assert torch.equal(t.log_alpha, torch.tensor([8.0, -8.0, 8.0]))
    # traverse / apply_wb see the layer as a Bayesian leaf with a weight and a bias
    net = VdNet()
    seen = net.traverse(lambda m: apply_wb(m, lambda p, module, type: (type, p), pass_module=True, pass_type=True))
    assert [k for k, _ in seen] == ["w", "b", "w", "b"]
    assert [type(p) for _, p in seen] == [WeightVariationalDropout, WeightNormal] * 2


@pytest.mark.parametrize("bias", [True, False])
def test_cpu_forward_is_the_formula(bias):
    torch.manual_seed(1)
    layer = VariationalDropoutLinear(20, 12, bias=bias)
    with torch.no_grad():
        layer.weight.log_sigma2.copy_(-6 + torch.randn(12, 20))
    x = torch.randn(9, 20)
    torch.manual_seed(77)
    y = layer(x)
    torch.manual_seed(77)
    eps = torch.randn(9, 12)
    ref, _, _ = lrt64(x.double(), x.double() ** 2, layer.weight.mean.double(), torch.exp(layer.weight.log_sigma2.double()),
                      layer.bias.mean.double() if bias else None, sigma64(layer.bias.scale) ** 2 if bias else None, eps.double())
    assert torch.allclose(y.double(), ref, atol=1e-5, rtol=1e-5)
    assert torch.equal(layer(x, sample=False), y)                  # the same noise again
    assert layer(torch.randn(20)).shape == (12,)
    assert layer(torch.randn(9, 3, 20)).shape == (9, 3, 12)
    with pytest.raises(RuntimeError):
        layer(x, sample=False)                                     # the recorded noise has another shape now
    y.sum().backward()
    assert layer.weight.mean.grad is not None and layer.weight.log_sigma2.grad.abs().sum() > 0


def test_kl_divergence_of_a_mixed_model_matches_float64():
    torch.manual_seed(2)

    class Net(BayesianNetworkModule):
        def __init__(self):
            super().__init__(12, 3, samples=1)
            self.layers = torch.nn.Sequential(NormalLinear(12, 9), torch.nn.ReLU(), VariationalDropoutLinear(9, 3))

        def _forward(self, x):
            return self.layers(x)

    net = Net()
    with torch.no_grad():
        net.layers[2].weight.log_sigma2.copy_(-6 + 3 * torch.randn(3, 9))
    terms = []
    for layer in (net.layers[0], net.layers[2]):
        for p in (layer.weight, layer.bias):
            if isinstance(p, WeightVariationalDropout):
                terms.append(kl64(p.mean.detach(), p.log_sigma2.detach()).mean())
            else:
                q = torch.distributions.Normal(p.mean.detach().double(), sigma64(p.scale.detach()))
                prior = torch.distributions.Normal(torch.tensor(0.0, dtype=torch.float64), torch.tensor(0.1).double())   # fp32 0.1
                terms.append(torch.distributions.kl_divergence(q, prior).mean())
    want = torch.stack(terms).mean() / 4.0                          # mean over tensors of per-tensor means, / n_batches
    got = KLDivergence(4)(net)
    assert abs(got.item() - want.item()) <= 1e-5 * (1 + abs(want.item())), (got.item(), want.item())
    assert abs(net.kl_divergence(4).item() - got.item()) <= 1e-7
    one = net.layers[2].kl_divergence()
    assert abs(one.item() - ((terms[2] + terms[3]) / 2).item()) <= 1e-5 * (1 + one.item())
    got.backward()
    assert net.layers[2].weight.mean.grad is not None and net.layers[2].weight.log_sigma2.grad is not None


def test_kl_analytic_gradient_is_float64_autograd():
    """The analytic gradient the kernel implements (kl_grad64) IS float64 autograd of the torch expression, on the whole grid: both
    clamp sides, theta = 0 (exactly 0 there, no NaN).  The expression itself is the formula (kl64)."""
    theta, ls2 = wide_grid()
    t64, l64 = theta.double().requires_grad_(), ls2.double().requires_grad_()
    kl = ops.vd_kl_elements(t64, l64)
    assert torch.allclose(kl, kl64(theta, ls2), rtol=1e-13, atol=0)
    gt, gl = torch.autograd.grad(kl.sum(), (t64, l64))
    assert torch.isfinite(gt).all() and torch.isfinite(gl).all()
    wt, wl = kl_grad64(theta, ls2)
    assert torch.allclose(gt, wt, rtol=1e-12, atol=0) and torch.allclose(gl, wl, rtol=1e-12, atol=0)
    raw = log_alpha_raw64(theta, ls2)
    active = (raw < -8) | (raw > 8)
    assert active.any() and (~active).any() and (raw < -8).any() and (theta == 0).any()
    assert (gt[active] == 0).all() and (gl[active] == 0).all() and (gl[~active] < 0).all()
    # k1 sigmoid(-z), not k1 - k1 sigmoid(z): in fp32 the latter loses its digits at the upper end of the clamp
    la = torch.tensor([8.0])
    good = K1 * torch.sigmoid(-(K2 + K3 * la))
    assert abs(good.item() / (K1 / (1 + math.exp(K2 + K3 * 8.0))) - 1) < 1e-6


def test_prune_log_alpha_sparsity_and_refusals():
    torch.manual_seed(3)
    net = VdNet()
    spread_log_sigma2(net, 4)
    l0, l2 = net.layers[0], net.layers[2]
    la0, la2 = l0.weight.log_alpha.detach().clone(), l2.weight.log_alpha.detach().clone()
    d0, d2 = int((la0 > 3.0).sum()), int((la2 > 3.0).sum())
    assert 0 < d0 < la0.numel()
    assert l0.sparsity() == d0 / la0.numel() and net.sparsity() == (d0 + d2, la0.numel() + la2.numel())
    l0.threshold = 0.0
    assert l0.sparsity() == int((la0 > 0.0).sum()) / la0.numel()
    assert net.sparsity() == (int((la0 > 0.0).sum()) + d2, la0.numel() + la2.numel())
    # a gradient asked for while a threshold is set
    x = torch.randn(6, 40)
    with pytest.raises(ops.BnnHipError, match="inference"):
        l0(x)
    with torch.no_grad():
        ym = l0(x)
    l0.threshold = None
    # the masked forward is the unmasked one on the layer with the same elements overwritten by hand
    keep = (la0 <= 0.0)
    before = [p.detach().clone() for p in net.parameters()]
    prune.PruneLogAlpha(0.0)(net)
    assert torch.equal(l0.weight.mean.detach(), before[0] * keep)
    assert torch.equal(l0.weight.log_sigma2.detach(), torch.where(keep, before[1], torch.tensor(-30.0)))
    assert torch.equal(l0.bias.mean.detach(), before[2]) and torch.equal(l0.bias.scale.detach(), before[3])      # other posteriors: untouched
    assert (l2.weight.mean.detach() == 0).sum() == int((la2 > 0.0).sum())
    with torch.no_grad():
        yp = l0(x, sample=False)
    # pruned: variance e^-30 instead of 0 -- the means agree exactly, the noise term to 1e-6
    assert torch.allclose(yp, ym, atol=1e-5)
    plain = BayesianNetworkModule(4, 2)
    plain.layers = torch.nn.Sequential(NormalLinear(4, 2))
    snap = [p.detach().clone() for p in plain.parameters()]
    prune.PruneLogAlpha()(plain)
    assert all(torch.equal(a, b) for a, b in zip(plain.parameters(), snap))
    with pytest.raises(TypeError, match="PruneLogAlpha"):
        prune.PruneNormal()(net, 0.5)
    # a tracking moment pass: no moment backward
    with pytest.raises(ops.BnnHipError, match="no moment backward"):
        net.forward_moments(x)
    assert "VariationalDropoutLinear" in nn.container._MOMENTS_SUPPORTED


def test_cpu_moment_pass_is_the_float64_recursion():
    torch.manual_seed(5)
    net = VdNet()
    spread_log_sigma2(net, 6)
    nn.moment_activations(net)
    x = torch.randn(7, 40)
    for thr in (None, 1.0):
        net.layers[0].threshold = net.layers[2].threshold = thr
        mom = net.predictive_moments(x)
        h = ops.Moments(x, None)
        for layer in (net.layers[0], net.layers[2]):
            theta, ls2 = layer.weight.mean.detach().double(), layer.weight.log_sigma2.detach().double()
            s2 = torch.exp(ls2)
            if thr is not None:
                keep = ~(ops.vd_log_alpha(theta, ls2) > thr)
                theta, s2 = theta * keep, s2 * keep
            m = h.mean.double() @ theta.t() + layer.bias.mean.detach().double()
            v = (h.mean.double() ** 2) @ s2.t() + sigma64(layer.bias.scale.detach()) ** 2
            if h.var is not None:
                v = v + h.var @ (theta * theta + s2).t()
            h = ops.Moments(m, v)
            if layer is net.layers[0]:
                h = ops.moments_relu_f64(h)
        assert torch.allclose(mom.mean.double(), h.mean, rtol=1e-5, atol=1e-6) and torch.allclose(mom.var.double(), h.var, rtol=1e-5, atol=1e-9)


def test_training_separates_signal_from_noise_inputs():
    """A 16 -> 8 -> 1 regression whose inputs 8..15 are pure noise, torch only, seeded: after 600 Adam steps on MSE + 0.05 KL the
    first layer's log_alpha is clearly higher on the noise columns than on the signal columns, and the loss has fallen.  (Seeds 0,
    1, 2 gave signal / noise means 3.1 / 6.6, 2.5 / 6.5, 1.1 / 6.4 and a 100-fold lower MSE; the assertion is the gap alone.)"""
    torch.manual_seed(1)

    class Net(BayesianNetworkModule):
        def __init__(self):
            super().__init__(16, 1, samples=1)
            self.layers = torch.nn.Sequential(VariationalDropoutLinear(16, 8), torch.nn.ReLU(), VariationalDropoutLinear(8, 1))

        def _forward(self, x):
            return self.layers(x)

    net = Net()
    X = torch.randn(256, 16)
    Y = (X[:, :8] @ torch.randn(8)).unsqueeze(1) * 0.5 + 0.05 * torch.randn(256, 1)
    opt = torch.optim.Adam(net.parameters(), lr=0.03)
    first = None
    for _ in range(600):
        opt.zero_grad()
        mse = ((net(X) - Y) ** 2).mean()
        (mse + 0.05 * net.kl_divergence()).backward()
        opt.step()
        first = mse.item() if first is None else first
    la = net.layers[0].weight.log_alpha.detach()
    signal, noise = la[:, :8].mean().item(), la[:, 8:].mean().item()
    print("MSE %.4f -> %.4f, mean log_alpha: signal columns %.2f, noise columns %.2f, sparsity %s" % (first, mse.item(), signal, noise, net.sparsity()))
    assert noise > signal + 1.0
    assert mse.item() < 0.5 * first


def test_code_object_holds_the_new_kernels():
    """Symbol names and resource notes only: the dense weight-gradient tile of both posteriors in both compute modes (K10's k_lrt
    with the posterior's chain factor as its third template argument: 4 instantiations), both operand kernels and the three KL
    kernels are in the gfx950 code object, each once, and none of them uses scratch."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    want = [r"_ZN3bnn5k_lrtI%sLi2ENS_%sEEEvNS_7LrtArgsE$" % (t, chain) for t in "tf" for chain in ("14ChainLogSigma2", "8ChainRho")]
    want += [r"_ZN3bnn12k_vd_prepareILb1EEE", r"_ZN3bnn12k_vd_prepareILb0EEE", r"_ZN3bnn15k_vd_kl_partialE", r"_ZN3bnn13k_vd_kl_finalE",
             r"_ZN3bnn16k_vd_kl_backwardE"]
    for pat in want:
        found = [f for n, f in kernels.items() if re.match(pat, n)]
        assert len(found) == 1, (pat, sorted(n for n in kernels if "vd" in n or "k_lrtI" in n))
        assert int(found[0].get("vgpr_spill_count", 0)) == 0 and int(found[0].get("private_segment_fixed_size", 0)) == 0, (pat, found[0])


def test_argument_errors_are_reported_without_launching():
    """BNN_E_NULL / SHAPE / ALIGN / DTYPE / UNSUPPORTED / RANGE of the five new entries, each with bnn_last_error text; the pointers
    are plain integers that no refused call dereferences."""
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one, odd, off4 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)
    inf = math.inf

    def refused(rc, code, word):
        msg = lib.bnn_last_error().decode()
        assert rc == code and word in msg, (rc, code, msg)

    refused(lib.bnn_vd_prepare(one, None, 4, None, None, 0, inf, None, one, None, None), -1, "NULL")
    refused(lib.bnn_vd_prepare(one, one, 4, None, None, 0, inf, None, None, None, None), -1, "NULL")
    refused(lib.bnn_vd_prepare(one, one, 4, one, None, 2, inf, None, one, None, None), -1, "NULL")            # a bias without s2_b
    refused(lib.bnn_vd_prepare(one, one, 4, None, None, 0, 3.0, None, one, one, None), -1, "threshold")       # masked: theta_out
    refused(lib.bnn_vd_prepare(one, one, 4, None, None, 0, 3.0, one, one, None, None), -1, "threshold")       # masked: count_out
    refused(lib.bnn_vd_prepare(None, one, 4, None, None, 0, 3.0, one, one, one, None), -1, "theta")
    refused(lib.bnn_vd_prepare(one, one, 0, None, None, 0, inf, None, one, None, None), -2, "extent")
    refused(lib.bnn_vd_prepare(one, one, 4, None, None, -1, inf, None, one, None, None), -2, "extent")
    refused(lib.bnn_vd_prepare(one, one, 4, None, None, 0, math.nan, one, one, one, None), -5, "NaN")
    refused(lib.bnn_vd_prepare(one, odd, 4, None, None, 0, inf, None, one, None, None), -4, "misaligned")
    refused(lib.bnn_vd_prepare(one, one, 4, None, None, 0, 3.0, one, one, off4, None), -4, "misaligned")      # count_out: 8 bytes
    w = lambda *a: lib.bnn_vd_backward_weight(*a)                                                             # noqa: E731
    refused(w(one, 8, one, one, one, one, None, None, None, None, 4, 4, 8, 0, 0, None), -1, "NULL")
    refused(w(one, 8, one, one, None, one, one, None, None, None, 4, 4, 8, 0, 0, None), -1, "NULL")
    refused(w(one, 8, one, one, one, one, one, one, None, None, 4, 4, 8, 0, 0, None), -1, "NULL")             # partial bias
    refused(w(one, 8, one, one, one, one, one, None, None, None, 4, 0, 8, 0, 0, None), -2, "extent")
    refused(w(one, 4, one, one, one, one, one, None, None, None, 4, 4, 8, 0, 0, None), -2, "extent")          # ldx < K
    refused(w(one, 8, one, one, one, one, one, None, None, None, 4, 64 * 65535 + 1, 8, 0, 0, None), -5, "range")
    refused(w(one, 8, one, one, one, one, one, None, None, None, 4, 4, 8, 7, 0, None), -3, "compute")
    refused(w(one, 8, one, one, one, one, one, None, None, None, 4, 4, 8, 0, _lib.FLAG_X_BF16, None), -6, "bf16")
    refused(w(one, 8, one, one, one, off4, one, None, None, None, 4, 4, 8, 0, 0, None), -4, "misaligned")     # g_theta: 16 bytes
    refused(w(one, 8, one, one, one, one, off4, None, None, None, 4, 4, 8, 0, 0, None), -4, "misaligned")
    refused(w(odd, 8, one, one, one, one, one, None, None, None, 4, 4, 8, 0, 0, None), -4, "misaligned")

    def descs(*items):
        arr = (_lib.VdTensor * len(items))()
        for i, (t, l, n) in enumerate(items):
            arr[i].theta, arr[i].log_sigma2, arr[i].n = t, l, n
        return arr

    ok = descs((64, 64, 4))
    many = descs(*[(64, 64, 4)] * 129)
    assert lib.bnn_vd_kl_workspace_bytes(ok, 1) == 8 and lib.bnn_vd_kl_workspace_bytes(descs((64, 64, 2049), (64, 64, 1)), 2) == 24
    assert lib.bnn_vd_kl_workspace_bytes(None, 1) == -1 and lib.bnn_vd_kl_workspace_bytes(many, 129) == -1
    assert lib.bnn_vd_kl_workspace_bytes(descs((64, 64, 0)), 1) == -1
    refused(lib.bnn_vd_kl_forward(None, 1, one, one, None), -1, "NULL")
    refused(lib.bnn_vd_kl_forward(ok, 0, one, one, None), -2, "ntensors")
    refused(lib.bnn_vd_kl_forward(many, 129, one, one, None), -6, "ntensors")
    refused(lib.bnn_vd_kl_forward(descs((64, None, 4)), 1, one, one, None), -1, "NULL")
    refused(lib.bnn_vd_kl_forward(descs((64, 64, 0)), 1, one, one, None), -2, "empty")
    refused(lib.bnn_vd_kl_forward(descs((66, 64, 4)), 1, one, one, None), -4, "misaligned")
    refused(lib.bnn_vd_kl_forward(ok, 1, None, one, None), -1, "NULL")
    refused(lib.bnn_vd_kl_forward(ok, 1, one, None, None), -1, "NULL")
    refused(lib.bnn_vd_kl_forward(ok, 1, one, off4, None), -4, "misaligned")                                  # workspace: 8 bytes
    gp = (ctypes.c_void_p * 1)(64)
    gnull = (ctypes.c_void_p * 1)(None)
    godd = (ctypes.c_void_p * 1)(66)
    refused(lib.bnn_vd_kl_backward(ok, 1, None, gp, gp, 0, None), -1, "NULL")
    refused(lib.bnn_vd_kl_backward(ok, 1, one, None, gp, 0, None), -1, "NULL")
    refused(lib.bnn_vd_kl_backward(ok, 1, one, gp, gnull, 0, None), -1, "NULL")
    refused(lib.bnn_vd_kl_backward(ok, 1, one, godd, gp, 0, None), -4, "misaligned")
    refused(lib.bnn_vd_kl_backward(ok, 1, odd, gp, gp, 0, None), -4, "misaligned")
    refused(lib.bnn_vd_kl_backward(descs((64, 64, -3)), 1, one, gp, gp, 0, None), -2, "empty")
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


def make_params(N, K, bias, seed):
    g = torch.Generator().manual_seed(seed)
    theta = (torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5
    ls2 = -6 + 0.6 * torch.randn(N, K, generator=g)                # sigma around e^-3 = 0.05, as test_lrt_device's rho = -3
    mu_b = (torch.rand(N, generator=g) * 2 - 1) / K ** 0.5 if bias else None
    rho_b = -3 + 0.3 * torch.randn(N, generator=g) if bias else None
    return theta, ls2, mu_b, rho_b


def bound_s2(ls2):
    """|expf(l) - exp(l)|: 1 ulp of the function (2 u) and the rounding of the result, one denormal quantum where it is denormal."""
    return 3 * U * torch.exp(ls2.double()) + 2.0 ** -149


@gpu
@pytest.mark.parametrize("threshold", [None, 3.0, 0.0, -9.0])
def test_prepare_planes_mask_and_count(dev, threshold):
    """s2 within the expf bound of float64 over log_sigma2 in [-100, 20] (underflow to 0 and to denormals included); with a
    threshold the masked planes and the count are EXACT (no element within 1e-3 of a cut: asserted by wide_grid); the bias plane is
    bnn_lrt_prepare's."""
    theta, ls2 = wide_grid(thresholds=() if threshold is None else (threshold,))
    theta, ls2 = torch.cat([theta, theta[:5]]), torch.cat([ls2, ls2[:5]])          # not a multiple of the wave or the workgroup
    rho_b = torch.linspace(-20, 25, 7)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    th_out, s2, s2_b, count = ops._vd_prepare_raw(theta.to(dev), ls2.to(dev), rho_b.to(dev), threshold)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1
    want = torch.exp(ls2.double())
    assert (want[ls2 <= -88] < 2.0 ** -126).all() and (want > 1e8).any()          # denormal and underflowing results, and large ones
    assert_within(s2_b, sigma64(rho_b) ** 2, 1e-6 * sigma64(rho_b) ** 2, "s2_b")
    if threshold is None:
        assert count is None and th_out.data_ptr() != 0
        assert torch.equal(th_out.cpu(), theta)
        assert_within(s2, want, bound_s2(ls2), "s2")
        return
    drop = log_alpha_raw64(theta, ls2).clamp(-8, 8) > threshold
    assert drop.any() and (threshold < -8 or (~drop).any())
    assert int(count.item()) == int(drop.sum())
    assert torch.equal(th_out.cpu(), torch.where(drop, torch.zeros_like(theta), theta))
    assert (s2.cpu()[drop] == 0).all()
    if (~drop).any():                                               # (a threshold below -8 keeps nothing)
        assert_within(s2.cpu()[~drop], want[~drop], bound_s2(ls2)[~drop], "s2 (kept)")
    # the same count on another grid of the same data: 300 000 elements take the grid-stride loop
    big_t, big_l = wide_grid(300000, (threshold,), seed=1)
    c2 = ops.vd_dropped(big_t.to(dev), big_l.to(dev), threshold)
    assert int(c2.item()) == int((log_alpha_raw64(big_t, big_l).clamp(-8, 8) > threshold).sum())
    assert int(ops.vd_dropped(big_t.to(dev), big_l.to(dev), threshold).item()) == int(c2.item())


def vd_operands64(x, theta, ls2, mu_b, rho_b, mode, dev):
    """float64 operands as the kernel contracts them: (x, x^2, theta, s2, mu_b, sigma_b^2) (test_lrt_device.operands64)."""
    want_w = torch.exp(ls2.double())
    want_b = sigma64(rho_b) ** 2 if rho_b is not None else None
    if mode == "f32":
        return x.double(), x.double() ** 2, theta.double(), want_w, None if mu_b is None else mu_b.double(), want_b
    _, s2_w, s2_b, _ = ops._vd_prepare_raw(theta.to(dev), ls2.to(dev), None if rho_b is None else rho_b.to(dev))
    s2_w = s2_w.cpu()
    assert ((s2_w.double() - want_w).abs() <= bound_s2(ls2)).all()
    if rho_b is not None:
        s2_b = s2_b.cpu()
        assert ((s2_b.double() - want_b).abs() <= 1e-6 * want_b).all()
    return (rne_bf16(x), rne_bf16(x.float() * x.float()), rne_bf16(theta), rne_bf16(s2_w),
            None if mu_b is None else mu_b.double(), None if rho_b is None else s2_b.double())


FWD_SHAPES = [(33, 100, 7), (1, 64, 64), (65, 68, 130)]


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_matches_float64_on_the_keys_eps(dev, shape, shared, bias, mode):
    B, K, N = shape
    S = 3
    theta, ls2, mu_b, rho_b = make_params(N, K, bias, 11)
    g = torch.Generator().manual_seed(12)
    x = torch.randn((B, K) if shared else (S, B, K), generator=g)
    key = DrawKey(0x1234567890ABCDEF, 321, 3, S, 17, gen=_rng.generator_for(mode))          # sample0 = 3
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    put = lambda t: None if t is None else t.to(dev)                # noqa: E731
    y = ops.linear_vd(x.to(dev), theta.to(dev), ls2.to(dev), put(mu_b), put(rho_b), key, shared, mode)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 2            # the operand launch + ONE contraction launch for all S samples
    assert y.shape == (S, B, N) and y.dtype == torch.float32
    x64, xsq, th64, s2, mb, s2b = vd_operands64(x, theta, ls2, mu_b, rho_b, mode, dev)
    eps = twin_eps(key, S, (B, N), dev)
    ref, _, v = lrt64(x64, xsq, th64, s2, mb, s2b, eps)
    bound = forward_bound(mode, x64, th64, mb, ref, v, eps, K)
    assert_within(y, ref, bound, "y %s %s" % (shape, mode))
    if mode == "bf16":
        # bf16 activations: the input given as bf16 is what the kernel rounds an fp32 one to -- the same bits; a bf16 output is the
        # fp32 one rounded once more (half a bf16 ulp: 2^-9 |y|)
        # bf16 activations: a bf16 input is squared as it is (the fp32 one is squared first, then rounded), so it has a reference of
        # its own; a bf16 output is the fp32 one rounded once more (bf16 has an 8-bit significand: half an ulp is 2^-8 |y|)
        xb = x.to(dev).bfloat16()
        yb = ops.linear_vd(xb, theta.to(dev), ls2.to(dev), put(mu_b), put(rho_b), key, shared, mode)
        x64, xsq, th64, s2, mb, s2b = vd_operands64(xb.float().cpu(), theta, ls2, mu_b, rho_b, mode, dev)
        ref, _, v = lrt64(x64, xsq, th64, s2, mb, s2b, eps)
        bound = forward_bound(mode, x64, th64, mb, ref, v, eps, K)
        assert_within(yb, ref, bound, "y (bf16 in) %s" % (shape,))
        yo = ops.linear_vd(xb, theta.to(dev), ls2.to(dev), put(mu_b), put(rho_b), key, shared, mode, out_dtype=torch.bfloat16)
        assert yo.dtype == torch.bfloat16
        assert_within(yo.float(), ref, bound + 2.0 ** -8 * (ref.abs() + bound), "y (bf16 in, bf16 out) %s" % (shape,))
    else:
        with pytest.raises(ops.BnnHipError):
            ops.linear_vd(x.to(dev).bfloat16(), theta.to(dev), ls2.to(dev), put(mu_b), put(rho_b), key, shared, mode)     # no torch fallback


@gpu
@pytest.mark.parametrize("shared", [True, False])
def test_forward_on_the_wide_grid(dev, shared):
    """log_sigma2 from the wide grid: the variance plane spans e^-100 (0 in fp32) to e^20, v many decades."""
    B, K, N, S = 33, 100, 7, 3
    theta, _, mu_b, rho_b = make_params(N, K, True, 13)
    _, ls2 = wide_grid(N * K, seed=2)
    ls2 = ls2.reshape(N, K)
    ls2[3] = ls2[3].clamp_max(-30.0)                                # one output whose variance is the bias's alone
    g = torch.Generator().manual_seed(14)
    x = torch.randn((B, K) if shared else (S, B, K), generator=g)
    key = DrawKey(4242, 77, 0, S, 3, gen=_rng.generator_for("f32"))
    n0 = _lib.load().bnn_launch_count()
    y = ops.linear_vd(x.to(dev), theta.to(dev), ls2.to(dev), mu_b.to(dev), rho_b.to(dev), key, shared, "f32")
    assert _lib.load().bnn_launch_count() == n0 + 2
    x64, xsq, th64, s2, mb, s2b = vd_operands64(x, theta, ls2, mu_b, rho_b, "f32", dev)
    eps = twin_eps(key, S, (B, N), dev)
    ref, _, v = lrt64(x64, xsq, th64, s2, mb, s2b, eps)
    assert v.max() / v.min() > 1e10
    # per output column: the scale of a column is its own (the columns differ by many decades)
    for n in range(N):
        col = ref[..., n]
        assert_within(y[..., n], col, scaled_bound(col) + EPS_TWIN * torch.sqrt(v[..., n] + 1e-16), "y[:, %d] wide grid" % n)


def vd_backward64(x, xsq, x_epi, theta, s2, rho_b, v, eps, gy, shared, rnd=None, betas=None):
    """test_lrt_device.backward64 with s2 = exp(log_sigma2) in place of 2 sigma dsigma: g_log_sigma2 = (g_v^T x^2) s2."""
    inv = 0.5 / torch.sqrt(v + 1e-16)
    if shared:
        g_m, g_v = gy.sum(0), (gy * eps).sum(0) * inv
    else:
        g_m, g_v = gy, gy * eps * inv
    c_w = s2
    c_b = None if rho_b is None else 2 * sigma64(rho_b) * torch.sigmoid(rho_b.double())
    h_m, d_m = rnd(g_m, betas[0])
    h_v, d_v = rnd(g_v, betas[1])
    t1, a1, s1, _ = chain_layer(h_m, d_m, theta.t().contiguous(), None)
    t2, a2, s2_, _ = chain_layer(h_v, d_v, s2.t().contiguous(), None)
    gx = t1 + 2 * x_epi * t2
    out = [(gx, a1 + s1 + 2 * x_epi.abs() * (a2 + s2_) + 4 * U * (t1.abs() + 2 * x_epi.abs() * t2.abs()))]
    t, a, s, _ = chain_layer(h_m.t().contiguous(), d_m.t().contiguous(), x.t().contiguous(), None)
    out.append((t, a + s))
    t, a, s, _ = chain_layer(h_v.t().contiguous(), d_v.t().contiguous(), xsq.t().contiguous(), None)
    out.append((t * c_w, (a + s) * c_w + 16 * U * (t * c_w).abs()))           # expf and one product in fp32
    if rho_b is not None:
        M = g_m.shape[0]
        out.append((g_m.sum(0), gamma(M) * g_m.abs().sum(0) + betas[0].sum(0)))
        tb = g_v.sum(0)
        out.append((tb * c_b, (gamma(M) * g_v.abs().sum(0) + betas[1].sum(0)) * c_b + 16 * U * (tb * c_b).abs()))
    return out


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_matches_float64_on_the_keys_eps(dev, shape, shared, bias, mode):
    """g_x, g_theta, g_log_sigma2, g_mu_b, g_rho_b against float64 autograd of the formula on the same eps (fp32 mode) or its
    restatement on the operands as rounded (bf16 mode); the batch holds an all-zero input row."""
    B, K, N = shape
    S = 3
    params = make_params(N, K, bias, 31)
    g = torch.Generator().manual_seed(32)
    x = torch.randn((B, K) if shared else (S, B, K), generator=g)
    x[..., 5 % B, :] = 0
    gy = torch.randn(S, B, N, generator=g)
    key = DrawKey(777, 45, 1, S, 9, gen=_rng.generator_for(mode))
    leaves = [None if t is None else t.to(dev).requires_grad_() for t in (x,) + params]
    lib = _lib.load()
    y = ops.linear_vd(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], key, shared, mode)
    n0 = lib.bnn_launch_count()
    got = torch.autograd.grad(y, [t for t in leaves if t is not None], gy.to(dev))
    torch.cuda.synchronize()
    # the noise launch, the paired input- and weight-gradient contractions, the bias sums: nothing else ran
    assert lib.bnn_launch_count() == n0 + (4 if bias else 3)
    assert all(torch.isfinite(t).all() for t in got)
    theta, ls2, mu_b, rho_b = params
    eps = twin_eps(key, S, (B, N), dev)
    names = ["x", "weight.mean", "weight.log_sigma2"] + (["bias.mean", "bias.scale"] if bias else [])
    if mode == "f32":
        ref = [t.double().requires_grad_() for t in (x,) + params if t is not None]
        p64 = ref[1:] + ([None, None] if not bias else [])
        yr, _, _ = lrt64(ref[0], ref[0] * ref[0], p64[0], torch.exp(p64[1]), p64[2], None if not bias else sigma64(p64[3]) ** 2, eps)
        want = torch.autograd.grad((yr * gy.double()).sum(), ref)
        for n, a, w in zip(names, got, want):
            assert_within(a, w, scaled_bound(w), "g %s %s f32" % (n, shape))
        return
    x64, xsq, th64, s2, mb, s2b = vd_operands64(x, theta, ls2, mu_b, rho_b, mode, dev)
    _, _, v = lrt64(x64, xsq, th64, s2, mb, s2b, eps)
    gy64 = gy.double()
    rel_inv = 1.01 * 0.5 * gamma(K + 1) * v / (v + 1e-16) + 4 * U
    inv = 0.5 / torch.sqrt(v + 1e-16)
    term = gy64.abs() * inv * (eps.abs() * (rel_inv + 3 * U) + EPS_TWIN)
    if shared:
        beta_m = gamma(S) * gy64.abs().sum(0)
        beta_v = 1.01 * (term.sum(0) + gamma(S) * (gy64 * eps).abs().sum(0) * inv)
    else:
        beta_m, beta_v = torch.zeros_like(gy64), 1.01 * term
    flat = (lambda t: t) if shared else (lambda t: t.reshape(S * B, -1))
    # the epilogue multiplies by expf(log_sigma2) in fp32 (not by the bf16-rounded plane): exp64 here
    want = vd_backward64(flat(x64), flat(xsq), flat(x.double()), th64, s2, rho_b if bias else None, flat(v) if not shared else v,
                         flat(eps) if not shared else eps, flat(gy64) if not shared else gy64, shared,
                         rnd=lambda t, beta: round_hidden(t, beta)[:2], betas=(flat(beta_m), flat(beta_v)))
    c_true = torch.exp(ls2.double())
    w2, b2 = want[2]
    want[2] = (w2 / s2 * c_true, b2 / s2 * c_true)
    for n, a, (w, bound) in zip(names, got, want):
        assert_within(a.reshape(w.shape), w, bound + 1e-30, "g %s %s bf16" % (n, shape))


@gpu
@pytest.mark.parametrize("bias", [True, False])
def test_weight_gradient_epilogue_over_the_parameters_range(dev, bias):
    """bnn_vd_backward_weight called directly in the fp32 mode, (M, N, K) = (33, 7, 100) -- one partial tile in each direction -- and
    log_sigma2 from wide_grid's [-100, 20] (exp from 0 and denormals to 5e8): g_theta and the bias gradients are
    bnn_lrt_backward_weight's on the same x, g_m, g_v bit for bit (one tile, one host function; only the chain factor differs), and
    with t = g_v^T x^2, l = log_sigma2

        |g_log_sigma2 - t64 exp(l)| <= b_t exp(l) (1 + 4 u) + 4 u |t64| exp(l) + 2^-149

    test_variational_dropout_conv.py's epilogue bound (one 2-u expf and one product; below l = -87, where expf is a denormal, the
    fp64 product rounded once: ONE quantum), with b_t the allowance test_backward_matches_float64_on_the_keys_eps gives the fp32
    mode's contraction, scaled_bound(t64) (1e-5 of t's scale; the ordered fp32 chain over M = 33 addends stays below gamma(33)
    sum |g_v| x^2 = 2e-6 sum |g_v| x^2, which is inside it).  Worst err / bound the MI355X run printed: g_log_sigma2 0.397
    (with the epilogue that multiplied by the denormal expf, before the dense and the conv layer shared ChainLogSigma2:
    9.569, at an element below -87)."""
    M, N, K = 33, 7, 100
    _, ls2 = wide_grid(N * K, seed=5)
    assert ls2.min() <= -99 and ls2.max() >= 19 and ((ls2 >= -100) & (ls2 < -87)).any()
    ls2 = ls2.reshape(N, K)
    g = torch.Generator().manual_seed(43)
    x = torch.randn(M, K, generator=g)
    g_m = torch.randn(M, N, generator=g)
    g_v = torch.randn(M, N, generator=g)
    rho_w = -3 + 0.3 * torch.randn(N, K, generator=g)
    rho_b = -3 + 0.3 * torch.randn(N, generator=g)
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    xd, gmd, gvd, ld, rwd, rbd = (t.to(dev) for t in (x, g_m, g_v, ls2, rho_w, rho_b))
    outs = {}
    for which in ("lrt", "vd"):
        gw, gs = torch.empty_like(ld), torch.empty_like(ld)
        gmb, grb = (torch.empty_like(rbd), torch.empty_like(rbd)) if bias else (None, None)
        fn = lib.bnn_lrt_backward_weight if which == "lrt" else lib.bnn_vd_backward_weight
        n0 = lib.bnn_launch_count()
        _lib.check(fn(_lib.ptr(xd), K, _lib.ptr(gmd), _lib.ptr(gvd), _lib.ptr(rwd if which == "lrt" else ld), _lib.ptr(gw), _lib.ptr(gs),
                      _lib.ptr(rbd) if bias else None, _lib.ptr(gmb), _lib.ptr(grb), M, N, K, _lib.COMPUTE_F32, 0, st), which)
        torch.cuda.synchronize()
        assert lib.bnn_launch_count() == n0 + (2 if bias else 1)
        outs[which] = (gw, gs, gmb, grb)
    assert torch.equal(outs["vd"][0], outs["lrt"][0])                     # g_theta: the same tile, the same accumulation order
    if bias:
        assert torch.equal(outs["vd"][2], outs["lrt"][2]) and torch.equal(outs["vd"][3], outs["lrt"][3])
    t = g_v.double().t() @ x.double() ** 2
    b_t = scaled_bound(t)
    c = torch.exp(ls2.double())
    want = t * c
    assert (want.abs()[ls2 <= -95] < 2.0 ** -126).all() and want.abs().max() > 1e8
    assert_within(outs["vd"][1], want, b_t * c * (1 + 4 * U) + 4 * U * want.abs() + 2.0 ** -149, "g_log_sigma2, wide grid")


def _off_boundary(t, dev, off_floats=1):
    """t on the device, its first element off_floats floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=dev)
    start = (-(buf.data_ptr() // 4) % 4 + off_floats) % 4
    view = buf[start:start + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off_floats
    return view


@gpu
@pytest.mark.parametrize("offset", ["aligned", "theta+4", "log_sigma2+4"])
def test_kl_forward_and_backward(dev, offset):
    """Three tensors in one call, n = 1, 2049, 5000, over the theta x log_sigma2 grid (both clamp sides, theta = 0), aligned and with
    one operand 4 bytes off a 16-byte boundary; accumulate on and off; two calls bit-identical.

    Bound.  The device evaluates log_alpha, KL_e and dKL_e in float64 from the fp32 inputs and adds in float64, so against a
    float64 reference on the same inputs what remains is
      * float64 rounding: log_alpha = l - 2 ln|theta| carries <= (|l| + |ln theta^2|) 2^-53 + 2^-52 <= 4e-14 absolute (|l| <= 100,
        |ln theta^2| <= 140), times |dKL / dlog_alpha| <= 0.5 + k1 k3 / 4 < 0.74, i.e. <= 3e-14 per element, against KL_e >= 1.6e-4
        (its value at log_alpha = 8): <= 2e-10 relative; a dozen further float64 roundings and the summation order (n 2^-53) are
        below that.  Allowed: 1e-9 relative.
      * ONE rounding to fp32 of the per-tensor sum, and of every gradient element: u = 2^-24 relative.  The gradient of theta is
        d (-2 / theta) upstream / n with every factor a float64: the same two terms.
      * accumulate: g_old + g in fp32, one more rounding of the sum: u |g_old + g|.
    So |err| <= (u + 1e-9) |ref| (+ u |g_old + ref| when accumulating; + 2^-149: a result may be denormal).
    Where the clamp is active the gradient is exactly 0 (theta = 0 included), and no element is within 1e-3 of a clamp end.
    Worst err / bound the MI355X run printed: per-tensor sums 0.707, means 0.758 (two roundings allowed), g_theta 0.821,
    g_log_sigma2 0.791, accumulated g_theta 0.902, accumulated g_log_sigma2 0.972 -- the same figures at all three alignments."""
    ns = (1, 2049, 5000)
    tensors = [wide_grid(n, seed=3 + i) for i, n in enumerate(ns)]
    tensors[0] = (torch.tensor([0.3]), torch.tensor([-4.0]))                     # n = 1: inside the clamp
    thetas = [t.to(dev) for t, _ in tensors]
    ls2s = [l.to(dev) for _, l in tensors]
    if offset == "theta+4":
        thetas[1] = _off_boundary(tensors[1][0], dev)
    elif offset == "log_sigma2+4":
        ls2s[2] = _off_boundary(tensors[2][1], dev)
    else:
        assert all(t.data_ptr() % 16 == 0 for t in thetas + ls2s)
    for t in thetas + ls2s:
        t.requires_grad_()
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    out = ops.vd_kl(thetas, ls2s)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 2                                       # the partial launch + the fixed-order second pass
    assert out.shape == (3,) and out.dtype == torch.float32
    assert torch.equal(ops.vd_kl(thetas, ls2s), out)                              # identical calls: identical bits
    # ... and the element loads of an operand off the boundary add what the 16-byte loads add: the aligned call's bits
    assert torch.equal(ops.vd_kl([t.to(dev) for t, _ in tensors], [l.to(dev) for _, l in tensors]), out)
    want = torch.stack([kl64(t, l).sum() / n for (t, l), n in zip(tensors, ns)])
    assert_within(out, want, (2 * U + 1e-9) * want, "vd_kl means")               # the sum's rounding and the division's
    # the raw sums: one rounding
    arr = ops._vd_descs([t.detach() for t in thetas], [l.detach() for l in ls2s])
    ws = torch.empty(lib.bnn_vd_kl_workspace_bytes(arr, 3) // 8, dtype=torch.float64, device=dev)
    sums = torch.empty(3, device=dev)
    _lib.check(lib.bnn_vd_kl_forward(arr, 3, _lib.ptr(sums), _lib.ptr(ws), _lib.stream_ptr(dev)), "bnn_vd_kl_forward")
    wsum = torch.stack([kl64(t, l).sum() for t, l in tensors])
    assert_within(sums, wsum, (U + 1e-9) * wsum, "vd_kl sums")
    # backward, accumulate off: autograd; upstream differs per tensor
    up = torch.tensor([0.7, -1.3, 2.0])
    n1 = lib.bnn_launch_count()
    grads = torch.autograd.grad(out, thetas + ls2s, up.to(dev))
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n1 + 1
    refs = []
    for i, ((t, l), n) in enumerate(zip(tensors, ns)):
        gt, gl = kl_grad64(t, l)
        refs.append((gt * up[i].double() / n, gl * up[i].double() / n))
        raw = log_alpha_raw64(t, l)
        active = (raw < -8) | (raw > 8)
        for got, ref, what in ((grads[i], refs[i][0], "g_theta"), (grads[3 + i], refs[i][1], "g_log_sigma2")):
            assert (got.cpu()[active] == 0).all(), what
            assert_within(got, ref, (U + 1e-9) * ref.abs() + 2.0 ** -149, "%s n=%d %s" % (what, n, offset))
    raw = log_alpha_raw64(*tensors[2])
    assert (raw < -8).any() and (raw > 8).any() and ((raw > -8) & (raw < 8)).any() and (tensors[2][0] == 0).any()
    # accumulate on: onto a known gradient, twice the same bits
    g = torch.Generator().manual_seed(9)
    olds = [torch.randn(n, generator=g) for n in ns] + [torch.randn(n, generator=g) for n in ns]
    runs = []
    for _ in range(2):
        bufs = [o.to(dev) for o in olds]
        gt = (ctypes.c_void_p * 3)(*[b.data_ptr() for b in bufs[:3]])
        gl = (ctypes.c_void_p * 3)(*[b.data_ptr() for b in bufs[3:]])
        upd = up.to(dev)
        _lib.check(lib.bnn_vd_kl_backward(arr, 3, _lib.ptr(upd), gt, gl, 1, _lib.stream_ptr(dev)), "bnn_vd_kl_backward")
        torch.cuda.synchronize()
        runs.append([b.cpu() for b in bufs])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    for i in range(3):
        for got, old, ref, what in ((runs[0][i], olds[i], refs[i][0], "g_theta"), (runs[0][3 + i], olds[3 + i], refs[i][1], "g_log_sigma2")):
            tot = old.double() + ref
            assert_within(got, tot, (U + 1e-9) * ref.abs() + U * tot.abs() + 2.0 ** -149, "%s += n=%d %s" % (what, ns[i], offset))


def vd_net64(net, x, S, dev, thr=None):
    """The serial float64 restatement on the recorded noise keys, the noise read from the device stream of each key
    (test_lrt_device.net64)."""
    outs = []
    for s in range(S):
        h = x.double().cpu()
        for layer in net.layers:
            if isinstance(layer, VariationalDropoutLinear):
                key = layer.noise_key
                B, N = h.shape[0], layer.weight.mean.shape[0]
                eps = ops.eps_philox((B * N,), key, dev)[s].reshape(B, N).double().cpu()
                h, _, _ = lrt64(h, h * h, layer.weight.mean.detach().double().cpu(), torch.exp(layer.weight.log_sigma2.detach().double().cpu()),
                                layer.bias.mean.detach().double().cpu(), sigma64(layer.bias.scale.detach().cpu()) ** 2, eps)
            else:
                h = h.clamp_min(0)
        outs.append(h)
    return torch.stack(outs)


@gpu
def test_network_batched_pass_kl_and_training_step(dev):
    torch.manual_seed(6)
    S, B = 4, 32
    net = VdNet(S).to(dev)
    spread_log_sigma2(net, 7)
    with torch.no_grad():
        for m in (net.layers[0], net.layers[2]):
            m.weight.log_sigma2.sub_(4.0)                           # mostly signal: the outputs are not all noise
    net.mc_batched = True
    x = torch.randn(B, 40, device=dev)
    lib = _lib.load()
    bnn.manual_seed(100)
    n0 = lib.bnn_launch_count()
    with torch.no_grad():
        ys = net.forward_stacked(x, S)
    assert lib.bnn_launch_count() == n0 + 4            # per layer: the operand launch + one contraction launch for all S samples
    keys = [l.noise_key for l in net.layers if isinstance(l, VariationalDropoutLinear)]
    assert [k.nsamples for k in keys] == [S] * 2 and len({k.stream for k in keys}) == 2
    want = vd_net64(net, x, S, dev)
    assert_within(ys, want, scaled_bound(want), "2-layer VD net")
    # sample s of the batched pass IS the single-sample call on the key's sample sample0 + s: the same bits
    for s in range(S):
        bnn.manual_seed(100)
        with torch.no_grad():
            one = net.forward_stacked(x, 1, sample0=s)
        assert net.layers[0].noise_key.sample0 == s and net.layers[0].noise_key.nsamples == 1
        assert torch.equal(one[0], ys[s]), s
    # KL: the log-uniform KL of the two weights and the Gaussian KL of the two biases, mean of per-tensor means
    terms = []
    for layer in (net.layers[0], net.layers[2]):
        terms.append(kl64(layer.weight.mean.detach().cpu(), layer.weight.log_sigma2.detach().cpu()).mean())
        q = torch.distributions.Normal(layer.bias.mean.detach().double().cpu(), sigma64(layer.bias.scale.detach().cpu()))
        terms.append(torch.distributions.kl_divergence(q, torch.distributions.Normal(torch.tensor(0.0).double(), torch.tensor(0.1).double())).mean())
    wkl = torch.stack(terms).mean().item()
    n1 = lib.bnn_launch_count()
    kl = net.kl_divergence()
    assert lib.bnn_launch_count() > n1
    assert abs(kl.item() - wkl) <= 1e-5 * (1 + abs(wkl)), (kl.item(), wkl)
    assert abs(KLDivergence(7)(net).item() - wkl / 7) <= 1e-5 * (1 + abs(wkl)) / 7
    # ... and its gradient reaches all eight posterior tensors: float64 autograd of the same expression
    ref = {n: p.detach().double().cpu().requires_grad_() for n, p in net.named_parameters()}
    rterms = []
    for i in ("0", "2"):
        rterms.append(ops.vd_kl_elements(ref["layers.%s.weight.mean" % i], ref["layers.%s.weight.log_sigma2" % i]).mean())
        q = torch.distributions.Normal(ref["layers.%s.bias.mean" % i], F.softplus(ref["layers.%s.bias.scale" % i]) + 1e-10)
        rterms.append(torch.distributions.kl_divergence(q, torch.distributions.Normal(torch.tensor(0.0).double(), torch.tensor(0.1).double())).mean())
    torch.stack(rterms).mean().backward()
    net.zero_grad()
    kl.backward()
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        # the 1e-5 parity rule at the tensor's OWN scale (the gradients are 1e-4 and smaller: max(1, rms) would hide them)
        w = ref[n].grad
        assert_within(p.grad, w, 1e-5 * w.abs() + 1e-5 * w.pow(2).mean().sqrt(), "dKL / d" + n)
    net.zero_grad()
    # one Adam step moves all four posterior tensors of both layers
    before = [p.detach().clone() for p in net.parameters()]
    assert len(before) == 8
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    target = torch.randint(0, 5, (B,), device=dev)
    n2 = lib.bnn_launch_count()
    loss = KLDivergence()(net) + sum(F.cross_entropy(y, target) for y in net(x)) / S
    loss.backward()
    opt.step()
    assert lib.bnn_launch_count() >= n2 + 4 + 2 * 4 + 3
    for (name, p), b in zip(net.named_parameters(), before):
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), b), name
    assert net.sparsity()[1] == 40 * 24 + 24 * 5
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_predictive_moments_is_the_float64_recursion(dev, mode):
    """Layer by layer, each against float64 on the DEVICE's own input of that layer (test_moment_propagation's scheme): the fp32
    mode within 1e-5 of the output scale, the bf16 mode within the accumulation bound on the operands as rounded; the ReLU between
    them is bnn_moments_relu's launch (held to float64 in test_moment_propagation.py), and the pass through the network gives the
    chained calls' bits."""
    torch.manual_seed(8)
    bnn.set_compute(mode)
    net = VdNet().to(dev)
    spread_log_sigma2(net, 9)
    nn.moment_activations(net)
    x = torch.randn(19, 40, device=dev)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    mom = net.predictive_moments(x)
    assert lib.bnn_launch_count() == n0 + 5            # two operand launches, two contractions, the ReLU
    l0, l2 = net.layers[0], net.layers[2]
    pre = ops.moments_linear_vd(x, *l0._posterior(), compute=mode)
    hid = ops.moments_relu(pre)
    out = ops.moments_linear_vd(hid, *l2._posterior(), compute=mode)
    assert torch.equal(out.mean, mom.mean) and torch.equal(out.var, mom.var)
    for layer, a, got in ((l0, ops.Moments(x, None), pre), (l2, hid, out)):
        theta, ls2, mu_b, rho_b = [t.detach().cpu() for t in layer._posterior()]
        K = theta.shape[1]
        am = a.mean.cpu()
        av = None if a.var is None else a.var.cpu()
        if mode == "f32":
            r = ops.moments_linear_vd_f64(ops.Moments(am, av), theta, ls2, mu_b, rho_b)
            bm, bv = scaled_bound(r.mean), scaled_bound(r.var)
            m, v = r.mean, r.var
        else:
            _, s2d, _, _ = ops._vd_prepare_raw(theta.to(dev), ls2.to(dev), None)
            s2f = s2d.cpu()
            am_r, th_r, s2_r = rne_bf16(am), rne_bf16(theta), rne_bf16(s2f)
            asq_r = rne_bf16(am.float() * am.float())
            m = am_r @ th_r.t() + mu_b.double()
            v = asq_r @ s2_r.t() + sigma64(rho_b) ** 2
            a_abs = am_r.abs() @ th_r.abs().t() + mu_b.double().abs()
            n_v = K
            if av is not None:
                w2 = rne_bf16(torch.addcmul(s2f, theta, theta))     # fma(theta, theta, s2) in fp32, then rounded
                v = v + rne_bf16(av) @ w2.t()
                n_v = 2 * K
            bm, bv = gamma(K + 1) * a_abs + 1e-300, gamma(n_v + 1) * v + 1e-6 * sigma64(rho_b) ** 2 + 1e-300
        assert_within(got.mean, m, bm, "m %s %s" % (tuple(theta.shape), mode))
        assert_within(got.var, v, bv, "v %s %s" % (tuple(theta.shape), mode))
    # a folded ReLU is the same launch's epilogue: the standalone ReLU's bits
    l0.activation = 'relu'
    folded = ops.moments_linear_vd(x, *l0._posterior(), relu=True, compute=mode)
    assert torch.equal(folded.mean, hid.mean) and torch.equal(folded.var, hid.var)
    with pytest.raises(ops.BnnHipError, match="no moment backward"):
        net.forward_moments(x)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_threshold_is_the_hand_masked_layer(dev, mode):
    """With a threshold every path -- the sampling forward, the MC-batched pass, the moment pass -- gives the bits of the unmasked
    network whose dropped elements were overwritten by hand (theta = 0, log_sigma2 = -inf: s2 = 0), on the same keys."""
    torch.manual_seed(10)
    bnn.set_compute(mode)
    thr = 1.0
    S, B = 4, 16
    net = VdNet(S).to(dev)
    spread_log_sigma2(net, 11)
    with torch.no_grad():                                           # no log_alpha within 1e-3 of the threshold or of +-8 (asserted below)
        for m in (net.layers[0], net.layers[2]):
            raw = log_alpha_raw64(m.weight.mean.cpu(), m.weight.log_sigma2.cpu())
            near = ((raw - thr).abs() < 5e-3) | ((raw.abs() - 8).abs() < 5e-3)
            m.weight.log_sigma2.add_(0.02 * near.to(dev))
    nn.moment_activations(net)
    hand = VdNet(S).to(dev)
    nn.moment_activations(hand)
    hand.load_state_dict(net.state_dict())
    net.mc_batched = hand.mc_batched = True
    dropped = 0
    with torch.no_grad():
        for a, b in ((net.layers[0], hand.layers[0]), (net.layers[2], hand.layers[2])):
            raw = log_alpha_raw64(a.weight.mean.cpu(), a.weight.log_sigma2.cpu())
            assert not (((raw - thr).abs() < 1e-3) | ((raw.abs() - 8).abs() < 1e-3)).any()
            drop = (raw.clamp(-8, 8) > thr).to(dev)
            assert drop.any() and (~drop).any()
            dropped += int(drop.sum())
            b.weight.mean[drop] = 0
            b.weight.log_sigma2[drop] = -math.inf
            a.threshold = thr
    assert net.sparsity() == (dropped, 40 * 24 + 24 * 5)
    x = torch.randn(B, 40, device=dev)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    # the sampling forward of one layer, outside any pass
    with torch.no_grad():
        bnn.manual_seed(7)
        ya = net.layers[0](x)
        hand.layers[0].noise_key, hand.layers[0]._noise_shape = net.layers[0].noise_key, net.layers[0]._noise_shape
        yb = hand.layers[0](x, sample=False)
    assert torch.equal(ya, yb) and lib.bnn_launch_count() > n0
    # the MC-batched pass: same seed, same epochs -- but the two nets' noise streams differ: hand the keys over layer by layer
    with torch.no_grad():
        bnn.manual_seed(8)
        full = net.forward_stacked(x, S)
        for a, b in ((net.layers[0], hand.layers[0]), (net.layers[2], hand.layers[2])):
            b.noise_key, b._noise_shape = a.noise_key, a._noise_shape
        with _mc.McContext(S, B, sample0=0):
            h = hand.layers[0](x, sample=False)
            h = hand.layers[2](hand.layers[1](h), sample=False)
    assert torch.equal(full.reshape(S * B, -1), h)
    # the moment pass
    ma, mb = net.predictive_moments(x), hand.predictive_moments(x)
    assert torch.equal(ma.mean, mb.mean) and torch.equal(ma.var, mb.var)
    # the mask is for inference
    with pytest.raises(ops.BnnHipError, match="inference"):
        net.layers[0](x)
    with pytest.raises(ops.BnnHipError, match="inference"):
        net(x)
    # ... a gradient of the INPUT alone is not a posterior gradient: it goes through the masked layer
    for p in list(net.parameters()) + list(hand.parameters()):
        p.requires_grad_(False)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    bnn.manual_seed(9)
    net.layers[0](xa).sum().backward()
    hand.layers[0].noise_key = net.layers[0].noise_key
    hand.layers[0](xb, sample=False).sum().backward()
    assert torch.isfinite(xa.grad).all() and torch.equal(xa.grad, xb.grad)
