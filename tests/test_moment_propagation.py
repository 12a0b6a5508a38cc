"""Sampling-free inference by moment propagation (K16, csrc/bnn_moments.hip): a mean and a variance per activation through
NormalLinear / LocalReparamLinear,

    m = a_m mu_w^T + mu_b,   v = a_m^2 (sigma_w^2)^T + a_v (mu_w^2 + sigma_w^2)^T + sigma_b^2,

the moment-matched ReLU, and one sampling launch on the logits.  CPU tests: the recursion's exactness for one hidden layer against
weight sampling, the ReLU's limits, the host surface, the argument checks, the built code object.  GPU tests: the kernels against
float64 (ops.moments_f64 and friends), the network pass, the tails, graph capture.

Bounds.  fp32 mode: 1e-5 of the output scale (conftest.assert_close_scaled's rule, test_lrt_device.scaled_bound).  bf16 mode: the
reference is float64 on the six planes as the kernel rounds them (a_m, a_m^2 -- squared in fp32 first --, a_v, mu_w, sigma_w^2,
fma(mu_w, mu_w, sigma_w^2) in fp32 first, each to bf16, RNE); products of bf16 values are exact in fp32, so the device differs by
the fp32 accumulation alone: gamma_n sum |a| |b| with n the addends of the accumulator -- K + 1 for m, 2 K + 1 for v, whose two
sums share one accumulator (tests/golden/bf16ref.py).  Sampling: K10's bound, the scaled bound + 2e-5 sd (the device eps against
its CPU twin).  ReLU: RELU_MEAN_TOL / RELU_VAR_TOL below, 4 x the device's measured worst deviation from float64.
"""
import ctypes
import math
import re

import pytest
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, _rng, ops
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, NormalLinear, LocalReparamLinear
from bayesianneuralnetworks_amd._rng import DrawKey

from bf16ref import gamma, rne_bf16
from test_flipout_mc import _code_object_notes
from test_lrt_device import EPS_TWIN, assert_within, scaled_bound, sigma64, twin_eps

gpu = pytest.mark.gpu

# The moment-matched ReLU against float64, in units of s = sqrt(v) (mean) and of v (variance).  Measured on the MI355X over
# alpha in [-12, 12] (4801 points) at v = 1e-6, 0.3, 1, 47 (test_relu_matches_float64_on_a_grid prints them): worst mean deviation
# 9.313e-7 s (at v = 1e-6), worst variance deviation 1.887e-7 v (at v = 1e-6).  The constants are 4 x that: the margin covers
# inputs off the grid.  Both are below 1e-5, the project's parity rule.
RELU_MEAN_TOL = 3.73e-6
RELU_VAR_TOL = 7.55e-7


def params(N, K, bias, seed, rho0=-3.0):
    g = torch.Generator().manual_seed(seed)
    mu_w = (torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5
    rho_w = rho0 + 0.3 * torch.randn(N, K, generator=g)
    mu_b = (torch.rand(N, generator=g) * 2 - 1) / K ** 0.5 if bias else None
    rho_b = rho0 + 0.3 * torch.randn(N, generator=g) if bias else None
    return mu_w, rho_w, mu_b, rho_b


def six_se(samples, mean, var, what):
    """samples (S, ...) float64 against the claimed mean / var: every sample mean within 6 standard errors, every sample variance
    within 6 standard errors estimated from the samples' own fourth central moment (the outputs are not Gaussian)."""
    S = samples.shape[0]
    sm = samples.mean(0)
    d = samples - sm
    sv = (d * d).sum(0) / (S - 1)
    m4 = (d ** 4).mean(0)
    z_m = ((sm - mean).abs() / (sv / S).sqrt()).max().item()
    z_v = ((sv - var).abs() / ((m4 - sv * sv).clamp_min(0) / S).sqrt()).max().item()
    print("%s: worst mean %.2f standard errors, worst variance %.2f standard errors, worst |var ratio - 1| %.4f"
          % (what, z_m, z_v, (sv / var - 1).abs().max().item()))
    assert z_m <= 6 and z_v <= 6, (what, z_m, z_v)


class Mlp(BayesianNetworkModule):
    def __init__(self, widths, layer=NormalLinear, relu_module=True, samples=4):
        super().__init__(widths[0], widths[-1], samples=samples)
        mods = []
        for i, (k, n) in enumerate(zip(widths[:-1], widths[1:])):
            mods.append(layer(k, n))
            if i < len(widths) - 2:
                mods.append(torch.nn.ReLU() if relu_module else torch.nn.Identity())
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


def bayes_layers(net):
    return [m for m in net.layers if isinstance(m, (NormalLinear, LocalReparamLinear))]


def layer_specs(net):
    return [(m.weight.mean, m.weight.scale, m.bias.mean, m.bias.scale, m.activation == 'relu') for m in bayes_layers(net)]


# ================================================================================================ CPU
def test_one_hidden_layer_is_exact_against_weight_sampling():
    """6 -> 5 -> 3 with biases, 2 rows, 250 000 float64 weight draws: for ONE hidden ReLU layer the recursion's marginal mean and
    variance of every logit are exact (the hidden units are independent given a deterministic input)."""
    S = 250_000
    g = torch.Generator().manual_seed(2024)
    l1 = [t.double() for t in params(5, 6, True, 1, rho0=-1.0)]
    l2 = [t.double() for t in params(3, 5, True, 2, rho0=-1.0)]
    x = torch.randn(2, 6, generator=g, dtype=torch.float64)
    mom = ops.moments_f64(x, [(*l1, True), (*l2, False)])
    assert mom.mean.dtype == torch.float64 and mom.mean.shape == (2, 3) and (mom.var > 0).all()

    def draw(mu, rho):
        return mu + sigma64(rho) * torch.randn((S,) + tuple(mu.shape), generator=g, dtype=torch.float64)

    h = (torch.einsum("bk,snk->sbn", x, draw(l1[0], l1[1])) + draw(l1[2], l1[3]).unsqueeze(1)).clamp_min(0)
    y = torch.einsum("sbk,snk->sbn", h, draw(l2[0], l2[1])) + draw(l2[2], l2[3]).unsqueeze(1)
    six_se(y, mom.mean, mom.var, "6-5-3 against %d weight draws" % S)


def test_relu_limits_and_closed_form():
    f = ops.moments_relu_f64
    for v in (1e-6, 0.3, 47.0):
        s = math.sqrt(v)
        t64 = lambda a: torch.tensor([a], dtype=torch.float64)         # noqa: E731
        hi, lo = f(ops.Moments(t64(12 * s), t64(v))), f(ops.Moments(t64(-12 * s), t64(v)))
        assert abs(hi.mean.item() - 12 * s) <= 1e-12 * s and abs(hi.var.item() - v) <= 1e-12 * v       # passes the input
        assert 0 <= lo.mean.item() <= 1e-30 * s and 0 <= lo.var.item() <= 1e-30 * v                     # nothing comes through
    z = f(ops.Moments(torch.tensor([-2.0, 0.0, 3.0]), torch.zeros(3)))
    assert torch.equal(z.mean, torch.tensor([0.0, 0.0, 3.0], dtype=torch.float64)) and torch.equal(z.var, torch.zeros(3, dtype=torch.float64))
    assert f(ops.Moments(torch.tensor([-1.0, 2.0]))).var is None
    alpha = torch.linspace(-12, 12, 2401, dtype=torch.float64)
    for v in (1e-6, 0.3, 1.0, 47.0):
        vv = torch.full_like(alpha, v)
        m = alpha * math.sqrt(v)
        out = f(ops.Moments(m, vv))
        assert (out.var >= 0).all() and (out.mean >= 0).all()
        # E[y] and E[y^2] - E[y]^2 of max(N(m, v), 0), written the naive way in float64
        cdf = 0.5 * torch.special.erfc(-alpha / math.sqrt(2.0))
        pdf = torch.exp(-0.5 * alpha * alpha) / math.sqrt(2 * math.pi)
        mean = m * cdf + math.sqrt(v) * pdf
        var = (m * m + v) * cdf + m * math.sqrt(v) * pdf - mean * mean
        assert (out.mean - mean).abs().max() <= 1e-13 * math.sqrt(v)
        assert (out.var - var).abs().max() <= 1e-12 * v


def test_cpu_surface():
    torch.manual_seed(0)
    net = Mlp([6, 5, 3])
    assert bnn.nn.fuse_activations(net) == 1
    x = torch.randn(4, 6)
    keys = [(m.weight.draw_key, m.bias.draw_key) for m in bayes_layers(net)]
    e0 = _rng.default_generator.epoch_host
    mom = net.predictive_moments(x)
    want = ops.moments_f64(x, layer_specs(net))
    assert isinstance(mom, ops.Moments) and mom.mean.dtype == torch.float32 and not mom.mean.requires_grad
    assert torch.equal(mom.mean, want.mean.float()) and torch.equal(mom.var, want.var.float())
    assert _mc.moments_current() is None and _rng.default_generator.epoch_host == e0
    assert [(m.weight.draw_key, m.bias.draw_key) for m in bayes_layers(net)] == keys
    lrt = Mlp([6, 5, 3], layer=LocalReparamLinear, relu_module=False)
    lrt.load_state_dict(net.state_dict())
    lrt.layers[0].activation = 'relu'
    got = lrt.predictive_moments(x)
    assert torch.equal(got.mean, mom.mean) and torch.equal(got.var, mom.var)
    # the tails read the sampled logits
    torch.manual_seed(5)
    u = net.predictive_uncertainty(x, samples=8, inputs="logits", propagation="moments")
    torch.manual_seed(5)
    ys = ops.moments_sample(mom, None, 8)
    assert ys.shape == (8, 4, 3)
    r = ops.uncertainty_f64(ys, "logits")
    assert all(torch.equal(a, b) for a, b in zip(u, r))
    torch.manual_seed(5)
    assert torch.equal(net.predictive_mean(x, samples=8, propagation="moments"), ys.sum(0) * (1.0 / 8))
    torch.manual_seed(5)
    t = torch.tensor([0, 2, 1, 1])
    sc = net.predictive_score(x, t, samples=8, inputs="logits", propagation="moments")
    assert all(torch.equal(a, b) for a, b in zip(sc, ops.score_f64(ys, t, "logits")[0]))
    torch.manual_seed(5)
    rg = net.predictive_regression(x, samples=8, outputs="values", propagation="samples")
    assert rg.mean.shape == (4, 3) and not torch.equal(rg.mean, mom.mean)          # the sampler is still there
    # 'values' needs no sampling: the propagated moments are the answer
    rv = net.predictive_regression(x, outputs="values", propagation="moments")
    assert torch.equal(rv.mean, mom.mean) and torch.equal(rv.total, mom.var) and torch.equal(rv.epistemic, mom.var)
    assert torch.equal(rv.aleatoric, torch.zeros(4, 3))
    torch.manual_seed(5)
    rs = net.predictive_regression_score(x, torch.zeros(4, 3), samples=8, outputs="values", propagation="moments")
    assert all(torch.equal(a, b) for a, b in zip(rs, ops.regression_score_f64(ys, torch.zeros(4, 3), "values")[0]))
    # what this first version refuses
    with pytest.raises(ops.BnnHipError, match="NormalLinear / LocalReparamLinear"):
        Mlp([6, 5, 3]).predictive_moments(x)                        # the ReLU module was not folded
    with pytest.raises(ops.BnnHipError, match="KL"):
        net.predictive_mean(x, samples=2, kl=object(), propagation="moments")
    with pytest.raises(ValueError):
        net.predictive_uncertainty(x, inputs="logits", propagation="moment")
    net.layers[0].__dict__["_fuse_head"] = net.layers[2]           # what nn.fuse_activations(fuse_head=True) leaves behind
    with pytest.raises(ops.BnnHipError, match="fused head"):
        net.predictive_uncertainty(x, samples=2, inputs="logits", propagation="moments")
    del net.layers[0].__dict__["_fuse_head"]
    # a plain tensor comes back with var None
    class Plain(BayesianNetworkModule):
        def _forward(self, x):
            return 2 * x
    pm = Plain(6, 6).predictive_moments(x)
    assert pm.var is None and torch.equal(pm.mean, 2 * x)


def test_defaults_leave_the_sampling_paths_alone():
    """propagation defaults to 'samples': the same results and the same draw epochs as a call that omits the keyword."""
    torch.manual_seed(0)
    net = Mlp([6, 5, 3])
    x, t = torch.randn(4, 6), torch.tensor([0, 2, 1, 1])
    calls = [lambda **k: net.predictive_mean(x, 3, **k),
             lambda **k: net.predictive_uncertainty(x, 3, inputs="logits", **k),
             lambda **k: net.predictive_score(x, t, 3, inputs="logits", **k),
             lambda **k: net.predictive_regression(x, 3, outputs="values", **k),
             lambda **k: net.predictive_regression_score(x, torch.zeros(4, 3), 3, outputs="values", **k)]
    for call in calls:
        out = []
        for kw in ({}, {"propagation": "samples"}):
            torch.manual_seed(9)
            bnn.manual_seed(9)
            r = call(**kw)
            out.append(((r,) if torch.is_tensor(r) else tuple(r), _rng.default_generator.epoch_host))
        assert out[0][1] == out[1][1]
        assert all(torch.equal(a, b) for a, b in zip(out[0][0], out[1][0]))
    assert not hasattr(net, "moment_key")


def test_moment_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)
    fwd = lib.bnn_moments_forward
    assert fwd(None, None, 8, one, one, None, None, one, one, 4, 4, 8, 0, 0, None) == -1
    assert fwd(one, None, 8, one, one, one, None, one, one, 4, 4, 8, 0, 0, None) == -1           # mu_b without s2_b
    assert fwd(one, None, 8, one, one, None, None, one, None, 4, 4, 8, 0, 0, None) == -1          # no out_v
    assert fwd(one, None, 8, one, one, None, None, one, one, 4, 0, 8, 0, 0, None) == -2
    assert fwd(one, None, 4, one, one, None, None, one, one, 4, 4, 8, 0, 0, None) == -2           # lda < K
    assert fwd(one, None, 8, one, one, None, None, one, one, 64 * 65535 + 1, 4, 8, 0, 0, None) == -5
    assert fwd(one, None, 8, one, one, None, None, one, one, 4, 4, 8, 7, 0, None) == -3
    assert fwd(one, None, 8, one, one, None, None, one, one, 4, 4, 8, 0, _lib.FLAG_X_BF16, None) == -6          # bf16 a_m, fp32 mode
    assert fwd(one, one, 8, one, one, None, None, one, one, 4, 4, 8, 1, _lib.FLAG_X_BF16, None) == -6           # bf16 a_m beside a_v
    assert fwd(one, None, 8, one, one, None, None, one, one, 4, 4, 8, 0, _lib.FLAG_Y_BF16, None) == -6          # hidden moments are fp32
    assert fwd(one, None, 8, one, one, None, None, odd, one, 4, 4, 8, 0, 0, None) == -4
    assert fwd(one, odd, 8, one, one, None, None, one, one, 4, 4, 8, 0, 0, None) == -4
    assert fwd(one, None, 8, one, one, None, None, one, one, 0, 4, 8, 0, 0, None) == 0            # no rows: nothing to do
    relu = lib.bnn_moments_relu
    assert relu(one, None, one, one, 4, None) == -1
    assert relu(one, one, one, one, -1, None) == -2
    assert relu(one, one, odd, one, 4, None) == -4
    assert relu(one, one, one, one, 0, None) == 0
    r = _lib.Rng(seed=1, stream=5)
    rr = ctypes.byref(r)
    smp = lib.bnn_moments_sample
    assert smp(one, one, None, 4, 4, 1, rr, 0, None) == -1
    assert smp(one, one, one, 4, 4, 1, None, 0, None) == -1
    assert smp(one, one, one, 4, 0, 1, rr, 0, None) == -2
    assert smp(one, one, one, 4, 4, 0, rr, 0, None) == -2
    assert smp(one, one, one, 4, 4, 70000, rr, 0, None) == -5
    assert smp(one, one, one, 1 << 20, 1 << 12, 1, rr, 0, None) == -5
    assert b"2^32" in lib.bnn_last_error()
    bad = _lib.Rng(seed=1, stream=70000)
    assert smp(one, one, one, 4, 4, 1, ctypes.byref(bad), 0, None) == -5
    assert smp(one, one, one, 4, 4, 1, rr, _lib.FLAG_Y_BF16, None) == -6
    assert smp(one, one, odd, 4, 4, 1, rr, 0, None) == -4
    assert smp(one, one, one, 0, 4, 1, rr, 0, None) == 0
    assert lib.bnn_launch_count() == n0


def test_moment_kernels_do_not_spill():
    """Every instantiation of the three-contraction tile (bf16, fp32 x deterministic, Moments input) keeps both accumulator sets
    in registers, and the two elementwise kernels use no scratch either."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    tiles = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn9k_momentsI[tf]Lb[01]EEEvNS_7MomArgsE$", n)}
    assert len(tiles) == 4, sorted(kernels)
    rest = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn(14k_moments_relu|16k_moments_sampleILb[01]E)", n)}
    assert len(rest) == 3, sorted(kernels)
    for n, f in {**tiles, **rest}.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("private_segment_fixed_size", 0)) == 0, (n, f)


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


def linear_ref(mom, mu_w, rho_w, mu_b, rho_b, mode, dev):
    """float64 reference of ONE moments_linear call (no ReLU) with the bound on the device's deviation -> (m, v, bound_m, bound_v).
    mom: CPU Moments (fp32 values, the call's own input)."""
    am, av = mom.mean.double(), None if mom.var is None else mom.var.double()
    K = mu_w.shape[1]
    if mode == "f32":
        r = ops.moments_linear_f64(mom, mu_w, rho_w, mu_b, rho_b)
        return r.mean, r.var, scaled_bound(r.mean), scaled_bound(r.var)
    # bf16: the six planes as the loader rounds them; sigma^2 is the device's fp32 value (checked against float64)
    s2_w, s2_b = ops._lrt_prepare_raw(rho_w.to(dev), None if rho_b is None else rho_b.to(dev))
    s2_w = s2_w.cpu()
    assert ((s2_w.double() - sigma64(rho_w) ** 2).abs() <= 1e-6 * sigma64(rho_w) ** 2).all()
    p_mu, p_s2 = rne_bf16(mu_w), rne_bf16(s2_w)
    p_e2 = rne_bf16((mu_w.double() ** 2 + s2_w.double()).float())           # one fp32 fma, then bf16
    q_m, q_sq = rne_bf16(mom.mean), rne_bf16(mom.mean.float() * mom.mean.float())
    m = q_m @ p_mu.t()
    a = q_m.abs() @ p_mu.abs().t()
    v = q_sq @ p_s2.t()
    n_v = K
    if av is not None:
        v = v + rne_bf16(av) @ p_e2.t()
        n_v = 2 * K
    if mu_b is not None:
        s2_b = s2_b.cpu().double()
        m, a, v = m + mu_b.double(), a + mu_b.double().abs(), v + s2_b
    return m, v, gamma(K + 1) * a + 1e-300, gamma(n_v + 1) * v + 1e-300       # v is its own sum |a| |b|: every term is >= 0


def make_input(B, K, with_var, seed):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(B, K, generator=g)
    return ops.Moments(mean, 0.5 * torch.rand(B, K, generator=g) ** 2 if with_var else None)


SHAPES = [(3, 5, 7), (64, 64, 64), (65, 68, 130)]


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("with_var", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_contraction_matches_float64(dev, shape, with_var, bias, mode):
    B, N, K = shape
    p = params(N, K, bias, 11)
    mom = make_input(B, K, with_var, 12)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    a = ops.Moments(*to(dev, mom.mean, mom.var)) if with_var else mom.mean.to(dev)
    out = ops.moments_linear(a, *to(dev, *p), relu=False, compute=mode)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 2                    # the operand launch + ONE contraction launch
    assert out.mean.shape == (B, N) and out.mean.dtype == out.var.dtype == torch.float32
    m, v, bm, bv = linear_ref(mom, *p, mode, dev)
    what = "%s var=%s bias=%s %s" % (shape, with_var, bias, mode)
    assert_within(out.mean, m, bm, "m " + what)
    assert_within(out.var, v, bv, "v " + what)
    assert (out.var >= 0).all()
    again = ops.moments_linear(a, *to(dev, *p), relu=False, compute=mode)
    assert torch.equal(again.mean, out.mean) and torch.equal(again.var, out.var)
    if mode == "bf16" and not with_var:
        hb = ops.moments_linear(mom.mean.to(dev).bfloat16(), *to(dev, *p), relu=False, compute=mode)       # a bf16 input as it is
        mb, vb, bmb, bvb = linear_ref(ops.Moments(mom.mean.bfloat16().float()), *p, mode, dev)
        assert_within(hb.mean, mb, bmb, "m (bf16 input) " + what)
        assert_within(hb.var, vb, bvb, "v (bf16 input) " + what)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("with_var", [False, True])
def test_fused_relu_is_the_standalone_relu_bit_for_bit(dev, with_var, mode):
    B, N, K = 65, 68, 130
    p = to(dev, *params(N, K, True, 21))
    mom = make_input(B, K, with_var, 22)
    a = ops.Moments(*to(dev, mom.mean, mom.var)) if with_var else mom.mean.to(dev)
    pre = ops.moments_linear(a, *p, relu=False, compute=mode)
    fused = ops.moments_linear(a, *p, relu=True, compute=mode)
    alone = ops.moments_relu(pre)
    assert torch.equal(fused.mean, alone.mean) and torch.equal(fused.var, alone.var)
    assert not torch.equal(fused.mean, pre.mean)


def relu_deviation(got, m32, v32):
    """worst |device - float64| of moments_relu on fp32 inputs, in units of s (mean) and v (variance)"""
    ref = ops.moments_relu_f64(ops.Moments(m32, v32))
    s, v = v32.double().sqrt(), v32.double()
    return ((got.mean.double().cpu() - ref.mean).abs() / s).max().item(), ((got.var.double().cpu() - ref.var).abs() / v).max().item()


@gpu
def test_relu_matches_float64_on_a_grid(dev):
    """alpha in [-12, 12] at v = 1e-6, 0.3, 1, 47.  Measured on the MI355X: worst mean deviation 9.313e-7 s, worst variance
    deviation 1.887e-7 v (per v: 9.31e-7 / 1.89e-7, 8.71e-7 / 1.63e-7, 3.55e-7 / 1.31e-7, 5.56e-7 / 1.72e-7); the bounds
    RELU_MEAN_TOL = 3.73e-6 and RELU_VAR_TOL = 7.55e-7 are 4 x that (both <= 1e-5)."""
    alpha = torch.linspace(-12, 12, 4801, dtype=torch.float64)
    worst_m = worst_v = 0.0
    for v in (1e-6, 0.3, 1.0, 47.0):
        m32, v32 = (alpha * math.sqrt(v)).float(), torch.full_like(alpha, v).float()
        got = ops.moments_relu(ops.Moments(m32.to(dev), v32.to(dev)))
        assert (got.var >= 0).all() and (got.mean >= 0).all()
        dm, dv = relu_deviation(got, m32, v32)
        print("moments_relu v = %g: worst mean deviation %.3e s, worst variance deviation %.3e v" % (v, dm, dv))
        worst_m, worst_v = max(worst_m, dm), max(worst_v, dv)
    print("moments_relu: worst mean deviation %.3e s (bound %.1e), worst variance deviation %.3e v (bound %.1e)"
          % (worst_m, RELU_MEAN_TOL, worst_v, RELU_VAR_TOL))
    assert RELU_MEAN_TOL <= 1e-5 and RELU_VAR_TOL <= 1e-5
    assert worst_m <= RELU_MEAN_TOL and worst_v <= RELU_VAR_TOL
    # v == 0 and the far tails
    z = ops.moments_relu(ops.Moments(torch.tensor([-2.0, 0.0, 3.0, 1e30, -1e30], device=dev), torch.tensor([0.0, 0.0, 0.0, 1e-30, 1e-30], device=dev)))
    assert torch.equal(z.mean.cpu(), torch.tensor([0.0, 0.0, 3.0, 1e30, 0.0]))
    assert torch.equal(z.var.cpu(), torch.tensor([0.0, 0.0, 0.0, 1e-30, 0.0]))


@gpu
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", [5, 68])
@pytest.mark.parametrize("gen", [0, 1])
def test_sampling_matches_the_keys_cpu_twin(dev, gen, N, S):
    rows = 7
    g = torch.Generator().manual_seed(31)
    m, v = torch.randn(rows, N, generator=g), torch.rand(rows, N, generator=g) ** 2
    v[0, 0] = 0.0
    key = DrawKey(0x1234567890ABCDEF, 321, 3, S, 17, gen=gen)               # sample0 = 3
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    y = ops.moments_sample(ops.Moments(m.to(dev), v.to(dev)), key, S)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1 and y.shape == (S, rows, N)
    eps = twin_eps(key, S, (rows, N), dev)
    sd = torch.sqrt(v.double() + 1e-16)
    ref = m.double() + sd * eps
    assert_within(y, ref, scaled_bound(ref) + EPS_TWIN * sd, "moments_sample N=%d S=%d gen=%d" % (N, S, gen))
    assert torch.equal(ops.moments_sample(ops.Moments(m.to(dev), v.to(dev)), key, S), y)


def device_net(dev, layer=NormalLinear, seed=6):
    torch.manual_seed(seed)
    net = Mlp([20, 70, 66, 5])
    bnn.nn.fuse_activations(net)
    if layer is not NormalLinear:
        other = Mlp([20, 70, 66, 5], layer=layer, relu_module=False)
        other.load_state_dict(net.state_dict())
        for m in bayes_layers(other)[:-1]:
            m.activation = 'relu'
        net = other
    return net.to(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_network_pass(dev, mode):
    """20 -> 70 -> 66 -> 5, ReLU folded: predictive_moments is the chain of ops.moments_linear calls bit for bit; every layer is
    within its bound of float64 applied to the DEVICE's own input of that layer (the pre-activation against the contraction bound,
    the fused ReLU equal to moments_relu of it, and that within the ReLU bound of float64 on the device's pre-activation)."""
    bnn.set_compute(mode)
    net = device_net(dev)
    x = torch.randn(33, 20, device=dev)
    keys = [(m.weight.draw_key, m.bias.draw_key) for m in bayes_layers(net)]
    e0 = _rng.default_generator.epoch_host
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    mom = net.predictive_moments(x)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 6                    # per layer: the operand launch + ONE contraction launch
    assert _rng.default_generator.epoch_host == e0 and [(m.weight.draw_key, m.bias.draw_key) for m in bayes_layers(net)] == keys
    assert mom.mean.shape == (33, 5) and not mom.mean.requires_grad
    a = ops.Moments(x, None)
    for mu_w, rho_w, mu_b, rho_b, relu in layer_specs(net):
        cpu = ops.Moments(a.mean.cpu(), None if a.var is None else a.var.cpu())
        p = [t.detach() for t in (mu_w, rho_w, mu_b, rho_b)]
        pre = ops.moments_linear(a, *p, relu=False, compute=mode)
        m, v, bm, bv = linear_ref(cpu, *[t.cpu() for t in p], mode, dev)
        assert_within(pre.mean, m, bm, "layer %s m %s" % (tuple(mu_w.shape), mode))
        assert_within(pre.var, v, bv, "layer %s v %s" % (tuple(mu_w.shape), mode))
        nxt = ops.moments_linear(a, *p, relu=relu, compute=mode)
        if relu:
            alone = ops.moments_relu(pre)
            assert torch.equal(nxt.mean, alone.mean) and torch.equal(nxt.var, alone.var)
            dm, dv = relu_deviation(nxt, pre.mean.cpu(), pre.var.cpu())
            assert dm <= RELU_MEAN_TOL and dv <= RELU_VAR_TOL, (dm, dv)
        a = nxt
    assert torch.equal(a.mean, mom.mean) and torch.equal(a.var, mom.var)
    again = net.predictive_moments(x)
    assert torch.equal(again.mean, mom.mean) and torch.equal(again.var, mom.var)
    lrt = device_net(dev, LocalReparamLinear)
    got = lrt.predictive_moments(x)
    assert torch.equal(got.mean, mom.mean) and torch.equal(got.var, mom.var)
    assert all(m.noise_key is None for m in bayes_layers(lrt))
    with torch.enable_grad():
        assert not net.predictive_moments(x.clone().requires_grad_()).mean.requires_grad          # detached whatever the grad mode
    _lib.check_device(dev)


@gpu
def test_cost_does_not_grow_with_the_sample_count(dev):
    net = device_net(dev)
    x = torch.randn(33, 20, device=dev)
    lib = _lib.load()
    net.predictive_uncertainty(x, samples=2, inputs="logits", propagation="moments")        # takes the model's stream id
    counts = []
    for S in (2, 16):
        bnn.manual_seed(100)
        n0 = lib.bnn_launch_count()
        u = net.predictive_uncertainty(x, samples=S, sample0=1, inputs="logits", propagation="moments")
        torch.cuda.synchronize()
        counts.append(lib.bnn_launch_count() - n0)
        key = net.moment_key
        assert (key.stream, key.sample0, key.nsamples) == (net._moment_stream, 1, S)
        assert key.stream not in [m.weight._stream for m in bayes_layers(net)]
        want = ops.mc_uncertainty(ops.moments_sample(net.predictive_moments(x), key, S), "logits")
        assert all(torch.equal(a, b) for a, b in zip(u, want))
    assert counts[0] == counts[1] == 6 + 1 + 1                 # three layers, the sampling launch, the tail
    rv = net.predictive_regression(x, outputs="values", propagation="moments")
    mom = net.predictive_moments(x)
    assert torch.equal(rv.mean, mom.mean) and torch.equal(rv.total, mom.var) and not rv.aleatoric.any()


@gpu
def test_agrees_with_the_sampler_it_replaces(dev):
    """One hidden layer, fp32 mode, 8 rows: the logits of 2048 weight draws (forward_stacked, mc_batched) have sample mean and
    variance within 6 standard errors of predictive_moments -- exact for this depth."""
    torch.manual_seed(8)
    net = Mlp([20, 32, 5])
    bnn.nn.fuse_activations(net)
    with torch.no_grad():
        for m in bayes_layers(net):
            m.weight.scale.add_(1.5)                           # sigma ~ 0.2: a variance worth testing
    net = net.to(dev)
    net.mc_batched = True
    x = torch.randn(8, 20, device=dev)
    bnn.manual_seed(77)
    with torch.no_grad():
        ys = net.forward_stacked(x, 2048)
    assert ys.shape == (2048, 8, 5)
    mom = net.predictive_moments(x)
    six_se(ys.double().cpu(), mom.mean.double().cpu(), mom.var.double().cpu(), "2048 device weight draws")


@gpu
def test_graph_capture(dev):
    net = device_net(dev)
    x = torch.randn(33, 20, device=dev)
    bnn.manual_seed(3)
    net.predictive_uncertainty(x, samples=8, inputs="logits", propagation="moments")        # warm up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        u = net.predictive_uncertainty(x, samples=8, inputs="logits", propagation="moments")
    key = net.moment_key
    g.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in u]
    for t in u:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, u))
    want = ops.mc_uncertainty(ops.moments_sample(net.predictive_moments(x), key, 8), "logits")
    assert all(torch.equal(a, b) for a, b in zip(first, want))
    assert torch.isfinite(u.total).all() and (u.mean.sum(-1) - 1).abs().max() <= 1e-5
    _lib.check_device(dev)
