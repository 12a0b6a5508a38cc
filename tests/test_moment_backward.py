"""Training without sampling (K18, csrc/bnn_moments_bwd.hip): the backward of the dense moment layer

    g_a_m  = G_m mu_w + 2 a_m (.) (G_v sigma_w^2)        g_a_v  = G_v (mu_w^2 + sigma_w^2)
    g_mu_w = G_m^T a_m + 2 mu_w (.) (G_v^T a_v)          g_s2_w = G_v^T (a_m^2 + a_v),   g_rho_w = g_s2_w 2 sigma_w sigmoid(rho_w)

of the moment-matched ReLU and of the sampling launch, and BayesianNetworkModule.forward_moments / sample_moments on top of them.
CPU tests: the float64 path under torch autograd (gradcheck), the ReLU's analytic backward, the untouched inference surface, the
refusals, the built code object, the argument checks.  GPU tests: every kernel against float64, the network end to end, training.

Bounds.  Contractions, fp32 mode: 1e-5 of the output scale (test_lrt_device.scaled_bound).  bf16 mode: float64 on the five planes
as the kernel rounds them (RNE; the derived plane fma(p1, p1, p2) in fp32 first), so the device differs by its fp32 accumulation
alone: gamma_n sum |a| |b| per element with n the addends the element's accumulators see plus the epilogue fma -- 2 N + 2 for
g_a_m, N + 1 for g_a_v, 2 B + 2 for g_mu_w, B + 1 for g_s2_w -- and 16 U for the rho chain factor (sigma, sigmoid and three
products in fp32), as in test_lrt_device.backward64.  The bias sums read the fp32 G_m / G_v: gamma_B sum |G|.
ReLU backward: RELU_BWD_M_TOL / RELU_BWD_V_TOL below, 4 x the device's measured worst deviation from float64.
Sampling backward: K10's epilogue bound (test_lrt_device.test_backward_matches_float64_on_the_keys_eps) with an exact v.
"""
import ctypes
import math
import re

import pytest
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _rng, ops
from bayesianneuralnetworks_amd.nn import (BayesianNetworkModule, KLDivergence, LocalReparamLinear, MultivariateNormalLinear,
                                           NormalConv2d, NormalLinear)
from bayesianneuralnetworks_amd._rng import DrawKey

from bf16ref import gamma, rne_bf16
from test_flipout_mc import _code_object_notes
from test_lrt_device import EPS_TWIN, U, assert_within, make_params, scaled_bound, sigma64

gpu = pytest.mark.gpu

# The backward of the moment-matched ReLU against float64 (ops.moments_relu_backward_f64 on the fp32 inputs), g_m in units of
# |g_mean'| + s |g_var'| and g_v in units of |g_mean'| / s + |g_var'| (s = sqrt(v): the units in which the forward's test
# measures mean' and var').  Measured on the MI355X over alpha in [-12, 12] (4801 points) at v = 1e-6, 0.3, 1, 47
# (test_relu_backward_matches_float64_on_a_grid prints them): worst g_m deviation 1.019e-7 (at v = 47), worst g_v
# deviation 1.291e-7 (at v = 0.3).
# The constants are 4 x that, the margin of RELU_MEAN_TOL / ELU_*_TOL; both are below 1e-5, so the kernel evaluates in fp32.
RELU_BWD_M_TOL = 4.08e-7
RELU_BWD_V_TOL = 5.17e-7

GRID_V = (1e-6, 0.3, 1.0, 47.0)


class Net(BayesianNetworkModule):
    """widths[0] -> ... -> widths[-1], a ReLU behind every layer but the last: folded into the layer (activation = 'relu') or
    the nn.MomentReLU twin that nn.moment_activations puts in place of torch.nn.ReLU."""

    def __init__(self, widths, twins, layer=NormalLinear, samples=4):
        super().__init__(widths[0], widths[-1], samples=samples)
        mods = []
        for i, (k, n) in enumerate(zip(widths[:-1], widths[1:])):
            mods.append(layer(k, n))
            if i < len(widths) - 2:
                mods.append(torch.nn.ReLU())
        self.layers = torch.nn.Sequential(*mods)
        if twins:
            bnn.nn.moment_activations(self)
        else:
            bnn.nn.fuse_activations(self)

    def _forward(self, x):
        return self.layers(x)


def bayes(net):
    return [m for m in net.layers if isinstance(m, (NormalLinear, LocalReparamLinear))]


def set_params(net, seed, rho0=-2.0):
    """Posteriors with variances of a healthy size, so that every output's standard deviation is within a few orders of its mean."""
    ls = bayes(net)
    with torch.no_grad():
        for i, m in enumerate(ls):
            N, K = m.weight.mean.shape
            g = torch.Generator().manual_seed(seed + i)
            m.weight.mean.copy_((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5)
            m.weight.scale.copy_(rho0 + 0.3 * torch.randn(N, K, generator=g))
            m.bias.mean.copy_((torch.rand(N, generator=g) * 2 - 1) / K ** 0.5)
            m.bias.scale.copy_(rho0 + 0.3 * torch.randn(N, generator=g))
    return net


def leaves(net):
    return [p for m in bayes(net) for p in (m.weight.mean, m.weight.scale, m.bias.mean, m.bias.scale)]


def specs(tensors, nlayers):
    """[(mu_w, rho_w, mu_b, rho_b, relu)] for ops.moments_f64 from the flat list of leaves()."""
    return [tuple(tensors[4 * i:4 * i + 4]) + (i < nlayers - 1,) for i in range(nlayers)]


# ================================================================================================ CPU
@pytest.mark.parametrize("twins", [False, True], ids=["folded", "twins"])
def test_forward_moments_cpu_gradcheck(twins):
    """6 -> 5 -> 3 in float64: forward_moments is attached to the input and to every mu / rho, and its gradient is the finite
    difference's (gradcheck perturbs the parameters in place, so the network reads the perturbed values)."""
    torch.manual_seed(3)
    net = set_params(Net([6, 5, 3], twins), 40).double()
    assert isinstance(net.layers[1], bnn.nn.MomentReLU) == twins
    x = torch.randn(4, 6, dtype=torch.float64, requires_grad=True)
    g = torch.Generator().manual_seed(4)
    c1, c2 = torch.randn(4, 3, generator=g, dtype=torch.float64), torch.randn(4, 3, generator=g, dtype=torch.float64)
    ps = leaves(net)

    def f(x, *_):
        mom = net.forward_moments(x)
        assert isinstance(mom, ops.Moments) and mom.mean.requires_grad and mom.var.requires_grad and mom.mean.dtype == torch.float64
        return (c1 * mom.mean + c2 * mom.var).sum()

    assert torch.autograd.gradcheck(f, (x, *ps), eps=1e-6, atol=1e-7, rtol=1e-5)
    # the tracked pass computes what the inference pass computes
    mom, ref = net.forward_moments(x), net.predictive_moments(x)
    assert torch.equal(mom.mean.float(), ref.mean) and torch.equal(mom.var.float(), ref.var)
    # sampled outputs are differentiable in the moments, and no key is recorded on the CPU
    ys = net.sample_moments(mom, 5)
    assert ys.shape == (5, 4, 3) and ys.requires_grad and not hasattr(net, "moment_key")
    assert all(t is not None for t in torch.autograd.grad(ys.sum(), ps))
    with torch.no_grad():
        assert not net.forward_moments(x).mean.requires_grad


def relu_grid(v, n=4801):
    alpha = torch.linspace(-12, 12, n, dtype=torch.float64)
    m32, v32 = (alpha * math.sqrt(v)).float(), torch.full_like(alpha, v).float()
    g = torch.Generator().manual_seed(int(v * 1000) + 5)
    return m32, v32, torch.randn(n, generator=g), torch.randn(n, generator=g)


def test_relu_backward_formula_is_the_autograd_of_the_forward():
    for v in GRID_V:
        m32, v32, gm, gv = relu_grid(v)
        m, vv = m32.double().requires_grad_(), v32.double().requires_grad_()
        out = ops.moments_relu_f64(ops.Moments(m, vv), track=True)
        assert out.mean.requires_grad
        want = torch.autograd.grad([out.mean, out.var], [m, vv], [gm.double(), gv.double()])
        got = ops.moments_relu_backward_f64(ops.Moments(m32, v32), gm, gv)
        s = math.sqrt(v)
        assert ((got[0] - want[0]).abs() <= 1e-12 * (gm.abs() + s * gv.abs())).all(), v
        assert ((got[1] - want[1]).abs() <= 1e-12 * (gm.abs() / s + gv.abs())).all(), v
        assert not got[0].requires_grad
    # v == 0: both gradients pass where m > 0 (the formula, and the tracked forward's autograd)
    m0, v0 = torch.tensor([-2.0, 0.0, 3.0], dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    gm, gv = torch.tensor([1.5, -2.0, 0.5]), torch.tensor([4.0, 3.0, -7.0])
    g_m, g_v = ops.moments_relu_backward_f64(ops.Moments(m0, v0), gm, gv)
    assert torch.equal(g_m, torch.tensor([0.0, 0.0, 0.5], dtype=torch.float64))
    assert torch.equal(g_v, torch.tensor([0.0, 0.0, -7.0], dtype=torch.float64))
    m, vv = m0.clone().requires_grad_(), v0.clone().requires_grad_()
    out = ops.moments_relu_f64(ops.Moments(m, vv), track=True)
    assert torch.equal(out.mean.detach(), torch.tensor([0.0, 0.0, 3.0], dtype=torch.float64)) and not out.var.detach().any()
    a_m, a_v = torch.autograd.grad([out.mean, out.var], [m, vv], [gm.double(), gv.double()])
    assert torch.equal(a_m, g_m) and torch.equal(a_v, g_v)
    # where the forward clamped var' to 0 the g_var' terms are absent: far in the lower tail (Phi and phi subnormal in float64)
    # the bracket of var' rounds below 0 at thousands of these points
    al = torch.linspace(-38.8, -37.9, 9001, dtype=torch.float64)
    one = torch.ones_like(al)
    fwd = ops.moments_relu_f64(ops.Moments(al, one))
    cdf, cdc = 0.5 * torch.special.erfc(-al / math.sqrt(2.0)), 0.5 * torch.special.erfc(al / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * al * al) / math.sqrt(2.0 * math.pi)
    clamped = cdf + al * al * cdf * cdc + al * pdf * (cdc - cdf) - pdf * pdf < 0
    assert clamped.any() and not fwd.var[clamped].any()
    g_m, g_v = ops.moments_relu_backward_f64(ops.Moments(al, one), torch.zeros_like(al), one)
    assert not g_m[clamped].any() and not g_v[clamped].any()
    # a deterministic input is plain ReLU
    g_m, g_v = ops.moments_relu_backward_f64(ops.Moments(torch.tensor([-1.0, 2.0])), torch.tensor([3.0, 4.0]), None)
    assert g_v is None and torch.equal(g_m, torch.tensor([0.0, 4.0], dtype=torch.float64))


def test_untracked_calls_stay_detached_under_enable_grad():
    torch.manual_seed(0)
    net = set_params(Net([6, 5, 3], False), 50)
    x = torch.randn(4, 6, requires_grad=True)
    p = [t for t in leaves(net)]
    assert all(t.requires_grad for t in p)
    with torch.enable_grad():
        mom = net.predictive_moments(x)
        assert not mom.mean.requires_grad and not mom.var.requires_grad
        lin = ops.moments_linear_f64(x, *p[:4], relu=True)
        assert not lin.mean.requires_grad and not lin.var.requires_grad
        act = ops.moments_relu_f64(ops.Moments(x, x * x))
        assert not act.mean.requires_grad and not act.var.requires_grad
        chain = ops.moments_f64(x, specs(p, 2))
        assert not chain.mean.requires_grad and not chain.var.requires_grad
        assert not ops.moments_sample(ops.Moments(x, x * x), None, 3).requires_grad
        assert ops.moments_sample(ops.Moments(x, x * x), None, 3, track=True).requires_grad
        assert ops.moments_f64(x, specs(p, 2), track=True).var.requires_grad
    with torch.no_grad():                       # track asks for the graph; without grad mode there is none
        assert not ops.moments_f64(x, specs(p, 2), track=True).mean.requires_grad


def test_forward_moments_refuses_what_has_no_backward():
    class Conv(BayesianNetworkModule):
        def __init__(self):
            super().__init__(1, 2)
            self.conv = NormalConv2d(1, 2, 3)

        def _forward(self, x):
            return self.conv(x)

    with pytest.raises(ops.BnnHipError, match="NormalConv2d"):
        Conv().forward_moments(torch.randn(2, 1, 5, 5))

    elu = Net([6, 5, 3], True)
    elu.layers[1] = bnn.nn.MomentELU()
    with pytest.raises(ops.BnnHipError, match="MomentELU"):
        elu.forward_moments(torch.randn(2, 6))
    mvn = Net([6, 5, 3], True, layer=NormalLinear)
    mvn.layers[2] = MultivariateNormalLinear(5, 3)
    with pytest.raises(ops.BnnHipError, match="MultivariateNormalLinear"):
        mvn.forward_moments(torch.randn(2, 6))
    with pytest.raises(TypeError):
        mvn.sample_moments(torch.randn(2, 3))


def test_forward_moments_admitted_modules():
    """A deterministic Linear in front of the first Bayesian layer, Flatten, Identity, a LocalReparamLinear, a ReLU twin and a
    closing Softmax twin: the moments carry link='softmax', sample_moments applies it, and the gradient reaches every parameter
    (the deterministic front included)."""
    class Mixed(BayesianNetworkModule):
        def __init__(self):
            super().__init__(8, 3, samples=4)
            self.front = torch.nn.Linear(8, 6)
            self.layers = torch.nn.Sequential(torch.nn.Flatten(), NormalLinear(6, 5), torch.nn.ReLU(), torch.nn.Identity(),
                                              LocalReparamLinear(5, 3), torch.nn.Softmax(dim=-1))

        def _forward(self, x):
            return self.layers(torch.tanh(self.front(x)))

    torch.manual_seed(2)
    net = Mixed()
    bnn.nn.moment_activations(net)
    assert isinstance(net.layers[2], bnn.nn.MomentReLU) and isinstance(net.layers[5], bnn.nn.MomentSoftmax)
    assert type(net.front) is torch.nn.Linear
    x = torch.randn(4, 8)
    mom = net.forward_moments(x)
    assert mom.link == 'softmax' and mom.mean.shape == (4, 3) and mom.var.requires_grad
    ref = net.predictive_moments(x)
    assert ref.link == 'softmax' and torch.equal(mom.mean.float(), ref.mean) and torch.equal(mom.var.float(), ref.var)
    ps = net.sample_moments(mom)
    assert ps.shape == (4, 4, 3) and (ps.sum(-1) - 1).abs().max() <= 1e-6 and ps.requires_grad
    t = torch.tensor([0, 2, 1, 1]).repeat(4)
    grads = torch.autograd.grad(F.nll_loss(torch.log(ps.reshape(-1, 3)), t), list(net.parameters()))
    assert len(grads) == 10 and all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads)


def test_moment_backward_kernels_do_not_spill():
    """The four instantiations of the three-accumulator tile (input, weight gradient x bf16, fp32) keep their 48 accumulator
    registers and the staged operands in registers, and the ReLU's backward uses no scratch either."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    tiles = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn13k_moments_bwdI[tf]Li[01]EEEvNS_10MomBwdArgsE$", n)}
    assert len(tiles) == 4, sorted(kernels)
    rest = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn18k_moments_relu_bwdE", n)}
    assert len(rest) == 1, sorted(kernels)
    for n, f in {**tiles, **rest}.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("private_segment_fixed_size", 0)) == 0, (n, f)


def test_moment_backward_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)
    inp = lib.bnn_moments_backward_input
    assert inp(None, one, one, one, one, 8, one, one, 4, 4, 8, 0, 0, None) == -1
    assert inp(one, one, one, one, one, 8, one, None, 4, 4, 8, 0, 0, None) == -1                 # no g_a_v
    assert inp(one, one, one, one, one, 8, one, one, 4, 0, 8, 0, 0, None) == -2
    assert inp(one, one, one, one, one, 4, one, one, 4, 4, 8, 0, 0, None) == -2                  # lda < K
    assert inp(one, one, one, one, one, 8, one, one, 64 * 65535 + 1, 4, 8, 0, 0, None) == -5
    assert inp(one, one, one, one, one, 8, one, one, 4, 4, 8, 7, 0, None) == -3
    assert inp(one, one, one, one, one, 8, one, one, 4, 4, 8, 1, _lib.FLAG_X_BF16, None) == -6   # a_m is fp32 here
    assert inp(one, one, one, one, one, 8, one, one, 4, 4, 8, 0, _lib.FLAG_RELU, None) == -6
    assert inp(one, one, one, one, one, 8, odd, one, 4, 4, 8, 0, 0, None) == -4
    assert inp(one, odd, one, one, one, 8, one, one, 4, 4, 8, 0, 0, None) == -4
    assert inp(one, one, one, one, one, 8, one, one, 0, 4, 8, 0, 0, None) == 0                   # no rows: nothing to do
    wgt = lib.bnn_moments_backward_weight
    assert wgt(one, None, 8, one, one, one, one, one, one, None, None, None, 4, 4, 8, 0, 0, None) == -1        # no a_v: K10's entry
    assert wgt(one, one, 8, one, one, one, one, one, None, None, None, None, 4, 4, 8, 0, 0, None) == -1
    assert wgt(one, one, 8, one, one, one, one, one, one, one, one, None, 4, 4, 8, 0, 0, None) == -1           # partial bias
    assert wgt(one, one, 8, one, one, one, one, one, one, None, None, None, 4, 4, 0, 0, 0, None) == -2
    assert wgt(one, one, 4, one, one, one, one, one, one, None, None, None, 4, 4, 8, 0, 0, None) == -2         # lda < K
    assert wgt(one, one, 8, one, one, one, one, one, one, None, None, None, 64 * 65535 + 1, 4, 8, 0, 0, None) == -5
    assert wgt(one, one, 8, one, one, one, one, one, one, None, None, None, 4, 4, 8, 5, 0, None) == -3
    assert wgt(one, one, 8, one, one, one, one, one, one, None, None, None, 4, 4, 8, 0, _lib.FLAG_X_BF16, None) == -6
    assert wgt(one, one, 8, one, one, one, one, one, odd, None, None, None, 4, 4, 8, 0, 0, None) == -4
    assert wgt(one, one, 8, one, one, one, one, one, one, odd, one, one, 4, 4, 8, 0, 0, None) == -4
    rb = lib.bnn_moments_relu_backward
    assert rb(one, one, one, None, one, one, 4, None) == -1
    assert rb(one, one, one, one, one, one, -1, None) == -2
    assert rb(one, one, one, one, odd, one, 4, None) == -4
    assert rb(one, one, one, one, one, one, 0, None) == 0
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


def to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


BWD_SHAPES = [(33, 100, 7), (64, 96, 64), (130, 72, 70), (70, 1200, 10)]         # (B, K, N)


def contraction_case(B, K, N, bias):
    mu_w, rho_w, mu_b, rho_b = make_params(N, K, bias, 61)
    g = torch.Generator().manual_seed(62)
    a_m = torch.randn(B, K, generator=g)
    a_v = 0.5 * torch.rand(B, K, generator=g) ** 2
    a_v[a_v < 0.02] = 0.0                                       # a fifth of the variances are exact zeros
    a_v[B // 2] = 0.0                                           # and one whole row
    return a_m, a_v, torch.randn(B, N, generator=g), torch.randn(B, N, generator=g), mu_w, rho_w, rho_b


def contraction_device(dev, mode, a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b):
    """The two entries called as they are -> [g_a_m, g_a_v, g_mu_w, g_rho_w (, g_mu_b, g_rho_b)] and the device's fp32 sigma_w^2."""
    lib, p, st = _lib.load(), ops.ptr, ops.stream_ptr(dev)
    code = ops._compute_code(mode)
    B, K = a_m.shape
    N = mu_w.shape[0]
    s2_w, _ = ops._lrt_prepare_raw(rho_w, None)
    g_am, g_av = torch.empty_like(a_m), torch.empty_like(a_v)
    g_mu, g_rho = torch.empty_like(mu_w), torch.empty_like(rho_w)
    g_mb = None if rho_b is None else torch.empty_like(rho_b)
    g_rb = None if rho_b is None else torch.empty_like(rho_b)
    n0 = lib.bnn_launch_count()
    ops.check(lib.bnn_moments_backward_input(p(G_m), p(G_v), p(mu_w), p(s2_w), p(a_m), K, p(g_am), p(g_av), B, N, K, code, 0, st),
              "bnn_moments_backward_input")
    ops.check(lib.bnn_moments_backward_weight(p(a_m), p(a_v), K, p(G_m), p(G_v), p(mu_w), p(rho_w), p(g_mu), p(g_rho), p(rho_b), p(g_mb),
                                              p(g_rb), B, N, K, code, 0, st), "bnn_moments_backward_weight")
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + (2 if rho_b is None else 3)           # one launch per gradient pair + the bias sums
    return [g_am, g_av, g_mu, g_rho] + ([] if rho_b is None else [g_mb, g_rb]), s2_w


def contraction_reference(mode, a_m, a_v, G_m, G_v, mu_w, rho_w, rho_b, s2_dev):
    """-> [(name, float64 reference, bound)] in contraction_device's order (CPU tensors; s2_dev the device's fp32 sigma_w^2)."""
    B, N = G_m.shape
    d = lambda t: t.double()         # noqa: E731
    c_w = 2 * sigma64(rho_w) * torch.sigmoid(d(rho_w))
    c_b = None if rho_b is None else 2 * sigma64(rho_b) * torch.sigmoid(d(rho_b))
    if mode == "f32":
        s2 = sigma64(rho_w) ** 2
        assert ((d(s2_dev) - s2).abs() <= 1e-6 * s2).all()
        refs = [("g_a_m", d(G_m) @ d(mu_w) + 2 * d(a_m) * (d(G_v) @ s2)),
                ("g_a_v", d(G_v) @ (d(mu_w) ** 2 + s2)),
                ("g_mu_w", d(G_m).t() @ d(a_m) + 2 * d(mu_w) * (d(G_v).t() @ d(a_v))),
                ("g_rho_w", (d(G_v).t() @ (d(a_m) ** 2 + d(a_v))) * c_w)]
        if rho_b is not None:
            refs += [("g_mu_b", d(G_m).sum(0)), ("g_rho_b", d(G_v).sum(0) * c_b)]
        return [(n, r, scaled_bound(r)) for n, r in refs]
    # bf16: the planes as the loader rounds them; the derived plane is one fp32 fma first
    qm, qv = rne_bf16(G_m), rne_bf16(G_v)
    p0, p1, p2 = rne_bf16(mu_w), rne_bf16(s2_dev), rne_bf16((d(mu_w) ** 2 + d(s2_dev)).float())
    r0, r1, r2 = rne_bf16(a_m), rne_bf16(a_v), rne_bf16((d(a_m) ** 2 + d(a_v)).float())
    tiny = 1e-300
    out = [("g_a_m", qm @ p0 + 2 * d(a_m) * (qv @ p1),
            gamma(2 * N + 2) * (qm.abs() @ p0.abs() + 2 * d(a_m).abs() * (qv.abs() @ p1.abs())) + tiny),
           ("g_a_v", qv @ p2, gamma(N + 1) * (qv.abs() @ p2.abs()) + tiny),
           ("g_mu_w", qm.t() @ r0 + 2 * d(mu_w) * (qv.t() @ r1),
            gamma(2 * B + 2) * (qm.abs().t() @ r0.abs() + 2 * d(mu_w).abs() * (qv.abs().t() @ r1.abs())) + tiny)]
    t = qv.t() @ r2
    out.append(("g_rho_w", t * c_w, gamma(B + 1) * (qv.abs().t() @ r2.abs()) * c_w + 16 * U * (t * c_w).abs() + tiny))
    if rho_b is not None:
        out.append(("g_mu_b", d(G_m).sum(0), gamma(B) * d(G_m).abs().sum(0) + tiny))
        tb = d(G_v).sum(0)
        out.append(("g_rho_b", tb * c_b, gamma(B) * d(G_v).abs().sum(0) * c_b + 16 * U * (tb * c_b).abs() + tiny))
    return out


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_contraction_backward_matches_float64(dev, shape, bias, mode):
    B, K, N = shape
    case = contraction_case(B, K, N, bias)
    on_dev = to(dev, *case)
    got, s2_dev = contraction_device(dev, mode, *on_dev)
    want = contraction_reference(mode, *case, s2_dev.cpu())
    for a, (name, ref, bound) in zip(got, want):
        assert_within(a, ref, bound, "%s %s bias=%s %s" % (name, shape, bias, mode))
    again, _ = contraction_device(dev, mode, *on_dev)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def off16(t):
    """the same values one element past a fresh allocation: on its element, off every 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_inputs_off_16_bytes_give_the_same_bits(dev, mode):
    """Every input of the three entries may lie on its element (lrt_fetch loads one element; the ReLU is elementwise): the
    same bits as on 16 bytes.  (The contraction outputs must be 16-byte aligned: the argument-error test; ops allocates them.)"""
    case = to(dev, *contraction_case(33, 100, 7, True))
    want, _ = contraction_device(dev, mode, *case)
    got, _ = contraction_device(dev, mode, *[off16(t) for t in case])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    if mode == "f32":
        lib, p = _lib.load(), ops.ptr
        m32, v32, gm, gv = to(dev, *relu_grid(0.3, 1001))
        outs = []
        for f in (lambda t: t, off16):
            g_m, g_v = off16(torch.empty_like(m32)), off16(torch.empty_like(m32))
            a = [f(t) for t in (m32, v32, gm, gv)]                  # (held until the launch has run)
            ops.check(lib.bnn_moments_relu_backward(p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(g_m), p(g_v), m32.numel(),
                                                    ops.stream_ptr(dev)), "bnn_moments_relu_backward")
            torch.cuda.synchronize()
            outs.append((g_m.clone(), g_v.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def relu_bwd_deviation(g_m, g_v, m32, v32, gm, gv):
    """worst |device - float64| of the ReLU's backward on fp32 inputs, in the units stated at RELU_BWD_M_TOL"""
    want = ops.moments_relu_backward_f64(ops.Moments(m32, v32), gm, gv)
    s = v32.double().sqrt()
    dm = ((g_m.double().cpu() - want[0]).abs() / (gm.double().abs() + s * gv.double().abs())).max().item()
    dv = ((g_v.double().cpu() - want[1]).abs() / (gm.double().abs() / s + gv.double().abs())).max().item()
    return dm, dv


@gpu
def test_relu_backward_matches_float64_on_a_grid(dev):
    """alpha in [-12, 12] at v = 1e-6, 0.3, 1, 47, random output gradients.  Measured on the MI355X: worst g_m deviation
    1.019e-7, worst g_v deviation 1.291e-7 in the stated units (per v: 8.95e-8 / 4.08e-8, 8.21e-8 / 1.29e-7, 7.25e-8 / 1.11e-7,
    1.02e-7 / 1.17e-7); RELU_BWD_M_TOL = 4.08e-7 and RELU_BWD_V_TOL = 5.17e-7 are 4 x that (both <= 1e-5: fp32 evaluation on the
    forward's terms is enough)."""
    worst_m = worst_v = 0.0
    for v in GRID_V:
        m32, v32, gm, gv = relu_grid(v)
        m, vv = m32.to(dev).requires_grad_(), v32.to(dev).requires_grad_()
        out = ops.moments_relu(ops.Moments(m, vv), track=True)
        plain = ops.moments_relu(ops.Moments(m, vv))
        assert torch.equal(out.mean, plain.mean) and torch.equal(out.var, plain.var) and not plain.mean.requires_grad
        g_m, g_v = torch.autograd.grad([out.mean, out.var], [m, vv], [gm.to(dev), gv.to(dev)])
        assert torch.isfinite(g_m).all() and torch.isfinite(g_v).all()
        dm, dv = relu_bwd_deviation(g_m, g_v, m32, v32, gm, gv)
        print("moments_relu backward v = %g: worst g_m deviation %.3e, worst g_v deviation %.3e" % (v, dm, dv))
        worst_m, worst_v = max(worst_m, dm), max(worst_v, dv)
    print("moments_relu backward: worst g_m deviation %.3e (bound %.2e), worst g_v deviation %.3e (bound %.2e)"
          % (worst_m, RELU_BWD_M_TOL, worst_v, RELU_BWD_V_TOL))
    assert RELU_BWD_M_TOL <= 1e-5 and RELU_BWD_V_TOL <= 1e-5
    assert worst_m <= RELU_BWD_M_TOL and worst_v <= RELU_BWD_V_TOL
    # v == 0 and the far tails: both gradients pass where m > 0
    m = torch.tensor([-2.0, 0.0, 3.0, 1e30, -1e30], device=dev, requires_grad=True)
    vv = torch.tensor([0.0, 0.0, 0.0, 1e-30, 1e-30], device=dev, requires_grad=True)
    gm, gv = torch.tensor([1.5, -2.0, 0.5, 0.25, 8.0], device=dev), torch.tensor([4.0, 3.0, -7.0, 2.0, 9.0], device=dev)
    out = ops.moments_relu(ops.Moments(m, vv), track=True)
    g_m, g_v = torch.autograd.grad([out.mean, out.var], [m, vv], [gm, gv])
    assert torch.equal(g_m.cpu(), torch.tensor([0.0, 0.0, 0.5, 0.25, 0.0])) and torch.equal(g_v.cpu(), torch.tensor([0.0, 0.0, -7.0, 2.0, 0.0]))


def recovered_eps(y, m, v):
    """eps_s = (y_s - m) / sqrt(v + 1e-16) from the sampling launch's own output, float64 on the CPU"""
    return (y.detach().double().cpu() - m.detach().double().cpu()) / torch.sqrt(v.detach().double().cpu() + 1e-16)


@gpu
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("shape", [(5, 10), (33, 7)], ids=lambda s: "x".join(map(str, s)))
def test_sampling_backward_matches_float64_on_the_recovered_eps(dev, shape, S):
    """g_m = sum_s gy_s and g_v = sum_s gy_s eps_s / (2 sqrt(v + 1e-16)) with eps recovered from the forward's output.  The
    variances lie in [0.25, 1.25] and the means are O(1), so the recovery is sound: eps is recovered to U |y| / sd + 3 U |eps|,
    orders below the 2e-5 (EPS_TWIN) the epilogue bound allows the device's eps."""
    g = torch.Generator().manual_seed(71)
    m, v = torch.randn(shape, generator=g), 0.25 + torch.rand(shape, generator=g)
    gy = torch.randn((S,) + shape, generator=g)
    key = DrawKey(0x1234567890ABCDEF, 321, 3, S, 17, gen=_rng.generator_for("f32"))          # sample0 = 3
    md, vd = m.to(dev).requires_grad_(), v.to(dev).requires_grad_()
    lib = _lib.load()
    y = ops.moments_sample(ops.Moments(md, vd), key, S, track=True)
    assert y.requires_grad and torch.equal(y, ops.moments_sample(ops.Moments(md, vd), key, S)) and y.shape == (S,) + shape
    n0 = lib.bnn_launch_count()
    g_m, g_v = torch.autograd.grad(y, [md, vd], gy.to(dev))
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1                     # K10's noise launch, no new kernel
    eps, gy64, v64 = recovered_eps(y, md, vd), gy.double(), v.double()
    assert eps.abs().max() < 7
    inv = 0.5 / torch.sqrt(v64 + 1e-16)
    term = gy64.abs() * inv * (eps.abs() * (4 * U + 3 * U) + EPS_TWIN)         # v is exact: rel_inv = 4 U (+ 1e-16 and sqrt round)
    beta_m = gamma(S) * gy64.abs().sum(0) + 1e-300
    beta_v = 1.01 * (term.sum(0) + gamma(S) * (gy64 * eps).abs().sum(0) * inv)
    assert_within(g_m, gy64.sum(0), beta_m, "sample g_m %s S=%d" % (shape, S))
    assert_within(g_v, (gy64 * eps).sum(0) * inv, beta_v, "sample g_v %s S=%d" % (shape, S))


# End to end against float64 autograd of the CPU recursion.  The device result passes through a chain of stages, each within
# its own bound of float64 on its own inputs: 3 forward contractions and 2 ReLUs, the sampling launch, softmax / cross-entropy
# (torch), the sampling backward, 3 backward contractions and 2 ReLU backwards -- 13 stages.
# fp32 mode: every stage is within 1e-5 of its output's scale (the project's parity rule; the ReLU bounds are below it), so to
# first order, with every stage carrying the errors it receives at no more than the scale it carries its signal, the gradients
# are within 13 x 1e-5 of theirs.
# bf16 mode: the 6 contractions read operands rounded to bf16 (relative 2^-9 each, 2^-8 per product), so against float64 on the
# UNROUNDED operands a contraction is within 2^-8 sum |a| |b|, and sum |a| |b| <= sqrt(n) (the scale of the sum) for the n <= 33
# addends of this network's widest contraction (Cauchy-Schwarz on the rms): 6 x 2^-8 x sqrt(33), plus the fp32 stages' 13 x 1e-5.
E2E_TOL = {"f32": 13 * 1e-5, "bf16": 6 * 2.0 ** -8 * math.sqrt(33.0) + 13 * 1e-5}


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("twins", [False, True], ids=["folded", "twins"])
def test_network_gradients_end_to_end(dev, twins, mode):
    """20 -> 33 -> 17 -> 5 at B = 9: forward_moments is predictive_moments bit for bit; the gradients of
    cross_entropy(sample_moments(mom, 8)) (summed over the 72 rows) with respect to the input and all twelve posterior tensors
    match float64 autograd of ops.moments_f64 fed the eps recovered from the device's samples, within E2E_TOL of each gradient's
    scale; a second run on the same key gives the same bits."""
    bnn.set_compute(mode)
    torch.manual_seed(8)
    net = set_params(Net([20, 33, 17, 5], twins), 80).to(dev)
    g = torch.Generator().manual_seed(81)
    x, t = torch.randn(9, 20, generator=g), torch.randint(0, 5, (9,), generator=g)
    xd = x.to(dev).requires_grad_()
    ps = leaves(net)
    S = 8

    def run(key=None):
        mom = net.forward_moments(xd)
        ys = net.sample_moments(mom, S) if key is None else ops.moments_sample(mom, key, S, track=True)
        loss = F.cross_entropy(ys.reshape(-1, 5), t.to(dev).repeat(S), reduction="sum")
        return mom, ys, torch.autograd.grad(loss, [xd] + ps)

    mom, ys, got = run()
    ref = net.predictive_moments(xd)
    assert torch.equal(mom.mean, ref.mean) and torch.equal(mom.var, ref.var) and mom.mean.requires_grad
    key = net.moment_key
    assert (key.nsamples, key.sample0, key.stream) == (S, 0, net._moment_stream)
    _, ys2, again = run(key)
    assert torch.equal(ys, ys2) and all(torch.equal(a, b) for a, b in zip(got, again))
    # float64 autograd of the CPU recursion on the device's eps
    eps = recovered_eps(ys, mom.mean, mom.var)
    x64 = x.double().requires_grad_()
    p64 = [p.detach().double().cpu().requires_grad_() for p in ps]
    m64 = ops.moments_f64(x64, specs(p64, 3), track=True)
    y64 = m64.mean + torch.sqrt(m64.var + 1e-16) * eps
    want = torch.autograd.grad(F.cross_entropy(y64.reshape(-1, 5), t.repeat(S), reduction="sum"), [x64] + p64)
    names = ["x"] + ["layer %d %s" % (i, n) for i in range(3) for n in ("weight.mean", "weight.scale", "bias.mean", "bias.scale")]
    for n, a, w in zip(names, got, want):
        assert_within(a, w, scaled_bound(w, E2E_TOL[mode]), "%s %s %s" % (n, "twins" if twins else "folded", mode))


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_first_layer_takes_k10s_backward_bit_for_bit(dev, mode):
    """A deterministic input: the tracked layer's five gradients are bnn_lrt_backward_input / _weight called on the same G."""
    B, K, N = 33, 100, 7
    mu_w, rho_w, mu_b, rho_b = [t.to(dev).requires_grad_() for t in make_params(N, K, True, 91)]
    g = torch.Generator().manual_seed(92)
    x = torch.randn(B, K, generator=g).to(dev).requires_grad_()
    G_m, G_v = torch.randn(B, N, generator=g).to(dev), torch.randn(B, N, generator=g).to(dev)
    out = ops.moments_linear(x, mu_w, rho_w, mu_b, rho_b, compute=mode, track=True)
    plain = ops.moments_linear(x, mu_w, rho_w, mu_b, rho_b, compute=mode)
    assert torch.equal(out.mean, plain.mean) and torch.equal(out.var, plain.var) and not plain.var.requires_grad
    lib, p, st = _lib.load(), ops.ptr, ops.stream_ptr(dev)
    n0 = lib.bnn_launch_count()
    got = torch.autograd.grad([out.mean, out.var], [x, mu_w, rho_w, mu_b, rho_b], [G_m, G_v])
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 3                     # K10's input gradient, weight gradient and bias sums
    code = ops._compute_code(mode)
    s2_w, _ = ops._lrt_prepare_raw(rho_w.detach(), None)
    want = [torch.empty_like(t) for t in got]
    xx = x.detach()
    ops.check(lib.bnn_lrt_backward_input(p(G_m), p(G_v), p(mu_w.detach()), p(s2_w), p(xx), K, p(want[0]), B, N, K, code, 0, st),
              "bnn_lrt_backward_input")
    ops.check(lib.bnn_lrt_backward_weight(p(xx), K, p(G_m), p(G_v), p(rho_w.detach()), p(want[1]), p(want[2]), p(rho_b.detach()),
                                          p(want[3]), p(want[4]), B, N, K, code, 0, st), "bnn_lrt_backward_weight")
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@gpu
def test_forward_and_backward_are_graph_capturable(dev):
    """forward_moments, the sampling launch on a fixed key, the loss and the whole backward in ONE captured graph on a side
    stream: two replays give the eager gradients' bits (no entry synchronises, allocates outside torch or reads host state)."""
    torch.manual_seed(8)
    net = set_params(Net([20, 33, 17, 5], False), 80).to(dev)
    g = torch.Generator().manual_seed(82)
    xd = torch.randn(9, 20, generator=g).to(dev).requires_grad_()
    t = torch.randint(0, 5, (9,), generator=g).to(dev).repeat(4)
    ps = leaves(net)
    key = DrawKey(0x1234567890ABCDEF, 322, 0, 4, 19, gen=_rng.generator_for("f32"))

    def step():
        mom = net.forward_moments(xd)
        ys = ops.moments_sample(mom, key, 4, track=True)
        return torch.autograd.grad(F.cross_entropy(ys.reshape(-1, 5), t, reduction="sum") + mom.var.sum(), [xd] + ps)

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


def toy_regression(device, steps=200):
    """1 -> 32 -> 1 on y = sin(2 x) + 0.1 noise, B = 64, Adam on mean(((y - m)^2 + v) / (2 s_n^2)) + KL / B with s_n = 0.3: the
    expected Gaussian negative log-likelihood under the propagated moments -- no sample anywhere.  -> (net, [loss per step])"""
    torch.manual_seed(12)
    net = Net([1, 32, 1], False)
    g = torch.Generator().manual_seed(13)
    x = torch.linspace(-2, 2, 64).unsqueeze(1)
    y = torch.sin(2 * x) + 0.1 * torch.randn(64, 1, generator=g)
    net, x, y = net.to(device), x.to(device), y.to(device)
    opt = torch.optim.Adam(net.parameters(), lr=0.02)
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


def test_training_without_sampling_cpu():
    """The method's own curve (the float64 recursion under torch autograd): far below the half mark the device test asserts."""
    net, losses = toy_regression("cpu")
    print("toy regression, CPU float64 path: loss %.4f -> %.4f (ratio %.3f)" % (losses[0], losses[-1], losses[-1] / losses[0]))
    assert losses[-1] < 0.25 * losses[0]
    assert not hasattr(net, "moment_key")


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_training_without_sampling(dev, mode):
    """200 Adam steps of the sampling-free regression loss on the device: the loss falls below half its starting value (the CPU
    float64 path ends below a quarter, test_training_without_sampling_cpu), and no key is ever drawn."""
    bnn.set_compute(mode)
    net, losses = toy_regression(dev)
    print("toy regression, %s: loss %.4f -> %.4f (ratio %.3f)" % (mode, losses[0], losses[-1], losses[-1] / losses[0]))
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < 0.5 * losses[0]
    assert not hasattr(net, "moment_key")
