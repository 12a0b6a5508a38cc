"""LocalReparamLinear (K10, csrc/bnn_lrt.hip): the local-reparameterization estimator of NormalLinear's posterior,

    m = x mu_w^T + mu_b,   v = x^2 (sigma_w^2)^T + sigma_b^2,   y_s = m + sqrt(v + 1e-16) eps_s,

eps[b N + n] of the layer's noise key, sample sample0 + s.  CPU tests: the host surface, the torch expression, the moments, the
built code object.  GPU tests: the kernels against float64 on the key's own eps (the oracle's CPU twin of the stream).

Bounds.  fp32 mode: 1e-5 of the output scale (conftest.assert_close_scaled's rule) plus 2e-5 sqrt(v), the measured bound of the
device eps against its CPU twin (test_hip_parity.test_eps_stream_matches_cpu_twin).  bf16 mode: the reference is float64 on the
operands as the kernel rounds them (x, x^2 -- squared in fp32 first --, mu_w, sigma_w^2 to bf16, RNE); products of bf16 values are
exact in fp32, so the device differs by the fp32 accumulation of the two sums alone, gamma_{K+1} sum |a| |b| per element
(tests/golden/bf16ref.py), carried through sqrt and the product with eps.  In the bf16 backward the intermediate g_m / g_v are
rounded to bf16 as operands of the second contractions: an element whose error interval holds a rounding midpoint may round either
way on the device, and bf16ref.round_hidden carries that deviation into the bound.
"""
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, _rng, ops
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, KLDivergence, NormalLinear
from bayesianneuralnetworks_amd.nn import LocalReparamLinear
from bayesianneuralnetworks_amd._rng import DrawKey
from oracle import oracle as orc

from bf16ref import chain_layer, gamma, rne_bf16, round_hidden
from test_flipout_mc import _code_object_notes

U = 2.0 ** -24
EPS_TWIN = 2e-5          # device eps vs its CPU twin (measured bound of test_eps_stream_matches_cpu_twin)
gpu = pytest.mark.gpu


def sigma64(rho):
    return F.softplus(rho.double()) + 1e-10


def lrt64(x, xsq, mu, s2, mu_b, s2_b, eps):
    """(y, m, v) of the formula in float64; eps: (S, B, N); x (B, K) or (S, B, K)."""
    m = x @ mu.t()
    v = xsq @ s2.t()
    if mu_b is not None:
        m, v = m + mu_b, v + s2_b
    return m + torch.sqrt(v + 1e-16) * eps, m, v


def assert_within(got, ref, bound, what):
    got, ref, bound = got.detach().double().cpu(), ref.double(), bound.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    excess = (got - ref).abs() - bound
    worst = int(excess.argmax())
    print("%s: max |err| %.3e, worst err / bound %.3f" % (what, float((got - ref).abs().max()),
                                                         float(((got - ref).abs() / bound.clamp_min(1e-300)).max())))
    assert bool((excess <= 0).all()), "%s: |err| %.3e > bound %.3e at element %d (%d of %d out)" % (
        what, float((got - ref).abs().reshape(-1)[worst]), float(bound.reshape(-1)[worst]), worst, int((excess > 0).sum()), excess.numel())


def scaled_bound(ref, tol=1e-5):
    """conftest.assert_close_scaled's allowance as a tensor: tol max(1, rms(ref)) + tol |ref|."""
    ref = ref.double()
    return tol * max(1.0, float(ref.pow(2).mean().sqrt())) + tol * ref.abs()


def make_params(N, K, bias, seed):
    g = torch.Generator().manual_seed(seed)
    mu_w = (torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5
    rho_w = -3 + 0.3 * torch.randn(N, K, generator=g)
    mu_b = (torch.rand(N, generator=g) * 2 - 1) / K ** 0.5 if bias else None
    rho_b = -3 + 0.3 * torch.randn(N, generator=g) if bias else None
    return mu_w, rho_w, mu_b, rho_b


# ================================================================================================ CPU
def test_layer_is_exposed_but_not_in_all():
    import pytorch_bayesian.nn as alias
    assert alias.LocalReparamLinear is LocalReparamLinear
    assert "LocalReparamLinear" not in bnn.nn.__all__
    assert not issubclass(LocalReparamLinear, NormalLinear)          # the draw plan / fuse_activations pass it by


def test_state_dict_and_kl_are_normal_linears():
    torch.manual_seed(0)
    a, b = LocalReparamLinear(40, 24), NormalLinear(40, 24)
    assert sorted(a.state_dict()) == sorted(b.state_dict()) == ["bias.mean", "bias.scale", "weight.mean", "weight.scale"]
    b.load_state_dict(a.state_dict())
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k])
    with torch.no_grad():
        b.weight.mean.add_(1.0)
    a.load_state_dict(b.state_dict())
    assert torch.equal(a.weight.mean, b.weight.mean)

    class Net(BayesianNetworkModule):
        def __init__(self, layer):
            super().__init__(40, 24, samples=1)
            self.layers = torch.nn.Sequential(layer)

        def _forward(self, x):
            return self.layers(x)

    ka, kb = KLDivergence()(Net(a)), KLDivergence()(Net(b))
    assert ka.item() == kb.item()
    assert Net(a).kl_divergence().item() == kb.item()


@pytest.mark.parametrize("bias", [True, False])
def test_cpu_forward_is_the_formula(bias):
    torch.manual_seed(1)
    layer = LocalReparamLinear(20, 12, bias=bias)
    x = torch.randn(9, 20)
    torch.manual_seed(77)
    y = layer(x)
    torch.manual_seed(77)
    eps = torch.randn(9, 12)
    ref, _, _ = lrt64(x.double(), x.double() ** 2, layer.weight.mean.double(), sigma64(layer.weight.scale) ** 2,
                      layer.bias.mean.double() if bias else None, sigma64(layer.bias.scale) ** 2 if bias else None, eps.double())
    assert torch.allclose(y.double(), ref, atol=1e-5, rtol=1e-5)
    assert torch.equal(layer(x, sample=False), y)                  # the same noise again
    y1 = layer(torch.randn(20))
    assert y1.shape == (12,)
    assert layer(torch.randn(9, 3, 20)).shape == (9, 3, 12)
    with pytest.raises(RuntimeError):
        layer(x, sample=False)                                     # the recorded noise has another shape now


def test_cpu_expression_gradcheck():
    torch.manual_seed(2)
    layer = LocalReparamLinear(6, 5).double()
    x = torch.randn(4, 6, dtype=torch.float64, requires_grad=True)
    layer(x)                                                       # records the noise

    def f(x, mw, rw, mb, rb):
        return torch.func.functional_call(layer, {"weight.mean": mw, "weight.scale": rw, "bias.mean": mb, "bias.scale": rb},
                                          (x, False))

    assert torch.autograd.gradcheck(f, (x, layer.weight.mean, layer.weight.scale, layer.bias.mean, layer.bias.scale))


def test_cpu_moments_and_weight_sampling_has_the_same():
    """Every element's sample mean within 6 standard errors of m and |var / v - 1| <= 6 sqrt(2 / S); the same bounds hold for
    weight sampling (w = mu + sigma eps) of the same posterior: the two layers sample one distribution."""
    torch.manual_seed(0)
    B, K, N, S = 64, 96, 48, 4096
    layer = LocalReparamLinear(K, N, bias=False).double()
    with torch.no_grad():
        layer.weight.mean.copy_(torch.randn(N, K) * 0.1)
        layer.weight.scale.copy_(-3 + 0.3 * torch.randn(N, K))
    x = torch.randn(B, K, dtype=torch.float64)
    with torch.no_grad():
        mu, sig = layer.weight.mean, sigma64(layer.weight.scale)
        m, v = x @ mu.t(), (x * x) @ (sig * sig).t()
        ys = torch.stack([layer(x) for _ in range(S)])
        z = ((ys.mean(0) - m).abs() / (v / S).sqrt()).max().item()
        r = (ys.var(0, unbiased=True) / v - 1).abs().max().item()
        print("LRT: worst mean %.2f standard errors, worst |var / v - 1| %.3f (bound %.3f)" % (z, r, 6 * (2 / S) ** 0.5))
        assert z <= 6 and r <= 6 * (2 / S) ** 0.5
        S2 = 2048
        w = mu + sig * torch.randn(S2, N, K, dtype=torch.float64)
        yw = torch.einsum("bk,snk->sbn", x, w)
        z2 = ((yw.mean(0) - m).abs() / (v / S2).sqrt()).max().item()
        r2 = (yw.var(0, unbiased=True) / v - 1).abs().max().item()
        print("weight sampling: worst mean %.2f standard errors, worst |var / v - 1| %.3f (bound %.4f)" % (z2, r2, 6 * (2 / S2) ** 0.5))
        assert z2 <= 6 and r2 <= 6 * (2 / S2) ** 0.5


def test_lrt_kernels_do_not_spill():
    """Every instantiation of the paired-contraction tile (forward, input gradient, weight gradient x bf16, fp32; the third
    template argument is this posterior's chain factor, which only the weight gradient's epilogue uses) keeps both accumulator
    sets in registers, and the elementwise kernels use no scratch either."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    tiles = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn5k_lrtI[tf]Li[012]ENS_8ChainRhoEEEvNS_7LrtArgsE$", n)}
    assert len(tiles) == 6, sorted(kernels)
    rest = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn(13k_lrt_prepare|18k_lrt_bwd_epilogue|15k_lrt_bias_grad)", n)}
    assert len(rest) == 4, sorted(kernels)
    for n, f in {**tiles, **rest}.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("private_segment_fixed_size", 0)) == 0, (n, f)


def test_lrt_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)
    r = _lib.Rng(seed=1, stream=5)
    rr = ctypes.byref(r)
    assert lib.bnn_lrt_prepare(None, one, 4, None, None, 0, None) == -1
    assert lib.bnn_lrt_prepare(one, odd, 4, None, None, 0, None) == -4
    assert lib.bnn_lrt_forward(None, 8, one, one, None, None, one, None, 4, 4, 8, 1, 1, rr, 0, 0, None) == -1
    assert lib.bnn_lrt_forward(one, 8, one, one, one, None, one, None, 4, 4, 8, 1, 1, rr, 0, 0, None) == -1      # mu_b without s2_b
    assert lib.bnn_lrt_forward(one, 8, one, one, None, None, one, None, 4, 4, 8, 1, 1, None, 0, 0, None) == -1
    assert lib.bnn_lrt_forward(one, 8, one, one, None, None, one, None, 4, 0, 8, 1, 1, rr, 0, 0, None) == -2
    assert lib.bnn_lrt_forward(one, 4, one, one, None, None, one, None, 4, 4, 8, 1, 1, rr, 0, 0, None) == -2      # ldx < K
    assert lib.bnn_lrt_forward(one, 8, one, one, None, None, one, None, 4, 4, 8, 70000, 1, rr, 0, 0, None) == -5
    assert lib.bnn_lrt_forward(one, 8, one, one, None, None, one, None, 1 << 20, 1 << 12, 8, 1, 1, rr, 0, 0, None) == -5
    assert b"2^32" in lib.bnn_last_error()
    assert lib.bnn_lrt_forward(one, 8, one, one, None, None, one, None, 4, 4, 8, 1, 1, rr, 7, 0, None) == -3
    assert lib.bnn_lrt_forward(one, 8, one, one, None, None, one, None, 4, 4, 8, 1, 1, rr, 0, _lib.FLAG_Y_BF16, None) == -6
    assert lib.bnn_lrt_forward(one, 8, one, one, None, None, odd, None, 4, 4, 8, 1, 1, rr, 0, 0, None) == -4
    bad = _lib.Rng(seed=1, stream=70000)
    assert lib.bnn_lrt_forward(one, 8, one, one, None, None, one, None, 4, 4, 8, 1, 1, ctypes.byref(bad), 0, 0, None) == -5
    assert lib.bnn_lrt_backward_epilogue(one, None, one, one, 4, 4, 1, 1, rr, 0, None) == -1
    assert lib.bnn_lrt_backward_epilogue(one, one, one, one, 4, 4, 0, 1, rr, 0, None) == -2
    assert lib.bnn_lrt_backward_epilogue(one, one, odd, one, 4, 4, 1, 1, rr, 0, None) == -4
    assert lib.bnn_lrt_backward_input(one, one, one, one, one, 8, None, 4, 4, 8, 0, 0, None) == -1
    assert lib.bnn_lrt_backward_input(one, one, one, one, one, 8, one, 4, 4, 0, 0, 0, None) == -2
    assert lib.bnn_lrt_backward_input(one, one, one, one, one, 8, odd, 4, 4, 8, 0, 0, None) == -4
    assert lib.bnn_lrt_backward_weight(one, 8, one, one, one, one, None, None, None, None, 4, 4, 8, 0, 0, None) == -1
    assert lib.bnn_lrt_backward_weight(one, 8, one, one, one, one, one, one, None, None, 4, 4, 8, 0, 0, None) == -1  # partial bias
    assert lib.bnn_lrt_backward_weight(one, 8, one, one, one, one, one, None, None, None, 4, 4, 8, 0, _lib.FLAG_X_BF16, None) == -6
    assert lib.bnn_lrt_backward_weight(one, 8, one, one, one, odd, one, None, None, None, 4, 4, 8, 0, 0, None) == -4
    assert lib.bnn_launch_count() == n0


def test_backward_formulas_are_the_autograd_of_the_forward():
    """The explicit backward the bf16 GPU test restates (g_m, g_v, the paired contractions, the rho chain rule) IS float64
    autograd of the formula, zero input row included."""
    torch.manual_seed(3)
    B, K, N, S = 7, 10, 6, 3
    mu_w, rho_w, mu_b, rho_b = [t.double().requires_grad_() for t in make_params(N, K, True, 5)]
    x = torch.randn(B, K, dtype=torch.float64)
    x[2] = 0
    x.requires_grad_()
    eps, gy = torch.randn(S, B, N, dtype=torch.float64), torch.randn(S, B, N, dtype=torch.float64)
    y, _, v = lrt64(x, x * x, mu_w, sigma64(rho_w) ** 2, mu_b, sigma64(rho_b) ** 2, eps)
    want = torch.autograd.grad((y * gy).sum(), (x, mu_w, rho_w, mu_b, rho_b))
    with torch.no_grad():
        got = backward64(x, x * x, x, mu_w, sigma64(rho_w) ** 2, rho_w, rho_b, v, eps, gy, True)
    for g, w in zip(got, want):
        assert torch.allclose(g, w, atol=1e-12, rtol=1e-10)


def backward64(x, xsq, x_epi, mu, s2, rho_w, rho_b, v, eps, gy, shared, rnd=None, betas=None):
    """The backward of csrc/bnn_lrt.hip in float64.  shared: x (B, K), gy / eps (S, B, N), v (B, N); otherwise every row of the
    (S B, .) tensors is its own.  rnd: None, or the rounding of the intermediate operands g_m / g_v (bf16 mode) as
    rnd(t, beta) -> (h, dev); then betas = (beta_m, beta_v) and the result is [(gradient, bound), ...]."""
    inv = 0.5 / torch.sqrt(v + 1e-16)
    if shared:
        g_m, g_v = gy.sum(0), (gy * eps).sum(0) * inv
    else:
        g_m, g_v = gy, gy * eps * inv
    c_w = 2 * sigma64(rho_w) * torch.sigmoid(rho_w.double())
    c_b = None if rho_b is None else 2 * sigma64(rho_b) * torch.sigmoid(rho_b.double())
    if rnd is None:
        gx = g_m @ mu + 2 * x_epi * (g_v @ s2)
        out = [gx, g_m.t() @ x, (g_v.t() @ xsq) * c_w]
        if rho_b is not None:
            out += [g_m.sum(0), g_v.sum(0) * c_b]
        return out
    h_m, d_m = rnd(g_m, betas[0])
    h_v, d_v = rnd(g_v, betas[1])
    t1, a1, s1, _ = chain_layer(h_m, d_m, mu.t().contiguous(), None)
    t2, a2, s2_, _ = chain_layer(h_v, d_v, s2.t().contiguous(), None)
    gx = t1 + 2 * x_epi * t2
    out = [(gx, a1 + s1 + 2 * x_epi.abs() * (a2 + s2_) + 4 * U * (t1.abs() + 2 * x_epi.abs() * t2.abs()))]
    t, a, s, _ = chain_layer(h_m.t().contiguous(), d_m.t().contiguous(), x.t().contiguous(), None)
    out.append((t, a + s))
    t, a, s, _ = chain_layer(h_v.t().contiguous(), d_v.t().contiguous(), xsq.t().contiguous(), None)
    out.append((t * c_w, (a + s) * c_w + 16 * U * (t * c_w).abs()))           # sigma, sigmoid and three products in fp32
    if rho_b is not None:
        M = g_m.shape[0]
        out.append((g_m.sum(0), gamma(M) * g_m.abs().sum(0) + betas[0].sum(0)))          # the bias sums read the fp32 g_m / g_v
        tb = g_v.sum(0)
        out.append((tb * c_b, (gamma(M) * g_v.abs().sum(0) + betas[1].sum(0)) * c_b + 16 * U * (tb * c_b).abs()))
    return out


# ================================================================================================ GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


def _epoch_dev(dev):
    return int(_rng.default_generator.epoch_dev(dev)[0].item())


def twin_eps(key, S, shape, dev):
    ed = _epoch_dev(dev)
    return torch.from_numpy(np.stack([orc.eps_fill(key.seed, key.stream, key.sample0 + s, key.epoch_host, ed,
                                                   (shape[0] * shape[1],), key.gen).reshape(shape) for s in range(S)])).double()


def operands64(x, mu_w, rho_w, mu_b, rho_b, mode, dev):
    """float64 operands as the kernel contracts them: (x, x^2, mu_w, sigma_w^2, mu_b, sigma_b^2)."""
    want_w = sigma64(rho_w) ** 2
    want_b = sigma64(rho_b) ** 2 if rho_b is not None else None
    if mode == "f32":
        return x.double(), x.double() ** 2, mu_w.double(), want_w, None if mu_b is None else mu_b.double(), want_b
    # bf16: sigma^2 is computed in fp32 on the device and rounded from there -- take the device's fp32 value (checked against
    # float64 here), so that the reference rounds what the kernel rounds
    s2_w, s2_b = ops._lrt_prepare_raw(rho_w.to(dev), None if rho_b is None else rho_b.to(dev))
    s2_w = s2_w.cpu()
    assert ((s2_w.double() - want_w).abs() <= 1e-6 * want_w).all()
    if rho_b is not None:
        s2_b = s2_b.cpu()
        assert ((s2_b.double() - want_b).abs() <= 1e-6 * want_b).all()
    return (rne_bf16(x), rne_bf16(x.float() * x.float()), rne_bf16(mu_w), rne_bf16(s2_w),
            None if mu_b is None else mu_b.double(), None if rho_b is None else s2_b.double())


def forward_bound(mode, x64, mu64, mu_b, y, v, eps, K):
    sd = torch.sqrt(v + 1e-16)
    if mode == "f32":
        return scaled_bound(y) + EPS_TWIN * sd
    a_m = x64.abs() @ mu64.abs().t() + (0 if mu_b is None else mu_b.abs())
    b_m, b_v = gamma(K + 1) * a_m, gamma(K + 1) * v                     # v is its own sum |a| |b|: every term is >= 0
    b_sd = b_v / sd + 4 * U * sd                                          # sqrt is 1 / (2 sd)-Lipschitz; + 1e-16 and sqrt round
    return b_m + eps.abs() * b_sd + EPS_TWIN * sd + 2 * U * y.abs()


SHAPES = [(512, 784, 1200), (33, 100, 7), (1, 64, 64), (130, 1200, 10)]


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("S", [1, 4, 8, 33])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_matches_float64_on_the_keys_eps(dev, shape, S, shared, bias, mode):
    B, K, N = shape
    mu_w, rho_w, mu_b, rho_b = make_params(N, K, bias, 11)
    g = torch.Generator().manual_seed(12)
    x = torch.randn((B, K) if shared else (S, B, K), generator=g)
    key = DrawKey(0x1234567890ABCDEF, 321, 3, S, 17, gen=_rng.generator_for(mode))          # sample0 = 3
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    y = ops.linear_lrt(x.to(dev), mu_w.to(dev), rho_w.to(dev), None if mu_b is None else mu_b.to(dev),
                       None if rho_b is None else rho_b.to(dev), key, shared, mode)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 2            # the operand launch + ONE contraction launch for all S samples
    assert y.shape == (S, B, N) and y.dtype == torch.float32
    x64, xsq, mu64, s2, mb, s2b = operands64(x, mu_w, rho_w, mu_b, rho_b, mode, dev)
    eps = twin_eps(key, S, (B, N), dev)
    ref, _, v = lrt64(x64, xsq, mu64, s2, mb, s2b, eps)
    assert_within(y, ref, forward_bound(mode, x64, mu64, mb, ref, v, eps, K), "y %s S=%d %s" % (shape, S, mode))


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_shared_and_per_sample_inputs_give_the_same_bits(dev, mode):
    B, K, N, S = 33, 100, 24, 4
    mu_w, rho_w, mu_b, rho_b = [t.to(dev) for t in make_params(N, K, True, 21)]
    x = torch.randn(B, K, device=dev)
    key = DrawKey(99, 7, 2, S, 5, gen=_rng.generator_for(mode))
    a = ops.linear_lrt(x, mu_w, rho_w, mu_b, rho_b, key, True, mode)
    b = ops.linear_lrt(x.unsqueeze(0).repeat(S, 1, 1), mu_w, rho_w, mu_b, rho_b, key, False, mode)
    c = ops.linear_lrt(x, mu_w, rho_w, mu_b, rho_b, key, True, mode)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(a[0], a[1])


@gpu
def test_sample_flag_and_noise_key(dev):
    torch.manual_seed(4)
    layer = LocalReparamLinear(48, 20).to(dev)
    x = torch.randn(16, 48, device=dev)
    bnn.manual_seed(5)
    with pytest.raises(RuntimeError):
        layer(x, sample=False)                         # nothing recorded yet
    y0 = layer(x)
    k0 = layer.noise_key
    assert (k0.stream, k0.sample0, k0.nsamples, k0.gen) == (layer._noise_stream, 0, 1, _rng.GEN_PHILOX10_U24)
    assert layer._noise_stream not in (layer.weight._stream, layer.bias._stream)
    assert torch.equal(layer(x, sample=False), y0) and layer.noise_key is k0
    y1 = layer(x)
    assert layer.noise_key.epoch_host != k0.epoch_host and not torch.equal(y1, y0)
    with pytest.raises(RuntimeError):
        layer(x[:8], sample=False)                     # another output shape
    assert layer(x[0]).shape == (20,) and layer(x.reshape(4, 4, 48)).shape == (4, 4, 20)
    with _mc.McContext(4, 16, sample0=2):
        ys = layer(x)                                  # shared input: 16 rows in, 64 out
        assert ys.shape == (64, 20) and (layer.noise_key.sample0, layer.noise_key.nsamples) == (2, 4)
        assert torch.equal(layer(x.repeat(4, 1), sample=False), ys)
        with pytest.raises(RuntimeError):
            layer(x[:5])
    bnn.set_compute("bf16")
    layer(x)
    assert layer.noise_key.gen == _rng.generator_for("bf16")
    with pytest.raises(ops.BnnHipError):
        ops.linear_lrt(x.double(), layer.weight.mean, layer.weight.scale, None, None, k0, True, "f32")      # no torch fallback
    assert "features" in ops.lrt_eligible(x[:, :40], layer.weight.mean, 16, 1)
    assert "32 bits" in ops.lrt_eligible(torch.empty(0, 48), torch.empty(1 << 20, 48), 1 << 12, 1)


BWD_SHAPES = [(33, 100, 7), (64, 96, 48), (130, 200, 72)]


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_matches_float64_on_the_keys_eps(dev, shape, S, shared, bias, mode):
    """All five gradients; the batch holds an all-zero input row (v = sigma_b^2 there, and v = 0 without bias)."""
    B, K, N = shape
    params = make_params(N, K, bias, 31)
    g = torch.Generator().manual_seed(32)
    x = torch.randn((B, K) if shared else (S, B, K), generator=g)
    x[..., 5 % B, :] = 0
    gy = torch.randn(S, B, N, generator=g)
    key = DrawKey(777, 45, 1, S, 9, gen=_rng.generator_for(mode))
    leaves = [None if t is None else t.to(dev).requires_grad_() for t in (x,) + params]
    lib = _lib.load()
    y = ops.linear_lrt(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], key, shared, mode)
    n0 = lib.bnn_launch_count()
    got = torch.autograd.grad(y, [t for t in leaves if t is not None], gy.to(dev))
    torch.cuda.synchronize()
    # the noise launch, the paired input- and weight-gradient contractions, the bias sums: nothing else ran
    assert lib.bnn_launch_count() == n0 + (4 if bias else 3)
    assert all(torch.isfinite(t).all() for t in got)
    mu_w, rho_w, mu_b, rho_b = params
    eps = twin_eps(key, S, (B, N), dev)
    names = ["x", "weight.mean", "weight.scale"] + (["bias.mean", "bias.scale"] if bias else [])
    if mode == "f32":
        ref = [t.double().requires_grad_() for t in (x,) + params if t is not None]
        p64 = ref[1:] + ([None, None] if not bias else [])
        yr, _, _ = lrt64(ref[0], ref[0] * ref[0], p64[0], sigma64(p64[1]) ** 2, p64[2], None if not bias else sigma64(p64[3]) ** 2, eps)
        want = torch.autograd.grad((yr * gy.double()).sum(), ref)
        for n, a, w in zip(names, got, want):
            assert_within(a, w, scaled_bound(w), "g %s %s S=%d f32" % (n, shape, S))
        return
    x64, xsq, mu64, s2, mb, s2b = operands64(x, mu_w, rho_w, mu_b, rho_b, mode, dev)
    _, _, v = lrt64(x64, xsq, mu64, s2, mb, s2b, eps)
    gy64 = gy.double()
    # device deviations before g_m / g_v are rounded to bf16: v (the forward's accumulation bound), 1 / (2 sqrt(.)), eps, the products
    # and the fp32 sum over the samples
    rel_inv = 1.01 * 0.5 * gamma(K + 1) * v / (v + 1e-16) + 4 * U
    inv = 0.5 / torch.sqrt(v + 1e-16)
    term = gy64.abs() * inv * (eps.abs() * (rel_inv + 3 * U) + EPS_TWIN)
    if shared:
        beta_m = gamma(S) * gy64.abs().sum(0)
        beta_v = 1.01 * (term.sum(0) + gamma(S) * (gy64 * eps).abs().sum(0) * inv)
    else:
        beta_m, beta_v = torch.zeros_like(gy64), 1.01 * term
    flat = (lambda t: t) if shared else (lambda t: t.reshape(S * B, -1))
    want = backward64(flat(x64), flat(xsq), flat(x.double()), mu64, s2, rho_w, rho_b if bias else None, flat(v) if not shared else v,
                      flat(eps) if not shared else eps, flat(gy64) if not shared else gy64, shared,
                      rnd=lambda t, beta: round_hidden(t, beta)[:2], betas=(flat(beta_m), flat(beta_v)))
    for n, a, (w, bound) in zip(names, got, want):
        assert_within(a.reshape(w.shape), w, bound + 1e-30, "g %s %s S=%d bf16" % (n, shape, S))


@gpu
@pytest.mark.parametrize("gen", [0, 1])
def test_device_moments(dev, gen):
    torch.manual_seed(0)
    B, K, N, S = 64, 96, 48, 512
    mu_w, rho_w = torch.randn(N, K) * 0.1, -3 + 0.3 * torch.randn(N, K)
    x = torch.randn(B, K)
    n0 = _lib.load().bnn_launch_count()
    ys = ops.linear_lrt(x.to(dev), mu_w.to(dev), rho_w.to(dev), None, None, DrawKey(2024, 9, 0, S, 3, gen=gen), True, "f32").double().cpu()
    assert _lib.load().bnn_launch_count() == n0 + 2
    m, v = x.double() @ mu_w.double().t(), (x.double() ** 2) @ (sigma64(rho_w) ** 2).t()
    z = ((ys.mean(0) - m).abs() / (v / S).sqrt()).max().item()
    r = (ys.var(0, unbiased=True) / v - 1).abs().max().item()
    print("device gen %d: worst mean %.2f standard errors, worst |var / v - 1| %.3f (bound %.3f)" % (gen, z, r, 6 * (2 / S) ** 0.5))
    assert z <= 6 and r <= 6 * (2 / S) ** 0.5


class LrtNet(BayesianNetworkModule):
    def __init__(self, samples=4):
        super().__init__(40, 10, samples=samples)
        self.layers = torch.nn.Sequential(LocalReparamLinear(40, 64), torch.nn.ReLU(), LocalReparamLinear(64, 48), torch.nn.ReLU(),
                                          LocalReparamLinear(48, 10))

    def _forward(self, x):
        return self.layers(x)


def net64(net, x, S, dev):
    """The serial float64 restatement on the recorded noise keys.  The noise is read from the device stream of each key
    (ops.eps_philox: the stream test_forward_matches_float64_on_the_keys_eps ties to the CPU twin), so that the twin's 2e-5
    does not compound through three layers."""
    outs = []
    for s in range(S):
        h = x.double().cpu()
        for layer in net.layers:
            if isinstance(layer, LocalReparamLinear):
                key = layer.noise_key
                B, N = h.shape[0], layer.weight.mean.shape[0]
                eps = ops.eps_philox((B * N,), key, dev)[s].reshape(B, N).double().cpu()
                h, _, _ = lrt64(h, h * h, layer.weight.mean.detach().double().cpu(), sigma64(layer.weight.scale.detach().cpu()) ** 2,
                                layer.bias.mean.detach().double().cpu(), sigma64(layer.bias.scale.detach().cpu()) ** 2, eps)
            else:
                h = h.clamp_min(0)
        outs.append(h)
    return torch.stack(outs)


@gpu
def test_network_forward_predictive_and_training_step(dev):
    torch.manual_seed(6)
    S, B = 4, 32
    net = LrtNet(S).to(dev)
    net.mc_batched = True
    x = torch.randn(B, 40, device=dev)
    lib = _lib.load()
    bnn.manual_seed(100)
    n0 = lib.bnn_launch_count()
    with torch.no_grad():
        ys = torch.stack(net(x))
    assert lib.bnn_launch_count() == n0 + 6            # per layer: the operand launch + one contraction launch
    keys = [l.noise_key for l in net.layers if isinstance(l, LocalReparamLinear)]
    assert [k.nsamples for k in keys] == [S] * 3 and len({k.stream for k in keys}) == 3
    want = net64(net, x, S, dev)
    assert_within(ys, want, scaled_bound(want), "3-layer LRT net")
    # the MC reductions on it (same seed: the same keys, so the stacked outputs are these calls' samples)
    bnn.manual_seed(100)
    with torch.no_grad():
        pm = net.predictive_mean(x)
    assert (pm.double().cpu() - ys.double().cpu().mean(0)).abs().max() <= 1e-5
    bnn.manual_seed(100)
    with torch.no_grad():
        u = net.predictive_uncertainty(x, inputs="logits")
    r = ops.uncertainty_f64(ys.cpu(), "logits")
    tol = 1e-5 * max(1.0, float(np.log(10)))
    assert (u.mean.double().cpu() - r.mean.double()).abs().max() <= 1e-6
    for a, b in ((u.total, r.total), (u.aleatoric, r.aleatoric), (u.epistemic, r.epistemic)):
        assert (a.double().cpu() - b.double()).abs().max() <= tol
    # one training step
    before = [p.detach().clone() for p in net.parameters()]
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    target = torch.randint(0, 10, (B,), device=dev)
    n1 = lib.bnn_launch_count()
    loss = KLDivergence()(net) + sum(F.cross_entropy(y, target) for y in net(x)) / S
    loss.backward()
    opt.step()
    assert lib.bnn_launch_count() >= n1 + 6 + 3 * 4
    assert len(before) == 12
    for p, b in zip(net.parameters(), before):
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), b)
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_sharded_pass_reproduces_its_rows(dev, mode):
    torch.manual_seed(7)
    bnn.set_compute(mode)
    B = 16
    net = LrtNet(8).to(dev)
    net.mc_batched = True
    x = torch.randn(B, 40, device=dev)
    with torch.no_grad():
        bnn.manual_seed(55)
        full = net.forward_stacked(x, 8)
        bnn.manual_seed(55)
        lo = net.forward_stacked(x, 4, sample0=0)
        bnn.manual_seed(55)
        hi = net.forward_stacked(x, 4, sample0=4)
    assert net.layers[0].noise_key.sample0 == 4
    assert torch.equal(lo, full[:4]) and torch.equal(hi, full[4:])
