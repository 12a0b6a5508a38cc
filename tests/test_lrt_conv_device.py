"""LocalReparamConv1d / 2d / 3d (K11, k_lrt_conv3d of csrc/bnn_conv3d.hip): the local-reparameterization estimator of
NormalConvNd's posterior,

    m = convNd(x, mu_w, mu_b),   v = convNd(x^2, sigma_w^2, sigma_b^2),   y_s = m + sqrt(v + 1e-16) eps_s,

eps[(b O + o) P + p] of the layer's noise key, sample sample0 + s (LRT-conv noise contract, include/bnn_hip.h).  CPU tests: the
host surface, the torch expression, the backward restatement, the moments, the built code object, the entries' argument checks.
GPU tests: the kernels against float64 on the key's own eps (the oracle's CPU twin of the stream).

Bounds are test_lrt_device's.  Forward: the convolution is restated as the matrix product of the im2col panel (built here by
slicing, independently of torch's conv) with the weight laid out densely over all C T columns (zeros outside a row's group), so
that lrt64 and forward_bound apply as they stand with K = (C / groups) taps.  fp32: 1e-5 of the output scale plus
EPS_TWIN sqrt(v).  bf16: the reference contracts the operands as the kernel rounds them -- x, x^2 (squared in fp32 first), mu_w
and the DEVICE's fp32 sigma_w^2 (bnn_lrt_prepare's value, checked against float64 at 1e-6) to bf16, RNE, as they enter LDS -- and
the device differs by the fp32 accumulation alone, gamma_{K+1} sum |a| |b|, carried through the sqrt and the product with eps.
Backward, bf16: g_m / g_v are rounded to bf16 as operands of the gradient contractions; bf16ref.round_hidden carries an element
that may round either way on the device into the bound (it is not skipped), and the contractions are the bilinear maps
torch.nn.grad.convNd_input / convNd_weight in float64 on |operands| for the accumulation bound (gamma_{R+1}, R the reduction
length; the weight gradient adds at most 16 slab sums on top: gamma_{R+17}).

Backward launches: 1 (g_m, g_v: K10's epilogue) + 1 (input gradient) + 2 (weight-gradient slabs, their reduce) + 1 with a bias
(the bias sums) = 5 with a bias, 4 without.
"""
import ctypes
import itertools
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, _rng, ops
from bayesianneuralnetworks_amd.nn import (BayesianNetworkModule, KLDivergence, NormalConv1d, NormalConv2d, NormalConv3d,
                                           NormalConvNd, LocalReparamLinear)
from bayesianneuralnetworks_amd.nn import LocalReparamConv1d, LocalReparamConv2d, LocalReparamConv3d
from bayesianneuralnetworks_amd._rng import DrawKey

from bf16ref import gamma, rne_bf16, round_hidden
from test_flipout_mc import _code_object_notes
from test_lrt_device import EPS_TWIN, U, assert_within, forward_bound, lrt64, scaled_bound, sigma64, twin_eps

gpu = pytest.mark.gpu
CONV = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}
CONV_INPUT = {1: torch.nn.grad.conv1d_input, 2: torch.nn.grad.conv2d_input, 3: torch.nn.grad.conv3d_input}
CONV_WEIGHT = {1: torch.nn.grad.conv1d_weight, 2: torch.nn.grad.conv2d_weight, 3: torch.nn.grad.conv3d_weight}
LAYER = {1: LocalReparamConv1d, 2: LocalReparamConv2d, 3: LocalReparamConv3d}
NORMAL = {1: NormalConv1d, 2: NormalConv2d, 3: NormalConv3d}


class Case:
    """One conv geometry: B images (C, *sp) -> O channels."""

    def __init__(self, B, C, sp, O, k, s=1, p=0, d=1, g=1):
        nd = len(sp)
        tup = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * nd
        self.B, self.C, self.sp, self.O, self.g, self.nd = B, C, tuple(sp), O, g, nd
        self.k, self.s, self.p, self.d = tup(k), tup(s), tup(p), tup(d)
        self.out = tuple((self.sp[i] + 2 * self.p[i] - self.d[i] * (self.k[i] - 1) - 1) // self.s[i] + 1 for i in range(nd))
        self.P = int(np.prod(self.out))
        self.T = int(np.prod(self.k))
        self.K = C // g * self.T

    @property
    def geo(self):
        return self.s, self.p, self.d, self.g

    def conv(self, x, w, b=None):
        lead = x.shape[:-self.nd - 1]
        y = CONV[self.nd](x.reshape(-1, *x.shape[-self.nd - 1:]), w, b, *self.geo)
        return y.reshape(*lead, *y.shape[1:])

    def dgrad(self, g, w):
        """The input-gradient contraction as a bilinear map of (g (R, O, *out), w)."""
        return CONV_INPUT[self.nd]((g.shape[0], self.C) + self.sp, w, g, *self.geo)

    def wgrad(self, x, g):
        """The weight-gradient contraction as a bilinear map of (x (R, C, *sp), g (R, O, *out))."""
        return CONV_WEIGHT[self.nd](x, (self.O, self.C // self.g) + self.k, g, *self.geo)

    def params(self, bias, seed):
        g = torch.Generator().manual_seed(seed)
        mu_w = (torch.rand(self.O, self.C // self.g, *self.k, generator=g) * 2 - 1) / self.K ** 0.5
        rho_w = -3 + 0.3 * torch.randn(mu_w.shape, generator=g)
        mu_b = (torch.rand(self.O, generator=g) * 2 - 1) / self.K ** 0.5 if bias else None
        rho_b = -3 + 0.3 * torch.randn(self.O, generator=g) if bias else None
        return mu_w, rho_w, mu_b, rho_b

    def im2col(self, x):
        """(R, C, *sp) -> the panel (R P, C T), column c T + tap, by slicing the zero-padded input (no torch conv)."""
        xp = F.pad(x, [q for pp in reversed(self.p) for q in (pp, pp)])
        cols = []
        for tap in itertools.product(*[range(kk) for kk in self.k]):
            sl = tuple(slice(tap[i] * self.d[i], tap[i] * self.d[i] + (self.out[i] - 1) * self.s[i] + 1, self.s[i]) for i in range(self.nd))
            cols.append(xp[(slice(None), slice(None)) + sl])
        col = torch.stack(cols, 2).reshape(x.shape[0], self.C * self.T, self.P)
        return col.transpose(1, 2).reshape(x.shape[0] * self.P, self.C * self.T)

    def dense_w(self, w):
        """(O, C / g, *k) -> (O, C T): a row's own group's columns, zeros elsewhere."""
        Cg, Ng = self.C // self.g, self.O // self.g
        out = torch.zeros(self.O, self.C * self.T, dtype=w.dtype)
        for grp in range(self.g):
            out[grp * Ng:(grp + 1) * Ng, grp * Cg * self.T:(grp + 1) * Cg * self.T] = w[grp * Ng:(grp + 1) * Ng].reshape(Ng, Cg * self.T)
        return out

    def rows(self, t):
        """(..., R, O, *out) -> (..., R P, O): the panel's row order."""
        lead = t.shape[:-self.nd - 2]
        R = t.shape[-self.nd - 2]
        return t.reshape(*lead, R, self.O, self.P).transpose(-1, -2).reshape(*lead, R * self.P, self.O)


def formula64(case, x, mu_w, rho_w, mu_b, rho_b, eps):
    """(y, m, v) of the formula in float64 with torch's conv; x (B, C, ...) or (S, B, C, ...), eps (S, B, O, ...)."""
    m = case.conv(x, mu_w, mu_b)
    v = case.conv(x * x, sigma64(rho_w) ** 2, None if rho_b is None else sigma64(rho_b) ** 2)
    return m + torch.sqrt(v + 1e-16) * eps, m, v


def backward64(case, x, xsq, x_epi, mu, s2, rho_w, rho_b, v, eps, gy, shared, rnd=None, betas=None):
    """The backward of K11 in float64.  shared: x (B, C, ...), gy / eps (S, B, O, ...), v (B, O, ...); otherwise the (S, B) axes of
    every tensor are one axis of S B images.  rnd / betas as test_lrt_device.backward64: -> [(gradient, bound), ...]."""
    inv = 0.5 / torch.sqrt(v + 1e-16)
    if shared:
        g_m, g_v = gy.sum(0), (gy * eps).sum(0) * inv
    else:
        g_m, g_v = gy, gy * eps * inv
    c_w = 2 * sigma64(rho_w) * torch.sigmoid(rho_w.double())
    c_b = None if rho_b is None else 2 * sigma64(rho_b) * torch.sigmoid(rho_b.double())
    red = [0] + list(range(2, g_m.dim()))
    if rnd is None:
        out = [case.dgrad(g_m, mu) + 2 * x_epi * case.dgrad(g_v, s2), case.wgrad(x, g_m), case.wgrad(xsq, g_v) * c_w]
        if rho_b is not None:
            out += [g_m.sum(red), g_v.sum(red) * c_b]
        return out
    h_m, d_m = rnd(g_m, betas[0])
    h_v, d_v = rnd(g_v, betas[1])

    def pair(fn, a, da, b, R):
        """t = fn(a, b) with the device's accumulation bound and the slack the deviations da of a carry (b exact)."""
        t, ab = fn(a, b), fn(a.abs(), b.abs())
        slack = fn(da, b.abs())
        return t, gamma(R) * (ab + slack) + gamma(R, 2.0 ** -53) * ab, slack

    Kd = case.O // case.g * case.T + 1
    t1, a1, s1 = pair(case.dgrad, h_m, d_m, mu, Kd)
    t2, a2, s2_ = pair(case.dgrad, h_v, d_v, s2, Kd)
    out = [(t1 + 2 * x_epi * t2, a1 + s1 + 2 * x_epi.abs() * (a2 + s2_) + 4 * U * (t1.abs() + 2 * x_epi.abs() * t2.abs()))]
    R = g_m.shape[0] * case.P + 17                                       # every position of every image, and at most 16 slab sums
    sw = lambda a, da, b, n: pair(lambda p, q: case.wgrad(q, p), a, da, b, n)    # the deviating operand first
    t, a, s = sw(h_m, d_m, x, R)
    out.append((t, a + s))
    t, a, s = sw(h_v, d_v, xsq, R)
    out.append((t * c_w, (a + s) * c_w + 16 * U * (t * c_w).abs()))           # sigma, sigmoid and three products in fp32
    if rho_b is not None:
        M = g_m.shape[0] * case.P
        out.append((g_m.sum(red), gamma(M) * g_m.abs().sum(red) + betas[0].sum(red)))     # the bias sums read the fp32 g_m / g_v
        tb = g_v.sum(red)
        out.append((tb * c_b, (gamma(M) * g_v.abs().sum(red) + betas[1].sum(red)) * c_b + 16 * U * (tb * c_b).abs()))
    return out


class ConvNet(BayesianNetworkModule):
    def __init__(self, samples=4):
        super().__init__(3, 10, samples=samples)
        self.layers = torch.nn.Sequential(LocalReparamConv2d(3, 8, 3, padding=1), torch.nn.ReLU(),
                                          LocalReparamConv2d(8, 6, 3, stride=2, groups=2), torch.nn.Flatten(),
                                          LocalReparamLinear(6 * 3 * 3, 10))

    def _forward(self, x):
        return self.layers(x)


# ================================================================================================ CPU
def test_layers_are_exposed_but_not_in_all():
    import pytorch_bayesian.nn as alias
    for nd in (1, 2, 3):
        cls = LAYER[nd]
        assert getattr(alias, cls.__name__) is cls and getattr(bnn.nn, cls.__name__) is cls
        assert cls.__name__ not in bnn.nn.__all__
        # the draw plan and fuse_activations / fuse_head select NormalLinear by exact type; nothing selects these by isinstance
        assert not issubclass(cls, (NormalConvNd, LocalReparamLinear)) and not issubclass(cls, bnn.nn.NormalLinear)
    net = ConvNet()
    bnn.nn.fuse_activations(net)
    assert all(getattr(l, "activation", None) is None for l in net.layers)


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_state_dict_round_trips_with_normal_conv(nd):
    torch.manual_seed(0)
    a, b = LAYER[nd](4, 6, 3, groups=2), NORMAL[nd](4, 6, 3, groups=2)
    assert sorted(a.state_dict()) == sorted(b.state_dict()) == ["bias.mean", "bias.scale", "weight.mean", "weight.scale"]
    b.load_state_dict(a.state_dict())
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k])
    with torch.no_grad():
        b.weight.mean.add_(1.0)
    a.load_state_dict(b.state_dict())
    assert torch.equal(a.weight.mean, b.weight.mean)


def test_kl_is_normal_conv2ds_bit_for_bit():
    torch.manual_seed(0)
    a, b = LocalReparamConv2d(4, 6, 3), NormalConv2d(4, 6, 3)
    b.load_state_dict(a.state_dict())

    class Net(BayesianNetworkModule):
        def __init__(self, layer):
            super().__init__(4, 6, samples=1)
            self.layers = torch.nn.Sequential(layer)

        def _forward(self, x):
            return self.layers(x)

    ka, kb = KLDivergence()(Net(a)), KLDivergence()(Net(b))
    assert ka.item() == kb.item()
    assert Net(a).kl_divergence().item() == Net(b).kl_divergence().item() == kb.item()


CPU_CASES = {
    "bias": (Case(3, 4, (7, 8), 6, 3, 1, 1), True),
    "nobias": (Case(3, 4, (7, 8), 6, 3, 1, 1), False),
    "groups2": (Case(3, 4, (7, 8), 6, 3, 1, 1, 1, 2), True),
    "peraxis": (Case(2, 3, (9, 11), 5, (3, 2), (2, 1), (1, 2), (1, 2)), True),
    "1d": (Case(3, 4, (13,), 5, 4, 2, 1, 2), True),
    "3d": (Case(2, 3, (5, 6, 7), 4, (2, 3, 2), (1, 2, 1), (1, 0, 1), (2, 1, 1)), True),
}


@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_cpu_forward_is_the_formula(name):
    case, bias = CPU_CASES[name]
    torch.manual_seed(1)
    layer = LAYER[case.nd](case.C, case.O, case.k, case.s, case.p, case.d, case.g, bias)
    x = torch.randn(case.B, case.C, *case.sp)
    torch.manual_seed(77)
    y = layer(x)
    assert y.shape == (case.B, case.O) + case.out
    torch.manual_seed(77)
    eps = torch.randn(y.shape)
    # float64, on the im2col panel (no torch conv in the reference)
    ref, _, _ = lrt64(case.im2col(x.double()), case.im2col(x.double() ** 2), case.dense_w(layer.weight.mean.detach().double()),
                      case.dense_w(sigma64(layer.weight.scale.detach()) ** 2), layer.bias.mean.detach().double() if bias else None,
                      sigma64(layer.bias.scale.detach()) ** 2 if bias else None, case.rows(eps.double()))
    assert torch.allclose(case.rows(y.detach().double()), ref, atol=1e-5, rtol=1e-5)
    assert torch.equal(layer(x, sample=False), y)                  # the same noise again
    # unbatched, as NormalConvNd takes it: the same formula on the one image, on the reproduced noise
    torch.manual_seed(78)
    y1 = layer(x[0])
    assert y1.shape == (case.O,) + case.out
    torch.manual_seed(78)
    eps1 = torch.randn(y1.shape)
    ref1, _, _ = lrt64(case.im2col(x[:1].double()), case.im2col(x[:1].double() ** 2), case.dense_w(layer.weight.mean.detach().double()),
                       case.dense_w(sigma64(layer.weight.scale.detach()) ** 2), layer.bias.mean.detach().double() if bias else None,
                       sigma64(layer.bias.scale.detach()) ** 2 if bias else None, case.rows(eps1.double().unsqueeze(0)))
    assert torch.allclose(case.rows(y1.detach().double().unsqueeze(0)), ref1, atol=1e-5, rtol=1e-5)
    assert torch.equal(layer(x[0], sample=False), y1)
    with pytest.raises(RuntimeError):
        layer(x, sample=False)                                     # the recorded noise has another shape now


def test_cpu_expression_gradcheck():
    torch.manual_seed(2)
    layer = LocalReparamConv2d(2, 4, 3, stride=(2, 1), padding=(1, 0), groups=2).double()
    x = torch.randn(2, 2, 5, 4, dtype=torch.float64, requires_grad=True)
    layer(x)                                                       # records the noise

    def f(x, mw, rw, mb, rb):
        return torch.func.functional_call(layer, {"weight.mean": mw, "weight.scale": rw, "bias.mean": mb, "bias.scale": rb},
                                          (x, False))

    assert torch.autograd.gradcheck(f, (x, layer.weight.mean, layer.weight.scale, layer.bias.mean, layer.bias.scale))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("name", ["groups2", "peraxis", "1d", "3d"])
def test_backward_formulas_are_the_autograd_of_the_forward(name, shared, bias):
    """The explicit backward the GPU tests restate (g_m, g_v, the paired input- and weight-gradient contractions, the rho chain
    rule, the bias sums) IS float64 autograd of the formula; the batch holds an all-zero image (v = 0 there without a bias)."""
    case = CPU_CASES[name][0]
    torch.manual_seed(3)
    S = 3
    mu_w, rho_w, mu_b, rho_b = [None if t is None else t.double().requires_grad_() for t in case.params(bias, 5)]
    x = torch.randn(*((case.B,) if shared else (S, case.B)), case.C, *case.sp, dtype=torch.float64)
    x[(Ellipsis, 1) + (slice(None),) * (case.nd + 1)] = 0
    x.requires_grad_()
    eps = torch.randn(S, case.B, case.O, *case.out, dtype=torch.float64)
    gy = torch.randn_like(eps)
    y, _, v = formula64(case, x, mu_w, rho_w, mu_b, rho_b, eps)
    leaves = [t for t in (x, mu_w, rho_w, mu_b, rho_b) if t is not None]
    want = torch.autograd.grad((y * gy).sum(), leaves)
    flat = (lambda t: t) if shared else (lambda t: t.reshape(-1, *t.shape[2:]))
    with torch.no_grad():
        if not bias:
            assert (v[(Ellipsis, 1) + (slice(None),) * (case.nd + 1)] == 0).all()
        xd = x.detach()
        got = backward64(case, flat(xd), flat(xd * xd), flat(xd), mu_w, sigma64(rho_w) ** 2, rho_w, rho_b,
                         v if shared else flat(v), eps if shared else flat(eps), gy if shared else flat(gy), shared)
    for g, w in zip(got, want):
        assert torch.allclose(g.reshape(w.shape), w, atol=1e-12, rtol=1e-10)


def test_cpu_moments_and_weight_sampling_has_the_same():
    """Every output element's sample mean within 6 standard errors of m and |var / v - 1| <= 6 sqrt(2 / S), for this layer and for
    weight sampling (NormalConv2d) of the same posterior.  These are per-element MARGINALS only: weight sampling shares one
    filter bank between the positions of an image, so its cross-position covariance is not zero and this layer's is -- by design
    (the LRT-for-conv approximation)."""
    torch.manual_seed(0)
    S = 4096
    layer = LocalReparamConv2d(6, 8, 3, padding=1, bias=False).double()
    with torch.no_grad():
        layer.weight.mean.copy_(torch.randn(8, 6, 3, 3) * 0.1)
        layer.weight.scale.copy_(-3 + 0.3 * torch.randn(8, 6, 3, 3))
    x = torch.randn(4, 6, 5, 5, dtype=torch.float64)
    with torch.no_grad():
        mu, sig = layer.weight.mean, sigma64(layer.weight.scale)
        m, v = F.conv2d(x, mu, None, 1, 1), F.conv2d(x * x, sig * sig, None, 1, 1)
        ys = torch.stack([layer(x) for _ in range(S)])
        z = ((ys.mean(0) - m).abs() / (v / S).sqrt()).max().item()
        r = (ys.var(0, unbiased=True) / v - 1).abs().max().item()
        print("LRT conv: worst mean %.2f standard errors, worst |var / v - 1| %.3f (bound %.3f)" % (z, r, 6 * (2 / S) ** 0.5))
        assert z <= 6 and r <= 6 * (2 / S) ** 0.5
        normal = NormalConv2d(6, 8, 3, padding=1, bias=False).double()
        normal.load_state_dict(layer.state_dict())
        yw = torch.stack([normal(x) for _ in range(S)])
        z2 = ((yw.mean(0) - m).abs() / (v / S).sqrt()).max().item()
        r2 = (yw.var(0, unbiased=True) / v - 1).abs().max().item()
        print("weight sampling: worst mean %.2f standard errors, worst |var / v - 1| %.3f" % (z2, r2))
        assert z2 <= 6 and r2 <= 6 * (2 / S) ** 0.5


def test_lrt_conv_kernels_do_not_spill():
    """The paired-contraction conv tile has 3 uses (forward, input gradient, weight gradient) x 2 compute modes = 6 instantiations;
    each keeps both accumulator sets in registers, and the slab reduce (one instantiation per posterior's chain factor: 2) and the
    bias sums use no scratch either."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    tiles = {n: f for n, f in kernels.items() if re.match(r"_ZN3bnn12k_lrt_conv3dI[tf]Li[012]EEEvNS_9Conv3dGeoENS_11LrtConvArgsE$", n)}
    assert len(tiles) == 6, sorted(kernels)
    rest = {n: f for n, f in kernels.items()
            if re.match(r"_ZN3bnn(15k_lrt_conv_wsumINS_(8ChainRho|14ChainLogSigma2)EEEv|20k_lrt_conv_bias_gradE)", n)}
    assert len(rest) == 3, sorted(kernels)
    for n, f in {**tiles, **rest}.items():
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("private_segment_fixed_size", 0)) == 0, (n, f)


def test_lrt_conv_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one, odd, al4 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)
    r = _lib.Rng(seed=1, stream=5)
    rr = ctypes.byref(r)

    def shape(B=2, C=4, D=1, H=5, W=5, O=6, k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1), d=(1, 1, 1), g=1):
        return ctypes.byref(_lib.Conv3dShape(B, C, D, H, W, O, *k, *s, *p, *d, g))

    ok = shape()
    fwd, dgr, wgr, wsb = (lib.bnn_conv3d_lrt_forward, lib.bnn_conv3d_lrt_backward_input, lib.bnn_conv3d_lrt_backward_weight,
                          lib.bnn_conv3d_lrt_backward_weight_workspace_bytes)
    big = 1 << 30
    # ---- forward
    assert fwd(None, 0, one, one, None, None, one, None, ok, 1, rr, 0, None) == -1
    assert fwd(one, 0, one, one, None, None, one, None, None, 1, rr, 0, None) == -1               # no shape
    assert fwd(one, 0, one, one, one, None, one, None, ok, 1, rr, 0, None) == -1                  # mu_b without s2_b
    assert fwd(one, 0, one, one, None, None, one, None, ok, 1, None, 0, None) == -1               # no rng
    assert fwd(one, 0, one, one, None, None, one, None, shape(g=3), 1, rr, 0, None) == -2         # groups does not divide C, O
    assert fwd(one, 0, one, one, None, None, one, None, shape(k=(1, 9, 9), p=(0, 0, 0)), 1, rr, 0, None) == -2
    assert fwd(one, -4, one, one, None, None, one, None, ok, 1, rr, 0, None) == -2
    assert fwd(odd, 0, one, one, None, None, one, None, ok, 1, rr, 0, None) == -4
    assert fwd(one, 0, one, one, None, None, al4, None, ok, 1, rr, 0, None) == -4                 # y: 16 bytes
    assert fwd(one, 0, one, one, None, None, one, al4, ok, 1, rr, 0, None) == -4                  # v: 16 bytes
    assert fwd(one, 0, one, one, None, None, one, None, ok, 1, rr, 7, None) == -3                 # compute mode
    assert fwd(one, 0, one, one, None, None, one, None, shape(B=1 << 16, C=1 << 8, H=16, W=16), 1, rr, 0, None) == -5
    assert b"2^31" in lib.bnn_last_error()
    assert fwd(one, 0, one, one, None, None, one, None, shape(B=1 << 20, C=1, H=1, W=1, O=1 << 12, k=(1, 1, 1), p=(0, 0, 0)), 1, rr, 0, None) == -5
    assert fwd(one, 0, one, one, None, None, one, None, shape(g=2), 40000, rr, 0, None) == -5     # nsamples * groups > 65535
    bad = _lib.Rng(seed=1, stream=70000)
    assert fwd(one, 0, one, one, None, None, one, None, ok, 1, ctypes.byref(bad), 0, None) == -5
    # ---- input gradient
    assert dgr(one, None, one, one, one, one, ok, 1, 0, None) == -1
    assert dgr(one, one, one, one, one, None, ok, 1, 0, None) == -1
    assert dgr(one, one, one, one, one, one, shape(g=3), 1, 0, None) == -2
    assert dgr(one, one, one, one, one, odd, ok, 1, 0, None) == -4
    assert dgr(one, one, one, one, one, one, ok, 1, 9, None) == -3
    assert dgr(one, one, one, one, one, one, ok, 0, 0, None) == -2
    assert dgr(one, one, one, one, one, one, shape(B=1 << 16, C=1 << 8, H=16, W=16), 1, 0, None) == -5
    assert dgr(one, one, one, one, one, one, shape(g=2), 40000, 0, None) == -5
    # ---- weight gradient and its workspace query
    need = wsb(ok, 1)
    assert need > 0 and wsb(shape(g=3), 1) == -1 and wsb(shape(B=1 << 16, C=1 << 8, H=16, W=16), 1) == -1
    assert wgr(None, one, one, one, one, one, None, None, None, ok, 1, 0, one, big, None) == -1
    assert wgr(one, one, one, one, one, None, None, None, None, ok, 1, 0, one, big, None) == -1
    assert wgr(one, one, one, one, one, one, one, one, None, ok, 1, 0, one, big, None) == -1      # partial bias
    assert wgr(one, one, one, one, one, one, None, None, None, shape(g=3), 1, 0, one, big, None) == -2
    assert wgr(one, one, one, one, odd, one, None, None, None, ok, 1, 0, one, big, None) == -4
    assert wgr(one, one, one, one, one, one, None, None, None, ok, 1, 5, one, big, None) == -3
    assert wgr(one, one, one, one, one, one, None, None, None, shape(g=2), 40000, 0, one, big, None) == -5
    assert wgr(one, one, one, one, one, one, None, None, None, ok, 1, 0, one, need - 4, None) == -6   # workspace too small
    assert wgr(one, one, one, one, one, one, None, None, None, ok, 1, 0, None, 0, None) == -6
    assert lib.bnn_launch_count() == n0
    # the Python layer reports the same refusals with the reason, before anything is launched
    why = ops.conv_lrt_eligible(torch.empty(1).expand(1 << 16, 1 << 8, 16, 16), torch.empty(6, 1 << 8, 3, 3), 1, True,
                                (1, 1), (1, 1), (1, 1), 1)
    assert why is not None and "2^31" in why
    assert "channels" in ops.conv_lrt_eligible(torch.empty(2, 5, 8, 8), torch.empty(6, 4, 3, 3), 1, True, (1, 1), (1, 1), (1, 1), 1)
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


def conv_eps(key, S, case, dev):
    """The key's eps for S samples in the contract's order: (S, B, O, *out)."""
    return twin_eps(key, S, (case.B, case.O * case.P), dev).reshape(S, case.B, case.O, *case.out)


def operands64(case, x, mu_w, rho_w, mu_b, rho_b, mode, dev):
    """float64 operands as the kernel contracts them: (x, x^2, mu_w, sigma_w^2, mu_b, sigma_b^2)."""
    want_w = sigma64(rho_w) ** 2
    want_b = sigma64(rho_b) ** 2 if rho_b is not None else None
    if mode == "f32":
        return x.double(), x.double() ** 2, mu_w.double(), want_w, None if mu_b is None else mu_b.double(), want_b
    # bf16: the kernel rounds the fp32 sigma^2 of bnn_lrt_prepare as it enters LDS -- take the device's fp32 value (checked
    # against float64 here), so that the reference rounds what the kernel rounds
    s2_w, s2_b = ops._lrt_prepare_raw(rho_w.to(dev), None if rho_b is None else rho_b.to(dev))
    s2_w = s2_w.cpu()
    assert ((s2_w.double() - want_w).abs() <= 1e-6 * want_w).all()
    if rho_b is not None:
        s2_b = s2_b.cpu()
        assert ((s2_b.double() - want_b).abs() <= 1e-6 * want_b).all()
    return (rne_bf16(x), rne_bf16(x.float() * x.float()), rne_bf16(mu_w), rne_bf16(s2_w),
            None if mu_b is None else mu_b.double(), None if rho_b is None else s2_b.double())


def run_lrt(case, x, params, key, shared, mode, dev):
    mu_w, rho_w, mu_b, rho_b = params
    return ops.convNd_lrt(x, mu_w, rho_w, mu_b, rho_b, key, shared, *case.geo, mode)


FWD_CASES = {
    "lenet": Case(5, 64, (6, 6), 64, 3, 2, 1),                                       # (B, 64, 6, 6) -> 64, k3 s2 p1: P = 9
    "cifar": Case(3, 128, (4, 4), 128, 3, 1, 1),                                     # (B, 128, 4, 4) -> 128, k3 p1: P = 16
    "peraxis2d": Case(3, 5, (9, 11), 7, (3, 2), (2, 1), (1, 2), (1, 2)),             # P = 5 x 13 = 65, B P = 195
    "groups2": Case(4, 6, (7, 7), 10, 3, 1, 1, 1, 2),
    "1d": Case(4, 6, (19,), 9, 5, 2, 2),
    "3d": Case(2, 4, (5, 6, 7), 6, (2, 3, 2), (1, 2, 1), (1, 0, 1), (2, 1, 1)),      # P = 5 x 2 x 8 = 80
    "1x1": Case(3, 16, (5, 5), 12, 1),
}


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("S", [1, 4, 8, 33])
@pytest.mark.parametrize("name", sorted(FWD_CASES))
def test_forward_matches_float64_on_the_keys_eps(dev, name, S, shared, bias, mode):
    assert FWD_CASES["peraxis2d"].P % 2 == 1 and (FWD_CASES["peraxis2d"].B * FWD_CASES["peraxis2d"].P) % 64 != 0
    check_forward(dev, FWD_CASES[name], name, S, shared, bias, mode)


def check_forward(dev, case, name, S, shared, bias, mode):
    """One forward of `case` (named `name` in messages) against float64 on the key's eps, every element."""
    params = case.params(bias, 11)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(*((case.B,) if shared else (S, case.B)), case.C, *case.sp, generator=g)
    key = DrawKey(0x1234567890ABCDEF, 321, 3, S, 17, gen=_rng.generator_for(mode))          # sample0 = 3
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    y = run_lrt(case, x.to(dev), [None if t is None else t.to(dev) for t in params], key, shared, mode, dev)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 2            # the sigma^2 launch + ONE contraction launch for all S samples
    assert y.shape == (S, case.B, case.O) + case.out and y.dtype == torch.float32
    x64, xsq, mu64, s2, mb, s2b = operands64(case, x, *params, mode, dev)
    eps = case.rows(conv_eps(key, S, case, dev))
    flat = (lambda t: t) if shared else (lambda t: t.reshape(-1, *t.shape[2:]))
    col, colsq = case.im2col(flat(x64)), case.im2col(flat(xsq))
    if not shared:
        col, colsq = col.reshape(S, -1, col.shape[-1]), colsq.reshape(S, -1, col.shape[-1])
    mu2 = case.dense_w(mu64)
    ref, _, v = lrt64(col, colsq, mu2, case.dense_w(s2), mb, s2b, eps)
    assert_within(case.rows(y), ref, forward_bound(mode, col, mu2, mb, ref, v, eps, case.K), "y %s S=%d %s" % (name, S, mode))


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["lenet", "3d", "groups2"])
def test_shared_and_per_sample_inputs_and_repeated_calls_give_the_same_bits(dev, name, mode):
    case, S = FWD_CASES[name], 4
    params = [t.to(dev).requires_grad_() for t in case.params(True, 21)]
    x = torch.randn(case.B, case.C, *case.sp, device=dev).requires_grad_()
    xs = x.detach().unsqueeze(0).repeat(S, *([1] * x.dim())).requires_grad_()
    key = DrawKey(99, 7, 2, S, 5, gen=_rng.generator_for(mode))
    a = run_lrt(case, x, params, key, True, mode, dev)
    b = run_lrt(case, xs, params, key, False, mode, dev)
    c = run_lrt(case, x, params, key, True, mode, dev)
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
    layer = LocalReparamConv2d(6, 8, 3, padding=1).to(dev)
    x = torch.randn(5, 6, 7, 7, device=dev)
    bnn.manual_seed(5)
    with pytest.raises(RuntimeError):
        layer(x, sample=False)                         # nothing recorded yet
    y0 = layer(x)
    k0 = layer.noise_key
    assert y0.shape == (5, 8, 7, 7) and y0.dtype == torch.float32 and torch.isfinite(y0).all()
    assert (k0.stream, k0.sample0, k0.nsamples, k0.gen) == (layer._noise_stream, 0, 1, _rng.GEN_PHILOX10_U24)
    assert layer._noise_stream not in (layer.weight._stream, layer.bias._stream)
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
    bnn.set_compute("bf16")
    layer(x)
    assert layer.noise_key.gen == _rng.generator_for("bf16")
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    with pytest.raises(ops.BnnHipError):               # no torch fallback
        ops.convNd_lrt(x.double(), layer.weight.mean, layer.weight.scale, None, None, k0, True, (1, 1), (1, 1), (1, 1), 1, "f32")
    with pytest.raises(ops.BnnHipError, match="channels"):
        ops.convNd_lrt(x[:, :5], layer.weight.mean, layer.weight.scale, None, None, k0, True, (1, 1), (1, 1), (1, 1), 1, "f32")
    assert lib.bnn_launch_count() == n0
    l1, l3 = LocalReparamConv1d(6, 4, 3).to(dev), LocalReparamConv3d(6, 4, 2).to(dev)
    for layer_n, xn, shape in ((l1, torch.randn(2, 6, 9, device=dev), (2, 4, 7)), (l3, torch.randn(2, 6, 4, 4, 4, device=dev), (2, 4, 3, 3, 3))):
        assert layer_n(xn).shape == shape
        yu = layer_n(xn[0])
        assert yu.shape == shape[1:] and torch.isfinite(yu).all()
        assert torch.equal(layer_n(xn[:1], sample=False)[0], yu)


BWD_CASES = {
    "strided": Case(4, 8, (6, 6), 8, 3, 2, 1),
    "dilated": Case(3, 5, (9, 8), 6, 3, 1, 2, 2),
    "groups2": Case(4, 6, (7, 7), 10, 3, 1, 1, 1, 2),
    "3d": Case(2, 4, (5, 6, 7), 6, (2, 3, 2), (1, 2, 1), (1, 0, 1), (2, 1, 1)),
}


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("name", sorted(BWD_CASES))
def test_backward_matches_float64_on_the_keys_eps(dev, name, S, shared, bias, mode):
    """All five gradients, every element; image 1 of the batch is all zero (v = sigma_b^2 there, and v = 0 without bias)."""
    check_backward(dev, BWD_CASES[name], name, S, shared, bias, mode)


def check_backward(dev, case, name, S, shared, bias, mode):
    """One backward of `case` (named `name` in messages) against float64 on the key's eps -> the device's gradients."""
    params = case.params(bias, 31)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(*((case.B,) if shared else (S, case.B)), case.C, *case.sp, generator=g)
    x[(Ellipsis, 1) + (slice(None),) * (case.nd + 1)] = 0
    gy = torch.randn(S, case.B, case.O, *case.out, generator=g)
    key = DrawKey(777, 45, 1, S, 9, gen=_rng.generator_for(mode))
    leaves = [None if t is None else t.to(dev).requires_grad_() for t in (x,) + params]
    lib = _lib.load()
    y = run_lrt(case, leaves[0], leaves[1:], key, shared, mode, dev)
    n0 = lib.bnn_launch_count()
    got = torch.autograd.grad(y, [t for t in leaves if t is not None], gy.to(dev))
    torch.cuda.synchronize()
    # g_m / g_v, the paired input gradient, the paired weight-gradient slabs and their reduce, the bias sums: nothing else ran
    assert lib.bnn_launch_count() == n0 + (5 if bias else 4)
    assert all(torch.isfinite(t).all() for t in got)
    mu_w, rho_w, mu_b, rho_b = params
    eps = conv_eps(key, S, case, dev)
    names = ["x", "weight.mean", "weight.scale"] + (["bias.mean", "bias.scale"] if bias else [])
    if mode == "f32":
        ref = [t.double().requires_grad_() for t in (x,) + params if t is not None]
        p64 = ref[1:] + ([None, None] if not bias else [])
        yr, _, _ = formula64(case, ref[0], *p64, eps)
        want = torch.autograd.grad((yr * gy.double()).sum(), ref)
        for n, a, w in zip(names, got, want):
            assert_within(a, w, scaled_bound(w), "g %s %s S=%d f32" % (n, name, S))
        return got
    x64, xsq, mu64, s2, mb, s2b = operands64(case, x, mu_w, rho_w, mu_b, rho_b, mode, dev)
    v = case.conv(xsq, s2, s2b)                                          # every term >= 0: v is its own sum |a| |b|
    gy64 = gy.double()
    # device deviations before g_m / g_v are rounded to bf16: v (the forward's accumulation bound), 1 / (2 sqrt(.)), eps, the
    # products and the fp32 sum over the samples (test_lrt_device's construction, K = (C / groups) taps)
    rel_inv = 1.01 * 0.5 * gamma(case.K + 1) * v / (v + 1e-16) + 4 * U
    inv = 0.5 / torch.sqrt(v + 1e-16)
    term = gy64.abs() * inv * (eps.abs() * (rel_inv + 3 * U) + EPS_TWIN)
    if shared:
        beta_m = gamma(S) * gy64.abs().sum(0)
        beta_v = 1.01 * (term.sum(0) + gamma(S) * (gy64 * eps).abs().sum(0) * inv)
    else:
        beta_m, beta_v = torch.zeros_like(gy64), 1.01 * term
    flat = (lambda t: t) if shared else (lambda t: t.reshape(-1, *t.shape[2:]))
    want = backward64(case, flat(x64), flat(xsq), flat(x.double()), mu64, s2, rho_w, rho_b if bias else None,
                      v if shared else flat(v), eps if shared else flat(eps), gy64 if shared else flat(gy64), shared,
                      rnd=lambda t, beta: round_hidden(t, beta)[:2], betas=(flat(beta_m), flat(beta_v)))
    for n, a, (w, bound) in zip(names, got, want):
        assert_within(a.reshape(w.shape), w, bound + 1e-30, "g %s %s S=%d bf16" % (n, name, S))
    return got


@gpu
@pytest.mark.parametrize("gen", [0, 1])
def test_device_moments(dev, gen):
    torch.manual_seed(0)
    case, S = Case(4, 6, (5, 5), 8, 3, 1, 1), 512
    mu_w, rho_w = torch.randn(8, 6, 3, 3) * 0.1, -3 + 0.3 * torch.randn(8, 6, 3, 3)
    x = torch.randn(case.B, case.C, *case.sp)
    n0 = _lib.load().bnn_launch_count()
    ys = ops.convNd_lrt(x.to(dev), mu_w.to(dev), rho_w.to(dev), None, None, DrawKey(2024, 9, 0, S, 3, gen=gen), True, *case.geo,
                        "f32").double().cpu()
    assert _lib.load().bnn_launch_count() == n0 + 2
    assert torch.isfinite(ys).all()
    m, v = case.conv(x.double(), mu_w.double()), case.conv(x.double() ** 2, sigma64(rho_w) ** 2)
    z = ((ys.mean(0) - m).abs() / (v / S).sqrt()).max().item()
    r = (ys.var(0, unbiased=True) / v - 1).abs().max().item()
    print("device gen %d: worst mean %.2f standard errors, worst |var / v - 1| %.3f (bound %.3f)" % (gen, z, r, 6 * (2 / S) ** 0.5))
    assert z <= 6 and r <= 6 * (2 / S) ** 0.5


def net64(net, x, S, dev):
    """The serial float64 restatement on the recorded noise keys, the noise read from the device stream of each key
    (ops.eps_philox: the stream the forward test ties to the CPU twin), so that the twin's 2e-5 does not compound."""
    outs = []
    for s in range(S):
        h = x.double().cpu()
        for layer in net.layers:
            if isinstance(layer, (LocalReparamConv2d, LocalReparamLinear)):
                conv = isinstance(layer, LocalReparamConv2d)
                args = (layer.stride, layer.padding, layer.dilation, layer.groups) if conv else ()
                op = F.conv2d if conv else F.linear
                mu, s2 = layer.weight.mean.detach().double().cpu(), sigma64(layer.weight.scale.detach().cpu()) ** 2
                mb, s2b = layer.bias.mean.detach().double().cpu(), sigma64(layer.bias.scale.detach().cpu()) ** 2
                m, v = op(h, mu, mb, *args), op(h * h, s2, s2b, *args)
                eps = ops.eps_philox((m.numel(),), layer.noise_key, dev)[s].reshape(m.shape).double().cpu()
                h = m + torch.sqrt(v + 1e-16) * eps
            elif isinstance(layer, torch.nn.Flatten):
                h = h.flatten(1)
            else:
                h = h.clamp_min(0)
        outs.append(h)
    return torch.stack(outs)


@gpu
def test_network_forward_predictive_and_training_step(dev):
    torch.manual_seed(6)
    S, B = 4, 8
    net = ConvNet(S).to(dev)
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
    # per LRT layer: the sigma^2 launch + ONE contraction launch (the first sees the shared batch, the others S B rows); ReLU and
    # Flatten launch nothing of this library's
    assert [b - a for a, b in zip(counts, counts[1:])] == [2, 0, 2, 0, 2] and lib.bnn_launch_count() == n0 + 6
    lrt = [l for l in net.layers if hasattr(l, "noise_key")]
    keys = [l.noise_key for l in lrt]
    assert [k.nsamples for k in keys] == [S] * 3 and len({k.stream for k in keys}) == 3
    assert torch.isfinite(ys).all()
    want = net64(net, x, S, dev)
    assert_within(ys, want, scaled_bound(want), "conv-conv-linear LRT net")
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
    assert lib.bnn_launch_count() >= n1 + 6 + 4 + 5 + 4          # forward; the conv backwards (the first has no input gradient), the linear one
    assert len(before) == 12
    for p, b in zip(net.parameters(), before):
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), b)
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_sharded_pass_reproduces_its_rows(dev, mode):
    torch.manual_seed(7)
    bnn.set_compute(mode)
    net = ConvNet(8).to(dev)
    net.mc_batched = True
    x = torch.randn(6, 3, 7, 7, device=dev)
    with torch.no_grad():
        bnn.manual_seed(55)
        full = net.forward_stacked(x, 8)
        bnn.manual_seed(55)
        lo = net.forward_stacked(x, 4, sample0=0)
        bnn.manual_seed(55)
        hi = net.forward_stacked(x, 4, sample0=4)
    assert net.layers[0].noise_key.sample0 == 4
    assert torch.isfinite(full).all()
    assert torch.equal(lo, full[:4]) and torch.equal(hi, full[4:])
