"""Evidential regression in HIP (K13): the Normal-Inverse-Gamma head's activation (bnn_nig_head_forward / _backward, ops.nig_head,
NormalInverseGaussianLinear), its loss with the four gradients in one pass (bnn_nig_loss, ops.nig_loss,
NormalInverseGaussianLoss), the MC-mixture uncertainty (bnn_mc_evidential, ops.mc_evidential, ops.evidential_f64,
BayesianNetworkModule.predictive_evidential) and a tuple-valued head on the batched MC pass.

CPU: the C-ABI entries and their argument errors, the unchanged CPU paths of layer and loss, the float64 CPU path against a NumPy
restatement, the fixture recorded from the reference (tests/golden/nig_evidential.npz, make_golden_evidential.py).
GPU: every kernel against float64 of the same formula.

Bounds.
  head: the outputs are expf, log1pf and two additions in fp32 (each library function within 2 ulp), the backward expf, an
        addition, a division and a product: below 8 ulp = 4.8e-7 relative.  Asserted: 1e-6 |ref| per element; gamma is a copy.
  loss: |loss - ref| <= 1e-5 max(1, |ref|) and, per gradient tensor, max|g - ref| <= 1e-5 max|ref| against float64 autograd of
        the reference expression -- the project's fp32-parity figure; the reference's own fp32 evaluation stays below 1.2e-7 /
        7.7e-7 on these measures over the three alpha ranges used here.
  mc:   mean 1e-6 max(1, |ref|), the others 1e-5 max(1, |ref|) (those of test_predictive_regression.py), epistemic >= 0."""
import copy
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import seeded
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd.nn import (BayesianNetworkModule, NormalInverseGaussianLinear, NormalInverseGaussianLoss,
                                           NormalInverseGaussianUncertainty, NormalLinear)
from conftest import ROOT, load_golden

gpu = pytest.mark.gpu
CORNERS = [-30.0, -1e-3, 19.5, 20.0, 20.5, 60.0]


def N(t):
    return t.detach().double().cpu().numpy()


class hip_switch:
    """ops.EVIDENTIAL_HIP set for a block."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = ops.EVIDENTIAL_HIP
        ops.EVIDENTIAL_HIP = self.on

    def __exit__(self, *exc):
        ops.EVIDENTIAL_HIP = self.was


# ------------------------------------------------------------------------------------------------- float64 restatements
def softplus64(z):
    z = np.asarray(z, np.float64)
    return np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0))))


def sigmoid64(z):
    z = np.asarray(z, np.float64)
    return np.where(z > 20.0, 1.0, 1.0 / (1.0 + np.exp(-z)))


def head64(z, D):
    z = np.asarray(z, np.float64)
    return (z[..., :D], 1e-10 + softplus64(z[..., D:2 * D]), 1.0 + 1e-10 + softplus64(z[..., 2 * D:3 * D]),
            1e-10 + softplus64(z[..., 3 * D:]))


def torch_expression(gamma, upsilon, alpha, beta, y, reg_lambda):
    """NormalInverseGaussianLoss.forward as the reference writes it (loss.py:54-69), in the tensors' own dtype."""
    penalty = torch.mean(torch.abs(y - gamma) * (2 * upsilon + alpha))
    omega = 2 * beta * (1 + upsilon)
    nll = (0.5 * torch.log(math.pi / upsilon) - alpha * torch.log(omega)
           + (alpha + 0.5) * torch.log(upsilon * (y - gamma) ** 2 + omega) + torch.lgamma(alpha) - torch.lgamma(alpha + 0.5))
    return nll.mean() + reg_lambda * penalty


def loss_ref64(ts, y, reg_lambda):
    """float64 autograd of the reference expression: (loss, [four gradients]) as NumPy."""
    leaves = [t.detach().double().cpu().requires_grad_() for t in ts]
    loss = torch_expression(*leaves, y.detach().double().cpu(), reg_lambda)
    loss.backward()
    return loss.item(), [N(t.grad) for t in leaves]


def check_loss(loss, grads, want, want_grads, what=""):
    """The issue's bound; prints each figure before it asserts."""
    err = abs(float(loss) - want)
    print(what, "loss", float(loss), "ref", want, "err", err)
    assert err <= 1e-5 * max(1.0, abs(want)), (what, "loss", float(loss), want)
    for name, g, r in zip(("gamma", "upsilon", "alpha", "beta"), grads, want_grads):
        if g is None:
            continue
        e, scale = np.abs(N(g).reshape(r.shape) - r).max(), np.abs(r).max()
        print(what, "g_" + name, "err", e, "max|ref|", scale, "ratio", e / scale if scale else 0.0)
        assert e <= 1e-5 * scale, (what, "g_" + name, e, scale)


def evi64(g, u, a, b):
    """NumPy float64: the mixture moments of (S, rows, D) head outputs -> mean, total, aleatoric, epistemic."""
    g, u, a, b = (np.asarray(t, np.float64) for t in (g, u, a, b))
    ale_s = b / (a - 1.0)
    mean = g.mean(0)
    ale = ale_s.mean(0)
    epi = (ale_s / u).mean(0) + ((g - mean) ** 2).mean(0)
    return mean, ale + epi, ale, epi


def check_mc(u, ref, what=""):
    got = [N(t).reshape(ref[0].shape) for t in u]
    for name, g, r, rel in zip(("mean", "total", "aleatoric", "epistemic"), got, ref, (1e-6, 1e-5, 1e-5, 1e-5)):
        e = np.abs(g - r) - rel * np.maximum(1.0, np.abs(r))
        assert e.max() <= 0, (what, name, float(np.abs(g - r).max()), float(np.abs(r).max()))
    assert got[3].min() >= 0, (what, "epistemic < 0", got[3].min())


def nig_inputs(shape, alpha_range, gen, device="cpu"):
    """gamma, y ~ N(0, 1); upsilon, beta uniform in [0.05, 4]; alpha - 1 log-uniform in alpha_range."""
    lo, hi = alpha_range
    r = lambda: torch.rand(shape, generator=gen, device=device)          # noqa: E731
    gamma = torch.randn(shape, generator=gen, device=device)
    upsilon, beta = 0.05 + 3.95 * r(), 0.05 + 3.95 * r()
    alpha = 1.0 + torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * r())
    y = torch.randn(shape, generator=gen, device=device)
    return gamma, upsilon, alpha, beta, y


class EviNet(BayesianNetworkModule):
    """dims[0] - hidden ... - NIG(dims[-1]); the trunk layers are NormalLinear (bayes) or torch.nn.Linear."""

    def __init__(self, dims, samples=4, bayes=True):
        super().__init__(dims[0], dims[-1], samples)
        mods = []
        for i in range(len(dims) - 2):
            mods += [(NormalLinear if bayes else torch.nn.Linear)(dims[i], dims[i + 1]), torch.nn.ReLU()]
        mods.append(NormalInverseGaussianLinear(dims[-2], dims[-1]))
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


# ------------------------------------------------------------------------------------------------------------------ CPU
ENTRIES = ("bnn_nig_head_forward", "bnn_nig_head_backward", "bnn_nig_loss", "bnn_nig_loss_workspace_bytes", "bnn_mc_evidential")


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b(int|int64_t) %s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.bnn_abi_version() == 2
    assert lib.bnn_nig_loss_workspace_bytes(1) == 8
    # the plan is a function of the extent alone: one fp64 partial per 256-element workgroup up to the ceiling of 1024
    # workgroups, a grid-stride loop takes what is above it
    assert lib.bnn_nig_loss_workspace_bytes(256) == 8 and lib.bnn_nig_loss_workspace_bytes(257) == 16
    assert lib.bnn_nig_loss_workspace_bytes(1024 * 256) == lib.bnn_nig_loss_workspace_bytes(1024 * 256 + 1) == 8 * 1024
    assert lib.bnn_nig_loss_workspace_bytes(10 ** 9) == lib.bnn_nig_loss_workspace_bytes(10 ** 8) == 8 * 1024
    for name in ("nig_head", "nig_loss", "mc_evidential", "evidential_f64"):
        assert callable(getattr(ops, name))
    assert ops.EVIDENTIAL_HIP is True
    assert callable(BayesianNetworkModule.predictive_evidential)


def test_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    n0 = lib.bnn_launch_count()

    def fwd(z=one, rows=8, D=3, gamma=one, upsilon=one, alpha=one, beta=one):
        return lib.bnn_nig_head_forward(z, rows, D, gamma, upsilon, alpha, beta, None)

    for k in ("z", "gamma", "upsilon", "alpha", "beta"):
        assert fwd(**{k: None}) == -1 and b"NULL" in lib.bnn_last_error()
    assert fwd(rows=0) == -2 and fwd(D=0) == -2
    assert fwd(D=4097) == -5 and fwd(rows=2 ** 31) == -5

    def bwd(z=one, rows=8, D=3, g_z=one):
        return lib.bnn_nig_head_backward(z, None, None, None, None, rows, D, g_z, None)

    assert bwd(z=None) == -1 and bwd(g_z=None) == -1
    assert bwd(rows=0) == -2 and bwd(D=0) == -2
    assert bwd(D=4097) == -5 and bwd(rows=2 ** 31) == -5

    def loss(n=8, **kw):
        a = dict(gamma=one, upsilon=one, alpha=one, beta=one, y=one, loss=one, ws=one)
        a.update(kw)
        return lib.bnn_nig_loss(a["gamma"], a["upsilon"], a["alpha"], a["beta"], a["y"], n, 0.01, a["loss"], None, None, None,
                                None, a["ws"], None)

    for k in ("gamma", "upsilon", "alpha", "beta", "y", "loss", "ws"):
        assert loss(**{k: None}) == -1
    assert loss(n=0) == -2 and loss(n=-1) == -2
    assert loss(ws=ctypes.c_void_p(20)) == -4
    assert lib.bnn_nig_loss_workspace_bytes(0) == 0

    def mc(nsamples=4, rows=8, D=3, stride=None, **kw):
        a = dict(gamma=one, upsilon=one, alpha=one, beta=one, mean=one, total=one, ale=one, epi=one)
        a.update(kw)
        return lib.bnn_mc_evidential(a["gamma"], a["upsilon"], a["alpha"], a["beta"], rows * D if stride is None else stride,
                                     nsamples, rows, D, a["mean"], a["total"], a["ale"], a["epi"], None)

    for k in ("gamma", "upsilon", "alpha", "beta", "mean", "total", "ale", "epi"):
        assert mc(**{k: None}) == -1
    for k in ("nsamples", "rows", "D"):
        assert mc(**{k: 0}) == -2
    assert mc(nsamples=65537) == -5 and b"65536" in lib.bnn_last_error()
    assert mc(D=4097) == -5
    assert mc(rows=2 ** 31) == -5
    assert mc(stride=23) == -2                                              # overlapping samples
    assert lib.bnn_launch_count() == n0


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    with pytest.raises(_lib.BnnHipError):
        ops.nig_head(torch.zeros(5, 12), 3)
    five = [torch.ones(5, 3) * 2 for _ in range(5)]
    with pytest.raises(_lib.BnnHipError):
        ops.nig_loss(*five, 1e-2)
    with pytest.raises(_lib.BnnHipError):
        ops.mc_evidential(*[torch.ones(2, 5, 3) * 2 for _ in range(4)])
    with pytest.raises(ValueError):
        ops.evidential_f64(torch.ones(2, 5, 3), torch.ones(2, 5, 3), torch.ones(2, 5, 3), torch.ones(2, 5, 2))
    with pytest.raises(ValueError):
        ops.evidential_f64(*[torch.ones(3) for _ in range(4)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_paths_of_layer_and_loss_are_the_torch_expressions_bit_for_bit(dtype):
    torch.manual_seed(0)
    head = NormalInverseGaussianLinear(7, 3).to(dtype)
    x = torch.randn(11, 7, dtype=dtype)
    x[0, 0] = 60.0
    y = torch.randn(11, 3, dtype=dtype)
    sp = torch.nn.functional.softplus
    for on in (True, False):
        with hip_switch(on):
            xa = x.clone().requires_grad_()
            got = head(xa)
            loss = NormalInverseGaussianLoss(0.02)(*got, y)
            loss.backward()
            xb = x.clone().requires_grad_()
            g, u, a, b = torch.split(head.linear(xb), 3, dim=-1)
            want = (g, 1e-10 + sp(u), 1 + 1e-10 + sp(a), 1e-10 + sp(b))
            want_loss = torch_expression(*want, y, 0.02)
            want_loss.backward()
            for s, t in zip(got, want):
                assert s.dtype == dtype and torch.equal(s, t)
            assert torch.equal(loss, want_loss) and torch.equal(xa.grad, xb.grad)
            d = head(x, sample=True)
            assert isinstance(d, torch.distributions.Normal) and torch.equal(d.loc, want[0].detach())
            assert torch.equal(d.scale, torch.sqrt(want[3] / (want[1] * (want[2] - 1))).detach())


def test_evidential_f64_against_numpy_and_the_cpu_module_path():
    gen = torch.Generator().manual_seed(6)
    g, u, a, b, _ = nig_inputs((5, 4, 7, 3), (1e-3, 50.0), gen)
    got = ops.evidential_f64(g, u, a, b)
    assert isinstance(got, ops.PredictiveRegression) and all(t.shape == (4, 7, 3) and t.dtype == torch.float32 for t in got)
    for s, r in zip(got, evi64(g.numpy(), u.numpy(), a.numpy(), b.numpy())):
        assert np.allclose(N(s), r, rtol=2e-7, atol=0)                      # float64 inside, rounded once to float32
    one = ops.evidential_f64(g[:1], u[:1], a[:1], b[:1])                     # S = 1: the module's two outputs and gamma
    ale, epi = NormalInverseGaussianUncertainty()(u[0].double(), a[0].double(), b[0].double())
    assert torch.equal(one.mean, g[0]) and torch.equal(one.aleatoric, ale.float()) and torch.equal(one.epistemic, epi.float())
    # the module on CPU: the serial loop's tuples, stacked
    torch.manual_seed(1)
    net = EviNet([2, 16, 16, 2], samples=4)
    x = torch.randn(5, 2)
    torch.manual_seed(3)
    out = net(x)
    assert isinstance(out, list) and len(out) == 4 and all(isinstance(o, tuple) and len(o) == 4 for o in out)
    torch.manual_seed(3)
    p = net.predictive_evidential(x)
    want = ops.evidential_f64(*[torch.stack([o[k] for o in out]) for k in range(4)])
    for s, t in zip(p, want):
        assert s.shape == (5, 2) and torch.equal(s, t)
    assert float(p.epistemic.min()) > 0

    class Plain(BayesianNetworkModule):
        def _forward(self, x):
            return x

    with pytest.raises(ValueError):
        Plain(2, 2, 2).predictive_evidential(x)


@pytest.fixture(scope="module")
def fixture():
    return load_golden("nig_evidential")


def _identity_head(D, dtype, device="cpu"):
    head = NormalInverseGaussianLinear(4 * D, D).to(dtype)
    with torch.no_grad():
        head.linear.weight.copy_(torch.eye(4 * D, dtype=dtype))
        head.linear.bias.zero_()
    return head.to(device)


def _check_fixture(fx, device):
    """Our layer + loss + uncertainty on the fixture's z and y against the reference's float64 record (and its float32 one)."""
    D, lam = int(fx["D"]), float(fx["reg_lambda"])
    assert fx["z"].shape == (37, 12) and D == 3 and fx["z"].dtype == np.float32
    head = _identity_head(D, torch.float32, device)
    z = torch.from_numpy(fx["z"]).to(device).requires_grad_()
    outs = head(z)
    loss = NormalInverseGaussianLoss(lam)(*outs, torch.from_numpy(fx["y"]).to(device))
    loss.backward()
    for name, t in zip(("gamma", "upsilon", "alpha", "beta"), outs):
        r = fx[name + "_f64"]
        assert (np.abs(N(t) - r) <= 1e-6 * np.abs(r)).all(), name
        assert np.allclose(N(t), fx[name + "_f32"], rtol=1e-6, atol=0), name
    want, want_g = float(fx["loss_f64"]), fx["g_z_f64"]
    assert abs(loss.item() - want) <= 1e-5 * max(1.0, abs(want)), (loss.item(), want)
    assert np.abs(N(z.grad) - want_g).max() <= 1e-5 * np.abs(want_g).max()
    # the uncertainty on the reference's own float32 head outputs (beta / (alpha - 1) magnifies a last-bit difference in alpha
    # by 1 / (alpha - 1), and alpha is exactly 1 at the -30 corner: the record holds inf there)
    rec = [torch.from_numpy(fx[k + "_f32"]).to(device) for k in ("gamma", "upsilon", "alpha", "beta")]
    ale, epi = NormalInverseGaussianUncertainty()(*rec[1:])
    for name, t in (("aleatoric", ale), ("epistemic", epi)):
        assert np.isinf(fx[name + "_f32"]).any()
        assert np.allclose(N(t), fx[name + "_f32"], rtol=1e-6, atol=0), name
    return rec, ale, epi


def test_fixture_from_the_reference_against_the_cpu_path(fixture):
    for k in ("gamma", "upsilon", "alpha", "beta", "loss", "g_z", "aleatoric", "epistemic"):
        assert fixture[k + "_f32"].dtype == np.float32 and fixture[k + "_f64"].dtype == np.float64
    z = fixture["z"]
    for c in CORNERS:
        assert (z == np.float32(c)).sum() >= 3                               # every softplus corner, in each segment
    rec, ale, epi = _check_fixture(fixture, "cpu")
    one = ops.evidential_f64(*[t.unsqueeze(0) for t in rec])
    assert torch.equal(one.mean, rec[0])
    assert np.allclose(N(one.aleatoric), fixture["aleatoric_f32"], rtol=1e-6, atol=0)
    assert np.allclose(N(one.epistemic), fixture["epistemic_f32"], rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------------------------ GPU
DEV = torch.device("cuda:0")


def _head_zs(rows, D, gen):
    """Pre-activations N(0, 3^2) that together hold every softplus corner in a softplus segment (columns D .. 4 D - 1): one
    tensor where its rows * 3 D such slots can take the six corners, else as many tensors as it takes."""
    slots = [(r, c) for r in range(rows) for c in range(D, 4 * D)]
    zs, todo = [], list(CORNERS) * (3 if len(slots) >= 18 else 1)
    while todo:
        z = torch.randn(rows, 4 * D, generator=gen) * 3.0
        take, todo = todo[:len(slots)], todo[len(slots):]
        step = len(slots) // len(take)
        for j, c in enumerate(take):
            r, col = slots[j * step]
            z[r, col] = c
        zs.append(z)
    assert all(any((z[:, D:] == c).any() for z in zs) for c in CORNERS)
    return zs


@gpu
@pytest.mark.parametrize("D", [1, 3, 16, 17])
@pytest.mark.parametrize("rows", [1, 37, 257])
def test_head_forward_and_backward_against_float64(rows, D):
    gen = torch.Generator().manual_seed(rows * 100 + D)
    zs = _head_zs(rows, D, gen)
    gs = [torch.randn(rows, D, generator=gen) for _ in range(4)]
    lib = _lib.load()
    for z in reversed(zs):                                                  # (the last one checked is zs[0]: used below)
        zd = z.to(DEV).requires_grad_()
        n0 = lib.bnn_launch_count()
        outs = ops.nig_head(zd, D)
        assert lib.bnn_launch_count() == n0 + 1
        want = head64(z.numpy(), D)
        assert torch.equal(outs[0], zd.detach()[:, :D])
        for t, r in zip(outs, want):
            assert t.shape == (rows, D) and t.is_contiguous()
            assert (np.abs(N(t) - r) <= 1e-6 * np.abs(r)).all(), float((np.abs(N(t) - r) / np.abs(r)).max())
        # the whole backward through autograd: one launch
        n0 = lib.bnn_launch_count()
        full = torch.autograd.grad(sum((o * g.to(DEV)).sum() for o, g in zip(outs, gs)), zd, retain_graph=True)[0]
        assert lib.bnn_launch_count() == n0 + 1
        ref = np.concatenate([N(g) for g in gs], -1)
        ref[:, D:] *= sigmoid64(z.numpy())[:, D:]
        assert (np.abs(N(full) - ref) <= 1e-6 * np.abs(ref) + 1e-30).all()
    # the backward with each subset of the incoming gradients absent, through the C-ABI
    sig = sigmoid64(z.numpy())
    gd = [g.to(DEV) for g in gs]
    gz = torch.empty_like(zd.detach())
    for present in itertools.product((False, True), repeat=4):
        n0 = lib.bnn_launch_count()
        _lib.check(lib.bnn_nig_head_backward(_lib.ptr(zd.detach()), *[_lib.ptr(g) if p else None for g, p in zip(gd, present)],
                                             rows, D, _lib.ptr(gz), _lib.stream_ptr(DEV)), "bnn_nig_head_backward")
        assert lib.bnn_launch_count() == n0 + 1
        ref = np.concatenate([(N(g) if p else np.zeros((rows, D))) for g, p in zip(gs, present)], -1)
        ref[:, D:] *= sig[:, D:]
        assert (np.abs(N(gz) - ref) <= 1e-6 * np.abs(ref) + 1e-30).all(), present
        for k, p in enumerate(present):
            if not p:
                assert float(gz[:, k * D:(k + 1) * D].abs().max()) == 0
    # autograd: only gamma and alpha are used -> one launch, the other two segments exactly zero
    n0 = lib.bnn_launch_count()
    ((outs[0] * gd[0]).sum() + (outs[2] * gd[2]).sum()).backward()
    assert lib.bnn_launch_count() == n0 + 1
    ref = np.concatenate([N(gs[0]), np.zeros((rows, D)), N(gs[2]) * sig[:, 2 * D:3 * D], np.zeros((rows, D))], -1)
    assert (np.abs(N(zd.grad) - ref) <= 1e-6 * np.abs(ref) + 1e-30).all()
    # leading dims, and the layer
    z3 = z.to(DEV).view(1, rows, 4 * D)
    for s, t in zip(ops.nig_head(z3, D), outs):
        assert s.shape == (1, rows, D) and torch.equal(s[0], t)


@gpu
def test_fixture_from_the_reference_against_the_device_path(fixture):
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    rec, ale, epi = _check_fixture(fixture, DEV)
    assert lib.bnn_launch_count() == n0 + 4                                 # head forward, loss (2), head backward
    one = ops.mc_evidential(*[t.unsqueeze(0) for t in rec])
    assert torch.equal(one.mean, rec[0]) and torch.equal(one.aleatoric, ale) and torch.equal(one.epistemic, epi)
    assert torch.equal(one.total, (ale.double() + epi.double()).float())


ALPHA_RANGES = [(1e-3, 50.0), (1e3, 1e5), (1e5, 1e6)]
LOSS_SHAPES = [(1, 1), (37, 3), (257, 17), (2049, 129)]      # 2049 * 129 = 264 321 > 1024 workgroups * 256: the grid-stride loop


@gpu
@pytest.mark.parametrize("alpha_range", ALPHA_RANGES)
@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_loss_and_its_four_gradients_against_float64_autograd(shape, alpha_range):
    gen = torch.Generator().manual_seed(shape[0] * 10 + int(math.log10(alpha_range[1])))
    g, u, a, b, y = nig_inputs(shape, alpha_range, gen)
    if shape == (37, 3):
        y[0, 0] = g[0, 0]                                                   # |y - gamma| at exactly 0: gradient 0 (torch.abs)
    want, want_g = loss_ref64((g, u, a, b), y, 1e-2)
    lib = _lib.load()
    assert shape != LOSS_SHAPES[-1] or lib.bnn_nig_loss_workspace_bytes(g.numel()) // 8 * 256 < g.numel()
    leaves = [t.to(DEV).requires_grad_() for t in (g, u, a, b)]
    n0 = lib.bnn_launch_count()
    loss = NormalInverseGaussianLoss(1e-2)(*leaves, y.to(DEV))
    assert lib.bnn_launch_count() == n0 + 2
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    check_loss(loss.item(), [t.grad for t in leaves], want, want_g, (shape, alpha_range))


@gpu
def test_loss_strided_views_partial_gradients_no_grad_lambda_zero_reproducible_and_the_switch():
    lib = _lib.load()
    gen = torch.Generator().manual_seed(12)
    rows, D = 37, 3
    # the reference's own layout: torch.split views of z, activations applied out of place -> gamma is a strided view
    zz = torch.randn(rows, 4 * D, generator=gen)
    y = torch.randn(rows, D, generator=gen)
    sp = torch.nn.functional.softplus

    def views(z):
        g, u, a, b = torch.split(z, D, dim=-1)
        return g, 1e-10 + sp(u), 1 + 1e-10 + sp(a), 1e-10 + sp(b)

    z64 = zz.double().requires_grad_()
    want = torch_expression(*views(z64), y.double(), 1e-2)
    want.backward()
    zd = zz.to(DEV).requires_grad_()
    vs = views(zd)
    assert not vs[0].is_contiguous()
    loss = ops.nig_loss(*vs, y.to(DEV), 1e-2)
    loss.backward()
    assert abs(loss.item() - want.item()) <= 1e-5 * max(1.0, abs(want.item()))
    assert np.abs(N(zd.grad) - N(z64.grad)).max() <= 1e-5 * np.abs(N(z64.grad)).max()
    # all four strided: columns of one wider tensor
    g, u, a, b, y = nig_inputs((rows, D), (1e-3, 50.0), gen)
    wide = torch.cat([g, u, a, b], -1).to(DEV)
    yd = y.to(DEV)
    for lam in (1e-2, 0.0):
        want, want_g = loss_ref64((g, u, a, b), y, lam)
        # only some inputs requiring a gradient: the others' are neither computed nor returned
        for need in ((True, True, True, True), (False, True, False, True), (True, False, False, False)):
            leaves = [wide[:, k * D:(k + 1) * D].clone().requires_grad_(n) for k, n in enumerate(need)]
            n0 = lib.bnn_launch_count()
            loss = ops.nig_loss(*leaves, yd, lam)
            assert lib.bnn_launch_count() == n0 + 2
            loss.backward()
            assert [t.grad is not None for t in leaves] == list(need)
            check_loss(loss.item(), [t.grad for t in leaves], want, want_g, ("need", need, lam))
        strided = [wide[:, k * D:(k + 1) * D] for k in range(4)]
        assert not any(t.is_contiguous() for t in strided)
        with torch.no_grad():
            quiet = ops.nig_loss(*strided, yd, lam)
        assert not quiet.requires_grad
        check_loss(quiet.item(), [None] * 4, want, want_g, ("no_grad", lam))
        assert torch.equal(quiet, loss.detach())                            # the same bits whichever gradients are asked for
        # upstream scaling
        leaves = [t.clone().requires_grad_() for t in strided]
        (3.0 * ops.nig_loss(*leaves, yd, lam)).backward()
        check_loss(quiet.item(), [t.grad / 3.0 for t in leaves], want, want_g, ("scaled", lam))
    # two runs, bitwise
    big = [t.to(DEV) for t in nig_inputs((2049, 129), (1e-3, 50.0), gen)]
    runs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_() for t in big[:4]]
        loss = ops.nig_loss(*leaves, big[4], 1e-2)
        loss.backward()
        runs.append([loss.detach()] + [t.grad for t in leaves])
    assert all(torch.equal(s, t) for s, t in zip(*runs))
    # y with a gradient is refused on the device path; the switch off takes the torch-op path, within the same bound
    with pytest.raises(_lib.BnnHipError):
        ops.nig_loss(*strided, yd.clone().requires_grad_(), 1e-2)
    want, want_g = loss_ref64((g, u, a, b), y, 1e-2)
    # the module keeps the torch expression for such a y, as before K13: y gets its gradient and no kernel of ours runs
    leaves = [t.clone().requires_grad_() for t in strided]
    yg = yd.clone().requires_grad_()
    n0 = lib.bnn_launch_count()
    loss = NormalInverseGaussianLoss(1e-2)(*leaves, yg)
    loss.backward()
    assert lib.bnn_launch_count() == n0 and yg.grad is not None and yg.grad.shape == yd.shape
    check_loss(loss.item(), [t.grad for t in leaves], want, want_g, "y with a gradient")
    # an empty batch through the head keeps the torch path too (the entries refuse rows = 0)
    head = NormalInverseGaussianLinear(5, D).to(DEV)
    n0 = lib.bnn_launch_count()
    outs = head(torch.empty(0, 5, device=DEV))
    assert lib.bnn_launch_count() == n0 and [tuple(t.shape) for t in outs] == [(0, D)] * 4
    with hip_switch(False):
        leaves = [t.clone().requires_grad_() for t in strided]
        n0 = lib.bnn_launch_count()
        loss = NormalInverseGaussianLoss(1e-2)(*leaves, yd)
        loss.backward()
        assert lib.bnn_launch_count() == n0                                 # torch ops only
    check_loss(loss.item(), [t.grad for t in leaves], want, want_g, "switch off")


def _mc_inputs(S, rows, D, gen, offset=None):
    shape = (S, rows, D)
    g, u, a, b, _ = nig_inputs(shape, (1e-3, 50.0), gen, DEV)
    if offset is not None:
        g = (offset + 1e-2 * torch.randn(shape, generator=gen, device=DEV, dtype=torch.float64)).float()
    return g, u, a, b


def _mc_ref(ts):
    """float64 torch ops on the device (independent of the kernel), as NumPy: mean, total, aleatoric, epistemic."""
    g, u, a, b = (t.double() for t in ts)
    ale_s = b / (a - 1.0)
    mean = g.mean(0)
    ale = ale_s.mean(0)
    epi = (ale_s / u).mean(0) + ((g - mean) ** 2).mean(0)
    return [N(t) for t in (mean, ale + epi, ale, epi)]


@gpu
@pytest.mark.parametrize("D", [1, 3, 16, 17, 300, 1000, 1028, 4096])     # wide: <64,1>, <64,2>, <64,4>, <256,2>, <256,4>
@pytest.mark.parametrize("rows", [1, 37, 257])
@pytest.mark.parametrize("S", [1, 3, 8, 65, 130])
def test_mc_evidential_against_float64(S, rows, D):
    gen = torch.Generator(device=DEV).manual_seed(S * 7919 + rows * 31 + D)
    ts = _mc_inputs(S, rows, D, gen)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    u = ops.mc_evidential(*ts)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1
    assert isinstance(u, ops.PredictiveRegression) and all(t.shape == (rows, D) and t.dtype == torch.float32 for t in u)
    check_mc(u, _mc_ref(ts), (S, rows, D))
    if S == 1:
        # exactly the module's torch outputs, and gamma
        ale, epi = NormalInverseGaussianUncertainty()(ts[1][0], ts[2][0], ts[3][0])
        assert torch.equal(u.mean, ts[0][0]) and torch.equal(u.aleatoric, ale) and torch.equal(u.epistemic, epi)


@gpu
@pytest.mark.parametrize("S", [8, 65])
def test_mc_evidential_large_offset_keeps_the_variance_of_gamma(S):
    """gamma near 4096 with spread 1e-2 and heads whose own epistemic part is ~1e-9: the epistemic output IS the variance of
    gamma, which a raw sum of squares loses in the 4th - 5th digit even in fp64 (test_predictive_regression.py).  Relative."""
    gen = torch.Generator(device=DEV).manual_seed(S)
    g, u, a, b = _mc_inputs(S, 64, 3, gen, offset=4096.0)
    b = b * 1e-9
    u2 = ops.mc_evidential(g, u, a, b)
    ref = _mc_ref((g, u, a, b))
    check_mc(u2, ref, ("offset", S))
    assert ref[3].min() >= 1e-5
    assert (np.abs(N(u2.epistemic) - ref[3]) <= 1e-5 * ref[3]).all()
    for D in (17, 1028):                                                    # the wide split takes the same shift
        g, u, a, b = _mc_inputs(S, 5, D, gen, offset=4096.0)
        b = b * 1e-9
        ref = _mc_ref((g, u, a, b))
        assert (np.abs(N(ops.mc_evidential(g, u, a, b).epistemic) - ref[3]) <= 1e-5 * ref[3]).all()


@gpu
def test_mc_evidential_layouts_and_bitwise_reproducible():
    gen = torch.Generator(device=DEV).manual_seed(5)
    for shape in ((130, 257, 3), (65, 37, 17), (8, 9, 1028)):
        ts = _mc_inputs(*shape, gen)
        a, b = ops.mc_evidential(*ts), ops.mc_evidential(*ts)
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    # leading row dims and non-contiguous inputs
    ts = _mc_inputs(4, 21, 6, gen)
    want = ops.mc_evidential(*ts)
    nd = [t.view(4, 3, 7, 6).permute(0, 2, 1, 3).contiguous().transpose(1, 2) for t in ts]
    assert not nd[0].is_contiguous()
    got = ops.mc_evidential(*nd)
    assert all(s.shape == (3, 7, 6) and torch.equal(s.reshape(21, 6), t) for s, t in zip(got, want))
    # a misaligned base (no 16-B accesses) gives the same bits as the aligned one
    S, rows, D = 3, 5, 20
    ts = _mc_inputs(S, rows, D, gen)
    off = []
    for t in ts:
        buf = torch.empty(t.numel() + 1, device=DEV)
        buf[1:] = t.reshape(-1)
        off.append(buf[1:].view(S, rows, D))
    assert off[0].data_ptr() % 16 != 0 and off[0].is_contiguous()
    assert all(torch.equal(s, t) for s, t in zip(ops.mc_evidential(*off), ops.mc_evidential(*ts)))


@gpu
@pytest.mark.parametrize("batched", [True, False])
def test_model_with_a_bayesian_trunk_and_an_evidential_head(batched):
    """2-16-16-NIG(2), NormalLinear trunk, batch 5, 4 samples."""
    torch.manual_seed(2)
    net = EviNet([2, 16, 16, 2], samples=4).to(DEV)
    seeded.pin_streams(net, 1310)
    net.mc_batched = batched
    x = torch.randn(5, 2, device=DEV)
    lib = _lib.load()
    with torch.no_grad():
        out = net(x)
        assert isinstance(out, list) and len(out) == 4
        for o in out:
            assert isinstance(o, tuple) and len(o) == 4 and all(t.shape == (5, 2) for t in o)
        bnn.manual_seed(8)
        p = net.predictive_evidential(x, 4, 3)
        bnn.manual_seed(8)
        n0 = lib.bnn_launch_count()
        ys = net.forward_stacked(x, 4, 3)
        n_forward = lib.bnn_launch_count() - n0
        bnn.manual_seed(8)
        n0 = lib.bnn_launch_count()
        net.predictive_evidential(x, 4, 3)
        assert lib.bnn_launch_count() - n0 == n_forward + 1                 # the pass + ONE bnn_mc_evidential launch
    assert isinstance(ys, tuple) and len(ys) == 4 and all(t.shape == (4, 5, 2) for t in ys)
    assert float((ys[0][0] - ys[0][1]).abs().max()) > 0                     # the draws differ
    want = ops.evidential_f64(*[t.cpu() for t in ys])
    assert all(t.shape == (5, 2) for t in p)
    check_mc(p, [N(t) for t in want], ("model", batched))
    # training through the tuple-valued batched pass: every posterior parameter gets a gradient
    y = torch.randn(5, 2, device=DEV)
    crit = NormalInverseGaussianLoss()
    loss = sum(crit(*o, y) for o in net(x)) / 4
    loss.backward()
    assert all(p_.grad is not None and torch.isfinite(p_.grad).all() for p_ in net.parameters())


@gpu
def test_one_adam_step_of_the_simple_network_with_the_switch_on_and_off():
    """examples/Simple: 1-100-100-100-NIG(1), batch 128, Adam(5e-4).  From the same state, the loss and every parameter's
    gradient of the HIP path against the torch-op path (the bound of the module docstring), and the launches of the step."""
    torch.manual_seed(4)
    base = EviNet([1, 100, 100, 100, 1], samples=1, bayes=False).to(DEV)
    x = torch.linspace(-4, 4, 128, device=DEV).unsqueeze(1)
    y = x ** 3 + 3.0 * torch.randn(128, 1, device=DEV)
    lib = _lib.load()
    res = {}
    for on in (False, True):
        net = copy.deepcopy(base)
        opt = torch.optim.Adam(net.parameters(), lr=5e-4)
        with hip_switch(on):
            opt.zero_grad()
            n0 = lib.bnn_launch_count()
            loss = NormalInverseGaussianLoss()(*net(x), y)
            loss.backward()
            launches = lib.bnn_launch_count() - n0
            opt.step()
        res[on] = (loss.item(), [p.grad.clone() for p in net.parameters()], [p.detach().clone() for p in net.parameters()],
                   launches)
    assert res[False][3] == 0 and res[True][3] == 4                         # head 1 + loss 2 + head backward 1
    want, got = res[False], res[True]
    print("loss", got[0], "torch ops", want[0])
    assert abs(got[0] - want[0]) <= 1e-5 * max(1.0, abs(want[0]))
    for (name, _), g, r in zip(base.named_parameters(), got[1], want[1]):
        e, scale = float((g - r).abs().max()), float(r.abs().max())
        print(name, "err", e, "max|ref|", scale)
        assert e <= 1e-5 * scale, (name, e, scale)
    for p_on, p_off, p0 in zip(got[2], want[2], base.parameters()):
        assert not torch.equal(p_on, p0.detach())                           # the step moved every parameter
        assert float((p_on - p_off).abs().max()) <= 2 * 5e-4                # ... by at most lr either way
