"""Predictive regression (bnn_mc_regression, ops.mc_regression, BayesianNetworkModule.predictive_regression) and the Gaussian
likelihood that trains such a head (bnn_gaussian_nll, ops.gaussian_nll, nn.GaussianNLL): the mean of the per-sample means, the
mean of the per-sample variances (aleatoric), the variance of the per-sample means (epistemic) and their sum (total) -- the
bands of examples/Simple/uncertainty.py.

CPU: the C-ABI entries and their argument errors, the ops' refusals, the float64 CPU paths against a NumPy restatement.
GPU: the kernel against float64 over both work splits and the three output layouts, the offset case a raw sum of squares
fails, layouts, a fused head's partials, bitwise reproducibility, the epoch / KL tails, the module's paths and modes, the loss
and its gradient, and one training step end to end.

Tolerances (an fp64 sum rounded once to fp32 is within 6e-8 relative; v_exp_f32 on s log2(e), |s| <= 8, within ~1e-6):
mean 1e-6 max(1, |ref|); aleatoric / total 1e-5 max(1, |ref|); epistemic 1e-5 |ref| + 1e-12 (relative on purpose), and >= 0."""
import ctypes
import os
import re

import numpy as np
import pytest
import seeded
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, GaussianNLL, NormalLinear
from conftest import ROOT

gpu = pytest.mark.gpu
KINDS = ["values", "mean_logvar", "mean_var"]


def ref64(y, outputs):
    """float64 NumPy restatement (two-pass variance): y (S, rows, width) -> mean, total, aleatoric, epistemic (rows, D)."""
    y = np.asarray(y, dtype=np.float64)
    if outputs == "values":
        m, v = y, None
    else:
        D = y.shape[-1] // 2
        m = y[..., :D]
        v = np.exp(y[..., D:]) if outputs == "mean_logvar" else y[..., D:]
    mean = m.mean(0)
    epi = ((m - m.mean(0)) ** 2).mean(0)
    ale = np.zeros_like(mean) if v is None else v.mean(0)
    return mean, ale + epi, ale, epi


def N(t):
    return t.detach().double().cpu().numpy()


def check_against_ref(u, y, outputs, what=""):
    """The tolerances of the module docstring; prints nothing, reports the worst figure in the assertion."""
    y = np.asarray(y)
    y = y.reshape(y.shape[0], -1, y.shape[-1])
    mean, total, ale, epi = ref64(y, outputs)
    got = [N(t).reshape(mean.shape) for t in u]
    e = np.abs(got[0] - mean) - 1e-6 * np.maximum(1.0, np.abs(mean))
    assert e.max() <= 0, (what, "mean", np.abs(got[0] - mean).max())
    for name, g, r in (("total", got[1], total), ("aleatoric", got[2], ale)):
        e = np.abs(g - r) - 1e-5 * np.maximum(1.0, np.abs(r))
        assert e.max() <= 0, (what, name, np.abs(g - r).max(), float(np.abs(r).max()))
    e = np.abs(got[3] - epi) - (1e-5 * np.abs(epi) + 1e-12)
    assert e.max() <= 0, (what, "epistemic", float((np.abs(got[3] - epi) / np.maximum(epi, 1e-300)).max()))
    assert got[3].min() >= 0, (what, "epistemic < 0", got[3].min())
    return epi


def check_against_op(u, want, what=""):
    """The same tolerances with another launch's result as the reference."""
    for name, g, r, rel, floor in (("mean", u.mean, want.mean, 1e-6, 1.0), ("total", u.total, want.total, 1e-5, 1.0),
                                   ("aleatoric", u.aleatoric, want.aleatoric, 1e-5, 1.0)):
        g, r = N(g), N(r)
        assert (np.abs(g - r) <= rel * np.maximum(floor, np.abs(r))).all(), (what, name, np.abs(g - r).max())
    g, r = N(u.epistemic), N(want.epistemic)
    assert (np.abs(g - r) <= 1e-5 * np.abs(r) + 1e-12).all() and g.min() >= 0, (what, "epistemic", np.abs(g - r).max())


class MLP(BayesianNetworkModule):
    def __init__(self, dims, samples=4):
        super().__init__(dims[0], dims[-1], samples)
        mods = []
        for i in range(len(dims) - 1):
            mods.append(NormalLinear(dims[i], dims[i + 1]))
            if i < len(dims) - 2:
                mods.append(torch.nn.ReLU())
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    assert re.search(r"\bint bnn_mc_regression\s*\(", header)
    assert re.search(r"\bint bnn_gaussian_nll\s*\(", header)
    assert re.search(r"\bint64_t bnn_gaussian_nll_workspace_bytes\s*\(", header)
    lib = _lib.load()
    for name in ("bnn_mc_regression", "bnn_gaussian_nll", "bnn_gaussian_nll_workspace_bytes"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.bnn_abi_version() == 2
    assert (_lib.REG_VALUES, _lib.REG_MEAN_LOGVAR, _lib.REG_MEAN_VAR) == (0, 1, 2)
    assert lib.bnn_gaussian_nll_workspace_bytes(4, 100, 6) >= 8
    assert "GaussianNLL" not in bnn.nn.__all__ and bnn.nn.GaussianNLL is GaussianNLL


def test_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    n0 = lib.bnn_launch_count()

    def call(y=one, nparts=1, nsamples=4, rows=8, width=10, kind=0, mean=one, total=one, ale=one, epi=one, stride=None):
        return lib.bnn_mc_regression(y, rows * width if stride is None else stride, nparts, nsamples, rows, width, kind, mean,
                                     total, ale, epi, None, 0, None, 0, 1.0, None, None, None)

    assert call(y=None) == -1 and b"NULL" in lib.bnn_last_error()
    for k in ("mean", "total", "ale", "epi"):
        assert call(**{k: None}) == -1
    for k in ("nsamples", "rows", "width", "nparts"):
        assert call(**{k: 0}) == -2
    assert call(nsamples=65537) == -5
    assert call(width=4097) == -5
    assert call(rows=2 ** 31) == -5
    assert call(kind=3) == -5 and b"kind" in lib.bnn_last_error()
    assert call(kind=-1) == -5
    assert call(width=9, kind=1) == -2 and call(width=9, kind=2) == -2
    assert call(stride=79) == -2                                            # overlapping addends
    assert call(nsamples=1, nparts=2, stride=79) == -2
    # a KL tail with a bad description: its own code, nothing launched
    t = (_lib.KlTensor * 1)()
    t[0].mu, t[0].rho, t[0].n, t[0].prior_mu, t[0].prior_sigma = 16, 16, 8, 0.0, 0.1
    assert lib.bnn_mc_regression(one, 80, 1, 4, 8, 10, 0, one, one, one, one, None, 0, t, 1, 1.0, None, one, None) == -1

    def nll(y=one, nsamples=4, rows=8, width=6, target=one, loss=one, g=one, ws=one):
        return lib.bnn_gaussian_nll(y, nsamples, rows, width, target, loss, g, ws, None)

    for k in ("y", "target", "loss", "ws"):
        assert nll(**{k: None}) == -1
    for k in ("nsamples", "rows", "width"):
        assert nll(**{k: 0}) == -2
    assert nll(nsamples=65537) == -5
    assert nll(width=4098) == -5
    assert nll(rows=2 ** 31) == -5
    assert nll(width=7) == -2
    assert lib.bnn_launch_count() == n0


class _FakeKl(ops.KlDeferred):
    pass


def _pending_kl():
    h = _FakeKl()
    h.launched, h.done = False, False
    ops._tls.kl_carry = h
    return h


def test_op_refuses_cpu_tensors_and_unknown_outputs_and_leaves_no_kl_carry():
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression(torch.zeros(2, 3, 4), "values")
    for bad in (None, "logits", "MEAN_LOGVAR", 0):
        with pytest.raises(ValueError):
            ops.mc_regression(torch.zeros(2, 3, 4), bad)
        with pytest.raises(ValueError):
            ops.regression_f64(torch.zeros(2, 3, 4), bad)
    with pytest.raises(ValueError):
        ops.mc_regression(torch.zeros(2, 3, 4))                    # `outputs` is required
    try:
        h = _pending_kl()
        with pytest.raises(_lib.BnnHipError):
            ops.mc_regression(torch.zeros(2, 3, 4), "mean_var", kl=h)
        assert ops._tls.kl_carry is None
        h = _pending_kl()
        with pytest.raises(ValueError):
            ops.mc_regression(torch.zeros(2, 3, 4), None, kl=h)
        assert ops._tls.kl_carry is None
    finally:
        ops._tls.kl_carry = None


def _draw_state(net):
    """Every posterior tensor's recorded draw: its key (device) or its drawn value (CPU)."""
    out = []
    for m in net.modules():
        if isinstance(m, NormalLinear):
            for p in (m.weight, m.bias):
                k = p.draw_key
                out.append(None if k is None else (k.seed, k.stream, k.sample0, k.nsamples, k.epoch_host, k.gen))
                out.append(None if p._explicit is None else p._explicit.detach().clone())
    return out


def _same_state(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y)
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("outputs", KINDS)
def test_cpu_module_matches_float64_numpy_on_the_same_draws(outputs):
    torch.manual_seed(0)
    net = MLP([8, 16, 4])
    x = torch.randn(7, 8)
    rng_state, draws = torch.get_rng_state(), _draw_state(net)
    with pytest.raises(ValueError):
        net.predictive_regression(x, 4, outputs="logits")            # refused before a draw is consumed
    with pytest.raises(TypeError):
        net.predictive_regression(x, 4)                              # `outputs` is a required keyword
    assert torch.equal(torch.get_rng_state(), rng_state) and _same_state(_draw_state(net), draws)
    with pytest.raises(_lib.BnnHipError):
        net.predictive_regression(x, 4, outputs=outputs, advance=torch.zeros(1, dtype=torch.int32))
    torch.manual_seed(3)
    u = net.predictive_regression(x, 4, outputs=outputs)
    torch.manual_seed(3)
    ys = net.forward_stacked(x, 4)
    D = 4 if outputs == "values" else 2
    assert isinstance(u, ops.PredictiveRegression) and u._fields == ("mean", "total", "aleatoric", "epistemic")
    assert all(t.shape == (7, D) and t.dtype == torch.float32 for t in u)
    if outputs == "mean_var":
        ys = torch.cat([ys[..., :2], ys[..., 2:].abs()], -1)         # variances as given: make them variances
        u = ops.regression_f64(ys, outputs)
    check_against_ref(u, ys.detach().numpy(), outputs)
    for a, b in zip(u, ops.regression_f64(ys, outputs)):
        assert torch.equal(a, b)
    assert float(u.epistemic.min()) > 0
    if outputs == "values":
        assert float(u.aleatoric.abs().max()) == 0
    one = ops.regression_f64(ys[:1], outputs)                        # S = 1: no disagreement between the draws
    assert float(one.epistemic.abs().max()) == 0


def test_cpu_gaussian_nll_is_torchs_gaussian_nll_loss_and_gradient():
    gen = torch.Generator().manual_seed(4)
    S, B, D = 3, 5, 2
    m = torch.randn(S, B, D, generator=gen)
    s = torch.rand(S, B, D, generator=gen) * 7 - 4
    t = torch.randn(B, D, generator=gen)
    ys = torch.cat([m, s], -1).requires_grad_()
    loss = GaussianNLL()(ys, t)
    assert loss.dtype == torch.float32 and loss.shape == ()
    loss.backward()
    y64 = torch.cat([m, s], -1).double().requires_grad_()
    want = torch.nn.functional.gaussian_nll_loss(y64[..., :D], t.double().expand(S, B, D), torch.exp(y64[..., D:]), full=False,
                                                 eps=0.0, reduction="mean")
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-6 * max(1.0, abs(want.item()))
    assert (ys.grad.double() - y64.grad).abs().max() <= 1e-6 * max(1.0, float(y64.grad.abs().max()))
    # the list model(x) returns, and one un-stacked sample
    assert torch.equal(GaussianNLL()(list(ys.detach().unbind(0)), t), loss.detach())
    assert torch.equal(GaussianNLL()(ys.detach()[0], t), GaussianNLL()(ys.detach()[:1], t))
    with pytest.raises(ValueError):
        ops.gaussian_nll(torch.zeros(2, 5, 3), torch.zeros(5, 2))


# ------------------------------------------------------------------------------------------------------------------ GPU
DEV = torch.device("cuda:0")
S_AXIS = [1, 2, 8, 33, 100]             # 33: a 64-lane group that is not full; 100: more samples than 64 lanes; 1: epistemic == 0
ROWS_AXIS = [1, 5, 513]
WIDTH_AXIS = [2, 6, 16, 18, 20, 1024, 1028, 4096]    # 16 | 18: narrow | wide; 1024 | 1028: a wave | the workgroup per row; 18: no 16-B loads


def _inputs(S, rows, width, outputs, gen, device):
    """Means N(0, 1); log-variances uniform in [-8, 4]; variances uniform in [0, 3]."""
    if outputs == "values":
        return torch.randn(S, rows, width, generator=gen, device=device)
    D = width // 2
    m = torch.randn(S, rows, D, generator=gen, device=device)
    u = torch.rand(S, rows, D, generator=gen, device=device)
    return torch.cat([m, u * 12 - 8 if outputs == "mean_logvar" else u * 3], -1)


@gpu
@pytest.mark.parametrize("width", WIDTH_AXIS)
@pytest.mark.parametrize("rows", ROWS_AXIS)
@pytest.mark.parametrize("S", S_AXIS)
@pytest.mark.parametrize("outputs", KINDS)
def test_kernel_against_float64(outputs, S, rows, width):
    if outputs != "values" and width % 2:
        pytest.skip("a (mean, variance) layout has an even width")
    gen = torch.Generator(device=DEV).manual_seed(S * 7919 + rows * 31 + width)
    y = _inputs(S, rows, width, outputs, gen, DEV)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    u = ops.mc_regression(y, outputs)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1
    D = width if outputs == "values" else width // 2
    assert all(t.shape == (rows, D) and t.dtype == torch.float32 for t in u)
    check_against_ref(u, y.cpu().numpy(), outputs, (outputs, S, rows, width))
    if S == 1:
        assert float(u.epistemic.abs().max()) == 0
        assert torch.equal(u.mean, y[0, :, :D])
    if outputs == "values":
        assert float(u.aleatoric.abs().max()) == 0 and torch.equal(u.total, u.epistemic)


@gpu
@pytest.mark.parametrize("S", [8, 33])
def test_large_offset_keeps_the_relative_accuracy_of_the_epistemic_part(S):
    """fp32 values near 4096 with spread 1e-2: sum m^2 / S - mean^2 on the raw values is wrong in the 4th - 5th digit even in
    fp64; the shifted form is not."""
    gen = torch.Generator().manual_seed({8: 71, 33: 0}[S])          # seeds at which the reference's epistemic part is >= 1.8e-5
    y = (4096.0 + 1e-2 * torch.randn(S, 64, 3, generator=gen, dtype=torch.float64)).float()
    y64 = y.numpy().astype(np.float64)
    epi = ref64(y64, "values")[3]
    assert epi.min() >= 1.8e-5                                      # the relative test is well-posed
    raw = (y64 ** 2).mean(0) - y64.mean(0) ** 2
    assert (np.abs(raw - epi) / epi).max() > 3e-5                   # ... and the raw form, in float64, misses it
    u = ops.mc_regression(y.to(DEV), "values")
    check_against_ref(u, y.numpy(), "values", ("offset", S))


@gpu
def test_leading_row_dims_and_non_contiguous_input():
    gen = torch.Generator().manual_seed(5)
    S = 4
    base = _inputs(S, 3 * 7, 6, "mean_logvar", gen, "cpu").view(S, 3, 7, 6)
    yt = base.permute(0, 2, 1, 3).contiguous().to(DEV).transpose(1, 2)      # (S, 3, 7, 6), a transposed view
    big = torch.zeros(S, 3, 7, 9, device=DEV)
    big[..., 2:8] = base.to(DEV)
    ys = big[..., 2:8]                                                        # a sliced view
    assert not yt.is_contiguous() and not ys.is_contiguous()
    want = ops.mc_regression(base.to(DEV), "mean_logvar")
    for y in (yt, ys):
        for outputs, D in (("mean_logvar", 3), ("values", 6)):
            u = ops.mc_regression(y, outputs)
            assert all(t.shape == (3, 7, D) for t in u)
            check_against_ref(u, base.numpy(), outputs)
        for a, b in zip(ops.mc_regression(y, "mean_logvar"), want):
            assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("width", [2, 10, 16])
@pytest.mark.parametrize("M", [5, 64])
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("parts", [2, 8, 300])
def test_partials_give_the_bits_of_logits_then_the_kernel(parts, S, M, width):
    """A fused head's partials (parts, S, M, width) summed in the launch: the same bits as HeadPartials.logits() (bnn_mc_sum over
    the parts: sequential up to 32 addends, four quarters above) followed by the kernel."""
    gen = torch.Generator().manual_seed(parts * 100 + width)
    p = torch.randn(parts, S, M, width, generator=gen) * 0.5
    hp = ops.HeadPartials(p.to(DEV))
    logits = hp.logits()
    for outputs in KINDS:
        fused = ops.mc_regression(hp, outputs)
        plain = ops.mc_regression(logits, outputs)
        for a, b in zip(fused, plain):
            assert torch.equal(a, b)
        assert fused.mean.shape == (M, width if outputs == "values" else width // 2)


@gpu
def test_wide_partials_give_the_same_bits_too():
    gen = torch.Generator().manual_seed(77)
    for parts, S, M, width in ((3, 4, 5, 40), (40, 2, 3, 1032)):
        hp = ops.HeadPartials((torch.randn(parts, S, M, width, generator=gen) * 0.5).to(DEV))
        for outputs in KINDS:
            for a, b in zip(ops.mc_regression(hp, outputs), ops.mc_regression(hp.logits(), outputs)):
                assert torch.equal(a, b)


@gpu
def test_bitwise_reproducible():
    gen = torch.Generator().manual_seed(11)
    for shape, outputs in (((100, 513, 6), "mean_logvar"), ((33, 64, 1000), "mean_logvar"), ((8, 9, 4096), "values")):
        y = _inputs(*shape, outputs, gen, "cpu").to(DEV)
        a, b = ops.mc_regression(y, outputs), ops.mc_regression(y, outputs)
        for s, t in zip(a, b):
            assert torch.equal(s, t)
    ys = _inputs(33, 257, 32, "mean_logvar", gen, "cpu").to(DEV).requires_grad_()
    t = torch.randn(257, 16, generator=gen).to(DEV)
    out = []
    for _ in range(2):
        ys.grad = None
        loss = ops.gaussian_nll(ys, t)
        loss.backward()
        out.append((loss.detach().clone(), ys.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@gpu
def test_epoch_and_kl_tails_in_the_same_launch():
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    shapes = [(300, 40), (300,), (10, 300), (10,)]
    mus = [(torch.randn(s, generator=gen) * 0.1).to(DEV) for s in shapes]
    rhos = [(torch.randn(s, generator=gen) * 0.2 - 3.0).to(DEV) for s in shapes]
    priors = [(0.0, 0.1), (0.0, 0.1), (0.1, 0.5), (0.0, 1.0)]
    y = _inputs(8, 512, 10, "mean_logvar", gen, "cpu").to(DEV)
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)
    plain = ops.mc_regression(y, "mean_logvar")
    want_kl = ops.kl_normal_scalar(mus, rhos, priors, 3.0)
    h = ops.kl_normal_begin(mus, rhos, priors, n_batches=3.0)
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    u = ops.mc_regression(y, "mean_logvar", advance=cell, kl=h)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1 and h.done
    assert torch.equal(h.out[-1], want_kl.detach())
    assert torch.equal(h.out, ops.kl_normal(mus, rhos, priors, 3.0))
    assert int(cell.item()) == 1
    for a, b in zip(u, plain):
        assert torch.equal(a, b)
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression(y, "mean_logvar", kl=h)                             # finished already
    # the C-ABI: the epoch moves by exactly advance_inc, wide split included
    y2 = _inputs(3, 5, 1000, "values", gen, "cpu").to(DEV)
    outs = [torch.empty(5, 1000, device=DEV) for _ in range(4)]
    n0 = lib.bnn_launch_count()
    _lib.check(lib.bnn_mc_regression(_lib.ptr(y2), 5000, 1, 3, 5, 1000, 0, *[_lib.ptr(t) for t in outs], _lib.ptr(cell), 7,
                                     None, 0, 1.0, None, None, _lib.stream_ptr(DEV)), "bnn_mc_regression")
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1 and int(cell.item()) == 8
    check_against_ref(outs, N(y2), "values")


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("batched", [True, False])
def test_module_paths_equal_the_op_on_forward_stacked(mode, batched):
    torch.manual_seed(2)
    net = MLP([12, 32, 4], samples=6).to(DEV)
    seeded.pin_streams(net, 1210)
    net.mc_batched = batched
    x = torch.randn(130, 12, device=DEV)
    bnn.set_compute(mode)
    try:
        with torch.no_grad():
            bnn.manual_seed(8)
            u = net.predictive_regression(x, 6, 3, outputs="mean_logvar")
            bnn.manual_seed(8)
            ys = net.forward_stacked(x, 6, 3)
            want = ops.mc_regression(ys, "mean_logvar")
    finally:
        bnn.set_compute("f32")
    assert u.mean.shape == (130, 2)
    check_against_op(u, want, (mode, batched))
    check_against_ref(u, N(ys), "mean_logvar")


@gpu
def test_fused_head_mlp_costs_one_launch_more_than_the_layers():
    from bayesianneuralnetworks_amd.nn import fuse_activations
    lib = _lib.load()
    torch.manual_seed(1)
    net = MLP([16, 48, 4], samples=8).to(DEV)
    seeded.pin_streams(net, 1220)
    net.mc_batched = True
    fuse_activations(net, bf16_activations=True, fuse_head=True)
    x = torch.randn(64, 16, device=DEV)
    bnn.set_compute("bf16")
    try:
        with torch.no_grad():
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            u = net.predictive_regression(x, 8, outputs="mean_logvar")
            n_reg = lib.bnn_launch_count() - n0
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            hp = net._forward_batched_stacked(x, 8, 0, _lazy_head=True)
            n_layers = lib.bnn_launch_count() - n0
            assert isinstance(hp, ops.HeadPartials)
            ys = hp.logits()
            want = ops.mc_regression(ys, "mean_logvar")
    finally:
        bnn.set_compute("f32")
    assert n_reg == n_layers + 1
    for a, b in zip(u, want):
        assert torch.equal(a, b)
    check_against_ref(u, N(ys), "mean_logvar")


def _nll64(ys, t):
    """float64 NumPy: the loss and N * gradient of y (S, B, 2 D) against t (B, D)."""
    y = np.asarray(ys, np.float64)
    D = y.shape[-1] // 2
    m, s = y[..., :D], y[..., D:]
    r = np.asarray(t, np.float64)[None] - m
    e = np.exp(-s)
    return (0.5 * (s + r * r * e)).mean(), np.concatenate([-r * e, 0.5 * (1 - r * r * e)], -1)


@gpu
@pytest.mark.parametrize("D", [1, 3, 16, 130])
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("S", [1, 4, 33])
def test_gaussian_nll_loss_and_gradient_against_float64(S, B, D):
    gen = torch.Generator().manual_seed(S * 1000 + B * 10 + D)
    m = torch.randn(S, B, D, generator=gen)
    s = torch.rand(S, B, D, generator=gen) * 7 - 4
    t = torch.randn(B, D, generator=gen)
    y = torch.cat([m, s], -1)
    want, gN = _nll64(y.numpy(), t.numpy())
    lib = _lib.load()
    yd, td = y.to(DEV).requires_grad_(), t.to(DEV)
    n0 = lib.bnn_launch_count()
    loss = GaussianNLL()(yd, td)
    assert lib.bnn_launch_count() == n0 + 2
    loss.backward()
    n = S * B * D
    assert abs(loss.item() - want) <= 1e-5 * max(1.0, abs(want)), (loss.item(), want)
    err = np.abs(N(yd.grad) * n - gN).max()
    assert err <= 1e-5 * max(1.0, np.abs(gN).max()), (err, np.abs(gN).max())
    # no gradient asked for: the same loss bits
    assert torch.equal(ops.gaussian_nll(y.to(DEV), td), loss.detach())
    # the list of per-sample outputs; upstream scaling
    assert torch.equal(GaussianNLL()(list(y.to(DEV).unbind(0)), td), loss.detach())
    y2 = y.to(DEV).requires_grad_()
    (3.0 * ops.gaussian_nll(y2, td)).backward()
    assert torch.allclose(y2.grad, 3.0 * yd.grad, rtol=1e-6, atol=0)
    if S == 1:
        y1 = y[0].to(DEV).requires_grad_()                                  # (B, 2 D) is (1, B, 2 D)
        l1 = ops.gaussian_nll(y1, td)
        l1.backward()
        assert torch.equal(l1.detach(), loss.detach()) and torch.equal(y1.grad, yd.grad[0])


def _sigma64(rho):
    return 1e-10 + torch.nn.functional.softplus(rho.double())


@gpu
def test_training_step_gradients_match_float64_autograd_on_the_same_draws():
    """One loss = GaussianNLL(forward_stacked(x), t) + kl_divergence(10) on a 4-32-2 net, mc_batched, S = 4, batch 64, fp32 mode:
    every posterior parameter's gradient against float64 autograd of the same expression on the weights of the layers' draw keys
    (the device eps stream), to the fp32 bound of test_hip_parity.test_training_step_gradients_match_oracle (1e-4 + 1e-4 |ref|)."""
    from torch.distributions import Normal
    from torch.distributions.kl import kl_divergence
    S, B = 4, 64
    torch.manual_seed(9)
    net = MLP([4, 32, 2], samples=S).to(DEV)
    seeded.pin_streams(net, 1230)
    net.mc_batched = True
    bnn.manual_seed(21)
    x = torch.randn(B, 4, device=DEV)
    t = torch.randn(B, 1, device=DEV)
    loss = GaussianNLL()(net.forward_stacked(x), t) + net.kl_divergence(10)
    loss.backward()
    layers = [net.layers[0], net.layers[2]]
    leaves, drawn, kls = [], [], []
    for L in layers:
        pair = []
        for p in (L.weight, L.bias):
            mu = p.mean.detach().double().cpu().requires_grad_()
            rho = p.scale.detach().double().cpu().requires_grad_()
            eps = ops.eps_philox(tuple(p.mean.shape), p.draw_key, DEV).double().cpu()
            assert eps.shape[0] == S
            sig = _sigma64(rho)
            pair.append(mu + sig * eps)
            kls.append(kl_divergence(Normal(mu, sig), Normal(torch.tensor(0.0, dtype=torch.float64), torch.tensor(0.1, dtype=torch.float64))).mean())
            leaves += [mu, rho]
        drawn.append(pair)
    h = x.double().cpu().expand(S, B, 4)
    h = torch.relu(torch.baddbmm(drawn[0][1].unsqueeze(1), h, drawn[0][0].transpose(1, 2)))
    ys = torch.baddbmm(drawn[1][1].unsqueeze(1), h, drawn[1][0].transpose(1, 2))
    r = t.double().cpu() - ys[..., :1]
    want = (0.5 * (ys[..., 1:] + r * r * torch.exp(-ys[..., 1:]))).mean() + torch.stack(kls).mean() / 10
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-4 + 1e-4 * abs(want.item())
    got = [g for L in layers for p in (L.weight, L.bias) for g in (p.mean.grad, p.scale.grad)]
    assert len(got) == len(leaves) == 8
    for g, leaf in zip(got, leaves):
        assert g is not None and np.allclose(N(g), N(leaf.grad), rtol=1e-4, atol=1e-4), float((g.double().cpu() - leaf.grad).abs().max())
    assert float(sum(leaf.grad.abs().sum() for leaf in leaves)) > 0
