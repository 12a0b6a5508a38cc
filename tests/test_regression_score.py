"""Scoring a regression MC forward against its targets (bnn_mc_regression_score, ops.mc_regression_score,
ops.RegressionScoreState, ops.regression_score_f64, BayesianNetworkModule.predictive_regression_score): per element the predictive
mean and variance, the squared error, the NLL of the MC predictive (the equal-weight mixture of the per-sample Gaussians), that of
the moment-matched Gaussian, the mixture's CRPS and its probability integral transform; over a test set RMSE, NLL, CRPS,
sharpness and the PIT histogram with the calibration curve and interval coverage, accumulated on the device.

CPU: the float64 torch path and the module's CPU path against a NumPy restatement, closed forms (one Gaussian, one point, a
quadrature of the mixture's CRPS), a hand-built calibration case, the refusals, the C-ABI's argument errors.  GPU: the kernel
against float64 over both work splits and the three kinds, variance edge cases, NaN targets, a fused head's partials,
accumulation over batches, launch counts, the module's paths and modes, graph capture.

Tolerances (fp32 terms under fp64 sums, as test_predictive_score.py): sq_err, nll, gaussian_nll 1e-5 max(1, |want|); pit 1e-6;
crps 1e-5 T1 with T1 = (1/S) sum_s A(t - m_s, v_s) of the float64 reference -- T1 bounds both sums of the CRPS, which is >= 0."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import seeded
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, NormalLinear
from conftest import ROOT

gpu = pytest.mark.gpu
KINDS = {"values": 0, "mean_logvar": 1, "mean_var": 2}
# The PIT bins of the sweep.  An ensemble's pit ('values') is j / 2S, ON interior edges of 20 bins whatever the seed (S = 2:
# 1 / 2 = 10 / 20).  No 2S of the sweep is a multiple of 7, so j / 2S = i / 7 only at i = 0 or 7.
PB = 7
SCORES = ("sq_err", "nll", "gaussian_nll", "crps", "pit")

_erf = np.vectorize(math.erf, otypes=[np.float64])
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


# ---------------------------------------------------------------------------------------------------- float64 NumPy reference
def Phi(z):
    return 0.5 * _erfc(-np.asarray(z, np.float64) / math.sqrt(2.0))


def ref_A(mu, var):
    """A(mu, sigma^2) = mu (2 Phi(mu / sigma) - 1) + 2 sigma phi(mu / sigma); A(mu, 0) = |mu|; var < 0 or NaN: NaN."""
    mu, var = np.broadcast_arrays(np.asarray(mu, np.float64), np.asarray(var, np.float64))
    out = np.full(mu.shape, np.nan)
    zero = var == 0
    out[zero] = np.abs(mu[zero])
    pos = var > 0
    sg = np.sqrt(var[pos])
    z = mu[pos] / sg
    out[pos] = mu[pos] * _erf(z / math.sqrt(2.0)) + 2.0 * sg * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return out


def split(y, outputs):
    """y (S, R, W) -> float64 (m, v, ln v) each (S, R, D); ln v None for 'values'."""
    y = np.asarray(y, np.float64)
    if outputs == "values":
        return y, np.zeros_like(y), None
    D = y.shape[-1] // 2
    m, s = y[..., :D], y[..., D:]
    if outputs == "mean_logvar":
        return m, np.exp(s), s
    with np.errstate(invalid="ignore", divide="ignore"):
        return m, s, np.where(s > 0, np.log(np.where(s > 0, s, 1.0)), np.nan)


def ref_pit(y, t, outputs):
    m, v, _ = split(y, outputs)
    t = np.asarray(t, np.float64)[None]
    r = t - m
    with np.errstate(invalid="ignore", divide="ignore"):
        sg = np.sqrt(v)
        cdf = np.where(v > 0, Phi(r / np.where(v > 0, sg, 1.0)), (r > 0) + 0.5 * (r == 0))
    cdf = np.where(v >= 0, cdf, np.nan)
    return np.where(np.isnan(t[0]), np.nan, cdf.mean(0))


def ref_elems(y, t, outputs):
    """y (S, R, W), t (R, D) -> dict of float64 (R, D) arrays: the issue's formulas; T1 is the CRPS's first sum."""
    m, v, lnv = split(y, outputs)
    S = m.shape[0]
    t = np.asarray(t, np.float64)
    mean = m.mean(0)
    V = v.mean(0) + ((m - mean) ** 2).mean(0)
    e = mean - t
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(V == 0, np.nan, 0.5 * (np.log(2.0 * math.pi * np.where(V == 0, 1.0, V)) + e * e / np.where(V == 0, 1.0, V)))
        r = t[None] - m
        if lnv is None:
            nll = g
        else:
            inv = np.exp(-lnv) if outputs == "mean_logvar" else 1.0 / np.where(v > 0, v, 1.0)
            ell = -0.5 * (math.log(2.0 * math.pi) + lnv + r * r * inv)
            mx = ell.max(0)
            nll = -(mx + np.log(np.exp(ell - mx).sum(0)) - math.log(S))
    T1 = ref_A(r, v).mean(0)
    pair = np.zeros_like(mean)
    for i in range(S):                                              # the diagonal, then every unordered pair once
        pair += ref_A(0.0, 2.0 * v[i])
        if i + 1 < S:
            pair += 2.0 * ref_A(m[i][None] - m[i + 1:], v[i][None] + v[i + 1:]).sum(0)
    bad = ~(v >= 0).all(0)
    crps = np.where(bad, np.nan, T1 - pair / (2.0 * S * S))
    out = dict(mean=mean, variance=V, sq_err=e * e, nll=nll, gaussian_nll=g, crps=crps, pit=ref_pit(y, t, outputs), T1=T1)
    tn = np.isnan(t)
    for k in SCORES:
        out[k] = np.where(tn, np.nan, out[k])
    return out


def ref_state(ref, bins):
    """The accumulator's (D, 6 + bins) matrix of one batch, float64."""
    R, D = ref["pit"].shape
    v = np.zeros((D, 6 + bins))
    v[:, 0] = R
    for k, name in enumerate(("sq_err", "nll", "gaussian_nll", "crps", "variance")):
        v[:, 1 + k] = ref[name].sum(0)
    for d in range(D):
        p = ref["pit"][:, d]
        b = np.minimum(bins - 1, np.floor(p[~np.isnan(p)] * bins)).astype(np.int64)
        v[d, 6:] = np.bincount(b, minlength=bins)
    return v


def margins_hold(pit, bins):
    """Exact bins need every element's float64 pit more than 1e-5 from every interior edge k / bins."""
    p = pit[~np.isnan(pit)] * bins
    k = np.rint(p)
    return bool((np.where((k >= 1) & (k <= bins - 1), np.abs(p - k) / bins, 1.0) > 1e-5).all())


def tolerances(ref):
    return dict(sq_err=1e-5 * np.maximum(1.0, np.abs(ref["sq_err"])), nll=1e-5 * np.maximum(1.0, np.abs(ref["nll"])),
                gaussian_nll=1e-5 * np.maximum(1.0, np.abs(ref["gaussian_nll"])), crps=1e-5 * ref["T1"],
                pit=np.full(ref["pit"].shape, 1e-6))


def N(t):
    return t.detach().double().cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_elems(u, ref, what="", moments=True):
    """The issue's tolerances; returns the worst error / tolerance ratio per output."""
    shape = ref["pit"].shape
    tol = tolerances(ref)
    worst = {}
    if moments:
        assert (np.abs(N(u.mean).reshape(shape) - ref["mean"]) <= 1e-6 * np.maximum(1.0, np.abs(ref["mean"]))).all(), (what, "mean")
        assert (np.abs(N(u.variance).reshape(shape) - ref["variance"]) <= 1e-5 * np.abs(ref["variance"]) + 1e-12).all(), (what, "variance")
    for name in SCORES:
        got, want = N(getattr(u, name)).reshape(shape), ref[name]
        bad = np.isnan(want)
        assert (np.isnan(got) == bad).all(), (what, name, "NaN elements")
        inf = np.isinf(want)
        assert (got[inf] == want[inf]).all(), (what, name, "infinite elements")
        ok = ~bad & ~inf
        ratio = np.abs(got[ok] - want[ok]) / tol[name][ok]
        worst[name] = float(ratio.max()) if ratio.size else 0.0
    print("worst error / tolerance", what, {k: "%.3g" % v for k, v in worst.items()})
    for name in SCORES:
        assert worst[name] <= 1.0, (what, name, worst[name])
    return worst


def check_state(got, ref, bins, what=""):
    """Counts exact, sums within the per-element tolerance x n.  ref: the float64 elements of everything that went into `got`."""
    got = np.asarray(got, np.float64)
    want = ref_state(ref, bins)
    assert got.shape == want.shape
    assert (got[:, 0] == want[:, 0]).all() and (got[:, 6:] == want[:, 6:]).all(), (what, "counts")
    tol = tolerances(ref)
    tol["variance"] = 1e-5 * np.abs(ref["variance"]) + 1e-12
    for k, name in enumerate(("sq_err", "nll", "gaussian_nll", "crps", "variance")):
        for d in range(got.shape[0]):
            if np.isnan(want[d, 1 + k]):
                assert np.isnan(got[d, 1 + k]), (what, name, d)
            elif np.isinf(want[d, 1 + k]):
                assert got[d, 1 + k] == want[d, 1 + k], (what, name, d)
            else:
                assert abs(got[d, 1 + k] - want[d, 1 + k]) <= tol[name][:, d].sum(), (what, name, d, got[d, 1 + k], want[d, 1 + k])


# the issue's generator: per element a scale of {0.01, 1, 100} and an offset of {0, +-4096}; the samples' means 0.5 scale around a
# centre c, log-variances uniform in [-6, 3] + 2 ln scale, the target 1.5 scale around c
def make_case(S, rows, width, outputs, seed):
    """(y fp32 (S, rows, width), target fp32 (rows, D)) of one fixed seed."""
    gen = torch.Generator().manual_seed(seed)
    D = width if outputs == "values" else width // 2
    scale = torch.tensor([0.01, 1.0, 100.0], dtype=torch.float64)[torch.randint(0, 3, (rows, D), generator=gen)]
    offset = torch.tensor([0.0, 4096.0, -4096.0], dtype=torch.float64)[torch.randint(0, 3, (rows, D), generator=gen)]
    c = torch.randn(rows, D, generator=gen, dtype=torch.float64)
    m = (c + 0.5 * torch.randn(S, rows, D, generator=gen, dtype=torch.float64)) * scale + offset
    s = torch.rand(S, rows, D, generator=gen, dtype=torch.float64) * 9.0 - 6.0 + 2.0 * torch.log(scale)
    t = ((c + 1.5 * torch.randn(rows, D, generator=gen, dtype=torch.float64)) * scale + offset).float()
    if outputs == "values":
        return m.float(), t
    s = s.float()
    return torch.cat([m.float(), s if outputs == "mean_logvar" else torch.exp(s)], -1), t


def ndtri(p):
    """The standard normal quantile by Newton's method on Phi (math.erfc)."""
    x = 0.0
    for _ in range(60):
        x -= (0.5 * math.erfc(-x / math.sqrt(2.0)) - p) * math.sqrt(2.0 * math.pi) * math.exp(0.5 * x * x)
    return x


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
def test_entries_are_declared_bound_exported_and_sized():
    header = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    lib = _lib.load()
    for name in ("bnn_mc_regression_score", "bnn_mc_regression_score_workspace_bytes", "bnn_mc_regression_score_state_doubles"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert "bnn_regression_score.hip" in open(os.path.join(ROOT, "bayesianneuralnetworks_amd", "csrc", "Makefile")).read()
    assert lib.bnn_abi_version() == 2
    size = lib.bnn_mc_regression_score_state_doubles
    assert size(3, 20) == 3 * 26 == ops.regression_score_state_size(3, 20)
    assert size(4096, 128) == 4096 * 134 and size(1, 1) == 7
    assert size(0, 20) == 0 and size(4097, 20) == 0 and size(3, 0) == 0 and size(3, 129) == 0
    ws = lib.bnn_mc_regression_score_workspace_bytes
    assert ws(1, 8, 513, 16, 1, 1) >= 6 * 4 * 513 * 8               # six words per element with a state
    assert ws(3, 8, 513, 16, 1, 0) > 0                              # a fused head's rows, the parts added once
    assert ws(3, 8, 513, 16, 1, 1) >= ws(3, 8, 513, 16, 1, 0) + 6 * 4 * 513 * 8
    assert ws(1, 8, 513, 16, 1, 0) >= 0
    for bad in ((0, 8, 5, 4, 0, 1), (1, 0, 5, 4, 0, 1), (1, 1025, 5, 4, 0, 1), (1, 8, 0, 4, 0, 1), (1, 8, 5, 0, 0, 1),
                (1, 8, 5, 4097, 0, 1), (1, 8, 5, 4, 3, 1), (1, 8, 5, 5, 1, 1), (1, 8, 2 ** 31, 4, 0, 1)):
        assert ws(*bad) == 0, bad


def test_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    n0 = lib.bnn_launch_count()

    def call(y=one, nparts=1, nsamples=4, rows=8, width=6, kind=1, target=one, state=None, bins=20, ws=None, stride=None):
        return lib.bnn_mc_regression_score(y, rows * width if stride is None else stride, nparts, nsamples, rows, width, kind,
                                           target, one, one, one, one, one, one, one, state, bins, ws, None, 0, None)

    assert call(y=None) == -1 and b"NULL" in lib.bnn_last_error()
    assert call(target=None) == -1
    assert call(rows=0) == -2 and call(width=0) == -2 and call(nsamples=0) == -2 and call(nparts=0) == -2
    assert call(width=4098) == -5
    assert call(rows=2 ** 31) == -5
    assert call(nsamples=1025) == -5 and b"samples" in lib.bnn_last_error()
    assert call(kind=3) == -5 and b"kind" in lib.bnn_last_error()
    assert call(kind=-1) == -5
    assert call(width=5, kind=1) == -2 and call(width=5, kind=2) == -2       # odd width for a (mean, variance) layout
    assert call(stride=10) == -2                                     # overlapping addends
    for bins in (0, 129):
        assert call(state=one, bins=bins, ws=one) in (-2, -5)
    assert call(state=one, ws=None) == -1                            # a state needs the workspace
    assert call(nparts=3, ws=None) == -1                             # and so do a fused head's partials
    assert call(state=ctypes.c_void_p(20), ws=one) == -4 and call(state=one, ws=ctypes.c_void_p(18)) == -4
    assert lib.bnn_launch_count() == n0


def test_refusals():
    y, t = torch.zeros(2, 3, 4), torch.zeros(3, 2)
    for bad in (None, "logits", "MEAN_LOGVAR", 0):
        with pytest.raises(ValueError):
            ops.mc_regression_score(y, t, bad)
        with pytest.raises(ValueError):
            ops.regression_score_f64(y, t, bad)
    with pytest.raises(ValueError):
        ops.mc_regression_score(y, t)                                # `outputs` is required
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(y, t, "mean_logvar")                 # CPU tensors
    with pytest.raises(ValueError):
        ops.regression_score_f64(y, torch.zeros(3, 4), "mean_logvar")        # the target's shape is (*rows, D)
    with pytest.raises(ValueError):
        ops.regression_score_f64(torch.zeros(2, 3, 5), torch.zeros(3, 2), "mean_var")
    for D, bins in ((0, 20), (4097, 20), (2, 0), (2, 129)):
        with pytest.raises(ValueError):
            ops.RegressionScoreState("cpu", D, bins)
    net = MLP([6, 12, 4])
    x = torch.randn(7, 6)
    tt = torch.zeros(7, 2)
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        net.predictive_regression_score(x, tt, 4, outputs="logvar")  # refused before a draw is consumed
    with pytest.raises(TypeError):
        net.predictive_regression_score(x, tt, 4)                    # `outputs` is a required keyword
    assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(_lib.BnnHipError):
        net.predictive_regression_score(x, tt, 4, outputs="mean_logvar", advance=torch.zeros(1, dtype=torch.int32))


@pytest.mark.parametrize("outputs", list(KINDS))
def test_regression_score_f64_matches_float64_numpy(outputs):
    for S, rows, width, seed in ((1, 1, 2, 1), (8, 40, 6, 1), (5, 9, 34, 2), (33, 3, 4, 3)):
        y, t = make_case(S, rows, width, outputs, seed)
        if rows > 1:
            t[rows // 2, 0] = float("nan")                           # a NaN target among them
        ref = ref_elems(y.numpy(), t.numpy(), outputs)
        assert margins_hold(ref["pit"], PB)
        u, mat = ops.regression_score_f64(y, t, outputs, PB)
        assert isinstance(u, ops.RegressionScore) and mat.dtype == torch.float64 and u.crps.dtype == torch.float32
        check_elems(u, ref, (outputs, S, rows, width))
        check_state(mat.numpy(), ref, PB, (outputs, S, rows, width))
    # leading row dims
    y, t = make_case(4, 6, 6, outputs, 2)
    D = t.shape[-1]
    u, mat = ops.regression_score_f64(y.view(4, 2, 3, 6), t.view(2, 3, D), outputs)
    assert all(v.shape == (2, 3, D) for v in u) and mat.shape == (D, 26)
    check_elems(u, ref_elems(y.numpy(), t.numpy(), outputs))


def test_variance_edge_cases_in_float64():
    y, t = make_case(6, 9, 4, "mean_var", 5)
    y[::2, :, 2] = 0.0                                               # point masses among the samples of quantity 0
    y[1, 4, 3] = -1.0                                                # a negative variance in element (4, 1)
    ref = ref_elems(y.numpy(), t.numpy(), "mean_var")
    assert np.isnan(ref["nll"][:, 0]).all() and np.isfinite(ref["crps"][:, 0]).all() and np.isfinite(ref["pit"][:, 0]).all()
    assert all(np.isnan(ref[k][4, 1]) for k in ("nll", "crps", "pit")) and np.isfinite(ref["gaussian_nll"][4, 1])
    u, _ = ops.regression_score_f64(y, t, "mean_var")
    check_elems(u, ref, "edges")


def test_closed_forms_of_one_sample():
    gen = torch.Generator().manual_seed(9)
    m = torch.randn(1, 50, 1, generator=gen, dtype=torch.float64) * 3.0
    s = torch.rand(1, 50, 1, generator=gen, dtype=torch.float64) * 6.0 - 3.0
    t = torch.randn(50, 1, generator=gen, dtype=torch.float64) * 4.0
    u, _ = ops.regression_score_f64(torch.cat([m, s], -1), t, "mean_logvar")
    sg = np.exp(0.5 * s.numpy()[0])
    z = (t.numpy() - m.numpy()[0]) / sg
    want = sg * (z * (2.0 * Phi(z) - 1.0) + 2.0 * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) - 1.0 / math.sqrt(math.pi))
    assert np.abs(N(u.crps) - want).max() <= 1e-6 * np.abs(want).max()
    assert np.abs(ref_elems(torch.cat([m, s], -1).numpy(), t.numpy(), "mean_logvar")["crps"] - want).max() <= 1e-12
    assert np.abs(N(u.pit) - Phi(z)).max() <= 1e-7
    assert np.abs(N(u.nll) - N(u.gaussian_nll)).max() <= 1e-6        # one Gaussian is its own moment match
    # one point: the absolute error and a step
    v = torch.tensor([[[1.0], [2.0], [3.0]]], dtype=torch.float64)
    tv = torch.tensor([[0.5], [2.0], [7.0]], dtype=torch.float64)
    u, _ = ops.regression_score_f64(v, tv, "values")
    assert u.crps.reshape(-1).tolist() == [0.5, 0.0, 4.0] and u.pit.reshape(-1).tolist() == [0.0, 0.5, 1.0]
    assert torch.isnan(u.nll).all() and torch.isnan(u.gaussian_nll).all()    # no density: the variance is 0


def test_mixture_crps_is_the_integral_of_the_squared_cdf_difference():
    gen = torch.Generator().manual_seed(12)
    S = 5
    m = torch.randn(S, 1, 1, generator=gen, dtype=torch.float64) * 2.0
    s = torch.rand(S, 1, 1, generator=gen, dtype=torch.float64) * 3.0 - 2.0
    t = torch.tensor([[0.7]], dtype=torch.float64)
    y = torch.cat([m, s], -1)
    x = torch.linspace(-30.0, 30.0, 2 * 10 ** 6, dtype=torch.float64)
    F = torch.zeros_like(x)
    for i in range(S):
        F += 0.5 * torch.erfc(-(x - m[i, 0, 0]) / (torch.exp(0.5 * s[i, 0, 0]) * math.sqrt(2.0))) / S
    want = float(torch.trapezoid((F - (x >= t[0, 0]).to(torch.float64)) ** 2, x))
    ref = ref_elems(y.numpy(), t.numpy(), "mean_logvar")
    assert abs(float(ref["crps"][0, 0]) - want) <= 1e-5
    u, _ = ops.regression_score_f64(y, t, "mean_logvar")
    assert abs(float(u.crps) - want) <= 1e-5


def test_hand_built_calibration_case():
    """One standard normal, twenty targets on the mid-bin quantiles: one count in every bin, the calibration curve on the diagonal."""
    t = torch.tensor([[ndtri((k + 0.5) / 20.0)] for k in range(20)], dtype=torch.float64)
    y = torch.zeros(1, 20, 2, dtype=torch.float64)
    y[..., 1] = 1.0
    u, mat = ops.regression_score_f64(y, t, "mean_var", 20)
    assert np.abs(N(u.pit).reshape(20) - (np.arange(20) + 0.5) / 20.0).max() <= 1e-7
    st = ops.RegressionScoreState("cpu", 1, 20).add_(mat)
    r = st.result()
    assert isinstance(r, ops.RegressionScoreResult) and r.n == [20]
    assert r.pit_hist == [[1.0] * 20]
    assert [e for e, _ in r.calibration[0]] == [k / 20 for k in range(1, 21)]
    assert abs(r.calibration_error[0]) <= 1e-12
    assert r.coverage(0.9) == [0.9] and r.coverage(1.0) == [1.0] and r.coverage(0.5) == [0.5]
    with pytest.raises(ValueError):
        r.coverage(0.85)
    assert abs(r.sharpness[0] - 1.0) <= 1e-12
    assert abs(r.rmse[0] - math.sqrt(float((t ** 2).mean()))) <= 1e-6
    assert abs(r.nll[0] - r.gaussian_nll[0]) <= 1e-6 and abs(r.crps[0] - float(N(u.crps).mean())) <= 1e-7


@pytest.mark.parametrize("outputs", list(KINDS))
def test_cpu_module_matches_the_f64_path_on_the_same_draws(outputs):
    torch.manual_seed(0)
    net = MLP([6, 12, 4])
    x = torch.randn(7, 6)
    D = 4 if outputs == "values" else 2
    t = torch.randn(7, D)
    st = ops.RegressionScoreState("cpu", D)
    total = torch.zeros(D, 26, dtype=torch.float64)
    for seed in (3, 4):
        torch.manual_seed(seed)
        u = net.predictive_regression_score(x, t, 4, outputs=outputs, state=st)
        torch.manual_seed(seed)
        ys = net.forward_stacked(x, 4)
        if outputs == "mean_var":
            continue                                                 # (raw outputs as variances: negative ones, NaN scores)
        want, mat = ops.regression_score_f64(ys, t, outputs)
        total += mat
        for a, b in zip(u, want):
            assert a.shape == (7, D) and torch.equal(a, b)
        check_elems(u, ref_elems(ys.detach().numpy(), t.numpy(), outputs), outputs)
    if outputs != "mean_var":
        assert torch.equal(st.state, total)
        r = st.result()
        assert r.n == [14.0] * D and len(r.pit_hist) == D and all(sum(h) == 14 for h in r.pit_hist)
    assert st.reset() is st and float(st.state.abs().sum()) == 0.0
    with pytest.raises(_lib.BnnHipError):
        net.predictive_regression_score(x, t, 4, outputs=outputs, state=ops.ScoreState("cpu"))


def test_empty_state_gives_nan_ratios():
    r = ops.RegressionScoreState("cpu", 2, 4).result()
    assert r.n == [0.0, 0.0]
    for field in (r.rmse, r.nll, r.gaussian_nll, r.crps, r.sharpness, r.calibration_error, r.coverage(0.5)):
        assert len(field) == 2 and all(math.isnan(v) for v in field)
    assert r.pit_hist == [[0.0] * 4] * 2
    assert all(len(c) == 4 and all(math.isnan(obs) for _, obs in c) for c in r.calibration)


# ------------------------------------------------------------------------------------------------------------------ GPU
DEV = torch.device("cuda:0")

# (S, rows, width): the narrow / wide split at 16 / 17, the wave / workgroup split at 1024 / 1025, 16-byte and scalar loads
# (D % 4), more samples than the 64 lanes of a row, the S cap, single rows
SWEEP = [(1, 1, 1), (1, 1, 2), (2, 7, 6), (8, 513, 16), (33, 7, 17), (33, 7, 18), (65, 33, 2), (257, 7, 8), (1024, 2, 4),
         (8, 7, 300), (4, 5, 1024), (3, 5, 1025), (2, 3, 4096)]
CASES = [(S, rows, width, outputs) for S, rows, width in SWEEP for outputs in KINDS if outputs == "values" or width % 2 == 0]
# the seed of a case is the first for which margins_hold (asserted before anything runs)
SEEDS = {}


def _seed(S, rows, width, outputs):
    return SEEDS.get((S, rows, width, outputs), 0) + S * 7919 + rows * 31 + width


@functools.lru_cache(maxsize=None)
def _case(S, rows, width, outputs):
    y, t = make_case(S, rows, width, outputs, _seed(S, rows, width, outputs))
    assert margins_hold(ref_pit(y.numpy(), t.numpy(), outputs), PB), "pick another seed for this case"
    return y, t, ref_elems(y.numpy(), t.numpy(), outputs)


def _score(y, t, outputs, state=None, advance=None):
    return ops.mc_regression_score(y.to(DEV), t.to(DEV), outputs, state=state, advance=advance)


@gpu
@pytest.mark.parametrize("S,rows,width,outputs", CASES)
def test_kernel_against_float64(S, rows, width, outputs):
    y, t, ref = _case(S, rows, width, outputs)
    D = t.shape[-1]
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    u = _score(y, t, outputs)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1
    assert all(v.shape == (rows, D) and v.dtype == torch.float32 for v in u)
    check_elems(u, ref, (S, rows, width, outputs))
    # the mean and the variance are K12's bits
    k12 = ops.mc_regression(y.to(DEV), outputs)
    assert torch.equal(u.mean, k12.mean) and torch.equal(u.variance, k12.total)
    st = ops.RegressionScoreState(DEV, D, PB)
    st.workspace(1, S, rows, width, KINDS[outputs])
    n0 = lib.bnn_launch_count()
    v = _score(y, t, outputs, state=st)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() <= n0 + 2
    for a, b in zip(u, v):
        assert _same_bits(a, b)
    check_state(st.state.cpu().numpy(), ref, PB, (S, rows, width, outputs))


@gpu
def test_variance_edge_cases():
    for S, rows, width in ((6, 9, 4), (70, 5, 4), (6, 5, 40)):
        D = width // 2
        y, t = make_case(S, rows, width, "mean_var", 5 + S)
        y[::2, :, D] = 0.0                                           # point masses among the samples of quantity 0
        y[:, 0, D + 1] = 0.0                                         # only point masses: element (0, 1)
        y[1, rows - 1, D + 1] = -1.0                                 # a negative variance in element (rows - 1, 1)
        ref = ref_elems(y.numpy(), t.numpy(), "mean_var")
        assert np.isnan(ref["nll"][:, 0]).all() and np.isfinite(ref["crps"][:, 0]).all() and np.isfinite(ref["pit"][:, 0]).all()
        assert all(np.isnan(ref[k][rows - 1, 1]) for k in ("nll", "crps", "pit"))
        u = _score(y, t, "mean_var")
        check_elems(u, ref, ("edges", S, rows, width))
        assert torch.isnan(u.nll[:, 0]).all() and torch.isfinite(u.crps[:, 0]).all() and torch.isfinite(u.pit[:, 0]).all()
        assert all(bool(torch.isnan(getattr(u, k)[rows - 1, 1])) for k in ("nll", "crps", "pit"))


@gpu
@pytest.mark.parametrize("S,rows,width,outputs", [(8, 33, 6, "mean_logvar"), (8, 33, 5, "values"), (4, 9, 40, "mean_var"),
                                                  (3, 5, 2050, "mean_logvar")])
def test_nan_targets(S, rows, width, outputs):
    y, t = make_case(S, rows, width, outputs, 7 + width)
    D = t.shape[-1]
    bad = t.clone()
    where = [(3 % rows, 0), (rows - 1, D - 1), (rows // 2, D // 2)]
    for r, d in where:
        bad[r, d] = float("nan")
    s_ok, s_bad = ops.RegressionScoreState(DEV, D), ops.RegressionScoreState(DEV, D)
    good = _score(y, t, outputs, state=s_ok)
    u = _score(y, bad, outputs, state=s_bad)
    hit = torch.zeros(rows, D, dtype=torch.bool, device=DEV)
    for r, d in where:
        hit[r, d] = True
    assert _same_bits(u.mean, good.mean) and _same_bits(u.variance, good.variance)
    for name in SCORES:
        a, b = getattr(u, name), getattr(good, name)
        assert torch.isnan(a[hit]).all() and not torch.isnan(b).any()
        assert _same_bits(torch.where(hit, b, a), b)                 # every other element keeps its bits
    a, b = s_bad.state.cpu().numpy(), s_ok.state.cpu().numpy()
    cols = sorted({d for _, d in where})
    rest = [d for d in range(D) if d not in cols]
    assert (a[:, 0] == rows).all() and (b[:, 0] == rows).all()
    assert np.isnan(a[cols, 1:5]).all() and not np.isnan(b).any()
    assert (a[cols, 5] == b[cols, 5]).all()                          # the variance does not depend on the target
    assert (a[rest] == b[rest]).all()
    for d in cols:
        lost = sum(1 for _, dd in where if dd == d)
        assert a[d, 6:].sum() == rows - lost and b[d, 6:].sum() == rows      # a NaN pit counts in n and in no bin
        assert (a[d, 6:] <= b[d, 6:]).all()


@gpu
@pytest.mark.parametrize("parts,S,M,W", [(3, 4, 37, 6), (16, 8, 512, 2), (33, 70, 9, 16), (3, 4, 5, 40), (33, 2, 3, 1032)])
@pytest.mark.parametrize("outputs", list(KINDS))
def test_partials_give_the_bits_of_logits_then_the_launch(parts, S, M, W, outputs):
    gen = torch.Generator().manual_seed(parts * 100 + W)
    p = torch.randn(parts, S, M, W, generator=gen) * 0.5
    if outputs == "mean_var":
        p[..., W // 2:] = p[..., W // 2:].abs() + 0.01               # the parts add up to positive variances
    D = W if outputs == "values" else W // 2
    t = torch.randn(M, D, generator=gen).to(DEV)
    hp = ops.HeadPartials(p.to(DEV))
    s1, s2 = ops.RegressionScoreState(DEV, D), ops.RegressionScoreState(DEV, D)
    lib = _lib.load()
    s1.workspace(parts, S, M, W, KINDS[outputs])
    n0 = lib.bnn_launch_count()
    fused = ops.mc_regression_score(hp, t, outputs, state=s1)
    assert lib.bnn_launch_count() <= n0 + 2
    plain = ops.mc_regression_score(hp.logits(), t, outputs, state=s2)
    n0 = lib.bnn_launch_count()
    alone = ops.mc_regression_score(hp, t, outputs)
    assert lib.bnn_launch_count() == n0 + 1
    for a, b, c in zip(fused, plain, alone):
        assert not torch.isnan(a).any() and _same_bits(a, b) and _same_bits(a, c)
    assert torch.equal(s1.state, s2.state) and (s1.state[:, 0] == M).all()


# (S, rows, width, seed) of the three batches: fixed seeds whose elements all keep the margins at the default 20 bins
ACC = [(8, 1, 6, 100), (8, 7, 6, 100), (8, 513, 6, 100)]


@gpu
def test_accumulation_over_batches():
    batches = []
    for S, rows, width, seed in ACC:
        y, t = make_case(S, rows, width, "mean_logvar", seed)
        assert margins_hold(ref_pit(y.numpy(), t.numpy(), "mean_logvar"), 20), "pick another seed for this batch"
        batches.append((y, t, ref_elems(y.numpy(), t.numpy(), "mean_logvar")))
    both = {k: np.concatenate([b[2][k] for b in batches]) for k in batches[0][2]}
    st = ops.RegressionScoreState(DEV, 3)
    for y, t, _ in batches:
        _score(y, t, "mean_logvar", state=st)
    first = st.state.clone()
    check_state(first.cpu().numpy(), both, 20, "three batches")
    r = st.result()
    assert r.n == [521.0] * 3
    for d in range(3):
        assert abs(r.rmse[d] - math.sqrt(both["sq_err"][:, d].mean())) <= 1e-5 * max(1.0, math.sqrt(both["sq_err"][:, d].mean()))
        assert abs(r.crps[d] - both["crps"][:, d].mean()) <= 1e-5 * both["T1"][:, d].mean()
        assert abs(r.nll[d] - both["nll"][:, d].mean()) <= 1e-5 * np.maximum(1.0, np.abs(both["nll"][:, d])).mean()
        assert abs(r.sharpness[d] - math.sqrt(both["variance"][:, d].mean())) <= 1e-5 * math.sqrt(both["variance"][:, d].mean())
        hist = ref_state(both, 20)[d, 6:]
        assert r.pit_hist[d] == hist.tolist()
        assert abs(r.coverage(0.8)[d] - hist[2:18].sum() / 521.0) <= 1e-12
        cal = np.cumsum(hist) / 521.0
        assert np.abs(np.array([o for _, o in r.calibration[d]]) - cal).max() <= 1e-12
        assert abs(r.calibration_error[d] - np.abs(cal - np.arange(1, 21) / 20.0).mean()) <= 1e-12
    # a second identical run: the same bits; reset() zeroes
    again = ops.RegressionScoreState(DEV, 3)
    for y, t, _ in batches:
        _score(y, t, "mean_logvar", state=again)
    assert torch.equal(again.state, first)
    st.reset()
    assert float(st.state.abs().sum()) == 0.0 and st.result().n == [0.0] * 3


def _keys(layer):
    k = layer.weight.draw_key
    return (k.seed, k.stream, k.sample0, k.nsamples, k.epoch_host, k.gen)


@gpu
def test_fused_head_mlp_costs_at_most_one_extra_launch():
    from bayesianneuralnetworks_amd.nn import fuse_activations
    lib = _lib.load()
    torch.manual_seed(1)
    net = MLP([16, 48, 4], samples=8).to(DEV)
    seeded.pin_streams(net, 1220)
    net.mc_batched = True
    fuse_activations(net, bf16_activations=True, fuse_head=True)
    x = torch.randn(64, 16, device=DEV)
    t = torch.randn(64, 2, device=DEV)
    st = ops.RegressionScoreState(DEV, 2)
    bnn.set_compute("bf16")
    try:
        with torch.no_grad():
            bnn.manual_seed(4)
            hp = net._forward_batched_stacked(x, 8, 0, _lazy_head=True)
            assert isinstance(hp, ops.HeadPartials)
            st.workspace(hp.p.shape[0], 8, 64, 4, KINDS["mean_logvar"])
            ys = hp.logits()
            want = ops.mc_regression_score(ys, t, "mean_logvar")
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            u = net.predictive_regression_score(x, t, 8, outputs="mean_logvar")
            n_score = lib.bnn_launch_count() - n0
            keys_u = _keys(net.layers[2])
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            v = net.predictive_regression_score(x, t, 8, outputs="mean_logvar", state=st)
            n_state = lib.bnn_launch_count() - n0
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            net.predictive_regression(x, 8, outputs="mean_logvar")
            n_reg = lib.bnn_launch_count() - n0
            assert _keys(net.layers[2]) == keys_u                     # draws consumed as by predictive_regression
    finally:
        bnn.set_compute("f32")
    assert n_score == n_reg and n_state <= n_reg + 1
    for a, b, c in zip(u, v, want):
        assert _same_bits(a, b) and _same_bits(a, c)
    check_elems(u, ref_elems(N(ys), N(t), "mean_logvar"), "fused head")
    assert (st.state[:, 0] == 64).all()


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("batched", [True, False])
def test_module_paths_equal_the_op_on_forward_stacked(mode, batched):
    torch.manual_seed(2)
    net = MLP([12, 32, 2], samples=6).to(DEV)
    seeded.pin_streams(net, 1210)
    net.mc_batched = batched
    x = torch.randn(130, 12, device=DEV)
    t = torch.randn(130, 1, device=DEV)
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)
    bnn.set_compute(mode)
    try:
        with torch.no_grad():
            bnn.manual_seed(8)
            u = net.predictive_regression_score(x, t, 6, 2, outputs="mean_logvar", advance=cell)
            assert int(cell.item()) == 1
            bnn.manual_seed(8)
            ys = net.forward_stacked(x, 6, 2)
            want = ops.mc_regression_score(ys, t, "mean_logvar")
            bnn.manual_seed(8)
            net.predictive_regression_score(x, t, 6, 2, outputs="mean_logvar", advance=cell)
            assert int(cell.item()) == 2
    finally:
        bnn.set_compute("f32")
    for a, b in zip(u, want):
        assert a.shape == (130, 1) and torch.equal(a, b)
    check_elems(u, ref_elems(N(ys), N(t), "mean_logvar"), (mode, batched))


@gpu
def test_shapes_dtypes_and_devices():
    y, t = make_case(6, 15, 6, "mean_logvar", 5)
    y, t = y.view(6, 3, 5, 6), t.view(3, 5, 3)
    yt, tt = y.to(DEV).transpose(1, 2), t.to(DEV).transpose(0, 1)     # (6, 5, 3, 6) and (5, 3, 3), not contiguous
    u = ops.mc_regression_score(yt, tt, "mean_logvar")
    assert all(v.shape == (5, 3, 3) for v in u)
    ref = ref_elems(yt.cpu().contiguous().numpy().reshape(6, 15, 6), tt.cpu().contiguous().numpy().reshape(15, 3), "mean_logvar")
    check_elems(u, ref, "leading dims")
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(yt, tt.reshape(15, 3), "mean_logvar")        # the targets' shape is (*rows, D)
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(yt, tt.double(), "mean_logvar")
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(yt, tt.cpu(), "mean_logvar")
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(yt.double(), tt, "mean_logvar")
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(yt[..., :5], tt, "mean_var")                 # an odd width
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(yt, tt, "mean_logvar", state=ops.RegressionScoreState("cpu", 3))
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(yt, tt, "mean_logvar", state=ops.RegressionScoreState(DEV, 2))
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(yt, tt, "mean_logvar", state=ops.ScoreState(DEV))
    with pytest.raises(_lib.BnnHipError):
        ops.mc_regression_score(torch.zeros(1025, 1, 2, device=DEV), torch.zeros(1, 1, device=DEV), "mean_logvar")


@gpu
def test_captured_graph_replays_accumulate_and_advance():
    y, t = make_case(8, 130, 6, "mean_logvar", 21)
    y, t = y.to(DEV), t.to(DEV)
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)
    eager = ops.RegressionScoreState(DEV, 3)
    for _ in range(3):
        ops.mc_regression_score(y, t, "mean_logvar", state=eager, advance=cell)
    assert int(cell.item()) == 3
    st = ops.RegressionScoreState(DEV, 3)
    ops.mc_regression_score(y, t, "mean_logvar", state=st, advance=cell)     # warm up outside the capture (sizes the workspace)
    st.reset()
    cell.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # captured on a side stream: one linear chain of two launches
        ops.mc_regression_score(y, t, "mean_logvar", state=st, advance=cell)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(st.state, eager.state) and (st.state[:, 0] == 390).all()
    assert int(cell.item()) == 3
