"""Scoring an MC forward against its labels (bnn_mc_score, ops.mc_score, ops.ScoreState, ops.score_f64,
BayesianNetworkModule.predictive_score): per row the predictive mean, the NLL of the MC predictive, the expected per-sample NLL,
the Brier score, the confidence, the prediction and the entropy; over a test set the accuracy, ECE / MCE with the reliability
diagram and the accuracy-rejection curve, accumulated on the device.

CPU: the float64 torch path and the module's CPU path against a NumPy restatement, a hand-built calibration case, the refusals,
the C-ABI's argument errors.  GPU: the kernel against float64 over both work splits and both input kinds, the log-domain NLL,
a fused head's partials, accumulation over batches, invalid targets, launch counts, the module's paths and modes, graph capture."""
import ctypes
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
CB, EB = 15, 20                                                     # the default bins
# The bins of the tests on the uncertainty tests' generators.  Their one-hot rows (and the logits rows of scale 30, one-hot to
# 1e-13) put the confidence on k / S and the normalised entropy on ratios of logarithms of small integers -- ln 8 / ln 16 = 3 / 4,
# ln 8 / ln 1024 = 3 / 10 --, that is ON interior edges of 15 and 20 bins whatever the seed (S = 3: a confidence of 1 / 3 = 5 / 15).
# No S of the sweep is a multiple of 7 and no such ratio has a denominator that 11 divides, so these bin counts keep every row
# of a suitable seed away from the edges.
KB = (7, 11)


# ---------------------------------------------------------------------------------------------------- float64 NumPy reference
def ref_rows(y, t, inputs):
    """y (S, rows, C), t (rows) int64 -> dict of float64 per-row arrays (prediction int64): the issue's formulas."""
    y = np.asarray(y, dtype=np.float64)
    t = np.asarray(t, dtype=np.int64)
    S, R, C = y.shape
    ok = (t >= 0) & (t < C)
    tc = np.where(ok, t, 0)
    pick = lambda a: np.take_along_axis(a, np.broadcast_to(tc[None, :, None], (a.shape[0], R, 1)), -1)[..., 0]     # noqa: E731
    if inputs == "logits":
        z = y - y.max(-1, keepdims=True)
        lp = z - np.log(np.exp(z).sum(-1, keepdims=True))
        m = np.exp(lp).mean(0)
        lpy = pick(lp)                                              # (S, rows)
        mx = lpy.max(0)
        nll = -(mx + np.log(np.exp(lpy - mx).sum(0)) - np.log(S))
        enll = -lpy.mean(0)
        ent = -np.where(m > 0, m * np.log(np.where(m > 0, m, 1.0)), 0.0).sum(-1)
    else:
        m = y.mean(0)
        nll = -np.log(pick(m[None])[0] + 1e-10)
        enll = -np.log(pick(y) + 1e-10).mean(0)
        ent = -(m * np.log(m + 1e-10)).sum(-1)
    onehot = np.zeros_like(m)
    onehot[np.arange(R), tc] = 1.0
    brier = ((m - onehot) ** 2).sum(-1)
    nan = np.full(R, np.nan)
    pred = m.argmax(-1)                                             # numpy: the first (lowest) maximum
    return dict(mean=m, nll=np.where(ok, nll, nan), expected_nll=np.where(ok, enll, nan), brier=np.where(ok, brier, nan),
                confidence=m.max(-1), prediction=pred, entropy=ent, correct=ok & (pred == t))


def ref_bins(ref, C, cb=CB, eb=EB):
    cbin = np.minimum(cb - 1, np.floor(ref["confidence"] * cb)).astype(np.int64)
    ebin = np.clip(np.floor(ref["entropy"] / np.log(C) * eb), 0, eb - 1).astype(np.int64)
    return cbin, ebin


def ref_state(ref, C, cb=CB, eb=EB):
    """The accumulator's vector of one batch, float64."""
    cbin, ebin = ref_bins(ref, C, cb, eb)
    k = ref["correct"].astype(np.float64)
    v = np.zeros(5 + 3 * cb + 2 * eb)
    v[:5] = [len(k), ref["nll"].sum(), ref["expected_nll"].sum(), ref["brier"].sum(), k.sum()]
    for b in range(cb):
        sel = cbin == b
        v[5 + 3 * b:8 + 3 * b] = [sel.sum(), ref["confidence"][sel].sum(), k[sel].sum()]
    for b in range(eb):
        sel = ebin == b
        v[5 + 3 * cb + 2 * b:7 + 3 * cb + 2 * b] = [sel.sum(), k[sel].sum()]
    return v


def ref_result(v, cb=CB, eb=EB):
    """ece, mce, rejection [(coverage, accuracy)] of a state vector."""
    n = v[0]
    bins = v[5:5 + 3 * cb].reshape(cb, 3)
    full = bins[:, 0] > 0
    gap = np.abs(bins[full, 2] / bins[full, 0] - bins[full, 1] / bins[full, 0])
    ece = float((bins[full, 0] / n * gap).sum())
    e = v[5 + 3 * cb:].reshape(eb, 2).cumsum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rej = np.stack([e[:, 0] / n, e[:, 1] / e[:, 0]], -1)
    return ece, float(gap.max()), rej


def margins_hold(ref, C, cb=CB, eb=EB):
    """Exact predictions and bins need inputs away from ties and bin edges: every row's float64 top two means differ by more than
    1e-5 or are exactly equal, its confidence is more than 1e-5 from every interior edge k / cb, its normalised entropy more than
    1e-4 from every interior edge k / eb."""
    top = np.sort(ref["mean"], -1)[:, -2:]
    gap = top[:, 1] - top[:, 0]
    if not ((gap > 1e-5) | (gap == 0.0)).all():
        return False
    c = ref["confidence"] * cb
    h = ref["entropy"] / np.log(C) * eb
    dc = np.where((np.rint(c) >= 1) & (np.rint(c) <= cb - 1), np.abs(c - np.rint(c)) / cb, 1.0)
    dh = np.where((np.rint(h) >= 1) & (np.rint(h) <= eb - 1), np.abs(h - np.rint(h)) / eb, 1.0)
    return bool((dc > 1e-5).all() and (dh > 1e-4).all())


def N(t):
    return t.detach().double().cpu().numpy()


def check_rows(u, ref, C, what=""):
    """The issue's tolerances (fp32 per-sample terms under fp64 sums)."""
    R = ref["nll"].shape[0]
    assert np.abs(N(u.mean).reshape(R, C) - ref["mean"]).max() <= 1e-6, (what, "mean")
    assert np.abs(N(u.confidence).reshape(R) - ref["confidence"]).max() <= 1e-6, (what, "confidence")
    assert np.abs(N(u.entropy).reshape(R) - ref["entropy"]).max() <= 1e-5 * max(1.0, math.log(C)), (what, "entropy")
    for name in ("nll", "expected_nll", "brier"):
        got, want = N(getattr(u, name)).reshape(R), ref[name]
        bad = np.isnan(want)
        assert (np.isnan(got) == bad).all(), (what, name, "NaN rows")
        err = np.abs(got[~bad] - want[~bad]) - 1e-5 * np.maximum(1.0, np.abs(want[~bad]))
        assert (err <= 0).all(), (what, name, float(err.max()))
    assert u.prediction.dtype == torch.int64
    assert (u.prediction.cpu().numpy().reshape(R) == ref["prediction"]).all(), (what, "prediction")


def check_state(got, ref, what="", cb=CB, eb=EB):
    """Counts exact, sums within the per-row tolerance x n.  ref: the float64 rows of everything that went into `got`."""
    C = ref["mean"].shape[-1]
    got = np.asarray(got, dtype=np.float64)
    want = ref_state(ref, C, cb, eb)
    n = want[0]
    counts = [0, 4] + [5 + 3 * b + j for b in range(cb) for j in (0, 2)] + list(range(5 + 3 * cb, 5 + 3 * cb + 2 * eb))
    assert (got[counts] == want[counts]).all(), (what, "counts")
    for i, name in ((1, "nll"), (2, "expected_nll"), (3, "brier")):
        if np.isnan(want[i]):
            assert np.isnan(got[i]), (what, name)
        else:
            assert abs(got[i] - want[i]) <= 1e-5 * np.maximum(1.0, np.abs(ref[name])).sum(), (what, name, got[i], want[i])
    for b in range(cb):
        assert abs(got[6 + 3 * b] - want[6 + 3 * b]) <= 1e-6 * max(1.0, want[5 + 3 * b]), (what, "sum confidence", b)
    assert n == ref["nll"].shape[0]


# the generators of test_predictive_uncertainty.py: scales 0.3 / 3 / 30, offsets +-70; exact zeros and one-hot rows for probs
def _logits(S, rows, C, gen):
    scale = torch.tensor([0.3, 3.0, 30.0])[torch.randint(0, 3, (rows, 1), generator=gen)]
    offset = torch.tensor([0.0, 70.0, -70.0])[torch.randint(0, 3, (rows, 1), generator=gen)]
    return (torch.randn(S, rows, C, generator=gen) * scale + offset).clamp_(-80.0, 80.0)


def _probs(S, rows, C, gen):
    p = torch.softmax(torch.randn(S, rows, C, generator=gen) * 2.0, -1)
    p = p * (torch.rand(S, rows, C, generator=gen) > 0.3)                  # exact zeros
    p = p / p.sum(-1, keepdim=True).clamp_min(1e-30)
    hot = torch.nn.functional.one_hot(torch.randint(0, C, (S, rows), generator=gen), C).float()
    p = torch.where((torch.arange(rows) % 3 == 0).view(1, rows, 1), hot, p)   # one-hot rows
    return p.float()


def make_case(S, rows, C, inputs, seed):
    """(y fp32 (S, rows, C), uniform labels) of one fixed seed."""
    gen = torch.Generator().manual_seed(seed)
    y = _logits(S, rows, C, gen) if inputs == "logits" else _probs(S, rows, C, gen)
    t = torch.randint(0, C, (rows,), generator=gen)
    return y, t


class MLP(BayesianNetworkModule):
    def __init__(self, dims, samples=4, softmax=False):
        super().__init__(dims[0], dims[-1], samples)
        mods = []
        for i in range(len(dims) - 1):
            mods.append(NormalLinear(dims[i], dims[i + 1]))
            if i < len(dims) - 2:
                mods.append(torch.nn.ReLU())
        if softmax:
            mods.append(torch.nn.Softmax(dim=-1))
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    lib = _lib.load()
    for name in ("bnn_mc_score", "bnn_mc_score_workspace_bytes", "bnn_mc_score_state_doubles"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.bnn_mc_score_state_doubles(15, 20) == 5 + 45 + 40 == ops.score_state_size(15, 20)
    assert lib.bnn_mc_score_state_doubles(0, 20) == 0 and lib.bnn_mc_score_state_doubles(15, 129) == 0
    assert lib.bnn_mc_score_workspace_bytes(513) >= 513 * 20 and lib.bnn_mc_score_workspace_bytes(0) == 0
    assert "bnn_score.hip" in open(os.path.join(ROOT, "bayesianneuralnetworks_amd", "csrc", "Makefile")).read()


def test_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    n0 = lib.bnn_launch_count()

    def call(y=one, nparts=1, nsamples=4, rows=8, classes=10, kind=0, target=one, state=None, cb=15, eb=20, ws=None, stride=None):
        return lib.bnn_mc_score(y, rows * classes if stride is None else stride, nparts, nsamples, rows, classes, kind, target,
                                one, one, one, one, one, one, one, state, cb, eb, ws, None, 0, None)

    assert call(y=None) == -1 and b"NULL" in lib.bnn_last_error()
    assert call(target=None) == -1
    assert call(rows=0) == -2
    assert call(classes=1) in (-2, -5) and call(classes=0) in (-2, -5)
    assert call(classes=4097) == -5
    assert call(nsamples=0) == -2
    assert call(nsamples=65537) == -5
    assert call(nparts=0) == -2
    assert call(kind=2) == -5 and b"kind" in lib.bnn_last_error()
    assert call(stride=10) == -2                                     # overlapping addends
    for cb, eb in ((0, 20), (15, 0), (129, 20), (15, 129)):
        assert call(state=one, cb=cb, eb=eb, ws=one) in (-2, -5)
    assert call(state=one, ws=None) == -1                            # a state needs the workspace
    assert lib.bnn_launch_count() == n0


def test_refusals():
    y, t = torch.zeros(2, 3, 4), torch.zeros(3, dtype=torch.int64)
    for bad in (None, "softmax", "LOGITS", 0):
        with pytest.raises(ValueError):
            ops.mc_score(y, t, bad)
        with pytest.raises(ValueError):
            ops.score_f64(y, t, bad)
    with pytest.raises(ValueError):
        ops.mc_score(y, t)                                           # `inputs` is required
    with pytest.raises(_lib.BnnHipError):
        ops.mc_score(y, t, "logits")                                 # CPU tensors
    with pytest.raises(ValueError):
        ops.ScoreState("cpu", conf_bins=0)
    with pytest.raises(ValueError):
        ops.ScoreState("cpu", ent_bins=129)
    net = MLP([6, 12, 5])
    x = torch.randn(7, 6)
    tt = torch.zeros(7, dtype=torch.int64)
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        net.predictive_score(x, tt, 4, inputs="softmax")             # refused before a draw is consumed
    with pytest.raises(TypeError):
        net.predictive_score(x, tt, 4)                               # `inputs` is a required keyword
    assert torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_score_f64_matches_float64_numpy(inputs):
    for S, rows, C, seed in ((1, 1, 2, 1), (8, 40, 10, 1), (5, 9, 33, 2)):
        y, t = make_case(S, rows, C, inputs, seed)
        t[rows // 2] = -1 if rows > 1 else t[0]                      # an invalid target among them
        ref = ref_rows(y.numpy(), t.numpy(), inputs)
        assert margins_hold(ref, C, *KB)
        u, vec = ops.score_f64(y, t, inputs, *KB)
        assert isinstance(u, ops.PredictiveScore) and vec.dtype == torch.float64
        check_rows(u, ref, C, (S, rows, C))
        check_state(vec.numpy(), ref, (S, rows, C), *KB)
    # leading row dims
    y, t = make_case(4, 6, 5, inputs, 2)
    u, vec = ops.score_f64(y.view(4, 2, 3, 5), t.view(2, 3), inputs)
    assert u.mean.shape == (2, 3, 5) and u.nll.shape == u.prediction.shape == (2, 3)
    check_rows(u, ref_rows(y.numpy(), t.numpy(), inputs), 5)


@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_cpu_module_matches_float64_numpy_on_the_same_draws(inputs):
    torch.manual_seed(0)
    net = MLP([6, 12, 5], softmax=inputs == "probs")
    x = torch.randn(7, 6)
    t = torch.randint(0, 5, (7,))
    st = ops.ScoreState("cpu")
    refs = []
    for seed in (3, 4):
        torch.manual_seed(seed)
        u = net.predictive_score(x, t, 4, inputs=inputs, state=st)
        torch.manual_seed(seed)
        ys = net.forward_stacked(x, 4)
        refs.append(ref_rows(ys.detach().numpy(), t.numpy(), inputs))
        assert margins_hold(refs[-1], 5)
        assert u.mean.shape == (7, 5) and u.nll.shape == (7,) and u.prediction.dtype == torch.int64
        check_rows(u, refs[-1], 5)
    both = {k: np.concatenate([r[k] for r in refs]) for k in refs[0]}
    check_state(st.state.numpy(), both)
    r = st.result()
    ece, mce, rej = ref_result(ref_state(both, 5))
    assert r.n == 14 and abs(r.accuracy - both["correct"].mean()) <= 1e-12
    assert abs(r.nll - both["nll"].mean()) <= 1e-5 and abs(r.brier - both["brier"].mean()) <= 1e-5
    assert abs(r.ece - ece) <= 1e-6 and abs(r.mce - mce) <= 1e-6
    assert st.reset() is st and float(st.state.abs().sum()) == 0.0
    with pytest.raises(_lib.BnnHipError):
        net.predictive_score(x, t, 4, inputs=inputs, advance=torch.zeros(1, dtype=torch.int32))


def test_hand_built_calibration_case():
    """Ten rows of two classes, one sample, probabilities as given: the confidences, labels and entropies are known, so ECE, MCE,
    the reliability diagram (5 bins) and the rejection curve (4 bins) are written out by hand."""
    conf = [0.55, 0.58, 0.65, 0.72, 0.75, 0.85, 0.88, 0.95, 0.97, 0.99]
    right = [1, 0, 1, 1, 0, 1, 1, 1, 1, 0]
    y = torch.zeros(1, 10, 2, dtype=torch.float64)
    t = torch.zeros(10, dtype=torch.int64)
    for r, (c, k) in enumerate(zip(conf, right)):
        pred = r % 2                                                 # the confident class alternates
        y[0, r, pred], y[0, r, 1 - pred] = c, 1.0 - c
        t[r] = pred if k else 1 - pred
    # normalised entropies (bits): .9928 .9815 .9341 .8555 .8113 | .6098 .5294 | .2864 | .1944 .0808
    h = [-(c * math.log2(c) + (1 - c) * math.log2(1 - c)) for c in conf]
    assert [int(v * 4) for v in h] == [3, 3, 3, 3, 3, 2, 2, 1, 0, 0]
    u, vec = ops.score_f64(y, t, "probs", conf_bins=5, ent_bins=4)
    assert u.prediction.tolist() == [r % 2 for r in range(10)]
    assert np.abs(N(u.confidence) - np.array(conf)).max() <= 1e-7
    assert np.abs(N(u.entropy) / math.log(2) - np.array(h)).max() <= 1e-6
    st = ops.ScoreState("cpu", conf_bins=5, ent_bins=4).add_(vec)
    r = st.result()
    assert r.n == 10 and r.accuracy == 0.7
    # bins [.4, .6): rows 0-1, [.6, .8): rows 2-4, [.8, 1]: rows 5-9
    want_rel = [(0, None, None), (0, None, None), (2, 0.565, 0.5), (3, 2.12 / 3, 2 / 3), (5, 0.928, 0.8)]
    for (cnt, c, a), (wc, wconf, wacc) in zip(r.reliability, want_rel):
        assert cnt == wc
        if wc == 0:
            assert math.isnan(c) and math.isnan(a)
        else:
            assert abs(c - wconf) <= 1e-7 and abs(a - wacc) <= 1e-12
    assert abs(r.ece - (0.2 * 0.065 + 0.3 * (2.12 / 3 - 2 / 3) + 0.5 * 0.128)) <= 1e-7       # 0.089
    assert abs(r.mce - 0.128) <= 1e-7
    # keep the least uncertain 20 %, 30 %, 50 %, 100 %
    want_rej = [(0.2, 0.5), (0.3, 2 / 3), (0.5, 0.8), (1.0, 0.7)]
    for (cov, acc), (wcov, wacc) in zip(r.rejection, want_rej):
        assert abs(cov - wcov) <= 1e-12 and abs(acc - wacc) <= 1e-12
    assert abs(r.nll - np.mean([-math.log((c if k else 1 - c) + 1e-10) for c, k in zip(conf, right)])) <= 1e-6
    assert abs(r.brier - np.mean([2 * (1 - c) ** 2 if k else 2 * c ** 2 for c, k in zip(conf, right)])) <= 1e-6
    assert abs(r.expected_nll - r.nll) <= 1e-6                       # one sample


def test_empty_state_gives_nan_ratios():
    r = ops.ScoreState("cpu", 3, 2).result()
    assert r.n == 0
    for v in (r.accuracy, r.nll, r.expected_nll, r.brier, r.ece, r.mce):
        assert math.isnan(v)
    assert len(r.reliability) == 3 and all(c == 0 and math.isnan(a) and math.isnan(b) for c, a, b in r.reliability)
    assert len(r.rejection) == 2 and all(math.isnan(a) and math.isnan(b) for a, b in r.rejection)


# ------------------------------------------------------------------------------------------------------------------ GPU
DEV = torch.device("cuda:0")

# (S, rows, C): the narrow / wide split at 16 / 17, the wave / workgroup split at 1024 / 1025, more samples than the 64 lanes of a
# row, single rows; the seed of each (kind, case) is the first for which margins_hold (asserted before anything runs)
SWEEP = [(1, 1, 2), (2, 7, 10), (8, 513, 16), (33, 7, 17), (65, 33, 10), (257, 7, 100), (1024, 2, 10), (8, 7, 300), (8, 7, 1024),
         (3, 5, 1025), (2, 3, 4096)]
SEEDS = {(8, 513, 16, 'logits'): 5, (257, 7, 100, 'logits'): 2, (8, 7, 1024, 'logits'): 11, (3, 5, 1025, 'logits'): 2,
         (2, 3, 4096, 'logits'): 3, (8, 513, 16, 'probs'): 6}


def _seed(S, rows, C, inputs):
    return SEEDS.get((S, rows, C, inputs), 0) + S * 7919 + rows * 31 + C


def _score(y, t, inputs, state=None, advance=None):
    return ops.mc_score(y.to(DEV), t.to(DEV), inputs, state=state, advance=advance)


@gpu
@pytest.mark.parametrize("S,rows,C", SWEEP)
@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_kernel_against_float64(S, rows, C, inputs):
    y, t = make_case(S, rows, C, inputs, _seed(S, rows, C, inputs))
    ref = ref_rows(y.numpy(), t.numpy(), inputs)
    assert margins_hold(ref, C, *KB), "pick another seed for this case"
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    u = _score(y, t, inputs)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1
    assert u.mean.shape == (rows, C) and u.nll.shape == (rows,)
    check_rows(u, ref, C, (S, rows, C, inputs))
    # the mean and the entropy are K4's bits
    k4 = ops.mc_uncertainty(y.to(DEV), inputs)
    assert torch.equal(u.mean, k4.mean) and torch.equal(u.entropy, k4.total)
    st = ops.ScoreState(DEV, *KB)
    n0 = lib.bnn_launch_count()
    v = _score(y, t, inputs, state=st)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() <= n0 + 2
    for a, b in zip(u, v):
        assert torch.equal(a, b)
    check_state(st.state.cpu().numpy(), ref, (S, rows, C, inputs), *KB)


@gpu
@pytest.mark.parametrize("C", [10, 100])
def test_nll_is_formed_in_the_log_domain(C):
    """Row 0: the label 200 below the row's max in every sample (p_s[y] = e^-200 underflows fp32: -ln of the fp32 mean is inf);
    row 1: only one sample in 64 gives the label any mass."""
    gen = torch.Generator().manual_seed(C)
    y = torch.randn(64, 2, C, generator=gen)
    y[:, 0, 0] += 200.0
    y[1:, 1, 3] = -1000.0
    t = torch.tensor([C - 1, 3])
    ref = ref_rows(y.numpy(), t.numpy(), "logits")
    assert 195.0 < ref["nll"][0] < 205.0 and math.log(64) < ref["nll"][1] < math.log(64) + 12.0
    u = _score(y, t, "logits")
    got = N(u.nll)
    assert np.isfinite(got).all()
    assert (np.abs(got - ref["nll"]) <= 1e-5 * np.abs(ref["nll"])).all(), (got, ref["nll"])
    got = N(u.expected_nll)
    assert (np.abs(got - ref["expected_nll"]) <= 1e-5 * np.abs(ref["expected_nll"])).all(), (got, ref["expected_nll"])


@gpu
@pytest.mark.parametrize("parts,S,M,C", [(3, 4, 37, 10), (16, 8, 512, 10), (33, 2, 9, 10), (5, 4, 6, 40)])
@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_partials_give_the_bits_of_logits_then_the_launch(parts, S, M, C, inputs):
    gen = torch.Generator().manual_seed(parts * 100 + C)
    if inputs == "logits":
        p = torch.randn(parts, S, M, C, generator=gen) * 0.5
    else:
        p = torch.rand(parts, S, M, C, generator=gen) * (2.0 / (parts * C))     # non-negative: the parts sum to a probability-like row
    t = torch.randint(0, C, (M,), generator=gen).to(DEV)
    hp = ops.HeadPartials(p.to(DEV))
    s1, s2 = ops.ScoreState(DEV), ops.ScoreState(DEV)
    fused = ops.mc_score(hp, t, inputs, state=s1)
    plain = ops.mc_score(hp.logits(), t, inputs, state=s2)
    for a, b in zip(fused, plain):
        assert torch.equal(a, b)
    assert torch.equal(s1.state, s2.state) and float(s1.state[0]) == M


# (S, rows, C, seed) of the three batches: fixed seeds whose rows all keep the margins at the default bins (found by search: five
# rows in 513 of the logits generator have near-ties among their top two means)
ACC = {"logits": [(8, 1, 10, 100), (8, 7, 10, 100), (8, 513, 10, 2472)],
       "probs": [(8, 1, 10, 100), (8, 7, 10, 100), (8, 513, 10, 103)]}


def _batches(inputs):
    out = []
    for S, rows, C, seed in ACC[inputs]:
        y, t = make_case(S, rows, C, inputs, seed)
        ref = ref_rows(y.numpy(), t.numpy(), inputs)
        assert margins_hold(ref, C), "pick another seed for this batch"
        out.append((y, t, ref))
    return out


@gpu
@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_accumulation_over_batches(inputs):
    batches = _batches(inputs)
    both = {k: np.concatenate([b[2][k] for b in batches]) for k in batches[0][2]}
    st = ops.ScoreState(DEV)
    for y, t, _ in batches:
        _score(y, t, inputs, state=st)
    first = st.state.clone()
    check_state(first.cpu().numpy(), both, inputs)
    r = st.result()
    ece, mce, rej = ref_result(ref_state(both, 10))
    assert r.n == 521 and r.accuracy == both["correct"].mean()
    assert abs(r.ece - ece) <= 1e-5 and abs(r.mce - mce) <= 1e-5
    got = np.array(r.rejection)
    assert got.shape == rej.shape and (np.isnan(got) == np.isnan(rej)).all()
    assert np.nanmax(np.abs(got - rej)) <= 1e-5
    for name in ("nll", "expected_nll", "brier"):
        assert abs(getattr(r, name) - both[name].mean()) <= 1e-5 * max(1.0, float(np.abs(both[name]).mean()))
    # a second identical run: the same bits; reset() zeroes
    again = ops.ScoreState(DEV)
    for y, t, _ in batches:
        _score(y, t, inputs, state=again)
    assert torch.equal(again.state, first)
    st.reset()
    assert float(st.state.abs().sum()) == 0.0 and st.result().n == 0


@gpu
@pytest.mark.parametrize("C", [10, 100, 1100])
@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_invalid_targets(C, inputs):
    y, t = make_case(4, 33, C, inputs, 7 + C)
    bad = t.clone()
    bad[3], bad[17], bad[32] = -1, C, 2 ** 32                         # (2^32 narrows to class 0)
    t[32] = 0
    s_ok, s_bad = ops.ScoreState(DEV), ops.ScoreState(DEV)
    good = _score(y, t, inputs, state=s_ok)
    u = _score(y, bad, inputs, state=s_bad)
    rows = torch.tensor([3, 17, 32], device=DEV)
    keep = torch.ones(33, dtype=torch.bool, device=DEV)
    keep[rows] = False
    for name in ("nll", "expected_nll", "brier"):
        a, b = getattr(u, name), getattr(good, name)
        assert torch.isnan(a[rows]).all() and torch.equal(a[keep], b[keep]) and not torch.isnan(b).any()
    for name in ("mean", "confidence", "prediction", "entropy"):
        assert torch.equal(getattr(u, name), getattr(good, name))
    a, b = s_bad.state.cpu().numpy(), s_ok.state.cpu().numpy()
    assert np.isnan(a[1:4]).all() and not np.isnan(b).any()
    assert a[0] == b[0] == 33
    lost = float((good.prediction[rows] == t.to(DEV)[rows]).sum())      # those rows no longer count as correct
    assert a[4] == b[4] - lost
    cnt = [5 + 3 * k for k in range(CB)] + [5 + 3 * CB + 2 * k for k in range(EB)]
    csum = [6 + 3 * k for k in range(CB)]
    assert (a[cnt] == b[cnt]).all() and (a[csum] == b[csum]).all()
    assert a[[7 + 3 * k for k in range(CB)]].sum() == a[4] == a[[6 + 3 * CB + 2 * k for k in range(EB)]].sum()


def _keys(layer):
    k = layer.weight.draw_key
    return (k.seed, k.stream, k.sample0, k.nsamples, k.epoch_host, k.gen)


@gpu
def test_fused_head_mlp_costs_at_most_one_extra_launch():
    from bayesianneuralnetworks_amd.nn import fuse_activations
    lib = _lib.load()
    torch.manual_seed(1)
    net = MLP([784, 1200, 1200, 10], samples=4).to(DEV)
    seeded.pin_streams(net, 1000)
    net.mc_batched = True
    fuse_activations(net, bf16_activations=True, fuse_head=True)
    x = torch.randn(64, 784, device=DEV)
    t = torch.randint(0, 10, (64,), device=DEV)
    st = ops.ScoreState(DEV)
    st.workspace(64)
    bnn.set_compute("bf16")
    try:
        with torch.no_grad():
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            u = net.predictive_score(x, t, 4, inputs="logits")
            n_score = lib.bnn_launch_count() - n0
            keys_u = _keys(net.layers[4])
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            v = net.predictive_score(x, t, 4, inputs="logits", state=st)
            n_state = lib.bnn_launch_count() - n0
            bnn.manual_seed(4)
            hp = net._forward_batched_stacked(x, 4, 0, _lazy_head=True)
            assert isinstance(hp, ops.HeadPartials)
            logits = hp.logits()
            want = ops.mc_score(logits, t, "logits")
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            net.predictive_mean(x, 4)
            n_pm = lib.bnn_launch_count() - n0
            assert _keys(net.layers[4]) == keys_u                     # draws consumed as by predictive_mean
    finally:
        bnn.set_compute("f32")
    assert n_score == n_pm and n_state <= n_pm + 1
    for a, b, c in zip(u, v, want):
        assert torch.equal(a, b) and torch.equal(a, c)
    ref = ref_rows(N(logits), t.cpu().numpy(), "logits")
    for name in ("nll", "expected_nll", "brier"):
        assert (np.abs(N(getattr(u, name)) - ref[name]) <= 1e-5 * np.maximum(1.0, np.abs(ref[name]))).all()
    assert float(st.state[0]) == 64


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("batched", [True, False])
def test_module_paths_equal_the_op_on_forward_stacked(mode, batched):
    """Both modes: the bits of ops.mc_score on forward_stacked's output at the same sample0, and within the kernel's bounds of the
    float64 formulas on that output (the bound of test_predictive_uncertainty.py for the bf16 mode: the mode changes the
    network's outputs, not the tail)."""
    torch.manual_seed(2)
    net = MLP([64, 96, 10], samples=6).to(DEV)
    seeded.pin_streams(net, 1010)
    net.mc_batched = batched
    x = torch.randn(130, 64, device=DEV)
    t = torch.randint(0, 10, (130,), device=DEV)
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)
    bnn.set_compute(mode)
    try:
        with torch.no_grad():
            bnn.manual_seed(8)
            u = net.predictive_score(x, t, 6, 2, inputs="logits", advance=cell)
            assert int(cell.item()) == 1
            bnn.manual_seed(8)
            ys = net.forward_stacked(x, 6, 2)
            want = ops.mc_score(ys, t, "logits")
            bnn.manual_seed(8)
            net.predictive_score(x, t, 6, 2, inputs="logits", advance=cell)
            assert int(cell.item()) == 2
    finally:
        bnn.set_compute("f32")
    for a, b in zip(u, want):
        assert torch.equal(a, b)
    ref = ref_rows(N(ys), t.cpu().numpy(), "logits")
    R = 130
    assert np.abs(N(u.mean) - ref["mean"]).max() <= 1e-6
    assert np.abs(N(u.entropy) - ref["entropy"]).max() <= 1e-5 * math.log(10)
    for name in ("nll", "expected_nll", "brier"):
        assert (np.abs(N(getattr(u, name)).reshape(R) - ref[name]) <= 1e-5 * np.maximum(1.0, np.abs(ref[name]))).all(), name


@gpu
def test_leading_row_dims_and_non_contiguous_input():
    gen = torch.Generator().manual_seed(5)
    y = _logits(6, 3 * 5, 10, gen).view(6, 3, 5, 10)
    t = torch.randint(0, 10, (3, 5), generator=gen)
    yt, tt = y.to(DEV).transpose(1, 2), t.to(DEV).t()                 # (6, 5, 3, 10) and (5, 3), not contiguous
    u = ops.mc_score(yt, tt, "logits")
    assert u.mean.shape == (5, 3, 10) and u.nll.shape == u.prediction.shape == (5, 3)
    ref = ref_rows(yt.cpu().contiguous().numpy().reshape(6, 15, 10), tt.cpu().contiguous().numpy().reshape(15), "logits")
    for name in ("nll", "expected_nll", "brier"):
        assert (np.abs(N(getattr(u, name)).reshape(15) - ref[name]) <= 1e-5 * np.maximum(1.0, np.abs(ref[name]))).all()
    with pytest.raises(_lib.BnnHipError):
        ops.mc_score(yt, tt.reshape(15), "logits")                    # the labels' shape is the rows' shape
    with pytest.raises(_lib.BnnHipError):
        ops.mc_score(yt, tt.int(), "logits")
    with pytest.raises(_lib.BnnHipError):
        ops.mc_score(yt, tt, "logits", state=ops.ScoreState("cpu"))


@gpu
def test_captured_graph_replays_accumulate_and_advance():
    y, t = make_case(8, 130, 10, "logits", 21)
    y, t = y.to(DEV), t.to(DEV)
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)
    eager = ops.ScoreState(DEV)
    for _ in range(3):
        ops.mc_score(y, t, "logits", state=eager, advance=cell)
    assert int(cell.item()) == 3
    st = ops.ScoreState(DEV)
    ops.mc_score(y, t, "logits", state=st, advance=cell)             # warm up outside the capture (sizes the workspace)
    st.reset()
    cell.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # captured on a side stream: one linear chain of two launches
        ops.mc_score(y, t, "logits", state=st, advance=cell)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(st.state, eager.state) and float(st.state[0]) == 390
    assert int(cell.item()) == 3
