"""The three kernels that close a training step, held to float64: k_adam (optim.Adam), k_xent_rows / k_xent_final
(ops.cross_entropy) and k_kl_backward (the KL gradient), csrc/bnn_train.hip and csrc/bnn_kl.hip.

CPU: NumPy float64 restatements of the three operations, the bounds as functions, NumPy fp32 evaluations of the kernels' formulas
held to those bounds, float64 mutants that the bounds must reject, and optim.py's documented deviation from torch as an assertion.
GPU: every kernel against the float64 restatements under the same bounds, plus the structure (launch splits, unaligned storage,
param groups, captured replays, guard elements) bit for bit.

u = 2^-24 throughout (one fp32 rounding is at most u relative).

Adam, one step.  The reference takes lr, b1, b2, eps, wd through np.float32 first -- the C entry's arguments are floats -- and
is float64 from there on.  With  G = |g| + wd |p|,  M = b1 |m| + (1 - b1) G,  V = b2 v + (1 - b2) G^2  (the same sums as m', v'
with every term taken positive; M = |m'| and V = v' whenever the terms share a sign) and  D = step_size M / denom:
  m:  |m' - ref| <= 4 u M      roundings: g + wd p, 1 - b1, its product with g, the fma
  v:  |v' - ref| <= 6 u V      2 x the rounding of g + wd p, 1 - b2, two products, the fma
  p:  |p' - ref| <= 0.5 ulp32(ref) + D u (13 + 3 V / v' + 4 A(t)),   A(t) = b1^t / (1 - b1^t) + 0.5 b2^t / (1 - b2^t)
      13 = m' (4) + step_size (1 - b1^t and the division: 2) + m' / denom and the product with step_size (2) + the
      denominator without v' (the subtraction 1 - b2^t halved by the square root, sqrtf, the reciprocal: 2.5; the product, the
      addition of eps: 2) = 12.5, rounded up;  3 V / v' = v' (6, halved by the square root);  so c0 = 16 where nothing cancels,
      which is the issue's count; 4 A(t): powf within 2 ulp = 4 u relative on b^t, amplified by b^t / (1 - b^t), halved under the
      square root for b2.  The last subtraction rounds once: 0.5 ulp.
  D replaces |dp| of a naive count because an fp32 evaluation -- any, the NumPy one below included -- has an error relative to the
  TERMS of b1 m + (1 - b1)(g + wd p), not to their sum: with random signs some of 3000 elements cancel to 1e-4 of their terms.
  Where the terms share a sign D = |dp|.
  Measured on the CPU grid (NumPy fp32 of the kernel's formula, fma as one rounding): max ratio to the bound p 0.999 (0.23 beyond the last half ulp),
  m 0.61, v 0.62.  On the MI355X: p 0.999 (0.19 beyond the last half ulp), m 0.61, v 0.62.
  Trajectory (50 steps, fresh gradients): the running sum over the steps of the one-step p bounds, each taken on the float64
  trajectory.  That sum counts every step's own roundings once, each at its worst and all in one direction.  It does not count
  the error already carried in m and v re-entering later steps (a geometric tail: at most 1 / (1 - b1) = 10 times the m share
  of a step's bound, and the v share for as long as the run lasts); those are independent roundings of either sign, which add
  like sqrt(steps) while the running sum adds like steps.  The NumPy fp32 evaluation of the same run peaks at 0.60 of the
  running sum at step 5 (a few half-ulp roundings of p in a row) and is at 0.25 by step 50.
  Measured on the MI355X: at most 0.60 (at step 5) of the running sum.

Documented deviation (optim.py).  float64 Adam with fp32-rounded hyper-parameters against float64 Adam with the exact ones, on
the grid: see test_rounded_hyperparameters_deviation for the figures and what is asserted.

Cross-entropy, per row, for  loss = ln(se) - (x[y] - mx),  se = sum_c e_c,  e_c = exp(a_c),  a_c = x_c - mx,  p_c = e_c / se:
  |loss - ref| <= u (|ref| + |x[y] - mx| + 4 |ln se| + sum_c p_c (3 |a_c| + 2) + n_add)
      |ref|: the last subtraction; |x[y] - mx|: that subtraction; 4 |ln se|: log2 within 1 ulp = 2 u, times ln 2 (a rounded
      constant and a product); p_c (3 |a_c| + 2): a_c is rounded (u |a_c| on the exponent), exp is exp2(a_c log2 e) -- a
      rounded constant and a product, 2 u |a_c| -- within 1 ulp = 2 u;  n_add = sum_c min(1, e_c / (u se)) - 1: each of the
      C - 1 additions of the left-to-right sum errs by at most u se and by at most its addend.
  A correct, confident row has x[y] = mx, ln se ~ loss and n_add ~ 1: its bound is ~ 2 u = 1.2e-7 however large the logits.
  Observed maxima over the CPU cases (scales 4, 30, 100 at C = 10 and scale 100 at C = 1000, random and argmax targets):
  NumPy fp32 2.8e-5 (1.9e-7 on the argmax cases), torch fp32 on the CPU 2.8e-5 (1.8e-7 on the argmax cases); per case the largest bound is at most 8 x the larger observed
  maximum.  The ordering (mx + ln se) - x[y] that the kernel had is 18 to 70 x this bound on the argmax cases (NumPy fp32).
  MI355X, R = 1 calls, argmax targets: before the reordering 18.5, 27.4 and 69.7 x the bound (scale 30; 100; 100 at C = 1000 --
  the kernel of the parent commit under this test: 5 of the 8 regimes failed, the NumPy figures to the digit); after: at most 0.45 (0.74 with random targets) of the bound.
  Mean over R rows: the mean of the row bounds + 2 u |ref| (inv_R is a rounded float; the double mean is rounded to float once).
  Gradient, per element: |g - ref| <= (u / R) (p_c (3 |a_c| + 2 + E + 3) + |R ref| + [c = y]),  E = sum_k p_k (3 |a_k| + 2) +
  n_add the relative error of se; 3 = inv_R, inv_R / se, the product; |R ref|: the subtraction of the one-hot; [c = y]: the
  one-hot term is inv_R itself, a rounded float (exact only for R a power of two).  The first count had left that last rounding
  out -- it was inside the 3, which p_c multiplies -- and the kernel's target elements reached 1.13 x that count at R = 3
  (0.81 at C = 10, 1.13 at C = 64) on the MI355X.  With it: at most 0.99 of the bound (a target element at R = 255), 0.57 elsewhere.

KL gradient, per element, scale = upstream / (n T n_batches), A = sigma / ps^2, B = 1 / sigma, ds = dsoftplus(rho):
  |g_mu - ref|  <= 8 u |ref|          scale (a rounded float, times upstream: 2), 1 / (ps ps) (2), mu - prior_mu (1), two
                                      products (2) = 7
  |g_rho - ref| <= c(rho) u scale (A + B) ds,   c(rho) = 28 + 2 |rho| (w + w2)
      sigma_accurate: exp2(rho log2 e) errs by 2 u |rho| + 2 u, passed on with weight w = e / ((1 + e) log1p(e)) <= 1; log2
      (2 u) times ln 2 (1.5 u), the reciprocal (2 u), two products (2 u), the u - 1 trick itself (2 u), + 1e-10 (u): 12.5 u;
      none of it for rho > 20.  A and B each carry sigma's error; A the two roundings of 1 / ps^2 and a product, B a division: 3;
      the subtraction 1 relative to at most A + B; scale 2; two products 2; dsoftplus: 1 + E (1), the fast division (3) and
      E = exp(-rho) to 2 u |rho| + 2 u with weight w2 = E / (1 + E): 4 + 2 w2.  12.5 + 3 + 1 + 2 + 2 + 6 = 26.5 -> 28.
  MI355X: g_mu 0.39, g_rho 0.23 of the bound."""
import ctypes
import math

import numpy as np
import pytest
import torch

import posterior_range
from bayesianneuralnetworks_amd import _lib, ops, optim
from klref import softplus64, dsoftplus64, kl_grad64              # noqa: F401  (tests/golden, shared with test_train_step.py)

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
TINY = 2.0 ** -126               # below the smallest normal fp32 a value may lose bits or be flushed: an absolute floor

def N(t):
    return t.detach().double().cpu().numpy()


# =================================================================================================== float64 restatements
ADAM_HP = [(1e-3, .9, .999, 1e-8, 0.0), (3e-3, .9, .99, 1e-7, 1e-2), (1e-2, .5, .9, 1e-3, .1), (1e-3, 0.0, .999, 1e-8, 0.0),
           (1e-3, .9, .9999, 1e-8, 0.0)]
ADAM_T = [1, 2, 3, 10, 100, 1000, 5000, 100000, 2 ** 24 - 1]
ADAM_GSCALE = [1.0, 1e-6]
ADAM_N = 3001
ADAM_CASES = [(hp, t, s) for hp in ADAM_HP for t in ADAM_T for s in ADAM_GSCALE]
KL_CORNERS = [-30.0, -1e-3, 0.0, 19.5, 20.0, 20.5]
KL_CORNERS += [v for v in posterior_range.FIXED if v not in KL_CORNERS]      # every fixed value of the posterior-range grid
KL_PRIORS = [(0.0, 0.1), (0.3, 1.0)]
MUTANTS = ["no_bc2", "no_bc1", "t_plus_1", "eps_before_bc2", "eps_in_sqrt", "adamw", "b2_for_m"]


def hp64(hp, exact=False):
    """The hyper-parameters as float64: through np.float32 (the C entry's interface), or exactly as written."""
    return tuple(float(h) if exact else float(np.float32(h)) for h in hp)


def adam64(p, g, m, v, t, hp, exact=False, mutant=None):
    """One Adam step (torch.optim.Adam: L2 weight decay, no amsgrad) in float64 -> p', m', v'.  mutant: a wrong formula."""
    lr, b1, b2, eps, wd = hp64(hp, exact)
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    t = float(t + 1 if mutant == "t_plus_1" else t)
    gg = g if mutant == "adamw" else g + wd * p
    bm = b2 if mutant == "b2_for_m" else b1
    m1 = bm * m + (1.0 - bm) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    bc1 = 1.0 if mutant == "no_bc1" else 1.0 - b1 ** t
    bc2 = 1.0 if mutant == "no_bc2" else 1.0 - b2 ** t
    if mutant == "eps_before_bc2":
        denom = (np.sqrt(v1) + eps) / math.sqrt(bc2)
    elif mutant == "eps_in_sqrt":
        denom = np.sqrt(v1 / bc2 + eps)
    else:
        denom = np.sqrt(v1) / math.sqrt(bc2) + eps
    p0 = p * (1.0 - lr * wd) if mutant == "adamw" else p
    return p0 - (lr / bc1) * (m1 / denom), m1, v1


def fma32(a, b, c):
    """fp32 fused multiply-add (one rounding; the double product of two floats is exact)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def adam32(p, g, m, v, t, hp):
    """k_adam's formula, operation by operation, in NumPy fp32."""
    f = np.float32
    lr, b1, b2, eps, wd = (f(h) for h in hp)
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    one = f(1)
    bc1 = one - f(float(b1) ** float(t))
    bc2 = one - f(float(b2) ** float(t))
    step_size = lr / bc1
    inv_sqrt_bc2 = one / np.sqrt(bc2)
    gg = fma32(wd, p, g)
    m1 = fma32(b1, m, (one - b1) * gg)
    v1 = fma32(b2, v, (one - b2) * gg * gg)
    denom = np.sqrt(v1) * inv_sqrt_bc2 + eps
    return p - step_size * (m1 / denom), m1, v1


def adam_A(t, hp):
    _, b1, b2, _, _ = hp64(hp)
    a1 = 0.0 if b1 == 0 else b1 ** t / (1.0 - b1 ** t)
    return a1 + 0.5 * b2 ** t / (1.0 - b2 ** t)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def adam_bounds(p, g, m, v, t, hp):
    """(bound_p, bound_m, bound_v) of one step from (p, g, m, v, t): the docstring's formulas around the float64 step."""
    lr, b1, b2, eps, wd = hp64(hp)
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    pr, _, v1 = adam64(p, g, m, v, t, hp)
    G = np.abs(g) + wd * np.abs(p)
    M = b1 * np.abs(m) + (1.0 - b1) * G
    V = b2 * v + (1.0 - b2) * G * G
    denom = np.sqrt(v1) / math.sqrt(1.0 - b2 ** t) + eps
    D = lr / (1.0 - b1 ** t) * M / denom
    rv = np.where(v1 > 0, V / np.where(v1 > 0, v1, 1.0), 1.0)
    return 0.5 * ulp32(pr) + D * U * (13.0 + 3.0 * rv + 4.0 * adam_A(t, hp)), 4.0 * U * M, 6.0 * U * V


def adam_case_data(case):
    """p, g, m, v of one grid case: p ~ N(0, 1); g, m at the gradient scale with independent signs; v at its square."""
    hp, t, s = case
    rng = np.random.default_rng(1000 * ADAM_HP.index(hp) + 10 * ADAM_T.index(t) + ADAM_GSCALE.index(s))
    f = np.float32
    p = rng.standard_normal(ADAM_N).astype(f)
    g = (s * rng.standard_normal(ADAM_N)).astype(f)
    m = (0.5 * s * rng.standard_normal(ADAM_N)).astype(f)
    v = (s * s * (0.05 + rng.random(ADAM_N))).astype(f)
    return p, g, m, v


def adam_violations(got, case, data=None):
    """got = (p', m', v') after one step of `case` -> (fraction of elements outside any of the three bounds, the max ratios
    to the bounds of p, m, v, and of p's error beyond the last half ulp to the D term alone -- where the update is below an ulp
    of p the first ratio only shows that rounding)."""
    hp, t, _ = case
    p, g, m, v = data if data is not None else adam_case_data(case)
    ref = adam64(p, g, m, v, t, hp)
    bnd = adam_bounds(p, g, m, v, t, hp)
    out = np.zeros(np.asarray(p).shape, bool)
    ratios = []
    for a, r, b in zip(got, ref, bnd):
        e = np.abs(np.asarray(a, np.float64) - r)
        out |= ~(e <= b)
        ratios.append(float((e / np.where(b > 0, b, 1.0)).max()))
    half = 0.5 * ulp32(ref[0])
    ratios.append(float((np.maximum(np.abs(np.asarray(got[0], np.float64) - ref[0]) - half, 0.0) / (bnd[0] - half)).max()))
    return float(out.mean()), ratios


def assert_adam(got, case, data=None, what=""):
    frac, ratios = adam_violations(got, case, data)
    assert frac == 0.0, (what, case, "fraction outside %.4f" % frac, "max ratio p, m, v", ratios)
    return ratios


def logsumexp64(x):
    mx = x.max(axis=1, keepdims=True)
    return (mx + np.log(np.exp(x - mx).sum(axis=1, keepdims=True)))[:, 0]


def xent64(x, y):
    """float64: per-row losses, their mean, d mean / d logits."""
    x = np.asarray(x, np.float64)
    R = x.shape[0]
    lse = logsumexp64(x)
    rows = lse - x[np.arange(R), y]
    g = np.exp(x - lse[:, None])
    g[np.arange(R), y] -= 1.0
    return rows, rows.mean(), g / R


def _xent_terms(x, y):
    x = np.asarray(x, np.float64)
    R = x.shape[0]
    mx = x.max(axis=1, keepdims=True)
    a = x - mx
    e = np.exp(a)                                         # exp(-inf) = 0: a masked class contributes nothing
    se = e.sum(axis=1, keepdims=True)
    pc = e / se
    absa = np.where(np.isfinite(a), np.abs(a), 0.0)
    E = (pc * (3.0 * absa + 2.0)).sum(axis=1) + np.minimum(1.0, e / (U * se)).sum(axis=1) - 1.0
    return R, a, se[:, 0], pc, absa, E


def xent_row_bound(x, y):
    R, a, se, _, _, E = _xent_terms(x, y)
    rows = xent64(x, y)[0]
    return U * (np.abs(rows) + np.abs(a[np.arange(R), y]) + 4.0 * np.abs(np.log(se)) + E)


def xent_mean_bound(x, y):
    return float(xent_row_bound(x, y).mean() + 2.0 * U * abs(xent64(x, y)[1]))


def xent_grad_bound(x, y):
    R, _, _, pc, absa, E = _xent_terms(x, y)
    g = xent64(x, y)[2]
    onehot = np.zeros_like(pc)
    onehot[np.arange(R), y] = 1.0
    return (U / R) * (pc * (3.0 * absa + 2.0 + E[:, None] + 3.0) + np.abs(g * R) + onehot) + TINY


def xent32(x, y, ordering="reordered"):
    """The kernel's row loss in NumPy fp32, left-to-right sum.  reordered: ln(se) - (x[y] - mx); present: (mx + ln(se)) - x[y],
    what k_xent_rows computed before this file existed."""
    x = np.asarray(x, np.float32)
    R, C = x.shape
    mx = x.max(axis=1)
    se = np.zeros(R, np.float32)
    for c in range(C):
        se = se + np.exp(x[:, c] - mx)
    xy = x[np.arange(R), y]
    if ordering == "present":
        return ((mx + np.log(se)) - xy).astype(np.float64)
    return (np.log(se) - (xy - mx)).astype(np.float64)


XENT_REGIMES = [(scale, C, tgt) for scale, C in ((4, 10), (30, 10), (100, 10), (100, 1000)) for tgt in ("random", "argmax")]


def xent_regime(regime, rows=64):
    scale, C, tgt = regime
    gen = torch.Generator().manual_seed(100 * scale + C + (tgt == "argmax"))
    x = (torch.randn(rows, C, generator=gen) * scale)
    y = x.argmax(dim=1) if tgt == "argmax" else torch.randint(0, C, (rows,), generator=gen)
    return x, y


def assert_xent_rows(got, x, y, what=""):
    """Per-row losses against float64 under the per-row bound -> the max ratio to the bound."""
    ref, bnd = xent64(N(x), y.numpy())[0], xent_row_bound(N(x), y.numpy())
    e = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float((e / bnd).max()) if (bnd > 0).all() else float(e.max() > 0) * np.inf
    print(what, "rows: max err %.3e, max bound %.3e, max ratio %.3f" % (e.max(), bnd.max(), ratio))
    assert (e <= bnd).all(), (what, "max err %.3e" % e.max(), "ratio %.2f" % ratio, "%d of %d rows out" % ((e > bnd).sum(), e.size))
    return ratio


# =================================================================================================== CPU section
def test_adam_fp32_evaluation_is_inside_the_bound():
    worst = [0.0] * 4
    for case in ADAM_CASES:
        p, g, m, v = adam_case_data(case)
        r = assert_adam(adam32(p, g, m, v, case[1], case[0]), case, what="numpy fp32")
        worst = [max(a, b) for a, b in zip(worst, r)]
    print("adam numpy fp32: max ratio to the bound p %.3f m %.3f v %.3f, p beyond its last rounding %.3f" % tuple(worst))


def test_adam_bound_is_the_plain_count_where_nothing_cancels():
    """Where b1 m, (1 - b1) g and wd p share a sign, D = |dp| and the p bound is 0.5 ulp + |dp| u (16 + 4 A(t))."""
    for case in ADAM_CASES[::7]:
        hp, t, _ = case
        p, g, m, v = (np.abs(a) for a in adam_case_data(case))
        pr, _, _ = adam64(p, g, m, v, t, hp)
        want = 0.5 * ulp32(pr) + np.abs(pr - p) * U * (16.0 + 4.0 * adam_A(t, hp))
        assert np.allclose(adam_bounds(p, g, m, v, t, hp)[0], want, rtol=1e-12, atol=0)


def test_adam_bound_rejects_every_mutant():
    """Each wrong formula, in float64 (no rounding of its own), is outside the bound on more than half the elements of at least
    one grid case; the same helper passes the true formula in fp32 (the test above)."""
    for mutant in MUTANTS:
        best, where = 0.0, None
        for case in ADAM_CASES:
            p, g, m, v = adam_case_data(case)
            frac, _ = adam_violations(adam64(p, g, m, v, case[1], case[0], mutant=mutant), case)
            if frac > best:
                best, where = frac, case
        print("mutant %-15s rejected on %.1f %% of elements at %s" % (mutant, 100 * best, where))
        assert best > 0.5, (mutant, best, where)
        with pytest.raises(AssertionError):
            p, g, m, v = adam_case_data(where)
            assert_adam(adam64(p, g, m, v, where[1], where[0], mutant=mutant), where)


def adam_deviation(hp, t):
    """max over the case data (both gradient scales) of |p'(rounded hyper-parameters) - p'(exact)| / D, both in float64."""
    worst = 0.0
    for s in ADAM_GSCALE:
        p, g, m, v = adam_case_data((hp, t, s)) if (hp, t, s) in ADAM_CASES else adam_case_data((ADAM_HP[0], t, s))
        lr, b1, b2, eps, wd = hp64(hp)
        pr, _, v1 = adam64(p, g, m, v, t, hp)
        pe = adam64(p, g, m, v, t, hp, exact=True)[0]
        M = b1 * np.abs(m) + (1.0 - b1) * (np.abs(g) + wd * np.abs(p))
        D = lr / (1.0 - b1 ** t) * M / (np.sqrt(v1) / math.sqrt(1.0 - b2 ** t) + eps)
        worst = max(worst, float((np.abs(pr - pe) / D).max()))
    return worst


def adam_deviation_bound(hp):
    """Each hyper-parameter moves by at most u relative when rounded to fp32.  1 - b moves by u b / (1 - b): that is the
    relative change of (1 - b1) g in m' and, at most, of 1 - b1^t (t b^t / (1 - b^t) <= b / (1 - b)); the same for b2, halved
    twice by the square roots; lr and eps one u each; wd one u on g + wd p, which enters m' once and v' twice, halved."""
    _, b1, b2, _, wd = hp
    return U * (2.0 + 2.0 * (wd > 0) + 2.0 * b1 / (1.0 - b1) + b2 / (1.0 - b2))


def test_rounded_hyperparameters_deviation():
    """optim.py's docstring, as assertions.  float64 with fp32-rounded hyper-parameters against float64 with the exact ones,
    relative to D, from the planted states of the grid.  Measured: (0.9, 0.999) 6.7e-6 at t = 1..3, falling to 8e-7;
    (0.9, 0.99) 7.4e-7 at t = 1, 7.2e-7 late; (0.5, 0.9) 1.4e-7; (0.9, 0.9999) 8.3e-5 up to t = 100 (largest at t = 10),
    6.4e-5 at t = 5000.
      * everywhere inside the counted bound u (2 + 2 b1 / (1 - b1) + b2 / (1 - b2)) -- 6.1e-5 for the default betas, the
        docstring's figure;
      * for the betas the project uses, (0.9, 0.999) (the default; examples, bench) and (0.9, 0.99) (the suite), below 6e-5 and
        largest at t <= 3;
      * NOT for b2 = 0.9999: above 6e-5 there, and not largest at the first steps -- the docstring says so now."""
    for hp in ADAM_HP:
        dev = {t: adam_deviation(hp, t) for t in ADAM_T}
        print(hp, " ".join("%d:%.2e" % kv for kv in dev.items()), "bound %.2e" % adam_deviation_bound(hp))
        assert max(dev.values()) <= adam_deviation_bound(hp), (hp, dev)
    for hp in (ADAM_HP[0], ADAM_HP[1]):
        dev = {t: adam_deviation(hp, t) for t in ADAM_T}
        assert max(dev.values()) <= 6e-5, (hp, dev)
        assert max(dev[t] for t in (1, 2, 3)) == max(dev.values()), (hp, dev)
    dev = {t: adam_deviation(ADAM_HP[4], t) for t in ADAM_T}
    assert max(dev.values()) > 6e-5 and max(dev[t] for t in (1, 2, 3)) < max(dev.values()), dev


def test_xent_bound_holds_for_fp32_and_is_tight():
    """The reordered expression in NumPy fp32 and torch's fp32 cross_entropy on the CPU stay inside the per-row bound on every
    regime, and the bound is at most 8 x the larger of their observed maxima, regime by regime."""
    worst_np = worst_t = 0.0
    for regime in XENT_REGIMES:
        x, y = xent_regime(regime)
        ref, bnd = xent64(N(x), y.numpy())[0], xent_row_bound(N(x), y.numpy())
        got_np = xent32(x.numpy(), y.numpy())
        got_t = N(torch.nn.functional.cross_entropy(x, y, reduction="none"))
        assert_xent_rows(got_np, x, y, "numpy fp32 %s" % (regime,))
        assert_xent_rows(got_t, x, y, "torch fp32 %s" % (regime,))
        e_np, e_t = np.abs(got_np - ref).max(), np.abs(got_t - ref).max()
        worst_np, worst_t = max(worst_np, e_np), max(worst_t, e_t)
        print(regime, "max err numpy %.3e torch %.3e, max bound %.3e = %.2f x" % (e_np, e_t, bnd.max(), bnd.max() / max(e_np, e_t)))
        assert bnd.max() <= 8.0 * max(e_np, e_t), (regime, bnd.max(), e_np, e_t)
    print("observed maxima over the regimes: numpy fp32 %.3e, torch fp32 %.3e" % (worst_np, worst_t))


def test_xent_bound_rejects_the_present_ordering():
    """(mx + ln se) - x[y] rounds at the magnitude of the logits: outside the bound on the confident, correct rows."""
    for regime in XENT_REGIMES:
        scale, C, tgt = regime
        if tgt != "argmax" or scale < 30:
            continue
        x, y = xent_regime(regime)
        got = xent32(x.numpy(), y.numpy(), "present")
        bnd = xent_row_bound(N(x), y.numpy())
        e = np.abs(got - xent64(N(x), y.numpy())[0])
        print(regime, "present ordering: max err %.3e = %.1f x the bound, %d of %d rows out" % (e.max(), (e / bnd).max(), (e > bnd).sum(), e.size))
        assert (e / bnd).max() > 8.0                      # (rows whose se rounds to 1 are exact in either ordering)
        with pytest.raises(AssertionError):
            assert_xent_rows(got, x, y)


def test_xent_mean_and_gradient_bounds_hold_for_torch_fp32():
    """The R-scaled loss bound and the gradient bound against torch's fp32 evaluation on the CPU (a reference inside its own
    bound), and a wrong gradient -- softmax / R without the one-hot, or divided by R + 1 -- outside it."""
    for R, C, scale in ((257, 10, 4.0), (5, 1000, 30.0), (64, 3, 100.0)):
        gen = torch.Generator().manual_seed(R)
        x = (torch.randn(R, C, generator=gen) * scale).requires_grad_()
        y = torch.randint(0, C, (R,), generator=gen)
        loss = torch.nn.functional.cross_entropy(x, y)
        loss.backward()
        _, ref, gref = xent64(N(x), y.numpy())
        assert abs(loss.item() - ref) <= xent_mean_bound(N(x), y.numpy())
        gb = xent_grad_bound(N(x), y.numpy())
        assert (np.abs(N(x.grad) - gref) <= gb).all()
        assert not (np.abs(gref * R / (R + 1) - gref) <= gb).all()
        wrong = gref.copy()
        wrong[np.arange(R), y.numpy()] += 1.0 / R
        assert not (np.abs(wrong - gref) <= gb).all()
        assert not (np.abs(gref * (1.0 + 4.0 * U) - gref) <= gb).all()     # the target elements hold the bound to a few u


def test_kl_gradient_reference_is_the_derivative_of_the_kl():
    """The closed form against float64 autograd of torch's own kl_divergence, corners included."""
    gen = torch.Generator().manual_seed(3)
    rho = torch.cat([torch.tensor(KL_CORNERS, dtype=torch.float64), torch.randn(50, generator=gen, dtype=torch.float64) * 3 - 2])
    mu = torch.randn(rho.numel(), generator=gen, dtype=torch.float64)
    for prior in KL_PRIORS:
        m, r = mu.clone().requires_grad_(), rho.clone().requires_grad_()
        sg = 1e-10 + torch.nn.functional.softplus(r)
        pm, ps = float(np.float32(prior[0])), float(np.float32(prior[1]))
        kl = torch.distributions.kl_divergence(torch.distributions.Normal(m, sg), torch.distributions.Normal(pm, ps))
        (kl.mean() / 5 / 3 * 1.5).backward()
        g_mu, g_rho, _, _ = kl_grad64(mu.numpy(), rho.numpy(), prior, 5, 3, 1.5)
        assert np.allclose(N(m.grad), g_mu, rtol=1e-12, atol=1e-300)
        assert np.allclose(N(r.grad), g_rho, rtol=1e-9, atol=1e-18)



# =================================================================================================== GPU: Adam
def T32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)


def make_adam(params, hp):
    return optim.Adam(params, lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3], weight_decay=hp[4])


def planted_step(case, data):
    """One optim.Adam step from the planted (p, m, v, t - 1) -> (p', m', v', step) as float64 NumPy / float."""
    hp, t, _ = case
    p, g, m, v = data
    P = T32(p).requires_grad_()
    opt = make_adam([P], hp)
    P.grad = torch.zeros_like(P)
    opt.step()                                            # a real step creates the state and the counter ...
    st, group = opt.state[P], opt.param_groups[0]
    with torch.no_grad():                                 # ... which are then overwritten
        P.copy_(T32(p))
        st["exp_avg"].copy_(T32(m))
        st["exp_avg_sq"].copy_(T32(v))
        group["step"].fill_(float(t - 1))
    P.grad = T32(g)
    opt.step()
    return (N(P), N(st["exp_avg"]), N(st["exp_avg_sq"])), float(group["step"])


@gpu
@pytest.mark.parametrize("hp", ADAM_HP, ids=lambda hp: "lr%g-b%g-%g-eps%g-wd%g" % hp)
def test_adam_single_steps_from_a_planted_state(hp):
    worst = [0.0] * 4
    for t in ADAM_T:
        for s in ADAM_GSCALE:
            case = (hp, t, s)
            data = adam_case_data(case)
            got, step = planted_step(case, data)
            frac, r = adam_violations(got, case, data)
            print(case, "ratio to the bound p %.3f m %.3f v %.3f, outside %.4f, step %r" % (r[0], r[1], r[2], frac, step))
            assert step == float(t), (case, step)
            assert_adam(got, case, data, what="k_adam")
            worst = [max(a, b) for a, b in zip(worst, r)]
    print("k_adam", hp, "max ratio to the bound p %.3f m %.3f v %.3f, p beyond its last rounding %.3f" % tuple(worst))


STRUCT_HP = (3e-3, .9, .99, 1e-7, 1e-2)
STRUCT_SIZES = [1, 2, 3, 4, 5, 7, 2047, 2048, 2049, 4095, 4096, 4097]


def struct_sizes(k):
    rng = np.random.default_rng(k)
    sizes = [STRUCT_SIZES[i % len(STRUCT_SIZES)] for i in range(k)]
    rng.shuffle(sizes)
    return sizes


def run_layout(p0, grads, make):
    """Three steps over storage laid out by make(values) -> (list of parameter tensors, setter of gradients); -> the
    concatenated p, m, v."""
    params, set_grads = make(p0)
    opt = make_adam(params, STRUCT_HP)
    for g in grads:
        set_grads(params, g)
        opt.step()
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])          # noqa: E731
    return (cat(params), cat([opt.state[p]["exp_avg"] for p in params]), cat([opt.state[p]["exp_avg_sq"] for p in params]),
            float(opt.param_groups[0]["step"]))


def layout_cut(sizes):
    def make(p0):
        return [c.clone().requires_grad_() for c in torch.split(p0, sizes)], set_grads

    def set_grads(params, g):
        for p, c in zip(params, torch.split(g, sizes)):
            p.grad = c.clone()
    return make


def layout_view(p_view, g_view):
    """p and / or its gradient as base[1:] of a 16-byte aligned allocation: 4 bytes off, the scalar path of k_adam."""
    def off(t):
        base = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
        base[1:].copy_(t)
        v = base[1:]
        assert base.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    def make(p0):
        return [(off(p0) if p_view else p0.clone()).detach().requires_grad_()], set_grads

    def set_grads(params, g):
        params[0].grad = off(g) if g_view else g.clone()
    return make


@pytest.fixture(scope="module")
def struct_pool():
    """Values for the largest layout (100 tensors) and what ONE tensor of them becomes after three steps; every element's
    arithmetic is independent of its neighbours, so a shorter single tensor is a prefix of this one."""
    n = sum(struct_sizes(100)) + 8192
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen).to(DEV)
    grads = [torch.randn(n, generator=gen).to(DEV) for _ in range(3)]
    return p0, grads, run_layout(p0, grads, layout_cut([n]))


@gpu
@pytest.mark.parametrize("k", [49, 96, 97, 100])
def test_adam_split_into_tensors_is_bitwise_one_tensor(struct_pool, k):
    """49 ... 100 tensors: the second and third launch of bnn_adam_step (first_block restarts at 0; every launch reads the
    same t because the counter is bumped afterwards)."""
    p0, grads, one = struct_pool
    sizes = struct_sizes(k)
    n = sum(sizes)
    got = run_layout(p0[:n], [g[:n] for g in grads], layout_cut(sizes))
    assert got[3] == 3.0
    for name, a, b in zip("pmv", got[:3], one[:3]):
        assert torch.equal(a, b[:n]), (k, name, int((a != b[:n]).sum()))
    assert not torch.equal(got[0], p0[:n])


@gpu
@pytest.mark.parametrize("p_view,g_view", [(True, False), (False, True), (True, True)])
def test_adam_unaligned_storage_is_bitwise_aligned_storage(struct_pool, p_view, g_view):
    p0, grads, one = struct_pool
    n = 4096 + 2048 + 5                                   # three workgroups, a ragged last quad
    got = run_layout(p0[:n], [g[:n] for g in grads], layout_view(p_view, g_view))
    for name, a, b in zip("pmv", got[:3], one[:3]):
        assert torch.equal(a, b[:n]), (p_view, g_view, name, int((a != b[:n]).sum()))


def adam_state(opt, p):
    st = opt.state[p]
    return N(p), N(st["exp_avg"]), N(st["exp_avg_sq"])


@gpu
def test_adam_param_groups_missing_gradients_and_the_advance_cell():
    gen = torch.Generator().manual_seed(12)
    hps = [(1e-3, .9, .999, 1e-8, 0.0), (1e-2, .5, .9, 1e-3, .1)]
    a, b, c = (torch.randn(n, generator=gen).to(DEV).requires_grad_() for n in (2049, 300, 17))
    opt = optim.Adam([dict(params=[a, c], lr=hps[0][0], betas=hps[0][1:3], eps=hps[0][3], weight_decay=hps[0][4]),
                      dict(params=[b], lr=hps[1][0], betas=hps[1][1:3], eps=hps[1][3], weight_decay=hps[1][4])])
    cell = torch.zeros(4, dtype=torch.int32, device=DEV)
    c0 = c.detach().clone()
    zero = lambda n: np.zeros(n, np.float32)              # noqa: E731
    # steps 1, 2: both groups; step 3: only the second group has a gradient; c never has one
    plan = [("a", "b"), ("a", "b"), ("b",)]
    named = {"a": (a, hps[0]), "b": (b, hps[1])}
    prev = {"a": (N(a), zero(2049), zero(2049)), "b": (N(b), zero(300), zero(300))}
    for k, who in enumerate(plan):
        gs = {}
        for name, (q, _) in named.items():
            q.grad = torch.randn(q.shape, generator=gen).to(DEV) if name in who else None
            gs[name] = None if q.grad is None else N(q.grad)
        opt.step(advance=cell)
        assert int(cell[0]) == k + 1, "one bump per step(), in the last group's launch only"
        for name, (q, hp) in named.items():
            if name in who:
                t = sum(1 for w in plan[:k + 1] if name in w)
                p, m, v = prev[name]
                assert_adam(adam_state(opt, q), (hp, t, 1.0), (p, gs[name], m, v), what="group step %d" % (k + 1))
                prev[name] = tuple(x.astype(np.float32) for x in adam_state(opt, q))
            else:
                for x, y in zip(adam_state(opt, q), prev[name]):
                    assert np.array_equal(x, y), "a parameter without a gradient is untouched"
    assert float(opt.param_groups[0]["step"]) == 2.0 and float(opt.param_groups[1]["step"]) == 3.0
    assert torch.equal(c, c0) and (c not in opt.state or len(opt.state[c]) == 0)
    for q in (a, b):
        q.grad = None
    before = [t.clone() for t in (a, b)]
    opt.step(advance=cell)                                # no gradient anywhere: the cell still advances, nothing else
    assert int(cell[0]) == 4 and torch.equal(a, before[0]) and torch.equal(b, before[1])
    assert float(opt.param_groups[0]["step"]) == 2.0 and float(opt.param_groups[1]["step"]) == 3.0
    assert cell[1:].abs().sum().item() == 0
    _lib.check_device(DEV)


@gpu
def test_adam_captured_step_replayed_is_bitwise_eager():
    gen = torch.Generator().manual_seed(13)
    sizes = (2049, 5, 4096)
    p0 = [torch.randn(n, generator=gen).to(DEV) for n in sizes]
    g = [torch.randn(n, generator=gen).to(DEV) for n in sizes]

    def fresh():
        ps = [p.clone().requires_grad_() for p in p0]
        for p, gg in zip(ps, g):
            p.grad = gg.clone()
        return ps, make_adam(ps, STRUCT_HP)

    eager, o1 = fresh()
    for _ in range(4):
        o1.step()
    replay, o2 = fresh()
    o2.step()                                             # creates state and counter outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o2.step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert float(o2.param_groups[0]["step"]) == 4.0 == float(o1.param_groups[0]["step"])
    for a, b in zip(eager, replay):
        assert torch.equal(a, b)
        assert torch.equal(o1.state[a]["exp_avg"], o2.state[b]["exp_avg"])
        assert torch.equal(o1.state[a]["exp_avg_sq"], o2.state[b]["exp_avg_sq"])
    _lib.check_device(DEV)


@gpu
def test_adam_trajectory_against_float64():
    """50 steps, 3 ragged tensors, fresh gradients: against the float64 restatement carried along in float64, inside the
    running sum of the one-step bounds (taken on the float64 trajectory)."""
    gen = torch.Generator().manual_seed(14)
    hp = STRUCT_HP
    sizes = (1, 2049, 777)
    ps = [torch.randn(n, generator=gen).to(DEV).requires_grad_() for n in sizes]
    opt = make_adam(ps, hp)
    ref = [(N(p), np.zeros(n), np.zeros(n)) for p, n in zip(ps, sizes)]
    run = [np.zeros(n) for n in sizes]
    worst = 0.0
    for t in range(1, 51):
        for i, p in enumerate(ps):
            p.grad = torch.randn(p.shape, generator=gen).to(DEV)
            g = N(p.grad)
            run[i] = run[i] + adam_bounds(ref[i][0], g, ref[i][1], ref[i][2], t, hp)[0]
            ref[i] = adam64(ref[i][0], g, ref[i][1], ref[i][2], t, hp)
        opt.step()
        if t in (1, 2, 5, 10, 25, 50):
            for i, p in enumerate(ps):
                e = np.abs(N(p) - ref[i][0])
                worst = max(worst, float((e / run[i]).max()))
                assert (e <= run[i]).all(), (t, i, float((e / run[i]).max()))
    print("adam trajectory: max ratio to the running sum %.3f" % worst)
    assert float(opt.param_groups[0]["step"]) == 50.0


# =================================================================================================== GPU: cross-entropy
def hip_xent(x, y, grad=True):
    """ops.cross_entropy on the device -> (loss as a Python float, gradient as float64 NumPy or None)."""
    xd = x.detach().to(DEV).requires_grad_(grad)
    loss = ops.cross_entropy(xd, y.to(DEV))
    if grad:
        loss.backward()
    return loss, (N(xd.grad) if grad else None)


XENT_EXTENTS = [(3, C) for C in (1, 2, 10, 63, 64, 65, 1000, 4096)] + [(R, 10) for R in (1, 255, 256, 257, 16385)] + \
    [(65537, 3), (70000, 3)]


@gpu
@pytest.mark.parametrize("R,C", XENT_EXTENTS)
def test_xent_extents_against_float64(R, C):
    """1, 2, 65 partials at C = 10; 257 and 274 at C = 3: the second trip of k_xent_final's loop and all four of its waves."""
    gen = torch.Generator().manual_seed(R * 7 + C)
    x = torch.randn(R, C, generator=gen) * 4
    y = torch.randint(0, C, (R,), generator=gen)
    loss, g = hip_xent(x, y)
    _, ref, gref = xent64(N(x), y.numpy())
    bl, bg = xent_mean_bound(N(x), y.numpy()), xent_grad_bound(N(x), y.numpy())
    e, eg = abs(loss.item() - ref), np.abs(g - gref)
    w = np.unravel_index(np.argmax(eg / bg), eg.shape)
    print("R %d C %d: loss %.9g ref %.9g err %.3e bound %.3e (%.3f); gradient max ratio to the bound %.3f at %s (target %d, ref %.3e)"
          % (R, C, loss.item(), ref, e, bl, e / bl, (eg / bg).max(), w, int(y[w[0]]), gref[w]))
    assert e <= bl, (R, C, e, bl)
    assert (eg <= bg).all(), (R, C, float((eg / bg).max()))


@gpu
@pytest.mark.parametrize("regime", XENT_REGIMES, ids=lambda r: "scale%d-C%d-%s" % r)
def test_xent_single_rows_are_held_to_the_row_bound(regime):
    """R = 1 calls (the mean cannot hide a row's error), 64 rows per regime; then the same rows four at a time."""
    x, y = xent_regime(regime)
    xd, yd = x.to(DEV), y.to(DEV)
    got = torch.stack([ops.cross_entropy(xd[r:r + 1], yd[r:r + 1]) for r in range(x.shape[0])])
    assert_xent_rows(N(got), x, y, "k_xent_rows %s R = 1" % (regime,))
    got4 = N(torch.stack([ops.cross_entropy(xd[r:r + 4], yd[r:r + 4]) for r in range(0, x.shape[0], 4)]))
    for i, r in enumerate(range(0, x.shape[0], 4)):
        xs, ys = N(x[r:r + 4]), y[r:r + 4].numpy()
        assert abs(got4[i] - xent64(xs, ys)[1]) <= xent_mean_bound(xs, ys), (regime, r)


@gpu
def test_xent_masked_classes():
    """-inf on classes that are not the target: a finite loss equal to the reference, a gradient of exactly 0.0 there."""
    gen = torch.Generator().manual_seed(15)
    R, C = 300, 10
    x = torch.randn(R, C, generator=gen) * 4
    y = torch.randint(0, C, (R,), generator=gen)
    mask = torch.rand(R, C, generator=gen) < 0.4
    mask[torch.arange(R), y] = False
    x[mask] = float("-inf")
    loss, g = hip_xent(x, y)
    _, ref, gref = xent64(N(x), y.numpy())
    assert math.isfinite(loss.item()) and abs(loss.item() - ref) <= xent_mean_bound(N(x), y.numpy())
    assert (g[mask.numpy()] == 0.0).all() and mask.sum() > 500
    assert (np.abs(g - gref) <= xent_grad_bound(N(x), y.numpy())).all()


@gpu
@pytest.mark.parametrize("R,C", [(1, 10), (257, 33), (16385, 3)])
def test_xent_without_gradient_has_the_same_bits(R, C):
    gen = torch.Generator().manual_seed(16)
    x = torch.randn(R, C, generator=gen) * 4
    y = torch.randint(0, C, (R,), generator=gen)
    a, _ = hip_xent(x, y, grad=True)
    b, _ = hip_xent(x, y, grad=False)
    assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32))


@gpu
@pytest.mark.parametrize("bad", [-1, 10, 13, -100, 2 ** 32 + 1])
def test_xent_target_out_of_range_is_nan_in_its_row_only(bad):
    """The defined behaviour: NaN loss, NaN gradient row, every other gradient row as in the all-valid run.  (Rows 16..47 of
    64: even a kernel that indexed with the bad target would stay inside the logits.)"""
    gen = torch.Generator().manual_seed(17)
    R, C = 64, 10
    x = torch.randn(R, C, generator=gen) * 4
    y = torch.randint(0, C, (R,), generator=gen)
    loss0, g0 = hip_xent(x, y)
    assert math.isfinite(loss0.item())
    for row in (16, 31, 47):
        yb = y.clone()
        yb[row] = bad
        loss, g = hip_xent(x, yb)
        assert math.isnan(loss.item()), (bad, row, loss.item())
        assert np.isnan(g[row]).all(), (bad, row, g[row])
        keep = np.arange(R) != row
        assert np.array_equal(g[keep], g0[keep]), (bad, row)
        assert math.isnan(hip_xent(x, yb, grad=False)[0].item())
    _lib.check_device(DEV)


# =================================================================================================== GPU: KL gradient
KL_RAGGED = [1, 3, 2047, 2048, 2049, 5000, 7, 64]
KL_NB, KL_UP = 3.0, 1.5


def softplus_inv64(s):
    return np.log(np.expm1(s))


def kl_tensors(sizes, offset_view=False):
    """mu, rho per tensor (fp32, on the device) and the prior of each.  rho ~ N(-3, 1.5^2) with the corners in front; every
    5000-element tensor has sigma within 1e-3 (relative) of its prior's: the factor sigma / ps^2 - 1 / sigma cancels there."""
    rng = np.random.default_rng(len(sizes))
    mus, rhos, priors = [], [], []
    for i, n in enumerate(sizes):
        prior = KL_PRIORS[i % 2]
        mu = rng.standard_normal(n).astype(np.float32)
        rho = (1.5 * rng.standard_normal(n) - 3.0).astype(np.float32)
        k = min(n, len(KL_CORNERS))
        rho[:k] = KL_CORNERS[:k]
        if n == 5000:
            rho[k:] = softplus_inv64(prior[1] * (1.0 + 1e-3 * rng.uniform(-1, 1, n - k))).astype(np.float32)
        ts = []
        for a in (mu, rho):
            if offset_view:
                base = torch.empty(n + 1, dtype=torch.float32, device=DEV)
                base[1:].copy_(T32(a))
                t = base[1:]
                assert t.data_ptr() % 16 == 4
            else:
                t = T32(a)
            ts.append(t.detach().requires_grad_())
        mus.append(ts[0])
        rhos.append(ts[1])
        priors.append(prior)
    return mus, rhos, priors


def check_kl_grads(mus, rhos, priors, g_mus, g_rhos, what):
    worst_m = worst_r = 0.0
    T = len(mus)
    for i in range(T):
        rm, rr, bm, br = kl_grad64(N(mus[i]), N(rhos[i]), priors[i], T, KL_NB, KL_UP)
        em, er = np.abs(N(g_mus[i]) - rm), np.abs(N(g_rhos[i]) - rr)
        worst_m = max(worst_m, float((em / np.maximum(bm, 1e-300)).max()))
        worst_r = max(worst_r, float((er / br).max()))
        assert (em <= bm).all(), (what, i, mus[i].numel(), "g_mu", float((em / np.maximum(bm, 1e-300)).max()))
        assert (er <= br).all(), (what, i, mus[i].numel(), "g_rho", float((er / br).max()), N(rhos[i])[np.argmax(er / br)])
    print(what, "max ratio to the bound: g_mu %.3f, g_rho %.3f" % (worst_m, worst_r))


class kl_unfused:
    def __enter__(self):
        self.was = ops.FUSE_KL_GRADIENT
        ops.FUSE_KL_GRADIENT = False

    def __exit__(self, *exc):
        ops.FUSE_KL_GRADIENT = self.was


@gpu
@pytest.mark.parametrize("layout", ["ragged72", "five", "offset_view"])
def test_kl_backward_against_float64(layout):
    """72 tensors: the second launch of bnn_kl_backward (64 per launch).  Through autograd with the upstream scalar 1.5."""
    sizes = {"ragged72": KL_RAGGED * 9, "five": [2049, 5000, 1, 64, 5000], "offset_view": [2049]}[layout]
    mus, rhos, priors = kl_tensors(sizes, offset_view=layout == "offset_view")
    with kl_unfused():
        kl = ops.kl_normal_scalar(mus, rhos, priors, n_batches=KL_NB)
        (kl * KL_UP).backward()
    check_kl_grads(mus, rhos, priors, [m.grad for m in mus], [r.grad for r in rhos], layout)
    _lib.check_device(DEV)


@gpu
@pytest.mark.parametrize("accumulate", [0, 1])
def test_kl_backward_accumulate_and_guard_elements(accumulate):
    """bnn_kl_backward itself: accumulate = 0 overwrites a NaN-filled buffer completely, accumulate = 1 adds to a known one
    (one rounding: fl(buffer + gradient), bit for bit), and neither writes past n -- eight guard floats follow each tensor."""
    sizes = KL_RAGGED * 9
    T, G, SENTINEL = len(sizes), 8, 777.0
    mus, rhos, priors = kl_tensors(sizes)
    lib = _lib.load()
    up = torch.full((1,), KL_UP, device=DEV)
    gen = torch.Generator().manual_seed(18)

    def run(acc, fill):
        bufs = []
        for _ in range(2):
            bs = []
            for n in sizes:
                b = torch.full((n + G,), SENTINEL, device=DEV)
                b[:n] = fill(n)
                bs.append(b)
            bufs.append(bs)
        before = [[b.clone() for b in bs] for bs in bufs]
        arr = ops._kl_descs([m.detach() for m in mus], [r.detach() for r in rhos], priors)
        gm = (ctypes.c_void_p * T)(*[b.data_ptr() for b in bufs[0]])
        gr = (ctypes.c_void_p * T)(*[b.data_ptr() for b in bufs[1]])
        _lib.check(lib.bnn_kl_backward(arr, T, KL_NB, _lib.ptr(up), gm, gr, acc, _lib.stream_ptr(DEV)), "bnn_kl_backward")
        torch.cuda.synchronize()
        for bs in bufs:
            for b, n in zip(bs, sizes):
                assert (b[n:] == SENTINEL).all(), "a guard element was written"
        return before, bufs

    _, plain = run(0, lambda n: torch.full((n,), float("nan"), device=DEV))
    for bs in plain:
        for b, n in zip(bs, sizes):
            assert torch.isfinite(b[:n]).all(), "accumulate = 0 left part of a NaN-filled buffer"
    check_kl_grads(mus, rhos, priors, [b[:n] for b, n in zip(plain[0], sizes)], [b[:n] for b, n in zip(plain[1], sizes)],
                   "bnn_kl_backward")
    if accumulate:
        before, acc = run(1, lambda n: torch.randn(n, generator=gen).to(DEV) * 1e-3)
        for k in range(2):
            for b0, b1, g, n in zip(before[k], acc[k], plain[k], sizes):
                assert torch.equal(b1[:n], b0[:n] + g[:n])
    _lib.check_device(DEV)
