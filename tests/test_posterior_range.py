"""Every kernel site that turns rho into sigma, sigma^2, ln sigma or d sigma / d rho, held to float64 over rho's whole range.

The rest of the suite runs those sites at rho ~ -2 .. -3, where the six device functions (sigma_draw, sigma_accurate, sigma_lrt /
dsigma_lrt, dsoftplus, mvn_softplus) agree to 3e-7 and an absolute 1e-5 cannot tell a wrong one from a right one.  Here rho is
tests/posterior_range.RHO_GRID -- the pruned value -30, the collapsed -100, the threshold 20 and its neighbours, fp32's exp
overflow at +-88 -- and every comparison is element by element against the bounds that module derives from the device code:
a RELATIVE bound at the sites that square, log or differentiate sigma, the draw's ABSOLUTE bound at the sites that draw a weight.

CPU tests: the bounds admit torch's own fp32 expression and the numpy emulations of the device functions with every native unit
moved by +-1 ulp, and reject the mutants a refactor could introduce.  Four more mutants cannot be rejected by ANY bound that
admits one fp32 rounding, because in fp32 they compute the same bits as the code; test_mutants_that_no_fp32_bound_can_reject
proves that for each instead of pretending otherwise:
  threshold >= instead of >        softplus(20) = 20 + 2.1e-9, and fl(20 + 2.1e-9) = 20;  d softplus = 1 - 2.1e-9 rounds to 1
  threshold at 15                  for rho in (15, 20] of the fixed grid (19.5, 19.9, 20^-, 20) softplus(rho) - rho <= 3.4e-9
  the floor added twice above 20   fl(rho + 2e-10) = rho for rho > 20
  a draw without the floor         1e-10 |eps| against the draw's own absolute term 2^-24 |eps| = 6e-8 |eps|
GPU tests (marked gpu): the entries of ops and the layers on grid posteriors.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import posterior_range as P
from klref import TINY, U

gpu = pytest.mark.gpu
G = P.RHO_GRID
G64 = G.astype(np.float64)


def T64(a):
    return torch.from_numpy(np.array(a, np.float64))             # (a copy: a broadcast view is not writable)


def grid_mu(shape, seed=0):
    """mu ~ N(0, 0.1), seeded, fp32."""
    return (0.1 * np.random.default_rng(1000 + seed).standard_normal(shape)).astype(np.float32)


# ================================================================================================ CPU
def test_grid_holds_every_corner():
    assert G.dtype == np.float32 and G.shape == (64,)
    for v in (-100.0, -88.0, -30.0, -16.6, 19.9, 20.0, 20.5, 89.0, 100.0):
        assert np.float32(v) in G[:P.N_FIXED]
    assert np.nextafter(np.float32(20), np.float32(0)) in G and np.nextafter(np.float32(20), np.float32(np.inf)) in G
    rest = G[P.N_FIXED:]
    assert rest.min() >= -60 and rest.max() <= 30 and len(np.unique(rest)) == 31
    assert P.MVN_OFF_GRID.min() == -80 and (P.MVN_OFF_GRID[G >= -80] == G[G >= -80]).all()
    assert 1.2 < P.RHO_ARG < 1.25


def test_bounds_admit_torch_fp32():
    """torch's own fp32 expression, its autograd derivative, Normal.log_prob and kl_divergence on it lie inside the accurate bounds
    against float64 at every grid value: the bounds are not tighter than the reference itself."""
    rho = torch.from_numpy(G.copy()).requires_grad_()
    sg = 1e-10 + F.softplus(rho)
    P.assert_within(sg.detach().numpy(), P.sigma64(G), P.bound_sigma(G), "torch fp32 sigma", G)
    P.assert_within(sg.detach().numpy(), P.sigma64(G), P.bound_sigma(G, "lrt"), "torch fp32 sigma (ocml count)", G)
    (ds,) = torch.autograd.grad(sg.sum(), rho)
    P.assert_within(ds.numpy(), P.dsigma64(G), P.bound_dsigma(G), "torch fp32 dsigma", G)
    P.assert_within(ds.numpy(), P.dsigma64(G), P.bound_dsigma(G, "lrt"), "torch fp32 dsigma (ocml count)", G)
    P.assert_within((sg * sg).detach().numpy(), P.s2_64(G), P.bound_s2(G), "torch fp32 sigma^2", G)
    mu = grid_mu(64)
    dist = torch.distributions.Normal(torch.from_numpy(mu), sg.detach())
    lp = dist.log_prob(torch.zeros(64))
    P.assert_within(lp.numpy(), P.logprob0_64(mu, G), P.bound_logprob0(mu, G), "torch fp32 log_prob(0)", G)
    for pm, ps in ((0.0, 0.1), (0.3, 1.0)):
        pm32, ps32 = float(np.float32(pm)), float(np.float32(ps))
        kl = torch.distributions.kl_divergence(dist, torch.distributions.Normal(torch.tensor(pm), torch.tensor(ps)))
        P.assert_within(kl.numpy(), P.kl64(mu, G, pm32, ps32), P.bound_kl_elem(mu, G, pm32, ps32), "torch fp32 kl_divergence", G)
    i = int(np.where(G == -100)[0][0])
    assert 20.0 < P.kl64(0.0, G, 0.0, 1.0)[i] < 23.0            # -ln(1e-10) - 0.5: the collapsed posterior's KL is not small


EMULATIONS = {
    "sigma_draw": (P.emu_sigma_draw, P.sigma64, P.bound_sigma_draw),
    "sigma_accurate": (P.emu_sigma_accurate, P.sigma64, P.bound_sigma),
    "sigma_lrt": (P.emu_sigma_lrt, P.sigma64, lambda r: P.bound_sigma(r, "lrt")),
    "dsoftplus": (P.emu_dsoftplus, P.dsigma64, P.bound_dsigma),
    "dsigma_lrt": (P.emu_dsigma_lrt, P.dsigma64, lambda r: P.bound_dsigma(r, "lrt")),
}


@pytest.mark.parametrize("name", sorted(EMULATIONS))
def test_emulation_is_inside_its_own_bound(name):
    """... on the grid, correctly rounded units first, then every native unit moved by +-1 ulp (27 combinations)."""
    emu, ref, bound = EMULATIONS[name]
    P.assert_within(emu(G), ref(G), bound(G), "emu " + name, G)
    for nat in P.PERTURBED:
        P.assert_within(emu(G, nat), ref(G), bound(G), "emu %s, units moved (%d, %d, %d) ulp" % (name, nat.d_exp, nat.d_log, nat.d_rcp), G)


def test_mvn_and_product_emulations_are_inside_their_bounds():
    diag = np.arange(64) % 2 == 0
    s = np.where(diag, G, P.MVN_OFF_GRID)
    for nat in P.PERTURBED:
        P.assert_within(P.emu_mvn_softplus(s, nat), P.mvn_v64(s, False), P.bound_mvn_v(s, False), "emu mvn_softplus", s)
        P.assert_within(P.emu_mvn_v(s, diag, nat), P.mvn_v64(s, diag), P.bound_mvn_v(s, diag), "emu mvn_v", s)
        P.assert_within(P.emu_mvn_l(s, diag, nat), P.mvn_l64(s, diag), P.bound_mvn_l(s, diag), "emu mvn_l", s)
        sl, dl = P.emu_sigma_lrt(G, nat), P.emu_dsigma_lrt(G, nat)
        P.assert_within(sl * sl, P.s2_64(G), P.bound_s2(G, "lrt"), "emu sigma_lrt^2", G)
        P.assert_within(np.float32(2.0) * sl * dl, P.ds2_64(G), P.bound_ds2(G, "lrt"), "emu 2 sigma_lrt dsigma_lrt", G)
        sa = P.emu_sigma_accurate(G, nat)
        P.assert_within(nat.log2(sa) * P.LN2, P.lnsigma64(G), P.bound_lnsigma(G), "emu ln sigma_accurate", G)


def _sigma_sites(**kw):
    """(site, mutant output, reference, accurate bound) of the two accurate sigma functions under one mutation."""
    return [("sigma_accurate", P.emu_sigma_accurate(G, **kw), P.sigma64(G), P.bound_sigma(G)),
            ("sigma_lrt", P.emu_sigma_lrt(G, **kw), P.sigma64(G), P.bound_sigma(G, "lrt"))]


def _dsigma_sites(**kw):
    return [("dsoftplus", P.emu_dsoftplus(G, **kw), P.dsigma64(G), P.bound_dsigma(G)),
            ("dsigma_lrt", P.emu_dsigma_lrt(G, **kw), P.dsigma64(G), P.bound_dsigma(G, "lrt"))]


ACCURATE_MUTANTS = {
    # name -> (sites, a grid value at which every site must reject it)
    "sigma_draw_for_accurate": (lambda: [("sigma_accurate <- sigma_draw", P.emu_sigma_draw(G), P.sigma64(G), P.bound_sigma(G)),
                                         ("sigma_lrt <- sigma_draw", P.emu_sigma_draw(G), P.sigma64(G), P.bound_sigma(G, "lrt"))], -20.0),
    "threshold_absent": (lambda: _sigma_sites(thr="none"), 89.0),
    "floor_dropped": (lambda: _sigma_sites(floor="dropped"), -30.0),
    "dsoftplus_of_minus_rho": (lambda: _dsigma_sites(negate=True), -30.0),
    "dsigma_taken_as_sigma": (lambda: [("dsoftplus <- sigma_accurate", P.emu_sigma_accurate(G), P.dsigma64(G), P.bound_dsigma(G)),
                                       ("dsigma_lrt <- sigma_lrt", P.emu_sigma_lrt(G), P.dsigma64(G), P.bound_dsigma(G, "lrt"))], -30.0),
    "s2_not_squared": (lambda: [("sigma_accurate for s2", P.emu_sigma_accurate(G), P.s2_64(G), P.bound_s2(G)),
                                ("sigma_lrt for s2", P.emu_sigma_lrt(G), P.s2_64(G), P.bound_s2(G, "lrt"))], -2.0),
}


@pytest.mark.parametrize("name", sorted(ACCURATE_MUTANTS))
def test_accurate_bound_rejects_mutant(name):
    sites, at = ACCURATE_MUTANTS[name]
    for site, got, ref, bound in sites():
        out = P.rejected_at(got, ref, bound, G)
        print("%s / %s: rejected at %d grid values: %s" % (name, site, len(out), np.array2string(out, precision=4)))
        assert np.float32(at) in out.astype(np.float32), "mutant %s at site %s is NOT rejected at rho = %g (rejected at %s)" % (
            name, site, at, out)


def test_sigma_draw_for_accurate_is_rejected_over_the_whole_underflow_range():
    """sigma_draw is 1e-10 on (-30, -17.3) where sigma is up to 4e-8, 6 % off at -16, 0.9 % at -12: inside the
    draw's absolute bound and far outside the accurate one, at every grid value from -30 to -8."""
    got, ref = P.emu_sigma_draw(G).astype(np.float64), P.sigma64(G)
    out = P.rejected_at(got, ref, P.bound_sigma(G), G)
    for v in (-30.0, -20.0, -17.0, -16.6, -16.0, -14.0, -12.0, -10.0, -8.0):
        assert np.float32(v) in out.astype(np.float32), v
    rel = np.abs(got - ref) / ref
    assert (got[(G > -30) & (G < -17.4)] == np.float32(1e-10)).all()
    assert 0.03 < rel[G == -16][0] < 0.09 and 0.004 < rel[G == -12][0] < 0.012
    assert P.worst_ratio(got, ref, P.bound_sigma_draw(G)).max() <= 1.0


def test_draw_bound_rejects_its_mutant():
    """A draw with sigma(|rho|): rejected at every negative fixed grid value down to -100."""
    rho = G
    eps = np.ones(64)
    mu = grid_mu(64).astype(np.float64)
    ref = mu + P.sigma64(rho) * eps
    ok = mu + P.emu_sigma_draw(rho).astype(np.float64) * eps
    assert P.worst_ratio(ok, ref, P.bound_draw(ref, eps, rho)).max() <= 1.0
    bad = mu + P.emu_sigma_draw(rho, fold=True).astype(np.float64) * eps
    out = P.rejected_at(bad, ref, P.bound_draw(ref, eps, rho), rho)
    for v in (-100.0, -30.0, -5.0, -2.0, -1e-3):
        assert np.float32(v) in out.astype(np.float32), "a draw with sigma(|rho|) is NOT rejected at rho = %g" % v


def test_mutants_that_no_fp32_bound_can_reject():
    """Four mutants compute, at every FIXED grid value, a number that differs from the float64 reference by less than half
    an fp32 rounding (the first three), or by less than 1 / 500 of the draw's own absolute term (the fourth): they are the code's
    own bits, so a bound that admits one fp32 rounding admits them.  The figures are asserted, so that a change of the grid or of
    the functions that makes one of them visible fails here and moves it to ACCURATE_MUTANTS."""
    g, g64 = G[:P.N_FIXED], G64[:P.N_FIXED]
    for thr in ("ge", "15"):
        hit = (g64 >= 20.0) if thr == "ge" else (g64 > 15.0)
        mut_s = np.where(hit, g64, P.softplus64(g64)) + 1e-10
        mut_d = np.where(hit, 1.0, P.dsigma64(g64))
        dev_s = np.abs(mut_s - P.sigma64(g64)) / P.sigma64(g64) / U
        dev_d = np.abs(mut_d - P.dsigma64(g64)) / P.dsigma64(g64) / U
        print("threshold %s: largest deviation %.3g u (sigma), %.3g u (dsigma)" % (thr, dev_s.max(), dev_d.max()))
        assert dev_s.max() < 0.5 and dev_d.max() < 0.5
        for emu in (P.emu_sigma_accurate, P.emu_sigma_lrt):
            assert P.worst_ratio(emu(g, thr=thr), P.sigma64(g), P.bound_sigma(g, "lrt")).max() <= 1.0
    for emu in (P.emu_sigma_accurate, P.emu_sigma_lrt):
        assert (emu(g, floor="twice") == emu(g)).all()                      # bit for bit
    no_floor, with_floor = P.emu_sigma_draw(G, floor=False).astype(np.float64), P.emu_sigma_draw(G).astype(np.float64)
    assert (np.abs(no_floor - with_floor) <= 1.0001e-10 + 2.0 * U * with_floor).all() and 1.0001e-10 < U / 500
    assert P.worst_ratio(no_floor, P.sigma64(G), P.bound_sigma_draw(G)).max() <= 1.0


def test_module_cpu_twins_take_the_grid():
    """WeightNormal.stddev / .variance / .dist and LocalReparamLinear's torch expression on grid posteriors against float64."""
    from bayesianneuralnetworks_amd.nn import LocalReparamLinear
    from bayesianneuralnetworks_amd.nn.core import WeightNormal
    w = WeightNormal(8, 8)
    mu = grid_mu((8, 8))
    with torch.no_grad():
        w.mean.copy_(torch.from_numpy(mu))
        w.scale.copy_(torch.from_numpy(P.tile(G, (8, 8))))
    rho = w.scale.detach().numpy()
    P.assert_within(w.stddev.detach().numpy(), P.sigma64(rho), P.bound_sigma(rho), "WeightNormal.stddev", rho)
    P.assert_within(w.variance.detach().numpy(), P.s2_64(rho), P.bound_s2(rho), "WeightNormal.variance", rho)
    P.assert_within(w.dist.log_prob(torch.zeros(8, 8)).detach().numpy(), P.logprob0_64(mu, rho), P.bound_logprob0(mu, rho),
                    "WeightNormal.dist.log_prob(0)", rho)
    layer = LocalReparamLinear(64, 3)
    mu_w, mu_b = grid_mu((3, 64), 1), grid_mu(3, 2)
    rho_w, rho_b = np.stack([P.tile(G, (64,), s) for s in (0, 5, 11)]), G[[4, 17, 32]].copy()       # bias: -30, 0, 100
    with torch.no_grad():
        for p, v in ((layer.weight.mean, mu_w), (layer.weight.scale, rho_w), (layer.bias.mean, mu_b), (layer.bias.scale, rho_b)):
            p.copy_(torch.from_numpy(v))
    x = torch.eye(64)                                                       # row k: m = mu_w[:, k] + mu_b, v = s2_w[:, k] + s2_b
    torch.manual_seed(5)
    y = layer(x).detach().numpy().astype(np.float64)
    eps = layer._cpu_eps.numpy().astype(np.float64)
    m = mu_w.T.astype(np.float64) + mu_b
    v = P.s2_64(rho_w).T + P.s2_64(rho_b)
    bv = P.bound_s2(rho_w).T + P.bound_s2(rho_b) + 65 * U * v              # 64 products (63 of them 0) and the bias: gamma_65
    sd = np.sqrt(v + 1e-16)
    bound = (bv / (2.0 * sd) + U * sd) * np.abs(eps) + 66 * U * np.abs(m) + 2 * U * np.abs(m + sd * eps) + TINY
    P.assert_within(y, m + sd * eps, bound, "LocalReparamLinear on the CPU", np.broadcast_to(rho_w.T, y.shape))


# ================================================================================================ GPU
GENS = [0, 1]            # _rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16


@pytest.fixture
def dev():
    """The device, with the device epoch words at zero (the keys below are explicit; an earlier test's captured graph may have
    bumped them) and the compute mode put back afterwards."""
    assert torch.cuda.is_available()
    import bayesianneuralnetworks_amd as bnn
    from bayesianneuralnetworks_amd._rng import default_generator
    for cell in default_generator._epoch_dev.values():
        cell.zero_()
    yield torch.device("cuda:0")
    bnn.set_compute("f32")


def D(t):
    return t.detach().double().cpu().numpy()


def dkey(stream, S, gen=0, seed=20261021):
    from bayesianneuralnetworks_amd._rng import DrawKey
    return DrawKey(seed, stream, 1, S, 4, 0, gen)


def put(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bf16_within(got, ref, bound, site, rho):
    """A bf16 output: inside the rounding interval of [ref - bound, ref + bound], reported as |err| over bound + half a bf16 ulp."""
    from bf16ref import rounding_interval, ulp_bf16
    g, r, b = T64(D(got)), T64(ref), T64(np.broadcast_to(bound, np.shape(ref)))
    lo, hi = rounding_interval(r, b)
    bad = ~((g >= lo) & (g <= hi))
    full = b + 0.5 * ulp_bf16(torch.maximum(r.abs(), torch.full_like(r, TINY)))
    P.assert_within(g.numpy(), ref, full.numpy(), site, rho)
    assert not bool(bad.any()), "%s: %d elements outside the rounding interval of the bound" % (site, int(bad.sum()))


def _sigma_operand(rho_t, rows, cols, bf16):
    """bnn_draw_multi kind 2 (BNN_DRAW_SIGMA: the sigma operand of a Flipout layer) of one (rows, cols) tensor."""
    from bayesianneuralnetworks_amd import _lib, ops
    ld = (cols + 7) // 8 * 8
    out = torch.zeros((rows, ld), dtype=torch.bfloat16 if bf16 else torch.float32, device=rho_t.device)
    arr = (_lib.DrawTensor * 1)()
    ops._draw_slot(arr[0], rho_t, rho_t, rows, cols, out.data_ptr(), ld, rows * ld, _lib.BF16 if bf16 else _lib.F32, kind=_lib.DRAW_SIGMA)
    ops._draw_launch(arr, 1, 1, rho_t.device)
    assert bool((out[:, cols:] == 0).all()) or not bf16
    return out[:, :cols]


@gpu
@pytest.mark.parametrize("n", [64, 67])
def test_posterior_accurate_elementwise_entries(dev, n):
    """ops.sigma, ops.sample_affine_eps, ops.prune_score and the sigma operand of bnn_draw_multi (kind 2): sigma_accurate sites,
    relative bound.  64: the 16-byte path alone; 67: its scalar tail, which holds -40, -30 and -20."""
    from bayesianneuralnetworks_amd import ops
    rho, mu = P.tile(G, (n,), shift=n % 64 or 1), grid_mu(n, n)
    eps = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    r, m, e = put(rho, dev), put(mu, dev), put(eps, dev)
    P.assert_within(D(ops.sigma(r)), P.sigma64(rho), P.bound_sigma(rho), "bnn_sigma", rho)
    ref = mu.astype(np.float64) + P.sigma64(rho) * eps
    P.assert_within(D(ops.sample_affine_eps(m, r, e)), ref, P.bound_affine_accurate(ref, eps, rho), "bnn_sample_affine_eps", rho)
    P.assert_within(D(ops.prune_score(m, r)), P.logprob0_64(mu, rho), P.bound_logprob0(mu, rho), "bnn_prune_score", rho)
    rows, cols = (4, 16) if n == 64 else (1, 67)
    r2 = r.reshape(rows, cols)
    P.assert_within(D(_sigma_operand(r2, rows, cols, False)).reshape(-1), P.sigma64(rho), P.bound_sigma(rho), "bnn_draw_multi kind 2, fp32", rho)
    bf16_within(_sigma_operand(r2, rows, cols, True).reshape(-1), P.sigma64(rho), P.bound_sigma(rho), "bnn_draw_multi kind 2, bf16", rho)


def _g_rho_draw(eps, rho, S):
    """g_rho = (sum_s g_s eps_s) dsoftplus(rho) for g = 1 -> (ref, bound): gamma_{S + 2} on the sum and the product, and
    dsoftplus's relative error."""
    ds = P.dsigma64(rho)
    ref = eps.sum(0) * ds
    return ref, P.gamma(S + 2) * np.abs(eps).sum(0) * ds + P.rel_dsigma(rho) * np.abs(ref) + TINY


@gpu
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("n", [64, 67])
def test_posterior_draw_elementwise_entries(dev, n, gen):
    """ops.sample_affine_philox (fp32 and bf16 output, both generators) under the draw bound on the key's own eps, and its
    backward bnn_sample_affine_bwd (keyed and eps-supplied) with an upstream gradient of ones."""
    from bayesianneuralnetworks_amd import ops
    S = 3
    rho, mu = P.tile(G, (n,), shift=n % 64 or 1), grid_mu(n, n + gen)
    r, m = put(rho, dev), put(mu, dev)
    key = dkey(7, S, gen)
    eps = D(ops.eps_philox((n,), key, dev))
    assert np.isfinite(eps).all() and np.abs(eps).max() < 7
    ref = mu.astype(np.float64) + P.sigma64(rho) * eps
    w32 = ops._sample_affine_philox_raw(m, r, key)
    P.assert_within(D(w32), ref, P.bound_draw(ref, eps, rho), "bnn_sample_affine_philox fp32, gen %d" % gen, np.broadcast_to(rho, ref.shape))
    bf16_within(ops._sample_affine_philox_raw(m, r, key, torch.bfloat16), ref, P.bound_draw(ref, eps, rho),
                "bnn_sample_affine_philox bf16, gen %d" % gen, np.broadcast_to(rho, ref.shape))
    mg, rg = m.clone().requires_grad_(), r.clone().requires_grad_()
    w = ops.sample_affine_philox(mg, rg, key)
    assert torch.equal(w, w32)
    g_mu, g_rho = torch.autograd.grad(w, (mg, rg), torch.ones_like(w))
    assert bool((g_mu == S).all())
    gref, gb = _g_rho_draw(eps, rho, S)
    P.assert_within(D(g_rho), gref, gb, "bnn_sample_affine_bwd keyed, gen %d" % gen, rho)
    e1 = put(eps[0].astype(np.float32), dev)
    w1 = ops.sample_affine_eps(mg, rg, e1)
    _, g_rho1 = torch.autograd.grad(w1, (mg, rg), torch.ones_like(w1))
    gref, gb = _g_rho_draw(eps[:1], rho, 1)
    P.assert_within(D(g_rho1), gref, gb, "bnn_sample_affine_bwd eps supplied", rho)


@gpu
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("shape", [(8, 64), (5, 68)], ids=["8x64", "5x68"])
def test_posterior_draw_layers(dev, shape, S, gen):
    """ops.draw_layers / bnn_draw_multi kind 0: the bf16 weight (flat items at S = 1 and whole rows of 8, items spread over the
    samples at S = 3, the general item at 68 columns), the fp32 bias with a ragged tail, and the three bf16 planes of the fp32
    draw.  Draw bound, on the keys' own eps."""
    from bayesianneuralnetworks_amd import ops
    N, K = shape
    rho_w, mu_w = P.tile(G, (N, K), shift=3), grid_mu((N, K), K)
    rho_b, mu_b = P.tile(G, (N,), shift=3 + gen), grid_mu(N, 9)          # -40, -30, -20, -17, -16.6, ...
    kw, kb = dkey(11, S, gen), dkey(12, S, gen)
    t = [put(a, dev) for a in (mu_w, rho_w, mu_b, rho_b)]
    eps_w, eps_b = D(ops.eps_philox((N, K), kw, dev)), D(ops.eps_philox((N,), kb, dev))
    ref_w = mu_w.astype(np.float64) + P.sigma64(rho_w) * eps_w
    ref_b = mu_b.astype(np.float64) + P.sigma64(rho_b) * eps_b
    pre = ops.draw_layers([(t[0], t[1], t[2], t[3], kw, kb)], S)[0]
    assert bool((pre.w[:, :, K:] == 0).all())
    bf16_within(pre.w[:, :, :K], ref_w, P.bound_draw(ref_w, eps_w, rho_w), "bnn_draw_multi kind 0 bf16, gen %d" % gen,
                np.broadcast_to(rho_w, ref_w.shape))
    P.assert_within(D(pre.b), ref_b, P.bound_draw(ref_b, eps_b, rho_b), "bnn_draw_multi kind 0 fp32 bias, gen %d" % gen,
                    np.broadcast_to(rho_b, ref_b.shape))
    assert torch.equal(pre.w[:, :, :K], ops._sample_affine_philox_raw(t[0], t[1], kw, torch.bfloat16))      # one device function
    if gen == 0:
        pre3 = ops.draw_layers([(t[0], t[1], t[2], t[3], kw, kb)], S, x3=True)[0]
        w3 = pre3.w.double().sum(0)[:, :, :K]                         # h + m + l = the fp32 draw up to 2^-27 |w|
        P.assert_within(D(w3), ref_w, P.bound_draw(ref_w, eps_w, rho_w) + 0.25 * U * np.abs(ref_w), "bnn_draw_multi kind 0, three planes",
                        np.broadcast_to(rho_w, ref_w.shape))


@gpu
@pytest.mark.parametrize("gen", GENS)
def test_posterior_flipout_draw_and_weight_backward(dev, gen):
    """bnn_draw_multi BNN_DRAW_FLIPOUT (w = mu + sigma R S^T: a draw site, eps = +-1) and bnn_flipout_weight_backward with an
    upstream gradient of ones: g_rho = (sum_s R_s S_s^T) dsoftplus(rho)."""
    import ctypes
    from bayesianneuralnetworks_amd import _lib, ops
    O, K, S = 8, 64, 3
    rho, mu = P.tile(G, (O, K), shift=5), grid_mu((O, K), 3)
    r, m = put(rho, dev), put(mu, dev)
    key = dkey(13, S, gen)
    sg = D(ops.flipout_signs(key, 1, O + K, dev))[:, 0]
    eps = sg[:, :O, None] * sg[:, None, O:]
    assert set(np.unique(eps)) == {-1.0, 1.0}
    ref = mu.astype(np.float64) + P.sigma64(rho) * eps
    P.assert_within(D(ops.flipout_draw(m, r, key)), ref, P.bound_draw(ref, eps, rho), "BNN_DRAW_FLIPOUT fp32, gen %d" % gen,
                    np.broadcast_to(rho, ref.shape))
    wb = ops.flipout_draw(m, r, key, torch.bfloat16, pad=True)
    assert wb.shape[-1] == 64 or bool((wb[:, :, K:] == 0).all())
    bf16_within(wb[:, :, :K], ref, P.bound_draw(ref, eps, rho), "BNN_DRAW_FLIPOUT bf16, gen %d" % gen, np.broadcast_to(rho, ref.shape))
    gw = torch.ones((S, O, K), device=dev)
    g_mu, g_rho = torch.empty_like(m), torch.empty_like(r)
    rs = ops._rng_struct(key, dev)
    _lib.check(_lib.load().bnn_flipout_weight_backward(_lib.ptr(gw), O * K, _lib.ptr(r), _lib.ptr(g_mu), _lib.ptr(g_rho), O, K, S,
                                                       ctypes.byref(rs), _lib.stream_ptr(dev)), "bnn_flipout_weight_backward")
    assert bool((g_mu == S).all())
    gref, gb = _g_rho_draw(eps, rho, S)
    P.assert_within(D(g_rho), gref, gb, "bnn_flipout_weight_backward, gen %d" % gen, rho)


# ------------------------------------------------------------------------------------------------ sigma^2 sites
def _g_rho_s2(g_v, rho):
    """g_rho = g_v ds2(rho) with sigma_lrt / dsigma_lrt: their bound, the product's rounding, the contraction's one exact term (an
    fp32-mode contraction may split an operand in three bf16 planes: 2^-27) and the final product."""
    ref = g_v * P.ds2_64(rho)
    return ref, np.abs(g_v) * (P.bound_ds2(rho, "lrt") + 3.0 * U * P.ds2_64(rho)) + TINY


@gpu
@pytest.mark.parametrize("shape", [(5, 64), (3, 68)], ids=["5x64", "3x68"])
def test_posterior_sigma2_dense_sites(dev, shape):
    """bnn_lrt_prepare, bnn_lrt_backward_weight (a deterministic input) and bnn_moments_backward_weight (an input with a variance)
    on a one-row input of ones: s2 against s2_64, g_rho = g_v ds2_64, weight and bias."""
    from bayesianneuralnetworks_amd import ops
    N, K = shape
    rho_w, mu_w = P.tile(G, (N, K), shift=1), grid_mu((N, K), 4)
    rho_b, mu_b = P.tile(G, (N,), shift=2), grid_mu(N, 5)                 # -87, -40, -30, -20, -17
    s2_w, s2_b = ops._lrt_prepare_raw(put(rho_w, dev), put(rho_b, dev))
    P.assert_within(D(s2_w), P.s2_64(rho_w), P.bound_s2(rho_w, "lrt"), "bnn_lrt_prepare weight", rho_w)
    P.assert_within(D(s2_b), P.s2_64(rho_b), P.bound_s2(rho_b, "lrt"), "bnn_lrt_prepare bias", rho_b)
    g_v = (0.5 + np.random.default_rng(K).random((1, N))).astype(np.float32)
    g_m = grid_mu((1, N), 6)
    for site, with_var in (("bnn_lrt_backward_weight", False), ("bnn_moments_backward_weight", True)):
        p = [put(a, dev).requires_grad_() for a in (mu_w, rho_w, mu_b, rho_b)]
        ones = torch.ones((1, K), device=dev)
        a = ops.Moments(ones, torch.zeros_like(ones)) if with_var else ones
        out = ops.moments_linear(a, p[0], p[1], p[2], p[3], track=True)
        grads = torch.autograd.grad((out.mean, out.var), p, (put(g_m, dev), put(g_v, dev)))
        ref, b = _g_rho_s2(g_v[0][:, None].astype(np.float64), rho_w)
        P.assert_within(D(grads[1]), ref, b, site + " g_rho weight", rho_w)
        ref, b = _g_rho_s2(g_v[0].astype(np.float64), rho_b)
        P.assert_within(D(grads[3]), ref, b, site + " g_rho bias", rho_b)
        assert np.array_equal(D(grads[2]), g_m[0].astype(np.float64))


@gpu
@pytest.mark.parametrize("shape", [(8, 8), (5, 13)], ids=["8x8", "5x13"])
def test_posterior_sigma2_conv3d_sites(dev, shape):
    """bnn_conv3d_lrt_backward_weight and bnn_conv3d_moments_backward_weight (weight and bias): a 1 x 1 x 1 kernel on one voxel of
    ones, so every weight's g_rho is g_v[o] ds2_64(rho)."""
    from bayesianneuralnetworks_amd import ops
    O, C = shape
    rho_w, mu_w = P.tile(G, (O, C, 1, 1, 1), shift=7), grid_mu((O, C, 1, 1, 1), 7)
    rho_b, mu_b = P.tile(G, (O,), shift=2), grid_mu(O, 8)
    g_v = (0.5 + np.random.default_rng(C).random((1, O, 1, 1, 1))).astype(np.float32)
    g_m = grid_mu((1, O, 1, 1, 1), 6)
    for site, with_var in (("bnn_conv3d_lrt_backward_weight", False), ("bnn_conv3d_moments_backward_weight", True)):
        p = [put(a, dev).requires_grad_() for a in (mu_w, rho_w, mu_b, rho_b)]
        ones = torch.ones((1, C, 1, 1, 1), device=dev)
        a = ops.Moments(ones, torch.zeros_like(ones)) if with_var else ones
        out = ops.moments_convNd(a, p[0], p[1], p[2], p[3], (1, 1, 1), (0, 0, 0), (1, 1, 1), track=True)
        grads = torch.autograd.grad((out.mean, out.var), p, (put(g_m, dev), put(g_v, dev)))
        gv = g_v.reshape(O).astype(np.float64)
        ref, b = _g_rho_s2(gv[:, None, None, None, None], rho_w)
        P.assert_within(D(grads[1]), ref, b, site + " g_rho weight", rho_w)
        ref, b = _g_rho_s2(gv, rho_b)
        P.assert_within(D(grads[3]), ref, b, site + " g_rho bias", rho_b)


# ------------------------------------------------------------------------------------------------ KL
KL_PRIORS = [(0.0, 0.1), (0.3, 1.0)]


def _kl_sums(mus, rhos, priors):
    """Per-tensor float64 KL sums, the KLDivergence scalar, and the bounds: kl_elem's own per element, gamma_9 on the absolute
    terms for a thread's 8 fp32 additions and the output's rounding (everything above a thread's sum is added in double)."""
    sums, bounds = [], []
    for mu, rho, (pm, ps) in zip(mus, rhos, priors):
        pm, ps = float(np.float32(pm)), float(np.float32(ps))
        k = P.kl64(mu, rho, pm, ps)
        sums.append(k.sum())
        bounds.append(P.bound_kl_elem(mu, rho, pm, ps).sum() + P.gamma(9) * np.abs(k).sum())
    T = len(mus)
    scalar = sum(s / m.size for s, m in zip(sums, mus)) / T
    b_scalar = sum((b + U * abs(s)) / m.size for s, b, m in zip(sums, bounds, mus)) / T + U * abs(scalar)
    return np.array(sums + [scalar]), np.array(bounds + [b_scalar])


@gpu
def test_posterior_kl_forward_sums(dev):
    """ops.kl_normal on grid posteriors of 64, 67 and 2048 + 67 elements against the float64 sums; at rho = -100 one element's KL is
    about 20 (prior 0.1) and must not be lost.  Then the same KL carried by ops.draw_layers' launch (the flat draw items hold the
    posterior in registers) and finished by ops.mc_mean: the same bits."""
    from bayesianneuralnetworks_amd import ops
    sizes = [64, 67, 2048 + 67, 67]
    mus = [grid_mu(n, 20 + i) for i, n in enumerate(sizes)]
    rhos = [P.tile(G, (n,), shift=i) for i, n in enumerate(sizes)]
    rhos[3] = P.tile(G[G <= 0], (67,))               # no term of 5e5 from rho = 100 beside the collapsed elements' 20
    priors = [KL_PRIORS[i % 2] for i in range(4)]
    ref, bound = _kl_sums(mus, rhos, priors)
    out = ops.kl_normal([put(m, dev) for m in mus], [put(r, dev) for r in rhos], priors)
    P.assert_within(D(out), ref, bound, "bnn_kl_forward")
    i100 = int(np.where(rhos[3] == -100)[0][0])
    assert P.kl64(mus[3], rhos[3], float(np.float32(0.3)), 1.0)[i100] > 20.0 > 1000 * bound[3]     # one such element is 1000 bounds
    N, K, S = 8, 64, 1
    mu_w, rho_w, mu_b, rho_b = grid_mu((N, K), 30), P.tile(G, (N, K), shift=9), grid_mu(N, 31), P.tile(G, (N,), shift=2)
    t = [put(a, dev) for a in (mu_w, rho_w, mu_b, rho_b)]
    ref, bound = _kl_sums([mu_w, mu_b], [rho_w, rho_b], KL_PRIORS)
    want = ops.kl_normal([t[0], t[2]], [t[1], t[3]], KL_PRIORS)
    P.assert_within(D(want), ref, bound, "bnn_kl_forward, layer")
    h = ops.kl_normal_begin([t[0], t[2]], [t[1], t[3]], KL_PRIORS, carry=True)
    ops.draw_layers([(t[0], t[1], t[2], t[3], dkey(21, S, 1), dkey(22, S, 1))], S, kl=h)
    assert h.launched
    ops.mc_mean(torch.zeros((S, 2, 4), device=dev), kl=h)
    P.assert_within(D(h.out), ref, bound, "KL carried by bnn_draw_multi")
    assert torch.equal(h.out, want)


# ------------------------------------------------------------------------------------------------ draws fused into a contraction
def _layer_operands(N, K, S, mode, dev, bias=True, shift=3):
    """Grid posterior of a (N, K) layer on the device, its keys (the generator the layer would key with in `mode`), the keys' eps
    and the float64 draws."""
    from bayesianneuralnetworks_amd import _rng, ops
    gen = _rng.generator_for(mode)
    post = [grid_mu((N, K), K + N), P.tile(G, (N, K), shift=shift), grid_mu(N, N), P.tile(G, (N,), shift=shift + 1)]
    kw, kb = dkey(31, S, gen), dkey(32, S, gen)
    eps_w, eps_b = D(ops.eps_philox((N, K), kw, dev)), D(ops.eps_philox((N,), kb, dev))
    ref_w = post[0].astype(np.float64) + P.sigma64(post[1]) * eps_w
    ref_b = post[2].astype(np.float64) + P.sigma64(post[3]) * eps_b
    if not bias:
        post[2] = post[3] = None
    return dict(post=post, t=[None if a is None else put(a, dev) for a in post], kw=kw, kb=kb, eps_w=eps_w, eps_b=eps_b,
                ref_w=ref_w, ref_b=ref_b)


def _one_weight_per_output(L, mode, S):
    """y_s[k, n] = W_s[n, k] + b_s[n] (an identity input: every other product is an exact zero) -> (ref, bound): the draw bound of
    the weight (contracted as bf16 in the bf16 mode) and of the bias, and three roundings of y (the bias addition, the fp32 mode's
    three-plane operands, the store)."""
    rho_w, rho_b = L["post"][1], L["post"][3]
    bf = mode == "bf16"
    ref = L["ref_w"].transpose(0, 2, 1) + L["ref_b"][:, None, :]
    bw = P.bound_draw(L["ref_w"], L["eps_w"], rho_w, bf16=bf).transpose(0, 2, 1)
    bb = P.bound_draw(L["ref_b"], L["eps_b"], rho_b)[:, None, :]
    return ref, bw + bb + 3.0 * U * np.abs(ref), np.broadcast_to(rho_w.T, ref.shape)


@gpu
@pytest.mark.parametrize("N", [5, 16, 37])
@pytest.mark.parametrize("mode,K", [("f32", 64), ("f32", 67), ("bf16", 64), ("bf16", 68)],
                         ids=["f32", "f32_generic", "bf16_dense", "bf16_fused"])
def test_posterior_linear_sampled_on_identity(dev, mode, K, N):
    """(K = 67: no 16-byte loads, so the generic tile kernel k_gemm_nt draws the weights.)"""
    _linear_on_identity(dev, mode, K, N, 3)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_posterior_linear_sampled_on_identity_one_sample(dev, mode):
    """One sample: the weight-gradient launch is not split over the samples, so wgrad_store / wgrad_bias_store apply dsoftplus
    themselves (with three samples k_wgrad_reduce and bnn_sample_affine_bwd do)."""
    _linear_on_identity(dev, mode, 64, 37, 1)


def _linear_on_identity(dev, mode, K, N, S):
    """ops.linear_sampled with x = I_K: bnn_linear_forward_sampled (fp32 compute, and bf16 compute at K = 68, where the draw-once
    path does not take the layer) and bnn_draw_multi + bnn_dense_forward (bf16, K = 64), the narrow kernel (N <= 16), a wider one
    and a ragged last column (37).  Then the backward on an upstream gradient of ones under tests/golden/bwdref's own bound, whose
    g_rho = (sum_s eps_s) dsoftplus(rho) is relative to dsoftplus at every grid value."""
    import bwdref
    from bayesianneuralnetworks_amd import ops
    from test_operand_alignment import linear_plan
    L = _layer_operands(N, K, S, mode, dev)
    mu_w, rho_w, mu_b, rho_b = [t.clone().requires_grad_() for t in L["t"]]
    x = torch.eye(K, device=dev).expand(S, K, K).contiguous().requires_grad_()
    y = ops.linear_sampled(x, mu_w, rho_w, mu_b, rho_b, L["kw"], L["kb"], False, mode)
    ref, bound, rho_at = _one_weight_per_output(L, mode, S)
    P.assert_within(D(y), ref, bound, "ops.linear_sampled %s K %d N %d" % (mode, K, N), rho_at)
    if N <= 16 and (mode == "f32" or K % 8 != 0):
        # bnn_linear_forward_sampled_kl, both compute modes (bf16 at K = 68: the draw-once path does not take the layer): the narrow
        # layer's launch carries a KL's first pass; the layer's bits and the KL's are unchanged
        kl_t = ([L["t"][0], L["t"][2]], [L["t"][1], L["t"][3]])
        want = ops.kl_normal(kl_t[0], kl_t[1], KL_PRIORS)
        h = ops.kl_normal_begin(kl_t[0], kl_t[1], KL_PRIORS, carry=True)
        with torch.no_grad():
            y2 = ops.linear_sampled(x, mu_w, rho_w, mu_b, rho_b, L["kw"], L["kb"], False, mode)
        assert h.launched and torch.equal(y2, y.detach())
        ops.mc_mean(y2, kl=h)
        kref, kbound = _kl_sums([L["post"][0], L["post"][2]], [L["post"][1], L["post"][3]], KL_PRIORS)
        P.assert_within(D(h.out), kref, kbound, "KL carried by bnn_linear_forward_sampled_kl")
        assert torch.equal(h.out, want)
    gy = torch.ones_like(y)
    grads = torch.autograd.grad(y, (x, mu_w, rho_w, mu_b, rho_b), gy)
    al = dict(mu=True, rho=True, x=True, x8=True, gy=True)
    spec, _, _ = linear_plan(K, K, N, mode, False, False, False, False, al, S=S)
    w32 = ops._sample_affine_philox_raw(L["t"][0], L["t"][1], L["kw"])
    wbf = ops._sample_affine_philox_raw(L["t"][0], L["t"][1], L["kw"], torch.bfloat16)
    op = dict(spec=spec, kl=None, x=x.detach().cpu(), g=gy.cpu(), y=None, mu_w=L["t"][0].cpu(), rho_w=L["t"][1].cpu(),
              mu_b=L["t"][2].cpu(), rho_b=L["t"][3].cpu(), eps_w=torch.from_numpy(L["eps_w"]), eps_b=torch.from_numpy(L["eps_b"]),
              w32=w32.cpu(), wbf=wbf.cpu())
    got = dict(zip(("gx", "g_mu_w", "g_rho_w", "g_mu_b", "g_rho_b"), (g.detach().cpu() for g in grads)))
    worst = bwdref.check(got, bwdref.layer_backward(op), "linear backward %s K %d N %d" % (mode, K, N))
    for k, v in worst.items():
        P.RATIOS["linear backward %s (%s)" % (k, spec["wgrad"])] = max(P.RATIOS.get("linear backward %s (%s)" % (k, spec["wgrad"]), 0.0), v)
    print("linear backward %s K %d N %d %s: worst err / bound %s" % (mode, K, N, spec, {k: round(v, 3) for k, v in worst.items()}))
    # relative to dsoftplus: the pruned and the collapsed elements' gradients of 1e-13 .. 1e-38 are checked, not rounded away
    ds = P.dsigma64(L["post"][1])
    small = ds < 1e-12
    assert small.any() and (np.abs(D(grads[2]))[small] <= 7.0 * S * ds[small] * (1.0 + 1e-3) + TINY).all()


@gpu
def test_posterior_input_gradient_redraw_is_the_forward_draw(dev):
    """bnn_linear_backward_input_sampled with gy = I returns the weights it re-draws: bit for bit the forward's draw in fp32
    compute (the forward on x = I returns them too), and inside the draw bound at every grid value."""
    from bayesianneuralnetworks_amd import ops
    from test_operand_alignment import linear_plan
    n, S = 24, 3
    L = _layer_operands(n, n, S, "f32", dev, bias=False)
    spec, _, _ = linear_plan(n, n, n, "f32", False, False, False, False, dict(mu=True, rho=True, x=True, x8=True, gy=True), S=S)
    assert spec["gx"] == "redraw_f32"
    x = torch.eye(n, device=dev).expand(S, n, n).contiguous().requires_grad_()
    y = ops.linear_sampled(x, L["t"][0], L["t"][1], None, None, L["kw"], None, False, "f32")
    (gx,) = torch.autograd.grad(y, x, torch.eye(n, device=dev).expand(S, n, n).contiguous())
    rho_at = np.broadcast_to(L["post"][1], L["ref_w"].shape)
    P.assert_within(D(gx), L["ref_w"], P.bound_draw(L["ref_w"], L["eps_w"], L["post"][1]), "bnn_linear_backward_input_sampled re-draw", rho_at)
    w32 = ops._sample_affine_philox_raw(L["t"][0], L["t"][1], L["kw"])
    assert torch.equal(gx, w32), "the re-drawn weights differ from bnn_sample_affine_philox's in %d elements" % int((gx != w32).sum())
    assert torch.equal(y.detach().transpose(1, 2), w32), "the forward's draw differs from bnn_sample_affine_philox's"


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(8, 8), (5, 13)], ids=["8x8", "5x13"])
@pytest.mark.parametrize("nd", [2, 3])
def test_posterior_conv_sampled_on_one_hot_images(dev, nd, shape, mode):
    """The sampled conv2d forward and bnn_conv3d_forward_drawn with a 1 x 1 (x 1) kernel on image b = the one-hot of channel b:
    y_s[b, o] = W_s[o, b] + b_s[o].  The conv3d backward (bnn_conv3d_backward_weight + bnn_sample_affine_bwd) on ones."""
    from bayesianneuralnetworks_amd import ops
    O, C = shape
    S = 3
    L = _layer_operands(O, C, S, mode, dev, shift=9)
    one = (1,) * nd
    mu_w, rho_w = (t.reshape((O, C) + one).clone().requires_grad_() for t in L["t"][:2])
    mu_b, rho_b = (t.clone().requires_grad_() for t in L["t"][2:])
    x = torch.eye(C, device=dev).reshape((C, C) + one).contiguous()
    zero = (0,) * nd
    if nd == 2:
        with torch.no_grad():
            y = ops.conv2d_sampled(x, mu_w, rho_w, mu_b, rho_b, L["kw"], L["kb"], True, one, zero, one, 1, mode)
    else:
        y = ops.conv3d_sampled(x, mu_w, rho_w, mu_b, rho_b, L["kw"], L["kb"], True, one, zero, one, 1, mode)
    ref, bound, rho_at = _one_weight_per_output(L, mode, S)
    P.assert_within(D(y).reshape(S, C, O), ref, bound, "conv%dd sampled %s %dx%d" % (nd, mode, O, C), rho_at)
    if nd == 3:
        grads = torch.autograd.grad(y, (rho_w, rho_b), torch.ones_like(y))
        # gw_s[o, c] = sum_b gy x = 1 (exact in both modes), gb_s[o] = C
        gref, gb = _g_rho_draw(L["eps_w"], L["post"][1], S)
        P.assert_within(D(grads[0]).reshape(O, C), gref, gb, "conv3d weight sums -> bnn_sample_affine_bwd, %s" % mode, L["post"][1])
        gref, gb = _g_rho_draw(C * L["eps_b"], L["post"][3], S)
        P.assert_within(D(grads[1]), gref, gb, "conv3d bias sums -> bnn_sample_affine_bwd, %s" % mode, L["post"][3])


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(8, 8), (5, 13)], ids=["8x8", "5x13"])
def test_posterior_flipout_conv3d_on_one_hot_images(dev, shape, mode):
    """FlipOutNormalConv3d's entries on the same images: y_s[b, o] = mean[o, b] + R_s[b, o] S_s[b, b] sigma[o, b], sigma the
    accurate operand of bnn_draw_multi kind 2; the weight-sum kernel k_conv3d_flip_wsum on ones gives
    g_scale[o, c] = (sum_s R_s[c, o] S_s[c, c]) dsoftplus(rho)."""
    from bayesianneuralnetworks_amd import ops
    O, C = shape
    S = 3
    rho, mu = P.tile(G, (O, C), shift=9), grid_mu((O, C), 12)
    m = put(mu.reshape(O, C, 1, 1, 1), dev).requires_grad_()
    r = put(rho.reshape(O, C, 1, 1, 1), dev).requires_grad_()
    signs = ops.flipout_signs(dkey(51, S), C, O + C, dev)                   # (S, B = C, O + C): R then S per example
    sg = D(signs)
    eps = np.einsum("sco,sc->soc", sg[:, :, :O], sg[:, np.arange(C), O + np.arange(C)])
    x = torch.eye(C, device=dev).reshape(C, C, 1, 1, 1).contiguous()
    y = ops.conv3d_flipout(x, m, r, signs, S, True, (1, 1, 1), (0, 0, 0), (1, 1, 1), mode)
    s64 = P.sigma64(rho)
    ref = (mu.astype(np.float64) + eps * s64).transpose(0, 2, 1)            # (S, b, o)
    b = P.bound_sigma(rho)
    if mode == "bf16":                                                     # both operands are rounded to bf16
        b = b + P.half_ulp_bf16(s64 + b) + P.half_ulp_bf16(mu)
    bound = np.broadcast_to(b.T, ref.shape) + 3.0 * U * np.abs(ref)
    P.assert_within(D(y).reshape(S, C, O), ref, bound, "bnn_conv3d_flipout_forward %s %dx%d" % (mode, O, C), np.broadcast_to(rho.T, ref.shape))
    (g_scale,) = torch.autograd.grad(y, r, torch.ones_like(y))
    gref, gb = _g_rho_draw(eps, rho, S)
    P.assert_within(D(g_scale).reshape(O, C), gref, gb, "k_conv3d_flip_wsum, %s" % mode, rho)


# ------------------------------------------------------------------------------------------------ MVN
def _mvn_case(O, shift):
    """K = 8: the grid on the diagonal, the grid clipped at -80 below it, +5 above it (never read)."""
    K = 8
    scale = np.full((O, K, K), 5.0, np.float32)
    diag = np.zeros((O, K, K), bool)
    d = P.tile(G, (O, K), shift=shift)
    low = P.tile(P.MVN_OFF_GRID, (O, K * (K - 1) // 2), shift=shift + 11)
    il = np.tril_indices(K, -1)
    for o in range(O):
        scale[o][np.arange(K), np.arange(K)] = d[o]
        scale[o][il] = low[o]
        diag[o][np.arange(K), np.arange(K)] = True
    tri = np.tril(np.ones((K, K), bool))[None]
    return K, grid_mu((O, K), O), scale, diag, np.broadcast_to(tri, scale.shape)


@gpu
@pytest.mark.parametrize("O,shift", [(1, 0), (5, 0), (5, 24)])
def test_posterior_mvn_entries(dev, O, shift):
    """ops.mvn_draw and its backward, ops.mvn_kl and its backward, ops.mvn_moments_prepare against mvn_l64 / mvn_v64 and their
    derivatives.  O = 5 with shifts 0 and 24 puts every grid value on a diagonal."""
    from bayesianneuralnetworks_amd import ops
    from test_mvn_device import _epoch_dev, mvn_uniforms
    K, mu, scale, diag, tri = _mvn_case(O, shift)
    S = 3
    L64 = np.where(tri, P.mvn_l64(scale, diag), 0.0)
    V64 = np.where(tri, P.mvn_v64(scale, diag), 0.0)
    bL = np.where(tri, P.bound_mvn_l(scale, diag), 0.0)
    m, sc = put(mu, dev), put(scale, dev)
    key = dkey(41, S)
    u = np.stack([mvn_uniforms(key, s, _epoch_dev(dev), O, K) for s in range(S)])                  # (S, O, K)
    ref = mu.astype(np.float64) + np.einsum("oij,soj->soi", L64, u)
    absum = np.abs(mu) + np.einsum("oij,soj->soi", L64, u)
    bound = np.einsum("oij,soj->soi", bL, u) + P.gamma(K + 2) * absum + TINY
    P.assert_within(D(ops.mvn_draw(m, sc, key)), ref, bound, "bnn_mvn_draw", np.broadcast_to(scale[:, np.arange(K), np.arange(K)], ref.shape))
    # backward on ones: g_scale[o, i, j] = (sum_s u_s[o, j]) dL / ds, dL / ds = dsoftplus(s) / (2 L)
    mg, sg = m.clone().requires_grad_(), sc.clone().requires_grad_()
    w, _ = ops.mvn_draw_layer(mg, sg, None, None, key, None)
    g_mu, g_sc = torch.autograd.grad(w, (mg, sg), torch.ones_like(w))
    assert bool((g_mu == S).all()) and bool((g_sc[torch.from_numpy(~tri).to(dev)] == 0).all())
    usum = np.broadcast_to(u.sum(0)[:, None, :], scale.shape)
    dL = P.dmvn_l64(scale, diag)
    gref = np.where(tri, usum * dL, 0.0)
    rel = P.rel_dsigma(scale) + P.rel_mvn_l(scale, diag) + 3.0 * U
    gb = np.where(tri, (P.gamma(S + 1) + rel) * usum * dL, 0.0) + TINY
    P.assert_within(D(g_sc), gref, gb, "bnn_mvn_draw_backward", scale)
    # KL against an isotropic prior: mean over rows of 0.5 / s0^2 (sum V^2 + |mu - m0|^2) - sum ln V_ii + K (ln s0 - 1/2)
    m0, s0 = 0.25, 0.5
    mg, sg = m.clone().requires_grad_(), sc.clone().requires_grad_()
    kl = ops.mvn_kl([mg], [sg], [(m0, s0)])
    Vd = V64[:, np.arange(K), np.arange(K)]
    dm2 = (mu.astype(np.float64) - m0) ** 2
    ref_kl = (0.5 / s0 ** 2 * ((V64 ** 2).sum((1, 2)) + dm2.sum(1)) - np.log(Vd).sum(1) + K * (np.log(s0) - 0.5)).mean()
    bV = np.where(tri, P.bound_mvn_v(scale, diag), 0.0)
    b_ln = (P.rel_sigma(scale, "mvn_v") + 3.0 * U * np.abs(np.log(np.where(diag, V64, 1.0))))[diag].reshape(O, K)
    b_kl = (0.5 / s0 ** 2 * ((2.0 * V64 * bV).sum((1, 2)) + P.gamma(K + 2) * (V64 ** 2).sum((1, 2)) + 4.0 * U * dm2.sum(1))
            + b_ln.sum(1) + 4.0 * U * (np.abs(np.log(Vd)).sum(1) + K)).mean() + U * abs(ref_kl)
    P.assert_within(D(kl), np.array([ref_kl]), np.array([b_kl]), "bnn_mvn_kl")
    g_mu, g_sc = torch.autograd.grad(kl.sum(), (mg, sg))
    dv = V64 / s0 ** 2 - np.where(diag, 1.0 / np.where(diag, V64, 1.0), 0.0)
    gref = np.where(tri, dv * P.dmvn_v64(scale, diag), 0.0) / O
    mag = (V64 / s0 ** 2 + np.where(diag, 1.0 / np.where(diag, V64, 1.0), 0.0)) * P.dmvn_v64(scale, diag) / O
    relv = np.where(diag, P.rel_sigma(scale, "mvn_v"), P.rel_sigma(scale, "mvn_v_off"))
    # (dsoftplus below 2^-126 is flushed in fp32, and 1 / V = 1e10 on a collapsed diagonal scales that back up: TINY times the factor)
    gb = np.where(tri, (relv + P.rel_dsigma(scale) + 6.0 * U) * mag + TINY * (mag / P.dmvn_v64(scale, diag)), 0.0) + TINY
    P.assert_within(D(g_sc), gref, gb, "bnn_mvn_kl_backward", scale)
    # the moment head's operands: E_w = mu + 1/2 sum_j L, G_w = E_w^2 + 1/12 sum_j L^2, weight rows (O, K) with (O, K, K) scales
    E_w, G_w, _, _ = ops.mvn_moments_prepare(m, sc, None, None)
    s1, s2 = L64.sum(2), (L64 ** 2).sum(2)
    E64 = mu.astype(np.float64) + 0.5 * s1
    bE = 0.5 * bL.sum(2) + P.gamma(K + 2) * (np.abs(mu) + 0.5 * s1) + TINY
    P.assert_within(D(E_w), E64, bE, "bnn_mvn_moments_prepare E_w")
    G64_ = E64 ** 2 + s2 / 12.0
    bG = 2.0 * np.abs(E64) * bE + bE ** 2 + ((2.0 * L64 * bL).sum(2) + P.gamma(K + 3) * s2) / 12.0 + 3.0 * U * G64_ + TINY
    P.assert_within(D(G_w), G64_, bG, "bnn_mvn_moments_prepare G_w")


# ------------------------------------------------------------------------------------------------ pruned networks, end to end
FAMILIES = ["normal_f32", "normal_bf16", "lrt", "flipout", "conv3d", "moments_dense", "moments_conv"]


def _build(family):
    from bayesianneuralnetworks_amd import nn as bnn_nn
    if family == "moments_dense":
        from test_moment_backward import Net
        return Net([16, 40, 5], False, samples=3)
    if family == "conv3d":
        mods = [bnn_nn.NormalConv3d(2, 8, 3, padding=1), torch.nn.ReLU(), bnn_nn.NormalConv3d(8, 4, 1)]
    elif family == "moments_conv":
        mods = [bnn_nn.NormalConv2d(1, 4, 3), torch.nn.ELU(), bnn_nn.NormalConv2d(4, 6, 3, stride=2, padding=1)]
    else:
        layer = {"normal_f32": bnn_nn.NormalLinear, "normal_bf16": bnn_nn.NormalLinear, "lrt": bnn_nn.LocalReparamLinear,
                 "flipout": bnn_nn.FlipoutNormalLinear}[family]
        mods = [layer(16, 40), torch.nn.ReLU(), layer(40, 5)]

    class Net(bnn_nn.BayesianNetworkModule):
        def __init__(self):
            super().__init__(16, 5, samples=3)
            self.layers = torch.nn.Sequential(*mods)
            if family == "moments_conv":
                bnn_nn.moment_activations(self)

        def _forward(self, x):
            return self.layers(x)

    return Net()


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_posterior_pruned_network_end_to_end(dev, family, monkeypatch):
    """A two-layer net of each family after PruneNormal()(net, 0.5): (a) the pruned entries are exactly (0, -30) and the others
    untouched; (b) the keyed forward is the float64 forward on the same eps within the family's own bound (the suite's 1e-5 of
    the output scale in fp32; tests/golden/bf16ref's chain bound on the device's bf16 draws in bf16; test_moment_backward's and
    test_moment_conv_backward's E2E_TOL for the dense and the conv moment pass); (c) KLDivergence is float64 torch's within 1e-6 relative; (d) the gradients of the loss and of
    the KL with respect to every mean and scale are float64 autograd's -- the error of a scale's gradient is measured relative to
    dsigma64 at each element, so a pruned element's likelihood gradient of order 1e-13 is checked, not rounded away.  (d) of the
    bf16 family's likelihood is test_posterior_pruned_backward_layer_by_layer's, under the bf16 kernels' own derived bound."""
    import bayesianneuralnetworks_amd as bnn
    from bayesianneuralnetworks_amd import ops
    from bayesianneuralnetworks_amd.nn import KLDivergence
    from bayesianneuralnetworks_amd.prune import PruneNormal
    from klref import kl_grad64
    from test_lrt_device import scaled_bound
    bf = family == "normal_bf16"
    bnn.set_compute("bf16" if bf else "f32")
    if family == "moments_conv":
        from bayesianneuralnetworks_amd.nn import _settings
        monkeypatch.setattr(_settings, "_conv_moment_training", True)          # nn.conv_moment_training(), for this test
    torch.manual_seed(50)
    net = _build(family).to(dev)
    net.mc_batched = True
    S = 3
    layers = P.bayes_layers(net)
    posts = [q for m in layers for q in ((m.weight, m.bias) if m.bias is not None else (m.weight,))]
    before = [(q.mean.detach().clone(), q.scale.detach().clone()) for q in posts]
    PruneNormal()(net, 0.5)
    for q, (m0, s0) in zip(posts, before):                                                    # (a)
        mask = q.scale.detach() == -30
        assert int(mask.sum()) == int(0.5 * q.scale.numel()) and bool((q.mean.detach()[mask] == 0).all())
        assert torch.equal(q.mean.detach()[~mask], m0[~mask]) and torch.equal(q.scale.detach()[~mask], s0[~mask])
    gen = torch.Generator().manual_seed(51)
    x = torch.randn({"conv3d": (3, 2, 4, 4, 4), "moments_conv": (3, 1, 10, 10)}.get(family, (7, 16)), generator=gen)
    bnn.manual_seed(52)
    moments = family.startswith("moments")
    if moments:
        mom = net.forward_moments(x.to(dev))
        got = torch.stack([mom.mean, mom.var])
    else:
        got = torch.stack(net(x.to(dev)))
    c = torch.randn(got.shape[1:], generator=gen).double()
    params = [t for q in posts for t in (q.mean, q.scale)]
    p64 = []
    for m in layers:
        ts = [m.weight.mean, m.weight.scale] + ([m.bias.mean, m.bias.scale] if m.bias is not None else [None, None])
        p64.append([None if t is None else t.detach().double().cpu().requires_grad_() for t in ts])
    flat64 = [t for q in p64 for t in q if t is not None]
    x64 = x.double()
    if bf:
        from bf16ref import bf16_chain_ref64, rne_bf16
        for s in range(S):                                                                    # (b), bf16
            chain = []
            for m in layers:
                w = ops._sample_affine_philox_raw(m.weight.mean.detach(), m.weight.scale.detach(), m.weight._key, torch.bfloat16)[s]
                b = ops._sample_affine_philox_raw(m.bias.mean.detach(), m.bias.scale.detach(), m.bias._key)[s]
                chain.append((w.double().cpu(), b.double().cpu()))
            r = bf16_chain_ref64(rne_bf16(x64), chain)
            P.assert_within(D(got[s]), r["out"].numpy(), r["bound"].numpy() + TINY, "pruned %s forward" % family)
    else:
        if family == "moments_conv":
            # the CPU twin of the net in float64 is the family's reference (test_moment_conv_backward): the same recursion
            # under torch autograd, on the pruned parameters
            from test_moment_conv_backward import E2E_TOL as CONV_TOL
            twin = _build(family)
            twin.load_state_dict(net.state_dict())
            twin = twin.double()
            flat64 = [t for m in P.bayes_layers(twin) for q in (m.weight, m.bias) for t in (q.mean, q.scale)]
            want, tol = twin.forward_moments(x64), CONV_TOL[("b", "f32")]
        else:
            want, tol = P.ref_forward(family, net, x64, p64, S, dev), 1e-5
        if family == "moments_dense":
            from test_moment_backward import E2E_TOL
            tol = E2E_TOL["f32"]
        if moments:
            want = torch.stack([want.mean, want.var])
        for i in range(got.shape[0]):                                                         # (b)
            P.assert_within(D(got[i]), want[i].detach().numpy(), scaled_bound(want[i].detach(), tol).numpy(), "pruned %s forward" % family)
    kl = KLDivergence()(net)                                                                  # (c)
    T = len(posts)
    kl64 = sum(torch.distributions.kl_divergence(torch.distributions.Normal(mu, P.sg_torch(rho)), torch.distributions.Normal(*P.PRIOR)).mean()
               for mu, rho in zip(flat64[0::2], flat64[1::2])) / T
    P.assert_within(D(kl), kl64.detach().numpy(), 1e-6 * abs(float(kl64.detach())), "pruned %s KLDivergence" % family)
    g_kl = torch.autograd.grad(kl, params)                                                    # (d), the KL's part
    for i, (mu, rho) in enumerate(zip(flat64[0::2], flat64[1::2])):
        rm, rr, bm, br = kl_grad64(mu.detach().numpy(), rho.detach().numpy(), P.PRIOR, T, 1.0, 1.0)
        P.assert_within(D(g_kl[2 * i]), rm, bm + TINY, "pruned %s KL gradient, mean" % family)
        P.assert_within(D(g_kl[2 * i + 1]), rr, br + TINY, "pruned %s KL gradient, scale" % family, rho.detach().numpy())
    if bf:
        return
    n = got.shape[0]
    g_dev = torch.autograd.grad((got.double() * c.to(dev)).sum() / n, params)                 # (d), the likelihood's part
    g_ref = torch.autograd.grad((want * c).sum() / n, flat64)
    for i, (mu, rho) in enumerate(zip(flat64[0::2], flat64[1::2])):
        gm, gr = g_ref[2 * i].numpy(), g_ref[2 * i + 1].numpy()
        P.assert_within(D(g_dev[2 * i]), gm, scaled_bound(g_ref[2 * i], tol).numpy(), "pruned %s loss gradient, mean" % family)
        rho_ = rho.detach().numpy()
        ds = P.dsigma64(rho_)
        gs = gr / ds                                                                          # d loss / d sigma
        rel = P.rel_sigma(rho_) + P.rel_dsigma(rho_) + U
        b = ds * (tol * max(1.0, float(np.sqrt((gs ** 2).mean()))) + (tol + rel) * np.abs(gs)) + TINY
        P.assert_within(D(g_dev[2 * i + 1]), gr, b, "pruned %s loss gradient, scale" % family, rho_)
        pruned = rho_ == -30
        assert pruned.any() and np.abs(gr[pruned]).max() < 1e-9 and b[pruned].max() < 1e-15


@gpu
@pytest.mark.parametrize("kl_c", [0.0, None], ids=["loss", "loss_and_kl"])
@pytest.mark.parametrize("dims", [(16, 40, 5), (16, 40, 24)], ids=["narrow_head", "wide_head"])
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_posterior_pruned_backward_layer_by_layer(dev, mode, dims, kl_c):
    """The backward of a real training step through a PRUNED two-layer NormalLinear net (fused ReLU and, in bf16, a bf16 hidden
    activation and bf16 gx; the KL gradient fused into the weight-gradient launches), every layer's g_mu, g_rho and gx held to
    tests/golden/bwdref.layer_backward on the operands the device consumed -- test_train_step's capture, which runs at the init
    rho only, here with half of every tensor at (0, -30).  The head of 5 takes the narrow kernel and its re-draw, the head of 24
    the general weight-gradient kernel and the fused re-draw input gradient.  Without the KL term the bound of a pruned
    element's g_rho is itself of the order of dsigma64(-30) = 9.4e-14 times the sum of |gy x eps|: a kernel that lost dsoftplus
    there, or took it at +30, is 1e13 bounds out."""
    import bwdref
    import test_train_step as tts
    from bayesianneuralnetworks_amd.prune import PruneNormal
    B, S = 7, 3
    plan = tts.finish_plan(tts.layer_plan(dims, S, mode, False), B)
    cfg = dict(dims=dims, B=B, S=S, mode=mode, x_bf16=False, names=[p["names"] for p in plan])
    ops_, gots, _, plan = tts.device_step(cfg, 3, prepare=lambda net: PruneNormal()(net, 0.5), kl_c=tts.KL_C if kl_c is None else kl_c)
    for i, (op, got) in enumerate(zip(ops_, gots)):
        for name in ("rho_w", "rho_b"):
            r = op[name]
            assert int((r == -30).sum()) == int(0.5 * r.numel()), (i, name)
        ref = bwdref.layer_backward(op)
        assert set(ref) == set(got)
        what = "pruned %s %s layer %d (%s)" % (mode, "x".join(map(str, dims)), i, ", ".join(plan[i]["names"]))
        worst = bwdref.check(got, ref, what)
        print("%s: worst err / bound %s" % (what, {k: round(v, 3) for k, v in worst.items()}))
        for k, v in worst.items():
            site = "pruned %s step %s" % (mode, k)
            P.RATIOS[site] = max(P.RATIOS.get(site, 0.0), v)
        if kl_c == 0.0:
            for name, g in (("rho_w", "g_rho_w"), ("rho_b", "g_rho_b")):
                pruned = op[name].reshape(ref[g][0].shape) == -30
                rb, bb = ref[g][0][pruned].abs(), ref[g][1][pruned]
                assert float(rb.max()) < 1e-9 and float(bb.max()) < 1e-15, (what, g, float(rb.max()), float(bb.max()))
