"""The MC-batched path across sample counts: every code path the reductions and the backward pick by S.

(a) bnn_mc_sum / bnn_mc_sum_kl / HeadPartials against a NumPy fp32 model of their summation order, bit for bit, at addend
    counts on both sides of the sequential (<= 32), register-split (<= 256) and chunked (> 256) bodies;
(b) bnn_mc_uncertainty with thousands of parts / samples (widened parametrization in test_predictive_uncertainty.py);
(c) predictive_mean / predictive_uncertainty of the 784-1200-1200-10 net with its head fused, S = 1 .. 300, against float64 on
    the layers' recorded keys -- where parts x S passes 256, and across dense_pick_tile's small-S tiles;
(d) the backward across its switches (narrow head at the workspace boundary, the weight gradient's sample split, the shared
    input's sum over S) against float64 autograd."""
import ctypes

import numpy as np
import pytest
import seeded
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd._rng import DrawKey
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, NormalLinear, fuse_activations
from conftest import assert_close_scaled

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


# ------------------------------------------------------------------------------------------------ the summation order
def model_sum(Y, scale):
    """The order of bnn_mc_sum in fp32: Y (A, n) addends in addend order -> scale * sum.  Up to 32 addends: one sequential sum
    from +0; above: four quarters of ceil(A / 4) addends, each summed sequentially from +0, added left to right."""
    Y = np.asarray(Y, dtype=np.float32)
    A, n = Y.shape
    if A <= 32:
        quarters = [(0, A)]
    else:
        per = -(-A // 4)
        quarters = [(min(w * per, A), min((w + 1) * per, A)) for w in range(4)]
    total = None
    for s0, s1 in quarters:
        a = np.zeros(n, dtype=np.float32)
        for v in range(s0, s1):
            a = a + Y[v]
        total = a if total is None else total + a
    return total * np.float32(scale)


def test_model_order_on_the_cpu():
    """The model is a different order from numpy's pairwise sum -- and exactly the sequential one at 32 addends or fewer."""
    rng = np.random.RandomState(0)
    Y = (rng.randn(300, 5) * np.exp(rng.randn(300, 1) * 4)).astype(np.float32)
    seq = np.zeros(5, np.float32)
    for v in range(32):
        seq = seq + Y[v]
    assert np.array_equal(model_sum(Y[:32], 1.0), seq)
    per = 75
    q = [np.zeros(5, np.float32) for _ in range(4)]
    for w in range(4):
        for v in range(w * per, (w + 1) * per):
            q[w] = q[w] + Y[v]
    assert np.array_equal(model_sum(Y, 0.5), (((q[0] + q[1]) + q[2]) + q[3]) * np.float32(0.5))
    assert not np.array_equal(model_sum(Y, 1.0), Y.sum(0))


ADDENDS = [1, 2, 8, 9, 31, 32, 33, 63, 64, 65, 128, 255, 256, 257, 300, 1000, 4096]
OUTPUTS = [1, 63, 64, 65, 3001]


def _addends(A, n, stride, seed):
    """(A, stride) fp32: mixed magnitudes and signs (rounding visible in every order), junk in the gap past n."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(A, stride, generator=g) * torch.exp2(torch.randint(-6, 7, (A, 1), generator=g).float())
    y[:, n:] = float("nan")                                          # never read: a read would poison the sum
    return y


def _mc_sum(lib, y, stride, A, n, scale, out, acc):
    return lib.bnn_mc_sum(_lib.ptr(y), stride, A, n, scale, _lib.ptr(out), acc, None, 0, _lib.stream_ptr(y.device))


def _f32_ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32)))


@gpu
@pytest.mark.parametrize("n", OUTPUTS)
@pytest.mark.parametrize("A", ADDENDS)
def test_mc_sum_is_the_model(A, n):
    lib = _lib.load()
    stride = n + 37
    scale = np.float32(0.3)
    yc = _addends(A, n, stride, A * 1000 + n)
    y = yc.to(DEV)
    Y = yc[:, :n].numpy()
    want = model_sum(Y, scale)
    out = torch.full((n,), 7.0, device=DEV)
    assert _mc_sum(lib, y, stride, A, n, float(scale), out, 0) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (A, n, int((got != want).sum()))
    # bitwise equal across two calls
    out2 = torch.empty(n, device=DEV)
    assert _mc_sum(lib, y, stride, A, n, float(scale), out2, 0) == 0
    assert torch.equal(out, out2)
    # the recursive-summation bound of the float64 sum
    exact = Y.astype(np.float64).sum(0) * np.float64(scale)
    bound = (A + 1) * 2.0 ** -24 * np.float64(scale) * np.abs(Y).astype(np.float64).sum(0)
    assert (np.abs(got - exact) <= bound).all(), (A, n, float((np.abs(got - exact) - bound).max()))
    # accumulate: out + t, the product t rounded in the model; an FMA may skip that rounding (<= 1 ulp + half an ulp of t)
    base = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 4
    acc = base.to(DEV)
    assert _mc_sum(lib, y, stride, A, n, float(scale), acc, 1) == 0
    t = want
    want_acc = base.numpy() + t
    err = np.abs(acc.cpu().numpy().astype(np.float64) - want_acc.astype(np.float64))
    assert (err <= _f32_ulp(want_acc) + 0.5 * _f32_ulp(t)).all(), (A, n, float(err.max()))
    torch.cuda.synchronize()


def _kl_params(seed):
    g = torch.Generator().manual_seed(seed)
    mus = [(torch.randn(37, 11, generator=g) * 0.1).to(DEV), (torch.randn(5000, generator=g) * 0.1).to(DEV)]
    rhos = [(torch.randn(37, 11, generator=g) * 0.2 - 3.0).to(DEV), (torch.randn(5000, generator=g) * 0.2 - 3.0).to(DEV)]
    return mus, rhos, [(0.0, 0.1), (0.1, 1.0)]


@gpu
@pytest.mark.parametrize("n", [1, 65, 3001])
@pytest.mark.parametrize("A", ADDENDS)
def test_mc_sum_kl_gives_the_bits_of_mc_sum_and_of_kl_normal(A, n):
    """The step-tail kernel: its reduction is bnn_mc_sum's, bit for bit; its KL is kl_normal's, bit for bit."""
    lib = _lib.load()
    stride = n + 5
    yc = _addends(A, n, stride, A * 7 + n)
    y = yc.to(DEV)
    plain = torch.empty(n, device=DEV)
    assert _mc_sum(lib, y, stride, A, n, 0.125, plain, 0) == 0
    mus, rhos, priors = _kl_params(A)
    h = ops.kl_normal_begin(mus, rhos, priors, n_batches=3.0)
    out = torch.empty(n, device=DEV)
    assert lib.bnn_mc_sum_kl(_lib.ptr(y), stride, A, n, 0.125, _lib.ptr(out), 0, None, 0, h.arr, h.T, h.n_batches,
                             _lib.ptr(h.out), _lib.ptr(h.ws), _lib.stream_ptr(DEV)) == 0
    assert torch.equal(out, plain)
    assert np.array_equal(out.cpu().numpy(), model_sum(yc[:, :n].numpy(), 0.125))
    assert torch.equal(h.out, ops.kl_normal(mus, rhos, priors, n_batches=3.0))


@gpu
@pytest.mark.parametrize("parts,S", [(2, 16), (3, 11), (33, 1), (16, 16), (16, 17), (40, 30), (257, 2), (300, 1)])
def test_head_partials_are_the_model(parts, S):
    """HeadPartials.logits() sums over `parts` addends, mc_mean(HeadPartials) over parts * S (addend v = part * S + s, scale
    1 / S): both the model's bits, on both sides of 32 and of 256."""
    M, Nh = 37, 10
    g = torch.Generator().manual_seed(parts * 31 + S)
    p = torch.randn(parts, S, M, Nh, generator=g) * torch.exp2(torch.randint(-4, 5, (parts, S, 1, 1), generator=g).float())
    hp = ops.HeadPartials(p.to(DEV))
    lg = hp.logits().cpu().numpy()
    assert np.array_equal(lg.reshape(-1), model_sum(p.numpy().reshape(parts, -1), 1.0))
    pm = ops.mc_mean(hp).cpu().numpy()
    want = model_sum(p.numpy().reshape(parts * S, M * Nh), np.float32(1.0 / S))
    assert np.array_equal(pm.reshape(-1), want), (parts, S)
    assert torch.equal(ops.mc_mean(hp), ops.mc_mean(hp))


@gpu
def test_uncertainty_kernel_at_4096_samples_against_float64():
    """bnn_mc_uncertainty over 4096 plain samples and over 300 parts x 16 samples, against float64."""
    from test_predictive_uncertainty import check_against_ref
    g = torch.Generator().manual_seed(4096)
    y = torch.randn(4096, 65, 10, generator=g) * 3.0
    u = ops.mc_uncertainty(y.to(DEV), "logits")
    check_against_ref(u, y.numpy(), "logits", "S = 4096")
    p = torch.randn(300, 16, 65, 10, generator=g) * 0.2
    hp = ops.HeadPartials(p.to(DEV))
    u = ops.mc_uncertainty(hp, "logits")
    check_against_ref(u, p.double().sum(0).numpy(), "logits", "300 parts")


# ------------------------------------------------------------------------------------------------ module level
class MLP(BayesianNetworkModule):
    def __init__(self, dims, samples):
        super().__init__(dims[0], dims[-1], samples)
        mods = []
        for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
            mods.append(NormalLinear(a, b))
            if i < len(dims) - 2:
                mods.append(torch.nn.ReLU())
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


def _net(seed, base=1000):
    torch.manual_seed(seed)
    net = MLP([784, 1200, 1200, 10], 4).to(DEV)
    seeded.pin_streams(net, base)
    net.mc_batched = True
    fuse_activations(net, bf16_activations=True, fuse_head=True)
    return net


def _one_sample(key, s):
    return DrawKey(key.seed, key.stream, key.sample0 + s, 1, key.epoch_host, key.epoch_dev_delta, key.gen)


def _draw64(p, s, bf16):
    """Sample s of a Normal parameter re-created from its recorded key in float64 (mu + (softplus(rho) + 1e-10) eps), rounded
    to bf16 as the bf16 mode's draw is."""
    eps = ops.eps_philox(tuple(p.mean.shape), _one_sample(p.draw_key, s), DEV)[0].double()
    w = p.mean.detach().double() + (F.softplus(p.scale.detach().double()) + 1e-10) * eps
    return w.float().bfloat16().double() if bf16 else w


def _net_ref64(net, x, S, bf16):
    """float64 logits (S, B, 10) of the recorded draws, sample by sample on the device; operands rounded as the mode rounds them
    (bf16: input, drawn weights and the hidden activations in bf16, biases fp32).  Also max |head weight|, max |hidden 2|."""
    lins = [net.layers[0], net.layers[2], net.layers[4]]
    rb = (lambda t: t.float().bfloat16().double()) if bf16 else (lambda t: t)
    outs, wmax, hmax = [], 0.0, 0.0
    for s in range(S):
        h = rb(x.double())
        for li, lin in enumerate(lins):
            w = _draw64(lin.weight, s, bf16)
            b = _draw64(lin.bias, s, False)
            if bf16:
                b = b.float().double()
            h = h @ w.t() + b
            if li < 2:
                h = rb(h.clamp_min(0))
            if li == 1:
                hmax = max(hmax, float(h.abs().max()))
            if li == 2:
                wmax = max(wmax, float(w.abs().max()))
        outs.append(h.cpu())
    return torch.stack(outs), wmax, hmax


def _device_chain_ref64(net, x, S, h1):
    """The bf16 mode's chain checked layer by layer in float64 on the device's own operands (bf16ref): the weights drawn again on
    the layers' recorded keys (the draw kernels are checked against their twins elsewhere), the hidden layer 1 the net stored (h1, captured) and the hidden layer 2
    of a plain dense launch on it.  Each stored hidden value must be a bf16 rounding of a value within the accumulation bound of
    its exact float64 value.  -> (want (S, M, 10) float64 logits on the stored hidden values, acc (S, M, 10) their accumulation
    bound, a (S, M, 10) the head's sum |h| |w| + |b|)."""
    from bf16ref import chain_layer, relu, rounding_interval
    lins = [net.layers[0], net.layers[2], net.layers[4]]
    pre = ops.draw_layers([(l.weight.mean, l.weight.scale, l.bias.mean, l.bias.scale, l.weight.draw_key, l.bias.draw_key)
                           for l in lins], S)
    M = x.shape[0]
    assert h1.dtype == torch.bfloat16 and h1.numel() == S * M * 1200, (h1.dtype, tuple(h1.shape))
    h1 = h1.reshape(S, M, 1200).contiguous()                # whatever the captured view's pitch: dense rows, samples M * K apart
    h2 = ops._dense_raw(h1, M * 1200, M, pre[1], 1200, True, torch.bfloat16)
    xb = x.bfloat16().double().cpu()
    want, acc, a_head = [], [], []
    for s in range(S):
        ws = []
        for li, lin in enumerate(lins):
            K = lin.weight.mean.shape[1]
            w = pre[li].w[s, :, :K].double().cpu()
            b = pre[li].b[s].double().cpu()
            ws.append((w, b))
        h = xb
        for li, dev_h in enumerate((h1[s], h2[s])):
            t, bnd, _, _ = chain_layer(h, None, *ws[li])
            lo, hi = rounding_interval(t, bnd, relu)
            h = dev_h.double().cpu()
            out = (h < lo) | (h > hi)
            assert not bool(out.any()), ("stored hidden %d outside its rounding interval" % (li + 1), s, int(out.sum()))
        t, bnd, _, a = chain_layer(h, None, *ws[2])
        want.append(t); acc.append(bnd); a_head.append(a)
    return torch.stack(want), torch.stack(acc), torch.stack(a_head)


def _softmax_unc_tol(C, dz):
    """How far the uncertainty of logits dz apart (max abs) may move: |d mean| <= e^(2 dz) - 1; entropies <= 2 dz (1 + C / e)."""
    return float(np.expm1(2 * dz)) + 1e-6, 1e-5 * max(1.0, float(np.log(C))) + 2 * dz * (1 + C / np.e)


def _check_module(net, x, S, seed, bf16):
    lib = _lib.load()
    M = x.shape[0]
    parts = lib.bnn_dense_head_parts(M, 1200, S)
    assert parts >= 1
    with torch.no_grad():
        bnn.manual_seed(seed)
        box = []
        hnd = net.layers[2].register_forward_pre_hook(lambda m, a: box.append(a[0]))
        try:
            pm = net.predictive_mean(x, S)
        finally:
            hnd.remove()
        keys = (net.layers[0].weight.draw_key, net.layers[4].weight.draw_key)
        assert keys[0].nsamples == S and keys[1].nsamples == S
        if bf16:
            # derived bounds (bf16ref) on the device's own operands: the logits within their accumulation bound; the mean within
            # the mean of those plus the reduction's own rounding (parts x S addends, the 1 / S scale)
            assert len(box) == 1
            want, acc, a_head = _device_chain_ref64(net, x, S, box[0])
            wm = want.mean(0)
            from bf16ref import gamma
            bound_pm = acc.mean(0) + gamma(parts * S + 2) * (a_head + acc).mean(0)
            err = (pm.double().cpu() - wm).abs()
            assert bool((err <= bound_pm).all()), ("predictive_mean S = %d (%d parts)" % (S, parts), float((err / bound_pm).max()),
                                                   int((err > bound_pm).sum()))
        else:
            want, _, _ = _net_ref64(net, x, S, False)
            wm = want.mean(0)
            assert_close_scaled(pm.double().cpu().numpy(), wm.numpy(), 1e-5, "predictive_mean S = %d (%d parts)" % (S, parts))
        # the same draws through the uncertainty launch; each sample's logits against float64
        bnn.manual_seed(seed)
        hp = net._forward_batched_stacked(x, S, 0, _lazy_head=True)
        assert isinstance(hp, ops.HeadPartials) and hp.p.shape == (parts, S, M, 10)
        lg = hp.logits()
        if bf16:
            err = (lg.double().cpu() - want).abs()
            assert bool((err <= acc).all()), ("logits S = %d" % S, float((err / acc).max()), int((err > acc).sum()))
        else:
            assert_close_scaled(lg.double().cpu().numpy(), want.numpy(), 1e-5, "logits S = %d" % S)
        dz = float((lg.double().cpu() - want).abs().max())
        bnn.manual_seed(seed)
        u = net.predictive_uncertainty(x, S, inputs="logits")
        for a, b in zip(u, ops.mc_uncertainty(lg, "logits")):
            assert torch.equal(a, b)
        ref = ops.uncertainty_f64(want, "logits")
        tm, te = _softmax_unc_tol(10, dz)
        assert float((u.mean.double().cpu() - ref.mean.double()).abs().max()) <= tm
        for name in ("total", "aleatoric", "epistemic"):
            err = float((getattr(u, name).double().cpu() - getattr(ref, name).double()).abs().max())
            assert err <= te, (name, S, err, te)
    return parts


@gpu
@pytest.mark.parametrize("S", [1, 10, 16, 17, 20, 100, 300])
def test_fused_head_mlp_across_sample_counts_vs_float64(S):
    net = _net(5)
    x = torch.randn(64, 784, generator=torch.Generator().manual_seed(S)).to(DEV)
    bnn.set_compute("bf16")
    try:
        parts = _check_module(net, x, S, 100 + S, True)
    finally:
        bnn.set_compute("f32")
    if S in (17, 20):
        assert parts * S > 256, (parts, S)


SWEEP_BASES = [1, 411, 2000, 9001, 30011, 65000]          # pinned stream bases: six different draws of every posterior


@gpu
@pytest.mark.parametrize("S", [1, 8, 17, 300])
@pytest.mark.parametrize("base", SWEEP_BASES)
def test_fused_head_mlp_over_pinned_draws(base, S):
    """The S-sweep's check on six pinned draws each: a kernel must pass on many draws, not on one."""
    net = _net(5, base)
    x = torch.randn(64, 784, generator=torch.Generator().manual_seed(S)).to(DEV)
    bnn.set_compute("bf16")
    try:
        _check_module(net, x, S, 100 + S, True)
    finally:
        bnn.set_compute("f32")


def _predictive_mean_s1():
    """test_fused_head_mlp_across_sample_counts_vs_float64[1]'s predictive mean (its net, input, seed and pinned streams)."""
    net = _net(5)
    x = torch.randn(64, 784, generator=torch.Generator().manual_seed(1)).to(DEV)
    bnn.set_compute("bf16")
    try:
        with torch.no_grad():
            bnn.manual_seed(101)
            return net.predictive_mean(x, 1).cpu()
    finally:
        bnn.set_compute("f32")


@gpu
def test_fused_head_draws_do_not_depend_on_what_ran_before(tmp_path):
    """The S = 1 fused-head predictive mean in a fresh process, and here after 1000 unrelated posterior tensors took stream ids:
    bit for bit the same (pinned streams: a test's draws are its own)."""
    import os
    import subprocess
    import sys
    from bayesianneuralnetworks_amd.nn.core import WeightNormal
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "pm.pt")
    code = ("import sys, torch; sys.path[:0] = [%r, %r, %r]; import test_mc_sample_counts as t; "
            "torch.save(t._predictive_mean_s1(), %r)" % (root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden"), out))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    fresh = torch.load(out)
    unrelated = [WeightNormal(1) for _ in range(1000)]
    assert unrelated[-1]._stream - unrelated[0]._stream == 999
    here = _predictive_mean_s1()
    assert here.dtype == fresh.dtype and torch.equal(here.view(torch.int32), fresh.view(torch.int32))


@gpu
def test_f32_mode_predictive_mean_at_300_samples_vs_float64():
    net = _net(6)
    x = torch.randn(64, 784, generator=torch.Generator().manual_seed(3)).to(DEV)
    bnn.set_compute("f32")
    S = 300
    with torch.no_grad():
        bnn.manual_seed(12)
        y = net._forward_batched_stacked(x, S, 0, _lazy_head=True)
        nadd = y.p.shape[0] * S if isinstance(y, ops.HeadPartials) else S
        assert nadd > 256
        bnn.manual_seed(12)
        pm = net.predictive_mean(x, S)
        want, _, _ = _net_ref64(net, x, S, False)
    assert_close_scaled(pm.double().cpu().numpy(), want.mean(0).numpy(), 1e-5, "f32 predictive_mean S = 300")


def _pick_tile_1200(M, S):
    """dense_pick_tile (csrc/bnn_dense.hip) for the 1200-wide hidden layer: 1 (128 x 160), 3 (64 x 160) or 4 (32 x 160)."""
    cols, tile = 8, 1
    if -(-M // 128) * cols * S < 128 and M > 64:
        tile = 3
        if -(-M // 64) * cols * S < 128 and M > 32:
            tile = 4
    return tile


@gpu
@pytest.mark.parametrize("S", [2, 5, 20])
def test_fused_head_across_the_small_sample_tiles(S):
    """M = 200: tile 4 at S = 2, tile 3 at S = 5, tile 1 at S = 20 (parts x S > 256) -- each against float64."""
    M = 200
    assert _pick_tile_1200(M, S) == {2: 4, 5: 3, 20: 1}[S]
    net = _net(7)
    x = torch.randn(M, 784, generator=torch.Generator().manual_seed(M + S)).to(DEV)
    bnn.set_compute("bf16")
    try:
        _check_module(net, x, S, 200 + S, True)
    finally:
        bnn.set_compute("f32")


# ------------------------------------------------------------------------------------------------ backward
def _rel_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / max(1e-30, float(want.abs().max())))


def _post(shape, seed, bias=True):
    import seeded
    gen = torch.Generator().manual_seed(seed)
    return [t.to(DEV) if t is not None else None for t in seeded.posterior(gen, shape, bias)]


def _sampled_ref64(x, shared, post, kw, kb, G):
    """float64 autograd of y[s] = x[s] (mu_w + sigma eps_w[s])^T + mu_b + sigma eps_b[s] on the keys' eps -> (gx, g_mu_w, g_rho_w,
    g_mu_b, g_rho_b) of sum(y * G)."""
    mw, rw, mb, rb = post
    S = kw.nsamples
    ew = ops.eps_philox(tuple(mw.shape), kw, DEV).double()
    eb = ops.eps_philox(tuple(mb.shape), kb, DEV).double()
    leaves = [t.detach().double().requires_grad_() for t in (x, mw, rw, mb, rb)]
    xx, m_w, r_w, m_b, r_b = leaves
    w = m_w + (F.softplus(r_w) + 1e-10) * ew
    b = m_b + (F.softplus(r_b) + 1e-10) * eb
    xs = xx.expand(S, *xx.shape) if shared else xx
    y = torch.einsum("smk,snk->smn", xs, w) + b.unsqueeze(1)
    (y * G.double()).sum().backward()
    return [t.grad for t in leaves]


def _sampled_grads(x, shared, post, kw, kb, G):
    leaves = [x.detach().clone().requires_grad_()] + [t.detach().clone().requires_grad_() for t in post]
    y = ops.linear_sampled(leaves[0], *leaves[1:], kw, kb, shared, compute="f32")
    (y * G).sum().backward()
    torch.cuda.synchronize()
    return [t.grad for t in leaves]


def _check_grads(got, want, tol, what):
    for name, g, w in zip(("gx", "g_mu_w", "g_rho_w", "g_mu_b", "g_rho_b"), got, want):
        if w is None:
            continue
        assert g is not None, (what, name)
        err = _rel_err(g, w)
        assert err <= tol, (what, name, err)


def _narrow_max_samples(M, N, K, ws_bytes):
    """Largest S whose narrow head backward fits the workspace slabs: S (2 Z N K + Z N + N) 4 bytes, Z = ceil(M / 256), behind
    the workspace's reserved 64 KiB."""
    Z = -(-M // 256)
    return (ws_bytes - (64 << 10)) // ((2 * Z * N * K + Z * N + N) * 4)


@gpu
def test_narrow_head_backward_at_the_workspace_boundary():
    """BASELINE-shaped head (K = 1200, N = 10, M = 512): the largest S that fits runs the narrow kernel, S + 1 is refused with
    BNN_E_UNSUPPORTED and runs the general kernels; both against float64, and the narrow kernel against the general one."""
    M, N, K = 512, 10, 1200
    lib = _lib.load()
    ws = _lib.ensure_workspace(DEV)
    Smax = _narrow_max_samples(M, N, K, ws.numel())
    assert Smax >= 1
    post = _post((N, K), 21)
    mw, rw = post[0], post[1]
    for S, rc_want in ((Smax, 0), (Smax + 1, _lib.E_UNSUPPORTED)):
        kw = DrawKey(77, 501, 0, S, 3)
        x = torch.randn(S, M, K, device=DEV)
        gy = torch.randn(S, M, N, device=DEV)
        gx, gm, gr = torch.empty_like(x), torch.empty_like(mw), torch.empty_like(rw)
        rs = ops._rng_struct(kw, DEV)
        rc = lib.bnn_linear_backward_narrow_sampled(_lib.ptr(x), M * K, K, _lib.ptr(gy), M * N, N, _lib.ptr(mw), _lib.ptr(rw),
                                                   _lib.ptr(gx), M * K, K, _lib.ptr(gm), _lib.ptr(gr), None, None, None, M, N, K, S,
                                                   ctypes.byref(rs), None, None, 0, 0, _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert rc == rc_want, (S, rc)
    for S in (Smax, Smax + 1):
        kw, kb = DrawKey(77, 511, 0, S, 3), DrawKey(77, 512, 0, S, 3)
        g = torch.Generator().manual_seed(S)
        x0 = torch.randn(M, K, generator=g).to(DEV)
        G = torch.randn(S, M, N, generator=g).to(DEV)
        xs = x0.expand(S, M, K).contiguous()
        got = _sampled_grads(xs, False, post, kw, kb, G)
        _check_grads(got, _sampled_ref64(xs, False, post, kw, kb, G), 1e-4, "narrow S = %d" % S)
        if S == Smax:
            # the same gradients through the general kernels (a shared input that wants its gradient never takes the narrow one)
            gen = _sampled_grads(x0, True, post, kw, kb, G)
            assert _rel_err(got[0].sum(0), gen[0]) <= 1e-4
            for a, b in zip(got[1:], gen[1:]):
                assert _rel_err(a, b) <= 1e-4


@gpu
@pytest.mark.parametrize("S", [1, 2, 7, 8, 9])
def test_weight_gradient_sample_split_vs_float64(S):
    """N x K = 40 x 96 (one tile): the weight gradient splits the samples over min(S, 8) workgroups -- S = 9 unevenly."""
    M, N, K = 33, 40, 96
    post = _post((N, K), 30 + S)
    kw, kb = DrawKey(5, 601, 0, S, 2), DrawKey(5, 602, 0, S, 2)
    g = torch.Generator().manual_seed(S)
    x = torch.randn(S, M, K, generator=g).to(DEV)
    G = torch.randn(S, M, N, generator=g).to(DEV)
    _check_grads(_sampled_grads(x, False, post, kw, kb, G), _sampled_ref64(x, False, post, kw, kb, G), 1e-4, "split S = %d" % S)


SHARED_S = [33, 300]


@gpu
@pytest.mark.parametrize("S", SHARED_S)
def test_shared_input_gradient_normal_linear(S):
    M, N, K = 16, 40, 64
    post = _post((N, K), 40 + S)
    kw, kb = DrawKey(9, 701, 0, S, 4), DrawKey(9, 702, 0, S, 4)
    g = torch.Generator().manual_seed(S)
    x = torch.randn(M, K, generator=g).to(DEV)
    G = torch.randn(S, M, N, generator=g).to(DEV)
    _check_grads(_sampled_grads(x, True, post, kw, kb, G), _sampled_ref64(x, True, post, kw, kb, G), 1e-4, "shared S = %d" % S)


@gpu
@pytest.mark.parametrize("S", SHARED_S)
def test_shared_input_gradient_plain_linear(S):
    M, N, K = 16, 40, 64
    g = torch.Generator().manual_seed(S)
    x = torch.randn(M, K, generator=g).to(DEV).requires_grad_()
    w = torch.randn(S, N, K, generator=g).to(DEV).requires_grad_()
    b = torch.randn(S, N, generator=g).to(DEV).requires_grad_()
    G = torch.randn(S, M, N, generator=g).to(DEV)
    (ops.linear_plain(x, w, b, True) * G).sum().backward()
    torch.cuda.synchronize()
    x64, w64, b64 = (t.detach().double().requires_grad_() for t in (x, w, b))
    ((torch.einsum("mk,snk->smn", x64, w64) + b64.unsqueeze(1)) * G.double()).sum().backward()
    for name, a, r in (("gx", x.grad, x64.grad), ("gw", w.grad, w64.grad), ("gb", b.grad, b64.grad)):
        assert _rel_err(a, r) <= 1e-4, (name, S)


@gpu
@pytest.mark.parametrize("S", SHARED_S)
def test_shared_input_gradient_flipout_linear(S):
    M, O, K = 16, 40, 64
    g = torch.Generator().manual_seed(S)
    mu = (torch.randn(O, K, generator=g) * 0.1).to(DEV).requires_grad_()
    rho = (torch.randn(O, K, generator=g) * 0.2 - 3.0).to(DEV).requires_grad_()
    x = torch.randn(M, K, generator=g).to(DEV).requires_grad_()
    G = torch.randn(S, M, O, generator=g).to(DEV)
    key = DrawKey(13, 801, 0, S, 6)
    assert ops.flipout_drawable(mu)
    (ops.linear_flipout_mc(x, mu, rho, key, True) * G).sum().backward()
    torch.cuda.synchronize()
    sg = ops.flipout_signs(key, 1, O + K, DEV)[:, 0].double()              # (S, O + K): R = [:, :O], S = [:, O:]
    x64, m64, r64 = (t.detach().double().requires_grad_() for t in (x, mu, rho))
    w = m64 + (F.softplus(r64) + 1e-10) * (sg[:, :O].unsqueeze(2) * sg[:, O:].unsqueeze(1))
    (torch.einsum("mk,sok->smo", x64, w) * G.double()).sum().backward()
    for name, a, r in (("gx", x.grad, x64.grad), ("g_mu", mu.grad, m64.grad), ("g_rho", rho.grad, r64.grad)):
        assert _rel_err(a, r) <= 1e-4, (name, S)
