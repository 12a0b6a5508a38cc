"""MultivariateNormalLinear on the MC-batched device path (nn.keyed_mvn_draws): keyed per-sample draws (bnn_mvn_draw, its
backward bnn_mvn_draw_backward; ops.mvn_draw, ops.mvn_draw_layer) and the closed-form KL against an isotropic prior
(bnn_mvn_kl, bnn_mvn_kl_backward; ops.mvn_kl).

CPU: a float64 twin of the MVN-noise contract (include/bnn_hip.h) on the oracle's Philox -- the dropout mask's uniforms at
element o K + j, then w_s = mu + L u_s -- checked against WeightMultivariateNormal.sample_with_noise; the switch and the CPU path.
GPU: the draw against the twin with derived bounds, bit-for-bit invariances, the layer in an MC pass (both modes), its
backward, the KL against float64 torch, the CIFAR10 example net and predictive_uncertainty.

Draw bound: w_s[i] sums i + 2 fp32 terms (mu and i + 1 products), so |w - w64| <= gamma_{K+1} (|mu| + sum L u) from the
summation (Higham eq. 3.5), plus EPS_L sum L u for the error of L itself: softplus on the native exp2 / log2 / rcp units
(log1p(e) = ln(u) e / (u - 1): a few ulp relative) and a correctly rounded sqrt, EPS_L = 2^-20 covering both."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.distributions import MultivariateNormal, Normal
from torch.distributions.kl import kl_divergence

from conftest import assert_close_scaled, load_golden, allclose
import bf16ref
from test_mc_dropout import mask_uniforms

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, _rng, ops
from bayesianneuralnetworks_amd._rng import DrawKey
from bayesianneuralnetworks_amd.nn import (BayesianNetworkModule, KLDivergence, MultivariateNormalLinear, NormalLinear,
                                           WeightMultivariateNormal, keyed_mvn_draws)
from bayesianneuralnetworks_amd.nn import _settings

gpu = pytest.mark.gpu
EPS_L = 2.0 ** -20
GENS = [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16]


# ------------------------------------------------------------------------------------------------ the twin
def mvn_uniforms(key, s, epoch_dev, rows, K):
    """u_s[o][j] (rows, K) of sample key.sample0 + s: the mask uniform of element o K + j, fp32 values as float64."""
    u = mask_uniforms(key.seed, key.stream, key.sample0 + s, key.epoch_host, (epoch_dev + key.epoch_dev_delta) & 0xFFFFFFFF,
                      rows * K, key.gen)
    return u.astype(np.float64).reshape(rows, K)


def tril_l64(scale):
    """L = sqrt(tril(softplus(scale)) + 1e-10 I) in float64 (torch's softplus, threshold 20); only the lower triangle is read."""
    sc = np.asarray(scale, dtype=np.float64)
    K = sc.shape[-1]
    sp = np.where(sc > 20, sc, np.log1p(np.exp(np.minimum(sc, 20))))
    return np.sqrt(np.tril(sp) + 1e-10 * np.eye(K))


def mvn_twin(mu, scale, u):
    """mu (rows, K), scale (rows, K, K), u (rows, K) -> (w, sum_j L |u|) float64."""
    L = tril_l64(scale)
    return np.asarray(mu, np.float64) + np.einsum("oij,oj->oi", L, u), np.einsum("oij,oj->oi", L, np.abs(u))


def twin_draws(mu, scale, key, epoch_dev):
    """(S, *mu.shape) float64 twin draws of a device key and the summation bound's sum L u."""
    mu2 = mu.detach().double().cpu().numpy()
    K = mu2.shape[-1]
    rows = mu2.size // K
    sc = scale.detach().double().cpu().numpy().reshape(rows, K, K)
    ws, ls = [], []
    for s in range(key.nsamples):
        w, l = mvn_twin(mu2.reshape(rows, K), sc, mvn_uniforms(key, s, epoch_dev, rows, K))
        ws.append(w.reshape(mu2.shape))
        ls.append(l.reshape(mu2.shape))
    return np.stack(ws), np.stack(ls)


def _epoch_dev(dev):
    return int(_rng.default_generator.epoch_dev(dev)[0].item())


def _posterior(O, K, gen, upper=5.0):
    mu = (torch.rand(O, K, generator=gen) * 2 - 1) / K ** 0.5
    scale = torch.randn(O, K, K, generator=gen) * 0.15 - 2.0
    scale = torch.where(torch.ones(K, K, dtype=torch.bool).triu(1), torch.full_like(scale, upper), scale)
    return mu, scale


# ------------------------------------------------------------------------------------------------ CPU
def test_switch_exists_and_defaults_off():
    assert _settings.keyed_mvn_enabled() is False
    assert "keyed_mvn_draws" not in bnn.nn.__all__ and "keyed_mvn_draws" not in bnn.__all__
    keyed_mvn_draws(True)
    try:
        assert _settings.keyed_mvn_enabled() is True
    finally:
        keyed_mvn_draws(False)
    assert _settings.keyed_mvn_enabled() is False


@pytest.mark.parametrize("gen", GENS)
def test_twin_matches_sample_with_noise(gen):
    torch.manual_seed(0)
    w = WeightMultivariateNormal(7, 33)
    with torch.no_grad():
        w.mean.normal_()
        w.scale.copy_(_posterior(7, 33, torch.Generator().manual_seed(1), upper=-100.0)[1])
    key = DrawKey(0x1234_5678_9ABC, 17, 3, 1, 9, gen=gen)
    u = mvn_uniforms(key, 0, 5, 7, 33)
    w.sample_with_noise(torch.from_numpy(u).float())
    want, lu = mvn_twin(w.mean.detach().numpy(), w.scale.detach().numpy(), u)
    got = w.sampled.detach().double().numpy()
    # torch's fp32 matmul against float64: K + 1 addends
    assert (np.abs(got - want) <= bf16ref.gamma(34) * (np.abs(w.mean.detach().numpy()) + lu) + 4e-7 * lu + 1e-12).all()
    # the upper triangle is never read: any value there gives the same twin
    sc2 = w.scale.detach().numpy().copy()
    sc2[:, np.triu_indices(33, 1)[0], np.triu_indices(33, 1)[1]] = 5.0
    assert np.array_equal(mvn_twin(w.mean.detach().numpy(), sc2, u)[0], want)


def test_twin_uniform_layout_bias_is_one_row():
    key = DrawKey(99, 4, 0, 1, 2, gen=_rng.GEN_PHILOX10_U24)
    assert np.array_equal(mvn_uniforms(key, 0, 0, 1, 10)[0], mvn_uniforms(key, 0, 0, 2, 5).reshape(-1))


def test_cpu_net_unchanged_with_switch_on():
    class Net(BayesianNetworkModule):
        def __init__(self):
            super().__init__(6, 3, 3)
            self.layers = torch.nn.Sequential(NormalLinear(6, 8), torch.nn.ReLU(), MultivariateNormalLinear(8, 3))

        def _forward(self, x):
            return self.layers(x)

    torch.manual_seed(4)
    net = Net()
    x = torch.randn(5, 6)
    torch.manual_seed(7)
    off = torch.stack(net(x))
    keyed_mvn_draws(True)
    try:
        torch.manual_seed(7)
        on = torch.stack(net(x))
        kl_on = KLDivergence()(net)
    finally:
        keyed_mvn_draws(False)
    assert torch.equal(on, off)
    assert torch.equal(kl_on, KLDivergence()(net))
    assert net.layers[2].weight.draw_key is None and net.layers[2].weight._mvn_stream is None


# ------------------------------------------------------------------------------------------------ GPU: the draw
@pytest.fixture
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def keyed():
    keyed_mvn_draws(True)
    yield
    keyed_mvn_draws(False)
    bnn.set_compute("f32")


def _launches():
    return _lib.load().bnn_launch_count()


@gpu
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("O,K,bias", [(10, 128, False), (1, 10, True), (7, 33, False), (64, 257, False), (3, 1024, False)])
@pytest.mark.parametrize("S", [1, 2, 8, 17])
def test_mvn_draw_matches_twin(dev, gen, O, K, bias, S):
    g = torch.Generator().manual_seed(O * 1000 + K + S)
    mu, scale = _posterior(O, K, g)
    if bias:
        mu, scale = mu[0], scale[0]                         # (O,) with (O, O): one row
    mu, scale = mu.to(dev), scale.to(dev)
    key = DrawKey(0xDEAD_BEEF_0123, 41, 2, S, 6, gen=gen)
    w = ops.mvn_draw(mu, scale, key)
    assert w.shape == (S,) + tuple(mu.shape) and w.dtype == torch.float32
    want, lu = twin_draws(mu, scale, key, _epoch_dev(dev))
    absmu = np.abs(mu.double().cpu().numpy())
    bound = bf16ref.gamma(K + 1) * (absmu + lu) + EPS_L * lu
    err = np.abs(w.double().cpu().numpy() - want)
    assert (err <= bound).all(), (float(err.max()), float((err - bound).max()))


@gpu
@pytest.mark.parametrize("gen", GENS)
def test_mvn_draw_is_bitwise_invariant(dev, gen):
    mu, scale = (t.to(dev) for t in _posterior(64, 257, torch.Generator().manual_seed(3)))
    k8 = DrawKey(77, 12, 0, 8, 3, gen=gen)
    k4 = DrawKey(77, 12, 4, 4, 3, gen=gen)
    w8 = ops.mvn_draw(mu, scale, k8)
    assert torch.equal(ops.mvn_draw(mu, scale, k4), w8[4:])
    assert torch.equal(ops.mvn_draw(mu, scale, k8), w8)
    # the upper triangle has no effect
    assert torch.equal(ops.mvn_draw(mu, scale.tril() + torch.ones_like(scale).triu(1) * -100, k8), w8)
    # above 16 samples the triangle is streamed per group of samples: the values are the same
    k20 = DrawKey(77, 12, 0, 20, 3, gen=gen)
    assert torch.equal(ops.mvn_draw(mu, scale, k20)[:8], w8)


@gpu
def test_mvn_draw_refuses_bad_arguments(dev):
    mu, scale = torch.zeros(4, 8, device=dev), torch.zeros(4, 8, 7, device=dev)
    with pytest.raises(_lib.BnnHipError):
        ops.mvn_draw(mu, scale, DrawKey(1, 1, 0, 1, 0))
    with pytest.raises(_lib.BnnHipError):
        ops.mvn_draw(torch.zeros(4, 8), torch.zeros(4, 8, 8), DrawKey(1, 1, 0, 1, 0))


# ------------------------------------------------------------------------------------------------ GPU: the layer in an MC pass
def _layer_ref(x, layer, S, dev):
    """float64 F.linear of x on the twin draws of the layer's recorded keys -> (S, rows, O), and the drawn fp32 operands."""
    ed = _epoch_dev(dev)
    w, _ = twin_draws(layer.weight.mean, layer.weight.scale, layer.weight.draw_key, ed)
    b, _ = twin_draws(layer.bias.mean, layer.bias.scale, layer.bias.draw_key, ed)
    return torch.from_numpy(w), torch.from_numpy(b)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shared", [True, False])
def test_mvn_layer_in_mc_pass(dev, keyed, mode, shared):
    S, B, K, O = 4, 32, 128, 10
    torch.manual_seed(5)
    layer = MultivariateNormalLinear(K, O).to(dev)
    x = torch.randn(B if shared else S * B, K, generator=torch.Generator().manual_seed(2)).to(dev)
    bnn.set_compute(mode)
    bnn.manual_seed(3)
    sampled_before = layer.sampled[0].clone()
    with torch.no_grad(), _mc.McContext(S, B):
        n0 = _launches()
        y = layer(x)
        assert _launches() == n0 + 2
    assert torch.equal(layer.sampled[0], sampled_before)
    y = y.reshape(S, B, O)
    assert not torch.equal(y[0], y[1])
    w64, b64 = _layer_ref(x, layer, S, dev)
    xs = x.double().cpu().reshape(1 if shared else S, B, K).expand(S, B, K)
    if mode == "f32":
        want = torch.stack([F.linear(xs[s], w64[s], b64[s]) for s in range(S)])
        assert_close_scaled(y.double().cpu().numpy(), want.numpy(), 1e-5, "f32")
    else:
        # the device's drawn weights (bit-identical to the layer's: the same kernel on the same keys), rounded to bf16
        wd = ops.mvn_draw(layer.weight.mean, layer.weight.scale, layer.weight.draw_key).double().cpu()
        bd = ops.mvn_draw(layer.bias.mean, layer.bias.scale, layer.bias.draw_key).double().cpu()
        for s in range(S):
            t, acc, _, _ = bf16ref.chain_layer(bf16ref.rne_bf16(xs[s]), None, bf16ref.rne_bf16(wd[s]), bd[s])
            err = (y[s].double().cpu() - t).abs()
            assert bool((err <= acc).all()), (s, float((err - acc).max()))
    # sample=False reuses the recorded keys; a pass of another S refuses them
    with torch.no_grad(), _mc.McContext(S, B):
        y2 = layer(x, sample=False)
    assert torch.equal(y2.reshape(S, B, O), y)
    with torch.no_grad(), _mc.McContext(S + 1, B), pytest.raises(RuntimeError, match="sample=False"):
        layer(x[:B] if shared else torch.cat([x, x[:B]]), sample=False)


@gpu
@pytest.mark.parametrize("first", [True, False])
def test_mvn_net_gives_every_sample_its_own_head(dev, keyed, first):
    S, B = 4, 16

    class Net(BayesianNetworkModule):
        def __init__(self):
            super().__init__(12, 5, S)
            mods = [MultivariateNormalLinear(12, 5)] if first else [NormalLinear(12, 24), torch.nn.ReLU(),
                                                                      MultivariateNormalLinear(24, 5)]
            self.layers = torch.nn.Sequential(*mods)

        def _forward(self, x):
            return self.layers(x)

    torch.manual_seed(8)
    net = Net().to(dev)
    net.mc_batched = True
    head = net.layers[-1]
    seen = {}
    hk = head.register_forward_hook(lambda m, i, o: seen.update(x=i[0].detach(), y=o.detach()))
    x = torch.randn(B, 12, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        ys = torch.stack(net(x))
    hk.remove()
    assert seen["x"].shape[0] == (B if first else S * B)
    assert not torch.equal(ys[0], ys[1])
    w64, b64 = _layer_ref(seen["x"], head, S, dev)
    xs = seen["x"].double().cpu().reshape(1 if first else S, B, -1).expand(S, B, -1)
    want = torch.stack([F.linear(xs[s], w64[s], b64[s]) for s in range(S)])
    assert_close_scaled(seen["y"].double().cpu().reshape(S, B, 5).numpy(), want.numpy(), 1e-5, "head")


# ------------------------------------------------------------------------------------------------ GPU: backward
def _ref_draws64(mu, scale, u):
    """The reference's expression (core.py:60-92) in float64 autograd on given uniforms u (S, rows, K)."""
    K = mu.shape[-1]
    var = torch.tril(F.softplus(scale)) + 1e-10 * torch.eye(K, dtype=torch.float64)
    std = var.sqrt()
    return mu + torch.matmul(std, u.unsqueeze(-1)).squeeze(-1)


@gpu
@pytest.mark.parametrize("shared", [True, False])
def test_mvn_layer_backward_matches_float64_autograd(dev, keyed, shared):
    S, B, K, O = 3, 16, 40, 6
    torch.manual_seed(11)
    layer = MultivariateNormalLinear(K, O).to(dev)
    x = torch.randn(B if shared else S * B, K, generator=torch.Generator().manual_seed(6)).to(dev).requires_grad_(True)
    gy = torch.randn(S * B, O, generator=torch.Generator().manual_seed(7)).to(dev)
    bnn.manual_seed(2)

    def run():
        for p in layer.parameters():
            p.grad = None
        x.grad = None
        with _mc.McContext(S, B):
            y = layer(x, sample=False) if layer.weight.draw_key is not None else layer(x)
        (y * gy).sum().backward()
        return [t.grad.clone() for t in (layer.weight.mean, layer.weight.scale, layer.bias.mean, layer.bias.scale, x)]

    got = run()
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    ed = _epoch_dev(dev)
    kw, kb = layer.weight.draw_key, layer.bias.draw_key
    uw = torch.from_numpy(np.stack([mvn_uniforms(kw, s, ed, O, K) for s in range(S)]))
    ub = torch.from_numpy(np.stack([mvn_uniforms(kb, s, ed, 1, O)[0] for s in range(S)]))
    p64 = [t.detach().double().cpu().requires_grad_(True) for t in (layer.weight.mean, layer.weight.scale, layer.bias.mean,
                                                                    layer.bias.scale)]
    x64 = x.detach().double().cpu().requires_grad_(True)
    w = _ref_draws64(p64[0], p64[1], uw)                                   # (S, O, K)
    b = _ref_draws64(p64[2], p64[3], ub)                                   # (S, O)
    xs = x64.reshape(1 if shared else S, B, K).expand(S, B, K)
    y64 = torch.stack([F.linear(xs[s], w[s], b[s]) for s in range(S)]).reshape(S * B, O)
    (y64 * gy.double().cpu()).sum().backward()
    names = ("g_mu_w", "g_scale_w", "g_mu_b", "g_scale_b", "g_x")
    for g, ref, name in zip(got, p64 + [x64], names):
        assert_close_scaled(g.double().cpu().numpy(), ref.grad.numpy(), 1e-5, name)
    assert bool((got[1].triu(1) == 0).all()) and bool((got[3].triu(1) == 0).all())


# ------------------------------------------------------------------------------------------------ GPU: KL
def _kl64(entries, n_batches):
    """float64 KLDivergence: entries of (posterior kind, params, prior) -> the scalar, with autograd on the params."""
    means = []
    for kind, ps, prior in entries:
        if kind == "mvn":
            mu, scale = ps
            K = mu.shape[-1]
            V = torch.tril(F.softplus(scale)) + 1e-10 * torch.eye(K, dtype=torch.float64)
            pr = MultivariateNormal(prior.loc.double(), scale_tril=prior.scale_tril.double())
            means.append(kl_divergence(MultivariateNormal(mu, scale_tril=V), pr).mean())
        else:
            mu, rho = ps
            means.append(kl_divergence(Normal(mu, 1e-10 + F.softplus(rho)), Normal(float(prior.loc), float(prior.scale))).mean())
    return torch.stack(means).mean() / n_batches


def _check_kl(net, entries_of, n_batches, dev):
    params = [p for p in net.parameters()]
    for p in params:
        p.grad = None
    kl = KLDivergence(n_batches)(net)
    kl.backward()
    p64 = {id(p): p.detach().double().cpu().requires_grad_(True) for p in params}
    want = _kl64(entries_of(p64), n_batches)
    want.backward()
    assert abs(kl.item() - want.item()) <= 1e-5 * abs(want.item()), (kl.item(), want.item())
    for p in params:
        assert_close_scaled(p.grad.double().cpu().numpy(), p64[id(p)].grad.numpy(), 2e-5, "grad %s" % (tuple(p.shape),))


class _Wrap(BayesianNetworkModule):
    def __init__(self, *mods):
        super().__init__(1, 1, 1)
        self.layers = torch.nn.Sequential(*mods)


@gpu
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("prior", ["default", "iso"])
def test_mvn_kl_matches_float64(dev, keyed, fuse, prior):
    torch.manual_seed(13)
    if prior == "default":
        layer = MultivariateNormalLinear(48, 7)
    else:
        layer = MultivariateNormalLinear(48, 7, weight_prior=MultivariateNormal(torch.full((7, 48), 0.5),
                                                                                scale_tril=2.0 * torch.eye(48).repeat(7, 1, 1)),
                                         bias_prior=MultivariateNormal(torch.full((7,), 0.5), scale_tril=2.0 * torch.eye(7)))
    net = _Wrap(layer).to(dev)
    bnn.nn.fuse_kl_gradient(fuse)
    try:
        n0 = _launches()
        with torch.no_grad():
            KLDivergence(3.0)(net)
        assert _launches() == n0 + 2                         # weight and bias in one bnn_mvn_kl call
        _check_kl(net, lambda p: [("mvn", (p[id(layer.weight.mean)], p[id(layer.weight.scale)]), layer.weight_prior),
                                  ("mvn", (p[id(layer.bias.mean)], p[id(layer.bias.scale)]), layer.bias_prior)], 3.0, dev)
    finally:
        bnn.nn.fuse_kl_gradient(False)


@gpu
@pytest.mark.parametrize("fuse", [False, True])
def test_mixed_model_kl_matches_float64(dev, keyed, fuse):
    torch.manual_seed(14)
    a, m = NormalLinear(20, 16), MultivariateNormalLinear(16, 5)
    net = _Wrap(a, torch.nn.ReLU(), m).to(dev)
    bnn.nn.fuse_kl_gradient(fuse)
    try:
        _check_kl(net, lambda p: [("normal", (p[id(a.weight.mean)], p[id(a.weight.scale)]), a.weight_prior),
                                  ("normal", (p[id(a.bias.mean)], p[id(a.bias.scale)]), a.bias_prior),
                                  ("mvn", (p[id(m.weight.mean)], p[id(m.weight.scale)]), m.weight_prior),
                                  ("mvn", (p[id(m.bias.mean)], p[id(m.bias.scale)]), m.bias_prior)], 2.0, dev)
        # compute_kl of one tensor: the same closed form
        k1 = KLDivergence().compute_kl(m.weight, m, 'w')
        with torch.no_grad():
            w64 = m.weight.mean.double().cpu(), m.weight.scale.double().cpu()
            want = _kl64([("mvn", w64, m.weight_prior)], 1.0)
        assert abs(k1.item() - want.item()) <= 1e-5 * abs(want.item())
    finally:
        bnn.nn.fuse_kl_gradient(False)


@gpu
def test_non_isotropic_prior_keeps_torch_path(dev, keyed):
    torch.manual_seed(15)
    tril = torch.eye(9).repeat(4, 1, 1)
    tril[:, 3, 1] = 0.25
    layer = MultivariateNormalLinear(9, 4, weight_prior=MultivariateNormal(torch.zeros(4, 9), scale_tril=tril), bias=False)
    net = _Wrap(layer).to(dev)
    assert ops.mvn_isotropic(layer.weight_prior) is None
    n0 = _launches()
    kl = KLDivergence()(net)
    assert _launches() == n0
    keyed_mvn_draws(False)
    assert torch.equal(kl, KLDivergence()(net))


@gpu
def test_mvn_golden_fixture_with_switch_on(dev, keyed):
    g = load_golden("mvn_linear_128x10")
    layer = MultivariateNormalLinear(128, 10)
    with torch.no_grad():
        layer.weight.mean.copy_(torch.from_numpy(g["mu_w"])); layer.weight.scale.copy_(torch.from_numpy(g["scale_w"]))
        layer.bias.mean.copy_(torch.from_numpy(g["mu_b"])); layer.bias.scale.copy_(torch.from_numpy(g["scale_b"]))
    layer = layer.to(dev)
    layer.weight.sample_with_noise(torch.from_numpy(g["u_w"]).to(dev))
    layer.bias.sample_with_noise(torch.from_numpy(g["u_b"]).to(dev))
    layer.sampled = (layer.weight.sampled, layer.bias.sampled)
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    y = layer(x, sample=False)                      # outside an MC pass: the torch path
    assert allclose(y.detach().cpu().numpy(), g["y"])
    n0 = _launches()
    kl = KLDivergence(number_of_batches=float(g["n_batches"]))(_Wrap(layer))
    assert _launches() == n0 + 2                    # the HIP closed form
    assert abs(kl.item() - float(g["kl"])) <= 1e-5 * abs(float(g["kl"]))
    ((y * torch.from_numpy(g["gy"]).to(dev)).sum() + kl).backward()
    for got, want in ((layer.weight.mean.grad, "g_mu_w"), (layer.weight.scale.grad, "g_scale_w"),
                      (layer.bias.mean.grad, "g_mu_b"), (layer.bias.scale.grad, "g_scale_b"), (x.grad, "g_x")):
        assert allclose(got.detach().cpu().numpy(), g[want], 2e-5), want


# ------------------------------------------------------------------------------------------------ GPU: networks
@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_cifar10_net_with_keyed_head(dev, keyed, mode):
    from torch.nn import Linear, Conv2d, BatchNorm2d, ELU, Softmax, Flatten, Sequential
    from bayesianneuralnetworks_amd.nn import NormalConv2d
    S, B = 4, 16

    class BCNN(BayesianNetworkModule):
        def __init__(self):
            super().__init__(3, 10, S)
            self.layers = Sequential(Conv2d(3, 64, 5, padding=2, stride=2), BatchNorm2d(64), ELU(), Conv2d(64, 128, 5, padding=2, stride=2), ELU(),
                                     Conv2d(128, 128, 5, padding=2, stride=2), ELU(), Conv2d(128, 128, 3, padding=1), ELU(),
                                     Conv2d(128, 128, 3, padding=1), ELU(), NormalConv2d(128, 128, 3, padding=1), ELU(), Flatten(),
                                     Linear(2048, 128), ELU(), MultivariateNormalLinear(128, 10), Softmax(dim=-1))

        def _forward(self, x):
            return self.layers(x)

    torch.manual_seed(23)
    net = BCNN().to(dev).eval()
    net.mc_batched = True
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(dev)
    conv, head = net.layers[11], net.layers[16]
    seen = {}
    hks = [conv.register_forward_hook(lambda m, i, o: seen.update(cx=i[0].detach(), cy=o.detach())),
           head.register_forward_hook(lambda m, i, o: seen.update(hx=i[0].detach(), hy=o.detach()))]
    bnn.set_compute(mode)
    try:
        bnn.manual_seed(11)
        n0 = _launches()
        with torch.no_grad():
            ys = net(x)
        assert _launches() == n0 + 4                # conv: draw + implicit GEMM; head: draw + dense
    finally:
        for h in hks:
            h.remove()
    assert len(ys) == S and not torch.equal(ys[0], ys[1])
    assert seen["hx"].shape == (S * B, 128)
    tol = 1e-5 if mode == "f32" else 2e-2
    # the conv on its recorded keys (K1 draws), as in the existing CIFAR10 test
    w = ops._sample_affine_philox_raw(conv.weight.mean.detach(), conv.weight.scale.detach(), conv.weight.draw_key).double().cpu()
    b = ops._sample_affine_philox_raw(conv.bias.mean.detach(), conv.bias.scale.detach(), conv.bias.draw_key).double().cpu()
    for s in range(S):
        want = F.conv2d(seen["cx"].double().cpu(), w[s], b[s], 1, 1).numpy()
        assert_close_scaled(seen["cy"][s * B:(s + 1) * B].double().cpu().numpy(), want, tol, "conv %d" % s)
    # the head on the twin draws of its recorded keys
    w64, b64 = _layer_ref(seen["hx"], head, S, dev)
    hx = seen["hx"].double().cpu().reshape(S, B, 128)
    for s in range(S):
        want = F.linear(hx[s], w64[s], b64[s])
        if mode == "f32":
            assert_close_scaled(seen["hy"][s * B:(s + 1) * B].double().cpu().numpy(), want.numpy(), 1e-5, "head %d" % s)
        else:
            wd = ops.mvn_draw(head.weight.mean, head.weight.scale, head.weight.draw_key).double().cpu()
            bd = ops.mvn_draw(head.bias.mean, head.bias.scale, head.bias.draw_key).double().cpu()
            t, acc, _, _ = bf16ref.chain_layer(bf16ref.rne_bf16(hx[s]), None, bf16ref.rne_bf16(wd[s]), bd[s])
            err = (seen["hy"][s * B:(s + 1) * B].double().cpu() - t).abs()
            assert bool((err <= acc).all()), (s, float((err - acc).max()))


@gpu
def test_predictive_uncertainty_of_mvn_headed_net(dev, keyed):
    S, B = 8, 64

    class Net(BayesianNetworkModule):
        def __init__(self):
            super().__init__(16, 6, S)
            self.layers = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ELU(), MultivariateNormalLinear(32, 6))

        def _forward(self, x):
            return self.layers(x)

    torch.manual_seed(31)
    net = Net().to(dev).eval()
    net.mc_batched = True
    x = torch.randn(B, 16, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        bnn.manual_seed(5)
        ys = net._forward_batched_stacked(x, S, 0)
        bnn.manual_seed(5)
        got = net.predictive_uncertainty(x, inputs="logits")
    want = ops.uncertainty_f64(ys, "logits")
    assert float(got.epistemic.max()) > 1e-4
    for name in ("mean", "total", "aleatoric", "epistemic"):
        a, b = getattr(got, name).double().cpu(), getattr(want, name).double().cpu()
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(np.log(6))), name


# ------------------------------------------------------------------------------------------------ code object
def test_mvn_kernels_do_not_spill():
    """Every MVN kernel keeps its state in registers: no VGPR or SGPR spills, no scratch."""
    tools = ["/opt/rocm/llvm/bin/llvm-objcopy", "/opt/rocm/llvm/bin/clang-offload-bundler", "/opt/rocm/llvm/bin/llvm-readelf"]
    if not all(os.path.exists(t) for t in tools) or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("ROCm LLVM tools or the library not found")
    notes = ""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([tools[0], "--dump-section=.hip_fatbin=" + fat, _lib.LIB_PATH, os.path.join(d, "lib.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
        for i, a in enumerate(starts):
            part, co = os.path.join(d, "b%d.bin" % i), os.path.join(d, "b%d.co" % i)
            open(part, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.check_call([tools[1], "--unbundle", "--type=o", "--input=" + part,
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
            notes += subprocess.check_output([tools[2], "--notes", co]).decode()
    seen = 0
    for block in notes.split("- .agpr_count")[1:]:
        f = dict(re.findall(r"\.(name|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if re.match(r"_ZN3bnn\d+k_mvn_", f.get("name", "")):
            seen += 1
            assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, f
            assert int(f.get("private_segment_fixed_size", 0)) == 0, f
    assert seen == 13          # draw and backward at 1, 2, 4, 8, 16 samples per pass; KL partial, final, backward
