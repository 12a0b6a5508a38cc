"""Predictive uncertainty (bnn_mc_uncertainty, ops.mc_uncertainty, BayesianNetworkModule.predictive_uncertainty): the mean of
the per-sample probabilities, its entropy (total), the mean per-sample entropy (aleatoric) and their difference (epistemic,
the mutual information) -- examples/MNIST/uncertainty.py:47-52 with the split a Bayesian network is trained for.

CPU: the C-ABI entry and its argument errors, the op's refusals, the float64 CPU path against a NumPy restatement.
GPU: the kernel against float64 over both work splits and both input kinds, bitwise reproducibility, the fused head's
partial logits, the module's paths and modes, the MNIST example net, and the epoch / KL tails."""
import ctypes
import os
import re

import numpy as np
import pytest
import seeded
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, Entropy, NormalLinear
from conftest import ROOT, load_golden

gpu = pytest.mark.gpu


def ref64(y, inputs):
    """float64 NumPy restatement: y (S, rows, C) -> mean (rows, C), total, aleatoric, epistemic (rows)."""
    y = np.asarray(y, dtype=np.float64)
    if inputs == "logits":
        z = y - y.max(-1, keepdims=True)
        e = np.exp(z)
        p = e / e.sum(-1, keepdims=True)
        h = np.log(e.sum(-1)) - (p * z).sum(-1)
        m = p.mean(0)
        total = -np.where(m > 0, m * np.log(np.where(m > 0, m, 1.0)), 0.0).sum(-1)
    else:
        h = -(y * np.log(y + 1e-10)).sum(-1)
        m = y.mean(0)
        total = -(m * np.log(m + 1e-10)).sum(-1)
    ale = h.mean(0)
    return m, total, ale, total - ale


def N(t):
    return t.detach().double().cpu().numpy()


def check_against_ref(u, y, inputs, what=""):
    """The issue's tolerances: mean 1e-6; total / aleatoric / epistemic 1e-5 max(1, log C); epistemic >= -1e-5."""
    C = y.shape[-1]
    y = np.asarray(y).reshape(y.shape[0], -1, C)
    m, total, ale, epi = ref64(y, inputs)
    tol = 1e-5 * max(1.0, float(np.log(C)))
    got = [N(t).reshape(r.shape) for t, r in zip(u, (m, total, ale, epi))]
    assert np.abs(got[0] - m).max() <= 1e-6, (what, "mean", np.abs(got[0] - m).max())
    for name, g, r in zip(("total", "aleatoric", "epistemic"), got[1:], (total, ale, epi)):
        assert np.abs(g - r).max() <= tol, (what, name, np.abs(g - r).max(), tol)
    assert got[3].min() >= -1e-5, (what, "epistemic", got[3].min())


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
    assert re.search(r"\bint bnn_mc_uncertainty\s*\(", header)
    assert "bnn_mc_uncertainty" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.bnn_mc_uncertainty is not None
    assert lib.bnn_abi_version() == 2


def test_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    n0 = lib.bnn_launch_count()

    def call(y=one, nparts=1, nsamples=4, rows=8, classes=10, kind=0, mean=one, total=one, ale=one, epi=one):
        return lib.bnn_mc_uncertainty(y, rows * classes, nparts, nsamples, rows, classes, kind, mean, total, ale, epi,
                                      None, 0, None, 0, 1.0, None, None, None)

    assert call(y=None) == -1 and b"NULL" in lib.bnn_last_error()
    for k in ("mean", "total", "ale", "epi"):
        assert call(**{k: None}) == -1
    assert call(nsamples=0) == -2
    assert call(nsamples=65537) == -5
    assert call(classes=0) == -2
    assert call(classes=4097) == -5
    assert call(nparts=0) == -2
    assert call(kind=2) == -5 and b"kind" in lib.bnn_last_error()
    assert call(rows=0) == -2
    assert lib.bnn_mc_uncertainty(one, 10, 1, 4, 8, 10, 0, one, one, one, one, None, 0, None, 0, 1.0, None, None, None) == -2   # overlapping addends
    # a KL tail with a bad description: its own code, nothing launched
    t = (_lib.KlTensor * 1)()
    t[0].mu, t[0].rho, t[0].n, t[0].prior_mu, t[0].prior_sigma = 16, 16, 8, 0.0, 0.1
    assert lib.bnn_mc_uncertainty(one, 80, 1, 4, 8, 10, 0, one, one, one, one, None, 0, t, 1, 1.0, None, one, None) == -1
    assert lib.bnn_launch_count() == n0


class _FakeKl(ops.KlDeferred):
    pass


def _pending_kl():
    h = _FakeKl()
    h.launched, h.done = False, False
    ops._tls.kl_carry = h
    return h


def test_op_refuses_cpu_tensors_and_unknown_inputs_and_leaves_no_kl_carry():
    with pytest.raises(_lib.BnnHipError):
        ops.mc_uncertainty(torch.zeros(2, 3, 4), "logits")
    for bad in (None, "softmax", "LOGITS", 0):
        with pytest.raises(ValueError):
            ops.mc_uncertainty(torch.zeros(2, 3, 4), bad)
    with pytest.raises(ValueError):
        ops.mc_uncertainty(torch.zeros(2, 3, 4))                   # `inputs` is required
    try:
        h = _pending_kl()
        with pytest.raises(_lib.BnnHipError):
            ops.mc_uncertainty(torch.zeros(2, 3, 4), "probs", kl=h)
        assert ops._tls.kl_carry is None
        h = _pending_kl()
        with pytest.raises(ValueError):
            ops.mc_uncertainty(torch.zeros(2, 3, 4), None, kl=h)
        assert ops._tls.kl_carry is None
    finally:
        ops._tls.kl_carry = None


@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_cpu_module_matches_float64_numpy_on_the_same_draws(inputs):
    torch.manual_seed(0)
    net = MLP([6, 12, 5], softmax=inputs == "probs")
    x = torch.randn(7, 6)
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        net.predictive_uncertainty(x, 4, inputs="softmax")           # refused before a draw is consumed
    with pytest.raises(TypeError):
        net.predictive_uncertainty(x, 4)                             # `inputs` is a required keyword
    assert torch.equal(torch.get_rng_state(), state)
    torch.manual_seed(3)
    u = net.predictive_uncertainty(x, 4, inputs=inputs)
    torch.manual_seed(3)
    ys = net.forward_stacked(x, 4)
    assert isinstance(u, ops.PredictiveUncertainty)
    assert u.mean.shape == (7, 5) and u.total.shape == u.aleatoric.shape == u.epistemic.shape == (7,)
    assert all(t.dtype == torch.float32 for t in u)
    m, total, ale, epi = ref64(ys.detach().numpy(), inputs)
    for g, r in zip(u, (m, total, ale, epi)):
        assert np.abs(N(g) - r).max() <= 1e-6
    if inputs == "probs":
        assert abs(u.total.mean().item() - Entropy(-1)(ys.mean(0)).item()) <= 1e-6
    assert len(list(net.layers)) == (4 if inputs == "probs" else 3)   # the model is left as it was


# ------------------------------------------------------------------------------------------------------------------ GPU
DEV = torch.device("cuda:0")

# (S, rows, C): every value of each axis -- S {1, 2, 8, 33, 257, 4096}, rows {1, 7, 512, 4099}, C {2, 10, 16, 17, 100, 1000,
# 4096} -- plus both wide work splits' chunk counts (300, 2048); each case <= 256 MB of input
SWEEP = [(1, 1, 2), (2, 7, 10), (8, 512, 16), (33, 4099, 17), (257, 512, 100), (4096, 1, 1000), (8, 7, 4096), (2, 4099, 1000),
         (33, 7, 4096), (4096, 7, 10), (257, 4099, 2), (1, 512, 4096), (8, 4099, 10), (4096, 1, 4096), (8, 7, 300), (33, 7, 2048)]


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


@gpu
@pytest.mark.parametrize("S,rows,C", SWEEP)
@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_kernel_against_float64(S, rows, C, inputs):
    gen = torch.Generator().manual_seed(S * 7919 + rows * 31 + C)
    y = _logits(S, rows, C, gen) if inputs == "logits" else _probs(S, rows, C, gen)
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    u = ops.mc_uncertainty(y.to(DEV), inputs)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1
    assert u.mean.shape == (rows, C) and u.total.shape == (rows,)
    check_against_ref(u, y.numpy(), inputs, (S, rows, C, inputs))
    # S identical copies of one sample: no disagreement between the draws
    same = ops.mc_uncertainty(y[:1].to(DEV).expand(S, rows, C), inputs)
    assert N(same.epistemic).__abs__().max() <= 1e-5


@gpu
def test_leading_row_dims_and_non_contiguous_input():
    gen = torch.Generator().manual_seed(5)
    y = _logits(6, 3 * 5, 10, gen).view(6, 3, 5, 10)
    yt = y.to(DEV).transpose(1, 2)                                            # (6, 5, 3, 10), not contiguous
    u = ops.mc_uncertainty(yt, "logits")
    assert u.mean.shape == (5, 3, 10) and u.epistemic.shape == (5, 3)
    check_against_ref(u, yt.cpu().contiguous().numpy(), "logits")


@gpu
@pytest.mark.parametrize("parts,S,M,C", [(3, 4, 37, 10), (16, 8, 512, 10), (33, 2, 9, 10), (100, 3, 5, 16), (5, 4, 6, 40),
                                         (40, 2, 3, 1000), (257, 2, 9, 10), (300, 3, 5, 16)])
@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_partial_logits_give_the_bits_of_logits_then_the_kernel(parts, S, M, C, inputs):
    """A fused head's partials (parts, S, M, C) summed in the launch: the same bits as HeadPartials.logits() (bnn_mc_sum over
    the parts: sequential up to 32 addends, four quarters above) followed by the kernel."""
    gen = torch.Generator().manual_seed(parts * 100 + C)
    if inputs == "logits":
        p = torch.randn(parts, S, M, C, generator=gen) * 0.5
    else:
        p = torch.rand(parts, S, M, C, generator=gen) * (2.0 / (parts * C))     # non-negative: the parts sum to a probability-like row
    hp = ops.HeadPartials(p.to(DEV))
    fused = ops.mc_uncertainty(hp, inputs)
    plain = ops.mc_uncertainty(hp.logits(), inputs)
    for a, b in zip(fused, plain):
        assert torch.equal(a, b)


@gpu
def test_bitwise_reproducible():
    gen = torch.Generator().manual_seed(11)
    y = _logits(4096, 16, 1000, gen).to(DEV)                                 # 262 MB
    a = ops.mc_uncertainty(y, "logits")
    b = ops.mc_uncertainty(y, "logits")
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    check_against_ref(a, y.cpu().numpy(), "logits")


def _keys(layer):
    k = layer.weight.draw_key
    return (k.seed, k.stream, k.sample0, k.nsamples, k.epoch_host, k.gen)


@gpu
def test_fused_head_mlp_costs_no_extra_launch():
    from bayesianneuralnetworks_amd.nn import fuse_activations
    lib = _lib.load()
    torch.manual_seed(1)
    net = MLP([784, 1200, 1200, 10], samples=8).to(DEV)
    seeded.pin_streams(net, 1000)
    net.mc_batched = True
    fuse_activations(net, bf16_activations=True, fuse_head=True)
    x = torch.randn(512, 784, device=DEV)
    bnn.set_compute("bf16")
    try:
        with torch.no_grad():
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            u = net.predictive_uncertainty(x, 8, inputs="logits")
            n_unc = lib.bnn_launch_count() - n0
            keys_u = _keys(net.layers[4])
            bnn.manual_seed(4)
            hp = net._forward_batched_stacked(x, 8, 0, _lazy_head=True)
            assert isinstance(hp, ops.HeadPartials)
            logits = hp.logits()
            want = ops.mc_uncertainty(logits, "logits")
            bnn.manual_seed(4)
            n0 = lib.bnn_launch_count()
            pm = net.predictive_mean(x, 8)
            n_pm = lib.bnn_launch_count() - n0
            assert _keys(net.layers[4]) == keys_u
    finally:
        bnn.set_compute("f32")
    assert n_unc == n_pm
    for a, b in zip(u, want):
        assert torch.equal(a, b)
    lg = N(logits)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    assert np.abs(N(u.mean) - (e / e.sum(-1, keepdims=True)).mean(0)).max() <= 1e-6
    assert pm.shape == (512, 10)
    check_against_ref(u, lg, "logits")


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("batched", [True, False])
def test_module_paths_equal_the_op_on_forward_stacked(mode, batched):
    torch.manual_seed(2)
    net = MLP([64, 96, 10], samples=6).to(DEV)
    seeded.pin_streams(net, 1010)
    net.mc_batched = batched
    x = torch.randn(130, 64, device=DEV)
    bnn.set_compute(mode)
    try:
        with torch.no_grad():
            bnn.manual_seed(8)
            u = net.predictive_uncertainty(x, 6, inputs="logits")
            bnn.manual_seed(8)
            ys = net.forward_stacked(x, 6)
            want = ops.mc_uncertainty(ys, "logits")
    finally:
        bnn.set_compute("f32")
    for a, b in zip(u, want):
        assert torch.equal(a, b)
    check_against_ref(u, N(ys), "logits")


def _bcnn(sd, samples):
    """examples/MNIST/model.py:20-33 with this package's layers (ends in Softmax)."""
    from torch.nn import Conv2d, BatchNorm2d, ELU, Softmax, Flatten
    from bayesianneuralnetworks_amd.nn import NormalConv2d

    class BCNN(BayesianNetworkModule):
        def __init__(self):
            super().__init__(1, 10, samples)
            self.layers = torch.nn.Sequential(
                Conv2d(1, 32, 5, padding=2, stride=2), BatchNorm2d(32), ELU(),
                Conv2d(32, 32, 3, padding=1, stride=1), ELU(),
                Conv2d(32, 64, 3, padding=0, stride=2), ELU(),
                NormalConv2d(64, 64, 3, padding=1, stride=2), ELU(), Flatten(),
                NormalLinear(576, 10), Softmax(dim=-1))

        def _forward(self, x):
            return self.layers(x)

    net = BCNN()
    net.load_state_dict(sd, strict=True)
    net.eval()
    return net


@gpu
@pytest.mark.parametrize("batched", [False, True])
def test_mnist_example_net_probs(batched):
    g = load_golden("mnist_bcnn_pretrained")
    sd = {k[4:].replace("__", "."): torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd__")}
    net = _bcnn(sd, 4).to(DEV)
    net.mc_batched = batched
    x = torch.from_numpy(g["x"]).to(DEV)
    with torch.no_grad():
        bnn.manual_seed(6)
        u = net.predictive_uncertainty(x, inputs="probs")
        bnn.manual_seed(6)
        preds = net(x)                                                      # examples/MNIST/uncertainty.py:47
    stacked = torch.stack(preds, dim=0)
    check_against_ref(u, N(stacked), "probs")
    assert abs(u.total.mean().item() - Entropy(dim=-1)(stacked.mean(dim=0)).item()) <= 1e-6


@gpu
def test_epoch_and_kl_tails_in_the_same_launch():
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    shapes = [(300, 40), (300,), (10, 300), (10,)]
    mus = [(torch.randn(s, generator=gen) * 0.1).to(DEV) for s in shapes]
    rhos = [(torch.randn(s, generator=gen) * 0.2 - 3.0).to(DEV) for s in shapes]
    priors = [(0.0, 0.1), (0.0, 0.1), (0.1, 0.5), (0.0, 1.0)]
    y = _logits(8, 512, 10, gen).to(DEV)
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)
    plain = ops.mc_uncertainty(y, "logits")
    h = ops.kl_normal_begin(mus, rhos, priors, n_batches=3.0)
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    u = ops.mc_uncertainty(y, "logits", advance=cell, kl=h)
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1 and h.done
    assert torch.equal(h.out, ops.kl_normal(mus, rhos, priors, 3.0))
    assert int(cell.item()) == 1
    for a, b in zip(u, plain):
        assert torch.equal(a, b)
    with pytest.raises(_lib.BnnHipError):
        ops.mc_uncertainty(y, "logits", kl=h)                                 # finished already
    # the C-ABI: the epoch moves by exactly advance_inc, wide split included
    y2 = _logits(3, 5, 1000, gen).to(DEV)
    outs = [torch.empty(5, 1000, device=DEV)] + [torch.empty(5, device=DEV) for _ in range(3)]
    n0 = lib.bnn_launch_count()
    _lib.check(lib.bnn_mc_uncertainty(_lib.ptr(y2), 5000, 1, 3, 5, 1000, 0, *[_lib.ptr(t) for t in outs], _lib.ptr(cell), 7,
                                      None, 0, 1.0, None, None, _lib.stream_ptr(DEV)), "bnn_mc_uncertainty")
    torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 1 and int(cell.item()) == 8
    check_against_ref(outs, N(y2), "logits")
