"""MC dropout on the MC-batched device path (bnn_mc_dropout, bnn_mc_dropout_backward, bnn_dense_forward_dropout; ops.mc_dropout,
ops.linear_mc_dropout; MCDropoutLinear / MCDropoutConvNd inside an McContext) -- the reference's Titanic example
(examples/Titanic/model.py, train.py) with a mask of its own for every MC sample.

CPU: a NumPy twin of the dropout-mask contract (include/bnn_hip.h) on the oracle's Philox core, its statistics and edge
cases, the argument errors of every new C-ABI entry, and the unchanged serial CPU path.
GPU: the Titanic-shaped net against float64 on the twin's masks (forward, uncertainty, training), kernel parity with bit-exact
masks over the dense kernel's tile instantiations, the conv layers, launch counts, graph replay and the drop statistics."""
import ctypes
import math
import re

import numpy as np
import pytest
import seeded
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _rng, ops
from bayesianneuralnetworks_amd._rng import DrawKey
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, MCDropoutLinear, MCDropoutConv1d, MCDropoutConv2d
from oracle import oracle as orc

gpu = pytest.mark.gpu
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN, E_RANGE, E_UNSUPPORTED = -1, -2, -3, -4, -5, -6     # BNN_E_* (include/bnn_hip.h)
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the twin
def philox_np(c, k0, k1, rounds):
    """Philox4x32-`rounds` on arrays of counters: c = (c0, c1, c2, c3) uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & M32 for v in c)
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(rounds):
        p0 = c0 * np.uint64(0xD2511F53)
        p1 = c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def mask_uniforms(seed, stream, sample, epoch_host, epoch_dev, n, gen):
    """The contract's uniform u of elements 0 .. n - 1 of one sample, fp32."""
    e = np.arange(n, dtype=np.uint64)
    ctr1 = np.uint64(((stream << 16) | (sample & 0xFFFF)) & 0xFFFFFFFF)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    if gen == _rng.GEN_PHILOX10_U24:
        nb = (n + 3) // 4
        b = np.arange(nb, dtype=np.uint64)
        w = np.stack(philox_np((b, np.full(nb, ctr1), np.full(nb, epoch_host), np.full(nb, epoch_dev)), k0, k1, 10), 1)
        x = w.reshape(-1)[:n]                                        # word e % 4 of block e / 4
        return (((x >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)   # one rounding, as the fma
    nb = (n + 7) // 8
    b = np.arange(nb, dtype=np.uint64)
    w = np.stack(philox_np((b, np.full(nb, ctr1), np.full(nb, epoch_host), np.full(nb, epoch_dev)), k0, k1, 7), 1)
    word = w[(e >> np.uint64(3)).astype(np.int64), ((e & np.uint64(7)) >> np.uint64(1)).astype(np.int64)]
    h = np.where((e & np.uint64(1)) == 0, word & np.uint64(0xFFFF), word >> np.uint64(16))
    return ((h.astype(np.float64) + 0.5) * 2.0 ** -16).astype(np.float32)


def mask_twin(key, s, epoch_dev, rows, feats, p):
    """keep (rows, feats) bool and the fp32 scale of sample key.sample0 + s (contract: dropped iff u < p, or p == 1)."""
    p32 = np.float32(p)
    u = mask_uniforms(key.seed, key.stream, key.sample0 + s, key.epoch_host, (epoch_dev + key.epoch_dev_delta) & 0xFFFFFFFF,
                      rows * feats, key.gen)
    keep = ~(u < p32) & (p32 < np.float32(1))
    scale = np.float32(1) / (np.float32(1) - p32) if p32 < 1 else np.float32(0)
    return keep.reshape(rows, feats), scale


def apply_twin(x32, keep, scale):
    """fp32: y = keep ? x * scale : 0 (one rounding)."""
    return np.where(keep, x32.astype(np.float32) * scale, np.float32(0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ CPU
def test_twin_philox_is_the_oracle_core():
    rng = np.random.default_rng(3)
    for rounds, fn in ((10, lambda c, k: orc.philox4x32_10(c, k)), (7, lambda c, k: orc.philox4x32_r(c, k, 7))):
        for _ in range(16):
            c = rng.integers(0, 2 ** 32, 4, dtype=np.uint64)
            k = rng.integers(0, 2 ** 32, 2, dtype=np.uint64)
            got = philox_np(tuple(np.array([v]) for v in c), int(k[0]), int(k[1]), rounds)
            want = fn(c.astype(np.uint32), k.astype(np.uint32))
            assert [int(g[0]) for g in got] == [int(v) for v in want]


def test_twin_uniforms_follow_the_contract_layout():
    # element e of the 24-bit stream is word e % 4 of block e / 4; of the 16-bit stream half (e % 2) of word (e % 8) / 2 of
    # block e / 8 -- spelled out with the oracle's one-block calls
    seed, stream, sample, eh, ed = 0x1234_5678_9ABC_DEF0, 7, 3, 11, 2
    key = [seed & 0xFFFFFFFF, seed >> 32]
    u10 = mask_uniforms(seed, stream, sample, eh, ed, 21, _rng.GEN_PHILOX10_U24)
    u7 = mask_uniforms(seed, stream, sample, eh, ed, 21, _rng.GEN_PHILOX7_U16)
    for e in range(21):
        x = orc.philox4x32_10([e // 4, (stream << 16) | sample, eh, ed], key)[e % 4]
        assert u10[e] == np.float32(((int(x) >> 8) + 0.5) * 2.0 ** -24)
        w = int(orc.philox4x32_r([e // 8, (stream << 16) | sample, eh, ed], key, 7)[(e % 8) // 2])
        h = (w & 0xFFFF) if e % 2 == 0 else (w >> 16)
        assert u7[e] == np.float32((h + 0.5) * 2.0 ** -16)


@pytest.mark.parametrize("gen", [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16])
@pytest.mark.parametrize("p", [0.2, 0.5])
def test_twin_drop_fraction(gen, p):
    key = DrawKey(987654321, 42, 0, 1, 5, gen=gen)
    keep, scale = mask_twin(key, 0, 0, 200, 500, p)
    assert abs((1.0 - keep.mean()) - p) < 1e-2
    assert scale == np.float32(1) / np.float32(1 - np.float32(p))


@pytest.mark.parametrize("gen", [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16])
def test_twin_edge_probabilities(gen):
    key = DrawKey(5, 9, 0, 1, 0, gen=gen)
    keep, scale = mask_twin(key, 0, 0, 64, 33, 0.0)
    assert keep.all() and scale == 1.0
    keep, scale = mask_twin(key, 0, 0, 64, 33, 1.0)
    assert not keep.any()


def _rng_arg(nsamples=1, gen=0, stream=3):
    r = _lib.Rng()
    r.seed, r.stream, r.sample0, r.epoch_host, r.epoch_dev_delta, r.epoch_dev, r.generator = 1, stream, 0, 0, 0, None, gen
    return r


FAKE = ctypes.c_void_p(1 << 20)           # never dereferenced: every call below is refused before a launch
FAKE2 = ctypes.c_void_p((1 << 20) + 2)    # 2-B aligned only


def test_mc_dropout_entry_refuses_bad_arguments():
    lib = _lib.load()
    r = ctypes.byref(_rng_arg())
    call = lambda x=FAKE, xs=0, y=FAKE, ys=64, rows=8, f=8, s=2, p=0.5, dt=_lib.F32, rng=r: \
        lib.bnn_mc_dropout(x, xs, y, ys, rows, f, s, p, dt, rng, None)
    assert call(x=None) == E_NULL
    assert call(y=None) == E_NULL
    assert call(rng=None) == E_NULL
    for p in (float("nan"), -0.1, 1.5):
        assert call(p=p) == E_RANGE
    assert call(s=65536) == E_RANGE
    assert call(s=0) == E_SHAPE
    assert call(f=0) == E_SHAPE
    assert call(rows=1 << 20, f=1 << 12, ys=1 << 32) == E_RANGE
    assert call(xs=5) == E_SHAPE                    # neither shared (0) nor a whole sample apart
    assert call(ys=10) == E_SHAPE
    assert call(dt=7) == E_DTYPE
    assert call(x=FAKE2) == E_ALIGN
    bad_stream = ctypes.byref(_rng_arg(stream=1 << 16))
    assert call(rng=bad_stream) == E_RANGE
    assert call(rng=ctypes.byref(_rng_arg(gen=9))) == E_RANGE


def test_mc_dropout_backward_entry_refuses_bad_arguments():
    lib = _lib.load()
    r = ctypes.byref(_rng_arg())
    call = lambda g=FAKE, gs=64, gx=FAKE, gxs=64, rows=8, f=8, s=2, p=0.5, sm=0, rng=r: \
        lib.bnn_mc_dropout_backward(g, gs, gx, gxs, rows, f, s, p, sm, rng, None)
    assert call(g=None) == E_NULL
    assert call(gx=None) == E_NULL
    assert call(rng=None) == E_NULL
    for p in (float("nan"), -1e-3, 1.0001):
        assert call(p=p) == E_RANGE
    assert call(s=70000) == E_RANGE
    assert call(gs=3) == E_SHAPE
    assert call(gxs=3) == E_SHAPE
    assert call(g=FAKE2) == E_ALIGN


def test_dense_forward_dropout_entry_refuses_bad_arguments():
    lib = _lib.load()
    r = ctypes.byref(_rng_arg())
    M, N, K = 32, 64, 64

    def call(x=FAKE, xs=0, w=FAKE, ws=0, ldw=64, b=None, y=FAKE, ys=M * N, ldy=N, s=2, flags=0, p=0.5, rng=r, k=K):
        return lib.bnn_dense_forward_dropout(x, xs, k, w, ws, ldw, b, 0, y, ys, ldy, M, N, k, s, flags, p, rng, None)
    assert call(x=None) == E_NULL
    assert call(w=None) == E_NULL
    assert call(y=None) == E_NULL
    assert call(rng=None) == E_NULL
    for p in (float("nan"), -0.5, 2.0):
        assert call(p=p) == E_RANGE
    assert call(s=65536) == E_RANGE
    assert call(ys=-1) == E_SHAPE
    assert call(ys=N) == E_SHAPE                    # samples overlap
    assert call(y=FAKE2) == E_ALIGN
    assert call(x=FAKE2) == E_UNSUPPORTED           # the dense kernel's 16-B rows
    assert call(k=12) == E_UNSUPPORTED              # K % 8 != 0
    assert call(flags=8) == E_UNSUPPORTED           # unknown flag


def test_drop_prob_is_checked_like_f_dropout():
    for p in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="dropout probability has to be between 0 and 1"):
            ops.check_drop_prob(p)


class Titanic(BayesianNetworkModule):
    """examples/Titanic/model.py"""

    def __init__(self, in_features=9, out_features=2, samples=100):
        super().__init__(in_features, out_features, samples)
        self.layers = torch.nn.Sequential(MCDropoutLinear(in_features, 256, drop_prob=.2), torch.nn.ELU(),
                                          MCDropoutLinear(256, out_features, drop_prob=.2), torch.nn.Softmax(dim=-1))

    def _forward(self, x):
        return self.layers(x)


def test_serial_cpu_path_is_the_reference():
    torch.manual_seed(0)
    first = _rng.new_stream_id()
    net = Titanic(samples=4)
    assert _rng.new_stream_id() == first + 1              # MC-dropout layers take no stream id at construction
    net.mc_batched = True                                 # (a CPU input runs the serial loop anyway)
    x = torch.randn(16, 9)
    torch.manual_seed(11)
    ys = net(x)
    torch.manual_seed(11)
    l1, l2 = net.layers[0].linear, net.layers[2].linear
    for y in ys:
        h = F.elu(F.dropout(F.linear(x, l1.weight, l1.bias), .2, True, False))
        want = torch.softmax(F.dropout(F.linear(h, l2.weight, l2.bias), .2, True, False), -1)
        assert torch.equal(y, want)
    assert net.layers[0].dropout_key is None and net.layers[0]._dropout_stream is None


# ------------------------------------------------------------------------------------------------ GPU helpers
def _epoch_dev(dev):
    return int(_rng.default_generator.epoch_dev(dev)[0].item())


def _mask64(key, s, rows, feats, p, dev):
    keep, scale = mask_twin(key, s, _epoch_dev(dev), rows, feats, p)
    return torch.from_numpy(np.where(keep, np.float64(scale), 0.0))


def _titanic_ref(net, x, S, dev, sample_offset=0):
    """float64 recomputation of the batched Titanic forward on the twin's masks for the layers' recorded keys -> (S, B, 2)."""
    l1, l2 = net.layers[0], net.layers[2]
    x64 = x.detach().cpu().double()
    W1, b1 = l1.linear.weight.detach().cpu().double(), l1.linear.bias.detach().cpu().double()
    W2, b2 = l2.linear.weight.detach().cpu().double(), l2.linear.bias.detach().cpu().double()
    B = x.shape[0]
    outs = []
    for s in range(S):
        h = F.elu(F.linear(x64, W1, b1) * _mask64(l1.dropout_key, s, B, 256, .2, dev))
        outs.append(torch.softmax(F.linear(h, W2, b2) * _mask64(l2.dropout_key, s, B, 2, .2, dev), -1))
    return torch.stack(outs)


def _scaled_err(got, want):
    got, want = got.detach(), want.detach()
    return float((got - want).abs().max() / max(1.0, float(want.abs().max())))


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    yield d
    bnn.set_compute("f32")


# ------------------------------------------------------------------------------------------------ GPU: the bug
@gpu
@pytest.mark.parametrize("mode,S", [("f32", 8), ("f32", 100), ("bf16", 8)])
def test_titanic_batched_samples_differ_and_match_the_twin(dev, mode, S):
    bnn.set_compute(mode)
    torch.manual_seed(1)
    net = Titanic(samples=S).to(dev)
    seeded.pin_streams(net, 1000)
    net.mc_batched = True
    bnn.manual_seed(77)
    x = torch.randn(64, 9, device=dev)
    ys = torch.stack(net(x))
    assert ys.shape == (S, 64, 2)
    flat = ys.reshape(S, -1)
    for a in range(S):
        for b in range(a + 1, S):
            assert not torch.equal(flat[a], flat[b]), (a, b)
    k1, k2 = net.layers[0].dropout_key, net.layers[2].dropout_key
    assert k1 is not None and k2 is not None and k1.stream != k2.stream and k1.nsamples == S
    assert k1.gen == _rng.generator_for(mode)
    want = _titanic_ref(net, x, S, dev)
    err = _scaled_err(ys.double().cpu(), want)
    assert err <= (1e-5 if mode == "f32" else 2e-2), err


@gpu
def test_titanic_predictive_uncertainty_has_epistemic_part(dev):
    torch.manual_seed(2)
    net = Titanic(samples=16).to(dev)
    seeded.pin_streams(net, 1010)
    net.mc_batched = True
    bnn.manual_seed(5)
    x = torch.randn(128, 9, device=dev)
    u = net.predictive_uncertainty(x, inputs="probs")
    ys = _titanic_ref(net, x, 16, dev).float()
    want = ops.uncertainty_f64(ys, "probs")
    assert float(u.epistemic.min()) > 0.0
    for name in ("mean", "total", "aleatoric", "epistemic"):
        g, w = getattr(u, name).double().cpu(), getattr(want, name).double().cpu()
        assert (g - w).abs().max() <= 1e-5 * max(1.0, float(w.abs().max())), name
    m = net.predictive_mean(x)
    assert torch.allclose(m.double().cpu(), _titanic_ref(net, x, 16, dev).mean(0), atol=1e-5)


# ------------------------------------------------------------------------------------------------ GPU: kernel parity
def _key(S, gen, stream=4321, epoch=17, sample0=0):
    return DrawKey(0xDEADBEEF12345678, stream, sample0, S, epoch, gen=gen)


@gpu
@pytest.mark.parametrize("S", [1, 3, 8, 100])
@pytest.mark.parametrize("gen", [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shared", [True, False])
def test_mc_dropout_kernel_is_the_twin(dev, S, gen, dtype, shared):
    R, Fd = 13, 37                                        # ragged: quads straddle rows
    key = _key(S, gen, sample0=5)
    x = torch.randn((R if shared else S * R), Fd, device=dev).to(dtype)
    y = ops.mc_dropout(x, 0.3, key, shared)
    assert y.shape == (S * R, Fd) and y.dtype == dtype
    xs = x.float().cpu().numpy()
    for s in range(S):
        keep, scale = mask_twin(key, s, _epoch_dev(dev), R, Fd, 0.3)
        want = apply_twin(xs if shared else xs[s * R:(s + 1) * R], keep, scale)
        if dtype == torch.bfloat16:
            want = orc.bf16_round(want)
        got = y[s * R:(s + 1) * R].float().cpu().numpy()
        assert np.array_equal(got, want), s


@gpu
@pytest.mark.parametrize("p", [0.0, 1.0])
def test_mc_dropout_edge_probabilities(dev, p):
    x = torch.randn(8, 20, device=dev)
    y = ops.mc_dropout(x, p, _key(3, 0), True)
    want = x.repeat(3, 1) if p == 0.0 else torch.zeros(24, 20, device=dev)
    assert torch.equal(y, want)


@gpu
@pytest.mark.parametrize("shared", [True, False])
def test_mc_dropout_backward_is_mask_times_gradient(dev, shared):
    S, R, Fd = 5, 9, 30
    key = _key(S, 0)
    x = torch.randn((R if shared else S * R), Fd, device=dev, requires_grad=True)
    g = torch.randn(S * R, Fd, device=dev)
    ops.mc_dropout(x, 0.4, key, shared).backward(g)
    gn = g.cpu().numpy()
    parts = []
    for s in range(S):
        keep, scale = mask_twin(key, s, _epoch_dev(dev), R, Fd, 0.4)
        parts.append(apply_twin(gn[s * R:(s + 1) * R], keep, scale))
    if shared:
        want = parts[0].copy()
        for q in parts[1:]:
            want = (want + q).astype(np.float32)                # fp32, sample order
    else:
        want = np.concatenate(parts)
    assert np.array_equal(x.grad.cpu().numpy(), want)


# (M, N, K, S): the 256 x 80 tile (N <= 80), 128 x 160 (N % 80 == 0), 256 x 128 (others), the 64- / 32-row versions of 128 x 160
# (few workgroups), the narrow N <= 16 kernel, and ragged M / N / K-tails (N % 4 != 0: the element-wise mask path)
DENSE_SHAPES = [(100, 64, 72, 3), (512, 1200, 784, 8), (300, 200, 136, 2), (512, 160, 64, 16), (70, 160, 40, 1),
                (33, 10, 24, 5), (77, 203, 200, 3), (129, 81, 520, 2)]


@gpu
@pytest.mark.parametrize("shape", DENSE_SHAPES)
@pytest.mark.parametrize("fan", [True, False])
@pytest.mark.parametrize("gen", [_rng.GEN_PHILOX10_U24, _rng.GEN_PHILOX7_U16])
def test_dense_forward_dropout_parity(dev, shape, fan, gen):
    M, N, K, S = shape
    p = 0.25
    key = _key(S, gen, stream=99)
    torch.manual_seed(M + N + K)
    x = torch.randn((M if fan else S * M), K, device=dev)
    w = torch.randn(N, K, device=dev) / math.sqrt(K)
    b = torch.randn(N, device=dev)
    y = ops.linear_mc_dropout(x, w, b, p, key, fan, "bf16")
    x64 = torch.from_numpy(orc.bf16_round(x.cpu().numpy())).double()
    w64 = torch.from_numpy(orc.bf16_round(w.cpu().numpy())).double()
    h = F.linear(x64, w64, b.cpu().double())
    ones = ops.mc_dropout(torch.ones(M, N, device=dev), p, key, True)       # the standalone mask
    for s in range(S):
        keep, scale = mask_twin(key, s, _epoch_dev(dev), M, N, p)
        hs = h if fan else h[s * M:(s + 1) * M]
        want = hs * torch.from_numpy(np.where(keep, np.float64(scale), 0.0))
        got = y[s * M:(s + 1) * M].double().cpu()
        assert (got - want).abs().max() <= 1e-4 * max(1.0, float(want.abs().max())), s
        zero = (got == 0).numpy()
        assert np.array_equal(zero, ~keep), s                               # the fused mask is the contract's, bit for bit
        assert np.array_equal(zero, (ones[s * M:(s + 1) * M] == 0).cpu().numpy()), s


# ------------------------------------------------------------------------------------------------ GPU: training
@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_titanic_training_gradients(dev, mode):
    bnn.set_compute(mode)
    S, B = 10, 96
    torch.manual_seed(3)
    net = Titanic(samples=S).to(dev)
    seeded.pin_streams(net, 1020)
    net.mc_batched = True
    bnn.manual_seed(9)
    x = torch.randn(B, 9, device=dev)
    t = torch.randint(0, 2, (B,), device=dev)
    preds = net(x)
    loss = torch.stack([F.cross_entropy(pred, t) for pred in preds]).mean()     # examples/Titanic/train.py
    loss.backward()
    # float64 autograd on the twin masks of the recorded keys
    l1, l2 = net.layers[0], net.layers[2]
    ps = [l1.linear.weight, l1.linear.bias, l2.linear.weight, l2.linear.bias]
    ref = [q.detach().cpu().double().requires_grad_(True) for q in ps]
    x64, t64 = x.cpu().double(), t.cpu()
    outs = []
    for s in range(S):
        h = F.elu(F.linear(x64, ref[0], ref[1]) * _mask64(l1.dropout_key, s, B, 256, .2, dev))
        outs.append(F.cross_entropy(torch.softmax(F.linear(h, ref[2], ref[3]) * _mask64(l2.dropout_key, s, B, 2, .2, dev), -1), t64))
    torch.stack(outs).mean().backward()
    tol = 1e-5 if mode == "f32" else 2e-2
    for q, r in zip(ps, ref):
        err = _scaled_err(q.grad.double().cpu(), r.grad)
        assert err <= tol, err


# ------------------------------------------------------------------------------------------------ GPU: conv layers
class ConvNet(BayesianNetworkModule):
    def __init__(self, conv, samples):
        super().__init__(1, 1, samples)
        self.conv = conv

    def _forward(self, x):
        return self.conv(x)


@gpu
@pytest.mark.parametrize("kind", ["2d", "1d"])
def test_mc_dropout_conv_batched(dev, kind):
    S, B = 6, 5
    torch.manual_seed(4)
    if kind == "2d":
        layer = MCDropoutConv2d(3, 4, 3, padding=1, drop_prob=0.3)
        x = torch.randn(B, 3, 7, 6, device=dev)
        conv = F.conv2d
    else:
        layer = MCDropoutConv1d(3, 4, 3, drop_prob=0.3)
        x = torch.randn(B, 3, 11, device=dev)
        conv = F.conv1d
    net = ConvNet(layer, S).to(dev)
    net.mc_batched = True
    rows = []
    hook = layer.conv.register_forward_hook(lambda m, i, o: rows.append(i[0].shape[0]))
    x.requires_grad_(True)
    y = net.forward_stacked(x)
    hook.remove()
    assert rows == [B]                                    # the conv ran once, on the un-replicated batch
    assert y.shape == (S, B) + tuple(y.shape[2:])
    g = torch.randn_like(y)
    y.backward(g)
    key = layer.dropout_key
    w64 = layer.weight.detach().cpu().double().requires_grad_(True)
    b64 = layer.bias.detach().cpu().double().requires_grad_(True)
    x64 = x.detach().cpu().double().requires_grad_(True)
    h = conv(x64, w64, b64, padding=layer.conv.padding)
    Fd = h[0].numel()
    want = torch.stack([h * _mask64(key, s, B, Fd, 0.3, dev).view(h.shape) for s in range(S)])
    assert _scaled_err(y.detach().double().cpu(), want.detach()) <= 1e-5
    want.backward(g.double().cpu())
    for got, ref in ((x.grad, x64.grad), (layer.weight.grad, w64.grad), (layer.bias.grad, b64.grad)):
        assert _scaled_err(got.double().cpu(), ref) <= 1e-5


# ------------------------------------------------------------------------------------------------ GPU: paths, graphs, statistics
class Wide(BayesianNetworkModule):
    def __init__(self, samples):
        super().__init__(64, 32, samples)
        self.layers = torch.nn.Sequential(MCDropoutLinear(64, 128, drop_prob=.2), torch.nn.ReLU(), MCDropoutLinear(128, 32, drop_prob=.2))

    def _forward(self, x):
        return self.layers(x)


@gpu
def test_bf16_forward_is_one_fused_launch_per_layer(dev):
    bnn.set_compute("bf16")
    lib = _lib.load()
    net = Wide(8).to(dev)
    net.mc_batched = True
    x = torch.randn(256, 64, device=dev)
    with torch.no_grad():
        net.forward_stacked(x)                            # first call converts the weights to bf16 once
        torch.cuda.synchronize()
        n0 = lib.bnn_launch_count()
        y = net.forward_stacked(x)
        torch.cuda.synchronize()
    assert lib.bnn_launch_count() == n0 + 2, lib.bnn_launch_count() - n0
    assert y.shape == (8, 256, 32)
    _lib.check_device(dev)


@gpu
def test_captured_graph_replays_draw_fresh_masks(dev):
    x = torch.randn(32, 48, device=dev)
    cell = _rng.default_generator.epoch_dev(dev)
    key = _key(4, 0)
    lib = _lib.load()
    ops.mc_dropout(x, 0.5, key, True)                     # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.mc_dropout(x, 0.5, key, True)
        _lib.check(lib.bnn_rng_advance(ctypes.c_void_p(cell.data_ptr()), 1, _lib.stream_ptr(dev)), "bnn_rng_advance")
    g.replay()
    torch.cuda.synchronize()
    a = y.clone()
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(a, y)
    assert torch.equal(a == 0, torch.from_numpy(np.concatenate(
        [~mask_twin(key, s, _epoch_dev(dev) - 2, 32, 48, 0.5)[0] for s in range(4)])).to(dev))
    _lib.check_device(dev)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_device_drop_fraction(dev, mode):
    bnn.set_compute(mode)
    layer = MCDropoutLinear(100, 100, drop_prob=0.3)
    net = ConvNet(layer, 8).to(dev)
    net.mc_batched = True
    with torch.no_grad():
        layer.linear.bias.fill_(1.0)
        layer.linear.weight.zero_()
        y = net.forward_stacked(torch.randn(100, 100, device=dev))
    frac = float((y == 0).float().mean())
    assert abs(frac - 0.3) < 1e-2, frac
    assert torch.all((y == 0) | (y == np.float32(1) / np.float32(0.7)))
    _lib.check_device(dev)


# ------------------------------------------------------------------------------------------------ the fused epilogue's registers
def _code_object_notes():
    import os
    import subprocess
    import tempfile
    llvm = "/opt/rocm/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not found")
    lib = _lib.LIB_PATH
    notes = ""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([tools[0], "--dump-section=.hip_fatbin=" + fat, lib, os.path.join(d, "lib.so")])
        blob = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]      # one bundle per translation unit
        for i, a in enumerate(starts):
            part, co = os.path.join(d, "b%d.bin" % i), os.path.join(d, "b%d.co" % i)
            open(part, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.check_call([tools[1], "--unbundle", "--type=o", "--input=" + part,
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
            notes += subprocess.check_output([tools[2], "--notes", co]).decode()
    return notes


def test_dropout_epilogue_does_not_spill():
    """Every k_dense_bf16 instantiation with the dropout epilogue keeps the GEMM in registers: the mask must not stretch the
    accumulators' live range (the first version spilled ~1930 VGPRs per lane and ran the layer 8 x slower)."""
    notes = _code_object_notes()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        if "name" in fields:
            kernels[fields["name"]] = fields
    drop = {n: f for n, f in kernels.items() if n.startswith("_ZN3bnn12k_dense_bf16") and n.endswith("Lb1EEEvNS_11DenseParamsE")}
    assert len(drop) == 16, sorted(drop)
    for n, f in drop.items():
        assert int(f.get("vgpr_spill_count", 0)) <= 4 and int(f.get("private_segment_fixed_size", 0)) <= 64, (n, f)


@gpu
def test_unexpected_rows_in_the_batched_pass_raise(dev):
    from bayesianneuralnetworks_amd import _mc
    layer = MCDropoutLinear(8, 16).to(dev)
    with _mc.McContext(4, 8):
        with pytest.raises(RuntimeError, match="mc_batched"):
            layer(torch.randn(5, 8, device=dev))
        assert layer(torch.randn(8, 8, device=dev)).shape == (32, 16)
    assert layer(torch.randn(5, 8, device=dev), sample=False).shape == (5, 16)
