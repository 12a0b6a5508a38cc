"""The rounding-aware float64 reference of bf16 layer chains (tests/golden/bf16ref.py), on the CPU: it flags a hidden value next
to a bf16 rounding midpoint and covers both of its roundings; with nothing ambiguous its bound is the accumulation bound; an fp32
model of the device passes it, and a device that is wrong by one bf16 ulp of one weight, one sample's bias, one Flipout sign or
one dropout mask entry does not."""
import pytest
import torch

from bf16ref import bf16_chain_ref64, rne_bf16, ulp_bf16


def _bf(t):
    return t.float().bfloat16().double()


def test_rne_bf16_is_one_rounding():
    g = torch.Generator().manual_seed(0)
    v = torch.randn(100000, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-20, 20, (100000,), generator=g)).double()
    # away from fp32 double rounding, torch's fp32 -> bf16 (RNE) is the reference
    assert torch.equal(rne_bf16(v.float().double()), v.float().bfloat16().double())
    # ties go to even; a value a hair above a midpoint goes up although its fp32 rounding is the midpoint itself
    one = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert rne_bf16(one).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]
    assert one[2].float().double().item() == 1.0 + 2.0 ** -8 and one[2].float().bfloat16().item() == 1.0     # twice: wrong
    assert ulp_bf16(torch.tensor([1.0, 1.5, 2.0, -3.0])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6]


@pytest.mark.parametrize("side", [-1, 1])
def test_a_value_next_to_a_midpoint_is_flagged_and_both_roundings_are_covered(side):
    # layer 1 (K = 1): t = 1 * 1 + b, b = 2^-8 +- 2^-26 -- within fp32 accumulation of the midpoint 1 + 2^-8 of 1 and 1 + 2^-7
    b1 = torch.tensor([2.0 ** -8 + side * 2.0 ** -26], dtype=torch.float64)
    x = torch.ones(1, 1, dtype=torch.float64)
    w1 = torch.ones(1, 1, dtype=torch.float64)
    w2 = torch.tensor([[3.0]], dtype=torch.float64)
    r = bf16_chain_ref64(x, [(w1, b1), (w2, None)])
    assert bool(r["ambiguous"][0].all())
    for h in (1.0, 1.0 + 2.0 ** -7):                       # either rounding of the hidden value, summed in fp32
        dev = torch.tensor(3.0 * h, dtype=torch.float32).double()
        assert abs(dev - r["out"]).item() <= r["bound"].item()
    assert r["slack"].item() == 3.0 * 2.0 ** -7
    # far enough from the midpoint (2^-20 away): not ambiguous, the bound is the accumulation bound alone
    r = bf16_chain_ref64(x, [(w1, b1 + side * 2.0 ** -20), (w2, None)])
    assert not bool(r["ambiguous"][0].any()) and r["slack"].item() == 0.0 and torch.equal(r["bound"], r["acc"])


def _chain(seed, M=16, dims=(64, 48, 40, 10)):
    g = torch.Generator().manual_seed(seed)
    x = _bf(torch.randn(M, dims[0], generator=g))
    layers = [(_bf(torch.randn(o, i, generator=g) / i ** 0.5), torch.randn(o, generator=g).double() * 0.1)
              for i, o in zip(dims[:-1], dims[1:])]
    return x, layers


def _device_model(x, layers, sum_order=1):
    """The device's arithmetic in fp32: bf16 operands, fp32 sums in a summation order of its own, ReLU, bf16 hidden values."""
    h = x.float()
    for i, (w, b) in enumerate(layers):
        w = w.float()
        if sum_order == 1:
            y = h @ w.t()
        else:                                              # k-reversed sequential sums
            y = torch.zeros(h.shape[0], w.shape[0])
            for k in reversed(range(w.shape[1])):
                y = y + h[:, k:k + 1] * w[:, k]
        y = y + b.float() if b is not None else y
        h = y.clamp_min(0).bfloat16().float() if i < len(layers) - 1 else y
    return h.double()


@pytest.mark.parametrize("seed", range(8))
def test_the_bound_holds_for_the_device_model_and_equals_the_accumulation_bound_without_ambiguity(seed):
    x, layers = _chain(seed)
    r = bf16_chain_ref64(x, layers)
    for order in (1, 2):
        assert bool(((_device_model(x, layers, order) - r["out"]).abs() <= r["bound"]).all()), order
    # rows none of whose hidden inputs (any layer) is ambiguous: no slack reaches them, the bound is the accumulation bound
    amb_rows = torch.zeros(x.shape[0], dtype=torch.bool)
    for a in r["ambiguous"]:
        amb_rows |= a.any(1)
    clean = ~amb_rows
    assert bool(clean.any())
    assert bool((r["slack"][clean] == 0).all()) and torch.equal(r["bound"][clean], r["acc"][clean])
    # where the head's own input is ambiguous, the bound exceeds the accumulation bound by the slack that element carries (an
    # ambiguity in layer 1 reaches the head only by making a layer-2 value ambiguous: an unambiguous one rounds one way)
    last = r["ambiguous"][-1].any(1)
    assert bool((r["slack"][last].sum(1) > 0).all()) and bool((r["bound"][last] >= r["acc"][last]).all())


def test_an_exact_chain_has_no_ambiguity_and_a_zero_slack():
    # small positive integers: every sum is exact in fp32 and every hidden value a bf16 number far from a midpoint (and from
    # ReLU's kink at 0, where [-b, b] holds tiny values that round to nonzero bf16 numbers)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(1, 4, (8, 16), generator=g).double()
    layers = [(torch.randint(1, 3, (12, 16), generator=g).double(), torch.randint(1, 3, (12,), generator=g).double()),
              (torch.randint(-2, 3, (5, 12), generator=g).double(), None)]
    r = bf16_chain_ref64(x, layers)
    assert not bool(r["ambiguous"][0].any()) and bool((r["slack"] == 0).all()) and torch.equal(r["bound"], r["acc"])
    assert torch.equal(_device_model(x, layers), r["out"])


def _rejected(dev, r):
    return bool(((dev - r["out"]).abs() > r["bound"]).any())


@pytest.mark.parametrize("seed", range(4))
def test_mutations_are_rejected(seed):
    x, layers = _chain(seed)
    r = bf16_chain_ref64(x, layers)
    assert not _rejected(_device_model(x, layers), r)
    # one head weight one bf16 ulp off (the one on the largest hidden value of row 0)
    hid = _device_model(x, layers[:-1]).clamp_min(0)
    hid = hid.bfloat16().double()
    j = int(hid[0].abs().argmax())
    w = layers[-1][0].clone()
    w[0, j] = w[0, j] + ulp_bf16(w[0, j:j + 1])[0] * torch.sign(w[0, j])
    assert _rejected(_device_model(x, layers[:-1] + [(w, layers[-1][1])]), r)
    # one sample's bias dropped: the same chain drawn for two samples, the device forgets sample 1's head bias
    x2, layers2 = _chain(seed + 100)
    r2 = bf16_chain_ref64(x2, layers2)
    assert not _rejected(_device_model(x2, layers2), r2)
    assert _rejected(_device_model(x2, layers2[:-1] + [(layers2[-1][0], None)]), r2)


@pytest.mark.parametrize("seed", range(4))
def test_a_flipped_flipout_sign_or_dropout_mask_entry_is_rejected(seed):
    g = torch.Generator().manual_seed(seed)
    x, layers = _chain(seed)
    O, K = layers[-1][0].shape
    mu = torch.randn(O, K, generator=g).double() / K ** 0.5
    sd = torch.rand(O, K, generator=g).double() * 0.1 + 0.05
    R = torch.where(torch.rand(O, generator=g) < 0.5, -1.0, 1.0).double()
    S = torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0).double()
    flip_w = lambda R, S: _bf(mu + sd * R[:, None] * S[None, :])
    r = bf16_chain_ref64(x, layers[:-1] + [(flip_w(R, S), None)])
    assert not _rejected(_device_model(x, layers[:-1] + [(flip_w(R, S), None)]), r)
    R2 = R.clone(); R2[0] = -R2[0]
    assert _rejected(_device_model(x, layers[:-1] + [(flip_w(R2, S), None)]), r)
    hid = _device_model(x, layers[:-1]).clamp_min(0).bfloat16().double()
    j = int(hid[0].abs().argmax())
    S2 = S.clone(); S2[j] = -S2[j]
    assert _rejected(_device_model(x, layers[:-1] + [(flip_w(R, S2), None)]), r)
    # dropout: the mask scales hidden layer 1 (keep 1 / (1 - p) or 0) before the head; one entry flipped
    p = 0.25
    mask = torch.where(torch.rand(K, generator=g) < p, 0.0, 1.0 / (1 - p)).double()
    head = (layers[-1][0] * mask[None, :], layers[-1][1])    # a column mask of the head's input is a masked weight column
    r = bf16_chain_ref64(x, layers[:-1] + [head])
    assert not _rejected(_device_model(x, layers[:-1] + [head]), r)
    live = [k for k in range(K) if hid[0, k] != 0]
    k = max(live, key=lambda k: float(hid[0, k].abs()))
    m2 = mask.clone(); m2[k] = 0.0 if m2[k] != 0 else 1.0 / (1 - p)
    assert _rejected(_device_model(x, layers[:-1] + [(layers[-1][0] * m2[None, :], layers[-1][1])]), r)
