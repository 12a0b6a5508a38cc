"""Every conv2d kernel on per-axis geometry: KH != KW, stride_h != stride_w, pad_h != pad_w, dil_h != dil_w, H != W -- and the flat
im2col kernel (k_im2col), which only images past 64 KiB reach.

bnn_conv2d_shape_t carries the four (h, w) pairs separately and every 2-d convolution kernel decodes them separately; a kernel
that read one member of a pair where it meant the other is invisible to cases written with one scalar per pair.  CASES below
is one table of fully anisotropic shapes, each tagged with the paths it is meant for.

CPU (-m "not gpu"): the table can tell the axes apart (float64 F.conv2d with one pair swapped is another output), holds the
edges by name, and every case routes where its tags say (the predicates of ops.py, which ask the built library's host query
bnn_conv2d_dense_images, and the rules of bnn_conv2d_workspace_bytes / launch_im2col).  The oracle pin (orc.conv2d on these cases) is in test_oracle_golden.py.
GPU: every path against float64 F.conv2d fed what the kernel is fed, at the tolerance its square-shaped sibling test holds --
the sibling's own body, called with pairs (test_dense_path.py, test_hip_parity.py, test_flipout_mc.py).  No case is skipped:
a case that does not route where its tag says fails."""
import collections
import json

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, allclose_scaled, assert_close_scaled
import test_dense_path as tdp
import test_flipout_mc as tfm
import test_hip_parity as thp

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _mc, ops
from bayesianneuralnetworks_amd.nn import FlipOutNormalConv2d, NormalConv2d

gpu = pytest.mark.gpu

Case = collections.namedtuple("Case", "tags B C O H W k st pad dil groups")

# tags: dense           k_conv_bf16 on drawn weights: bnn_conv2d_dense_forward (bf16) and bnn_conv2d_dense_forward_x3 (fp32 parity)
#       flipout         its Flipout instantiations: bnn_conv2d_flipout_forward, bnn_conv2d_flipout_forward_x3 (one fused launch) and
#                       the keyed bnn_conv2d_flipout_forward_mc (O = 32 or 64)
#       flipout_x3_two  Flipout in the fp32 parity mode as two bnn_conv2d_dense_forward_x3 launches (O = 128)
#       generic         the generic sampled kernel, no workspace (groups = 2, K % 8 != 0 or O < 16); its backward is torch's on HIP draws
#       panel           k_im2col_img + the fused GEMM forward, k_nchw_to_rows / k_im2col_img / k_col2im backward (image <= 64 KiB)
#       flat            the same through k_im2col: C H W floats past 64 KiB
CASES = [
    #     tags                        B   C    O    H   W   (KH, KW) (sh, sw) (ph, pw) (dh, dw) groups
    Case(("dense", "flipout"),        13, 64,  64,  7,  5,  (3, 2),  (2, 1),  (1, 0),  (1, 2),  1),   # H W % 4 != 0; B = 10 + 3 images
    Case(("dense", "flipout_x3_two"), 9,  128, 128, 4,  6,  (1, 3),  (1, 2),  (0, 1),  (2, 1),  1),   # KH = 1 < KW
    Case(("dense", "flipout_x3_two"), 3,  64,  128, 8,  3,  (3, 1),  (2, 1),  (1, 0),  (2, 1),  1),   # KW = 1 < KH
    Case(("dense", "flipout"),        17, 128, 64,  5,  8,  (2, 3),  (1, 2),  (1, 2),  (2, 1),  1),   # B = 3 x 5 + 2 images
    Case(("dense", "flipout"),        3,  256, 64,  6,  4,  (3, 3),  (1, 2),  (2, 1),  (2, 1),  1),   # C = 256, square window
    Case(("dense", "flipout"),        4,  64,  64,  9,  8,  (2, 1),  (1, 1),  (2, 0),  (1, 1),  1),   # pad_h > dil_h (KH - 1): rows of padding only
    Case(("dense",),                  2,  64,  64,  15, 16, (2, 3),  (2, 1),  (1, 2),  (1, 2),  1),   # OH x OW = 8 x 16 = 128, the pixel limit
    Case(("dense", "flipout"),        3,  128, 64,  3,  7,  (3, 2),  (1, 2),  (0, 1),  (1, 1),  1),   # OH = 1 < OW
    Case(("dense", "flipout_x3_two"), 5,  64,  128, 9,  2,  (2, 2),  (3, 1),  (1, 0),  (2, 1),  1),   # OW = 1 < OH
    Case(("flipout",),                7,  64,  32,  6,  9,  (3, 2),  (1, 2),  (1, 0),  (2, 1),  1),   # O = 32: four keyed samples a workgroup
    Case(("generic",),                3,  4,   6,   9,  7,  (3, 2),  (2, 1),  (2, 0),  (1, 2),  2),   # groups = 2, K = 12
    Case(("generic",),                2,  5,   24,  6,  8,  (2, 3),  (1, 2),  (0, 1),  (2, 1),  1),   # K = 30
    Case(("generic",),                4,  8,   7,   5,  6,  (1, 4),  (1, 2),  (0, 2),  (1, 1),  1),   # O = 7
    Case(("generic",),                2,  16,  32,  8,  5,  (3, 1),  (2, 1),  (1, 0),  (2, 1),  2),   # groups = 2, K = 24
    Case(("panel",),                  3,  8,   16,  7,  6,  (3, 2),  (2, 1),  (1, 0),  (1, 2),  1),
    Case(("panel",),                  2,  16,  24,  5,  9,  (2, 3),  (1, 2),  (2, 1),  (2, 1),  1),
    Case(("panel",),                  4,  24,  40,  4,  10, (1, 3),  (1, 3),  (0, 4),  (1, 1),  1),   # pad_w > dil_w (KW - 1): columns of padding only
    Case(("panel",),                  2,  8,   32,  10, 3,  (5, 1),  (2, 1),  (2, 0),  (1, 1),  1),
    Case(("flat",),                   2,  64,  16,  17, 17, (3, 2),  (2, 1),  (1, 0),  (1, 2),  1),   # 18 496 floats an image
    Case(("flat",),                   2,  8,   16,  48, 47, (2, 3),  (3, 2),  (0, 1),  (2, 1),  1),   # 18 048
    Case(("flat",),                   1,  16,  24,  33, 32, (1, 4),  (2, 3),  (0, 2),  (1, 2),  1),   # 16 896
    Case(("flat",),                   1,  32,  16,  12, 43, (3, 3),  (2, 1),  (1, 2),  (2, 1),  1),   # 16 512
]
PATHS = ("dense", "flipout", "flipout_x3_two", "generic", "panel", "flat")
PAIRS = ("k", "st", "pad", "dil")
# the three images past 64 KiB are given as (64, 17, 17), (8, 48, 47), (16, 33, 32): the first is square, the one case here with
# H = W (a fourth, 12 x 43, stands beside it); its four geometry pairs are unequal like everywhere else
SQUARE_IMAGE_CASES = [c for c in CASES if (c.C, c.H, c.W) == (64, 17, 17)]


def _cid(c, tag=None):
    return "%s-%dx%dx%dx%dx%d-k%dx%d-s%dx%d-p%dx%d-d%dx%d-g%d" % ((tag or "+".join(c.tags), c.B, c.C, c.O, c.H, c.W) + c.k + c.st + c.pad +
                                                                    c.dil + (c.groups,))


def _of(tag):
    return [pytest.param(c, id=_cid(c, tag)) for c in CASES if tag in c.tags]


def _out_hw(c):
    return ((c.H + 2 * c.pad[0] - c.dil[0] * (c.k[0] - 1) - 1) // c.st[0] + 1,
            (c.W + 2 * c.pad[1] - c.dil[1] * (c.k[1] - 1) - 1) // c.st[1] + 1)


def _shape(c, B=None):
    return ops._conv_shape((B or c.B, c.C, c.H, c.W), (c.O, c.C // c.groups) + c.k, c.st, c.pad, c.dil, c.groups)


def _takes_the_panel(c):
    """bnn_conv2d_workspace_bytes > 0: the im2col panel + fused GEMM forward (csrc/bnn_gemm.hip)."""
    K = c.C // c.groups * c.k[0] * c.k[1]
    return c.groups == 1 and K % 8 == 0 and K >= 32 and c.O >= 16


def _panel_backward(c):
    """_SampledConv2d.backward goes through the panel kernels (ops.py)."""
    return c.groups == 1 and (c.C * c.k[0] * c.k[1]) % 8 == 0 and c.O % 8 == 0


def _image_kernel(c):
    """launch_im2col takes k_im2col_img (the image staged in LDS): C H W floats within 64 KiB and 22-bit indices."""
    OH, OW = _out_hw(c)
    K = c.C * c.k[0] * c.k[1]
    return c.C * c.H * c.W * 4 <= 64 * 1024 and OH * OW * (K // 8) < (1 << 22) and K < (1 << 22)


def _images_per_workgroup(c):
    """conv_dense_launch's tile of the bf16 launch (bnn_conv2d_dense_images): images whose 128 rows and bytes fit one workgroup."""
    return ops._conv_lds_images(_shape(c, B=128)[0], _lib.CONV_DENSE)


class _Stub:
    """What the eligibility predicates of ops.py read of a device tensor, without a device."""
    is_cuda, dtype, requires_grad = True, torch.float32, False

    def __init__(self, *shape):
        self.shape = tuple(shape)

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        return 0


# ================================================================================================== CPU: the table
def _reference_pair(c, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(min(c.B, 2), c.C, c.H, c.W, generator=g, dtype=torch.float64)
    w = torch.randn(c.O, c.C // c.groups, *c.k, generator=g, dtype=torch.float64)
    return x, w


def _swapped(c, pair, x, w):
    """float64 conv2d of the case with ONE pair read the other way round (the window: the same weight memory read as (KW, KH))."""
    geo = dict(st=c.st, pad=c.pad, dil=c.dil)
    if pair == "k":
        w = w.reshape(w.shape[0], w.shape[1], w.shape[3], w.shape[2])
    else:
        geo[pair] = geo[pair][::-1]
    try:
        return F.conv2d(x, w, None, geo["st"], geo["pad"], geo["dil"], c.groups)
    except RuntimeError:                                   # the swapped window does not fit the padded image: no output at all
        return None


@pytest.mark.parametrize("c", [pytest.param(c, id=_cid(c)) for c in CASES])
def test_table_distinguishes_the_axes(c):
    """Swapping any one unequal pair gives another shape or moves the float64 output by more than 1e-2 of its scale -- three decades
    above the tightest GPU tolerance below, so a kernel that mixes up an axis cannot pass."""
    x, w = _reference_pair(c)
    true = F.conv2d(x, w, None, c.st, c.pad, c.dil, c.groups)
    assert tuple(true.shape[-2:]) == _out_hw(c)
    unequal = [p for p in PAIRS if getattr(c, p)[0] != getattr(c, p)[1]]
    assert unequal
    for p in unequal:
        alt = _swapped(c, p, x, w)
        assert alt is None or alt.shape != true.shape or not allclose_scaled(alt.numpy(), true.numpy(), 1e-2), (p, c)
    assert c.H != c.W or c in SQUARE_IMAGE_CASES


def test_table_covers_every_pair_on_every_path():
    assert len(SQUARE_IMAGE_CASES) == 1
    for path in PATHS:
        cases = [c for c in CASES if path in c.tags]
        for p in PAIRS:
            n = sum(getattr(c, p)[0] != getattr(c, p)[1] for c in cases)
            assert n >= 2, (path, p, n)
    assert all(set(c.tags) <= set(PATHS) and c.tags for c in CASES)


def test_table_holds_the_edges():
    dense = [c for c in CASES if "dense" in c.tags]

    def some(pred, cases=CASES):
        return any(pred(c) for c in cases)

    assert some(lambda c: c.k[0] == 1 < c.k[1]), "KH = 1 < KW"
    assert some(lambda c: c.k[1] == 1 < c.k[0]), "KW = 1 < KH"
    assert some(lambda c: c.k[0] == 1 < c.k[1], dense) and some(lambda c: c.k[1] == 1 < c.k[0], dense), "... on k_conv_bf16 too"
    assert some(lambda c: c.k[0] % 2 != c.k[1] % 2 and min(c.k) > 1), "an even window on one axis only"
    assert some(lambda c: c.pad[0] == 0 < c.pad[1]) and some(lambda c: c.pad[1] == 0 < c.pad[0]), "padding on one axis only"
    assert some(lambda c: c.pad[0] > c.dil[0] * (c.k[0] - 1) and c.pad[1] <= c.dil[1] * (c.k[1] - 1)), "border rows of padding only"
    assert some(lambda c: c.pad[1] > c.dil[1] * (c.k[1] - 1) and c.pad[0] <= c.dil[0] * (c.k[0] - 1)), "border columns of padding only"
    assert some(lambda c: _out_hw(c)[0] == 1 < _out_hw(c)[1]), "OH = 1 < OW"
    assert some(lambda c: _out_hw(c)[1] == 1 < _out_hw(c)[0]), "OW = 1 < OH"
    assert some(lambda c: (c.H * c.W) % 4 != 0, dense), "H W % 4 != 0: the scalar image fill of k_conv_bf16"
    assert some(lambda c: _out_hw(c)[0] * _out_hw(c)[1] == 128 and _out_hw(c)[0] != _out_hw(c)[1], dense), "OH OW = 128, OH != OW"
    assert some(lambda c: 1 < _images_per_workgroup(c) < c.B and c.B % _images_per_workgroup(c) != 0, dense), "a ragged last image tile"
    assert some(lambda c: c.groups == 2) and some(lambda c: c.groups == 1 and (c.C * c.k[0] * c.k[1]) % 8 != 0) and \
        some(lambda c: c.groups == 1 and c.O < 16), "the three reasons for the generic kernel"


@pytest.mark.parametrize("c", [pytest.param(c, id=_cid(c)) for c in CASES])
def test_table_routes_where_its_tags_say(c):
    """The predicates of ops.py and the rules of bnn_conv2d_workspace_bytes / launch_im2col, on the CPU."""
    sh, OH, OW = _shape(c)
    assert (OH, OW) == _out_hw(c) and OH >= 1 and OW >= 1
    dense = ops.conv_dense_eligible(sh, OH, OW) and ops.conv_dense_x3_eligible(sh, OH, OW)
    assert dense == ("dense" in c.tags), "bnn_conv2d_dense_forward / _x3"
    geo = (c.st, c.pad, c.dil)
    x, mean = _Stub(c.B, c.C, c.H, c.W), _Stub(c.O, c.C // c.groups, *c.k)
    with torch.no_grad():
        if "flipout" in c.tags:
            assert ops.conv2d_flipout_eligible(x, mean, *geo, c.groups), "bnn_conv2d_flipout_forward"
            assert ops.conv2d_flipout_x3_fused_eligible(x, mean, *geo), "bnn_conv2d_flipout_forward_x3"
            for S in MC_SAMPLES:
                assert ops.conv2d_flipout_mc_eligible(x, mean, *geo, c.groups, S, True), ("bnn_conv2d_flipout_forward_mc, shared x", S)
                assert ops.conv2d_flipout_mc_eligible(_Stub(S * c.B, c.C, c.H, c.W), mean, *geo, c.groups, S, False), ("... per-sample x", S)
        if "flipout_x3_two" in c.tags:
            assert not ops.conv2d_flipout_x3_fused_eligible(x, mean, *geo)
            assert ops.conv2d_plain_x3_eligible(x, _Stub(1, *mean.shape), *geo, c.groups, "f32"), "two bnn_conv2d_dense_forward_x3 launches"
    if "generic" in c.tags:
        assert not _takes_the_panel(c) and not _panel_backward(c) and not dense
    if "panel" in c.tags or "flat" in c.tags:
        # (neither implicit GEMM may take the forward from the panel in either compute mode)
        assert _takes_the_panel(c) and _panel_backward(c)
        assert not ops.conv_dense_eligible(sh, OH, OW) and not ops.conv_dense_x3_eligible(sh, OH, OW)
        assert _image_kernel(c) == ("panel" in c.tags), "k_im2col_img within 64 KiB, k_im2col past it"


# A seeded sweep on top of the table, drawn per axis by rejection at collection time: every drawn case is one both implicit GEMMs
# take, none is left out later.
def _sweep_accept(case):
    B, C, O, H, W, k, st, pad, dil, shared = case
    sh, OH, OW = ops._conv_shape((B, C, H, W), (O, C) + k, st, pad, dil, 1)
    return H != W and sum(a != b for a, b in (k, st, pad, dil)) >= 2 and ops.conv_dense_eligible(sh, OH, OW) and \
        ops.conv_dense_x3_eligible(sh, OH, OW)


SWEEP = tdp._random_conv_cases(8, 20261016, per_axis=True, accept=_sweep_accept)
MC_SAMPLES = (1, 2, 3, 8)                                # keyed Flipout: 1, 2 and 4 samples a workgroup, a ragged last group


def test_sweep_is_complete():
    assert len(SWEEP) == 8 and all(_sweep_accept(c) for c in SWEEP)


def test_predicates_answer_as_recorded():
    """golden/conv2d_lds_fit.json: the five predicates' answers from when ops.py did the LDS arithmetic by hand (a strided sweep and,
    per (launch, C, O), the largest image that fits with the next one up) and the bf16 launch's images per workgroup: all unchanged."""
    with open(GOLDEN + "/conv2d_lds_fit.json") as f:
        doc = json.load(f)
    B = doc["B"]
    assert len(doc["cases"]) > 3000
    for C, O, H, W, k, st, pad, dil, g, S, shared, *want in doc["cases"]:
        geo = ((st, st), (pad, pad), (dil, dil))
        x, xs, mean = _Stub(B, C, H, W), _Stub(B if shared else S * B, C, H, W), _Stub(O, C // g, k, k)
        sh, OH, OW = ops._conv_shape(x.shape, mean.shape, *geo, g)
        got = [ops.conv_dense_eligible(sh, OH, OW), ops.conv_dense_x3_eligible(sh, OH, OW), ops.conv2d_flipout_eligible(x, mean, *geo, g),
               ops.conv2d_flipout_x3_fused_eligible(x, mean, *geo) if g == 1 else None,      # (no groups argument: recorded for 1)
               ops.conv2d_flipout_mc_eligible(xs, mean, *geo, g, S, bool(shared)), ops._conv_lds_images(sh, _lib.CONV_DENSE)]
        assert got == want, (C, O, H, W, k, st, pad, dil, g, S, shared)


# ================================================================================================== GPU
@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from oracle import oracle as orc
    return dict(bnn=bnn, lib=_lib.load(), _lib=_lib, ops=ops, orc=orc, dev=torch.device("cuda:0"))


@pytest.fixture(autouse=True)
def _device_epoch_word_starts_at_zero():
    """The oracles here are keyed on device epoch 0 (as in test_hip_parity.py); the compute mode is left as found."""
    from bayesianneuralnetworks_amd._rng import default_generator
    for cell in default_generator._epoch_dev.values():
        cell.zero_()
    yield
    bnn.set_compute("f32")


def _end(env, *tensors):
    for t in tensors:
        assert torch.isfinite(t).all()
    _lib.check_device(env["dev"])


# ---- the LDS-resident implicit GEMM on drawn weights
@gpu
@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_sample_x"])
@pytest.mark.parametrize("c", _of("dense"))
def test_dense_bf16_vs_float64(env, c, shared):
    """bnn_conv2d_dense_forward: draw + ONE contraction, every image against float64 on the device's own bf16 weights, 1e-5."""
    tdp.test_conv_dense_path_vs_oracle(env, c.B, c.C, c.O, c.H, c.W, c.k, c.st, c.pad, c.dil, shared)
    _end(env)


@gpu
@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_sample_x"])
@pytest.mark.parametrize("c", _of("dense"))
def test_dense_x3_f32_vs_float64(env, c, shared):
    """bnn_conv2d_dense_forward_x3 under no_grad: 1e-5 of the output scale against float64; with gradients wanted the panel agrees."""
    tdp.test_conv_f32_mode_without_the_panel_vs_double(env, c.B, c.C, c.O, c.H, c.W, c.k, c.st, c.pad, c.dil, shared)
    _end(env)


@gpu
@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("case", SWEEP, ids=lambda v: "dense_sweep-" + "x".join(str(i) for i in v[:5]))
def test_dense_sweep_per_axis(env, case, mode):
    body = tdp.test_conv_dense_path_vs_oracle if mode == "bf16" else tdp.test_conv_f32_mode_without_the_panel_vs_double
    body(env, *case)
    _end(env)


# ---- Flipout on the same kernel
@gpu
@pytest.mark.parametrize("c", _of("flipout"))
def test_flipout_bf16_one_launch_vs_oracle(env, c):
    """bnn_conv2d_flipout_forward: weights prep + ONE contraction, 1e-5 against the oracle on the bf16 operands."""
    tdp.test_flipout_conv_fused_kernel_vs_oracle(env, c.B, c.C, c.O, (c.H, c.W), c.k, c.st, c.pad, c.dil)
    _end(env)


@gpu
@pytest.mark.parametrize("c", _of("flipout") + _of("flipout_x3_two"))
def test_flipout_x3_f32_vs_float64(env, c):
    """bnn_conv2d_flipout_forward_x3 (O <= 64: one fused contraction) and its two-launch form (O = 128): 1e-5 against float64."""
    tdp.test_flipout_conv_f32_mode_without_the_panel_vs_double(env, c.B, c.C, c.O, (c.H, c.W), c.k, c.st, c.pad, c.dil)
    _end(env)


def _flip_mc_reference(layer, x, S, B, shared, dev):
    mean, std = layer.weight.mean.detach().cpu().double(), layer.weight.stddev.detach().cpu().double()
    x64, ed = x.cpu().double(), tfm._epoch_dev(dev)
    return torch.stack([tfm._flip_conv64(x64 if shared else x64[s * B:(s + 1) * B], mean, std, layer.flip_key, s, ed, layer.stride,
                                         layer.padding, layer.dilation) for s in range(S)])


@gpu
@pytest.mark.parametrize("S", MC_SAMPLES)
@pytest.mark.parametrize("c", _of("flipout"))
def test_flipout_mc_keyed_shared_x(env, c, S):
    """bnn_conv2d_flipout_forward_mc through an mc_batched net, all S samples in one launch on the un-replicated batch: float64 on
    the signs rebuilt from layer.flip_key (the bound of test_flipout_mc.py's conv cases), samples that differ, two launches."""
    dev = env["dev"]
    bnn.set_compute("bf16")
    torch.manual_seed(c.B + c.C + S)
    layer = FlipOutNormalConv2d(c.C, c.O, c.k, stride=c.st, padding=c.pad, dilation=c.dil).to(dev)
    net = tfm.OneLayer(layer, S)
    net.mc_batched = True
    x = torch.randn(c.B, c.C, c.H, c.W, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        y = net.forward_stacked(x)
        key = layer.flip_key
        assert key is not None and key.nsamples == S
        n0 = env["lib"].bnn_launch_count()
        with _mc.McContext(S, c.B):
            y2 = layer(x, sample=False)                              # the recorded key again: the same launches, counted
        assert env["lib"].bnn_launch_count() == n0 + 2, "bf16 [mean | stddev] operand + ONE keyed contraction"
    assert layer.flip_key is key and torch.equal(y2.reshape(y.shape), y)
    err = tfm._scaled_err(y, _flip_mc_reference(layer, x, S, c.B, True, dev))
    assert err <= 2e-2, err
    assert S == 1 or not torch.equal(y[0], y[1])
    _end(env, y)


@gpu
@pytest.mark.parametrize("c", _of("flipout"))
def test_flipout_mc_keyed_per_sample_x(env, c):
    dev = env["dev"]
    S = 3
    bnn.set_compute("bf16")
    torch.manual_seed(c.B + c.O)
    layer = FlipOutNormalConv2d(c.C, c.O, c.k, stride=c.st, padding=c.pad, dilation=c.dil).to(dev)
    x = torch.randn(S * c.B, c.C, c.H, c.W, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad(), _mc.McContext(S, c.B):
        n0 = env["lib"].bnn_launch_count()
        y = layer(x)
        assert env["lib"].bnn_launch_count() == n0 + 2
    y = y.reshape(S, c.B, *y.shape[1:])
    err = tfm._scaled_err(y, _flip_mc_reference(layer, x, S, c.B, False, dev))
    assert err <= 2e-2, err
    _end(env, y)


# ---- the generic sampled kernel and torch's backward on the HIP draws
@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("c", _of("generic"))
def test_generic_sampled_kernel_vs_oracle(env, c, bias, mode):
    """bnn_conv2d_forward_sampled without a workspace: ONE launch, allclose 1e-5 against the oracle's conv2d on the oracle's draw."""
    thp.test_conv_fused_philox_vs_oracle(env, (c.B, c.C, c.H, c.W, c.O, c.k, c.st, c.pad, c.dil, c.groups, bias), mode)
    _end(env)


def _bwd_cfg(c, S, bias, shared):
    return (S, c.B, c.C, c.H, c.W, c.O, c.k, c.st, c.pad, c.dil, bias, shared, c.groups)


@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_sample_x"])
@pytest.mark.parametrize("c", _of("generic"))
def test_generic_torch_backward_on_hip_draws(env, c, shared, mode):
    """_SampledConv2d.backward where the panel does not apply (groups = 2, K % 8 != 0, O % 8 != 0): torch's conv gradients on the
    K1 draws, against float64 autograd -- x, mu, rho and the bias pair."""
    thp.test_sampled_conv2d_backward_vs_float64_autograd(env, _bwd_cfg(c, 2, True, shared), mode)
    _end(env)


# ---- the im2col panel: forward GEMM, rows, col2im
@gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_sample_x"])
@pytest.mark.parametrize("c", _of("panel") + _of("flat"))
def test_panel_sampled_forward_backward(env, c, shared, mode):
    """ops.conv2d_sampled with gradients for x, mu, rho and the bias pair: k_im2col_img (panel) or k_im2col (flat), the fused GEMM,
    k_nchw_to_rows, k_col2im -- y 1e-5 / 2e-2, gradients 2e-5 / 3e-2 (fp32 / bf16) against float64 autograd, >= 7 launches."""
    thp.test_sampled_conv2d_backward_vs_float64_autograd(env, _bwd_cfg(c, 2 if "flat" in c.tags else 3, True, shared), mode)
    _end(env)


@gpu
@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_sample_x"])
@pytest.mark.parametrize("c", _of("panel") + _of("flat"))
def test_panel_plain_forward_backward(env, c, shared):
    """ops.conv2d_plain with gradients for x, w and b through the same panel kernels in fp32: 1e-5 / 2e-5 against float64."""
    thp.test_plain_conv2d_backward_panel_vs_float64_autograd(env, shared, (2, c.B, c.C, c.H, c.W, c.O, c.k, c.st, c.pad, c.dil))
    _end(env)


# ---- nn/conv.py with tuple arguments
PLUMBING = [pytest.param(c, id=_cid(c, "plumbing_" + t)) for t in ("dense", "generic", "panel", "flat") for c in CASES if t in c.tags][::2]


def _twin_on(dev, cpu, other):
    """`other`, built with the same arguments, with the parameters of `cpu`, on the device (a layer that has sampled holds a non-leaf
    tensor and cannot be deep-copied)."""
    other.load_state_dict(cpu.state_dict())
    return other.to(dev)


@gpu
@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "grad"])
@pytest.mark.parametrize("c", PLUMBING)
def test_plumbing_normal_conv2d_tuple_arguments(env, c, grad):
    """NormalConv2d built with (h, w) tuples: the device output equals the same layer's CPU (_torch_conv) output on the same
    explicit eps, for a batch and for one 3-d image."""
    dev = env["dev"]
    torch.manual_seed(c.B + c.H)
    cpu = NormalConv2d(c.C, c.O, c.k, c.st, c.pad, c.dil, c.groups, True)
    assert (cpu.kernel_size, cpu.stride, cpu.padding, cpu.dilation) == (c.k, c.st, c.pad, c.dil)
    layer = _twin_on(dev, cpu, NormalConv2d(c.C, c.O, c.k, c.st, c.pad, c.dil, c.groups, True))
    g = torch.Generator().manual_seed(9)
    ew, eb = torch.randn(cpu.weight.mean.shape, generator=g), torch.randn(c.O, generator=g)
    x = torch.randn(c.B, c.C, c.H, c.W, generator=g)
    cpu.weight.sample_with_eps(ew)
    cpu.bias.sample_with_eps(eb)
    layer.weight.sample_with_eps(ew.to(dev))
    layer.bias.sample_with_eps(eb.to(dev))
    with torch.no_grad():
        want, want3 = cpu(x, sample=False), cpu(x[0], sample=False)
    assert want.shape[-2:] == _out_hw(c) and want3.dim() == 3
    with torch.set_grad_enabled(grad):
        y, y3 = layer(x.to(dev), sample=False), layer(x[0].to(dev), sample=False)
    assert y.requires_grad == grad
    assert_close_scaled(y.detach().cpu().numpy(), want.numpy(), 1e-5, "NormalConv2d %s" % (c,))
    assert_close_scaled(y3.detach().cpu().numpy(), want3.numpy(), 1e-5, "NormalConv2d, one 3-d image %s" % (c,))
    _end(env, y, y3)


@gpu
@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "grad"])
@pytest.mark.parametrize("c", [q for q in PLUMBING if q.values[0].groups == 1])      # (the reference's sign tensor S has C / groups channels)
def test_plumbing_flipout_conv2d_tuple_arguments(env, c, grad):
    """FlipOutNormalConv2d built with (h, w) tuples: the device output equals the same layer's CPU output on the same signs."""
    dev = env["dev"]
    torch.manual_seed(c.B + c.W)
    cpu = FlipOutNormalConv2d(c.C, c.O, c.k, c.st, c.pad, c.dil, c.groups)
    assert (cpu.kernel_size, cpu.stride, cpu.padding, cpu.dilation) == (c.k, c.st, c.pad, c.dil)
    layer = _twin_on(dev, cpu, FlipOutNormalConv2d(c.C, c.O, c.k, c.st, c.pad, c.dil, c.groups))
    x = torch.randn(c.B, c.C, c.H, c.W, generator=torch.Generator().manual_seed(10))
    cpu.sample(c.B, (1, 1))
    layer.R, layer.S = cpu.R.to(dev), cpu.S.to(dev)
    with torch.no_grad():
        want = cpu(x, sample=False)
    with torch.set_grad_enabled(grad):
        y = layer(x.to(dev), sample=False)
    assert y.requires_grad == grad and want.shape[-2:] == _out_hw(c)
    assert_close_scaled(y.detach().cpu().numpy(), want.numpy(), 1e-5, "FlipOutNormalConv2d %s" % (c,))
    _end(env, y)
