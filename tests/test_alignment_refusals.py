"""Every C entry of include/bnn_hip.h that documents or implements a 16-byte (or wider-than-the-element) alignment requirement
refuses an operand that breaks it -- that operand alone, everything else legal -- with the documented code, a message that names
alignment, and no launch.  Runs without a device ("Operand alignment", lists the rows).

The refusals are host checks on the pointer VALUE; nothing is dereferenced on the host.  Without a device the pointers are plain
integers.  With one they point into a live, zero-filled device buffer (tests/alignment.py's offset_view), each operand with a
region of its own that holds the call's tiny extents many times over: were a check missing, the launch it guards would stay inside
memory this test owns and the assertion on the code would fail -- no stray access.  That buffer holds a finite sentinel and is
bit-identical after every refusal.

Several entries refuse with one compound check ("needs K % 8 == 0, 16-B aligned rows, ...") whose message names alignment whatever
tripped it.  So every sweep ends with a CONTROL: the same call with every operand on 16 bytes gets past the argument checks -- on
a device it launches into the owned buffer and answers BNN_OK; without one it reaches the launch (a non-negative runtime status) or
a later refusal that does not name alignment (no workspace registered)."""
import ctypes

import pytest
import torch

from alignment import SENTINEL, guards_intact, offset_view
from bayesianneuralnetworks_amd import _lib, ops

REGION = 1 << 18                                    # bytes per operand: 256 KiB (the largest operand below is 72 KiB)
M, N, K, S = 8, 8, 8, 1


class Pointers:
    """P(name) -> an address on a 16-byte boundary, one region per name; P(name, off) -> the same address `off` bytes on."""

    def __init__(self):
        self.names = {}
        self.buf = None
        if torch.cuda.is_available():
            base = torch.full((64 * REGION // 4,), SENTINEL, dtype=torch.float32, device="cuda:0")
            self.buf = offset_view(base, 0, guard=64, fill=SENTINEL)      # asserted: inside the allocation, room on both sides
            self.base = self.buf.data_ptr()
            _lib.ensure_workspace(self.buf.device)
        else:
            self.base = 1 << 20
        assert self.base % 16 == 0

    def intact(self):
        """Nothing has written to the owned buffer or its guards (always true without a device: there is no buffer)."""
        if self.buf is None:
            return True
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all()) and guards_intact(self.buf, SENTINEL)

    def refill(self):
        if self.buf is not None:
            torch.cuda.synchronize()
            self.buf.fill_(SENTINEL)

    def __call__(self, name, off=0):
        i = self.names.setdefault(name, len(self.names))
        assert i < 63 and 0 <= off < 16
        return ctypes.c_void_p(self.base + i * REGION + off)


@pytest.fixture(scope="module")
def P():
    return Pointers()


def rng(stream=8):
    return ctypes.byref(_lib.Rng(seed=1, stream=stream))


def refused(call, code, what):
    """`call()` answers `code`, bnn_last_error names alignment, and bnn_launch_count does not move."""
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    rc = call()
    msg = lib.bnn_last_error()
    assert rc == code, (what, rc, code, msg)
    assert names_alignment(msg), (what, msg)
    assert lib.bnn_launch_count() == n0, what


def names_alignment(msg):
    return b"align" in msg or b"16 bytes" in msg or b"16-B" in msg


def sweep(P, build, operands, code, offs=(4, 8)):
    """build(ptr) makes the call from ptr(name) -> pointer.  Each operand in turn is moved by each offset, alone; nothing is
    written; then the control: the same call with every operand on 16 bytes is not refused for its arguments."""
    lib = _lib.load()
    for name in operands:
        for off in offs:
            refused(lambda: build(lambda n: P(n, off if n == name else 0)), code, (build.__name__, name, off))
    assert P.intact(), (build.__name__, "a refused call wrote to the buffer")
    rc = build(lambda n: P(n, 0))
    msg = lib.bnn_last_error()
    if P.buf is not None:
        assert rc == 0, (build.__name__, "control", rc, msg)
    else:
        assert rc >= 0 or not names_alignment(msg), (build.__name__, "control", rc, msg)
    P.refill()
    return lib


F32, BF16C = _lib.COMPUTE_F32, _lib.COMPUTE_BF16
XBF, YBF = _lib.FLAG_X_BF16, _lib.FLAG_Y_BF16


def test_fused_input_gradient_refuses_posterior_and_gy_off_16_bytes(P):
    """bnn_linear_backward_input_sampled: mu_w, rho_w and gy are read in 16-B pieces -> BNN_E_UNSUPPORTED (callers draw W_s and use
    bnn_linear_backward_input, as ops._SampledLinear.backward does)."""
    lib = _lib.load()

    def dgrad_f32(p):
        return lib.bnn_linear_backward_input_sampled(p("gy"), M * N, N, p("mu_w"), p("rho_w"), p("gx"), M * K, K, M, N, K, S, rng(), F32, 0, None)

    def dgrad_bf16(p):
        return lib.bnn_linear_backward_input_sampled(p("gy"), M * N, N, p("mu_w"), p("rho_w"), p("gx"), M * K, K, M, N, K, S, rng(), BF16C,
                                                     XBF | YBF, None)

    sweep(P, dgrad_f32, ("gy", "mu_w", "rho_w"), _lib.E_UNSUPPORTED)
    sweep(P, dgrad_bf16, ("mu_w", "rho_w"), _lib.E_UNSUPPORTED)
    sweep(P, dgrad_bf16, ("gy",), _lib.E_UNSUPPORTED, offs=(2, 8))


def test_weight_gradients_refuse_outputs_off_16_bytes(P):
    """bnn_linear_backward_weight_sampled (g_mu, g_rho) and bnn_linear_backward_weight (gw) store four consecutive k at once when
    K % 4 == 0 -> BNN_E_ALIGN."""
    lib = _lib.load()

    def wgrad_sampled(p):
        return lib.bnn_linear_backward_weight_sampled(p("x"), M * K, K, p("gy"), M * N, N, p("rho_w"), p("g_mu"), p("g_rho"), None, None, None,
                                                      M, N, K, S, rng(), None, None, F32, 0, 0, None)

    def wgrad_plain(p):
        return lib.bnn_linear_backward_weight(p("x"), M * K, K, p("gy"), M * N, N, p("gw"), N * K, M, N, K, S, F32, 0, 0, None)

    sweep(P, wgrad_sampled, ("g_mu", "g_rho"), _lib.E_ALIGN)
    sweep(P, wgrad_plain, ("gw",), _lib.E_ALIGN)


def test_narrow_backward_refuses_every_operand_it_reads_four_at_a_time(P):
    """bnn_linear_backward_narrow_sampled: mu_w, rho_w, g_mu, g_rho on 16 bytes, x and gx on four elements (16 bytes fp32, 8 bytes
    bf16) -> BNN_E_ALIGN, which ops._wgrad_sampled_raw reads as "not here"."""
    lib = _lib.load()

    def narrow(p, flags=0):
        return lib.bnn_linear_backward_narrow_sampled(p("x"), M * K, K, p("gy"), M * N, N, p("mu_w"), p("rho_w"), p("gx"), M * K, K,
                                                      p("g_mu"), p("g_rho"), None, None, None, M, N, K, S, rng(), None, None, flags, 0, None)

    def narrow_bf16(p):
        return narrow(p, XBF | YBF)

    sweep(P, narrow, ("mu_w", "rho_w", "g_mu", "g_rho", "x", "gx"), _lib.E_ALIGN)
    sweep(P, narrow_bf16, ("x", "gx"), _lib.E_ALIGN, offs=(2, 4))


def test_forward_with_bf16_activations_refuses_operands_off_16_bytes(P):
    """bnn_linear_forward_sampled / bnn_linear_forward with BNN_FLAG_X_BF16: the bf16 path exists on 16-B aligned x and weights
    only -> BNN_E_UNSUPPORTED (ops copies such operands)."""
    lib = _lib.load()

    def fwd_sampled(p):
        return lib.bnn_linear_forward_sampled(p("x"), M * K, K, p("mu_w"), p("rho_w"), None, None, p("y"), M * N, N, M, N, K, S, rng(), None,
                                              BF16C, XBF, None)

    def fwd_plain(p):
        return lib.bnn_linear_forward(p("x"), M * K, K, p("w"), N * K, None, 0, p("y"), M * N, N, M, N, K, S, BF16C, XBF, None)

    sweep(P, fwd_sampled, ("mu_w", "rho_w"), _lib.E_UNSUPPORTED)
    sweep(P, fwd_sampled, ("x",), _lib.E_UNSUPPORTED, offs=(2, 8))
    sweep(P, fwd_plain, ("w",), _lib.E_UNSUPPORTED)
    sweep(P, fwd_plain, ("x",), _lib.E_UNSUPPORTED, offs=(2, 8))


def test_draw_once_entries_refuse_rows_off_16_bytes(P):
    """bnn_dense_forward (x, w), bnn_dense_forward_head (the head's weights), bnn_draw_multi (a bf16 output), bnn_split_bf16x3 and bnn_transpose_bf16 (both sides),
    bnn_conv2d_im2col (the panel), bnn_conv2d_dense_forward (the drawn weights)."""
    lib = _lib.load()

    def dense(p):
        return lib.bnn_dense_forward(p("x"), M * K, K, p("w"), N * 64, 64, None, 0, p("y"), M * N, N, M, N, K, S, 0, None)

    sweep(P, dense, ("x", "w"), _lib.E_UNSUPPORTED, offs=(2, 8))

    def dense_head(p):
        return lib.bnn_dense_forward_head(p("x"), M * K, K, p("w"), 24 * 64, 64, None, 0, p("wh"), 10 * 64, 64, None, 0, 10, p("partials"),
                                          M, 24, K, S, 0, None)

    sweep(P, dense_head, ("wh",), _lib.E_UNSUPPORTED, offs=(2, 8))

    def draw(p):
        t = (_lib.DrawTensor * 1)()
        t[0].mu, t[0].rho, t[0].out = p("mu_w").value, p("rho_w").value, p("w").value
        t[0].rows, t[0].cols, t[0].ld, t[0].out_sample_stride, t[0].out_dtype = N, K, 64, N * 64, _lib.BF16
        t[0].rng.seed, t[0].rng.stream = 1, 8
        return lib.bnn_draw_multi(t, 1, S, None, 0, None, None)

    sweep(P, draw, ("w",), _lib.E_ALIGN, offs=(2, 8))

    def split(p):
        return lib.bnn_split_bf16x3(p("x"), M, K, K, p("planes"), 64, M * 64, None)

    def transpose(p):
        return lib.bnn_transpose_bf16(p("w"), N * 64, 64, p("wt"), K * 64, 64, N, K, S, None)

    sweep(P, split, ("x",), _lib.E_UNSUPPORTED)
    sweep(P, split, ("planes",), _lib.E_UNSUPPORTED, offs=(2, 8))
    sweep(P, transpose, ("w", "wt"), _lib.E_UNSUPPORTED, offs=(2, 8))

    sh = _lib.Conv2dShape(B=2, C=8, H=6, W=6, O=8, KH=3, KW=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1, groups=1)

    def im2col(p):
        return lib.bnn_conv2d_im2col(p("x"), 0, ctypes.byref(sh), 1, p("panel"), 0, None)

    sweep(P, im2col, ("panel",), _lib.E_UNSUPPORTED)

    shd = _lib.Conv2dShape(B=2, C=64, H=6, W=6, O=64, KH=3, KW=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1, groups=1)
    assert lib.bnn_conv2d_dense_images(ctypes.byref(shd), _lib.CONV_DENSE, 1, 1) > 0

    def conv_dense(p):
        return lib.bnn_conv2d_dense_forward(p("x"), 0, p("w"), 64 * 576, 576, None, 0, p("y"), 2 * 64 * 36, ctypes.byref(shd), S, 0, None)

    sweep(P, conv_dense, ("w",), _lib.E_UNSUPPORTED, offs=(2, 8))


def test_lrt_and_moment_entries_refuse_outputs_off_16_bytes(P):
    """K10 / K16 / K11: operands on their element, every output (and bnn_moments_sample's moments) on 16 bytes -> BNN_E_ALIGN."""
    lib = _lib.load()

    def lrt_forward(p):
        return lib.bnn_lrt_forward(p("x"), K, p("mu_w"), p("s2_w"), None, None, p("y"), p("v"), M, N, K, S, 0, rng(), F32, 0, None)

    def lrt_dgrad(p):
        return lib.bnn_lrt_backward_input(p("g_m"), p("g_v"), p("mu_w"), p("s2_w"), p("x"), K, p("gx"), M, N, K, F32, 0, None)

    def lrt_wgrad(p):
        return lib.bnn_lrt_backward_weight(p("x"), K, p("g_m"), p("g_v"), p("rho_w"), p("g_mu"), p("g_rho"), None, None, None, M, N, K, F32, 0, None)

    def moments_forward(p):
        return lib.bnn_moments_forward(p("x"), None, K, p("mu_w"), p("s2_w"), None, None, p("y"), p("v"), M, N, K, F32, 0, None)

    def moments_sample(p):
        return lib.bnn_moments_sample(p("m"), p("v"), p("y"), M, N, S, rng(), 0, None)

    sweep(P, lrt_forward, ("y", "v"), _lib.E_ALIGN)
    sweep(P, lrt_dgrad, ("gx",), _lib.E_ALIGN)
    sweep(P, lrt_wgrad, ("g_mu", "g_rho"), _lib.E_ALIGN)
    sweep(P, moments_forward, ("y", "v"), _lib.E_ALIGN)
    sweep(P, moments_sample, ("m", "v", "y"), _lib.E_ALIGN)

    sh3, _ = ops._conv3d_shape((2, 3, 4, 5, 6), (5, 3, 3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 1)

    def conv_lrt_forward(p):
        return lib.bnn_conv3d_lrt_forward(p("x"), 0, p("mu_w"), p("s2_w"), None, None, p("y"), p("v"), ctypes.byref(sh3), S, rng(), F32, None)

    sweep(P, conv_lrt_forward, ("y", "v"), _lib.E_ALIGN)


class _Stub:
    """What the eligibility predicates read of a tensor, at an address no real tensor of that dtype can have."""

    def __init__(self, shape, dtype, ptr):
        self.shape, self.dtype, self._ptr = tuple(shape), dtype, ptr

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        return self._ptr

    def element_size(self):
        return 2 if self.dtype == torch.bfloat16 else 4


def test_lrt_predicates_name_the_reason():
    """ops.lrt_eligible / ops.conv_lrt_eligible answer a reason instead of a launch: an input that is not on its element is
    "input pointer is not aligned to its element size" (any element-aligned address is taken: the K10 / K11 kernels load one
    element at a time, test_operand_alignment.py runs them there) -- and nothing is launched to find that out."""
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    mu = _Stub((7, 20), torch.float32, 4096)
    why = "input pointer is not aligned to its element size"
    assert ops.lrt_eligible(_Stub((33, 20), torch.float32, 4096 + 2), mu, 33, 3) == why
    assert ops.lrt_eligible(_Stub((33, 20), torch.bfloat16, 4096 + 1), mu, 33, 3) == why
    for off in (0, 4, 8):
        assert ops.lrt_eligible(_Stub((33, 20), torch.float32, 4096 + off), mu, 33, 3) is None
    for off in (0, 2, 8):
        assert ops.lrt_eligible(_Stub((33, 20), torch.bfloat16, 4096 + off), mu, 33, 3) is None
    w = _Stub((5, 3, 3, 3), torch.float32, 4096)
    geo = ((1, 1), (1, 1), (1, 1), 1)
    assert ops.conv_lrt_eligible(_Stub((2, 3, 6, 6), torch.float32, 4096 + 2), w, 3, True, *geo) == why
    for off in (0, 4, 8):
        assert ops.conv_lrt_eligible(_Stub((2, 3, 6, 6), torch.float32, 4096 + off), w, 3, True, *geo) is None
    assert lib.bnn_launch_count() == n0


def test_python_predicates_follow_the_pointer():
    """The predicates of ops.py that pick a path by data_ptr() % 16: true on a 16-byte boundary, false 4 (2) and 8 bytes off it --
    two offsets, so that a test of `% 8` cannot stand in for `% 16`."""
    f32, bf = torch.float32, torch.bfloat16
    assert ops.dense_eligible(_Stub((24, 40), f32, 4096)) and ops.flipout_drawable(_Stub((24, 40), f32, 4096))
    for off in (4, 8):
        assert not ops.dense_eligible(_Stub((24, 40), f32, 4096 + off))
        assert not ops.flipout_drawable(_Stub((24, 40), f32, 4096 + off))
        assert not ops._aligned16(_Stub((1,), f32, 4096 + off)) and not ops._aligned16(_Stub((1,), f32, 4096), _Stub((1,), f32, 4096 + off))

    class Dev(_Stub):
        is_cuda, requires_grad = True, False

        def stride(self, i):
            st = [1] * len(self.shape)
            for j in range(len(self.shape) - 2, -1, -1):
                st[j] = st[j + 1] * self.shape[j + 1]
            return st[i]

    Act = Dev
    # the fp32 mode's three-plane dense path: the posterior AND the input on 16 bytes
    assert ops.x3_eligible(Dev((72, 40), f32, 4096), Dev((24, 40), f32, 4096), 72)
    for off in (4, 8):
        assert not ops.x3_eligible(Dev((72, 40), f32, 4096 + off), Dev((24, 40), f32, 4096), 72)
        assert not ops.x3_eligible(Dev((72, 40), f32, 4096), Dev((24, 40), f32, 4096 + off), 72)
    # the one-launch Flipout convolutions (the first `flipout` case of test_conv2d_geometry.CASES): the mean on 16 bytes
    x, geo = Dev((13, 64, 7, 5), f32, 4096), ((2, 1), (1, 0), (1, 2))
    for off, want in ((0, True), (4, False), (8, False)):
        mean = Dev((64, 64, 3, 2), f32, 4096 + off)
        with torch.no_grad():
            assert ops.conv2d_flipout_eligible(x, mean, *geo, 1) == want
            assert ops.conv2d_flipout_x3_fused_eligible(x, mean, *geo) == want
            assert ops.conv2d_flipout_mc_eligible(x, mean, *geo, 1, 3, True) == want
    assert ops.rows_pitch(Act((72, 40), bf, 4096), 40) == (40, 72 * 40)
    for off in (2, 8):
        assert ops.rows_pitch(Act((72, 40), bf, 4096 + off), 40) is None
