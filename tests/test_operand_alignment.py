"""The public device surface on operands that do not start on a 16-byte boundary.

Every tensor the allocator hands out is 256-byte aligned, so the rest of the suite runs the aligned side of every `pointer & 15`
branch of the host wrappers and the kernels.  Here each call is made twice -- on operands as allocated, and on the same values as
tests/alignment.py's offset views (4 and 8 bytes off for fp32, 2 and 8 for bf16, NaN all around) -- with one operand ROLE moved
at a time (the posterior tensors, the input, grad_outputs), then all three together.  Each case asks for

  no exception   a contiguous tensor of the right dtype is a legal operand wherever it starts;
  accuracy       the offset result is held to float64 under the bound the family's own test file uses (imported, not restated);
  bit equality   with the aligned run for everything the RNG contract makes positional (draws, noise, masks), and for a
                 contraction or reduction only where both runs execute the same kernel on the same addends in the same order --
                 each test says why it may ask for that.

DESIGN.md, "Operand alignment", lists what every entry does below 16 bytes and names the test here that runs it."""
import ctypes

import numpy as np
import pytest
import torch

import bwdref
import seeded
import test_evidential as tev
import test_hip_parity as thp
import test_predictive_regression as tpr
import test_predictive_score as tps
import test_predictive_uncertainty as tpu
import test_regression_score as trs
import test_train_step as tts
import test_train_tail as ttt
from alignment import as_param, guards_intact, offset_view, offsets, output_view, same_bits
from conftest import assert_close_scaled
from test_conv2d_geometry import CASES as CONV_CASES

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _rng, ops
from bayesianneuralnetworks_amd._rng import DrawKey

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S = 3
ROLES = ("posterior", "input", "grad", "all")
F32_OFFS = offsets(torch.float32)
BF16_OFFS = offsets(torch.bfloat16)


@pytest.fixture(autouse=True)
def _generator_state_is_put_back():
    """The draws here are keyed explicitly; what the module tests touch of the process-wide generator (seed, draw counter, the
    device epoch words) and the compute mode go back as found."""
    from bayesianneuralnetworks_amd._rng import default_generator as g
    saved = (g._seed, g._torch_seed, g.epoch_host)
    cells = [(c, c.clone()) for c in g._epoch_dev.values()]
    for c in g._epoch_dev.values():
        c.zero_()
    yield
    g._seed, g._torch_seed, g.epoch_host = saved
    for c, was in cells:
        c.copy_(was)
    bnn.set_compute("f32")


def key(stream, mode="f32", nsamples=S):
    return DrawKey(20261019, stream, 0, nsamples, 5, 0, _rng.generator_for(mode))


def off_for(t, i):
    """The i-th offset of t's dtype (bytes)."""
    o = offsets(t.dtype)
    return o[i % len(o)]


class Placer:
    """Puts the operands of one call where the case wants them: the tensors whose role is moved become offset views, the others
    fresh copies as allocated.  role 'all' moves every role and alternates the two offsets, so that no two neighbours share one."""

    def __init__(self, role, which):
        self.role, self.which, self.n = role, which, 0

    def __call__(self, role, t):
        if t is None:
            return None
        t = t.to(DEV)
        if self.role == "aligned" or (self.role != "all" and role != self.role):
            t = t.clone()
            assert t.data_ptr() % 16 == 0
            return t
        i = self.which + (self.n if self.role == "all" else 0)
        self.n += 1
        return offset_view(t, off_for(t, i))

    def al(self, role):
        return self.role == "aligned" or (self.role != "all" and role != self.role)


def launches():
    return _lib.load().bnn_launch_count()


def variants():
    return [pytest.param(r, w, id="%s-%d" % (r, w)) for r in ROLES for w in (0, 1)]


# ===================================================================================================== draws
DRAW_SHAPES = [(24, 40), (5, 12), (3, 7)]       # `regular` when aligned; cols % 4 == 0 only; ragged


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("shape", DRAW_SHAPES, ids=lambda s: "%dx%d" % s)
def test_sample_affine_philox_is_positional(shape, which):
    """bnn_sample_affine_philox (fp32 and bf16 output) and bnn_eps_philox-keyed draws: element e of sample s depends on (key, s, e)
    and the values of mu[e], rho[e] alone.  mu alone, rho alone and both moved: the same bits as from aligned tensors (the entry
    takes its 16-B loads only when both are aligned, csrc/bnn_elementwise.hip launch_philox)."""
    gen = torch.Generator().manual_seed(shape[0] * 100 + shape[1])
    mu, rho, _, _ = seeded.posterior(gen, shape, bias=False)
    mu, rho = mu.to(DEV), rho.to(DEV)
    k = key(11)
    for dt in (torch.float32, torch.bfloat16):
        want = ops._sample_affine_philox_raw(mu, rho, k, dt)
        assert want.shape == (S,) + shape and bool(torch.isfinite(want.float()).all())
        for move_mu, move_rho in ((1, 0), (0, 1), (1, 1)):
            m = offset_view(mu, off_for(mu, which)) if move_mu else mu
            r = offset_view(rho, off_for(rho, which + 1)) if move_rho else rho
            got = ops._sample_affine_philox_raw(m, r, k, dt)
            assert same_bits(got, want), (shape, dt, move_mu, move_rho)


def _draw_specs(N, K, mode):
    gen = torch.Generator().manual_seed(N * 1000 + K)
    mu_w, rho_w, mu_b, rho_b = (t.to(DEV) for t in seeded.posterior(gen, (N, K)))
    return mu_w, rho_w, mu_b, rho_b, key(21, mode), key(22, mode)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("kind", ["bf16", "x3", "flipout"])
@pytest.mark.parametrize("shape", DRAW_SHAPES[:2], ids=lambda s: "%dx%d" % s)
def test_draw_layers_is_positional(shape, kind, which):
    """bnn_draw_multi through ops.draw_layers -- bf16 weights (the `flat` / `regular` paths when aligned, the general body
    otherwise), the three planes of the fp32 draw, a Flipout draw -- and the fp32 bias that rides along: bit-equal wherever mu / rho
    start, padding columns included (they are zeros either way)."""
    N, K = shape
    mode = "f32" if kind == "x3" else "bf16"
    mu_w, rho_w, mu_b, rho_b, kw, kb = _draw_specs(N, K, mode)
    extra = (0, _lib.DRAW_FLIPOUT) if kind == "flipout" else ()

    def draw(mw, rw, mb, rb):
        pre = ops.draw_layers([(mw, rw, mb, rb, kw, kb) + extra], S, x3=(kind == "x3"))[0]
        torch.cuda.synchronize()
        return pre

    want = draw(mu_w, rho_w, mu_b, rho_b)
    assert bool(torch.isfinite(want.w.float()).all()) and want.w.shape[-1] == ops._pad64(K)
    for move in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 1), (1, 1, 1, 1)):
        ts = [offset_view(t, off_for(t, which + i)) if mv else t for i, (t, mv) in enumerate(zip((mu_w, rho_w, mu_b, rho_b), move))]
        got = draw(*ts)
        assert same_bits(got.w, want.w) and same_bits(got.b, want.b), (shape, kind, move)


def test_draw_layers_refuses_ragged_rows_wherever_they_start():
    """cols % 4 != 0 with more than one row is bnn_draw_multi's documented BNN_E_UNSUPPORTED (a Philox block is 4 consecutive
    elements): the same refusal, before any launch, for an aligned and for a moved posterior."""
    mu_w, rho_w, mu_b, rho_b, kw, kb = _draw_specs(3, 7, "bf16")
    for m, r in ((mu_w, rho_w), (offset_view(mu_w, 4), offset_view(rho_w, 8))):
        n0 = launches()
        with pytest.raises(_lib.BnnHipError, match="cols"):
            ops.draw_layers([(m, r, mu_b, rho_b, kw, kb)], S)
        assert launches() == n0


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
def test_tap_major_conv_draw_is_positional(x3, which):
    """A conv weight (8, 8, 3, 3) written tap-major: aligned it takes the LDS-transposing `tapg` items (host: al16(mu), al16(rho)),
    moved the general body's scattered 2-byte stores.  The same bits in the same places."""
    gen = torch.Generator().manual_seed(9)
    mu_w, rho_w, mu_b, rho_b = (t.to(DEV) for t in seeded.posterior(gen, (8, 8, 3, 3)))
    kw, kb = key(23, "f32" if x3 else "bf16"), key(24)

    def draw(mw, rw):
        return ops.draw_layers([(mw.reshape(8, 72), rw.reshape(8, 72), mu_b, rho_b, kw, kb, 9)], S, x3=x3)[0]

    want = draw(mu_w, rho_w)
    for move_mu, move_rho in ((1, 0), (0, 1), (1, 1)):
        got = draw(offset_view(mu_w, off_for(mu_w, which)) if move_mu else mu_w,
                   offset_view(rho_w, off_for(rho_w, which + 1)) if move_rho else rho_w)
        assert same_bits(got.w, want.w) and same_bits(got.b, want.b), (x3, move_mu, move_rho)


@pytest.mark.parametrize("which", [0, 1])
def test_flipout_draw_and_signs_are_positional(which):
    """ops.flipout_draw (fp32, and bf16 zero-padded) on a moved posterior: the same bits; ops.flipout_signs has no tensor operand
    but its output, which may be anywhere (the entry asks for 4 bytes)."""
    mu, rho, _, _, _, _ = _draw_specs(24, 40, "f32")
    k = key(31)
    m, r = offset_view(mu, off_for(mu, which)), offset_view(rho, off_for(rho, which + 1))
    for dt, pad in ((torch.float32, False), (torch.bfloat16, True)):
        want = ops.flipout_draw(mu, rho, k, dt, pad)
        for a, b in ((m, rho), (mu, r), (m, r)):
            assert same_bits(ops.flipout_draw(a, b, k, dt, pad), want)
    want = ops.flipout_signs(k, 1, 64, DEV)
    assert bool((want.abs() == 1).all())
    out = output_view((S, 1, 64), torch.float32, DEV, F32_OFFS[which])
    r_ = ops._rng_struct(k, DEV)
    _lib.check(_lib.load().bnn_flipout_signs(_lib.ptr(out), 64, 1, 64, S, ctypes.byref(r_), _lib.stream_ptr(DEV)), "bnn_flipout_signs")
    torch.cuda.synchronize()
    assert same_bits(out, want) and guards_intact(out)


@pytest.mark.parametrize("which", [0, 1])
def test_mvn_draw_is_positional(which):
    """ops.mvn_draw: w_s = mu + L u_s with keyed, positional uniforms.  mu is read one element at a time in both runs: a moved mu
    gives the aligned run's bits.  `scale` is read in 16-B pieces only where it is aligned (csrc/bnn_mvn.hip, d.vec), and the
    code does not promise one order of the row's products for both forms: a moved scale is held to the float64 twin of
    test_mvn_device.py under that file's bound for the draw."""
    import test_mvn_device as tmv
    gen = torch.Generator().manual_seed(5)
    mu, scale = tmv._posterior(6, 8, gen)
    mu, scale = mu.to(DEV), scale.to(DEV)
    k = key(41)
    want = ops.mvn_draw(mu, scale, k)
    assert same_bits(ops.mvn_draw(offset_view(mu, off_for(mu, which)), scale, k), want)
    got = ops.mvn_draw(mu, offset_view(scale, off_for(scale, which)), k)
    twin, lu = tmv.twin_draws(mu, scale, k, tmv._epoch_dev(DEV))
    bound = tmv.bf16ref.gamma(8 + 1) * (np.abs(mu.double().cpu().numpy()) + lu) + tmv.EPS_L * lu     # (test_mvn_draw_vs_twin's)
    err = np.abs(got.double().cpu().numpy() - twin)
    assert (err <= bound).all(), (float(err.max()), float((err - bound).max()))


# ===================================================================================================== ops.linear_sampled
def linear_plan(M, K, N, mode, shared, x_bf16, y_bf16, relu, al, S=S):
    """What ops._SampledLinear runs for a call whose input requires a gradient, from its own dispatch conditions and the host
    checks of the entries it calls (csrc/bnn_gemm.hip linear_common / bnn_linear_backward_input_sampled, csrc/bnn_linear_bwd.hip
    bnn_linear_backward_narrow_sampled) -> (bwdref spec, forward launches, backward launches).  al: which of 'mu', 'rho', 'x',
    'gy' start on 16 bytes ('x8': x on 8).  S: the number of MC samples (this module's, unless the caller runs another)."""
    bf = mode == "bf16"
    dense = bf and K % 8 == 0 and al["mu"]
    if dense:
        fwd = 2                                                  # bnn_draw_multi + bnn_dense_forward
    elif M >= ops.DRAW_ONCE_MIN_ROWS and N > 16 and K % 8 == 0 and al["mu"] and al["rho"]:
        fwd = 3                                                  # two bnn_sample_affine_philox + bnn_linear_forward
    else:
        fwd = 1                                                  # the fused kernel, or the generic tile kernel
    drawn = dense and not shared and x_bf16 and N > 16 and N % 8 == 0
    g_bf = y_bf16
    gy_al = relu or al["gy"]                                     # the fused ReLU's backward writes a fresh gy
    gx_bf16 = x_bf16 and not shared
    bwd = 1 if relu else 0
    if N <= 16 and K % 4 == 0 and not g_bf and not shared and al["mu"] and al["rho"] and (al["x8"] if x_bf16 else al["x"]):
        return dict(wgrad="narrow", bias_bf16=False, gx="narrow", gx_bf16=gx_bf16), fwd, bwd + 2
    if drawn and g_bf and gx_bf16:
        how, n = "drawn", 2                                      # bnn_transpose_bf16 + bnn_dense_forward
    elif K % 4 == 0 and N % (8 if g_bf else 4) == 0 and (bf or (not g_bf and not gx_bf16)) and al["mu"] and al["rho"] and gy_al:
        how, n = "redraw_bf16" if bf else "redraw_f32", 1
    else:
        how, n = "plain", 2                                      # bnn_sample_affine_philox + bnn_linear_backward_input
    bwd += n + (1 if shared else 0)                              # (a shared input: bnn_mc_sum over the samples)
    tiles = -(-K // 128) * -(-N // 64)
    nsplit = min(S, 8) if tiles < 64 else 1
    assert (nsplit * 2 * N * K + S * N) * 4 <= tts.WS_SLAB_BYTES
    bwd += 1 if nsplit == 1 else 4                               # split: + k_wgrad_reduce, bnn_colsum, bnn_sample_affine_bwd
    return dict(wgrad=mode, bias_bf16=bf and nsplit == 1, gx=how, gx_bf16=gx_bf16), fwd, bwd


def forward64(x, w, b, mode, relu):
    """y = x w^T + b as bwdref's contraction with the bias as the weight of a column of ones -> (ref, bound): gamma_{K + 2} on
    sum |x| |w| + |b|, the operands rounded to bf16 first in the bf16 mode (x here; w is passed rounded)."""
    x, w, b = bwdref.D(x), bwdref.D(w), bwdref.D(b)
    x = x.expand(w.shape[0], -1, -1)
    xa = torch.cat([x, torch.ones_like(x[..., :1])], -1)
    wa = torch.cat([w.transpose(1, 2), b.unsqueeze(1)], 1)
    ref, bound = bwdref.dgrad64(xa, wa, mode == "bf16")
    return (ref.clamp_min(0) if relu else ref), bound


class LinearCase:
    """The operands of one ops.linear_sampled call on the CPU, and what does not depend on where they lie on the device."""

    def __init__(self, M, K, N, mode, shared, x_bf16=False, y_bf16=False, relu=False, seed=0):
        self.M, self.K, self.N, self.mode, self.shared, self.x_bf16, self.y_bf16, self.relu = M, K, N, mode, shared, x_bf16, y_bf16, relu
        gen = torch.Generator().manual_seed(1000 * K + N + seed)
        self.post = seeded.posterior(gen, (N, K))
        x = torch.randn((M, K) if shared else (S, M, K), generator=gen)
        self.x = x.to(torch.bfloat16) if x_bf16 else x
        gy = torch.randn(S, M, N, generator=gen)
        self.gy = gy.to(torch.bfloat16) if y_bf16 else gy
        self.kw, self.kb = key(51, mode), key(52, mode)
        mu_w, rho_w, mu_b, rho_b = (t.to(DEV) for t in self.post)
        self.eps_w, self.eps_b = ops.eps_philox((N, K), self.kw, DEV).cpu(), ops.eps_philox((N,), self.kb, DEV).cpu()
        self.w32 = ops._sample_affine_philox_raw(mu_w, rho_w, self.kw).cpu()
        self.wbf = ops._sample_affine_philox_raw(mu_w, rho_w, self.kw, torch.bfloat16).cpu()
        self.b32 = ops._sample_affine_philox_raw(mu_b, rho_b, self.kb).cpu()
        self.y_ref = forward64(self.x.reshape(-1, M, K), self.wbf if mode == "bf16" else self.w32, self.b32, mode, relu)

    def run(self, place):
        mu_w, rho_w, mu_b, rho_b = (as_param(place("posterior", t)) for t in self.post)
        x = as_param(place("input", self.x))
        gy = place("grad", self.gy)
        al = dict(mu=mu_w.data_ptr() % 16 == 0, rho=rho_w.data_ptr() % 16 == 0, x=x.data_ptr() % 16 == 0, x8=x.data_ptr() % 8 == 0,
                  gy=gy.data_ptr() % 16 == 0)
        spec, fwd, bwd = linear_plan(self.M, self.K, self.N, self.mode, self.shared, self.x_bf16, self.y_bf16, self.relu, al)
        n0 = launches()
        y = ops.linear_sampled(x, mu_w, rho_w, mu_b, rho_b, self.kw, self.kb, self.shared, self.mode, self.relu,
                               torch.bfloat16 if self.y_bf16 else torch.float32)
        n1 = launches()
        grads = torch.autograd.grad(y, (x, mu_w, rho_w, mu_b, rho_b), gy)
        torch.cuda.synchronize()
        n2 = launches()
        return dict(y=y.detach(), grads=grads, spec=spec, fwd=(n1 - n0, fwd), bwd=(n2 - n1, bwd), al=al)

    def check(self, out, what):
        """y and the five gradients of one run under bwdref's bounds for the kernels that run's operands select."""
        bad, ratio = bwdref.compare(out["y"].cpu(), self.y_ref[0], self.y_ref[1], self.y_bf16)
        print("%s: y worst |err| / bound %.4f" % (what, float(ratio.max())))
        assert not bool(bad.any()) and not bool(torch.isnan(ratio).any()), (what, "y", int(bad.sum()), float(ratio.max()))
        assert out["fwd"][0] == out["fwd"][1], (what, "forward launches (got, planned)", out["fwd"], out["al"])
        assert out["bwd"][0] == out["bwd"][1], (what, "backward launches (got, planned)", out["bwd"], out["spec"], out["al"])
        mu_w, rho_w, mu_b, rho_b = self.post
        op = dict(spec=out["spec"], kl=None, x=self.x.reshape(-1, self.M, self.K), g=self.gy, y=out["y"].cpu() if self.relu else None,
                  mu_w=mu_w, rho_w=rho_w, mu_b=mu_b, rho_b=rho_b, eps_w=self.eps_w, eps_b=self.eps_b, w32=self.w32, wbf=self.wbf)
        gx, g_mu_w, g_rho_w, g_mu_b, g_rho_b = out["grads"]
        ref = bwdref.layer_backward(op)
        if self.shared:
            # the input is shared: ops adds the S fp32 partial gradients (bnn_mc_sum) -- bwdref's rule for S more additions of the
            # same addends: gamma_{N + 1 + S} on sum_s |gy_s| |W_s|, gy rounded where the kernel rounds it (bwdref.layer_backward)
            how = out["spec"]["gx"]
            gy64 = bwdref.rne_bf16(bwdref.D(self.gy)) if how == "redraw_bf16" else bwdref.D(self.gy)
            a = (gy64.abs() @ bwdref.D(self.w32 if how in ("plain", "redraw_f32") else self.wbf).abs()).sum(0)
            d = self.N + 1 + S
            ref["gx"] = (ref["gx"][0].sum(0), bwdref.gamma(d) * a + bwdref.gamma(d, bwdref.U64) * a + bwdref.TINY, False)
        got = dict(gx=gx, g_mu_w=g_mu_w, g_rho_w=g_rho_w, g_mu_b=g_mu_b, g_rho_b=g_rho_b)
        worst = bwdref.check({k: v.detach().cpu() for k, v in got.items()}, ref, what)
        print("%s: %s worst |err| / bound %s" % (what, out["spec"], {k: round(v, 4) for k, v in worst.items()}))


LINEAR_SHAPES = {
    "generic": (72, 40, 24),                                    # the fused kernel's tile, ragged in M, K and N
    "narrow": (72, 40, 10),                                     # the one-pass head backward
}


@pytest.mark.parametrize("role,which", variants())
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_sample_x"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(LINEAR_SHAPES))
def test_linear_sampled_forward_and_backward(shape, mode, shared, relu, role, which):
    """ops.linear_sampled with gradients for x, mu, rho and the bias pair.  A moved mu_w / rho_w sends the forward from the
    sampler-paced (fp32) or draw-once dense (bf16) kernel to the generic tile kernel, the narrow head's backward to the general
    kernels (BNN_E_ALIGN is "not here"), and the fused input gradient -- which bnn_linear_backward_input_sampled refuses for a
    moved mu_w, rho_w or gy -- to bnn_sample_affine_philox + bnn_linear_backward_input.  Without the ReLU the moved gy reaches the
    kernels as it is; with it, bnn_relu_backward re-materialises gy first.  The launch counts confirm the path the bound is taken
    for.  The forward of a run whose grad_outputs alone moved is the aligned forward: bit-equal."""
    M, K, N = LINEAR_SHAPES[shape]
    case = LinearCase(M, K, N, mode, shared, relu=relu)
    base = case.run(Placer("aligned", 0))
    case.check(base, "%s aligned" % shape)
    out = case.run(Placer(role, which))
    case.check(out, "%s %s-%d" % (shape, role, which))
    if role == "grad":
        assert same_bits(out["y"], base["y"])


@pytest.mark.parametrize("role,which", variants())
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_sample_x"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_linear_sampled_draw_once_threshold(mode, shared, relu, role, which):
    """M = ops.DRAW_ONCE_MIN_ROWS, where the fp32 mode draws the weights once (bnn_sample_affine_philox) and runs the explicit-
    weight kernel -- unless mu_w or rho_w is moved, then the fused kernel draws in the GEMM.  The same draws either way."""
    case = LinearCase(ops.DRAW_ONCE_MIN_ROWS, 40, 24, mode, shared, relu=relu)
    out = case.run(Placer(role, which))
    case.check(out, "draw-once %s %s-%d" % (mode, role, which))
    if mode == "f32":                                        # (measured launches: three with the draw-once forward, one without)
        assert out["fwd"][0] == (1 if role in ("posterior", "all") else 3)


@pytest.mark.parametrize("role,which", variants())
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_linear_sampled_bf16_activations(relu, role, which):
    """bf16 compute with a bf16 per-sample input and a bf16 output: aligned, the forward reads x in place through the dense kernel
    (ops.rows_pitch) and the input gradient contracts on the drawn weights (ops._dgrad_drawn_raw).  A moved x is copied for the
    dense kernel; a moved bf16 gy is cloned before the LDS-DMA reads it; a moved posterior sends both passes to the fused kernels,
    which take bf16 activations on 16-B aligned operands only -- ops copies what is not."""
    case = LinearCase(72, 40, 24, "bf16", False, x_bf16=True, y_bf16=True, relu=relu)
    base = case.run(Placer("aligned", 0))
    assert base["spec"]["gx"] == "drawn"
    case.check(base, "bf16 activations aligned")
    out = case.run(Placer(role, which))
    case.check(out, "bf16 activations %s-%d" % (role, which))
    if role in ("input", "grad"):
        assert out["spec"]["gx"] == "drawn" and same_bits(out["y"], base["y"])       # the same kernels on a copy of the operand
    if role == "grad" and not relu:
        assert same_bits(out["grads"][0], base["grads"][0])


# ===================================================================================================== one shape each
def _plain_case(seed=0):
    gen = torch.Generator().manual_seed(70 + seed)
    M, K, N = 37, 20, 12
    return (torch.randn(S, M, K, generator=gen), torch.randn(S, N, K, generator=gen) * 0.2, torch.randn(S, N, generator=gen) * 0.1,
            torch.randn(S, M, N, generator=gen))


@pytest.mark.parametrize("role,which", variants())
def test_linear_plain(role, which):
    """ops.linear_plain forward and backward on explicit weights: y, gx, gw, gb against float64 under bwdref's contraction bound
    (gamma_{d} on the sum of |products|, d the contraction length plus the bias or the S samples)."""
    x, w, b, gy = _plain_case()
    put = Placer(role, which)
    xd, wd, bd = as_param(put("input", x)), as_param(put("posterior", w)), as_param(put("posterior", b))
    y = ops.linear_plain(xd, wd, bd, False, "f32")
    gx, gw, gb = torch.autograd.grad(y, (xd, wd, bd), put("grad", gy))
    ref, bound = forward64(x, w, b, "f32", False)
    for name, got, (r, bd_) in (("y", y, (ref, bound)), ("gx", gx, bwdref.dgrad64(bwdref.D(gy), bwdref.D(w), False)),
                               ("gw", gw, bwdref.dgrad64(bwdref.D(gy).transpose(1, 2), bwdref.D(x), False)),
                               ("gb", gb, bwdref.dgrad64(bwdref.D(gy).transpose(1, 2), torch.ones(S, gy.shape[1], 1, dtype=torch.float64), False))):
        bad, ratio = bwdref.compare(got.detach().cpu(), r.reshape(got.shape), bd_.reshape(got.shape), False)
        assert not bool(bad.any()) and not bool(torch.isnan(ratio).any()), (name, role, float(ratio.max()))


@pytest.mark.parametrize("role,which", variants())
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_linear_lrt_is_bit_equal(mode, role, which):
    """ops.linear_lrt: every global load of the K10 kernels is one element wide (csrc/bnn_lrt_tile.hpp lrt_fetch) and their 16-B
    stores go to outputs ops allocates, so a moved operand runs the same kernels on the same addends in the same order: y and all
    five gradients bit-equal to the aligned run, which test_lrt_device.py holds to float64 -- and the noise is positional."""
    import test_lrt_device as tld
    B, K, N = tld.SHAPES[1]                                   # (the first entry is the benchmark's layer: the next one)
    gen = torch.Generator().manual_seed(81)
    post = seeded.posterior(gen, (N, K))
    x, gy = torch.randn(S, B, K, generator=gen), torch.randn(S, B, N, generator=gen)
    k = key(61, mode)
    assert ops.lrt_eligible(x, post[0], B, S) is None

    def run(put):
        ps = [as_param(put("posterior", t)) for t in post]
        xd = as_param(put("input", x))
        y = ops.linear_lrt(xd, *ps, k, False, mode)
        return [y.detach()] + list(torch.autograd.grad(y, [xd] + ps, put("grad", gy)))

    want, got = run(Placer("aligned", 0)), run(Placer(role, which))
    for name, a, b in zip(("y", "gx", "g_mu_w", "g_rho_w", "g_mu_b", "g_rho_b"), got, want):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b), (name, mode, role)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("moved", ["posterior", "input", "all"])
def test_moments_linear_relu_sample_are_bit_equal(moved, which):
    """ops.moments_linear / moments_relu / moments_sample: the K16 kernels fetch like K10's (one element per load), the ReLU is
    elementwise, and bnn_moments_sample -- which refuses moments off 16 bytes -- gets a copy from ops: the same kernels on the
    same values, so every output is bit-equal to the aligned run (held to float64 by test_moment_propagation.py); the samples are
    positional in the key."""
    gen = torch.Generator().manual_seed(91)
    B, K, N = 37, 20, 12
    post = [t.to(DEV) for t in seeded.posterior(gen, (N, K))]
    am, av = torch.randn(B, K, generator=gen).to(DEV), torch.rand(B, K, generator=gen).to(DEV)
    k = key(71)

    def run(put):
        mom = ops.Moments(put(am, "input"), put(av, "input"))
        out = ops.moments_linear(mom, *[put(t, "posterior") for t in post])
        rel = ops.moments_relu(ops.Moments(put(out.mean, "input"), put(out.var, "input")))
        smp = ops.moments_sample(ops.Moments(put(rel.mean, "input"), put(rel.var, "input")), k, S)
        return [out.mean, out.var, rel.mean, rel.var, smp]

    n = [0]

    def mv(t, role):
        if moved not in (role, "all"):
            return t
        n[0] += 1
        return offset_view(t, off_for(t, which + n[0]))

    want, got = run(lambda t, role: t), run(mv)
    for a, b in zip(got, want):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b)


def contraction64(a, b, extra=0):
    """a @ b in float64 with bwdref's bound (bwdref.dgrad64's rule): every addend passes through at most L fp32 additions and one
    product rounding, plus `extra` roundings the caller's operands carry -> gamma_{L + 1 + extra} sum |a| |b|."""
    a, b = bwdref.D(a), bwdref.D(b)
    m = a.abs() @ b.abs()
    d = a.shape[-1] + 1 + extra
    return a @ b, bwdref.gamma(d) * m + bwdref.gamma(d, bwdref.U64) * m + bwdref.TINY


def held(got, ref_bound, what):
    ref, bound = ref_bound
    bad, ratio = bwdref.compare(got.detach().cpu(), ref.reshape(got.shape), bound.reshape(got.shape), False)
    assert not bool(bad.any()) and not bool(torch.isnan(ratio).any()), (what, int(bad.sum()), float(ratio.max()))


@pytest.mark.parametrize("which", [0, 1])
def test_mc_dropout_masks_are_positional(which):
    """ops.mc_dropout (elementwise, keyed masks) on a moved activation, fp32 and bf16: the bits of the aligned run."""
    x = torch.randn(37, 24, generator=torch.Generator().manual_seed(95)).to(DEV)
    k = key(81)
    for t in (x, x.to(torch.bfloat16)):
        want = ops.mc_dropout(t, 0.3, k, True)
        assert same_bits(ops.mc_dropout(offset_view(t, off_for(t, which)), 0.3, k, True), want)


@pytest.mark.parametrize("role,which", variants())
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_linear_mc_dropout_forward_and_backward(mode, role, which):
    """ops.linear_mc_dropout with gradients for x, w and b, one role moved at a time, against float64 on the twin masks of
    test_mc_dropout.py: y = (x w^T + b) mask, mask = keep / (1 - p).  The zeros of y are the contract's mask bit for bit.
    fp32 mode (bnn_linear_forward, then bnn_mc_dropout): bwdref's contraction bound with two more roundings for the scale and the
    product.  bf16 mode (ONE bnn_dense_forward_dropout launch on bf16 copies of x and w, made by ops: the same kernel on the same
    values wherever x, w and b lie): the forward is bit-equal to the aligned run, which test_mc_dropout.py holds to float64.
    Backward (both modes fp32: the masked gradient, then bnn_linear_backward_input / _weight, bnn_colsum): the same bound, the
    masked gradient carrying the two roundings."""
    import test_mc_dropout as tmd
    gen = torch.Generator().manual_seed(95)
    B, K, N, p_ = 37, 24, 12, 0.3
    x, w, b = torch.randn(B, K, generator=gen), torch.randn(N, K, generator=gen) * 0.3, torch.randn(N, generator=gen)
    gy = torch.randn(S * B, N, generator=gen)
    k = key(81)

    def run(put):
        xd, wd, bd = as_param(put("input", x)), as_param(put("posterior", w)), as_param(put("posterior", b))
        y = ops.linear_mc_dropout(xd, wd, bd, p_, k, True, mode)
        return [y.detach()] + list(torch.autograd.grad(y, (xd, wd, bd), put("grad", gy)))

    y0 = run(Placer("aligned", 0))[0]
    y, gx, gw, gb = run(Placer(role, which))
    mask = torch.stack([tmd._mask64(k, s_, B, N, p_, DEV) for s_ in range(S)])                  # (S, B, N)
    assert bool(((y.reshape(S, B, N).cpu() == 0) == (mask == 0)).all())
    if mode == "bf16":
        assert same_bits(y, y0)
    else:
        h, bh = forward64(x.unsqueeze(0), w.unsqueeze(0), b.unsqueeze(0), "f32", False)
        held(y.reshape(S, B, N), (h * mask, (bh + 2 * bwdref.U * h.abs()) * mask + bwdref.TINY), "y")
    g = bwdref.D(gy).reshape(S, B, N) * mask                                                    # carries two roundings
    held(gx, tuple(t.sum(0) for t in contraction64(g, bwdref.D(w).expand(S, N, K), 2 + S)), "gx")
    g2 = g.reshape(S * B, N)
    held(gw, contraction64(g2.t(), bwdref.D(x).repeat(S, 1), 2), "gw")
    held(gb, contraction64(g2.t(), torch.ones(S * B, 1, dtype=torch.float64), 2), "gb")


@pytest.mark.parametrize("role,which", variants())
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_linear_flipout_mc_forward_and_backward(mode, role, which):
    """ops.linear_flipout_mc with gradients for x, mu and rho: W_s = mu + sigma R_s S_s^T is bwdref's sampled layer with
    eps_s = R_s S_s^T (the device's own keyed signs).  The draw is positional (test_flipout_draw_and_signs_are_positional), so
    the reference contracts on the aligned draw; y and gx under bwdref's contraction bound (bf16 mode: operands rounded to bf16
    first, as the dense kernel reads them), g_mu and g_rho under bwdref.wgrad64 (fp32 kernels in both modes)."""
    gen = torch.Generator().manual_seed(97)
    B, K, N = 37, 24, 16
    mu, rho, _, _ = seeded.posterior(gen, (N, K), bias=False)
    x, gy = torch.randn(B, K, generator=gen), torch.randn(S, B, N, generator=gen)
    k = key(91, mode)
    sg = ops.flipout_signs(k, 1, N + K, DEV)[:, 0].double().cpu()                                # (S, N + K): R | S
    eps = sg[:, :N].unsqueeze(2) * sg[:, N:].unsqueeze(1)
    w32 = ops.flipout_draw(mu.to(DEV), rho.to(DEV), k).cpu()
    wbf = ops.flipout_draw(mu.to(DEV), rho.to(DEV), k, torch.bfloat16, pad=True)[:, :, :K].cpu()
    put = Placer(role, which)
    xd, md, rd = as_param(put("input", x)), as_param(put("posterior", mu)), as_param(put("posterior", rho))
    y = ops.linear_flipout_mc(xd, md, rd, k, True, mode)
    gx, g_mu, g_rho = torch.autograd.grad(y, (xd, md, rd), put("grad", gy))
    bf = mode == "bf16"
    xs = (bwdref.rne_bf16(bwdref.D(x)) if bf else bwdref.D(x)).expand(S, B, K)
    held(y, contraction64(xs, bwdref.D(wbf if bf else w32).transpose(1, 2)), "y")
    held(gx, tuple(t.sum(0) for t in contraction64(gy, w32, S)), "gx")                           # (summed over the samples: S more)
    r = bwdref.wgrad64(bwdref.D(x).unsqueeze(0), bwdref.D(gy), bwdref.D(mu), bwdref.D(rho), eps, None, None, False)
    for name, got in (("g_mu", g_mu), ("g_rho", g_rho)):
        held(got, r[name], name)


# ===================================================================================================== ops.conv2d_sampled
def _conv_cfg(c, shared):
    return (S, c.B, c.C, c.H, c.W, c.O, c.k, c.st, c.pad, c.dil, True, shared, c.groups)


def _smallest(tag):
    return min((c for c in CONV_CASES if tag in c.tags), key=lambda c: c.B * c.C * c.H * c.W * c.O * c.k[0] * c.k[1])


CONV_CFGS = {
    "panel": lambda shared: (S, 2, 8, 6, 6, 8, 3, 1, 1, 1, True, shared),         # C 8, O 8, k 3, 6 x 6, B 2: K = 72, the panel backward
    "generic_groups2": lambda shared: _conv_cfg(next(c for c in CONV_CASES if "generic" in c.tags and c.groups == 2), shared),
    "dense": lambda shared: _conv_cfg(_smallest("dense"), shared),
}
CONV_ROLE = dict(x="input", mu_w="posterior", rho_w="posterior", mu_b="posterior", rho_b="posterior", gy="grad")


@pytest.mark.parametrize("role,which", variants())
@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_sample_x"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CONV_CFGS))
def test_conv2d_sampled_forward_and_backward(name, mode, shared, role, which):
    """ops.conv2d_sampled with gradients for x, mu, rho and the bias pair, through the body and the tolerances of
    test_hip_parity.py's own conv backward check (float64 autograd on the oracle's draws), with the operands placed by this file.
    panel: the im2col backward, whose fused input gradient needs an aligned posterior (ops copies a moved one, so the same kernel
    runs on the same values: g_x is bit-equal to the aligned run); generic: groups = 2, torch's backward on the HIP draws; dense:
    the LDS-resident implicit GEMM in the bf16 mode (a moved x is staged with 4-byte loads, a moved mu_w sends the forward to the
    panel).  The forward of a run whose grad_outputs alone moved is the aligned forward: bit-equal."""
    env = dict(orc=__import__("oracle.oracle", fromlist=["oracle"]), dev=DEV, lib=_lib.load(), ops=ops)
    cfg = CONV_CFGS[name](shared)
    y0, g0 = thp.sampled_conv2d_backward_check(env, cfg, mode)
    put = Placer(role, which)
    y1, g1 = thp.sampled_conv2d_backward_check(env, cfg, mode, lambda n, t: put(CONV_ROLE[n], t))
    assert all(bool(torch.isfinite(g).all()) for g in g1)
    if role == "grad":
        assert same_bits(y1, y0)
    if name == "panel" and role == "posterior":
        assert same_bits(g1[0], g0[0])
    _lib.check_device(DEV)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_conv2d_dense_inference_follows_the_posterior(mode, which):
    """Inference on the smallest `dense` shape.  Aligned: the weights are drawn once and the LDS-resident implicit GEMM contracts
    them (bf16), or their three planes (fp32) -- two launches.  A moved posterior is not taken there (ops: mu_w on 16 bytes) nor by
    the panel (the host: al16(mu_w), al16(rho_w)): ONE launch of the generic kernel, the same draws, held to float64 like the
    aligned result.  A moved x stays on the implicit GEMM, which stages the image with 4-byte loads instead of 16-byte
    ones -- what reaches LDS, and everything after, is the same: bit-equal."""
    c = _smallest("dense")
    gen = torch.Generator().manual_seed(41)
    post = seeded.posterior(gen, (c.O, c.C) + c.k)
    x = torch.randn(c.B, c.C, c.H, c.W, generator=gen)
    kw, kb = key(111, mode), key(112, mode)

    def run(put):
        ps = [put("posterior", t) for t in post]
        xd = put("input", x)
        n0 = launches()
        with torch.no_grad():
            y = ops.conv2d_sampled(xd, *ps, kw, kb, True, c.st, c.pad, c.dil, 1, mode)
        torch.cuda.synchronize()
        return y, launches() - n0

    y0, n0 = run(Placer("aligned", 0))
    y1, n1 = run(Placer("posterior", which))
    y2, n2 = run(Placer("input", which))
    assert (n0, n1, n2) == (2, 1, 2), (n0, n1, n2)
    assert bool(torch.isfinite(y1).all()) and same_bits(y2, y0)
    # float64 F.conv2d on the draws of the keys, at the forward tolerance of test_hip_parity.py's sampled conv check
    mu_w, rho_w, mu_b, rho_b = (t.to(DEV) for t in post)
    w64 = ops._sample_affine_philox_raw(mu_w, rho_w, kw).double().cpu()
    b64 = ops._sample_affine_philox_raw(mu_b, rho_b, kb).double().cpu()
    y64 = torch.stack([torch.nn.functional.conv2d(x.double(), w64[s_], b64[s_], c.st, c.pad, c.dil) for s_ in range(S)])
    for y, what in ((y0, "aligned"), (y1, "moved posterior")):
        assert_close_scaled(y.cpu().numpy(), y64.numpy(), thp.CONV2D_TOL[mode][0], "dense conv, " + what)


@pytest.mark.parametrize("which", [0, 1])
def test_conv2d_plain_inference_follows_the_weight(which):
    """ops.conv2d_plain, fp32 inference on one explicit weight of the same shape: aligned, the weight's three planes and the
    implicit GEMM (two launches); a moved weight goes to the explicit-weight kernel, whose panel wants al16(w) too: one launch of
    the generic kernel; both against float64 F.conv2d at test_hip_parity.py's forward tolerance."""
    c = _smallest("dense")
    gen = torch.Generator().manual_seed(43)
    w = torch.randn(1, c.O, c.C, *c.k, generator=gen) * 0.05
    x = torch.randn(c.B, c.C, c.H, c.W, generator=gen).to(DEV)
    out = []
    for wd in (w.to(DEV), offset_view(w.to(DEV), F32_OFFS[which])):
        n0 = launches()
        with torch.no_grad():
            y = ops.conv2d_plain(x, wd, None, True, c.st, c.pad, c.dil, 1, "f32")
        torch.cuda.synchronize()
        out.append((y, launches() - n0))
    assert (out[0][1], out[1][1]) == (2, 1), (out[0][1], out[1][1])
    y64 = torch.nn.functional.conv2d(x.double().cpu(), w[0].double(), None, c.st, c.pad, c.dil)
    for (y, _), what in zip(out, ("aligned", "moved weight")):
        assert_close_scaled(y.reshape(y64.shape).cpu().numpy(), y64.numpy(), thp.CONV2D_TOL["f32"][0], "conv2d_plain, " + what)


# ===================================================================================================== conv3d
@pytest.mark.parametrize("role,which", variants())
def test_conv3d_sampled_is_bit_equal(role, which):
    """ops.conv3d_sampled, the second case of test_conv3d_device._sweep(): the K7 kernels read x, the drawn weights and gy one
    element at a time and ask for element alignment only (csrc/bnn_conv3d.hip), and the draw is positional -- a moved operand
    runs the same kernels on the same addends: y and the gradients are bit-equal to the aligned run, which test_conv3d_device.py
    holds to float64 with its derived bound."""
    import test_conv3d_device as t3
    C, O, vol, k, st, pad, dil, groups, bias, S_, shared = t3._sweep()[1]
    assert bias and S_ == S and shared
    B, tri = 2, (lambda v: (v,) * 3 if isinstance(v, int) else tuple(v))
    k, st, pad, dil = tri(k), tri(st), tri(pad), tri(dil)
    gen = torch.Generator().manual_seed(33)
    post = seeded.posterior(gen, (O, C // groups) + k)
    x = torch.randn((B, C) + vol, generator=gen)
    kw, kb = key(101), key(102)

    def run(put):
        ps = [as_param(put("posterior", t)) for t in post]
        xd = as_param(put("input", x))
        y = ops.conv3d_sampled(xd, *ps, kw, kb, True, st, pad, dil, groups, "f32")
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(34))
        return [y.detach()] + list(torch.autograd.grad(y, [xd] + ps, put("grad", gy)))

    want, got = run(Placer("aligned", 0)), run(Placer(role, which))
    for name, a, b in zip(("y", "gx", "g_mu_w", "g_rho_w", "g_mu_b", "g_rho_b"), got, want):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b), (name, role)


@pytest.mark.parametrize("role,which", variants())
def test_conv3d_flipout_is_bit_equal(role, which):
    """ops.conv3d_flipout, the second case of test_flipout_conv3d_device.SWEEP: the K9 kernels are K7's (element loads of x, the
    [mean | stddev] operand ops draws itself, the signs and gy; element alignment is all the entries ask) -- a moved x, mean,
    scale, sign tensor or gy runs the same kernels on the same addends: y and the three gradients are bit-equal to the aligned
    run, which test_flipout_conv3d_device.py holds to float64 with its derived bound."""
    import test_flipout_conv3d_device as tf3
    C, O, vol, k, st, pad, dil, S_, shared = tf3.SWEEP[1]
    assert S_ == S and not shared
    B, tri = 2, (lambda v: (v,) * 3 if isinstance(v, int) else tuple(v))
    k, st, pad, dil = tri(k), tri(st), tri(pad), tri(dil)
    gen = torch.Generator().manual_seed(35)
    mean, scale, _, _ = seeded.posterior(gen, (O, C) + k, bias=False)
    x = torch.randn((S, B, C) + vol, generator=gen)
    signs = ops.flipout_signs(key(121), B, O + C, DEV).cpu()

    def run(put):
        ps = [as_param(put("posterior", t)) for t in (mean, scale)]
        xd = as_param(put("input", x))
        y = ops.conv3d_flipout(xd, *ps, put("input", signs), S, False, st, pad, dil, "f32")
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(36))
        return [y.detach()] + list(torch.autograd.grad(y, [xd] + ps, put("grad", gy)))

    want, got = run(Placer("aligned", 0)), run(Placer(role, which))
    for name, a, b in zip(("y", "gx", "g_mean", "g_scale"), got, want):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b), (name, role)


@pytest.mark.parametrize("role,which", variants())
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_conv_lrt_is_bit_equal(mode, role, which):
    """ops.convNd_lrt, the second case of test_lrt_conv_device.FWD_CASES: the K11 kernels load x, mu_w, sigma_w^2 and the two
    gradient planes one element at a time and store 16 bytes only to outputs ops allocates; ops.conv_lrt_eligible takes any
    element-aligned x.  The same kernels on the same addends, the noise positional in the key: y and the five gradients are
    bit-equal to the aligned run, which test_lrt_conv_device.py holds to float64."""
    import test_lrt_conv_device as tlc
    case = list(tlc.FWD_CASES.values())[1]
    post = case.params(True, 5)
    x = torch.randn((S, case.B, case.C) + tuple(case.sp), generator=torch.Generator().manual_seed(37))
    k = key(131, mode)
    assert ops.conv_lrt_eligible(x, post[0], S, False, *case.geo) is None

    def run(put):
        ps = [as_param(put("posterior", t)) for t in post]
        xd = as_param(put("input", x))
        y = ops.convNd_lrt(xd, *ps, k, False, *case.geo, mode)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(38))
        return [y.detach()] + list(torch.autograd.grad(y, [xd] + ps, put("grad", gy)))

    want, got = run(Placer("aligned", 0)), run(Placer(role, which))
    for name, a, b in zip(("y", "gx", "g_mu_w", "g_rho_w", "g_mu_b", "g_rho_b"), got, want):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b), (name, mode, role)


# ===================================================================================================== Flipout conv2d
def _flip2d_case():
    c = _smallest("flipout")
    gen = torch.Generator().manual_seed(45)
    mean, scale, _, _ = seeded.posterior(gen, (c.O, c.C) + c.k, bias=False)
    x = torch.randn(c.B, c.C, c.H, c.W, generator=gen)
    sgn = lambda n: (torch.rand(c.B, n, 1, 1, generator=gen) < 0.5).float() * 2 - 1          # noqa: E731
    return c, mean, scale, x, sgn(c.O), sgn(c.C)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("moved", ["scale", "input", "signs", "all"])
def test_conv2d_flipout_one_launch_forms_are_bit_equal(moved, which):
    """The smallest `flipout` case of test_conv2d_geometry.CASES through ops.conv2d_flipout (bf16), ops.conv2d_flipout_x3_fused
    (fp32 planes) and the keyed ops.conv2d_flipout_mc, which the layers take when the MEAN is on 16 bytes.  What else may move:
    the scale / stddev (the tap-major operand is then written by bnn_draw_multi's general body instead of the LDS-transposing
    items: the same bits, test_tap_major_conv_draw_is_positional), x (the image is staged with 4-byte instead of 16-byte loads:
    the same values in LDS) and the sign tensors (ops makes its own contiguous copies).  The contraction is the same kernel on
    the same operands: bit-equal to the aligned run, which test_conv2d_geometry.py holds to float64."""
    c, mean, scale, x, R, Sg = _flip2d_case()
    geo = (c.st, c.pad, c.dil)
    n = [which]

    def mv(t, role):
        t = t.to(DEV)
        if moved != "all" and moved != role:
            return t
        n[0] += 1
        return offset_view(t, off_for(t, n[0]))

    def run(on):
        put = mv if on else (lambda t, role: t.to(DEV))
        m, sc, xd = mean.to(DEV), put(scale, "scale"), put(x, "input")
        std = put(ops.sigma(scale.to(DEV)), "scale")
        with torch.no_grad():
            assert ops.conv2d_flipout_eligible(xd, m, *geo, 1) and ops.conv2d_flipout_x3_fused_eligible(xd, m, *geo)
            return [ops.conv2d_flipout(xd, m, sc, put(R, "signs"), put(Sg, "signs"), *geo),
                    ops.conv2d_flipout_x3_fused(xd, m, std, put(R, "signs"), put(Sg, "signs"), *geo),
                    ops.conv2d_flipout_mc(xd, m, sc, key(141, "bf16"), True, *geo)]

    want, got = run(False), run(True)
    for name, a, b in zip(("conv2d_flipout", "conv2d_flipout_x3_fused", "conv2d_flipout_mc"), got, want):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b), (name, moved)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_flipout_conv2d_layer_with_a_moved_mean(mode, which):
    """FlipOutNormalConv2d at inference with its weight tensors re-seated off 16 bytes: none of the one-launch forms takes a moved
    mean (ops.conv2d_flipout_eligible, _x3_fused_eligible, the pointer test in nn/conv.py in front of conv2d_flipout_x3), so
    the layer runs two ops.conv2d_plain contractions (the mean's on the generic kernel), held to float64 of
    conv(x, mean) + R conv(x S, stddev) at test_hip_parity.py's forward tolerance.  Both `flipout` (O = 64) and
    `flipout_x3_two` (O = 128) shapes, the smallest of each."""
    from bayesianneuralnetworks_amd.nn import FlipOutNormalConv2d
    bnn.set_compute(mode)
    for tag in ("flipout", "flipout_x3_two"):
        c = _smallest(tag)
        torch.manual_seed(7)
        layer = FlipOutNormalConv2d(c.C, c.O, c.k, stride=c.st, padding=c.pad, dilation=c.dil).to(DEV)
        x = torch.randn(c.B, c.C, c.H, c.W, generator=torch.Generator().manual_seed(8)).to(DEV)
        for i, p_ in enumerate((layer.weight.mean, layer.weight.scale)):
            p_.data = offset_view(p_.data, off_for(p_.data, which + i))
        layer.sample(c.B, layer._ones)
        with torch.no_grad():
            y = layer(x, sample=False)
        m64, s64 = layer.weight.mean.detach().double().cpu(), layer.weight.stddev.detach().double().cpu()
        x64, R, Sg = x.double().cpu(), layer.R.double().cpu(), layer.S.double().cpu()
        conv = lambda h, w: torch.nn.functional.conv2d(h, w, None, c.st, c.pad, c.dil)     # noqa: E731
        want = conv(x64, m64) + conv(x64 * Sg, s64) * R
        assert_close_scaled(y.cpu().numpy(), want.numpy(), thp.CONV2D_TOL[mode][0], "FlipOutNormalConv2d %s %s" % (tag, mode))


# ===================================================================================================== MVN layer and KL
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("moved", ["mu", "scale", "grad", "all"])
def test_mvn_draw_layer_and_kl(moved, which):
    """ops.mvn_draw_layer (weight and bias in one launch, with autograd) and ops.mvn_kl on moved means, scales and grad_outputs.
    The kernels read `scale` and write g_scale in 16-B pieces only where both are aligned (csrc/bnn_mvn.hip, d.vec) and the code
    promises no common order for the two forms, so everything is held to float64 under test_mvn_device.py's own bounds: the
    draws to the twin (gamma_{K + 1} (|mu| + L |u|) + EPS_L L |u|), the draw's gradients to float64 autograd of the reference
    expression on the twin's uniforms at 1e-5 of the scale, the KL at 1e-5 relative and its gradients at 2e-5 of the scale."""
    import test_mvn_device as tmv
    from torch.distributions import MultivariateNormal
    O, K = 6, 8
    gen = torch.Generator().manual_seed(5)
    mu_w, sc_w = tmv._posterior(O, K, gen)
    mu_b, sc_b = (t[0] for t in tmv._posterior(1, O, gen))
    kw, kb = key(151), key(152)
    n = [which]

    def mv(t, role):
        t = t.to(DEV)
        if moved in (role, "all"):
            n[0] += 1
            t = offset_view(t, off_for(t, n[0]))
        return t

    ps = [as_param(mv(mu_w, "mu")), as_param(mv(sc_w, "scale")), as_param(mv(mu_b, "mu")), as_param(mv(sc_b, "scale"))]
    w, b = ops.mvn_draw_layer(ps[0], ps[1], ps[2], ps[3], kw, kb)
    ed = tmv._epoch_dev(DEV)
    gws = [torch.randn(w.shape, generator=gen), torch.randn(b.shape, generator=gen)]
    grads = torch.autograd.grad([w, b], ps, [mv(g, "grad") for g in gws])
    for got, m_, s_, k_, Kc in ((w, mu_w, sc_w, kw, K), (b, mu_b, sc_b, kb, O)):
        twin, lu = tmv.twin_draws(m_, s_, k_, ed)
        bound = tmv.bf16ref.gamma(Kc + 1) * (np.abs(m_.double().numpy()) + lu) + tmv.EPS_L * lu
        err = np.abs(got.detach().double().cpu().numpy() - twin)
        assert (err <= bound).all(), (float(err.max()), float((err - bound).max()))
    p64 = [t.double().requires_grad_(True) for t in (mu_w, sc_w, mu_b, sc_b)]
    u = lambda k_, rows, Kc: torch.from_numpy(np.stack([tmv.mvn_uniforms(k_, s_, ed, rows, Kc) for s_ in range(S)])).double()   # noqa: E731
    w64 = tmv._ref_draws64(p64[0], p64[1], u(kw, O, K))
    b64 = tmv._ref_draws64(p64[2], p64[3], u(kb, 1, O).reshape(S, O))
    ((w64 * gws[0].double()).sum() + (b64 * gws[1].double()).sum()).backward()
    for name, g, r in zip(("g_mu_w", "g_scale_w", "g_mu_b", "g_scale_b"), grads, p64):
        assert_close_scaled(g.double().cpu().numpy(), r.grad.numpy(), 1e-5, "mvn_draw_layer " + name)
    # the KL against an isotropic prior
    prior = (0.0, 0.5)
    leaves = [as_param(mv(mu_w, "mu")), as_param(mv(sc_w, "scale"))]
    kl = ops.mvn_kl([leaves[0]], [leaves[1]], [prior])
    g_kl = torch.autograd.grad(kl.sum(), leaves, None)
    q64 = [t.double().requires_grad_(True) for t in (mu_w, sc_w)]
    pr = MultivariateNormal(torch.full((K,), prior[0], dtype=torch.float64), scale_tril=prior[1] * torch.eye(K, dtype=torch.float64))
    want = tmv._kl64([("mvn", (q64[0], q64[1]), pr)], 1)
    want.backward()
    assert abs(kl[0].item() - want.item()) <= 1e-5 * abs(want.item()), (kl[0].item(), want.item())
    for name, g, r in zip(("g_mu", "g_scale"), g_kl, q64):
        assert_close_scaled(g.double().cpu().numpy(), r.grad.numpy(), 2e-5, "mvn_kl " + name)


# ===================================================================================================== tails
ROWS, WIDTH = 5, 8


def _moved(t, which, fill=None):
    return offset_view(t.to(DEV), off_for(t, which))


@pytest.mark.parametrize("which", [0, 1])
def test_mc_mean_with_and_without_out(which):
    """ops.mc_mean: bnn_mc_sum adds the S samples of an element in sample order in one thread, one element per load: bit-equal
    for a moved y, and for a moved `out=`, whose sentinel guards stay as they were."""
    y = torch.randn(S, ROWS, WIDTH, generator=torch.Generator().manual_seed(1)).to(DEV)
    want = ops.mc_mean(y)
    assert_close_scaled(want.cpu().numpy(), y.double().mean(0).cpu().numpy(), 1e-6, "mc_mean")
    assert same_bits(ops.mc_mean(_moved(y, which)), want)
    out = output_view((ROWS, WIDTH), torch.float32, DEV, F32_OFFS[which])
    assert ops.mc_mean(_moved(y, which + 1), out=out) is out
    torch.cuda.synchronize()
    assert same_bits(out, want) and guards_intact(out)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("width", [WIDTH, 20], ids=["narrow", "wide"])
@pytest.mark.parametrize("inputs", ["logits", "probs"])
def test_mc_uncertainty_and_score(inputs, width, which):
    """ops.mc_uncertainty / ops.mc_score on a moved y (and moved labels): held to float64 by the two files' own checks.  Width 8
    takes the narrow split, whose loads are one element wide wherever y starts -- the same kernel, the same order: bit-equal to
    the aligned run; width 20 takes the wide split, whose 16-B loads and mean stores fall back to element ones (tail_vec)."""
    y, t = tps.make_case(S, ROWS, width, inputs, 3)
    u0 = ops.mc_uncertainty(y.to(DEV), inputs)
    u = ops.mc_uncertainty(_moved(y, which), inputs)
    tpu.check_against_ref(u, y.numpy(), inputs, ("moved", inputs, width))
    ref = tps.ref_rows(y.numpy(), t.numpy(), inputs)
    top = np.sort(ref["mean"], -1)[:, -2:]                    # (exact predictions need rows away from ties; no bins are used here)
    assert (top[:, 1] - top[:, 0] > 1e-5).all(), "pick another seed for this case"
    s0 = ops.mc_score(y.to(DEV), t.to(DEV), inputs)
    s = ops.mc_score(_moved(y, which), _moved(t, which), inputs)
    tps.check_rows(s, ref, width, ("moved", inputs, width))
    if width == WIDTH:
        assert all(same_bits(a, b) for a, b in zip(u, u0)) and all(same_bits(a, b) for a, b in zip(s, s0))


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("width", [WIDTH, 40], ids=["narrow", "wide"])
@pytest.mark.parametrize("outputs", ["values", "mean_logvar", "mean_var"])
def test_mc_regression_and_score(outputs, width, which):
    """ops.mc_regression / ops.mc_regression_score on a moved y and target, against the two files' float64 checks; bit-equal to
    the aligned run at width 8 (the narrow split: element loads either way)."""
    y, t = trs.make_case(S, ROWS, width, outputs, 3)
    u0 = ops.mc_regression(y.to(DEV), outputs)
    u = ops.mc_regression(_moved(y, which), outputs)
    tpr.check_against_ref(u, y.numpy(), outputs, ("moved", outputs, width))
    s0 = ops.mc_regression_score(y.to(DEV), t.to(DEV), outputs)
    s = ops.mc_regression_score(_moved(y, which), _moved(t, which + 1), outputs)
    trs.check_elems(s, trs.ref_elems(y.numpy(), t.numpy(), outputs), ("moved", outputs, width))
    if width == WIDTH:
        assert all(same_bits(a, b) for a, b in zip(u, u0)) and all(same_bits(a, b) for a, b in zip(s, s0))


@pytest.mark.parametrize("which", [0, 1])
def test_gaussian_nll(which):
    """ops.gaussian_nll and its gradient on moved ys and target: the loss is a fixed-order fp64 sum of per-element terms read one
    element at a time -- bit-equal to the aligned run -- and both are held to float64 as in test_predictive_regression.py."""
    gen = torch.Generator().manual_seed(5)                   # (test_gaussian_nll_loss_and_gradient_against_float64's inputs)
    D = WIDTH // 2
    y = torch.cat([torch.randn(S, ROWS, D, generator=gen), torch.rand(S, ROWS, D, generator=gen) * 7 - 4], -1)
    t = torch.randn(ROWS, D, generator=gen)
    want, gN = tpr._nll64(y.numpy(), t.numpy())
    y0 = y.to(DEV).requires_grad_()
    l0 = ops.gaussian_nll(y0, t.to(DEV))
    l0.backward()
    y1 = as_param(_moved(y, which))
    l1 = ops.gaussian_nll(y1, _moved(t, which + 1))
    l1.backward()
    assert same_bits(l1.detach(), l0.detach()) and same_bits(y1.grad, y0.grad)
    assert abs(l1.item() - want) <= 1e-5 * max(1.0, abs(want)), (l1.item(), want)
    err = np.abs(tpr.N(y1.grad) * (S * ROWS * D) - gN).max()
    assert err <= 1e-5 * max(1.0, np.abs(gN).max()), (err, np.abs(gN).max())


@pytest.mark.parametrize("which", [0, 1])
def test_nig_head_loss_and_mc_evidential(which):
    """ops.nig_head forward and backward (elementwise: the 16-B and the element form evaluate nig_act / dsigma per element, bit-
    equal), ops.nig_loss against test_evidential.py's float64 autograd under its bound, ops.mc_evidential under its check."""
    D = WIDTH // 4
    gen = torch.Generator().manual_seed(13)
    z = (torch.randn(ROWS, 4 * D, generator=gen) * 3.0).to(DEV)
    gs = [torch.randn(ROWS, D, generator=gen).to(DEV) for _ in range(4)]
    z0, z1 = z.clone().requires_grad_(), as_param(_moved(z, which))
    o0, o1 = ops.nig_head(z0, D), ops.nig_head(z1, D)
    assert all(same_bits(a.detach(), b.detach()) for a, b in zip(o0, o1))
    g0 = torch.autograd.grad(sum((o * g).sum() for o, g in zip(o0, gs)), z0)[0]
    g1 = torch.autograd.grad(sum((o * _moved(g, which + i)).sum() for i, (o, g) in enumerate(zip(o1, gs))), z1)[0]
    assert same_bits(g0, g1)
    ts = tev.nig_inputs((ROWS, WIDTH), (1e-3, 50.0), torch.Generator().manual_seed(14))
    want, want_grads = tev.loss_ref64(ts[:4], ts[4], 1e-2)
    leaves = [as_param(_moved(t, which + i)) for i, t in enumerate(ts[:4])]
    loss = ops.nig_loss(*leaves, _moved(ts[4], which), 1e-2)
    grads = torch.autograd.grad(loss, leaves)
    tev.check_loss(loss.item(), grads, want, want_grads, "moved nig_loss")
    mc = tev.nig_inputs((S, ROWS, WIDTH), (1e-3, 50.0), torch.Generator().manual_seed(15))[:4]
    u = ops.mc_evidential(*[_moved(t, which + i) for i, t in enumerate(mc)])
    tev.check_mc(u, tev.evi64(*[t.numpy() for t in mc]), "moved mc_evidential")
    u0 = ops.mc_evidential(*[t.to(DEV) for t in mc])
    assert same_bits(u.mean, u0.mean)


@pytest.mark.parametrize("which", [0, 1])
def test_cross_entropy(which):
    """ops.cross_entropy on moved logits and labels: one thread per row, element loads, a fixed-order fp64 sum -- bit-equal to
    the aligned run -- and the rows are held to float64 by test_train_tail.py's own check."""
    x, y = ttt.xent_regime(ttt.XENT_REGIMES[0], rows=ROWS)
    x0 = x.to(DEV).requires_grad_()
    l0 = ops.cross_entropy(x0, y.to(DEV))
    l0.backward()
    x1 = as_param(_moved(x, which))
    l1 = ops.cross_entropy(x1, _moved(y, which))
    l1.backward()
    assert same_bits(l1.detach(), l0.detach()) and same_bits(x1.grad, x0.grad)
    _, ref, gref = ttt.xent64(ttt.N(x), y.numpy())
    assert abs(l1.item() - ref) <= ttt.xent_mean_bound(ttt.N(x), y.numpy())
    assert (np.abs(ttt.N(x1.grad) - gref) <= ttt.xent_grad_bound(ttt.N(x), y.numpy())).all()


# ===================================================================================================== a whole network
NET_DIMS, NET_B = (40, 24, 24, 10), 72


def _build_net(seed, reseat):
    """A 40-24-24-10 NormalLinear MLP with a seeded posterior on DEV; reseat: its twelve parameter tensors become consecutive views
    of ONE flat fp32 buffer that begins with the head's 10-float bias mean and ends with its 10-float bias scale -- everything in
    between starts 8 bytes off a 16-byte boundary."""
    from bayesianneuralnetworks_amd.nn import NormalLinear
    net = tpu.MLP(list(NET_DIMS), samples=S)
    pgen = torch.Generator().manual_seed(1000 + seed)
    layers = [m for m in net.layers if isinstance(m, NormalLinear)]
    with torch.no_grad():
        for m in layers:
            for p_, v in zip((m.weight.mean, m.weight.scale, m.bias.mean, m.bias.scale), seeded.posterior(pgen, tuple(m.weight.mean.shape))):
                p_.copy_(v)
    net = net.to(DEV)
    seeded.pin_streams(net, 5000)
    net.mc_batched = True
    if reseat:
        head = layers[-1]
        order = [head.bias.mean] + [p for m in layers for p in (m.weight.mean, m.weight.scale, m.bias.mean, m.bias.scale)
                                    if p is not head.bias.mean and p is not head.bias.scale] + [head.bias.scale]
        flat = torch.full((sum(p.numel() for p in order) + 128,), float("nan"), device=DEV)
        at = 64                                                     # 64 NaNs, then the first tensor on a 16-byte boundary
        for p in order:
            view = flat[at:at + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            at += p.numel()
        assert order[0].data_ptr() % 16 == 0 and all(p.data_ptr() % 16 == 8 for p in order[1:-1])
        net._flat = flat
    return net, layers


def _net_step(net, layers, mode):
    """forward_stacked, (ys * g).sum() + c KL with the KL gradient fused into the layers' launches, backward -> per layer the
    operands bwdref reads and the gradients."""
    from bayesianneuralnetworks_amd.nn import KLDivergence, fuse_activations, fuse_kl_gradient
    for m in layers:
        m.compute = mode
    fuse_activations(net, bf16_activations=False)
    bnn.manual_seed(77)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(NET_B, NET_DIMS[0], generator=gen).to(DEV)
    gy0 = torch.randn(S, NET_B, NET_DIMS[-1], generator=gen).to(DEV)
    cap = [dict() for _ in layers]
    handles = []
    for i, m in enumerate(layers):
        def hook(mod, inp, out, i=i):
            cap[i]["x"], cap[i]["y"] = inp[0].detach(), out.detach()
            out.register_hook(lambda g, i=i: cap[i].__setitem__("g", g.detach().clone()))
        handles.append(m.register_forward_hook(hook))
    saved = ops.FUSE_KL_GRADIENT
    fuse_kl_gradient(True)
    try:
        ys = net.forward_stacked(x, S)
        loss = (ys * gy0).sum() + tts.KL_C * KLDivergence(number_of_batches=tts.N_BATCHES)(net)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        fuse_kl_gradient(saved)
        for h in handles:
            h.remove()
    assert not ops._tls.kl_pending, "a parked KL gradient was left behind"
    return x, ys.detach(), cap


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_network_on_one_flat_parameter_buffer(mode):
    """mc_batched forward, loss.backward() with fuse_kl_gradient, one optim.Adam step and predictive_uncertainty of a 40-24-24-10
    MLP whose parameters are views of one flat buffer, 8 bytes off, against the same network on its own storage: the same keys
    and bit-equal draws; every layer's gradients (likelihood + fused KL, the head's narrow kernel refused and its parked KL entry
    handed on to the general kernels) under bwdref's bound for the kernels its alignment selects; Adam from equal gradients
    bit-equal (k_adam applies one update function per element in its 16-B and its element form)."""
    from bayesianneuralnetworks_amd import optim
    nets = {r: _build_net(3, r) for r in (False, True)}
    runs = {}
    for reseat, (net, layers) in nets.items():
        x, ys, cap = _net_step(net, layers, mode)
        assert bool(torch.isfinite(ys).all())
        L = len(layers)
        kl = dict(up=float(np.float32(tts.KL_C)), T=2 * L, n_batches=float(tts.N_BATCHES), prior_w=tts.PRIOR, prior_b=tts.PRIOR)
        draws = []
        for i, m in enumerate(layers):
            K, N = NET_DIMS[i], NET_DIMS[i + 1]
            kw, kb = m.weight.draw_key, m.bias.draw_key
            mu_w, rho_w, mu_b, rho_b = (t.detach() for t in (m.weight.mean, m.weight.scale, m.bias.mean, m.bias.scale))
            shared, relu = i == 0, i < L - 1
            al = dict(mu=mu_w.data_ptr() % 16 == 0, rho=rho_w.data_ptr() % 16 == 0, x=cap[i]["x"].data_ptr() % 16 == 0,
                      x8=cap[i]["x"].data_ptr() % 8 == 0, gy=True)
            assert al["mu"] == (not reseat) and al["rho"] == (not reseat)
            spec, _, _ = linear_plan(NET_B, K, N, mode, shared, False, False, relu, al)
            if i == 0:
                spec = dict(spec, gx=None)                                # the network's input carries no gradient
            w32 = ops._sample_affine_philox_raw(mu_w, rho_w, kw)
            draws.append((tpu._keys(m), w32, ops._sample_affine_philox_raw(mu_b, rho_b, kb)))
            op = dict(spec=spec, kl=kl, x=cap[i]["x"].reshape(-1, NET_B, K), g=cap[i]["g"].reshape(S, NET_B, N),
                      y=cap[i]["y"].reshape(S, NET_B, N) if relu else None, mu_w=mu_w, rho_w=rho_w, mu_b=mu_b, rho_b=rho_b,
                      eps_w=ops.eps_philox((N, K), kw, DEV), eps_b=ops.eps_philox((N,), kb, DEV), w32=w32,
                      wbf=ops._sample_affine_philox_raw(mu_w, rho_w, kw, torch.bfloat16))
            got = dict(g_mu_w=m.weight.mean.grad, g_rho_w=m.weight.scale.grad, g_mu_b=m.bias.mean.grad, g_rho_b=m.bias.scale.grad)
            if i > 0:
                got["gx"] = cap[i - 1]["g"].reshape(S, NET_B, K)
            ref = bwdref.layer_backward({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in op.items()})
            worst = bwdref.check({k: v.detach().cpu() for k, v in got.items()}, ref, "%s layer %d %s" % ("flat" if reseat else "own", i, spec))
            print("reseat %s layer %d %s: worst |err| / bound %s" % (reseat, i, spec, {k: round(v, 4) for k, v in worst.items()}))
        runs[reseat] = dict(x=x, ys=ys, draws=draws)
    for (ka, wa, ba), (kb_, wb, bb) in zip(runs[False]["draws"], runs[True]["draws"]):
        assert ka == kb_ and same_bits(wa, wb) and same_bits(ba, bb)
    assert_close_scaled(runs[True]["ys"].cpu().numpy(), runs[False]["ys"].double().cpu().numpy(), 1e-5 if mode == "f32" else 2e-2, "ys")
    # one Adam step from the SAME gradients (the flat net takes the aligned net's): bit-equal parameters, NaN guards untouched
    params = {r: [p for m in nets[r][1] for p in (m.weight.mean, m.weight.scale, m.bias.mean, m.bias.scale)] for r in nets}
    for p0, p1 in zip(params[False], params[True]):
        p1.grad = p0.grad.clone()
    for r in nets:
        optim.Adam(params[r], lr=1e-2).step()
    torch.cuda.synchronize()
    for p0, p1 in zip(params[False], params[True]):
        assert p1.data_ptr() % 16 in (0, 8) and same_bits(p0.data, p1.data)
    flat = nets[True][0]._flat
    assert bool(torch.isnan(flat[:64]).all()) and bool(torch.isnan(flat[-60:]).all())
    # inference on the flat net: the module path equals the op on forward_stacked, and float64
    net = nets[True][0]
    with torch.no_grad():
        bnn.manual_seed(8)
        u = net.predictive_uncertainty(runs[True]["x"], S, inputs="logits")
        bnn.manual_seed(8)
        ys = net.forward_stacked(runs[True]["x"], S)
        want = ops.mc_uncertainty(ys, "logits")
    for a, b in zip(u, want):
        assert torch.equal(a, b)
    tpu.check_against_ref(u, tpu.N(ys), "logits")
    # a moved INPUT on the net that owns its storage: the fp32 mode's three-plane dense path wants x on 16 bytes (ops.x3_eligible,
    # bnn_split_bf16x3) and the bf16 mode casts x into a fresh operand -- the same draws, the forward within the sibling tolerance
    net = nets[False][0]
    with torch.no_grad():
        bnn.manual_seed(9)
        ya = net.forward_stacked(runs[False]["x"], S)
        bnn.manual_seed(9)
        yb = net.forward_stacked(offset_view(runs[False]["x"], 8), S)
    assert_close_scaled(yb.cpu().numpy(), ya.double().cpu().numpy(), 1e-5 if mode == "f32" else 2e-2, "moved input")
    _lib.check_device(DEV)
