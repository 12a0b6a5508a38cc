"""The backward of every autograd function that goes through the shared backward steps of ops.py (_wgrad_sampled_raw,
_wgrad_plain_raw, the conv panel layout steps, the torch conv fallback): its launch count, pinned, and its gradients against float64
autograd on the same draws -- at the smallest shapes that reach each step.  (The sampled linear layer's three dispatches are pinned by
test_train_step.py.)"""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_scaled

from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd._rng import DrawKey

gpu = pytest.mark.gpu
S = 2
CONV = dict(B=2, C=8, H=6, W=6, O=8, k=3)                   # K = 72 and O = 8: multiples of 8, the panel backward
LIN = dict(M=8, K=16, N=8)

# bnn_launch_count over backward(), call by call, as measured on the commit before these steps were shared:
LAUNCHES = {
    # bnn_nchw_to_rows 1 + bnn_conv2d_im2col 1 + bnn_linear_backward_weight_sampled 4 (one tile and S = 2: the samples are split over
    # two workgroups, so the bias pair takes bnn_colsum + bnn_sample_affine_bwd inside the call, then the weight-gradient kernel and
    # its reduction over the slabs) + bnn_linear_backward_input_sampled 1 + bnn_conv2d_col2im 1 (which also sums a shared x)
    ("sampled_conv_panel", True, "f32"): 8, ("sampled_conv_panel", False, "f32"): 8,
    ("sampled_conv_panel", True, "bf16"): 8, ("sampled_conv_panel", False, "bf16"): 8,
    # groups = 2: bnn_sample_affine_philox (the weights again), torch's conv gradients (not counted), bnn_sample_affine_bwd for the
    # weight pair and for the bias pair
    ("sampled_conv_fallback", True, "f32"): 3, ("sampled_conv_fallback", False, "f32"): 3,
    # rows + im2col + bnn_linear_backward_weight + bnn_linear_backward_input + col2im + bnn_colsum
    ("plain_conv", True, "f32"): 6, ("plain_conv", False, "f32"): 6,
    # bnn_linear_backward_input (+ bnn_mc_sum over the samples for a shared x) + bnn_linear_backward_weight + bnn_colsum
    ("plain_linear", True, "f32"): 4, ("plain_linear", False, "f32"): 3,
    # bnn_draw_multi (the fp32 Flipout draw again) + bnn_linear_backward_input (+ bnn_mc_sum) + bnn_linear_backward_weight +
    # bnn_flipout_weight_backward
    ("flipout_linear", True, "f32"): 5, ("flipout_linear", False, "f32"): 4,
    # bnn_mc_dropout_backward (sums a shared x's samples itself) + bnn_linear_backward_input + _weight + bnn_colsum
    ("mc_dropout_linear", True, "bf16"): 4, ("mc_dropout_linear", False, "bf16"): 4,
}


def _scaled(got, want, tol, what):                          # test_hip_parity.py: tol (max(1, rms) + |want|), element by element
    assert_close_scaled(got.numpy(), want.numpy(), tol, what)


def _rel_max(got, want, tol, what):                         # test_mc_sample_counts.py: of the gradient's largest element
    assert float((got - want).abs().max() / max(1e-30, float(want.abs().max()))) <= tol, what


def _rel_max1(got, want, tol, what):                        # test_mc_dropout.py: ... or of 1 where that is smaller
    assert float((got - want).abs().max() / max(1.0, float(want.abs().max()))) <= tol, what


def _param(gen, *shape, scale=0.1, shift=0.0):
    return (torch.randn(*shape, generator=gen) * scale + shift).cuda().requires_grad_(True)


def _draw64(mu, rho, key):
    """The key's draws as a float64 expression of (mu, rho): eps taken off the device's own fp32 draw."""
    w = ops._sample_affine_philox_raw(mu.detach().contiguous(), rho.detach().contiguous(), key).double().cpu()
    m64, r64 = (t.detach().double().cpu().requires_grad_(True) for t in (mu, rho))
    sig = 1e-10 + F.softplus(r64)
    eps = ((w - m64) / sig).detach()
    return m64 + sig * eps, [m64, r64]


def _sampled_conv(shared, mode, groups):
    """-> (y, leaves, reference(x64) -> (y64, leaves64), gradient check, its tolerance): those of test_hip_parity.py's
    test_sampled_conv2d_backward_vs_float64_autograd, 2e-5 (fp32) / 3e-2 (bf16) of the gradient's scale."""
    c, gen = CONV, torch.Generator().manual_seed(31)
    wshape = (c["O"], c["C"] // groups, c["k"], c["k"])
    mu, rho = _param(gen, *wshape), _param(gen, *wshape, scale=0.15, shift=-2.0)
    mub, rhob = _param(gen, c["O"]), _param(gen, c["O"], scale=0.15, shift=-2.0)
    kw, kb = DrawKey(5, 40, 0, S, 3), DrawKey(5, 41, 0, S, 3)
    x = _param(gen, *(((), (S,))[not shared] + (c["B"], c["C"], c["H"], c["W"])), scale=1.0)
    y = ops.conv2d_sampled(x, mu, rho, mub, rhob, kw, kb, shared, (1, 1), (1, 1), (1, 1), groups, mode)

    def ref(x64):
        (w, lw), (b, lb) = _draw64(mu, rho, kw), _draw64(mub, rhob, kb)
        return torch.stack([F.conv2d(x64 if shared else x64[s], w[s], b[s], 1, 1, 1, groups) for s in range(S)]), lw + lb
    return y, [x, mu, rho, mub, rhob], ref, _scaled, (2e-5 if mode == "f32" else 3e-2)


def _plain_conv(shared, mode):
    """Tolerance: test_plain_conv2d_backward_panel_vs_float64_autograd's 2e-5."""
    c, gen = CONV, torch.Generator().manual_seed(32)
    w, b = _param(gen, S, c["O"], c["C"], c["k"], c["k"], scale=0.2), _param(gen, S, c["O"])
    x = _param(gen, *(((), (S,))[not shared] + (c["B"], c["C"], c["H"], c["W"])), scale=1.0)
    y = ops.conv2d_plain(x, w, b, shared, (1, 1), (1, 1), (1, 1), 1, mode)

    def ref(x64):
        w64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (w, b))
        return torch.stack([F.conv2d(x64 if shared else x64[s], w64[s], b64[s], 1, 1) for s in range(S)]), [w64, b64]
    return y, [x, w, b], ref, _scaled, 2e-5


def _plain_linear(shared, mode):
    """Tolerance: test_mc_sample_counts.py's test_shared_input_gradient_plain_linear, 1e-4 of the gradient's largest element."""
    M, K, N = LIN["M"], LIN["K"], LIN["N"]
    gen = torch.Generator().manual_seed(33)
    x = _param(gen, *(((), (S,))[not shared] + (M, K)), scale=1.0)
    w, b = _param(gen, S, N, K, scale=1.0), _param(gen, S, N, scale=1.0)
    y = ops.linear_plain(x, w, b, shared, mode)

    def ref(x64):
        w64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (w, b))
        xs = x64.unsqueeze(0).expand(S, M, K) if shared else x64
        return torch.einsum("smk,snk->smn", xs, w64) + b64.unsqueeze(1), [w64, b64]
    return y, [x, w, b], ref, _rel_max, 1e-4


def _flipout_linear(shared, mode):
    """Tolerance: test_shared_input_gradient_flipout_linear's 1e-4, on the signs ops.flipout_signs rebuilds from the key."""
    M, K, O = LIN["M"], LIN["K"], LIN["N"]
    gen = torch.Generator().manual_seed(34)
    mu, rho = _param(gen, O, K), _param(gen, O, K, scale=0.2, shift=-3.0)
    x = _param(gen, *((M, K) if shared else (S * M, K)), scale=1.0)
    key = DrawKey(13, 801, 0, S, 6)
    assert ops.flipout_drawable(mu)
    y = ops.linear_flipout_mc(x, mu, rho, key, shared, mode)

    def ref(x64):
        sg = ops.flipout_signs(key, 1, O + K, x.device)[:, 0].double().cpu()            # (S, O + K): R = [:, :O], S = [:, O:]
        m64, r64 = (t.detach().double().cpu().requires_grad_(True) for t in (mu, rho))
        w = m64 + (F.softplus(r64) + 1e-10) * (sg[:, :O].unsqueeze(2) * sg[:, O:].unsqueeze(1))
        xs = x64.unsqueeze(0).expand(S, M, K) if shared else x64.view(S, M, K)
        return torch.einsum("smk,sok->smo", xs, w), [m64, r64]
    return y, [x, mu, rho], ref, _rel_max, 1e-4


def _mc_dropout_linear(shared, mode):
    """Tolerance: test_mc_dropout.py's bf16-mode gradient bound, 2e-2 of the gradient's scale; the masks are the device's own
    (ops.mc_dropout of ones).  The backward contracts in fp32 on the fp32 x and w, so the float64 expression is on them too."""
    M, K, N, p = LIN["M"], LIN["K"], LIN["N"], 0.25
    gen = torch.Generator().manual_seed(35)
    x = _param(gen, *((M, K) if shared else (S * M, K)), scale=1.0)
    w, b = _param(gen, N, K, scale=0.25), _param(gen, N, scale=1.0)
    key = DrawKey(7, 99, 0, S, 17)
    y = ops.linear_mc_dropout(x, w, b, p, key, shared, mode)

    def ref(x64):
        mask = ops.mc_dropout(torch.ones(M, N, device=x.device), p, key, True).double().cpu()        # (S * M, N)
        w64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (w, b))
        return F.linear(torch.cat([x64] * S) if shared else x64, w64, b64) * mask, [w64, b64]
    return y, [x, w, b], ref, _rel_max1, 2e-2


BUILD = {"sampled_conv_panel": lambda sh, m: _sampled_conv(sh, m, 1), "sampled_conv_fallback": lambda sh, m: _sampled_conv(sh, m, 2),
         "plain_conv": _plain_conv, "plain_linear": _plain_linear, "flipout_linear": _flipout_linear, "mc_dropout_linear": _mc_dropout_linear}


@gpu
@pytest.mark.parametrize("layer,shared,mode", list(LAUNCHES), ids=lambda v: {True: "shared_x", False: "per_sample_x"}.get(v, v))
def test_backward_launch_count_and_gradients(layer, shared, mode):
    lib = _lib.load()
    y, leaves, ref, check, tol = BUILD[layer](shared, mode)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(36))
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    grads = torch.autograd.grad(y, leaves, gy.cuda())
    torch.cuda.synchronize()
    launches = lib.bnn_launch_count() - n0
    print("%s shared=%s %s: %d launches in backward()" % (layer, shared, mode, launches))
    x64 = leaves[0].detach().double().cpu().requires_grad_(True)
    y64, leaves64 = ref(x64)
    want = torch.autograd.grad(y64, [x64] + leaves64, gy.double().reshape(y64.shape))
    for i, (got, w_) in enumerate(zip(grads, want)):
        assert torch.isfinite(got).all()
        check(got.detach().double().cpu().reshape(w_.shape), w_, tol, "%s gradient %d" % (layer, i))
    assert launches == LAUNCHES[(layer, shared, mode)]
    _lib.check_device(y.device)
