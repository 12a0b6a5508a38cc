"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol
include/bnn_hip.h declares (no compute without a GPU), the Module surface matches the
reference's (names, attributes, state_dict keys, traversal semantics, error behaviour)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch.distributions import Normal

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib
from bayesianneuralnetworks_amd.nn import *          # noqa: F401,F403
from bayesianneuralnetworks_amd.prune import PruneNormal
from bayesianneuralnetworks_amd.utils import _item_or_list, _single, _pair, _triple, apply_wb, traverse
from conftest import ROOT, allclose, load_golden


def test_library_loads_and_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    declared = set(re.findall(r"\b(bnn_[a-z0-9_]+)\s*\(", header))
    declared -= {"bnn_rng", "bnn_kl_tensor", "bnn_conv2d_shape"}
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in declared:
        assert getattr(lib, name) is not None
    # pure host queries only -- nothing is launched without a GPU
    assert lib.bnn_abi_version() == 2
    assert lib.bnn_arch() == b"gfx950"
    assert lib.bnn_kl_workspace_bytes(6) > 0


def test_argument_errors_are_reported_without_launching():
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    assert lib.bnn_sample_affine_eps(None, None, None, None, 4, 0, None) == -1
    assert b"NULL" in lib.bnn_last_error()
    r = _lib.Rng(seed=1, stream=70000)
    one = ctypes.c_void_p(16)
    assert lib.bnn_eps_philox(one, 4, 1, 4, ctypes.byref(r), None) == -5
    assert lib.bnn_linear_forward(one, 0, 4, one, 0, None, 0, one, 0, 4, 2, 0, 4, 1, 0, 0, None) == -2
    sh = _lib.Conv2dShape(B=1, C=3, H=5, W=5, O=4, KH=3, KW=3, stride_h=1, stride_w=1, pad_h=0, pad_w=0,
                          dil_h=1, dil_w=1, groups=2)
    assert lib.bnn_conv2d_forward(one, 0, one, 0, None, 0, one, 0, ctypes.byref(sh), 1, 0, 0, None, 0, None) == -2
    assert b"divisible by groups" in lib.bnn_last_error()
    assert lib.bnn_launch_count() == n0


def test_cuda_only_ops_refuse_cpu_tensors():
    from bayesianneuralnetworks_amd import ops
    with pytest.raises(_lib.BnnHipError):
        ops.sigma(torch.zeros(4))
    # the two-halves KL and the MC reduction that finishes it: no CPU path either, and nothing is left pending
    with pytest.raises(_lib.BnnHipError):
        ops.kl_normal_begin([torch.zeros(8)], [torch.zeros(8)], [(0.0, 0.1)], carry=True)
    assert ops._tls.kl_carry is None
    with pytest.raises(_lib.BnnHipError):
        ops.mc_mean(torch.zeros(2, 4))


def test_new_entry_points_reject_bad_arguments_without_launching():
    """bnn_kl_forward_partial / bnn_mc_sum_kl / bnn_linear_forward_sampled_kl: argument errors are negative codes with a
    message, before anything touches the GPU (runs without one)."""
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one = ctypes.c_void_p(16)
    t = (_lib.KlTensor * 1)()
    t[0].mu, t[0].rho, t[0].n, t[0].prior_mu, t[0].prior_sigma = 16, 16, 8, 0.0, 0.1
    assert lib.bnn_kl_forward_partial(None, 1, one, None) < 0
    assert lib.bnn_kl_forward_partial(t, 1, None, None) < 0
    assert b"workspace" in lib.bnn_last_error()
    t[0].prior_sigma = 0.0
    assert lib.bnn_kl_forward_partial(t, 1, one, None) < 0
    assert b"prior_sigma" in lib.bnn_last_error()
    t[0].prior_sigma = 0.1
    assert lib.bnn_mc_sum_kl(None, 8, 2, 8, 1.0, one, 0, None, 0, t, 1, 1.0, one, one, None) < 0
    assert lib.bnn_mc_sum_kl(one, 8, 2, 8, 1.0, one, 0, None, 0, t, 1, 0.0, one, one, None) < 0
    assert b"n_batches" in lib.bnn_last_error()
    assert lib.bnn_mc_sum_kl(one, 8, 2, 8, 1.0, one, 0, None, 0, t, 1, 1.0, None, one, None) < 0
    # the layer's own argument checks come first
    assert lib.bnn_linear_forward_sampled_kl(None, 0, 8, one, one, None, None, one, 0, 8, 4, 8, 8, 1, None, None, 0, 0,
                                             t, 1, one, None) < 0
    assert lib.bnn_launch_count() == n0


def test_device_error_word_status_path_is_wired():
    """bnn_check_device (the host half of the fused kernel's hand-off timeout report): exported, argument-checked, and a
    device with no registered workspace has no word to read -- BNN_OK without touching a GPU."""
    lib = _lib.load()
    assert _lib.E_DEVICE == -7
    assert lib.bnn_check_device(-1, None) == -5 and b"out of range" in lib.bnn_last_error()
    assert lib.bnn_check_device(64, None) == -5
    assert lib.bnn_check_device(63, None) == 0
    header = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    assert "BNN_E_DEVICE = -7" in header
    # the kernel side: every bounded wait reports through the word and skips its store
    src = open(os.path.join(ROOT, "bayesianneuralnetworks_amd", "csrc", "bnn_linear.hip")).read()
    assert src.count("handoff_ok &= lds_wait_ge(") == 2 and "kDevErrHandoffTimeout" in src


def test_stream_ids_never_wrap():
    from bayesianneuralnetworks_amd import _rng
    import itertools
    saved = _rng._stream_ids
    try:
        _rng._stream_ids = itertools.count(0xFFFF)
        assert _rng.new_stream_id() == 0xFFFF
        with pytest.raises(RuntimeError, match="exhausted"):
            _rng.new_stream_id()
    finally:
        _rng._stream_ids = saved


def test_kl_divergence_convenience_methods():
    """`.kl_divergence()` of BASELINE.json's north_star == the reference's module form KLDivergence(n)(model), loss.py:30-38."""
    torch.manual_seed(5)

    class Net(BayesianNetworkModule):
        def __init__(self):
            super().__init__(6, 3, samples=2)
            self.layers = torch.nn.Sequential(NormalLinear(6, 5), torch.nn.ReLU(), NormalLinear(5, 3))

        def _forward(self, x):
            return self.layers(x)

    net = Net()
    assert torch.equal(net.kl_divergence(7), KLDivergence(7)(net))
    layer = net.layers[0]
    per = [torch.distributions.kl.kl_divergence(p.dist, Normal(0, .1)).mean() for p in (layer.weight, layer.bias)]
    assert torch.allclose(layer.kl_divergence(), torch.stack(per).mean())
    assert bnn.nn.BayesianConv2d is NormalConv2d


def test_draw_once_entry_points_reject_bad_arguments_without_launching():
    """bnn_draw_multi / bnn_dense_forward / bnn_conv2d_dense_forward / bnn_conv2d_flipout_forward: argument errors are
    negative codes with a message before anything touches the GPU (runs without one)."""
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    one = ctypes.c_void_p(16)
    t = (_lib.DrawTensor * 1)()
    t[0].mu, t[0].rho, t[0].out, t[0].rows, t[0].cols, t[0].ld, t[0].out_sample_stride = 16, 16, 16, 4, 8, 64, 256
    t[0].out_dtype, t[0].rng.seed, t[0].rng.stream = _lib.BF16, 1, 1
    assert lib.bnn_draw_multi(None, 1, 1, None, 0, None, None) == -1
    assert lib.bnn_draw_multi(t, 9, 1, None, 0, None, None) == -5                       # > 8 tensors per launch
    t[0].cols = 6                                                                        # rows > 1 need cols % 4 == 0
    assert lib.bnn_draw_multi(t, 1, 1, None, 0, None, None) == _lib.E_UNSUPPORTED and b"cols" in lib.bnn_last_error()
    t[0].cols, t[0].rng.stream = 8, 70000
    assert lib.bnn_draw_multi(t, 1, 1, None, 0, None, None) == -5                       # stream id out of range
    t[0].rng.stream, t[0].kind = 1, 4                                                   # kinds 0 .. 3
    assert lib.bnn_draw_multi(t, 1, 1, None, 0, None, None) == -5 and b"kind" in lib.bnn_last_error()
    # dense: weights must be zero-padded to a multiple of 64 columns; K % 8 == 0
    assert lib.bnn_dense_forward(one, 0, 72, one, 16 * 72, 72, None, 0, one, 64, 16, 4, 16, 72, 1, 0, None) == _lib.E_UNSUPPORTED
    assert b"roundup" in lib.bnn_last_error()
    assert lib.bnn_dense_forward(None, 0, 64, one, 0, 64, None, 0, one, 64, 16, 4, 16, 64, 1, 0, None) == -1
    assert lib.bnn_dense_forward(one, 0, 64, one, 0, 64, None, 0, one, 64, 16, 4, 16, 64, 1, 64, None) == _lib.E_UNSUPPORTED   # unknown flag
    # fp32 parity mode on three-plane operands: plane strides are checked, a narrow layer writes fp32 only, three-plane draws are
    # plain draws
    ok_args = (one, 64 * 64, 0, 64, one, 32 * 64, 32 * 64, 64, None, 0, one, 0, 64 * 32, 32, 64, 32, 64, 1)
    assert lib.bnn_dense_forward_x3(None, *ok_args[1:], 0, None) == -1
    bad = list(ok_args); bad[1] = 8                                                     # plane stride < one plane
    assert lib.bnn_dense_forward_x3(*bad, 0, None) == -2 and b"plane stride" in lib.bnn_last_error()
    narrow = (one, 64 * 64, 0, 64, one, 16 * 64, 16 * 64, 64, None, 0, one, 64 * 16, 64 * 16, 16, 64, 16, 64, 1)
    assert lib.bnn_dense_forward_x3(*narrow, _lib.FLAG_Y_BF16, None) == _lib.E_UNSUPPORTED and b"narrow" in lib.bnn_last_error()
    assert lib.bnn_split_bf16x3(None, 4, 8, 8, one, 64, 256, None) == -1
    assert lib.bnn_split_bf16x3(one, 4, 12, 12, one, 64, 256, None) == _lib.E_UNSUPPORTED
    assert lib.bnn_split_bf16x3(one, 0, 8, 8, one, 64, 256, None) == 0                   # no rows: nothing to do
    assert lib.bnn_transpose_bf16(None, 64, 8, one, 64, 8, 4, 8, 1, None) == -1
    assert lib.bnn_transpose_bf16(one, 64, 12, one, 64, 8, 4, 12, 1, None) == _lib.E_UNSUPPORTED   # cols % 8
    assert lib.bnn_transpose_bf16(one, 64, 8, one, 64, 8, 16, 8, 1, None) == -2                    # BNN_E_SHAPE: ld_out < rows
    assert lib.bnn_transpose_bf16(one, 64, 8, one, 64, 8, 0, 8, 1, None) == 0                      # no rows: nothing to do
    sh = _lib.Conv2dShape(B=2, C=48, H=6, W=6, O=64, KH=3, KW=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1, groups=1)
    assert lib.bnn_conv2d_dense_forward(one, 0, one, 0, 448, None, 0, one, 0, ctypes.byref(sh), 1, 0, None) == _lib.E_UNSUPPORTED
    assert b"C = 64" in lib.bnn_last_error()
    sh.C = 64
    assert lib.bnn_conv2d_flipout_forward(one, one, 576, None, one, one, ctypes.byref(sh), 0, None) == -1
    sh.O = 128                                                                           # Flipout: 2 O must be 64 or 128
    assert lib.bnn_conv2d_flipout_forward(one, one, 576, one, one, one, ctypes.byref(sh), 0, None) == _lib.E_UNSUPPORTED
    # the launches' fit as a host query: 0 where they answer BNN_E_UNSUPPORTED for the shape, the images per workgroup where they launch
    assert lib.bnn_conv2d_dense_images(ctypes.byref(sh), _lib.CONV_FLIPOUT, 1, 1) == 0
    assert lib.bnn_conv2d_dense_images(ctypes.byref(sh), _lib.CONV_DENSE, 1, 1) == 2     # 128 // 36 = 3 images, B = 2 of them
    assert lib.bnn_conv2d_dense_images(None, _lib.CONV_DENSE, 1, 1) == -1
    assert lib.bnn_conv2d_dense_images(ctypes.byref(sh), 5, 1, 1) == -5 and b"variant" in lib.bnn_last_error()
    assert lib.bnn_conv2d_dense_images(ctypes.byref(sh), _lib.CONV_FLIPOUT_MC, 0, 1) == -2      # BNN_E_SHAPE: no samples
    sh.KH = 9                                                                            # kernel larger than the padded input
    assert lib.bnn_conv2d_dense_images(ctypes.byref(sh), _lib.CONV_DENSE, 1, 1) == -2
    assert lib.bnn_launch_count() == n0


def test_exports_match_reference_names():
    # pytorch_bayesian/nn/__init__.py:7-35
    names = ['BayesianModule', 'BayesianNetworkModule', 'WeightNormal', 'WeightMultivariateNormal',
             'BayesianLinear', 'NormalLinear', 'MultivariateNormalLinear', 'FlipoutNormalLinear',
             'NormalInverseGaussianLinear', 'MCDropoutLinear', 'BayesianConvNd', 'NormalConvNd',
             'NormalConv1d', 'NormalConv2d', 'NormalConv3d', 'FlipOutNormalConvNd', 'FlipOutNormalConv1d',
             'FlipOutNormalConv2d', 'FlipOutNormalConv3d', 'MCDropoutConvNd', 'MCDropoutConv1d',
             'MCDropoutConv2d', 'MCDropoutConv3d', 'KLDivergence', 'Entropy', 'NormalInverseGaussianLoss',
             'NormalInverseGaussianUncertainty']
    assert sorted(bnn.nn.__all__) == sorted(names)
    for n in names:
        assert hasattr(bnn.nn, n)
    assert bnn.__version__.startswith('0.0.4')
    import pytorch_bayesian
    from pytorch_bayesian.nn import NormalLinear as NL
    from pytorch_bayesian.prune import PruneNormal as PN
    from pytorch_bayesian.utils import apply_wb as aw
    assert NL is NormalLinear and PN is PruneNormal and aw is apply_wb


def test_state_dict_keys_and_pretrained_shapes():
    layer = NormalLinear(576, 10)
    assert list(layer.state_dict().keys()) == ['weight.mean', 'weight.scale', 'bias.mean', 'bias.scale']
    conv = NormalConv2d(64, 64, 3, padding=1, stride=2)
    assert conv.weight.shape == (64, 64, 3, 3) and conv.bias.shape == (64,)
    assert conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.padding == (1, 1)
    assert conv.dilation == (1, 1) and conv.transposed is False and conv.groups == 1
    g = load_golden("linear_mnist_pretrained")
    layer.load_state_dict({'weight.mean': torch.from_numpy(g["mu_w"]), 'weight.scale': torch.from_numpy(g["rho_w"]),
                           'bias.mean': torch.from_numpy(g["mu_b"]), 'bias.scale': torch.from_numpy(g["rho_b"])})
    assert np.array_equal(layer.weight.mean.detach().numpy(), g["mu_w"])


def test_weightnormal_surface():
    # tests/test_nn/test_core.py:14-39
    from torch.nn.parameter import Parameter
    for shape in [(1,), (3, 4), (5, 6, 7)]:
        wn = WeightNormal(*shape)
        assert isinstance(wn.mean, Parameter) and isinstance(wn.scale, Parameter)
        assert wn.mean.shape == shape and wn.shape == wn.mean.shape
        assert wn.device == wn.mean.device and wn.requires_grad == wn.mean.requires_grad
        assert isinstance(wn.sampled, torch.Tensor) and isinstance(wn.dist, Normal)
        assert wn.size() == shape and wn.size(0) == shape[0]
        torch.nn.init.constant_(wn.mean, 0)
        torch.nn.init.constant_(wn.scale, -100)
        wn.sample()
        assert (wn.stddev > 0).all() and (wn.stddev ** 2 == wn.variance).all()
        assert torch.allclose(wn.sampled, torch.zeros(shape), atol=1e-5)


def test_cpu_resident_layers_follow_the_reference_draw_order():
    """CPU tensors use the reference's own expression on torch's global generator
    (core.py:45, dense.py:46-54): same seed -> the fixture's w, b, y."""
    g = load_golden("linear_7x11")
    layer = NormalLinear(11, 7)
    with torch.no_grad():
        layer.weight.mean.copy_(torch.from_numpy(g["mu_w"]))
        layer.weight.scale.copy_(torch.from_numpy(g["rho_w"]))
        layer.bias.mean.copy_(torch.from_numpy(g["mu_b"]))
        layer.bias.scale.copy_(torch.from_numpy(g["rho_b"]))
    torch.manual_seed(int(g["eps_seed"]))
    y = layer(torch.from_numpy(g["x"]))
    assert allclose(layer.sampled[0].detach().numpy(), g["w"])
    assert allclose(layer.sampled[1].detach().numpy(), g["b"])
    assert allclose(y.detach().numpy(), g["y"])
    y2 = layer(torch.from_numpy(g["x"]), sample=False)
    assert torch.equal(y, y2)


class ComposableBNN(BayesianNetworkModule):
    def __init__(self, i, o, arch):
        super().__init__(i, o, samples=1)
        self.arch = arch

    def _forward(self, x, *a, **k):
        return self.arch(x)


def test_container_surface():
    # tests/test_nn/test_container.py:16-33
    bm = BayesianModule(3, 5, Normal(0, 1))
    assert bm.in_channels == 3 and bm.out_channels == 5
    assert bm.weight_prior is bm.bias_prior
    bnm = BayesianNetworkModule(3, 5, 10)
    assert (bnm.in_channels, bnm.out_channels, bnm.samples) == (3, 5, 10)
    with pytest.raises(NotImplementedError):
        bnm.forward(torch.zeros(2, 3, 5))


def test_utils_semantics():
    # tests/test_utils.py + tests/conftest.py:26-145
    for ex in [(0,), (1,), (2, 3), [0], [1], [2, 3]]:
        assert _item_or_list(ex) == (ex[0] if len(ex) == 1 else ex)
    assert _single(2.3) == (2.3,) and _pair(1) == (1, 1) and _triple(0) == (0, 0, 0)
    assert _pair((2, 3)) == (2, 3)
    lin = torch.nn.Linear(3, 3)
    assert apply_wb(lin, lambda x: None) is None
    assert apply_wb(lin, lambda x: x.shape) == [(3, 3), (3,)]
    nl = NormalLinear(3, 3, Normal(0, 1))        # conftest.py:91 quirk: Normal lands in `bias`
    assert nl.bias is not None
    assert apply_wb(nl, lambda x, type: type, pass_type=True) == ['w', 'b']
    assert apply_wb(nl, lambda x, module: x.shape, pass_module=True) == [(3, 3), (3,)]
    assert traverse(lin, lambda x: [x]) is None
    assert traverse(BayesianModule(3, 3, Normal(0, 1)), lambda x: [type(x.weight_prior)]) == [Normal]
    assert traverse(NormalLinear(3, 3, False, Normal(0, 1)), lambda x: [x.bias is not None]) == [False]
    net = ComposableBNN(3, 4, torch.nn.Sequential(NormalLinear(3, 4), NormalLinear(4, 2), NormalLinear(2, 1)))
    assert traverse(net, lambda x: [x.weight.shape]) == [torch.Size([4, 3]), torch.Size([2, 4]), torch.Size([1, 2])]
    # a Bayesian layer nested in a non-listed container is skipped (utils.py:51-52)
    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = NormalLinear(2, 2)
    assert traverse(ComposableBNN(2, 2, Wrap()), lambda x: [1]) is None


def test_kl_divergence_cpu_modules_and_errors():
    # tests/test_nn/test_loss.py:23-34 and the fixture value of make_golden.linear_case
    with pytest.raises(ValueError):
        KLDivergence()(ComposableBNN(3, 4, torch.nn.Linear(3, 4)))
    g = load_golden("linear_7x11")
    layer = NormalLinear(11, 7, True, Normal(float(g["prior_mu"]), float(g["prior_sigma"])))
    with torch.no_grad():
        layer.weight.mean.copy_(torch.from_numpy(g["mu_w"]))
        layer.weight.scale.copy_(torch.from_numpy(g["rho_w"]))
        layer.bias.mean.copy_(torch.from_numpy(g["mu_b"]))
        layer.bias.scale.copy_(torch.from_numpy(g["rho_b"]))
    kl = KLDivergence(number_of_batches=3)(ComposableBNN(11, 7, layer))
    assert abs(kl.item() - float(g["kl"])) < 1e-6


def test_prune_normal_fraction():
    # tests/test_prune.py:7-24 (passes a tensor to log_prob: the reference's int fails on torch 2.x)
    net = ComposableBNN(3, 4, torch.nn.Sequential(NormalLinear(30, 40), NormalLinear(40, 20)))
    before = net.traverse(lambda m: apply_wb(m, lambda x, module: x.mean.clone(), pass_module=True))
    PruneNormal()(net, 0.5)
    after = net.traverse(lambda m: apply_wb(m, lambda x, module: x.mean.clone(), pass_module=True))
    frac = torch.stack([(a != b).float().mean() for b, a in zip(before, after)]).mean()
    assert abs(frac - 0.5) < 2e-2
    assert (net.arch[0].weight.scale == -30).float().mean() == 0.5


def test_out_of_scope_layers_keep_reference_semantics():
    # collapsed-posterior KATs of tests/test_nn/test_dense.py:73-95, 196-229 and test_conv.py:149-215
    fl = FlipoutNormalLinear(5, 3)
    torch.nn.init.constant_(fl.weight.mean, 1)
    torch.nn.init.constant_(fl.weight.scale, -100)
    assert allclose(fl(torch.ones(3, 5)).detach().numpy(), np.full((3, 3), 5.0))
    fc = FlipOutNormalConv2d(3, 4, 3, padding=1)
    torch.nn.init.constant_(fc.weight.mean, 1)
    torch.nn.init.constant_(fc.weight.scale, -100)
    x = torch.ones(7, 3, 10, 10)
    want = torch.nn.functional.conv2d(x, torch.ones(4, 3, 3, 3), None, 1, 1)
    assert allclose(fc(x).detach().numpy(), want.numpy())
    nig = NormalInverseGaussianLinear(6, 2)
    out = nig(torch.ones(4, 6))
    assert len(out) == 4 and all(o.shape == (4, 2) for o in out)
    assert isinstance(nig(torch.ones(4, 6), sample=True), Normal)
    md = MCDropoutLinear(100, 100, drop_prob=0.3)
    assert abs((md(torch.ones(50, 100)) == 0).float().mean() - 0.3) < 5e-2
    mc = MCDropoutConv2d(2, 3, 3)
    assert mc.weight is mc.conv.weight
    mv = MultivariateNormalLinear(6, 3)
    assert mv(torch.ones(2, 6)).shape == (2, 3) and mv.weight.scale.shape == (3, 6, 6)
    ent = Entropy(-1)
    with pytest.warns(RuntimeWarning):
        ent(torch.zeros(2))
    assert abs(ent(torch.tensor([0.5, 0.5])).item() - np.log(2)) < 1e-6


def test_mc_batched_is_opt_in_and_cpu_uses_the_serial_loop():
    net = ComposableBNN(3, 4, torch.nn.Sequential(NormalLinear(3, 4)))
    assert net.mc_batched is False
    ys = net(torch.ones(2, 3), samples=3)
    assert isinstance(ys, list) and len(ys) == 3
    assert isinstance(net(torch.ones(2, 3)), torch.Tensor)


def test_training_callers_refuse_cpu_tensors_loudly():
    """optim.Adam / ops.cross_entropy / the backward entry points exist only as HIP: no CPU fallback."""
    import bayesianneuralnetworks_amd as bnn
    from bayesianneuralnetworks_amd import ops, optim
    from bayesianneuralnetworks_amd._lib import BnnHipError
    p = torch.nn.Parameter(torch.ones(3))
    p.grad = torch.ones(3)
    with pytest.raises(BnnHipError):
        optim.Adam([p]).step()
    with pytest.raises(ValueError):
        optim.Adam([p], lr=-1.0)
    with pytest.raises(BnnHipError):
        ops.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.long))
    assert bnn.optim.Adam is optim.Adam


def test_gradient_reducer_rejects_non_fp32_parameters():
    from bayesianneuralnetworks_amd import distributed as bd
    with pytest.raises(TypeError):
        bd.GradAllReducer([torch.nn.Parameter(torch.ones(2, dtype=torch.float64))])


def test_fuse_activations_marks_compute_format_hand_overs_and_x3_round_trip():
    """nn.fuse_activations(bf16_activations=True): a fused NormalLinear that feeds another NormalLinear may hand its hidden
    activation on in the compute format (bf16 in 'bf16' mode, three bf16 planes in the 'f32' mode); the last layer may not.
    ops.X3Activation.float() is the exact three-term sum (host logic, CPU tensors)."""
    import torch
    from bayesianneuralnetworks_amd import ops
    from bayesianneuralnetworks_amd.nn import NormalLinear, fuse_activations
    seq = torch.nn.Sequential(NormalLinear(16, 32), torch.nn.ReLU(), NormalLinear(32, 24), torch.nn.ReLU(), NormalLinear(24, 10))
    assert fuse_activations(seq, bf16_activations=True) == 2
    l1, l2, l3 = seq[0], seq[2], seq[4]
    assert l1.activation == l2.activation == 'relu' and l3.activation is None
    assert isinstance(seq[1], torch.nn.Identity) and isinstance(seq[3], torch.nn.Identity)
    assert l1.out_dtype == torch.bfloat16 and l2.out_dtype == torch.bfloat16
    assert l1.out_x3 and l2.out_x3                      # both consumers can read planes (the 10-wide head: K = 24 <= 2048)
    assert not getattr(l3, "out_x3", False)
    v = torch.randn(6, 40) * torch.logspace(-3, 3, 40)
    h = v.bfloat16()
    r = v - h.float()
    m = r.bfloat16()
    l = (r - m.float()).bfloat16()
    planes = torch.zeros(3, 2, 3, 64, dtype=torch.bfloat16)
    planes[:, :, :, :40] = torch.stack([h, m, l]).reshape(3, 2, 3, 40)
    act = ops.X3Activation(planes, 40)
    assert act.shape == (6, 40) and act.dim() == 2 and not act.is_cuda
    back = act.float()
    assert back.shape == (6, 40) and (back - v).abs().max() <= v.abs().max() * 2.0 ** -23


def test_rows_pitch_reads_the_strides_off_the_view():
    """the dense path launches with the (row pitch, sample stride) rows_pitch validated, never with values
    re-derived from M and K -- one padded row per sample (S, 1, K) sits stride(0) apart."""
    from bayesianneuralnetworks_amd import ops
    buf = torch.zeros(4, 1, 1216, dtype=torch.bfloat16)
    v = buf[:, :, :1200]                                   # what _dense_raw(pad_rows=True) returns for M = 1
    assert ops.rows_pitch(v, 1200) == (1200, 1216)
    buf = torch.zeros(4, 16, 1216, dtype=torch.bfloat16)
    assert ops.rows_pitch(buf[:, :, :1200], 1200) == (1216, 16 * 1216)
    assert ops.rows_pitch(buf[0, :, :1200], 1200) == (1216, 16 * 1216)
    assert ops.rows_pitch(buf[:, :8, :1200], 1200) == (1216, 16 * 1216)        # a row slice: samples still 16 rows apart
    assert ops.rows_pitch(torch.zeros(2, 3, 64, dtype=torch.bfloat16), 64) == (64, 192)
    assert ops.rows_pitch(torch.zeros(3, 64), 64) is None                                       # fp32
    assert ops.rows_pitch(torch.zeros(3, 68, dtype=torch.bfloat16)[:, :64], 64) is None         # pitch not whole 16-B chunks
    assert ops.rows_pitch(torch.zeros(8, 128, dtype=torch.bfloat16)[:, ::2], 64) is None        # element stride 2
    assert ops.rows_pitch(torch.zeros(1, 64, dtype=torch.bfloat16).expand(4, 64).unsqueeze(1), 64) is None   # samples overlap (stride 0)
    assert ops.rows_regular(buf[:, :, :1200], 1200) and not ops.rows_regular(torch.zeros(3, 64), 64)


def test_deepcopy_of_a_fresh_model():
    """copy.deepcopy of a model that has never run: the draws the posteriors keep from construction (`.sampled`, on the CPU a
    tensor WITH its autograd graph, which torch refuses to deep-copy) arrive detached, with their values; parameters, stream ids and
    recorded keys are the copy's own; the original is untouched and still trains through its draw."""
    import copy

    class Net(BayesianNetworkModule):
        def __init__(self):
            super().__init__(6, 3, samples=2)
            self.layers = torch.nn.Sequential(NormalLinear(6, 5), torch.nn.ReLU(), bnn.nn.LocalReparamLinear(5, 4), torch.nn.ReLU(),
                                              MultivariateNormalLinear(4, 3))

        def _forward(self, x):
            return self.layers(x)

    torch.manual_seed(0)
    net = Net()
    w0 = net.layers[0].weight
    assert w0.sampled.grad_fn is not None and net.layers[4].sampled[0].grad_fn is not None      # what used to make deepcopy raise
    twin = copy.deepcopy(net)
    for (n, p), (m, q) in zip(net.named_parameters(), twin.named_parameters()):
        assert n == m and torch.equal(p, q) and p.data_ptr() != q.data_ptr() and q.is_leaf and q.requires_grad
    t0 = twin.layers[0].weight
    assert torch.equal(t0.sampled, w0.sampled) and t0.sampled.grad_fn is None and w0.sampled.grad_fn is not None
    for a, b in zip(twin.layers[4].sampled, net.layers[4].sampled):
        assert torch.equal(a, b) and a.grad_fn is None
    assert t0._stream == w0._stream and twin.layers[2]._noise_stream == net.layers[2]._noise_stream
    assert twin.layers[4].weight_prior is not net.layers[4].weight_prior
    x = torch.randn(3, 6)
    torch.manual_seed(1)
    a = torch.stack(net(x))
    torch.manual_seed(1)
    b = torch.stack(twin(x))
    assert torch.equal(a, b)
    b.sum().backward()
    assert all(p.grad is None for p in net.parameters()) and all(q.grad is not None for q in twin.parameters())
    net.layers[0](x, sample=False).sum().backward()                 # the original's construction-time draw still carries its graph
    assert net.layers[0].weight.mean.grad is not None
