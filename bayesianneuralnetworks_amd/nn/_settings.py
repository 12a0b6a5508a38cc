"""Compute-mode switch of the contraction kernels.

'f32'  : fp32 operands and accumulation -- the parity path (1e-5 vs the reference); wide forward layers run as three-way
        bf16 splits on the bf16 MFMA (fp32-accurate, csrc/bnn_linear.hip kComputeBf16x3), the rest on v_mfma_f32_16x16x4_f32;
'bf16' : operands rounded to bf16, fp32 accumulate (v_mfma_f32_16x16x32_bf16) -- the
         throughput configuration BASELINE.json names (tolerance stated in tests/DESIGN.md).
"""
_default = "f32"


def set_compute(mode):
    global _default
    if mode not in ("f32", "bf16"):
        raise ValueError("compute mode must be 'f32' or 'bf16'")
    _default = mode


def get_compute():
    return _default


def fuse_kl_gradient(enable=True):
    """Opt-in for training loops of the form `(likelihood + KLDivergence(...)(model)).backward()` (the reference's
    train.py:57-64): KLDivergence's backward then leaves its gradient to the layers' weight-gradient launches,
    which add the closed form in their final store (ops._tls.kl_pending) -- no separate KL pass, no accumulation add
    per parameter.  Leave it off when the KL gradient is taken with torch.autograd.grad(): the parked gradient
    reaches `.grad`, not the returned tuple."""
    from .. import ops
    ops.FUSE_KL_GRADIENT = bool(enable)


_keyed_mvn = False


def keyed_mvn_draws(enable=True):
    """Opt-in (default off) for the full-covariance posterior on the device: with it on, a MultivariateNormalLinear inside a
    BayesianNetworkModule's MC-batched pass gives every MC sample a keyed draw of its own (layer.weight.draw_key /
    layer.bias.draw_key; MVN-noise contract in include/bnn_hip.h) -- one bnn_mvn_draw launch for the weight and bias of all S
    samples, one dense launch, a HIP backward -- and KLDivergence takes the closed-form HIP KL for a WeightMultivariateNormal on
    the device with an isotropic prior (the default one).  With it off nothing about these layers changes: in a batched pass the
    layer draws once for all S samples, as before.  Making it the default is a separate step: the CIFAR10 network's launch-count
    test pins the draw-once head."""
    global _keyed_mvn
    _keyed_mvn = bool(enable)


def keyed_mvn_enabled():
    return _keyed_mvn


_conv_moment_training = False


def conv_moment_training(enable=True):
    """Opt-in (default off) for training conv nets without sampling (K19): with it on, BayesianNetworkModule.forward_moments also
    admits NormalConv1d / 2d / 3d, LocalReparamConv1d / 2d / 3d, nn.MomentELU and nn.MomentLinear -- their moment layers keep the
    autograd graph, and every backward launch is HIP (k_moments_conv3d_bwd, bnn_moments_elu_backward; K11's launches for a
    deterministic input, K18's for MomentLinear).  With it off forward_moments refuses exactly what it refused before, with the
    same messages.  Multivariate-normal and evidential layers stay refused either way; Flipout and MC-dropout layers
    unless nn.moment_estimator_layers() is on (K22).  Making it the
    default is a separate step: tests/test_moment_backward.py::test_forward_moments_refuses_what_has_no_backward pins the
    refusal of NormalConv2d and MomentELU."""
    global _conv_moment_training
    _conv_moment_training = bool(enable)


def conv_moment_training_enabled():
    return _conv_moment_training


_moment_estimator_layers = False


def moment_estimator_layers(enable=True):
    """Opt-in (default off) for sampling-free passes through the layers whose randomness is an estimator's rather than a weight
    posterior's draw (K22): with it on, BayesianNetworkModule.predictive_moments and the predictive_* methods with
    propagation='moments' admit MCDropoutLinear, MCDropoutConv1d / 2d / 3d, FlipoutNormalLinear and FlipOutNormalConv1d / 2d / 3d;
    forward_moments admits the dense ones, and the conv ones when nn.conv_moment_training() is on as well.  An MC-dropout layer
    runs its contraction on the moments (ops.moments_affine / ops.moments_conv_affine; its own linear / conv on a deterministic
    input) and then ONE bnn_moments_dropout launch that pushes the mask through the activation nn.moment_activations found
    behind it -- exact, where moment-matching the mask in front of a ReLU / ELU is not; directly in front of an
    nn.MomentSoftmax it hands on the pre-dropout moments with dropout = p and the predictive_* tails mask the drawn logits.  A
    Flipout layer runs its Normal* parent's moment pass on the same parameters (no bias).  With it off every refusal and every
    message stays what it was.  Making it the default is a separate step:
    tests/test_moment_conv_backward.py pins forward_moments' refusals of these layers by name."""
    global _moment_estimator_layers
    _moment_estimator_layers = bool(enable)


def moment_estimator_layers_enabled():
    return _moment_estimator_layers


def fuse_activations(module, bf16_activations=False, fuse_head=False):
    """Opt-in graph rewrite inside every torch.nn.Sequential:

    * a `NormalLinear` directly followed by `torch.nn.ReLU` gets the ReLU folded into its kernel
      epilogue (layer.activation = 'relu'); the ReLU module becomes `torch.nn.Identity`.
      Numerics unchanged (max(y, 0) of the same fp32 accumulator); one launch and one round trip
      of the activation tensor fewer per layer.
    * bf16_activations=True additionally lets a fused NormalLinear whose output feeds the next
      NormalLinear (through the Identity) emit that hidden activation in bf16 -- used only while
      the compute mode is 'bf16', where the consumer would round it to bf16 anyway, so results
      are identical to fp32 hidden activations; it halves the consumer's activation stream.  In the
      'f32' mode the same pairs (wide consumer, inference) pass the activation as the three bf16
      planes of its fp32 value (ops.X3Activation, exact to 2^-24), the operand format of the dense
      kernel's parity mode.
    * fuse_head=True (with bf16_activations): a hidden layer whose consumer is the classifier head (<= 16 outputs) at the END
      of the Sequential additionally learns that (`_fuse_head`): `BayesianNetworkModule.predictive_mean` then runs the pair as
      ONE launch (bnn_dense_forward_head) and the head's logits exist only as partial sums that the MC reduction adds up.
      Opt-in because it is only right when `_forward` returns that Sequential's output AS IT IS (anything applied to the
      logits afterwards -- a softmax -- would meet partial sums, not a tensor).

    Returns the number of fused pairs."""
    import torch
    from .dense import NormalLinear
    fused = 0
    for m in module.modules():
        if isinstance(m, torch.nn.Sequential):
            names = list(m._modules.keys())
            for a, b in zip(names[:-1], names[1:]):
                la, lb = m._modules[a], m._modules[b]
                if type(la) is NormalLinear and type(lb) is torch.nn.ReLU and la.activation is None:
                    la.activation = 'relu'
                    m._modules[b] = torch.nn.Identity()
                    fused += 1
            if bf16_activations:
                mods = [m._modules[n] for n in names]
                for i, la in enumerate(mods):
                    if type(la) is NormalLinear and la.activation == 'relu':
                        j = i + 1
                        while j < len(mods) and type(mods[j]) is torch.nn.Identity:
                            j += 1
                        if j < len(mods) and type(mods[j]) is NormalLinear and mods[j].in_channels % 8 == 0:
                            # a narrow consumer that ENDS the Sequential: under predictive_mean (bf16 mode, inference) the pair
                            # runs as one launch (ops._dense_head_raw) -- the layer learns who its head is
                            if fuse_head and mods[j].weight.mean.shape[0] <= 16 and j == len(mods) - 1:
                                la.__dict__["_fuse_head"] = mods[j]      # (not a submodule registration)
                            la.out_dtype = torch.bfloat16
                            # ... and in the fp32 parity mode, when the consumer runs on the dense kernels too, as the three
                            # bf16 planes they read (ops.X3Activation): same values, no split pass
                            la.out_x3 = mods[j].weight.mean.shape[0] > 16 or mods[j].in_channels <= 2048
    return fused


def moment_activations(module):
    """Opt-in rewrite for sampling-free inference (BayesianNetworkModule.predictive_moments, propagation='moments'), in the style
    of fuse_activations.  Inside every torch.nn.Sequential:

    * `torch.nn.ReLU`, `torch.nn.ELU` and a `torch.nn.Softmax(dim=-1)` become `nn.MomentReLU`, `nn.MomentELU` and
      `nn.MomentSoftmax`: subclasses that return the parent's bits on tensors, so every sampling path is unchanged, and that
      take and return an ops.Moments in a moment pass (MomentSoftmax does not transform: it sets link='softmax', which the
      predictive_* tails apply to the sampled logits -- it must end the network).
    * a `torch.nn.Linear` that lies behind a Bayesian layer of the same Sequential (the CIFAR10 example has one) becomes an
      `nn.MomentLinear` IN PLACE (the module is re-classed: its parameters and hooks are its own): a deterministic dense layer
      that hands moments on, m = a_m w^T + b, v = a_v (w^2)^T.
    * likewise behind a Bayesian layer of the same Sequential (K20), and re-classed in place in the same way: `torch.nn.MaxPool1d /
      2d / 3d`, `AvgPool1d / 2d / 3d`, `AdaptiveAvgPool1d / 2d / 3d` and `BatchNorm1d / 2d / 3d` become `nn.MomentMaxPool*`,
      `nn.MomentAvgPool*`, `nn.MomentAdaptiveAvgPool*` and `nn.MomentBatchNorm*` (their parent on tensors; a BatchNorm keeps its
      parameters and buffers).  In front of the first Bayesian layer they stay what they are.  A pool directly behind a conv
      layer gets that layer's plain moments (no activation is fused in front of it).
    * a twin directly behind a NormalConv1d / 2d / 3d or LocalReparamConv1d / 2d / 3d is made known to that layer
      (`_moment_act`, a __dict__ entry, not a submodule): in a moment pass the activation runs in the conv launch's epilogue
      (the standalone launch's bits) and the twin passes the result through.  Behind a dense layer the twins use the
      standalone launches.  FlipOutNormalConv1d / 2d / 3d and VariationalDropoutConv1d / 2d / 3d are told in the same way.
    * a twin directly behind an MCDropoutLinear or MCDropoutConv1d / 2d / 3d is made known to that layer as well (K22,
      nn.moment_estimator_layers): in a moment pass the layer's ONE bnn_moments_dropout launch pushes its mask through that
      activation and the twin passes the result through; an `nn.MomentSoftmax` directly behind it is recorded as 'softmax' --
      the layer then hands on its pre-dropout moments and the softmax keeps the mask for the predictive_* tails (dropout = p).
      Anything else behind the layer clears the entry.  After changing such a Sequential call this function again: a stale
      entry raises ops.BnnHipError in the pass.

    Idempotent; state_dict keys are unchanged (the activations have no state).  Returns the number of modules replaced."""
    import torch
    from .container import BayesianModule, MomentReLU, MomentELU, MomentLinear, MomentSoftmax, _MOMENT_RECLASS
    from .conv import (NormalConv1d, NormalConv2d, NormalConv3d, LocalReparamConv1d, LocalReparamConv2d, LocalReparamConv3d)
    from .conv import (FlipOutNormalConv1d, FlipOutNormalConv2d, FlipOutNormalConv3d, MCDropoutConv1d, MCDropoutConv2d, MCDropoutConv3d)
    from .conv import VariationalDropoutConv1d, VariationalDropoutConv2d, VariationalDropoutConv3d
    from .dense import MCDropoutLinear
    convs = (NormalConv1d, NormalConv2d, NormalConv3d, LocalReparamConv1d, LocalReparamConv2d, LocalReparamConv3d,
             FlipOutNormalConv1d, FlipOutNormalConv2d, FlipOutNormalConv3d,
             VariationalDropoutConv1d, VariationalDropoutConv2d, VariationalDropoutConv3d)
    dropouts = (MCDropoutLinear, MCDropoutConv1d, MCDropoutConv2d, MCDropoutConv3d)
    replaced = 0
    for m in module.modules():
        if not isinstance(m, torch.nn.Sequential):
            continue
        behind = False                                        # a Bayesian layer of this Sequential lies in front
        for name, child in list(m._modules.items()):
            twin = None
            if type(child) is torch.nn.Linear and behind:
                child.__class__ = MomentLinear
                replaced += 1
            elif type(child) in _MOMENT_RECLASS and behind:
                child.__class__ = _MOMENT_RECLASS[type(child)]
                replaced += 1
            behind = behind or isinstance(child, BayesianModule)
            if type(child) is torch.nn.ReLU:
                twin = MomentReLU(inplace=child.inplace)
            elif type(child) is torch.nn.ELU:
                twin = MomentELU(alpha=child.alpha, inplace=child.inplace)
            elif type(child) is torch.nn.Softmax and child.dim == -1:
                twin = MomentSoftmax(dim=-1)
            if twin is not None:
                twin.train(child.training)
                m._modules[name] = twin
                replaced += 1
        mods = list(m._modules.values())
        for la, lb in zip(mods[:-1], mods[1:]):
            if type(la) in convs:
                if isinstance(lb, (MomentReLU, MomentELU)):
                    la.__dict__["_moment_act"] = lb._moment_spec()
                else:
                    la.__dict__.pop("_moment_act", None)
            elif type(la) in dropouts:
                # K22: the mask goes through the activation behind the layer in the layer's own launch; a softmax cannot take
                # it (softmax(0) != 0), so there the layer hands the mask on to the predictive_* tails
                if isinstance(lb, (MomentReLU, MomentELU)):
                    la.__dict__["_moment_act"] = lb._moment_spec()
                elif isinstance(lb, MomentSoftmax):
                    la.__dict__["_moment_act"] = 'softmax'
                else:
                    la.__dict__.pop("_moment_act", None)
        if mods and type(mods[-1]) in dropouts:
            mods[-1].__dict__.pop("_moment_act", None)
    return replaced
