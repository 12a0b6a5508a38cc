"""BayesianModule / BayesianNetworkModule with the reference's surface
(pytorch_bayesian/nn/container.py:6-37) plus the MI355X execution options:

  * mc_batched  -- run all `samples` MC draws of every Bayesian layer in one grid per layer
                   instead of the serial Python loop of container.py:36-37;
  * forward_sharded -- shard the MC axis over the ranks of a torch.distributed (RCCL)
                   process group and all-reduce [KL sums || sum of predictions] once.
"""
import torch
from torch.nn import Module

from .. import _mc
from ..utils import _item_or_list, traverse
from ..utils.utils import deepcopy_detached


class BayesianModule(Module):
    """container.py:6-14: holds the priors and channel counts."""

    def __init__(self, in_channels, out_channels, prior, bias_prior=None):
        super().__init__()
        self.weight_prior = prior
        self.bias_prior = bias_prior if bias_prior else prior   # container.py:12
        self.in_channels = in_channels
        self.out_channels = out_channels

    __deepcopy__ = deepcopy_detached           # (a MultivariateNormalLinear's .sampled carries its graph)

    def kl_divergence(self, number_of_batches=1):
        """Convenience BASELINE.json's north_star names (the reference has only the module form, loss.py:11-38):
        `KLDivergence(number_of_batches)` over this layer's own weight / bias posteriors."""
        from .loss import KLDivergence
        return KLDivergence(number_of_batches)(_Single(self))


class _Single:
    """A one-layer 'model' for KLDivergence.forward: traverse(fn) visits just that layer."""

    def __init__(self, layer):
        self.layer = layer

    def traverse(self, fn, *args, **kwargs):
        return traverse(self.layer, fn, *args, **kwargs)


_MOMENTS_SUPPORTED = ("moment propagation supports NormalLinear / LocalReparamLinear / VariationalDropoutLinear (the last for inference only), ReLU folded into them by "
                      "nn.fuse_activations, MultivariateNormalLinear (inference only), NormalConv1d / 2d / 3d and LocalReparamConv1d / 2d / 3d, "
                      "VariationalDropoutConv1d / 2d / 3d (inference only), the activations "
                      "nn.moment_activations rewrites (ReLU, ELU, a torch.nn.Linear behind a Bayesian layer, and a Softmax over the last "
                      "axis that ends the network; behind a Bayesian layer also MaxPool / AvgPool / AdaptiveAvgPool 1d / 2d / 3d and an "
                      "eval-mode BatchNorm1d / 2d / 3d), "
                      "reshaping modules such as torch.nn.Flatten, and torch.nn.Identity")


_MOMENTS_SUPPORTED_K22 = ("; with nn.moment_estimator_layers switched on also MCDropoutLinear, MCDropoutConv1d / 2d / 3d (the mask "
                          "pushed through the ReLU / ELU behind the layer, or handed to the tail in front of a closing Softmax), "
                          "FlipoutNormalLinear and FlipOutNormalConv1d / 2d / 3d")


def _estimator_layers():
    """The layer classes nn.moment_estimator_layers admits to a moment pass (K22); () while the switch is off."""
    from . import _settings
    if not _settings.moment_estimator_layers_enabled():
        return ()
    from .dense import MCDropoutLinear, FlipoutNormalLinear
    from .conv import (MCDropoutConv1d, MCDropoutConv2d, MCDropoutConv3d, FlipOutNormalConv1d, FlipOutNormalConv2d,
                       FlipOutNormalConv3d)
    return (MCDropoutLinear, FlipoutNormalLinear, MCDropoutConv1d, MCDropoutConv2d, MCDropoutConv3d, FlipOutNormalConv1d,
            FlipOutNormalConv2d, FlipOutNormalConv3d)


def _refuse_pending(y, who):
    """The output of a moment pass must not carry a mask that no nn.MomentSoftmax took over (K22)."""
    if y._pending is not None:
        from .. import ops
        raise ops.BnnHipError("%s: the network's output carries the pending mask (dropout=%r) of an MC-dropout layer that "
                              "nn.moment_activations found in front of an nn.MomentSoftmax, and no such softmax followed: call "
                              "nn.moment_activations again after changing a Sequential" % (who, y._pending))


def _moments_supported():
    """_MOMENTS_SUPPORTED, naming the K22 layers while nn.moment_estimator_layers is on."""
    return _MOMENTS_SUPPORTED + (_MOMENTS_SUPPORTED_K22 if _estimator_layers() else "")


def _moment_twin_forward(self, parent, x, apply):
    """forward of nn.MomentReLU / MomentELU: a tensor takes the parent's forward (its bits, on every sampling path); an
    ops.Moments is moment-matched by `apply` -- unless the conv launch that produced it already ran this activation in its
    epilogue (nn.moment_activations told that layer; the Moments says which activation it carries).  Moments that an MC-dropout
    layer folded its mask into with NO activation (K22: _act == 'identity' -- nn.moment_activations never told that layer about
    this module) are refused: a dropped unit is a spike at zero, and the Gaussian recursion of this module on mask-matched moments
    would be the wrong answer, silently."""
    from .. import ops
    if not isinstance(x, ops.Moments):
        return parent.forward(self, x)
    ops._refuse_link(x, type(self).__name__)
    if x._act is not None:
        if x._act != self._moment_spec():
            raise ops.BnnHipError("%s: the layer in front fused %r into its launch, this module is %r: call "
                                  "nn.moment_activations again after changing a Sequential" % (type(self).__name__, x._act, self._moment_spec()))
        return ops.Moments(x.mean, x.var)
    return apply(x)


class MomentReLU(torch.nn.ReLU):
    """torch.nn.ReLU that also takes an ops.Moments inside a moment pass (ops.moments_relu / moments_relu_f64); on tensors it
    is its parent.  Put in place by nn.moment_activations."""

    def _moment_spec(self):
        return 'relu'

    def forward(self, x):
        from .. import ops
        ctx = _mc.moments_current()
        track = ctx is not None and ctx.track                          # forward_moments: keep the graph
        return _moment_twin_forward(self, torch.nn.ReLU, x, lambda mom: ops.moments_relu(mom, track) if mom.mean.is_cuda
                                    else ops.moments_relu_f64(mom, track))


class MomentELU(torch.nn.ELU):
    """torch.nn.ELU that also takes an ops.Moments inside a moment pass (ops.moments_elu / moments_elu_f64); on tensors it is
    its parent.  Put in place by nn.moment_activations."""

    def _moment_spec(self):
        return ('elu', float(self.alpha))

    def forward(self, x):
        from .. import ops
        ctx = _mc.moments_current()
        track = ctx is not None and ctx.track                          # forward_moments: keep the graph
        return _moment_twin_forward(self, torch.nn.ELU, x, lambda mom: ops.moments_elu(mom, self.alpha, track) if mom.mean.is_cuda
                                    else ops.moments_elu_f64(mom, self.alpha, track))


class MomentLinear(torch.nn.Linear):
    """torch.nn.Linear that also takes an ops.Moments inside a moment pass -- a deterministic dense layer BEHIND a Bayesian one,
    as in the CIFAR10 example: m = a_m w^T + b, v = a_v (w^2)^T (ops.moments_affine: K16's launch with sigma^2 = 0; CPU:
    ops.moments_affine_f64).  On tensors it is its parent.  nn.moment_activations re-classes a Linear in place: its parameters,
    hooks and state_dict are the module's own."""

    def forward(self, x):
        from .. import ops
        from . import _settings
        if not isinstance(x, ops.Moments):
            return torch.nn.Linear.forward(self, x)
        ctx = _mc.moments_current()
        track = ctx is not None and ctx.track                          # forward_moments: keep the graph
        if not x.mean.is_cuda:
            out = ops.moments_affine_f64(x, self.weight, self.bias, track)
        else:
            out = ops.moments_affine(x, self.weight, self.bias, compute=_settings.get_compute(), track=track)
        if ctx is not None and ctx.covariance:                           # a covariance pass (K21): should this layer be the head
            ctx.last_dense = (type(self).__name__, self.out_features)
            if self.out_features <= ops.HEAD_COV_MAX_N:
                out._head = ops.head_operands(x, self.weight)
        return out


class MomentSoftmax(torch.nn.Softmax):
    """torch.nn.Softmax over the last axis that, inside a moment pass, does NOT transform: it hands on the logit moments with
    link='softmax', which the predictive_* tails apply to the sampled logits.  It must end the network: every layer refuses
    moments that carry a link.  On tensors it is its parent."""

    def forward(self, x):
        from .. import ops
        if not isinstance(x, ops.Moments):
            return torch.nn.Softmax.forward(self, x)
        pending, x._pending = x._pending, None                            # (K22) the mask of the MC-dropout layer in front
        try:
            ops._refuse_link(x, "MomentSoftmax")
        finally:
            x._pending = pending
        if self.dim not in (-1, x.dim() - 1):
            raise ops.BnnHipError("MomentSoftmax: softmax over axis %r of %d; only the last axis is supported" % (self.dim, x.dim()))
        # the one module that keeps a covariance (K21) and a pending mask (K22: dropout = p, applied to the drawn logits)
        out = ops.Moments(x.mean, x.var, link='softmax', cov=x.cov, dropout=pending)
        out._head = x._head
        return out


def _moment_track():
    ctx = _mc.moments_current()
    return ctx is not None and ctx.track                               # forward_moments: keep the graph


def _moment_pool_forward(self, x, nd, op, kernel_size, stride, padding, dilation, count_include_pad):
    """An ops.Moments through a pooling twin (K20): ops.moments_pool on the device, ops.moments_pool_f64 on the CPU; one item
    (C, *spatial) is a batch of one, as for its parent."""
    from .. import ops
    who = type(self).__name__
    ops._refuse_link(x, who)
    if getattr(self, "ceil_mode", False):
        raise ops.BnnHipError("%s: ceil_mode=True is not supported in a moment pass" % who)
    if getattr(self, "return_indices", False):
        raise ops.BnnHipError("%s: return_indices=True is not supported in a moment pass (a Gaussian maximum has no index)" % who)
    if getattr(self, "divisor_override", None) is not None:
        raise ops.BnnHipError("%s: divisor_override is not supported in a moment pass" % who)
    if x.dim() not in (nd + 1, nd + 2):
        raise ops.BnnHipError("%s: moments of shape %s (expected %d or %d axes)" % (who, tuple(x.shape), nd + 1, nd + 2))
    one = x.dim() == nd + 1
    if one:
        x = ops.Moments(x.mean.unsqueeze(0), None if x.var is None else x.var.unsqueeze(0))
    if kernel_size is None:                                            # adaptive: the average pool with kernel = stride = in / out
        out = self.output_size if isinstance(self.output_size, (tuple, list)) else (self.output_size,) * nd
        out = tuple(n if o is None else int(o) for o, n in zip(out, x.shape[2:]))
        if len(out) != nd or any(o < 1 or n % o for o, n in zip(out, x.shape[2:])):
            raise ops.BnnHipError("%s: the input extents %s are no multiple of the output extents %s: only then is adaptive "
                                  "average pooling a pooling with one window size" % (who, tuple(x.shape[2:]), out))
        kernel_size = stride = tuple(n // o for o, n in zip(out, x.shape[2:]))
    fn = ops.moments_pool if x.mean.is_cuda else ops.moments_pool_f64
    y = fn(x, op, kernel_size, stride, padding, dilation, count_include_pad, _moment_track())
    if one:
        y = ops.Moments(y.mean.squeeze(0), None if y.var is None else y.var.squeeze(0))
    return y


def _max_pool_twin(parent, nd):
    def forward(self, x):
        from .. import ops
        if not isinstance(x, ops.Moments):
            return parent.forward(self, x)
        return _moment_pool_forward(self, x, nd, 'max', self.kernel_size, self.stride, self.padding, self.dilation, True)
    return forward


def _avg_pool_twin(parent, nd):
    def forward(self, x):
        from .. import ops
        if not isinstance(x, ops.Moments):
            return parent.forward(self, x)
        return _moment_pool_forward(self, x, nd, 'avg', self.kernel_size, self.stride, self.padding, 1, self.count_include_pad)
    return forward


def _adaptive_avg_pool_twin(parent, nd):
    def forward(self, x):
        from .. import ops
        if not isinstance(x, ops.Moments):
            return parent.forward(self, x)
        return _moment_pool_forward(self, x, nd, 'avg', None, None, 0, 1, True)
    return forward


def _batchnorm_twin(parent):
    def forward(self, x):
        from .. import ops
        if not isinstance(x, ops.Moments):
            return parent.forward(self, x)
        if _moment_track():
            raise ops.BnnHipError("forward_moments: %s has no moment backward" % type(self).__name__)
        return ops.moments_batchnorm(x, self) if x.mean.is_cuda else ops.moments_batchnorm_f64(x, self)
    return forward


class MomentMaxPool1d(torch.nn.MaxPool1d):
    """torch.nn.MaxPool1d that also takes an ops.Moments inside a moment pass (ops.moments_pool / moments_pool_f64: the window
    folded pairwise with the moment-matched maximum of two Gaussians); on tensors it is its parent.  nn.moment_activations
    re-classes a MaxPool1d behind a Bayesian layer in place.  ceil_mode and return_indices are refused in a moment pass."""
    forward = _max_pool_twin(torch.nn.MaxPool1d, 1)


class MomentMaxPool2d(torch.nn.MaxPool2d):
    """MomentMaxPool1d for torch.nn.MaxPool2d."""
    forward = _max_pool_twin(torch.nn.MaxPool2d, 2)


class MomentMaxPool3d(torch.nn.MaxPool3d):
    """MomentMaxPool1d for torch.nn.MaxPool3d."""
    forward = _max_pool_twin(torch.nn.MaxPool3d, 3)


class MomentAvgPool1d(torch.nn.AvgPool1d):
    """torch.nn.AvgPool1d that also takes an ops.Moments inside a moment pass (mean' = sum m / n, var' = sum v / n^2: exact for
    independent elements); on tensors it is its parent.  ceil_mode is refused in a moment pass."""
    forward = _avg_pool_twin(torch.nn.AvgPool1d, 1)


class MomentAvgPool2d(torch.nn.AvgPool2d):
    """MomentAvgPool1d for torch.nn.AvgPool2d; divisor_override is refused in a moment pass."""
    forward = _avg_pool_twin(torch.nn.AvgPool2d, 2)


class MomentAvgPool3d(torch.nn.AvgPool3d):
    """MomentAvgPool1d for torch.nn.AvgPool3d; divisor_override is refused in a moment pass."""
    forward = _avg_pool_twin(torch.nn.AvgPool3d, 3)


class MomentAdaptiveAvgPool1d(torch.nn.AdaptiveAvgPool1d):
    """torch.nn.AdaptiveAvgPool1d that also takes an ops.Moments inside a moment pass: the average pool with kernel = stride =
    in / out, refused where the input extent is no multiple of the output extent.  On tensors it is its parent."""
    forward = _adaptive_avg_pool_twin(torch.nn.AdaptiveAvgPool1d, 1)


class MomentAdaptiveAvgPool2d(torch.nn.AdaptiveAvgPool2d):
    """MomentAdaptiveAvgPool1d for torch.nn.AdaptiveAvgPool2d."""
    forward = _adaptive_avg_pool_twin(torch.nn.AdaptiveAvgPool2d, 2)


class MomentAdaptiveAvgPool3d(torch.nn.AdaptiveAvgPool3d):
    """MomentAdaptiveAvgPool1d for torch.nn.AdaptiveAvgPool3d."""
    forward = _adaptive_avg_pool_twin(torch.nn.AdaptiveAvgPool3d, 3)


class MomentBatchNorm1d(torch.nn.BatchNorm1d):
    """torch.nn.BatchNorm1d that also takes an ops.Moments inside a moment pass: in eval mode, with running statistics, the
    per-channel affine map of ops.moments_batchnorm / moments_batchnorm_f64; training mode is refused (the batch statistics of a
    random activation are not part of the recursion), and so is forward_moments (no backward).  On tensors it is its parent."""
    forward = _batchnorm_twin(torch.nn.BatchNorm1d)


class MomentBatchNorm2d(torch.nn.BatchNorm2d):
    """MomentBatchNorm1d for torch.nn.BatchNorm2d."""
    forward = _batchnorm_twin(torch.nn.BatchNorm2d)


class MomentBatchNorm3d(torch.nn.BatchNorm3d):
    """MomentBatchNorm1d for torch.nn.BatchNorm3d."""
    forward = _batchnorm_twin(torch.nn.BatchNorm3d)


# torch class -> its twin: what nn.moment_activations re-classes in place behind a Bayesian layer
_MOMENT_RECLASS = {
    torch.nn.MaxPool1d: MomentMaxPool1d, torch.nn.MaxPool2d: MomentMaxPool2d, torch.nn.MaxPool3d: MomentMaxPool3d,
    torch.nn.AvgPool1d: MomentAvgPool1d, torch.nn.AvgPool2d: MomentAvgPool2d, torch.nn.AvgPool3d: MomentAvgPool3d,
    torch.nn.AdaptiveAvgPool1d: MomentAdaptiveAvgPool1d, torch.nn.AdaptiveAvgPool2d: MomentAdaptiveAvgPool2d,
    torch.nn.AdaptiveAvgPool3d: MomentAdaptiveAvgPool3d,
    torch.nn.BatchNorm1d: MomentBatchNorm1d, torch.nn.BatchNorm2d: MomentBatchNorm2d, torch.nn.BatchNorm3d: MomentBatchNorm3d,
}
_MOMENT_BATCHNORMS = (MomentBatchNorm1d, MomentBatchNorm2d, MomentBatchNorm3d)


def _moments_asked(propagation, who, kl=None, covariance=False):
    """propagation == 'moments'?  ValueError for anything but 'samples' / 'moments', and for covariance=True (K21: correlated
    draws from the head's covariance) without propagation='moments' (and then no KL is left pending)."""
    if propagation == 'samples':
        if covariance:
            from .. import ops
            ops._kl_uncarry(kl)
            raise ValueError("%s: covariance=True needs propagation='moments' (stochastic forwards are correlated as they are)" % who)
        return False
    if propagation == 'moments':
        return True
    from .. import ops
    ops._kl_uncarry(kl)
    raise ValueError("%s: propagation must be 'samples' or 'moments', got %r" % (who, propagation))


def _on_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _refuse_cpu_tails(who, tails, *given):
    """x is not on the device, so `tails` ("advance is a tail" / "advance / kl are tails") of the device launch cannot run."""
    if any(t is not None for t in given):
        from .. import ops
        raise ops.BnnHipError("%s: %s of the device launch; x is not on the device" % (who, tails))


def _refuse_device_state(who, state, state_type):
    if state is not None and not (isinstance(state, state_type) and state.device.type == "cpu"):
        from .. import ops
        raise ops.BnnHipError("%s: x is not on the device, so state must be a %s on the CPU" % (who, state_type.__name__))


def _scaled_sum(ys, scale, out):
    """predictive_mean without the device tail: scale * sum over the samples, into `out` when given."""
    m = ys.sum(0) * scale
    if out is not None:
        out.copy_(m.reshape(out.shape))
        return out
    return m


class BayesianNetworkModule(Module):
    """container.py:17-37.  Subclasses implement `_forward`."""

    def __init__(self, in_channels, out_channels, samples=10):
        super().__init__()
        self.samples = samples
        self.in_channels = in_channels
        self.out_channels = out_channels
        # Opt-in: valid when every layer after the first Bayesian one treats batch rows
        # independently (no train-mode BatchNorm downstream of a Bayesian layer).
        self.mc_batched = False

    def _forward(self, x, *args, **kwargs):
        raise NotImplementedError('self._forward() not implemented')

    def traverse(self, fn, *args, **kwargs):
        return traverse(self, fn, *args, **kwargs)

    def kl_divergence(self, number_of_batches=1):
        """`KLDivergence(number_of_batches)(self)` (loss.py:30-38) -- the `.kl_divergence()` BASELINE.json's north_star names."""
        from .loss import KLDivergence
        return KLDivergence(number_of_batches)(self)

    def sparsity(self):
        """(dropped, total) over every VariationalDropoutLinear and VariationalDropoutConv1d / 2d / 3d of the network: the weights
        with log_alpha above the layer's threshold (3.0 where it is None), and all of them -- layer.sparsity()'s count, summed."""
        from .dense import VariationalDropoutLinear
        from .conv import VariationalDropoutConvNd
        dropped = total = 0
        for m in self.modules():
            if isinstance(m, (VariationalDropoutLinear, VariationalDropoutConvNd)):
                d, t = m._dropped()
                dropped, total = dropped + d, total + t
        return dropped, total

    def forward(self, x, samples=None, *args, **kwargs):
        if samples is None:
            samples = self.samples
        if self.mc_batched and samples > 1 and isinstance(x, torch.Tensor) and x.is_cuda:
            return _item_or_list(self._forward_batched(x, samples, 0, *args, **kwargs))
        # container.py:36-37: the serial MC loop
        return _item_or_list([self._forward(x, *args, **kwargs) for _ in range(samples)])

    # ------------------------------------------------------------------ MI355X paths
    def _forward_batched(self, x, samples, sample0, *args, **kwargs):
        """One pass, all samples per layer launch.  Returns the list of per-sample outputs
        (views of one (S*B, ...) tensor)."""
        ys = self._forward_batched_stacked(x, samples, sample0, *args, **kwargs)
        if isinstance(ys, tuple):
            # a tuple-valued head (NormalInverseGaussianLinear): S tuples, as the serial loop returns
            return list(zip(*[t.unbind(0) for t in ys]))
        return list(ys.unbind(0))

    def predictive_mean(self, x, samples=None, sample0=0, out=None, scale=None, advance=None, kl=None, *args,
                        propagation='samples', covariance=False, **kwargs):
        """scale (default 1 / samples) * sum over the MC samples of `_forward(x)` -- torch.stack(preds).mean(0) of
        examples/MNIST/uncertainty.py:50 -- as the tail of ONE batched pass: the caller wants the mean, not the samples, so a
        hidden layer may run fused with the classifier head behind it (nn.fuse_activations; bnn_dense_forward_head) and the
        reduction adds that pair's partial logits in the same launch.  out / advance / kl: as ops.mc_mean.
        propagation='moments': the samples are drawn from ONE sampling-free pass (predictive_moments; _moment_outputs)."""
        from .. import ops
        if samples is None:
            samples = self.samples
        tail = self.mc_batched and _on_device(x)                    # the device launch reduces; else the sum below
        if _moments_asked(propagation, "predictive_mean", None, covariance):
            ys = self._moment_outputs("predictive_mean", x, samples, sample0, kl, args, kwargs, covariance)
            tail, kl = ys.is_cuda, None                             # _moment_outputs has taken kl
            if not tail:
                _refuse_cpu_tails("predictive_mean", "advance is a tail", advance)
        elif tail:
            ys = self._forward_batched_stacked(x, samples, sample0, *args, _lazy_head=True, **kwargs)
        else:
            ys = self.forward_stacked(x, samples, sample0, *args, **kwargs)
        scale = (1.0 / samples) if scale is None else scale
        return ops.mc_mean(ys, out=out, scale=scale, advance=advance, kl=kl) if tail else _scaled_sum(ys, scale, out)

    def predictive_uncertainty(self, x, samples=None, sample0=0, *, inputs, advance=None, kl=None, propagation='samples',
                               covariance=False, **kwargs):
        """Predictive mean and uncertainty of `samples` MC draws of `_forward(x)` -> ops.PredictiveUncertainty(mean, total,
        aleatoric, epistemic): total = H(mean), aleatoric = mean over samples of H(p_s), epistemic = total - aleatoric (the
        mutual information, BALD).  inputs: 'logits' (p_s = softmax of the outputs) or 'probs' (outputs used as given, e.g. a
        net ending in torch.nn.Softmax) -- required.  Draws are consumed as by predictive_mean with the same arguments.
          mc_batched on CUDA: one batched pass (a hidden layer fused with its head hands on partial logits) + ONE
                              bnn_mc_uncertainty launch, which also runs the `advance` / `kl` tails (as ops.mc_mean);
          other CUDA:         forward_stacked (the serial loop), then the same launch;
          CPU:                forward_stacked, then ops.uncertainty_f64 (the same formulas in float64).
        propagation='moments': the `samples` logits are drawn from ONE sampling-free pass (predictive_moments; _moment_outputs)
        instead of `samples` stochastic forwards; the tail is the same.  covariance=True (with propagation='moments' only, else
        ValueError; the same keyword on predictive_mean / _score / _regression / _regression_score): the logits are drawn
        CORRELATED from the head's N x N covariance (predictive_moments(covariance=True), bnn_moments_sample_cov) -- the mutual
        information depends on how the logits move together; the default draws them independent, as before."""
        from .. import ops
        ops._unc_kind(inputs, "predictive_uncertainty", kl)         # before a draw is consumed
        moments = _moments_asked(propagation, "predictive_uncertainty", kl, covariance)
        if not _on_device(x):
            _refuse_cpu_tails("predictive_uncertainty", "advance / kl are tails", advance, kl)
            return ops.uncertainty_f64(self._tail_inputs("predictive_uncertainty", x, samples, sample0, moments, kl, kwargs, covariance), inputs)
        y = self._tail_inputs("predictive_uncertainty", x, samples, sample0, moments, kl, kwargs, covariance)
        return ops.mc_uncertainty(y, inputs, advance=advance, kl=kl)

    def predictive_score(self, x, target, samples=None, sample0=0, *, inputs, state=None, advance=None, propagation='samples',
                         covariance=False, **kwargs):
        """`samples` MC draws of `_forward(x)` scored against the labels `target` (int64, one per row) -> ops.PredictiveScore(mean,
        nll, expected_nll, brier, confidence, prediction, entropy): nll = -ln mean[y] of the MC predictive, expected_nll the mean
        per-sample NLL (the ELBO's data term), brier, the confidence max_c mean[c] with its class, and H(mean).  inputs: 'logits'
        or 'probs' as predictive_uncertainty -- required.  state: an ops.ScoreState on x's device that this batch is added to, so
        that one state carries a test set (accuracy, NLL, Brier, ECE / MCE with the reliability diagram, the accuracy-rejection
        curve: ScoreState.result(), the only host copy).  Draws are consumed as by predictive_mean with the same arguments.
          mc_batched on CUDA: one batched pass (a hidden layer fused with its head hands on partial logits) + ONE bnn_mc_score
                              launch (two with a state), which also runs the `advance` tail (as ops.mc_mean);
          other CUDA:         forward_stacked (the serial loop), then the same launch;
          CPU:                forward_stacked, then ops.score_f64 (the same formulas in float64), added to a CPU state.
        propagation='moments': as predictive_uncertainty."""
        from .. import ops
        ops._unc_kind(inputs, "predictive_score")                   # before a draw is consumed
        moments = _moments_asked(propagation, "predictive_score", None, covariance)
        if not _on_device(x):
            _refuse_cpu_tails("predictive_score", "advance is a tail", advance)
            _refuse_device_state("predictive_score", state, ops.ScoreState)
            cb, eb = (state.conf_bins, state.ent_bins) if state is not None else (15, 20)
            ys = self._tail_inputs("predictive_score", x, samples, sample0, moments, None, kwargs, covariance)
            out, vec = ops.score_f64(ys, target, inputs, cb, eb)
            if state is not None:
                state.add_(vec)
            return out
        y = self._tail_inputs("predictive_score", x, samples, sample0, moments, None, kwargs, covariance)
        return ops.mc_score(y, target, inputs, state=state, advance=advance)

    def predictive_regression(self, x, samples=None, sample0=0, *, outputs, advance=None, kl=None, propagation='samples',
                              covariance=False, **kwargs):
        """Predictive mean and variance decomposition of `samples` MC draws of a real-valued `_forward(x)` ->
        ops.PredictiveRegression(mean, total, aleatoric, epistemic), each (*rows, D): the moments of the equal-weight mixture of
        the per-sample predictives -- aleatoric = mean of the per-sample variances, epistemic = variance of the per-sample means,
        total = their sum.  outputs: 'values' (point predictions: aleatoric is 0), 'mean_logvar' (D means then D log-variances,
        what nn.GaussianNLL trains) or 'mean_var' (D means then D variances) -- required.  Draws are consumed as by
        predictive_mean with the same arguments.
          mc_batched on CUDA: one batched pass (a hidden layer fused with its <= 16-wide head hands on partials) + ONE
                              bnn_mc_regression launch, which also runs the `advance` / `kl` tails (as ops.mc_mean);
          other CUDA:         forward_stacked (the serial loop), then the same launch;
          CPU:                forward_stacked, then ops.regression_f64 (the same formulas in float64).
        propagation='moments': as predictive_uncertainty -- except outputs='values', which needs no sampling: the propagated
        moments ARE the answer (mean, total = epistemic = var, aleatoric = 0), `samples` is not used and nothing is drawn."""
        from .. import ops
        ops._reg_kind(outputs, "predictive_regression", kl)         # before a draw is consumed
        moments = _moments_asked(propagation, "predictive_regression", kl, covariance)
        if moments and outputs == 'values':
            if advance is not None:
                raise ops.BnnHipError("predictive_regression: outputs='values' with propagation='moments' has no tail launch "
                                      "to run `advance` in")
            self._moment_refusals("predictive_regression", kl)
            mom = self.predictive_moments(x, covariance=covariance, **kwargs)
            if mom.dropout is not None:
                raise ops.BnnHipError("predictive_regression: outputs='values' with propagation='moments' reads the propagated "
                                      "moments as they are; these are the PRE-dropout moments of an MC-dropout head whose mask "
                                      "(dropout=%r) is still to be applied to samples, in front of a %s link"
                                      % (mom.dropout, mom.link))
            if mom.link is not None:
                raise ops.BnnHipError("predictive_regression: outputs='values' with propagation='moments' reads the propagated "
                                      "moments as they are; this network ends in a %s link" % mom.link)
            var = torch.zeros_like(mom.mean) if mom.var is None else mom.var
            return ops.PredictiveRegression(mom.mean, var, torch.zeros_like(mom.mean), var.clone())
        if not _on_device(x):
            _refuse_cpu_tails("predictive_regression", "advance / kl are tails", advance, kl)
            return ops.regression_f64(self._tail_inputs("predictive_regression", x, samples, sample0, moments, kl, kwargs, covariance), outputs)
        y = self._tail_inputs("predictive_regression", x, samples, sample0, moments, kl, kwargs, covariance)
        return ops.mc_regression(y, outputs, advance=advance, kl=kl)

    def predictive_regression_score(self, x, target, samples=None, sample0=0, *, outputs, state=None, advance=None,
                                    propagation='samples', covariance=False, **kwargs):
        """`samples` MC draws of a real-valued `_forward(x)` scored against the targets `target` (*rows, D) ->
        ops.RegressionScore(mean, variance, sq_err, nll, gaussian_nll, crps, pit), each (*rows, D): the proper scores of the MC
        predictive -- the equal-weight mixture of the per-sample Gaussians -- and its probability integral transform.  outputs:
        'values', 'mean_logvar' or 'mean_var' as predictive_regression -- required.  state: an ops.RegressionScoreState on x's
        device that this batch is added to, so that one state carries a test set (RMSE, NLL, CRPS, sharpness, the PIT histogram
        with the calibration curve and interval coverage: RegressionScoreState.result(), the only host copy).  Draws are consumed
        as by predictive_mean with the same arguments.  Not covered: the evidential head's Student-t predictive, a KL tail,
        more than 1024 samples.
          mc_batched on CUDA: one batched pass (a hidden layer fused with its <= 16-wide head hands on partials) + ONE
                              bnn_mc_regression_score launch (two with a state), which also runs the `advance` tail;
          other CUDA:         forward_stacked (the serial loop), then the same launch;
          CPU:                forward_stacked, then ops.regression_score_f64 (the same formulas in float64), added to a CPU state.
        propagation='moments': as predictive_uncertainty."""
        from .. import ops
        ops._reg_kind(outputs, "predictive_regression_score")       # before a draw is consumed
        moments = _moments_asked(propagation, "predictive_regression_score", None, covariance)
        if not _on_device(x):
            _refuse_cpu_tails("predictive_regression_score", "advance is a tail", advance)
            _refuse_device_state("predictive_regression_score", state, ops.RegressionScoreState)
            bins = state.pit_bins if state is not None else 20
            ys = self._tail_inputs("predictive_regression_score", x, samples, sample0, moments, None, kwargs, covariance)
            out, mat = ops.regression_score_f64(ys, target, outputs, bins)
            if state is not None:
                state.add_(mat)
            return out
        y = self._tail_inputs("predictive_regression_score", x, samples, sample0, moments, None, kwargs, covariance)
        return ops.mc_regression_score(y, target, outputs, state=state, advance=advance)

    def predictive_evidential(self, x, samples=None, sample0=0, **kwargs):
        """Predictive mean and variance decomposition of `samples` MC draws of a network whose `_forward(x)` ends in an
        evidential head and returns its (gamma, upsilon, alpha, beta) -> ops.PredictiveRegression(mean, total, aleatoric,
        epistemic), each (*rows, D): the moments of the equal-weight mixture of the S heads -- aleatoric = mean of the heads'
        beta / (alpha - 1), epistemic = mean of the heads' beta / (upsilon (alpha - 1)) plus the variance of gamma over the
        draws of the trunk, total = their sum.  samples = 1 gives gamma and NormalInverseGaussianUncertainty's two outputs.
        Draws are consumed as by predictive_regression with the same arguments.
          mc_batched on CUDA: one batched pass + ONE bnn_mc_evidential launch;
          other CUDA:         forward_stacked (the serial loop), then the same launch;
          CPU:                forward_stacked, then ops.evidential_f64 (the same formulas in float64)."""
        from .. import ops
        if samples is None:
            samples = self.samples
        ys = self.forward_stacked(x, samples, sample0, **kwargs)
        if not (isinstance(ys, tuple) and len(ys) == 4):
            raise ValueError("predictive_evidential: _forward must return (gamma, upsilon, alpha, beta), got %s"
                             % type(ys).__name__)
        if not _on_device(x):
            return ops.evidential_f64(*ys)
        return ops.mc_evidential(*ys)

    def predictive_moments(self, x, *args, covariance=False, **kwargs):
        """Sampling-free inference: ONE pass of `_forward(x)` that carries a mean and a variance per activation through the
        network (moment propagation: Frey & Hinton 1999; Hernandez-Lobato & Adams 2015; Wu et al. 2019) -> ops.Moments(mean, var)
        of the output, fp32.  Every NormalLinear / LocalReparamLinear runs as ops.moments_linear (one bnn_moments_forward launch
        beside its operand launch, both compute modes; ReLU folded by nn.fuse_activations is moment-matched in that launch); the
        cost does not depend on a sample count and no mc_batched is needed.  With ONE hidden ReLU layer every output's marginal
        mean and variance are exact; from the second hidden layer on the recursion treats a layer's inputs as independent
        Gaussians (the usual diagonal-covariance approximation); the outputs' covariance is carried only with covariance=True (below).
        NormalConv1d / 2d / 3d and LocalReparamConv1d / 2d / 3d run as ops.moments_convNd (K17: per output element the marginal
        moments are exact for a deterministic input; the correlation between the positions of an output map is dropped);
        VariationalDropoutLinear and VariationalDropoutConv1d / 2d / 3d as ops.moments_linear_vd / ops.moments_convNd_vd (K23, K24:
        the same launches on the planes theta and exp(log_sigma2), masked by the layer's threshold).
        Supported: those layers, ReLU folded into the dense ones by nn.fuse_activations, what nn.moment_activations rewrites
        (ReLU, ELU, a torch.nn.Linear behind a Bayesian layer, a Softmax over the last axis that ends the network: the result
        then carries link='softmax' and holds the LOGIT moments; K20: max / average / adaptive average pooling 1d / 2d / 3d and
        an eval-mode BatchNorm1d / 2d / 3d behind a Bayesian layer -- ops.moments_pool, ops.moments_batchnorm), modules that only
        reshape (torch.nn.Flatten, x.view),
        torch.nn.Identity, and any deterministic module in FRONT of the first Bayesian layer; anything else raises
        ops.BnnHipError.  A `_forward` that
        returns a plain tensor gives it back with var None.  CPU tensors: the same recursion in float64 (ops.moments_f64),
        rounded to fp32 at the end.  Inference only: nothing is drawn, no draw epoch is consumed, no key is recorded, and the
        result is detached whatever the grad mode.
        K21: MultivariateNormalLinear (the CIFAR10 example's head) runs as ops.moments_mvn_linear -- the exact moments of its own
        sampler (uniform noise through the element-wise square root of the triangle) for independent inputs.  covariance=True:
        the result also carries cov (*rows, N, N), the covariance of the N outputs of a row, from ONE bnn_moments_head_cov launch:
        the outputs of a dense head share their input, Cov(y_o, y_p) = sum_k E[w_ok] E[w_pk] Var[a_k] (+ an MVN head's bias
        covariance).  With one hidden layer and a deterministic input the hidden activations are independent and cov is exact.
        The network must end in a dense layer of at most 32 outputs (NormalLinear, LocalReparamLinear, nn.MomentLinear,
        MultivariateNormalLinear), with nothing but a closing nn.MomentSoftmax behind it; otherwise ops.BnnHipError says why.
        ops.moments_sample and the predictive_* tails (covariance=True) draw correlated outputs from it.
        K22, with nn.moment_estimator_layers() switched on (off by default: these layers are then refused as before):
        MCDropoutLinear and MCDropoutConv1d / 2d / 3d run their deterministic contraction on the moments (ops.moments_affine /
        ops.moments_conv_affine; the layer's own linear / conv on a deterministic input) and then ONE bnn_moments_dropout launch
        that pushes the mask through the ReLU / ELU nn.moment_activations found behind the layer (the identity without one):
        mean' = q M, var' = q V + q p M^2 with (M, V) the activation's moments at N(m / q, v / q^2) -- exact for a Gaussian
        pre-activation and for a deterministic one, so a net of the Titanic example's shape has exact logit moments.  An
        MC-dropout layer directly in front of the closing nn.MomentSoftmax hands on its PRE-dropout moments and the result carries
        dropout = p: the predictive_* tails mask the drawn logits (keyed masks on a model-level stream, model.moment_mask_key).
        FlipoutNormalLinear runs NormalLinear's pass on its parameters (its sign sampler's own marginal mean and variance);
        FlipOutNormalConv1d / 2d / 3d run NormalConv's, the moments of the weight posterior N(mu, sigma^2) that KLDivergence
        regularises (the reference's conv sign sampler shares one sign per input channel across the kernel taps, so its own
        marginal variance, sum_c (sum_tap x sigma)^2, differs from the posterior's sum x^2 sigma^2).  covariance=True is refused
        at a head of these kinds.
        Not covered: the backward of K21, covariance between hidden activations or conv positions, non-default priors, the
        evidential head."""
        from .. import ops
        from .dense import NormalLinear, LocalReparamLinear, MultivariateNormalLinear, VariationalDropoutLinear
        from .conv import (NormalConv1d, NormalConv2d, NormalConv3d, LocalReparamConv1d, LocalReparamConv2d, LocalReparamConv3d,
                           VariationalDropoutConv1d, VariationalDropoutConv2d, VariationalDropoutConv3d)
        admitted = (NormalLinear, LocalReparamLinear, VariationalDropoutLinear, MultivariateNormalLinear, NormalConv1d, NormalConv2d, NormalConv3d,
                    LocalReparamConv1d, LocalReparamConv2d, LocalReparamConv3d, VariationalDropoutConv1d, VariationalDropoutConv2d,
                    VariationalDropoutConv3d) + _estimator_layers()
        for m in self.modules():
            if isinstance(m, BayesianModule) and type(m) not in admitted:
                raise ops.BnnHipError("predictive_moments: %s is not supported; %s" % (type(m).__name__, _moments_supported()))
        with torch.no_grad(), _mc.MomentContext(covariance=covariance) as mctx:
            try:
                y = self._forward(x, *args, **kwargs)
            except (TypeError, AttributeError) as e:
                raise ops.BnnHipError("predictive_moments: a module of this network cannot take a mean and a variance (%s); %s"
                                      % (e, _moments_supported())) from e
        if torch.is_tensor(y):
            y = ops.Moments(y.detach(), None)
        if not isinstance(y, ops.Moments):
            raise ops.BnnHipError("predictive_moments: _forward returned %s; %s" % (type(y).__name__, _moments_supported()))
        _refuse_pending(y, "predictive_moments")
        if covariance:
            if y._head is None:
                dense = mctx.last_dense
                from .dense import MOMENT_ESTIMATOR_LAYERS
                if dense is not None and dense[0] in MOMENT_ESTIMATOR_LAYERS:
                    raise ops.BnnHipError("predictive_moments: covariance=True is not covered at a %s head: an MC-dropout layer's "
                                          "outputs are uncorrelated only through masks that the covariance launch does not know, and "
                                          "a Flipout layer's outputs share their signs (K21 carries the covariance of NormalLinear, "
                                          "LocalReparamLinear, nn.MomentLinear and MultivariateNormalLinear heads)" % dense[0])
                if dense is None:
                    why = "its last layer is not dense: the pass went through no dense layer at all"
                elif dense[1] > ops.HEAD_COV_MAX_N and y.dim() and y.shape[-1] == dense[1]:
                    why = "its head %s has %d outputs" % dense
                else:
                    why = ("something stands behind its last dense layer %s (a folded ReLU, an activation or another module): the "
                           "covariance is carried at the head only" % dense[0])
                raise ops.BnnHipError("predictive_moments: covariance=True needs the network to end in a dense layer of at most %d outputs "
                                      "(NormalLinear, LocalReparamLinear, nn.MomentLinear, MultivariateNormalLinear; a closing "
                                      "nn.MomentSoftmax may follow); %s" % (ops.HEAD_COV_MAX_N, why))
            y = ops.moments_resolve_cov(y)
        if not y.mean.is_cuda:
            return ops.Moments(y.mean.to(torch.float32), None if y.var is None else y.var.to(torch.float32), y.link,
                               cov=None if y.cov is None else y.cov.to(torch.float32), dropout=y.dropout)
        return y

    def _moment_refusals(self, who, kl):
        from .. import ops
        if kl is not None:
            ops._kl_uncarry(kl)
            raise ops.BnnHipError("%s: propagation='moments' draws no weights and has no KL tail (kl=)" % who)
        if any(m.__dict__.get("_fuse_head") is not None for m in self.modules()):
            raise ops.BnnHipError("%s: propagation='moments' has no fused head: this network was rewritten with "
                                  "nn.fuse_activations(fuse_head=True), whose hidden layer hands on partial logits" % who)

    def _moment_outputs(self, who, x, samples, sample0, kl, args, kwargs, covariance=False):
        """propagation='moments': what a predictive_* tail reads -- the (S, *rows, C) outputs drawn from the propagated moments
        by ONE bnn_moments_sample launch, independent across outputs, on a model-level noise stream (its id is taken at first
        use, so that a model's layers keep theirs; the key is recorded as model.moment_key).  CPU: torch.randn."""
        self._moment_refusals(who, kl)
        mom = self.predictive_moments(x, *args, covariance=covariance, **kwargs)
        return self._sample_link(mom, samples, sample0, False)

    def _sample_link(self, mom, samples, sample0, track):
        """`samples` draws from the output moments on the model's moment stream, through the link the moments carry."""
        from .. import ops
        from .._rng import DrawKey, default_generator, generator_for, new_stream_id
        from . import _settings
        link = (lambda ys: torch.softmax(ys, -1)) if mom.link == 'softmax' else (lambda ys: ys)
        p = mom.dropout                      # K22: the mask of an MC-dropout head, applied to the drawn logits in front of the link
        if not mom.mean.is_cuda:
            ys = ops.moments_sample(mom, None, samples, track)
            if p is not None:                # F.dropout's mask and scale, one mask per sample, row and logit
                ys = ys * (torch.rand(ys.shape) >= p).to(ys.dtype) * (0.0 if p >= 1.0 else 1.0 / (1.0 - p))
            return link(ys)
        if self.__dict__.get("_moment_stream") is None:
            self.__dict__["_moment_stream"] = new_stream_id()
        key = DrawKey(default_generator.seed, self.__dict__["_moment_stream"], sample0, samples, default_generator.next_epoch(),
                      gen=generator_for(_settings.get_compute()))
        self.__dict__["moment_key"] = key
        ys = ops.moments_sample(mom, key, samples, track)
        if p is not None:
            # the keyed masks of the mask contract on a model-level stream of its own (taken at first use), the key on the moment
            # key's seed, epoch and sample0: sample s = row // rows of the (S * rows, ...) stack; bnn_mc_dropout_backward when tracked
            if self.__dict__.get("_moment_mask_stream") is None:
                self.__dict__["_moment_mask_stream"] = new_stream_id()
            mkey = DrawKey(key.seed, self.__dict__["_moment_mask_stream"], sample0, samples, key.epoch_host, gen=key.gen)
            self.__dict__["moment_mask_key"] = mkey
            flat = ys.reshape((-1,) + tuple(ys.shape[2:])) if ys.dim() > 2 else ys
            flat = flat if track and torch.is_grad_enabled() else flat.detach()
            ys = ops.mc_dropout(flat, p, mkey, shared=False).reshape(ys.shape)
        return link(ys)

    def forward_moments(self, x, *args, **kwargs):
        """Training without sampling (Wu et al. 2019): predictive_moments' ONE pass of `_forward(x)` with its autograd graph ->
        ops.Moments(mean, var) of the output, attached to the input and to every posterior tensor.  Nothing is drawn, no key is
        recorded; the gradient of a loss on the moments is deterministic.  Device: fp32 moments, every backward launch is HIP
        (K18, csrc/bnn_moments_bwd.hip; the first layer's deterministic input takes K10's).  CPU: the float64 recursion under
        torch autograd, float64 moments.  Admitted: NormalLinear, LocalReparamLinear, ReLU folded into them
        (nn.fuse_activations) or rewritten to nn.MomentReLU (nn.moment_activations), reshapes, torch.nn.Identity, a closing
        nn.MomentSoftmax, deterministic modules in front of the first Bayesian layer.  The conv layers, nn.MomentELU,
        nn.MomentLinear and the Flipout / MC-dropout / multivariate-normal / evidential layers raise ops.BnnHipError.
        With nn.conv_moment_training() switched on (K19) NormalConv1d / 2d / 3d, LocalReparamConv1d / 2d / 3d, nn.MomentELU and
        nn.MomentLinear are admitted too: the conv backward is k_moments_conv3d_bwd (csrc/bnn_conv3d.hip; K11's launches for a
        deterministic input), the ELU's bnn_moments_elu_backward, MomentLinear's K18's two launches; the other layers stay refused.
        The pooling twins nn.MomentMaxPool / MomentAvgPool / MomentAdaptiveAvgPool 1d / 2d / 3d (K20) are admitted with no switch:
        their backward is bnn_moments_pool3d_backward; nn.MomentBatchNorm1d / 2d / 3d has no backward and is refused by name.
        With nn.moment_estimator_layers() switched on (K22) MCDropoutLinear and FlipoutNormalLinear are admitted, and nn.MomentELU
        with them; MCDropoutConv / FlipOutNormalConv 1d / 2d / 3d when nn.conv_moment_training() is on as well.  The mask's
        backward is bnn_moments_dropout_backward, the deterministic contractions' K18's / K19's launches with a zero sigma^2
        plane; a mask handed to sample_moments (an MC-dropout head in front of the softmax) has bnn_mc_dropout_backward.
        Regression: mean(((y - mom.mean)^2 + mom.var) / (2 s^2)) needs no sample; classification: sample_moments."""
        from .. import ops
        from . import _settings
        from .dense import NormalLinear, LocalReparamLinear
        from .conv import (NormalConv1d, NormalConv2d, NormalConv3d, LocalReparamConv1d, LocalReparamConv2d, LocalReparamConv3d)
        convs_on = _settings.conv_moment_training_enabled()
        admitted = (NormalLinear, LocalReparamLinear) + ((NormalConv1d, NormalConv2d, NormalConv3d, LocalReparamConv1d,
                                                           LocalReparamConv2d, LocalReparamConv3d) if convs_on else ())
        # K22 (nn.moment_estimator_layers): the dense estimator layers, and their conv forms with nn.conv_moment_training
        admitted += tuple(c for c in _estimator_layers() if convs_on or "Conv" not in c.__name__)
        for m in self.modules():
            if isinstance(m, _MOMENT_BATCHNORMS):                                   # (named first, whatever else the network holds)
                raise ops.BnnHipError("forward_moments: %s has no moment backward (K20 propagates moments through an eval-mode "
                                      "BatchNorm for inference only); the pooling twins nn.MomentMaxPool / MomentAvgPool / "
                                      "MomentAdaptiveAvgPool 1d / 2d / 3d have one" % type(m).__name__)
        for m in self.modules():
            # (K22: with nn.moment_estimator_layers on, nn.MomentELU is admitted without nn.conv_moment_training -- behind an
            # MC-dropout layer it only passes on what bnn_moments_dropout computed, elsewhere its backward is K19's launch)
            if (isinstance(m, BayesianModule) and type(m) not in admitted) or (
                    not convs_on and isinstance(m, (MomentLinear,) if _estimator_layers() else (MomentELU, MomentLinear))):
                raise ops.BnnHipError("forward_moments: %s has no moment backward; training without sampling supports "
                                      "NormalLinear / LocalReparamLinear, ReLU (folded, or nn.MomentReLU), reshaping modules, "
                                      "torch.nn.Identity and a closing nn.MomentSoftmax%s" % (type(m).__name__, (
                                          ", and (nn.conv_moment_training) NormalConv / LocalReparamConv 1d / 2d / 3d, nn.MomentELU "
                                          "and nn.MomentLinear") if convs_on else ""))
        with _mc.MomentContext(track=True):
            try:
                y = self._forward(x, *args, **kwargs)
            except (TypeError, AttributeError) as e:
                raise ops.BnnHipError("forward_moments: a module of this network cannot take a mean and a variance (%s); %s"
                                      % (e, _moments_supported())) from e
        if torch.is_tensor(y):
            y = ops.Moments(y, None)
        if not isinstance(y, ops.Moments):
            raise ops.BnnHipError("forward_moments: _forward returned %s; %s" % (type(y).__name__, _moments_supported()))
        _refuse_pending(y, "forward_moments")
        return y

    def sample_moments(self, mom, samples=None, sample0=0):
        """`samples` (default self.samples) independent draws from forward_moments' output, (S, *rows, C), differentiable in
        the moments: ONE bnn_moments_sample launch on the model's moment stream (a fresh epoch per call, the key recorded as
        model.moment_key; its backward re-creates eps from that key), torch.softmax applied when the moments carry
        link='softmax'.  Classification trains on these cheap sampled outputs with the usual cross-entropy."""
        from .. import ops
        if not isinstance(mom, ops.Moments):
            raise TypeError("sample_moments: expected an ops.Moments, got %s" % type(mom).__name__)
        if mom.cov is not None:
            raise ops.BnnHipError("sample_moments: moments that carry a covariance have no backward; ops.moments_sample draws from them "
                                  "at inference")
        return self._sample_link(mom, self.samples if samples is None else samples, sample0, True)

    def _tail_inputs(self, who, x, samples, sample0, moments, kl, kwargs, covariance=False):
        """The (S, *rows, C) outputs a predictive_* tail reads.  `moments`: drawn from the propagated moments (_moment_outputs).
        Else `samples` stochastic forwards: for x on the device with mc_batched one batched pass whose fused head, if any, hands
        on its partials (ops.HeadPartials); otherwise the stacked outputs of the serial loop."""
        if samples is None:
            samples = self.samples
        if moments:
            return self._moment_outputs(who, x, samples, sample0, kl, (), kwargs, covariance)
        if self.mc_batched and _on_device(x):
            return self._forward_batched_stacked(x, samples, sample0, _lazy_head=True, **kwargs)
        return self.forward_stacked(x, samples, sample0, **kwargs)

    def _forward_batched_stacked(self, x, samples, sample0, *args, _lazy_head=False, **kwargs):
        B = x.shape[0]
        with _mc.McContext(samples, B, sample0) as ctx:
            ctx.lazy_head = _lazy_head
            drawn = self._draw_plan(ctx, x)
            try:
                y = self._forward(x, *args, **kwargs)
            finally:
                for m in drawn:
                    m._predrawn = None
        from .. import ops
        if isinstance(y, ops.HeadPartials):
            return y if _lazy_head else y.logits()
        if isinstance(y, tuple) and y and all(isinstance(t, torch.Tensor) for t in y):
            return tuple(self._stack_samples(t, samples, B) for t in y)
        return self._stack_samples(y, samples, B)

    @staticmethod
    def _stack_samples(y, samples, B):
        if y.shape[0] == B * samples:
            return y.view(samples, B, *y.shape[1:])
        if y.shape[0] == B:
            # no Bayesian layer saw the batch: every draw is the same deterministic output
            return y.unsqueeze(0).expand(samples, *y.shape)
        raise RuntimeError("mc_batched: _forward returned %d rows for batch %d x %d samples"
                           % (y.shape[0], B, samples))

    def _draw_plan(self, ctx, x=None):
        """bf16 compute mode: the posteriors of EVERY NormalLinear of the network are drawn for this forward's S samples
        in ONE launch (ops.draw_layers -> bnn_draw_multi) before `_forward` runs; each layer then finds its drawn
        weights (consumed on first use: a layer called twice draws again, like the reference's per-call sample(),
        dense.py:56-58).  The plan itself leaves the layers' state alone: the keys travel in the Predrawn entry and a layer
        records them -- exactly as its own sample() would -- when it uses the entry.  Returns the layers it drew for."""
        from .. import ops
        from . import _settings
        from .. import _lib
        from .dense import NormalLinear, FlipoutNormalLinear, _flipout_fresh_key
        if not ops.DRAW_ONCE_BF16:
            return []
        todo, todo3, flips = [], [], []
        infer = not torch.is_grad_enabled()
        for m in self.modules():
            if type(m) is FlipoutNormalLinear and m.weight.mean.is_cuda and ops.flipout_drawable(m.weight.mean) and \
                    m._compute_mode() == "bf16":
                # its per-sample weights mu + sigma R_s S_s^T ride in the same launch (BNN_DRAW_FLIPOUT).  Like a NormalLinear's, the
                # draw is made on a fresh key before `_forward` runs: a layer then called with sample=False (or not at all) does not
                # use it -- it keeps its recorded flip_key -- and the draw (one item of this launch) is wasted work, not a wrong result
                flips.append(m)
                continue
            if type(m) is not NormalLinear or not m.weight.mean.is_cuda or not ops.dense_eligible(m.weight.mean):
                continue
            if (m.compute or _settings.get_compute()) == "bf16":
                todo.append(m)
            elif ops.DENSE_X3_F32 and (infer or not m._trainable()) and ctx.base_batch >= 64 and \
                    (m.weight.mean.shape[0] > 16 or m.weight.mean.shape[1] <= 2048):
                todo3.append(m)         # fp32 parity mode, inference: the same plan with three-plane draws (ops.linear_sampled_x3)
        if not todo and not todo3 and not flips:
            return []

        def specs_of(mods):
            # The plan draws on FRESH keys but does not touch the layers: a layer adopts its keys only when it consumes the
            # drawn weights with sample=True (NormalLinear.forward); one called with sample=False, or never reached by
            # `_forward`, keeps its recorded draw or its user-assigned `.sampled` (dense.py:56-58: `if sample: self.sample()`).
            specs = []
            for m in mods:
                kw, kb = m._fresh_keys(ctx.samples, ctx.sample0)
                specs.append((m.weight.mean.detach(), m.weight.scale.detach(),
                              m.bias.mean.detach() if m.bias is not None else None,
                              m.bias.scale.detach() if m.bias is not None else None, kw, kb))
            return specs

        kl = ops._tls.kl_carry
        pre = []
        if todo or flips:
            specs = specs_of(todo) + [(m.weight.mean.detach(), m.weight.scale.detach(), None, None, _flipout_fresh_key(m, ctx), None, 0, _lib.DRAW_FLIPOUT)
                                      for m in flips]
            todo = todo + flips
            pre = ops.draw_layers(specs, ctx.samples, kl=kl)
        if todo3:
            # fp32 parity mode: the network input's three bf16 planes (what the first dense layer would launch bnn_split_bf16x3
            # for) ride in the same launch; the layer that is called with this very tensor takes them (ctx.x_planes)
            split = None
            if x is not None and x.dim() == 2 and x.dtype == torch.float32 and x.is_cuda and x.stride(1) == 1 and x.is_contiguous() and \
                    x.shape[1] % 8 == 0 and x.data_ptr() % 16 == 0 and not (torch.is_grad_enabled() and x.requires_grad):
                split = x
            pre += ops.draw_layers(specs_of(todo3), ctx.samples, kl=kl if (kl is not None and not kl.launched) else None, x3=True, split=split)
            if split is not None and ops._tls.last_split is not None:
                ctx.x_planes = (x, ops._tls.last_split)
                ops._tls.last_split = None
        todo = todo + todo3
        if kl is not None and kl.launched:
            ops._tls.kl_carry = None
        for m, p_ in zip(todo, pre):
            m._predrawn = (ctx, p_)
        return todo

    def forward_stacked(self, x, samples=None, sample0=0, *args, **kwargs):
        """(S, B, ...) tensor of all MC outputs (batched path when enabled).  A tuple-valued `_forward` (an evidential head) gives
        a tuple of (S, B, ...) tensors; the serial loop stacks each component with one `torch.stack` copy (four for that head)."""
        if samples is None:
            samples = self.samples
        if self.mc_batched and isinstance(x, torch.Tensor) and x.is_cuda:
            return self._forward_batched_stacked(x, samples, sample0, *args, **kwargs)
        out = [self._forward(x, *args, **kwargs) for _ in range(samples)]
        if out and isinstance(out[0], tuple):
            return tuple(torch.stack(ts) for ts in zip(*out))       # a tuple-valued head: each component stacked
        return torch.stack(out)
