"""Convolutional Bayesian layers (pytorch_bayesian/nn/conv.py).

NormalConv2d is the hot path: an implicit-GEMM MFMA kernel whose B-operand loader draws the
filter bank (bnn_conv2d_forward_sampled).  NormalConv1d runs on the same kernels (images of height 1).  NormalConv3d draws
all S MC samples in one launch and contracts them in one implicit-GEMM launch, backward included (bnn_conv3d_forward_drawn,
csrc/bnn_conv3d.hip).  The FlipOut variants run on HIP on the device (2-d, 1-d as 2-d at height 1, and 3-d with groups == 1 on
the Flipout tiles of csrc/bnn_conv3d.hip); in a network's
MC-batched device pass their signs are keyed per MC sample (bnn_conv2d_flipout_forward_mc, bnn_flipout_signs).  The MC-dropout
variants run their torch conv once and apply the keyed masks of a network's MC-batched device pass in HIP (bnn_mc_dropout).
LocalReparamConv1d / 2d / 3d (not reference names) sample the Gaussian pre-activation instead of the weights: one operand launch
and ONE paired-contraction launch for all S samples (bnn_conv3d_lrt_forward; 1-d and 2-d as unit depth / height), HIP backward.
VariationalDropoutConv1d / 2d / 3d (not reference names either) are sparse variational dropout on those kernels: the posterior
N(theta, exp(log_sigma2)) under a log-uniform prior (bnn_vd_prepare, bnn_conv3d_vd_backward_weight; K24).
"""
import math

import torch
from torch.distributions import Normal
from torch.nn import init

from .. import _mc, ops
from . import _settings
from ..utils import _single, _pair, _triple
from .container import BayesianModule
from .core import WeightNormal
from .dense import (_NormalSampling, _init_normal_posterior, _mc_dropout_plan, _mc_dropout_key, _flipout_plan, _flipout_mc_key,
                    _lrt_noise_plan, _mc_dropout_forward_moments, _LrtNoise, _CONV_WORDING)


class BayesianConvNd(BayesianModule):
    """conv.py:9-40."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation,
                 transposed, groups, bias, weight, prior, bias_prior=None):
        super().__init__(in_channels, out_channels, prior, bias_prior)
        # conv.py:15-18
        if in_channels % groups != 0:
            raise ValueError('in_channels must be divisible by groups')
        if out_channels % groups != 0:
            raise ValueError('out_channels must be divisible by groups')
        self.kernel_size = kernel_size
        self.stride = stride
        self.padding = padding
        self.dilation = dilation
        self.transposed = transposed
        self.groups = groups
        if transposed:
            self.weight = weight(in_channels, out_channels // groups, *kernel_size)
        else:
            self.weight = weight(out_channels, in_channels // groups, *kernel_size)
        if bias:
            self.bias = weight(out_channels)
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        pass


def _conv_forward_moments(layer, x):
    """A Gaussian conv layer inside a moment pass (_mc.MomentContext; BayesianNetworkModule.predictive_moments): x a tensor (a
    deterministic input) or an ops.Moments, (B, C, *spatial) or one image (C, *spatial) -> the ops.Moments of the output, with
    the moment-matched activation in the launch's epilogue when nn.moment_activations found one directly behind the layer
    (layer._moment_act; the twin module then passes the result through).  Device: ops.moments_convNd
    (bnn_conv3d_moments_forward, fp32 moments in both compute modes); CPU: the same recursion in float64
    (ops.moments_convNd_f64).  Nothing is drawn, no draw epoch is consumed, draw_key / noise_key stay as they are; the result
    is detached in an inference pass and keeps its autograd graph in a tracked one (BayesianNetworkModule.forward_moments, K19)."""
    mom = x if isinstance(x, ops.Moments) else ops.Moments(x, None)
    if not torch.is_tensor(mom.mean):
        raise TypeError("%s takes a tensor or ops.Moments in a moment pass, got %s" % (type(layer).__name__, type(x).__name__))
    ops._refuse_link(mom, type(layer).__name__)
    nd = layer.weight.mean.dim() - 2
    if mom.mean.dim() == nd + 1:
        out = _conv_forward_moments(layer, ops.Moments(mom.mean.unsqueeze(0), None if mom.var is None else mom.var.unsqueeze(0)))
        res = ops.Moments(out.mean.squeeze(0), out.var.squeeze(0))
        res._act = out._act
        return res
    act = layer.__dict__.get("_moment_act")
    b = layer.bias is not None
    args = (layer.weight.mean, layer.weight.scale, layer.bias.mean if b else None, layer.bias.scale if b else None,
            layer.stride, layer.padding, layer.dilation, layer.groups)
    ctx = _mc.moments_current()
    track = ctx is not None and ctx.track                              # forward_moments: keep the graph (K19)
    if not mom.mean.is_cuda:
        out = ops.moments_convNd_f64(mom, *args, activation=act, track=track)
    else:
        out = ops.moments_convNd(mom, *args, activation=act, compute=layer._compute_mode(), track=track)
    out._act = act
    return out


class NormalConvNd(_NormalSampling, BayesianConvNd):
    """conv.py:43-73.  Inside BayesianNetworkModule.predictive_moments NormalConv1d / 2d / 3d draw nothing: they take and
    return a mean and a variance per element (_conv_forward_moments, K17)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation,
                 transposed, groups, bias, prior):
        super().__init__(in_channels, out_channels, _single(kernel_size), stride, padding, dilation,
                         transposed, groups, bias, WeightNormal, prior)

    def reset_parameters(self):
        _init_normal_posterior(self)
        self.sample()

    def _forward_moments(self, x):
        return _conv_forward_moments(self, x)

    def _torch_conv(self, op, x, sample):
        if sample:
            self.sample()
        return op(x, *self.sampled, self.stride, self.padding, self.dilation, self.groups)


class NormalConv1d(NormalConvNd):
    """conv.py:76-96."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias=True, prior=Normal(0, .1)):
        super().__init__(in_channels, out_channels, _single(kernel_size), _single(stride),
                         _single(padding), _single(dilation), False, groups, bias, prior)

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            return self._forward_moments(x)                              # predictive_moments: moments in, moments out, no draw
        if not x.is_cuda or x.dim() not in (2, 3):
            return self._torch_conv(torch.nn.functional.conv1d, x, sample)
        # device: a 1-d convolution is the 2-d one on images of height 1 -- the same HIP kernels (implicit GEMM where the shape
        # allows it), the same draws (the flat element order of (O, C, k) and (O, C, 1, k) is the same)
        x3 = x.unsqueeze(0) if x.dim() == 2 else x
        y = _device_conv2d(self, x3.unsqueeze(2), lambda t: t.unsqueeze(2), (1,) + tuple(self.stride), (0,) + tuple(self.padding),
                           (1,) + tuple(self.dilation), sample).squeeze(2)
        return y.squeeze(0) if x.dim() == 2 else y


def _device_conv2d(layer, x, view, stride, padding, dilation, sample):
    """NormalConv2d.forward on the device (conv.py:112-119) for a layer whose weight tensors `view` turns into (O, C, KH, KW)."""
    S, _, shared, per = layer._mc_plan(x, sample)
    x5 = x if shared else x.reshape(S, per, *x.shape[1:])
    keys = layer._keys(S)
    mode = layer._compute_mode()
    if keys is not None:
        y = ops.conv2d_sampled(x5, view(layer.weight.mean), view(layer.weight.scale),
                               layer.bias.mean if layer.bias is not None else None,
                               layer.bias.scale if layer.bias is not None else None,
                               keys[0], keys[1], shared, stride, padding, dilation, layer.groups, mode)
    else:
        w, b = layer.sampled
        w = view(w)
        y = ops.conv2d_plain(x5, w.unsqueeze(0).expand(S, *w.shape),
                             None if b is None else b.unsqueeze(0).expand(S, -1), shared,
                             stride, padding, dilation, layer.groups, mode)
    return y.reshape(S * per, *y.shape[2:])


class NormalConv2d(NormalConvNd):
    """conv.py:99-119."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias=True, prior=Normal(0, .1)):
        super().__init__(in_channels, out_channels, _pair(kernel_size), _pair(stride),
                         _pair(padding), _pair(dilation), False, groups, bias, prior)

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            return self._forward_moments(x)                              # predictive_moments: moments in, moments out, no draw
        if not x.is_cuda:
            # CPU-resident module: the reference's own op sequence (conv.py:112-119)
            return self._torch_conv(torch.nn.functional.conv2d, x, sample)
        if x.dim() == 3:
            return self.forward(x.unsqueeze(0), sample).squeeze(0)
        return _device_conv2d(self, x, lambda t: t, self.stride, self.padding, self.dilation, sample)


class NormalConv3d(NormalConvNd):
    """conv.py:122-142."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias=True, prior=Normal(0, .1)):
        super().__init__(in_channels, out_channels, _triple(kernel_size), _triple(stride),
                         _triple(padding), _triple(dilation), False, groups, bias, prior)

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            return self._forward_moments(x)                              # predictive_moments: moments in, moments out, no draw
        if not x.is_cuda:
            # CPU-resident module: the reference's own op sequence (conv.py:138-142)
            return self._torch_conv(torch.nn.functional.conv3d, x, sample)
        if x.dim() == 4:
            return self.forward(x.unsqueeze(0), sample).squeeze(0)
        # device: every MC sample of the context on its own keyed draw -- one draw launch, one implicit-GEMM launch
        S, _, shared, per = self._mc_plan(x, sample)
        x6 = x if shared else x.reshape(S, per, *x.shape[1:])
        keys = self._keys(S)
        geo = (self.stride, self.padding, self.dilation, self.groups)
        if keys is not None:
            y = ops.conv3d_sampled(x6, self.weight.mean, self.weight.scale,
                                   self.bias.mean if self.bias is not None else None,
                                   self.bias.scale if self.bias is not None else None,
                                   keys[0], keys[1], shared, *geo, self._compute_mode())
        else:
            y = ops.conv3d_plain(x6, *self.sampled, S, shared, *geo, self._compute_mode())
        return y.reshape(S * per, *y.shape[2:])


class LocalReparamConvNd(_LrtNoise, _NormalSampling, BayesianConvNd):
    """The local-reparameterization estimator of NormalConvNd's posterior (Kingma, Salimans, Welling 2015; the conv variant of
    LocalReparamLinear).  With independent Gaussian w and b every output element of the convolution is Gaussian, so the layer
    samples IT instead of the weights:

        m   = convNd(x,   mu_w,      mu_b,      stride, padding, dilation, groups)
        v   = convNd(x^2, sigma_w^2, sigma_b^2, stride, padding, dilation, groups)        sigma = 1e-10 + softplus(rho)
        y_s = m + sqrt(v + 1e-16) eps_s,        eps_s ~ N(0, 1), one per output element and MC sample

    What the estimator is and is not: per output element y_s has EXACTLY the marginal mean and variance of weight sampling.  The
    weights of a convolution are shared by the positions of one image, so weight sampling correlates the positions of an output
    map and this layer does not -- the usual LRT-for-conv approximation.  It is a different estimator from Flipout too, which
    perturbs the weights per example.

    Parameters, initialisation and state_dict keys are NormalConvNd's (weight.mean, weight.scale, bias.mean, bias.scale): a
    checkpoint of one loads into the other, and KLDivergence, .kl_divergence(), traverse, apply_wb and PruneNormal see an ordinary
    Gaussian conv layer.  The network draw plan and nn.fuse_activations select by exact type and pass this layer by.

    Device input: bnn_lrt_prepare + bnn_conv3d_lrt_forward (csrc/bnn_conv3d.hip, k_lrt_conv3d; both compute modes; 1-d and 2-d
    layers on unit depth / height), fp32 output, HIP backward, no torch fallback (BnnHipError with the kernel's reason).  In a
    BayesianNetworkModule's MC-batched pass a layer that sees the shared batch (B rows) contracts m and v ONCE and returns S B
    rows; one that sees S B rows contracts per sample.  layer.noise_key is the DrawKey of the last device call, on a stream of
    the layer's own: element (b O + o) P + p of sample s is that eps of the key's sample sample0 + s (include/bnn_hip.h, LRT-conv
    noise contract).  sample=False reuses it.  CPU tensors: the expression above in torch with torch.randn_like.

    Inside BayesianNetworkModule.predictive_moments the layer is NormalConvNd's moment layer (same parameters, same bits)."""

    _op = None
    _nd = 0

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, prior):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, False, groups, bias, WeightNormal, prior)
        self._init_noise()                          # (_noise_shape: one sample's INPUT shape (B, C, *spatial); it fixes the output's)

    def reset_parameters(self):
        _init_normal_posterior(self)
        self.sample()

    def _forward_moments(self, x):
        return _conv_forward_moments(self, x)

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            return self._forward_moments(x)                              # predictive_moments: NormalConvNd's moment layer, no noise
        conv = type(self)._op
        geo = (self.stride, self.padding, self.dilation, self.groups)
        if not x.is_cuda:
            has_b = self.bias is not None
            m = conv(x, self.weight.mean, self.bias.mean if has_b else None, *geo)
            v = conv(x * x, self.weight.variance, self.bias.variance if has_b else None, *geo)
            return self._cpu_sample(m, v, sample)
        if x.dim() == self._nd + 1:
            return self.forward(x.unsqueeze(0), sample).squeeze(0)
        S, s0, shared, per = _lrt_noise_plan(x)
        mode = self._compute_mode()
        xs = x if shared else x.reshape(S, per, *x.shape[1:])
        key = self._call_key(sample, (per,) + tuple(x.shape[1:]), S, s0, mode, _CONV_WORDING)
        y = ops.convNd_lrt(xs, self.weight.mean, self.weight.scale,
                           self.bias.mean if self.bias is not None else None,
                           self.bias.scale if self.bias is not None else None, key, shared, *geo, mode)
        return y.reshape(S * per, *y.shape[2:])


def _local_reparam(name, ntuple, op, nd):
    class _LocalReparam(LocalReparamConvNd):
        _op = staticmethod(op)
        _nd = nd

        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                     groups=1, bias=True, prior=Normal(0, .1)):
            super().__init__(in_channels, out_channels, ntuple(kernel_size), ntuple(stride), ntuple(padding),
                             ntuple(dilation), groups, bias, prior)
    _LocalReparam.__name__ = _LocalReparam.__qualname__ = name
    return _LocalReparam


LocalReparamConv1d = _local_reparam('LocalReparamConv1d', _single, torch.nn.functional.conv1d, 1)
LocalReparamConv2d = _local_reparam('LocalReparamConv2d', _pair, torch.nn.functional.conv2d, 2)
LocalReparamConv3d = _local_reparam('LocalReparamConv3d', _triple, torch.nn.functional.conv3d, 3)


class VariationalDropoutConvNd(_LrtNoise, BayesianConvNd):
    """Sparse variational dropout for convolutions (Molchanov, Ashukha, Vetrov 2017; not a reference name; the conv variant of
    VariationalDropoutLinear): a conv layer that learns which of its weights -- and with them which whole filters -- to drop.
    Every weight has the posterior N(theta, sigma^2) -- `weight` is a WeightVariationalDropout (out, in / groups, *kernel) with
    Parameters mean (theta) and log_sigma2 -- and a log-uniform prior; the pre-activation is sampled by local
    reparameterization as LocalReparamConvNd samples it,

        m   = convNd(x,   theta,           mu_b,      stride, padding, dilation, groups)
        v   = convNd(x^2, exp(log_sigma2), sigma_b^2, stride, padding, dilation, groups)
        y_s = m + sqrt(v + 1e-16) eps_s,        eps_s ~ N(0, 1), one per output element and MC sample

    and KLDivergence / .kl_divergence() add the log-uniform KL of the weight (ops.vd_kl: every such tensor of a model, dense and
    conv, in one call; no prior argument: the prior is fixed) beside the Gaussian KL of the bias against `bias_prior`.  `bias` is
    None or a WeightNormal; state_dict keys weight.mean, weight.log_sigma2, bias.mean, bias.scale.  Initialisation: the mean as
    NormalConvNd's, log_sigma2 = -10, the bias as VariationalDropoutLinear's.

    Device input: bnn_vd_prepare + bnn_conv3d_lrt_forward (both compute modes; 1-d and 2-d layers on unit depth / height), fp32
    input and output; the backward is HIP (bnn_lrt_backward_epilogue, bnn_conv3d_lrt_backward_input,
    bnn_conv3d_vd_backward_weight); no torch conv and no torch fallback (BnnHipError with the kernel's reason).  In a
    BayesianNetworkModule's MC-batched pass a layer that sees the shared batch contracts m and v ONCE for all S samples, one that
    sees S B rows contracts per sample; noise_key and sample=False mean what they mean on LocalReparamConvNd (the LRT-conv noise
    contract of include/bnn_hip.h).  CPU tensors: the expression above in torch with torch.randn_like.

    threshold (an attribute, default None): with a float every path -- the sampling forward, the MC-batched pass, the moment
    pass -- drops the weights with log_alpha > threshold (theta = 0 and variance 0).  The mask is for inference: a call that would
    need a gradient of a posterior tensor while a threshold is set raises ops.BnnHipError.  sparsity() is the fraction of weights
    with log_alpha > threshold (3.0 while threshold is None), filter_sparsity() the fraction of output filters ALL of whose
    weights are: a filter that can be taken out of the layer.

    Inside BayesianNetworkModule.predictive_moments the layer is NormalConvNd's moment layer on the planes theta and
    exp(log_sigma2) (ops.moments_convNd_vd: bnn_conv3d_moments_forward, the ELU / ReLU nn.moment_activations found behind it in
    the epilogue); a tracking pass (forward_moments) raises ops.BnnHipError: there is no moment backward.  The network draw plan
    and nn.fuse_activations select by exact type and pass this layer by.  Out of scope: bf16 activations (K11 takes fp32), the
    multiplicative parametrisation, compacting a pruned model into smaller layers, distributed.forward_sharded's KL sharding."""

    compute = None      # None -> module-wide default (nn.set_compute)
    _op = None
    _nd = 0

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, bias_prior, threshold):
        from .core import WeightVariationalDropout
        # the weight's prior is the log-uniform one; BayesianConvNd would build the bias from the weight's class
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, False, groups, False,
                         WeightVariationalDropout, None, bias_prior)
        if bias:
            del self._parameters['bias']            # (registered as None by the base class, whose reset_parameters set the weight)
            self.bias = WeightNormal(out_channels)
            self._reset_bias()
        self.threshold = threshold
        self._init_noise()                          # (_noise_shape: one sample's INPUT shape (B, C, *spatial))

    def _reset_bias(self):
        fan_in, _ = init._calculate_fan_in_and_fan_out(self.weight.mean)
        bound = 1 / math.sqrt(fan_in)
        init.uniform_(self.bias.mean, -bound, bound)
        init.normal_(self.bias.scale, -2.0, 0.15)

    def reset_parameters(self):
        init.kaiming_uniform_(self.weight.mean, a=math.sqrt(5))
        init.constant_(self.weight.log_sigma2, -10.0)
        if self.bias is not None:
            self._reset_bias()

    def _compute_mode(self):
        return self.compute or _settings.get_compute()

    def _posterior(self):
        b = self.bias is not None
        return (self.weight.mean, self.weight.log_sigma2, self.bias.mean if b else None, self.bias.scale if b else None)

    def _threshold(self):
        return None if self.threshold is None else float(self.threshold)

    def _dropped_mask(self):
        """The weights with log_alpha > threshold (3.0 while threshold is None), a bool tensor of the weight's shape: on the device
        read off bnn_vd_prepare's masked plane (ops.vd_dropped_mask), on the CPU the float64 expression -- one rule, the kernels'."""
        thr = 3.0 if self.threshold is None else float(self.threshold)
        w = self.weight
        with torch.no_grad():
            if w.mean.is_cuda:
                return ops.vd_dropped_mask(w.mean, w.log_sigma2, thr)
            return ops.vd_log_alpha(w.mean.double(), w.log_sigma2.double()) > thr

    def _dropped(self):
        return int(self._dropped_mask().sum().item()), self.weight.mean.numel()

    def sparsity(self):
        """The fraction of weights with log_alpha > threshold (3.0 while threshold is None)."""
        dropped, total = self._dropped()
        return dropped / total

    def filter_sparsity(self):
        """The fraction of output filters all of whose weights have log_alpha > threshold (3.0 while threshold is None)."""
        mask = self._dropped_mask()
        return int(mask.reshape(mask.shape[0], -1).all(dim=1).sum().item()) / mask.shape[0]

    def _forward_moments(self, x):
        mom = x if isinstance(x, ops.Moments) else ops.Moments(x, None)
        if not torch.is_tensor(mom.mean):
            raise TypeError("%s takes a tensor or ops.Moments in a moment pass, got %s" % (type(self).__name__, type(x).__name__))
        ops._refuse_link(mom, type(self).__name__)
        if _mc.moments_current().track:
            raise ops.BnnHipError("%s has no moment backward (inference only)" % type(self).__name__)
        if mom.mean.dim() == self._nd + 1:
            out = self._forward_moments(ops.Moments(mom.mean.unsqueeze(0), None if mom.var is None else mom.var.unsqueeze(0)))
            res = ops.Moments(out.mean.squeeze(0), out.var.squeeze(0))
            res._act = out._act
            return res
        act = self.__dict__.get("_moment_act")
        args = self._posterior() + (self.stride, self.padding, self.dilation, self.groups)
        if not mom.mean.is_cuda:
            out = ops.moments_convNd_vd_f64(mom, *args, activation=act, threshold=self._threshold())
        else:
            out = ops.moments_convNd_vd(mom, *args, activation=act, compute=self._compute_mode(), threshold=self._threshold())
        out._act = act
        return out

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            return self._forward_moments(x)                              # predictive_moments: moments in, moments out, no noise
        conv = type(self)._op
        geo = (self.stride, self.padding, self.dilation, self.groups)
        thr = self._threshold()
        theta, ls2, mu_b, rho_b = self._posterior()
        if not x.is_cuda:
            ops._vd_refuse_masked_grad(type(self).__name__, thr, theta, ls2, mu_b, rho_b)
            s2 = self.weight.variance
            if thr is not None:
                keep = ~(self.weight.log_alpha > thr)
                theta, s2 = theta * keep, s2 * keep
            m = conv(x, theta, mu_b, *geo)
            v = conv(x * x, s2, self.bias.variance if self.bias is not None else None, *geo)
            return self._cpu_sample(m, v, sample)
        if x.dim() == self._nd + 1:
            return self.forward(x.unsqueeze(0), sample).squeeze(0)
        S, s0, shared, per = _lrt_noise_plan(x)
        mode = self._compute_mode()
        xs = x if shared else x.reshape(S, per, *x.shape[1:])
        key = self._call_key(sample, (per,) + tuple(x.shape[1:]), S, s0, mode, _CONV_WORDING)
        y = ops.convNd_vd(xs, theta, ls2, mu_b, rho_b, key, shared, *geo, mode, threshold=thr)
        return y.reshape(S * per, *y.shape[2:])


def _variational_dropout(name, ntuple, op, nd):
    class _VariationalDropout(VariationalDropoutConvNd):
        _op = staticmethod(op)
        _nd = nd

        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                     groups=1, bias=True, bias_prior=Normal(0, .1), threshold=None):
            super().__init__(in_channels, out_channels, ntuple(kernel_size), ntuple(stride), ntuple(padding),
                             ntuple(dilation), groups, bias, bias_prior, threshold)
    _VariationalDropout.__name__ = _VariationalDropout.__qualname__ = name
    _VariationalDropout.__doc__ = "VariationalDropoutConvNd with %d spatial ax%s." % (nd, "is" if nd == 1 else "es")
    return _VariationalDropout


VariationalDropoutConv1d = _variational_dropout('VariationalDropoutConv1d', _single, torch.nn.functional.conv1d, 1)
VariationalDropoutConv2d = _variational_dropout('VariationalDropoutConv2d', _pair, torch.nn.functional.conv2d, 2)
VariationalDropoutConv3d = _variational_dropout('VariationalDropoutConv3d', _triple, torch.nn.functional.conv3d, 3)


def _flipout_conv2d_device(layer, x, R, S, view, stride, padding, dilation):
    """conv.py:207-221 on the device for a 4-d x and sign tensors R (B, O, 1, 1), S (B, C, 1, 1) broadcast over its rows; `view`
    turns the layer's weight tensors into (O, C, KH, KW)."""
    # both contractions are the HIP implicit GEMM (the sign tensors are per EXAMPLE, conv.py:154-161, so they cannot be folded
    # into the weight)
    comp = _settings.get_compute()
    geo = (stride, padding, dilation, layer.groups)
    mean, scale = view(layer.weight.mean), view(layer.weight.scale)
    needs_grad = torch.is_grad_enabled() and (x.requires_grad or layer._trainable())
    if comp == "bf16" and not needs_grad and ops.conv2d_flipout_eligible(x, mean, *geo):
        # one launch for both contractions: shared A tile, S in the fragment's sign bits, R in the epilogue
        return ops.conv2d_flipout(x, mean, scale, R, S, *geo[:3])
    if comp == "f32" and not needs_grad and layer.groups == 1 and ops.conv2d_flipout_x3_fused_eligible(x, mean, *geo[:3]):
        # fp32 parity mode, inference: ONE contraction launch on three-plane operands (S in the sign bits, R in the epilogue)
        return ops.conv2d_flipout_x3_fused(x, mean, view(layer.weight.stddev), R, S, *geo[:3])
    if (comp == "f32" and not needs_grad and mean.data_ptr() % 16 == 0 and
            ops.conv2d_plain_x3_eligible(x, mean.detach().unsqueeze(0), *geo, comp)):
        # fp32 parity mode, inference: both contractions as implicit GEMMs on three-plane operands, no im2col panel
        return ops.conv2d_flipout_x3(x, mean, view(layer.weight.stddev), R, S, *geo[:3])
    out = ops.conv2d_plain(x, mean.unsqueeze(0), None, True, *geo, comp)[0]
    noise = ops.conv2d_plain(x * S.expand_as(x), view(layer.weight.stddev).unsqueeze(0), None, True, *geo, comp)[0]
    return out + noise * R.expand_as(out)


class FlipOutNormalConvNd(NormalConvNd):
    """conv.py:145-161: per-example sign tensors R (B, out, 1..) and S (B, in/groups.., 1..); no bias.

    In a BayesianNetworkModule's MC-batched pass on the device (mc_batched = True) every MC sample gets signs of its own, keyed
    like a posterior draw (layer.flip_key; sign contract in include/bnn_hip.h, conv layout).  2-d (and 1-d, as 2-d at height 1):
    in the bf16 mode at inference ONE keyed launch for all S samples (bnn_conv2d_flipout_forward_mc: the mean contraction of a
    shared input computed once, no sign tensor in memory); otherwise the signs are materialized (bnn_flipout_signs), a shared
    input is fanned out to S * B rows and the launches above run on it.  3-d (groups == 1): one sign launch (bnn_flipout_signs)
    and the Flipout implicit GEMM on the shared B rows or the S * B rows (bnn_conv3d_flipout_forward, HIP backward); the serial
    device path runs the same kernels with one sample on layer.R / layer.S; other group counts keep the torch expression.
    sample=False in such a pass reuses flip_key.  layer.R / layer.S keep the values of the last serial-loop (torch.rand) call."""

    _op = None
    _ones = ()

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation,
                 transposed, groups, prior):
        super().__init__(in_channels, out_channels, _single(kernel_size), stride, padding, dilation,
                         transposed, groups, False, prior)
        self.flip_key = None            # DrawKey of the last MC-batched device signs
        self._flip_stream = None

    def sample(self, batch_size=1, additional_dims=()):
        dev = self.weight.device
        self.R = (torch.rand(batch_size, self.weight.size(0), *additional_dims, device=dev) - .5).sign()
        self.S = (torch.rand(batch_size, self.weight.size(1), *additional_dims, device=dev) - .5).sign()

    @property
    def sampled(self):
        return (self.R, self.S)

    def forward(self, x, sample=True):
        # conv.py:182-196 (1d), 213-227 (2d), 244-258 (3d)
        if _mc.moments_current() is not None:
            # a moment pass (nn.moment_estimator_layers, K22): the moments of the layer's weight posterior N(mu, sigma^2), the
            # distribution KLDivergence regularises -- bit for bit NormalConvNd's pass, no bias.  (The reference's conv sign
            # sampler shares one sign per input channel across the kernel taps, so its own marginal variance is
            # sum_c (sum_tap x sigma)^2 rather than sum x^2 sigma^2: it differs from the posterior's.)
            return _conv_forward_moments(self, x)
        plan = _flipout_plan(self, x)
        if plan is not None:
            return self._forward_mc(x, sample, *plan)
        if sample:
            self.sample(x.size(0), self._ones)
        if x.is_cuda and x.dim() == 4 and type(self)._op is torch.nn.functional.conv2d:
            return _flipout_conv2d_device(self, x, self.R, self.S, lambda t: t, self.stride, self.padding, self.dilation)
        if x.is_cuda and x.dim() == 5 and len(self._ones) == 3:
            y = self._serial3d(x)
            if y is not None:
                return y
        conv = type(self)._op
        out = conv(x, self.weight.mean, self.bias, self.stride, self.padding, self.dilation, self.groups)
        noise = conv(x * self.S.expand_as(x), self.weight.stddev, self.bias, self.stride, self.padding,
                     self.dilation, self.groups)
        out += noise * self.R.expand_as(out)
        return out

    def _forward_mc(self, x, sample, ctx, shared):
        nd = len(self._ones)
        if x.dim() != nd + 2:
            raise RuntimeError("mc_batched: %s needs a batched (N, C, ...) input, got shape %s" % (type(self).__name__, tuple(x.shape)))
        key = _flipout_mc_key(self, ctx, sample)
        S = key.nsamples
        O, C = self.weight.size(0), self.weight.size(1)
        B = x.shape[0] if shared else x.shape[0] // S
        if nd == 1:
            # a 1-d convolution is the 2-d one on images of height 1 (as NormalConv1d): the same launches, the same signs
            geo = ((1,) + tuple(self.stride), (0,) + tuple(self.padding), (1,) + tuple(self.dilation))
            return self._mc2d(x.unsqueeze(2), key, shared, B, lambda t: t.unsqueeze(2), geo).squeeze(2)
        if nd == 2:
            return self._mc2d(x, key, shared, B, lambda t: t, (self.stride, self.padding, self.dilation))
        if ops.conv3d_flipout_eligible((B,) + tuple(x.shape[1:]), self.weight.mean.shape, S, self.stride, self.padding,
                                       self.dilation, self.groups):
            # 3-d: one sign launch, then the Flipout implicit GEMM on the shared B rows or the S * B rows (no fan-out)
            sg = ops.flipout_signs(key, B, O + C, x.device)
            x6 = x if shared else x.reshape(S, B, *x.shape[1:])
            y = ops.conv3d_flipout(x6, self.weight.mean, self.weight.scale, sg, S, shared, self.stride, self.padding,
                                   self.dilation, _settings.get_compute())
            return y.reshape(S * B, *y.shape[2:])
        # 3-d, a shape the HIP entries refuse (groups != 1, index range): the reference expression (conv.py:244-258) on
        # materialized keyed signs and the fanned-out input
        sg = ops.flipout_signs(key, B, O + C, x.device).reshape(S * B, O + C)
        R, Sg = sg[:, :O].reshape(S * B, O, 1, 1, 1), sg[:, O:].reshape(S * B, C, 1, 1, 1)
        xf = x.unsqueeze(0).expand(S, *x.shape).reshape(S * B, *x.shape[1:]) if shared else x
        conv = type(self)._op
        out = conv(xf, self.weight.mean, None, self.stride, self.padding, self.dilation, self.groups)
        noise = conv(xf * Sg, self.weight.stddev, None, self.stride, self.padding, self.dilation, self.groups)
        return out + noise * R

    def _serial3d(self, x):
        """conv.py:244-258 on the device for a 5-d x and the recorded layer.R / layer.S: the Flipout implicit GEMM with ONE sample
        (the B x (O + C) sign copy).  None: the HIP entries refuse the shape, or the recorded signs are not one per example."""
        B, O, C = x.shape[0], self.weight.size(0), self.weight.size(1)
        R, Sg = self.R, self.S
        if (R.numel() != B * O or Sg.numel() != B * C or not R.is_cuda or not Sg.is_cuda or
                not ops.conv3d_flipout_eligible(tuple(x.shape), self.weight.mean.shape, 1, self.stride, self.padding, self.dilation,
                                                self.groups)):
            return None
        sg = torch.cat([R.reshape(B, O), Sg.reshape(B, C)], 1).float()
        y = ops.conv3d_flipout(x, self.weight.mean, self.weight.scale, sg, 1, True, self.stride, self.padding, self.dilation,
                               _settings.get_compute())
        return y[0]

    def _mc2d(self, x, key, shared, B, view, geo):
        S = key.nsamples
        O, C = self.weight.size(0), self.weight.size(1)
        comp = _settings.get_compute()
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or self._trainable())
        if comp == "bf16" and not needs_grad and \
                ops.conv2d_flipout_mc_eligible(x, view(self.weight.mean), *geo, self.groups, S, shared):
            # ONE launch for all S samples, the signs made from the key inside it
            return ops.conv2d_flipout_mc(x, view(self.weight.mean), view(self.weight.scale), key, shared, *geo)
        # materialized keyed signs on the fanned-out input, the launches of the serial device path
        sg = ops.flipout_signs(key, B, O + C, x.device).reshape(S * B, O + C)
        R, Sg = sg[:, :O].reshape(S * B, O, 1, 1), sg[:, O:].reshape(S * B, C, 1, 1)
        xf = x.unsqueeze(0).expand(S, *x.shape).reshape(S * B, *x.shape[1:]) if shared else x
        return _flipout_conv2d_device(self, xf, R, Sg, view, *geo)


def _flipout(ntuple, op, ones):
    class _FlipOut(FlipOutNormalConvNd):
        _op = staticmethod(op)
        _ones = ones

        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                     groups=1, prior=Normal(0, .1)):
            super().__init__(in_channels, out_channels, ntuple(kernel_size), ntuple(stride),
                             ntuple(padding), ntuple(dilation), False, groups, prior)
    return _FlipOut


FlipOutNormalConv1d = _flipout(_single, torch.nn.functional.conv1d, (1,))
FlipOutNormalConv1d.__name__ = FlipOutNormalConv1d.__qualname__ = 'FlipOutNormalConv1d'
FlipOutNormalConv2d = _flipout(_pair, torch.nn.functional.conv2d, (1, 1))
FlipOutNormalConv2d.__name__ = FlipOutNormalConv2d.__qualname__ = 'FlipOutNormalConv2d'
FlipOutNormalConv3d = _flipout(_triple, torch.nn.functional.conv3d, (1, 1, 1))
FlipOutNormalConv3d.__name__ = FlipOutNormalConv3d.__qualname__ = 'FlipOutNormalConv3d'


class MCDropoutConvNd(BayesianModule):
    """conv.py:254-262."""

    def __init__(self, in_channels, out_channels, drop_prob):
        super().__init__(in_channels, out_channels, None)
        self.drop_prob = drop_prob
        self.dropout_key = None         # DrawKey of the last MC-batched device mask (nn.dense._mc_dropout_key)
        self._dropout_stream = None


def _mcdropout(name, conv_cls):
    class _MCDropout(MCDropoutConvNd):
        # conv.py:265-326: a stock ConvNd followed by F.dropout that stays on while `sample`;
        # .weight / .bias alias the inner conv's Parameters.
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                     groups=1, bias=True, drop_prob=0.5):
            super().__init__(in_channels, out_channels, drop_prob)
            self.conv = conv_cls(in_channels, out_channels, kernel_size, stride, padding, dilation,
                                 groups, bias)
            self.weight = self.conv.weight
            self.bias = self.conv.bias

        def forward(self, x, sample=True):
            if _mc.moments_current() is not None:                       # a moment pass (K22): moments in, moments out, no mask
                c = self.conv
                if c.padding_mode != 'zeros' or isinstance(c.padding, str):
                    raise ops.BnnHipError("%s: a moment pass takes zero padding given as numbers, got padding=%r, padding_mode=%r"
                                          % (type(self).__name__, c.padding, c.padding_mode))
                geo = (c.stride, c.padding, c.dilation, c.groups)
                return _mc_dropout_forward_moments(
                    self, x, sample, c,
                    lambda mom, track: ops.moments_conv_affine(mom, c.weight, c.bias, *geo, compute=_settings.get_compute(),
                                                               track=track),
                    lambda mom, track: ops.moments_conv_affine_f64(mom, c.weight, c.bias, *geo, track=track))
            plan = _mc_dropout_plan(self, x, sample)
            if plan is None:
                return torch.nn.functional.dropout(self.conv(x), self.drop_prob, sample, False)
            # MC-batched pass on the device: the conv runs once on the rows it is given (B when the input is shared), then
            # the keyed masks of every sample (bnn_mc_dropout: fan-out to S * B rows, or one mask per sample)
            ctx, shared = plan
            ops.check_drop_prob(self.drop_prob)
            return ops.mc_dropout(self.conv(x), self.drop_prob, _mc_dropout_key(self, ctx), shared)
    _MCDropout.__name__ = _MCDropout.__qualname__ = name
    return _MCDropout


MCDropoutConv1d = _mcdropout('MCDropoutConv1d', torch.nn.Conv1d)
MCDropoutConv2d = _mcdropout('MCDropoutConv2d', torch.nn.Conv2d)
MCDropoutConv3d = _mcdropout('MCDropoutConv3d', torch.nn.Conv3d)
