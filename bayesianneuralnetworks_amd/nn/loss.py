"""Losses (pytorch_bayesian/nn/loss.py).

KLDivergence is the hot path (K3): every mean-field Gaussian tensor of the model that lives
on the GPU and has a scalar Normal prior goes through ONE multi-tensor HIP launch
(bnn_kl_forward).  With nn.keyed_mvn_draws() on, a WeightMultivariateNormal on the GPU with an isotropic prior (the default
one) takes the closed form in HIP (bnn_mvn_kl, every such tensor in one call).  Other posteriors (tensor-valued or
non-isotropic priors, CPU tensors) use torch.distributions and are averaged in.
"""
import math
import warnings

import torch
from torch.nn import Module
from torch.distributions import MultivariateNormal, Normal
from torch.distributions.kl import kl_divergence

from .. import ops
from ..utils import apply_wb
from . import _settings
from .core import WeightNormal, WeightMultivariateNormal, WeightVariationalDropout
from .dense import MultivariateNormalLinear


def _scalar_normal(prior):
    if not isinstance(prior, Normal):
        return None
    if prior.loc.numel() != 1 or prior.scale.numel() != 1:
        return None
    return float(prior.loc), float(prior.scale)


def _hip_mvn_prior(param, prior):
    """(m0, sigma0) when the HIP closed form takes this tensor: the switch on, a WeightMultivariateNormal on the device, an
    isotropic MultivariateNormal prior of its event size (checked once per prior object); else None."""
    if not (_settings.keyed_mvn_enabled() and isinstance(param, WeightMultivariateNormal) and param.mean.is_cuda
            and isinstance(prior, MultivariateNormal) and prior.event_shape[-1:] == param.mean.shape[-1:]):
        return None
    try:
        torch.broadcast_shapes(prior.batch_shape, param.mean.shape[:-1])
    except RuntimeError:
        return None
    return ops.mvn_isotropic(prior)


def _vd_kl_mean(param):
    """The mean log-uniform KL of one WeightVariationalDropout (0-d): ops.vd_kl on the device, the torch expression on the CPU."""
    if param.mean.is_cuda:
        return ops.vd_kl([param.mean], [param.log_sigma2])[0]
    return ops.vd_kl_elements(param.mean, param.log_sigma2).mean()


class KLDivergence(Module):
    """loss.py:11-38: mean over all weight/bias tensors of mean(KL(q || prior)), / n_batches.

    A WeightVariationalDropout (the weight of nn.VariationalDropoutLinear and of nn.VariationalDropoutConv1d / 2d / 3d, whatever
    its shape) contributes the mean over its elements of the KL to the log-uniform prior (Molchanov et al. 2017's approximation; the layer's prior argument is not read for it), averaged in like
    every other tensor: the reference's convention -- mean over tensors of per-tensor means, / n_batches -- is kept.  On the
    device all such tensors of a model go through ONE ops.vd_kl call (bnn_vd_kl_forward), each in its place in the list, and the
    Gaussian tensors beside them (the layers' biases) through ONE bnn_kl_forward call."""

    def __init__(self, number_of_batches=1):
        super().__init__()
        self.n_batches = number_of_batches

    @staticmethod
    def _prior_of(module, type):
        prior = module.weight_prior if type == 'w' else module.bias_prior
        return prior

    def compute_kl(self, param, module, type):
        """loss.py:16-28 for one tensor -> its mean KL (0-d tensor)."""
        if isinstance(param, WeightVariationalDropout):
            return _vd_kl_mean(param)
        prior = self._prior_of(module, type)
        sn = _scalar_normal(prior)
        if isinstance(param, WeightNormal) and param.mean.is_cuda and sn is not None:
            out = ops.kl_normal([param.mean], [param.scale], [sn], 1.0)
            return out[1]
        iso = _hip_mvn_prior(param, prior)
        if iso is not None:
            return ops.mvn_kl([param.mean], [param.scale], [iso])[0]
        if isinstance(module, MultivariateNormalLinear):
            prior = MultivariateNormal(prior.mean.to(param.device),
                                       scale_tril=prior.scale_tril.to(param.device))
        return kl_divergence(param.dist, prior).mean()

    def forward(self, model):
        entries = model.traverse(
            lambda m: apply_wb(m, lambda p, module, type: (p, module, type),
                               pass_module=True, pass_type=True))
        if entries is None:
            # loss.py:34-36
            raise ValueError('KLDivergence was not able to find BayasianModules')
        fused, other, mvn, vd = [], [], [], []
        for param, module, type in entries:
            if isinstance(param, WeightVariationalDropout):
                if param.mean.is_cuda:
                    vd.append((len(other), param))
                    other.append(None)
                else:
                    other.append(_vd_kl_mean(param))
                continue
            prior = self._prior_of(module, type)
            sn = _scalar_normal(prior)
            iso = _hip_mvn_prior(param, prior)
            if isinstance(param, WeightNormal) and param.mean.is_cuda and sn is not None:
                fused.append((param, sn))
            elif iso is not None:
                mvn.append((len(other), param, iso))
                other.append(None)
            else:
                other.append(self.compute_kl(param, module, type))
        if mvn:
            # every full-covariance tensor with an isotropic prior in ONE bnn_mvn_kl call, in its place in the list
            kls = ops.mvn_kl([p.mean for _, p, _ in mvn], [p.scale for _, p, _ in mvn], [iso for _, _, iso in mvn])
            for k, (i, _, _) in enumerate(mvn):
                other[i] = kls[k]
        if vd:
            # every variational-dropout tensor in ONE bnn_vd_kl_forward call, in its place in the list
            kls = ops.vd_kl([p.mean for _, p in vd], [p.log_sigma2 for _, p in vd])
            for k, (i, _) in enumerate(vd):
                other[i] = kls[k]
            if fused:
                # the Gaussian tensors beside them (the layers' biases) still take ONE bnn_kl_forward call: at n_batches = 1 its
                # scalar is the mean over those tensors of their per-tensor means, which enters the mean over all tensors with
                # their number as its weight
                fm = ops.kl_normal_scalar([p.mean for p, _ in fused], [p.scale for p, _ in fused], [sn for _, sn in fused], 1.0)
                return (torch.stack(other).sum() + len(fused) * fm) / ((len(other) + len(fused)) * self.n_batches)
        if fused and not other:
            return ops.kl_normal_scalar([p.mean for p, _ in fused], [p.scale for p, _ in fused],
                                        [sn for _, sn in fused], self.n_batches)
        means = list(other)
        if fused:
            # mixed model: per-tensor means from the fused launch's scalar with n_batches = 1
            for p, sn in fused:
                means.append(ops.kl_normal([p.mean], [p.scale], [sn], 1.0)[1])
        return torch.stack(means).mean() / self.n_batches


class Entropy(Module):
    """loss.py:41-51."""

    def __init__(self, dim=0):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        if (x == 0).all():
            warnings.warn('Entropy received a tensor containing all zeros', RuntimeWarning)
        return (-x * torch.log(x + 1e-10)).sum(dim=self.dim).mean()


class GaussianNLL(Module):
    """The heteroscedastic Gaussian likelihood that trains a regression head in 'mean_logvar' layout (D means then D
    log-variances), averaged over the MC samples: forward(ys, target) with ys the stacked (S, B, 2 D) tensor
    (`model.forward_stacked(x)`), the list of S per-sample (B, 2 D) outputs `model(x)` returns, or one (B, 2 D) output; target
    (B, D).  = torch.nn.functional.gaussian_nll_loss(m, target, exp(s)) over the stacked samples, without the constant term.
    On the device the loss and its gradient come out of one HIP pass (ops.gaussian_nll).  Not in the reference (its
    examples/Simple regression trains an evidential head); the companion of BayesianNetworkModule.predictive_regression."""

    def forward(self, ys, target):
        if isinstance(ys, (list, tuple)):
            ys = torch.stack(list(ys))
        return ops.gaussian_nll(ys, target)


class NormalInverseGaussianLoss(Module):
    """loss.py:54-69: evidential-regression NLL + reg_lambda * |y - gamma| (2 upsilon + alpha).  Five CUDA fp32 tensors of one
    shape: ops.nig_loss (one HIP pass; y then carries no gradient); anything else: the torch expression below."""

    def __init__(self, reg_lambda=1e-2):
        super().__init__()
        self.reg_lambda = reg_lambda

    def nll(self, y, gamma, upsilon, alpha, beta):
        omega = 2 * beta * (1 + upsilon)
        return (0.5 * torch.log(math.pi / upsilon)
                - alpha * torch.log(omega)
                + (alpha + 0.5) * torch.log(upsilon * (y - gamma) ** 2 + omega)
                + torch.lgamma(alpha) - torch.lgamma(alpha + 0.5))

    def forward(self, gamma, upsilon, alpha, beta, y):
        ts = (gamma, upsilon, alpha, beta, y)
        if ops.EVIDENTIAL_HIP and ops._is_dev_f32(*ts) and all(t.shape == gamma.shape for t in ts) and gamma.numel() > 0 and \
                not (y.requires_grad and torch.is_grad_enabled()):
            # K13: the loss and the gradients of the inputs that require one in one HIP pass (a y that wants a gradient keeps
            # the torch expression below; only the explicit ops.nig_loss refuses it)
            return ops.nig_loss(gamma, upsilon, alpha, beta, y, self.reg_lambda)
        penalty = torch.mean(torch.abs(y - gamma) * (2 * upsilon + alpha))
        return self.nll(y, gamma, upsilon, alpha, beta).mean() + self.reg_lambda * penalty


class NormalInverseGaussianUncertainty(Module):
    """loss.py:72-79."""

    def forward(self, upsilon, alpha, beta):
        aleatoric = beta / (alpha - 1)
        return (aleatoric, aleatoric / upsilon)
