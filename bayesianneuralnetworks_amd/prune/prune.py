"""Signal-to-noise pruning (pytorch_bayesian/prune/prune.py:5-22).  On the device the score log N(0; mu, sigma) is
a HIP kernel (bnn_prune_score); the top-k selection and the masked assignment are torch ops on the device.
PruneLogAlpha is the threshold rule of sparse variational dropout (nn.VariationalDropoutLinear, nn.VariationalDropoutConv1d / 2d / 3d)."""
import torch

from ..utils import apply_wb


class PruneNormal:

    def __call__(self, module, percentage=0.5):
        self.prune(module, percentage)

    def prune_param(self, param, percentage):
        """prune.py:10-17: the `percentage` entries whose posterior puts the most density on 0
        get mean = 0, scale = -30.  (log_prob is given a tensor: current torch rejects the
        reference's Python-int argument.)"""
        from ..nn.core import WeightVariationalDropout
        if isinstance(param, WeightVariationalDropout):
            raise TypeError("PruneNormal ranks Gaussian posteriors by their density at 0 and writes scale = -30; a "
                            "WeightVariationalDropout has no scale and is pruned by its log_alpha: use prune.PruneLogAlpha")
        if param.mean.is_cuda:
            from .. import ops
            log_prob = ops.prune_score(param.mean, param.scale)
        else:
            zero = torch.zeros((), device=param.mean.device, dtype=param.mean.dtype)
            log_prob = param.dist.log_prob(zero)
        flat = log_prob.flatten()
        k = int(percentage * flat.size(0))
        _, idx = torch.topk(flat, k)
        mask = torch.zeros_like(flat).scatter(0, idx, 1).bool().view(log_prob.shape)
        param.mean[mask] = 0
        param.scale[mask] = -30

    def prune(self, module, percentage=0.5):
        with torch.no_grad():
            module.traverse(lambda m: apply_wb(m, self.prune_param, percentage))


class PruneLogAlpha:
    """Called like PruneNormal: `PruneLogAlpha(threshold)(model)`.  On every WeightVariationalDropout the weights with
    log_alpha > threshold get mean = 0, log_sigma2 = -30 (alpha > e^3 = 20 at the default: the noise outweighs the weight);
    other posteriors are left alone.  A one-off host-side utility like PruneNormal: the mask and the assignment are torch ops."""

    def __init__(self, threshold=3.0):
        self.threshold = float(threshold)

    def __call__(self, module):
        self.prune(module)

    def prune_param(self, param):
        from ..nn.core import WeightVariationalDropout
        if not isinstance(param, WeightVariationalDropout):
            return
        from .. import ops
        # float64, as the kernels evaluate log_alpha (bnn_vd_prepare's mask, layer.sparsity()): one rule everywhere
        mask = ops.vd_log_alpha(param.mean.double(), param.log_sigma2.double()) > self.threshold
        param.mean[mask] = 0
        param.log_sigma2[mask] = -30

    def prune(self, module):
        with torch.no_grad():
            module.traverse(lambda m: apply_wb(m, self.prune_param))
