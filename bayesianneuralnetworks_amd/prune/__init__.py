"""Pruning of Gaussian posteriors (exports of pytorch_bayesian/prune/__init__.py:1-5).

`PruneNormal()(model, fraction)` zeroes the `fraction` of every posterior tensor whose density at 0 is
highest; on the device the score is the HIP kernel bnn_prune_score (see prune.py).
`PruneLogAlpha(threshold)(model)` (not a reference name, not in __all__) drops the weights of every WeightVariationalDropout whose
log_alpha exceeds the threshold: the rule sparse variational dropout was trained for."""
from . import prune as _impl

PruneNormal = _impl.PruneNormal
PruneLogAlpha = _impl.PruneLogAlpha
__all__ = ('PruneNormal',)
