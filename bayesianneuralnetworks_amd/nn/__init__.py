from .container import BayesianModule, BayesianNetworkModule
from .container import MomentReLU, MomentELU, MomentLinear, MomentSoftmax   # (not in __all__: that list is the reference's)
from .container import (MomentMaxPool1d, MomentMaxPool2d, MomentMaxPool3d, MomentAvgPool1d, MomentAvgPool2d, MomentAvgPool3d,
                        MomentAdaptiveAvgPool1d, MomentAdaptiveAvgPool2d, MomentAdaptiveAvgPool3d,
                        MomentBatchNorm1d, MomentBatchNorm2d, MomentBatchNorm3d)   # (K20; not in __all__ either)
from .core import WeightNormal, WeightMultivariateNormal
from .core import WeightVariationalDropout   # (not in __all__: that list is the reference's)
from .dense import (BayesianLinear, NormalLinear, MultivariateNormalLinear, FlipoutNormalLinear,
                    NormalInverseGaussianLinear, MCDropoutLinear,
                    LocalReparamLinear, VariationalDropoutLinear)   # (not in __all__: that list is the reference's)
from .conv import (BayesianConvNd, NormalConvNd, NormalConv1d, NormalConv2d, NormalConv3d,
                   FlipOutNormalConvNd, FlipOutNormalConv1d, FlipOutNormalConv2d, FlipOutNormalConv3d,
                   MCDropoutConvNd, MCDropoutConv1d, MCDropoutConv2d, MCDropoutConv3d,
                   LocalReparamConvNd, LocalReparamConv1d, LocalReparamConv2d, LocalReparamConv3d,   # (not in __all__ either)
                   VariationalDropoutConvNd, VariationalDropoutConv1d, VariationalDropoutConv2d,
                   VariationalDropoutConv3d)                                                         # (nor these)
from .recurrent import NormalLSTM   # (K25; not in __all__ either)
from .loss import KLDivergence, Entropy, NormalInverseGaussianLoss, NormalInverseGaussianUncertainty
from .loss import GaussianNLL   # (not in __all__ either)
from ._settings import set_compute, get_compute, fuse_activations, fuse_kl_gradient, keyed_mvn_draws, moment_activations
from ._settings import conv_moment_training, conv_moment_training_enabled
from ._settings import moment_estimator_layers, moment_estimator_layers_enabled

# the names pytorch_bayesian/nn/__init__.py:7-35 exports
__all__ = [
    'BayesianModule', 'BayesianNetworkModule', 'WeightNormal', 'WeightMultivariateNormal',
    'BayesianLinear', 'NormalLinear', 'MultivariateNormalLinear', 'FlipoutNormalLinear',
    'NormalInverseGaussianLinear', 'MCDropoutLinear', 'BayesianConvNd', 'NormalConvNd',
    'NormalConv1d', 'NormalConv2d', 'NormalConv3d', 'FlipOutNormalConvNd', 'FlipOutNormalConv1d',
    'FlipOutNormalConv2d', 'FlipOutNormalConv3d', 'MCDropoutConvNd', 'MCDropoutConv1d',
    'MCDropoutConv2d', 'MCDropoutConv3d', 'KLDivergence', 'Entropy', 'NormalInverseGaussianLoss',
    'NormalInverseGaussianUncertainty',
]

# BASELINE.json's north_star uses these two names for the layers above
BayesianConv2d = NormalConv2d
