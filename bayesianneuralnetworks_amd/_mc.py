"""Monte-Carlo batching context.

BayesianNetworkModule.forward (pytorch_bayesian/nn/container.py:32-37) runs `_forward`
`samples` times in a Python loop.  When a network opts in (mc_batched=True) the loop is
replaced by ONE pass in which every Bayesian layer launches all S samples in one grid:
rows [s*B, (s+1)*B) of an activation belong to MC sample s.  A Bayesian layer that still
sees the un-replicated batch (B rows) reads it with sample stride 0, so the deterministic
prefix of a network (e.g. the stock Conv2d stack of examples/MNIST/model.py:21-27) runs
once instead of S times.
"""
import threading

_state = threading.local()


class McContext:
    def __init__(self, samples, base_batch, sample0=0):
        self.samples = samples
        self.base_batch = base_batch
        self.sample0 = sample0
        # set by BayesianNetworkModule.predictive_mean: the caller reduces the outputs over the MC axis itself, so a hidden layer
        # may fuse the classifier head behind it and hand on partial logits (ops.HeadPartials) instead of a tensor
        self.lazy_head = False
        # (x, planes): the network input and its three bf16 planes, split by the draw plan's launch (fp32 parity mode)
        self.x_planes = None

    def __enter__(self):
        self.prev = getattr(_state, "ctx", None)
        _state.ctx = self
        return self

    def __exit__(self, *exc):
        _state.ctx = self.prev
        return False


def current():
    return getattr(_state, "ctx", None)


class MomentContext:
    """Set by BayesianNetworkModule.predictive_moments for ONE pass of `_forward`: inside it NormalLinear, LocalReparamLinear,
    NormalConv1d / 2d / 3d and LocalReparamConv1d / 2d / 3d take a tensor (a deterministic input) or an ops.Moments and hand on
    the mean and variance of their output (ops.moments_linear, ops.moments_convNd) instead of samples.  They draw nothing and record no key.  Thread-local, like McContext, and kept apart
    from it: an MC-batched pass and a moment pass do not see each other.  track=True (BayesianNetworkModule.forward_moments):
    the dense layers and nn.MomentReLU keep the autograd graph (ops.moments_linear(track=True)), and so do the conv layers,
    nn.MomentELU and nn.MomentLinear (ops.moments_convNd / moments_elu / moments_affine(track=True)); the default is inference.
    covariance=True (predictive_moments(covariance=True), K21): a dense layer of at most 32 outputs attaches to the Moments it
    returns what the outputs' covariance needs (ops.head_operands); the pass resolves it when that layer turns out to be the head."""

    def __init__(self, track=False, covariance=False):
        self.track = bool(track)
        self.covariance = bool(covariance)
        self.last_dense = None          # (type name, outputs) of the last dense layer a covariance pass went through

    def __enter__(self):
        self.prev = getattr(_state, "moments", None)
        _state.moments = self
        return self

    def __exit__(self, *exc):
        _state.moments = self.prev
        return False


def moments_current():
    return getattr(_state, "moments", None)
