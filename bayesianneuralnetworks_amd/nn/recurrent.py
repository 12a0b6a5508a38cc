"""Recurrent Bayesian layers.  The reference has none; NormalLSTM follows Fortunato et al. 2017, "Bayesian Recurrent Neural
Networks": a mean-field Gaussian posterior over the whole cell, ONE weight draw per MC sample shared by all T steps of that sample.
"""
import torch
from torch.distributions import Normal

from .. import _mc, ops
from .container import BayesianModule
from .core import WeightNormal
from .dense import _NormalSampling, _init_normal_posterior


def lstm_recurrence(x, w, b, hidden_size):
    """The cell in torch ops, in x's dtype: x (rows, T, I), w (4 H, I + H), b (4 H) or None -> the hidden states (rows, T, H),
    h_0 = c_0 = 0.  The CPU path of NormalLSTM (on layer.sampled)."""
    H = hidden_size
    rows, T = x.shape[0], x.shape[1]
    if w.shape != (4 * H, x.shape[-1] + H):
        raise ValueError("lstm_recurrence: weight %s does not fit an input of %d features and %d hidden units"
                         % (tuple(w.shape), x.shape[-1], H))
    h = x.new_zeros(rows, H)
    c = x.new_zeros(rows, H)
    hs = []
    for t in range(T):
        z = torch.cat((x[:, t], h), dim=1)
        G = z @ w.t()
        if b is not None:
            G = G + b
        i, f, g, o = G.split(H, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
    return torch.stack(hs, dim=1)


class NormalLSTM(_NormalSampling, BayesianModule):
    """A Bayesian LSTM layer (not a reference name).  The posterior is ONE WeightNormal for the whole cell: `weight` (4 H, I + H),
    columns [0, I) acting on x_t and [I, I + H) on h_{t-1}, rows in torch's gate order i, f, g, o, and `bias` (4 H) or None --
    so KLDivergence, .kl_divergence(), traverse, apply_wb, PruneNormal and state_dict (weight.mean, weight.scale, bias.mean,
    bias.scale) see an ordinary Gaussian layer.  Initialisation: NormalLinear's, with fan-in I + H.

        G_t = x_t W_x^T + h_{t-1} W_h^T + b,   (i, f, g, o) = split(G_t)
        c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g),   h_t = sigmoid(o) tanh(c_t),   h_0 = c_0 = 0

    One weight draw per MC sample is shared by all T steps of that sample (the variational-RNN rule).  Input: batch-first
    (rows, T, I), rows = B (the shared input of an MC-batched pass) or S * B (behind another Bayesian layer) -- _mc_plan's
    convention; (T, I) is a batch of one.  Output: (S * B, T, H), or with return_sequences=False the last hidden state (S * B, H),
    so that the layer sits in a Sequential in front of a dense head.

    Device input: ops.lstm_sampled -- the draw (bnn_sample_affine_philox on weight.draw_key / bias.draw_key), the input projection
    of all steps in one bnn_linear_forward, then ONE bnn_lstm_step_forward launch per time step; the backward is HIP as well
    (bnn_lstm_step_backward per step, then the linear layer's entries once over T * rows rows).  fp32 operands and accumulation in
    both compute modes; the layer draws on the mode's eps stream.  sample=False reuses the recorded keys, as NormalLinear does;
    weights assigned through .sampled run the same kernels (ops.lstm_plain), expanded over the samples.  CPU tensors: the
    expression above in torch on layer.sampled.

    Out of scope: a moment pass (raises ops.BnnHipError), a non-zero initial state, batch_first=False, packed sequences,
    projections, stacked / bidirectional cells in one module (stack layers in a Sequential), nn.fuse_activations / fuse_head and
    the draw plan (both select NormalLinear by exact type and pass this layer by)."""

    def __init__(self, input_size, hidden_size, bias=True, prior=Normal(0, .1), return_sequences=True):
        BayesianModule.__init__(self, input_size, hidden_size, prior)
        if input_size < 1 or hidden_size < 1:
            raise ValueError("NormalLSTM: input_size and hidden_size must be at least 1")
        self.input_size, self.hidden_size, self.return_sequences = input_size, hidden_size, bool(return_sequences)
        self.weight = WeightNormal(4 * hidden_size, input_size + hidden_size)
        if bias:
            self.bias = WeightNormal(4 * hidden_size)
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        _init_normal_posterior(self)
        self.sample()

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            raise ops.BnnHipError("%s has no moment pass: propagate samples through a recurrent layer (propagation='samples')"
                                  % type(self).__name__)
        if x.dim() == 2:
            return self.forward(x.unsqueeze(0), sample).squeeze(0)
        if x.dim() != 3 or x.shape[-1] != self.input_size:
            raise ValueError("%s takes a batch-first (rows, T, %d) input, got %s" % (type(self).__name__, self.input_size, tuple(x.shape)))
        H = self.hidden_size
        if not x.is_cuda:
            if sample:
                self.sample()
            w, b = self.sampled
            hs = lstm_recurrence(x, w, b, H)
            return hs if self.return_sequences else hs[:, -1]
        S, _, shared, per = self._mc_plan(x, sample)
        keys = self._keys(S)
        x2 = x.float() if shared else x.float().reshape(S, per, *x.shape[1:])
        has_b = self.bias is not None
        if keys is not None:
            y = ops.lstm_sampled(x2, self.weight.mean, self.weight.scale, self.bias.mean if has_b else None,
                                 self.bias.scale if has_b else None, keys[0], keys[1], shared, self.return_sequences)
        else:
            # weights were set explicitly (user-assigned .sampled): the same kernels on them, expanded over the samples
            w, b = self.sampled
            y = ops.lstm_plain(x2, w.float().unsqueeze(0).expand(S, -1, -1), None if b is None else b.float().unsqueeze(0).expand(S, -1),
                               shared, self.return_sequences)
        return y.reshape(S * per, *y.shape[2:])
