"""Dense Bayesian layers (pytorch_bayesian/nn/dense.py).

NormalLinear is the hot path.  On a CUDA/HIP input its forward is draw once + dense GEMM: the posterior is drawn for
all S MC samples of the call by bnn_draw_multi (ONE launch for every NormalLinear of a network when a
BayesianNetworkModule's draw plan runs first), then contracted by bnn_dense_forward (bf16 mode: bf16 operands, fp32
accumulate) or bnn_dense_forward_x3 (fp32 parity mode at inference: three bf16 planes per operand).  Training-time fp32
forwards, narrow fp32 layers and A/B runs take the round-1 fused kernel (bnn_linear_forward_sampled: the draw inside the
B-operand loader of the GEMM).  MCDropoutLinear runs on HIP in a network's MC-batched device pass (keyed masks,
bnn_dense_forward_dropout / bnn_mc_dropout) and keeps F.dropout elsewhere.  FlipoutNormalLinear draws mu + sigma R S^T
with keyed signs per MC sample in that pass (bnn_draw_multi kind BNN_DRAW_FLIPOUT).  MultivariateNormalLinear keeps the
reference's torch expression unless nn.keyed_mvn_draws() is on: then in that pass every MC sample gets a keyed draw of its own
(bnn_mvn_draw, then the HIP linear).  Inside BayesianNetworkModule.predictive_moments (a _mc.MomentContext) NormalLinear and
LocalReparamLinear draw nothing: they take and return a mean and a variance per activation (ops.moments_linear, K16), and so does
MultivariateNormalLinear (ops.moments_mvn_linear, K21: the exact moments of its uniform-noise sampler).  The evidential head is outside the HIP scope and runs as PyTorch-ROCm
ops with the reference's semantics so that its examples keep working.
"""
import math

import torch
from torch.nn import init
from torch.distributions import Normal
from torch.distributions.multivariate_normal import MultivariateNormal

from .. import _mc, ops
from .._rng import DrawKey, default_generator, generator_for, new_stream_id
from . import _settings
from .container import BayesianModule
from .core import WeightNormal, WeightMultivariateNormal


class BayesianLinear(BayesianModule):
    """dense.py:9-24: allocates weight (out, in) and bias (out) posteriors of type `weight`."""

    def __init__(self, in_features, out_features, bias, weight, prior, bias_prior=None):
        super().__init__(in_features, out_features, prior, bias_prior)
        self.weight = weight(out_features, in_features)
        if bias:
            self.bias = weight(out_features)
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        pass


def _init_normal_posterior(layer):
    """dense.py:34-42 / conv.py:53-61: kaiming-uniform means, rho ~ N(-2, 0.15)."""
    init.kaiming_uniform_(layer.weight.mean, a=math.sqrt(5))
    init.normal_(layer.weight.scale, -2.0, 0.15)
    if layer.bias is not None:
        fan_in, _ = init._calculate_fan_in_and_fan_out(layer.weight.mean)
        bound = 1 / math.sqrt(fan_in)
        init.uniform_(layer.bias.mean, -bound, bound)
        init.normal_(layer.bias.scale, -2.0, 0.15)


class _NormalSampling:
    """sample()/.sampled shared by NormalLinear and NormalConvNd (dense.py:46-54, conv.py:65-73)."""

    compute = None      # None -> module-wide default (nn.set_compute)
    activation = None   # 'relu': max(., 0) fused into the kernel epilogue (nn.fuse_activations)
    out_dtype = None    # torch.bfloat16: emit a bf16 hidden activation (bf16 compute mode only)

    def sample(self, nsamples=1, sample0=0):
        # weight first, then bias (dense.py:47-51); one epoch for the layer's draw
        epoch = default_generator.next_epoch() if self.weight.mean.is_cuda else None
        gen = generator_for(self._compute_mode())       # the eps stream is part of the key: whoever re-creates the draw reads it there
        self.weight.sample(nsamples, sample0, epoch, gen)
        if self.bias is not None:
            self.bias.sample(nsamples, sample0, epoch, gen)

    def _fresh_keys(self, nsamples, sample0):
        """The DrawKeys sample(nsamples, sample0) would record, without recording them (the network's draw plan draws on
        them ahead of the layer's call; _adopt_keys records them when the layer uses that draw)."""
        from .._rng import DrawKey
        epoch = default_generator.next_epoch()
        gen = generator_for(self._compute_mode())
        kw = DrawKey(default_generator.seed, self.weight._stream, sample0, nsamples, epoch, gen=gen)
        kb = DrawKey(default_generator.seed, self.bias._stream, sample0, nsamples, epoch, gen=gen) if self.bias is not None else None
        return kw, kb

    def _adopt_keys(self, kw, kb):
        self.weight._key, self.weight._explicit = kw, None
        if self.bias is not None:
            self.bias._key, self.bias._explicit = kb, None

    @property
    def sampled(self):
        return (self.weight.sampled, self.bias.sampled if self.bias is not None else None)

    @sampled.setter
    def sampled(self, value):
        w, b = value
        self.weight.sampled = w
        if self.bias is not None and b is not None:
            self.bias.sampled = b

    def _compute_mode(self):
        return self.compute or _settings.get_compute()

    def _trainable(self):
        """Does any posterior tensor of the layer want a gradient?  (The inference-only paths have no autograd node: a frozen mean
        with a trainable scale or bias must not take them.)"""
        ps = [self.weight.mean, self.weight.scale]
        if self.bias is not None:
            ps += [self.bias.mean, self.bias.scale]
        return any(p.requires_grad for p in ps)

    def _forward_moments(self, x):
        """The layer inside a moment pass (_mc.MomentContext; BayesianNetworkModule.predictive_moments): x a tensor (a
        deterministic input) or an ops.Moments -> the ops.Moments of the output, with the moment-matched ReLU when
        nn.fuse_activations folded one into the layer (activation == 'relu').  Device: ops.moments_linear (bnn_moments_forward,
        hidden moments fp32 in both compute modes); CPU: the same recursion in float64 (ops.moments_linear_f64).  Nothing is
        drawn, no draw epoch is consumed, draw_key / noise_key stay as they are; the result is detached unless the context
        tracks (BayesianNetworkModule.forward_moments: training without sampling)."""
        mom = x if isinstance(x, ops.Moments) else ops.Moments(x, None)
        if not torch.is_tensor(mom.mean):
            raise TypeError("%s takes a tensor or ops.Moments in a moment pass, got %s" % (type(self).__name__, type(x).__name__))
        ops._refuse_link(mom, type(self).__name__)
        b = self.bias is not None
        args = (self.weight.mean, self.weight.scale, self.bias.mean if b else None, self.bias.scale if b else None)
        ctx = _mc.moments_current()
        track = ctx.track
        if not mom.mean.is_cuda:
            out = ops.moments_linear_f64(mom, *args, relu=self.activation == 'relu', track=track)
        else:
            out = ops.moments_linear(mom, *args, relu=self.activation == 'relu', compute=self._compute_mode(), track=track)
        if ctx.covariance:
            # a covariance pass (K21): should this layer be the head, its outputs share the input -- the biases are independent
            ctx.last_dense = (type(self).__name__, self.weight.mean.shape[0])
            if self.activation is None and self.weight.mean.shape[0] <= ops.HEAD_COV_MAX_N:
                out._head = ops.head_operands(mom, self.weight.mean)
        return out

    def _mc_plan(self, x, sample):
        """-> (S, sample0, shared_x, rows_per_sample) for the current MC context."""
        ctx = _mc.current()
        if ctx is None or ctx.samples == 1:
            S, s0 = 1, (ctx.sample0 if ctx else 0)
            shared, per = True, x.shape[0]
        else:
            S, s0 = ctx.samples, ctx.sample0
            if x.shape[0] == ctx.base_batch:
                shared, per = True, x.shape[0]
            elif x.shape[0] == ctx.base_batch * S:
                shared, per = False, ctx.base_batch
            else:
                raise RuntimeError("mc_batched: layer input has %d rows, expected %d or %d"
                                   % (x.shape[0], ctx.base_batch, ctx.base_batch * S))
        if sample:
            self.sample(S, s0)
        return S, s0, shared, per

    def _x3_call(self, x, rows):
        """fp32 parity mode on the dense kernel?  Inference only (the backward kernels take the fused path's saved tensors),
        a 2-D fp32 input or an X3Activation, a wide layer."""
        if not ops.DENSE_X3_F32:
            return False
        if torch.is_grad_enabled() and (self._trainable() or (torch.is_tensor(x) and x.requires_grad)):
            return False
        if torch.is_tensor(x) and (x.dim() != 2 or x.dtype != torch.float32):
            return False
        x2 = x if isinstance(x, ops.X3Activation) else x
        return ops.x3_eligible(x2, self.weight.mean, rows)

    def _try_fused_head(self, x2, shared, per, S, mode, predrawn, sample_head):
        """This hidden layer + the classifier head behind it in ONE launch (bnn_dense_forward_head)?  Only when the caller has
        said it will reduce the outputs itself (predictive_mean -> McContext.lazy_head), in the bf16 mode, at inference, with
        both layers' weights drawn by the network's plan for THIS forward -- otherwise None (the plain path runs)."""
        ctx = _mc.current()
        head = self.__dict__.get("_fuse_head")
        if head is None or ctx is None or not ctx.lazy_head or mode != "bf16" or predrawn is None or torch.is_grad_enabled():
            return None
        hd = getattr(head, "_predrawn", None)
        if hd is None or hd[0] is not ctx or self.out_dtype != torch.bfloat16 or head._compute_mode() != "bf16" or head.activation is not None:
            return None
        K = x2.shape[-1]
        if not ops.dense_head_eligible(per, self.weight.mean.shape[0], predrawn, hd[1]) or predrawn.w.dim() != 3:
            return None
        if x2.dtype == torch.bfloat16:
            pitch = ops.rows_pitch(x2, K)
            xb, ldx, xs = (x2, pitch[0], pitch[1]) if pitch is not None else (x2.contiguous(), K, per * K)
        else:
            xb, ldx, xs = x2.contiguous().to(torch.bfloat16), K, per * K
        head._predrawn = None                                   # the head's drawn weights are consumed here ...
        head._adopt_keys(hd[1].key_w, hd[1].key_b)              # ... and this is its sample() for this forward
        hp = ops._dense_head_raw(xb, 0 if shared else xs, per, predrawn, K, self.activation == 'relu', hd[1], ldx=ldx)
        hp.head = head
        return hp

    def _keys(self, S):
        kw = self.weight.draw_key
        kb = self.bias.draw_key if self.bias is not None else None
        if kw is None or (self.bias is not None and kb is None):
            return None
        if kw.nsamples != S:
            if S == 1:
                return kw.last_sample(), (kb.last_sample() if kb is not None else None)
            raise RuntimeError("sample=False: the recorded draw has %d MC samples, this call needs %d"
                               % (kw.nsamples, S))
        return kw, kb


class NormalLinear(_NormalSampling, BayesianLinear):
    """dense.py:27-60."""

    def __init__(self, in_features, out_features, bias=True, prior=Normal(0, .1)):
        super().__init__(in_features, out_features, bias, WeightNormal, prior)

    def reset_parameters(self):
        _init_normal_posterior(self)
        self.sample()                                                   # dense.py:44

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            return self._forward_moments(x)                              # predictive_moments: moments in, moments out, no draw
        if not x.is_cuda:
            # CPU-resident module: the reference's own op sequence (dense.py:56-60)
            if sample:
                self.sample()
            y = torch.nn.functional.linear(x, *self.sampled)
            return torch.relu(y) if self.activation == 'relu' else y
        if isinstance(x, ops.HeadPartials):
            # the hidden layer in front of this head contracted with this layer's drawn weights in its own launch
            # (ops._dense_head_raw): nothing left to do here but pass the partial logits on
            if x.head is not self:
                raise RuntimeError("a fused hidden layer's partial logits reached a layer that is not its head")
            return x
        if x.dim() == 1:
            return self.forward(x.unsqueeze(0), sample).squeeze(0)
        # weights already drawn for this forward by the network's draw plan (container._draw_plan)?  Consumed on use.
        predrawn = None
        pd = getattr(self, "_predrawn", None)
        if pd is not None:
            self._predrawn = None
            if sample and pd[0] is _mc.current():
                predrawn, sample = pd[1], False
                self._adopt_keys(predrawn.key_w, predrawn.key_b)        # this call's sample(): the plan drew on these keys
        S, _, shared, per = self._mc_plan(x, sample)
        keys = self._keys(S)
        mode = self._compute_mode()
        if keys is not None and mode != "bf16" and self._x3_call(x, per):
            # fp32 parity mode, inference: the draw-once dense path on three bf16 planes per operand (ops.linear_sampled_x3);
            # a hidden layer that feeds another dense layer hands its result on in that format (out_x3, nn.fuse_activations)
            K = x.shape[-1]
            ctx = _mc.current()
            xpl = ctx.x_planes if ctx is not None else None
            if xpl is not None and torch.is_tensor(x) and shared and x.data_ptr() == xpl[0].data_ptr() and x.shape == xpl[0].shape:
                x = ops.X3Activation(xpl[1], K)         # the input's planes were split by the draw plan's launch
            x2 = x if isinstance(x, ops.X3Activation) else (x.reshape(-1, K) if shared else x.reshape(S, -1, K))
            pre3 = predrawn if (predrawn is not None and predrawn.w.dim() == 4) else None
            # the classifier head behind this layer in the same launch (predictive_mean, nn.fuse_activations(fuse_head=True))?
            head_pre, head = None, self.__dict__.get("_fuse_head")
            if head is not None and ctx is not None and ctx.lazy_head and pre3 is not None and head.activation is None:
                hd = getattr(head, "_predrawn", None)
                if hd is not None and hd[0] is ctx and head._compute_mode() != "bf16" and \
                        ops.dense_head_x3_eligible(per, self.weight.mean.shape[0], pre3, hd[1]):
                    head._predrawn = None
                    head._adopt_keys(hd[1].key_w, hd[1].key_b)
                    head_pre = hd[1]
            y = ops.linear_sampled_x3(x2, shared, per, self.weight.mean.detach(), self.weight.scale.detach(),
                                      self.bias.mean.detach() if self.bias is not None else None,
                                      self.bias.scale.detach() if self.bias is not None else None,
                                      keys[0], keys[1], relu=self.activation == 'relu',
                                      planes_out=bool(getattr(self, "out_x3", False)),
                                      predrawn=pre3, head_pre=head_pre)
            if isinstance(y, ops.HeadPartials):
                y.head = head
                return y
            if isinstance(y, ops.X3Activation):
                return y
            return y.reshape(S * per, y.shape[-1])
        if isinstance(x, ops.X3Activation):
            x = x.float()
        lead = x.shape[1:-1]
        K = x.shape[-1]
        x2 = x.reshape(-1, K) if shared else x.reshape(S, -1, K)
        if keys is not None:
            odt = torch.bfloat16 if (self.out_dtype == torch.bfloat16 and mode == "bf16") else torch.float32
            hp = self._try_fused_head(x2, shared, per, S, mode, predrawn, sample_head=True)
            if hp is not None:
                return hp
            y = ops.linear_sampled(x2, self.weight.mean, self.weight.scale,
                                   self.bias.mean if self.bias is not None else None,
                                   self.bias.scale if self.bias is not None else None,
                                   keys[0], keys[1], shared, mode, relu=self.activation == 'relu',
                                   out_dtype=odt, predrawn=predrawn if (mode == "bf16" and predrawn is not None and predrawn.w.dim() == 3) else None)
        else:
            # weights were set explicitly (parity mode / user-assigned .sampled)
            w, b = self.sampled
            y = ops.linear_plain(x2.float(), w.unsqueeze(0).expand(S, -1, -1), None if b is None else
                                 b.unsqueeze(0).expand(S, -1), shared, mode)
            if self.activation == 'relu':
                y = torch.relu(y)
        return y.reshape(S * per, *lead, y.shape[-1])


def _lrt_noise_plan(x):
    """-> (S, sample0, shared_x, rows of x per sample) for the current MC context (the row convention of _mc_plan): what the
    local-reparameterization layers (LocalReparamLinear, LocalReparamConvNd) key their noise on."""
    ctx = _mc.current()
    if ctx is None or ctx.samples == 1:
        return 1, (ctx.sample0 if ctx else 0), True, x.shape[0]
    if x.shape[0] == ctx.base_batch:
        return ctx.samples, ctx.sample0, True, x.shape[0]
    if x.shape[0] == ctx.base_batch * ctx.samples:
        return ctx.samples, ctx.sample0, False, ctx.base_batch
    raise RuntimeError("mc_batched: layer input has %d rows, expected %d or %d"
                       % (x.shape[0], ctx.base_batch, ctx.base_batch * ctx.samples))


_DENSE_WORDING = ("a %s", "needs")                          # sample=False on another shape: the dense layers' words, the convs'
_CONV_WORDING = ("an input of %s gave the", "has")


class _LrtNoise:
    """The noise state of a local-reparameterization layer (LocalReparamLinear / ConvNd, VariationalDropoutLinear / ConvNd): the
    layer's own eps stream, the DrawKey of its last device call with what one sample of that call looked like, the eps of its
    last CPU call."""

    def _init_noise(self):
        self._noise_stream = new_stream_id()        # the layer's own eps stream, beside those of its posterior tensors
        self.noise_key = None                       # DrawKey of the last device call
        self._noise_shape = None                    # one sample of that call: dense (rows, out_features), conv the INPUT's shape
        self._cpu_eps = None

    def _call_key(self, sample, shape, S, sample0, mode, wording):
        """-> the DrawKey of a device call of S samples from sample0 on, `shape` per sample: a fresh one, recorded (sample), or the
        recorded one (sample=False; its last sample where a single pass follows an S-sample call).  wording: how the layer words
        a shape that does not match, (the recorded one, the verb of this call's)."""
        if sample:
            self.noise_key = DrawKey(default_generator.seed, self._noise_stream, sample0, S, default_generator.next_epoch(),
                                     gen=generator_for(mode))
            self._noise_shape = shape
        key = self.noise_key
        if key is None or self._noise_shape != shape:
            raise RuntimeError("sample=False: %s noise recorded, this call %s %s per sample"
                               % ("no" if key is None else wording[0] % (self._noise_shape,), wording[1], shape))
        if key.nsamples != S:
            if S != 1:
                raise RuntimeError("sample=False: the recorded noise has %d MC samples, this call needs %d" % (key.nsamples, S))
            key = key.last_sample()
        return key

    def _cpu_sample(self, m, v, sample):
        """m + sqrt(v + 1e-16) eps on CPU tensors: eps drawn here (sample) or the last call's."""
        if sample:
            self._cpu_eps = torch.randn_like(m)
        elif self._cpu_eps is None or self._cpu_eps.shape != m.shape:
            raise RuntimeError("sample=False: no noise of shape %s was drawn by an earlier call" % (tuple(m.shape),))
        return m + torch.sqrt(v + 1e-16) * self._cpu_eps


class LocalReparamLinear(_LrtNoise, _NormalSampling, BayesianLinear):
    """The local-reparameterization estimator of NormalLinear's posterior (Kingma, Salimans, Welling 2015): with independent
    Gaussian w and b the pre-activation is Gaussian per output element, so the layer samples IT instead of the weights:

        m = x mu_w^T + mu_b,   v = x^2 (sigma_w^2)^T + sigma_b^2,   y_s = m + sqrt(v + 1e-16) eps_s,   eps_s ~ N(0, 1)

    with one eps per output element and MC sample (S B N numbers, not S N K), independent across the rows of a batch.
    Parameters, initialisation and state_dict keys are NormalLinear's (weight.mean, weight.scale, bias.mean, bias.scale; sigma =
    1e-10 + softplus(rho)): a checkpoint of one loads into the other, and KLDivergence, .kl_divergence(), traverse, apply_wb and
    PruneNormal see an ordinary Gaussian layer.

    Device input: bnn_lrt_prepare + bnn_lrt_forward (csrc/bnn_lrt.hip), both compute modes.  In a BayesianNetworkModule's
    MC-batched pass all S samples run in ONE contraction launch: a layer that sees the shared batch (B rows) contracts m and v once
    and its S outputs differ in the epilogue only; one that sees S B rows contracts per sample.  Outside such a pass (or with
    S = 1) it is one sample on the same kernels.  layer.noise_key is the DrawKey of the last device call: element b N + n of
    sample s is eps[b N + n] of that key's sample sample0 + s (include/bnn_hip.h, LRT-noise contract), whatever the tile, the
    input layout or the GPU of a sharded run.  sample=False reuses noise_key.  CPU tensors: the expression above in torch with
    torch.randn_like.

    Inside BayesianNetworkModule.predictive_moments the layer is NormalLinear's moment layer (same parameters, same bits) and
    honours activation == 'relu' there.

    Out of scope: nn.fuse_activations / fuse_head and the network draw plan (there is no tensor to pre-draw; both select
    NormalLinear by exact type and pass this layer by), the three-plane (x3) hand-over.  The conv variant is
    nn.LocalReparamConv1d / 2d / 3d (nn/conv.py)."""

    def __init__(self, in_features, out_features, bias=True, prior=Normal(0, .1)):
        super().__init__(in_features, out_features, bias, WeightNormal, prior)
        self._init_noise()

    def reset_parameters(self):
        _init_normal_posterior(self)
        self.sample()

    def _noise_plan(self, x):
        return _lrt_noise_plan(x)

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            return self._forward_moments(x)                              # predictive_moments: moments in, moments out, no noise
        if not x.is_cuda:
            m = torch.nn.functional.linear(x, self.weight.mean, self.bias.mean if self.bias is not None else None)
            v = torch.nn.functional.linear(x * x, self.weight.variance, self.bias.variance if self.bias is not None else None)
            return self._cpu_sample(m, v, sample)
        if x.dim() == 1:
            return self.forward(x.unsqueeze(0), sample).squeeze(0)
        S, s0, shared, per = self._noise_plan(x)
        mode = self._compute_mode()
        lead = x.shape[1:-1]
        K = x.shape[-1]
        N = self.weight.mean.shape[0]
        x2 = x.reshape(-1, K) if shared else x.reshape(S, -1, K)
        key = self._call_key(sample, (x2.shape[-2], N), S, s0, mode, _DENSE_WORDING)
        odt = torch.bfloat16 if (self.out_dtype == torch.bfloat16 and mode == "bf16") else torch.float32
        y = ops.linear_lrt(x2, self.weight.mean, self.weight.scale,
                           self.bias.mean if self.bias is not None else None,
                           self.bias.scale if self.bias is not None else None, key, shared, mode, out_dtype=odt)
        return y.reshape(S * per, *lead, N)


class VariationalDropoutLinear(_LrtNoise, BayesianLinear):
    """Sparse variational dropout (Molchanov, Ashukha, Vetrov 2017; not a reference name): a dense layer that learns which of its
    weights to drop.  Every weight has the posterior N(theta, sigma^2) -- `weight` is a WeightVariationalDropout with Parameters
    mean (theta) and log_sigma2 -- and a log-uniform prior; the pre-activation is sampled by local reparameterization,

        m = x theta^T + mu_b,   v = x^2 exp(log_sigma2)^T + sigma_b^2,   y_s = m + sqrt(v + 1e-16) eps_s,   eps_s ~ N(0, 1)

    and KLDivergence / .kl_divergence() add the log-uniform KL of the weight (ops.vd_kl; no prior argument: the prior is fixed)
    beside the Gaussian KL of the bias against `bias_prior`.  Training drives log_alpha = log_sigma2 - ln(theta^2) up for every
    weight the data does not need; prune.PruneLogAlpha, layer.threshold and layer.sparsity() then need only a threshold on it.
    `bias` is None or a WeightNormal, as LocalReparamLinear's; state_dict keys weight.mean, weight.log_sigma2, bias.mean,
    bias.scale.  Initialisation: the mean as NormalLinear's, log_sigma2 = -10.

    Device input: bnn_vd_prepare + bnn_lrt_forward, both compute modes, bf16 activations in the bf16 mode; the backward is HIP
    (bnn_lrt_backward_epilogue, bnn_lrt_backward_input, bnn_vd_backward_weight).  In a BayesianNetworkModule's MC-batched pass all S
    samples run in ONE contraction launch; noise_key and sample=False mean what they mean on LocalReparamLinear (the LRT-noise
    contract of include/bnn_hip.h).  CPU tensors: the expression above in torch with torch.randn_like.

    threshold (an attribute, default None): with a float every path -- the sampling forward, the MC-batched pass, the moment
    pass -- drops the weights with log_alpha > threshold (theta = 0 and variance 0).  The mask is for inference: a call that would
    need a gradient of a posterior tensor while a threshold is set raises ops.BnnHipError.  sparsity() is the fraction of weights
    with log_alpha > threshold (3.0 while threshold is None).

    Inside BayesianNetworkModule.predictive_moments the layer is NormalLinear's moment layer on the variance plane
    exp(log_sigma2) (bnn_moments_forward) and honours activation == 'relu'; a tracking pass (forward_moments) raises
    ops.BnnHipError: there is no moment backward.  Out of scope: conv variants, nn.fuse_activations / fuse_head and the draw plan
    (both select NormalLinear by exact type), the multiplicative parametrisation, distributed.forward_sharded's KL sharding."""

    compute = None      # None -> module-wide default (nn.set_compute)
    activation = None   # 'relu': honoured in a moment pass
    out_dtype = None    # torch.bfloat16: emit a bf16 hidden activation (bf16 compute mode only)

    def __init__(self, in_features, out_features, bias=True, bias_prior=Normal(0, .1), threshold=None):
        BayesianModule.__init__(self, in_features, out_features, None, bias_prior)     # the weight's prior is the log-uniform one
        from .core import WeightVariationalDropout
        self.weight = WeightVariationalDropout(out_features, in_features)
        if bias:
            self.bias = WeightNormal(out_features)
        else:
            self.register_parameter('bias', None)
        self.threshold = threshold
        self._init_noise()
        self.reset_parameters()

    def reset_parameters(self):
        init.kaiming_uniform_(self.weight.mean, a=math.sqrt(5))
        init.constant_(self.weight.log_sigma2, -10.0)
        if self.bias is not None:
            fan_in, _ = init._calculate_fan_in_and_fan_out(self.weight.mean)
            bound = 1 / math.sqrt(fan_in)
            init.uniform_(self.bias.mean, -bound, bound)
            init.normal_(self.bias.scale, -2.0, 0.15)

    def _compute_mode(self):
        return self.compute or _settings.get_compute()

    def _posterior(self):
        b = self.bias is not None
        return (self.weight.mean, self.weight.log_sigma2, self.bias.mean if b else None, self.bias.scale if b else None)

    def _threshold(self):
        return None if self.threshold is None else float(self.threshold)

    def sparsity(self):
        """The fraction of weights with log_alpha > threshold (3.0 while threshold is None)."""
        dropped, total = self._dropped()
        return dropped / total

    def _dropped(self):
        thr = 3.0 if self.threshold is None else float(self.threshold)
        w = self.weight
        if w.mean.is_cuda:
            dropped = int(ops.vd_dropped(w.mean, w.log_sigma2, thr).item())
        else:
            with torch.no_grad():
                dropped = int((ops.vd_log_alpha(w.mean.double(), w.log_sigma2.double()) > thr).sum().item())   # fp64, as the kernel
        return dropped, w.mean.numel()

    def _forward_moments(self, x):
        mom = x if isinstance(x, ops.Moments) else ops.Moments(x, None)
        if not torch.is_tensor(mom.mean):
            raise TypeError("%s takes a tensor or ops.Moments in a moment pass, got %s" % (type(self).__name__, type(x).__name__))
        ops._refuse_link(mom, type(self).__name__)
        ctx = _mc.moments_current()
        if ctx.track:
            raise ops.BnnHipError("%s has no moment backward (inference only)" % type(self).__name__)
        relu = self.activation == 'relu'
        if not mom.mean.is_cuda:
            out = ops.moments_linear_vd_f64(mom, *self._posterior(), relu=relu, threshold=self._threshold())
        else:
            out = ops.moments_linear_vd(mom, *self._posterior(), relu=relu, compute=self._compute_mode(),
                                        threshold=self._threshold())
        if ctx.covariance:
            ctx.last_dense = (type(self).__name__, self.weight.mean.shape[0])       # (no covariance is carried at this layer)
        return out

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            return self._forward_moments(x)                              # predictive_moments: moments in, moments out, no noise
        thr = self._threshold()
        theta, ls2, mu_b, rho_b = self._posterior()
        if not x.is_cuda:
            ops._vd_refuse_masked_grad(type(self).__name__, thr, theta, ls2, mu_b, rho_b)
            s2 = self.weight.variance
            if thr is not None:
                keep = ~(self.weight.log_alpha > thr)
                theta, s2 = theta * keep, s2 * keep
            m = torch.nn.functional.linear(x, theta, mu_b)
            v = torch.nn.functional.linear(x * x, s2, self.bias.variance if self.bias is not None else None)
            return self._cpu_sample(m, v, sample)
        if x.dim() == 1:
            return self.forward(x.unsqueeze(0), sample).squeeze(0)
        S, s0, shared, per = _lrt_noise_plan(x)
        mode = self._compute_mode()
        lead = x.shape[1:-1]
        K = x.shape[-1]
        N = theta.shape[0]
        x2 = x.reshape(-1, K) if shared else x.reshape(S, -1, K)
        key = self._call_key(sample, (x2.shape[-2], N), S, s0, mode, _DENSE_WORDING)
        odt = torch.bfloat16 if (self.out_dtype == torch.bfloat16 and mode == "bf16") else torch.float32
        y = ops.linear_vd(x2, theta, ls2, mu_b, rho_b, key, shared, mode, out_dtype=odt, threshold=thr)
        return y.reshape(S * per, *lead, N)


def _flipout_plan(layer, x):
    """Inside a BayesianNetworkModule's MC-batched pass (an McContext) on a device tensor: -> (ctx, shared), shared = x holds the
    un-replicated batch (ctx.base_batch rows) rather than S * B rows (sample = row // B).  None: the reference's torch.rand signs
    (serial loop, CPU, no context).  Unlike _mc_dropout_plan this holds for sample=False too: the recorded flip_key is reused."""
    ctx = _mc.current()
    if ctx is None or not isinstance(x, torch.Tensor) or not x.is_cuda:
        return None
    if x.dim() >= 2 and x.shape[0] == ctx.base_batch:
        return ctx, True
    if x.dim() >= 2 and x.shape[0] == ctx.base_batch * ctx.samples:
        return ctx, False
    # torch.rand here would draw ONE set of signs for what the pass treats as S samples
    raise RuntimeError("mc_batched: %s got an input of shape %s; expected (%d, ...) or (%d, ...) rows (batch %d x %d samples)"
                       % (type(layer).__name__, tuple(x.shape), ctx.base_batch, ctx.base_batch * ctx.samples,
                          ctx.base_batch, ctx.samples))


def _flipout_fresh_key(layer, ctx):
    """A fresh DrawKey for the Flipout signs of this MC-batched forward (the RNG contract's sign part), NOT recorded.  The stream id
    is taken at the layer's first MC-batched device forward, so that a model's existing layers keep their ids and draws."""
    from .._rng import DrawKey, new_stream_id
    if getattr(layer, "_flip_stream", None) is None:
        layer._flip_stream = new_stream_id()
    return DrawKey(default_generator.seed, layer._flip_stream, ctx.sample0, ctx.samples, default_generator.next_epoch(),
                   gen=generator_for(_settings.get_compute()))


def _flipout_mc_key(layer, ctx, sample):
    """sample: a fresh key, recorded as layer.flip_key.  sample=False: the recorded key, which must have the pass's S samples."""
    if sample:
        layer.flip_key = _flipout_fresh_key(layer, ctx)
        return layer.flip_key
    key = getattr(layer, "flip_key", None)
    if key is None or key.nsamples != ctx.samples:
        raise RuntimeError("sample=False: %s has %s Flipout signs recorded, this MC-batched pass needs %d samples"
                           % (type(layer).__name__, "no" if key is None else "%d samples of" % key.nsamples, ctx.samples))
    return key


class FlipoutNormalLinear(NormalLinear):
    """dense.py:63-83: y = x mu^T + ((x * S) sigma^T) * R with random sign vectors; no bias.

    In a BayesianNetworkModule's MC-batched pass on the device (mc_batched = True) every MC sample gets signs of its own, keyed
    like a posterior draw (layer.flip_key; sign contract in include/bnn_hip.h): per sample the layer is w_s = mu + sigma (.) R_s
    S_s^T, drawn by bnn_draw_multi (kind BNN_DRAW_FLIPOUT; in the bf16 mode inside the network's one draw launch) and contracted by the dense
    kernel (bf16) or bnn_linear_forward (fp32).  sample=False in such a pass reuses flip_key.  layer.R / layer.S keep the values
    of the last serial-loop (torch.rand) call: the batched pass never materializes them."""

    def __init__(self, in_features, out_features, prior=Normal(0, .1)):
        super().__init__(in_features, out_features, False, prior)
        self.flip_key = None            # DrawKey of the last MC-batched device signs
        self._flip_stream = None

    def sample(self, *unused):
        dev = self.weight.device
        self.R = (torch.rand(self.weight.size(0), device=dev) - .5).sign()
        self.S = (torch.rand(self.weight.size(1), device=dev) - .5).sign()

    @property
    def sampled(self):
        return (self.R, self.S)

    def forward(self, x, sample=True):
        ctx = _mc.moments_current()
        if ctx is not None:
            # a moment pass (nn.moment_estimator_layers, K22): under the layer's own sign sampler an output's marginal mean and
            # variance are NormalLinear's on the same parameters (E[S_k S_k'] = 0 removes the cross terms); no bias.  The
            # covariance between outputs is not NormalLinear's (the signs are shared), so this layer is no covariance head.
            out = self._forward_moments(x)
            if ctx.covariance:
                out._head = None
            return out
        plan = _flipout_plan(self, x)
        if plan is not None:
            return self._forward_mc(x, sample, *plan)
        if sample:
            self.sample()
        if not x.is_cuda:
            perturbation = torch.matmul(x * self.S, self.weight.stddev.t()) * self.R
            # the reference hands the perturbation to F.linear as its bias argument (dense.py:83)
            return torch.nn.functional.linear(x, self.weight.mean, perturbation)
        # device: x mu^T + ((x * S) sigma^T) * R == x (mu + sigma * (R (x) S))^T -- the sampled-weight
        # affine with eps = outer(R, S) (HIP K1, eps supplied) and ONE HIP contraction instead of two;
        # both have HIP backwards, so d/d mean, d/d scale, d/dx come out of the same kernels.
        eps = torch.outer(self.R, self.S)
        w = ops.sample_affine_eps(self.weight.mean, self.weight.scale, eps)
        K = x.shape[-1]
        y = ops.linear_plain(x.reshape(-1, K).float(), w.unsqueeze(0), None, True, self._compute_mode())
        return y.reshape(*x.shape[:-1], y.shape[-1])

    def _forward_mc(self, x, sample, ctx, shared):
        predrawn = None
        pd = getattr(self, "_predrawn", None)
        if pd is not None:
            self._predrawn = None
            if sample and pd[0] is ctx:
                predrawn = pd[1]                    # drawn by the network's plan (container._draw_plan) on this key
                self.flip_key = predrawn.key_w
        key = predrawn.key_w if predrawn is not None else _flipout_mc_key(self, ctx, sample)
        S = key.nsamples
        O, K = self.weight.mean.shape
        x2 = x.reshape(-1, K)
        mode = self._compute_mode()
        if ops.flipout_drawable(self.weight.mean):
            y = ops.linear_flipout_mc(x2, self.weight.mean, self.weight.scale, key, shared, mode,
                                      predrawn if mode == "bf16" else None)
        else:
            # K % 8 != 0: the reference expression on materialized keyed signs, both contractions on the HIP linear
            sg = ops.flipout_signs(key, 1, O + K, x.device)
            R, Sg = sg[:, :, :O], sg[:, :, O:]                                                # (S, 1, O), (S, 1, K)
            xs = x2.float().reshape(1 if shared else S, -1, K)
            out = ops.linear_plain(xs.reshape(-1, K), self.weight.mean.unsqueeze(0), None, True, mode).reshape(xs.shape[0], -1, O)
            noise = ops.linear_plain(xs * Sg, self.weight.stddev.unsqueeze(0).expand(S, O, K), None, False, mode)
            y = out + noise * R
        return y.reshape(-1, *x.shape[1:-1], O)


class MultivariateNormalLinear(BayesianLinear):
    """dense.py:86-138.  PyTorch ops, unless nn.keyed_mvn_draws() is on and the layer runs on the device inside a
    BayesianNetworkModule's MC-batched pass: then every MC sample gets a keyed draw of its own (weight.draw_key, bias.draw_key;
    MVN-noise contract in include/bnn_hip.h), two launches per forward, and sample=False reuses the recorded keys."""

    def __init__(self, in_features, out_features, bias=True, weight_prior=None, bias_prior=None):
        if not weight_prior:
            weight_prior = MultivariateNormal(torch.zeros(out_features, in_features),
                                              torch.eye(in_features).repeat(out_features, 1, 1))
        if bias and not bias_prior:
            bias_prior = MultivariateNormal(torch.zeros(out_features), torch.eye(out_features))
        super().__init__(in_features, out_features, bias, WeightMultivariateNormal,
                         weight_prior, bias_prior)

    @staticmethod
    def _mask_upper(scale):
        with torch.no_grad():
            upper = torch.triu(torch.ones_like(scale), 1).to(torch.bool)
            scale[upper] = -100

    def reset_parameters(self):
        _init_normal_posterior(self)
        self._mask_upper(self.weight.scale)
        if self.bias is not None:
            self._mask_upper(self.bias.scale)
        self.sample()

    def sample(self):
        self.weight.sample()
        if self.bias is not None:
            self.bias.sample()
            self.sampled = (self.weight.sampled, self.bias.sampled)
        else:
            self.sampled = (self.weight.sampled, None)

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:
            return self._forward_moments(x)                              # predictive_moments: moments in, moments out, no draw
        if _settings.keyed_mvn_enabled() and isinstance(x, torch.Tensor) and x.is_cuda and _mc.current() is not None:
            return self._forward_keyed(x, sample, _mc.current())
        if sample:
            self.sample()
        return torch.nn.functional.linear(x, *self.sampled)

    def _posterior(self):
        b = self.bias is not None
        return (self.weight.mean, self.weight.scale, self.bias.mean if b else None, self.bias.scale if b else None)

    def _moments_prepared(self, cpu=False):
        """ops.mvn_moments_prepare's four outputs for the layer's posterior (CPU input: mvn_moments_prepare_f64's), computed again
        only when a parameter has changed (repeated inference batches pay one launch).  "Changed" is what the parameters' autograd
        version counters say ("State that outlives a call")."""
        if not cpu and torch.cuda.is_current_stream_capturing():
            # a captured pass is replayed on whatever the parameters hold THEN, and a replay advances no version: the prepare
            # launch goes into the graph, and the cache keeps what it held for the eager callers
            return ops.mvn_moments_prepare(*self._posterior())
        ps = [p for p in self._posterior() if p is not None]
        tag = (cpu,) + tuple((p.data_ptr(), p._version, tuple(p.shape)) for p in ps)
        cached = self.__dict__.get("_moments_cache")
        if cached is None or cached[0] != tag:
            cached = (tag, (ops.mvn_moments_prepare_f64 if cpu else ops.mvn_moments_prepare)(*self._posterior()))
            self.__dict__["_moments_cache"] = cached
        return cached[1]

    def _forward_moments(self, x):
        """The layer inside a moment pass (K21): x a tensor (a deterministic input) or an ops.Moments -> the ops.Moments of the
        output under the layer's own sampler (uniform noise through the element-wise square root of the triangle) -- exact for
        independent input elements.  Device: ops.moments_mvn_linear (bnn_mvn_moments_forward, the prepare launch cached on the
        layer); CPU: ops.moments_mvn_linear_f64.  Inference only: a tracking pass (forward_moments) raises ops.BnnHipError.  In a
        covariance pass a layer of at most 32 outputs leaves the operands of its outputs' covariance on the result."""
        mom = x if isinstance(x, ops.Moments) else ops.Moments(x, None)
        if not torch.is_tensor(mom.mean):
            raise TypeError("%s takes a tensor or ops.Moments in a moment pass, got %s" % (type(self).__name__, type(x).__name__))
        ops._refuse_link(mom, type(self).__name__)
        ctx = _mc.moments_current()
        if ctx.track:
            raise ops.BnnHipError("%s has no moment backward (inference only)" % type(self).__name__)
        cpu = not mom.mean.is_cuda
        prepared = self._moments_prepared(cpu)
        out = (ops.moments_mvn_linear_f64 if cpu else ops.moments_mvn_linear)(mom, *self._posterior(), prepared=prepared)
        if ctx.covariance:
            ctx.last_dense = (type(self).__name__, self.weight.mean.shape[0])
            if self.weight.mean.shape[0] <= ops.HEAD_COV_MAX_N:
                out._head = ops.head_operands(mom, prepared[0], prepared[3])
        return out

    def _mvn_keys(self, ctx, sample):
        """sample: fresh keys for the pass's S samples, recorded as weight.draw_key / bias.draw_key.  sample=False: the recorded
        keys, which must cover the pass's S samples."""
        if sample:
            epoch = default_generator.next_epoch()
            gen = generator_for(_settings.get_compute())
            self.weight.draw_key = self.weight.fresh_key(ctx.samples, ctx.sample0, epoch, gen)
            if self.bias is not None:
                self.bias.draw_key = self.bias.fresh_key(ctx.samples, ctx.sample0, epoch, gen)
        kw = self.weight.draw_key
        kb = self.bias.draw_key if self.bias is not None else None
        if kw is None or kw.nsamples != ctx.samples or (self.bias is not None and (kb is None or kb.nsamples != ctx.samples)):
            raise RuntimeError("sample=False: %s has %s keyed draws recorded, this MC-batched pass needs %d samples"
                               % (type(self).__name__, "no" if kw is None else "%d samples of" % kw.nsamples, ctx.samples))
        return kw, kb

    def _forward_keyed(self, x, sample, ctx):
        """Every MC sample of the pass on its own keyed draw: ONE bnn_mvn_draw launch for the weight and bias of all S samples,
        ONE dense launch (ops.linear_plain) on the (S, O, K) weights -- shared B-row input or S * B rows.  layer.sampled keeps
        the last torch-path draw."""
        S = ctx.samples
        if x.dim() >= 2 and x.shape[0] == ctx.base_batch:
            shared, per = True, ctx.base_batch
        elif x.dim() >= 2 and x.shape[0] == ctx.base_batch * S:
            shared, per = False, ctx.base_batch
        else:
            raise RuntimeError("mc_batched: %s got an input of shape %s; expected (%d, ...) or (%d, ...) rows (batch %d x %d samples)"
                               % (type(self).__name__, tuple(x.shape), ctx.base_batch, ctx.base_batch * S, ctx.base_batch, S))
        kw, kb = self._mvn_keys(ctx, sample)
        w, b = ops.mvn_draw_layer(self.weight.mean, self.weight.scale,
                                  self.bias.mean if self.bias is not None else None,
                                  self.bias.scale if self.bias is not None else None, kw, kb)
        K = x.shape[-1]
        lead = x.shape[1:-1]
        x2 = x.reshape(-1, K) if shared else x.reshape(S, -1, K)
        y = ops.linear_plain(x2.float(), w, b, shared, _settings.get_compute())
        return y.reshape(S * per, *lead, y.shape[-1])


class NormalInverseGaussianLinear(BayesianModule):
    """dense.py:141-162: evidential head, deterministic Linear(in, 4*out) + softplus splits.  On a CUDA fp32 input the splits,
    softplus and offsets are one HIP launch (ops.nig_head; the Linear stays torch's); CPU and other dtypes: torch ops."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__(in_features, out_features, None)
        self.linear = torch.nn.Linear(in_features, 4 * out_features, bias)

    def forward(self, x, sample=False):
        z = self.linear(x)
        if ops.EVIDENTIAL_HIP and z.is_cuda and z.dtype == torch.float32 and z.numel() > 0:
            # K13: the split, the three softplus and the offsets in one launch (and one backward)
            gamma, upsilon, alpha, beta = ops.nig_head(z, self.out_channels)
        else:
            sp = torch.nn.functional.softplus
            gamma, upsilon, alpha, beta = torch.split(z, self.out_channels, dim=-1)
            upsilon = 1e-10 + sp(upsilon)
            alpha = 1 + 1e-10 + sp(alpha)
            beta = 1e-10 + sp(beta)
        if not sample:
            return (gamma, upsilon, alpha, beta)
        return Normal(gamma.clone(), torch.sqrt(beta / (upsilon * (alpha - 1))))


def _mc_dropout_plan(layer, x, sample):
    """Inside a BayesianNetworkModule's MC-batched pass (an McContext) on a device tensor with `sample`: -> (ctx, shared), shared =
    x holds the un-replicated batch (ctx.base_batch rows: the layer fans out to S * B rows) rather than S * B rows (one mask per
    sample, sample = row // B).  None: the reference's F.dropout path (serial loop, CPU, sample=False)."""
    ctx = _mc.current()
    if not sample or ctx is None or not isinstance(x, torch.Tensor) or not x.is_cuda:
        return None
    if x.dim() >= 2 and x.shape[0] == ctx.base_batch:
        return ctx, True
    if x.dim() >= 2 and x.shape[0] == ctx.base_batch * ctx.samples:
        return ctx, False
    # F.dropout here would draw ONE mask from torch's generator for what the pass treats as S samples
    raise RuntimeError("mc_batched: %s got an input of shape %s; expected (%d, ...) or (%d, ...) rows (batch %d x %d samples)"
                       % (type(layer).__name__, tuple(x.shape), ctx.base_batch, ctx.base_batch * ctx.samples,
                          ctx.base_batch, ctx.samples))


def _mc_dropout_key(layer, ctx):
    """A fresh DrawKey for the masks of this MC-batched forward (the RNG contract's mask part), recorded as layer.dropout_key.
    The stream id is taken at the layer's first MC-batched device forward, so that a model's existing layers keep their ids."""
    from .._rng import DrawKey, new_stream_id
    if getattr(layer, "_dropout_stream", None) is None:
        layer._dropout_stream = new_stream_id()
    key = DrawKey(default_generator.seed, layer._dropout_stream, ctx.sample0, ctx.samples, default_generator.next_epoch(),
                  gen=generator_for(_settings.get_compute()))
    layer.dropout_key = key
    return key


MOMENT_ESTIMATOR_LAYERS = ("MCDropoutLinear", "MCDropoutConv1d", "MCDropoutConv2d", "MCDropoutConv3d", "FlipoutNormalLinear",
                           "FlipOutNormalConv1d", "FlipOutNormalConv2d", "FlipOutNormalConv3d")     # nn.moment_estimator_layers (K22)


def _mc_dropout_forward_moments(layer, x, sample, plain, contract, contract_f64):
    """An MC-dropout layer inside a moment pass (_mc.MomentContext, nn.moment_estimator_layers; K22): x a tensor (a deterministic
    input) or an ops.Moments -> the ops.Moments of the layer's output.  The contraction is deterministic: `contract` on the
    device (ops.moments_affine / moments_conv_affine), `contract_f64` on the CPU, the layer's own `plain` module on a
    deterministic device input.  Then the mask: ONE ops.moments_dropout launch that pushes it through the activation
    nn.moment_activations found behind the layer (layer._moment_act; the twin then passes the result through; none: the
    identity, and an activation twin that meets such moments raises) -- exact for Gaussian pre-activations, where moment-matching the mask in front of a ReLU / ELU is not.  Directly
    in front of an nn.MomentSoftmax (softmax(0) != 0: nothing to fold into) the PRE-dropout moments go on with the mask pending,
    and the softmax hands them to the predictive_* tails with dropout = p.  sample=False applies no dropout, as elsewhere.
    Nothing is drawn and no key is recorded."""
    mom = x if isinstance(x, ops.Moments) else ops.Moments(x, None)
    name = type(layer).__name__
    if not torch.is_tensor(mom.mean):
        raise TypeError("%s takes a tensor or ops.Moments in a moment pass, got %s" % (name, type(x).__name__))
    ops._refuse_link(mom, name)
    ops.check_drop_prob(layer.drop_prob)
    p = float(layer.drop_prob)
    ctx = _mc.moments_current()
    track = ctx.track
    cuda = mom.mean.is_cuda
    if not cuda:
        pre = contract_f64(mom, track)
    elif mom.var is None:
        pre = ops.Moments(plain(mom.mean) if ops._tracking(track) else plain(mom.mean).detach(), None)
    else:
        pre = contract(mom, track)
    if ctx.covariance:
        ctx.last_dense = (name, pre.shape[-1] if pre.dim() else 0)
    if not sample:
        return pre
    act = layer.__dict__.get("_moment_act")
    if act == 'softmax':
        pre._pending = p
        return pre
    out = ops.moments_dropout(pre, p, act, track) if cuda else ops.moments_dropout_f64(pre, p, act, track)
    # what the mask was pushed through: the twin behind passes a matching spec and refuses every other one -- 'identity' among
    # them, so that a hand-placed nn.MomentReLU / MomentELU the layer was never told about cannot moment-match the masked output
    out._act = 'identity' if act is None else act
    return out


class MCDropoutLinear(BayesianModule):
    """dense.py:165-179: dropout stays active while `sample` is true.

    In a BayesianNetworkModule's MC-batched pass on the device (mc_batched = True) every MC sample gets a mask of its own, keyed
    like a posterior draw (layer.dropout_key; mask contract in include/bnn_hip.h): the first such layer sees the un-replicated
    batch, runs its GEMM ONCE and fans out S masked copies; later ones run one GEMM over S * B rows.  bf16 compute mode: one
    bnn_dense_forward_dropout launch (mask in the epilogue); fp32 parity mode and K % 8 != 0: the HIP linear, then bnn_mc_dropout.
    The serial loop, CPU tensors and sample=False keep the reference's F.dropout."""

    def __init__(self, in_features, out_features, bias=True, drop_prob=0.5):
        super().__init__(in_features, out_features, None)
        self.drop_prob = drop_prob
        self.linear = torch.nn.Linear(in_features, out_features, bias)
        self.dropout_key = None
        self._dropout_stream = None
        self._w_bf16 = None

    def _weight_bf16(self):
        """The weight as the dense kernel's bf16 operand, converted again only when the weight has changed -- by its autograd version
        counter ("State that outlives a call")."""
        w = self.linear.weight
        if torch.cuda.is_current_stream_capturing():
            # a replay reads the weight of ITS time and advances no version: the conversion is part of the graph
            return ops.mean_bf16(w.detach())
        tag = (w.data_ptr(), w._version, tuple(w.shape))
        if self._w_bf16 is None or self._w_bf16[0] != tag:
            self._w_bf16 = (tag, ops.mean_bf16(w.detach()))
        return self._w_bf16[1]

    def forward(self, x, sample=True):
        if _mc.moments_current() is not None:                           # a moment pass (K22): moments in, moments out, no mask
            w, b = self.linear.weight, self.linear.bias
            return _mc_dropout_forward_moments(
                self, x, sample, self.linear,
                lambda mom, track: ops.moments_affine(mom, w, b, compute=_settings.get_compute(), track=track),
                lambda mom, track: ops.moments_affine_f64(mom, w, b, track))
        plan = _mc_dropout_plan(self, x, sample)
        if plan is None:
            return torch.nn.functional.dropout(self.linear(x), self.drop_prob, sample, False)
        ctx, shared = plan
        ops.check_drop_prob(self.drop_prob)
        key = _mc_dropout_key(self, ctx)
        compute = _settings.get_compute()
        w, b = self.linear.weight, self.linear.bias
        if x.dim() == 2:
            wb = self._weight_bf16() if ops.linear_mc_dropout_fusable(x, w, compute) else None
            return ops.linear_mc_dropout(x, w, b, self.drop_prob, key, shared, compute, w_bf16=wb)
        # (rows, ..., K): the HIP linear over every position, then the masks over (rows, ... * N)
        K = x.shape[-1]
        x2 = x.reshape(-1, K).float()
        h = ops.linear_plain(x2, w.unsqueeze(0), None if b is None else b.unsqueeze(0), True, compute)
        return ops.mc_dropout(h.view(*x.shape[:-1], w.shape[0]), self.drop_prob, key, shared)
