"""State that outlives a call: a model that has been called, had its parameters changed and is called again, held to a COLD TWIN.

Every other test file holds ONE call to a float64 reference on freshly built operands.  The package keeps state across calls --
the bf16 copy of an MC-dropout weight, the prepare launch of a multivariate-normal head, drawn weights handed from the network's
draw plan to its layers, KL gradients parked for the weight-gradient launches, a KL whose first pass waits for a launch to carry
it -- and a wrong answer that comes from stale state is as wrong as one that comes from a kernel.  The protocol ("State
that outlives a call"):

  1. live = build(); cold = copy.deepcopy(live) BEFORE any forward.  cold runs nothing before step 4.
  2. seed; y0 = P(live): every cache is warm, every lazily created stream id is assigned (and copied to cold, module by module).
  3. live's parameters change by a method M; cold.load_state_dict(live.state_dict()).
  4. seed; y1 = P(live) and seed; yc = P(cold): y1 and yc have the same bits, and y1 differs from y0 (the change was no no-op).

Bit equality is the bound: both runs are the same kernels on the same values and keys at allocator-aligned addresses, and DESIGN.md
states for every family used here that identical calls give identical bits (the one exception it names, the pooling backward's
atomics on overlapping windows, is not run here).  The nets are tiny on purpose: every fault this file looks for is host-side.

Part B replays captured steps (bench.py's TrainStep pattern) against a twin that ran the same steps eagerly, part C holds
optim.Adam to autograd's version counter, part D runs passes that end in a host-side exception and asks that nothing of them
reaches the next pass.
"""
import contextlib
import copy
import itertools

import pytest
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, _rng, nn, ops, optim, prune
from bayesianneuralnetworks_amd._rng import default_generator
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, KLDivergence, NormalLinear
from bayesianneuralnetworks_amd.nn.container import _Single

from alignment import same_bits

pytestmark = pytest.mark.gpu

B, S = 4, 3                     # batch rows, MC samples
SEED = 1234                     # of every compared pass
MODES = ["f32", "bf16"]


# ------------------------------------------------------------------------------------------------ process-wide state
@pytest.fixture
def dev(monkeypatch):
    """The device, with every process-wide switch and counter this file touches put back at the end: compute mode, the KL-fusion,
    keyed-MVN and estimator-layer switches, the eps generator (seed, draw counter, device epoch words), torch's generators.  Stream
    ids come from a counter of the test's own, so that its draws do not depend on which tests ran before it."""
    d = torch.device("cuda:0")
    _lib.ensure_workspace(d)
    from bayesianneuralnetworks_amd.nn import _settings
    saved = (_settings.get_compute(), ops.FUSE_KL_GRADIENT, _settings.keyed_mvn_enabled(), _settings.moment_estimator_layers_enabled())
    torch_seed, cpu_state, cuda_state = torch.initial_seed(), torch.get_rng_state(), torch.cuda.get_rng_state(d)
    gen = (default_generator._seed, default_generator._torch_seed, default_generator.epoch_host)
    cells = [(cell, cell.clone()) for cell in default_generator._epoch_dev.values()]
    monkeypatch.setattr(_rng, "_stream_ids", itertools.count(30001))
    nn.keyed_mvn_draws(True)
    nn.moment_estimator_layers(True)
    yield d
    torch.cuda.synchronize()
    bnn.set_compute(saved[0])
    nn.fuse_kl_gradient(saved[1])
    nn.keyed_mvn_draws(saved[2])
    nn.moment_estimator_layers(saved[3])
    ops._tls.kl_carry = None
    torch.manual_seed(torch_seed)
    torch.set_rng_state(cpu_state)
    torch.cuda.set_rng_state(cuda_state, d)
    default_generator._seed, default_generator._torch_seed, default_generator.epoch_host = gen
    for cell, was in cells:
        cell.copy_(was)


def seed(s=SEED):
    """torch's generators (F.dropout, torch.rand of the serial loop) and the eps stream: draw counter and device epoch word at 0."""
    torch.manual_seed(s)
    bnn.manual_seed(s)


# ------------------------------------------------------------------------------------------------ the nets
class Seq(BayesianNetworkModule):
    def __init__(self, *mods):
        super().__init__(1, 1, samples=S)
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


def _dense(make):
    """The family as the middle of 16 -> 16 -> 16 -> 8 (K % 8 == 0: the bf16 mode takes the fused launches)."""
    return lambda: (Seq(NormalLinear(16, 16), torch.nn.ReLU(), make(), torch.nn.ReLU(), NormalLinear(16, 8)), (B, 16))


def _conv(make, nd):
    """The family as the middle of a conv net: 2 channels on 5-wide extents -> 2 -> 3 channels on 3-wide ones -> 8 outputs."""
    front = (nn.NormalConv1d, nn.NormalConv2d, nn.NormalConv3d)[nd - 1]
    return lambda: (Seq(front(2, 2, 3, padding=1), torch.nn.ReLU(), make(), torch.nn.ReLU(), torch.nn.Flatten(),
                        NormalLinear(3 * 3 ** nd, 8)), (B, 2) + (5,) * nd)


# name -> (builder -> (net, input shape), index of the family's layer in net.layers, has a moment pass)
FAMILIES = {
    "NormalLinear": (_dense(lambda: nn.NormalLinear(16, 16)), 2, True),
    "NormalConv1d": (_conv(lambda: nn.NormalConv1d(2, 3, 3), 1), 2, True),
    "NormalConv2d": (_conv(lambda: nn.NormalConv2d(2, 3, 3), 2), 2, True),
    "NormalConv3d": (_conv(lambda: nn.NormalConv3d(2, 3, 3), 3), 2, True),
    "FlipoutNormalLinear": (_dense(lambda: nn.FlipoutNormalLinear(16, 16)), 2, True),
    "FlipOutNormalConv2d": (_conv(lambda: nn.FlipOutNormalConv2d(2, 3, 3), 2), 2, True),
    "FlipOutNormalConv3d": (_conv(lambda: nn.FlipOutNormalConv3d(2, 3, 3), 3), 2, True),
    "LocalReparamLinear": (_dense(lambda: nn.LocalReparamLinear(16, 16)), 2, True),
    "LocalReparamConv1d": (_conv(lambda: nn.LocalReparamConv1d(2, 3, 3), 1), 2, True),
    "LocalReparamConv2d": (_conv(lambda: nn.LocalReparamConv2d(2, 3, 3), 2), 2, True),
    "LocalReparamConv3d": (_conv(lambda: nn.LocalReparamConv3d(2, 3, 3), 3), 2, True),
    "VariationalDropoutLinear": (_dense(lambda: nn.VariationalDropoutLinear(16, 16)), 2, True),
    "VariationalDropoutConv1d": (_conv(lambda: nn.VariationalDropoutConv1d(2, 3, 3), 1), 2, True),
    "VariationalDropoutConv2d": (_conv(lambda: nn.VariationalDropoutConv2d(2, 3, 3), 2), 2, True),
    "VariationalDropoutConv3d": (_conv(lambda: nn.VariationalDropoutConv3d(2, 3, 3), 3), 2, True),
    "MultivariateNormalLinear": (_dense(lambda: nn.MultivariateNormalLinear(16, 16)), 2, True),
    # the same family as the HEAD (where the CIFAR10 example has it): the only place a covariance pass reads its prepare launch
    "MultivariateNormalLinear-head": (lambda: (Seq(NormalLinear(16, 16), torch.nn.ReLU(), NormalLinear(16, 16), torch.nn.ReLU(),
                                                   nn.MultivariateNormalLinear(16, 8)), (B, 16)), 4, True),
    "MCDropoutLinear": (_dense(lambda: nn.MCDropoutLinear(16, 16, drop_prob=0.25)), 2, True),
    "MCDropoutConv1d": (_conv(lambda: nn.MCDropoutConv1d(2, 3, 3, drop_prob=0.25), 1), 2, True),
    "MCDropoutConv2d": (_conv(lambda: nn.MCDropoutConv2d(2, 3, 3, drop_prob=0.25), 2), 2, True),
    # T = 3, I = 4, H = 8 behind a dense layer that acts on every time step; no moment pass (the layer refuses one)
    "NormalLSTM": (lambda: (Seq(NormalLinear(4, 4), torch.nn.ReLU(), nn.NormalLSTM(4, 8, return_sequences=False), torch.nn.ReLU(),
                                NormalLinear(8, 8)), (B, 3, 4)), 2, False),
}


def build(family, dev):
    """-> (live, cold, x, the family's layer in live).  The posterior comes from a generator seeded per family; cold is the deep copy
    taken before live's first forward."""
    make, at, _ = FAMILIES[family]
    torch.manual_seed(100 + list(FAMILIES).index(family))
    net, shape = make()
    nn.moment_activations(net)                      # (ReLU -> its twin, which is ReLU on tensors: the sampling passes are unchanged)
    live = net.to(dev)
    cold = copy.deepcopy(live)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(dev)
    return live, cold, x, live.layers[at]


def copy_streams(live, cold):
    """Stream ids are handed out at first use for the Flipout signs, the dropout masks, the keyed MVN draws and the model's moment
    draws (_flip_stream, _dropout_stream, _mvn_stream, _moment_stream, _moment_mask_stream): cold takes live's, module by module."""
    for ml, mc in zip(live.modules(), cold.modules()):
        assert type(ml) is type(mc)
        for k, v in ml.__dict__.items():
            if k.endswith("_stream"):
                mc.__dict__[k] = v


# ------------------------------------------------------------------------------------------------ the passes P
def p_serial(net, x):
    net.mc_batched = False
    with torch.no_grad():
        return (torch.stack(net(x)),)


def p_stacked(net, x):
    net.mc_batched = True
    with torch.no_grad():
        return (net.forward_stacked(x, S),)


def p_stacked_train(net, x):
    """The training forward (grad mode on: the paths that save for a backward)."""
    net.mc_batched = True
    return (net.forward_stacked(x, S).detach(),)


def p_mean(net, x):
    net.mc_batched = True
    with torch.no_grad():
        return (net.predictive_mean(x, S),)


def p_moments(net, x):
    """The moment pass: the propagated moments themselves and predictive_mean's draws from them."""
    net.mc_batched = True
    with torch.no_grad():
        mom = net.predictive_moments(x)
        return (mom.mean, mom.var, net.predictive_mean(x, S, propagation='moments'))


def p_cov(net, x):
    net.mc_batched = True
    with torch.no_grad():
        mom = net.predictive_moments(x, covariance=True)
        return (mom.mean, mom.var, mom.cov, net.predictive_mean(x, S, propagation='moments', covariance=True))


PASSES = {"serial": p_serial, "stacked": p_stacked, "stacked_train": p_stacked_train, "mean": p_mean, "moments": p_moments,
          "cov": p_cov}


# ------------------------------------------------------------------------------------------------ the methods M
def _backward(net, x):
    """A real loss.backward() through the MC-batched training forward."""
    net.mc_batched = True
    seed(7)
    ys = net.forward_stacked(x, S)
    gy = torch.randn(ys.shape, generator=torch.Generator().manual_seed(8)).to(ys.device)
    (ys * gy).sum().backward()
    assert all(p.grad is not None for p in net.parameters())


def m_adam(net, x, layer):
    opt = optim.Adam(net.parameters(), lr=1e-2)
    _backward(net, x)
    opt.step()


def m_adam_advance(net, x, layer):
    opt = optim.Adam(net.parameters(), lr=1e-2)
    _backward(net, x)
    opt.step(advance=default_generator.epoch_dev(x.device))


def m_sgd(net, x, layer):
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    _backward(net, x)
    opt.step()


def m_load(net, x, layer):
    net.load_state_dict({k: v * 1.01 if v.is_floating_point() else v for k, v in net.state_dict().items()})


def m_mul(net, x, layer):
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.01)


def m_prune(net, x, layer):
    """PruneNormal on every Gaussian layer, PruneLogAlpha on a variational-dropout one (threshold -6: log_alpha = -10 - ln theta^2
    exceeds it for |theta| < e^-2, a good part of the freshly initialised weights).  KLDivergence's traversal -- PruneNormal's too --
    reads layer.weight, which an MC-dropout layer does not have, and PruneNormal's device score takes no full-covariance scale: those
    two families' own weights get what a prune writes, a masked in-place assignment of zeros to every other element."""
    from bayesianneuralnetworks_amd.nn.core import WeightNormal, WeightVariationalDropout
    with torch.no_grad():
        for m in net.layers:
            w = getattr(m, "weight", None)
            if isinstance(w, WeightVariationalDropout):
                prune.PruneLogAlpha(-6.0)(_Single(m))
            elif isinstance(w, WeightNormal):
                prune.PruneNormal()(_Single(m), 0.5)
        own = [p for n, p in layer.named_parameters() if n in ("linear.weight", "conv.weight")] or \
            ([layer.weight.mean] if isinstance(layer, nn.MultivariateNormalLinear) else [])
        for p in own:
            mask = torch.zeros(p.shape, dtype=torch.bool, device=p.device)
            mask.view(-1)[::2] = True
            p[mask] = 0


def m_cpu_round_trip(net, x, layer):
    net.cpu()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.01)
    net.to(x.device)


METHODS = {"a-adam": m_adam, "b-adam-advance": m_adam_advance, "c-sgd": m_sgd, "d-load_state_dict": m_load, "e-mul_": m_mul,
           "f-prune": m_prune, "g-cpu-round-trip": m_cpu_round_trip}


def supported(family, pname):
    if pname == "cov":
        return family == "MultivariateNormalLinear-head"
    if pname == "moments":
        return FAMILIES[family][2]
    return True


# every M on every family with its MC-batched pass; the other passes with M = (a) and (d)
CASES = [(f, "stacked", m) for f in FAMILIES for m in METHODS] + \
        [(f, p, m) for f in FAMILIES for p in PASSES if p != "stacked" and supported(f, p) for m in ("a-adam", "d-load_state_dict")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family,pname,method", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_cold_twin(dev, family, pname, method, mode):
    bnn.set_compute(mode)
    live, cold, x, layer = build(family, dev)
    P = PASSES[pname]
    seed()
    y0 = P(live, x)
    METHODS[method](live, x, layer)
    copy_streams(live, cold)
    cold.load_state_dict(live.state_dict())
    seed()
    y1 = P(live, x)
    seed()
    yc = P(cold, x)
    torch.cuda.synchronize()
    assert len(y0) == len(y1) == len(yc)
    assert all(bool(torch.isfinite(t).all()) for t in y1)
    stale = [i for i, (a, c) in enumerate(zip(y1, yc)) if not same_bits(a, c)]
    assert not stale, "outputs %s of the called-changed-called net differ from the cold twin's (max |diff| %s)" % (
        stale, [float((y1[i].float() - yc[i].float()).abs().max()) for i in stale])
    assert any(not same_bits(a, b) for a, b in zip(y1, y0)), "the change %s was invisible to this pass: a broken case" % method
    _lib.check_device(dev)


# ------------------------------------------------------------------------------------------------ B: captured steps replayed
def mixed_net(head, dev):
    """NormalLinear(16, 16) - ReLU - head: 'mcd' an MCDropoutLinear(16, 8) (its bf16 weight copy is cached), 'mvn' a
    MultivariateNormalLinear(16, 8) (its prepare launch is cached)."""
    torch.manual_seed(300 + ("mcd", "mvn").index(head))
    h = nn.MCDropoutLinear(16, 8, drop_prob=0.25) if head == "mcd" else nn.MultivariateNormalLinear(16, 8)
    net = Seq(NormalLinear(16, 16), torch.nn.ReLU(), h)
    nn.moment_activations(net)
    live = net.to(dev)
    live.mc_batched = True
    cold = copy.deepcopy(live)
    x = torch.randn(B, 16, generator=torch.Generator().manual_seed(5)).to(dev)
    target = torch.randint(0, 8, (B,), generator=torch.Generator().manual_seed(6)).to(dev).repeat(S)
    return live, cold, x, target


class Trainer:
    """bench.py's TrainStep on a small net: body = forward_stacked, cross-entropy + KL, backward; then optim.Adam.step."""

    def __init__(self, net, x, target, head):
        self.net, self.x, self.target = net, x, target
        # (KLDivergence's traversal reads layer.weight, which an MC-dropout layer does not have: that net's KL is its front layer's)
        self.kl = (lambda: net.layers[0].kl_divergence(100)) if head == "mcd" else (lambda: KLDivergence(100)(net))
        self.opt = optim.Adam(net.parameters(), lr=1e-2)

    def body(self):
        ys = self.net.forward_stacked(self.x, S)
        loss = ops.cross_entropy(ys.reshape(S * B, -1), self.target) + self.kl()
        loss.backward()

    def eager(self, advance=None, cold=False):
        self.opt.zero_grad(set_to_none=True)
        if cold:
            drop_caches(self.net)
        self.body()
        self.opt.step(advance=advance)

    def state(self):
        out = [p.detach() for p in self.net.parameters()]
        for p in self.net.parameters():
            out += [self.opt.state[p]["exp_avg"], self.opt.state[p]["exp_avg_sq"]]
        return out + [g["step"] for g in self.opt.param_groups]


def drop_caches(net):
    """The twin of a replayed step trusts no cache: before each of its eager steps the two version-keyed ones are dropped (the bf16
    copy of an MC-dropout weight, the prepare launch of a multivariate-normal layer), so that it is the reference whatever their
    keys can see."""
    for m in net.modules():
        if "_w_bf16" in m.__dict__:
            m._w_bf16 = None
        m.__dict__.pop("_moments_cache", None)


@contextlib.contextmanager
def side_stream(dev):
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        yield
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()


def warm_adam(dev):
    """optim.Adam's launch once outside a capture, on a tensor of its own."""
    p = torch.nn.Parameter(torch.zeros(8, device=dev))
    p.grad = torch.ones(8, device=dev)
    optim.Adam([p]).step(advance=default_generator.epoch_dev(dev))
    torch.cuda.synchronize()


@pytest.mark.parametrize("warmup", ["i-no-change", "ii-three-steps"])
@pytest.mark.parametrize("head", ["mcd", "mvn"])
def test_captured_training_step_replayed(dev, head, warmup):
    """body + optim.Adam.step(advance=cell) in ONE capture (one linear chain on one stream), replayed 3 times: every parameter and both
    Adam moments equal a cold twin's that ran the same steps eagerly on the same host epochs and device epoch.  Warm-up (i) runs the
    body eagerly and changes no parameter before the capture -- the case a version key cannot see: whatever a cache holds at the
    capture is what its key names; (ii) is bench.py's three eager steps."""
    bnn.set_compute("bf16")
    nn.fuse_kl_gradient(True)
    live, cold, x, target = mixed_net(head, dev)
    cell = default_generator.epoch_dev(dev)
    warm_adam(dev)
    t = Trainer(live, x, target, head)
    seed()
    with side_stream(dev):
        if warmup == "i-no-change":
            t.body()                                # caches warm, kernels loaded, no step: the parameters are the initial ones
        else:
            for _ in range(3):
                t.eager()
    e_cap = default_generator.epoch_host            # the host epochs the capture bakes into its keys
    if warmup == "i-no-change":
        t.opt.ensure_state()                        # moments and step counter exist before the capture, not inside it
    t.opt.zero_grad(set_to_none=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t.body()
        t.opt.step(advance=cell)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    got = [v.clone() for v in t.state()]
    assert int(cell[0]) == 3
    # the cold twin: the same eager steps from the same seed, then the captured step three times eagerly, each on the capture's epochs
    copy_streams(live, cold)
    c = Trainer(cold, x, target, head)
    seed()
    if warmup != "i-no-change":
        for _ in range(3):
            c.eager(cold=True)
    for _ in range(3):
        default_generator.epoch_host = e_cap
        c.eager(advance=cell, cold=True)
    torch.cuda.synchronize()
    want = c.state()
    names = [n for n, _ in live.named_parameters()]
    names = names + [n + "." + k for n in names for k in ("exp_avg", "exp_avg_sq")] + ["step"]
    off = [n for n, a, b in zip(names, got, want) if not torch.equal(a, b)]
    assert not off, "after 3 replays these differ from the eager twin: %s" % off
    assert not ops._tls.kl_pending
    _lib.check_device(dev)


@pytest.mark.parametrize("propagation", ["samples", "moments"])
@pytest.mark.parametrize("head", ["mcd", "mvn"])
def test_captured_inference_replayed_after_training(dev, head, propagation):
    """predictive_mean captured with warm caches, two eager training steps, replay: the trained parameters' predictive_mean, as the
    cold twin computes it eagerly on the capture's host epochs."""
    bnn.set_compute("bf16")
    nn.fuse_kl_gradient(True)
    live, cold, x, target = mixed_net(head, dev)
    t = Trainer(live, x, target, head)
    seed()
    out = torch.empty(B, 8, device=dev)
    with side_stream(dev), torch.no_grad():
        live.predictive_mean(x, S, out=out, propagation=propagation)        # warm: caches filled, stream ids assigned
    e_cap = default_generator.epoch_host
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        live.predictive_mean(x, S, out=out, propagation=propagation)
    e_end = default_generator.epoch_host
    for _ in range(2):
        t.eager()
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = out.clone()
    copy_streams(live, cold)
    cold.load_state_dict(live.state_dict())
    default_generator.epoch_host = e_cap
    with torch.no_grad():
        want = cold.predictive_mean(x, S, propagation=propagation)
    assert default_generator.epoch_host == e_end
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all())
    assert same_bits(got, want.reshape(got.shape)), float((got - want.reshape(got.shape)).abs().max())
    _lib.check_device(dev)


# ------------------------------------------------------------------------------------------------ C: the version counter
def two_layer(dev):
    torch.manual_seed(400)
    net = Seq(NormalLinear(16, 16), torch.nn.ReLU(), NormalLinear(16, 8)).to(dev)
    net.mc_batched = True
    x = torch.randn(B, 16, generator=torch.Generator().manual_seed(5)).to(dev)
    target = torch.randint(0, 8, (B,), generator=torch.Generator().manual_seed(6)).to(dev).repeat(S)
    return net, x, target


def test_adam_step_advances_the_version_of_what_it_wrote(dev):
    net, x, _ = two_layer(dev)
    seed()
    net.forward_stacked(x, S).sum().backward()
    frozen = net.layers[2].bias.scale
    frozen.grad = None                                  # a parameter without a gradient is not stepped
    before = {n: p._version for n, p in net.named_parameters()}
    was = {n: p.detach().clone() for n, p in net.named_parameters()}
    optim.Adam(net.parameters(), lr=1e-2).step()
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        if p is frozen:
            assert p._version == before[n] and torch.equal(p, was[n]), n
        else:
            assert p._version > before[n] and not torch.equal(p, was[n]), n


@pytest.mark.parametrize("which", ["torch.optim.Adam", "bnn.optim.Adam"])
def test_backward_through_a_graph_retained_across_a_step_raises(dev, which):
    """loss.backward(retain_graph=True); step(); loss.backward(): the graph saved the parameters the step has overwritten, and
    autograd says so -- for optim.Adam exactly as for torch.optim.Adam."""
    nn.fuse_kl_gradient(False)
    net, x, target = two_layer(dev)
    opt = (torch.optim.Adam if which == "torch.optim.Adam" else optim.Adam)(net.parameters(), lr=1e-2)
    seed()
    ys = net.forward_stacked(x, S)
    loss = ops.cross_entropy(ys.reshape(S * B, -1), target) + KLDivergence(10)(net)
    loss.backward(retain_graph=True)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ D: passes that end in an exception
def _step(net, x, target):
    net.zero_grad(set_to_none=True)
    seed()
    ys = net.forward_stacked(x, S)
    loss = ops.cross_entropy(ys.reshape(S * B, -1), target) + KLDivergence(10)(net)
    return ys, loss


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fuse", [True, False], ids=["fused-kl", "plain-kl"])
def test_failed_backward_leaves_nothing_behind(dev, fuse, mode):
    """A tensor hook on the logits raises in the middle of loss.backward() -- after KLDivergence's node has run (and, with
    nn.fuse_kl_gradient, parked its gradients: autograd runs no queued callback of a pass that raised).  The next, clean step's
    gradients are the cold twin's, which only ran the clean step."""
    bnn.set_compute(mode)
    nn.fuse_kl_gradient(fuse)
    live, x, target = two_layer(dev)
    cold = copy.deepcopy(live)
    ys, loss = _step(live, x, target)

    def boom(g):
        raise RuntimeError("the hook's own failure")

    ys.register_hook(boom)
    with pytest.raises(RuntimeError, match="the hook's own failure"):
        loss.backward()
    torch.cuda.synchronize()
    for net in (live, cold):
        _, loss = _step(net, x, target)
        loss.backward()
    torch.cuda.synchronize()
    assert not ops._tls.kl_pending, "a parked KL gradient was left behind"
    for (n, p), q in zip(live.named_parameters(), cold.parameters()):
        assert p.grad is not None and same_bits(p.grad, q.grad), (n, float((p.grad - q.grad).abs().max()))
    _lib.check_device(dev)


def test_the_calling_thread_sees_the_parked_entries(dev):
    """`assert not ops._tls.kl_pending` after a backward (tests/test_train_step.py, tests/test_operand_alignment.py, above) only says
    something if the caller's `ops._tls.kl_pending` is the dict the backward parks in -- and a device's autograd nodes run on the
    engine's thread for that device, not on the caller's.  A hook on the logits runs on that thread after KLDivergence's node has
    parked: it sees entries, in the very dict the calling thread reads."""
    nn.fuse_kl_gradient(True)
    net, x, target = two_layer(dev)
    ys, loss = _step(net, x, target)
    seen = []
    ys.register_hook(lambda g: seen.append((ops._tls.kl_pending, len(ops._tls.kl_pending))))
    loss.backward()
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][1] == 4, seen                 # two layers, weight and bias each
    assert seen[0][0] is ops._tls.kl_pending, "the backward parks in a dict that the calling thread cannot see"
    assert not ops._tls.kl_pending


def _begin_kl(net):
    ls = [m for m in net.layers if isinstance(m, NormalLinear)]
    mus = [t for m in ls for t in (m.weight.mean, m.bias.mean)]
    rhos = [t for m in ls for t in (m.weight.scale, m.bias.scale)]
    return ops.kl_normal_begin(mus, rhos, [(0.0, 0.1)] * len(mus), 10.0, carry=True)


def test_failed_forward_leaves_nothing_behind(dev):
    """bf16 mode: the network's draw plan draws every layer's weights before _forward runs and carries the first pass of a KL begun
    with carry=True.  The second layer raises on the host (a wrong feature count, refused before any launch).  Afterwards no KL
    waits to be carried, no layer holds drawn weights of the dead pass, and the next forward and KL are the cold twin's."""
    bnn.set_compute("bf16")
    live, x, _ = two_layer(dev)
    cold = copy.deepcopy(live)
    good = live.layers[2]
    bad = NormalLinear(24, 8).to(dev)
    live.layers[2] = bad
    with torch.no_grad():
        seed()
        h = _begin_kl(cold)                                 # (any four posteriors: this KL is never finished)
        with pytest.raises(ops.BnnHipError, match="input has 16 features, weight expects 24"):
            live.predictive_mean(x, S, kl=h)
        live.layers[2] = good
        assert ops._tls.kl_carry is None
        assert all(getattr(m, "_predrawn", None) is None for m in list(live.modules()) + [bad])
        res = []
        for net in (live, cold):
            seed()
            h = _begin_kl(net)
            y = net.predictive_mean(x, S, kl=h)
            assert ops._tls.kl_carry is None
            res.append((y, h.out))
    torch.cuda.synchronize()
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
    assert bool(torch.isfinite(res[0][1]).all()) and float(res[0][1][-1]) > 0
    _lib.check_device(dev)
