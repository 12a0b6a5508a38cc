"""Training-step and inference time of nn.NormalLSTM (K25, csrc/bnn_lstm.hip) on the GPU box, against the same layer composed
from what the package had before it: the same draw on the same keys, then per time step ONE ops.linear_plain contraction on
[x_t, h_{t-1}] and torch's gate arithmetic (cat, chunk, sigmoid, tanh, products, adds) -- the baseline a user could build, and a
cross-check of the outputs.  The network: NormalLSTM(I, H, return_sequences=False) -> NormalLinear(H, 2 D), mc_batched,
B = 64, T = 64, I = 32, H = 256, D = 4, S = 8, fp32 mode.  A training step: MC-batched forward, KLDivergence, GaussianNLL, backward,
optim.Adam; an inference pass: predictive_regression(outputs='mean_logvar') under no_grad.  Both nets in ONE process: the launches of
one step / pass, five alternating windows of at least 20 steps and half a second each (host clock around a device synchronise),
the medians and their ratio.
usage: python tools/bench_lstm_step.py > profiles/<date>_lstm_step.txt"""
import os
import sys
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bayesianneuralnetworks_amd as bnn                                    # noqa: E402
from bayesianneuralnetworks_amd import _lib, _mc, nn, ops, optim            # noqa: E402

dev = torch.device("cuda:0")
B, T, I, H, D, S = 64, 64, 32, 256, 4, 8


class ComposedLSTM(nn.NormalLSTM):
    """NormalLSTM's forward from the entries of the parent commit: same posterior, same keys, same weights."""

    def forward(self, x, sample=True):
        S_, _, shared, per = self._mc_plan(x, sample)
        kw, kb = self._keys(S_)
        w = ops.sample_affine_philox(self.weight.mean, self.weight.scale, kw)
        b = ops.sample_affine_philox(self.bias.mean, self.bias.scale, kb)
        xs = x.unsqueeze(0).expand(S_, *x.shape) if shared else x.view(S_, per, *x.shape[1:])
        h = c = x.new_zeros(S_, per, self.hidden_size)
        hs = []
        for t in range(x.shape[1]):
            G = ops.linear_plain(torch.cat((xs[:, :, t], h), dim=2), w, b, False, "f32")
            i, f, g, o = G.chunk(4, dim=2)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            hs.append(h)
        y = torch.stack(hs, dim=2) if self.return_sequences else h
        return y.reshape(S_ * per, *y.shape[2:])


class Net(nn.BayesianNetworkModule):
    def __init__(self):
        super().__init__(I, 2 * D, samples=S)
        self.lstm = nn.NormalLSTM(I, H, return_sequences=False)
        self.head = nn.NormalLinear(H, 2 * D)
        self.mc_batched = True

    def _forward(self, x):
        return self.head(self.lstm(x))


class AtenOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def train_step(net, opt, x, target):
    opt.zero_grad(set_to_none=True)
    loss = net.kl_divergence(100) + nn.GaussianNLL()(net.forward_stacked(x, S), target)
    loss.backward()
    opt.step()
    return loss


def infer(net, opt, x, target):
    with torch.no_grad():
        return net.predictive_regression(x, S, outputs='mean_logvar').mean


def window(fn, args, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


bnn.set_compute("f32")
lib = _lib.load()
_lib.ensure_workspace(dev)
torch.manual_seed(0)
x = torch.randn(B, T, I, device=dev)
target = torch.randn(B, D, device=dev)

# cross-check: one layer, one draw, both forwards (sample=False reuses the recorded keys)
layer = nn.NormalLSTM(I, H).to(dev)
with torch.no_grad(), _mc.McContext(S, B):
    y_fused = layer(x)
    layer.__class__ = ComposedLSTM
    y_comp = layer(x, sample=False)
print("cross-check: fused against composed on the same keys, max |diff| %.3e, rms(h) %.3f"
      % (float((y_fused - y_comp).abs().max()), float(y_fused.square().mean().sqrt())), flush=True)

fused = Net().to(dev)
comp = Net().to(dev)
comp.load_state_dict(fused.state_dict())
comp.lstm.__class__ = ComposedLSTM
nets = {"fused": (fused, optim.Adam(fused.parameters(), lr=1e-3)), "composed": (comp, optim.Adam(comp.parameters(), lr=1e-3))}
for what, fn in (("training step", train_step), ("inference pass", infer)):
    for name, (net, opt) in nets.items():
        for _ in range(3):
            fn(net, opt, x, target)
        torch.cuda.synchronize()
        with AtenOps() as seen:
            n0 = lib.bnn_launch_count()
            fn(net, opt, x, target)
            torch.cuda.synchronize()
            print("%s, %s: %d HIP launches of this library, %d aten operators" % (what, name, lib.bnn_launch_count() - n0, seen.n), flush=True)
    # a window lasts at least half a second: 20 steps, or as many as that takes
    count = {name: max(20, int(500.0 / window(fn, (*nets[name], x, target), 5)) + 1) for name in nets}
    print("%s: steps per window %s" % (what, ", ".join("%s %d" % kv for kv in count.items())), flush=True)
    times = {"fused": [], "composed": []}
    for rep in range(5):
        for name in ("fused", "composed") if rep % 2 == 0 else ("composed", "fused"):
            times[name].append(window(fn, (*nets[name], x, target), count[name]))
    for name in times:
        print("%s, %s: ms per window %s" % (what, name, " ".join("%.4f" % v for v in times[name])), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print("%s: median fused %.4f ms, composed %.4f ms, composed / fused %.2f" % (what, med["fused"], med["composed"], med["composed"] / med["fused"]),
          flush=True)
