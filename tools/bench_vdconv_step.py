"""Training-step time of VariationalDropoutConv2d (K24, k_lrt_conv_wsum<ChainLogSigma2> of csrc/bnn_conv3d.hip) against LocalReparamConv2d (K11) on
the GPU box: the LeNet tail at K19's shape -- (1024, 64, 6, 6) -> conv(64, 64, 3, stride 2, padding 1) -> ReLU -> Flatten ->
dense(576, 10) -- S = 8, both compute modes, both nets in ONE process.  The `vd` net is VariationalDropoutConv2d +
VariationalDropoutLinear, the `lrt` net LocalReparamConv2d + LocalReparamLinear.  A step: MC-batched forward, KLDivergence,
cross-entropy, backward, optim.Adam.  Per mode: the HIP launches of one step, five alternating windows of 100 steps (host clock
around a device synchronise), the medians and their ratio, then the four parts of a step timed with device events (medians of 20).
The contractions of the two nets are the same launches on another variance plane; what differs is the operand launch
(bnn_vd_prepare / bnn_lrt_prepare), the weight gradient's reduce epilogue and the KL (bnn_vd_kl_* in float64 / bnn_kl_*).
usage: python tools/bench_vdconv_step.py > profiles/<date>_vdconv_step.txt"""
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bayesianneuralnetworks_amd as bnn                                    # noqa: E402
from bayesianneuralnetworks_amd import _lib, nn, optim                      # noqa: E402

dev = torch.device("cuda:0")
B, S = 1024, 8


def make(conv, dense):
    class Net(nn.BayesianNetworkModule):
        def __init__(self):
            super().__init__(64, 10, samples=S)
            self.layers = torch.nn.Sequential(conv(64, 64, 3, stride=2, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), dense(576, 10))

        def _forward(self, x):
            return self.layers(x)

    torch.manual_seed(0)
    net = Net().to(dev)
    net.mc_batched = True
    return net, optim.Adam(net.parameters(), lr=1e-3)


def step(net, opt, x, t):
    opt.zero_grad(set_to_none=True)
    ys = net.forward_stacked(x, S)
    loss = net.kl_divergence(100) + F.cross_entropy(ys.reshape(S * B, 10), t.repeat(S))
    loss.backward()
    opt.step()
    return loss


def window(net, opt, x, t, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step(net, opt, x, t)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


lib = _lib.load()
x = torch.randn(B, 64, 6, 6, device=dev)
t = torch.randint(0, 10, (B,), device=dev)
for mode in ("f32", "bf16"):
    bnn.set_compute(mode)
    nets = {"vd": make(nn.VariationalDropoutConv2d, nn.VariationalDropoutLinear), "lrt": make(nn.LocalReparamConv2d, nn.LocalReparamLinear)}
    for name, (net, opt) in nets.items():
        for _ in range(10):
            step(net, opt, x, t)
        torch.cuda.synchronize()
        n0 = lib.bnn_launch_count()
        loss = step(net, opt, x, t)
        torch.cuda.synchronize()
        print("%s %s: %d HIP launches per step, loss %.4f" % (mode, name, lib.bnn_launch_count() - n0, loss.item()), flush=True)
    times = {"vd": [], "lrt": []}
    for rep in range(5):
        for name in ("vd", "lrt") if rep % 2 == 0 else ("lrt", "vd"):
            times[name].append(window(*nets[name], x, t, 100))
    for name in times:
        print("%s %s: step ms per window %s" % (mode, name, " ".join("%.4f" % v for v in times[name])), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print("%s: median step vd %.4f ms, lrt %.4f ms, ratio vd / lrt %.3f" % (mode, med["vd"], med["lrt"], med["vd"] / med["lrt"]), flush=True)
    # where a difference comes from: the parts of one step, timed with device events
    for name, (net, opt) in nets.items():
        parts = {}
        ev = lambda: torch.cuda.Event(enable_timing=True)                   # noqa: E731
        for _ in range(20):
            opt.zero_grad(set_to_none=True)
            e = [ev() for _ in range(5)]
            e[0].record(); ys = net.forward_stacked(x, S)
            e[1].record(); kl = net.kl_divergence(100)
            e[2].record(); loss = kl + F.cross_entropy(ys.reshape(S * B, 10), t.repeat(S)); loss.backward()
            e[3].record(); opt.step()
            e[4].record(); torch.cuda.synchronize()
            for i, k in enumerate(("forward", "kl", "loss+backward", "adam")):
                parts.setdefault(k, []).append(e[i].elapsed_time(e[i + 1]))
        print("%s %s parts (median ms): %s" % (mode, name, ", ".join("%s %.4f" % (k, sorted(v)[len(v) // 2]) for k, v in parts.items())), flush=True)
