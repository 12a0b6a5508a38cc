"""MultivariateNormalLinear on the MC-batched device path (GPU box): device-event timing after warm-up, median of repeated windows.
  new:   nn.keyed_mvn_draws() on -- one layer call in an MC context of S samples on a shared input (bnn_mvn_draw for the weight and
         bias of all S samples + one dense launch), forward and forward + backward; the draw launch alone; the closed-form KL
         (bnn_mvn_kl, bnn_mvn_kl_backward), forward and forward + backward.
  old:   what it replaces -- S serial torch-path layer(x) calls on the device (the reference's MC loop), forward and forward +
         backward; torch's KL through KLDivergence.compute_kl with the switch off, forward and forward + backward.
Reports ms and, for the launches that stream the lower triangle of scale, its bytes (weight O K (K + 1) / 2 + bias O (O + 1) / 2
floats) per second as a share of 6.3 TB/s.  One JSON line per measurement.
usage: bench_mvn.py [--shape head|wide|all] [--iters N] [--windows W]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _mc, ops
from bayesianneuralnetworks_amd.nn import KLDivergence, MultivariateNormalLinear, keyed_mvn_draws

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=("head", "wide", "all"), default="all")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()

HBM = 6.3e12
SHAPES = {"head": (10, 128, 256, 8), "wide": (512, 1024, 256, 8)}      # O, K, B, S: the CIFAR10 head, a wide layer
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / args.iters)
    return statistics.median(ts)


def run(name, O, K, B, S):
    torch.manual_seed(0)
    layer = MultivariateNormalLinear(K, O).to(dev)
    x = torch.randn(B, K, device=dev)
    kl = KLDivergence()
    tri = 4.0 * (O * K * (K + 1) / 2 + O * (O + 1) / 2)

    def report(route, what, ms, streams=False):
        rec = {"shape": name, "route": route, "pass": what, "O": O, "K": K, "B": B, "S": S, "ms": round(ms, 4)}
        if streams:
            rec["triangle_GBps"] = round(tri / ms / 1e6, 1)
            rec["hbm_share"] = round(tri / ms / 1e-3 / HBM, 4)
        print(json.dumps(rec), flush=True)

    def new_fwd():
        with torch.no_grad(), _mc.McContext(S, B, 0):
            layer(x)

    def new_bwd():
        with _mc.McContext(S, B, 0):
            y = layer(x)
        y.backward(torch.ones_like(y))

    def new_draw():
        kw, kb = layer.weight.fresh_key(S, 0, 0, 0), layer.bias.fresh_key(S, 0, 0, 0)
        ops._mvn_draw_raw([layer.weight.mean.detach(), layer.bias.mean.detach()],
                          [layer.weight.scale.detach(), layer.bias.scale.detach()], [kw, kb])

    def kl_fwd():
        with torch.no_grad():
            kl(_Wrap(layer))

    def kl_bwd():
        kl(_Wrap(layer)).backward()

    def old_fwd():
        with torch.no_grad():
            for _ in range(S):
                layer(x)

    def old_bwd():
        ys = [layer(x) for _ in range(S)]
        torch.autograd.backward(ys, [torch.ones_like(t) for t in ys])

    keyed_mvn_draws(True)
    for mode in ("f32", "bf16"):
        bnn.set_compute(mode)
        report("keyed MC pass (%s): bnn_mvn_draw + dense" % mode, "forward", timed(new_fwd))
        report("keyed MC pass (%s): bnn_mvn_draw + dense" % mode, "forward+backward", timed(new_bwd))
    bnn.set_compute("f32")
    report("bnn_mvn_draw alone (weight + bias, all S)", "forward", timed(new_draw), True)
    report("bnn_mvn_kl", "forward", timed(kl_fwd), True)
    report("bnn_mvn_kl", "forward+backward", timed(kl_bwd))
    keyed_mvn_draws(False)
    report("S serial torch-path layer(x) calls", "forward", timed(old_fwd))
    report("S serial torch-path layer(x) calls", "forward+backward", timed(old_bwd))
    report("torch kl_divergence via compute_kl", "forward", timed(kl_fwd), True)
    report("torch kl_divergence via compute_kl", "forward+backward", timed(kl_bwd))
    for p in layer.parameters():
        p.grad = None
    del layer
    torch.cuda.empty_cache()


class _Wrap(bnn.nn.BayesianNetworkModule):
    def __init__(self, layer):
        super().__init__(1, 1, 1)
        self.layers = torch.nn.Sequential(layer)


for name in (("head", "wide") if args.shape == "all" else (args.shape,)):
    run(name, *SHAPES[name])
