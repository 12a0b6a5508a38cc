"""Sampling-free inference through a conv tail (K17, csrc/bnn_conv3d.hip k_moments_conv3d) against the sampler it replaces, on the
GPU box.  The network is the MNIST example's Bayesian tail: input (B, 64, 6, 6) -> NormalConv2d(64, 64, 3, stride 2, padding 1)
-> ELU -> flatten -> NormalLinear(576, 10) -> softmax, B = 1024; device-event timing after warm-up, median of repeated windows.
  moments: predictive_uncertainty(inputs='probs', propagation='moments') after nn.moment_activations -- per Bayesian layer the
           operand launch + ONE contraction launch (the ELU in the conv launch's epilogue), one sampling launch, the softmax,
           the tail;
  samples: the same call on the MC-batched weight-sampling path (the route of the commit before K17): S stochastic forwards;
  layers:  every launch of the moment pass on its own -- bnn_lrt_prepare, bnn_conv3d_moments_forward without activation, with
           the fused ELU, with a Moments input (algorithmic TFLOP/s: 4 B P O K deterministic, 6 B P O K with a variance), the
           standalone bnn_moments_elu on the B O P pre-activations (the fp64 evaluation's cost), the dense head;
  variance: how far the moment route's logit variance is from 2048 device weight draws (16 rows): worst and median ratio --
           the correlation between the positions of an output map, which the pass drops.  Reported, not asserted.
Every (what, mode) runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per
measurement.
usage: bench_moments_conv.py [--batch 1024] [--samples 8,32,100] [--iters N] [--windows W]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--samples", default="8,32,100")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--what", choices=["moments", "samples", "layers", "variance"])
ap.add_argument("--mode", choices=["bf16", "f32"])
ap.add_argument("--step-timeout", type=int, default=150)
args = ap.parse_args()

if args.what is None:
    for what in ("moments", "samples", "layers", "variance"):
        for mode in ("bf16", "f32"):
            cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--mode", mode, "--batch", str(args.batch),
                   "--samples", args.samples, "--iters", str(args.iters), "--windows", str(args.windows)]
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            if rc != 0:
                sys.exit("bench_moments_conv: %s / %s ended with status %d; nothing more is started" % (what, mode, rc))
    sys.exit(0)

import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, NormalConv2d, NormalLinear

assert args.windows >= 5
dev = torch.device("cuda:0")
B = args.batch
SAMPLES = [int(s) for s in args.samples.split(",")]


class Flatten(torch.nn.Module):
    def forward(self, x):
        return x.view(x.size(0), -1)


class Tail(BayesianNetworkModule):
    def __init__(self, softmax=True):
        super().__init__(64, 10, samples=SAMPLES[0])
        mods = [NormalConv2d(64, 64, 3, padding=1, stride=2), torch.nn.ELU(), Flatten(), NormalLinear(576, 10)]
        self.layers = torch.nn.Sequential(*mods, *([torch.nn.Softmax(dim=-1)] if softmax else []))

    def _forward(self, x):
        return self.layers(x)


def timed(fn):
    for _ in range(3):
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
    return statistics.median(ts), min(ts), max(ts)


def report(row, t=None):
    row.update({"mode": args.mode, "B": B})
    if t is not None:
        row.update({"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)})
    print(json.dumps(row), flush=True)


torch.manual_seed(0)
bnn.set_compute(args.mode)
net = Tail().to(dev)
x = torch.randn(B, 64, 6, 6, device=dev)

if args.what == "moments":
    bnn.nn.moment_activations(net)
    for S in SAMPLES:
        report({"what": "predictive_uncertainty(inputs='probs', propagation='moments')", "S": S},
               timed(lambda: net.predictive_uncertainty(x, S, inputs="probs", propagation="moments")))
    report({"what": "predictive_moments", "S": 0}, timed(lambda: net.predictive_moments(x)))
elif args.what == "samples":
    net.mc_batched = True
    with torch.no_grad():
        for S in SAMPLES:
            report({"what": "predictive_uncertainty(inputs='probs') (MC-batched samples)", "S": S},
                   timed(lambda: net.predictive_uncertainty(x, S, inputs="probs")))
elif args.what == "layers":
    conv, lin = net.layers[0], net.layers[3]
    cp = [t.detach() for t in (conv.weight.mean, conv.weight.scale, conv.bias.mean, conv.bias.scale)]
    lp = [t.detach() for t in (lin.weight.mean, lin.weight.scale, lin.bias.mean, lin.bias.scale)]
    geo = (conv.stride, conv.padding, conv.dilation, conv.groups)
    lib = _lib.load()
    code = ops._compute_code(args.mode)
    st = _lib.stream_ptr(dev)
    P = _lib.ptr
    report({"what": "bnn_lrt_prepare (conv)"}, timed(lambda: ops._lrt_prepare_raw(cp[1], cp[3])))
    s2_w, s2_b = ops._lrt_prepare_raw(cp[1], cp[3])
    sh, _ = ops._conv3d_shape((B, 64, 1, 6, 6), (64, 64, 1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 1), 1)
    import ctypes
    om, ov = torch.empty(B, 64, 3, 3, device=dev), torch.empty(B, 64, 3, 3, device=dev)
    xv = torch.rand_like(x)
    work = B * 9 * 64 * 576
    for name, a_v, flags, mult in (("deterministic", None, 0, 4.0), ("deterministic + ELU", None, _lib.FLAG_ELU, 4.0),
                                   ("deterministic + ReLU", None, _lib.FLAG_RELU, 4.0), ("moments", xv, 0, 6.0),
                                   ("moments + ELU", xv, _lib.FLAG_ELU, 6.0)):
        def launch():
            _lib.check(lib.bnn_conv3d_moments_forward(P(x), P(a_v), P(cp[0]), P(s2_w), P(cp[2]), P(s2_b), P(om), P(ov),
                                                      ctypes.byref(sh), code, flags, 1.0, st), "bnn_conv3d_moments_forward")
        t = timed(launch)
        report({"what": "bnn_conv3d_moments_forward", "input": name, "tflops": round(mult * work / t[0] / 1e9, 2)}, t)
    pre = ops.moments_convNd(x, *cp, *geo, compute=args.mode)
    report({"what": "bnn_moments_elu", "n": pre.mean.numel()}, timed(lambda: ops.moments_elu(pre, 1.0)))
    report({"what": "bnn_moments_relu", "n": pre.mean.numel()}, timed(lambda: ops.moments_relu(pre)))
    act = ops.moments_elu(pre, 1.0).flatten(1)
    report({"what": "moments_linear 576 -> 10 (operand launch + bnn_moments_forward)"},
           timed(lambda: ops.moments_linear(act, *lp, compute=args.mode)))
else:
    S, rows = 2048, 16
    with torch.no_grad():
        for p in (net.layers[0].weight.scale, net.layers[3].weight.scale):
            p.add_(1.0)                                       # sigma ~ 0.13: a variance worth comparing
    logits = Tail(softmax=False).to(dev)
    logits.load_state_dict(net.state_dict())
    logits.mc_batched = True
    bnn.nn.moment_activations(net)
    xs = x[:rows]
    bnn.manual_seed(7)
    with torch.no_grad():
        ys = logits.forward_stacked(xs, S)
    sv, sm = ys.double().var(0), ys.double().mean(0)
    mom = net.predictive_moments(xs)
    ratio = (mom.var.double() / sv).flatten()
    zm = ((mom.mean.double() - sm).abs() / (sv / S).sqrt()).max().item()
    report({"what": "logit variance, moments / 2048 weight draws", "rows": rows, "ratio_min": round(ratio.min().item(), 4),
            "ratio_max": round(ratio.max().item(), 4), "ratio_median": round(ratio.median().item(), 4),
            "worst_ratio": round(max(ratio.max().item(), 1.0 / ratio.min().item()), 4),
            "mean_worst_standard_errors": round(zm, 2)})
_lib.check_device(dev)
