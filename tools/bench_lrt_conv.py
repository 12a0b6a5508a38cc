"""LocalReparamConv2d / 3d (K11, k_lrt_conv3d of csrc/bnn_conv3d.hip) against NormalConv2d / 3d (their own launches: draw +
contraction; this change does not touch that route, so it is the parent commit's) on the MC-batched device path (GPU box):
device-event timing after warm-up, median of repeated windows, forward and forward + backward (input and posterior gradients).
  shapes:  lenet   (1024, 64, 6, 6) -> 64, k3 s2 p1;   cifar   (256, 128, 4, 4) -> 128, k3 p1;
           volume  (8, 32, 32, 32, 32) -> 64, k3 p1 (K7's)
  shared:      the layer sees the un-replicated batch (B rows in, S B rows out);   per-sample:  it sees S B rows.
  lrt:    one layer call in an MC context of S samples -- the sigma^2 launch + ONE paired-contraction launch;
  normal: NormalConvNd's route for the same call.
Every (shape, case, mode) runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line
per measurement: ms, and the algorithmic TFLOP/s of the route (one contraction = 2 B P O (C / groups) taps; lrt: 2 of them, once for
a shared input, S times otherwise; normal: S of them; forward + backward = 3 x forward).
usage: bench_lrt_conv.py [--samples 8] [--iters N] [--windows W]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"lenet": (2, 1024, 64, (6, 6), 64, 3, 2, 1), "cifar": (2, 256, 128, (4, 4), 128, 3, 1, 1),
          "volume": (3, 8, 32, (32, 32, 32), 64, 3, 1, 1)}

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--shape", choices=sorted(SHAPES))
ap.add_argument("--case", choices=["shared", "per-sample"])
ap.add_argument("--mode", choices=["bf16", "f32"])
ap.add_argument("--step-timeout", type=int, default=240)
args = ap.parse_args()

if args.case is None:
    for shape in ([args.shape] if args.shape else ["lenet", "cifar", "volume"]):
        for case in ("shared", "per-sample"):
            for mode in ("bf16", "f32"):
                cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--case", case, "--mode", mode,
                       "--samples", str(args.samples), "--iters", str(args.iters), "--windows", str(args.windows)]
                rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
                if rc != 0:
                    sys.exit("bench_lrt_conv: %s / %s / %s ended with status %d; nothing more is started" % (shape, case, mode, rc))
    sys.exit(0)

import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _mc
from bayesianneuralnetworks_amd.nn import LocalReparamConv2d, LocalReparamConv3d, NormalConv2d, NormalConv3d

assert args.windows >= 5
dev = torch.device("cuda:0")
nd, B, C, sp, O, k, stride, pad = SHAPES[args.shape]
S = args.samples
shared = args.case == "shared"
torch.manual_seed(0)
bnn.set_compute(args.mode)
lrt_cls, normal_cls = (LocalReparamConv2d, NormalConv2d) if nd == 2 else (LocalReparamConv3d, NormalConv3d)
layers = {"lrt": lrt_cls(C, O, k, stride, pad).to(dev), "normal": normal_cls(C, O, k, stride, pad).to(dev)}
x = torch.randn(B if shared else S * B, C, *sp, device=dev)
out = [(n + 2 * pad - k) // stride + 1 for n in sp]
P = 1
for n in out:
    P *= n
gy = torch.randn(S * B, O, *out, device=dev)
one = 2.0 * B * P * O * C * k ** nd
flop = {"lrt": 2 * one * (1 if shared else S), "normal": one * S}


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


def fwd(layer):
    with torch.no_grad(), _mc.McContext(S, B, 0):
        layer(x)


def fwd_bwd(layer):
    xg = x.detach().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    with _mc.McContext(S, B, 0):
        y = layer(xg)
    y.backward(gy)


for name, layer in layers.items():
    for what, fn, mult in (("forward", fwd, 1), ("forward+backward", fwd_bwd, 3)):
        ms, lo, hi = timed(lambda: fn(layer))
        print(json.dumps({"layer": name, "shape": args.shape, "case": args.case, "mode": args.mode, "pass": what, "B": B, "C": C,
                          "O": O, "P": P, "S": S, "ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "tflops": round(mult * flop[name] / ms / 1e9, 2)}), flush=True)
