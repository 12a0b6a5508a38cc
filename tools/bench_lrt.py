"""LocalReparamLinear (K10, csrc/bnn_lrt.hip) against NormalLinear (draw + dense) on the MC-batched device path (GPU box):
device-event timing after warm-up, median of repeated windows, forward and forward + backward (input and posterior gradients).
  shared:      784 -> 1200 on the un-replicated batch (B rows in, S B rows out): the first Bayesian layer of a network;
  per-sample:  1200 -> 1200 on S B rows: every later layer.
  lrt:    one layer call in an MC context of S samples -- the operand launch + ONE paired-contraction launch;
  normal: NormalLinear's route for the same call -- the draw of the S weights (bnn_draw_multi) + the dense contraction per sample
          (bf16), or the fused sampled GEMM (fp32 training path).
Every (case, mode) runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per
measurement: ms, and the algorithmic TFLOP/s of the route (lrt: 2 contractions of 2 B N K, once for a shared input, S times
otherwise; normal: S contractions of 2 B N K; forward + backward = 3 x forward).
usage: bench_lrt.py [--batch 512] [--samples 8] [--iters N] [--windows W]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--case", choices=["shared", "per-sample"])
ap.add_argument("--mode", choices=["bf16", "f32"])
ap.add_argument("--step-timeout", type=int, default=120)
args = ap.parse_args()

if args.case is None:
    for case in ("shared", "per-sample"):
        for mode in ("bf16", "f32"):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--mode", mode, "--batch", str(args.batch),
                   "--samples", str(args.samples), "--iters", str(args.iters), "--windows", str(args.windows)]
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            if rc != 0:
                sys.exit("bench_lrt: %s / %s ended with status %d; nothing more is started" % (case, mode, rc))
    sys.exit(0)

import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _mc
from bayesianneuralnetworks_amd.nn import LocalReparamLinear, NormalLinear

assert args.windows >= 5
dev = torch.device("cuda:0")
B, S = args.batch, args.samples
K, N = (784, 1200) if args.case == "shared" else (1200, 1200)
shared = args.case == "shared"
torch.manual_seed(0)
bnn.set_compute(args.mode)
layers = {"lrt": LocalReparamLinear(K, N).to(dev), "normal": NormalLinear(K, N).to(dev)}
x = torch.randn(B if shared else S * B, K, device=dev)
gy = torch.randn(S * B, N, device=dev)
flop = {"lrt": 2.0 * 2 * B * N * K * (1 if shared else S), "normal": 2.0 * B * N * K * S}


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
        print(json.dumps({"layer": name, "case": args.case, "mode": args.mode, "pass": what, "B": B, "K": K, "N": N, "S": S,
                          "ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "tflops": round(mult * flop[name] / ms / 1e9, 2)}), flush=True)
