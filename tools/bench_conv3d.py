"""NormalConv3d on the MC-batched device path (GPU box): device-event timing after warm-up, median of repeated windows.
  new:   one layer call in an MC context of S samples on a shared input -- one draw launch + one implicit-GEMM launch
         (csrc/bnn_conv3d.hip); forward, and forward + backward (input and posterior gradients).
  old:   the route it replaces -- K1 draw of the S weights and biases (ops._sample_affine_philox_raw), then torch conv3d
         (MIOpen, fp32) once per sample; forward, and forward + backward through autograd.
Reports ms, achieved TFLOP/s (2 B O OD OH OW (C/groups) KD KH KW per sample forward, 3x that for forward + backward) and the
share of the MFMA peak of the mode (bf16 2.5 PF dense, fp32 157.3 TF).  One JSON line per measurement.
usage: bench_conv3d.py [--batch 8] [--cin 32] [--cout 64] [--vol 32] [--samples 8] [--iters N] [--windows W]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _mc, ops
from bayesianneuralnetworks_amd.nn import NormalConv3d

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--cin", type=int, default=32)
ap.add_argument("--cout", type=int, default=64)
ap.add_argument("--vol", type=int, default=32)
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()

PEAK = {"bf16": 2.5e15, "f32": 157.3e12}
dev = torch.device("cuda:0")
B, C, O, V, S = args.batch, args.cin, args.cout, args.vol, args.samples
torch.manual_seed(0)
layer = NormalConv3d(C, O, 3, padding=1).to(dev)
x = torch.randn(B, C, V, V, V, device=dev)
flop_fwd = 2.0 * B * O * V ** 3 * C * 27 * S


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


def new_fwd():
    with torch.no_grad(), _mc.McContext(S, B, 0):
        layer(x)


def new_bwd():
    xg = x.detach().requires_grad_(True)
    with _mc.McContext(S, B, 0):
        y = layer(xg)
    y.backward(torch.ones_like(y))


def old_fwd(grad=False):
    with torch.set_grad_enabled(grad):
        kw, kb = layer._fresh_keys(S, 0)
        w = ops.sample_affine_philox(layer.weight.mean, layer.weight.scale, kw)
        b = ops.sample_affine_philox(layer.bias.mean, layer.bias.scale, kb)
        xg = x.detach().requires_grad_(grad)
        ys = [torch.nn.functional.conv3d(xg, w[s], b[s], 1, 1) for s in range(S)]
        if grad:
            torch.autograd.backward(ys, [torch.ones_like(t) for t in ys])


for mode in ("bf16", "f32"):
    bnn.set_compute(mode)
    for what, fn, flop in (("forward", new_fwd, flop_fwd), ("forward+backward", new_bwd, 3 * flop_fwd)):
        ms = timed(fn)
        print(json.dumps({"route": "conv3d MC-batched (2 launches fwd)", "mode": mode, "pass": what, "B": B, "C": C, "O": O,
                          "vol": V, "S": S, "ms": round(ms, 4), "tflops": round(flop / ms / 1e9, 2),
                          "peak_share": round(flop / ms / 1e-3 / PEAK[mode], 4)}), flush=True)
bnn.set_compute("f32")
for what, fn, flop in (("forward", lambda: old_fwd(False), flop_fwd), ("forward+backward", lambda: old_fwd(True), 3 * flop_fwd)):
    ms = timed(fn)
    print(json.dumps({"route": "K1 draw + torch conv3d per sample (MIOpen fp32)", "mode": "f32", "pass": what, "B": B, "C": C,
                      "O": O, "vol": V, "S": S, "ms": round(ms, 4), "tflops": round(flop / ms / 1e9, 2),
                      "peak_share": round(flop / ms / 1e-3 / PEAK["f32"], 4)}), flush=True)
