"""FlipOutNormalConv3d on the MC-batched device path (GPU box): device-event timing after warm-up, median of repeated windows.
  new:   one layer call in an MC context of S samples on a shared input -- one operand draw, one sign launch, one Flipout
         implicit-GEMM launch (csrc/bnn_conv3d.hip); forward, and forward + backward (input, weight.mean and weight.scale gradients).
  old:   the route it replaces, rebuilt here -- ops.flipout_signs, the shared input fanned out to S * B rows, two torch conv3d calls
         (MIOpen, fp32) and the elementwise sign products; forward, and forward + backward through autograd.
Reports ms, achieved TFLOP/s (two contractions: 4 B O OD OH OW C KD KH KW per sample forward, 3x that for forward + backward) and
the share of the MFMA peak of the mode (bf16 2.5 PF dense, fp32 157.3 TF).  One JSON line per measurement.
usage: bench_flipout3d.py [--batch 8] [--cin 32] [--cout 64] [--vol 32] [--samples 8] [--iters N] [--windows W]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _mc, ops
from bayesianneuralnetworks_amd.nn import FlipOutNormalConv3d

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
layer = FlipOutNormalConv3d(C, O, 3, padding=1).to(dev)
x = torch.randn(B, C, V, V, V, device=dev)
flop_fwd = 4.0 * B * O * V ** 3 * C * 27 * S


def timed(fn, iters=None, windows=None):
    iters, windows = iters or args.iters, windows or args.windows
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
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
        key = layer.flip_key
        sg = ops.flipout_signs(key, B, O + C, dev).reshape(S * B, O + C)
        R, Sg = sg[:, :O].reshape(S * B, O, 1, 1, 1), sg[:, O:].reshape(S * B, C, 1, 1, 1)
        xg = x.detach().requires_grad_(grad)
        xf = xg.unsqueeze(0).expand(S, *xg.shape).reshape(S * B, *xg.shape[1:])
        out = torch.nn.functional.conv3d(xf, layer.weight.mean, None, 1, 1)
        noise = torch.nn.functional.conv3d(xf * Sg, layer.weight.stddev, None, 1, 1)
        y = out + noise * R
        if grad:
            y.backward(torch.ones_like(y))


def report(route, mode, what, ms, flop):
    print(json.dumps({"route": route, "mode": mode, "pass": what, "B": B, "C": C, "O": O, "vol": V, "S": S, "ms": round(ms, 4),
                      "tflops": round(flop / ms / 1e9, 2), "peak_share": round(flop / ms / 1e-3 / PEAK[mode], 4)}), flush=True)


for mode in ("bf16", "f32"):
    bnn.set_compute(mode)
    for what, fn, flop in (("forward", new_fwd, flop_fwd), ("forward+backward", new_bwd, 3 * flop_fwd)):
        report("flipout conv3d MC-batched (3 launches fwd)", mode, what, timed(fn), flop)
bnn.set_compute("f32")
with _mc.McContext(S, B, 0), torch.no_grad():
    layer(x)                                                    # a key for the old route's signs
for what, fn, flop in (("forward", lambda: old_fwd(False), flop_fwd), ("forward+backward", lambda: old_fwd(True), 3 * flop_fwd)):
    report("signs + fan-out + 2x torch conv3d (MIOpen fp32)", "f32", what, timed(fn, 2, 3), flop)
