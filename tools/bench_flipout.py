"""Flipout on the MC-batched path (GPU box): device-event timing, median of repeated windows, FashionMNIST shapes
(examples/FashionMNIST/model.py: Flipout conv 64 -> 64, 3 x 3, stride 2, pad 1 on 6 x 6 images; Flipout linear 576 -> 10).
  kernel: ONE keyed bnn_conv2d_flipout_forward_mc launch for S samples of a shared input against S launches of
          bnn_conv2d_flipout_forward on the fanned-out input, and against ONE such launch on all S * B fanned-out images
          (same [mean | stddev] operand, sign tensors and the fanned-out input prepared outside);
  net:    the FashionMNIST net's forward, MC-batched (mc_batched = True) against the serial device loop, fp32 and bf16 modes.
usage: bench_flipout.py [--batch 512] [--samples 8] [--iters N] [--windows W]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd._rng import DrawKey
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, FlipOutNormalConv2d, FlipoutNormalLinear

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=7)
args = ap.parse_args()

lib = _lib.load()
dev = torch.device("cuda:0")
_lib.ensure_workspace(dev)
P = _lib.ptr
B, S = args.batch, args.samples


class FashionNet(BayesianNetworkModule):
    def __init__(self, samples):
        super().__init__(1, 10, samples)
        self.layers = torch.nn.Sequential(
            torch.nn.Conv2d(1, 32, 5, padding=2, stride=2), torch.nn.BatchNorm2d(32), torch.nn.ELU(),
            torch.nn.Conv2d(32, 32, 3, padding=1, stride=1), torch.nn.ELU(),
            torch.nn.Conv2d(32, 64, 3, padding=0, stride=2), torch.nn.ELU(),
            FlipOutNormalConv2d(64, 64, 3, padding=1, stride=2), torch.nn.ELU(),
            torch.nn.Flatten(), FlipoutNormalLinear(576, 10), torch.nn.Softmax(dim=-1))

    def _forward(self, x):
        return self.layers(x)


def median_us(fn):
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
        ts.append(e0.elapsed_time(e1) / args.iters * 1e3)
    return round(statistics.median(ts), 2)


def shape(b):
    sh = _lib.Conv2dShape()
    sh.B, sh.C, sh.H, sh.W, sh.O, sh.KH, sh.KW = b, 64, 6, 6, 64, 3, 3
    sh.stride_h = sh.stride_w = 2
    sh.pad_h = sh.pad_w = 1
    sh.dil_h = sh.dil_w = 1
    sh.groups = 1
    return sh


def kernel_case():
    torch.manual_seed(0)
    layer = FlipOutNormalConv2d(64, 64, 3, padding=1, stride=2).to(dev)
    w2 = ops.flipout_conv_weights(layer.weight.mean, layer.weight.scale)
    kp = w2.shape[1]
    x = torch.randn(B, 64, 6, 6, device=dev)
    xf = x.unsqueeze(0).expand(S, *x.shape).contiguous()
    key = DrawKey(1234, 77, 0, S, 5, gen=1)
    sg = ops.flipout_signs(key, B, 128, dev)
    R, Sg = sg[:, :, :64].contiguous(), sg[:, :, 64:].contiguous()
    y = torch.empty(S * B, 64, 3, 3, device=dev)
    sh1, shS = shape(B), shape(B)
    r = ops._rng_struct(key, dev)
    sp = _lib.stream_ptr(dev)

    def fused():
        lib.bnn_conv2d_flipout_forward_mc(P(x), 0, P(w2), kp, P(y), B * 64 * 9, ctypes.byref(shS), S, ctypes.byref(r), 0, sp)

    def per_sample():
        for s in range(S):
            lib.bnn_conv2d_flipout_forward(P(xf[s]), P(w2), kp, P(Sg[s]), P(R[s]), P(y[s * B:(s + 1) * B]), ctypes.byref(sh1), 0, sp)
    shF = shape(S * B)

    def fanned():
        # ONE existing launch on the S * B fanned-out images with their materialized signs: the same machine fill as the fused
        # launch, so the difference is what sharing the mean contraction (and making the signs in the kernel) gains
        lib.bnn_conv2d_flipout_forward(P(xf), P(w2), kp, P(Sg), P(R), P(y), ctypes.byref(shF), 0, sp)
    a, b, c = median_us(fused), median_us(per_sample), median_us(fanned)
    _lib.check_device(dev)
    return dict(case="flipout_conv_kernel", B=B, S=S, fused_mc_us=a, s_launches_us=b, fanned_one_launch_us=c,
                ratio_vs_s_launches=round(a / b, 3), ratio_vs_fanned=round(a / c, 3))


def net_case(mode):
    bnn.set_compute(mode)
    torch.manual_seed(0)
    net = FashionNet(S).to(dev).eval()
    x = torch.randn(B, 1, 28, 28, device=dev)
    res = dict(case="fashion_net_forward", mode=mode, B=B, S=S)
    with torch.no_grad():
        net.mc_batched = True
        res["mc_batched_us"] = median_us(lambda: net.forward_stacked(x))
        net.mc_batched = False
        res["serial_loop_us"] = median_us(lambda: net.forward_stacked(x))
    res["speedup"] = round(res["serial_loop_us"] / res["mc_batched_us"], 2)
    _lib.check_device(dev)
    return res


print(json.dumps(kernel_case()))
for m in ("bf16", "f32"):
    print(json.dumps(net_case(m)))
