"""MC dropout on the MC-batched path (GPU box): device-event timing, median of repeated windows.
  mlp:     the BASELINE MLP shape as an MC-dropout net (784-1200-1200-10, ReLU, p = 0.2, batch 512, S = 8), bf16 mode;
  titanic: the Titanic net (9-256-2, ELU, Softmax, p = 0.2) at batch 1024, S = 100, fp32 and bf16 modes.
Each net's forward runs three ways on the same data: the MC-batched path (mc_batched = True), the serial device loop
(mc_batched = False: the reference's S x (nn.Linear + F.dropout)) and torch's batched equivalent (x expanded to S copies,
F.linear + F.dropout over S * B rows).  The kernel legs compare bnn_dense_forward_dropout with bnn_dense_forward on the same
operands (fan-out: the first layer; per sample: the second).  usage: bench_mc_dropout.py [--iters N] [--windows W]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd._rng import DrawKey
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, MCDropoutLinear

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=7)
args = ap.parse_args()

lib = _lib.load()
dev = torch.device("cuda:0")
_lib.ensure_workspace(dev)
P = _lib.ptr


class Net(BayesianNetworkModule):
    def __init__(self, sizes, act, samples, head=None):
        super().__init__(sizes[0], sizes[-1], samples)
        mods = []
        for i in range(len(sizes) - 1):
            mods.append(MCDropoutLinear(sizes[i], sizes[i + 1], drop_prob=.2))
            if i + 2 < len(sizes):
                mods.append(act())
        if head is not None:
            mods.append(head)
        self.layers = torch.nn.Sequential(*mods)

    def _forward(self, x):
        return self.layers(x)


def torch_batched(net, x, S):
    h = x.unsqueeze(0).expand(S, *x.shape).reshape(S * x.shape[0], -1)
    for m in net.layers:
        h = F.dropout(m.linear(h), m.drop_prob, True) if isinstance(m, MCDropoutLinear) else m(h)
    return h


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


def net_case(name, sizes, act, B, S, mode, head=None):
    bnn.set_compute(mode)
    torch.manual_seed(0)
    net = Net(sizes, act, S, head).to(dev)
    x = torch.randn(B, sizes[0], device=dev)
    res = dict(case=name, mode=mode, B=B, S=S)
    with torch.no_grad():
        net.mc_batched = True
        n0 = lib.bnn_launch_count()
        net.forward_stacked(x)
        torch.cuda.synchronize()
        res["launches_first"] = lib.bnn_launch_count() - n0
        n0 = lib.bnn_launch_count()
        net.forward_stacked(x)
        torch.cuda.synchronize()
        res["launches"] = lib.bnn_launch_count() - n0
        res["mc_batched_us"] = median_us(lambda: net.forward_stacked(x))
        net.mc_batched = False
        res["serial_loop_us"] = median_us(lambda: net.forward_stacked(x))
        res["torch_batched_us"] = median_us(lambda: torch_batched(net, x, S))
    bnn.set_compute("f32")
    print(json.dumps(res), flush=True)


def kernel_case(name, M, N, K, S, fan):
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((1 if fan else S), M, K, device=dev, generator=g).to(torch.bfloat16)
    w = ops.mean_bf16(torch.randn(N, K, device=dev, generator=g))
    kp = w.shape[-1]
    b = torch.randn(N, device=dev, generator=g)
    y = torch.empty(S, M, N, device=dev)
    r = ops._rng_struct(DrawKey(1, 77, 0, S, 0), dev)
    st = _lib.stream_ptr(dev)
    xs = 0 if fan else M * K

    def plain():
        _lib.check(lib.bnn_dense_forward(P(x), xs, K, P(w), 0, kp, P(b), 0, P(y), M * N, N, M, N, K, S, 0, st), "bnn_dense_forward")

    def fused():
        _lib.check(lib.bnn_dense_forward_dropout(P(x), xs, K, P(w), 0, kp, P(b), 0, P(y), M * N, N, M, N, K, S, 0, 0.2,
                                                 ctypes.byref(r), st), "bnn_dense_forward_dropout")
    res = dict(case=name, M=M, N=N, K=K, S=S, fan_out=fan, dense_forward_us=median_us(plain), dense_forward_dropout_us=median_us(fused))
    res["ratio"] = round(res["dense_forward_dropout_us"] / res["dense_forward_us"], 3)
    print(json.dumps(res), flush=True)


kernel_case("mlp_layer1_fanout", 512, 1200, 784, 8, True)
kernel_case("mlp_layer2_per_sample", 512, 1200, 1200, 8, False)
net_case("mlp", [784, 1200, 1200, 10], torch.nn.ReLU, 512, 8, "bf16")
net_case("titanic", [9, 256, 2], torch.nn.ELU, 1024, 100, "f32", torch.nn.Softmax(dim=-1))
net_case("titanic", [9, 256, 2], torch.nn.ELU, 1024, 100, "bf16", torch.nn.Softmax(dim=-1))
_lib.check_device(dev)
