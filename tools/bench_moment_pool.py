"""Moments through pooling (K20) on the GPU box: device-event timing, median of repeated windows.
  launch: forward and backward of the 2 x 2 / 2 moment-matched max pool (bnn_moments_pool3d_forward / _backward) on
          (1024, 64, 12, 12) and (512, 32, 28, 28), beside the standalone bnn_moments_elu launch on the same input element count
          and the launch's HBM byte floor (bytes moved / --hbm-gbs);
  net:    the LeNet-shaped net (NormalConv2d 1 -> 4, ELU, MaxPool2d(2), NormalConv2d 4 -> 6, ELU, AvgPool2d(2), NormalLinear,
          Softmax) at B = 512: predictive_uncertainty by moment propagation against the MC-batched sampler at S = 8, 32, 100, both
          compute modes, as ratios.
Every case runs in a child process of its own under a time limit, and nothing is started after a case that failed.
usage: bench_moment_pool.py [--iters N] [--windows W] [--timeout SECONDS] [--hbm-gbs 8000] [--case NAME]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--timeout", type=int, default=120)
ap.add_argument("--hbm-gbs", type=float, default=8000.0)
ap.add_argument("--case", default=None)
args = ap.parse_args()

CASES = ["launch:1024,64,12,12", "launch:512,32,28,28", "net:f32", "net:bf16"]

if args.case is None:
    for case in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--iters", str(args.iters), "--windows", str(args.windows),
               "--hbm-gbs", str(args.hbm_gbs)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(case=case, failed=rc)))
            sys.exit(1)
    sys.exit(0)

import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd import nn as bnn_nn
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, NormalConv2d, NormalLinear

lib = _lib.load()
dev = torch.device("cuda:0")
_lib.ensure_workspace(dev)
P = _lib.ptr


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


class LeNet(BayesianNetworkModule):
    def __init__(self, samples):
        super().__init__(1, 10, samples)
        tn = torch.nn
        self.layers = tn.Sequential(NormalConv2d(1, 4, 3), tn.ELU(), tn.MaxPool2d(2), NormalConv2d(4, 6, 3), tn.ELU(), tn.AvgPool2d(2),
                                    tn.Flatten(), NormalLinear(24, 10), tn.Softmax(dim=-1))
        bnn_nn.moment_activations(self)

    def _forward(self, x):
        return self.layers(x)


def launch_case(shape):
    torch.manual_seed(0)
    m, v = torch.randn(shape, device=dev), torch.rand(shape, device=dev) + 1e-3
    out_shape = shape[:2] + (shape[2] // 2, shape[3] // 2)
    om, ov = torch.empty(out_shape, device=dev), torch.empty(out_shape, device=dev)
    G_m, G_v = torch.randn(out_shape, device=dev), torch.randn(out_shape, device=dev)
    gm, gv, em, ev = torch.empty_like(m), torch.empty_like(v), torch.empty_like(m), torch.empty_like(v)
    sh = ops._pool3d_shape(shape, (2, 2), (2, 2), (0, 0), (1, 1))
    sp = _lib.stream_ptr(dev)
    n_in, n_out = m.numel(), om.numel()
    res = dict(case="max_pool_2x2", shape=list(shape))
    res["forward_us"] = median_us(lambda: lib.bnn_moments_pool3d_forward(P(m), P(v), P(om), P(ov), ctypes.byref(sh), _lib.POOL_MAX, 0, sp))
    res["backward_us"] = median_us(lambda: lib.bnn_moments_pool3d_backward(P(m), P(v), P(G_m), P(G_v), P(gm), P(gv), ctypes.byref(sh),
                                                                           _lib.POOL_MAX, 0, sp))
    res["elu_same_elements_us"] = median_us(lambda: lib.bnn_moments_elu(P(m), P(v), P(em), P(ev), n_in, 1.0, sp))
    # bytes: the forward reads 2 n_in and writes 2 n_out floats; the backward zeroes 2 n_in, reads 2 n_in + 2 n_out, writes 2 n_in
    res["forward_hbm_floor_us"] = round(4 * (2 * n_in + 2 * n_out) / (args.hbm_gbs * 1e3), 2)
    res["backward_hbm_floor_us"] = round(4 * (6 * n_in + 2 * n_out) / (args.hbm_gbs * 1e3), 2)
    _lib.check_device(dev)
    return res


def net_case(mode):
    bnn.set_compute(mode)
    torch.manual_seed(0)
    net = LeNet(8).to(dev).eval()
    net.mc_batched = True
    x = torch.randn(512, 1, 28, 28, device=dev)[:, :, :14, :14].contiguous()
    res = dict(case="lenet_predictive_uncertainty", mode=mode, B=512)
    with torch.no_grad():
        for S in (8, 32, 100):
            mo = median_us(lambda: net.predictive_uncertainty(x, samples=S, inputs="probs", propagation="moments"))
            sa = median_us(lambda: net.predictive_uncertainty(x, samples=S, inputs="probs"))
            res["S%d" % S] = dict(moments_us=mo, sampled_us=sa, ratio=round(mo / sa, 3))
    _lib.check_device(dev)
    return res


kind, _, arg = args.case.partition(":")
print(json.dumps(launch_case(tuple(int(t) for t in arg.split(","))) if kind == "launch" else net_case(arg)), flush=True)
