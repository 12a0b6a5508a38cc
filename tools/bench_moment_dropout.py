"""MC dropout in a sampling-free pass (K22) on the GPU box: device-event timing, median of repeated windows.
  launch: bnn_moments_dropout (identity, ReLU, ELU) and bnn_moments_dropout_backward (ELU) at n = 512 x 1200, beside the standalone
          bnn_moments_elu / bnn_moments_elu_backward launches on the same elements;
  net:    the Titanic-shaped net (MCDropoutLinear 9 -> 256, ELU, MCDropoutLinear 256 -> 2, Softmax; p = 0.2) at B = 512:
          predictive_uncertainty(inputs='probs') by moment propagation against the MC-batched sampler at S = 8, 32, 100, both
          compute modes, as ratios.
Every case runs in a child process of its own under a time limit, and nothing is started after a case that failed.
usage: bench_moment_dropout.py [--iters N] [--windows W] [--timeout SECONDS] [--case NAME]"""
import argparse
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
ap.add_argument("--case", default=None)
args = ap.parse_args()

CASES = ["launch:614400", "net:f32", "net:bf16"]

if args.case is None:
    for case in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--iters", str(args.iters), "--windows", str(args.windows)]
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
from bayesianneuralnetworks_amd import _lib
from bayesianneuralnetworks_amd import nn as bnn_nn
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, MCDropoutLinear

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


class Titanic(BayesianNetworkModule):
    def __init__(self, samples):
        super().__init__(9, 2, samples)
        tn = torch.nn
        self.layers = tn.Sequential(MCDropoutLinear(9, 256, drop_prob=0.2), tn.ELU(), MCDropoutLinear(256, 2, drop_prob=0.2),
                                    tn.Softmax(dim=-1))
        bnn_nn.moment_activations(self)

    def _forward(self, x):
        return self.layers(x)


def launch_case(n):
    torch.manual_seed(0)
    m, v = torch.randn(n, device=dev), torch.rand(n, device=dev) + 1e-3
    G_m, G_v = torch.randn(n, device=dev), torch.randn(n, device=dev)
    om, ov, gm, gv = (torch.empty(n, device=dev) for _ in range(4))
    sp = _lib.stream_ptr(dev)
    res = dict(case="moments_dropout", n=n, p=0.2)
    for name, flag in (("identity", 0), ("relu", _lib.FLAG_RELU), ("elu", _lib.FLAG_ELU)):
        res["dropout_%s_us" % name] = median_us(lambda: lib.bnn_moments_dropout(P(m), P(v), P(om), P(ov), n, 0.2, flag, 1.0, sp))
    res["elu_alone_us"] = median_us(lambda: lib.bnn_moments_elu(P(m), P(v), P(om), P(ov), n, 1.0, sp))
    res["dropout_elu_backward_us"] = median_us(lambda: lib.bnn_moments_dropout_backward(P(m), P(v), P(G_m), P(G_v), P(gm), P(gv), n, 0.2,
                                                                                        _lib.FLAG_ELU, 1.0, sp))
    res["elu_backward_alone_us"] = median_us(lambda: lib.bnn_moments_elu_backward(P(m), P(v), P(G_m), P(G_v), P(gm), P(gv), n, 1.0, sp))
    _lib.check_device(dev)
    return res


def net_case(mode):
    bnn.set_compute(mode)
    bnn_nn.moment_estimator_layers()
    torch.manual_seed(0)
    net = Titanic(8).to(dev).eval()
    net.mc_batched = True
    x = torch.randn(512, 9, device=dev)
    res = dict(case="titanic_predictive_uncertainty", mode=mode, B=512, hidden=256)
    with torch.no_grad():
        for S in (8, 32, 100):
            mo = median_us(lambda: net.predictive_uncertainty(x, samples=S, inputs="probs", propagation="moments"))
            sa = median_us(lambda: net.predictive_uncertainty(x, samples=S, inputs="probs"))
            res["S%d" % S] = dict(moments_us=mo, sampled_us=sa, ratio=round(mo / sa, 3))
    _lib.check_device(dev)
    return res


kind, _, arg = args.case.partition(":")
print(json.dumps(launch_case(int(arg)) if kind == "launch" else net_case(arg)), flush=True)
