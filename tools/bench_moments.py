"""Sampling-free inference (K16, csrc/bnn_moments.hip) against the sampler it replaces, on the GPU box: 784-1200-1200-10 at
B = 512, device-event timing after warm-up, median of repeated windows.
  moments: predictive_uncertainty(propagation='moments') -- per layer the operand launch + ONE three-contraction launch, then one
           sampling launch and the tail; the S samples exist only as logits;
  samples: predictive_uncertainty on the MC-batched path (nn.fuse_activations with bf16 activations and the fused head, the
           draw-once dense route in the bf16 mode): S stochastic forwards in one pass.
  layers:  every launch of the moment pass on its own -- the operand launch (bnn_lrt_prepare), the contraction
           (bnn_moments_forward, with its algorithmic TFLOP/s: 4 B N K for a deterministic input, 6 B N K for a Moments input),
           the sampling launch and the tail at each S.
Every (what, mode) runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per
measurement.
usage: bench_moments.py [--batch 512] [--samples 8,32,100] [--iters N] [--windows W]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--samples", default="8,32,100")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--what", choices=["moments", "samples", "layers"])
ap.add_argument("--mode", choices=["bf16", "f32"])
ap.add_argument("--step-timeout", type=int, default=150)
args = ap.parse_args()

if args.what is None:
    for what in ("moments", "samples", "layers"):
        for mode in ("bf16", "f32"):
            cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--mode", mode, "--batch", str(args.batch),
                   "--samples", args.samples, "--iters", str(args.iters), "--windows", str(args.windows)]
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            if rc != 0:
                sys.exit("bench_moments: %s / %s ended with status %d; nothing more is started" % (what, mode, rc))
    sys.exit(0)

import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd._rng import DrawKey, generator_for
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, NormalLinear

assert args.windows >= 5
dev = torch.device("cuda:0")
B = args.batch
SAMPLES = [int(s) for s in args.samples.split(",")]
WIDTHS = [784, 1200, 1200, 10]


class Net(BayesianNetworkModule):
    def __init__(self):
        super().__init__(WIDTHS[0], WIDTHS[-1], samples=SAMPLES[0])
        self.layers = torch.nn.Sequential(NormalLinear(784, 1200), torch.nn.ReLU(), NormalLinear(1200, 1200), torch.nn.ReLU(),
                                          NormalLinear(1200, 10))

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


def report(row, t):
    row.update({"mode": args.mode, "B": B, "ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)})
    print(json.dumps(row), flush=True)


torch.manual_seed(0)
bnn.set_compute(args.mode)
net = Net().to(dev)
x = torch.randn(B, 784, device=dev)

if args.what == "moments":
    bnn.nn.fuse_activations(net)
    for S in SAMPLES:
        report({"what": "predictive_uncertainty(propagation='moments')", "S": S},
               timed(lambda: net.predictive_uncertainty(x, S, inputs="logits", propagation="moments")))
    report({"what": "predictive_moments", "S": 0}, timed(lambda: net.predictive_moments(x)))
elif args.what == "samples":
    bnn.nn.fuse_activations(net, bf16_activations=True, fuse_head=True)
    net.mc_batched = True
    with torch.no_grad():
        for S in SAMPLES:
            report({"what": "predictive_uncertainty (MC-batched samples)", "S": S},
                   timed(lambda: net.predictive_uncertainty(x, S, inputs="logits")))
else:
    lib = _lib.load()
    code = ops._compute_code(args.mode)
    st = _lib.stream_ptr(dev)
    a_m, a_v = x, None
    for i, (K, N) in enumerate(zip(WIDTHS[:-1], WIDTHS[1:])):
        layer = net.layers[2 * i]
        mu_w, rho_w, mu_b, rho_b = [t.detach() for t in (layer.weight.mean, layer.weight.scale, layer.bias.mean, layer.bias.scale)]
        report({"what": "bnn_lrt_prepare", "K": K, "N": N}, timed(lambda: ops._lrt_prepare_raw(rho_w, rho_b)))
        s2_w, s2_b = ops._lrt_prepare_raw(rho_w, rho_b)
        om, ov = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
        flags = _lib.FLAG_RELU if i < 2 else 0
        P = _lib.ptr

        def launch():
            _lib.check(lib.bnn_moments_forward(P(a_m), P(a_v), K, P(mu_w), P(s2_w), P(mu_b), P(s2_b), P(om), P(ov), B, N, K, code,
                                               flags, st), "bnn_moments_forward")

        t = timed(launch)
        flop = (6.0 if a_v is not None else 4.0) * B * N * K
        report({"what": "bnn_moments_forward", "K": K, "N": N, "input": "moments" if a_v is not None else "deterministic",
                "relu": bool(flags), "tflops": round(flop / t[0] / 1e9, 2)}, t)
        a_m, a_v = om, ov
    mom = ops.Moments(a_m, a_v)
    for S in SAMPLES:
        key = DrawKey(1, 7, 0, S, 0, gen=generator_for(args.mode))
        report({"what": "bnn_moments_sample", "S": S}, timed(lambda: ops.moments_sample(mom, key, S)))
        ys = ops.moments_sample(mom, key, S)
        report({"what": "bnn_mc_uncertainty", "S": S}, timed(lambda: ops.mc_uncertainty(ys, "logits")))
_lib.check_device(dev)
