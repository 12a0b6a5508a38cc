"""Training without sampling (K18, csrc/bnn_moments_bwd.hip) against the nearest sampled route, on the GPU box: 784-1200-1200-10
at B = 512, device-event timing after warm-up, median of repeated windows (minimum and maximum stated).
  moments:  one step = forward_moments + sample_moments(S) + cross-entropy + backward (torch.autograd.grad on all twelve
            posterior tensors): per layer the operand launch and ONE contraction forward, the ReLU out of place, ONE sampling
            launch on the logits; backward K10's launches for the first layer and the three-accumulator launches behind it.
  baseline: the same network of LocalReparamLinear layers on the MC-batched path at S samples: forward + cross-entropy +
            backward.  It uses nothing K18 adds, so the same file times it at the parent commit (--package PATH puts another
            checkout's package in front of this one's).
  layers:   the two new contraction launches (bnn_moments_backward_input / _weight, with their algorithmic TFLOP/s: 6 B N K
            each) and the ReLU's backward for the two layers that take a Moments input.
Every (what, mode) runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per
measurement.
usage: bench_moments_train.py [--batch 512] [--samples 8] [--iters N] [--windows W] [--what moments|baseline|layers] [--package PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--what", choices=["moments", "baseline", "layers"])
ap.add_argument("--mode", choices=["bf16", "f32"])
ap.add_argument("--package", default=None)
ap.add_argument("--step-timeout", type=int, default=150)
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.package) if args.package else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if args.mode is None:
    for what in ([args.what] if args.what else ["moments", "baseline", "layers"]):
        for mode in ("bf16", "f32"):
            cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--mode", mode, "--batch", str(args.batch),
                   "--samples", str(args.samples), "--iters", str(args.iters), "--windows", str(args.windows)]
            if args.package:
                cmd += ["--package", args.package]
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            if rc != 0:
                sys.exit("bench_moments_train: %s / %s ended with status %d; nothing more is started" % (what, mode, rc))
    sys.exit(0)

import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, LocalReparamLinear

assert args.windows >= 5 and args.what is not None
dev = torch.device("cuda:0")
B, S = args.batch, args.samples
WIDTHS = [784, 1200, 1200, 10]


class Net(BayesianNetworkModule):
    def __init__(self):
        super().__init__(WIDTHS[0], WIDTHS[-1], samples=S)
        self.layers = torch.nn.Sequential(LocalReparamLinear(784, 1200), torch.nn.ReLU(), LocalReparamLinear(1200, 1200),
                                          torch.nn.ReLU(), LocalReparamLinear(1200, 10))

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
target = torch.randint(0, 10, (B,), device=dev).repeat(S)
params = [p for p in net.parameters()]

if args.what == "moments":
    bnn.nn.moment_activations(net)                                  # ReLU -> nn.MomentReLU (the parent on tensors)

    def step():
        ys = net.sample_moments(net.forward_moments(x), S)
        return torch.autograd.grad(F.cross_entropy(ys.reshape(-1, 10), target), params)

    report({"what": "forward_moments + sample_moments + cross-entropy + backward", "S": S}, timed(step))
    report({"what": "forward_moments + sample_moments + cross-entropy (no backward)", "S": S},
           timed(lambda: F.cross_entropy(net.sample_moments(net.forward_moments(x), S).reshape(-1, 10), target)))
elif args.what == "baseline":
    net.mc_batched = True

    def step():
        ys = torch.stack(net(x, S))
        return torch.autograd.grad(F.cross_entropy(ys.reshape(-1, 10), target), params)

    report({"what": "LocalReparamLinear MC-batched forward + cross-entropy + backward", "S": S}, timed(step))
    report({"what": "LocalReparamLinear MC-batched forward + cross-entropy (no backward)", "S": S},
           timed(lambda: F.cross_entropy(torch.stack(net(x, S)).reshape(-1, 10), target)))
else:
    lib = _lib.load()
    code = ops._compute_code(args.mode)
    st = _lib.stream_ptr(dev)
    P = _lib.ptr
    for K, N in zip(WIDTHS[1:-1], WIDTHS[2:]):                      # the layers whose input carries a variance
        g = torch.Generator(device=dev).manual_seed(1)
        a_m, a_v = torch.randn(B, K, device=dev, generator=g), torch.rand(B, K, device=dev, generator=g)
        G_m, G_v = torch.randn(B, N, device=dev, generator=g), torch.randn(B, N, device=dev, generator=g)
        mu_w, rho_w = torch.randn(N, K, device=dev, generator=g) / K ** 0.5, torch.full((N, K), -3.0, device=dev)
        s2_w, _ = ops._lrt_prepare_raw(rho_w, None)
        g_am, g_av, g_mu, g_rho = torch.empty_like(a_m), torch.empty_like(a_v), torch.empty_like(mu_w), torch.empty_like(rho_w)
        r_m, r_v = torch.empty_like(a_m), torch.empty_like(a_v)

        def dgrad():
            _lib.check(lib.bnn_moments_backward_input(P(G_m), P(G_v), P(mu_w), P(s2_w), P(a_m), K, P(g_am), P(g_av), B, N, K, code, 0,
                                                      st), "bnn_moments_backward_input")

        def wgrad():
            _lib.check(lib.bnn_moments_backward_weight(P(a_m), P(a_v), K, P(G_m), P(G_v), P(mu_w), P(rho_w), P(g_mu), P(g_rho), None,
                                                       None, None, B, N, K, code, 0, st), "bnn_moments_backward_weight")

        def relu_bwd():
            _lib.check(lib.bnn_moments_relu_backward(P(a_m), P(a_v), P(g_am), P(g_av), P(r_m), P(r_v), B * K, st),
                       "bnn_moments_relu_backward")

        for name, fn in (("bnn_moments_backward_input", dgrad), ("bnn_moments_backward_weight", wgrad)):
            t = timed(fn)
            grid = ((K + 63) // 64) * (((B if fn is dgrad else N) + 63) // 64)
            report({"what": name, "K": K, "N": N, "workgroups": grid, "tflops": round(6.0 * B * N * K / t[0] / 1e9, 2)}, t)
        report({"what": "bnn_moments_relu_backward", "n": B * K}, timed(relu_bwd))
_lib.check_device(dev)
