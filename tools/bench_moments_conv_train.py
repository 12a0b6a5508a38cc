"""Training conv nets without sampling (K19, csrc/bnn_conv3d.hip k_moments_conv3d_bwd) against the nearest sampled route, on the
GPU box: device-event timing after warm-up, median of repeated windows (minimum and maximum stated).
  networks: tail  -- the MNIST example's Bayesian tail on (B, 64, 6, 6): NormalConv2d(64, 64, 3, stride 2, padding 1) -> ELU ->
                     flatten -> NormalLinear(576, 10); its conv sees a deterministic input (K11's backward launches);
            deep  -- the same with NormalConv2d(64, 64, 3, padding 1) -> ELU in front, so that the tail's conv takes a Moments
                     input: the three-accumulator launches and the ELU's backward run.
  moments:  one step = forward_moments + sample_moments(S) + cross-entropy + backward (torch.autograd.grad on every posterior
            tensor), with nn.conv_moment_training switched on.
  baseline: the same networks of LocalReparamConv2d / LocalReparamLinear layers on the MC-batched path at S samples: forward +
            cross-entropy + backward.  It uses nothing K19 adds, so the same file times it at the parent commit (--package PATH
            puts another checkout's package in front of this one's).
  layers:   the two new contraction launches (bnn_conv3d_moments_backward_input / _weight, with their algorithmic TFLOP/s:
            6 B P O K each) and bnn_moments_elu_backward at the deep network's shapes.
Every (what, net, mode) runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per
measurement.
usage: bench_moments_conv_train.py [--batch 1024] [--samples 8] [--iters N] [--windows W] [--what moments|baseline|layers]
                                   [--package PATH]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--what", choices=["moments", "baseline", "layers"])
ap.add_argument("--net", choices=["tail", "deep"])
ap.add_argument("--mode", choices=["bf16", "f32"])
ap.add_argument("--package", default=None)
ap.add_argument("--step-timeout", type=int, default=150)
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.package) if args.package else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if args.mode is None:
    for what in ([args.what] if args.what else ["moments", "baseline", "layers"]):
        for net in (["deep"] if what == "layers" else ["tail", "deep"]):
            for mode in ("bf16", "f32"):
                cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--net", net, "--mode", mode, "--batch", str(args.batch),
                       "--samples", str(args.samples), "--iters", str(args.iters), "--windows", str(args.windows)]
                if args.package:
                    cmd += ["--package", args.package]
                rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
                if rc != 0:
                    sys.exit("bench_moments_conv_train: %s / %s / %s ended with status %d; nothing more is started" % (what, net, mode, rc))
    sys.exit(0)

import torch
import torch.nn.functional as F

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd.nn import (BayesianNetworkModule, LocalReparamConv2d, LocalReparamLinear, NormalConv2d, NormalLinear)

assert args.windows >= 5 and args.what is not None and args.net is not None
dev = torch.device("cuda:0")
B, S = args.batch, args.samples


class Net(BayesianNetworkModule):
    def __init__(self, conv, linear, deep):
        super().__init__(64, 10, samples=S)
        front = [conv(64, 64, 3, padding=1), torch.nn.ELU()] if deep else []
        self.layers = torch.nn.Sequential(*front, conv(64, 64, 3, stride=2, padding=1), torch.nn.ELU(), torch.nn.Flatten(),
                                          linear(576, 10))

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
    row.update({"net": args.net, "mode": args.mode, "B": B, "ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)})
    print(json.dumps(row), flush=True)


torch.manual_seed(0)
bnn.set_compute(args.mode)
x = torch.randn(B, 64, 6, 6, device=dev)
target = torch.randint(0, 10, (B,), device=dev).repeat(S)

if args.what == "moments":
    net = Net(NormalConv2d, NormalLinear, args.net == "deep").to(dev)
    params = [p for p in net.parameters()]
    bnn.nn.moment_activations(net)                                  # ELU -> nn.MomentELU (the parent on tensors)
    bnn.nn.conv_moment_training(True)

    def step():
        ys = net.sample_moments(net.forward_moments(x), S)
        return torch.autograd.grad(F.cross_entropy(ys.reshape(-1, 10), target), params)

    report({"what": "forward_moments + sample_moments + cross-entropy + backward", "S": S}, timed(step))
    report({"what": "forward_moments + sample_moments + cross-entropy (no backward)", "S": S},
           timed(lambda: F.cross_entropy(net.sample_moments(net.forward_moments(x), S).reshape(-1, 10), target)))
elif args.what == "baseline":
    net = Net(LocalReparamConv2d, LocalReparamLinear, args.net == "deep").to(dev)
    params = [p for p in net.parameters()]
    net.mc_batched = True

    def step():
        ys = torch.stack(net(x, S))
        return torch.autograd.grad(F.cross_entropy(ys.reshape(-1, 10), target), params)

    report({"what": "LocalReparamConv2d / Linear MC-batched forward + cross-entropy + backward", "S": S}, timed(step))
    report({"what": "LocalReparamConv2d / Linear MC-batched forward + cross-entropy (no backward)", "S": S},
           timed(lambda: F.cross_entropy(torch.stack(net(x, S)).reshape(-1, 10), target)))
else:
    lib = _lib.load()
    code = ops._compute_code(args.mode)
    st = _lib.stream_ptr(dev)
    P = _lib.ptr
    C = O = 64
    sh, (_, OH, OW) = ops._conv3d_shape((B, C, 1, 6, 6), (O, C, 1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 1), 1)
    g = torch.Generator(device=dev).manual_seed(1)
    a_m, a_v = torch.randn(B, C, 6, 6, device=dev, generator=g), torch.rand(B, C, 6, 6, device=dev, generator=g)
    G_m, G_v = torch.randn(B, O, OH, OW, device=dev, generator=g), torch.randn(B, O, OH, OW, device=dev, generator=g)
    mu_w, rho_w = torch.randn(O, C, 3, 3, device=dev, generator=g) / 24.0, torch.full((O, C, 3, 3), -3.0, device=dev)
    s2_w, _ = ops._lrt_prepare_raw(rho_w, None)
    g_am, g_av, g_mu, g_rho = torch.empty_like(a_m), torch.empty_like(a_v), torch.empty_like(mu_w), torch.empty_like(rho_w)
    r_m, r_v = torch.empty_like(a_m), torch.empty_like(a_v)
    nb = lib.bnn_conv3d_moments_wgrad_workspace(ctypes.byref(sh))
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)

    def dgrad():
        _lib.check(lib.bnn_conv3d_moments_backward_input(P(G_m), P(G_v), P(mu_w), P(s2_w), P(a_m), P(g_am), P(g_av), ctypes.byref(sh), code,
                                                         st), "bnn_conv3d_moments_backward_input")

    def wgrad():
        _lib.check(lib.bnn_conv3d_moments_backward_weight(P(a_m), P(a_v), P(G_m), P(G_v), P(mu_w), P(rho_w), P(g_mu), P(g_rho), None, None,
                                                          None, ctypes.byref(sh), code, P(ws), nb, st), "bnn_conv3d_moments_backward_weight")

    def elu_bwd():
        _lib.check(lib.bnn_moments_elu_backward(P(a_m), P(a_v), P(g_am), P(g_av), P(r_m), P(r_v), a_m.numel(), 1.0, st),
                   "bnn_moments_elu_backward")

    flop = 6.0 * B * OH * OW * O * C * 9
    for name, fn in (("bnn_conv3d_moments_backward_input", dgrad), ("bnn_conv3d_moments_backward_weight", wgrad)):
        t = timed(fn)
        row = {"what": name, "shape": "(%d, 64, 6, 6) -> 64, 3 x 3, stride 2, padding 1" % B, "tflops": round(flop / t[0] / 1e9, 2)}
        if fn is wgrad:
            row["slabs"] = nb // (3 * O * C * 9 * 4)
        report(row, t)
    report({"what": "bnn_moments_elu_backward", "n": a_m.numel()}, timed(elu_bwd))
_lib.check_device(dev)
