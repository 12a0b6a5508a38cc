"""The head of a sampling-free pass (K21, csrc/bnn_moments_head.hip) on the GPU box: the CIFAR10 example's model with its real
MultivariateNormalLinear(128, 10) head at B = 256, device-event timing after warm-up, median of repeated windows.
  moments:    predictive_uncertainty(inputs='probs', propagation='moments') with covariance off and on (on: one
              bnn_moments_head_cov launch more, and the correlated sampler in place of the independent one), and
              predictive_moments alone, at every S;
  samples:    predictive_uncertainty on the MC-batched path with nn.keyed_mvn_draws() on: S stochastic forwards in one pass.  It
              uses nothing K21 adds, so the same file times it at the parent commit: --package PATH puts another checkout's
              package in front of this one's (the baseline of the comparison is that run, not this tree's);
  launches:   the four new launches on their own at the head's shape (O = 10, K = 128): bnn_mvn_moments_prepare,
              bnn_mvn_moments_forward, bnn_moments_head_cov, bnn_moments_sample_cov at every S (beside bnn_moments_sample).
Every (what, mode) runs in a child process of its own under a time limit; the first failure ends the run.  One JSON line per
measurement.
usage: bench_moments_head.py [--batch 256] [--samples 20,32,100] [--iters N] [--windows W] [--what samples --package PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--samples", default="20,32,100")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--what", choices=["moments", "samples", "launches"])
ap.add_argument("--mode", choices=["bf16", "f32"])
ap.add_argument("--step-timeout", type=int, default=150)
ap.add_argument("--package", default=None)
args = ap.parse_args()
if args.package and args.what != "samples":
    sys.exit("bench_moments_head: --package times the sampler of another checkout: give --what samples and a --mode")

sys.path.insert(0, os.path.abspath(args.package) if args.package else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if args.what is None:
    for what in ("moments", "samples", "launches"):
        for mode in ("bf16", "f32"):
            cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--mode", mode, "--batch", str(args.batch),
                   "--samples", args.samples, "--iters", str(args.iters), "--windows", str(args.windows)]
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            if rc != 0:
                sys.exit("bench_moments_head: %s / %s ended with status %d; nothing more is started" % (what, mode, rc))
    sys.exit(0)

import torch

import bayesianneuralnetworks_amd as bnn
from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd._rng import DrawKey, generator_for
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, MultivariateNormalLinear, NormalConv2d

assert args.windows >= 5
dev = torch.device("cuda:0")
B = args.batch
SAMPLES = [int(s) for s in args.samples.split(",")]


class Flatten(torch.nn.Module):
    def forward(self, x):
        return x.view(x.size(0), -1)


class Net(BayesianNetworkModule):
    """examples/CIFAR10/model.py's layer sequence."""

    def __init__(self):
        super().__init__(3, 10, samples=SAMPLES[0])
        c2, elu = torch.nn.Conv2d, torch.nn.ELU
        self.layers = torch.nn.Sequential(
            c2(3, 64, 5, padding=2, stride=2), torch.nn.BatchNorm2d(64), elu(), c2(64, 128, 5, padding=2, stride=2), elu(),
            c2(128, 128, 5, padding=2, stride=2), elu(), c2(128, 128, 3, padding=1), elu(), c2(128, 128, 3, padding=1), elu(),
            NormalConv2d(128, 128, 3, padding=1), elu(), Flatten(), torch.nn.Linear(2048, 128), elu(),
            MultivariateNormalLinear(128, 10), torch.nn.Softmax(dim=-1))

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
    if args.package:
        assert os.path.abspath(bnn.__file__).startswith(os.path.abspath(args.package) + os.sep)      # that checkout's package ran
        row["package"] = args.package
    row.update({"mode": args.mode, "B": B, "ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)})
    print(json.dumps(row), flush=True)


torch.manual_seed(0)
bnn.set_compute(args.mode)
net = Net().to(dev).eval()
x = torch.randn(B, 3, 32, 32, device=dev)

if args.what == "moments":
    bnn.nn.moment_activations(net)
    with torch.no_grad():
        for cov in (False, True):
            for S in SAMPLES:
                report({"what": "predictive_uncertainty(propagation='moments')", "covariance": cov, "S": S},
                       timed(lambda: net.predictive_uncertainty(x, S, inputs="probs", propagation="moments", covariance=cov)))
            report({"what": "predictive_moments", "covariance": cov, "S": 0}, timed(lambda: net.predictive_moments(x, covariance=cov)))
elif args.what == "samples":
    bnn.nn.keyed_mvn_draws(True)
    net.mc_batched = True
    with torch.no_grad():
        for S in SAMPLES:
            report({"what": "predictive_uncertainty (MC-batched samples, keyed MVN draws)", "S": S},
                   timed(lambda: net.predictive_uncertainty(x, S, inputs="probs")))
else:
    head = net.layers[16]
    post = [t.detach() for t in (head.weight.mean, head.weight.scale, head.bias.mean, head.bias.scale)]
    O, K = post[0].shape
    a_m, a_v = torch.randn(B, K, device=dev), 0.1 * torch.rand(B, K, device=dev)
    report({"what": "bnn_mvn_moments_prepare", "O": O, "K": K}, timed(lambda: ops.mvn_moments_prepare(*post)))
    prepared = ops.mvn_moments_prepare(*post)
    report({"what": "bnn_mvn_moments_forward", "O": O, "K": K},
           timed(lambda: ops.moments_mvn_linear(ops.Moments(a_m, a_v), *post, prepared=prepared)))
    mom = ops.moments_mvn_linear(ops.Moments(a_m, a_v), *post, prepared=prepared)
    ho = ops.HeadOperands(a_v, prepared[0], prepared[3])
    report({"what": "bnn_moments_head_cov", "N": O, "K": K}, timed(lambda: ops.moments_head_cov(ho, mom.var)))
    full = ops.Moments(mom.mean, mom.var, cov=ops.moments_head_cov(ho, mom.var))
    for S in SAMPLES:
        key = DrawKey(1, 7, 0, S, 0, gen=generator_for(args.mode))
        report({"what": "bnn_moments_sample", "S": S}, timed(lambda: ops.moments_sample(mom, key, S)))
        report({"what": "bnn_moments_sample_cov", "S": S}, timed(lambda: ops.moments_sample(full, key, S)))
_lib.check_device(dev)
