"""Device-event timing of the regression tail against the torch sequences it replaces, on the same tensors (GPU box):
  ops.mc_regression(y, 'mean_logvar')      vs  exp, mean(0), var(0, unbiased=False), add;
  ops.gaussian_nll forward + backward      vs  torch.nn.functional.gaussian_nll_loss(m, t, exp(s)) with autograd
at (S=8, rows=512, width=20), a step's tail, and (S=32, rows=65536, width=2), the many-rows shape.
Every case is warmed up before any is timed; a figure is the median over --windows timed windows of --iters back-to-back calls."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bayesianneuralnetworks_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--windows", type=int, default=25)
args = ap.parse_args()

dev = torch.device("cuda:0")
HBM_TBPS = 8.0


def case(S, rows, width):
    g = torch.Generator(device=dev).manual_seed(1)
    D = width // 2
    y = torch.cat([torch.randn(S, rows, D, device=dev, generator=g), torch.rand(S, rows, D, device=dev, generator=g) * 7 - 4], -1)
    t = torch.randn(rows, D, device=dev, generator=g)
    yg = y.clone().requires_grad_()

    def hip_moments():
        return ops.mc_regression(y, "mean_logvar")

    def torch_moments():
        m, v = y[..., :D], torch.exp(y[..., D:])
        ale, epi = v.mean(0), m.var(0, unbiased=False)
        return m.mean(0), ale + epi, ale, epi

    def hip_nll():
        yg.grad = None
        ops.gaussian_nll(yg, t).backward()

    def torch_nll():
        yg.grad = None
        torch.nn.functional.gaussian_nll_loss(yg[..., :D], t, torch.exp(yg[..., D:])).backward()

    return dict(S=S, rows=rows, width=width, moments_bytes=y.numel() * 4 + 4 * rows * D * 4, nll_bytes=2 * y.numel() * 4 + t.numel() * 4,
                fns=dict(hip_moments=hip_moments, torch_moments=torch_moments, hip_nll=hip_nll, torch_nll=torch_nll))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


cases = [case(8, 512, 20), case(32, 65536, 2)]
for c in cases:                                 # warm every case (code objects, caches, clocks) before timing any
    for fn in c["fns"].values():
        for _ in range(20):
            fn()
torch.cuda.synchronize()
for c in cases:
    out = {k: v for k, v in c.items() if k != "fns"}
    for k, fn in c["fns"].items():
        us = sorted(window(fn, args.iters) for _ in range(args.windows))
        out[k + "_us"] = round(statistics.median(us), 2)
        out[k + "_us_min_max"] = [round(us[0], 2), round(us[-1], 2)]
    out["hip_moments_frac_of_hbm"] = round(c["moments_bytes"] / out["hip_moments_us"] / 1e6 / HBM_TBPS, 4)
    out["hip_nll_frac_of_hbm"] = round(c["nll_bytes"] / out["hip_nll_us"] / 1e6 / HBM_TBPS, 4)
    print(json.dumps(out))
_lib.check_device(dev)
