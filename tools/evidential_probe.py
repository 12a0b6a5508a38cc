"""Device-event timing of the evidential family (K13) with ops.EVIDENTIAL_HIP on and off, on the same tensors (GPU box).  Off is
the torch-op chain of the reference on the device -- what the layers ran before K13 -- and is the baseline.
  step:  one training step of examples/Simple's network (1-100-100-100-NIG(1), batch 128, Adam 5e-4): zero_grad, forward,
         NormalInverseGaussianLoss, backward, optimizer step;
  loss:  NormalInverseGaussianLoss forward + backward on head outputs of (65536, 4), and of (1048576, 4), where the device's
         time and not the host's per-call cost decides (the fp64 evaluation of every element shows there);
  head:  NormalInverseGaussianLinear's activation forward + backward on z (rows, 16) (D = 4) at the same two row counts, the
         Linear left out.
Every case is warmed up in both modes before any is timed; the two modes alternate window by window; a figure is the median over
--windows timed windows of --iters back-to-back calls.  Launches are counted per call: `launches_hip` = launches of this library
(bnn_launch_count), `torch_ops` = aten operators torch ran on the device beside them (views and allocations left out; one kernel
each for the pointwise and reduction operators of these chains)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from bayesianneuralnetworks_amd import _lib, ops
from bayesianneuralnetworks_amd.nn import BayesianNetworkModule, NormalInverseGaussianLinear, NormalInverseGaussianLoss

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--windows", type=int, default=25)
args = ap.parse_args()

dev = torch.device("cuda:0")
lib = _lib.load()


class Simple(BayesianNetworkModule):
    def __init__(self):
        super().__init__(1, 1, samples=1)
        L, R = torch.nn.Linear, torch.nn.ReLU
        self.layers = torch.nn.Sequential(L(1, 100), R(), L(100, 100), R(), L(100, 100), R(), NormalInverseGaussianLinear(100, 1))

    def _forward(self, x):
        return self.layers(x)


def step_case():
    torch.manual_seed(0)
    net = Simple().to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    crit = NormalInverseGaussianLoss()
    x = torch.linspace(-4, 4, 128, device=dev).unsqueeze(1)
    y = x ** 3 + 3.0 * torch.randn(128, 1, device=dev)

    def fn():
        opt.zero_grad()
        crit(*net(x), y).backward()
        opt.step()

    return fn


def loss_case(rows=65536, D=4):
    g = torch.Generator(device=dev).manual_seed(1)
    r = lambda: torch.rand(rows, D, device=dev, generator=g)          # noqa: E731
    leaves = [torch.randn(rows, D, device=dev, generator=g), 0.05 + 3.95 * r(), 1.0 + 0.001 + 50 * r(), 0.05 + 3.95 * r()]
    leaves = [t.requires_grad_() for t in leaves]
    y = torch.randn(rows, D, device=dev, generator=g)
    crit = NormalInverseGaussianLoss()

    def fn():
        for t in leaves:
            t.grad = None
        crit(*leaves, y).backward()

    return fn


def head_case(rows=65536, D=4):
    g = torch.Generator(device=dev).manual_seed(2)
    head = NormalInverseGaussianLinear(4 * D, D).to(dev)
    z = (torch.randn(rows, 4 * D, device=dev, generator=g) * 3).requires_grad_()
    ups = [torch.randn(rows, D, device=dev, generator=g) for _ in range(4)]
    sp = torch.nn.functional.softplus

    def fn():
        z.grad = None
        if ops.EVIDENTIAL_HIP:
            outs = ops.nig_head(z, D)
        else:                                   # NormalInverseGaussianLinear.forward behind its Linear
            ga, u, a, b = torch.split(z, head.out_channels, dim=-1)
            outs = (ga, 1e-10 + sp(u), 1 + 1e-10 + sp(a), 1e-10 + sp(b))
        torch.autograd.backward(outs, ups)

    return fn


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


_VIEWS = ("split", "view", "detach", "alias", "expand", "as_strided", "unsqueeze", "squeeze", "select", "slice", "t.default",
          "transpose", "permute", "_unsafe_view", "reshape", "unbind", "empty", "zeros", "ones", "is_same_size", "stride", "size")


class _CountOps(TorchDispatchMode):
    """aten operators reaching the device backend (below autograd, so the backward's own too); views and allocations left out.
    Each is one kernel for the pointwise and reduction ops counted here (addmm / mm: one library GEMM)."""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.__name__ if hasattr(func, "__name__") else str(func)
        if not any(name.startswith(v) or ("." + v) in name for v in _VIEWS):
            self.n += 1
        return func(*args, **(kwargs or {}))


def launches(fn):
    """(launches of this library, aten operators torch ran on the device) of one call"""
    torch.cuda.synchronize()
    n0 = lib.bnn_launch_count()
    with _CountOps() as c:
        fn()
    torch.cuda.synchronize()
    return lib.bnn_launch_count() - n0, c.n


cases = {"step_simple_b128": step_case(), "loss_65536x4": loss_case(), "head_65536x4": head_case(),
         "loss_1048576x4": loss_case(1 << 20), "head_1048576x4": head_case(1 << 20)}
for fn in cases.values():                       # warm every case in both modes (code objects, caches, clocks) before timing any
    for on in (True, False):
        ops.EVIDENTIAL_HIP = on
        for _ in range(20):
            fn()
torch.cuda.synchronize()
for name, fn in cases.items():
    us = {True: [], False: []}
    for _ in range(args.windows):
        for on in (True, False):                # alternate the two modes window by window
            ops.EVIDENTIAL_HIP = on
            us[on].append(window(fn, args.iters))
    out = {"case": name, "iters": args.iters, "windows": args.windows}
    for on, key in ((True, "hip"), (False, "torch_ops")):
        ops.EVIDENTIAL_HIP = on
        v = sorted(us[on])
        out[key + "_us"] = round(statistics.median(v), 2)
        out[key + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
        out[key + "_launches_hip"], out[key + "_torch_ops"] = launches(fn)
    out["speedup"] = round(out["torch_ops_us"] / out["hip_us"], 2)
    print(json.dumps(out), flush=True)
ops.EVIDENTIAL_HIP = True
_lib.check_device(dev)
