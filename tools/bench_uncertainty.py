"""Device-event timing of bnn_mc_uncertainty against bnn_mc_sum (the predictive mean alone) at the same shapes (GPU box):
  (S=8, rows=512, C=10)             the BASELINE step's tail, plain and as 16 x 8 fused-head partial logits;
  (S=32, rows=4096, C=1000) fp32    524 MB read: the bandwidth shape (floor 524 MB / 8 TB/s = 66 us).
Every shape is warmed up before any is timed.  Launches go straight to the C-ABI on preallocated outputs."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bayesianneuralnetworks_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
args = ap.parse_args()

lib = _lib.load()
dev = torch.device("cuda:0")
st = _lib.stream_ptr(dev)
P = _lib.ptr


def case(name, parts, S, rows, C):
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.randn(parts, S, rows, C, device=dev, generator=g) * 3.0
    n = rows * C
    mean_sum = torch.empty(rows, C, device=dev)
    outs = [torch.empty(rows, C, device=dev)] + [torch.empty(rows, device=dev) for _ in range(3)]

    def mc_sum():               # ops.mc_mean: every (part, sample) addend in one launch
        _lib.check(lib.bnn_mc_sum(P(y), n, parts * S, n, 1.0 / S, P(mean_sum), 0, None, 0, st), "bnn_mc_sum")

    def unc():
        _lib.check(lib.bnn_mc_uncertainty(P(y), n, parts, S, rows, C, _lib.UNC_LOGITS, *[P(t) for t in outs], None, 0,
                                          None, 0, 1.0, None, None, st), "bnn_mc_uncertainty")
    return dict(name=name, parts=parts, S=S, rows=rows, C=C, bytes=y.numel() * 4, fns=dict(mc_sum=mc_sum, uncertainty=unc))


def timeit(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


cases = [case("baseline_tail", 1, 8, 512, 10), case("baseline_tail_head_partials", 16, 8, 512, 10),
         case("bandwidth", 1, 32, 4096, 1000)]
for c in cases:                                 # warm every shape (code objects, caches, clocks) before timing any
    for fn in c["fns"].values():
        for _ in range(20):
            fn()
torch.cuda.synchronize()
for c in cases:
    iters = args.iters if c["bytes"] < (64 << 20) else max(20, args.iters // 10)
    res = {k: timeit(fn, iters) for k, fn in c["fns"].items()}
    out = {k: v for k, v in c.items() if k != "fns"}
    out.update({"%s_us" % k: round(v, 2) for k, v in res.items()})
    out.update({"%s_TBps" % k: round(c["bytes"] / v / 1e6, 3) for k, v in res.items()})
    print(json.dumps(out))
_lib.check_device(dev)
