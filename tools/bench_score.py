"""Device-event timing of bnn_mc_score (K14) against bnn_mc_uncertainty (K4) at K4's three shapes (GPU box):
  (S=8, rows=512, C=10)             the BASELINE step's tail, plain and as 16 x 8 fused-head partial logits;
  (S=32, rows=4096, C=1000) fp32    524 MB read: the bandwidth shape.
score: the per-row launch alone; score_state: with the accumulator (the second one-workgroup launch).  --k4-lib: another build
of the library (the parent commit's) to take bnn_mc_uncertainty from.  Every shape is warmed up before any is timed; the figure
is the median of --reps windows of back-to-back calls between two device events, the entries' windows alternating."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bayesianneuralnetworks_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--k4-lib", default=None)
args = ap.parse_args()

lib = _lib.load()
k4 = lib
if args.k4_lib:
    k4 = ctypes.CDLL(args.k4_lib)
    res, argtypes = _lib.SIGNATURES["bnn_mc_uncertainty"]
    k4.bnn_mc_uncertainty.restype, k4.bnn_mc_uncertainty.argtypes = res, argtypes
dev = torch.device("cuda:0")
st = _lib.stream_ptr(dev)
P = _lib.ptr


def case(name, parts, S, rows, C):
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.randn(parts, S, rows, C, device=dev, generator=g) * 3.0
    t = torch.randint(0, C, (rows,), device=dev, generator=g)
    n = rows * C
    outs = [torch.empty(rows, C, device=dev)] + [torch.empty(rows, device=dev) for _ in range(3)]
    mean = torch.empty(rows, C, device=dev)
    rowf = [torch.empty(rows, device=dev) for _ in range(5)]
    pred = torch.empty(rows, dtype=torch.int64, device=dev)
    state = torch.zeros(lib.bnn_mc_score_state_doubles(15, 20), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.bnn_mc_score_workspace_bytes(rows) // 4, device=dev)

    def unc():
        _lib.check(k4.bnn_mc_uncertainty(P(y), n, parts, S, rows, C, _lib.UNC_LOGITS, *[P(o) for o in outs], None, 0,
                                         None, 0, 1.0, None, None, st), "bnn_mc_uncertainty")

    def score(sp=None, wp=None):
        _lib.check(lib.bnn_mc_score(P(y), n, parts, S, rows, C, _lib.UNC_LOGITS, P(t), P(mean), P(rowf[0]), P(rowf[1]), P(rowf[2]),
                                    P(rowf[3]), P(pred), P(rowf[4]), sp, 15, 20, wp, None, 0, st), "bnn_mc_score")

    return dict(name=name, parts=parts, S=S, rows=rows, C=C, bytes=y.numel() * 4,
                fns=dict(uncertainty=unc, score=score, score_state=lambda: score(P(state), P(ws))))


def window(fn, iters):
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
    times = {k: [] for k in c["fns"]}
    for _ in range(args.reps):
        for k, fn in c["fns"].items():
            times[k].append(window(fn, iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {k: v for k, v in c.items() if k != "fns"}
    out.update({"%s_us" % k: round(v, 2) for k, v in med.items()})
    out.update({"%s_spread_us" % k: round(max(v) - min(v), 2) for k, v in times.items()})
    out.update({"%s_TBps" % k: round(c["bytes"] / v / 1e6, 3) for k, v in med.items()})
    out["score_over_uncertainty"] = round(med["score"] / med["uncertainty"], 3)
    out["score_state_over_uncertainty"] = round(med["score_state"] / med["uncertainty"], 3)
    print(json.dumps(out))
_lib.check_device(dev)
