"""Output bits of the four one-launch MC tails (ops.mc_uncertainty, mc_score, mc_regression, mc_evidential) as one line per case:
  entry kind fused S rows width layout sha256(all outputs' bytes)
over the cross product of their dispatch branches at the smallest shapes that reach them: widths 2 .. 4096 (narrow, and every
(threads per row, chunks) of the wide split), rows 1 / 37, S 1 / 3 / 8 / 65, every kind, plain tensors, HeadPartials of 3 and 33
parts, and views one float off 16-B alignment (scalar loads / stores although width % 4 == 0); mc_score with and without a
ScoreState, whose doubles are hashed too.  Inputs are slices of ONE seeded pool generated on the CPU and copied over (gathers,
abs, products and softmax on the device: the same bits every run); probabilities are the softmax of the same logits.
Two builds of the library computed the same bits iff their outputs are the same text: tools/ab.sh python tools/mc_tail_digest.py
(GPU box; one process, a few seconds)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bayesianneuralnetworks_amd import _lib, ops

dev = torch.device("cuda:0")
POOL = 1 << 22
pool = torch.from_numpy((np.random.RandomState(20261019).standard_normal(POOL) * 3.0).astype(np.float32)).to(dev)

WIDTHS = (2, 10, 16, 17, 40, 300, 1000, 1028, 4096)
LAYOUTS = (("plain", 1, 0), ("offset", 1, 1), ("parts3", 3, 0), ("parts3-offset", 3, 1), ("parts33", 33, 0))


def take(shape, salt, off=0):
    """A contiguous fp32 tensor of `shape` out of the pool, `off` floats past a 16-B boundary."""
    n = int(np.prod(shape))
    idx = (torch.arange(n, device=dev) * 2654435761 + salt * 40503) % POOL
    buf = torch.empty(n + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[off:off + n]
    torch.index_select(pool, 0, idx, out=out)
    return out.view(shape)


def keep(t, off):
    """t's values in fresh storage `off` floats past a 16-B boundary (what an elementwise op on a view does not keep)."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
    out = buf[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def digest(outs):
    h = hashlib.sha256()
    for t in outs:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def line(entry, kind, parts, S, rows, width, layout, outs):
    print(entry, kind, int(parts > 1), S, rows, width, layout, digest(outs))


def wrap(y, parts):
    return ops.HeadPartials(y) if parts > 1 else y[0]


salt = 0
for width in WIDTHS:
    for rows in (1, 37):
        for S in (1, 3, 8, 65):
            target = (torch.arange(rows, device=dev) * 7 + S) % width
            if rows > 1:
                target[0] = -1                              # a row without a label: NaN scores, hashed like any value
            for layout, parts, off in LAYOUTS:
                salt += 1
                z = take((parts, S, rows, width), salt, off)
                p = keep(torch.softmax(z, -1) / parts, off)            # the parts of a sample add up to a distribution
                for kind, y in (("logits", z), ("probs", p)):
                    line("mc_uncertainty", kind, parts, S, rows, width, layout, ops.mc_uncertainty(wrap(y, parts), kind))
                    line("mc_score", kind, parts, S, rows, width, layout, ops.mc_score(wrap(y, parts), target, kind))
                    state = ops.ScoreState(dev)
                    outs = ops.mc_score(wrap(y, parts), target, kind, state=state)
                    line("mc_score", kind, parts, S, rows, width, layout + "+state", list(outs) + [state.state])
                line("mc_regression", "values", parts, S, rows, width, layout, ops.mc_regression(wrap(z, parts), "values"))
                if width % 2 == 0:
                    v = z.clone()
                    v[..., width // 2:] *= z[..., width // 2:]         # variances as given: squares
                    v = keep(v, off)
                    line("mc_regression", "mean_logvar", parts, S, rows, width, layout, ops.mc_regression(wrap(z, parts), "mean_logvar"))
                    line("mc_regression", "mean_var", parts, S, rows, width, layout, ops.mc_regression(wrap(v, parts), "mean_var"))
                if parts == 1:                              # the evidential tail takes no partials
                    g = z[0]
                    u = keep(take((S, rows, width), salt + 1000).abs() + 0.1, off)         # upsilon > 0
                    a = keep(take((S, rows, width), salt + 2000).abs() + 1.5, off)         # alpha > 1
                    b = keep(take((S, rows, width), salt + 3000).abs() + 0.1, off)
                    line("mc_evidential", "nig", 1, S, rows, width, layout, ops.mc_evidential(g, u, a, b))
torch.cuda.synchronize()
_lib.check_device(dev)
