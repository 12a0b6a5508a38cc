"""Output bits of every extern "C" entry of csrc/bnn_conv3d.hip (the tile of csrc/bnn_conv3d_tile.hpp) as one line per case:
  entry mode geometry S shared sha256(all outputs' bytes)
K7 (bnn_conv3d_forward_drawn / _backward_input / _backward_weight), K9 (bnn_conv3d_flipout_*) and K11 (bnn_conv3d_lrt_*) with an
input shared by the S = 3 samples and with one per sample (K11's backward: one image set / S image sets), K17
(bnn_conv3d_moments_forward) with and without a_v x activation none / ReLU / ELU, K19 (bnn_conv3d_moments_backward_input /
_weight), each in both compute modes, on four geometries -- the smallest that reach an edge of the 128 x 64 x 32 tile each:
  a  B 2, C 3, 5 x 6 x 7, O 5, kernel (3, 2, 3), padding (1, 0, 1): K 54 (two k-tiles, the last ragged), M 350 (three m-tiles,
     the last ragged), P 175 (scalar epilogue), several weight-gradient slabs
  b  B 1, C 4, 4 x 4 x 8, O 140, groups 2, kernel (1, 3, 3), stride (1, 2, 2), padding (0, 1, 1): Ng 70 (two n-tiles, the last
     ragged), K 18 (one partial k-tile), P 32 and Pin 128 (vector epilogues), taps that no stride step reaches; not K9 (groups)
  c  B 3, C 2, 7 x 5 x 9, O 4, kernel (2, 2, 2), stride (2, 1, 1), padding (1, 1, 0), dilation (2, 1, 2): per-axis geometry,
     P 168 (vector), Pin 315 (scalar)
  d  B 4, C 70, 1 x 1 x 16, O 3, kernel (1, 1, 3), padding (0, 0, 1): the 1-d view, Cg 70 (two n-tiles in DGRAD), K 210 (two
     m-tiles in WGRAD)
Inputs are slices of ONE seeded pool generated on the CPU and copied over (abs, squares, signs and bf16 rounding on the device:
the same bits every run).  Two builds of the library computed the same bits iff their outputs are the same text:
tools/ab.sh python tools/conv3d_digest.py (GPU box; one process, a few seconds)."""
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bayesianneuralnetworks_amd import _lib, ops

dev = torch.device("cuda:0")
POOL = 1 << 20
pool = torch.from_numpy(np.random.RandomState(20261020).standard_normal(POOL).astype(np.float32)).to(dev)
S = 3
GEOMETRIES = (
    ("a", (2, 3, 5, 6, 7), (5, 3, 3, 2, 3), (1, 1, 1), (1, 0, 1), (1, 1, 1), 1),
    ("b", (1, 4, 4, 4, 8), (140, 2, 1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 1), 2),
    ("c", (3, 2, 7, 5, 9), (4, 2, 2, 2, 2), (2, 1, 1), (1, 1, 0), (2, 1, 2), 1),
    ("d", (4, 70, 1, 1, 16), (3, 70, 1, 1, 3), (1, 1, 1), (0, 0, 1), (1, 1, 1), 1),
)
salt = [0]


def take(*shape):
    """A contiguous fp32 tensor of `shape` out of the pool (another slice at every call)."""
    salt[0] += 1
    n = int(np.prod(shape))
    idx = (torch.arange(n, device=dev) * 2654435761 + salt[0] * 40503) % POOL
    return pool[idx].view(shape)


def digest(outs):
    h = hashlib.sha256()
    for t in outs:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


lib = _lib.load()
st = _lib.stream_ptr(dev)
P = _lib.ptr


def call(entry, *args):
    _lib.check(getattr(lib, entry)(*args), entry)


def line(entry, mode, geo, shared, outs):
    print(entry, mode, geo, S, shared, digest(outs), flush=True)


def workspace(nbytes):
    assert nbytes >= 0
    return torch.zeros(max(nbytes, 4), dtype=torch.uint8, device=dev), nbytes


for geo, xs, wsh, stride, padding, dilation, groups in GEOMETRIES:
    sh, out_sp = ops._conv3d_shape(xs, wsh, stride, padding, dilation, groups)
    shp = ctypes.byref(sh)
    B, C, O = xs[0], xs[1], wsh[0]
    K = int(np.prod(wsh[1:]))
    ys = (B, O) + tuple(out_sp)
    for mode, code in (("f32", _lib.COMPUTE_F32), ("bf16", _lib.COMPUTE_BF16)):
        bf = code == _lib.COMPUTE_BF16
        n = O * K
        ld = (n + 7) // 8 * 8 if bf else n                        # a weight row: bf16 padded to a multiple of 8
        wdt = torch.bfloat16 if bf else torch.float32
        w = torch.zeros((S, ld), dtype=wdt, device=dev)            # K7: one drawn weight row per sample
        w[:, :n] = (take(S, n) * 0.2).to(wdt)
        bias = take(S, O)
        mean, scale = take(n) * 0.2, take(n)                       # K9: [mean | stddev] rows, rho for the weight gradient
        wf = torch.zeros((2, ld), dtype=wdt, device=dev)
        wf[0, :n], wf[1, :n] = mean.to(wdt), (scale.abs() * 0.1).to(wdt)
        mu_w, rho_w = take(n) * 0.2, take(n) - 3.0                 # K11 / K17 / K19
        s2_w = (take(n) * 0.1).square()
        mu_b, s2_b, rho_b = take(O), take(O).square(), take(O) - 3.0
        rng = _lib.Rng(seed=20261020, stream=5)
        for shared in (1, 0):
            x = take(*xs) if shared else take(S, *xs)
            x_ss = 0 if shared else x[0].numel()
            gy = take(S, *ys)
            signs = torch.where(take(S, B, O + C) < 0, -1.0, 1.0)
            sg_ss = B * (O + C)

            y = torch.zeros((S,) + ys, device=dev)
            call("bnn_conv3d_forward_drawn", P(x), x_ss, P(w), ld, P(bias), O, P(y), shp, S, code, st)
            line("bnn_conv3d_forward_drawn", mode, geo, shared, [y])
            gx = torch.zeros_like(x)
            call("bnn_conv3d_backward_input", P(gy), P(w), ld, P(gx), shared, shp, S, code, st)
            line("bnn_conv3d_backward_input", mode, geo, shared, [gx])
            gw, gb = torch.zeros((S, O, K), device=dev), torch.zeros((S, O), device=dev)
            ws, nb = workspace(lib.bnn_conv3d_backward_weight_workspace_bytes(shp, S))
            call("bnn_conv3d_backward_weight", P(x), x_ss, P(gy), P(gw), P(gb), shp, S, code, P(ws), nb, st)
            line("bnn_conv3d_backward_weight", mode, geo, shared, [gw, gb])

            if groups == 1:
                y = torch.zeros((S,) + ys, device=dev)
                call("bnn_conv3d_flipout_forward", P(x), x_ss, P(wf), P(signs), sg_ss, P(y), shp, S, code, st)
                line("bnn_conv3d_flipout_forward", mode, geo, shared, [y])
                gx = torch.zeros_like(x)
                call("bnn_conv3d_flipout_backward_input", P(gy), P(wf), P(signs), sg_ss, P(gx), shared, shp, S, code, st)
                line("bnn_conv3d_flipout_backward_input", mode, geo, shared, [gx])
                g_mean, g_scale = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
                ws, nb = workspace(lib.bnn_conv3d_flipout_backward_weight_workspace_bytes(shp, S))
                call("bnn_conv3d_flipout_backward_weight", P(x), x_ss, P(gy), P(signs), sg_ss, P(scale), P(g_mean), P(g_scale), shp, S,
                     code, P(ws), nb, st)
                line("bnn_conv3d_flipout_backward_weight", mode, geo, shared, [g_mean, g_scale])

            y = torch.zeros((S,) + ys, device=dev)
            v = torch.zeros(ys if shared else (S,) + ys, device=dev)
            call("bnn_conv3d_lrt_forward", P(x), x_ss, P(mu_w), P(s2_w), P(mu_b), P(s2_b), P(y), P(v), shp, S, ctypes.byref(rng), code, st)
            line("bnn_conv3d_lrt_forward", mode, geo, shared, [y, v])
            nsets = 1 if shared else S                             # the backward's image sets
            g_m, g_v = take(nsets, *ys), take(nsets, *ys)
            gx = torch.zeros_like(x)
            call("bnn_conv3d_lrt_backward_input", P(g_m), P(g_v), P(mu_w), P(s2_w), P(x), P(gx), shp, nsets, code, st)
            line("bnn_conv3d_lrt_backward_input", mode, geo, shared, [gx])
            g_mu_w, g_rho_w = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            g_mu_b, g_rho_b = torch.zeros(O, device=dev), torch.zeros(O, device=dev)
            ws, nb = workspace(lib.bnn_conv3d_lrt_backward_weight_workspace_bytes(shp, nsets))
            call("bnn_conv3d_lrt_backward_weight", P(x), P(g_m), P(g_v), P(rho_w), P(g_mu_w), P(g_rho_w), P(rho_b), P(g_mu_b), P(g_rho_b),
                 shp, nsets, code, P(ws), nb, st)
            line("bnn_conv3d_lrt_backward_weight", mode, geo, shared, [g_mu_w, g_rho_w, g_mu_b, g_rho_b])

        # K17 / K19: no sample axis (the S and shared columns: 1 and whether a_v is absent)
        a_m, a_v = take(*xs), take(*xs).abs()
        for var in (a_v, None):
            for act, flags in (("none", 0), ("relu", _lib.FLAG_RELU), ("elu", _lib.FLAG_ELU)):
                out_m, out_v = torch.zeros(ys, device=dev), torch.zeros(ys, device=dev)
                call("bnn_conv3d_moments_forward", P(a_m), P(var), P(mu_w), P(s2_w), P(mu_b), P(s2_b), P(out_m), P(out_v), shp, code, flags,
                     1.0, st)
                print("bnn_conv3d_moments_forward:" + act, mode, geo, 1, int(var is None), digest([out_m, out_v]), flush=True)
        G_m, G_v = take(*ys), take(*ys)
        g_am, g_av = torch.zeros_like(a_m), torch.zeros_like(a_m)
        call("bnn_conv3d_moments_backward_input", P(G_m), P(G_v), P(mu_w), P(s2_w), P(a_m), P(g_am), P(g_av), shp, code, st)
        print("bnn_conv3d_moments_backward_input", mode, geo, 1, 0, digest([g_am, g_av]), flush=True)
        g_mu_w, g_rho_w = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        g_mu_b, g_rho_b = torch.zeros(O, device=dev), torch.zeros(O, device=dev)
        ws, nb = workspace(lib.bnn_conv3d_moments_wgrad_workspace(shp))
        call("bnn_conv3d_moments_backward_weight", P(a_m), P(a_v), P(G_m), P(G_v), P(mu_w), P(rho_w), P(g_mu_w), P(g_rho_w), P(rho_b),
             P(g_mu_b), P(g_rho_b), shp, code, P(ws), nb, st)
        print("bnn_conv3d_moments_backward_weight", mode, geo, 1, 0, digest([g_mu_w, g_rho_w, g_mu_b, g_rho_b]), flush=True)
torch.cuda.synchronize()
_lib.check_device(dev)
