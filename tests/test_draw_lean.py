"""GPU: the lean instantiation of the draw launch (csrc/bnn_dense.hip, k_draw_multi LEAN) -- taken when every tensor of a
launch is a Philox-7 / u16 draw (or kind 1 / 2 / 3) with no taps, no Flipout and no three-plane output.  It must give the
general instantiation's bits: the BASELINE net's six tensors (flat weights with the KL first pass in their items, the
small-tensor spread of the head and the fp32 biases), on a device-epoch key, equal K1 bit for bit with zero padding; the
same launch with BNN_DRAW_LEAN=0 (the general instantiation, in a fresh process) writes the same bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [784, 1200, 1200, 10]
S = 8


def _draw_baseline(out_path):
    """Draws the BASELINE net's six tensors in ONE launch (KL carried) and saves every output as raw bytes."""
    import bayesianneuralnetworks_amd  # noqa: F401
    from bayesianneuralnetworks_amd import _lib, ops
    from bayesianneuralnetworks_amd._rng import DrawKey, GEN_PHILOX7_U16, default_generator
    dev = torch.device("cuda:0")
    lib = _lib.load()
    cell = default_generator.epoch_dev(dev)
    saved = cell.clone()
    cell[0] = 3                                     # the device epoch word the draw reads (restored below)
    layers, mus, rhos = [], [], []
    for i, (k, n) in enumerate(zip(DIMS[:-1], DIMS[1:])):
        gen = torch.Generator().manual_seed(40 + i)
        mw, rw, mb, rb = [t.to(dev) for t in seeded.posterior(gen, (n, k), True)]
        kw = DrawKey(0x1234_5678_9ABC, 2 * i + 1, 0, S, 5, epoch_dev_delta=1, gen=GEN_PHILOX7_U16)
        kb = DrawKey(0x1234_5678_9ABC, 2 * i + 2, 0, S, 5, epoch_dev_delta=1, gen=GEN_PHILOX7_U16)
        layers.append((mw, rw, mb, rb, kw, kb))
        mus += [mw, mb]
        rhos += [rw, rb]
    priors = [(0.0, 0.1)] * 6
    ref_kl = ops.kl_normal(mus, rhos, priors, 2.0)
    h = ops.kl_normal_begin(mus, rhos, priors, 2.0, carry=True)
    n0 = lib.bnn_launch_count()
    pre = ops.draw_layers(layers, S, kl=h)
    assert lib.bnn_launch_count() == n0 + 1 and h.launched
    ops._tls.kl_carry = None
    ops.mc_mean(torch.zeros(S, 8, device=dev), kl=h)
    torch.cuda.synchronize()
    assert torch.equal(h.out, ref_kl)
    blobs = {}
    for li, ((mw, rw, mb, rb, kw, kb), p_) in enumerate(zip(layers, pre)):
        K = mw.shape[1]
        assert torch.equal(p_.w[:, :, :K], ops._sample_affine_philox_raw(mw, rw, kw, out_dtype=torch.bfloat16))
        assert not p_.w[:, :, K:].any()
        assert torch.equal(p_.b, ops._sample_affine_philox_raw(mb, rb, kb))
        blobs[f"w{li}"] = p_.w.view(torch.int16).cpu().numpy()
        blobs[f"b{li}"] = p_.b.view(torch.int32).cpu().numpy()
    blobs["kl"] = h.out.view(torch.int32).cpu().numpy()
    cell.copy_(saved)
    if out_path:
        np.savez(out_path, **blobs)
    return blobs


def test_baseline_draw_lean_equals_k1_and_general(tmp_path):
    assert torch.cuda.is_available()
    lean = _draw_baseline(None)
    path = str(tmp_path / "general.npz")
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_draw_lean as t; t._draw_baseline(%r)"
            % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), path))
    env = dict(os.environ, BNN_DRAW_LEAN="0")
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=600, cwd=ROOT)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(lean)
        for k in z.files:
            assert np.array_equal(z[k], lean[k]), k
