#!/usr/bin/env python3
"""Generate tests/golden/nig_evidential.npz by running the REAL reference's evidential family on CPU.

Run in the build container only (the reference does not exist on the GPU box):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_evidential.py

Like make_golden.py it imports pytorch_bayesian 0.0.4 (BNN_REFERENCE, default /root/reference; read-only), drives its own
NormalInverseGaussianLinear / NormalInverseGaussianLoss / NormalInverseGaussianUncertainty on seeded inputs and stores numbers
only.  The head's Linear is made the identity on a 12-wide input (weight = I, bias = 0), so that the layer's input IS the
pre-activation z and the recorded gradient is d loss / d z.  Everything is recorded twice: in float32 (keys *_f32) and in
float64 (*_f64, the layer cast with .double() on the same z and y)."""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("BNN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
import pytorch_bayesian  # noqa: E402
from pytorch_bayesian.nn import (NormalInverseGaussianLinear, NormalInverseGaussianLoss,  # noqa: E402
                                 NormalInverseGaussianUncertainty)

assert pytorch_bayesian.__version__ == "0.0.4"
OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(1)
torch.use_deterministic_algorithms(True)

ROWS, D, REG_LAMBDA = 37, 3, 1e-2


def run(z, y, dtype):
    head = NormalInverseGaussianLinear(4 * D, D).to(dtype)
    with torch.no_grad():
        head.linear.weight.copy_(torch.eye(4 * D, dtype=dtype))
        head.linear.bias.zero_()
    zz = z.detach().clone().to(dtype).requires_grad_()
    gamma, upsilon, alpha, beta = head(zz)
    loss = NormalInverseGaussianLoss(REG_LAMBDA)(gamma, upsilon, alpha, beta, y.to(dtype))
    loss.backward()
    ale, epi = NormalInverseGaussianUncertainty()(upsilon, alpha, beta)
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    sfx = "_f32" if dtype == torch.float32 else "_f64"
    out = {"gamma": gamma, "upsilon": upsilon, "alpha": alpha, "beta": beta, "loss": loss, "g_z": zz.grad,
           "aleatoric": ale, "epistemic": epi}
    return {k + sfx: v.detach().numpy().astype(np_dtype) for k, v in out.items()}


def main():
    gen = torch.Generator().manual_seed(20261018)
    z = torch.randn(ROWS, 4 * D, generator=gen) * 2.0
    # the softplus corners, one in each of the three softplus segments
    corners = torch.tensor([-30.0, -1e-3, 19.5, 20.0, 20.5, 60.0])
    z[0:6, D] = corners
    z[6:12, 2 * D + 1] = corners
    z[12:18, 3 * D + 2] = corners
    y = torch.randn(ROWS, D, generator=gen)
    rec = {"z": z.numpy().astype(np.float32), "y": y.numpy().astype(np.float32),
           "reg_lambda": np.float64(REG_LAMBDA), "D": np.int64(D)}
    rec.update(run(z, y, torch.float32))
    rec.update(run(z, y, torch.float64))
    path = os.path.join(OUT, "nig_evidential.npz")
    np.savez(path, **rec)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
