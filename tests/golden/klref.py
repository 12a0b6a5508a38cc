"""float64 restatements of the softplus epilogue and of the closed-form KL gradient, with the per-operation error counts of the
device's fp32 evaluation (csrc/bnn_kl.hip:k_kl_backward and kl_grad_terms in csrc/bnn_linear_bwd.hip).  Shared by
tests/test_train_tail.py, whose docstring derives the counts, and tests/golden/bwdref.py."""
import numpy as np

U = 2.0 ** -24                   # one fp32 rounding is at most u relative
TINY = 2.0 ** -126               # below the smallest normal fp32 a value may lose bits or be flushed: an absolute floor


def softplus64(r):
    r = np.asarray(r, np.float64)
    return np.where(r > 20.0, r, np.log1p(np.exp(np.minimum(r, 20.0))))


def dsoftplus64(r):
    r = np.asarray(r, np.float64)
    return np.where(r > 20.0, 1.0, 1.0 / (1.0 + np.exp(-r)))


def kl_grad64(mu, rho, prior, n_tensors, n_batches, upstream):
    """float64 closed form -> g_mu, g_rho, and the bounds on both.  The prior goes through np.float32 (bnn_kl_tensor_t)."""
    mu, rho = np.asarray(mu, np.float64), np.asarray(rho, np.float64)
    pm, ps = float(np.float32(prior[0])), float(np.float32(prior[1]))
    sg = 1e-10 + softplus64(rho)
    ds = dsoftplus64(rho)
    sc = float(upstream) / (mu.size * n_tensors * float(n_batches))
    g_mu = sc * (mu - pm) / ps ** 2
    g_rho = sc * (sg / ps ** 2 - 1.0 / sg) * ds
    rc = np.minimum(rho, 20.0)
    e = np.exp(rc)
    w = np.where(rho > 20.0, 0.0, e / ((1.0 + e) * np.log1p(e)))
    w2 = np.where(rho > 20.0, 0.0, 1.0 - dsoftplus64(rc))
    c = 28.0 + 2.0 * np.abs(rho) * (w + w2)
    # dsoftplus below 2^-126 (rho < -87.3) is flushed or loses bits in fp32 whatever computes it, and the factor in front of it
    # (1 / sigma = 1e10 for a collapsed posterior) scales that loss back into the normal range: TINY times the factor, there only
    mag = abs(sc) * (sg / ps ** 2 + 1.0 / sg)
    return g_mu, g_rho, 8.0 * U * np.abs(g_mu), c * U * mag * ds + np.where(ds < TINY, mag * TINY, 0.0)
