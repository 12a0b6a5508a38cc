"""A float64 backward of ONE sampled linear layer, y_s = x_s W_s^T + b_s with W_s = mu + sigma(rho) eps_s, on the operands the
device consumed (teacher forcing), with a derived per-element bound on what the HIP kernels may return instead.

Operands (a dict, every tensor on the CPU; values are whatever the device stored, converted to float64):
  x      (S, M, K), or (1, M, K) for an input all samples share          the layer's saved input (fp32 or bf16 values)
  g      (S, M, N)   the gradient that reached the layer's output        (fp32 or bf16 values)
  y      (S, M, N) or None   the layer's stored output, when its ReLU is fused into the epilogue
  mu_w, rho_w (N, K);  mu_b, rho_b (N,) or None
  eps_w  (S, N, K), eps_b (S, N)   the draws' eps (ops.eps_philox on the layer's DrawKeys)
  w32, wbf (S, N, K)   the drawn weights in fp32 and rounded to bf16 (ops._sample_affine_philox_raw); only what spec["gx"] reads
  kl     None, or dict(up, T, n_batches, prior_w, prior_b): the upstream scalar of the KL term, the number of posterior tensors in
         it, its number_of_batches and the (mu, sigma) priors -- KLDivergence's gradient is  up / (n T n_batches) d KL_sum
  spec   dict(wgrad="bf16" | "f32" | "narrow",  bias_bf16=bool,  gx=None | "narrow" | "drawn" | "redraw_bf16" | "redraw_f32" | "plain",
              gx_bf16=bool): which kernels ran (the test derives it from the dispatch conditions of the host functions)

Rounding points, with where they come from (csrc/bnn_linear_bwd.hip unless said otherwise):
  fused ReLU      gy = g (y > 0) on the stored y, bits of g passed through: k_relu_bwd / k_relu_bwd_bf16x8.  Exact.
  wgrad "bf16"    k_wgrad_bf16<XBF, GBF> / k_wgrad_bf16_dma8: an fp32 operand is rounded to bf16, nearest-even, on load
                  (load8_bf16<false>: pack_bf16x2); bf16 x bf16 products are exact in fp32; v_mfma_f32_16x16x32_bf16 accumulates
                  the M rows of a sample in fp32.  wgrad_sample_end: gmu += acc, grho = fma(acc, eps_s, grho) per sample.
                  wgrad_store (nsplit = 1) or k_wgrad_reduce (the sample split): + the KL terms, then grho *= dsoftplus(rho).
  wgrad "f32"     k_wgrad_f32: the same with no operand rounding; products round once (v_mfma_f32_16x16x4_f32).
  wgrad "narrow"  k_head_bwd (N <= 16): x as stored (bf16 or fp32, widened exactly), gy fp32, fma chains over a thread's rows,
                  16 row partials, then per (sample, row slice) slab  t  and  t * eps_s  (one more rounding); k_head_tail adds the
                  slabs, the KL terms, and multiplies by dsoftplus(rho).  The weights of its gx are fma(sigma(rho), eps, mu) in
                  fp32 -- NOT rounded to bf16, although a bf16 forward contracted rounded ones -- and gx rounds once on store
                  when it is bf16 (pack_bf16x2).
  bias            fused in the wgrad kernels (nsplit = 1): column sums by one more MFMA on the B fragment -- so in a "bf16" kernel
                  the sums are over gy ROUNDED TO BF16 even when gy is stored as fp32 (spec["bias_bf16"]) -- then
                  wgrad_bias_sample_end / wgrad_bias_store: sum_s c_s, fma(c_s, eps_b,s, .), + KL, * dsoftplus(rho_b).
                  With the sample split: bnn_colsum on gy as stored, bnn_sample_affine_bwd, bnn_kl_backward(accumulate = 1).
                  Narrow: column sums of the fp32 gy in k_head_bwd, folded and finished by k_head_tail.
                  In every case the bias gradient IS the weight gradient of an input of ones with K = 1; it is computed so here.
  gx "drawn"      ops._dgrad_drawn_raw: bf16 gy times the bf16 weights the forward drew, fp32 accumulation over N
                  (bnn_dense_forward), stored as bf16.
  gx "redraw_*"   bnn_linear_backward_input_sampled (k_linear_sym, B_SAMPLED_T, csrc/bnn_linear.hip): bf16 compute rounds an fp32 gy
                  and the re-drawn W_s to bf16 and accumulates in fp32; fp32 compute rounds nothing.  Stored as bf16 or fp32
                  (a shared input's fp32 partial is rounded afterwards by the caller: the same single rounding).
  gx "plain"      k_dgrad_plain on fp32 weights drawn by bnn_sample_affine_philox: gy as stored, fma chain over N in fp32.
  KL terms        kl_grad_terms: c = up * fl(1 / (n T n_batches)); the counts are klref.kl_grad64's (test_train_tail.py).

Bound.  A sum of products whose every addend passes through at most d fp32 additions (any order, any tree; fma or exact
products; one extra rounding per product where products are rounded) differs from the exact sum by at most gamma_d sum |a| |b|
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1 / 4.2).  With A_s = |gy_s|^T |x_s|:
  g_mu :  d = M + S + 3 covers the M rows, the S samples (split or not), the product rounding and the KL addend:
          gamma_d (sum_s A_s + |kl_mu|) + 8 u |kl_mu|                                              (8 u: kl_grad64's count)
  g_rho:  P = sum_s dW_s eps_s is bounded the same way with the addends A_s |eps_s| and one more rounding (the narrow kernel's
          t * eps): e_P = gamma_{d + 1} sum_s A_s |eps_s|.  dsoftplus(rho) errs by (6 + 2 |rho| w2) u relative
          (test_train_tail.py: 1 + E, the fast division, E = exp(-rho) with weight w2 = 1 - dsoftplus), the addition of the KL
          part and the final product round once each:
          ds e_P + (8 + 2 |rho| w2) u ds (|P| + e_P) + u |kl_rho| + bound_kl_rho
  gx   :  gamma_{N + 1} sum_n |gy| |W|, and a bf16 output as an interval (bf16ref.rounding_interval).
Every bound carries float64's own error (gamma with u = 2^-53 on the same sums) and the fp32 denormal floor 2^-126; nothing
else is added and no element is excluded.
"""
import numpy as np
import torch

from bf16ref import gamma, rne_bf16, rounding_interval, ulp_bf16
from klref import TINY, U, dsoftplus64, kl_grad64

U64 = 2.0 ** -53


def D(t):
    return None if t is None else torch.as_tensor(t).detach().double().cpu()


def relu_mask(g, y):
    """The fused ReLU's backward: g where the STORED y is positive, zero elsewhere."""
    return g if y is None else g * (y > 0)


def _kl(mu, rho, prior, kl):
    """-> (g_mu, g_rho, bound_mu, bound_rho) of the KL term for one tensor as float64 torch tensors; zeros without a KL."""
    if kl is None:
        z = torch.zeros_like(mu)
        return z, z, z, z
    out = kl_grad64(mu.numpy(), rho.numpy(), prior, kl["T"], kl["n_batches"], kl["up"])
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).reshape(mu.shape) for a in out)


def wgrad64(x, gy, mu, rho, eps, prior, kl, round_ops):
    """g_mu, g_rho of one posterior tensor (N, K) -> {"g_mu": (ref, bound), "g_rho": (ref, bound)}.
    x (S | 1, M, K), gy (S, M, N), eps (S, N, K); round_ops: the kernel rounds its operands to bf16."""
    S, M, _ = gy.shape
    if round_ops:
        x, gy = rne_bf16(x), rne_bf16(gy)
    x = x.expand(S, -1, -1)
    dW = gy.transpose(1, 2) @ x                                    # (S, N, K)
    A = gy.abs().transpose(1, 2) @ x.abs()
    km, kr, bkm, bkr = _kl(mu, rho, prior, kl)
    d = M + S + 3
    g_mu = dW.sum(0) + km
    a_mu = A.sum(0) + km.abs()
    b_mu = gamma(d) * a_mu + bkm + gamma(d, U64) * a_mu + TINY
    ds = torch.from_numpy(np.ascontiguousarray(dsoftplus64(rho.numpy()))).reshape(rho.shape)
    w2 = torch.where(rho > 20.0, torch.zeros_like(ds), 1.0 - ds)
    P = (dW * eps).sum(0)
    T = (A * eps.abs()).sum(0)
    e_P = gamma(d + 1) * T
    g_rho = P * ds + kr
    b_rho = ds * e_P + (8.0 + 2.0 * rho.abs() * w2) * U * ds * (P.abs() + e_P) + U * kr.abs() + bkr + gamma(d + 1, U64) * T * ds + TINY
    return {"g_mu": (g_mu, b_mu), "g_rho": (g_rho, b_rho)}


def dgrad64(gy, w, round_gy):
    """gx[s] = gy[s] @ w[s] -> (ref, bound before the output's own rounding).  gy (S, M, N), w (S, N, K)."""
    if round_gy:
        gy = rne_bf16(gy)
    N = gy.shape[2]
    a = gy.abs() @ w.abs()
    return gy @ w, gamma(N + 1) * a + gamma(N + 1, U64) * a + TINY


def layer_backward(op):
    """-> {tensor name: (ref, bound, is_bf16)} for g_mu_w, g_rho_w, (g_mu_b, g_rho_b), (gx) of one layer; see the module docstring."""
    spec, kl = op["spec"], op.get("kl")
    x, g, y = D(op["x"]), D(op["g"]), D(op.get("y"))
    mu_w, rho_w = D(op["mu_w"]), D(op["rho_w"])
    gy = relu_mask(g, y)
    S, M, N = gy.shape
    out = {}
    rw = spec["wgrad"] == "bf16"
    r = wgrad64(x, gy, mu_w, rho_w, D(op["eps_w"]), kl["prior_w"] if kl else None, kl, rw)
    out["g_mu_w"], out["g_rho_w"] = r["g_mu"] + (False,), r["g_rho"] + (False,)
    if op.get("mu_b") is not None:
        ones = torch.ones(1, M, 1, dtype=torch.float64)
        r = wgrad64(ones, gy, D(op["mu_b"]).reshape(N, 1), D(op["rho_b"]).reshape(N, 1), D(op["eps_b"]).reshape(S, N, 1),
                    kl["prior_b"] if kl else None, kl, spec["bias_bf16"])
        out["g_mu_b"] = (r["g_mu"][0].reshape(N), r["g_mu"][1].reshape(N), False)
        out["g_rho_b"] = (r["g_rho"][0].reshape(N), r["g_rho"][1].reshape(N), False)
    how = spec.get("gx")
    if how is not None:
        w = D(op["w32"] if how in ("narrow", "redraw_f32", "plain") else op["wbf"])
        ref, b = dgrad64(gy, w, how == "redraw_bf16")
        out["gx"] = (ref, b, bool(spec["gx_bf16"]))
    return out


def compare(got, ref, bound, is_bf16):
    """-> (bad, ratio): the elements of `got` the bound rejects, and |got - ref| relative to the bound (for a bf16 output: to the
    bound plus the half ulp its own rounding may add -- reported only; `bad` is decided by the interval)."""
    got = D(got).reshape(ref.shape)
    err = (got - ref).abs()
    if is_bf16:
        lo, hi = rounding_interval(ref, bound)
        bad = ~((got >= lo) & (got <= hi))
        ratio = err / (bound + 0.5 * ulp_bf16(torch.maximum(ref.abs(), torch.full_like(ref, TINY))))
    else:
        bad = ~(err <= bound)
        ratio = err / bound
    return bad, ratio


def check(got, expected, what=""):
    """Hold the device's tensors `got` {name: tensor} to layer_backward's result -> {name: worst ratio}; raises AssertionError
    naming the tensor, the worst element, its error and its bound."""
    worst, fails = {}, []
    for name, (ref, bound, is_bf16) in expected.items():
        bad, ratio = compare(got[name], ref, bound, is_bf16)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        worst[name] = float(ratio.max())
        if bool(bad.any()):
            g = D(got[name]).reshape(ref.shape)
            score = torch.where(bad, ratio, torch.full_like(ratio, -1.0))
            i = int(torch.argmax(score))
            idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
            fails.append("%s %s: %d of %d elements outside the bound; worst at %s: got %.9g, ref %.9g, |err| %.3e, bound %.3e%s"
                         % (what, name, int(bad.sum()), bad.numel(), idx, float(g.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                            float((g - ref).abs().reshape(-1)[i]), float(bound.reshape(-1)[i]),
                            " (bf16 output: interval check)" if is_bf16 else ""))
    assert not fails, "\n".join(fails)
    return worst
