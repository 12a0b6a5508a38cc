"""A float64 reference for chains of bf16 contractions that knows where bf16 rounding is ambiguous.

A bf16 layer chain on the device contracts bf16 operands (bf16 x bf16 products are exact in fp32) with fp32 accumulation, adds
an fp32 bias, and rounds the hidden activation to bf16 with round-to-nearest-even.  The float64 result `t` of the same bf16
operands differs from the device's fp32 result by at most

    b = gamma_{K+1} (sum_k |x_k| |w_k| + |bias|),   gamma_n = n u / (1 - n u),  u = 2^-24,

whatever the summation order (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5).  A hidden value
whose interval [t - b - slack, t + b + slack] holds a bf16 rounding midpoint may round either way on the device: it is
AMBIGUOUS, and its possible deviation from the reference's rounding (one bf16 ulp, or more where the interval holds several
midpoints) is carried into the next layer as slack: sum_j dev_j |w_ij|.  Everywhere else the reference's rounding IS the
device's rounding, and the bound is the accumulation bound alone.

The hidden value is rounded to bf16 straight from float64 (not float64 -> fp32 -> bf16: that rounds twice).
"""
import torch

U32 = 2.0 ** -24


def gamma(n, u=U32):
    """gamma_n = n u / (1 - n u): the recursive-summation constant of n addends (any order)."""
    return n * u / (1.0 - n * u)


def rne_bf16(v):
    """float64 -> the nearest bf16 value (ties to even) as float64, in one rounding.  Normal range only (|v| >= 2^-126 or 0)."""
    v = v.double()
    m, e = torch.frexp(v)                        # v = m 2^e, 0.5 <= |m| < 1
    return torch.ldexp(torch.round(torch.ldexp(m, torch.full_like(e, 8))), e - 8)     # 8 significant bits; round(): half to even


def ulp_bf16(v):
    """The spacing of bf16 numbers at |v| (the ulp of the binade |v| lies in)."""
    _, e = torch.frexp(v.double())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def chain_layer(h, dev_h, w, b):
    """One contraction in float64: h (M, K) the reference's bf16 operand, dev_h (M, K) or None its per-element possible deviation
    on the device, w (N, K) the exact bf16 weight, b (N,) the fp32 bias or None.
    -> (t, acc, slack, a): the exact result, the device's accumulation bound, the slack the deviations of h carry, and
    sum |h| |w| + |b| (all (M, N) float64)."""
    wa = w.abs()
    t = h @ w.t()
    a = h.abs() @ wa.t()
    slack = torch.zeros_like(t) if dev_h is None else dev_h @ wa.t()
    if b is not None:
        t = t + b
        a = a + b.abs()
    K = w.shape[1]
    # the device sums K + 1 addends of |h + dev| |w| <= the reference's a plus the slack; float64's own error rides along
    acc = gamma(K + 1) * (a + slack) + gamma(K + 1, 2.0 ** -53) * a
    return t, acc, slack, a


def rounding_interval(t, beta, act=None):
    """(lo, hi): the smallest and largest bf16 value the device may store for exact hidden values t whose device value before the
    rounding lies in [t - beta, t + beta] (act: a monotone activation applied before the rounding -- ReLU, or None)."""
    f = (lambda v: v) if act is None else act
    return rne_bf16(f(t - beta)), rne_bf16(f(t + beta))


def relu(v):
    return v.clamp_min(0)


def round_hidden(t, beta, act=None):
    """Round the hidden values t (exact) to bf16 as the device may: the device's value before rounding lies in [t - beta, t + beta];
    act (a monotone activation applied before the rounding: ReLU, or None) and RNE are monotone, so the device's bf16 value lies
    between the roundings of the interval's ends.  -> (h, dev, ambiguous): the reference's rounding of t, the largest possible
    deviation from it (0 where unambiguous), the elements whose interval holds a rounding midpoint."""
    h = rne_bf16(t if act is None else act(t))
    lo, hi = rounding_interval(t, beta, act)
    ambiguous = lo != hi
    dev = torch.maximum((hi - h).abs(), (h - lo).abs())
    return h, dev, ambiguous


def bf16_chain_ref64(x, layers, relu=True):
    """float64 reference of a chain of bf16 dense layers with a per-element bound on the device's deviation from it.

    x: (M, K0) float64, the bf16 input operand's values; layers: [(w (N, K) float64 holding bf16 values, b (N,) float64 holding
    fp32 values, or None)]; every layer but the last applies ReLU (relu=True) and rounds to bf16; the last stays fp32.
    -> dict: out (M, N) the reference; bound (M, N) the bound on |device - out| (acc + slack); acc the last layer's accumulation
    bound; slack what ambiguous hidden values carry into it (0 where no hidden input is ambiguous); a the last layer's
    sum |h| |w| + |b|; ambiguous [per hidden layer (M, N) bool]."""
    act = globals()["relu"] if relu else None
    h, dev = x.double(), None
    amb = []
    for w, b in layers[:-1]:
        t, acc, slack, _ = chain_layer(h, dev, w.double(), None if b is None else b.double())
        h, dev, ambiguous = round_hidden(t, acc + slack, act)
        amb.append(ambiguous)
    w, b = layers[-1]
    t, acc, slack, a = chain_layer(h, dev, w.double(), None if b is None else b.double())
    return {"out": t, "bound": acc + slack, "acc": acc, "slack": slack, "a": a, "ambiguous": amb}
