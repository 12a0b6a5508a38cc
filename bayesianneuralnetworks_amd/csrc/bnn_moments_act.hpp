// bnn_moments_act.hpp -- moment-matched activations of a Gaussian pre-activation N(m, v): the device functions that the fused
// epilogues (k_moments, bnn_moments.hip; k_moments_conv3d, bnn_conv3d.hip) and the standalone elementwise launches
// (k_moments_relu, k_moments_elu) both call, so that fused and standalone agree bit for bit; and their backwards
// (k_moments_relu_bwd, k_moments_elu_bwd, bnn_moments_bwd.hip).  K20: the moment-matched maximum of two Gaussians, the step a
// max-pooling window is folded with, and its backward (k_moments_pool3d, k_moments_pool3d_bwd, bnn_moments_pool.hip).
#pragma once
#include "bnn_device.hpp"

namespace bnn {

// ReLU of a Gaussian pre-activation N(m, v) by moment matching, s = sqrt(v), alpha = m / s, Phi / phi the standard normal cdf / pdf:
//     mean' = s (alpha Phi + phi)
//     var'  = v (Phi + alpha^2 Phi Phi_c + alpha phi (Phi_c - Phi) - phi^2),   Phi_c = Phi(-alpha),   clamped at 0
// (E[y^2] - mean'^2 with m^2 never subtracted from m^2 + v).  Beyond |alpha| = 40 Phi_c and phi are zero in fp32 and the form is
// its own limit: the input passes (alpha > 0) or (0, 0) comes out; v == 0 (alpha infinite or 0 / 0) takes that branch too.
// The terms are one function (moments_relu_terms) that the forward and its backward (moments_relu_bwd_dev) both evaluate.
struct ReluTerms { float s, alpha, cdf, cdc, pdf, mean, r; };      // mean = mean', r = the bracket of var' (var' = max(v r, 0))

// false: the limit branch (|alpha| >= 40, v == 0, NaN), where only s and alpha are set
__device__ __forceinline__ bool moments_relu_terms(float m, float v, ReluTerms &t)
{
    t.s = sqrtf(v);
    t.alpha = m / t.s;
    if (!(fabsf(t.alpha) < 40.0f)) return false;
    t.cdf = 0.5f * erfcf(-0.70710678118654752f * t.alpha);
    t.cdc = 0.5f * erfcf(0.70710678118654752f * t.alpha);
    t.pdf = 0.39894228040143268f * expf(-0.5f * t.alpha * t.alpha);
    t.mean = t.s * (t.alpha * t.cdf + t.pdf);
    t.r = t.cdf + t.alpha * t.alpha * t.cdf * t.cdc + t.alpha * t.pdf * (t.cdc - t.cdf) - t.pdf * t.pdf;
    return true;
}

__device__ __forceinline__ void moments_relu_dev(float m, float v, float &om, float &ov)
{
    ReluTerms t;
    if (!moments_relu_terms(m, v, t)) {
        om = fmaxf(m, 0.0f);
        ov = m > 0.0f ? v : 0.0f;
        return;
    }
    om = t.mean;
    ov = fmaxf(v * t.r, 0.0f);
}

// Backward of moments_relu_dev (K18): (g_m, g_v) from the gradients (gm', gv') of its two outputs, on the forward's own terms:
//     d mean'/d m = Phi                    d mean'/d v = phi / (2 s)
//     d var'/d m  = 2 mean' Phi(-alpha)    d var'/d v  = Phi - mean' phi / s
// Where the forward clamped var' (v r < 0, decided on the forward's r) the gv' terms are absent.  The limit branch passes both
// gradients for m > 0 and nothing otherwise, which is also the convention at v == 0.
__device__ __forceinline__ void moments_relu_bwd_dev(float m, float v, float gom, float gov, float &gm, float &gv)
{
    ReluTerms t;
    if (!moments_relu_terms(m, v, t)) {
        gm = m > 0.0f ? gom : 0.0f;
        gv = m > 0.0f ? gov : 0.0f;
        return;
    }
    const float ps = t.pdf / t.s;
    if (v * t.r < 0.0f) gov = 0.0f;
    gm = gom * t.cdf + gov * (2.0f * t.mean * t.cdc);
    gv = gom * (0.5f * ps) + gov * (t.cdf - t.mean * ps);
}

// ELU (x > 0: x; else a (exp(x) - 1)) of a Gaussian pre-activation N(m, v) by moment matching.  The positive part is the ReLU's;
// the negative part g = (exp(x) - 1) [x <= 0] has N1 = E[g] = E_1 - Phi_c and N2 = E[g^2] = E_2 - 2 E_1 + Phi_c with
// E_k = E[exp(k x); x <= 0] = exp(k m + k^2 v / 2) Phi(-alpha - k s):
//     mean' = P1 + a N1,                                  P1 = s (alpha Phi + phi)
//     var'  = v r(alpha) + a^2 (N2 - N1^2) - 2 a P1 N1,   r the ReLU's bracket above,   clamped at 0
// -- the variance as the sum of the two parts' own variances and their (non-negative) cross term, so m^2 is never subtracted from
// m^2 + v.  What is left cancels in N2 and in N2 - N1^2, absolutely to a few ulp of a^2: in fp32 that is 1e-7 a^2 / v in units of
// v and useless for small v, so the function works in fp64 (the inputs and the two results are fp32) and the cancellation costs
// 1e-16 a^2 / v -- below fp32's own rounding of the result for every v >= 1e-9 a^2.
// Every Gaussian tail comes from ONE function, X_k = erfcx(|t_k| / sqrt 2) at t_k = alpha + k s, k = 0, 1, 2 (a rolled loop: one
// copy of its code), and g = exp(-alpha^2 / 2):  Phi(-t_k) exp(k m + k^2 v / 2) = g X_k / 2 for t_k >= 0, which neither overflows
// nor underflows before the answer does, and exp(k m + k^2 v / 2) - g X_k / 2 for t_k < 0, where the exponent
// k s (alpha + k s / 2) is below -k^2 v / 2 <= 0 and the difference loses at most one bit.
// v == 0 (and a NaN v) gives (elu(m), 0); large alpha passes the input; large negative alpha tends to
// (a (exp(m + v / 2) - 1), a^2 exp(2 m + v) (exp(v) - 1)), finite and non-negative.
__device__ __forceinline__ void moments_elu_dev(float mf, float vf, float a_elu, float &om, float &ov)
{
    const double m = (double)mf, v = (double)vf, a = (double)a_elu;
    if (!(vf > 0.0f)) {
        om = mf > 0.0f ? mf : (float)(a * expm1(m));
        ov = 0.0f;
        return;
    }
    const double s = sqrt(v), alpha = m / s;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;            // X_0, X_1, X_2 after the loop
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        x0 = x1;
        x1 = x2;
        x2 = erfcx(0.70710678118654752 * fabs(alpha + (double)k * s));
    }
    const double g = exp(-0.5 * alpha * alpha);
    const double h0 = 0.5 * g * x0, h1 = 0.5 * g * x1, h2 = 0.5 * g * x2;
    const double cdc = alpha >= 0.0 ? h0 : 1.0 - h0, cdf = alpha >= 0.0 ? 1.0 - h0 : h0;
    const double pdf = 0.39894228040143268 * g;
    const double e1 = alpha + s >= 0.0 ? h1 : exp(m + 0.5 * v) - h1;
    const double e2 = alpha + 2.0 * s >= 0.0 ? h2 : exp(2.0 * (m + v)) - h2;
    const double p1 = s * (alpha * cdf + pdf);
    const double r = cdf + alpha * alpha * cdf * cdc + alpha * pdf * (cdc - cdf) - pdf * pdf;
    const double n1 = e1 - cdc, n2 = e2 - 2.0 * e1 + cdc;
    om = (float)(p1 + a * n1);
    ov = (float)fmax(v * r + a * a * (n2 - n1 * n1) - 2.0 * a * p1 * n1, 0.0);
}

// Backward of moments_elu_dev (K19): (g_m, g_v) from the gradients (gm', gv') of its two outputs.  With d_m E f = E f' and
// d_v E f = E f'' / 2 for f = elu and f = elu^2 (f' jumps by 1 - a at 0, where x has the density phi / s):
//     d mean'/d m = Phi + a E_1                           d mean'/d v = (a E_1 + (1 - a) phi / s) / 2
//     d var'/d m  = 2 P1 + 2 a^2 (E_2 - E_1) - 2 mean' (Phi + a E_1)
//     d var'/d v  = Phi + a^2 (2 E_2 - E_1) - mean' (a E_1 + (1 - a) phi / s)
// (a = 0: moments_relu_bwd_dev's).  For large negative alpha d var'/d m tends to 2 a^2 (E_2 - E_1^2) through a cancellation of
// the forward's N2 - N1^2 kind: fp64, as the forward.  The forward keeps its own code (its bits and registers are pinned), so
// the terms are evaluated again here, through the same X_k = erfcx loop.  Where the forward clamped var' (decided on the
// forward's own sum) the gv' terms are absent.  v == 0 (and a NaN v) takes the limits, m == 0 on the positive side:
//     g_m = gm' elu'(m),   g_v = gv' elu'(m)^2 + gm' a exp(m) [m < 0] / 2
__device__ __forceinline__ void moments_elu_bwd_dev(float mf, float vf, float a_elu, float gom, float gov, float &gm, float &gv)
{
    const double m = (double)mf, v = (double)vf, a = (double)a_elu;
    if (!(vf > 0.0f)) {
        const double d = mf < 0.0f ? a * exp(m) : 1.0;
        gm = (float)((double)gom * d);
        gv = (float)((double)gov * d * d + (mf < 0.0f ? 0.5 * d * (double)gom : 0.0));
        return;
    }
    const double s = sqrt(v), alpha = m / s;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        x0 = x1;
        x1 = x2;
        x2 = erfcx(0.70710678118654752 * fabs(alpha + (double)k * s));
    }
    const double g = exp(-0.5 * alpha * alpha);
    const double h0 = 0.5 * g * x0, h1 = 0.5 * g * x1, h2 = 0.5 * g * x2;
    const double cdc = alpha >= 0.0 ? h0 : 1.0 - h0, cdf = alpha >= 0.0 ? 1.0 - h0 : h0;
    const double pdf = 0.39894228040143268 * g;
    const double e1 = alpha + s >= 0.0 ? h1 : exp(m + 0.5 * v) - h1;
    const double e2 = alpha + 2.0 * s >= 0.0 ? h2 : exp(2.0 * (m + v)) - h2;
    const double p1 = s * (alpha * cdf + pdf);
    const double r = cdf + alpha * alpha * cdf * cdc + alpha * pdf * (cdc - cdf) - pdf * pdf;
    const double n1 = e1 - cdc, n2 = e2 - 2.0 * e1 + cdc;
    const double mean = p1 + a * n1;
    const double go_v = v * r + a * a * (n2 - n1 * n1) - 2.0 * a * p1 * n1 < 0.0 ? 0.0 : (double)gov;
    const double dm = cdf + a * e1, dv = a * e1 + (1.0 - a) * pdf / s;
    gm = (float)((double)gom * dm + go_v * (2.0 * p1 + 2.0 * a * a * (e2 - e1) - 2.0 * mean * dm));
    gv = (float)((double)gom * (0.5 * dv) + go_v * (cdf + a * a * (2.0 * e2 - e1) - mean * dv));
}

// MC dropout behind a Gaussian pre-activation z ~ N(m, v), pushed through the activation f that follows in ONE step (K22):
// y = f(b z / q) with b ~ Bernoulli(q) independent of z, q = 1 - p, f(0) = 0 (the identity, ReLU, ELU), so y = b f(z / q).  With
// (M, V) the moments of f at the Gaussian N(m / q, v / q^2) -- moments_relu_dev / moments_elu_dev; the identity's are the input:
//     mean' = q M
//     var'  = q V + q p M^2
// (the mixture of the spike at 0 and f's distribution: both addends >= 0, E[y^2] - mean'^2 is never formed).  Exact for a Gaussian
// and for a deterministic z (v == 0, through the activations' own limit branches, which a NaN takes too).  act: 0, BNN_FLAG_RELU or
// BNN_FLAG_ELU -- a constant where the kernels call this.  The identity and the ReLU work in fp32; the ELU scales its input and
// recombines its results in fp64, as moments_elu_dev works inside.  p == 0 is the activation alone, its bits; p == 1 is (0, 0) and
// nothing is divided by q.
__device__ __forceinline__ void moments_act_dev(float m, float v, int act, float a_elu, float &om, float &ov)
{
    if (act == BNN_FLAG_RELU) moments_relu_dev(m, v, om, ov);
    else if (act == BNN_FLAG_ELU) moments_elu_dev(m, v, a_elu, om, ov);
    else { om = m; ov = v; }
}

__device__ __forceinline__ void moments_dropout_dev(float m, float v, float p, int act, float a_elu, float &om, float &ov)
{
    if (p == 0.0f) {
        moments_act_dev(m, v, act, a_elu, om, ov);
        return;
    }
    if (p >= 1.0f) {
        om = 0.0f;
        ov = 0.0f;
        return;
    }
    float M, V;
    if (act == BNN_FLAG_ELU) {
        const double q = 1.0 - (double)p;
        moments_elu_dev((float)((double)m / q), (float)((double)v / (q * q)), a_elu, M, V);
        om = (float)(q * (double)M);
        ov = (float)(q * (double)V + q * (double)p * (double)M * (double)M);
        return;
    }
    const float q = 1.0f - p;
    moments_act_dev(m / q, v / (q * q), act, a_elu, M, V);
    om = q * M;
    ov = q * V + q * p * M * M;
}

// Backward of moments_dropout_dev: (g_m, g_v) from the gradients (gm', gv') of its two outputs.  With (M, V) as above,
//     gM = q gm' + 2 q p M gv',    gV = q gv'
// go through the activation's own backward at (m / q, v / q^2) (moments_relu_bwd_dev / moments_elu_bwd_dev; the identity passes
// them), and g_m = g_mi / q, g_v = g_vi / q^2.  M is the forward's, evaluated again.  p == 0: the activation's backward alone, its
// bits; p == 1: zeros.
__device__ __forceinline__ void moments_act_bwd_dev(float m, float v, int act, float a_elu, float gom, float gov, float &gm, float &gv)
{
    if (act == BNN_FLAG_RELU) moments_relu_bwd_dev(m, v, gom, gov, gm, gv);
    else if (act == BNN_FLAG_ELU) moments_elu_bwd_dev(m, v, a_elu, gom, gov, gm, gv);
    else { gm = gom; gv = gov; }
}

__device__ __forceinline__ void moments_dropout_bwd_dev(float m, float v, float p, int act, float a_elu, float gom, float gov, float &gm,
                                                        float &gv)
{
    if (p == 0.0f) {
        moments_act_bwd_dev(m, v, act, a_elu, gom, gov, gm, gv);
        return;
    }
    if (p >= 1.0f) {
        gm = 0.0f;
        gv = 0.0f;
        return;
    }
    float M, V, gmi, gvi;
    if (act == BNN_FLAG_ELU) {
        const double q = 1.0 - (double)p;
        const float mi = (float)((double)m / q), vi = (float)((double)v / (q * q));
        moments_elu_dev(mi, vi, a_elu, M, V);
        const float gM = (float)(q * (double)gom + 2.0 * q * (double)p * (double)M * (double)gov), gV = (float)(q * (double)gov);
        moments_elu_bwd_dev(mi, vi, a_elu, gM, gV, gmi, gvi);
        gm = (float)((double)gmi / q);
        gv = (float)((double)gvi / (q * q));
        return;
    }
    const float q = 1.0f - p, mi = m / q, vi = v / (q * q);
    moments_act_dev(mi, vi, act, a_elu, M, V);
    moments_act_bwd_dev(mi, vi, act, a_elu, q * gom + 2.0f * q * p * M * gov, q * gov, gmi, gvi);
    gm = gmi / q;
    gv = gvi / (q * q);
}

// Maximum of two independent Gaussians N(m1, v1), N(m2, v2) by moment matching (K20; Clark 1961), the step a max-pooling window
// is folded with.  theta^2 = v1 + v2, d = m1 - m2, alpha = d / theta, Phi = Phi(alpha), Phi_c = Phi(-alpha), phi = phi(alpha):
//     mean' = m1 Phi + m2 Phi_c + theta phi
//     var'  = v1 Phi + v2 Phi_c + d^2 Phi Phi_c + d theta phi (Phi_c - Phi) - theta^2 phi^2,   clamped at 0
// -- the ReLU's form above with (m2, v2) = (0, 0): m^2 is never subtracted from m^2 + v, and what cancels is relative to d^2, not
// to v, so the step works in fp64 like the ELU (the running maximum of a window stays fp64 until the window's one rounding).
// The smaller tail is 0.5 erfc(|alpha| / sqrt 2) and the other one its complement; beyond |alpha| = 39 tail and phi are zero in
// fp64 and the larger input passes exactly.  theta^2 == 0 (both variances zero; a NaN takes this branch too) is the plain
// maximum: the larger element's (m, v), the first one on a tie.
struct MaxTerms { double theta, d, cdf, cdc, pdf, sum; bool plain; };      // sum: var' before its clamp

__device__ __forceinline__ void moments_max_terms(double m1, double v1, double m2, double v2, MaxTerms &t)
{
    const double th2 = v1 + v2;
    t.plain = !(th2 > 0.0);
    if (t.plain) return;
    t.theta = sqrt(th2);
    t.d = m1 - m2;
    const double alpha = t.d / t.theta;
    const double h = 0.5 * erfc(0.70710678118654752 * fabs(alpha));
    t.cdc = alpha >= 0.0 ? h : 1.0 - h;
    t.cdf = alpha >= 0.0 ? 1.0 - h : h;
    t.pdf = 0.39894228040143268 * exp(-0.5 * alpha * alpha);
    const double tp = t.theta * t.pdf;
    t.sum = v1 * t.cdf + v2 * t.cdc + t.d * t.d * t.cdf * t.cdc + t.d * tp * (t.cdc - t.cdf) - tp * tp;
}

// (m1, v1) <- the moment-matched maximum of (m1, v1) and (m2, v2)
__device__ __forceinline__ void moments_max_step(double &m1, double &v1, double m2, double v2)
{
    MaxTerms t;
    moments_max_terms(m1, v1, m2, v2, t);
    if (t.plain) {
        if (m2 > m1) { m1 = m2; v1 = v2; }
        return;
    }
    m1 = m1 * t.cdf + m2 * t.cdc + t.theta * t.pdf;
    v1 = fmax(t.sum, 0.0);
}

// Backward of moments_max_step on the same terms: from (gm, gv), the gradients of its two results, the gradients of the second
// operand (g2m, g2v); (gm, gv) become those of the first.  With M = mean' (m1 - M = d Phi_c - theta phi, m2 - M = -d Phi -
// theta phi: the shifted forms, nothing of the size of the means cancels):
//     d mean'/d m1 = Phi          d mean'/d m2 = Phi_c          d mean'/d v1 = d mean'/d v2 = phi / (2 theta)
//     d var'/d m1  = 2 Phi (d Phi_c - theta phi) + 2 v1 phi / theta
//     d var'/d m2  = -2 Phi_c (d Phi + theta phi) + 2 v2 phi / theta
//     d var'/d v1  = Phi + alpha v2 phi / theta^2 - (d Phi + theta phi) phi / theta
//     d var'/d v2  = Phi_c - alpha v1 phi / theta^2 + (d Phi_c - theta phi) phi / theta
// Where the step clamped var' (decided on its own sum) the gv terms are absent; the plain maximum sends both gradients to the
// element it took.
__device__ __forceinline__ void moments_max_step_bwd(double m1, double v1, double m2, double v2, double &gm, double &gv, double &g2m,
                                                     double &g2v)
{
    MaxTerms t;
    moments_max_terms(m1, v1, m2, v2, t);
    if (t.plain) {
        const bool second = m2 > m1;
        g2m = second ? gm : 0.0;
        g2v = second ? gv : 0.0;
        if (second) { gm = 0.0; gv = 0.0; }
        return;
    }
    const double go_v = t.sum < 0.0 ? 0.0 : gv;
    const double pt = t.pdf / t.theta, tp = t.theta * t.pdf, apt = t.d * pt / (t.theta * t.theta);      // alpha phi / theta^2
    const double up = t.d * t.cdf + tp, dn = t.d * t.cdc - tp;                                          // M - m2, m1 - M
    const double g1m = gm * t.cdf + go_v * (2.0 * t.cdf * dn + 2.0 * v1 * pt);
    const double g1v = gm * (0.5 * pt) + go_v * (t.cdf + v2 * apt - up * pt);
    g2m = gm * t.cdc + go_v * (-2.0 * t.cdc * up + 2.0 * v2 * pt);
    g2v = gm * (0.5 * pt) + go_v * (t.cdc - v1 * apt + dn * pt);
    gm = g1m;
    gv = g1v;
}

}  // namespace bnn
