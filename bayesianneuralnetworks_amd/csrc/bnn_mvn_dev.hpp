// bnn_mvn_dev.hpp -- the element of WeightMultivariateNormal's factor, L = sqrt(tril(softplus(scale)) + 1e-10 I) taken element by
// element, as ONE device function: the keyed draw, its backward and the KL (bnn_mvn.hip) and the moment pass of the layer
// (bnn_moments_head.hip) all take L or V from here, so the bits of L are the same whoever forms it.
#pragma once
#include "bnn_device.hpp"

namespace bnn {

// softplus(x), torch's (beta 1, threshold 20), to a few ulp relative for every x: log1p(e) = ln(u) e / (u - 1), u = 1 + e
// (the rounding of u cancels; log1p(e) = e when u == 1) on the native exp2 / log2 / rcp units.
__device__ __forceinline__ float mvn_softplus(float x)
{
    const float e = __builtin_amdgcn_exp2f(x * 1.44269504088896341f);
    const float u = 1.0f + e;
    const float d = u - 1.0f;
    float sp = __builtin_amdgcn_logf(u) * 0.693147180559945309f * (e * __builtin_amdgcn_rcpf(d));
    sp = (d == 0.0f) ? e : sp;
    return x > 20.0f ? x : sp;
}

// V[i][j] = softplus(scale) + (i == j ? 1e-10 : 0) -- WeightMultivariateNormal.variance on the lower triangle
__device__ __forceinline__ float mvn_v(float s, bool diag)
{
    const float v = mvn_softplus(s);
    return diag ? v + 1e-10f : v;
}

// L[i][j] = sqrt(V[i][j]) on the lower triangle -- WeightMultivariateNormal.stddev
__device__ __forceinline__ float mvn_l(float s, bool diag) { return __builtin_sqrtf(mvn_v(s, diag)); }

}  // namespace bnn
