// bnn_lrt_tile.hpp -- the loader pieces of the 64 x 64 register-staged contraction tile that K10 (bnn_lrt.hip) and K16
// (bnn_moments.hip) share: the operand fetch of one thread's share of a 64 x BK tile and the fp32 / bf16 LDS conversion.
#pragma once
#include "bnn_device.hpp"

namespace bnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr int kLrtTile = 64;
constexpr int kLrtThreads = 256;

__device__ __forceinline__ float lrt_ld(const void *p, int64_t i, bool bf)
{
    return bf ? __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(p)[i] << 16) : reinterpret_cast<const float *>(p)[i];
}

// One thread's share of a 64 x BK operand tile.  TR = false: the contraction index is contiguous in memory (element (r, c) at
// p[r ld + c]; a wave reads runs of BK consecutive c).  TR = true: the row index is (element (r, c) at p[c ld + r]; a wave reads
// 64 consecutive r).  Out-of-range elements are zero.
template <bool TR, int BK>
__device__ __forceinline__ void lrt_fetch(float (&v)[BK / 4], const void *p, bool bf, int64_t ld, int row0, int rows, int c0, int cdim)
{
#pragma unroll
    for (int it = 0; it < BK / 4; ++it) {
        const int idx = it * kLrtThreads + (int)threadIdx.x;
        const int r = TR ? idx % kLrtTile : idx / BK;
        const int c = TR ? idx / kLrtTile : idx % BK;
        const bool ok = row0 + r < rows && c0 + c < cdim;
        const int64_t off = TR ? (int64_t)(c0 + c) * ld + (row0 + r) : (int64_t)(row0 + r) * ld + (c0 + c);
        v[it] = ok ? lrt_ld(p, off, bf) : 0.f;
    }
}

template <typename T> __device__ __forceinline__ T lrt_cvt(float v);
template <> __device__ __forceinline__ float lrt_cvt<float>(float v) { return v; }
template <> __device__ __forceinline__ uint16_t lrt_cvt<uint16_t>(float v) { return f2bf(v); }

}  // namespace bnn
