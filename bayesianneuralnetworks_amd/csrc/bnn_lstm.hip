// bnn_lstm.hip -- K25: one time step of the Bayesian LSTM cell (nn.NormalLSTM, Fortunato et al. 2017), forward and backward,
// all S MC samples in ONE launch per step.  No call site in the reference (it has no recurrent layer).
//
//   G_t = Gx_t + h_{t-1} W_h^T            Gx_t = x_t W_x^T + b for all steps at once, by bnn_linear_forward, before the loop
//   (i, f, g, o) = split(G_t)             rows of W_h in torch's gate order: unit j owns rows j, H + j, 2 H + j, 3 H + j
//   c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g),   h_t = sigmoid(o) tanh(c_t)
//
// Tile.  A workgroup is ONE wave.  It owns L_TR = 16 rows of one sample x L_TU = 16 hidden units and holds the four gate
// columns of its units in four 16 x 16 accumulators of v_mfma_f32_16x16x4_f32 (exact fp32 operands, fp32 accumulate; four
// independent accumulators are what the instruction's 40-cycle dependent latency asks for).  Operands go from global memory
// straight into the MFMA's one-register fragments -- lane l holds A[row l & 15][k-group l >> 4] -- so there is no LDS and no
// barrier: a lane loads four consecutive k of its row (one 16-byte load where the pointer, the pitch and H allow it, four
// element loads otherwise; zeros beyond the row count, the unit count and H) and spends them on four MFMA steps, the next
// 16 k in flight while the current 16 multiply.  Grid (row tiles, unit tiles, S): no workgroup depends on another one.
//
// Accumulation order.  An MFMA is a k-ordered fmaf chain on its C operand (programming guide, "FP32-input MFMA").  Forward: C
// starts at Gx_t; for kb = 0, 16, ... and i = 0 .. 3 the products of k = kb + i, kb + 4 + i, kb + 8 + i, kb + 12 + i are added in
// that order (k >= H adds +0).  Backward: C starts at 0; for jb = 0, 16, ..., i = 0 .. 3 and gate q = 0 .. 3 the products of
// n = q H + jb + i, + 4, + 8, + 12.  Both orders are functions of H alone: S, the row count and the grid do not enter, there is
// no atomic and no split, so two calls give the same bits and a one-sample call gives the bits of that sample in a batch.
//
// sigmoid and tanh are written out so that their roundings can be counted (u = 2^-24; expf is the device library's, 1 ulp = 2 u):
//   sigmoid(x) = 1 / (1 + expf(-x))                    relative error <= 4 u (expf 2 u damped by e / (1 + e) < 1, the sum u, the
//                                                      correctly rounded quotient u); |x| <= 88: expf(88) = 1.7e38 is finite
//   tanh(x)    = copysign((1 - e) / (1 + e), x),       e = expf(-2 |x|) in (0, 1]: nothing can overflow; absolute error <= 5 u
//                                                      (numerator 2 u, denominator 2 u relative, quotient u)
// The backward forms dG_t from the saved gate activations itself (pointwise; every unit tile of a row tile recomputes it, the
// tile with blockIdx.y == 0 stores it, together with g_c for step t - 1) and contracts it with W_h over all 4 H gate columns.
#include "bnn_device.hpp"

namespace bnn {

constexpr int L_TR = 16;       // rows of one sample per workgroup          (ops.LSTM_TILE_ROWS)
constexpr int L_TU = 16;       // hidden units per workgroup                (ops.LSTM_TILE_UNITS)
constexpr int L_KB = 16;       // k per loop iteration: four MFMA steps of four

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float lstm_sigmoid(float x)
{
    return 1.0f / (1.0f + expf(-x));
}

__device__ __forceinline__ float lstm_tanh(float x)
{
    const float e = expf(-2.0f * fabsf(x));
    return copysignf((1.0f - e) / (1.0f + e), x);
}

// four consecutive elements row[k .. k + 3] of a row of n elements; zeros where ok is false or k + i >= n
template <bool VEC>
__device__ __forceinline__ float4 lstm_load4(const float *row, int k, int n, bool ok)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ok || k >= n) return v;
    if (VEC) return *reinterpret_cast<const float4 *>(row + k);       // n % 4 == 0: k + 3 < n
    v.x = row[k];
    if (k + 1 < n) v.y = row[k + 1];
    if (k + 2 < n) v.z = row[k + 2];
    if (k + 3 < n) v.w = row[k + 3];
    return v;
}

template <bool VEC>
__device__ __forceinline__ void lstm_store4(float *row, int k, int n, float4 v)
{
    if (k >= n) return;
    if (VEC) { *reinterpret_cast<float4 *>(row + k) = v; return; }
    row[k] = v.x;
    if (k + 1 < n) row[k + 1] = v.y;
    if (k + 2 < n) row[k + 2] = v.z;
    if (k + 3 < n) row[k + 3] = v.w;
}

__device__ __forceinline__ float f4_get(const float4 &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

struct LstmFwd {
    const float *gx; int64_t ldgx;
    const float *w; int64_t w_ss;
    const float *hp; int64_t ldhp;
    const float *cp; int64_t ldcp;
    float *h; int64_t ldh;
    float *c; int64_t ldc;
    float *gates; int64_t ldgt;
    int64_t rows;
    int H;
};

// VEC: h_prev rows and W_h rows are read 16 bytes at a time (H % 4 == 0, both on 16 bytes, pitches multiples of 4)
template <bool VEC>
__global__ __launch_bounds__(64) void k_lstm_step_fwd(LstmFwd p)
{
    const int lane = (int)threadIdx.x, l15 = lane & 15, kg = lane >> 4;
    const int H = p.H;
    const int64_t s = blockIdx.z, r0 = (int64_t)blockIdx.x * L_TR;
    const int j = (int)blockIdx.y * L_TU + l15;                      // the lane's unit: B-operand column and C/D column
    const bool j_ok = j < H;
    const int64_t srow = s * p.rows;                                 // first row of the sample in every (S, rows, .) operand

    // C starts at Gx_t: C/D element reg of a lane is row kg * 4 + reg, column l15
    f32x4 acc[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t r = r0 + kg * 4 + reg;
        const bool ok = j_ok && r < p.rows;
        const float *g = p.gx + (srow + (ok ? r : 0)) * p.ldgx + (ok ? j : 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q][reg] = ok ? g[(int64_t)q * H] : 0.f;
    }

    if (p.hp) {
        const int64_t ar = r0 + l15;                                 // the lane's A-operand row
        const bool a_ok = ar < p.rows;
        const float *arow = p.hp + (srow + (a_ok ? ar : 0)) * p.ldhp;
        const float *wrow[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) wrow[q] = p.w + s * p.w_ss + ((int64_t)q * H + (j_ok ? j : 0)) * H;
        float4 a = lstm_load4<VEC>(arow, 4 * kg, H, a_ok), b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = lstm_load4<VEC>(wrow[q], 4 * kg, H, j_ok);
        for (int kb = 0; kb < H; kb += L_KB) {
            const int kn = kb + L_KB + 4 * kg;                       // the next iteration's operands (zeros past H)
            const float4 an = lstm_load4<VEC>(arow, kn, H, a_ok);
            float4 bn[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) bn[q] = lstm_load4<VEC>(wrow[q], kn, H, j_ok);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_get(a, i), f4_get(b[q], i), acc[q], 0, 0, 0);
            a = an;
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = bn[q];
        }
    }

    // the cell update on the lane's four (row, unit) elements
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t r = r0 + kg * 4 + reg;
        if (!j_ok || r >= p.rows) continue;
        const float gi = lstm_sigmoid(acc[0][reg]), gf = lstm_sigmoid(acc[1][reg]);
        const float gg = lstm_tanh(acc[2][reg]), go = lstm_sigmoid(acc[3][reg]);
        const float cprev = p.cp ? p.cp[(srow + r) * p.ldcp + j] : 0.f;
        const float c = __builtin_fmaf(gf, cprev, gi * gg);
        p.c[(srow + r) * p.ldc + j] = c;
        p.h[(srow + r) * p.ldh + j] = go * lstm_tanh(c);
        if (p.gates) {
            float *gt = p.gates + (srow + r) * p.ldgt + j;
            gt[0] = gi; gt[H] = gf; gt[2 * (int64_t)H] = gg; gt[3 * (int64_t)H] = go;
        }
    }
}

struct LstmBwd {
    const float *gates; int64_t ldgt;
    const float *cp; int64_t ldcp;
    const float *c; int64_t ldc;
    const float *gho; int64_t ldgho;
    const float *ghi;           // (S, rows, H) contiguous, or NULL (zeros)
    const float *gci;           // likewise
    const float *w; int64_t w_ss;
    float *dg; int64_t lddg;
    float *ghp;                 // (S, rows, H) contiguous
    float *gcp;                 // (S, rows, H) contiguous
    int64_t rows;
    int H;
};

// the pointwise operands of four consecutive units jj .. jj + 3 of one row
struct LstmBwdRaw {
    float4 gi, gf, gg, go, cp, c, gho, ghi, gci;
};

template <bool VEC>
__device__ __forceinline__ LstmBwdRaw lstm_bwd_load(const LstmBwd &p, int64_t row, bool ok, int jj)
{
    const int H = p.H;
    LstmBwdRaw v;
    const float *gt = p.gates + row * p.ldgt;
    v.gi = lstm_load4<VEC>(gt, jj, H, ok);
    v.gf = lstm_load4<VEC>(gt + H, jj, H, ok);
    v.gg = lstm_load4<VEC>(gt + 2 * (int64_t)H, jj, H, ok);
    v.go = lstm_load4<VEC>(gt + 3 * (int64_t)H, jj, H, ok);
    v.cp = lstm_load4<VEC>(p.cp ? p.cp + row * p.ldcp : nullptr, jj, H, ok && p.cp);
    v.c = lstm_load4<VEC>(p.c + row * p.ldc, jj, H, ok);
    v.gho = lstm_load4<VEC>(p.gho ? p.gho + row * p.ldgho : nullptr, jj, H, ok && p.gho);
    v.ghi = lstm_load4<VEC>(p.ghi ? p.ghi + row * H : nullptr, jj, H, ok && p.ghi);
    v.gci = lstm_load4<VEC>(p.gci ? p.gci + row * H : nullptr, jj, H, ok && p.gci);
    return v;
}

// dG of one (row, unit) from the saved activations; d[q] the gradient of gate q's pre-activation, gcp of c_{t-1}
__device__ __forceinline__ void lstm_bwd_point(float gi, float gf, float gg, float go, float cp, float c, float gho, float ghi,
                                               float gci, float d[4], float &gcp)
{
    const float gh = gho + ghi;
    const float tc = lstm_tanh(c);
    const float dc = __builtin_fmaf(gh * go, __builtin_fmaf(-tc, tc, 1.0f), gci);
    d[0] = (dc * gg) * (gi * (1.0f - gi));
    d[1] = (dc * cp) * (gf * (1.0f - gf));
    d[2] = (dc * gi) * __builtin_fmaf(-gg, gg, 1.0f);
    d[3] = (gh * tc) * (go * (1.0f - go));
    gcp = dc * gf;
}

// VEC: every pointwise operand and dG are read / written 16 bytes at a time (H % 4 == 0, all on 16 bytes, pitches multiples of 4);
// W_h is read by the element in both forms (the contraction index runs down its rows)
template <bool VEC>
__global__ __launch_bounds__(64) void k_lstm_step_bwd(LstmBwd p)
{
    const int lane = (int)threadIdx.x, l15 = lane & 15, kg = lane >> 4;
    const int H = p.H;
    const int64_t s = blockIdx.z, r0 = (int64_t)blockIdx.x * L_TR;
    const int j = (int)blockIdx.y * L_TU + l15;                      // output unit: B-operand column and C/D column
    const bool j_ok = j < H;
    const int64_t srow = s * p.rows;
    const int64_t ar = r0 + l15;                                     // the row whose dG this lane forms (A-operand row)
    const bool a_ok = ar < p.rows;
    const int64_t arow = srow + (a_ok ? ar : 0);
    const bool store = blockIdx.y == 0;
    const float *wcol = p.w + s * p.w_ss + (j_ok ? j : 0);

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    LstmBwdRaw v = lstm_bwd_load<VEC>(p, arow, a_ok, 4 * kg);
    for (int jb = 0; jb < H; jb += L_KB) {
        const int jj = jb + 4 * kg;                                  // this lane: units jj .. jj + 3, one per MFMA group of four
        const LstmBwdRaw vn = lstm_bwd_load<VEC>(p, arow, a_ok, jj + L_KB);
        float b[4][4];                                               // W_h[q H + jj + i][j]
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                b[i][q] = (j_ok && jj + i < H) ? wcol[((int64_t)q * H + jj + i) * H] : 0.f;
        float d[4][4], gcp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            lstm_bwd_point(f4_get(v.gi, i), f4_get(v.gf, i), f4_get(v.gg, i), f4_get(v.go, i), f4_get(v.cp, i), f4_get(v.c, i),
                           f4_get(v.gho, i), f4_get(v.ghi, i), f4_get(v.gci, i), d[i], gcp[i]);
        if (store && a_ok) {
            float *dgr = p.dg + arow * p.lddg;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                lstm_store4<VEC>(dgr + (int64_t)q * H, jj, H, make_float4(d[0][q], d[1][q], d[2][q], d[3][q]));
            lstm_store4<VEC>(p.gcp + arow * H, jj, H, make_float4(gcp[0], gcp[1], gcp[2], gcp[3]));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(d[i][q], b[i][q], acc, 0, 0, 0);
        v = vn;
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t r = r0 + kg * 4 + reg;
        if (j_ok && r < p.rows) p.ghp[(srow + r) * H + j] = acc[reg];
    }
}

static inline bool lstm_al16(const void *p) { return !misaligned(p, 15); }
static inline bool lstm_al4(const void *p) { return !misaligned(p, 3); }
// (nsamples, rows, ld) addresses at most 2^62 elements
static inline bool lstm_extent_ok(int64_t rows, int64_t ld, int nsamples)
{
    return ld <= 0x7FFFFFFF && rows * ld <= ((int64_t)1 << 62) / nsamples;
}

static int lstm_check_dims(const char *who, int64_t rows, int64_t H, int nsamples, int64_t w_sample_stride)
{
    if (rows < 1 || H < 1 || nsamples < 1) { set_error("%s: rows, H and nsamples must be at least 1", who); return BNN_E_SHAPE; }
    if (rows > 0x7FFFFFFF || H > (int64_t)L_TU * 65535 || nsamples > 65535) {
        set_error("%s: extent too large (rows < 2^31, H <= %d, nsamples <= 65535)", who, L_TU * 65535);
        return BNN_E_RANGE;
    }
    if (w_sample_stride < 4 * H * H) { set_error("%s: w_sample_stride is below 4 H H", who); return BNN_E_SHAPE; }
    if (w_sample_stride > ((int64_t)1 << 62) / nsamples) { set_error("%s: W_h extent too large", who); return BNN_E_RANGE; }
    return BNN_OK;
}

}  // namespace bnn

using namespace bnn;

extern "C" int bnn_lstm_step_forward(const float *gx, int64_t ldgx, const float *w_h, int64_t w_sample_stride, const float *h_prev,
                                     int64_t ldh_prev, const float *c_prev, int64_t ldc_prev, float *h, int64_t ldh, float *c,
                                     int64_t ldc, float *gates, int64_t ldgates, int64_t rows, int64_t H, int nsamples, void *stream)
{
    const char *who = "bnn_lstm_step_forward";
    if (!gx || !w_h || !h || !c) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if ((h_prev == nullptr) != (c_prev == nullptr)) { set_error("%s: h_prev and c_prev must be given together", who); return BNN_E_NULL; }
    int rc = lstm_check_dims(who, rows, H, nsamples, w_sample_stride);
    if (rc) return rc;
    if (ldgx < 4 * H || ldh < H || ldc < H || (h_prev && (ldh_prev < H || ldc_prev < H)) || (gates && ldgates < 4 * H)) {
        set_error("%s: a row pitch is below the row length", who);
        return BNN_E_SHAPE;
    }
    if (!lstm_extent_ok(rows, ldgx, nsamples) || !lstm_extent_ok(rows, ldh, nsamples) || !lstm_extent_ok(rows, ldc, nsamples) ||
        (h_prev && (!lstm_extent_ok(rows, ldh_prev, nsamples) || !lstm_extent_ok(rows, ldc_prev, nsamples))) ||
        (gates && !lstm_extent_ok(rows, ldgates, nsamples))) {
        set_error("%s: nsamples * rows * pitch is out of range", who);
        return BNN_E_RANGE;
    }
    if (!lstm_al4(gx) || !lstm_al4(w_h) || !lstm_al4(h_prev) || !lstm_al4(c_prev) || !lstm_al4(h) || !lstm_al4(c) || !lstm_al4(gates)) {
        set_error("%s: pointer not aligned to its element", who);
        return BNN_E_ALIGN;
    }
    LstmFwd p{};
    p.gx = gx; p.ldgx = ldgx; p.w = w_h; p.w_ss = w_sample_stride; p.hp = h_prev; p.ldhp = ldh_prev; p.cp = c_prev; p.ldcp = ldc_prev;
    p.h = h; p.ldh = ldh; p.c = c; p.ldc = ldc; p.gates = gates; p.ldgt = ldgates; p.rows = rows; p.H = (int)H;
    const bool vec = H % 4 == 0 && lstm_al16(w_h) && w_sample_stride % 4 == 0 && (!h_prev || (lstm_al16(h_prev) && ldh_prev % 4 == 0));
    const dim3 grid((unsigned)((rows + L_TR - 1) / L_TR), (unsigned)((H + L_TU - 1) / L_TU), (unsigned)nsamples);
    if (vec) hipLaunchKernelGGL(k_lstm_step_fwd<true>, grid, dim3(64), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(k_lstm_step_fwd<false>, grid, dim3(64), 0, (hipStream_t)stream, p);
    return check_launch(who);
}

extern "C" int bnn_lstm_step_backward(const float *gates, int64_t ldgates, const float *c_prev, int64_t ldc_prev, const float *c,
                                      int64_t ldc, const float *g_h_out, int64_t ldg_h_out, const float *g_h_in, const float *g_c_in,
                                      const float *w_h, int64_t w_sample_stride, float *dg, int64_t lddg, float *g_h_prev,
                                      float *g_c_prev, int64_t rows, int64_t H, int nsamples, void *stream)
{
    const char *who = "bnn_lstm_step_backward";
    if (!gates || !c || !w_h || !dg || !g_h_prev || !g_c_prev) { set_error("%s: NULL pointer", who); return BNN_E_NULL; }
    if ((g_h_in == nullptr) != (g_c_in == nullptr)) { set_error("%s: g_h_in and g_c_in must be given together", who); return BNN_E_NULL; }
    int rc = lstm_check_dims(who, rows, H, nsamples, w_sample_stride);
    if (rc) return rc;
    if (ldgates < 4 * H || lddg < 4 * H || ldc < H || (c_prev && ldc_prev < H) || (g_h_out && ldg_h_out < H)) {
        set_error("%s: a row pitch is below the row length", who);
        return BNN_E_SHAPE;
    }
    if (!lstm_extent_ok(rows, ldgates, nsamples) || !lstm_extent_ok(rows, lddg, nsamples) || !lstm_extent_ok(rows, ldc, nsamples) ||
        (c_prev && !lstm_extent_ok(rows, ldc_prev, nsamples)) || (g_h_out && !lstm_extent_ok(rows, ldg_h_out, nsamples))) {
        set_error("%s: nsamples * rows * pitch is out of range", who);
        return BNN_E_RANGE;
    }
    if (!lstm_al4(gates) || !lstm_al4(c_prev) || !lstm_al4(c) || !lstm_al4(g_h_out) || !lstm_al4(g_h_in) || !lstm_al4(g_c_in) ||
        !lstm_al4(w_h) || !lstm_al4(dg) || !lstm_al4(g_h_prev) || !lstm_al4(g_c_prev)) {
        set_error("%s: pointer not aligned to its element", who);
        return BNN_E_ALIGN;
    }
    LstmBwd p{};
    p.gates = gates; p.ldgt = ldgates; p.cp = c_prev; p.ldcp = ldc_prev; p.c = c; p.ldc = ldc; p.gho = g_h_out; p.ldgho = ldg_h_out;
    p.ghi = g_h_in; p.gci = g_c_in; p.w = w_h; p.w_ss = w_sample_stride; p.dg = dg; p.lddg = lddg; p.ghp = g_h_prev; p.gcp = g_c_prev;
    p.rows = rows; p.H = (int)H;
    const bool vec = H % 4 == 0 && lstm_al16(gates) && ldgates % 4 == 0 && lstm_al16(c) && ldc % 4 == 0 &&
                     (!c_prev || (lstm_al16(c_prev) && ldc_prev % 4 == 0)) && (!g_h_out || (lstm_al16(g_h_out) && ldg_h_out % 4 == 0)) &&
                     lstm_al16(g_h_in) && lstm_al16(g_c_in) && lstm_al16(dg) && lddg % 4 == 0 && lstm_al16(g_c_prev);
    const dim3 grid((unsigned)((rows + L_TR - 1) / L_TR), (unsigned)((H + L_TU - 1) / L_TU), (unsigned)nsamples);
    if (vec) hipLaunchKernelGGL(k_lstm_step_bwd<true>, grid, dim3(64), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(k_lstm_step_bwd<false>, grid, dim3(64), 0, (hipStream_t)stream, p);
    return check_launch(who);
}
