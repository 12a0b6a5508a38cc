// bnn_knobs.hpp -- every environment variable the library reads, each read once per process.
//
// The production library (make) reads two.  The rest exist only in the diagnostic library (make diag, -DBNN_DIAG ->
// libbnn_hip_diag.so, same ABI, loaded through BNN_HIP_LIB): in a production build each of them is a constexpr function that
// returns its default, so the branches behind it -- and the kernel instantiations only they launch -- are not compiled, and
// neither the knob's name nor a getenv of it is in the library.  Device code tests a diagnostic flag under
// `if constexpr (kDiagBuild)` only.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace bnn {

#ifdef BNN_DIAG
constexpr bool kDiagBuild = true;
#define BNN_FRESH_ERROR "diagnostic build (BNN_DIAG)"      // bnn_last_error() before any error: tells the two builds apart
#else
constexpr bool kDiagBuild = false;
#define BNN_FRESH_ERROR ""
#endif

namespace knob {

inline int env_int(const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; }
inline bool env_starts(const char *name, const char *prefix)
{
    const char *e = getenv(name);
    if (!e) return false;
    while (*prefix) if (*e++ != *prefix++) return false;
    return true;
}
inline uint64_t env_address(const char *name) { const char *e = getenv(name); return e ? strtoull(e, nullptr, 0) : 0ull; }

#define BNN_KNOB(TYPE, NAME, READ) inline TYPE NAME() { static const TYPE v = READ; return v; }
#ifdef BNN_DIAG
#define BNN_DIAG_KNOB(TYPE, NAME, READ, DEFAULT) BNN_KNOB(TYPE, NAME, READ)
#else
#define BNN_DIAG_KNOB(TYPE, NAME, READ, DEFAULT) constexpr TYPE NAME() { return DEFAULT; }
#endif

// ---- read by every build: each selects a second CORRECT kernel, the suite's bit-for-bit reference in a fresh process
// BNN_DENSE_TILE=0..5: the dense launch's tile (dense_pick_tile); unset or out of range = the heuristic
BNN_KNOB(int, dense_tile, env_int("BNN_DENSE_TILE", -1))
// BNN_DRAW_LEAN=0: the draw launch always takes the full kernel, never the lean one
BNN_KNOB(bool, draw_no_lean, env_starts("BNN_DRAW_LEAN", "0"))

// ---- read by the diagnostic build only
// timing-only phase skips: the launch returns BNN_OK with WRONG results (announced once on stderr, wrong_results below)
// BNN_DENSE_DIAG=n: the DIAG instantiation of k_dense_bf16 (1, 2, 5, 7, 8, 9 skip phases; 3, 4, 6 stay correct)
BNN_DIAG_KNOB(int, dense_diag, env_int("BNN_DENSE_DIAG", 0), 0)
// BNN_CONV_DIAG=bits: k_conv_bf16 skips 1 the image fill, 2 the k loop, 4 the output copy
BNN_DIAG_KNOB(int, conv_diag, env_int("BNN_CONV_DIAG", 0), 0)
// BNN_WGRAD_DIAG=bits: k_wgrad_bf16_dma8 skips 1 the fragment reads and MFMAs, 2 the LDS-DMA
BNN_DIAG_KNOB(int, wgrad_diag, env_int("BNN_WGRAD_DIAG", 0), 0)
// BNN_WGRAD_NOEPS=1: the sampled weight gradient runs as the plain one (no eps epilogue)
BNN_DIAG_KNOB(bool, wgrad_noeps, env_starts("BNN_WGRAD_NOEPS", "1"), false)
// a raw device address the kernel writes time stamps to (results stay correct)
// BNN_DENSE_STAMPS=<address>: with BNN_DENSE_DIAG=6..9, five stamps per workgroup of k_dense_bf16 (tools/dense_stamps.py)
BNN_DIAG_KNOB(uint64_t, dense_stamps, env_address("BNN_DENSE_STAMPS"), 0)
// BNN_STAMPS=<address>: the STAMPS instantiation of k_linear_sym (tools/stamps.py)
BNN_DIAG_KNOB(uint64_t, linear_stamps, env_address("BNN_STAMPS"), 0)
// A/B switches that force a correct path some input takes anyway
// BNN_DENSE_XCD=0: k_dense_bf16 walks its tiles in plain sample-major order
BNN_DIAG_KNOB(bool, dense_no_xcd, env_starts("BNN_DENSE_XCD", "0"), false)
// BNN_DRAW_TAPG=0: conv weights are drawn without the tap-group transpose
BNN_DIAG_KNOB(bool, draw_no_tapg, env_starts("BNN_DRAW_TAPG", "0"), false)
// BNN_DRAW_KL_ITEMS=0: the KL first pass that rides on a draw launch runs on workgroups of its own
BNN_DIAG_KNOB(bool, draw_no_kl_items, env_starts("BNN_DRAW_KL_ITEMS", "0"), false)
// BNN_DRAW_SPLIT=n: the draw launch splits its samples over n grid rows (0 = the heuristic)
BNN_DIAG_KNOB(int, draw_split, env_int("BNN_DRAW_SPLIT", 0), 0)
// BNN_XCD_A=n: k_linear_sym's XCD grid takes n sample groups (-1 = the least-L2-fill choice)
BNN_DIAG_KNOB(int, linear_xcd_a, env_int("BNN_XCD_A", -1), -1)
// BNN_LINEAR_KERNEL=v1: linear and conv forwards take the generic tile kernel, as misaligned operands do
BNN_DIAG_KNOB(bool, linear_force_v1, env_starts("BNN_LINEAR_KERNEL", "v1"), false)

#undef BNN_DIAG_KNOB
#undef BNN_KNOB

// one line on stderr, the first time a launch site finds its wrong-result knob active
#ifdef BNN_DIAG
#define BNN_WRONG_RESULTS_ONCE(NAME) \
    do { static const int once = fprintf(stderr, "libbnn_hip_diag: %s is set: timing-only launches, their results are WRONG\n", NAME); (void)once; } while (0)
#else
#define BNN_WRONG_RESULTS_ONCE(NAME) do { } while (0)
#endif

}  // namespace knob
}  // namespace bnn
