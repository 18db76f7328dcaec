// arb_resampler.h -- launcher of the pfb_arb_resampler kernel (csrc/arb_resampler.hip), used by
// csrc/capi_arbresamp.hip.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace grhip {

// Limits of the kernel (GRHIP_EINVAL beyond them, include/grhip.h):
//   both tap banks sit in LDS as (h, dh) pairs, rows padded to an odd stride S = tpf | 1:  R * S <= ARB_MAX_TAP_PAIRS
//   the input span of a tile sits in LDS beside them:                                      ARB_SPAN_BYTES
//   the per-output position inside a tile is 32-bit: dec_rate + 1 <= ARB_MAX_DEC, i.e. filter_size / rate < 2^20
constexpr int ARB_THREADS = 256;
constexpr int ARB_MAX_TILE = 1024;
constexpr int ARB_MAX_TAP_PAIRS = 4096;                 // 32 KB
constexpr int ARB_SPAN_BYTES = 32 * 1024;
constexpr unsigned ARB_MAX_DEC = 1u << 20;

// One output's place in the schedule when it has to come from a float walk (rate > filter_size): the
// first input item the two filters read, the filter index j and the interpolation weight acc.
struct ArbStep {
    long long count;
    int j;
    float acc;
};

// The index schedule of one call.  Closed form (steps == nullptr), output k of the launch:
//   T_k = A0 + k*F,  pos_k = j0 + k*D + (T_k >> 23),  count_k = c0 + pos_k / R,  j_k = pos_k % R,
//   acc_k = (T_k & (2^23 - 1)) * 2^-23.
// count_k indexes the logical input: `lead` zeros, then the n_phys items at `in`.
struct ArbSched {
    long long c0 = 0;
    unsigned long long j0 = 0, A0 = 0;
    unsigned F = 0, D = 0;
    const ArbStep *steps = nullptr;         // device array of nout entries, or nullptr for the closed form
};

struct ArbLaunch {
    const void *in = nullptr;               // float2 (ccf) or float (fff) items
    long long in_stride = 0, lead = 0, n_phys = 0;
    void *out = nullptr;
    long long out_stride = 0, nout = 0;
    int n_streams = 1;
    const float2 *taps = nullptr;           // [R][S] (h, dh) pairs, reversed: taps[j][t] multiplies in[count + t]
    int R = 1, tpf = 1, S = 1;
    int tile = 1;                           // outputs per workgroup
    int span_cap = 0;                       // LDS items reserved for a tile's input span
    ArbSched sc;
};

// complex: float2 items (ccf) else float (fff); generic: the reference's generic order, bit-exact
int arb_resampler_launch(bool complex, bool generic, const ArbLaunch &a, hipStream_t st);

}  // namespace grhip
