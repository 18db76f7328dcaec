// arb_resampler.h -- launcher of the pfb_arb_resampler kernel (csrc/arb_resampler.hip), used by
// csrc/capi_arbresamp.hip.  The index schedule it carries (ArbSched, ArbStep) is csrc/sched_plan.h.  Not part of the
// ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "sched_plan.h"

namespace grhip {

// Limits of the kernel (GRHIP_EINVAL beyond them, include/grhip.h):
//   both tap banks sit in LDS as (h, dh) pairs, rows padded to an odd stride S = tpf | 1:  R * S <= ARB_MAX_TAP_PAIRS
//   the input span of a tile sits in LDS beside them:                                      ARB_SPAN_BYTES
//   the per-output position inside a tile is 32-bit:                                       ARB_MAX_DEC (sched_plan.h)
constexpr int ARB_THREADS = 256;
constexpr int ARB_MAX_TILE = 1024;
constexpr int ARB_MAX_TAP_PAIRS = 4096;                 // 32 KB
constexpr int ARB_SPAN_BYTES = 32 * 1024;

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
    ArbSched sc;                            // sched_plan.h
};

// complex: float2 items (ccf) else float (fff); generic: the reference's generic order, bit-exact
int arb_resampler_launch(bool complex, bool generic, const ArbLaunch &a, hipStream_t st);

}  // namespace grhip
