// frac_interp.h -- launcher of the fractional_interpolator kernel (csrc/frac_interp.hip), used by
// csrc/capi_fracinterp.hip.  The index schedule it carries (FracSched) is csrc/sched_plan.h.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "sched_plan.h"

namespace grhip {

// Limits of the kernel (GRHIP_EINVAL beyond them, include/grhip.h):
//   the input span of a tile sits in LDS beside the 129 x 8 tap bank:                      FRAC_SPAN_BYTES
//   the per-output position inside a tile is 32-bit, and F = interp_ratio * 2^24 times a tile's outputs stays far
//   below 2^63:  interp_ratio < FRAC_MAX_RATIO
constexpr int FRAC_THREADS = 256;
constexpr int FRAC_TILE = 1024;                         // outputs per workgroup, at most
constexpr int FRAC_SPAN_BYTES = 32 * 1024;
constexpr float FRAC_MAX_RATIO = 1048576.0f;            // 2^20

struct FracLaunch {
    const void *in = nullptr;                   // float2 (cc) or float (ff) items
    long long in_stride = 0, n_phys = 0;
    void *out = nullptr;
    long long out_stride = 0, nout = 0;
    int n_streams = 1;
    const float *taps = nullptr;                // DeviceTables::mmse_rev: [8][129], taps[t][imu] multiplies in[ii + t]
    int tile = 1;                               // outputs per workgroup
    int span_cap = 0;                           // LDS items reserved for a tile's input span
    FracSched sc;                               // sched_plan.h (with FRAC_NTAPS and FRAC_NSTEPS)
};

// complex: float2 items (cc) else float (ff); generic: the reference's generic order, bit-exact
int frac_interp_launch(bool complex, bool generic, const FracLaunch &a, hipStream_t st);

}  // namespace grhip
