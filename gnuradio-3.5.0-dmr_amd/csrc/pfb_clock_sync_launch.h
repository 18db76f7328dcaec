// pfb_clock_sync_launch.h -- launcher of the polyphase clock-recovery walk (internal): gr_pfb_clock_sync_ccf.
#pragma once
#include <hip/hip_runtime.h>

#include "grhip_internal.h"
#include "pfb_clock_sync.h"

namespace grhip {

constexpr int PCS_WIN = 2048;               // items of xz that a wavefront holds in LDS at a time
constexpr int PCS_GROUP = 64;               // symbols whose results are staged in LDS before they are stored
// the longest history and the furthest a symbol reaches behind its limit `lo` fit a window with room to spare
static_assert(PCS_MAX_OSPS * PCS_CARRY + PCS_MAX_OSPS + PCS_MAX_TPF + 2 * PCS_MAX_SPS <= PCS_WIN / 2, "a window holds a symbol's reach");

struct PcsLaunch {
    const float2 *in;           // [S][n] gr_complex, new items only
    float2 *out;                // [S][out_cap] gr_complex
    float *err, *rate, *k;      // [S][out_cap] floats each, or all three null
    int *produced;              // [S]
    int n, nstreams;
    long long out_cap;
    long long arrived;          // items of xz (the zeros in front included) that the calls before have brought
    const float *bank, *dbank;  // [nfilters][tpf] each, an arm's taps reversed: tap j of the row works on xz[pos + j]
    PcsParams p;
    PcsState *state;            // [S], read at the start and written at the end
    float2 *hist;               // [S][pcs_hist()] the last items of xz, oldest first
};

// generic: gr_fir_ccf_generic's summation order (GRHIP_MODE_GENERIC); otherwise fused products and tree sums
int pfb_clock_sync_launch(bool generic, const PcsLaunch &a, hipStream_t st);

}  // namespace grhip
