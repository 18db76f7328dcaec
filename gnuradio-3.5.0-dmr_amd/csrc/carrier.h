// carrier.h -- launchers of the carrier-tracking loops (internal): digital_costas_loop_cc, gr_pll_freqdet_cf,
// gr_pll_refout_cc and gr_pll_carriertracking_cc.
#pragma once
#include <hip/hip_runtime.h>

#include "grhip_internal.h"

namespace grhip {

// samples of one stream that a wavefront holds in LDS at a time
constexpr int CARRIER_WIN = 1024;

enum { PLL_FREQDET = 0, PLL_REFOUT = 1, PLL_CARRIERTRACKING = 2 };

// what a stream remembers: gri_control_loop's d_phase and d_freq, and gr_pll_carriertracking_cc's d_locksig
struct CarrierState {
    float phase, freq, locksig, pad;
};

// gri_control_loop's d_alpha, d_beta, d_max_freq, d_min_freq; gr_pll_carriertracking_cc's d_lock_threshold, d_squelch_enable
struct CarrierParams {
    float alpha, beta, max_freq, min_freq, lock_threshold;
    int squelch;
};

struct CarrierLaunch {
    const float2 *in;       // [S][n] gr_complex
    void *out;              // [S][n] gr_complex (float for pll_freqdet_cf); must not overlap in
    float *freq_out;        // costas only: [S][n] floats or null
    int n, nstreams;
    CarrierParams p;
    CarrierState *state;    // [S], read at the start and written at the end
};

// kind: PLL_*; atan_tab: the 257 floats of gr_fast_atan2f on the device
int pll_launch(int kind, const CarrierLaunch &a, const float *atan_tab, hipStream_t st);
// order 2, 4 or 8; fast_nco false: the float-rounded double sine and cosine (GRHIP_MODE_GENERIC)
int costas_launch(int order, bool fast_nco, const CarrierLaunch &a, hipStream_t st);

}  // namespace grhip
