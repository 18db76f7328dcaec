// fll_band_edge.h -- launcher of the band-edge frequency-lock loop (internal): digital_fll_band_edge_cc.
#pragma once
#include <hip/hip_runtime.h>

#include "carrier.h"
#include "fll_taps.h"
#include "grhip_internal.h"

namespace grhip {

constexpr int FLL_WIN = CARRIER_WIN;            // steps of one stream that a wavefront holds in LDS at a time
constexpr int FLL_RING = 2048;                  // derotated samples kept in LDS: a power of two, >= FLL_MAX_TAPS - 1 + 64
// phase_wrap: this many trips of the reference's subtract loop each way, a double remainder beyond (fll_band_edge.hip)
constexpr int FLL_WRAP_TRIPS = 256;

struct FllLaunch {
    const float2 *in;           // [S][n] gr_complex
    float2 *out;                // [S][n] gr_complex; must not overlap in
    float *frq, *phs, *err;     // [S][n] floats each, or all three null
    int n, nstreams, fs;
    const float2 *lower, *upper;    // fs taps each, as the reference stores them (reversed)
    CarrierParams p;
    CarrierState *state;        // [S] phase and frequency, read at the start and written at the end
    float2 *xh;                 // [S][fs] the last fs inputs, oldest first
    float2 *dh;                 // [S][fs] the last fs - 1 derotated samples, oldest first (the last item of a row is unused)
};

// generic: the reference's arithmetic (GRHIP_MODE_GENERIC); otherwise the float NCO, fused products and tree sums
int fll_band_edge_launch(bool generic, const FllLaunch &a, hipStream_t st);

}  // namespace grhip
