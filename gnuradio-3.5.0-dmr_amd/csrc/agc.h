// agc.h -- launchers of the gain loops (internal): gr_agc_cc, gr_agc_ff, gr_agc2_cc and gr_agc2_ff.
#pragma once
#include <hip/hip_runtime.h>

#include "grhip_internal.h"

namespace grhip {

// the chunked form of agc_cc / agc_ff cuts a call's item axis into chunks of AGC_CHUNK items, from the call's first item
constexpr int AGC_CHUNK = 256;

enum { AGC_LAW_AGC = 0, AGC_LAW_AGC2 = 1 };

// gri_agc_cc.h:69-72 / gri_agc2_cc.h:84-88; `rate` is _rate for agc and _attack_rate for agc2, `decay` is agc2's alone
struct AgcParams {
    float rate, decay, reference, max_gain;
};

struct AgcLaunch {
    const void *in;         // [S][n] gr_complex (cc) or float
    void *out;              // [S][n]; must not overlap in
    int n, nstreams;
    bool cc;
    int law;
    AgcParams p;
    float *gain;            // [S]: _gain of every stream, read at the start and written at the end
};

// true where the chunked form may run: the law is agc's, the call is longer than one chunk, and rate, reference and
// max_gain are finite with rate >= 0 and reference >= 0 (the clamp-affine form needs b = rate * reference >= 0)
bool agc_can_chunk(const AgcLaunch &a);
// bytes of scratch the chunked form needs: the chunks' triples, flags and start gains (the serial walk needs none)
size_t agc_scratch_bytes(const AgcLaunch &a);
// chunked: the three passes of agc.hip (only where agc_can_chunk); otherwise the serial walk, bit for bit the reference
int agc_launch(bool chunked, const AgcLaunch &a, void *scratch, hipStream_t st);

}  // namespace grhip
