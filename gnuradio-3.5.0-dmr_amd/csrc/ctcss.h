// ctcss.h -- launcher of gr_ctcss_squelch_ff's detector (internal): three Goertzel filters over the same samples, one
// decision per block of len samples, expanded into the mute bits that squelch.hip's walk and emit read.
#pragma once
#include <hip/hip_runtime.h>

#include "squelch.h"

namespace grhip {

constexpr int CTCSS_MAX_LEN = 1 << 20;

// Every stream has taken the same number of samples since the last restart, so the length of the unfinished block is
// one number for the whole handle and the host keeps it.
struct CtcssLaunch {
    int len;                    // samples per decision
    int pending;                // samples of the unfinished block in `carry`, 0 .. len - 1, the same for every stream
    float level;
    float wr[3], wi[3];         // left guard, tone, right guard (gri_goertzel's d_wr, d_wi)
    const float2 *tab;          // FAST: [3][len], goertzel_build_table of each tone
    float *carry;               // [S][len]: the raw samples of every stream's unfinished block
    unsigned char *mute;        // [S]: every stream's last decision (d_mute)
};

// blocks that complete in a call of n samples per stream
inline long long ctcss_blocks(const CtcssLaunch &c, int n) { return ((long long)c.pending + n) / c.len; }

// The scratch of a call: squelch_tail_scratch_bytes(a), then a decision byte and the three magnitudes (|l|, |c|, |r|) of
// every block that completes in it, [S][blocks] each.  ctcss_magnitudes_offset is where the magnitudes start.
size_t ctcss_scratch_bytes(const CtcssLaunch &c, const SquelchLaunch &a);
size_t ctcss_magnitudes_offset(const CtcssLaunch &c, const SquelchLaunch &a);

// One call: a.in / a.out / a.produced / a.n / a.nstreams / a.ramp / a.gate / a.state / a.table as for squelch_launch
// (floats; cc, simple, alpha and threshold are not read).  Evaluates the blocks that complete, stores the new tail and
// the last decision, writes the flag words and runs squelch_tail_launch.
int ctcss_launch(bool fast, const CtcssLaunch &c, const SquelchLaunch &a, void *scratch, hipStream_t st);

}  // namespace grhip
