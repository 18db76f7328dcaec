// squelch.h -- launchers of the power squelch blocks (internal): gr_pwr_squelch_cc, gr_pwr_squelch_ff and
// gr_simple_squelch_cc.
#pragma once
#include <hip/hip_runtime.h>

#include "grhip_internal.h"

namespace grhip {

// FAST detector: the item axis is cut into chunks of SQ_CHUNK items (a whole number of 64-bit flag words), as
// single_pole_iir's FAST form does (spectrum.h), with the state and the carry in double.
constexpr int SQ_CHUNK = 256;
constexpr int SQ_MAX_RAMP = 1 << 24;            // the envelope table holds ramp + 1 doubles

// the reference's enum order (general/gr_squelch_base_cc.h:37)
enum { SQ_MUTED = 0, SQ_ATTACK = 1, SQ_UNMUTED = 2, SQ_DECAY = 3 };

// what one stream remembers between calls (gr_squelch_base_cc.h:33-37 and the detector's previous output)
struct SquelchState {
    double y;               // gr_single_pole_iir's d_prev_output
    double envelope;        // d_envelope
    int state;              // d_state
    int ramped;             // d_ramped
};

// the machine as it stands in front of the first sample of a 64-sample flag word, and where that sample's output goes
struct SquelchEntry {
    double envelope;
    int state, ramped;
    int off;                // items the stream has emitted in this call before the word (gating)
    int pad;
};

struct SquelchLaunch {
    const void *in;         // [S][n] gr_complex (cc) or float
    void *out;              // stream s from out + s * n items; must not overlap in
    int *produced;          // [S]
    int n, nstreams;
    bool cc, simple, gate;
    int ramp;
    double alpha, threshold;
    SquelchState *state;    // [S]
    const double *table;    // 0.5 - cos((M_PI * k) / ramp) / 2.0 for k = 0 .. table_len - 1 (ramp > 0)
};

// bytes of scratch one call needs: flag words, word entries, chunk ends and starts
size_t squelch_scratch_bytes(bool fast, const SquelchLaunch &a);
int squelch_launch(bool fast, const SquelchLaunch &a, void *scratch, hipStream_t st);

// The tail of a call on its own, for a block with another detector (ctcss.hip): walk or scan, then emit.  The caller has
// written the mute bits of sample i of stream s to bit (i & 63) of word s * nwords + (i >> 6), nwords = (n + 63) / 64, at the
// head of `scratch` (squelch_tail_scratch_bytes of it: the words, then the entries), and, where there is neither ramp
// nor gating, state[s].state (the last flag) and produced[s] = n, which nothing downstream would write.
size_t squelch_tail_scratch_bytes(const SquelchLaunch &a);
int squelch_tail_launch(const SquelchLaunch &a, void *scratch, hipStream_t st);

}  // namespace grhip
