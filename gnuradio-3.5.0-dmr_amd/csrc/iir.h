// iir.h -- launchers of gr_iir_filter_ffd (internal): the direct-form-I recurrence of filter/gri_iir.h:126-163.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "grhip_internal.h"

namespace grhip {

// the chunked form cuts a call's item axis into chunks of IIR_CHUNK items, from the call's first item
constexpr int IIR_CHUNK = 256;
constexpr int IIR_MAX_TAPS = 64;        // on either side
constexpr int IIR_MAX_K = 8;            // feedback order (m - 1) the chunked form takes
constexpr int IIR_HIST = IIR_MAX_TAPS;  // stride of one stream's delay line, inputs and outputs alike

// C^IIR_CHUNK, C the K x K companion matrix of the feedback taps, row-major in an 8 x 8 frame.  (The power for the
// short last chunk is not needed: the state a call leaves is the one the last chunk's walk ends in.)
struct IirCarry {
    double full[IIR_MAX_K * IIR_MAX_K];
};

struct IirLaunch {
    const float *in;        // stream s at in + s * in_stride
    float *out;             // stream s at out + s * out_stride; must not overlap in
    long long in_stride, out_stride;    // items between streams (n_items where they lie back to back)
    int n_items, nstreams;
    int n, m;               // feed-forward and feedback tap counts (n >= 1, m >= 1)
    const double *taps;     // device: ff[IIR_MAX_TAPS] then fb[IIR_MAX_TAPS]
    float *xstate;          // [S][IIR_HIST]: xstate[k] = the input k + 1 items before the next call's first (k < n - 1)
    double *ystate;         // [S][IIR_HIST]: the same for the outputs, in double (the reference's d_prev_output; k < m - 1)
};

// whether the chunked form may run these taps (K <= IIR_MAX_K, every tap finite, max over j = 1 .. IIR_CHUNK of
// ||C^j||_inf <= 64), and C^IIR_CHUNK if so (`out` may be null)
bool iir_plan(const std::vector<double> &ff, const std::vector<double> &fb, IirCarry *out);
// bytes of scratch the chunked form needs: every chunk's zero-state end and true start, IIR_MAX_K doubles each
size_t iir_scratch_bytes(const IirLaunch &a);
// the serial walk, one wavefront per stream: bit for bit the reference
int iir_walk_launch(const IirLaunch &a, hipStream_t st);
// the passes of iir.hip's chunked form; needs n_items > IIR_CHUNK and m - 1 <= IIR_MAX_K
int iir_chunked_launch(const IirLaunch &a, const IirCarry &c, void *scratch, hipStream_t st);

}  // namespace grhip
