// pfb_synth.h -- launcher of the polyphase synthesis filterbank kernels (csrc/pfb_synth.hip), used by
// csrc/capi_pfbsynth.hip for gr_pfb_synthesis_filterbank_ccf.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace grhip {

constexpr int SY_MAX_CHANS = 256;           // numchans the kernels take (the general path's DFT is the direct M x M sum)
constexpr int SY_MAX_TPF = 1 << 16;         // taps per branch
constexpr int SY_FUSED_MAX_CHANS = 16;      // fused kernel: 2 <= M <= 16, tpf <= 513, while its tile fits the LDS
constexpr size_t SY_LDS_MAX = 160 * 1024;

// One call of the block.  Output vector n (0 <= n < nvec) of the call: bin i is item n + i of its stream (the
// reference's `(in+i)[n]`), V_n = forward DFT of the bins, branch f is fed u_f[n] = V_n[M-1-f] and writes
// out[n*M + f] = sum_q h_f[q] u_f[n-q].  u_f[-k] (k = 1 .. tpf-1) is what the branch's delay line holds from earlier
// calls: row tpf-1-k of state_old (oldest first).  The launch leaves the same rows for the next call in state_new (another buffer).
struct PfbSynthArgs {
    int M = 1, tpf = 1, numsigs = 1;
    const float2 *in = nullptr;         // stream s at in + s*stride, in_items readable items each
    long long stride = 0, in_items = 0;
    float2 *out = nullptr;              // nvec*M items
    long long nvec = 0;
    const float *taps_rev = nullptr;    // [M][tpf], branch f reversed: taps_rev[f*tpf + k] = h_f[tpf-1-k]
    const float *taps_t = nullptr;      // [tpf][M], the same transposed: taps_t[k*M + f] (general path)
    const float2 *tw = nullptr;         // [M] e^{-2 pi j k/M}, quarter turns exact
    const float2 *state_old = nullptr;  // [tpf-1][M]: row j, column f = u_f[j - (tpf-1)]
    float2 *state_new = nullptr;
    float2 *scratch = nullptr;          // general path: [tpf-1 + nvec][M] branch inputs
};

// whether (M, tpf) runs on the fused kernel (decided by the shape alone, never by the call's size)
bool pfb_synth_fused(int M, int tpf);

int launch_pfb_synth(const PfbSynthArgs &a, bool generic, hipStream_t st);

}  // namespace grhip
