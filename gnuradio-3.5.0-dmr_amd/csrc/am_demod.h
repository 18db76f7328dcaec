// am_demod.h -- launchers of the AM demodulator hier block (internal): blks2.am_demod_cf / demod_10k0a3e_cf,
// gr_complex_to_mag -> gr_add_const_ff(-1) -> gr_fir_filter_fff(audio_decim, audio_taps) (blks2impl/am_demod.py:42-58).
#pragma once
#include <hip/hip_runtime.h>

#include "grhip_internal.h"

namespace grhip {

constexpr int AMD_TILE = 4096;          // input samples per workgroup of the fused kernel
constexpr int AMD_MAX_HIST = 1024;      // ntaps - 1 the fused kernel takes
constexpr int AMD_R = 8;                // adjacent outputs a lane forms from one register window (audio_decim == 1)
constexpr int AMD_FRONT = 16;           // words in front of the delay line in LDS: the window of a zero-padded last tap block
constexpr int AMD_SLOTS = (AMD_FRONT + AMD_MAX_HIST + AMD_TILE) / AMD_R * (AMD_R + 1) + AMD_R + 1;   // one word of padding per AMD_R

// what a stream carries from call to call: the last H = ntaps - 1 values of v = |x| - 1, oldest first, [S][H].
// Zero at a stream's start: the FIR's delay line holds zeros of ITS input, not |0| - 1.
struct AmdState {
    float *hist;
};

// ---- the pieces of the composed path ------------------------------------------------------------------------------
// row[s * row_stride + k] = hist[s][k] (k < H) and row[s * row_stride + H + i] = (float)(|in[s][i]| - 1.0f)
int amd_v_launch(const float2 *in, int n_in, int nstreams, const float *hist, int H, float *row, long long row_stride, hipStream_t st);
// after the call: hist[s][k] = row[s * row_stride + n_in + k], *d_produced = produced (if not null)
int amd_tail_launch(int n_in, int nstreams, const float *row, long long row_stride, int H, float *hist, int *d_produced,
                    int produced, hipStream_t st);

// ---- the fused kernel ---------------------------------------------------------------------------------------------
struct AmdFused {
    const float2 *in;       // [S][n_in]
    float *out;             // [S][produced]
    int n_in, nstreams;
    int produced, o0, D;    // output j of the call sits on its item o0 + j D
    int ntaps;              // 1 .. AMD_MAX_HIST + 1
    const float *taps;      // device, forward order, zero-padded to a multiple of AMD_R entries
    AmdState rd, wr;        // state read by the tiles at the call's start, written by the last (two copies)
    int *d_produced;        // or null
};
int amd_fused_launch(const AmdFused &a, hipStream_t st);

}  // namespace grhip
