// fm_demod.h -- launchers of the FM demodulator hier block (internal): blks2.fm_demod_cf / blks2.nbfm_rx,
// gr_quadrature_demod_cf -> fm_deemph (one gr_iir_filter_ffd) -> gr_fir_filter_fff(audio_decim, audio_taps).
#pragma once
#include <hip/hip_runtime.h>

#include "grhip_internal.h"

namespace grhip {

constexpr int FMD_TILE = 8192;          // input samples per workgroup of the fused kernel
constexpr int FMD_MAX_HIST = 1024;      // ntaps - 1 the fused kernel takes
constexpr int FMD_SLOTS = 12288;        // floats of LDS: FMD_MAX_HIST + FMD_TILE + FMD_TILE / 8 + FMD_MAX_HIST and one word of padding per 64

// what a stream carries from call to call, one entry (or row) per stream
struct FmdState {
    float2 *last;       // [S]: the last complex sample
    float *xs;          // [S][IIR_HIST]: the de-emphasis filter's last input (entry 0)
    double *ys;         // [S][IIR_HIST]: its last accumulator (entry 0)
    float *hist;        // [S][H]: the last H = ntaps - 1 de-emphasised floats, oldest first
};

// ---- the pieces of the composed path ------------------------------------------------------------------------------
// q[s * q_stride + i] = gain * atan2 of in[s][i] conj(in[s][i - 1]), in[s][-1] = last[s]: gr_quadrature_demod_cf.cc:57-59
int fmd_demod_launch(const float2 *in, int n_in, int nstreams, float gain, const float *atan_tab, const float2 *last, float *q,
                     long long q_stride, hipStream_t st);
// row[s * row_stride + k] = hist[s][k], k < H: the FIR's delay line in front of the call's de-emphasised samples
int fmd_hist_in_launch(const float *hist, int H, int nstreams, float *row, long long row_stride, hipStream_t st);
// after the call: last[s] = in[s][n_in - 1], hist[s][k] = row[s * row_stride + n_in + k], *d_produced = produced (if not null)
int fmd_tail_launch(const float2 *in, int n_in, int nstreams, const float *row, long long row_stride, int H, float2 *last,
                    float *hist, int *d_produced, int produced, hipStream_t st);

// ---- the fused kernel ---------------------------------------------------------------------------------------------
struct FmdFused {
    const float2 *in;       // [S][n_in]
    float *out;             // [S][produced]
    int n_in, nstreams;
    int produced, o0, D;    // output j of the call sits on its item o0 + j D
    int ntaps;              // 1 .. FMD_MAX_HIST + 1
    const float *taps;      // device, forward order: taps[k] multiplies the de-emphasised sample k items back
    float gain;
    const float *atan_tab;
    int deemph;             // 0: no de-emphasis (the FIR reads the demodulator's output)
    double b0, b1, a1;      // y[t] = b0 q[t] + b1 q[t-1] + a1 y[t-1]
    int W0;                 // warm-up items in front of a tile that does not reach the call's start; >= 1 with deemph
    FmdState rd, wr;        // state read by the first tile, written by the last (two copies: tiles run in any order)
    int *d_produced;        // or null
};
int fmd_fused_launch(const FmdFused &a, hipStream_t st);

}  // namespace grhip
