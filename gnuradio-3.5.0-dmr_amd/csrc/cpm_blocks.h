// cpm_blocks.h -- launchers of the continuous-phase transmitter's kernels (csrc/cpm.hip): gr_frequency_modulator_fc,
// gr_bytes_to_syms, gr_char_to_float, gr_chunks_to_symbols_bf and the fused modulator of cpmmod_bc / gmsk_mod.  Used by
// csrc/capi_cpm.hip.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace grhip {

constexpr int FM_THREADS = 256;
constexpr int FM_PER = 8;                       // consecutive items of a tile per lane
constexpr int FM_TILE = FM_THREADS * FM_PER;    // items per workgroup of the scan

inline long long fm_tiles(long long n) { return (n + FM_TILE - 1) / FM_TILE; }

// S streams back to back: in [S][n] floats, out [S][n] complex; phase one double per stream, read and left as the
// reference's d_phase after a work call of n items (the wrap of gr_frequency_modulator_fc.cc:66-69 included).
// The serial walk: one wavefront per stream, the reference's statements.
int fm_walk_launch(const float *in, float2 *out, long long n, int nstreams, double sensitivity, double *phase, hipStream_t st);
// The scan: `scratch` holds nstreams * fm_tiles(n) doubles (unused where n <= FM_TILE: one launch).
int fm_scan_launch(const float *in, float2 *out, long long n, int nstreams, double sensitivity, double *phase, double *scratch,
                   hipStream_t st);

// What the fused modulator reads in place of frequency samples: per stream n_in bytes at in + s * n_in, each one
// symbol (float)(signed char) (cpmmod_bc) or, with `bits`, eight symbols -1 / +1, MSB first (gmsk_mod); hist [S][nt - 1]
// the symbols in front of the call (left up to date); rows the taps of cpm.h's cpm_filter_rows.  Output o of a call is
// filter o % sps at symbol o / sps, summed in gr_fir_fff_generic's order.  freq: null, or [S][n] for the frequency
// samples.
struct CpmFused {
    const unsigned char *in = nullptr;
    long long n_in = 0;
    bool bits = false;
    float *hist = nullptr;
    const float *rows = nullptr;
    int sps = 1, nt = 1;
    float *freq = nullptr;
};
// n = outputs per stream (symbols * sps); needs cpm_fused_fits(sps, nt); scratch as for fm_scan_launch
int cpm_fused_launch(const CpmFused &src, float2 *out, long long n, int nstreams, double sensitivity, double *phase, double *scratch,
                     hipStream_t st);
// hist [S][nt - 1] <- the last nt - 1 symbols of (hist, the call's nsym symbols); one lane per stream
int cpm_history_launch(const CpmFused &src, long long nsym, int nstreams, hipStream_t st);

// ---- one lane per output item; strides in items ---------------------------------------------------------------------------
// out[s][8 i + b] = bit 7 - b of in[s][i] as -1 / +1 (gr_bytes_to_syms.cc:57-68)
int bytes_to_syms_launch(const unsigned char *in, long long in_stride, float *out, long long out_stride, long long n_bytes, int nstreams,
                         hipStream_t st);
// out[s][i] = (float)(signed char)in[s][i] (gri_char_to_float.cc:26-40)
int char_to_float_launch(const unsigned char *in, long long in_stride, float *out, long long out_stride, long long n, int nstreams,
                         hipStream_t st);
// out[i D + d] = table[in[i] D + d], zeros where the D entries do not lie inside the table (as chunks_to_symbols_bc)
int chunks_to_symbols_bf_launch(const unsigned char *in, float *out, long long n, const float *table, unsigned table_size, unsigned D,
                                hipStream_t st);

}  // namespace grhip
