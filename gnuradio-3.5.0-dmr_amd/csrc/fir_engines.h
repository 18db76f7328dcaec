// fir_engines.h -- the fast engines of the FIR family behind one handle: the plan (fir_plan.h), the device operands of
// every engine the plan uses, and one build and one launch function per engine (capi_fir.hip).  gr_fir_filter,
// gri_fir_filter_with_buffer and XlatingCore each hold one.
#pragma once
#include "fir_kernels.h"
#include "fir_plan.h"
#include "grhip_internal.h"

namespace grhip {

// what every engine launch is given.  x item 0 = input[0] of output 0; items with index < n_lo or >= n_in read as zero.
// Several streams: stream s at x + s * x_stride, its outputs at out + s * out_stride.
struct FirIo {
    const void *x;
    long long n_in, n_out;
    void *out;
    int n_streams = 1;
    long long x_stride = 0, n_lo = 0, out_stride = 0;
    int parity() const { return (int)((((uintptr_t)x) >> 3) & 1); }    // of the stream's 16-byte alignment (complex items)
};

struct FirEngines {
    FirPlan plan;
    int ntaps = 0, decim = 1;
    DevBuf d_hp; int Tq = 0;                        // tiled kernel: phase-major taps [tiled_decim][Tq]
    SchedBuf sched;                                 // its tile queue (one launch at a time per handle)
    DevBuf d_mf_A[2]; int mf_kexp = 0;              // matrix-core engine: operand tables [alignment parity], tap scale
    SchedBuf mf_sched;
    DevBuf d_ols_tw, d_ols_H; int ols_L = 0, ols_fold = 0;     // overlap-save engine: twiddles, spectrum of the taps
    DevBuf d_hidec_taps;                            // high-decimation kernel: padded taps
    DevBuf d_ri_hp; int ri_Tq = 0;                  // real-input kernel: phase-major taps

    // the kernels' limits for a shape, and the diagnostic knobs (fir_plan.h)
    static FirCaps caps(int ntaps, int decim, int tiled_decim);
    static FirTuning tuning();

    // One build step per engine.  c: the taps in correlation order (c[k] multiplies x[nD + k]), tw floats per tap.
    int build_tiled(const float *c, int tw);
    int build_mfma(const float *c, float fwT0 = 0.f);          // fwT0 != 0: freq_xlating's pre-mix form (mfma_tables.h)
    int build_ols(const float *c, int tw);
    int build_hidec(const float *c, int tw);
    int build_realin(const float *c);
    // gr_fir_filter's engines for `kind`: the plan and every engine it uses.  rev: the reversed taps (correlation order)
    int build_plain(FirKind kind, int decimation, const float *rev, int n);

    // One launch per engine.  The caller hands in the argument struct with what belongs to it (pre-mix tables, carries,
    // gain); the common part -- input, counts, strides, alignment parity and operand table, vec_store, tile queue --
    // is filled in here.
    int launch_mfma(FirMfmaArgs a, const FirIo &io, bool premix, int epi, hipStream_t st);
    int launch_tiled(FirTiledArgs a, const FirIo &io, bool ctaps, bool premix, int epi, hipStream_t st);
    int launch_hidec(bool ctaps, const FirIo &io, const float2 *gtab, const float2 *etab, const float2 *vtab, hipStream_t st);
    int launch_ols(bool real_data, const FirIo &io, hipStream_t st);       // history in front of io.x = the engine's previous samples
    int launch_realin(bool in_short, const FirIo &io, const float2 *gtab, hipStream_t st);
    // a call of gr_fir_filter (ekind fff / ccf / ccc / fcc / scc) by the plan's route; taps_rev: for the generic kernel
    int run_plain(FirKind ekind, int mode, const float *taps_rev, const void *d_in, void *d_out, long long n, int dec, hipStream_t st);
};

}  // namespace grhip
