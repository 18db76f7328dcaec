// xlating_core.h -- host-side state of gr_freq_xlating_fir_filter_ccc shared by
// the plain block handle, the fused xlating->demod block and the DMR chain.
//
// Reference: filter/gr_freq_xlating_fir_filter_XXX.cc.t:46-123, gr_rotator.h:29-52.
//
// The rotator phase is a serial float recurrence that is data independent
// (SURVEY F4/H1): its value for output k depends only on (phase_incr, k).  It is
// generated once on the host with the exact recurrence, kept in HBM as a table
// (8 bytes per output), extended on demand while a stream runs and reused by
// every capture that starts from a fresh block (reset()).
#pragma once
#include <complex>
#include <cstdlib>
#include <vector>

#include "fir_engines.h"
#include "grhip_internal.h"

namespace grhip {

struct XlatingCore {
    // parameters
    int decim = 1;
    std::vector<std::complex<float>> proto;
    double center_freq = 0, sampling_freq = 1;

    // set before build(): the handle only ever demodulates (xlating_demod, dmr_chain).  Its plan then prefers the
    // engines with a fused demodulator (fir_plan_xlating)
    bool for_demod = false;
    // set before build(): the items the handle reads -- 0 complex (ccc, ccf), 1 float (fcf, fcc), 2 int16 (scf, scc).
    // Real items run the inner gr_fir_fcc / gr_fir_scc (fir_realin.hip, or the generic-order kernel) + rotator table;
    // build() then skips the complex-input engines' tables
    int in_kind = 0;
    // set before build(): the prototype taps are float (?cf kinds), so proto[i] * exp(...) is float * complex = (a*c, a*d)
    bool real_tap_type = false;
    // built by build()
    int ntaps = 0;
    std::vector<std::complex<float>> ctaps;     // composite taps, reference arithmetic
    std::complex<float> incr{1.f, 0.f};         // normalised d_phase_incr
    double omega = 0;                           // (double)(float)fwT0
    DevBuf d_taps_generic;                      // ctaps (d_taps order of the inner gr_fir_ccc)
    FirEngines eng;                             // the plan and the fast engines' operands
    // what only a frequency-translating filter has: the phasor tables of the pre-mix forms (real prototype)
    DevBuf d_wtab, d_stab, d_vtab;              // tiled kernel
    DevBuf d_hidec_etab, d_hidec_vtab;          // high-decimation kernel
    float mf_wstep[2] = {1.f, 0.f};             // matrix-core engine
    DevBuf d_mf_wlane[2], d_mf_stab, d_mf_vtab; // [alignment parity]
    int mf_cu_cap = 0;                          // FirMfmaArgs::max_cus of the next launches (the chain's masked FIR stream)
    int mf_wg_cap = 0;                          // FirMfmaArgs::max_wg_per_cu of the next launches (the chain's pipeline sets 1)
    DevBuf scratch_y;

    // rotator table: phases of outputs [tab_start, tab_start+tab_len)
    long long pos = 0;                          // outputs produced since construction/reset
    long long tab_start = 0, tab_len = 0;
    std::complex<float> gen_phase{1.f, 0.f};    // generator state at tab_start+tab_len
    unsigned gen_counter = 0;
    std::complex<float> built_incr{0.f, 0.f};
    DevBuf d_rot;

    int build(int device);
    // set_center_freq/set_taps path: new taps and increment, rotator phase and
    // counter carry on (only set_phase_incr is called, .cc.t:82)
    int rebuild_keep_phase(int device)
    {
        std::complex<float> ph(1.f, 0.f);
        unsigned cnt = 0;
        long long tab_end = tab_start + tab_len;
        if (pos == tab_end) { ph = gen_phase; cnt = gen_counter; }
        else if (pos >= tab_start && pos < tab_end) {
            hipError_t e = hipMemcpy(&ph, d_rot.as<std::complex<float>>() + (pos - tab_start), sizeof(ph),
                                     hipMemcpyDeviceToHost);
            if (e != hipSuccess) return fail(GRHIP_ERUNTIME, "rotator state readback failed");
            cnt = gen_counter - (unsigned)(tab_end - pos);
        }
        long long keep_pos = pos;
        int rc = build(device);          // resets pos and the table
        if (rc) return rc;
        pos = keep_pos; tab_start = keep_pos; tab_len = 0;
        gen_phase = ph; gen_counter = cnt;
        return GRHIP_OK;
    }
    void reset();
    int ensure_rot(long long n, const float2 **gtab, hipStream_t st);
    int phase_before_pos(std::complex<float> *g);
    // the frame of the demodulator's carried sample, chosen before pointers or lengths are known: true = the fused
    // demodulator on the pre-mixed accumulators (EPILOGUE_DEMOD_FUSED, composite frame)
    bool demod_is_direct(int mode, bool demod, bool batched = false) const
    {
        FirCall c;
        c.mode = mode; c.demod = demod; c.batched = batched;
        return fir_route(eng.plan, c).epilogue == EPILOGUE_DEMOD_FUSED;
    }
    // the demodulator as a second kernel: fir(y, y_stride) writes the FIR's outputs behind one carried sample per stream
    template <class Fir>
    int demod_second(const FirIo &io, float gain, const float2 *y_prev, float2 *y_last, const float *atan_tab, hipStream_t st,
                     Fir &&fir);
    // d_in item 0 = input[0] of output 0 (oldest history item); items with index
    // < n_lo or >= n_in read as zero.  n_streams > 1: stream s at d_in + s*x_stride,
    // outputs at d_y/d_demod + s*out_stride, y_prev[s] / y_last[s].
    int run(int mode, const float2 *d_in, long long n_in, long long n_out, float2 *d_y, float *d_demod,
            float gain, const float2 *y_prev, float2 *y_last, const float *atan_tab, hipStream_t st,
            int n_streams = 1, long long x_stride = 0, long long n_lo = 0, long long out_stride = 0);
};

}  // namespace grhip
