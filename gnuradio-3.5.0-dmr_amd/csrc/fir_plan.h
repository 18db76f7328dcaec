// fir_plan.h -- which engine runs a call of the FIR family, decided in one place.
//
// Plain C++: no HIP header, no device.  The kernels' own limits come in as data (FirCaps, filled by the callers from
// tiled_supported / mfma_supported / hidec_supported / realin_supported); everything else that chooses an engine -- the
// measured crossovers, the rules of a demodulating handle, the per-call conditions -- is here and nowhere else.
// host/fir_plan_test.cc runs it on the CPU.
#pragma once
#include <cstring>

#include "../../include/grhip.h"

namespace grhip {

inline bool mode_valid(int m) { return m == GRHIP_MODE_FAST || m == GRHIP_MODE_GENERIC || m == GRHIP_MODE_FAST_VALU || m == GRHIP_MODE_FAST_REFTAPS; }
inline bool mode_fast(int m) { return m != GRHIP_MODE_GENERIC; }          // FAST, FAST_VALU or FAST_REFTAPS
inline bool mode_matrix(int m) { return m == GRHIP_MODE_FAST || m == GRHIP_MODE_FAST_REFTAPS; }   // matrix cores allowed

enum FirKind { FIR_FFF = 0, FIR_CCF = 1, FIR_CCC = 2, FIR_FCC = 3, FIR_SCC = 4, FIR_FSF = 5 };
// complex taps (interleaved): ccc and the real-input kinds with complex output
inline bool fir_kind_ctaps(FirKind k) { return k == FIR_CCC || k == FIR_FCC || k == FIR_SCC; }
inline bool fir_kind_parse(const char *s, FirKind *k)
{
    static const char *const names[] = {"fff", "ccf", "ccc", "fcc", "scc", "fsf"};
    for (int i = 0; i < 6; ++i)
        if (!strcmp(s, names[i])) { *k = (FirKind)i; return true; }
    return false;
}

// gr_fft_filter_ccc's fused overlap-save engine: 4096-point blocks, up to 2049 taps (fft_kernels.hip)
constexpr int OLS_N = 4096, OLS_MAX_TAPS = 2049;

// what the kernels take of a shape (decimation, tap count): the tiled kernel (at fir_tiled_decim()) with real and with
// complex taps, the matrix-core engine, the high-decimation direct kernel, the real-input kernel
struct FirCaps { bool tiled_real = false, tiled_cplx = false, mfma = false, hidec = false, realin = false; };

// diagnostic builds (-DGRHIP_DIAG) set these from GRHIP_HIDEC / GRHIP_OLS_MIN; -1: the measured rules
// hidec 0 / 1: the high-decimation kernel never / wherever it is supported (tools/bench_decim.py); ols_min: gr_fir_filter's
// tiled/engine crossover for both tap kinds (0: engine wherever it can, 9999: never; tools/bench_ols_crossover.py)
struct FirTuning { int hidec = -1, ols_min = -1; };

struct FirPlan {
    // xlating: freq_xlating (rotator epilogue, demodulator, batches); real_in: float / int16 items (the real-input kernel or
    // the generic one); fff: float data on the tiled kernel's float-pair mode (gr_fir_fff, gr_fir_fsf)
    bool xlating = false, real_in = false, fff = false;
    int tiled_decim = 0;        // decimation the tiled kernel runs at (0: not tried)
    bool use_tiled = false, premix = false;
    // FAST mode for the shapes the tiled kernel does not take (other decimations, long filters): the overlap-save engine
    // of gr_fft_filter_ccc (fft_kernels.hip), any decimation
    bool use_ols = false, prefer_ols = false;
    // ... the high-decimation direct kernel where a polyphase component has few taps (fir_kernels.hip)
    bool use_hidec = false, hidec_premix = false;
    // ... the matrix-core engine for long real-tap filters on complex data (fir_mfma.hip)
    bool use_mfma = false;
    bool use_realin = false;
};

// the decimation gr_fir_filter's tiled kernel runs at: float data runs the complex kernel on overlapped pairs at twice
// the decimation (0: no such instance)
inline int fir_tiled_decim(FirKind kind, int decim) { return kind != FIR_FFF && kind != FIR_FSF ? decim : decim <= 2 ? 2 * decim : 0; }

inline bool ols_in_range(int ntaps, int decim) { return ntaps >= 48 && ntaps <= OLS_MAX_TAPS && (OLS_N - (ntaps - 1)) / decim >= 1; }

// the matrix cores pay from 24 taps per polyphase component
inline bool mfma_wanted(const FirCaps &caps, int decim, int ntaps) { return caps.mfma && ntaps / decim >= 24; }

// the high-decimation direct kernel where it beats (or replaces) the overlap-save engine
inline bool hidec_wanted(const FirCaps &caps, const FirTuning &tn, int decim, int ntaps, bool ctaps, bool have_ols)
{
    if (!caps.hidec || tn.hidec == 0) return false;
    if (tn.hidec == 1 || !have_ols) return true;
    // MACs per input sample (complex taps count twice) against what the engine delivers for the shape
    // (profiles/r02_decim_engines.log, round 2's kernels on both sides): the direct kernel runs at roughly 400 Gsamples/s
    // at 8 MACs, 320-400 at 20, 250 at 40, 130-200 at 80; the engine at 330-400 where its inverse folds (decimation 8, 16),
    // 210-250 elsewhere up to ~500 taps, less for longer filters.
    const double w = (double)ntaps / decim * (ctaps ? 2.0 : 1.0);
    if (decim == 8 || decim == 16) return w <= 16.0;
    if (w <= 32.0) return true;
    return w <= 48.0 && ntaps <= 512 && decim >= 5;
}

// Taps per polyphase component above which the overlap-save engine takes over from the tiled vector kernel (single-stream
// calls).  Measured on MI355X (tools/bench_ols_crossover.py, profiles/r02_ols_crossover.log): the tiled kernel runs at
// about 15000 / (taps per phase) Gsamples/s with real taps and half that with complex taps, the engine (round 2:
// persistent, resident twiddles) at 230-290 whatever the filter.
inline int ols_crossover(const FirTuning &tn, bool complex_taps, int decim)
{
    if (tn.ols_min >= 0) return tn.ols_min;
    // measured crossovers (taps per phase): real taps 48 / 60 / 28 at decimation 1 / 2 / 4, complex taps 40 / 40 / 26
    // (the engine's folded inverse makes it fastest at 4, the full-size inverse of decimation 1 comes next)
    if (complex_taps) return decim >= 4 ? 26 : 40;
    return decim >= 4 ? 28 : decim == 2 ? 60 : 48;
}

// gr_fir_filter_{fff,ccf,ccc,fcc,scc,fsf}.  caps.tiled_* are those of fir_tiled_decim(kind, decim).
inline FirPlan fir_plan_plain(FirKind kind, int decim, int ntaps, const FirCaps &caps, const FirTuning &tn = FirTuning())
{
    FirPlan p;
    p.real_in = kind == FIR_FCC || kind == FIR_SCC;
    if (p.real_in) { p.use_realin = caps.realin; return p; }
    const FirKind ekind = kind == FIR_FSF ? FIR_FFF : kind;         // fsf runs fff's engines and converts
    p.fff = ekind == FIR_FFF;
    p.tiled_decim = fir_tiled_decim(kind, decim);
    p.use_tiled = ntaps > 0 && p.tiled_decim != 0 && (ekind == FIR_CCC ? caps.tiled_cplx : caps.tiled_real);
    p.use_mfma = ekind == FIR_CCF && mfma_wanted(caps, decim, ntaps);
    p.use_ols = ols_in_range(ntaps, decim);
    p.use_hidec = !p.use_tiled && !p.fff && hidec_wanted(caps, tn, decim, ntaps, ekind == FIR_CCC, p.use_ols);
    // (float data: the tiled kernel's float-pair mode runs at about 50000 / taps Gsamples/s, the real-data engine at
    // 250-290: the engine where the float-pair mode does not reach, and from 176 taps per phase on)
    p.prefer_ols = p.use_ols && (!p.use_tiled || ntaps / decim > (p.fff ? 176 : ols_crossover(tn, ekind == FIR_CCC, decim)));
    return p;
}

// gr_freq_xlating_fir_filter_XXX.  in_kind: the items read -- 0 complex, 1 float, 2 int16; real_proto: every prototype
// tap has a zero imaginary part; for_demod: the handle only ever demodulates (xlating_demod, dmr_chain).
inline FirPlan fir_plan_xlating(int in_kind, bool real_proto, bool for_demod, int decim, int ntaps, const FirCaps &caps,
                                const FirTuning &tn = FirTuning())
{
    FirPlan p;
    p.xlating = true;
    p.real_in = in_kind != 0;                   // real items: gr_fir_fcc / gr_fir_scc over the composite taps
    if (p.real_in) { p.use_realin = caps.realin; return p; }
    p.tiled_decim = decim;
    // real prototype: the pre-mix form, x'[u] = x[u] e^{jwu} under the real prototype taps
    if (ntaps > 0 && real_proto && caps.tiled_real) p.use_tiled = p.premix = true;
    else if (ntaps > 0 && caps.tiled_cplx) p.use_tiled = true;
    p.use_mfma = real_proto && mfma_wanted(caps, decim, ntaps);
    p.use_ols = ols_in_range(ntaps, decim);
    // single-stream calls only, batched launches stay tiled.  Not gr_fir_filter's crossover: behind the engine this block
    // still needs the rotator-table multiply and (fused form) the stand-alone demodulator as passes of their own, which
    // the tiled kernel does in its epilogue -- the round-1 crossover stays for real prototypes (the matrix-core engine
    // comes first there anyway); complex prototypes cost the tiled kernel twice the FMAs: measured 190 (tiled) against
    // 226 Gsamples/s (engine + rotator pass) at 64 taps per phase, D = 4
    p.prefer_ols = p.use_ols && (!p.use_tiled || ntaps / decim > (real_proto ? 120 : 56));
    // real prototype: pre-mix form, half the FMAs for one more multiply per staged sample -- pays from about 16
    // taps per polyphase component (tools/bench_decim.py)
    p.hidec_premix = real_proto && ntaps > 0 && ntaps / decim >= 16;
    p.use_hidec = !p.use_tiled && hidec_wanted(caps, tn, decim, ntaps, !p.hidec_premix, p.use_ols);
    if (for_demod && real_proto && ntaps > 0) {
        // A demodulating handle: whatever engine has the fused demodulator.  Those need no rotator phases, whose exact
        // recurrence is computed on the host at ~3 ns per output and bounds a STREAMING block on any other path
        // (measured: 1-8 Gsamples/s against 200-320)
        if (p.use_tiled && p.premix) p.prefer_ols = false;
        // (up to 1024 taps: beyond, the f32 direct sum of the pre-mixed products leaves the 1e-5 tolerance -- 1.04e-5 measured
        // at 1200 taps -- and the engine, with its host-side rotator phases, stays)
        else if (!p.use_tiled && ntaps <= 1024 && caps.hidec) p.use_hidec = p.hidec_premix = true;
    }
    return p;
}

// ---- the per-call route ------------------------------------------------------------------------------------------
// ENG_EINVAL: no engine takes the call (GRHIP_EINVAL); ENG_GENERIC: the generic-order kernel (bit-exact);
// ENG_GENERIC_DEMOD: generic-order FIR + rotator + demodulator in one kernel (bit-exact)
enum FirEngine { ENG_EINVAL, ENG_GENERIC, ENG_GENERIC_DEMOD, ENG_REALIN, ENG_TILED, ENG_MFMA, ENG_HIDEC, ENG_OLS };
// ROTATE: times the rotator's phase table; DEMOD_FUSED: the demodulator on the pre-mixed accumulators (EPI_DEMOD) -- no
// rotator phases, carry in the composite frame; DEMOD_SECOND: rotate, then the stand-alone demodulator over y
enum FirEpilogue { EPILOGUE_NONE, EPILOGUE_ROTATE, EPILOGUE_DEMOD_FUSED, EPILOGUE_DEMOD_SECOND };
struct FirRoute { FirEngine engine; FirEpilogue epilogue; bool need_rot; };     // need_rot: the call reads rotator phases

struct FirCall {
    int mode = GRHIP_MODE_FAST;
    bool demod = false;             // xlating: the output is the demodulator's
    bool batched = false;           // xlating: n_streams != 1 || n_lo != 0
    bool same_decim = true;         // gr_fir_filter: the call's decimation is the handle's (filterNdec may ask another)
    bool in_aligned = true, out_aligned = true;     // real items: input pointer item aligned (float 4, int16 2 bytes), output 8 bytes
    bool odd_stride_multi = false;  // several streams an odd number of items apart
    bool generic_fused = true;      // false: launch_fir_generic_demod has declined the shape (returned 1), ask again
    long long n = 2;                // outputs (float data: a single output has no pair)
};

inline FirRoute fir_route(const FirPlan &p, const FirCall &c)
{
    const bool fast = mode_fast(c.mode), matrix = mode_matrix(c.mode);
    const FirEpilogue plain = p.xlating ? EPILOGUE_ROTATE : EPILOGUE_NONE;
    if ((p.real_in || !p.xlating) && (c.demod || c.batched)) return {ENG_EINVAL, EPILOGUE_NONE, false};
    if (p.real_in)
        return {fast && p.use_realin && c.same_decim && c.in_aligned && c.out_aligned ? ENG_REALIN : ENG_GENERIC, plain, p.xlating};
    if (!p.xlating) {
        if (!c.same_decim) return {ENG_GENERIC, EPILOGUE_NONE, false};      // the operands are laid out for one decimation
        if (matrix && p.use_mfma) return {ENG_MFMA, EPILOGUE_NONE, false};
        // (gr_fir_fff: output pairs; a single output goes through the generic kernel)
        if (fast && p.use_tiled && !p.prefer_ols && (!p.fff || c.n >= 2)) return {ENG_TILED, EPILOGUE_NONE, false};
        if (fast && p.use_hidec) return {ENG_HIDEC, EPILOGUE_NONE, false};
        if (fast && p.use_ols && (p.prefer_ols || !p.use_tiled)) return {ENG_OLS, EPILOGUE_NONE, false};
        return {ENG_GENERIC, EPILOGUE_NONE, false};
    }
    const bool mfma_now = matrix && p.use_mfma && !c.odd_stride_multi;
    // fused demodulator of the high-decimation direct kernel (pre-mix form)
    const bool hidec_direct = !mfma_now && c.demod && fast && p.use_hidec && p.hidec_premix;
    // fused demodulator of the tiled kernel: FAST mode, real prototype taps (single-stream calls of a long filter go
    // through the overlap-save engine instead; batched launches -- several streams, or history supplied by range
    // check -- always take the tiled kernel)
    const bool direct = mfma_now ? c.demod
                                 : hidec_direct || (c.demod && fast && p.use_tiled && p.premix && (c.batched || !p.prefer_ols));
    const FirEpilogue epi = direct ? EPILOGUE_DEMOD_FUSED : c.demod ? EPILOGUE_DEMOD_SECOND : EPILOGUE_ROTATE;
    if (mfma_now) return {ENG_MFMA, epi, !direct};
    if (hidec_direct) return {ENG_HIDEC, epi, false};
    const bool ols_now = fast && (p.prefer_ols || (p.use_hidec && !p.use_tiled)) && !c.batched;
    if (fast && p.use_tiled && !ols_now) return {ENG_TILED, epi, !direct};
    if (ols_now) return {p.use_hidec ? ENG_HIDEC : ENG_OLS, epi, true};
    // generic order: the demodulator in the same kernel where there is one (that kernel also takes several streams and
    // synthesises a fresh capture's history), else as a second kernel over y
    if (c.demod && c.generic_fused) return {ENG_GENERIC_DEMOD, EPILOGUE_ROTATE, true};
    if (c.batched) return {ENG_EINVAL, EPILOGUE_NONE, false};
    return {ENG_GENERIC, epi, true};
}

// a demodulating batch (several captures, history by range check) has a fast engine in `mode`
inline bool fir_has_batched_engine(const FirPlan &p, int mode)
{
    FirCall c;
    c.mode = mode; c.demod = true; c.batched = true;
    const FirEngine e = fir_route(p, c).engine;
    return e == ENG_TILED || e == ENG_MFMA || e == ENG_HIDEC;
}

}  // namespace grhip
