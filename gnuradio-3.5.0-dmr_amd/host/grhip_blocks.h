// grhip_blocks.h -- drop-in gr_sync_block / gr_sync_decimator / gr_block subclasses
// over the C ABI of libgrhip.so.  One class per reference block, with the
// reference's factory signature, io_signature, history, relative rate, setter
// names and exception types:
//
//   grhip_fir_filter_ccf / _fff / _ccc      <- gr_fir_filter_XXX   (filter/gr_fir_filter_XXX.h.t:36-66)
//   grhip_freq_xlating_fir_filter_{ccc,ccf,fcf,fcc,scf,scc} <- gr_freq_xlating_fir_filter_XXX (the family handle)
//   grhip_quadrature_demod_cf                <- gr_quadrature_demod_cf (general/gr_quadrature_demod_cf.h)
//   grhip_clock_recovery_mm_ff               <- digital_clock_recovery_mm_ff (gr-digital/include/...h:44-92)
//   grhip_binary_slicer_fb                   <- digital_binary_slicer_fb
//   grhip_correlate_access_code_bb           <- digital_correlate_access_code_bb
//   gr_fft_vcc_hip (grhip_make_fft_vcc)       <- gr_fft_vcc_fftw, on the abstract gr_fft_vcc base (general/gr_fft_vcc.h:41-59)
//   grhip_fft_filter_ccc / _fff              <- gr_fft_filter_ccc / _fff (filter/gr_fft_filter_fff.cc:44-97)
//   grhip_fft_vfc                            <- gr_fft_vfc (general/gr_fft_vfc.cc:42-118)
//   grhip_pfb_channelizer_ccf                <- gr_pfb_channelizer_ccf (filter/gr_pfb_channelizer_ccf.h:115-178)
//   grhip_pfb_arb_resampler_ccf / _fff       <- gr_pfb_arb_resampler_ccf / _fff (filter/gr_pfb_arb_resampler_ccf.h:96-178)
//   grhip_fractional_interpolator_ff / _cc   <- gr_fractional_interpolator_ff / _cc (filter/gr_fractional_interpolator_ff.h:41-66)
//   grhip_interp_fir_filter_XXX              <- gr_interp_fir_filter_XXX (filter/gr_interp_fir_filter_XXX.h.t)
//   grhip_rational_resampler_base_XXX        <- gr_rational_resampler_base_XXX (filter/gr_rational_resampler_base_XXX.h.t)
//   grhip_pfb_interpolator_ccf               <- gr_pfb_interpolator_ccf (filter/gr_pfb_interpolator_ccf.h)
//   grhip_pfb_synthesis_filterbank_ccf       <- gr_pfb_synthesis_filterbank_ccf (filter/gr_pfb_synthesis_filterbank_ccf.h)
//   grhip_hilbert_fc / grhip_filter_delay_fc <- gr_hilbert_fc (filter/gr_hilbert_fc.h), gr_filter_delay_fc (filter/gr_filter_delay_fc.h)
//   grhip_goertzel_fc                        <- gr_goertzel_fc (filter/gr_goertzel_fc.h)
//   grhip_dc_blocker_ff / _cc                <- gr_dc_blocker_ff / _cc (filter/gr_dc_blocker_ff.h:60-100)
//   grhip_moving_average_XX                  <- gr_moving_average_XX (gengen/gr_moving_average_XX.h.t)
//   grhip_integrate_XX                       <- gr_integrate_XX (gengen/gr_integrate_XX.h.t)
//   gr_make_complex_to_mag_squared, gr_make_single_pole_iir_filter_ff, gr_make_nlog10_ff, gr_make_keep_one_in_n
//                                            <- the factories of the same names (general/gr_complex_to_xxx.h,
//                                               filter/gr_single_pole_iir_filter_ff.h, general/gr_nlog10_ff.h, general/gr_keep_one_in_n.h)
//   gr_make_logpwrfft_c / _f                 <- blks2.logpwrfft_c / _f (python/gnuradio/blks2impl/logpwrfft.py:26-154)
//   gr_make_pwr_squelch_cc / _ff, gr_make_simple_squelch_cc
//                                            <- the factories of the same names (general/gr_pwr_squelch_cc.h,
//                                               general/gr_pwr_squelch_ff.h, general/gr_simple_squelch_cc.h)
//   gr_make_ctcss_squelch_ff                 <- gr_make_ctcss_squelch_ff (general/gr_ctcss_squelch_ff.h)
//   digital_make_costas_loop_cc, gr_make_pll_freqdet_cf / _refout_cc / _carriertracking_cc
//                                            <- the factories of the same names (gr-digital/include/
//                                               digital_costas_loop_cc.h, general/gr_pll_*.h)
//   digital_make_fll_band_edge_cc            <- digital_make_fll_band_edge_cc (gr-digital/include/digital_fll_band_edge_cc.h)
//   gr_make_pfb_clock_sync_ccf               <- gr_make_pfb_clock_sync_ccf (filter/gr_pfb_clock_sync_ccf.h)
//   digital_make_constellation_bpsk / _qpsk / _dqpsk / _8psk / _calcdist / _psk / _rect, digital_make_constellation_decoder_cb,
//   digital_make_constellation_receiver_cb, gr_make_diff_decoder_bb, gr_make_map_bb
//                                            <- the factories of the same names (gr-digital/include/digital_constellation*.h,
//                                               general/gr_diff_decoder_bb.h, gr_map_bb.h); grhip_make_constellation_demod_cb
//                                               is generic_demod's tail behind timing recovery (generic_mod_demod.py:296-313)
//   grhip_make_packed_to_unpacked_bb / _unpacked_to_packed_bb, grhip_make_diff_encoder_bb, grhip_make_chunks_to_symbols_bc
//                                            <- gr_make_packed_to_unpacked_bb, gr_make_unpacked_to_packed_bb, gr_make_diff_encoder_bb,
//                                               gr_make_chunks_to_symbols_bc (gengen/gr_*_XX.h.t, general/gr_diff_encoder_bb.h), the
//                                               same arguments; grhip_make_generic_mod is digital.generic_mod
//                                               (generic_mod_demod.py:76-157) as one block
//   gr_make_scrambler_bb, gr_make_descrambler_bb, gr_make_additive_scrambler_bb
//                                            <- the factories of the same names (general/gr_scrambler_bb.h,
//                                               gr_descrambler_bb.h, gr_additive_scrambler_bb.h)
//   gr_make_frequency_modulator_fc, gr_make_bytes_to_syms, gr_make_char_to_float, grhip_make_chunks_to_symbols_bf
//                                            <- the factories of the same names (general/gr_frequency_modulator_fc.h,
//                                               gr_bytes_to_syms.h, gr_char_to_float.h, gengen/gr_chunks_to_symbols_XX.h.t)
//   digital_make_cpmmod_bc, digital_make_gmskmod_bc, grhip_make_gmsk_mod
//                                            <- digital_make_cpmmod_bc, digital_make_gmskmod_bc (gr-digital/lib) and
//                                               digital.gmsk_mod (gr-digital/python/gmsk.py:55-120), one block each;
//                                               grhip_cpm_phase_response_taps is gr_cpm::phase_response
//   fsm, trellis_make_encoder_XX, trellis_make_metrics_X, trellis_make_constellation_metrics_cf, trellis_make_viterbi_X,
//   trellis_make_viterbi_combined_XX
//                                            <- the class and the factories of the same names (gr-trellis/src/lib/fsm.h,
//                                               trellis_encoder_XX.h.t, trellis_metrics_X.h.t,
//                                               trellis_constellation_metrics_cf.h, trellis_viterbi_X.h.t,
//                                               trellis_viterbi_combined_XX.h.t)
//   gr_make_agc_cc / _ff, gr_make_agc2_cc / _ff
//                                            <- the factories of the same names (general/gr_agc_cc.h, gr_agc_ff.h,
//                                               gr_agc2_cc.h, gr_agc2_ff.h)
//   gr_make_iir_filter_ffd, gr_make_fm_deemph <- gr_make_iir_filter_ffd (filter/gr_iir_filter_ffd.h), blks2.fm_deemph
//   gr_make_fm_demod_cf, gr_make_nbfm_rx     <- blks2.fm_demod_cf / blks2.nbfm_rx (blks2impl/fm_demod.py, nbfm_rx.py), one block
//   grhip_optfir_low_pass_taps               <- optfir.low_pass (gnuradio/optfir.py:45-54), host arithmetic
//   gr_make_complex_to_mag                   <- gr_complex_to_mag
//   gr_make_am_demod_cf, gr_make_demod_10k0a3e_cf   <- blks2.am_demod_cf / demod_10k0a3e_cf (blks2impl/am_demod.py), one block
//   gr_make_demod_20k0f3e_cf, gr_make_demod_200kf3e_cf   <- the FM presets of blks2impl/fm_demod.py:74-111
//
// Ownership.  A C handle has one owner, grhip_detail::handle: move-only, null until a create call has filled it, and
// it calls the handle's destroy function exactly once.  A block derives from grhip_detail::block<GNU Radio base,
// handle type, destroy, set_mode>, which holds that owner as the member d_h (so a constructor that throws after
// create releases the handle, and no block can be copied), forwards the base's constructor arguments, and has
// set_mode, checked() and the work / general_work / forecast shapes that several blocks share.  A block keeps its
// constructor non-public, befriends grhip_detail::factory once, and its factory function calls factory::make.
// A macro here pastes names only: typedefs, a table of the grhip_NAME_* functions a template asks for, a one-line
// class with its constructor, the factory.  Code that does something lives in a template or a plain function.  Four
// families of two to four blocks (dc_blocker, integrate, the spectrum blocks, pwr_squelch) are still stamped as whole
// classes, where a template and its table would be longer: such a macro opens and closes its class itself, and every
// member in it, work included, forwards one call.  The header needs C++17 (host/Makefile builds with -std=c++17) and,
// of GNU Radio, only the constructors and members that gr_shim.h mirrors.
//
// output_multiple is the REFERENCE's for every block (1; nsamples for fft_filter_ccc; the
// channeliser's own), so a finite flowgraph produces exactly the items the reference block
// produces, tail included.  The scheduler then hands a block at most half a 64 KiB buffer per
// call (runtime/gr_block_executor.cc:76-78, runtime/gr_flat_flowgraph.cc:37,100): correct, but
// launch-bound on a GPU.  An application that streams can opt in to larger calls
// with grhip_set_batch_items(block, n) below: it multiplies output_multiple, which GNU Radio
// 3.5 honours when it sizes buffers (runtime/gr_flat_flowgraph.cc:102-104,118) -- at the
// documented price of every raised output_multiple in GNU Radio: when the upstream finishes,
// fewer than one multiple of outputs can no longer be requested and that tail is dropped
// (runtime/gr_block_executor.cc:335-348).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/grhip.h"
#include "gr_shim.h"

namespace grhip_detail {
// status -> the exception type the reference throws for the same precondition
inline void check(int rc)
{
    if (rc >= 0) return;
    std::string msg = std::string(grhip_strerror(rc)) + ": " + grhip_last_error();
    switch (rc) {
    case GRHIP_EINVAL: throw std::invalid_argument(msg);
    case GRHIP_ERANGE: throw std::out_of_range(msg);
    case GRHIP_ENOMEM: throw std::bad_alloc();
    default: throw std::runtime_error(msg);
    }
}

// the one owner of a C handle: null until a create call fills it through out(), released exactly once
template <class H, void (*DESTROY)(H *)> class handle {
    H *d_p = nullptr;
public:
    handle() {}
    explicit handle(H *p) : d_p(p) {}
    handle(handle &&o) noexcept : d_p(o.d_p) { o.d_p = nullptr; }
    handle &operator=(handle &&o) noexcept
    {
        if (this != &o) {
            reset();
            d_p = o.d_p;
            o.d_p = nullptr;
        }
        return *this;
    }
    handle(const handle &) = delete;
    handle &operator=(const handle &) = delete;
    ~handle() { reset(); }
    void reset()
    {
        if (d_p) DESTROY(d_p);
        d_p = nullptr;
    }
    H **out()                                       // what a create call takes; releases what was held before
    {
        reset();
        return &d_p;
    }
    H *get() const { return d_p; }
    operator H *() const { return d_p; }            // so that the C calls read grhip_xxx_work(d_h, ...)
};

// the one place that makes a block: every block class befriends it and keeps its constructor non-public
struct factory {
    template <class B, class... A> static boost::shared_ptr<B> make(A &&...a)
    {
        return gnuradio::get_initial_sptr(new B(std::forward<A>(a)...));
    }
};

// as many units of input as there are, cut so that no more than noutput_items come out of a block that keeps one
// unit in `every` (gr_keep_one_in_n.cc:80); produced(h, n) tells the count for n units without changing the state
template <class H, class F> inline int cut_to_output(H *h, F produced, int n, int noutput_items, int every)
{
    while (n > 0 && produced(h, n) > noutput_items) {
        const int over = produced(h, n) - noutput_items;
        n -= over > 1 ? (over - 1) * every : 1;
    }
    return n;
}

// the base of every block: BASE is the GNU Radio class and gets the constructor's arguments, d_h owns the handle
template <class BASE, class H, void (*DESTROY)(H *), auto SET_MODE = nullptr> class block : public BASE {
protected:
    handle<H, DESTROY> d_h;
    template <class... A> explicit block(A &&...a) : BASE(std::forward<A>(a)...) {}
    // the result of a C call, after check() has thrown for a failure
    static int checked(int r)
    {
        check(r);
        return r;
    }
    // forecast: every input needs the items that a C call answers for noutput_items
    template <class F> void forecast_each(F forecast, int noutput_items, gr_vector_int &req)
    {
        const int n = checked(forecast(d_h, noutput_items));
        for (size_t i = 0; i < req.size(); i++) req[i] = n;
    }
    // general_work over a C entry that reports the items it consumed
    template <class F>
    int work_consumed(F general_work, int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                      gr_vector_void_star &out)
    {
        int consumed = 0;
        int r = checked(general_work(d_h, noutput_items, ninput_items[0], in[0], out[0], &consumed));
        this->consume_each(consumed);
        return r;
    }
    // general_work that uses all the inputs and reports the outputs copied (gr_squelch_base_cc.cc:42-93)
    template <class F>
    int work_all_inputs(F work, int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                        gr_vector_void_star &out)
    {
        const int n = noutput_items < ninput_items[0] ? noutput_items : ninput_items[0];
        int produced = 0;
        check(work(d_h, n, in[0], out[0], &produced));
        this->consume_each(n);
        return produced;
    }
public:
    // numeric mode of the handle (GRHIP_MODE_*), for the blocks whose handle has one
    template <class F = decltype(SET_MODE), class = typename std::enable_if<!std::is_same<F, std::nullptr_t>::value>::type>
    void set_mode(int mode)
    {
        check(SET_MODE(d_h, mode));
    }
};
}  // namespace grhip_detail

// the base of the block over handle grhip_NAME, with and without the handle's set_mode
#define GRHIP_BLOCK(GRBASE, NAME) grhip_detail::block<GRBASE, grhip_##NAME, grhip_##NAME##_destroy, grhip_##NAME##_set_mode>
#define GRHIP_BLOCK_NO_MODE(GRBASE, NAME) grhip_detail::block<GRBASE, grhip_##NAME, grhip_##NAME##_destroy>
// one entry of a table of C functions: T::create is grhip_NAME_create
#define GRHIP_FN(NAME, F) static constexpr auto F = &grhip_##NAME##_##F

// opt-in batching (see the header comment): work() calls of n times the block's own output multiple
template <class BLOCK_SPTR> inline void grhip_set_batch_items(const BLOCK_SPTR &b, int n)
{
    if (n < 1) throw std::invalid_argument("grhip_set_batch_items: n must be >= 1");
    b->set_output_multiple(b->output_multiple() * n);
}

// ---------------------------------------------------------------------------
// gr_fir_filter_XXX
// ---------------------------------------------------------------------------
template <class IN, class OUT, class TAP> class grhip_fir_filter_base : public GRHIP_BLOCK_NO_MODE(gr_sync_decimator, fir_filter) {
protected:
    grhip_fir_filter_base(const char *name, const char *kind, int decimation, const std::vector<TAP> &taps,
                          int device)
        : block(name, gr_make_io_signature(1, 1, sizeof(IN)), gr_make_io_signature(1, 1, sizeof(OUT)), decimation)
    {
        grhip_detail::check(grhip_fir_filter_create(d_h.out(), kind, decimation, (const float *)taps.data(), taps.size(),
                                                    device));
        set_history(grhip_fir_filter_history(d_h));          // set_history(d_fir->ntaps()), .cc.t:51
    }
public:
    void set_taps(const std::vector<TAP> &taps)                // .cc.t:59-64
    {
        grhip_detail::check(grhip_fir_filter_set_taps(d_h, (const float *)taps.data(), taps.size()));
    }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int r = checked(grhip_fir_filter_work(d_h, noutput_items, in[0], out[0]));
        if (r == 0) set_history(grhip_fir_filter_history(d_h));   // taps changed: history may have too
        return r;
    }
};

#define GRHIP_FIR_CLASS(NAME, KIND, IN, OUT, TAP)                                                          \
    class NAME : public grhip_fir_filter_base<IN, OUT, TAP> {                                              \
        friend struct grhip_detail::factory;                                                               \
        NAME(int decimation, const std::vector<TAP> &taps, int device)                                     \
            : grhip_fir_filter_base<IN, OUT, TAP>(#KIND, &#KIND[11], decimation, taps, device) {}          \
    };                                                                                                     \
    typedef boost::shared_ptr<NAME> NAME##_sptr;                                                           \
    inline NAME##_sptr grhip_make_##KIND(int decimation, const std::vector<TAP> &taps, int device = 0)     \
    {                                                                                                      \
        return grhip_detail::factory::make<NAME>(decimation, taps, device);                                \
    }
// &"fir_filter_ccf"[11] == "ccf"
GRHIP_FIR_CLASS(grhip_fir_filter_ccf, fir_filter_ccf, gr_complex, gr_complex, float)
GRHIP_FIR_CLASS(grhip_fir_filter_fff, fir_filter_fff, float, float, float)
GRHIP_FIR_CLASS(grhip_fir_filter_ccc, fir_filter_ccc, gr_complex, gr_complex, gr_complex)
GRHIP_FIR_CLASS(grhip_fir_filter_fcc, fir_filter_fcc, float, gr_complex, gr_complex)
GRHIP_FIR_CLASS(grhip_fir_filter_scc, fir_filter_scc, short, gr_complex, gr_complex)
GRHIP_FIR_CLASS(grhip_fir_filter_fsf, fir_filter_fsf, float, short, float)
#undef GRHIP_FIR_CLASS

// ---------------------------------------------------------------------------
// gr_freq_xlating_fir_filter_{ccc,ccf,fcf,fcc,scf,scc}: one template over the family handle
// (filter/gr_freq_xlating_fir_filter_XXX.h.t:64-99, .cc.t:38-123)
// ---------------------------------------------------------------------------
template <class IN, class TAP>
class grhip_freq_xlating_fir_filter_blk : public GRHIP_BLOCK(gr_sync_decimator, freq_xlating_fir_filter) {
public:
    grhip_freq_xlating_fir_filter_blk(const char *name, const char *kind, int decimation, const std::vector<TAP> &taps,
                                      double center_freq, double sampling_freq, int device)
        : block(name, gr_make_io_signature(1, 1, sizeof(IN)), gr_make_io_signature(1, 1, sizeof(gr_complex)), decimation)
    {
        grhip_detail::check(grhip_freq_xlating_fir_filter_create(d_h.out(), kind, decimation, (const float *)taps.data(),
                                                                 taps.size(), center_freq, sampling_freq, device));
        set_history(grhip_freq_xlating_fir_filter_history(d_h));
    }
    void set_center_freq(double f) { grhip_detail::check(grhip_freq_xlating_fir_filter_set_center_freq(d_h, f)); }
    void set_taps(const std::vector<TAP> &taps)
    {
        grhip_detail::check(grhip_freq_xlating_fir_filter_set_taps(d_h, (const float *)taps.data(), taps.size()));
    }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int r = checked(grhip_freq_xlating_fir_filter_work(d_h, noutput_items, in[0], out[0]));
        if (r == 0) set_history(grhip_freq_xlating_fir_filter_history(d_h));   // set_history(ntaps), return 0 (.cc.t:109-114)
        return r;
    }
};
#define GRHIP_XLATING_CLASS(SUF, IN, TAP)                                                                          \
    typedef grhip_freq_xlating_fir_filter_blk<IN, TAP> grhip_freq_xlating_fir_filter_##SUF##_blk;                  \
    typedef boost::shared_ptr<grhip_freq_xlating_fir_filter_##SUF##_blk> grhip_freq_xlating_fir_filter_##SUF##_sptr; \
    inline grhip_freq_xlating_fir_filter_##SUF##_sptr grhip_make_freq_xlating_fir_filter_##SUF(                     \
        int decimation, const std::vector<TAP> &taps, double center_freq, double sampling_freq, int device = 0)     \
    {                                                                                                              \
        return grhip_detail::factory::make<grhip_freq_xlating_fir_filter_##SUF##_blk>(                            \
            "freq_xlating_fir_filter_" #SUF, #SUF, decimation, taps, center_freq, sampling_freq, device);         \
    }
GRHIP_XLATING_CLASS(ccc, gr_complex, gr_complex)
GRHIP_XLATING_CLASS(ccf, gr_complex, float)
GRHIP_XLATING_CLASS(fcf, float, float)
GRHIP_XLATING_CLASS(fcc, float, gr_complex)
GRHIP_XLATING_CLASS(scf, short, float)
GRHIP_XLATING_CLASS(scc, short, gr_complex)
#undef GRHIP_XLATING_CLASS

// ---------------------------------------------------------------------------
// gr_quadrature_demod_cf
// ---------------------------------------------------------------------------
class grhip_quadrature_demod_cf_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_block, quadrature_demod_cf) {
    friend struct grhip_detail::factory;
    grhip_quadrature_demod_cf_blk(float gain, int device)
        : block("quadrature_demod_cf", gr_make_io_signature(1, 1, sizeof(gr_complex)), gr_make_io_signature(1, 1, sizeof(float)))
    {
        grhip_detail::check(grhip_quadrature_demod_cf_create(d_h.out(), gain, device));
        set_history(2);                                        // gr_quadrature_demod_cf.cc:37
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_quadrature_demod_cf_work(d_h, noutput_items, in[0], out[0]));
    }
};
typedef boost::shared_ptr<grhip_quadrature_demod_cf_blk> grhip_quadrature_demod_cf_sptr;
inline grhip_quadrature_demod_cf_sptr grhip_make_quadrature_demod_cf(float gain, int device = 0)
{
    return grhip_detail::factory::make<grhip_quadrature_demod_cf_blk>(gain, device);
}

// ---------------------------------------------------------------------------
// digital_clock_recovery_mm_ff  (a gr_block: general_work + forecast + consume_each)
// ---------------------------------------------------------------------------
class grhip_clock_recovery_mm_ff_blk : public GRHIP_BLOCK_NO_MODE(gr_block, clock_recovery_mm_ff) {
    friend struct grhip_detail::factory;
    grhip_clock_recovery_mm_ff_blk(float omega, float gain_omega, float mu, float gain_mu,
                                   float omega_relative_limit, int device)
        : block("clock_recovery_mm_ff", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(float)))
    {
        grhip_detail::check(grhip_clock_recovery_mm_ff_create(d_h.out(), omega, gain_omega, mu, gain_mu,
                                                              omega_relative_limit, device));
        set_relative_rate(1.0 / omega);                        // .cc:64
    }
public:
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        forecast_each(grhip_clock_recovery_mm_ff_forecast, noutput_items, req);
    }
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                     gr_vector_void_star &out) override
    {
        int consumed = 0;
        int r = checked(grhip_clock_recovery_mm_ff_general_work(d_h, noutput_items, ninput_items[0], (const float *)in[0],
                                                                (float *)out[0], &consumed));
        consume_each(consumed);
        return r;
    }
    float mu() const { return grhip_clock_recovery_mm_ff_mu(d_h); }
    float omega() const { return grhip_clock_recovery_mm_ff_omega(d_h); }
    float gain_mu() const { return grhip_clock_recovery_mm_ff_gain_mu(d_h); }
    float gain_omega() const { return grhip_clock_recovery_mm_ff_gain_omega(d_h); }
    void set_gain_mu(float v) { grhip_detail::check(grhip_clock_recovery_mm_ff_set_gain_mu(d_h, v)); }
    void set_gain_omega(float v) { grhip_detail::check(grhip_clock_recovery_mm_ff_set_gain_omega(d_h, v)); }
    void set_mu(float v) { grhip_detail::check(grhip_clock_recovery_mm_ff_set_mu(d_h, v)); }
    void set_omega(float v) { grhip_detail::check(grhip_clock_recovery_mm_ff_set_omega(d_h, v)); }
};
typedef boost::shared_ptr<grhip_clock_recovery_mm_ff_blk> grhip_clock_recovery_mm_ff_sptr;
inline grhip_clock_recovery_mm_ff_sptr grhip_make_clock_recovery_mm_ff(float omega, float gain_omega, float mu,
                                                                       float gain_mu, float omega_relative_limit,
                                                                       int device = 0)
{
    return grhip_detail::factory::make<grhip_clock_recovery_mm_ff_blk>(omega, gain_omega, mu, gain_mu, omega_relative_limit,
                                                                       device);
}

// ---------------------------------------------------------------------------
// digital_binary_slicer_fb, digital_correlate_access_code_bb
// ---------------------------------------------------------------------------
class grhip_binary_slicer_fb_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_block, binary_slicer_fb) {
    friend struct grhip_detail::factory;
    explicit grhip_binary_slicer_fb_blk(int device)
        : block("binary_slicer_fb", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(unsigned char)))
    {
        grhip_detail::check(grhip_binary_slicer_fb_create(d_h.out(), device));
    }
public:
    int work(int n, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_binary_slicer_fb_work(d_h, n, (const float *)in[0], (unsigned char *)out[0]));
    }
};
typedef boost::shared_ptr<grhip_binary_slicer_fb_blk> grhip_binary_slicer_fb_sptr;
inline grhip_binary_slicer_fb_sptr grhip_make_binary_slicer_fb(int device = 0)
{
    return grhip_detail::factory::make<grhip_binary_slicer_fb_blk>(device);
}

// digital_clock_recovery_mm_cc (gr-digital/include/digital_clock_recovery_mm_cc.h:44-110): one complex input,
// one complex output and the optional float error output (the shim's io signature carries one item size, so the
// second port is described by the comment only; general_work looks at out.size() like the reference)
class grhip_clock_recovery_mm_cc_blk : public GRHIP_BLOCK_NO_MODE(gr_block, clock_recovery_mm_cc) {
    friend struct grhip_detail::factory;
    grhip_clock_recovery_mm_cc_blk(float omega, float gain_omega, float mu, float gain_mu, float omega_relative_limit,
                                   int device)
        : block("clock_recovery_mm_cc", gr_make_io_signature(1, 1, sizeof(gr_complex)), gr_make_io_signature(1, 2, sizeof(gr_complex)))
    {
        grhip_detail::check(grhip_clock_recovery_mm_cc_create(d_h.out(), omega, gain_omega, mu, gain_mu,
                                                              omega_relative_limit, device));
        set_relative_rate(1.0 / omega);                        // .cc:68
        set_history(3);                                        // .cc:69
    }
    float get(int (*f)(grhip_clock_recovery_mm_cc *, float *)) const
    {
        float v = 0;
        grhip_detail::check(f(d_h, &v));
        return v;
    }
public:
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        forecast_each(grhip_clock_recovery_mm_cc_forecast, noutput_items, req);
    }
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                     gr_vector_void_star &out) override
    {
        int consumed = 0;
        float *err = out.size() >= 2 ? (float *)out[1] : nullptr;          // .cc:124-126
        int r = checked(grhip_clock_recovery_mm_cc_general_work(d_h, noutput_items, ninput_items[0], in[0], out[0], err, &consumed));
        consume_each(consumed);
        return r;
    }
    float mu() const { return get(grhip_clock_recovery_mm_cc_mu); }
    float omega() const { return get(grhip_clock_recovery_mm_cc_omega); }
    float gain_mu() const { return get(grhip_clock_recovery_mm_cc_gain_mu); }
    float gain_omega() const { return get(grhip_clock_recovery_mm_cc_gain_omega); }
    void set_gain_mu(float v) { grhip_detail::check(grhip_clock_recovery_mm_cc_set_gain_mu(d_h, v)); }
    void set_gain_omega(float v) { grhip_detail::check(grhip_clock_recovery_mm_cc_set_gain_omega(d_h, v)); }
    void set_mu(float v) { grhip_detail::check(grhip_clock_recovery_mm_cc_set_mu(d_h, v)); }
    void set_omega(float v) { grhip_detail::check(grhip_clock_recovery_mm_cc_set_omega(d_h, v)); }
};
typedef boost::shared_ptr<grhip_clock_recovery_mm_cc_blk> grhip_clock_recovery_mm_cc_sptr;
inline grhip_clock_recovery_mm_cc_sptr grhip_make_clock_recovery_mm_cc(float omega, float gain_omega, float mu,
                                                                       float gain_mu, float omega_relative_limit,
                                                                       int device = 0)
{
    return grhip_detail::factory::make<grhip_clock_recovery_mm_cc_blk>(omega, gain_omega, mu, gain_mu, omega_relative_limit,
                                                                       device);
}

// pager_slicer_fb (gr-pager/lib/pager_slicer_fb.h:30-58), gr_unpack_k_bits_bb (general/gr_unpack_k_bits_bb.h)
class grhip_pager_slicer_fb_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_block, pager_slicer_fb) {
    friend struct grhip_detail::factory;
    grhip_pager_slicer_fb_blk(float alpha, int device)
        : block("slicer_fb", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(unsigned char)))
    {
        grhip_detail::check(grhip_pager_slicer_fb_create(d_h.out(), alpha, device));
    }
public:
    float dc_offset() const
    {
        float v = 0;
        grhip_detail::check(grhip_pager_slicer_fb_dc_offset(d_h, &v));
        return v;
    }
    int work(int n, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_pager_slicer_fb_work(d_h, n, (const float *)in[0], (unsigned char *)out[0]));
    }
};
typedef boost::shared_ptr<grhip_pager_slicer_fb_blk> grhip_pager_slicer_fb_sptr;
inline grhip_pager_slicer_fb_sptr grhip_make_pager_slicer_fb(float alpha, int device = 0)
{
    return grhip_detail::factory::make<grhip_pager_slicer_fb_blk>(alpha, device);
}

class grhip_unpack_k_bits_bb_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_interpolator, unpack_k_bits_bb) {
    friend struct grhip_detail::factory;
    grhip_unpack_k_bits_bb_blk(unsigned k, int device)
        : block("unpack_k_bits_bb", gr_make_io_signature(1, 1, sizeof(unsigned char)),
                gr_make_io_signature(1, 1, sizeof(unsigned char)), k)
    {
        // the reference throws std::out_of_range("interpolation must be > 0") (.cc:45-46)
        grhip_detail::check(grhip_unpack_k_bits_bb_create(d_h.out(), k, device));
    }
public:
    int work(int n, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_unpack_k_bits_bb_work(d_h, n, (const unsigned char *)in[0], (unsigned char *)out[0]));
    }
};
typedef boost::shared_ptr<grhip_unpack_k_bits_bb_blk> grhip_unpack_k_bits_bb_sptr;
inline grhip_unpack_k_bits_bb_sptr grhip_make_unpack_k_bits_bb(unsigned k, int device = 0)
{
    return grhip_detail::factory::make<grhip_unpack_k_bits_bb_blk>(k, device);
}

// gr_framer_sink_1 (general/gr_framer_sink_1.h:34-107): same constructor argument, same messages in the same queue
class grhip_framer_sink_1_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_block, framer_sink_1) {
    friend struct grhip_detail::factory;
    gr_msg_queue_sptr d_target_queue;
    std::vector<unsigned char> d_buf;
    grhip_framer_sink_1_blk(gr_msg_queue_sptr target_queue, int device)
        : block("framer_sink_1", gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(0, 0, 0)),
          d_target_queue(target_queue), d_buf(4096)
    {
        grhip_detail::check(grhip_framer_sink_1_create(d_h.out(), device));
    }
public:
    int work(int n, gr_vector_const_void_star &in, gr_vector_void_star &) override
    {
        int r = checked(grhip_framer_sink_1_work(d_h, n, (const unsigned char *)in[0]));
        int m = checked(grhip_framer_sink_1_message_count(d_h, nullptr));
        for (int i = 0; i < m; i++) {
            int woff = 0;
            int len = checked(grhip_framer_sink_1_pop(d_h, &woff, d_buf.data(), (int)d_buf.size()));
            gr_message_sptr msg = gr_make_message(0, woff, 0, len);      // .cc:140-141, 168-170
            if (len) memcpy(msg->msg(), d_buf.data(), len);
            d_target_queue->insert_tail(msg);
        }
        return r;
    }
};
typedef boost::shared_ptr<grhip_framer_sink_1_blk> grhip_framer_sink_1_sptr;
inline grhip_framer_sink_1_sptr grhip_make_framer_sink_1(gr_msg_queue_sptr target_queue, int device = 0)
{
    return grhip_detail::factory::make<grhip_framer_sink_1_blk>(target_queue, device);
}

class grhip_correlate_access_code_bb_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_block, correlate_access_code_bb) {
    friend struct grhip_detail::factory;
    grhip_correlate_access_code_bb_blk(const std::string &access_code, int threshold, int device)
        : block("correlate_access_code_bb", gr_make_io_signature(1, 1, sizeof(char)), gr_make_io_signature(1, 1, sizeof(char)))
    {
        // the reference throws std::out_of_range("access_code is > 64 bits") (.cc:54-57)
        grhip_detail::check(grhip_correlate_access_code_bb_create(d_h.out(), access_code.data(), access_code.size(),
                                                                  threshold, device));
    }
public:
    bool set_access_code(const std::string &code)             // .cc:64-85: false if longer than 64
    {
        return grhip_correlate_access_code_bb_set_access_code(d_h, code.data(), code.size()) == GRHIP_OK;
    }
    int work(int n, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_correlate_access_code_bb_work(d_h, n, (const unsigned char *)in[0], (unsigned char *)out[0]));
    }
};
typedef boost::shared_ptr<grhip_correlate_access_code_bb_blk> grhip_correlate_access_code_bb_sptr;
inline grhip_correlate_access_code_bb_sptr grhip_make_correlate_access_code_bb(const std::string &access_code,
                                                                               int threshold, int device = 0)
{
    return grhip_detail::factory::make<grhip_correlate_access_code_bb_blk>(access_code, threshold, device);
}

// ---------------------------------------------------------------------------
// gr_fft_vcc_hip: sits where gr_fft_vcc_fftw sits (general/gr_fft_vcc_fftw.h:36-58).  The base class owns size, window,
// direction and shift; its set_window() is not virtual and only stores the vector, so work() hands a changed
// window to the device before it transforms (the FFTW subclass reads d_window in work() too, .cc:68-76).
// ---------------------------------------------------------------------------
class gr_fft_vcc_hip : public GRHIP_BLOCK_NO_MODE(gr_fft_vcc, fft_vcc) {
    friend struct grhip_detail::factory;
    std::vector<float> d_sent;
    gr_fft_vcc_hip(int fft_size, bool forward, const std::vector<float> &window, bool shift, int device)
        : block("fft_vcc_hip", fft_size, forward, window, shift), d_sent(d_window)
    {
        grhip_detail::check(grhip_fft_vcc_create(d_h.out(), fft_size, forward, d_window.data(), d_window.size(), shift, device));
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        if (d_window != d_sent) {
            grhip_detail::check(grhip_fft_vcc_set_window(d_h, d_window.data(), d_window.size()));
            d_sent = d_window;
        }
        return checked(grhip_fft_vcc_work(d_h, noutput_items, in[0], out[0]));
    }
};
typedef boost::shared_ptr<gr_fft_vcc_hip> gr_fft_vcc_hip_sptr;
inline gr_fft_vcc_hip_sptr gr_make_fft_vcc_hip(int fft_size, bool forward, const std::vector<float> &window,
                                               bool shift = false, int device = 0)
{
    if (fft_size <= 0) throw std::out_of_range("gr_fft_vcc_hip: invalid fft_size");      // gri_fft.cc:104-105
    return grhip_detail::factory::make<gr_fft_vcc_hip>(fft_size, forward, window, shift, device);
}

// the block-level factory of round 1 keeps its name
typedef gr_fft_vcc_hip grhip_fft_vcc_blk;
typedef gr_fft_vcc_hip_sptr grhip_fft_vcc_sptr;
inline grhip_fft_vcc_sptr grhip_make_fft_vcc(int fft_size, bool forward, const std::vector<float> &window,
                                             bool shift = false, int device = 0)
{
    return gr_make_fft_vcc_hip(fft_size, forward, window, shift, device);
}

// ---------------------------------------------------------------------------
// gr_pfb_channelizer_ccf  (numchans inputs, one output of numchans-complex vectors)
// ---------------------------------------------------------------------------
// gr_fft_filter_ccc (filter/gr_fft_filter_ccc.h): gr_sync_decimator, history 1, output multiple nsamples
class grhip_fft_filter_ccc_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_decimator, fft_filter_ccc) {
    friend struct grhip_detail::factory;
    grhip_fft_filter_ccc_blk(int decimation, const std::vector<gr_complex> &taps, int device)
        : block("fft_filter_ccc", gr_make_io_signature(1, 1, sizeof(gr_complex)), gr_make_io_signature(1, 1, sizeof(gr_complex)),
                decimation)
    {
        grhip_detail::check(grhip_fft_filter_ccc_create(d_h.out(), decimation, (const float *)taps.data(), taps.size(), device));
        set_history(1);
        set_output_multiple(grhip_fft_filter_ccc_nsamples(d_h));          // gr_fft_filter_ccc.cc:69
    }
public:
    void set_taps(const std::vector<gr_complex> &taps)
    {
        grhip_detail::check(grhip_fft_filter_ccc_set_taps(d_h, (const float *)taps.data(), taps.size()));
    }
    int work(int n, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int r = checked(grhip_fft_filter_ccc_work(d_h, n, in[0], out[0]));
        if (r == 0) set_output_multiple(grhip_fft_filter_ccc_nsamples(d_h));   // .cc:113-118
        return r;
    }
};
typedef boost::shared_ptr<grhip_fft_filter_ccc_blk> grhip_fft_filter_ccc_sptr;
inline grhip_fft_filter_ccc_sptr grhip_make_fft_filter_ccc(int decimation, const std::vector<gr_complex> &taps, int device = 0)
{
    return grhip_detail::factory::make<grhip_fft_filter_ccc_blk>(decimation, taps, device);
}

// gr_fft_filter_fff (filter/gr_fft_filter_fff.h, .cc:44-97): gr_sync_decimator on floats, history 1, output multiple nsamples
class grhip_fft_filter_fff_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_decimator, fft_filter_fff) {
    friend struct grhip_detail::factory;
    grhip_fft_filter_fff_blk(int decimation, const std::vector<float> &taps, int device)
        : block("fft_filter_fff", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(float)), decimation)
    {
        grhip_detail::check(grhip_fft_filter_fff_create(d_h.out(), decimation, taps.data(), taps.size(), device));
        set_history(1);                                                       // gr_fft_filter_fff.cc:51
        set_output_multiple(grhip_fft_filter_fff_nsamples(d_h));          // .cc:59-60
    }
public:
    void set_taps(const std::vector<float> &taps)                             // .cc:69-73
    {
        grhip_detail::check(grhip_fft_filter_fff_set_taps(d_h, taps.data(), taps.size()));
    }
    int work(int n, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int r = checked(grhip_fft_filter_fff_work(d_h, n, in[0], out[0]));
        if (r == 0) set_output_multiple(grhip_fft_filter_fff_nsamples(d_h));   // .cc:83-88
        return r;
    }
};
typedef boost::shared_ptr<grhip_fft_filter_fff_blk> grhip_fft_filter_fff_sptr;
inline grhip_fft_filter_fff_sptr grhip_make_fft_filter_fff(int decimation, const std::vector<float> &taps, int device = 0)
{
    return grhip_detail::factory::make<grhip_fft_filter_fff_blk>(decimation, taps, device);
}

// gr_fft_vfc (general/gr_fft_vfc.h, .cc:42-118): gr_sync_block, items of fft_size floats in, fft_size complex out; forward only
class grhip_fft_vfc_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_block, fft_vfc) {
    friend struct grhip_detail::factory;
    unsigned int d_fft_size;
    grhip_fft_vfc_blk(int fft_size, bool forward, const std::vector<float> &window, int device)
        : block("fft_vfc", gr_make_io_signature(1, 1, fft_size * sizeof(float)),
                gr_make_io_signature(1, 1, fft_size * sizeof(gr_complex))),
          d_fft_size(fft_size)
    {
        if (!forward) throw std::invalid_argument("fft_vfc: forward must == true");     // .cc:54-57
        grhip_detail::check(grhip_fft_vfc_create(d_h.out(), fft_size, forward, window.data(), window.size(), device));
    }
public:
    bool set_window(const std::vector<float> &window)                         // .cc:109-118
    {
        return checked(grhip_fft_vfc_set_window(d_h, window.data(), window.size())) == 1;
    }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_fft_vfc_work(d_h, noutput_items, in[0], out[0]));
    }
};
typedef boost::shared_ptr<grhip_fft_vfc_blk> grhip_fft_vfc_sptr;
inline grhip_fft_vfc_sptr grhip_make_fft_vfc(int fft_size, bool forward, const std::vector<float> &window, int device = 0)
{
    if (fft_size <= 0) throw std::out_of_range("fft_vfc: invalid fft_size");            // gri_fft.cc:104-105
    return grhip_detail::factory::make<grhip_fft_vfc_blk>(fft_size, forward, window, device);
}

// gr_pfb_decimator_ccf (filter/gr_pfb_decimator_ccf.h:100-140)
class grhip_pfb_decimator_ccf_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_block, pfb_decimator_ccf) {
    friend struct grhip_detail::factory;
    grhip_pfb_decimator_ccf_blk(unsigned decim, const std::vector<float> &taps, unsigned channel, int device)
        : block("pfb_decimator_ccf", gr_make_io_signature(decim, decim, sizeof(gr_complex)),
                gr_make_io_signature(1, 1, sizeof(gr_complex)))
    {
        grhip_detail::check(grhip_pfb_decimator_ccf_create(d_h.out(), decim, taps.data(), taps.size(), channel, device));
        set_history(grhip_pfb_decimator_ccf_history(d_h));           // .cc:108
    }
public:
    void set_taps(const std::vector<float> &taps)
    {
        grhip_detail::check(grhip_pfb_decimator_ccf_set_taps(d_h, taps.data(), taps.size()));
        set_history(grhip_pfb_decimator_ccf_history(d_h));
    }
    int work(int n, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_pfb_decimator_ccf_work(d_h, n, in.data(), out[0]));
    }
};
typedef boost::shared_ptr<grhip_pfb_decimator_ccf_blk> grhip_pfb_decimator_ccf_sptr;
inline grhip_pfb_decimator_ccf_sptr grhip_make_pfb_decimator_ccf(unsigned decim, const std::vector<float> &taps,
                                                                 unsigned channel = 0, int device = 0)
{
    return grhip_detail::factory::make<grhip_pfb_decimator_ccf_blk>(decim, taps, channel, device);
}

class grhip_pfb_channelizer_ccf_blk : public GRHIP_BLOCK_NO_MODE(gr_block, pfb_channelizer_ccf) {
    friend struct grhip_detail::factory;
    unsigned d_numchans;
    grhip_pfb_channelizer_ccf_blk(unsigned numchans, const std::vector<float> &taps, float oversample_rate, int device)
        : block("pfb_channelizer_ccf", gr_make_io_signature(numchans, numchans, sizeof(gr_complex)),
                gr_make_io_signature(1, 1, numchans * sizeof(gr_complex))),
          d_numchans(numchans)
    {
        // std::invalid_argument when numchans/oversample_rate is not an integer (.cc:57-60)
        grhip_detail::check(grhip_pfb_channelizer_ccf_create(d_h.out(), numchans, taps.data(), taps.size(), oversample_rate,
                                                             device));
        set_history(grhip_pfb_channelizer_ccf_history(d_h));
        set_relative_rate(1.0 / (numchans / oversample_rate));    // set_relative_rate(1.0/intp), .cc:62
        set_output_multiple(grhip_pfb_channelizer_ccf_output_multiple(d_h));     // gr_pfb_channelizer_ccf.cc:92
    }
public:
    void set_taps(const std::vector<float> &taps)
    {
        grhip_detail::check(grhip_pfb_channelizer_ccf_set_taps(d_h, taps.data(), taps.size()));
        set_history(grhip_pfb_channelizer_ccf_history(d_h));
    }
    int general_work(int noutput_items, gr_vector_int &, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int consumed = 0;
        int r = checked(grhip_pfb_channelizer_ccf_general_work(d_h, noutput_items, in.data(), out[0], &consumed));
        consume_each(consumed);
        return r;
    }
};
typedef boost::shared_ptr<grhip_pfb_channelizer_ccf_blk> grhip_pfb_channelizer_ccf_sptr;
inline grhip_pfb_channelizer_ccf_sptr grhip_make_pfb_channelizer_ccf(unsigned numchans, const std::vector<float> &taps,
                                                                     float oversample_rate = 1, int device = 0)
{
    return grhip_detail::factory::make<grhip_pfb_channelizer_ccf_blk>(numchans, taps, oversample_rate, device);
}

// ---------------------------------------------------------------------------
// gr_pfb_arb_resampler_ccf / _fff  (a gr_block: general_work + consume_each, gr_block's default forecast)
// ---------------------------------------------------------------------------
template <class T, class ITEM>
class grhip_pfb_arb_resampler_blk : public grhip_detail::block<gr_block, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    grhip_pfb_arb_resampler_blk(float rate, const std::vector<float> &taps, unsigned filter_size, int device)
        : grhip_pfb_arb_resampler_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(ITEM)), gr_make_io_signature(1, 1, sizeof(ITEM)))
    {
        grhip_detail::check(T::create(this->d_h.out(), rate, taps.data(), taps.size(), filter_size, device));
        this->set_history((unsigned)this->checked(T::history(this->d_h)));         // tpf + 1 (.cc:118)
        this->set_relative_rate(rate);                                             // set_rate (.h:169)
    }
public:
    void set_rate(float rate)
    {
        grhip_detail::check(T::set_rate(this->d_h, rate));
        this->set_relative_rate(rate);
    }
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                     gr_vector_void_star &out) override
    {
        return this->work_consumed(T::general_work, noutput_items, ninput_items, in, out);
    }
};

#define GRHIP_ARB_BLOCK(SUF, ITEM)                                                                                     \
    namespace grhip_detail {                                                                                           \
    struct pfb_arb_resampler_##SUF##_fns {                                                                             \
        typedef grhip_pfb_arb_resampler_##SUF H;                                                                       \
        static constexpr const char *name = "pfb_arb_resampler_" #SUF;                                                 \
        GRHIP_FN(pfb_arb_resampler_##SUF, create); GRHIP_FN(pfb_arb_resampler_##SUF, destroy);                         \
        GRHIP_FN(pfb_arb_resampler_##SUF, set_rate); GRHIP_FN(pfb_arb_resampler_##SUF, set_mode);                      \
        GRHIP_FN(pfb_arb_resampler_##SUF, history); GRHIP_FN(pfb_arb_resampler_##SUF, general_work);                   \
    };                                                                                                                 \
    }                                                                                                                  \
    typedef grhip_pfb_arb_resampler_blk<grhip_detail::pfb_arb_resampler_##SUF##_fns, ITEM>                             \
        grhip_pfb_arb_resampler_##SUF##_blk;                                                                           \
    typedef boost::shared_ptr<grhip_pfb_arb_resampler_##SUF##_blk> grhip_pfb_arb_resampler_##SUF##_sptr;               \
    inline grhip_pfb_arb_resampler_##SUF##_sptr grhip_make_pfb_arb_resampler_##SUF(                                   \
        float rate, const std::vector<float> &taps, unsigned filter_size = 32, int device = 0)                        \
    {                                                                                                                  \
        return grhip_detail::factory::make<grhip_pfb_arb_resampler_##SUF##_blk>(rate, taps, filter_size, device);     \
    }

GRHIP_ARB_BLOCK(ccf, gr_complex)
GRHIP_ARB_BLOCK(fff, float)
#undef GRHIP_ARB_BLOCK

// ---------------------------------------------------------------------------
// gr_fractional_interpolator_ff / _cc  (a gr_block: general_work + consume_each, its own forecast, relative rate
// 1 / interp_ratio; filter/gr_fractional_interpolator_ff.h:41-66).  std::out_of_range where the reference throws it.
// ---------------------------------------------------------------------------
template <class T, class ITEM>
class grhip_fractional_interpolator_blk : public grhip_detail::block<gr_block, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    grhip_fractional_interpolator_blk(float phase_shift, float interp_ratio, int device)
        : grhip_fractional_interpolator_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(ITEM)),
                                                   gr_make_io_signature(1, 1, sizeof(ITEM)))
    {
        grhip_detail::check(T::create(this->d_h.out(), phase_shift, interp_ratio, device));
        this->set_relative_rate(1.0 / interp_ratio);                               // .cc:49
    }
public:
    float mu() const { return T::mu(this->d_h); }
    float interp_ratio() const { return T::interp_ratio(this->d_h); }
    void set_mu(float mu) { grhip_detail::check(T::set_mu(this->d_h, mu)); }
    void set_interp_ratio(float r) { grhip_detail::check(T::set_interp_ratio(this->d_h, r)); }
    void forecast(int noutput_items, gr_vector_int &ninput_items_required) override
    {
        this->forecast_each(T::forecast, noutput_items, ninput_items_required);    // .cc:57-65
    }
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                     gr_vector_void_star &out) override
    {
        return this->work_consumed(T::general_work, noutput_items, ninput_items, in, out);
    }
};

#define GRHIP_FRAC_BLOCK(SUF, ITEM)                                                                                    \
    namespace grhip_detail {                                                                                           \
    struct fractional_interpolator_##SUF##_fns {                                                                       \
        typedef grhip_fractional_interpolator_##SUF H;                                                                 \
        static constexpr const char *name = "fractional_interpolator_" #SUF;                                           \
        GRHIP_FN(fractional_interpolator_##SUF, create); GRHIP_FN(fractional_interpolator_##SUF, destroy);             \
        GRHIP_FN(fractional_interpolator_##SUF, set_mode); GRHIP_FN(fractional_interpolator_##SUF, mu);                \
        GRHIP_FN(fractional_interpolator_##SUF, interp_ratio); GRHIP_FN(fractional_interpolator_##SUF, set_mu);        \
        GRHIP_FN(fractional_interpolator_##SUF, set_interp_ratio); GRHIP_FN(fractional_interpolator_##SUF, forecast);  \
        GRHIP_FN(fractional_interpolator_##SUF, general_work);                                                         \
    };                                                                                                                 \
    }                                                                                                                  \
    typedef grhip_fractional_interpolator_blk<grhip_detail::fractional_interpolator_##SUF##_fns, ITEM>                 \
        grhip_fractional_interpolator_##SUF##_blk;                                                                     \
    typedef boost::shared_ptr<grhip_fractional_interpolator_##SUF##_blk> grhip_fractional_interpolator_##SUF##_sptr;   \
    inline grhip_fractional_interpolator_##SUF##_sptr grhip_make_fractional_interpolator_##SUF(                       \
        float phase_shift, float interp_ratio, int device = 0)                                                        \
    {                                                                                                                  \
        return grhip_detail::factory::make<grhip_fractional_interpolator_##SUF##_blk>(phase_shift, interp_ratio, device); \
    }

GRHIP_FRAC_BLOCK(ff, float)
GRHIP_FRAC_BLOCK(cc, gr_complex)
#undef GRHIP_FRAC_BLOCK

// ---------------------------------------------------------------------------
// gr_interp_fir_filter_XXX  (a gr_sync_interpolator: history nt, output_multiple I; filter/gr_interp_fir_filter_XXX.h.t)
// gr_rational_resampler_base_XXX  (a gr_block: gr_block's history stays 1, the reference's own forecast, relative
// rate I/D; filter/gr_rational_resampler_base_XXX.h.t)
// ---------------------------------------------------------------------------
template <class ITEM, class TAP> class grhip_interp_fir_filter_blk : public GRHIP_BLOCK(gr_sync_interpolator, interp_fir_filter) {
public:
    grhip_interp_fir_filter_blk(const char *kind, unsigned interpolation, const std::vector<TAP> &taps, int device)
        : block(std::string("interp_fir_filter_") + kind, gr_make_io_signature(1, 1, sizeof(ITEM)),
                gr_make_io_signature(1, 1, sizeof(ITEM)), interpolation)
    {
        grhip_detail::check(grhip_interp_fir_filter_create(d_h.out(), kind, interpolation,
                                                           reinterpret_cast<const float *>(taps.data()), taps.size(),
                                                           device));
        sync_history();
    }
    void set_taps(const std::vector<TAP> &taps)
    {
        grhip_detail::check(grhip_interp_fir_filter_set_taps(d_h, reinterpret_cast<const float *>(taps.data()),
                                                             taps.size()));
    }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int r = checked(grhip_interp_fir_filter_work(d_h, noutput_items, in[0], out[0]));
        sync_history();                                                 // install_taps: set_history(nt)
        return r;
    }
private:
    void sync_history() { set_history((unsigned)checked(grhip_interp_fir_filter_history(d_h))); }
};

template <class ITEM, class TAP> class grhip_rational_resampler_base_blk : public GRHIP_BLOCK(gr_block, rational_resampler_base) {
public:
    grhip_rational_resampler_base_blk(const char *kind, unsigned interpolation, unsigned decimation,
                                      const std::vector<TAP> &taps, int device)
        : block(std::string("rational_resampler_base_") + kind, gr_make_io_signature(1, 1, sizeof(ITEM)),
                gr_make_io_signature(1, 1, sizeof(ITEM)))
    {
        grhip_detail::check(grhip_rational_resampler_base_create(d_h.out(), kind, interpolation, decimation,
                                                                 reinterpret_cast<const float *>(taps.data()),
                                                                 taps.size(), device));
        set_relative_rate(1.0 * interpolation / decimation);          // .cc.t:63
    }
    unsigned interpolation() const { return (unsigned)grhip_rational_resampler_base_interpolation(d_h); }
    unsigned decimation() const { return (unsigned)grhip_rational_resampler_base_decimation(d_h); }
    // the block's own history (nt), which hides gr_block's: the scheduler keeps seeing 1 (.h.t:51,72-73)
    unsigned resampler_history() const { return (unsigned)grhip_rational_resampler_base_history(d_h); }
    void set_taps(const std::vector<TAP> &taps)
    {
        grhip_detail::check(grhip_rational_resampler_base_set_taps(d_h, reinterpret_cast<const float *>(taps.data()),
                                                                   taps.size()));
    }
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        forecast_each(grhip_rational_resampler_base_forecast, noutput_items, req);
    }
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                     gr_vector_void_star &out) override
    {
        return work_consumed(grhip_rational_resampler_base_general_work, noutput_items, ninput_items, in, out);
    }
};

#define GRHIP_RS_BLOCKS(SUF, ITEM, TAP)                                                                                \
    typedef grhip_interp_fir_filter_blk<ITEM, TAP> grhip_interp_fir_filter_##SUF;                                     \
    typedef boost::shared_ptr<grhip_interp_fir_filter_##SUF> grhip_interp_fir_filter_##SUF##_sptr;                    \
    inline grhip_interp_fir_filter_##SUF##_sptr grhip_make_interp_fir_filter_##SUF(                                   \
        unsigned interpolation, const std::vector<TAP> &taps, int device = 0)                                         \
    {                                                                                                                  \
        return grhip_detail::factory::make<grhip_interp_fir_filter_##SUF>(#SUF, interpolation, taps, device);         \
    }                                                                                                                  \
    typedef grhip_rational_resampler_base_blk<ITEM, TAP> grhip_rational_resampler_base_##SUF;                         \
    typedef boost::shared_ptr<grhip_rational_resampler_base_##SUF> grhip_rational_resampler_base_##SUF##_sptr;        \
    inline grhip_rational_resampler_base_##SUF##_sptr grhip_make_rational_resampler_base_##SUF(                       \
        unsigned interpolation, unsigned decimation, const std::vector<TAP> &taps, int device = 0)                    \
    {                                                                                                                  \
        return grhip_detail::factory::make<grhip_rational_resampler_base_##SUF>(#SUF, interpolation, decimation,      \
                                                                                taps, device);                         \
    }

GRHIP_RS_BLOCKS(ccf, gr_complex, float)
GRHIP_RS_BLOCKS(fff, float, float)
GRHIP_RS_BLOCKS(ccc, gr_complex, gr_complex)
#undef GRHIP_RS_BLOCKS

// ---------------------------------------------------------------------------
// gr_pfb_interpolator_ccf  (a gr_sync_interpolator by interp: history tpf; filter/gr_pfb_interpolator_ccf.h)
// gr_pfb_synthesis_filterbank_ccf  (a gr_sync_interpolator by numchans: 1..numchans inputs, history tpf + 1;
// filter/gr_pfb_synthesis_filterbank_ccf.h).  set_taps latches; the next work() installs the taps, returns 0 and the
// history follows (the library's convention, as grhip_interp_fir_filter_XXX).
// ---------------------------------------------------------------------------
class grhip_pfb_interpolator_ccf_blk : public GRHIP_BLOCK(gr_sync_interpolator, pfb_interpolator_ccf) {
    friend struct grhip_detail::factory;
    grhip_pfb_interpolator_ccf_blk(unsigned interp, const std::vector<float> &taps, int device)
        : block("pfb_interpolator_ccf", gr_make_io_signature(1, 1, sizeof(gr_complex)),
                gr_make_io_signature(1, 1, sizeof(gr_complex)), interp)
    {
        grhip_detail::check(grhip_pfb_interpolator_ccf_create(d_h.out(), interp, taps.data(), taps.size(), device));
        sync_history();
    }
    // set_history(d_taps_per_filter), .cc:101
    void sync_history() { set_history((unsigned)checked(grhip_pfb_interpolator_ccf_history(d_h))); }
public:
    void set_taps(const std::vector<float> &taps)
    {
        grhip_detail::check(grhip_pfb_interpolator_ccf_set_taps(d_h, taps.data(), taps.size()));
    }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int r = checked(grhip_pfb_interpolator_ccf_work(d_h, noutput_items, in[0], out[0]));
        sync_history();
        return r;
    }
};
typedef boost::shared_ptr<grhip_pfb_interpolator_ccf_blk> grhip_pfb_interpolator_ccf_sptr;
inline grhip_pfb_interpolator_ccf_sptr grhip_make_pfb_interpolator_ccf(unsigned interp, const std::vector<float> &taps,
                                                                       int device = 0)
{
    return grhip_detail::factory::make<grhip_pfb_interpolator_ccf_blk>(interp, taps, device);
}

class grhip_pfb_synthesis_filterbank_ccf_blk : public GRHIP_BLOCK(gr_sync_interpolator, pfb_synthesis_filterbank_ccf) {
    friend struct grhip_detail::factory;
    grhip_pfb_synthesis_filterbank_ccf_blk(unsigned numchans, const std::vector<float> &taps, int device)
        : block("pfb_synthesis_filterbank_ccf", gr_make_io_signature(1, numchans, sizeof(gr_complex)),
                gr_make_io_signature(1, 1, sizeof(gr_complex)), numchans)                       // .cc:43-46
    {
        grhip_detail::check(grhip_pfb_synthesis_filterbank_ccf_create(d_h.out(), numchans, taps.data(), taps.size(), device));
        sync_history();
    }
    // set_history(d_taps_per_filter + 1), .cc:103
    void sync_history() { set_history((unsigned)checked(grhip_pfb_synthesis_filterbank_ccf_history(d_h))); }
public:
    unsigned taps_per_filter() const { return (unsigned)grhip_pfb_synthesis_filterbank_ccf_taps_per_filter(d_h); }
    void set_taps(const std::vector<float> &taps)
    {
        grhip_detail::check(grhip_pfb_synthesis_filterbank_ccf_set_taps(d_h, taps.data(), taps.size()));
    }
    // the connected inputs are the streams (numsigs = input_items.size(), .cc:129)
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int r = checked(grhip_pfb_synthesis_filterbank_ccf_work(d_h, noutput_items, in.data(), (int)in.size(), out[0]));
        sync_history();
        return r;
    }
};
typedef boost::shared_ptr<grhip_pfb_synthesis_filterbank_ccf_blk> grhip_pfb_synthesis_filterbank_ccf_sptr;
inline grhip_pfb_synthesis_filterbank_ccf_sptr grhip_make_pfb_synthesis_filterbank_ccf(unsigned numchans,
                                                                                       const std::vector<float> &taps,
                                                                                       int device = 0)
{
    return grhip_detail::factory::make<grhip_pfb_synthesis_filterbank_ccf_blk>(numchans, taps, device);
}

// ---------------------------------------------------------------------------
// gr_hilbert_fc(ntaps)  (gr_sync_block, float -> complex, history ntaps | 1; filter/gr_hilbert_fc.cc:39-50)
// gr_filter_delay_fc(taps)  (gr_sync_block, 1 or 2 float inputs -> complex, history ntaps; filter/gr_filter_delay_fc.cc:38-46)
// gr_goertzel_fc(rate, len, freq)  (gr_sync_decimator by len, float -> complex; filter/gr_goertzel_fc.cc:38-50)
// ---------------------------------------------------------------------------
class grhip_hilbert_fc_blk : public GRHIP_BLOCK(gr_sync_block, hilbert_fc) {
    friend struct grhip_detail::factory;
    grhip_hilbert_fc_blk(unsigned ntaps, int device)
        : block("hilbert_fc", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(gr_complex)))
    {
        grhip_detail::check(grhip_hilbert_fc_create(d_h.out(), ntaps, device));
        set_history((unsigned)grhip_hilbert_fc_history(d_h));           // set_history(d_ntaps), .cc:49
    }
public:
    std::vector<float> taps() const
    {
        std::vector<float> t((size_t)grhip_hilbert_fc_ntaps(d_h));
        grhip_detail::check(grhip_hilbert_fc_taps(d_h, t.data(), t.size()));
        return t;
    }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_hilbert_fc_work(d_h, noutput_items, in[0], out[0]));
    }
};
typedef boost::shared_ptr<grhip_hilbert_fc_blk> grhip_hilbert_fc_sptr;
inline grhip_hilbert_fc_sptr grhip_make_hilbert_fc(unsigned ntaps, int device = 0)
{
    return grhip_detail::factory::make<grhip_hilbert_fc_blk>(ntaps, device);
}

class grhip_filter_delay_fc_blk : public GRHIP_BLOCK(gr_sync_block, filter_delay_fc) {
    friend struct grhip_detail::factory;
    grhip_filter_delay_fc_blk(const std::vector<float> &taps, int device)
        : block("filter_delay_fc", gr_make_io_signature(1, 2, sizeof(float)), gr_make_io_signature(1, 1, sizeof(gr_complex)))
    {
        grhip_detail::check(grhip_filter_delay_fc_create(d_h.out(), taps.data(), taps.size(), device));
        set_history((unsigned)grhip_filter_delay_fc_history(d_h));      // set_history(d_fir->ntaps()), .cc:45
    }
public:
    // the connected inputs decide the form (input_items.size(), .cc:61)
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_filter_delay_fc_work(d_h, noutput_items, in[0], in.size() > 1 ? in[1] : nullptr, out[0]));
    }
};
typedef boost::shared_ptr<grhip_filter_delay_fc_blk> grhip_filter_delay_fc_sptr;
inline grhip_filter_delay_fc_sptr grhip_make_filter_delay_fc(const std::vector<float> &taps, int device = 0)
{
    return grhip_detail::factory::make<grhip_filter_delay_fc_blk>(taps, device);
}

class grhip_goertzel_fc_blk : public GRHIP_BLOCK(gr_sync_decimator, goertzel_fc) {
    friend struct grhip_detail::factory;
    grhip_goertzel_fc_blk(int rate, int len, float freq, int device)
        : block("goertzel_fc", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(gr_complex)),
                len < 1 ? 1 : len)
    {
        grhip_detail::check(grhip_goertzel_fc_create(d_h.out(), rate, len, freq, device));
    }
public:
    void set_freq(float freq) { grhip_detail::check(grhip_goertzel_fc_set_freq(d_h, freq)); }
    void set_rate(int rate) { grhip_detail::check(grhip_goertzel_fc_set_rate(d_h, rate)); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return checked(grhip_goertzel_fc_work(d_h, noutput_items, in[0], out[0]));
    }
};
typedef boost::shared_ptr<grhip_goertzel_fc_blk> grhip_goertzel_fc_sptr;
inline grhip_goertzel_fc_sptr grhip_make_goertzel_fc(int rate, int len, float freq, int device = 0)
{
    return grhip_detail::factory::make<grhip_goertzel_fc_blk>(rate, len, freq, device);
}

// ---------------------------------------------------------------------------
// gr_dc_blocker_ff / _cc (D = 32, long_form = true)  (gr_sync_block, history 1; filter/gr_dc_blocker_ff.cc:63-103)
// gr_moving_average_XX (length, scale, max_iter = 4096)  (gr_sync_block, history length; gengen/gr_moving_average_XX.cc.t:38-62)
// gr_integrate_XX (decim)  (gr_sync_decimator by decim; gengen/gr_integrate_XX.cc.t:38-46)
// ---------------------------------------------------------------------------
#define GRHIP_DC_BLOCKER_BLK(SFX, ITEM)                                                                                \
    class grhip_dc_blocker_##SFX##_blk : public GRHIP_BLOCK(gr_sync_block, dc_blocker_##SFX) {                         \
        friend struct grhip_detail::factory;                                                                           \
        grhip_dc_blocker_##SFX##_blk(int D, bool long_form, int device)                                                \
            : block("dc_blocker_" #SFX, gr_make_io_signature(1, 1, sizeof(ITEM)), gr_make_io_signature(1, 1, sizeof(ITEM))) \
        {                                                                                                              \
            grhip_detail::check(grhip_dc_blocker_##SFX##_create(d_h.out(), D, long_form ? 1 : 0, device));             \
        }                                                                                                              \
    public:                                                                                                            \
        int get_group_delay() { return grhip_dc_blocker_##SFX##_group_delay(d_h); }                                    \
        int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override                  \
        {                                                                                                              \
            return checked(grhip_dc_blocker_##SFX##_work(d_h, noutput_items, in[0], out[0]));                          \
        }                                                                                                              \
    };                                                                                                                 \
    typedef boost::shared_ptr<grhip_dc_blocker_##SFX##_blk> grhip_dc_blocker_##SFX##_sptr;                             \
    inline grhip_dc_blocker_##SFX##_sptr grhip_make_dc_blocker_##SFX(int D = 32, bool long_form = true, int device = 0) \
    {                                                                                                                  \
        return grhip_detail::factory::make<grhip_dc_blocker_##SFX##_blk>(D, long_form, device);                        \
    }
GRHIP_DC_BLOCKER_BLK(ff, float)
GRHIP_DC_BLOCKER_BLK(cc, gr_complex)
#undef GRHIP_DC_BLOCKER_BLK

namespace grhip_detail {
inline int ma_create(grhip_moving_average_ff **h, int n, float s, int m, int d) { return grhip_moving_average_ff_create(h, n, s, m, d); }
inline int ma_create(grhip_moving_average_cc **h, int n, gr_complex s, int m, int d) { return grhip_moving_average_cc_create(h, n, s.real(), s.imag(), m, d); }
inline int ma_create(grhip_moving_average_ss **h, int n, short s, int m, int d) { return grhip_moving_average_ss_create(h, n, s, m, d); }
inline int ma_create(grhip_moving_average_ii **h, int n, int s, int m, int d) { return grhip_moving_average_ii_create(h, n, s, m, d); }
inline int ma_set(grhip_moving_average_ff *h, int n, float s) { return grhip_moving_average_ff_set_length_and_scale(h, n, s); }
inline int ma_set(grhip_moving_average_cc *h, int n, gr_complex s) { return grhip_moving_average_cc_set_length_and_scale(h, n, s.real(), s.imag()); }
inline int ma_set(grhip_moving_average_ss *h, int n, short s) { return grhip_moving_average_ss_set_length_and_scale(h, n, s); }
inline int ma_set(grhip_moving_average_ii *h, int n, int s) { return grhip_moving_average_ii_set_length_and_scale(h, n, s); }
}  // namespace grhip_detail

// work re-reads the history after the call: a latched set_length_and_scale has taken effect by then (.cc.t:72)
template <class H, void (*DESTROY)(H *), int (*SET_MODE)(H *, int), auto HISTORY, auto WORK, class ITEM>
class grhip_moving_average_blk : public grhip_detail::block<gr_sync_block, H, DESTROY, SET_MODE> {
protected:
    grhip_moving_average_blk(const char *name, int length, ITEM scale, int max_iter, int device)
        : grhip_moving_average_blk::block(name, gr_make_io_signature(1, 1, sizeof(ITEM)), gr_make_io_signature(1, 1, sizeof(ITEM)))
    {
        grhip_detail::check(grhip_detail::ma_create(this->d_h.out(), length, scale, max_iter, device));
        this->set_history((unsigned)length);                                        // .cc.t:49
    }
public:
    void set_length_and_scale(int length, ITEM scale) { grhip_detail::check(grhip_detail::ma_set(this->d_h, length, scale)); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int r = this->checked(WORK(this->d_h, noutput_items, in[0], out[0]));
        this->set_history((unsigned)HISTORY(this->d_h));
        return r;
    }
};
#define GRHIP_MOVING_AVERAGE_BLK(SFX, ITEM)                                                                            \
    class grhip_moving_average_##SFX##_blk                                                                             \
        : public grhip_moving_average_blk<grhip_moving_average_##SFX, grhip_moving_average_##SFX##_destroy,            \
                                          grhip_moving_average_##SFX##_set_mode, grhip_moving_average_##SFX##_history, \
                                          grhip_moving_average_##SFX##_work, ITEM> {                                   \
        friend struct grhip_detail::factory;                                                                           \
        grhip_moving_average_##SFX##_blk(int length, ITEM scale, int max_iter, int device)                             \
            : grhip_moving_average_blk("moving_average_" #SFX, length, scale, max_iter, device) {}                     \
    };                                                                                                                 \
    typedef boost::shared_ptr<grhip_moving_average_##SFX##_blk> grhip_moving_average_##SFX##_sptr;                     \
    inline grhip_moving_average_##SFX##_sptr grhip_make_moving_average_##SFX(int length, ITEM scale, int max_iter = 4096, int device = 0) \
    {                                                                                                                  \
        return grhip_detail::factory::make<grhip_moving_average_##SFX##_blk>(length, scale, max_iter, device);         \
    }
GRHIP_MOVING_AVERAGE_BLK(ff, float)
GRHIP_MOVING_AVERAGE_BLK(cc, gr_complex)
GRHIP_MOVING_AVERAGE_BLK(ss, short)
GRHIP_MOVING_AVERAGE_BLK(ii, int)
#undef GRHIP_MOVING_AVERAGE_BLK

#define GRHIP_INTEGRATE_BLK(SFX, ITEM)                                                                                 \
    class grhip_integrate_##SFX##_blk : public GRHIP_BLOCK(gr_sync_decimator, integrate_##SFX) {                       \
        friend struct grhip_detail::factory;                                                                           \
        grhip_integrate_##SFX##_blk(int decim, int device)                                                             \
            : block("integrate_" #SFX, gr_make_io_signature(1, 1, sizeof(ITEM)), gr_make_io_signature(1, 1, sizeof(ITEM)), \
                    decim < 1 ? 1 : decim)                                                                             \
        {                                                                                                              \
            grhip_detail::check(grhip_integrate_##SFX##_create(d_h.out(), decim, device));                             \
        }                                                                                                              \
    public:                                                                                                            \
        int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override                  \
        {                                                                                                              \
            return checked(grhip_integrate_##SFX##_work(d_h, noutput_items, in[0], out[0]));                           \
        }                                                                                                              \
    };                                                                                                                 \
    typedef boost::shared_ptr<grhip_integrate_##SFX##_blk> grhip_integrate_##SFX##_sptr;                               \
    inline grhip_integrate_##SFX##_sptr grhip_make_integrate_##SFX(int decim, int device = 0)                          \
    {                                                                                                                  \
        return grhip_detail::factory::make<grhip_integrate_##SFX##_blk>(decim, device);                                \
    }
GRHIP_INTEGRATE_BLK(ff, float)
GRHIP_INTEGRATE_BLK(cc, gr_complex)
GRHIP_INTEGRATE_BLK(ss, short)
GRHIP_INTEGRATE_BLK(ii, int)
#undef GRHIP_INTEGRATE_BLK

// ---------------------------------------------------------------------------
// gr_complex_to_mag_squared (vlen = 1), gr_single_pole_iir_filter_ff (alpha, vlen = 1), gr_nlog10_ff (n, vlen = 1, k = 0):
// gr_sync_block, history 1 (general/gr_complex_to_xxx.cc:180-203, filter/gr_single_pole_iir_filter_ff.cc:32-81,
// general/gr_nlog10_ff.cc:31-64).  gr_keep_one_in_n (item_size, n): gr_block, general_work
// (general/gr_keep_one_in_n.cc:31-105).
// ---------------------------------------------------------------------------
#define GRHIP_SPECTRUM_BLK(NAME, IN_T, CTOR_DECL, CREATE_ARGS, EXTRA)                                                  \
    class grhip_##NAME##_blk : public GRHIP_BLOCK(gr_sync_block, NAME) {                                               \
        friend struct grhip_detail::factory;                                                                           \
        grhip_##NAME##_blk CTOR_DECL                                                                                   \
            : block(#NAME, gr_make_io_signature(1, 1, sizeof(IN_T) * (vlen ? vlen : 1)),                               \
                    gr_make_io_signature(1, 1, sizeof(float) * (vlen ? vlen : 1)))                                     \
        {                                                                                                              \
            grhip_detail::check(grhip_##NAME##_create CREATE_ARGS);                                                    \
        }                                                                                                              \
    public:                                                                                                            \
        EXTRA                                                                                                          \
        int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override                  \
        {                                                                                                              \
            return checked(grhip_##NAME##_work(d_h, noutput_items, in[0], out[0]));                                    \
        }                                                                                                              \
    };                                                                                                                 \
    typedef boost::shared_ptr<grhip_##NAME##_blk> grhip_##NAME##_sptr;
GRHIP_SPECTRUM_BLK(complex_to_mag_squared, gr_complex, (unsigned int vlen, int device), (d_h.out(), (int)vlen, device), )
inline grhip_complex_to_mag_squared_sptr gr_make_complex_to_mag_squared(unsigned int vlen = 1, int device = 0)
{
    return grhip_detail::factory::make<grhip_complex_to_mag_squared_blk>(vlen, device);
}
// gr_complex_to_mag (vlen = 1): general/gr_complex_to_xxx.cc:143-171
GRHIP_SPECTRUM_BLK(complex_to_mag, gr_complex, (unsigned int vlen, int device), (d_h.out(), (int)vlen, device), )
inline grhip_complex_to_mag_sptr gr_make_complex_to_mag(unsigned int vlen = 1, int device = 0)
{
    return grhip_detail::factory::make<grhip_complex_to_mag_blk>(vlen, device);
}
GRHIP_SPECTRUM_BLK(single_pole_iir_filter_ff, float, (double alpha, unsigned int vlen, int device), (d_h.out(), alpha, (int)vlen, device),
                   void set_taps(double alpha) { grhip_detail::check(grhip_single_pole_iir_filter_ff_set_taps(d_h, alpha)); })
inline grhip_single_pole_iir_filter_ff_sptr gr_make_single_pole_iir_filter_ff(double alpha, unsigned int vlen = 1, int device = 0)
{
    return grhip_detail::factory::make<grhip_single_pole_iir_filter_ff_blk>(alpha, vlen, device);
}
GRHIP_SPECTRUM_BLK(nlog10_ff, float, (float n, unsigned vlen, float k, int device), (d_h.out(), n, (int)vlen, k, device), )
inline grhip_nlog10_ff_sptr gr_make_nlog10_ff(float n, unsigned vlen = 1, float k = 0, int device = 0)
{
    return grhip_detail::factory::make<grhip_nlog10_ff_blk>(n, vlen, k, device);
}
#undef GRHIP_SPECTRUM_BLK

class grhip_keep_one_in_n_blk : public GRHIP_BLOCK_NO_MODE(gr_block, keep_one_in_n) {
    friend struct grhip_detail::factory;
    int d_n = 1;
    grhip_keep_one_in_n_blk(size_t item_size, int n, int device)
        : block("keep_one_in_n", gr_make_io_signature(1, 1, (int)item_size), gr_make_io_signature(1, 1, (int)item_size))
    {
        grhip_detail::check(grhip_keep_one_in_n_create(d_h.out(), item_size, n, device));
        set_n(n);
    }
public:
    void set_n(int n)
    {
        d_n = n < 1 ? 1 : n;
        grhip_detail::check(grhip_keep_one_in_n_set_n(d_h, n));
        set_relative_rate(1.0 / d_n);
    }
    // forecast is gr_block's own, as in the reference (it overrides none): a finite stream is consumed to its last item.
    // as many inputs as there are, cut so that no more than noutput_items come out (gr_keep_one_in_n.cc:80)
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                     gr_vector_void_star &out) override
    {
        const int ni = grhip_detail::cut_to_output(d_h.get(), grhip_keep_one_in_n_produced, ninput_items[0], noutput_items, d_n);
        int r = checked(ni > 0 ? grhip_keep_one_in_n_work(d_h, ni, in[0], out[0]) : 0);
        consume_each(ni > 0 ? ni : 0);
        return r;
    }
};
typedef boost::shared_ptr<grhip_keep_one_in_n_blk> grhip_keep_one_in_n_sptr;
inline grhip_keep_one_in_n_sptr gr_make_keep_one_in_n(size_t item_size, int n, int device = 0)
{
    return grhip_detail::factory::make<grhip_keep_one_in_n_blk>(item_size, n, device);
}

// ---------------------------------------------------------------------------
// blks2.logpwrfft_c / logpwrfft_f (blks2impl/logpwrfft.py:26-154; a hier block there: stream_to_vector_decimator ->
// fft_vcc | fft_vfc -> complex_to_mag_squared -> single_pole_iir_filter_ff -> nlog10_ff), here one gr_block: items of one
// sample in, fft_size floats out, relative rate 1 / (fft_size decimation).  The reference's argument order and its
// setter and getter names; `win` is what the reference's window function returns for fft_size (doubles; empty: the
// default, window.blackmanharris).
// ---------------------------------------------------------------------------
template <class T, class IN_T>
class grhip_logpwrfft_blk : public grhip_detail::block<gr_block, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    int d_fft_size;
    grhip_logpwrfft_blk(double sample_rate, int fft_size, double ref_scale, double frame_rate, double avg_alpha, bool average,
                        const std::vector<double> &win, int device)
        : grhip_logpwrfft_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(IN_T)),
                                     gr_make_io_signature(1, 1, sizeof(float) * (fft_size > 0 ? fft_size : 1))),
          d_fft_size(fft_size)
    {
        grhip_detail::check(T::create(this->d_h.out(), sample_rate, fft_size, ref_scale, frame_rate, avg_alpha, average, win.data(),
                                      win.size(), device));
        update_rate();
    }
    void update_rate() { this->set_relative_rate(1.0 / ((double)d_fft_size * decimation())); }
public:
    void set_decimation(double decim)
    {
        grhip_detail::check(T::set_decimation(this->d_h, decim));
        update_rate();
    }
    void set_vec_rate(double r)
    {
        grhip_detail::check(T::set_vec_rate(this->d_h, r));
        update_rate();
    }
    void set_sample_rate(double r)
    {
        grhip_detail::check(T::set_sample_rate(this->d_h, r));
        update_rate();
    }
    void set_average(bool average) { grhip_detail::check(T::set_average(this->d_h, average)); }
    void set_avg_alpha(double a) { grhip_detail::check(T::set_avg_alpha(this->d_h, a)); }
    double sample_rate() const { return T::sample_rate(this->d_h); }
    int decimation() const { return T::decimation(this->d_h); }
    double frame_rate() const { return T::frame_rate(this->d_h); }
    bool average() const { return T::average(this->d_h) != 0; }
    double avg_alpha() const { return T::avg_alpha(this->d_h); }
    // one whole frame per output at least (stream_to_vector is a decimator by fft_size)
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        for (size_t i = 0; i < req.size(); i++) req[i] = noutput_items * d_fft_size;
    }
    // as many whole frames as there are, cut so that no more than noutput_items come out (gr_keep_one_in_n.cc:80)
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                     gr_vector_void_star &out) override
    {
        const int n = decimation();
        const int nf = grhip_detail::cut_to_output(this->d_h.get(), T::produced, ninput_items[0] / d_fft_size, noutput_items, n);
        int r = this->checked(nf > 0 ? T::work(this->d_h, nf, in[0], out[0]) : 0);
        this->consume_each(nf > 0 ? nf * d_fft_size : 0);
        return r;
    }
};
#define GRHIP_LOGPWRFFT_BLK(NAME, IN_T)                                                                                \
    namespace grhip_detail {                                                                                           \
    struct NAME##_fns {                                                                                                \
        typedef grhip_##NAME H;                                                                                        \
        static constexpr const char *name = #NAME;                                                                     \
        GRHIP_FN(NAME, create); GRHIP_FN(NAME, destroy); GRHIP_FN(NAME, set_mode); GRHIP_FN(NAME, set_decimation);     \
        GRHIP_FN(NAME, set_vec_rate); GRHIP_FN(NAME, set_sample_rate); GRHIP_FN(NAME, set_average);                    \
        GRHIP_FN(NAME, set_avg_alpha); GRHIP_FN(NAME, sample_rate); GRHIP_FN(NAME, decimation);                        \
        GRHIP_FN(NAME, frame_rate); GRHIP_FN(NAME, average); GRHIP_FN(NAME, avg_alpha); GRHIP_FN(NAME, produced);      \
        GRHIP_FN(NAME, work);                                                                                          \
    };                                                                                                                 \
    }                                                                                                                  \
    typedef grhip_logpwrfft_blk<grhip_detail::NAME##_fns, IN_T> grhip_##NAME##_blk;                                    \
    typedef boost::shared_ptr<grhip_##NAME##_blk> grhip_##NAME##_sptr;                                                 \
    inline grhip_##NAME##_sptr gr_make_##NAME(double sample_rate, int fft_size, double ref_scale, double frame_rate,   \
                                              double avg_alpha, bool average,                                          \
                                              const std::vector<double> &win = std::vector<double>(), int device = 0)  \
    {                                                                                                                  \
        return grhip_detail::factory::make<grhip_##NAME##_blk>(sample_rate, fft_size, ref_scale, frame_rate, avg_alpha, \
                                                               average, win, device);                                  \
    }
GRHIP_LOGPWRFFT_BLK(logpwrfft_c, gr_complex)
GRHIP_LOGPWRFFT_BLK(logpwrfft_f, float)
#undef GRHIP_LOGPWRFFT_BLK

// ---------------------------------------------------------------------------
// gr_pwr_squelch_cc / _ff (db, alpha = 0.0001, ramp = 0, gate = false): gr_block; general_work takes noutput_items
// inputs, consumes them all and returns the items produced, fewer with gating (general/gr_squelch_base_cc.cc:42-93,
// gr_pwr_squelch_cc.h:30-62).  gr_simple_squelch_cc (threshold_db, alpha = 0.0001): gr_sync_block
// (general/gr_simple_squelch_cc.h:30-63).
// ---------------------------------------------------------------------------
namespace grhip_detail {
inline std::vector<float> squelch_range()
{
    std::vector<float> r(3);
    r[0] = -50.0;
    r[1] = +50.0;
    r[2] = (r[1] - r[0]) / 100;
    return r;
}
}  // namespace grhip_detail

#define GRHIP_PWR_SQUELCH_BLK(NAME, ITEM)                                                                              \
    class grhip_##NAME##_blk : public GRHIP_BLOCK(gr_block, NAME) {                                                    \
        friend struct grhip_detail::factory;                                                                           \
        grhip_##NAME##_blk(double db, double alpha, int ramp, bool gate, int device)                                   \
            : block(#NAME, gr_make_io_signature(1, 1, sizeof(ITEM)), gr_make_io_signature(1, 1, sizeof(ITEM)))         \
        {                                                                                                              \
            grhip_detail::check(grhip_##NAME##_create(d_h.out(), db, alpha, ramp, gate, device));                      \
        }                                                                                                              \
    public:                                                                                                            \
        double threshold() const { return grhip_##NAME##_threshold(d_h); }                                             \
        void set_threshold(double db) { grhip_detail::check(grhip_##NAME##_set_threshold(d_h, db)); }                  \
        void set_alpha(double alpha) { grhip_detail::check(grhip_##NAME##_set_alpha(d_h, alpha)); }                    \
        int ramp() const { return grhip_##NAME##_ramp(d_h); }                                                          \
        void set_ramp(int ramp) { grhip_detail::check(grhip_##NAME##_set_ramp(d_h, ramp)); }                           \
        bool gate() const { return grhip_##NAME##_gate(d_h) != 0; }                                                    \
        void set_gate(bool gate) { grhip_detail::check(grhip_##NAME##_set_gate(d_h, gate)); }                          \
        bool unmuted() const { return checked(grhip_##NAME##_unmuted(d_h, 0)) != 0; }                                  \
        std::vector<float> squelch_range() const { return grhip_detail::squelch_range(); }                             \
        int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,                \
                         gr_vector_void_star &out) override                                                            \
        {                                                                                                              \
            return work_all_inputs(grhip_##NAME##_work, noutput_items, ninput_items, in, out);                         \
        }                                                                                                              \
    };                                                                                                                 \
    typedef boost::shared_ptr<grhip_##NAME##_blk> grhip_##NAME##_sptr;                                                 \
    inline grhip_##NAME##_sptr gr_make_##NAME(double db, double alpha = 0.0001, int ramp = 0, bool gate = false,       \
                                              int device = 0)                                                          \
    {                                                                                                                  \
        return grhip_detail::factory::make<grhip_##NAME##_blk>(db, alpha, ramp, gate, device);                         \
    }
GRHIP_PWR_SQUELCH_BLK(pwr_squelch_cc, gr_complex)
GRHIP_PWR_SQUELCH_BLK(pwr_squelch_ff, float)
#undef GRHIP_PWR_SQUELCH_BLK

class grhip_simple_squelch_cc_blk : public GRHIP_BLOCK(gr_sync_block, simple_squelch_cc) {
    friend struct grhip_detail::factory;
    grhip_simple_squelch_cc_blk(double threshold_db, double alpha, int device)
        : block("simple_squelch_cc", gr_make_io_signature(1, 1, sizeof(gr_complex)), gr_make_io_signature(1, 1, sizeof(gr_complex)))
    {
        grhip_detail::check(grhip_simple_squelch_cc_create(d_h.out(), threshold_db, alpha, device));
    }
public:
    bool unmuted() const { return checked(grhip_simple_squelch_cc_unmuted(d_h, 0)) != 0; }
    void set_alpha(double alpha) { grhip_detail::check(grhip_simple_squelch_cc_set_alpha(d_h, alpha)); }
    void set_threshold(double decibels) { grhip_detail::check(grhip_simple_squelch_cc_set_threshold(d_h, decibels)); }
    double threshold() const { return grhip_simple_squelch_cc_threshold(d_h); }
    std::vector<float> squelch_range() const { return grhip_detail::squelch_range(); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int produced = 0;
        grhip_detail::check(grhip_simple_squelch_cc_work(d_h, noutput_items, in[0], out[0], &produced));
        return noutput_items ? produced : 0;
    }
};
typedef boost::shared_ptr<grhip_simple_squelch_cc_blk> grhip_simple_squelch_cc_sptr;
inline grhip_simple_squelch_cc_sptr gr_make_simple_squelch_cc(double threshold_db, double alpha = 0.0001, int device = 0)
{
    return grhip_detail::factory::make<grhip_simple_squelch_cc_blk>(threshold_db, alpha, device);
}

// ---------------------------------------------------------------------------
// gr_ctcss_squelch_ff(rate, freq, level = 0.01, len = 0, ramp = 0, gate = false): gr_block over gr_squelch_base_ff;
// general_work consumes every input and returns the items produced (general/gr_ctcss_squelch_ff.h:33-66,
// gr_squelch_base_ff.cc:42-93).  The blocks of len samples run across general_work calls.
// ---------------------------------------------------------------------------
class grhip_ctcss_squelch_ff_blk : public GRHIP_BLOCK(gr_block, ctcss_squelch_ff) {
    friend struct grhip_detail::factory;
    grhip_ctcss_squelch_ff_blk(int rate, float freq, float level, int len, int ramp, bool gate, int device)
        : block("ctcss_squelch_ff", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(float)))
    {
        grhip_detail::check(grhip_ctcss_squelch_ff_create(d_h.out(), rate, freq, level, len, ramp, gate, device));
    }
public:
    float level() const { return grhip_ctcss_squelch_ff_level(d_h); }
    void set_level(float level) { grhip_detail::check(grhip_ctcss_squelch_ff_set_level(d_h, level)); }
    int len() const { return grhip_ctcss_squelch_ff_len(d_h); }
    int ramp() const { return grhip_ctcss_squelch_ff_ramp(d_h); }
    void set_ramp(int ramp) { grhip_detail::check(grhip_ctcss_squelch_ff_set_ramp(d_h, ramp)); }
    bool gate() const { return grhip_ctcss_squelch_ff_gate(d_h) != 0; }
    void set_gate(bool gate) { grhip_detail::check(grhip_ctcss_squelch_ff_set_gate(d_h, gate)); }
    bool unmuted() const { return checked(grhip_ctcss_squelch_ff_unmuted(d_h, 0)) != 0; }
    std::vector<float> squelch_range() const
    {
        std::vector<float> r(3);
        grhip_detail::check(grhip_ctcss_squelch_ff_squelch_range(r.data()));
        return r;
    }
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in,
                     gr_vector_void_star &out) override
    {
        return work_all_inputs(grhip_ctcss_squelch_ff_work, noutput_items, ninput_items, in, out);
    }
};
typedef boost::shared_ptr<grhip_ctcss_squelch_ff_blk> grhip_ctcss_squelch_ff_sptr;
inline grhip_ctcss_squelch_ff_sptr gr_make_ctcss_squelch_ff(int rate, float freq, float level = 0.01, int len = 0, int ramp = 0,
                                                            bool gate = false, int device = 0)
{
    return grhip_detail::factory::make<grhip_ctcss_squelch_ff_blk>(rate, freq, level, len, ramp, gate, device);
}

// ---------------------------------------------------------------------------
// gr_agc_cc / _ff (rate = 1e-4, reference = 1.0, gain = 1.0, max_gain = 0.0) and gr_agc2_cc / _ff (attack_rate = 1e-1,
// decay_rate = 1e-2, reference = 1.0, gain = 1.0, max_gain = 0.0): gr_sync_blocks, history 1, with the accessors and
// setters of gri_agc_cc / gri_agc2_cc that the reference's blocks inherit (general/gr_agc_cc.h:33-52,
// gr_agc2_cc.h:34-54).  The gain carries across work calls; the setters act at once.
// ---------------------------------------------------------------------------
namespace grhip_detail {
// what the four have in common: reference, gain and max_gain, and work.  T is the table GRHIP_AGC_FNS builds
template <class T, class ITEM> class agc_block : public block<gr_sync_block, typename T::H, T::destroy, T::set_mode> {
protected:
    agc_block() : agc_block::block(T::name, gr_make_io_signature(1, 1, sizeof(ITEM)), gr_make_io_signature(1, 1, sizeof(ITEM))) {}
public:
    float reference() const { return T::reference(this->d_h); }
    float max_gain() const { return T::max_gain(this->d_h); }
    float gain() const
    {
        float g = 0.f;
        check(T::gain(this->d_h, 0, &g));
        return g;
    }
    void set_reference(float reference) { check(T::set_reference(this->d_h, reference)); }
    void set_gain(float gain) { check(T::set_gain(this->d_h, gain)); }
    void set_max_gain(float max_gain) { check(T::set_max_gain(this->d_h, max_gain)); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        check(T::work(this->d_h, noutput_items, in[0], out[0]));
        return noutput_items;
    }
};
}  // namespace grhip_detail
#define GRHIP_AGC_FNS(NAME)                                                                                              \
    namespace grhip_detail {                                                                                             \
    struct NAME##_fns {                                                                                                  \
        typedef grhip_##NAME H;                                                                                          \
        static constexpr const char *name = #NAME;                                                                       \
        GRHIP_FN(NAME, destroy); GRHIP_FN(NAME, set_mode); GRHIP_FN(NAME, reference); GRHIP_FN(NAME, max_gain);          \
        GRHIP_FN(NAME, gain); GRHIP_FN(NAME, set_reference); GRHIP_FN(NAME, set_gain); GRHIP_FN(NAME, set_max_gain);     \
        GRHIP_FN(NAME, work);                                                                                            \
    };                                                                                                                   \
    }

#define GRHIP_AGC_BLK(NAME, ITEM)                                                                                        \
    GRHIP_AGC_FNS(NAME)                                                                                                  \
    class grhip_##NAME##_blk : public grhip_detail::agc_block<grhip_detail::NAME##_fns, ITEM> {                          \
        friend struct grhip_detail::factory;                                                                             \
        grhip_##NAME##_blk(float rate, float reference, float gain, float max_gain, int device)                          \
        {                                                                                                                \
            grhip_detail::check(grhip_##NAME##_create(d_h.out(), rate, reference, gain, max_gain, device));              \
        }                                                                                                                \
    public:                                                                                                              \
        float rate() const { return grhip_##NAME##_rate(d_h); }                                                          \
        void set_rate(float rate) { grhip_detail::check(grhip_##NAME##_set_rate(d_h, rate)); }                           \
    };                                                                                                                   \
    typedef boost::shared_ptr<grhip_##NAME##_blk> grhip_##NAME##_sptr;                                                   \
    inline grhip_##NAME##_sptr gr_make_##NAME(float rate = 1e-4, float reference = 1.0, float gain = 1.0,                \
                                              float max_gain = 0.0, int device = 0)                                      \
    {                                                                                                                    \
        return grhip_detail::factory::make<grhip_##NAME##_blk>(rate, reference, gain, max_gain, device);                 \
    }

#define GRHIP_AGC2_BLK(NAME, ITEM)                                                                                       \
    GRHIP_AGC_FNS(NAME)                                                                                                  \
    class grhip_##NAME##_blk : public grhip_detail::agc_block<grhip_detail::NAME##_fns, ITEM> {                          \
        friend struct grhip_detail::factory;                                                                             \
        grhip_##NAME##_blk(float attack_rate, float decay_rate, float reference, float gain, float max_gain, int device) \
        {                                                                                                                \
            grhip_detail::check(grhip_##NAME##_create(d_h.out(), attack_rate, decay_rate, reference, gain, max_gain, device)); \
        }                                                                                                                \
    public:                                                                                                              \
        float attack_rate() const { return grhip_##NAME##_attack_rate(d_h); }                                            \
        float decay_rate() const { return grhip_##NAME##_decay_rate(d_h); }                                              \
        void set_attack_rate(float rate) { grhip_detail::check(grhip_##NAME##_set_attack_rate(d_h, rate)); }             \
        void set_decay_rate(float rate) { grhip_detail::check(grhip_##NAME##_set_decay_rate(d_h, rate)); }               \
    };                                                                                                                   \
    typedef boost::shared_ptr<grhip_##NAME##_blk> grhip_##NAME##_sptr;                                                   \
    inline grhip_##NAME##_sptr gr_make_##NAME(float attack_rate = 1e-1, float decay_rate = 1e-2, float reference = 1.0,  \
                                              float gain = 1.0, float max_gain = 0.0, int device = 0)                    \
    {                                                                                                                    \
        return grhip_detail::factory::make<grhip_##NAME##_blk>(attack_rate, decay_rate, reference, gain, max_gain,       \
                                                               device);                                                  \
    }

GRHIP_AGC_BLK(agc_cc, gr_complex)
GRHIP_AGC_BLK(agc_ff, float)
GRHIP_AGC2_BLK(agc2_cc, gr_complex)
GRHIP_AGC2_BLK(agc2_ff, float)
#undef GRHIP_AGC_BLK
#undef GRHIP_AGC2_BLK
#undef GRHIP_AGC_FNS

// ---------------------------------------------------------------------------
// digital_costas_loop_cc (loop_bw, order; 1 input, 1..2 outputs: gr-digital/include/digital_costas_loop_cc.h:61-112) and
// gr_pll_freqdet_cf, gr_pll_refout_cc, gr_pll_carriertracking_cc (loop_bw, max_freq, min_freq;
// general/gr_pll_freqdet_cf.h:33-34 and siblings): gr_sync_blocks, history 1, with gri_control_loop's setters and
// getters under their names (general/gri_control_loop.h:99-200).  Phase and frequency carry across work calls; the
// setters act at once.  A value the reference refuses (std::out_of_range, std::invalid_argument) throws
// std::invalid_argument here.
// ---------------------------------------------------------------------------
namespace grhip_detail {
// gri_control_loop's interface over the handle of a block<BASE, ...>.  T is the table GRHIP_LOOP_FNS builds
template <class BASE, class T> class loop_block : public block<BASE, typename T::H, T::destroy, T::set_mode> {
protected:
    template <class... A> explicit loop_block(A &&...a) : loop_block::block(std::forward<A>(a)...) {}
public:
    void set_loop_bandwidth(float bw) { check(T::set_loop_bandwidth(this->d_h, bw)); }
    void set_damping_factor(float df) { check(T::set_damping_factor(this->d_h, df)); }
    void set_alpha(float alpha) { check(T::set_alpha(this->d_h, alpha)); }
    void set_beta(float beta) { check(T::set_beta(this->d_h, beta)); }
    void set_frequency(float freq) { check(T::set_frequency(this->d_h, freq)); }
    void set_phase(float phase) { check(T::set_phase(this->d_h, phase)); }
    float get_loop_bandwidth() const { return T::get_loop_bandwidth(this->d_h); }
    float get_damping_factor() const { return T::get_damping_factor(this->d_h); }
    float get_alpha() const { return T::get_alpha(this->d_h); }
    float get_beta() const { return T::get_beta(this->d_h); }
    float get_frequency() const
    {
        float v = 0.f;
        check(T::get_frequency(this->d_h, 0, &v));
        return v;
    }
    float get_phase() const
    {
        float v = 0.f;
        check(T::get_phase(this->d_h, 0, &v));
        return v;
    }
};
}  // namespace grhip_detail
#define GRHIP_LOOP_FNS(NAME)                                                                                             \
    namespace grhip_detail {                                                                                             \
    struct NAME##_fns {                                                                                                  \
        typedef grhip_##NAME H;                                                                                          \
        static constexpr const char *name = #NAME;                                                                       \
        GRHIP_FN(NAME, create); GRHIP_FN(NAME, destroy); GRHIP_FN(NAME, set_mode); GRHIP_FN(NAME, work);                 \
        GRHIP_FN(NAME, set_loop_bandwidth); GRHIP_FN(NAME, set_damping_factor); GRHIP_FN(NAME, set_alpha);               \
        GRHIP_FN(NAME, set_beta); GRHIP_FN(NAME, set_frequency); GRHIP_FN(NAME, set_phase);                              \
        GRHIP_FN(NAME, get_loop_bandwidth); GRHIP_FN(NAME, get_damping_factor); GRHIP_FN(NAME, get_alpha);               \
        GRHIP_FN(NAME, get_beta); GRHIP_FN(NAME, get_frequency); GRHIP_FN(NAME, get_phase);                              \
    };                                                                                                                   \
    }
#define GRHIP_LOOP_BLOCK(GRBASE, NAME) grhip_detail::loop_block<GRBASE, grhip_detail::NAME##_fns>
GRHIP_LOOP_FNS(pll_freqdet_cf)
GRHIP_LOOP_FNS(pll_refout_cc)
GRHIP_LOOP_FNS(pll_carriertracking_cc)
GRHIP_LOOP_FNS(costas_loop_cc)
GRHIP_LOOP_FNS(fll_band_edge_cc)
GRHIP_LOOP_FNS(constellation_receiver_cb)
GRHIP_LOOP_FNS(constellation_demod_cb)
#undef GRHIP_LOOP_FNS

// the three PLLs: complex in, OUT_ITEM out
template <class T, class OUT_ITEM> class grhip_pll_blk : public grhip_detail::loop_block<gr_sync_block, T> {
    friend struct grhip_detail::factory;
protected:
    grhip_pll_blk(float loop_bw, float max_freq, float min_freq, int device)
        : grhip_pll_blk::loop_block(T::name, gr_make_io_signature(1, 1, sizeof(gr_complex)), gr_make_io_signature(1, 1, sizeof(OUT_ITEM)))
    {
        grhip_detail::check(T::create(this->d_h.out(), loop_bw, max_freq, min_freq, device));
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(T::work(this->d_h, noutput_items, in[0], out[0]));
        return noutput_items;
    }
};
typedef grhip_pll_blk<grhip_detail::pll_freqdet_cf_fns, float> grhip_pll_freqdet_cf_blk;
typedef grhip_pll_blk<grhip_detail::pll_refout_cc_fns, gr_complex> grhip_pll_refout_cc_blk;
class grhip_pll_carriertracking_cc_blk : public grhip_pll_blk<grhip_detail::pll_carriertracking_cc_fns, gr_complex> {
    friend struct grhip_detail::factory;
    using grhip_pll_blk::grhip_pll_blk;
public:
    // general/gr_pll_carriertracking_cc.h:84-90
    bool lock_detector()
    {
        int locked = 0;
        grhip_detail::check(grhip_pll_carriertracking_cc_lock_detector(d_h, 0, &locked));
        return locked != 0;
    }
    bool squelch_enable(bool enable)
    {
        grhip_detail::check(grhip_pll_carriertracking_cc_squelch_enable(d_h, enable ? 1 : 0));
        return enable;
    }
    float set_lock_threshold(float threshold)
    {
        grhip_detail::check(grhip_pll_carriertracking_cc_set_lock_threshold(d_h, threshold));
        return threshold;
    }
};
#define GRHIP_PLL_MAKE(NAME)                                                                                             \
    typedef boost::shared_ptr<grhip_##NAME##_blk> grhip_##NAME##_sptr;                                                   \
    inline grhip_##NAME##_sptr gr_make_##NAME(float loop_bw, float max_freq, float min_freq, int device = 0)             \
    {                                                                                                                    \
        return grhip_detail::factory::make<grhip_##NAME##_blk>(loop_bw, max_freq, min_freq, device);                     \
    }
GRHIP_PLL_MAKE(pll_freqdet_cf)
GRHIP_PLL_MAKE(pll_refout_cc)
GRHIP_PLL_MAKE(pll_carriertracking_cc)
#undef GRHIP_PLL_MAKE

class grhip_costas_loop_cc_blk : public GRHIP_LOOP_BLOCK(gr_sync_block, costas_loop_cc) {
    friend struct grhip_detail::factory;
    grhip_costas_loop_cc_blk(float loop_bw, int order, int device)
        : loop_block("costas_loop_cc", gr_make_io_signature(1, 1, sizeof(gr_complex)),
                     gr_make_io_signature2(1, 2, sizeof(gr_complex), sizeof(float)))     // digital_costas_loop_cc.cc:43-45
    {
        grhip_detail::check(grhip_costas_loop_cc_create(d_h.out(), loop_bw, order, device));
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        // the second output is optional (digital_costas_loop_cc.cc:119)
        grhip_detail::check(grhip_costas_loop_cc_work(d_h, noutput_items, in[0], out[0], out.size() >= 2 ? out[1] : nullptr));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_costas_loop_cc_blk> grhip_costas_loop_cc_sptr;
inline grhip_costas_loop_cc_sptr digital_make_costas_loop_cc(float loop_bw, int order, int device = 0)
{
    return grhip_detail::factory::make<grhip_costas_loop_cc_blk>(loop_bw, order, device);
}
// ---------------------------------------------------------------------------
// digital_fll_band_edge_cc (samps_per_sym, rolloff, filter_size, bandwidth; 1 input, 1 or 4 outputs: the derotated
// samples and, with all four connected, the loop's frequency, phase and error; gr-digital/include/
// digital_fll_band_edge_cc.h).  A gr_sync_block with history filter_size + 1, as the reference's: the scheduler hands
// work the filter_size items before the new ones too, the handle keeps what it needs of the past itself and takes the
// new items only (include/grhip.h states what is computed).  gr_firdes::root_raised_cosine comes with it.
// ---------------------------------------------------------------------------
class grhip_fll_band_edge_cc_blk : public GRHIP_LOOP_BLOCK(gr_sync_block, fll_band_edge_cc) {
    friend struct grhip_detail::factory;
    static std::vector<int> iosig() { return {(int)sizeof(gr_complex), (int)sizeof(float), (int)sizeof(float), (int)sizeof(float)}; }
    grhip_fll_band_edge_cc_blk(float samps_per_sym, float rolloff, int filter_size, float bandwidth, int device)
        : loop_block("fll_band_edge_cc", gr_make_io_signature(1, 1, sizeof(gr_complex)),
                     gr_make_io_signaturev(1, 4, iosig()))                                   // digital_fll_band_edge_cc.cc:51-57
    {
        grhip_detail::check(grhip_fll_band_edge_cc_create(d_h.out(), samps_per_sym, rolloff, filter_size, bandwidth, device));
        set_history(filter_size + 1);                                                       // :187
    }
public:
    void set_samples_per_symbol(float sps) { grhip_detail::check(grhip_fll_band_edge_cc_set_samples_per_symbol(d_h, sps)); }
    void set_rolloff(float rolloff) { grhip_detail::check(grhip_fll_band_edge_cc_set_rolloff(d_h, rolloff)); }
    void set_filter_size(int filter_size)
    {
        grhip_detail::check(grhip_fll_band_edge_cc_set_filter_size(d_h, filter_size));
        set_history(filter_size + 1);
    }
    float get_samples_per_symbol() const { return grhip_fll_band_edge_cc_get_samples_per_symbol(d_h); }
    float get_rolloff() const { return grhip_fll_band_edge_cc_get_rolloff(d_h); }
    int get_filter_size() const { return checked(grhip_fll_band_edge_cc_get_filter_size(d_h)); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        const gr_complex *fresh = (const gr_complex *)in[0] + (history() - 1);
        const bool aux = out.size() == 4;                                                   // :219
        grhip_detail::check(grhip_fll_band_edge_cc_work(d_h, noutput_items, fresh, out[0], aux ? out[1] : nullptr,
                                                         aux ? out[2] : nullptr, aux ? out[3] : nullptr));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_fll_band_edge_cc_blk> grhip_fll_band_edge_cc_sptr;
inline grhip_fll_band_edge_cc_sptr digital_make_fll_band_edge_cc(float samps_per_sym, float rolloff, int filter_size, float bandwidth,
                                                                 int device = 0)
{
    return grhip_detail::factory::make<grhip_fll_band_edge_cc_blk>(samps_per_sym, rolloff, filter_size, bandwidth, device);
}

// ---------------------------------------------------------------------------
// gr_pfb_clock_sync_ccf (sps, loop_bw, taps, filter_size = 32, init_phase = 0, max_rate_deviation = 1.5, osps = 1; 1 input,
// 1 or 4 outputs: the symbols and, with all four connected, the loop's error, rate and phase; filter/
// gr_pfb_clock_sync_ccf.h).  A gr_block with history taps_per_filter + floor(sps), as the reference's: the scheduler
// hands general_work those items before the new ones too, the handle keeps what it needs of the past itself and takes
// the new items only (include/grhip.h states what is computed).  general_work takes as many new items as noutput_items
// surely holds the symbols of (osps (items + floor(sps)) <= noutput_items), consumes them all and returns the items
// produced; a symbol whose last items have not arrived comes with a later call.  output_multiple() is osps (floor(sps) + 1),
// so that a scheduler never offers less space than one new item may need.  set_taps is not offered.
// ---------------------------------------------------------------------------
class grhip_pfb_clock_sync_ccf_blk : public GRHIP_BLOCK(gr_block, pfb_clock_sync_ccf) {
    friend struct grhip_detail::factory;
    int d_nfilters = 0, d_tpf = 0, d_isps = 0, d_osps = 0;
    static std::vector<int> iosig() { return {(int)sizeof(gr_complex), (int)sizeof(float), (int)sizeof(float), (int)sizeof(float)}; }
    grhip_pfb_clock_sync_ccf_blk(double sps, float loop_bw, const std::vector<float> &taps, unsigned int filter_size, float init_phase,
                                 float max_rate_deviation, int osps, int device)
        : block("pfb_clock_sync_ccf", gr_make_io_signature(1, 1, sizeof(gr_complex)), gr_make_io_signaturev(1, 4, iosig()))  // .cc:58-60
    {
        grhip_detail::check(grhip_pfb_clock_sync_ccf_create(d_h.out(), sps, loop_bw, taps.data(), (int)taps.size(),
                                                             filter_size > 0x7fffffffu ? -1 : (int)filter_size, init_phase,
                                                             max_rate_deviation, osps, device));
        grhip_detail::check(grhip_pfb_clock_sync_taps(taps.data(), (int)taps.size(), (int)filter_size, nullptr, nullptr, &d_tpf));
        d_nfilters = (int)filter_size;
        d_isps = (int)floor(sps);
        d_osps = osps;
        set_history(d_tpf + d_isps);                                                        // .cc:245
        // the least output space that surely holds the symbols of one new item (general_work below); the reference
        // sets none and leaves noutput_items - osps of its space unused instead (.cc:379)
        set_output_multiple(d_osps * (d_isps + 1));
    }
    float stream_float(int (*get)(grhip_pfb_clock_sync_ccf *, int, float *)) const
    {
        float v = 0;
        grhip_detail::check(get(d_h, 0, &v));
        return v;
    }
    std::vector<std::vector<float> > bank(int (*get)(grhip_pfb_clock_sync_ccf *, float *, size_t, int *, int *)) const
    {
        std::vector<float> flat((size_t)d_nfilters * d_tpf);
        int nf = 0, tpf = 0;
        grhip_detail::check(get(d_h, flat.data(), flat.size(), &nf, &tpf));
        std::vector<std::vector<float> > b(nf);
        for (int f = 0; f < nf; ++f) b[f].assign(flat.begin() + (size_t)f * tpf, flat.begin() + (size_t)(f + 1) * tpf);
        return b;
    }
public:
    std::vector<std::vector<float> > get_taps() const { return bank(grhip_pfb_clock_sync_ccf_get_taps); }
    std::vector<std::vector<float> > get_diff_taps() const { return bank(grhip_pfb_clock_sync_ccf_get_diff_taps); }
    std::vector<float> get_channel_taps(int channel) const { return get_taps().at(channel); }
    std::vector<float> get_diff_channel_taps(int channel) const { return get_diff_taps().at(channel); }
    void set_loop_bandwidth(float bw) { grhip_detail::check(grhip_pfb_clock_sync_ccf_set_loop_bandwidth(d_h, bw)); }
    void set_damping_factor(float df) { grhip_detail::check(grhip_pfb_clock_sync_ccf_set_damping_factor(d_h, df)); }
    void set_alpha(float alpha) { grhip_detail::check(grhip_pfb_clock_sync_ccf_set_alpha(d_h, alpha)); }
    void set_beta(float beta) { grhip_detail::check(grhip_pfb_clock_sync_ccf_set_beta(d_h, beta)); }
    void set_max_rate_deviation(float m) { grhip_detail::check(grhip_pfb_clock_sync_ccf_set_max_rate_deviation(d_h, m)); }
    float get_loop_bandwidth() const { return grhip_pfb_clock_sync_ccf_get_loop_bandwidth(d_h); }
    float get_damping_factor() const { return grhip_pfb_clock_sync_ccf_get_damping_factor(d_h); }
    float get_alpha() const { return grhip_pfb_clock_sync_ccf_get_alpha(d_h); }
    float get_beta() const { return grhip_pfb_clock_sync_ccf_get_beta(d_h); }
    float get_clock_rate() const { return stream_float(grhip_pfb_clock_sync_ccf_get_clock_rate); }
    float k() const { return stream_float(grhip_pfb_clock_sync_ccf_k); }
    float error() const { return stream_float(grhip_pfb_clock_sync_ccf_error); }
    int slips() const
    {
        int v = 0;
        grhip_detail::check(grhip_pfb_clock_sync_ccf_slips(d_h, 0, &v));
        return v;
    }
    bool check_topology(int, int noutputs) { return noutputs == 1 || noutputs == 4; }       // .cc:108-112
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        const int hist = (int)history() - 1;
        const long long fresh_n = (long long)ninput_items[0] - hist, room = (long long)(noutput_items / d_osps) - d_isps;
        const int n = (int)(fresh_n < room ? fresh_n : room);
        if (n <= 0) {
            consume_each(0);
            return 0;
        }
        const gr_complex *fresh = (const gr_complex *)in[0] + hist;
        const bool aux = out.size() == 4;                                                   // .cc:361
        int produced = 0;
        grhip_detail::check(grhip_pfb_clock_sync_ccf_work(d_h, n, fresh, noutput_items, out[0], aux ? out[1] : nullptr, aux ? out[2] : nullptr,
                                                           aux ? out[3] : nullptr, &produced));
        consume_each(n);
        return produced;
    }
};
typedef boost::shared_ptr<grhip_pfb_clock_sync_ccf_blk> grhip_pfb_clock_sync_ccf_sptr;
inline grhip_pfb_clock_sync_ccf_sptr gr_make_pfb_clock_sync_ccf(double sps, float loop_bw, const std::vector<float> &taps,
                                                                unsigned int filter_size = 32, float init_phase = 0,
                                                                float max_rate_deviation = 1.5, int osps = 1, int device = 0)
{
    return grhip_detail::factory::make<grhip_pfb_clock_sync_ccf_blk>(sps, loop_bw, taps, filter_size, init_phase, max_rate_deviation,
                                                                     osps, device);
}

// gr_firdes::root_raised_cosine(gain, sampling_freq, symbol_rate, alpha, ntaps)
inline std::vector<float> grhip_firdes_root_raised_cosine_taps(double gain, double sampling_freq, double symbol_rate, double alpha, int ntaps)
{
    size_t n = 0;
    const int rc = grhip_firdes_root_raised_cosine(gain, sampling_freq, symbol_rate, alpha, ntaps, nullptr, 0, &n);
    if (rc != GRHIP_ERANGE) grhip_detail::check(rc);
    std::vector<float> taps(n);
    grhip_detail::check(grhip_firdes_root_raised_cosine(gain, sampling_freq, symbol_rate, alpha, ntaps, taps.data(), n, &n));
    return taps;
}
// ---------------------------------------------------------------------------
// digital_constellation and its kinds (gr-digital/include/digital_constellation.h), digital_constellation_decoder_cb
// (constellation), digital_constellation_receiver_cb (constellation, loop_bw, fmin, fmax; 1 input, 1 or 4 outputs),
// gr_diff_decoder_bb (modulus), gr_map_bb (map), and constellation_demod_cb, the tail of generic_demod
// (gr-digital/python/generic_mod_demod.py:296-313) as one block.  A constellation is a host object; a block copies the
// one it is made from.  What the reference refuses with std::runtime_error throws std::invalid_argument here.
// ---------------------------------------------------------------------------
namespace grhip_detail {
typedef handle<grhip_constellation, grhip_constellation_destroy> constellation_handle;
}
class grhip_constellation_obj {
    grhip_detail::constellation_handle d_h;
public:
    explicit grhip_constellation_obj(grhip_constellation *h) : d_h(h) {}
    explicit grhip_constellation_obj(grhip_detail::constellation_handle &&h) : d_h(std::move(h)) {}
    const grhip_constellation *handle() const { return d_h; }
    std::vector<gr_complex> points() const
    {
        std::vector<gr_complex> p((size_t)grhip_constellation_points(d_h, nullptr, 0));
        grhip_constellation_points(d_h, (float *)p.data(), p.size());
        return p;
    }
    std::vector<unsigned int> pre_diff_code() const
    {
        std::vector<unsigned int> c((size_t)grhip_constellation_pre_diff_code(d_h, nullptr, 0));
        grhip_constellation_pre_diff_code(d_h, c.data(), c.size());
        return c;
    }
    bool apply_pre_diff_code() const { return grhip_constellation_apply_pre_diff_code(d_h) != 0; }
    unsigned int rotational_symmetry() const { return (unsigned)grhip_constellation_rotational_symmetry(d_h); }
    unsigned int dimensionality() const { return (unsigned)grhip_constellation_dimensionality(d_h); }
    unsigned int arity() const { return (unsigned)grhip_constellation_arity(d_h); }
    unsigned int bits_per_symbol() const { return (unsigned)grhip_constellation_bits_per_symbol(d_h); }
    unsigned int decision_maker(const gr_complex *sample) const
    {
        unsigned k = 0;
        grhip_detail::check(grhip_constellation_decision_maker(d_h, (const float *)sample, &k));
        return k;
    }
    unsigned int decision_maker_pe(const gr_complex *sample, float *phase_error) const
    {
        unsigned k = 0;
        grhip_detail::check(grhip_constellation_decision_maker_pe(d_h, (const float *)sample, &k, phase_error));
        return k;
    }
};
typedef boost::shared_ptr<grhip_constellation_obj> grhip_constellation_sptr;
namespace grhip_detail {
inline grhip_constellation_sptr constellation(int rc, constellation_handle &h)
{
    check(rc);
    return grhip_constellation_sptr(new grhip_constellation_obj(std::move(h)));
}
}  // namespace grhip_detail
#define GRHIP_CONSTELLATION_FIXED(KIND)                                                                                  \
    inline grhip_constellation_sptr digital_make_constellation_##KIND()                                                  \
    {                                                                                                                    \
        grhip_detail::constellation_handle h;                                                                            \
        const int rc = grhip_constellation_create_##KIND(h.out());                                                       \
        return grhip_detail::constellation(rc, h);                                                                       \
    }
GRHIP_CONSTELLATION_FIXED(bpsk)
GRHIP_CONSTELLATION_FIXED(qpsk)
GRHIP_CONSTELLATION_FIXED(dqpsk)
GRHIP_CONSTELLATION_FIXED(8psk)
#undef GRHIP_CONSTELLATION_FIXED
inline grhip_constellation_sptr digital_make_constellation_calcdist(std::vector<gr_complex> constellation, std::vector<unsigned int> pre_diff_code,
                                                                    unsigned int rotational_symmetry, unsigned int dimensionality)
{
    grhip_detail::constellation_handle h;
    const int rc = grhip_constellation_create_calcdist(h.out(), (const float *)constellation.data(), constellation.size(), pre_diff_code.data(),
                                                       pre_diff_code.size(), rotational_symmetry, dimensionality);
    return grhip_detail::constellation(rc, h);
}
inline grhip_constellation_sptr digital_make_constellation_psk(std::vector<gr_complex> constellation, std::vector<unsigned int> pre_diff_code,
                                                               unsigned int n_sectors)
{
    grhip_detail::constellation_handle h;
    const int rc = grhip_constellation_create_psk(h.out(), (const float *)constellation.data(), constellation.size(), pre_diff_code.data(),
                                                  pre_diff_code.size(), n_sectors);
    return grhip_detail::constellation(rc, h);
}
inline grhip_constellation_sptr digital_make_constellation_rect(std::vector<gr_complex> constellation, std::vector<unsigned int> pre_diff_code,
                                                                unsigned int rotational_symmetry, unsigned int real_sectors,
                                                                unsigned int imag_sectors, float width_real_sectors, float width_imag_sectors)
{
    grhip_detail::constellation_handle h;
    const int rc = grhip_constellation_create_rect(h.out(), (const float *)constellation.data(), constellation.size(), pre_diff_code.data(),
                                                   pre_diff_code.size(), rotational_symmetry, real_sectors, imag_sectors, width_real_sectors,
                                                   width_imag_sectors);
    return grhip_detail::constellation(rc, h);
}

// digital_constellation_decoder_cb.cc:39-78: a gr_block, `dimensionality` complex items per output byte
class grhip_constellation_decoder_cb_blk : public GRHIP_BLOCK_NO_MODE(gr_block, constellation_decoder_cb) {
    friend struct grhip_detail::factory;
    unsigned d_dim;
    grhip_constellation_decoder_cb_blk(grhip_constellation_sptr c, int device)
        : block("constellation_decoder_cb", gr_make_io_signature(1, 1, sizeof(gr_complex)), gr_make_io_signature(1, 1, sizeof(unsigned char))),
          d_dim(c->dimensionality())
    {
        set_relative_rate(1.0 / ((double)d_dim));
        grhip_detail::check(grhip_constellation_decoder_cb_create(d_h.out(), c->handle(), device));
    }
public:
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        for (size_t i = 0; i < req.size(); i++) req[i] = noutput_items * d_dim;
    }
    int general_work(int noutput_items, gr_vector_int &, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_constellation_decoder_cb_work(d_h, noutput_items, in[0], out[0]));
        consume_each(noutput_items * d_dim);
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_constellation_decoder_cb_blk> grhip_constellation_decoder_cb_sptr;
inline grhip_constellation_decoder_cb_sptr digital_make_constellation_decoder_cb(grhip_constellation_sptr constellation, int device = 0)
{
    return grhip_detail::factory::make<grhip_constellation_decoder_cb_blk>(constellation, device);
}

// gr_diff_decoder_bb.cc:36-61: a gr_sync_block with history 2.  in[0] is the byte in front of the first output's; the
// handle keeps that byte itself (the last one of the call before, 0 at the start, which is what the scheduler's
// history holds), so the work call hands it the items from in[1] on.
class grhip_diff_decoder_bb_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_block, diff_decoder_bb) {
    friend struct grhip_detail::factory;
    grhip_diff_decoder_bb_blk(unsigned int modulus, int device)
        : block("diff_decoder_bb", gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(1, 1, sizeof(unsigned char)))
    {
        set_history(2);
        grhip_detail::check(grhip_diff_decoder_bb_create(d_h.out(), modulus, device));
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_diff_decoder_bb_work(d_h, noutput_items, (const unsigned char *)in[0] + 1, out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_diff_decoder_bb_blk> grhip_diff_decoder_bb_sptr;
inline grhip_diff_decoder_bb_sptr gr_make_diff_decoder_bb(unsigned int modulus, int device = 0)
{
    return grhip_detail::factory::make<grhip_diff_decoder_bb_blk>(modulus, device);
}

// gr_map_bb.cc:36-60
class grhip_map_bb_blk : public GRHIP_BLOCK_NO_MODE(gr_sync_block, map_bb) {
    friend struct grhip_detail::factory;
    grhip_map_bb_blk(const std::vector<int> &map, int device)
        : block("map_bb", gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(1, 1, sizeof(unsigned char)))
    {
        grhip_detail::check(grhip_map_bb_create(d_h.out(), map.data(), map.size(), device));
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_map_bb_work(d_h, noutput_items, in[0], out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_map_bb_blk> grhip_map_bb_sptr;
inline grhip_map_bb_sptr gr_make_map_bb(const std::vector<int> &map, int device = 0)
{
    return grhip_detail::factory::make<grhip_map_bb_blk>(map, device);
}

// digital_constellation_receiver_cb.cc:52-122: a gr_block with gri_control_loop's interface; outputs 2 .. 4 (error,
// phase, frequency) are connected all three or not at all
class grhip_constellation_receiver_cb_blk : public GRHIP_LOOP_BLOCK(gr_block, constellation_receiver_cb) {
    friend struct grhip_detail::factory;
    grhip_constellation_receiver_cb_blk(grhip_constellation_sptr c, float loop_bw, float fmin, float fmax, int device)
        : loop_block("constellation_receiver_cb", gr_make_io_signature(1, 1, sizeof(gr_complex)),
                     gr_make_io_signature2(1, 4, sizeof(char), sizeof(float)))                    // :50-56
    {
        grhip_detail::check(grhip_constellation_receiver_cb_create(d_h.out(), c->handle(), loop_bw, fmin, fmax, device));
    }
public:
    int form() const { return grhip_constellation_receiver_cb_form(d_h); }
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        const int n = std::min(noutput_items, ninput_items[0]);                                 // :102
        const bool four = out.size() == 4;                                                      // :96
        grhip_detail::check(grhip_constellation_receiver_cb_work(d_h, n, in[0], out[0], four ? out[1] : nullptr, four ? out[2] : nullptr,
                                                                 four ? out[3] : nullptr));
        consume_each(n);
        return n;
    }
};
typedef boost::shared_ptr<grhip_constellation_receiver_cb_blk> grhip_constellation_receiver_cb_sptr;
inline grhip_constellation_receiver_cb_sptr digital_make_constellation_receiver_cb(grhip_constellation_sptr constellation, float loop_bw,
                                                                                   float fmin, float fmax, int device = 0)
{
    return grhip_detail::factory::make<grhip_constellation_receiver_cb_blk>(constellation, loop_bw, fmin, fmax, device);
}

// the receiver, diff_decoder_bb(arity) if differential, map_bb(invert_code(pre_diff_code)) if gray_coded and the
// constellation applies one, unpack_k_bits_bb(bits_per_symbol): bits_per_symbol bytes out per complex item in
class grhip_constellation_demod_cb_blk : public GRHIP_LOOP_BLOCK(gr_sync_interpolator, constellation_demod_cb) {
    friend struct grhip_detail::factory;
    grhip_constellation_demod_cb_blk(grhip_constellation_sptr c, float loop_bw, float fmin, float fmax, bool differential, bool gray_coded, int device)
        : loop_block("constellation_demod_cb", gr_make_io_signature(1, 1, sizeof(gr_complex)),
                     gr_make_io_signature(1, 1, sizeof(unsigned char)), std::max(1u, c->bits_per_symbol()))
    {
        grhip_detail::check(grhip_constellation_demod_cb_create(d_h.out(), c->handle(), loop_bw, fmin, fmax, differential, gray_coded, device));
    }
public:
    int form() const { return grhip_constellation_demod_cb_form(d_h); }
    int engine() const { return grhip_constellation_demod_cb_engine(d_h); }
    void set_engine(int engine) { grhip_detail::check(grhip_constellation_demod_cb_set_engine(d_h, engine)); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_constellation_demod_cb_work(d_h, noutput_items / (int)interpolation(), in[0], out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_constellation_demod_cb_blk> grhip_constellation_demod_cb_sptr;
inline grhip_constellation_demod_cb_sptr grhip_make_constellation_demod_cb(grhip_constellation_sptr constellation, float loop_bw, float fmin,
                                                                           float fmax, bool differential = true, bool gray_coded = true,
                                                                           int device = 0)
{
    return grhip_detail::factory::make<grhip_constellation_demod_cb_blk>(constellation, loop_bw, fmin, fmax, differential, gray_coded, device);
}
#undef GRHIP_LOOP_BLOCK

// ---------------------------------------------------------------------------
// The modulator: gr_packed_to_unpacked_bb / gr_unpacked_to_packed_bb (bits_per_chunk, endianness;
// gengen/gr_packed_to_unpacked_XX.h.t, gr_unpacked_to_packed_XX.h.t: gr_blocks with their own forecast),
// gr_diff_encoder_bb (modulus; general/gr_diff_encoder_bb.h: a gr_sync_block), gr_chunks_to_symbols_bc (symbol_table,
// D = 1; gengen/gr_chunks_to_symbols_XX.h.t: a gr_sync_interpolator by D) and generic_mod
// (gr-digital/python/generic_mod_demod.py:76-157) as one gr_block.  One stream each.
// ---------------------------------------------------------------------------
template <class T>
class grhip_repack_bb_blk : public grhip_detail::block<gr_block, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    grhip_repack_bb_blk(unsigned int bits_per_chunk, gr_endianness_t endianness, int device)
        : grhip_repack_bb_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(1, 1, sizeof(unsigned char)))
    {
        grhip_detail::check(T::create(this->d_h.out(), bits_per_chunk, (int)endianness, device));      // refuses 0 and above 8
        this->set_relative_rate(T::unpacks ? 8.0 / bits_per_chunk : bits_per_chunk / 8.0);              // .cc.t:55 / :53
    }
public:
    void forecast(int noutput_items, gr_vector_int &ninput_items_required) override
    {
        this->forecast_each(T::forecast, noutput_items, ninput_items_required);                         // .cc.t:62 / :59
    }
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        return this->work_consumed(T::general_work, noutput_items, ninput_items, in, out);
    }
};
namespace grhip_detail {
struct packed_to_unpacked_bb_fns {
    typedef grhip_packed_to_unpacked_bb H;
    static constexpr const char *name = "packed_to_unpacked_bb";
    static constexpr bool unpacks = true;
    GRHIP_FN(packed_to_unpacked_bb, create); GRHIP_FN(packed_to_unpacked_bb, destroy); GRHIP_FN(packed_to_unpacked_bb, set_mode);
    GRHIP_FN(packed_to_unpacked_bb, forecast); GRHIP_FN(packed_to_unpacked_bb, general_work);
};
struct unpacked_to_packed_bb_fns {
    typedef grhip_unpacked_to_packed_bb H;
    static constexpr const char *name = "unpacked_to_packed_bb";
    static constexpr bool unpacks = false;
    GRHIP_FN(unpacked_to_packed_bb, create); GRHIP_FN(unpacked_to_packed_bb, destroy); GRHIP_FN(unpacked_to_packed_bb, set_mode);
    GRHIP_FN(unpacked_to_packed_bb, forecast); GRHIP_FN(unpacked_to_packed_bb, general_work);
};
}  // namespace grhip_detail
typedef grhip_repack_bb_blk<grhip_detail::packed_to_unpacked_bb_fns> grhip_packed_to_unpacked_bb_blk;
typedef grhip_repack_bb_blk<grhip_detail::unpacked_to_packed_bb_fns> grhip_unpacked_to_packed_bb_blk;
typedef boost::shared_ptr<grhip_packed_to_unpacked_bb_blk> grhip_packed_to_unpacked_bb_sptr;
typedef boost::shared_ptr<grhip_unpacked_to_packed_bb_blk> grhip_unpacked_to_packed_bb_sptr;
inline grhip_packed_to_unpacked_bb_sptr grhip_make_packed_to_unpacked_bb(unsigned int bits_per_chunk, gr_endianness_t endianness, int device = 0)
{
    return grhip_detail::factory::make<grhip_packed_to_unpacked_bb_blk>(bits_per_chunk, endianness, device);
}
inline grhip_unpacked_to_packed_bb_sptr grhip_make_unpacked_to_packed_bb(unsigned int bits_per_chunk, gr_endianness_t endianness, int device = 0)
{
    return grhip_detail::factory::make<grhip_unpacked_to_packed_bb_blk>(bits_per_chunk, endianness, device);
}

class grhip_diff_encoder_bb_blk : public GRHIP_BLOCK(gr_sync_block, diff_encoder_bb) {
    friend struct grhip_detail::factory;
    grhip_diff_encoder_bb_blk(unsigned int modulus, int device)
        : block("diff_encoder_bb", gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(1, 1, sizeof(unsigned char)))
    {
        grhip_detail::check(grhip_diff_encoder_bb_create(d_h.out(), modulus, device));
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_diff_encoder_bb_work(d_h, noutput_items, in[0], out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_diff_encoder_bb_blk> grhip_diff_encoder_bb_sptr;
inline grhip_diff_encoder_bb_sptr grhip_make_diff_encoder_bb(unsigned int modulus, int device = 0)
{
    return grhip_detail::factory::make<grhip_diff_encoder_bb_blk>(modulus, device);
}

class grhip_chunks_to_symbols_bc_blk : public GRHIP_BLOCK(gr_sync_interpolator, chunks_to_symbols_bc) {
    friend struct grhip_detail::factory;
    std::vector<gr_complex> d_symbol_table;
    grhip_chunks_to_symbols_bc_blk(const std::vector<gr_complex> &symbol_table, const int D, int device)
        : block("chunks_to_symbols_bc", gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(1, 1, sizeof(gr_complex)),
                (unsigned)(D < 1 ? 1 : D)),
          d_symbol_table(symbol_table)
    {
        grhip_detail::check(grhip_chunks_to_symbols_bc_create(d_h.out(), (const float *)symbol_table.data(), symbol_table.size(), D, device));
    }
public:
    int D() const { return (int)interpolation(); }
    std::vector<gr_complex> symbol_table() const { return d_symbol_table; }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_chunks_to_symbols_bc_work(d_h, noutput_items / (int)interpolation(), in[0], out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_chunks_to_symbols_bc_blk> grhip_chunks_to_symbols_bc_sptr;
inline grhip_chunks_to_symbols_bc_sptr grhip_make_chunks_to_symbols_bc(const std::vector<gr_complex> &symbol_table, const int D = 1, int device = 0)
{
    return grhip_detail::factory::make<grhip_chunks_to_symbols_bc_blk>(symbol_table, D, device);
}

// generic_mod: bytes in, complex samples out.  The handle takes new bytes only and keeps what the chain's blocks would
// keep, so a call consumes whole bytes: as many as still fit noutput_items, which the handle tells in advance
// (max_produced).  The output multiple is what one byte can bring at most, so that a call always has room for a byte;
// forecast asks for the bytes that are sure to fit, at least one.
class grhip_generic_mod_blk : public GRHIP_BLOCK(gr_block, generic_mod) {
    friend struct grhip_detail::factory;
    int d_k = 1;
    double d_sps = 2;
    grhip_generic_mod_blk(grhip_constellation_sptr c, double samples_per_symbol, bool differential, double excess_bw, bool gray_coded, int device)
        : block("generic_mod", gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(1, 1, sizeof(gr_complex)))
    {
        grhip_detail::check(grhip_generic_mod_create(d_h.out(), c->handle(), samples_per_symbol, differential, excess_bw, gray_coded, device));
        d_k = bits_per_symbol();
        d_sps = samples_per_symbol;
        set_relative_rate(8.0 / d_k * d_sps);
        set_output_multiple((int)most(1));
    }
    // no call of n bytes brings more: the symbols that n bytes and k - 1 carried bits complete, each at most
    // ceil(samples_per_symbol) samples
    long long most(long long n_bytes) const { return ((8 * n_bytes + d_k - 1) / d_k) * (long long)std::ceil(d_sps); }
public:
    int bits_per_symbol() const { return grhip_generic_mod_bits_per_symbol(d_h); }
    double samples_per_symbol() const { return grhip_generic_mod_samples_per_symbol(d_h); }
    int engine() const { return grhip_generic_mod_engine(d_h); }
    void set_engine(int engine) { grhip_detail::check(grhip_generic_mod_set_engine(d_h, engine)); }
    std::vector<float> taps() const
    {
        std::vector<float> t((size_t)grhip_generic_mod_ntaps(d_h));
        grhip_generic_mod_taps(d_h, t.data(), t.size());
        return t;
    }
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        long long n = (long long)(noutput_items / (std::ceil(d_sps) * 8.0 / d_k));
        while (n > 1 && most(n) > noutput_items) --n;
        for (size_t i = 0; i < req.size(); i++) req[i] = n < 1 ? 1 : (int)n;
    }
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        long long n = std::min<long long>(ninput_items[0], (long long)(noutput_items / relative_rate()) + 1);
        while (n > 0 && grhip_generic_mod_max_produced(d_h, (int)n) > noutput_items) --n;       // the most bytes whose samples fit
        long long produced = 0;
        if (n > 0) grhip_detail::check(grhip_generic_mod_work(d_h, (int)n, in[0], out[0], noutput_items, &produced));
        consume_each((int)n);
        return (int)produced;
    }
};
typedef boost::shared_ptr<grhip_generic_mod_blk> grhip_generic_mod_sptr;
inline grhip_generic_mod_sptr grhip_make_generic_mod(grhip_constellation_sptr constellation, double samples_per_symbol = 2, bool differential = false,
                                                     double excess_bw = 0.35, bool gray_coded = true, int device = 0)
{
    return grhip_detail::factory::make<grhip_generic_mod_blk>(constellation, samples_per_symbol, differential, excess_bw, gray_coded, device);
}

// ---------------------------------------------------------------------------
// gr_scrambler_bb, gr_descrambler_bb (mask, seed, len) and gr_additive_scrambler_bb (mask, seed, len, count = 0):
// general/gr_scrambler_bb.h:31-32, gr_descrambler_bb.h:31-32, gr_additive_scrambler_bb.h:31-32.  gr_sync_blocks of
// bytes, history 1; the register (and d_bits) live in the handle, so work() may be cut anywhere.  One stream each.
// ---------------------------------------------------------------------------
template <class T>
class grhip_lfsr_bb_blk : public grhip_detail::block<gr_sync_block, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    // (mask, seed, len[, count], device), as T::create takes them
    template <class... A> explicit grhip_lfsr_bb_blk(A... args)
        : grhip_lfsr_bb_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(1, 1, sizeof(unsigned char)))
    {
        grhip_detail::check(T::create(this->d_h.out(), args...));                  // len above 31 throws, gri_lfsr.h:109-110
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(T::work(this->d_h, noutput_items, in[0], out[0]));
        return noutput_items;
    }
};
namespace grhip_detail {
#define GRHIP_LFSR_FNS(NAME)                                                                                           \
    struct NAME##_fns {                                                                                               \
        typedef grhip_##NAME H;                                                                                       \
        static constexpr const char *name = #NAME;                                                                    \
        GRHIP_FN(NAME, create); GRHIP_FN(NAME, destroy); GRHIP_FN(NAME, set_mode); GRHIP_FN(NAME, work);              \
    };
GRHIP_LFSR_FNS(scrambler_bb)
GRHIP_LFSR_FNS(descrambler_bb)
GRHIP_LFSR_FNS(additive_scrambler_bb)
#undef GRHIP_LFSR_FNS
}  // namespace grhip_detail
typedef grhip_lfsr_bb_blk<grhip_detail::scrambler_bb_fns> grhip_scrambler_bb_blk;
typedef grhip_lfsr_bb_blk<grhip_detail::descrambler_bb_fns> grhip_descrambler_bb_blk;
typedef grhip_lfsr_bb_blk<grhip_detail::additive_scrambler_bb_fns> grhip_additive_scrambler_bb_blk;
typedef boost::shared_ptr<grhip_scrambler_bb_blk> grhip_scrambler_bb_sptr;
typedef boost::shared_ptr<grhip_descrambler_bb_blk> grhip_descrambler_bb_sptr;
typedef boost::shared_ptr<grhip_additive_scrambler_bb_blk> grhip_additive_scrambler_bb_sptr;
inline grhip_scrambler_bb_sptr gr_make_scrambler_bb(int mask, int seed, int len, int device = 0)
{
    return grhip_detail::factory::make<grhip_scrambler_bb_blk>(mask, seed, len, device);
}
inline grhip_descrambler_bb_sptr gr_make_descrambler_bb(int mask, int seed, int len, int device = 0)
{
    return grhip_detail::factory::make<grhip_descrambler_bb_blk>(mask, seed, len, device);
}
inline grhip_additive_scrambler_bb_sptr gr_make_additive_scrambler_bb(int mask, int seed, int len, int count = 0, int device = 0)
{
    return grhip_detail::factory::make<grhip_additive_scrambler_bb_blk>(mask, seed, len, count, device);
}

// ---------------------------------------------------------------------------
// gr-trellis.  fsm (gr-trellis/src/lib/fsm.h:39-74) is a host object with the reference's constructors and accessors;
// a block copies the one it is made from.  trellis_encoder_XX (FSM, ST) is a gr_sync_block; trellis_metrics_X
// (O, D, TABLE, TYPE) and trellis_constellation_metrics_cf (constellation, TYPE) are gr_blocks with
// set_relative_rate(O / D), set_output_multiple(O) and D * noutput_items / O inputs (trellis_metrics_X.cc.t:53-70);
// trellis_viterbi_X (FSM, K, S0, SK) is a gr_block with set_relative_rate(1 / O), set_output_multiple(K) and
// O * noutput_items inputs (trellis_viterbi_X.cc.t:60-72).  One stream each.  What the reference indexes out of range
// for (an input symbol >= I, sizes that do not fit) throws std::invalid_argument here.
// ---------------------------------------------------------------------------
class fsm {
    grhip_detail::handle<grhip_fsm, grhip_fsm_destroy> d_h;
    static size_t count(int rc)
    {
        grhip_detail::check(rc);
        return (size_t)rc;
    }
    std::vector<int> table(int (*get)(const grhip_fsm *, int *, int)) const
    {
        if (!d_h) return std::vector<int>();
        std::vector<int> v(count(get(d_h, nullptr, 0)));
        grhip_detail::check(get(d_h, v.data(), (int)v.size()));
        return v;
    }
    std::vector<std::vector<int> > lists(int (*get)(const grhip_fsm *, int, int *, int)) const
    {
        std::vector<std::vector<int> > ll((size_t)S());
        for (int j = 0; j < S(); j++) {
            ll[j].resize(count(get(d_h, j, nullptr, 0)));
            grhip_detail::check(get(d_h, j, ll[j].data(), (int)ll[j].size()));
        }
        return ll;
    }
public:
    fsm() {}                                        // fsm.cc:34-45: I = S = O = 0 and empty tables; no block takes it
    fsm(const fsm &FSM)
    {
        if (FSM.d_h) *this = fsm(FSM.I(), FSM.S(), FSM.O(), FSM.NS(), FSM.OS());
    }
    fsm(fsm &&) = default;
    fsm &operator=(fsm &&) = default;
    fsm &operator=(const fsm &FSM)
    {
        fsm copy(FSM);
        d_h = std::move(copy.d_h);
        return *this;
    }
    fsm(int I, int S, int O, const std::vector<int> &NS, const std::vector<int> &OS)
    {
        grhip_detail::check(grhip_fsm_create(d_h.out(), I, S, O, NS.data(), (int)NS.size(), OS.data(), (int)OS.size()));
    }
    explicit fsm(const char *name) { grhip_detail::check(grhip_fsm_create_file(d_h.out(), name)); }
    fsm(int k, int n, const std::vector<int> &G) { grhip_detail::check(grhip_fsm_create_generator(d_h.out(), k, n, G.data(), (int)G.size())); }
    fsm(int mod_size, int ch_length) { grhip_detail::check(grhip_fsm_create_isi(d_h.out(), mod_size, ch_length)); }
    fsm(int P, int M, int L) { grhip_detail::check(grhip_fsm_create_cpm(d_h.out(), P, M, L)); }
    fsm(const fsm &FSM1, const fsm &FSM2) { grhip_detail::check(grhip_fsm_create_joint(d_h.out(), FSM1.d_h, FSM2.d_h)); }
    fsm(const fsm &FSM, int n) { grhip_detail::check(grhip_fsm_create_radix(d_h.out(), FSM.d_h, n)); }
    const grhip_fsm *handle() const { return d_h; }
    int I() const { return d_h ? grhip_fsm_I(d_h) : 0; }
    int S() const { return d_h ? grhip_fsm_S(d_h) : 0; }
    int O() const { return d_h ? grhip_fsm_O(d_h) : 0; }
    bool connected() const { return d_h && grhip_fsm_connected(d_h) != 0; }        // false where the reference prints its message
    std::vector<int> NS() const { return table(grhip_fsm_NS); }
    std::vector<int> OS() const { return table(grhip_fsm_OS); }
    std::vector<int> TMl() const { return table(grhip_fsm_TMl); }
    std::vector<int> TMi() const { return table(grhip_fsm_TMi); }
    std::vector<std::vector<int> > PS() const { return lists(grhip_fsm_PS); }
    std::vector<std::vector<int> > PI() const { return lists(grhip_fsm_PI); }
};

typedef enum { TRELLIS_EUCLIDEAN = GRHIP_TRELLIS_EUCLIDEAN, TRELLIS_HARD_SYMBOL, TRELLIS_HARD_BIT } trellis_metric_type_t;

// T names the C entries and the item types of one signature
template <class T>
class grhip_trellis_encoder_blk : public grhip_detail::block<gr_sync_block, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    fsm d_FSM;
    grhip_trellis_encoder_blk(const fsm &FSM, int ST, int device)
        : grhip_trellis_encoder_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(typename T::in_t)), gr_make_io_signature(1, 1, sizeof(typename T::out_t))),
          d_FSM(FSM)
    {
        grhip_detail::check(T::create(this->d_h.out(), d_FSM.handle(), ST, device));
    }
public:
    fsm FSM() const { return d_FSM; }
    int ST() const
    {
        int st = 0;
        grhip_detail::check(T::ST(this->d_h, 0, &st));
        return st;
    }
    void set_ST(int ST) { grhip_detail::check(T::set_ST(this->d_h, ST)); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(T::work(this->d_h, noutput_items, in[0], out[0]));
        return noutput_items;
    }
};

// the block of trellis_metrics_X and of trellis_constellation_metrics_cf: what differs is how the handle is made
template <class T>
class grhip_trellis_metrics_blk : public grhip_detail::block<gr_block, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    int d_O, d_D;
    template <class... A> explicit grhip_trellis_metrics_blk(A... args)
        : grhip_trellis_metrics_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(typename T::in_t)), gr_make_io_signature(1, 1, sizeof(float)))
    {
        grhip_detail::check(T::make(this->d_h.out(), args...));
        d_O = T::O(this->d_h);
        d_D = T::D(this->d_h);
        this->set_relative_rate(1.0 * d_O / ((double)d_D));
        this->set_output_multiple(d_O);
    }
public:
    int O() const { return d_O; }
    int D() const { return d_D; }
    trellis_metric_type_t TYPE() const { return (trellis_metric_type_t)T::TYPE(this->d_h); }
    template <class V> void set_TABLE(const std::vector<V> &table)
    {
        static_assert(sizeof(V) == sizeof(typename T::in_t), "TABLE holds the block's input items");
        grhip_detail::check(T::set_TABLE(this->d_h, table.data(), (int)table.size()));
    }
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        for (size_t i = 0; i < req.size(); i++) req[i] = d_D * noutput_items / d_O;
    }
    int general_work(int noutput_items, gr_vector_int &, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(T::work(this->d_h, noutput_items / d_O, in[0], out[0]));
        this->consume_each(d_D * noutput_items / d_O);
        return noutput_items;
    }
};

template <class T>
class grhip_trellis_viterbi_blk : public grhip_detail::block<gr_block, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    fsm d_FSM;
    int d_K, d_S0, d_SK;
    grhip_trellis_viterbi_blk(const fsm &FSM, int K, int S0, int SK, int device)
        : grhip_trellis_viterbi_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(typename T::out_t))),
          d_FSM(FSM), d_K(K), d_S0(S0), d_SK(SK)
    {
        grhip_detail::check(T::create(this->d_h.out(), d_FSM.handle(), K, S0, SK, device));
        this->set_relative_rate(1.0 / ((double)d_FSM.O()));
        this->set_output_multiple(d_K);
    }
public:
    fsm FSM() const { return d_FSM; }
    int K() const { return d_K; }
    int S0() const { return d_S0; }
    int SK() const { return d_SK; }
    long long dead_ends() const
    {
        long long n = 0;
        grhip_detail::check(T::dead_ends(this->d_h, &n));
        return n;
    }
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        for (size_t i = 0; i < req.size(); i++) req[i] = d_FSM.O() * noutput_items;
    }
    int general_work(int noutput_items, gr_vector_int &, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(T::work(this->d_h, noutput_items, in[0], out[0]));
        this->consume_each(d_FSM.O() * noutput_items);
        return noutput_items;
    }
};

// trellis_viterbi_combined_XX (FSM, K, S0, SK, D, TABLE, TYPE): trellis_viterbi_combined_XX.cc.t:62-75, a gr_block with
// set_relative_rate(1 / D), set_output_multiple(K) and D * noutput_items inputs
template <class T>
class grhip_trellis_viterbi_combined_blk : public grhip_detail::block<gr_block, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    fsm d_FSM;
    int d_K, d_S0, d_SK, d_D;
    std::vector<typename T::in_t> d_TABLE;
    trellis_metric_type_t d_TYPE;
    grhip_trellis_viterbi_combined_blk(const fsm &FSM, int K, int S0, int SK, int D, const std::vector<typename T::in_t> &TABLE,
                                       trellis_metric_type_t TYPE, int device)
        : grhip_trellis_viterbi_combined_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(typename T::in_t)),
                                                    gr_make_io_signature(1, 1, sizeof(typename T::out_t))),
          d_FSM(FSM), d_K(K), d_S0(S0), d_SK(SK), d_D(D), d_TABLE(TABLE), d_TYPE(TYPE)
    {
        grhip_detail::check(T::create(this->d_h.out(), d_FSM.handle(), K, S0, SK, D, d_TABLE.data(), (int)d_TABLE.size(), (int)TYPE, device));
        this->set_relative_rate(1.0 / ((double)d_D));
        this->set_output_multiple(d_K);
    }
public:
    fsm FSM() const { return d_FSM; }
    int K() const { return d_K; }
    int S0() const { return d_S0; }
    int SK() const { return d_SK; }
    int D() const { return d_D; }
    std::vector<typename T::in_t> TABLE() const { return d_TABLE; }
    trellis_metric_type_t TYPE() const { return d_TYPE; }
    void set_TABLE(const std::vector<typename T::in_t> &table)
    {
        grhip_detail::check(T::set_TABLE(this->d_h, table.data(), (int)table.size()));
        d_TABLE = table;
    }
    int engine() const { return this->checked(T::engine(this->d_h)); }
    void set_engine(int e) { grhip_detail::check(T::set_engine(this->d_h, e)); }
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        for (size_t i = 0; i < req.size(); i++) req[i] = d_D * noutput_items;
    }
    int general_work(int noutput_items, gr_vector_int &, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(T::work(this->d_h, noutput_items, in[0], out[0]));
        this->consume_each(d_D * noutput_items);
        return noutput_items;
    }
};

namespace grhip_detail {
#define GRHIP_TRELLIS_COMMON(NAME)                                                                                     \
    typedef grhip_##NAME H;                                                                                           \
    static constexpr const char *name = #NAME;                                                                        \
    GRHIP_FN(NAME, create); GRHIP_FN(NAME, destroy); GRHIP_FN(NAME, set_mode); GRHIP_FN(NAME, work);
#define GRHIP_TRELLIS_ENCODER_FNS(NAME, IN, OUT)                                                                       \
    struct NAME##_fns {                                                                                               \
        GRHIP_TRELLIS_COMMON(NAME)                                                                                    \
        typedef IN in_t;                                                                                              \
        typedef OUT out_t;                                                                                            \
        GRHIP_FN(NAME, ST); GRHIP_FN(NAME, set_ST);                                                                   \
    };
GRHIP_TRELLIS_ENCODER_FNS(trellis_encoder_bb, unsigned char, unsigned char)
GRHIP_TRELLIS_ENCODER_FNS(trellis_encoder_bs, unsigned char, short)
GRHIP_TRELLIS_ENCODER_FNS(trellis_encoder_bi, unsigned char, int)
GRHIP_TRELLIS_ENCODER_FNS(trellis_encoder_ss, short, short)
GRHIP_TRELLIS_ENCODER_FNS(trellis_encoder_si, short, int)
GRHIP_TRELLIS_ENCODER_FNS(trellis_encoder_ii, int, int)
#undef GRHIP_TRELLIS_ENCODER_FNS
#define GRHIP_TRELLIS_METRICS_FNS(NAME, IN)                                                                            \
    struct NAME##_fns {                                                                                               \
        GRHIP_TRELLIS_COMMON(NAME)                                                                                    \
        typedef IN in_t;                                                                                              \
        GRHIP_FN(NAME, O); GRHIP_FN(NAME, D); GRHIP_FN(NAME, TYPE); GRHIP_FN(NAME, set_TABLE);                        \
        static int make(H **h, int O, int D, const std::vector<IN> &TABLE, trellis_metric_type_t TYPE, int device)    \
        {                                                                                                             \
            return create(h, O, D, TABLE.data(), (int)TABLE.size(), (int)TYPE, device);                               \
        }                                                                                                             \
    };
GRHIP_TRELLIS_METRICS_FNS(trellis_metrics_s, short)
GRHIP_TRELLIS_METRICS_FNS(trellis_metrics_i, int)
GRHIP_TRELLIS_METRICS_FNS(trellis_metrics_f, float)
GRHIP_TRELLIS_METRICS_FNS(trellis_metrics_c, gr_complex)
#undef GRHIP_TRELLIS_METRICS_FNS
struct trellis_constellation_metrics_cf_fns {
    GRHIP_TRELLIS_COMMON(trellis_constellation_metrics_cf)
    typedef gr_complex in_t;
    GRHIP_FN(trellis_constellation_metrics_cf, O); GRHIP_FN(trellis_constellation_metrics_cf, D); GRHIP_FN(trellis_constellation_metrics_cf, TYPE);
    static int make(H **h, grhip_constellation_sptr constellation, trellis_metric_type_t TYPE, int device)
    {
        return create(h, constellation->handle(), (int)TYPE, device);
    }
};
#define GRHIP_TRELLIS_VITERBI_FNS(NAME, OUT)                                                                           \
    struct NAME##_fns {                                                                                               \
        GRHIP_TRELLIS_COMMON(NAME)                                                                                    \
        typedef OUT out_t;                                                                                            \
        GRHIP_FN(NAME, dead_ends);                                                                                    \
    };
GRHIP_TRELLIS_VITERBI_FNS(trellis_viterbi_b, unsigned char)
GRHIP_TRELLIS_VITERBI_FNS(trellis_viterbi_s, short)
GRHIP_TRELLIS_VITERBI_FNS(trellis_viterbi_i, int)
#undef GRHIP_TRELLIS_VITERBI_FNS
#define GRHIP_TRELLIS_COMBINED_FNS(NAME, IN, OUT)                                                                      \
    struct NAME##_fns {                                                                                               \
        GRHIP_TRELLIS_COMMON(NAME)                                                                                    \
        typedef IN in_t;                                                                                              \
        typedef OUT out_t;                                                                                            \
        GRHIP_FN(NAME, set_TABLE); GRHIP_FN(NAME, set_engine); GRHIP_FN(NAME, engine);                                \
    };
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_sb, short, unsigned char)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_ss, short, short)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_si, short, int)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_ib, int, unsigned char)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_is, int, short)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_ii, int, int)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_fb, float, unsigned char)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_fs, float, short)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_fi, float, int)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_cb, gr_complex, unsigned char)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_cs, gr_complex, short)
GRHIP_TRELLIS_COMBINED_FNS(trellis_viterbi_combined_ci, gr_complex, int)
#undef GRHIP_TRELLIS_COMBINED_FNS
#undef GRHIP_TRELLIS_COMMON
}  // namespace grhip_detail

// the reference's factory names and signatures, one block type and one sptr each
#define GRHIP_TRELLIS_ENCODER(SUF)                                                                                     \
    typedef grhip_trellis_encoder_blk<grhip_detail::trellis_encoder_##SUF##_fns> grhip_trellis_encoder_##SUF##_blk;   \
    typedef boost::shared_ptr<grhip_trellis_encoder_##SUF##_blk> grhip_trellis_encoder_##SUF##_sptr;                  \
    inline grhip_trellis_encoder_##SUF##_sptr trellis_make_encoder_##SUF(const fsm &FSM, int ST, int device = 0)      \
    {                                                                                                                 \
        return grhip_detail::factory::make<grhip_trellis_encoder_##SUF##_blk>(FSM, ST, device);                       \
    }
GRHIP_TRELLIS_ENCODER(bb)
GRHIP_TRELLIS_ENCODER(bs)
GRHIP_TRELLIS_ENCODER(bi)
GRHIP_TRELLIS_ENCODER(ss)
GRHIP_TRELLIS_ENCODER(si)
GRHIP_TRELLIS_ENCODER(ii)
#undef GRHIP_TRELLIS_ENCODER
#define GRHIP_TRELLIS_METRICS(SUF, IN)                                                                                 \
    typedef grhip_trellis_metrics_blk<grhip_detail::trellis_metrics_##SUF##_fns> grhip_trellis_metrics_##SUF##_blk;   \
    typedef boost::shared_ptr<grhip_trellis_metrics_##SUF##_blk> grhip_trellis_metrics_##SUF##_sptr;                  \
    inline grhip_trellis_metrics_##SUF##_sptr trellis_make_metrics_##SUF(int O, int D, const std::vector<IN> &TABLE,  \
                                                                         trellis_metric_type_t TYPE, int device = 0)  \
    {                                                                                                                 \
        return grhip_detail::factory::make<grhip_trellis_metrics_##SUF##_blk>(O, D, TABLE, TYPE, device);             \
    }
GRHIP_TRELLIS_METRICS(s, short)
GRHIP_TRELLIS_METRICS(i, int)
GRHIP_TRELLIS_METRICS(f, float)
GRHIP_TRELLIS_METRICS(c, gr_complex)
#undef GRHIP_TRELLIS_METRICS
typedef grhip_trellis_metrics_blk<grhip_detail::trellis_constellation_metrics_cf_fns> grhip_trellis_constellation_metrics_cf_blk;
typedef boost::shared_ptr<grhip_trellis_constellation_metrics_cf_blk> grhip_trellis_constellation_metrics_cf_sptr;
inline grhip_trellis_constellation_metrics_cf_sptr trellis_make_constellation_metrics_cf(grhip_constellation_sptr constellation,
                                                                                         trellis_metric_type_t TYPE, int device = 0)
{
    return grhip_detail::factory::make<grhip_trellis_constellation_metrics_cf_blk>(constellation, TYPE, device);
}
#define GRHIP_TRELLIS_VITERBI(SUF)                                                                                     \
    typedef grhip_trellis_viterbi_blk<grhip_detail::trellis_viterbi_##SUF##_fns> grhip_trellis_viterbi_##SUF##_blk;   \
    typedef boost::shared_ptr<grhip_trellis_viterbi_##SUF##_blk> grhip_trellis_viterbi_##SUF##_sptr;                  \
    inline grhip_trellis_viterbi_##SUF##_sptr trellis_make_viterbi_##SUF(const fsm &FSM, int K, int S0, int SK, int device = 0) \
    {                                                                                                                 \
        return grhip_detail::factory::make<grhip_trellis_viterbi_##SUF##_blk>(FSM, K, S0, SK, device);                \
    }
GRHIP_TRELLIS_VITERBI(b)
GRHIP_TRELLIS_VITERBI(s)
GRHIP_TRELLIS_VITERBI(i)
#undef GRHIP_TRELLIS_VITERBI
#define GRHIP_TRELLIS_COMBINED(SUF, IN)                                                                                \
    typedef grhip_trellis_viterbi_combined_blk<grhip_detail::trellis_viterbi_combined_##SUF##_fns> grhip_trellis_viterbi_combined_##SUF##_blk; \
    typedef boost::shared_ptr<grhip_trellis_viterbi_combined_##SUF##_blk> grhip_trellis_viterbi_combined_##SUF##_sptr; \
    inline grhip_trellis_viterbi_combined_##SUF##_sptr trellis_make_viterbi_combined_##SUF(                           \
        const fsm &FSM, int K, int S0, int SK, int D, const std::vector<IN> &TABLE, trellis_metric_type_t TYPE, int device = 0) \
    {                                                                                                                 \
        return grhip_detail::factory::make<grhip_trellis_viterbi_combined_##SUF##_blk>(FSM, K, S0, SK, D, TABLE, TYPE, device); \
    }
GRHIP_TRELLIS_COMBINED(sb, short)
GRHIP_TRELLIS_COMBINED(ss, short)
GRHIP_TRELLIS_COMBINED(si, short)
GRHIP_TRELLIS_COMBINED(ib, int)
GRHIP_TRELLIS_COMBINED(is, int)
GRHIP_TRELLIS_COMBINED(ii, int)
GRHIP_TRELLIS_COMBINED(fb, float)
GRHIP_TRELLIS_COMBINED(fs, float)
GRHIP_TRELLIS_COMBINED(fi, float)
GRHIP_TRELLIS_COMBINED(cb, gr_complex)
GRHIP_TRELLIS_COMBINED(cs, gr_complex)
GRHIP_TRELLIS_COMBINED(ci, gr_complex)
#undef GRHIP_TRELLIS_COMBINED

// ---------------------------------------------------------------------------
// The continuous-phase transmitter.  gr_frequency_modulator_fc (general/gr_frequency_modulator_fc.h:32-56): a
// gr_sync_block, float in, complex out; the phase lives in the handle and is wrapped at the end of every work call, as
// the reference's, so the output depends on where the scheduler cuts.  gr_bytes_to_syms (general/gr_bytes_to_syms.h),
// gr_char_to_float (general/gr_char_to_float.h) and gr_chunks_to_symbols_bf keep nothing.  One stream each.
// ---------------------------------------------------------------------------
class grhip_frequency_modulator_fc_blk : public GRHIP_BLOCK(gr_sync_block, frequency_modulator_fc) {
    friend struct grhip_detail::factory;
    grhip_frequency_modulator_fc_blk(double sensitivity, int device)
        : block("frequency_modulator_fc", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(gr_complex)))
    {
        grhip_detail::check(grhip_frequency_modulator_fc_create(d_h.out(), sensitivity, device));
    }
public:
    void set_sensitivity(float sens) { grhip_detail::check(grhip_frequency_modulator_fc_set_sensitivity(d_h, sens)); }
    float sensitivity() const { return grhip_frequency_modulator_fc_sensitivity(d_h); }
    double phase() const
    {
        double p = 0.0;
        grhip_detail::check(grhip_frequency_modulator_fc_phase(d_h, 0, &p));
        return p;
    }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_frequency_modulator_fc_work(d_h, noutput_items, in[0], out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_frequency_modulator_fc_blk> grhip_frequency_modulator_fc_sptr;
inline grhip_frequency_modulator_fc_sptr gr_make_frequency_modulator_fc(double sensitivity, int device = 0)
{
    return grhip_detail::factory::make<grhip_frequency_modulator_fc_blk>(sensitivity, device);
}

class grhip_bytes_to_syms_blk : public GRHIP_BLOCK(gr_sync_interpolator, bytes_to_syms) {
    friend struct grhip_detail::factory;
    explicit grhip_bytes_to_syms_blk(int device)
        : block("bytes_to_syms", gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(1, 1, sizeof(float)), 8)
    {
        grhip_detail::check(grhip_bytes_to_syms_create(d_h.out(), device));
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_bytes_to_syms_work(d_h, noutput_items / 8, in[0], out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_bytes_to_syms_blk> grhip_bytes_to_syms_sptr;
inline grhip_bytes_to_syms_sptr gr_make_bytes_to_syms(int device = 0) { return grhip_detail::factory::make<grhip_bytes_to_syms_blk>(device); }

class grhip_char_to_float_blk : public GRHIP_BLOCK(gr_sync_block, char_to_float) {
    friend struct grhip_detail::factory;
    explicit grhip_char_to_float_blk(int device)
        : block("gr_char_to_float", gr_make_io_signature(1, 1, sizeof(char)), gr_make_io_signature(1, 1, sizeof(float)))
    {
        grhip_detail::check(grhip_char_to_float_create(d_h.out(), device));
    }
public:
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_char_to_float_work(d_h, noutput_items, in[0], out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_char_to_float_blk> grhip_char_to_float_sptr;
inline grhip_char_to_float_sptr gr_make_char_to_float(int device = 0) { return grhip_detail::factory::make<grhip_char_to_float_blk>(device); }

class grhip_chunks_to_symbols_bf_blk : public GRHIP_BLOCK(gr_sync_interpolator, chunks_to_symbols_bf) {
    friend struct grhip_detail::factory;
    std::vector<float> d_symbol_table;
    grhip_chunks_to_symbols_bf_blk(const std::vector<float> &symbol_table, const int D, int device)
        : block("chunks_to_symbols_bf", gr_make_io_signature(1, 1, sizeof(unsigned char)), gr_make_io_signature(1, 1, sizeof(float)),
                (unsigned)(D < 1 ? 1 : D)),
          d_symbol_table(symbol_table)
    {
        grhip_detail::check(grhip_chunks_to_symbols_bf_create(d_h.out(), symbol_table.data(), symbol_table.size(), D, device));
    }
public:
    int D() const { return (int)interpolation(); }
    std::vector<float> symbol_table() const { return d_symbol_table; }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_chunks_to_symbols_bf_work(d_h, noutput_items / (int)interpolation(), in[0], out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_chunks_to_symbols_bf_blk> grhip_chunks_to_symbols_bf_sptr;
inline grhip_chunks_to_symbols_bf_sptr grhip_make_chunks_to_symbols_bf(const std::vector<float> &symbol_table, const int D = 1, int device = 0)
{
    return grhip_detail::factory::make<grhip_chunks_to_symbols_bf_blk>(symbol_table, D, device);
}

// gr_cpm::phase_response (general/gr_cpm.h:40-74): host arithmetic, no device
inline std::vector<float> grhip_cpm_phase_response_taps(int type, unsigned samples_per_sym, unsigned L, double beta = 0.3)
{
    const int n = grhip_cpm_phase_response(type, samples_per_sym, L, beta, nullptr, 0);
    grhip_detail::check(n);
    std::vector<float> t((size_t)n);
    grhip_detail::check(grhip_cpm_phase_response(type, samples_per_sym, L, beta, t.data(), t.size()));
    return t;
}

// digital_cpmmod_bc, digital_gmskmod_bc (gr-digital/lib/digital_cpmmod_bc.h:33-95, digital_gmskmod_bc.h:32-60) and gmsk_mod
// (gr-digital/python/gmsk.py:55-120), each one gr_sync_interpolator on new items only: symbols (gmsk_mod: bytes) in,
// samples_per_sym (8 * samples_per_symbol) complex items out for each.  A work call of the block is a work call of the
// inner modulator: its phase wrap falls where the scheduler cuts.  One stream each.
template <class T>
class grhip_cpm_hier_blk : public grhip_detail::block<gr_sync_interpolator, typename T::H, T::destroy, T::set_mode> {
    friend struct grhip_detail::factory;
    // per: output items per input item; then the arguments of T::create
    template <class... A> explicit grhip_cpm_hier_blk(unsigned per, A... args)
        : grhip_cpm_hier_blk::block(T::name, gr_make_io_signature(1, 1, sizeof(char)), gr_make_io_signature(1, 1, sizeof(gr_complex)), per)
    {
        grhip_detail::check(T::create(this->d_h.out(), args...));
    }
public:
    int engine() const { return T::engine(this->d_h); }
    void set_engine(int engine) { grhip_detail::check(T::set_engine(this->d_h, engine)); }
    int samples_per_symbol() const { return T::samples_per_symbol(this->d_h); }
    std::vector<float> get_taps() const                                        // digital_cpmmod_bc.h:92
    {
        std::vector<float> t((size_t)T::filter_taps(this->d_h, nullptr, 0));
        T::filter_taps(this->d_h, t.data(), t.size());
        return t;
    }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(T::work(this->d_h, noutput_items / (int)this->interpolation(), in[0], out[0], nullptr));
        return noutput_items;
    }
};
namespace grhip_detail {
#define GRHIP_CPM_FNS(NAME)                                                                                            \
    struct NAME##_fns {                                                                                               \
        typedef grhip_##NAME H;                                                                                       \
        static constexpr const char *name = #NAME;                                                                    \
        GRHIP_FN(NAME, create); GRHIP_FN(NAME, destroy); GRHIP_FN(NAME, set_mode); GRHIP_FN(NAME, work);              \
        GRHIP_FN(NAME, engine); GRHIP_FN(NAME, set_engine); GRHIP_FN(NAME, samples_per_symbol); GRHIP_FN(NAME, filter_taps); \
    };
GRHIP_CPM_FNS(cpmmod_bc)
GRHIP_CPM_FNS(gmskmod_bc)
GRHIP_CPM_FNS(gmsk_mod)
#undef GRHIP_CPM_FNS
}  // namespace grhip_detail
typedef grhip_cpm_hier_blk<grhip_detail::cpmmod_bc_fns> grhip_cpmmod_bc_blk;
typedef grhip_cpm_hier_blk<grhip_detail::gmskmod_bc_fns> grhip_gmskmod_bc_blk;
typedef grhip_cpm_hier_blk<grhip_detail::gmsk_mod_fns> grhip_gmsk_mod_blk;
typedef boost::shared_ptr<grhip_cpmmod_bc_blk> grhip_cpmmod_bc_sptr;
typedef boost::shared_ptr<grhip_gmskmod_bc_blk> grhip_gmskmod_bc_sptr;
typedef boost::shared_ptr<grhip_gmsk_mod_blk> grhip_gmsk_mod_sptr;
inline grhip_cpmmod_bc_sptr digital_make_cpmmod_bc(int type, float h, unsigned samples_per_sym, unsigned L, double beta = 0.3, int device = 0)
{
    return grhip_detail::factory::make<grhip_cpmmod_bc_blk>(samples_per_sym, type, h, samples_per_sym, L, beta, device);
}
inline grhip_gmskmod_bc_sptr digital_make_gmskmod_bc(unsigned samples_per_sym = 2, double bt = 0.3, unsigned L = 4, int device = 0)
{
    return grhip_detail::factory::make<grhip_gmskmod_bc_blk>(samples_per_sym, samples_per_sym, bt, L, device);
}
inline grhip_gmsk_mod_sptr grhip_make_gmsk_mod(int samples_per_symbol = 2, double bt = 0.35, int device = 0)
{
    return grhip_detail::factory::make<grhip_gmsk_mod_blk>(8u * (unsigned)(samples_per_symbol < 1 ? 1 : samples_per_symbol), samples_per_symbol, bt, device);
}

// ---------------------------------------------------------------------------
// gr_iir_filter_ffd (fftaps, fbtaps in double; filter/gr_iir_filter_ffd.h:62-85): a gr_sync_block, history 1, float in
// and out.  set_taps is latched until the next work call, as the reference's is.  fm_deemph_taps and
// gr_make_fm_deemph are blks2.fm_deemph (blks2impl/fm_emph.py:44-72), one gr_iir_filter_ffd.
// ---------------------------------------------------------------------------
class grhip_iir_filter_ffd_blk : public GRHIP_BLOCK(gr_sync_block, iir_filter_ffd) {
    friend struct grhip_detail::factory;
    grhip_iir_filter_ffd_blk(const std::vector<double> &fftaps, const std::vector<double> &fbtaps, int device)
        : block("iir_filter_ffd", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(float)))
    {
        grhip_detail::check(grhip_iir_filter_ffd_create(d_h.out(), fftaps.data(), fftaps.size(), fbtaps.data(), fbtaps.size(), device));
    }
public:
    void set_taps(const std::vector<double> &fftaps, const std::vector<double> &fbtaps)
    {
        grhip_detail::check(grhip_iir_filter_ffd_set_taps(d_h, fftaps.data(), fftaps.size(), fbtaps.data(), fbtaps.size()));
    }
    bool chunked() const { return grhip_iir_filter_ffd_chunked(d_h) == 1; }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        grhip_detail::check(grhip_iir_filter_ffd_work(d_h, noutput_items, in[0], out[0]));
        return noutput_items;
    }
};
typedef boost::shared_ptr<grhip_iir_filter_ffd_blk> grhip_iir_filter_ffd_sptr;
inline grhip_iir_filter_ffd_sptr gr_make_iir_filter_ffd(const std::vector<double> &fftaps, const std::vector<double> &fbtaps,
                                                        int device = 0)
{
    return grhip_detail::factory::make<grhip_iir_filter_ffd_blk>(fftaps, fbtaps, device);
}

// (btaps, ataps) of blks2.fm_deemph(fs, tau)
inline void fm_deemph_taps(double fs, double tau, std::vector<double> &btaps, std::vector<double> &ataps)
{
    btaps.assign(2, 0.0);
    ataps.assign(2, 0.0);
    grhip_detail::check(grhip_fm_deemph_taps(fs, tau, btaps.data(), ataps.data()));
}
inline grhip_iir_filter_ffd_sptr gr_make_fm_deemph(double fs, double tau = 75e-6, int device = 0)
{
    std::vector<double> b, a;
    fm_deemph_taps(fs, tau, b, a);
    return gr_make_iir_filter_ffd(b, a, device);
}

// gr_firdes::low_pass(gain, sampling_freq, cutoff_freq, transition_width, window = WIN_HAMMING (0), beta = 6.76)
inline std::vector<float> grhip_firdes_low_pass_taps(double gain, double sampling_freq, double cutoff_freq, double transition_width,
                                                     int window = 0, double beta = 6.76)
{
    size_t n = 0;
    const int rc = grhip_firdes_low_pass(gain, sampling_freq, cutoff_freq, transition_width, window, beta, nullptr, 0, &n);
    if (rc != GRHIP_ERANGE) grhip_detail::check(rc);            // GRHIP_ERANGE: the size query's answer
    std::vector<float> taps(n);
    grhip_detail::check(grhip_firdes_low_pass(gain, sampling_freq, cutoff_freq, transition_width, window, beta, taps.data(), n, &n));
    return taps;
}

// ---------------------------------------------------------------------------
// blks2.fm_demod_cf / blks2.nbfm_rx (blks2impl/fm_demod.py:51-72, nbfm_rx.py:28-88) as ONE block: a gr_sync_decimator by
// audio_decim, complex in and float out, history 1 (the handle takes new items only and keeps every inner block's
// history itself).  gr_make_fm_demod_cf takes the audio taps as given; the presets below design them as the reference does.
// ---------------------------------------------------------------------------
class grhip_fm_demod_cf_blk : public GRHIP_BLOCK(gr_sync_decimator, fm_demod_cf) {
    friend struct grhip_detail::factory;
    grhip_fm_demod_cf_blk(float k, const std::vector<double> &fftaps, const std::vector<double> &fbtaps, int audio_decim,
                          const std::vector<float> &audio_taps, int device)
        : block("fm_demod_cf", gr_make_io_signature(1, 1, sizeof(gr_complex)), gr_make_io_signature(1, 1, sizeof(float)),
                audio_decim < 1 ? 1u : (unsigned)audio_decim)
    {
        grhip_detail::check(grhip_fm_demod_cf_create(d_h.out(), k, fftaps.data(), fftaps.size(), fbtaps.data(), fbtaps.size(), audio_decim,
                                                     audio_taps.data(), audio_taps.size(), device));
    }
public:
    int engine() const { return grhip_fm_demod_cf_engine(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int produced = 0;
        grhip_detail::check(grhip_fm_demod_cf_work(d_h, noutput_items * (int)decimation(), in[0], out[0], &produced));
        return produced;
    }
};
typedef boost::shared_ptr<grhip_fm_demod_cf_blk> grhip_fm_demod_cf_sptr;
// the chain on given taps: quadrature_demod_cf(k) -> iir_filter_ffd(fftaps, fbtaps) (both empty: none) -> fir_filter_fff
inline grhip_fm_demod_cf_sptr grhip_make_fm_demod_cf(float k, const std::vector<double> &fftaps, const std::vector<double> &fbtaps,
                                                     int audio_decim, const std::vector<float> &audio_taps, int device = 0)
{
    return grhip_detail::factory::make<grhip_fm_demod_cf_blk>(k, fftaps, fbtaps, audio_decim, audio_taps, device);
}
// blks2.fm_demod_cf(channel_rate, audio_decim, deviation, ..., tau) on given audio taps; tau <= 0: no de-emphasis
inline grhip_fm_demod_cf_sptr gr_make_fm_demod_cf(double channel_rate, int audio_decim, double deviation,
                                                  const std::vector<float> &audio_taps, double tau = 75e-6, int device = 0)
{
    std::vector<double> b, a;
    if (tau > 0) fm_deemph_taps(channel_rate, tau, b, a);
    return grhip_make_fm_demod_cf((float)(channel_rate / (2 * M_PI * deviation)), b, a, audio_decim, audio_taps, device);
}
// blks2.nbfm_rx(audio_rate, quad_rate, tau = 75e-6, max_dev = 5e3)
inline grhip_fm_demod_cf_sptr gr_make_nbfm_rx(int audio_rate, int quad_rate, double tau = 75e-6, double max_dev = 5e3, int device = 0)
{
    if (audio_rate <= 0 || quad_rate % audio_rate != 0)
        throw std::invalid_argument("quad_rate is not an integer multiple of audio_rate");
    return gr_make_fm_demod_cf(quad_rate, quad_rate / audio_rate, max_dev, grhip_firdes_low_pass_taps(1.0, quad_rate, 2.7e3, 0.5e3),
                               tau, device);
}

// optfir.low_pass(gain, Fs, freq1, freq2, passband_ripple_db, stopband_atten_db, nextra_taps = 2): doubles, as gr.remez
inline std::vector<double> grhip_optfir_low_pass_taps(double gain, double Fs, double freq1, double freq2, double passband_ripple_db,
                                                      double stopband_atten_db, int nextra_taps = 2)
{
    size_t n = 0;
    const int rc = grhip_optfir_low_pass(gain, Fs, freq1, freq2, passband_ripple_db, stopband_atten_db, nextra_taps, nullptr, 0, &n);
    if (rc != GRHIP_ERANGE || n == 0) grhip_detail::check(rc);  // GRHIP_ERANGE with a count: the size query's answer
    std::vector<double> taps(n);
    grhip_detail::check(grhip_optfir_low_pass(gain, Fs, freq1, freq2, passband_ripple_db, stopband_atten_db, nextra_taps, taps.data(), n, &n));
    return taps;
}
inline std::vector<float> grhip_optfir_low_pass_taps_f(double gain, double Fs, double freq1, double freq2)
{
    const std::vector<double> d = grhip_optfir_low_pass_taps(gain, Fs, freq1, freq2, 0.1, 60);
    return std::vector<float>(d.begin(), d.end());              // narrowed per tap, as gr.fir_filter_fff takes them
}

// blks2.fm_demod_cf(channel_rate, audio_decim, deviation, audio_pass, audio_stop, gain = 1.0, tau = 75e-6) with the
// reference's own audio filter, optfir.low_pass(gain, channel_rate, audio_pass, audio_stop, 0.1, 60) (fm_demod.py:60-66)
inline grhip_fm_demod_cf_sptr gr_make_fm_demod_cf(double channel_rate, int audio_decim, double deviation, double audio_pass,
                                                  double audio_stop, double gain = 1.0, double tau = 75e-6, int device = 0)
{
    return gr_make_fm_demod_cf(channel_rate, audio_decim, deviation, grhip_optfir_low_pass_taps_f(gain, channel_rate, audio_pass, audio_stop),
                               tau, device);
}
// blks2.demod_20k0f3e_cf (fm_demod.py:74-91): NBFM, 5 kHz deviation
inline grhip_fm_demod_cf_sptr gr_make_demod_20k0f3e_cf(double channel_rate, int audio_decim, int device = 0)
{
    return gr_make_fm_demod_cf(channel_rate, audio_decim, 5000, 3000, 4500, 1.0, 75e-6, device);
}
// blks2.demod_200kf3e_cf (fm_demod.py:93-111): WFM, 75 kHz deviation, audio gain 20.  At 320 kHz and audio_decim 10 the
// filter has 1164 taps, more than the fused FM kernel takes: engine() is 0 and the three blocks run in a row.
inline grhip_fm_demod_cf_sptr gr_make_demod_200kf3e_cf(double channel_rate, int audio_decim, int device = 0)
{
    return gr_make_fm_demod_cf(channel_rate, audio_decim, 75000, 15000, 16000, 20.0, 75e-6, device);
}

// ---------------------------------------------------------------------------
// blks2.am_demod_cf / blks2.demod_10k0a3e_cf (blks2impl/am_demod.py:42-76) as ONE block: a gr_sync_decimator by audio_decim,
// complex in and float out, history 1 (the handle takes new items only and keeps the FIR's delay line itself).
// ---------------------------------------------------------------------------
class grhip_am_demod_cf_blk : public GRHIP_BLOCK(gr_sync_decimator, am_demod_cf) {
    friend struct grhip_detail::factory;
    std::vector<float> d_taps;
    grhip_am_demod_cf_blk(int audio_decim, const std::vector<float> &audio_taps, int device)
        : block("am_demod_cf", gr_make_io_signature(1, 1, sizeof(gr_complex)), gr_make_io_signature(1, 1, sizeof(float)),
                audio_decim < 1 ? 1u : (unsigned)audio_decim),
          d_taps(audio_taps)
    {
        grhip_detail::check(grhip_am_demod_cf_create(d_h.out(), audio_decim, audio_taps.data(), audio_taps.size(), device));
    }
public:
    int engine() const { return grhip_am_demod_cf_engine(d_h); }
    const std::vector<float> &audio_taps() const { return d_taps; }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        int produced = 0;
        grhip_detail::check(grhip_am_demod_cf_work(d_h, noutput_items * (int)decimation(), in[0], out[0], &produced));
        return produced;
    }
};
typedef boost::shared_ptr<grhip_am_demod_cf_blk> grhip_am_demod_cf_sptr;
// the chain on given taps: complex_to_mag -> add_const_ff(-1) -> fir_filter_fff(audio_decim, audio_taps)
inline grhip_am_demod_cf_sptr grhip_make_am_demod_cf(int audio_decim, const std::vector<float> &audio_taps, int device = 0)
{
    return grhip_detail::factory::make<grhip_am_demod_cf_blk>(audio_decim, audio_taps, device);
}
// blks2.am_demod_cf(channel_rate, audio_decim, audio_pass, audio_stop)
inline grhip_am_demod_cf_sptr gr_make_am_demod_cf(double channel_rate, int audio_decim, double audio_pass, double audio_stop,
                                                  int device = 0)
{
    return grhip_make_am_demod_cf(audio_decim, grhip_optfir_low_pass_taps_f(0.5, channel_rate, audio_pass, audio_stop), device);
}
// blks2.demod_10k0a3e_cf(channel_rate, audio_decim): audio 5 kHz / 5.5 kHz
inline grhip_am_demod_cf_sptr gr_make_demod_10k0a3e_cf(double channel_rate, int audio_decim, int device = 0)
{
    return gr_make_am_demod_cf(channel_rate, audio_decim, 5000, 5500, device);
}
