// blocks_surface_test.cc -- the public surface of grhip_blocks.h / grhip_fir_kernels.h as static_asserts, and handle
// ownership at run time on a fake handle.  Host only: no block is constructed, so nothing of libgrhip.so is needed and
// the program links without it; it runs under the address and undefined-behaviour sanitizers.
//
// Part 1 states, for every factory, its exact function type, that a call with only the non-defaulted arguments yields
// the _sptr type, and the GNU Radio base of the block class; and for every public accessor and setter its return type.
// Part 2 drives grhip_detail::handle and grhip_detail::block with a handle type whose destroy function records its calls.
#include <cstdio>
#include <type_traits>
#include <utility>

#include "grhip_fir_kernels.h"

#define SAME(...) static_assert(std::is_same<__VA_ARGS__>::value, #__VA_ARGS__)
#define V(...) std::declval<__VA_ARGS__>()
// FACTORY(function, block class, GNU Radio base, (a call with the non-defaulted arguments), exact function type)
#define FACTORY(F, BLK, BASE, CALL, ...)                                                                               \
    SAME(decltype(&F), __VA_ARGS__);                                                                                   \
    SAME(decltype(F CALL), boost::shared_ptr<BLK>);                                                                    \
    static_assert(std::is_base_of<BASE, BLK>::value, #BLK " derives from " #BASE)
// RET(class, member call, return type)
#define RET(X, CALL, ...) SAME(decltype(std::declval<X &>().CALL), __VA_ARGS__)
#define WORK(X) RET(X, work(0, V(gr_vector_const_void_star &), V(gr_vector_void_star &)), int)
#define GENERAL_WORK(X)                                                                                                \
    RET(X, general_work(0, V(gr_vector_int &), V(gr_vector_const_void_star &), V(gr_vector_void_star &)), int)
#define FORECAST(X) RET(X, forecast(0, V(gr_vector_int &)), void)

typedef std::vector<float> vf;
typedef std::vector<double> vd;
typedef std::vector<gr_complex> vc;
typedef std::vector<unsigned int> vu;

// ---- Part 1: the surface ------------------------------------------------------------------------------------------
SAME(decltype(&grhip_detail::check), void (*)(int));
SAME(decltype(grhip_set_batch_items(V(grhip_quadrature_demod_cf_sptr), 2)), void);

#define FIR_SURFACE(SUF, TAP)                                                                                          \
    FACTORY(grhip_make_fir_filter_##SUF, grhip_fir_filter_##SUF, gr_sync_decimator, (1, V(std::vector<TAP>)),          \
            grhip_fir_filter_##SUF##_sptr (*)(int, const std::vector<TAP> &, int));                                    \
    RET(grhip_fir_filter_##SUF, set_taps(V(std::vector<TAP>)), void);                                                  \
    WORK(grhip_fir_filter_##SUF)
FIR_SURFACE(ccf, float);
FIR_SURFACE(fff, float);
FIR_SURFACE(ccc, gr_complex);
FIR_SURFACE(fcc, gr_complex);
FIR_SURFACE(scc, gr_complex);
FIR_SURFACE(fsf, float);

#define XLATING_SURFACE(SUF, TAP)                                                                                      \
    FACTORY(grhip_make_freq_xlating_fir_filter_##SUF, grhip_freq_xlating_fir_filter_##SUF##_blk, gr_sync_decimator,    \
            (1, V(std::vector<TAP>), 0.0, 1.0),                                                                        \
            grhip_freq_xlating_fir_filter_##SUF##_sptr (*)(int, const std::vector<TAP> &, double, double, int));       \
    RET(grhip_freq_xlating_fir_filter_##SUF##_blk, set_center_freq(0.0), void);                                        \
    RET(grhip_freq_xlating_fir_filter_##SUF##_blk, set_taps(V(std::vector<TAP>)), void);                               \
    RET(grhip_freq_xlating_fir_filter_##SUF##_blk, set_mode(0), void);                                                 \
    WORK(grhip_freq_xlating_fir_filter_##SUF##_blk)
XLATING_SURFACE(ccc, gr_complex);
XLATING_SURFACE(ccf, float);
XLATING_SURFACE(fcf, float);
XLATING_SURFACE(fcc, gr_complex);
XLATING_SURFACE(scf, float);
XLATING_SURFACE(scc, gr_complex);

FACTORY(grhip_make_quadrature_demod_cf, grhip_quadrature_demod_cf_blk, gr_sync_block, (1.f),
        grhip_quadrature_demod_cf_sptr (*)(float, int));
WORK(grhip_quadrature_demod_cf_blk);

#define MM_SURFACE(SUF)                                                                                                \
    FACTORY(grhip_make_clock_recovery_mm_##SUF, grhip_clock_recovery_mm_##SUF##_blk, gr_block,                         \
            (1.f, 1.f, 1.f, 1.f, 1.f), grhip_clock_recovery_mm_##SUF##_sptr (*)(float, float, float, float, float, int)); \
    RET(grhip_clock_recovery_mm_##SUF##_blk, mu(), float);                                                             \
    RET(grhip_clock_recovery_mm_##SUF##_blk, omega(), float);                                                          \
    RET(grhip_clock_recovery_mm_##SUF##_blk, gain_mu(), float);                                                        \
    RET(grhip_clock_recovery_mm_##SUF##_blk, gain_omega(), float);                                                     \
    RET(grhip_clock_recovery_mm_##SUF##_blk, set_gain_mu(1.f), void);                                                  \
    RET(grhip_clock_recovery_mm_##SUF##_blk, set_gain_omega(1.f), void);                                               \
    RET(grhip_clock_recovery_mm_##SUF##_blk, set_mu(1.f), void);                                                       \
    RET(grhip_clock_recovery_mm_##SUF##_blk, set_omega(1.f), void);                                                    \
    FORECAST(grhip_clock_recovery_mm_##SUF##_blk);                                                                     \
    GENERAL_WORK(grhip_clock_recovery_mm_##SUF##_blk)
MM_SURFACE(ff);
MM_SURFACE(cc);

FACTORY(grhip_make_binary_slicer_fb, grhip_binary_slicer_fb_blk, gr_sync_block, (), grhip_binary_slicer_fb_sptr (*)(int));
WORK(grhip_binary_slicer_fb_blk);
FACTORY(grhip_make_pager_slicer_fb, grhip_pager_slicer_fb_blk, gr_sync_block, (1.f), grhip_pager_slicer_fb_sptr (*)(float, int));
RET(grhip_pager_slicer_fb_blk, dc_offset(), float);
WORK(grhip_pager_slicer_fb_blk);
FACTORY(grhip_make_unpack_k_bits_bb, grhip_unpack_k_bits_bb_blk, gr_sync_interpolator, (1u),
        grhip_unpack_k_bits_bb_sptr (*)(unsigned, int));
WORK(grhip_unpack_k_bits_bb_blk);
FACTORY(grhip_make_framer_sink_1, grhip_framer_sink_1_blk, gr_sync_block, (V(gr_msg_queue_sptr)),
        grhip_framer_sink_1_sptr (*)(gr_msg_queue_sptr, int));
WORK(grhip_framer_sink_1_blk);
FACTORY(grhip_make_correlate_access_code_bb, grhip_correlate_access_code_bb_blk, gr_sync_block, (V(std::string), 0),
        grhip_correlate_access_code_bb_sptr (*)(const std::string &, int, int));
RET(grhip_correlate_access_code_bb_blk, set_access_code(V(std::string)), bool);
WORK(grhip_correlate_access_code_bb_blk);

FACTORY(gr_make_fft_vcc_hip, gr_fft_vcc_hip, gr_fft_vcc, (8, true, V(vf)),
        gr_fft_vcc_hip_sptr (*)(int, bool, const vf &, bool, int));
FACTORY(grhip_make_fft_vcc, grhip_fft_vcc_blk, gr_fft_vcc, (8, true, V(vf)),
        grhip_fft_vcc_sptr (*)(int, bool, const vf &, bool, int));
SAME(grhip_fft_vcc_blk, gr_fft_vcc_hip);
SAME(grhip_fft_vcc_sptr, gr_fft_vcc_hip_sptr);
WORK(gr_fft_vcc_hip);

FACTORY(grhip_make_fft_filter_ccc, grhip_fft_filter_ccc_blk, gr_sync_decimator, (1, V(vc)),
        grhip_fft_filter_ccc_sptr (*)(int, const vc &, int));
RET(grhip_fft_filter_ccc_blk, set_taps(V(vc)), void);
WORK(grhip_fft_filter_ccc_blk);
FACTORY(grhip_make_fft_filter_fff, grhip_fft_filter_fff_blk, gr_sync_decimator, (1, V(vf)),
        grhip_fft_filter_fff_sptr (*)(int, const vf &, int));
RET(grhip_fft_filter_fff_blk, set_taps(V(vf)), void);
WORK(grhip_fft_filter_fff_blk);
FACTORY(grhip_make_fft_vfc, grhip_fft_vfc_blk, gr_sync_block, (8, true, V(vf)),
        grhip_fft_vfc_sptr (*)(int, bool, const vf &, int));
RET(grhip_fft_vfc_blk, set_window(V(vf)), bool);
WORK(grhip_fft_vfc_blk);

FACTORY(grhip_make_pfb_decimator_ccf, grhip_pfb_decimator_ccf_blk, gr_sync_block, (2u, V(vf)),
        grhip_pfb_decimator_ccf_sptr (*)(unsigned, const vf &, unsigned, int));
RET(grhip_pfb_decimator_ccf_blk, set_taps(V(vf)), void);
WORK(grhip_pfb_decimator_ccf_blk);
FACTORY(grhip_make_pfb_channelizer_ccf, grhip_pfb_channelizer_ccf_blk, gr_block, (2u, V(vf)),
        grhip_pfb_channelizer_ccf_sptr (*)(unsigned, const vf &, float, int));
RET(grhip_pfb_channelizer_ccf_blk, set_taps(V(vf)), void);
GENERAL_WORK(grhip_pfb_channelizer_ccf_blk);

#define ARB_SURFACE(SUF)                                                                                               \
    FACTORY(grhip_make_pfb_arb_resampler_##SUF, grhip_pfb_arb_resampler_##SUF##_blk, gr_block, (1.f, V(vf)),           \
            grhip_pfb_arb_resampler_##SUF##_sptr (*)(float, const vf &, unsigned, int));                               \
    RET(grhip_pfb_arb_resampler_##SUF##_blk, set_rate(1.f), void);                                                     \
    RET(grhip_pfb_arb_resampler_##SUF##_blk, set_mode(0), void);                                                       \
    GENERAL_WORK(grhip_pfb_arb_resampler_##SUF##_blk)
ARB_SURFACE(ccf);
ARB_SURFACE(fff);

#define FRAC_SURFACE(SUF)                                                                                              \
    FACTORY(grhip_make_fractional_interpolator_##SUF, grhip_fractional_interpolator_##SUF##_blk, gr_block, (0.f, 1.f), \
            grhip_fractional_interpolator_##SUF##_sptr (*)(float, float, int));                                        \
    RET(grhip_fractional_interpolator_##SUF##_blk, mu(), float);                                                       \
    RET(grhip_fractional_interpolator_##SUF##_blk, interp_ratio(), float);                                             \
    RET(grhip_fractional_interpolator_##SUF##_blk, set_mu(0.f), void);                                                 \
    RET(grhip_fractional_interpolator_##SUF##_blk, set_interp_ratio(1.f), void);                                       \
    RET(grhip_fractional_interpolator_##SUF##_blk, set_mode(0), void);                                                 \
    FORECAST(grhip_fractional_interpolator_##SUF##_blk);                                                               \
    GENERAL_WORK(grhip_fractional_interpolator_##SUF##_blk)
FRAC_SURFACE(ff);
FRAC_SURFACE(cc);

#define RS_SURFACE(SUF, TAP)                                                                                           \
    FACTORY(grhip_make_interp_fir_filter_##SUF, grhip_interp_fir_filter_##SUF, gr_sync_interpolator,                   \
            (2u, V(std::vector<TAP>)), grhip_interp_fir_filter_##SUF##_sptr (*)(unsigned, const std::vector<TAP> &, int)); \
    RET(grhip_interp_fir_filter_##SUF, set_taps(V(std::vector<TAP>)), void);                                           \
    RET(grhip_interp_fir_filter_##SUF, set_mode(0), void);                                                             \
    WORK(grhip_interp_fir_filter_##SUF);                                                                               \
    FACTORY(grhip_make_rational_resampler_base_##SUF, grhip_rational_resampler_base_##SUF, gr_block,                   \
            (2u, 3u, V(std::vector<TAP>)),                                                                             \
            grhip_rational_resampler_base_##SUF##_sptr (*)(unsigned, unsigned, const std::vector<TAP> &, int));        \
    RET(grhip_rational_resampler_base_##SUF, interpolation(), unsigned);                                               \
    RET(grhip_rational_resampler_base_##SUF, decimation(), unsigned);                                                  \
    RET(grhip_rational_resampler_base_##SUF, resampler_history(), unsigned);                                           \
    RET(grhip_rational_resampler_base_##SUF, set_taps(V(std::vector<TAP>)), void);                                     \
    RET(grhip_rational_resampler_base_##SUF, set_mode(0), void);                                                       \
    FORECAST(grhip_rational_resampler_base_##SUF);                                                                     \
    GENERAL_WORK(grhip_rational_resampler_base_##SUF)
RS_SURFACE(ccf, float);
RS_SURFACE(fff, float);
RS_SURFACE(ccc, gr_complex);

FACTORY(grhip_make_pfb_interpolator_ccf, grhip_pfb_interpolator_ccf_blk, gr_sync_interpolator, (2u, V(vf)),
        grhip_pfb_interpolator_ccf_sptr (*)(unsigned, const vf &, int));
RET(grhip_pfb_interpolator_ccf_blk, set_taps(V(vf)), void);
RET(grhip_pfb_interpolator_ccf_blk, set_mode(0), void);
WORK(grhip_pfb_interpolator_ccf_blk);
FACTORY(grhip_make_pfb_synthesis_filterbank_ccf, grhip_pfb_synthesis_filterbank_ccf_blk, gr_sync_interpolator, (2u, V(vf)),
        grhip_pfb_synthesis_filterbank_ccf_sptr (*)(unsigned, const vf &, int));
RET(grhip_pfb_synthesis_filterbank_ccf_blk, taps_per_filter(), unsigned);
RET(grhip_pfb_synthesis_filterbank_ccf_blk, set_taps(V(vf)), void);
RET(grhip_pfb_synthesis_filterbank_ccf_blk, set_mode(0), void);
WORK(grhip_pfb_synthesis_filterbank_ccf_blk);

FACTORY(grhip_make_hilbert_fc, grhip_hilbert_fc_blk, gr_sync_block, (5u), grhip_hilbert_fc_sptr (*)(unsigned, int));
RET(grhip_hilbert_fc_blk, set_mode(0), void);
RET(grhip_hilbert_fc_blk, taps(), vf);
WORK(grhip_hilbert_fc_blk);
FACTORY(grhip_make_filter_delay_fc, grhip_filter_delay_fc_blk, gr_sync_block, (V(vf)),
        grhip_filter_delay_fc_sptr (*)(const vf &, int));
RET(grhip_filter_delay_fc_blk, set_mode(0), void);
WORK(grhip_filter_delay_fc_blk);
FACTORY(grhip_make_goertzel_fc, grhip_goertzel_fc_blk, gr_sync_decimator, (8000, 8, 1.f),
        grhip_goertzel_fc_sptr (*)(int, int, float, int));
RET(grhip_goertzel_fc_blk, set_freq(1.f), void);
RET(grhip_goertzel_fc_blk, set_rate(1), void);
RET(grhip_goertzel_fc_blk, set_mode(0), void);
WORK(grhip_goertzel_fc_blk);

#define DC_BLOCKER_SURFACE(SUF)                                                                                        \
    FACTORY(grhip_make_dc_blocker_##SUF, grhip_dc_blocker_##SUF##_blk, gr_sync_block, (),                              \
            grhip_dc_blocker_##SUF##_sptr (*)(int, bool, int));                                                        \
    RET(grhip_dc_blocker_##SUF##_blk, get_group_delay(), int);                                                         \
    RET(grhip_dc_blocker_##SUF##_blk, set_mode(0), void);                                                              \
    WORK(grhip_dc_blocker_##SUF##_blk)
DC_BLOCKER_SURFACE(ff);
DC_BLOCKER_SURFACE(cc);

#define RUNNING_SURFACE(SUF, ITEM)                                                                                     \
    FACTORY(grhip_make_moving_average_##SUF, grhip_moving_average_##SUF##_blk, gr_sync_block, (4, V(ITEM)),            \
            grhip_moving_average_##SUF##_sptr (*)(int, ITEM, int, int));                                               \
    RET(grhip_moving_average_##SUF##_blk, set_length_and_scale(4, V(ITEM)), void);                                     \
    RET(grhip_moving_average_##SUF##_blk, set_mode(0), void);                                                          \
    WORK(grhip_moving_average_##SUF##_blk);                                                                            \
    FACTORY(grhip_make_integrate_##SUF, grhip_integrate_##SUF##_blk, gr_sync_decimator, (4),                           \
            grhip_integrate_##SUF##_sptr (*)(int, int));                                                               \
    RET(grhip_integrate_##SUF##_blk, set_mode(0), void);                                                               \
    WORK(grhip_integrate_##SUF##_blk)
RUNNING_SURFACE(ff, float);
RUNNING_SURFACE(cc, gr_complex);
RUNNING_SURFACE(ss, short);
RUNNING_SURFACE(ii, int);

FACTORY(gr_make_complex_to_mag_squared, grhip_complex_to_mag_squared_blk, gr_sync_block, (),
        grhip_complex_to_mag_squared_sptr (*)(unsigned int, int));
RET(grhip_complex_to_mag_squared_blk, set_mode(0), void);
WORK(grhip_complex_to_mag_squared_blk);
FACTORY(gr_make_complex_to_mag, grhip_complex_to_mag_blk, gr_sync_block, (), grhip_complex_to_mag_sptr (*)(unsigned int, int));
RET(grhip_complex_to_mag_blk, set_mode(0), void);
WORK(grhip_complex_to_mag_blk);
FACTORY(gr_make_single_pole_iir_filter_ff, grhip_single_pole_iir_filter_ff_blk, gr_sync_block, (0.5),
        grhip_single_pole_iir_filter_ff_sptr (*)(double, unsigned int, int));
RET(grhip_single_pole_iir_filter_ff_blk, set_mode(0), void);
RET(grhip_single_pole_iir_filter_ff_blk, set_taps(0.5), void);
WORK(grhip_single_pole_iir_filter_ff_blk);
FACTORY(gr_make_nlog10_ff, grhip_nlog10_ff_blk, gr_sync_block, (10.f), grhip_nlog10_ff_sptr (*)(float, unsigned, float, int));
RET(grhip_nlog10_ff_blk, set_mode(0), void);
WORK(grhip_nlog10_ff_blk);
FACTORY(gr_make_keep_one_in_n, grhip_keep_one_in_n_blk, gr_block, (sizeof(float), 3),
        grhip_keep_one_in_n_sptr (*)(size_t, int, int));
RET(grhip_keep_one_in_n_blk, set_n(3), void);
GENERAL_WORK(grhip_keep_one_in_n_blk);

#define LOGPWRFFT_SURFACE(NAME)                                                                                        \
    FACTORY(gr_make_##NAME, grhip_##NAME##_blk, gr_block, (1.0, 8, 1.0, 1.0, 1.0, true),                               \
            grhip_##NAME##_sptr (*)(double, int, double, double, double, bool, const vd &, int));                      \
    RET(grhip_##NAME##_blk, set_mode(0), void);                                                                        \
    RET(grhip_##NAME##_blk, set_decimation(1.0), void);                                                                \
    RET(grhip_##NAME##_blk, set_vec_rate(1.0), void);                                                                  \
    RET(grhip_##NAME##_blk, set_sample_rate(1.0), void);                                                               \
    RET(grhip_##NAME##_blk, set_average(true), void);                                                                  \
    RET(grhip_##NAME##_blk, set_avg_alpha(1.0), void);                                                                 \
    RET(grhip_##NAME##_blk, sample_rate(), double);                                                                    \
    RET(grhip_##NAME##_blk, decimation(), int);                                                                        \
    RET(grhip_##NAME##_blk, frame_rate(), double);                                                                     \
    RET(grhip_##NAME##_blk, average(), bool);                                                                          \
    RET(grhip_##NAME##_blk, avg_alpha(), double);                                                                      \
    FORECAST(grhip_##NAME##_blk);                                                                                      \
    GENERAL_WORK(grhip_##NAME##_blk)
LOGPWRFFT_SURFACE(logpwrfft_c);
LOGPWRFFT_SURFACE(logpwrfft_f);

#define PWR_SQUELCH_SURFACE(NAME)                                                                                      \
    FACTORY(gr_make_##NAME, grhip_##NAME##_blk, gr_block, (-10.0), grhip_##NAME##_sptr (*)(double, double, int, bool, int)); \
    RET(grhip_##NAME##_blk, set_mode(0), void);                                                                        \
    RET(grhip_##NAME##_blk, threshold(), double);                                                                      \
    RET(grhip_##NAME##_blk, set_threshold(1.0), void);                                                                 \
    RET(grhip_##NAME##_blk, set_alpha(1.0), void);                                                                     \
    RET(grhip_##NAME##_blk, ramp(), int);                                                                              \
    RET(grhip_##NAME##_blk, set_ramp(1), void);                                                                        \
    RET(grhip_##NAME##_blk, gate(), bool);                                                                             \
    RET(grhip_##NAME##_blk, set_gate(true), void);                                                                     \
    RET(grhip_##NAME##_blk, unmuted(), bool);                                                                          \
    RET(grhip_##NAME##_blk, squelch_range(), vf);                                                                      \
    GENERAL_WORK(grhip_##NAME##_blk)
PWR_SQUELCH_SURFACE(pwr_squelch_cc);
PWR_SQUELCH_SURFACE(pwr_squelch_ff);

FACTORY(gr_make_simple_squelch_cc, grhip_simple_squelch_cc_blk, gr_sync_block, (-10.0),
        grhip_simple_squelch_cc_sptr (*)(double, double, int));
RET(grhip_simple_squelch_cc_blk, set_mode(0), void);
RET(grhip_simple_squelch_cc_blk, unmuted(), bool);
RET(grhip_simple_squelch_cc_blk, set_alpha(1.0), void);
RET(grhip_simple_squelch_cc_blk, set_threshold(1.0), void);
RET(grhip_simple_squelch_cc_blk, threshold(), double);
RET(grhip_simple_squelch_cc_blk, squelch_range(), vf);
WORK(grhip_simple_squelch_cc_blk);

FACTORY(gr_make_ctcss_squelch_ff, grhip_ctcss_squelch_ff_blk, gr_block, (8000, 100.f),
        grhip_ctcss_squelch_ff_sptr (*)(int, float, float, int, int, bool, int));
RET(grhip_ctcss_squelch_ff_blk, set_mode(0), void);
RET(grhip_ctcss_squelch_ff_blk, level(), float);
RET(grhip_ctcss_squelch_ff_blk, set_level(1.f), void);
RET(grhip_ctcss_squelch_ff_blk, len(), int);
RET(grhip_ctcss_squelch_ff_blk, ramp(), int);
RET(grhip_ctcss_squelch_ff_blk, set_ramp(1), void);
RET(grhip_ctcss_squelch_ff_blk, gate(), bool);
RET(grhip_ctcss_squelch_ff_blk, set_gate(true), void);
RET(grhip_ctcss_squelch_ff_blk, unmuted(), bool);
RET(grhip_ctcss_squelch_ff_blk, squelch_range(), vf);
GENERAL_WORK(grhip_ctcss_squelch_ff_blk);

#define AGC_COMMON_SURFACE(NAME)                                                                                       \
    RET(grhip_##NAME##_blk, set_mode(0), void);                                                                        \
    RET(grhip_##NAME##_blk, reference(), float);                                                                       \
    RET(grhip_##NAME##_blk, max_gain(), float);                                                                        \
    RET(grhip_##NAME##_blk, gain(), float);                                                                            \
    RET(grhip_##NAME##_blk, set_reference(1.f), void);                                                                 \
    RET(grhip_##NAME##_blk, set_gain(1.f), void);                                                                      \
    RET(grhip_##NAME##_blk, set_max_gain(1.f), void);                                                                  \
    WORK(grhip_##NAME##_blk)
#define AGC_SURFACE(NAME)                                                                                              \
    FACTORY(gr_make_##NAME, grhip_##NAME##_blk, gr_sync_block, (), grhip_##NAME##_sptr (*)(float, float, float, float, int)); \
    RET(grhip_##NAME##_blk, rate(), float);                                                                            \
    RET(grhip_##NAME##_blk, set_rate(1.f), void);                                                                      \
    AGC_COMMON_SURFACE(NAME)
#define AGC2_SURFACE(NAME)                                                                                             \
    FACTORY(gr_make_##NAME, grhip_##NAME##_blk, gr_sync_block, (),                                                     \
            grhip_##NAME##_sptr (*)(float, float, float, float, float, int));                                          \
    RET(grhip_##NAME##_blk, attack_rate(), float);                                                                     \
    RET(grhip_##NAME##_blk, decay_rate(), float);                                                                      \
    RET(grhip_##NAME##_blk, set_attack_rate(1.f), void);                                                               \
    RET(grhip_##NAME##_blk, set_decay_rate(1.f), void);                                                                \
    AGC_COMMON_SURFACE(NAME)
AGC_SURFACE(agc_cc);
AGC_SURFACE(agc_ff);
AGC2_SURFACE(agc2_cc);
AGC2_SURFACE(agc2_ff);

// gri_control_loop's setters and getters
#define LOOP_SURFACE(X)                                                                                                \
    RET(X, set_mode(0), void);                                                                                         \
    RET(X, set_loop_bandwidth(1.f), void);                                                                             \
    RET(X, set_damping_factor(1.f), void);                                                                             \
    RET(X, set_alpha(1.f), void);                                                                                      \
    RET(X, set_beta(1.f), void);                                                                                       \
    RET(X, set_frequency(1.f), void);                                                                                  \
    RET(X, set_phase(1.f), void);                                                                                      \
    RET(X, get_loop_bandwidth(), float);                                                                               \
    RET(X, get_damping_factor(), float);                                                                               \
    RET(X, get_alpha(), float);                                                                                        \
    RET(X, get_beta(), float);                                                                                         \
    RET(X, get_frequency(), float);                                                                                    \
    RET(X, get_phase(), float)
#define PLL_SURFACE(NAME)                                                                                              \
    FACTORY(gr_make_##NAME, grhip_##NAME##_blk, gr_sync_block, (0.1f, 1.f, -1.f),                                      \
            grhip_##NAME##_sptr (*)(float, float, float, int));                                                        \
    LOOP_SURFACE(grhip_##NAME##_blk);                                                                                  \
    WORK(grhip_##NAME##_blk)
PLL_SURFACE(pll_freqdet_cf);
PLL_SURFACE(pll_refout_cc);
PLL_SURFACE(pll_carriertracking_cc);
RET(grhip_pll_carriertracking_cc_blk, lock_detector(), bool);
RET(grhip_pll_carriertracking_cc_blk, squelch_enable(true), bool);
RET(grhip_pll_carriertracking_cc_blk, set_lock_threshold(1.f), float);

FACTORY(digital_make_costas_loop_cc, grhip_costas_loop_cc_blk, gr_sync_block, (0.1f, 2),
        grhip_costas_loop_cc_sptr (*)(float, int, int));
LOOP_SURFACE(grhip_costas_loop_cc_blk);
WORK(grhip_costas_loop_cc_blk);

FACTORY(digital_make_fll_band_edge_cc, grhip_fll_band_edge_cc_blk, gr_sync_block, (2.f, 0.35f, 45, 0.1f),
        grhip_fll_band_edge_cc_sptr (*)(float, float, int, float, int));
LOOP_SURFACE(grhip_fll_band_edge_cc_blk);
RET(grhip_fll_band_edge_cc_blk, set_samples_per_symbol(2.f), void);
RET(grhip_fll_band_edge_cc_blk, set_rolloff(0.35f), void);
RET(grhip_fll_band_edge_cc_blk, set_filter_size(45), void);
RET(grhip_fll_band_edge_cc_blk, get_samples_per_symbol(), float);
RET(grhip_fll_band_edge_cc_blk, get_rolloff(), float);
RET(grhip_fll_band_edge_cc_blk, get_filter_size(), int);
WORK(grhip_fll_band_edge_cc_blk);

FACTORY(gr_make_pfb_clock_sync_ccf, grhip_pfb_clock_sync_ccf_blk, gr_block, (2.0, 0.1f, V(vf)),
        grhip_pfb_clock_sync_ccf_sptr (*)(double, float, const vf &, unsigned int, float, float, int, int));
RET(grhip_pfb_clock_sync_ccf_blk, set_mode(0), void);
RET(grhip_pfb_clock_sync_ccf_blk, get_taps(), std::vector<vf>);
RET(grhip_pfb_clock_sync_ccf_blk, get_diff_taps(), std::vector<vf>);
RET(grhip_pfb_clock_sync_ccf_blk, get_channel_taps(0), vf);
RET(grhip_pfb_clock_sync_ccf_blk, get_diff_channel_taps(0), vf);
RET(grhip_pfb_clock_sync_ccf_blk, set_loop_bandwidth(1.f), void);
RET(grhip_pfb_clock_sync_ccf_blk, set_damping_factor(1.f), void);
RET(grhip_pfb_clock_sync_ccf_blk, set_alpha(1.f), void);
RET(grhip_pfb_clock_sync_ccf_blk, set_beta(1.f), void);
RET(grhip_pfb_clock_sync_ccf_blk, set_max_rate_deviation(1.f), void);
RET(grhip_pfb_clock_sync_ccf_blk, get_loop_bandwidth(), float);
RET(grhip_pfb_clock_sync_ccf_blk, get_damping_factor(), float);
RET(grhip_pfb_clock_sync_ccf_blk, get_alpha(), float);
RET(grhip_pfb_clock_sync_ccf_blk, get_beta(), float);
RET(grhip_pfb_clock_sync_ccf_blk, get_clock_rate(), float);
RET(grhip_pfb_clock_sync_ccf_blk, k(), float);
RET(grhip_pfb_clock_sync_ccf_blk, error(), float);
RET(grhip_pfb_clock_sync_ccf_blk, slips(), int);
RET(grhip_pfb_clock_sync_ccf_blk, check_topology(1, 1), bool);
GENERAL_WORK(grhip_pfb_clock_sync_ccf_blk);

// the constellation objects: host objects, no GNU Radio base
SAME(grhip_constellation_sptr, boost::shared_ptr<grhip_constellation_obj>);
#define CONSTELLATION_FIXED_SURFACE(KIND)                                                                              \
    SAME(decltype(&digital_make_constellation_##KIND), grhip_constellation_sptr (*)());                                \
    SAME(decltype(digital_make_constellation_##KIND()), grhip_constellation_sptr)
CONSTELLATION_FIXED_SURFACE(bpsk);
CONSTELLATION_FIXED_SURFACE(qpsk);
CONSTELLATION_FIXED_SURFACE(dqpsk);
CONSTELLATION_FIXED_SURFACE(8psk);
SAME(decltype(&digital_make_constellation_calcdist), grhip_constellation_sptr (*)(vc, vu, unsigned int, unsigned int));
SAME(decltype(digital_make_constellation_calcdist(V(vc), V(vu), 4u, 1u)), grhip_constellation_sptr);
SAME(decltype(&digital_make_constellation_psk), grhip_constellation_sptr (*)(vc, vu, unsigned int));
SAME(decltype(digital_make_constellation_psk(V(vc), V(vu), 4u)), grhip_constellation_sptr);
SAME(decltype(&digital_make_constellation_rect),
     grhip_constellation_sptr (*)(vc, vu, unsigned int, unsigned int, unsigned int, float, float));
SAME(decltype(digital_make_constellation_rect(V(vc), V(vu), 4u, 2u, 2u, 1.f, 1.f)), grhip_constellation_sptr);
static_assert(std::is_constructible<grhip_constellation_obj, grhip_constellation *>::value, "made from a C handle");
static_assert(!std::is_convertible<grhip_constellation *, grhip_constellation_obj>::value, "explicitly only");
RET(grhip_constellation_obj, handle(), const grhip_constellation *);
RET(grhip_constellation_obj, points(), vc);
RET(grhip_constellation_obj, pre_diff_code(), vu);
RET(grhip_constellation_obj, apply_pre_diff_code(), bool);
RET(grhip_constellation_obj, rotational_symmetry(), unsigned int);
RET(grhip_constellation_obj, dimensionality(), unsigned int);
RET(grhip_constellation_obj, arity(), unsigned int);
RET(grhip_constellation_obj, bits_per_symbol(), unsigned int);
RET(grhip_constellation_obj, decision_maker(V(const gr_complex *)), unsigned int);
RET(grhip_constellation_obj, decision_maker_pe(V(const gr_complex *), V(float *)), unsigned int);

FACTORY(digital_make_constellation_decoder_cb, grhip_constellation_decoder_cb_blk, gr_block, (V(grhip_constellation_sptr)),
        grhip_constellation_decoder_cb_sptr (*)(grhip_constellation_sptr, int));
FORECAST(grhip_constellation_decoder_cb_blk);
GENERAL_WORK(grhip_constellation_decoder_cb_blk);
FACTORY(gr_make_diff_decoder_bb, grhip_diff_decoder_bb_blk, gr_sync_block, (4u), grhip_diff_decoder_bb_sptr (*)(unsigned int, int));
WORK(grhip_diff_decoder_bb_blk);
FACTORY(gr_make_map_bb, grhip_map_bb_blk, gr_sync_block, (V(std::vector<int>)),
        grhip_map_bb_sptr (*)(const std::vector<int> &, int));
WORK(grhip_map_bb_blk);
FACTORY(digital_make_constellation_receiver_cb, grhip_constellation_receiver_cb_blk, gr_block,
        (V(grhip_constellation_sptr), 0.1f, -1.f, 1.f),
        grhip_constellation_receiver_cb_sptr (*)(grhip_constellation_sptr, float, float, float, int));
LOOP_SURFACE(grhip_constellation_receiver_cb_blk);
RET(grhip_constellation_receiver_cb_blk, form(), int);
GENERAL_WORK(grhip_constellation_receiver_cb_blk);
FACTORY(grhip_make_constellation_demod_cb, grhip_constellation_demod_cb_blk, gr_sync_interpolator,
        (V(grhip_constellation_sptr), 0.1f, -1.f, 1.f),
        grhip_constellation_demod_cb_sptr (*)(grhip_constellation_sptr, float, float, float, bool, bool, int));
LOOP_SURFACE(grhip_constellation_demod_cb_blk);
RET(grhip_constellation_demod_cb_blk, form(), int);
RET(grhip_constellation_demod_cb_blk, engine(), int);
RET(grhip_constellation_demod_cb_blk, set_engine(0), void);
WORK(grhip_constellation_demod_cb_blk);

FACTORY(gr_make_iir_filter_ffd, grhip_iir_filter_ffd_blk, gr_sync_block, (V(vd), V(vd)),
        grhip_iir_filter_ffd_sptr (*)(const vd &, const vd &, int));
RET(grhip_iir_filter_ffd_blk, set_mode(0), void);
RET(grhip_iir_filter_ffd_blk, set_taps(V(vd), V(vd)), void);
RET(grhip_iir_filter_ffd_blk, chunked(), bool);
WORK(grhip_iir_filter_ffd_blk);
FACTORY(gr_make_fm_deemph, grhip_iir_filter_ffd_blk, gr_sync_block, (48000.0), grhip_iir_filter_ffd_sptr (*)(double, double, int));
SAME(decltype(&fm_deemph_taps), void (*)(double, double, vd &, vd &));

FACTORY(grhip_make_fm_demod_cf, grhip_fm_demod_cf_blk, gr_sync_decimator, (1.f, V(vd), V(vd), 4, V(vf)),
        grhip_fm_demod_cf_sptr (*)(float, const vd &, const vd &, int, const vf &, int));
RET(grhip_fm_demod_cf_blk, set_mode(0), void);
RET(grhip_fm_demod_cf_blk, engine(), int);
WORK(grhip_fm_demod_cf_blk);
// gr_make_fm_demod_cf has two forms: on given audio taps, and with the reference's own audio filter
SAME(decltype(static_cast<grhip_fm_demod_cf_sptr (*)(double, int, double, const vf &, double, int)>(&gr_make_fm_demod_cf)),
     grhip_fm_demod_cf_sptr (*)(double, int, double, const vf &, double, int));
SAME(decltype(gr_make_fm_demod_cf(1.0, 4, 5000.0, V(vf))), grhip_fm_demod_cf_sptr);
SAME(decltype(static_cast<grhip_fm_demod_cf_sptr (*)(double, int, double, double, double, double, double, int)>(&gr_make_fm_demod_cf)),
     grhip_fm_demod_cf_sptr (*)(double, int, double, double, double, double, double, int));
SAME(decltype(gr_make_fm_demod_cf(1.0, 4, 5000.0, 3000.0, 4500.0)), grhip_fm_demod_cf_sptr);
FACTORY(gr_make_nbfm_rx, grhip_fm_demod_cf_blk, gr_sync_decimator, (8000, 64000),
        grhip_fm_demod_cf_sptr (*)(int, int, double, double, int));
FACTORY(gr_make_demod_20k0f3e_cf, grhip_fm_demod_cf_blk, gr_sync_decimator, (64000.0, 8),
        grhip_fm_demod_cf_sptr (*)(double, int, int));
FACTORY(gr_make_demod_200kf3e_cf, grhip_fm_demod_cf_blk, gr_sync_decimator, (320000.0, 10),
        grhip_fm_demod_cf_sptr (*)(double, int, int));

FACTORY(grhip_make_am_demod_cf, grhip_am_demod_cf_blk, gr_sync_decimator, (4, V(vf)),
        grhip_am_demod_cf_sptr (*)(int, const vf &, int));
RET(grhip_am_demod_cf_blk, set_mode(0), void);
RET(grhip_am_demod_cf_blk, engine(), int);
RET(grhip_am_demod_cf_blk, audio_taps(), const vf &);
WORK(grhip_am_demod_cf_blk);
FACTORY(gr_make_am_demod_cf, grhip_am_demod_cf_blk, gr_sync_decimator, (64000.0, 8, 5000.0, 5500.0),
        grhip_am_demod_cf_sptr (*)(double, int, double, double, int));
FACTORY(gr_make_demod_10k0a3e_cf, grhip_am_demod_cf_blk, gr_sync_decimator, (64000.0, 8),
        grhip_am_demod_cf_sptr (*)(double, int, int));

// the tap designers
SAME(decltype(&grhip_firdes_root_raised_cosine_taps), vf (*)(double, double, double, double, int));
SAME(decltype(&grhip_firdes_low_pass_taps), vf (*)(double, double, double, double, int, double));
SAME(decltype(grhip_firdes_low_pass_taps(1.0, 1.0, 0.1, 0.1)), vf);
SAME(decltype(&grhip_optfir_low_pass_taps), vd (*)(double, double, double, double, double, double, int));
SAME(decltype(grhip_optfir_low_pass_taps(1.0, 1.0, 0.1, 0.2, 0.1, 60.0)), vd);
SAME(decltype(&grhip_optfir_low_pass_taps_f), vf (*)(double, double, double, double));

// grhip_fir_kernels.h: the kernel-level FIR classes, their sysconfig entries and the N-port adapters
#define FIR_KERNEL_SURFACE(SUF, I, O, TAP)                                                                             \
    static_assert(std::is_base_of<gr_fir_##SUF, gr_fir_##SUF##_hip>::value, "gr_fir_" #SUF "_hip is a gr_fir_" #SUF);  \
    static_assert(std::is_constructible<gr_fir_##SUF##_hip, const std::vector<TAP> &>::value, "device defaults to 0"); \
    static_assert(std::is_constructible<gr_fir_##SUF##_hip, const std::vector<TAP> &, int>::value, "(taps, device)");  \
    RET(gr_fir_##SUF##_hip, filter(V(const I *)), O);                                                                  \
    RET(gr_fir_##SUF##_hip, filterN(V(O *), V(const I *), 1ul), void);                                                 \
    RET(gr_fir_##SUF##_hip, filterNdec(V(O *), V(const I *), 1ul, 1u), void);                                          \
    RET(gr_fir_##SUF##_hip, set_taps(V(std::vector<TAP>)), void);                                                      \
    RET(gr_fir_##SUF##_hip, set_mode(0), void);                                                                        \
    SAME(decltype(&grhip_fir_sysconfig::create_gr_fir_##SUF), gr_fir_##SUF *(*)(const std::vector<TAP> &));            \
    SAME(decltype(&grhip_fir_sysconfig::get_gr_fir_##SUF##_info), void (*)(std::vector<gr_fir_##SUF##_info> *))
FIR_KERNEL_SURFACE(ccf, gr_complex, gr_complex, float);
FIR_KERNEL_SURFACE(fff, float, float, float);
FIR_KERNEL_SURFACE(ccc, gr_complex, gr_complex, gr_complex);
FIR_KERNEL_SURFACE(fcc, float, gr_complex, gr_complex);
FIR_KERNEL_SURFACE(scc, short, gr_complex, gr_complex);
FIR_KERNEL_SURFACE(fsf, float, short, float);

#define ADAPTER_SURFACE(BLK, BASE, ARG2)                                                                               \
    static_assert(std::is_base_of<BASE, BLK>::value, #BLK " derives from " #BASE);                                     \
    static_assert(std::is_constructible<BLK, size_t, ARG2>::value, "device defaults to 0");                            \
    static_assert(std::is_constructible<BLK, size_t, ARG2, int>::value, "(item size, count, device)");                 \
    SAME(decltype(grhip_make_adapter<BLK>(V(size_t), V(ARG2))), boost::shared_ptr<BLK>);                               \
    SAME(decltype(grhip_make_adapter<BLK>(V(size_t), V(ARG2), 0)), boost::shared_ptr<BLK>);                            \
    WORK(BLK)
ADAPTER_SURFACE(grhip_stream_to_streams_blk, gr_sync_decimator, size_t);
ADAPTER_SURFACE(grhip_streams_to_stream_blk, gr_sync_interpolator, size_t);
ADAPTER_SURFACE(grhip_vector_to_streams_blk, gr_sync_block, size_t);
ADAPTER_SURFACE(grhip_stream_to_vector_blk, gr_sync_decimator, size_t);
ADAPTER_SURFACE(grhip_head_blk, gr_sync_block, unsigned long long);
RET(grhip_head_blk, reset(), void);

// set_mode belongs to the blocks stated above and to no other
template <class X, class = void> struct has_set_mode : std::false_type {};
template <class X> struct has_set_mode<X, decltype(std::declval<X &>().set_mode(0))> : std::true_type {};
static_assert(has_set_mode<grhip_hilbert_fc_blk>::value, "the probe finds a set_mode that is there");
#define NO_SET_MODE(X) static_assert(!has_set_mode<X>::value, #X " has no set_mode")
NO_SET_MODE(grhip_fir_filter_ccf); NO_SET_MODE(grhip_fir_filter_fff); NO_SET_MODE(grhip_fir_filter_ccc);
NO_SET_MODE(grhip_fir_filter_fcc); NO_SET_MODE(grhip_fir_filter_scc); NO_SET_MODE(grhip_fir_filter_fsf);
NO_SET_MODE(grhip_quadrature_demod_cf_blk); NO_SET_MODE(grhip_clock_recovery_mm_ff_blk); NO_SET_MODE(grhip_clock_recovery_mm_cc_blk);
NO_SET_MODE(grhip_binary_slicer_fb_blk); NO_SET_MODE(grhip_pager_slicer_fb_blk); NO_SET_MODE(grhip_unpack_k_bits_bb_blk);
NO_SET_MODE(grhip_framer_sink_1_blk); NO_SET_MODE(grhip_correlate_access_code_bb_blk); NO_SET_MODE(gr_fft_vcc_hip);
NO_SET_MODE(grhip_fft_filter_ccc_blk); NO_SET_MODE(grhip_fft_filter_fff_blk); NO_SET_MODE(grhip_fft_vfc_blk);
NO_SET_MODE(grhip_pfb_decimator_ccf_blk); NO_SET_MODE(grhip_pfb_channelizer_ccf_blk); NO_SET_MODE(grhip_keep_one_in_n_blk);
NO_SET_MODE(grhip_constellation_decoder_cb_blk); NO_SET_MODE(grhip_diff_decoder_bb_blk); NO_SET_MODE(grhip_map_bb_blk);
NO_SET_MODE(grhip_stream_to_streams_blk); NO_SET_MODE(grhip_streams_to_stream_blk); NO_SET_MODE(grhip_vector_to_streams_blk);
NO_SET_MODE(grhip_stream_to_vector_blk); NO_SET_MODE(grhip_head_blk);

// no block, no kernel-level FIR and no constellation object can be copied: a copy would destroy the same handle twice
#define NO_COPY(X)                                                                                                     \
    static_assert(!std::is_copy_constructible<X>::value, #X " is not copy-constructible");                             \
    static_assert(!std::is_copy_assignable<X>::value, #X " is not copy-assignable")
NO_COPY(grhip_fir_filter_ccf); NO_COPY(grhip_fir_filter_fff); NO_COPY(grhip_fir_filter_ccc);
NO_COPY(grhip_fir_filter_fcc); NO_COPY(grhip_fir_filter_scc); NO_COPY(grhip_fir_filter_fsf);
NO_COPY(grhip_freq_xlating_fir_filter_ccc_blk); NO_COPY(grhip_freq_xlating_fir_filter_ccf_blk);
NO_COPY(grhip_freq_xlating_fir_filter_fcf_blk); NO_COPY(grhip_freq_xlating_fir_filter_fcc_blk);
NO_COPY(grhip_freq_xlating_fir_filter_scf_blk); NO_COPY(grhip_freq_xlating_fir_filter_scc_blk);
NO_COPY(grhip_quadrature_demod_cf_blk); NO_COPY(grhip_clock_recovery_mm_ff_blk); NO_COPY(grhip_clock_recovery_mm_cc_blk);
NO_COPY(grhip_binary_slicer_fb_blk); NO_COPY(grhip_pager_slicer_fb_blk); NO_COPY(grhip_unpack_k_bits_bb_blk);
NO_COPY(grhip_framer_sink_1_blk); NO_COPY(grhip_correlate_access_code_bb_blk); NO_COPY(gr_fft_vcc_hip);
NO_COPY(grhip_fft_filter_ccc_blk); NO_COPY(grhip_fft_filter_fff_blk); NO_COPY(grhip_fft_vfc_blk);
NO_COPY(grhip_pfb_decimator_ccf_blk); NO_COPY(grhip_pfb_channelizer_ccf_blk);
NO_COPY(grhip_pfb_arb_resampler_ccf_blk); NO_COPY(grhip_pfb_arb_resampler_fff_blk);
NO_COPY(grhip_fractional_interpolator_ff_blk); NO_COPY(grhip_fractional_interpolator_cc_blk);
NO_COPY(grhip_interp_fir_filter_ccf); NO_COPY(grhip_interp_fir_filter_fff); NO_COPY(grhip_interp_fir_filter_ccc);
NO_COPY(grhip_rational_resampler_base_ccf); NO_COPY(grhip_rational_resampler_base_fff); NO_COPY(grhip_rational_resampler_base_ccc);
NO_COPY(grhip_pfb_interpolator_ccf_blk); NO_COPY(grhip_pfb_synthesis_filterbank_ccf_blk);
NO_COPY(grhip_hilbert_fc_blk); NO_COPY(grhip_filter_delay_fc_blk); NO_COPY(grhip_goertzel_fc_blk);
NO_COPY(grhip_dc_blocker_ff_blk); NO_COPY(grhip_dc_blocker_cc_blk);
NO_COPY(grhip_moving_average_ff_blk); NO_COPY(grhip_moving_average_cc_blk); NO_COPY(grhip_moving_average_ss_blk);
NO_COPY(grhip_moving_average_ii_blk);
NO_COPY(grhip_integrate_ff_blk); NO_COPY(grhip_integrate_cc_blk); NO_COPY(grhip_integrate_ss_blk); NO_COPY(grhip_integrate_ii_blk);
NO_COPY(grhip_complex_to_mag_squared_blk); NO_COPY(grhip_complex_to_mag_blk); NO_COPY(grhip_single_pole_iir_filter_ff_blk);
NO_COPY(grhip_nlog10_ff_blk); NO_COPY(grhip_keep_one_in_n_blk); NO_COPY(grhip_logpwrfft_c_blk); NO_COPY(grhip_logpwrfft_f_blk);
NO_COPY(grhip_pwr_squelch_cc_blk); NO_COPY(grhip_pwr_squelch_ff_blk); NO_COPY(grhip_simple_squelch_cc_blk);
NO_COPY(grhip_ctcss_squelch_ff_blk);
NO_COPY(grhip_agc_cc_blk); NO_COPY(grhip_agc_ff_blk); NO_COPY(grhip_agc2_cc_blk); NO_COPY(grhip_agc2_ff_blk);
NO_COPY(grhip_pll_freqdet_cf_blk); NO_COPY(grhip_pll_refout_cc_blk); NO_COPY(grhip_pll_carriertracking_cc_blk);
NO_COPY(grhip_costas_loop_cc_blk); NO_COPY(grhip_fll_band_edge_cc_blk); NO_COPY(grhip_pfb_clock_sync_ccf_blk);
NO_COPY(grhip_constellation_obj); NO_COPY(grhip_constellation_decoder_cb_blk); NO_COPY(grhip_diff_decoder_bb_blk);
NO_COPY(grhip_map_bb_blk); NO_COPY(grhip_constellation_receiver_cb_blk); NO_COPY(grhip_constellation_demod_cb_blk);
NO_COPY(grhip_iir_filter_ffd_blk); NO_COPY(grhip_fm_demod_cf_blk); NO_COPY(grhip_am_demod_cf_blk);
NO_COPY(gr_fir_ccf_hip); NO_COPY(gr_fir_fff_hip); NO_COPY(gr_fir_ccc_hip);
NO_COPY(gr_fir_fcc_hip); NO_COPY(gr_fir_scc_hip); NO_COPY(gr_fir_fsf_hip);
NO_COPY(grhip_stream_to_streams_blk); NO_COPY(grhip_streams_to_stream_blk); NO_COPY(grhip_vector_to_streams_blk);
NO_COPY(grhip_stream_to_vector_blk); NO_COPY(grhip_head_blk);

// ---- Part 2: ownership, on a handle whose destroy function records what it was given ---------------------------------
struct fake_handle {
    int id;
};
static std::vector<fake_handle *> g_destroyed;
static void fake_destroy(fake_handle *h) { g_destroyed.push_back(h); }
static int fake_create(fake_handle **h, fake_handle *storage, int rc)
{
    if (rc >= 0) *h = storage;                      // a failing create leaves the handle null, as the C ABI's do
    return rc;
}
typedef grhip_detail::handle<fake_handle, fake_destroy> fake_owner;
NO_COPY(fake_owner);
static_assert(std::is_move_constructible<fake_owner>::value && std::is_move_assignable<fake_owner>::value, "the owner moves");

struct construction_failed {};
class fake_blk : public grhip_detail::block<gr_sync_block, fake_handle, fake_destroy> {
    friend struct grhip_detail::factory;
protected:
    fake_blk(fake_handle *storage, int create_rc)
        : block("fake", gr_make_io_signature(1, 1, sizeof(float)), gr_make_io_signature(1, 1, sizeof(float)))
    {
        if (fake_create(d_h.out(), storage, create_rc) < 0) throw construction_failed();
    }
public:
    fake_handle *held() const { return d_h.get(); }
    int work(int noutput_items, gr_vector_const_void_star &, gr_vector_void_star &) override { return noutput_items; }
};
NO_COPY(fake_blk);
// what grhip_pfb_arb_resampler_blk and grhip_interp_fir_filter_blk used to leak: the constructor throws after create
class fake_throwing_blk : public fake_blk {
    friend struct grhip_detail::factory;
    fake_throwing_blk(fake_handle *storage) : fake_blk(storage, 0) { throw construction_failed(); }
};

static int g_failures = 0;
#define EXPECT(C)                                                                                                      \
    do {                                                                                                               \
        if (!(C)) {                                                                                                    \
            printf("FAIL line %d: %s\n", __LINE__, #C);                                                                \
            ++g_failures;                                                                                              \
        }                                                                                                              \
    } while (0)

int main()
{
    fake_handle a{1}, b{2};

    // a block built on the base and destroyed calls destroy once, with its pointer
    {
        boost::shared_ptr<fake_blk> blk = grhip_detail::factory::make<fake_blk>(&a, 0);
        EXPECT(blk->held() == &a);
        EXPECT(blk->name() == "fake");
        EXPECT(g_destroyed.empty());
    }
    EXPECT(g_destroyed.size() == 1 && g_destroyed[0] == &a);
    g_destroyed.clear();

    // a derived constructor that throws after the handle was filled: destroy once, with that pointer
    bool threw = false;
    try {
        grhip_detail::factory::make<fake_throwing_blk>(&b);
    } catch (const construction_failed &) {
        threw = true;
    }
    EXPECT(threw);
    EXPECT(g_destroyed.size() == 1 && g_destroyed[0] == &b);
    g_destroyed.clear();

    // a create call that fails leaves the handle null: destroy never sees a pointer
    threw = false;
    try {
        grhip_detail::factory::make<fake_blk>(&a, -1);
    } catch (const construction_failed &) {
        threw = true;
    }
    EXPECT(threw);
    EXPECT(g_destroyed.empty());

    // a moved-from owner releases nothing; the one moved to releases once
    {
        fake_owner from;
        EXPECT(from.get() == nullptr);
        EXPECT(fake_create(from.out(), &a, 0) == 0);
        {
            fake_owner to(std::move(from));
            EXPECT(from.get() == nullptr && to.get() == &a);
            fake_owner assigned(&b);
            assigned = std::move(to);                   // releases what it held (&b), takes &a
            EXPECT(g_destroyed.size() == 1 && g_destroyed[0] == &b);
            EXPECT(to.get() == nullptr && assigned.get() == &a);
        }
        EXPECT(g_destroyed.size() == 2 && g_destroyed[1] == &a);
    }
    EXPECT(g_destroyed.size() == 2);
    g_destroyed.clear();

    // out() on a filled owner releases the old handle before the create call fills it again (gr_fir_XXX_hip::set_taps)
    {
        fake_owner o(&a);
        EXPECT(fake_create(o.out(), &b, 0) == 0);
        EXPECT(g_destroyed.size() == 1 && g_destroyed[0] == &a && o.get() == &b);
    }
    EXPECT(g_destroyed.size() == 2 && g_destroyed[1] == &b);

    if (g_failures) return 1;
    printf("blocks_surface_test: surface and ownership ok\n");
    return 0;
}
