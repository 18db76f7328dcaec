"""grhip -- Python face of libgrhip.so (ctypes over the C ABI in include/grhip.h).

Mirrors the names the reference's SWIG layer gives the same blocks
(gr.fir_filter_ccf, gr.freq_xlating_fir_filter_ccc, gr.quadrature_demod_cf,
digital.clock_recovery_mm_ff, digital.correlate_access_code_bb,
digital.binary_slicer_fb, pager.slicer_fb, gr.unpack_k_bits_bb, gr.fft_vcc, gr.fft_vfc, gr.fft_filter_ccc, gr.fft_filter_fff,
gr.pfb_channelizer_ccf, gr.pfb_arb_resampler_ccf / _fff, gr.fractional_interpolator_ff / _cc, gr.hilbert_fc,
gr.filter_delay_fc, gr.goertzel_fc, gr.firdes.hilbert, gr.dc_blocker_ff / _cc, gr.moving_average_XX,
gr.integrate_XX, gr.complex_to_mag_squared, gr.single_pole_iir_filter_ff, gr.nlog10_ff, gr.keep_one_in_n,
gr.pwr_squelch_cc / _ff, gr.simple_squelch_cc, gr.ctcss_squelch_ff, gr.agc_cc / _ff, gr.agc2_cc / _ff,
gr.iir_filter_ffd, blks2.fm_deemph, blks2.fm_demod_cf, blks2.nbfm_rx, gr.firdes.low_pass, gr.remez, optfir.low_pass /
high_pass / band_pass / band_reject (as optfir_*), gr.complex_to_mag, blks2.am_demod_cf, blks2.demod_10k0a3e_cf,
blks2.demod_20k0f3e_cf, blks2.demod_200kf3e_cf, gr.interp_fir_filter_XXX,
gr.rational_resampler_base_XXX, blks2.rational_resampler_XXX, gr.pfb_interpolator_ccf,
gr.pfb_synthesis_filterbank_ccf, gr.packed_to_unpacked_bb, gr.unpacked_to_packed_bb, gr.diff_encoder_bb,
gr.chunks_to_symbols_bc, digital.generic_mod, psk_mod, qam_mod, bpsk_mod, dbpsk_mod, qpsk_mod, dqpsk_mod,
gr.scrambler_bb, gr.descrambler_bb, gr.additive_scrambler_bb, digital.crc32 / update_crc32 (on a crc32 handle),
packet_utils.make_packet / unmake_packet in batches as packet_maker / packet_check, gr.frequency_modulator_fc,
gr.bytes_to_syms, gr.char_to_float, gr.chunks_to_symbols_bf, gr.cpm.phase_response (as cpm_phase_response),
gr.firdes.gaussian (as firdes_gaussian), digital.cpmmod_bc, digital.gmskmod_bc, digital.gmsk_mod, trellis.fsm,
trellis.encoder_XX / metrics_X / constellation_metrics_cf / viterbi_X / viterbi_combined_XX (as trellis_*)) with the same
constructor arguments; `work()` takes/returns numpy arrays with the
gr_sync_block contract (history items in front of the input).

There is no CPU fallback: every call goes to the HIP library and raises if it
is missing or no GPU is present.  The directory name is not a Python
identifier; load it with `import_grhip()` from grhip_loader.py (repo root).
"""
from .binding import *  # noqa: F401,F403
from .binding import __all__ as _b_all
from . import workload  # noqa: F401

__all__ = list(_b_all) + ["workload"]
