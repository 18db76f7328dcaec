"""Every device entry over the float range: what each row of tests/test_gpu_device_offsets.py does when its input is
multiplied by a power of two, and how far one non-finite sample may spread.  No GPU code: the tables and comparison
functions here are used by tests/test_gpu_float_range.py on the device and proven by tests/test_float_range_cpu.py on
the references alone.

A row's class is what its REFERENCE does under x -> s * x, s = 2^k:

    LINEAR          ref(s x) == s ref(x)            QUADRATIC       ref(s x) == s^2 ref(x)
    INVARIANT       ref(s x) == ref(x)              REFERENCE_ONLY  nothing to say beyond the reference at that scale
    SKIP            integer or byte data, no amplitude

bit for bit, because multiplying by a power of two commutes with every rounding while nothing underflows or
overflows.  A device variant that is data-independent float arithmetic has the same property bit for bit; the ones
that do not are listed in EXEMPT with the line of code that is the reason."""
import numpy as np

from conftest import bits_equal

LINEAR, QUADRATIC, INVARIANT, REFERENCE_ONLY, SKIP = "LINEAR", "QUADRATIC", "INVARIANT", "REFERENCE_ONLY", "SKIP"

SCALES = (-40, -16, 15, 40)     # an attenuated front end, int16 samples, and two far ends; every intermediate normal
SUBNORMAL = -66                 # x[i] * conj(x[i-1]) subnormal: the bit-exact demodulators only

# (row id, the variant's first words or "" for all, class, the reason, read from the reference or the kernel).  The
# first entry that matches decides.
CLASSES = [
    ("fir_filter", "", LINEAR, "a dot product with constant taps"),
    ("freq_xlating_fir_filter_ccc", "", LINEAR, "a dot product, then a product with a phasor of modulus 1"),
    ("xlating_demod", "", INVARIANT, "gain * atan2 of x[i] conj(x[i-1]): s^2 cancels in the quotient"),
    ("quadrature_demod_cf", "", INVARIANT, "gain * atan2 of x[i] conj(x[i-1]): s^2 cancels in the quotient"),
    ("pager_slicer_fb", "", REFERENCE_ONLY, "pager_slicer_fb compares against fixed levels around its running mean"),
    ("unpack_k_bits_bb", "", SKIP, "bytes"),
    ("framer_sink_1", "", SKIP, "bytes"),
    ("stream_to_streams", "", SKIP, "items are moved, never read as numbers"),
    ("streams_to_stream", "", SKIP, "items are moved, never read as numbers"),
    ("vector_to_streams", "", SKIP, "items are moved, never read as numbers"),
    ("fft_vcc", "", LINEAR, "window and butterflies: products with constants, sums"),
    ("fft_filter_ccc", "", LINEAR, "transform, product with the taps' transform, inverse transform"),
    ("pfb_channelizer_ccf", "", LINEAR, "polyphase dot products, then a transform"),
    ("pfb_channelizer_hier", "", LINEAR, "polyphase dot products, then a transform"),
    ("fft_vfc", "", LINEAR, "window and butterflies: products with constants, sums"),
    ("fft_filter_fff", "", LINEAR, "transform, product with the taps' transform, inverse transform"),
    ("pfb_decimator_ccf", "", LINEAR, "polyphase dot products, then one bin of a transform"),
    ("pfb_synthesis_filterbank_ccf", "", LINEAR, "a transform, then polyphase dot products"),
    ("pfb_interpolator_ccf", "", LINEAR, "polyphase dot products"),
    ("interp_fir_filter", "", LINEAR, "polyphase dot products"),
    ("rational_resampler_base", "", LINEAR, "polyphase dot products"),
    ("pfb_arb_resampler", "", LINEAR, "two dot products and a blend whose weight comes from the rate alone"),
    ("fractional_interpolator", "", LINEAR, "a dot product with the MMSE taps of a phase that comes from the ratio alone"),
    ("runsum", "moving_average_ss", SKIP, "int16"),
    ("runsum", "moving_average_ii", SKIP, "int32"),
    ("runsum", "integrate_ss", SKIP, "int16"),
    ("runsum", "", LINEAR, "sums, differences and one product with a constant"),
    ("spectrum", "complex_to_mag_squared", QUADRATIC, "re * re + im * im"),
    ("spectrum", "single_pole_iir_filter_ff", LINEAR, "y = alpha x + (1 - alpha) y from y = 0"),
    ("spectrum", "nlog10_ff", REFERENCE_ONLY, "a logarithm: the scale becomes an offset that is rounded"),
    ("keep_one_in_n", "", SKIP, "items are moved, never read as numbers"),
    ("logpwrfft", "", REFERENCE_ONLY, "ends in a logarithm"),
    ("squelch", "", REFERENCE_ONLY, "a power threshold"),
    ("ctcss_squelch_ff", "", REFERENCE_ONLY, "a tone level threshold"),
    ("agc2_cc", "", REFERENCE_ONLY, "the gain loop's reference level is absolute"),
    ("clock_recovery_mm_ff", "", REFERENCE_ONLY, "the timing error term is quadratic, the loop gains are not"),
    ("xlating_demod_run_captures", "", INVARIANT, "xlating_demod on several captures"),
    ("dmr_chain", "", INVARIANT, "everything behind the demodulator sees the same floats"),
]

# Variants of LINEAR, QUADRATIC and INVARIANT rows whose device result is NOT required to have the class property
# bit for bit against its own amplitude-1 result: (row id, a word of the variant, the code that is the reason).  They
# keep the comparison with the reference at every scale.
#
# None.  The two candidates were read and are held to the property:
#  - the matrix-core FIR (fir_filter ccf FAST with 64 taps at decimation 1 and 2, xlating_demod / run_captures /
#    dmr_chain FAST) scales a tile by 2^(14 - exponent of the tile's peak) (csrc/fir_mfma.hip:383-386, :1330-1334):
#    the input times 2^k moves that exponent by k and leaves every binary16 half and every product as it was;
#  - the chunked forms (running sums, single_pole_iir_filter_ff FAST) choose their path from the shape and the
#    coefficients, never from a sample; the fused demodulator's quotient is ldexp(num, -e) * rcp(mantissa(den))
#    (csrc/device_math.h), which cancels a common power of two exactly.
EXEMPT = []

FACTOR = {LINEAR: 1, QUADRATIC: 2, INVARIANT: 0}


def _matches(entry, row_id, variant):
    return entry[0] == row_id and (entry[1] == "" or variant.startswith(entry[1]))


def classify(row_id, variant):
    """(class, reason) of a row's variant; KeyError for a row the table does not know"""
    for e in CLASSES:
        if _matches(e, row_id, variant):
            return e[2], e[3]
    raise KeyError("no class for %s %s" % (row_id, variant))


def exempt(row_id, variant):
    """the reason why this variant need not be bit homogeneous, or None"""
    for rid, word, reason in EXEMPT:
        if rid == row_id and word in variant.split("-"):
            return reason
    return None


def bit_exact_demodulator(row_id, variant):
    """the variants that also run at SUBNORMAL"""
    return row_id == "quadrature_demod_cf" or (
        row_id in ("xlating_demod", "xlating_demod_run_captures") and variant.startswith("GENERIC"))


# Rows that cannot take every scale, because their reference cannot: with samples of 2^15 the first timing error of
# digital_clock_recovery_mm_ff (.cc:113-131) moves its position by 0.3 * 2^15 samples, before its buffer or behind it,
# and with 2^40 the step no longer fits the `int` it is converted to.  The restated reference follows it there, so it
# is never given such input; what the device does with a loud input is tests/test_gpu_mm_dynamics.py's subject.
ONLY_SCALES = {"clock_recovery_mm_ff": (-40, -16)}


def scales(row_id, variant):
    base = ONLY_SCALES.get(row_id, SCALES)
    return base + ((SUBNORMAL,) if bit_exact_demodulator(row_id, variant) else ())


def cases(rows):
    """(row, variant, class) for every variant of every row that has an amplitude"""
    out = []
    for row in rows:
        for variant in row.variants:
            cls = classify(row.id, variant)[0]
            if cls != SKIP:
                out.append((row, variant, cls))
    return out


def case_id(row, variant, *more):
    return "-".join(str(p) for p in ((row.id if not variant.startswith(row.id) else "", variant) + more) if p != "")


def flatten(ref):
    """the arrays of a Spec's reference list (per-stream references are lists of arrays of unequal lengths)"""
    out = []
    for r in ref:
        if isinstance(r, (list, tuple)):
            out += flatten(r)
        else:
            out.append(np.asarray(r))
    return out


def is_float(a):
    return a.dtype.kind in "fc"


def bad(a):
    """bool per item: not finite (either part of a complex item)"""
    return ~np.isfinite(a) if is_float(a) else np.zeros(a.shape, bool)


def scaled(base, cls, k):
    """what a result `base` at amplitude 1 becomes at amplitude 2^k under the class: float items times 2^(k * factor),
    exactly; integer items and items that are not finite (the pre-fill behind a short result) as they are"""
    base = np.asarray(base)
    if not is_float(base) or FACTOR[cls] == 0:
        return base
    f = np.float32(2.0) ** np.float32(k * FACTOR[cls])
    assert np.isfinite(f) and f > 0
    out = base.copy()
    m = ~bad(base)
    out[m] = base[m] * f
    return out


def assert_property(cls, k, at_k, at_1, what="result"):
    """lists of arrays at amplitude 2^k and at amplitude 1: the class property, bit for bit"""
    assert len(at_k) == len(at_1), (len(at_k), len(at_1))
    for i, (a, b) in enumerate(zip(at_k, at_1)):
        want = scaled(b, cls, k)
        if not bits_equal(a, want):
            a, want = np.asarray(a), np.asarray(want)
            if a.shape != want.shape or a.dtype != want.dtype:
                raise AssertionError("%s %d: %s %s against %s %s" % (what, i, a.shape, a.dtype, want.shape, want.dtype))
            w = a.dtype.itemsize
            diff = np.flatnonzero((np.ascontiguousarray(a).view(np.uint8).reshape(-1, w) !=
                                   np.ascontiguousarray(want).view(np.uint8).reshape(-1, w)).any(axis=1))
            raise AssertionError("%s %d at 2^%d is not %s in the one at amplitude 1: %d of %d item(s) differ, the first "
                                 "at %s" % (what, i, k, cls, diff.size, a.size, diff[:4]))


def flush_subnormals(a):
    """what a kernel that runs with denormals flushed would leave: for the harness check"""
    a = np.array(a, copy=True)
    parts = a.view(np.float32) if is_float(a) else a
    if is_float(a):
        parts[(np.abs(parts) < np.finfo(np.float32).tiny) & (parts != 0)] = 0
    return a


# ---------------------------------------------------------------------------------------------------------------
# one non-finite sample stays local
# ---------------------------------------------------------------------------------------------------------------
# Outputs that may be non-finite on the device next to the reference's own, on either side: (row id, words that all
# occur in the variant, slack, where it comes from).  A kernel that pads a tap row with zeros, or lets outputs share a
# loop over the union of their supports, multiplies a zero with a sample outside an output's support, and 0 * inf is
# NaN.  The numbers are derived from the padding for the shapes of the table, not measured; a variant that is not
# listed has none (every GENERIC variant, and the FAST kernels that run each row over its own taps only).  Never more
# than one tile of the kernel (TILE): that cap is a condition.
SLACK = [
    # csrc/fir_tiled.hip: Tq = taps per polyphase component rounded up to TILED_R = 8 (tiled_Tq); a component with
    # floor(ntaps / D) taps has Tq - floor(ntaps / D) zero taps, one output each.  fff runs as pairs at D = 2 * decim
    # (FP mode): one kernel output is two floats.
    ("fir_filter", ("ccf", "FAST", "t9", "d1"), 7, "fir_tiled: 9 taps padded to Tq = 16"),
    ("fir_filter", ("ccc", "FAST", "t9", "d1"), 7, "fir_tiled: 9 taps padded to Tq = 16"),
    ("fir_filter", ("ccf", "FAST", "t9", "d2"), 4, "fir_tiled: components of 5 and 4 taps padded to Tq = 8"),
    ("fir_filter", ("ccc", "FAST", "t9", "d2"), 4, "fir_tiled: components of 5 and 4 taps padded to Tq = 8"),
    ("fir_filter", ("fff", "FAST", "t9", "d1"), 8, "fir_tiled pairs, D = 2: components of 5 and 4 taps, Tq = 8, 2 floats each"),
    ("fir_filter", ("fff", "FAST", "t9", "d2"), 12, "fir_tiled pairs, D = 4: components of 3 and 2 taps, Tq = 8, 2 floats each"),
    # csrc/fir_mfma.hip, csrc/mfma_tables.h: a block of BLK = 16 outputs is a band matrix times KS k-steps of CHUNK = 32
    # samples, KS = 6 for short filters (ksteps_inst).  64 taps at decimation 2 fill 15 * 2 + 64 = 94 of the 192
    # columns, the rest are zeros: a sample up to 98 samples = 49 outputs behind a block's last window reaches all 16
    # outputs of the block, 15 + 49 = 64 outputs in front of the reference's first
    ("fir_filter", ("ccf", "FAST", "t64", "d2"), 64, "fir_mfma: 16-output blocks over 6 k-steps of 32 samples"),
    # csrc/fir_kernels.hip fir_hidec_kernel: a lane forms two adjacent outputs in one loop over k in [0, ntaps + D)
    # rounded up to NSUB = 2 P taps (P the power of two in D; D = 3: NSUB = 2) over a tap table padded with zeros: an
    # output meets up to D + NSUB - 1 samples outside its support, 1 + ceil((NSUB - 1) / D) outputs
    ("fir_filter", ("ccf", "FAST", "d3"), 2, "fir_hidec: pairs of outputs over ntaps + D taps rounded up to 2"),
    ("fir_filter", ("ccc", "FAST", "t9", "d3"), 2, "fir_hidec: pairs of outputs over ntaps + D taps rounded up to 2"),
    ("freq_xlating_fir_filter_ccc", ("FAST_VALU", "d3"), 2, "fir_hidec: pairs of outputs over ntaps + D taps rounded up to 2"),
    ("freq_xlating_fir_filter_ccc", ("FAST_VALU", "t9", "d1"), 7, "fir_tiled: 9 taps padded to Tq = 16"),
    # csrc/capi_pfbdec.hip:119: tpf4 = taps per filter rounded up to 4; 7 taps per filter here
    ("pfb_decimator_ccf", (), 1, "pfb_dec_kernel: 7 taps per filter padded to tpf4 = 8"),
    # csrc/fft_kernels.hip:544: tpfp = taps per filter rounded up to R = 8; 5 taps per filter here; one input step
    # is `oversample rate` output vectors
    ("pfb_channelizer_ccf", ("M8",), 3, "5 taps per filter padded to tpfp = 8"),
    ("pfb_channelizer_ccf", ("M5",), 3, "5 taps per filter padded to tpfp = 8"),
    ("pfb_channelizer_ccf", ("M8os2",), 6, "5 taps per filter padded to tpfp = 8, two output vectors per input step"),
    # csrc/resampler.hip rs_kernel, generic = false: the RG residues of a wave task (RG = P for P <= 4, rs_group) run
    # one loop over the union of their supports on tap rows padded with WP zeros: a sample in the union reaches all RG
    # outputs of the period
    ("rational_resampler_base", ("FAST", "I3"), 2, "rs_kernel: groups of RG = 3 residues share their loop"),
    ("rational_resampler_base", ("FAST", "I2"), 1, "rs_kernel: groups of RG = 2 residues share their loop"),
    # csrc/running_sum.hip win_fast_kernel: a window that starts at offset r != 0 of a block of D = length samples is
    # P[block end] - P[m - 1] + P[m + D - 1]; behind a non-finite sample both prefix sums of the block carry it, so
    # every window that starts later in that block has it too: up to D - 1 = 9 outputs
    ("runsum", ("moving_average_ff", "FAST"), 9, "win_fast_kernel: prefix sums within blocks of `length` = 10"),
    ("runsum", ("moving_average_cc", "FAST"), 9, "win_fast_kernel: prefix sums within blocks of `length` = 10"),
]
# outputs per tile of the kernels above (TILED_NT; hidec_outputs_per_tile at G = 1; PFBDEC_TILE; TT; 64 periods of P
# residues at the least; 256 R - halo >= 256)
TILE = {"fir_filter": 512, "freq_xlating_fir_filter_ccc": 512, "pfb_decimator_ccf": 1024, "pfb_channelizer_ccf": 512,
        "rational_resampler_base": 128, "runsum": 256}


def slack(row_id, variant):
    words = variant.split("-")
    for rid, need, n, _why in SLACK:
        if rid == row_id and all(w in words for w in need):
            return n
    return 0


def widen(mask, n):
    """the 1-D mask with every True spread n items to both sides"""
    mask = np.asarray(mask, bool)
    if n == 0 or not mask.any():
        return mask.copy()
    idx = np.flatnonzero(mask)
    out = mask.copy()
    for d in range(1, n + 1):
        out[np.clip(idx - d, 0, mask.size - 1)] = True
        out[np.clip(idx + d, 0, mask.size - 1)] = True
    return out


def assert_local(got, ref, n_slack, check):
    """got, ref: 1-D results of a run on an input with one non-finite sample (got may be longer than ref: a short
    result in a pre-filled buffer).  R, G: where the reference, the device is not finite.  R within G; G within R
    widened by n_slack; everything outside G under `check` as in a clean run."""
    got, ref = np.asarray(got), np.asarray(ref)
    p = ref.size
    assert got.ndim == 1 and ref.ndim == 1 and got.size >= p, (got.shape, ref.shape)
    R, G = bad(ref), bad(got[:p])
    assert R.any(), "the reference shows nothing of the non-finite sample: the case tests nothing"
    hidden = np.flatnonzero(R & ~G)
    assert hidden.size == 0, "%d non-finite output(s) of the reference are finite here, the first at %s" % (
        hidden.size, hidden[:4])
    extra = np.flatnonzero(G & ~widen(R, n_slack))
    assert extra.size == 0, ("%d non-finite output(s) more than %d away from the reference's (%d..%d), the first at %s"
                             % (extra.size, n_slack, np.flatnonzero(R)[0], np.flatnonzero(R)[-1], extra[:4]))
    g, r = got.copy(), ref.copy()
    g[:p][G] = 0
    r[G] = 0
    check(g, r)
