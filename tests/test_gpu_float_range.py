"""Every device entry of tests/test_gpu_device_offsets.py's table off amplitude 1 (tests/float_range.py holds the
classes, the exemptions and the slacks; tests/test_float_range_cpu.py proves them on the references).

Per row, variant and scale 2^k, on the row's larger size, at offsets (0, 0) with aligned strides:
 (a) the result against the block's own CPU reference of the scaled input, under the check the offsets table uses
     (bit for bit where the variant is bit exact, else its tolerance, which is relative to the peak);
 (b) for LINEAR, QUADRATIC and INVARIANT rows the class property on the device, bit for bit against the device's own
     result at amplitude 1 -- except the variants listed in float_range.EXEMPT.
The bit-exact demodulators also run at 2^-66, where x[i] conj(x[i-1]) is subnormal and only (a) holds.

Then one non-finite sample: see test_one_non_finite_sample_stays_local."""
import numpy as np
import pytest

import device_offsets as do
import float_range as fr
import test_gpu_device_offsets as tdo

pytestmark = pytest.mark.gpu

def _run(gpu, po, wl, row, variant, k, poison=None):
    """build the case at amplitude 2^k, run it once, compare with its reference; returns (spec, the payloads)"""
    with tdo.amplitude(2.0 ** k, poison):
        spec = row.build(gpu, po, wl, variant, max(row.sizes))
    ret, outs, post = tdo._run_once(gpu, spec, row.item_sizes(variant), 0, 0, "aligned" if row.strided else "",
                                    do.POISON)
    assert not isinstance(ret, Exception), ret
    if spec.ret is not None:
        assert ret == spec.ret, (ret, spec.ret)
    for o in outs:
        do.check_guards(o)
    if spec.ref_post is not None:
        assert post == spec.ref_post
    return spec, [o.payload() for o in outs]


def _against_reference(spec, got):
    for i, (g_, r_) in enumerate(zip(got, spec.ref)):
        check = spec.check[i] if isinstance(spec.check, list) else spec.check
        if isinstance(r_, list):
            check(g_, r_)
        else:
            check(g_.reshape(np.shape(r_)) if g_.size == np.size(r_) else g_, np.asarray(r_))


_UNIT = {}


def _at_amplitude_1(gpu, po, wl, row, variant):
    key = (row.id, variant)
    if key not in _UNIT:
        _UNIT[key] = _run(gpu, po, wl, row, variant, 0)[1]
    return _UNIT[key]


def _scale_cases():
    return [pytest.param(row, variant, cls, k, id=fr.case_id(row, variant, "k%d" % k))
            for row, variant, cls in fr.cases(tdo.ROWS) for k in fr.scales(row.id, variant)]


@pytest.mark.parametrize("row,variant,cls,k", _scale_cases())
def test_device_entry_at_scale(gpu, po, wl, row, variant, cls, k):
    spec, got = _run(gpu, po, wl, row, variant, k)
    _against_reference(spec, got)                                                   # (a)
    if cls == fr.REFERENCE_ONLY or k == fr.SUBNORMAL or fr.exempt(row.id, variant):
        return
    fr.assert_property(cls, k, got, _at_amplitude_1(gpu, po, wl, row, variant))     # (b)


# ---------------------------------------------------------------------------------------------------------------
# one non-finite sample
# ---------------------------------------------------------------------------------------------------------------
def _direct_form(row, variant):
    """the direct-form LINEAR rows.  Out on purpose: everything that goes through a transform, which spreads one NaN
    over its block as it must (fft_*, fft_filter_*, pfb_channelizer_hier and pfb_synthesis_filterbank_ccf, and the
    fir_filter variants that the plan of csrc/fir_plan.h gives to the overlap-save engine), and the demodulating rows, whose reference indexes its arctangent table with a NaN"""
    if row.id == "fir_filter":
        kind, mode, taps, decim = variant.split("-")
        if mode == "FAST" and taps == "t64":
            # csrc/fir_plan.h: ccf and ccc at decimation 1 (64 taps per component, above the crossovers of 48 and 40) and
            # ccc and fff at 3 (no tiled kernel) are the overlap-save engine.  What stays: the tiled kernel (ccc at 2, fff
            # at 1 and 2), the matrix-core engine (ccf at 2) and the high-decimation direct kernel (ccf at 3)
            return (kind, decim) not in (("ccf", "d1"), ("ccc", "d1"), ("ccc", "d3"), ("fff", "d3"))
        return True
    if row.id == "runsum":
        return variant.startswith("moving_average_ff") or variant.startswith("moving_average_cc")
    return row.id in ("freq_xlating_fir_filter_ccc", "pfb_decimator_ccf", "pfb_channelizer_ccf", "pfb_interpolator_ccf",
                      "interp_fir_filter", "rational_resampler_base", "pfb_arb_resampler", "fractional_interpolator")


def _poison_cases():
    return [pytest.param(row, variant, name, id=fr.case_id(row, variant, name))
            for row, variant, cls in fr.cases(tdo.ROWS) if _direct_form(row, variant) for name in ("inf", "nan")]


@pytest.mark.parametrize("row,variant,what", _poison_cases())
def test_one_non_finite_sample_stays_local(gpu, po, wl, row, variant, what):
    """tests/test_gpu_fir_mfma.py::test_one_non_finite_sample_stays_local for the direct-form rows: the middle sample
    of the input (in the middle tile) is +inf, or NaN.  R: the reference's non-finite outputs, G: the device's.  No
    member of R is finite on the device; G lies within R widened by the variant's slack (float_range.SLACK: 0 for the
    bit-exact variants, for the others what the kernel's padded taps can reach, never more than one tile); every
    output outside G is under the variant's usual check.  The taps are random or a windowed sinc off its zeros, so
    every polyphase row starts with a non-zero tap and R is the filter's support."""
    value = {"inf": np.float32(np.inf), "nan": np.float32(np.nan)}[what]
    with tdo.amplitude(1.0, value):
        spec = row.build(gpu, po, wl, variant, max(row.sizes))
    x = np.asarray(spec.ins[0]["arr"])
    assert fr.bad(x).sum() == 1, "the builder did not place the sample"
    ret, outs, _post = tdo._run_once(gpu, spec, row.item_sizes(variant), 0, 0, "aligned" if row.strided else "",
                                     do.POISON)
    assert not isinstance(ret, Exception), ret
    if spec.ret is not None:
        assert ret == spec.ret, (ret, spec.ret)
    for o in outs:
        do.check_guards(o)
    got, ref = outs[0].payload().reshape(-1), np.asarray(spec.ref[0])
    n_slack = fr.slack(row.id, variant)
    if ref.ndim == 2:                       # pfb_channelizer_ccf: [time, channel]; the sets are sets of output vectors
        got = got.reshape(ref.shape)
        R, G = fr.bad(ref).any(axis=1), fr.bad(got).any(axis=1)
        assert not (fr.bad(ref) & ~fr.bad(got)).any(), "a non-finite output of the reference is finite here"
        extra = np.flatnonzero(G & ~fr.widen(R, n_slack))
        assert R.any() and extra.size == 0, (extra[:4], np.flatnonzero(R)[[0, -1]])
        g, r = got.copy(), ref.copy()
        g[G], r[G] = 0, 0
        spec.check(g.reshape(-1), r)
        return
    fr.assert_local(got, ref, n_slack, spec.check)


@pytest.mark.parametrize("what", ["inf", "nan"])
@pytest.mark.parametrize("mode", ["GENERIC", "FAST"])
@pytest.mark.parametrize("block", ["hilbert_fc", "filter_delay_fc"])
def test_one_non_finite_sample_stays_local_analytic(gpu, po, block, mode, what):
    """hilbert_fc (19 taps: the kernel that uses the taps' structure in FAST) and filter_delay_fc (7 random taps: the
    kernel that uses every tap), on tests/test_gpu_analytic.py's input, references and tolerance.  Neither FAST kernel
    pads its taps (csrc/analytic.hip: `if (k < a.ntaps)`, `if (m < a.nodd)`), so there is no slack.  GENERIC and the
    dense FAST kernel: the reference's sets.  The sparse FAST kernel never multiplies a zero tap, which include/grhip.h
    states at gr_filter_delay_fc: its imaginary part is non-finite exactly at the odd distances from the sample, the
    reference's also at the even ones (0 * inf); the real part carries the sample itself."""
    import analytic_ref as ar
    from test_gpu_analytic import _close, _stream
    n = 3 * 1024 + 29
    if block == "hilbert_fc":
        nt, taps = 19, ar.firdes_hilbert(19)
        blk = gpu.hilbert_fc(nt)
    else:
        nt, taps = 7, np.random.default_rng(307).standard_normal(7).astype(np.float32)
        blk = gpu.filter_delay_fc(taps)
    x = _stream(900 + nt, n + nt - 1)
    s, h = len(x) // 2, nt // 2
    x[s] = {"inf": np.inf, "nan": np.nan}[what]
    blk.set_mode(getattr(gpu, "MODE_" + mode))
    got = np.asarray(blk.work(n, x))
    ref = ar.filter_delay_fc(po, taps, n, x)
    dist = np.abs(np.arange(n) + h - s)                                  # of the sample from each output's centre
    assert np.array_equal(fr.bad(ref.imag), dist <= h) and np.array_equal(fr.bad(ref.real), dist == 0)
    assert np.array_equal(fr.bad(got.real), dist == 0)
    if mode == "GENERIC":
        fr.assert_local(got, ref, 0, tdo.exact)
        return
    sparse = block == "hilbert_fc"
    assert blk.is_sparse() == sparse
    want_bad = (dist <= h) & (dist % 2 == 1) if sparse else dist <= h
    G = fr.bad(got.imag)
    assert np.array_equal(G, want_bad), (np.flatnonzero(G), np.flatnonzero(want_bad))
    clean = ~(dist <= h)                                                 # the float64 sum is NaN on the whole support
    ref64 = ar.filter_delay_fc64(taps, n, x)
    assert _close(got.imag[clean], ref64.imag[clean])
    keep = dist != 0
    assert np.array_equal(got.real[keep], x[h:h + n][keep])
    if sparse:
        # inside the support, at the even distances: the sum over the odd taps, which the sample is not part of
        y = x.astype(np.float64)
        y[s] = 0.0
        inner = (dist <= h) & ~want_bad
        want = ar.filter_delay_fc64(taps, n, y).imag
        assert np.abs(got.imag[inner] - want[inner]).max() <= 1e-5 * np.abs(want[clean]).max()


@pytest.mark.parametrize("k", fr.SCALES)
@pytest.mark.parametrize("mode", ["GENERIC", "FAST"])
def test_complex_to_mag_at_scale(gpu, mode, k):
    """complex_to_mag has no row in the offsets table.  Its one form in every mode is
    (float)sqrt((double)re * re + (double)im * im), every step rounded once (include/grhip.h): LINEAR.  Against that
    form in numpy bit for bit, and bit for bit 2^k times the device's own amplitude-1 result."""
    n = 3 * 256 + 37
    x = tdo._rc(np.random.default_rng(n), n, scaled=False)

    def run(a):
        xa = x * np.float32(a)
        blk = gpu.complex_to_mag()
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        want = np.sqrt(xa.real.astype(np.float64) ** 2 + xa.imag.astype(np.float64) ** 2).astype(np.float32)
        return np.asarray(blk.work(n, xa)), want

    got, want = run(2.0 ** k)
    assert np.isfinite(want).all() and (want >= np.finfo(np.float32).tiny).all()
    tdo.exact(got, want)
    fr.assert_property(fr.LINEAR, k, [got], [run(1.0)[0]])
