"""CPU tests of gr_rational_resampler_base_XXX / gr_interp_fir_filter_XXX: the closed-form schedule against the
reference's ctr walk, forecast, the tap bank, the blks2 front end, design_filter against the reference's own
gr_firdes taps (tests/golden/ref_firdes_kaiser.npz), and the product's refusals that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import resampler_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closed_form_equals_literal_walk():
    rng = np.random.default_rng(3)
    for I in range(1, 65):
        for D in range(1, 65):
            c0 = int(rng.integers(0, I))
            n = int(rng.integers(0, 200))
            a = rr.literal_walk(I, D, c0, n)
            b = rr.closed_form(I, D, c0, n)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (I, D, c0)
            assert a[2] == b[2] and a[3] == b[3], (I, D, c0)


def test_closed_form_over_random_call_splits():
    rng = np.random.default_rng(4)
    for _ in range(300):
        I, D = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        total = int(rng.integers(1, 600))
        fs, offs, ctr_end, consumed = rr.literal_walk(I, D, 0, total)
        ctr, base, got_f, got_o = 0, 0, [], []
        left = total
        while left:
            n = int(rng.integers(1, left + 1))
            f, o, ctr2, c = rr.closed_form(I, D, ctr, n)
            got_f.append(f)
            got_o.append(o + base)
            ctr, base, left = ctr2, base + c, left - n
        assert np.array_equal(np.concatenate(got_f), fs) and np.array_equal(np.concatenate(got_o), offs)
        assert ctr == ctr_end and base == consumed


def test_forecast_double_truncation():
    assert rr.forecast(3, 2, 101, 0) == int(1.0 * 2 / 3) + 100 == 100
    assert rr.forecast(3, 2, 101, 1) == 101
    assert rr.forecast(2, 3, 5, 1) == 3 + 4
    assert rr.forecast(160, 147, 101, 159) == 147 + 100
    assert rr.forecast(7, 1, 1, 5) == 1                  # max(1, 0 + 0)
    # (double)(n+1)*D/I truncated: 10 * 3 / 7 = 4.28 -> 4
    assert rr.forecast(7, 3, 2, 9) == 4 + 1
    for I, D, nt, n in [(5, 7, 3, 11), (160, 147, 101, 1000), (1, 3, 10, 0)]:
        assert rr.forecast(I, D, nt, n) == max(1, int((n + 1) * D / I) + nt - 1)


def test_front_padding_and_bank_split():
    taps = np.arange(1, 8, dtype=np.float32)           # 7 taps, I = 3: two zeros in FRONT
    p = rr.front_pad(taps, 3)
    assert list(p) == [0, 0, 1, 2, 3, 4, 5, 6, 7]
    nt, fwd = rr.bank(taps, 3)
    assert nt == 3
    assert fwd.tolist() == [[0, 2, 5], [0, 3, 6], [1, 4, 7]]
    nt, fwd = rr.bank(np.ones(12, np.float32), 4)       # a multiple of I: no padding
    assert nt == 3 and fwd.shape == (4, 3) and fwd.sum() == 12
    nt, fwd = rr.bank(np.array([2.0], np.float32), 5)   # one tap: four zeros, then the tap at filter 4
    assert nt == 1 and fwd[:, 0].tolist() == [0, 0, 0, 0, 2]


def test_restatement_call_splits_equal_whole_stream(po):
    rng = np.random.default_rng(5)
    for I, D, ntaps, cplx in [(3, 2, 20, True), (2, 3, 7, False), (5, 7, 11, True), (4, 1, 9, False)]:
        taps = rng.standard_normal(ntaps).astype(np.float32)
        x = rng.standard_normal(700).astype(np.float32)
        if cplx:
            x = (x + 1j * rng.standard_normal(700)).astype(np.complex64)
        ref = rr.whole_rational(po, I, D, taps, x)
        blk = rr.RationalRef(po, I, D, taps)
        rd, outs = 0, []
        while True:
            n = int(rng.integers(1, 60))
            while n and (rr.closed_form(I, D, blk.d_ctr, n)[1][-1] + blk.nt > len(x) - rd):
                n -= 1
            if n == 0:
                break
            out, c = blk.general_work(n, x[rd:])
            outs.append(out)
            rd += c
        got = np.concatenate(outs)
        assert len(got) == len(ref) and np.array_equal(got, ref)


# ---- blks2.rational_resampler_XXX / design_filter ----

def test_design_filter_matches_reference_firdes(g):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_firdes_kaiser.npz"))
    n = 0
    for k in z.files:
        if k == "note":
            continue
        I = int(k.split("_")[0][1:])
        fbw = float(k.split("fbw")[1])
        ref = z[k]
        got = g.design_filter(I, 7, fbw)
        assert got.dtype == np.float32 and len(got) == len(ref), k
        ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (k, int(ulp.max()))
        n += 1
    assert n == 12
    assert len(g.design_filter(1, 1, 0.4)) == 101 and len(g.design_filter(160, 147, 0.4)) == 16001


def test_design_filter_bandwidth_checks(g):
    for fbw in (0.5, 0.0, -0.1, 0.7):
        with pytest.raises(ValueError):
            g.design_filter(3, 2, fbw)


def test_blks2_argument_checks(g):
    for I, D in ((0, 1), (1, 0), (1.5, 2), (2, "3"), (-1, 2), (np.int64(2), 3)):
        for cls in (g.rational_resampler_ccf, g.rational_resampler_fff, g.rational_resampler_ccc):
            with pytest.raises(ValueError):
                cls(I, D)
    with pytest.raises(ValueError):
        g.rational_resampler_ccf(3, 2, fractional_bw=0.5)


def test_blks2_gcd_and_defaults(g, monkeypatch):
    made = []

    class Fake(object):
        def __init__(self, I, D, taps, device=0):
            made.append((I, D, np.asarray(taps)))

    monkeypatch.setattr(g.binding.rational_resampler_ccf, "_base", Fake)
    g.rational_resampler_ccf(6, 4)
    assert made[-1][0] == 3 and made[-1][1] == 2
    assert np.array_equal(made[-1][2], g.design_filter(3, 2, 0.4))        # default fractional_bw 0.4
    assert len(made[-1][2]) == 301                                          # nt = 101 per filter
    g.rational_resampler_ccf(320, 294, fractional_bw=0.25)
    assert made[-1][0] == 160 and made[-1][1] == 147
    assert np.array_equal(made[-1][2], g.design_filter(160, 147, 0.25))
    taps = np.arange(5, dtype=np.float32)
    g.rational_resampler_ccf(2, 3, taps=taps, fractional_bw=0.3)           # both: the taps win
    assert np.array_equal(made[-1][2], taps)


# ---- the product without a GPU ----

def _lib(g):
    return g.lib()


@pytest.mark.parametrize("kind", ["ccf", "fff", "ccc"])
def test_create_refusals_before_any_device(g, kind):
    L = _lib(g)
    h = C.c_void_p(0)
    taps = np.ones(8, np.complex64 if kind == "ccc" else np.float32)
    rs = L.grhip_rational_resampler_base_create
    ip = L.grhip_interp_fir_filter_create
    assert rs(C.byref(h), kind.encode(), 0, 2, taps.ctypes.data, 8, 0) == -2
    assert rs(C.byref(h), kind.encode(), 3, 0, taps.ctypes.data, 8, 0) == -2
    assert ip(C.byref(h), kind.encode(), 0, taps.ctypes.data, 8, 0) == -2
    assert rs(C.byref(h), kind.encode(), 3, 2, taps.ctypes.data, 0, 0) == -1
    assert ip(C.byref(h), kind.encode(), 3, taps.ctypes.data, 0, 0) == -1
    assert rs(C.byref(h), b"cfc", 3, 2, taps.ctypes.data, 8, 0) == -1
    # a period of 64 outputs that spans more input than the LDS holds
    assert rs(C.byref(h), kind.encode(), 1, 1000, taps.ctypes.data, 8, 0) == -1
    assert not h.value
