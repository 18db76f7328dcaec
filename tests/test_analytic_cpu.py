"""CPU tests of the real -> complex blocks: the product's firdes_hilbert (host arithmetic, no device) and the numpy
restatements of tests/analytic_ref.py against data recorded from the reference's own compiled code
(tests/golden/ref_hilbert_taps.npz, ref_goertzel.npz), the reference's QA vectors (ref_qa_analytic.json) within the QA
files' own tolerances, and the refusals of the new entries without a device."""
import json
import math
import os

import numpy as np
import pytest

import analytic_ref as ar

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
NTAPS = (3, 5, 7, 19, 51, 255, 1023)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def taps_fx():
    return np.load(os.path.join(HERE, "golden", "ref_hilbert_taps.npz"))


@pytest.fixture(scope="module")
def goertzel_fx():
    return np.load(os.path.join(HERE, "golden", "ref_goertzel.npz"))


@pytest.fixture(scope="module")
def qa():
    return json.load(open(os.path.join(HERE, "golden", "ref_qa_analytic.json")))


def test_fixture_holds_every_length_and_window(taps_fx):
    assert list(taps_fx["ntaps"]) == list(NTAPS) and list(taps_fx["windows"]) == list(ar.WINDOWS)
    for n in NTAPS:
        for w in ar.WINDOWS:
            assert len(taps_fx["taps_%d_w%d" % (n, w)]) == n


def test_product_firdes_hilbert_equals_reference_bits(g, taps_fx):
    for n in NTAPS:
        for w in ar.WINDOWS:
            got = g.firdes_hilbert(n, w, 6.76)
            assert got.dtype == f32 and np.array_equal(_bits(got), _bits(taps_fx["taps_%d_w%d" % (n, w)])), (n, w)
        assert np.array_equal(_bits(g.firdes_hilbert(n)), _bits(taps_fx["taps_%d_w%d" % (n, ar.WIN_RECTANGULAR)]))


def test_product_rectangular_is_hamming(g):
    assert (g.WIN_HAMMING, g.WIN_HANN, g.WIN_BLACKMAN, g.WIN_RECTANGULAR, g.WIN_KAISER, g.WIN_BLACKMAN_hARRIS) == ar.WINDOWS
    for n in NTAPS + (63, 101):
        assert np.array_equal(_bits(g.firdes_hilbert(n, g.WIN_RECTANGULAR)), _bits(g.firdes_hilbert(n, g.WIN_HAMMING)))
    assert not np.array_equal(g.firdes_hilbert(51, g.WIN_HANN), g.firdes_hilbert(51, g.WIN_HAMMING))


def test_product_firdes_hilbert_refusals(g):
    for n in (0, 2, 50, 1024):
        with pytest.raises(g.GrhipError) as e:
            g.firdes_hilbert(n)
        assert e.value.code == -2, n       # GRHIP_ERANGE: the reference throws std::out_of_range
    with pytest.raises(g.GrhipError) as e:
        g.firdes_hilbert(51, 6)
    assert e.value.code == -2


def test_restated_taps_equal_reference_bits(taps_fx):
    for n in NTAPS:
        for w in ar.WINDOWS:
            assert np.array_equal(_bits(ar.firdes_hilbert(n, w)), _bits(taps_fx["taps_%d_w%d" % (n, w)])), (n, w)
    with pytest.raises(ValueError):
        ar.firdes_hilbert(50)


def test_reference_taps_have_the_hilbert_structure(taps_fx):
    """what the sparse kernel relies on is a property of these floats, not of the construction: look at it"""
    for n in NTAPS:
        t = taps_fx["taps_%d_w%d" % (n, ar.WIN_RECTANGULAR)]
        h = n // 2
        assert not t[h::2].any() and not t[h::-2].any()
        i = np.arange(1, h + 1, 2)
        assert np.array_equal(t[h + i], -t[h - i])


def test_restated_goertzel_equals_reference_bits(goertzel_fx):
    d = goertzel_fx
    assert len(d["rate"]) == 5
    for k, (rate, ln, fr, nb) in enumerate(zip(d["rate"], d["len"], d["freq"], d["nblocks"])):
        got = ar.goertzel_fc(int(rate), int(ln), f32(fr), d["x_%d" % k])
        assert len(got) == nb and np.array_equal(_bits(got), _bits(d["out_%d" % k])), k


def test_reference_goertzel_loses_accuracy_at_low_frequency(goertzel_fx):
    """the float recurrence against the same recurrence in float64 with the same float coefficients"""
    d = goertzel_fx
    err = {}
    for k, (rate, ln, fr) in enumerate(zip(d["rate"], d["len"], d["freq"])):
        x = d["x_%d" % k]
        err[(int(rate), int(ln), float(fr))] = float(np.abs(d["out_%d" % k] - ar.goertzel64(int(rate), int(ln), f32(fr), x)).max())
    assert err[(8000, 64, 1000.0)] < 1e-6 and err[(8000, 2000, 5.0)] > 2e-5, err


def _qa_signal(qa, cos=False):
    s = qa["signal"]
    n = np.arange(s["n_input"])
    ph = 2 * math.pi * s["frequency"] / s["sampling_freq"] * n
    return (s["amplitude"] * (np.cos(ph) if cos else np.sin(ph))).astype(f32)


def _qa_close(got, want, places):
    want = np.array([complex(a, b) for a, b in want])
    return len(got) == len(want) and all(round(abs(a - b), places) == 0 for a, b in zip(got, want))


def test_restatements_reproduce_the_reference_qa_vectors(po, qa):
    nt = qa["signal"]["ntaps"]
    sin, cos = _qa_signal(qa), _qa_signal(qa, cos=True)
    hist = np.zeros(nt - 1, dtype=f32)
    xs, xc = np.concatenate([hist, sin]), np.concatenate([hist, cos])
    n = len(sin)
    assert _qa_close(ar.hilbert_fc(po, nt, n, xs), qa["hilbert"], qa["places"])
    assert abs(complex(*qa["hilbert"][nt // 2]).imag + 0.50004) < 1e-5          # the Hamming window in effect
    taps = ar.firdes_hilbert(nt)
    assert _qa_close(ar.filter_delay_fc(po, taps, n, xs), qa["filter_delay_fc_001_one_input"], qa["places"])
    assert _qa_close(ar.filter_delay_fc(po, taps, n, xs, xs), qa["filter_delay_fc_002_same_two_inputs"], qa["places"])
    assert _qa_close(ar.filter_delay_fc(po, taps, n, xs, xc), qa["filter_delay_fc_003_sin_cos"], qa["places"])


def test_restated_goertzel_reproduces_the_reference_qa_magnitudes(qa):
    q = qa["goertzel"]
    rate = q["rate"]
    x = np.array([math.cos(2 * math.pi * i * q["tone"] / rate) for i in range(rate)], dtype=f32)
    for c in q["cases"]:
        out = ar.goertzel_fc(rate, q["len"], c["bin"], x)
        assert len(out) == 1 and round(abs(abs(out[0]) - c["magnitude"]), q["places"]) == 0, c


@pytest.mark.parametrize("make", [lambda g: g.hilbert_fc(51), lambda g: g.filter_delay_fc([0.5, 0.25]),
                                  lambda g: g.goertzel_fc(8000, 400, 100.0)], ids=["hilbert", "filter_delay", "goertzel"])
def test_no_cpu_fallback(g, make):
    g.lib()
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(g.GrhipError) as e:
        make(g)
    assert e.value.code == -5      # GRHIP_ENODEV
    assert "no CPU fallback" in str(e.value)


def test_bad_arguments_refused_before_the_device(g):
    for make in (lambda: g.hilbert_fc(0), lambda: g.hilbert_fc(1), lambda: g.filter_delay_fc([]),
                 lambda: g.goertzel_fc(8000, 0, 100.0), lambda: g.goertzel_fc(0, 64, 100.0)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1  # GRHIP_EINVAL, with or without a GPU
