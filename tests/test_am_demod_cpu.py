"""CPU tests of complex_to_mag and am_demod_cf: the restatement of the AM chain in optfir_ref.py (the double-sqrt
magnitude in numpy -> a float add of -1 -> the oracle's generic-order fir_fff from a zero delay line) pinned on
magnitudes recorded from the reference's own arithmetic, and the new entries' presence and argument checks, which need
no device.

tests/golden/ref_complex_to_mag.npz was recorded by a throw-away program: std::abs(std::complex<float>) of libstdc++
(glibc 2.35's hypotf), g++ -O2, over 4096 pairs drawn with default_rng(20261019) -- `pairs` ([4096][2] float bit
patterns, re and im) and `mag` (the results' bit patterns): 2600 normals with mantissas on [1, 10) and exponents over
+-30 decades, the eight zero and signed-zero combinations with and without a finite partner, 400 pairs of denormals,
200 of a denormal with a value near 1e-38, 300 axis-aligned values from 1e-44 to 1e38, 300 pairs whose squares
overflow a float, the 64 combinations of (inf, -inf, nan, 0, 1, -2.5, 3e38, 1e-45) and standard normals for the rest."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import optfir_ref as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = np.load(os.path.join(HERE, "golden", "ref_complex_to_mag.npz"))
AM_OPS = ("create", "destroy", "set_mode", "set_streams", "produced", "engine", "tile", "outputs_per_lane", "max_taps",
          "work", "work_device")
MAG_OPS = ("create", "destroy", "set_mode", "set_streams", "work", "work_device")


def fixture_pairs():
    return np.ascontiguousarray(FIX["pairs"]).view(np.float32).reshape(-1, 2).copy().view(np.complex64).reshape(-1)


def same_or_both_nan(got, want_bits):
    want = np.ascontiguousarray(want_bits).view(np.float32)
    return bool(np.all((O.bits32(got) == want_bits) | (np.isnan(got) & np.isnan(want))))


def test_the_magnitude_restatement_equals_the_recorded_std_abs():
    x = fixture_pairs()
    assert len(x) == 4096
    got = O.mag(x)
    assert same_or_both_nan(got, FIX["mag"])
    want = FIX["mag"].view(np.float32)
    # the fixture does hold its edge cases
    assert np.isinf(want).sum() >= 28 and np.isnan(want).sum() == 11 and (want == 0).sum() >= 4
    sub = np.abs(x.real) < 1.1754944e-38
    assert (sub & (np.abs(x.imag) < 1.1754944e-38) & (want > 0)).sum() >= 400
    big = (np.abs(x.real.astype(np.float64)) > 1.9e19) & np.isfinite(want)
    assert big.sum() >= 100
    # an infinite part wins over a NaN
    both = (np.isinf(x.real) & np.isnan(x.imag)) | (np.isnan(x.real) & np.isinf(x.imag))
    assert both.sum() == 4 and np.all(np.isposinf(want[both]))


def test_the_am_chain_restatement_starts_from_a_zero_delay_line(po):
    x = fixture_pairs()[:2600]                         # the finite part of the recorded set
    v = O.am_v(x)
    m = FIX["mag"].view(np.float32)[:2600]
    assert O.bits32(v).tolist() == O.bits32(m + np.float32(-1.0)).tolist()
    taps = O.audio_taps(37)
    for D in (1, 2, 5):
        out = O.am_fir(po, v, D, taps)
        assert len(out) == O.am_outputs(len(v), D)
        # output 0 sees v[0] alone: the delay line holds zeros, not |0| - 1 = -1
        assert O.bits32(out[:1]).tolist() == O.bits32(np.float32(taps[0]) * v[:1]).tolist()
        ref = O.am_fir64(v, D, taps)
        fin = np.isfinite(ref)
        peak = np.max(np.abs(ref[fin]))
        assert np.max(np.abs(out[fin].astype(np.float64) - ref[fin])) <= 1e-5 * peak


def test_signal_has_the_stretches_the_gpu_tests_rely_on():
    x = O.am_signal(3, 8192)
    a = np.abs(x)
    assert a.max() > 25 and (a == 0).sum() >= 512 and ((a > 0) & (a < 2e-3)).sum() >= 1000
    assert abs(float(np.median(a[:2048])) - 1.0) < 0.3


def test_entries_are_declared_exported_and_check_their_arguments(g):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    lib = g.lib()
    assert set(re.findall(r"\bgrhip_am_demod_cf_([a-z0-9_]+)\s*\(", hdr)) == set(AM_OPS)
    assert set(re.findall(r"\bgrhip_complex_to_mag_([a-z0-9_]+)\s*\(", hdr)) - {"squared_" + op for op in MAG_OPS} == set(MAG_OPS)
    for op in AM_OPS:
        getattr(lib, "grhip_am_demod_cf_" + op)
    for op in MAG_OPS:
        getattr(lib, "grhip_complex_to_mag_" + op)
    for name in ("complex_to_mag", "am_demod_cf", "demod_10k0a3e_cf", "demod_20k0f3e_cf", "demod_200kf3e_cf"):
        assert name in g.__all__
    assert g.am_demod_cf.tile() == 4096 and g.am_demod_cf.outputs_per_lane() == 8 and g.am_demod_cf.max_taps() == 1025
    assert g.am_demod_cf.tile() % (256 * g.am_demod_cf.outputs_per_lane()) == 0
    # null handles
    null, buf = C.c_void_p(0), np.zeros(16, np.float32)
    for op, args in (("set_mode", (0,)), ("set_streams", (1,)), ("produced", (4,)), ("engine", ()),
                     ("work", (4, buf.ctypes.data, buf.ctypes.data, None)),
                     ("work_device", (4, buf.ctypes.data, buf.ctypes.data, None, None))):
        assert getattr(lib, "grhip_am_demod_cf_" + op)(null, *args) == -1, op
    for op, args in (("set_mode", (0,)), ("set_streams", (1,)), ("work", (4, buf.ctypes.data, buf.ctypes.data)),
                     ("work_device", (4, buf.ctypes.data, buf.ctypes.data, None))):
        assert getattr(lib, "grhip_complex_to_mag_" + op)(null, *args) == -1, op
    lib.grhip_am_demod_cf_destroy(null)
    lib.grhip_complex_to_mag_destroy(null)
    # bad arguments, refused before any device is touched
    h, taps = C.c_void_p(0), np.ones(4, np.float32)
    create = lib.grhip_am_demod_cf_create
    assert create(None, 1, taps.ctypes.data, 4, 0) == -1
    for decim, tp, n in ((0, taps.ctypes.data, 4), (-3, taps.ctypes.data, 4), (65537, taps.ctypes.data, 4),
                         (1, None, 4), (1, taps.ctypes.data, 0), (1, taps.ctypes.data, 65537)):
        assert create(C.byref(h), decim, tp, n, 0) == -1 and not h.value, (decim, n)
    assert lib.grhip_complex_to_mag_create(None, 1, 0) == -1
    assert lib.grhip_complex_to_mag_create(C.byref(h), 0, 0) == -1 and not h.value
    with pytest.raises(ValueError):
        g.am_demod_cf.from_taps(1.5, taps)
