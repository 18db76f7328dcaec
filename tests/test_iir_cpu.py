"""CPU tests of iir_filter_ffd and the host-only tap designers: the restatement (iir_ref.py) against outputs recorded
from the reference's own code (tests/golden/ref_iir.npz), the QA vectors of gr/qa_iir.py, grhip_fm_deemph_taps and
grhip_firdes_low_pass against the recorded taps bit for bit, the chunked form in Python within the bound that
include/grhip.h states, and the new entries' presence and argument checks, which need no device.

Test signal (iir_ref.signal(1)): n = 6037, standard_normal * 0.7 * env from default_rng(1) as float32, env = 1 on
[0, 1500), 0 on [1500, 2500), 30 on [2500, 4000) and 0.02 from 4000 on.  Tap sets: iir_ref.TAP_SETS (the de-emphasis
of blks2.fm_deemph at 32 kHz and 320 kHz, a biquad, a 4th-order set, n = 1 with m = 3, n = 5 with m = 2), the
unstable taps of qa_iir.py test 005 over 64 samples, and a set_taps from the biquad to the 32 kHz de-emphasis at
sample 4097.

The fixture was recorded by a throw-away program from the reference's filter/gri_iir.h, compiled unchanged with
g++ -O2 (-std=gnu++14 for its exception specifications) against a one-line stub gr_core_api.h (an empty GR_CORE_API):
gri_iir<float, float, double>, the instance behind gr_iir_filter_ffd, run through filter_n and set_taps.  It holds
  * per tap set and cut (`one` call, or `two` calls cut at 4097), under the key <set>_<cut>_: sha (SHA-256 over the
    output's bytes), head (the first 64 outputs' bits), mid (64 outputs from sample 2490 on) and tail (the last 64);
    the same under latch_ for the set_taps run; the taps themselves as bit patterns (taps_<set>_ff / _fb: the
    de-emphasis taps come from fm_emph.py's own lines run in Python);
  * unstable_out, the 64 outputs of test 005's taps, as bit patterns;
  * qa_out_001 .. 008, the outputs of the eight qa_iir.py cases (their set_taps calls included);
  * nbfm_taps_16000_32000 and nbfm_taps_8000_64000: gr_firdes::low_pass(1.0, quad_rate, 2.7e3, 0.5e3, WIN_HAMMING),
    the taps blks2.nbfm_rx builds, from general/gr_firdes.cc compiled unchanged against stub config.h, gr_core_api.h
    and gr_complex.h (two typedefs of std::complex).
tests/golden/ref_qa_iir.json holds the source data, tap sequences and expected_result tuples of qa_iir.py."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import iir_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = np.load(os.path.join(HERE, "golden", "ref_iir.npz"))
QA = json.load(open(os.path.join(HERE, "golden", "ref_qa_iir.json")))


def _pinned(key, out):
    assert R.bits(out[:64]).tolist() == FIX[key + "head"].tolist(), key
    assert R.bits(out[2490:2490 + 64]).tolist() == FIX[key + "mid"].tolist(), key
    assert R.bits(out[-64:]).tolist() == FIX[key + "tail"].tolist(), key
    assert R.digest(out) == bytes(FIX[key + "sha"]).hex(), key


def test_signal_and_taps_are_the_recorded_ones():
    x = R.signal(1)
    assert len(x) == R.N == 6037 and R.digest(x) == bytes(FIX["signal_sha"]).hex()
    for name, (ff, fb) in R.TAP_SETS.items():
        assert R.bits(np.array(ff, np.float64)).tolist() == FIX["taps_%s_ff" % name].tolist(), name
        assert R.bits(np.array(fb, np.float64)).tolist() == FIX["taps_%s_fb" % name].tolist(), name


@pytest.mark.parametrize("name", R.STABLE)
def test_restatement_equals_the_reference_bit_for_bit(name):
    ff, fb = R.TAP_SETS[name]
    x = R.signal(1)
    for tag, cuts in (("one", ()), ("two", (4097,))):
        out, _ = R.in_calls(R.serial, x, ff, fb, cuts)
        _pinned("%s_%s_" % (name, tag), out)


def test_unstable_taps_and_latched_set_taps():
    x = R.signal(1)
    out, _, _ = R.serial(x[:R.UNSTABLE_N], *R.UNSTABLE)
    assert R.bits(out).tolist() == FIX["unstable_out"].tolist()
    assert np.isfinite(out).all() and np.abs(out).max() > 1e20         # it does grow: roots 1.30 and -2.30
    a, _, _ = R.serial(x[:R.LATCH_AT], *R.TAP_SETS[R.LATCH[0]])
    b, _, _ = R.serial(x[R.LATCH_AT:], *R.TAP_SETS[R.LATCH[1]])        # from zeroed delay lines (gri_iir.h:95-110)
    _pinned("latch_", np.concatenate([a, b]))


@pytest.mark.parametrize("case", sorted(QA))
def test_qa_vectors(case):
    """the recorded outputs equal qa_iir.py's expected tuples, and the restatement equals them bit for bit"""
    q = QA[case]
    x = np.array(q["src"], np.float32)
    got = FIX["qa_out_" + case].view(np.float32)
    assert len(got) == len(q["expected"]) == 8
    for a, b in zip(got, q["expected"]):
        assert round(abs(float(a) - b), 7) == 0                         # assertFloatTuplesAlmostEqual
    ff, fb = q["taps"][-1]                                              # a set_taps before the first item: the last taps, zero state
    out, _, _ = R.serial(x, ff, fb)
    assert R.bits(out).tolist() == FIX["qa_out_" + case].tolist()


@pytest.mark.parametrize("name", R.STABLE)
def test_chunked_form_is_within_the_stated_bound(name):
    """every output of the chunked form within ulp_float(|y|) + 2^-40 peak of the serial walk's"""
    ff, fb = R.TAP_SETS[name]
    x = R.signal(1)
    assert R.can_chunk(ff, fb)
    ref, _, _ = R.serial(x, ff, fb)
    for cuts in ((), (257, 4097)):
        got, _ = R.chunked(x, ff, fb, cuts)
        diff = int(np.count_nonzero(R.bits(got) != R.bits(ref)))
        print("%s cuts %s: %d of %d outputs differ in bits" % (name, cuts, diff, len(ref)))
        assert R.within_fast_bound(got, ref), (name, cuts)


def test_chunked_falls_back_to_the_serial_walk():
    x = R.signal(1)
    ff, fb = R.TAP_SETS["biquad"]
    assert not R.can_chunk(ff, fb, 256) and R.can_chunk(ff, fb, 257)
    assert not R.can_chunk(*R.UNSTABLE) and not R.can_chunk(*R.K9)
    assert not R.can_chunk([float("nan"), 1.0], [0.0, 0.5]) and not R.can_chunk([1.0], [0.0, float("inf")])
    assert R.can_chunk([1.0, 2.0], [0.0])                               # no feedback: nothing to chain
    a, _, _ = R.chunked_call(x[:256], ff, fb)
    b, _, _ = R.serial(x[:256], ff, fb)
    assert R.bits(a).tolist() == R.bits(b).tolist()


# ---- the library's host-only entries ---------------------------------------------------------------------------------
def test_fm_deemph_taps_equal_the_recorded_ones(g):
    for fs, name in ((32e3, "deemph32k"), (320e3, "deemph320k")):
        b, a = g.fm_deemph_taps(fs, 75e-6)
        assert b.dtype == a.dtype == np.float64
        assert R.bits(b).tolist() == FIX["taps_%s_ff" % name].tolist()
        assert R.bits(a).tolist() == FIX["taps_%s_fb" % name].tolist()
        assert a[0] == 1.0 and -1.0 < a[1] < 0.0 and b[0] == b[1]      # the feedback is added: a negative a1
    lib = g.lib()
    two = (C.c_double * 2)()
    assert lib.grhip_fm_deemph_taps(32e3, 75e-6, None, two) == -1
    assert lib.grhip_fm_deemph_taps(32e3, 75e-6, two, None) == -1
    assert lib.grhip_fm_deemph_taps(0.0, 75e-6, two, two) == -1
    assert lib.grhip_fm_deemph_taps(32e3, 0.0, two, two) == -1
    assert lib.grhip_fm_deemph_taps(float("nan"), 75e-6, two, two) == -1


def test_firdes_low_pass_equals_the_reference_bit_for_bit(g):
    for audio, quad, ntaps in ((16000, 32000, 211), (8000, 64000, 423)):
        t = g.firdes_low_pass(1.0, quad, 2.7e3, 0.5e3, g.WIN_HAMMING)
        want = FIX["nbfm_taps_%d_%d" % (audio, quad)]
        assert t.dtype == np.float32 and len(t) == len(want) == ntaps
        assert R.bits(t).tolist() == want.tolist()
        assert R.bits(t).tolist() == R.bits(g.firdes_low_pass(1.0, quad, 2.7e3, 0.5e3)).tolist()   # Hamming by default


def test_firdes_low_pass_argument_checks(g):
    for args in ((1.0, 0.0, 2.7e3, 0.5e3), (1.0, -1.0, 2.7e3, 0.5e3), (1.0, 32e3, 0.0, 0.5e3), (1.0, 32e3, 16001.0, 0.5e3),
                 (1.0, 32e3, 2.7e3, 0.0), (1.0, 32e3, 2.7e3, -5.0), (1.0, float("nan"), 2.7e3, 0.5e3),
                 (1.0, 32e3, 2.7e3, 1e-9)):
        with pytest.raises(g.GrhipError) as e:
            g.firdes_low_pass(*args)
        assert e.value.code == -1, args
    for window in (-1, 5, 6):
        with pytest.raises(g.GrhipError) as e:
            g.firdes_low_pass(1.0, 32e3, 2.7e3, 0.5e3, window)
        assert e.value.code == -1
    assert len(g.firdes_low_pass(1.0, 32e3, 16000.0, 0.5e3)) == 211     # fa == fs / 2 passes, as in the reference
    lib = g.lib()
    n = C.c_size_t(0)
    buf = np.zeros(300, np.float32)
    assert lib.grhip_firdes_low_pass(1.0, 32e3, 2.7e3, 0.5e3, 0, 6.76, None, 0, C.byref(n)) == -2 and n.value == 211
    buf[:] = 7.0
    assert lib.grhip_firdes_low_pass(1.0, 32e3, 2.7e3, 0.5e3, 0, 6.76, buf.ctypes.data, 210, C.byref(n)) == -2
    assert (buf == 7.0).all()                                           # too small: nothing written
    assert lib.grhip_firdes_low_pass(1.0, 32e3, 2.7e3, 0.5e3, 0, 6.76, buf.ctypes.data, 300, C.byref(n)) == 0
    assert n.value == 211 and (buf[211:] == 7.0).all() and abs(float(buf[:211].sum()) - 1.0) < 1e-5
    assert lib.grhip_firdes_low_pass(1.0, 32e3, 2.7e3, 0.5e3, 0, 6.76, buf.ctypes.data, 300, None) == -1


def test_other_windows_keep_the_reference_tap_counts(g):
    # width_factor 3.3 / 3.1 / 5.5 / 2.0 / 10.0 over delta_f = 1 / 64, plus 0.5, truncated, made odd
    for window, n in ((g.WIN_HAMMING, 211), (g.WIN_HANN, 199), (g.WIN_BLACKMAN, 353), (g.WIN_RECTANGULAR, 129),
                      (g.WIN_KAISER, 641)):
        t = g.firdes_low_pass(2.0, 32e3, 4e3, 0.5e3, window)
        assert len(t) == n and np.isfinite(t).all()
        M = (n - 1) // 2                                                # gr_firdes.cc:138-142: this sum is what the gain scales
        assert abs(float(t[M]) + 2.0 * float(t[M + 1:].astype(np.float64).sum()) - 2.0) < 1e-4


OPS = ("create", "destroy", "set_taps", "set_mode", "set_streams", "chunked", "work", "work_device", "chunk")


def test_new_entries_are_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = g.lib()
    names = set(re.findall(r"\b(grhip_iir_filter_ffd_[a-z0-9_]+)\s*\(", hdr))
    assert names == {"grhip_iir_filter_ffd_" + op for op in OPS}
    for n in sorted(names) + ["grhip_fm_deemph_taps", "grhip_firdes_low_pass"]:
        assert hasattr(lib, n), n
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    for name in ("iir_filter_ffd", "fm_deemph", "fm_deemph_taps", "firdes_low_pass"):
        assert hasattr(g, name) and name in g.__all__
    assert g.iir_filter_ffd.chunk() == R.CHUNK == 256


def test_arguments_are_refused_before_the_device(g):
    lib = g.lib()
    h = C.c_void_p(0)
    one = (C.c_double * 1)(1.0)
    many = (C.c_double * 65)(*([0.0] * 65))
    create = lib.grhip_iir_filter_ffd_create
    assert create(None, one, 1, one, 1, 0) == -1
    assert create(C.byref(h), one, 1, one, 0, 0) == -1 and not h.value          # n > 0 with m == 0
    assert "feedback" in lib.grhip_last_error().decode()
    assert create(C.byref(h), many, 65, one, 1, 0) == -1 and not h.value        # more than 64 taps, either side
    assert create(C.byref(h), one, 1, many, 65, 0) == -1 and not h.value
    assert create(C.byref(h), None, 1, one, 1, 0) == -1 and not h.value
    for op, args in (("set_mode", (None, 0)), ("set_streams", (None, 1)), ("set_taps", (None, one, 1, one, 1)),
                     ("chunked", (None,)), ("work", (None, 0, None, None)), ("work_device", (None, 0, None, None, None))):
        assert getattr(lib, "grhip_iir_filter_ffd_" + op)(*args) == -1, op


FM_OPS = ("create", "destroy", "set_mode", "set_streams", "produced", "engine", "tile", "work", "work_device")


def test_fm_demod_entries_are_declared_exported_and_check_their_arguments(g):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = g.lib()
    names = set(re.findall(r"\b(grhip_fm_demod_cf_[a-z0-9_]+)\s*\(", hdr))
    assert names == {"grhip_fm_demod_cf_" + op for op in FM_OPS}
    assert all(hasattr(lib, n) for n in names)
    for name in ("fm_demod_cf", "nbfm_rx"):
        assert hasattr(g, name) and name in g.__all__
    assert g.fm_demod_cf.tile() == 8192
    # 75 us: the warm-up of a tile is 97 samples at 32 kHz and 998 at 320 kHz, both within tile() / 8
    for fs, w0 in ((32e3, 97), (320e3, 998)):
        a1 = R.deemph_taps(fs)[1][1]
        assert int(np.ceil(60 * np.log(2) / -np.log(abs(a1)))) == w0 <= g.fm_demod_cf.tile() // 8
    h = C.c_void_p(0)
    two = (C.c_double * 2)(0.5, 0.5)
    taps = (C.c_float * 3)(0.25, 0.5, 0.25)
    create = lib.grhip_fm_demod_cf_create
    assert create(None, 1.0, two, 2, two, 2, 4, taps, 3, 0) == -1
    assert create(C.byref(h), 1.0, two, 2, None, 0, 4, taps, 3, 0) == -1 and not h.value     # taps on one side only
    assert create(C.byref(h), 1.0, None, 0, two, 2, 4, taps, 3, 0) == -1 and not h.value
    assert create(C.byref(h), 1.0, two, 2, two, 2, 0, taps, 3, 0) == -1 and not h.value      # audio_decim < 1
    assert create(C.byref(h), 1.0, two, 2, two, 2, 4, taps, 0, 0) == -1 and not h.value      # no audio taps
    assert create(C.byref(h), 1.0, two, 2, two, 2, 4, None, 3, 0) == -1 and not h.value
    for op, args in (("set_mode", (None, 0)), ("set_streams", (None, 1)), ("produced", (None, 1)), ("engine", (None,)),
                     ("work", (None, 0, None, None, None)), ("work_device", (None, 0, None, None, None, None))):
        assert getattr(lib, "grhip_fm_demod_cf_" + op)(*args) == -1, op
    with pytest.raises(ValueError):
        g.nbfm_rx(16000, 40000)                                         # nbfm_rx.py:61-62, before any device is touched
    if g.device_count() == 0:
        with pytest.raises(g.GrhipError) as e:
            g.nbfm_rx(16000, 32000)
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)


def test_new_entries_refuse_to_run_without_a_device(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    for make in (lambda: g.iir_filter_ffd([1.0], [0.0]), lambda: g.fm_deemph(32e3), lambda: g.iir_filter_ffd([], [])):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
