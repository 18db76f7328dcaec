"""CPU tests of the constellation objects, constellation_receiver_cb, constellation_decoder_cb, diff_decoder_bb, map_bb and
the tail of constellation_demod_cb: the restatement (constellation_ref.py) and the library's host entries
(grhip_constellation_*, which need no device) against what the reference's own code gave
(tests/golden/ref_constellation.npz), the receiver's deviation contract and decision guard, and the new entries'
presence and argument checks.

The fixture was recorded once by a throw-away program compiled from the reference's own files -- gr-digital/lib/
digital_constellation.cc, digital_constellation_receiver_cb.cc, digital_constellation_decoder_cb.cc, general/
gri_control_loop.cc, gr_diff_decoder_bb.cc, gr_map_bb.cc, gr_unpack_k_bits_bb.cc, gr_expj.h and filter/gr_sincos.c
(with HAVE_SINCOSF, as a Linux build has it: glibc's sincosf), unchanged, with g++ -O2 (gcc for the C file) -- against
stub headers for gr_block, gr_sync_block, gr_sync_interpolator, gr_io_signature, gr_types, gr_complex, gr_prefs,
gr_core_api.h, digital_api.h, gruel/attributes.h and boost/enable_shared_from_this.hpp (std::shared_ptr).  It built
every constellation through the reference's factories from the points and codes that constellation_ref.py builds as
psk.py and qam.py do, ran the receiver as one call and as two calls cut at 4097 and required the two to agree bit for
bit, and ran the decoder block beside decision_maker and required equal symbols.  The file holds, floats as bit patterns:
  * dec_<kind>_: pts, code, info (rotational symmetry, dimensionality, arity, bits per symbol, apply_pre_diff_code), tab
    (the sector table), and dec / err, decision_maker_pe on constellation_ref.decision_samples() (4096 samples: random
    ones, points on the axes, on |re| = |im|, zeros of both signs, denormals, 1e-30 and 1e8 magnitudes, points beside
    the 16-point grid's borders; dec_samples_sha pins them).  Kinds: bpsk, qpsk, dqpsk, 8psk, psk<m>g / psk<m>n (psk of
    m = 2 .. 32 points with and without Gray code; the n ones' dec and err equalled the g ones' bit for bit and are
    not stored twice), rect16 (qam_constellation(16)), calcdist4, calcdist2d (5 symbols of 2 dimensions, 2048 items).
  * rx_<case>_: the receiver on constellation_ref.rx_signal(case) (in_sha pins it; 6037 random symbols, 0.15 rad, 0.01
    rad/sample, noise 0.02, 0.008 for 32 points; loop_bw 2 pi / 100, limits +-0.25; "limit": qpsk with an offset of 0.3
    rad/sample, so frequency_limit acts on 5966 samples): sym and phase whole; err and freq whole for qpsk and rect16
    and as the sections [s, s + 256), s = 0, 1400, 4000, 5781, for the others, which keeps the file below
    ref_carrier.npz's size; diff (gr_diff_decoder_bb(arity) on sym), map_d<differential> (gr_map_bb of the inverted
    pre-diff code, where the constellation applies one), tail_d<differential>g<gray> (the bits of the whole tail, packed).
  * bytes_in and bytes_diff_<modulus>, bytes_map_<tag> (+ _arg), bytes_unpack_<k> (packed): the byte blocks on 4097
    random bytes; moduli that are no power of two and above 256, maps longer than 256 and with entries outside a byte.
  * qa_in, qa_expected_bpsk / _qpsk: qa_constellation_decoder_cb.py's data, which the recorder's decoder block met.

Measured here, restatement against recording: the decisions and tables are equal; the phase errors differ by at most
one float ulp (calcdist2d, a sum of two: 4.8e-7); dev(recording) 1.06 .. 1.40e-6 rad and dev(restatement) 1.06 ..
1.40e-6 over the eight cases (DESIGN.md 4.23 has the table); every case meets the decision guard."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import constellation_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")
FIX = np.load(os.path.join(HERE, "golden", "ref_constellation.npz"))
KINDS = [k for k, _ in R.DEC_KINDS]
_CACHE = {}


def f32(a):
    return np.asarray(a).view(np.float32)


def ulps(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7fffffff), a), np.where(b < 0, -(b & 0x7fffffff), b)
    return int(np.abs(a - b).max())


def samples():
    if "x" not in _CACHE:
        _CACHE["x"] = R.decision_samples()
    return _CACHE["x"]


def recorded(name, what):
    """dec and err of a psk<m>n kind are the psk<m>g one's"""
    if what in ("dec", "err") and re.match(r"psk\d+n$", name):
        name = name[:-1] + "g"
    return FIX["dec_%s_%s" % (name, what)]


def handle(g, r):
    """the library's constellation for a restatement object"""
    if r.kind in ("bpsk", "qpsk", "dqpsk", "8psk"):
        return g.constellation(r.kind)
    if r.kind == "psk":
        return g.constellation_psk(r.points, r.pre_diff_code, r.n_sectors)
    if r.kind == "rect":
        return g.constellation_rect(r.points, r.pre_diff_code, r.rotational_symmetry, r.n_real, r.n_imag, r.w_real, r.w_imag)
    return g.constellation_calcdist(r.points, r.pre_diff_code, r.rotational_symmetry, r.dimensionality)


def err_close(name, mine, want, dim):
    """one float ulp per term (the arctangent here is the rounded double one, the recording's glibc's atan2f); a sum of
    `dim` terms of at most pi each may differ by dim ulps of pi and the sum's own rounding"""
    if dim == 1:
        assert ulps(mine, want) <= 1, name
    else:
        assert np.abs(mine.astype(np.float64) - want).max() <= (dim + 0.5) * 2.0 ** -22, name


def test_inputs_are_the_recorded_ones():
    assert bytes(FIX["dec_samples_sha"]) == bytes.fromhex(R.digest(samples()))
    for case in R.RX_CASES:
        assert bytes(FIX["rx_%s_in_sha" % case[0]]) == bytes.fromhex(R.digest(R.rx_signal(case))), case[0]


@pytest.mark.parametrize("name", KINDS)
def test_restatement_tables_and_decisions_equal_the_recording(name):
    c = dict(R.DEC_KINDS)[name]()
    assert R.bits(c.points.view(np.float32)).tolist() == recorded(name, "pts").tolist()
    assert c.pre_diff_code == recorded(name, "code").tolist()
    assert [c.rotational_symmetry, c.dimensionality, c.arity, c.bits_per_symbol(), int(c.apply_pre_diff_code)] == recorded(name, "info").tolist()
    tab = recorded(name, "tab")
    assert (c.sector_values is None and tab.size == 0) or c.sector_values.tolist() == tab.tolist()
    k, e = c.decision_maker_pe(samples())
    assert k.astype(np.uint8).tolist() == recorded(name, "dec").tolist()
    err_close(name, e, f32(recorded(name, "err")), c.dimensionality)


@pytest.mark.parametrize("name", KINDS)
def test_host_entries_equal_the_recording(g, name):
    """grhip_constellation_* through the library: no device needed"""
    r = dict(R.DEC_KINDS)[name]()
    h = handle(g, r)
    assert R.bits(h.points().view(np.float32)).tolist() == recorded(name, "pts").tolist()
    assert h.pre_diff_code() == recorded(name, "code").tolist()
    assert [h.rotational_symmetry(), h.dimensionality(), h.arity(), h.bits_per_symbol(), int(h.apply_pre_diff_code())] == recorded(name, "info").tolist()
    assert h.sector_values().tolist() == recorded(name, "tab").tolist()
    k, e = h.decision_maker_pe(samples())
    assert k.astype(np.uint8).tolist() == recorded(name, "dec").tolist()
    assert g.constellation.decision_maker(h, samples()).tolist() == k.tolist()
    err_close(name, e, f32(recorded(name, "err")), r.dimensionality)
    # and the restatement to the bit: both use the float-rounded double arctangent
    assert R.bits(e).tolist() == R.bits(r.decision_maker_pe(samples())[1]).tolist()


def test_helpers_build_what_psk_py_and_qam_py_build(g):
    for m in (2, 4, 8, 16, 32):
        for code in ("gray", "none"):
            h, r = g.psk_constellation(m, code), R.psk_constellation(m, code == "gray")
            assert R.bits(h.points().view(np.float32)).tolist() == recorded("psk%d%s" % (m, code[0]), "pts").tolist()
            assert h.pre_diff_code() == r.pre_diff_code == recorded("psk%d%s" % (m, code[0]), "code").tolist()
    h = g.qam_constellation(16, True, "none")
    assert R.bits(h.points().view(np.float32)).tolist() == recorded("rect16", "pts").tolist()
    assert h.sector_values().tolist() == recorded("rect16", "tab").tolist()
    for m, diff, gray in ((4, True, False), (16, False, True), (64, True, True), (64, False, False), (256, True, True)):
        h, r = g.qam_constellation(m, diff, "gray" if gray else "none"), R.qam_constellation(m, diff, gray)
        assert np.array_equal(h.points(), r.points) and np.array_equal(h.sector_values(), r.sector_values)
        assert sorted(set(h.sector_values().tolist())) == list(range(m))
    assert g.gray_code(8) == [0, 1, 3, 2, 6, 7, 5, 4] and g.invert_code([0, 1, 3, 2, 6, 7, 5, 4]) == [0, 1, 3, 2, 7, 6, 4, 5]
    with pytest.raises(ValueError):
        g.psk_constellation(6)
    with pytest.raises(ValueError):
        g.qam_constellation(8)


def test_qa_vectors_of_the_decoder(g):
    x = f32(FIX["qa_in"]).view(np.complex64)
    for name in ("bpsk", "qpsk"):
        want = FIX["qa_expected_" + name].tolist()
        assert R.Constellation(name).decision_maker(x).tolist() == want
        assert g.constellation(name).decision_maker(x).tolist() == want


def test_byte_blocks_equal_the_recording():
    b = FIX["bytes_in"]
    for key in FIX.files:
        if key.startswith("bytes_diff_"):
            assert R.diff_decoder(b, int(key.split("_")[-1])).tolist() == FIX[key].tolist(), key
        elif key.startswith("bytes_map_") and not key.endswith("_arg"):
            assert R.map_bb(b, FIX[key + "_arg"].tolist()).tolist() == FIX[key].tolist(), key
        elif key.startswith("bytes_unpack_"):
            k = int(key.split("_")[-1])
            assert R.unpack_k_bits(b, k).tolist() == np.unpackbits(FIX[key])[:len(b) * k].tolist(), key
    # in two calls, the carry being the last byte of the first
    for m in (3, 256):
        two = np.concatenate([R.diff_decoder(b[:1001], m), R.diff_decoder(b[1001:], m, prev=b[1000])])
        assert two.tolist() == FIX["bytes_diff_%d" % m].tolist()


@pytest.mark.parametrize("case", R.RX_CASES, ids=[c[0] for c in R.RX_CASES])
def test_tail_on_the_recorded_symbols(case):
    c, key = case[1](), "rx_%s_" % case[0]
    sym = FIX[key + "sym"]
    assert R.diff_decoder(sym, c.arity).tolist() == FIX[key + "diff"].tolist()
    k = c.bits_per_symbol()
    for d in (0, 1):
        for gr in (0, 1):
            want = np.unpackbits(FIX[key + "tail_d%dg%d" % (d, gr)])[:R.N * k]
            assert R.demod_tail(c, sym, d, gr).tolist() == want.tolist(), (d, gr)
            if gr and c.apply_pre_diff_code:
                y = FIX[key + "diff"] if d else sym
                assert R.map_bb(y, R.invert_code(c.pre_diff_code)).tolist() == FIX[key + "map_d%d" % d].tolist()
            else:
                assert key + "map_d%d" % d not in FIX.files or c.apply_pre_diff_code


def rx_runs(case):
    """the restatement's walk of one case in float32 (one call, and two cut at 4097) and in float64, computed once"""
    if case[0] not in _CACHE:
        c, x = case[1](), R.rx_signal(case)
        one = R.receiver(R.rx_loop(), c, x)
        loop = R.rx_loop()
        a, b = R.receiver(loop, c, x[:R.CUT]), R.receiver(loop, c, x[R.CUT:])
        r64 = R.receiver64(R.rx_loop(), c, x)
        _CACHE[case[0]] = (c, x, one, (a, b), r64)
    return _CACHE[case[0]]


@pytest.mark.parametrize("case", R.RX_CASES, ids=[c[0] for c in R.RX_CASES])
def test_receiver_stays_as_close_to_float64_as_the_reference(case):
    """dev(restatement) <= 2 dev(recording) + 4 ulp(2 pi), dev the largest circular phase difference from the float64
    recurrence on the same input; the decision guard; and with it the recording's symbols."""
    c, x, one, (a, b), r64 = rx_runs(case)
    key = "rx_%s_" % case[0]
    ref = f32(FIX[key + "phase"])
    dev_ref, dev = R.circ(ref, r64.phase), R.circ(one.phase, r64.phase)
    print("%s: dev(recording) %.3g dev(restatement) %.3g bound %.3g" % (case[0], dev_ref, dev, R.bound(dev_ref)))
    assert dev <= R.bound(dev_ref), (case[0], dev, dev_ref)
    assert R.guard(c, r64.derot), case[0]
    sym = FIX[key + "sym"]
    assert one.sym.tolist() == sym.tolist() and r64.sym.tolist() == sym.tolist()
    # two calls are one call
    for f in ("sym", "err", "phase", "freq"):
        assert np.concatenate([getattr(a, f), getattr(b, f)]).tobytes() == getattr(one, f).tobytes(), f
    # error and frequency within the 1e-5 that costas_loop_cc's float outputs are held to
    if case[0] in R.RX_FULL:
        e, fr = f32(FIX[key + "err"]), f32(FIX[key + "freq"])
        assert np.abs(one.err - e).max() <= 1e-5 and np.abs(one.freq - fr).max() <= 1e-5
    else:
        assert np.abs(R.secs(one.err) - f32(FIX[key + "err_sec"])).max() <= 1e-5
        assert np.abs(R.secs(one.freq) - f32(FIX[key + "freq_sec"])).max() <= 1e-5
    if case[0] == "limit":
        assert int(np.count_nonzero(ref == 0)) == 0 and np.count_nonzero(one.freq == np.float32(R.FMAX)) > 5000


def test_constellation_test_builds_and_passes():
    r = subprocess.run(["make", "-C", HOST, "constellation_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([os.path.join(HOST, "constellation_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "constellation_test ok" in r.stdout, r.stdout


LOOP_OPS = ("create", "destroy", "set_mode", "set_streams", "form", "set_loop_bandwidth", "set_damping_factor", "set_alpha",
            "set_beta", "set_frequency", "set_phase", "get_loop_bandwidth", "get_damping_factor", "get_alpha", "get_beta",
            "get_frequency", "get_phase", "work", "work_device")
BYTE_OPS = ("create", "destroy", "set_mode", "set_streams", "work", "work_device")
CONST_OPS = ("create_bpsk", "create_qpsk", "create_dqpsk", "create_8psk", "create_calcdist", "create_psk", "create_rect", "destroy",
             "arity", "dimensionality", "rotational_symmetry", "bits_per_symbol", "apply_pre_diff_code", "n_sectors", "points",
             "pre_diff_code", "sector_values", "decision_maker", "decision_maker_pe")
ENTRIES = ([("constellation_receiver_cb", op) for op in LOOP_OPS]
           + [("constellation_demod_cb", op) for op in LOOP_OPS + ("set_engine", "engine", "bits_per_symbol")]
           + [(b, op) for b in ("constellation_decoder_cb", "diff_decoder_bb", "map_bb") for op in BYTE_OPS])


def test_new_entries_are_declared_and_exported(g):
    sig = g.binding.signatures()
    lib = g.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", g.binding.lib_path()], stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r"\bT (grhip_\w+)", nm))
    names = ["grhip_constellation_" + op for op in CONST_OPS] + ["grhip_%s_%s" % e for e in ENTRIES]
    for n in names:
        assert n in sig and hasattr(lib, n) and n in exported, n
    for cls in ("constellation", "constellation_bpsk", "constellation_qpsk", "constellation_dqpsk", "constellation_8psk",
                "constellation_calcdist", "constellation_psk", "constellation_rect", "psk_constellation", "qam_constellation",
                "constellation_decoder_cb", "diff_decoder_bb", "map_bb", "constellation_receiver_cb", "constellation_demod_cb"):
        assert hasattr(g, cls) and cls in g.__all__, cls
    assert sig["grhip_constellation_decision_maker"][1] == [C.c_void_p, C.c_void_p, C.c_void_p]
    assert sig["grhip_constellation_receiver_cb_create"][1] == [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int]
    assert sig["grhip_constellation_receiver_cb_work_device"][1] == [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    assert sig["grhip_diff_decoder_bb_create"][1] == [C.c_void_p, C.c_uint, C.c_int]
    assert sig["grhip_constellation_demod_cb_get_beta"][0] is C.c_float


def test_refusals_come_before_the_device(g):
    """refused with GRHIP_EINVAL whether or not a device is there"""
    sq = [1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j]
    two_d = g.constellation_calcdist([1, 1, -1, -1], [], 1, 2)
    qpsk = g.constellation_qpsk()
    bad = [lambda: g.constellation_calcdist(np.ones(257), [], 1, 1),                       # arity 257
           lambda: g.constellation_calcdist(sq, [0, 1, 2], 4, 1),                          # the code's length
           lambda: g.constellation_calcdist(sq[:3], [], 4, 2),                             # no multiple of the dimensionality
           lambda: g.constellation_calcdist(sq, [], 4, 0),
           lambda: g.constellation_psk(sq, [], 0), lambda: g.constellation_psk(sq, [], 16385),
           lambda: g.constellation_rect(sq, [], 4, 129, 128, 1.0, 1.0), lambda: g.constellation_rect(sq, [], 4, 2, 2, 0.0, 1.0),
           lambda: g.constellation_rect(sq, [], 4, 2, 2, 1.0, float("nan")),
           lambda: g.constellation_receiver_cb(two_d, 0.0628, -0.25, 0.25),                # dimensionality 2 at the receiver
           lambda: g.constellation_demod_cb(two_d, 0.0628, -0.25, 0.25),
           lambda: g.constellation_demod_cb(g.constellation_calcdist([1], [], 1, 1), 0.0628, -0.25, 0.25),     # no bits
           lambda: g.constellation_receiver_cb(qpsk, -0.1, -0.25, 0.25), lambda: g.constellation_receiver_cb(qpsk, 0.0628, -0.25, 1025.0),
           lambda: g.constellation_receiver_cb(qpsk, 0.0628, float("nan"), 0.25),
           lambda: g.diff_decoder_bb(0)]
    for make in bad:
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1, str(e.value)
    assert g.constellation_calcdist(np.ones(256), [], 1, 1).arity() == 256
    assert g.constellation_psk(sq, [], 16384).sector_values().size == 16384
    lib = g.lib()
    for name in ("constellation_receiver_cb", "constellation_demod_cb"):
        for op, args in (("set_mode", (None, 0)), ("set_streams", (None, 1)), ("form", (None,)), ("set_alpha", (None, C.c_float(1))),
                         ("set_phase", (None, C.c_float(1))), ("get_phase", (None, 0, None))):
            assert getattr(lib, "grhip_%s_%s" % (name, op))(*args) == -1, (name, op)
        assert getattr(lib, "grhip_%s_get_alpha" % name)(None) == -1.0
    assert lib.grhip_constellation_receiver_cb_work(None, 0, None, None, None, None, None) == -1
    assert lib.grhip_constellation_receiver_cb_create(None, qpsk._h, 0.06, -0.25, 0.25, 0) == -1
    pp = C.c_void_p(0)
    assert lib.grhip_constellation_receiver_cb_create(C.byref(pp), None, 0.06, -0.25, 0.25, 0) == -1
    assert lib.grhip_constellation_decoder_cb_create(C.byref(pp), None, 0) == -1
    assert lib.grhip_constellation_arity(None) == -1 and lib.grhip_constellation_decision_maker(None, None, None) == -1
    assert lib.grhip_constellation_decision_maker(qpsk._h, None, None) == -1
    assert lib.grhip_constellation_create_psk(C.byref(pp), None, 4, None, 0, 4) == -1


def test_non_finite_samples_get_a_defined_decision(g):
    v = np.array([np.nan, np.inf, -np.inf, 0.0, 1e38, -1e38, 1.0], np.float32)
    x = np.zeros((len(v), len(v)), np.complex64)
    x.real, x.imag = v[:, None], v[None, :]
    x = x.reshape(-1)
    for name, make in R.DEC_KINDS:
        r = make()
        h = handle(g, r)
        xs = x[:len(x) // r.dimensionality * r.dimensionality]
        k = h.decision_maker(xs)
        assert k.max() < r.arity, name
        if r.kind != "calcdist":        # the restatement's clamps are the same ones; norms overflow differently in numpy
            with np.errstate(all="ignore"):
                assert k.tolist() == r.decision_maker(xs).tolist(), name


def test_new_entries_refuse_to_run_without_a_device(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    q = g.constellation_qpsk()
    for make in (lambda: g.constellation_receiver_cb(q, 0.0628, -0.25, 0.25), lambda: g.constellation_demod_cb(q, 0.0628, -0.25, 0.25),
                 lambda: g.constellation_decoder_cb(q), lambda: g.diff_decoder_bb(4), lambda: g.map_bb([1, 0])):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
