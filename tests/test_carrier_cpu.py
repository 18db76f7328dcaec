"""CPU tests of costas_loop_cc, pll_freqdet_cf, pll_refout_cc and pll_carriertracking_cc: the restatement
(carrier_ref.py) against tracks recorded from the reference's own code (tests/golden/ref_carrier.npz), the QA vectors,
the loop-gain arithmetic, the Costas deviation contract, and the new entries' presence and argument checks, which need
no device.

Test signals, n = 6037, seeds 1 .. 3, one call and two calls cut at 4097:
  * carrier_ref.pll_signal(seed, set): a complex tone from a random start phase whose frequency steps at 1500 and at
    4000 (the set's three frequencies), amplitude 1 on [0, 1500), 0 on [1500, 2500), 30 on [2500, 4000) and 0.02 from
    4000 on, noise of 5 % of the amplitude.  PLL_SETS: "limit" (frequency_limit acts on a few per cent of the samples),
    "wrap" (phase_wrap and both branches of mod_2pi), and the two loops of blks2impl/wfm_rcv_pll.py at demod_rate
    256 kHz, audio rate 32 kHz ("wfm_demod": 2 pi / 100 with +-2 pi 90e3 / demod_rate; "wfm_pilot": max_freq
    -2 pi 18990 / rate, min_freq -2 pi 19010 / rate).
  * carrier_ref.costas_signal(seed, set): seeded symbols of the QA's constellations (order 8 at amplitude 2) rotated
    by 0.2 rad plus a frequency offset, small noise.  COSTAS_SETS: one per order, "clip" (amplitude 3, noise 0.2: the detector
    exceeds 1) and "limit" (set_frequency(0.999) in front of an offset of 0.9995: the +-1 limit acts).

The fixture was recorded once by a throw-away program compiled from the reference's own files -- gri_control_loop.cc,
gr_fast_atan2f.cc, gr_sincos.c (with HAVE_SINCOSF, as a Linux build has it: glibc's sincosf), gr_expj.h, gr_math.h,
gr_fxpt.cc and the four blocks' .cc files, unchanged, with g++ -O2 -- against stub headers for gr_sync_block,
gr_io_signature, gr_types, gr_complex, gr_core_api.h and digital_api.h.  It ran every block as one call, as two calls cut
at 4097 and sample by sample (reading get_phase / get_frequency, and d_locksig, after every sample), and required the
three to agree bit for bit.  tests/golden/ref_carrier.npz holds, all as bit patterns:
  * gain_cases / gain_bits: alpha and beta for a dozen (loop_bw, damping);
  * qa_tone: the 100 samples that gr.sig_source_c(10e3, GR_COS_WAVE, 100, 1.0) gives the three PLL QAs, from
    gr_fxpt_nco.h as test_agc_cpu.py explains, and qa_out_<block>; qa_costas_in_/out_test01 .. 05, the QA's data drawn
    from random.Random(20111) since the QA's own is unseeded;
  * pll_<set>_s<seed>_: phase_sha, freq_sha (SHA-256 of the state behind every sample), freqdet_sha, phase_head,
    freq_head, state (final), and the sections [s, s + 256), s = 0, 1400, 2400, 3960, of pll_refout_cc's and
    pll_carriertracking_cc's outputs and of the lock signal (refout_sec, ct_sec, lock_sec), lock_final; for seed 1
    also lock_full, and the squelch run: sq_thr, sq_zero (packed: which outputs were zero), sq_sec;
  * costas_<set>_s<seed>_: state and the same sections of out, phase and freq; for seed 1 phase_full and, for orders 4
    and 8, out_full.
tests/golden/ref_qa_carrier.json holds the expected tuples of qa_pll_freqdet.py, qa_pll_refout.py and
qa_pll_carriertracking.py, and what qa_costas_loop_cc.py test01 .. 05 compare against.

Measured here (restatement against the recording): the lock signal deviates by at most 2^-19 = 1.9e-6 (one ulp at
its peak of 30); Costas, seed 1: dev(reference) 0.8 .. 1.5e-6 rad and dev(restatement) within 1.04 times that; the
restatement leaves the recording's bits within the first 200 samples, as the sincosf finding says."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import carrier_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")
FIX = np.load(os.path.join(HERE, "golden", "ref_carrier.npz"))
QA = json.load(open(os.path.join(HERE, "golden", "ref_qa_carrier.json")))
CUTS = (("one", ()), ("two", (R.CUT,)))
LOCK_DEV = 2.0 ** -19          # the largest |recorded lock signal - restatement| over every case
BLOCKS = ("costas_loop_cc", "pll_freqdet_cf", "pll_refout_cc", "pll_carriertracking_cc")
_CACHE = {}


def sha(a):
    return bytes.fromhex(R.digest(a))


def secs(a):
    return np.concatenate([a[s:s + R.SEC_LEN] for s in R.SECTIONS])


def pll_runs(ps, seed):
    """the restatement's walk of one signal, as one call and as two, computed once"""
    k = (ps[0], seed)
    if k not in _CACHE:
        x = R.pll_signal(seed, ps)
        loops = [R.pll_loop(ps), R.pll_loop(ps)]
        _CACHE[k] = (x, loops, [R.in_calls(R.pll, l, x, cuts) for l, (_, cuts) in zip(loops, CUTS)])
    return _CACHE[k]


def test_gains_bit_for_bit():
    for (bw, damp), want in zip(FIX["gain_cases"], FIX["gain_bits"]):
        a, b = R.gains(bw, damp)
        assert [int(R.bits(np.array([a], np.float32))[0]), int(R.bits(np.array([b], np.float32))[0])] == want.tolist(), (bw, damp)
    assert R.bits(np.array([R.DAMPING0]))[0] == 0x3f3504f3


def test_control_loop_test_builds_and_passes():
    r = subprocess.run(["make", "-C", HOST, "control_loop_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([os.path.join(HOST, "control_loop_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "control_loop_test ok" in r.stdout, r.stdout
    # csrc/control_loop.h's gains against the reference's
    args = [repr(float(np.float32(v))) for c in FIX["gain_cases"] for v in c]
    r = subprocess.run([os.path.join(HOST, "control_loop_test")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = [int(t, 16) for t in r.stdout.split()]
    assert got == FIX["gain_bits"].reshape(-1).tolist(), r.stdout


def test_fast_atan2f_restatement_equals_the_oracle(po):
    rng = np.random.default_rng(5)
    y, x = rng.standard_normal(20000).astype(np.float32), rng.standard_normal(20000).astype(np.float32)
    y[:100] *= 1e-4
    x[100:200] *= 1e-4
    y[200:210] = 0
    x[205:215] = 0
    assert R.bits(R.fast_atan2f(y, x)).tolist() == R.bits(po.fast_atan2f(y, x)).tolist()


@pytest.mark.parametrize("ps", R.PLL_SETS, ids=[p[0] for p in R.PLL_SETS])
def test_pll_state_and_freqdet_bit_for_bit(ps):
    for seed in R.SEEDS:
        key = "pll_%s_s%d_" % (ps[0], seed)
        x, loops, runs = pll_runs(ps, seed)
        assert len(x) == R.N == 6037
        for (tag, _), r in zip(CUTS, runs):
            assert R.bits(r.phases[1:65]).tolist() == FIX[key + "phase_head"].tolist(), (key, tag)
            assert R.bits(r.freqs[1:65]).tolist() == FIX[key + "freq_head"].tolist(), (key, tag)
            assert sha(r.phases[1:]) == bytes(FIX[key + "phase_sha"]), (key, tag)
            assert sha(r.freqs[1:]) == bytes(FIX[key + "freq_sha"]), (key, tag)
            assert sha(r.freqdet) == bytes(FIX[key + "freqdet_sha"]), (key, tag)
            assert R.bits(np.array([r.phases[-1], r.freqs[-1]])).tolist() == FIX[key + "state"].tolist(), (key, tag)


def test_every_path_of_the_pll_walk_fires():
    by = {}
    for ps in R.PLL_SETS:
        for seed in R.SEEDS:
            by[ps[0], seed] = pll_runs(ps, seed)[1][0]
    for seed in R.SEEDS:
        lim = by["limit", seed]
        assert 0.02 <= lim.limits / R.N <= 0.10, (seed, lim.limits)         # a few per cent
        w = by["wrap", seed]
        assert w.wraps > 1000 and w.mod_up > 500 and w.mod_down > 500, (seed, w.wraps, w.mod_up, w.mod_down)
        d = by["wfm_demod", seed]
        assert d.wraps > 100 and d.mod_up > 500 and d.mod_down > 500
        p = by["wfm_pilot", seed]
        assert p.limits > 1000 and p.wraps > 3000 and p.mod_up > 3000      # a band of 20 Hz: the limit is the rule


def ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float32)))


@pytest.mark.parametrize("ps", R.PLL_SETS, ids=[p[0] for p in R.PLL_SETS])
def test_sine_carrying_outputs_and_lock_signal(ps):
    worst = 0.0
    for seed in R.SEEDS:
        key = "pll_%s_s%d_" % (ps[0], seed)
        x, _, runs = pll_runs(ps, seed)
        xs = secs(x)
        mag = (np.abs(xs.real).astype(np.float64) + np.abs(xs.imag).astype(np.float64))
        for (tag, _), r in zip(CUTS, runs):
            want = FIX[key + "refout_sec"].view(np.complex64)
            got = secs(r.refout)
            for g, w in ((got.real, want.real), (got.imag, want.imag)):
                assert np.all(np.abs(g.astype(np.float64) - w) <= ulp(w)), (key, tag)        # one float ulp of the component
            want = FIX[key + "ct_sec"].view(np.complex64)
            got = secs(r.ct)
            tol = 4 * 2.0 ** -24 * mag      # a one-ulp change of sine and cosine, and three roundings
            assert np.all(np.abs(got.real.astype(np.float64) - want.real) <= tol), (key, tag)
            assert np.all(np.abs(got.imag.astype(np.float64) - want.imag) <= tol), (key, tag)
            want = FIX[key + "lock_sec"].view(np.float32)
            dev = float(np.max(np.abs(secs(r.locks[1:]).astype(np.float64) - want)))
            worst = max(worst, dev)
            assert dev <= LOCK_DEV, (key, tag, dev)
            assert abs(float(r.locks[-1]) - float(FIX[key + "lock_final"].view(np.float32)[0])) <= LOCK_DEV
            if seed == 1:
                full = FIX[key + "lock_full"].view(np.float32)
                dev = float(np.max(np.abs(r.locks[1:].astype(np.float64) - full)))
                worst = max(worst, dev)
                assert dev <= LOCK_DEV, (key, tag, dev)
    print("%s: lock signal deviates from the recording by at most %.3g (bound %.3g)" % (ps[0], worst, LOCK_DEV))


@pytest.mark.parametrize("ps", R.PLL_SETS, ids=[p[0] for p in R.PLL_SETS])
def test_squelch_decisions_are_the_references(ps):
    key = "pll_%s_s1_" % ps[0]
    thr = FIX[key + "sq_thr"].view(np.float32)[0]
    full = FIX[key + "lock_full"].view(np.float32)
    # the threshold keeps the recorded track 1000 deviations away from the decision
    margin = float(np.min(np.abs(np.abs(full.astype(np.float64)) - float(thr))))
    assert margin >= 1000 * LOCK_DEV, (margin, thr)
    x = R.pll_signal(1, ps)
    for tag, cuts in CUTS:
        r = R.in_calls(R.pll, R.pll_loop(ps), x, cuts, squelch=True, threshold=thr)
        assert np.array_equal(r.open, np.abs(full) > thr), tag
        zero = np.unpackbits(FIX[key + "sq_zero"])[:R.N].astype(bool)
        assert np.array_equal(r.ct == 0, zero), tag
        assert 100 < np.count_nonzero(r.open) < R.N - 100
        want = FIX[key + "sq_sec"].view(np.complex64)
        xs = secs(x)
        tol = 4 * 2.0 ** -24 * (np.abs(xs.real).astype(np.float64) + np.abs(xs.imag))
        assert np.all(np.abs(secs(r.ct) - want) <= 2 * tol)


SEED1 = [c for c in R.COSTAS_SETS]


@pytest.mark.parametrize("cs", SEED1, ids=[c[0] for c in SEED1])
def test_costas_stays_as_close_to_float64_as_the_reference(cs):
    """dev(restatement) <= 2 dev(reference recording) + 4 ulp(2 pi), dev the largest circular phase difference from the
    float64 recurrence on the same input; and the decision guard on the recorded outputs."""
    key = "costas_%s_s1_" % cs[0]
    x = R.costas_signal(1, cs)
    ref = FIX[key + "phase_full"].view(np.float32)
    r64 = R.costas64(R.costas_loop(cs), x, cs[1])
    dev_ref = R.circ(ref, r64.phases[1:])
    for tag, cuts in CUTS:
        loop = R.costas_loop(cs)
        r = R.in_calls(lambda l, seg: R.costas(l, seg, cs[1]), loop, x, cuts)
        dev = R.circ(r.phases, r64.phases)
        diff = np.flatnonzero(R.bits(r.phases[1:]) != R.bits(ref))
        first = int(diff[0]) if diff.size else -1
        print("%s %s: dev(reference) %.3g dev(restatement) %.3g; leaves the recording's bits at sample %d, largest "
              "difference %.3g rad" % (cs[0], tag, dev_ref, dev, first, R.circ(r.phases[1:], ref)))
        assert dev <= R.bound(dev_ref), (cs[0], tag, dev, dev_ref)
        assert np.abs(r.freq.astype(np.float64) - r64.freq).max() <= 1e-5
        if cs[0] == "clip":
            assert loop.clips > 50
        if cs[0] == "limit":
            assert loop.limits > 500 and loop.wraps > 500
    if cs[1] > 2:
        out = FIX[key + "out_full"].view(np.complex64)
        d = R.boundary_distance(cs[1], out)
        assert d.min() >= 1000 * dev_ref, (cs[0], d.min(), dev_ref)


def test_costas_sections_of_every_seed_follow_the_recording():
    """seeds 2 and 3 keep sections only: the restatement's outputs there are within 1e-5 of the recording's"""
    for cs in R.COSTAS_SETS:
        for seed in (2, 3):
            key = "costas_%s_s%d_" % (cs[0], seed)
            r = R.costas(R.costas_loop(cs), R.costas_signal(seed, cs), cs[1])
            assert np.abs(secs(r.out) - FIX[key + "out_sec"].view(np.complex64)).max() <= 1e-5 * cs[3] * 1.5
            assert R.circ(secs(r.phases[1:]), FIX[key + "phase_sec"].view(np.float32)) <= 1e-5
            assert np.abs(secs(r.freq) - FIX[key + "freq_sec"].view(np.float32)).max() <= 1e-5


def _places(a, b, places):
    return all(round(abs(complex(u) - complex(v)), places) == 0 for u, v in zip(a, b))


def test_qa_vectors_of_the_plls():
    """the recorded outputs equal the QAs' expected tuples to the QAs' places, and the restatement the recording"""
    tone = FIX["qa_tone"].view(np.complex64)
    assert len(tone) == 100
    r = R.pll(R.Loop(np.pi / 100.0, 1, -1), tone)
    got = FIX["qa_out_pll_freqdet_cf"].view(np.float32)
    exp = np.array(QA["pll_freqdet_cf"])
    assert len(got) == len(exp) == 100
    assert _places(got.astype(np.float64) * (10e3 / (2 * np.pi)), exp, 3)          # assertFloatTuplesAlmostEqual(..., 3)
    assert R.bits(r.freqdet).tolist() == FIX["qa_out_pll_freqdet_cf"].tolist()
    for name, places, mine in (("pll_refout_cc", 4, r.refout), ("pll_carriertracking_cc", 5, r.ct)):
        got = FIX["qa_out_" + name].view(np.complex64)
        e = np.array(QA[name])
        exp = e[:, 0] + 1j * e[:, 1]
        assert len(got) == len(exp) == 100
        assert _places(got, exp, places), name
        assert _places(mine, exp, places), name
        assert np.abs(mine - got).max() <= 2.0 ** -22


@pytest.mark.parametrize("name", ["test01", "test02", "test03", "test04", "test05"])
def test_qa_vectors_of_costas(name):
    q = QA["costas_" + name]
    x = FIX["qa_costas_in_" + name].view(np.complex64)
    got = FIX["qa_costas_out_" + name].view(np.complex64)
    e = np.array(q["expected"])
    exp = e[:, 0] + 1j * e[:, 1]
    assert len(x) == 100 and len(exp) == 100 - q["skip"]
    assert _places(got[q["skip"]:], exp, q["places"])
    mine = R.costas(R.Loop(q["loop_bw"], 1.0, -1.0), x, q["order"]).out
    assert _places(mine[q["skip"]:], exp, q["places"])
    assert np.abs(mine - got).max() <= 1e-5 * np.abs(x).max()


LOOP_OPS = ("create", "destroy", "set_mode", "set_streams", "set_loop_bandwidth", "set_damping_factor", "set_alpha",
            "set_beta", "set_frequency", "set_phase", "get_loop_bandwidth", "get_damping_factor", "get_alpha", "get_beta",
            "get_frequency", "get_phase", "work", "work_device")
CT_OPS = ("locksig", "lock_detector", "squelch_enable", "set_lock_threshold")


def test_new_entries_are_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = g.lib()
    for block in BLOCKS:
        names = set(re.findall(r"\b(grhip_%s_[a-z0-9_]+)\s*\(" % block, hdr))
        for op in LOOP_OPS + (CT_OPS if block == "pll_carriertracking_cc" else ()):
            assert "grhip_%s_%s" % (block, op) in names, (block, op)
        assert not [n for n in names if not hasattr(lib, n)]
        assert hasattr(g, block) and block in g.__all__
    sig = g.binding.signatures()
    import ctypes as C
    assert sig["grhip_costas_loop_cc_get_alpha"][0] is C.c_float
    assert sig["grhip_costas_loop_cc_work"][1] == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert sig["grhip_pll_freqdet_cf_create"][1] == [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int]


def test_null_arguments_are_refused_before_the_device(g):
    import ctypes as C
    lib = g.lib()
    one = C.c_float(1)
    for block in BLOCKS:
        wk = (None, 0, None, None, None) if block == "costas_loop_cc" else (None, 0, None, None)
        for op, args in (("set_mode", (None, 0)), ("set_streams", (None, 1)), ("set_loop_bandwidth", (None, one)),
                         ("set_damping_factor", (None, one)), ("set_alpha", (None, one)), ("set_beta", (None, one)),
                         ("set_frequency", (None, one)), ("set_phase", (None, one)), ("get_frequency", (None, 0, None)),
                         ("get_phase", (None, 0, None)), ("work", wk), ("work_device", wk + (None,))):
            f = getattr(lib, "grhip_%s_%s" % (block, op))
            assert f(*args) == -1, (block, op)                      # GRHIP_EINVAL
        assert getattr(lib, "grhip_%s_get_alpha" % block)(None) == -1.0
    for op, args in (("locksig", (None, 0, None)), ("lock_detector", (None, 0, None)), ("squelch_enable", (None, 1)),
                     ("set_lock_threshold", (None, one))):
        assert getattr(lib, "grhip_pll_carriertracking_cc_" + op)(*args) == -1
    assert lib.grhip_costas_loop_cc_create(None, 0.05, 2, 0) == -1
    assert lib.grhip_pll_refout_cc_create(None, 0.05, 1.0, -1.0, 0) == -1


def test_bad_order_and_the_caps_are_refused(g):
    """refused with GRHIP_EINVAL whether or not a device is there: the checks come first"""
    bad = [lambda: g.costas_loop_cc(0.05, o) for o in (0, 1, 3, 6, 16, -2)]
    bad += [lambda: g.costas_loop_cc(-0.05, 2), lambda: g.costas_loop_cc(float("nan"), 2), lambda: g.costas_loop_cc(1e19, 4)]
    for cls in (g.pll_freqdet_cf, g.pll_refout_cc, g.pll_carriertracking_cc):
        bad += [lambda c=cls: c(0.05, 1025.0, -1.0), lambda c=cls: c(0.05, 1.0, -1025.0), lambda c=cls: c(0.05, float("inf"), -1.0),
                lambda c=cls: c(0.05, 1.0, float("nan")), lambda c=cls: c(-1e-3, 1.0, -1.0)]
    for make in bad:
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1


def test_new_entries_refuse_to_run_without_a_device(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    for make in (lambda: g.costas_loop_cc(0.05, 2), lambda: g.costas_loop_cc(0.25, 8), lambda: g.pll_freqdet_cf(0.06, 2.2, -2.2),
                 lambda: g.pll_refout_cc(0.06, -3.72, -3.74), lambda: g.pll_carriertracking_cc(0.03, 1, -1)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
