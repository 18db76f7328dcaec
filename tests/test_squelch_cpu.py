"""CPU tests of the power squelch blocks: the restatement (squelch_ref.py) against outputs recorded from the reference's
own five source files (tests/golden/ref_squelch.npz), the no-exceptions condition of the test signal, hand-evaluated
cases of the machine, and the new entries' presence and argument checks, which need no device.

Test signal (squelch_ref.signal): N = 20000 samples from np.random.default_rng(seed), complex Gaussian noise 0.01 per
component, a unit tone at 0.05 cycles per sample on [3000, 7000), [9000, 9030), [9500, 9900), [12000, 16000),
[16040, 16100), [19990, 20000); _ff takes its real part.  (alpha, dB): (0.01, -20), (0.0001, -40), (0.3, -10), (1.0, -20).

The fixture was recorded from the reference's gr_pwr_squelch_cc.cc, gr_squelch_base_cc.cc, gr_pwr_squelch_ff.cc,
gr_squelch_base_ff.cc and gr_simple_squelch_cc.cc, compiled unchanged against stub headers for gr_block, gr_sync_block
and gr_io_signature, on the seed-1 signal in two calls split at sample 4097.  The 20000-sample input and the outputs
do not fit the fixture's size as bit patterns, so it holds their SHA-256 over the bit patterns (plus the input's first
items and every case's first 160 outputs from the first attack on, as bit patterns), the produced counts of both calls
and unmuted() after each.  A small sign-of-zero case is held in full."""
import hashlib
import os
import re

import numpy as np
import pytest

import squelch_ref as sq

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = np.load(os.path.join(HERE, "golden", "ref_squelch.npz"))
NAMES = [str(n) for n in FIX["names"]]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint32).tobytes()).hexdigest()


def test_the_signal_is_the_recorded_one():
    x = sq.signal(int(FIX["seed"]))
    assert len(x) == int(FIX["n"]) == sq.N
    assert np.array_equal(x.view(np.uint32)[:64], FIX["in_cc_head_bits"])
    assert np.array_equal(x.view(np.uint32)[6000:6064], FIX["in_cc_3000_bits"])
    assert _sha(x) == str(FIX["in_cc_sha256"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_no_exceptions_condition(seed):
    """the detector never comes within 1e-9 of the threshold (relative), serial or chunked, and both give the same flags"""
    x = sq.signal(seed)
    for kind_x in (x, x.real.astype(np.float32)):
        p = sq.power(kind_x)
        for alpha, db in sq.PAIRS:
            thr = 10.0 ** (db / 10)
            ys, yc = sq.detector(p, alpha), sq.detector_chunked(p, alpha)
            near = float(np.min(np.abs(ys - thr)) / thr)
            dev = float(np.max(np.abs(yc - ys) / np.maximum(np.abs(ys), 1e-300)))
            print("seed %d alpha %g: closest approach %.3g of the threshold, chunked - serial %.3g relative" % (seed, alpha, near, dev))
            assert near > 1e-9
            assert dev * 100 < 1e-9                                   # the guard band is at least 100 x the deviation
            assert np.array_equal(ys < thr, yc < thr)


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_restatement_matches_the_compiled_reference_bit_for_bit(i):
    m = re.match(r"(\w+) a=(\S+) db=(\S+) r=(\d+) g=(\d)", NAMES[i])
    kind, alpha, db, ramp, gate = m.group(1), float(m.group(2)), float(m.group(3)), int(m.group(4)), int(m.group(5))
    x = sq.signal(int(FIX["seed"]))
    if kind == "ff":
        x = x.real.astype(np.float32)
    blk = sq.SimpleSquelch(db, alpha) if kind == "simple" else sq.PwrSquelch(db, alpha, ramp, bool(gate), kind == "cc")
    split = int(FIX["split"])
    a = blk.work(x[:split]); ua = blk.unmuted()
    b = blk.work(x[split:]); ub = blk.unmuted()
    assert [len(a), len(b), int(ua), int(ub)] == FIX["counts"][i].tolist()
    out = np.concatenate([a, b])
    win = FIX["first_attack"][i]
    s = int(win[0])
    seg = out[s:s + 160].astype(np.complex64).view(np.uint32)
    assert np.array_equal(seg, win[1:1 + len(seg)].astype(np.uint32))
    assert _sha(out) == str(FIX["out_sha256"][i])


def test_sign_of_zero_case_matches_the_compiled_reference():
    z = FIX["signs_in_bits"].astype(np.uint32).view(np.complex64)
    for ramp in (0, 2):
        blk = sq.PwrSquelch(-20, 1.0, ramp, False, True)
        got = np.concatenate([blk.work(z[:5]), blk.work(z[5:])])
        want = FIX["signs_out_bits_ramp%d" % ramp].astype(np.uint32)
        assert np.array_equal(got.view(np.uint32), want)
        assert np.count_nonzero(want == 0x80000000) >= 8           # the case does exercise negative zeros


def test_machine_by_hand():
    # alpha 1: y is the sample's power; threshold -20 dB = 0.01.  ramp 2: envelope(1, 2) = 0.5 (to an ulp), (2, 2) -> 1.0
    x = np.array([0, 1, 1, 1, 1, 0, 0, 0, 1], np.float32)
    b = sq.PwrSquelch(-20, 1.0, 2, False, False)
    e1 = np.float32(1.0 * sq.envelope(1, 2))
    # trigger with the old envelope 0, two attack steps, unmuted; the decay's trigger at envelope 1, then e1, then muted
    assert b.work(x).tolist() == [0, 0, e1, 1, 1, 0, 0, 0, 0]
    assert b.state == sq.ATTACK and b.ramped == 0 and b.unmuted()
    g = sq.PwrSquelch(-20, 1.0, 2, True, False)
    assert g.work(x).tolist() == [0, e1, 1, 1, 0, 0, 0]            # the muted samples 0 and 7 are gone
    z = sq.PwrSquelch(-20, 1.0, 0, True, False)
    assert z.work(x).tolist() == [1, 1, 1, 1, 1] and z.envelope == 1.0
    assert abs(sq.PwrSquelch(-33.0).threshold() + 33.0) < 1e-12
    s = sq.SimpleSquelch(-20, 1.0)
    assert s.work(x.astype(np.complex64)).real.tolist() == x.tolist() and s.unmuted()


NEW = ["grhip_pwr_squelch_cc", "grhip_pwr_squelch_ff", "grhip_simple_squelch_cc"]


def test_new_entries_are_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(n for n in re.findall(r"\b(grhip_[a-z0-9_]+)\s*\(", hdr) if any(n.startswith(p + "_") for p in NEW)))
    for p in NEW:
        for op in ("create", "destroy", "work", "work_device", "set_mode", "set_streams", "set_threshold", "threshold",
                   "set_alpha", "unmuted", "state"):
            assert "%s_%s" % (p, op) in names
    for p in NEW[:2]:
        for op in ("ramp", "set_ramp", "gate", "set_gate"):
            assert "%s_%s" % (p, op) in names
    assert "grhip_simple_squelch_cc_set_ramp" not in names
    lib = g.lib()
    assert not [n for n in names if not hasattr(lib, n)]
    assert g.pwr_squelch_cc.chunk() == 256 and g.pwr_squelch_cc.squelch_range() == [-50.0, 50.0, 1.0]


def test_bad_arguments_are_refused_before_the_device(g):
    for make in (lambda: g.pwr_squelch_cc(-20, 1.5), lambda: g.pwr_squelch_ff(-20, -0.1, 4), lambda: g.simple_squelch_cc(-20, 2.0),
                 lambda: g.pwr_squelch_cc(-20, float("nan"))):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -2, str(e.value)                 # GRHIP_ERANGE
    for make in (lambda: g.pwr_squelch_cc(-20, 0.1, -1), lambda: g.pwr_squelch_ff(-20, 0.1, -5, True)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1, str(e.value)                 # GRHIP_EINVAL


def test_new_entries_refuse_to_run_without_a_device(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    for make in (lambda: g.pwr_squelch_cc(-20), lambda: g.pwr_squelch_ff(-20, 0.01, 64, True), lambda: g.simple_squelch_cc(-20, 0.01)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
