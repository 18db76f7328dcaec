"""CPU tests of ctcss_squelch_ff: the restatement (ctcss_ref.py) against outputs recorded from the reference's own source
files (tests/golden/ref_ctcss_squelch.npz), guard selection, the default block length, the condition under which the FAST
kernels may be held to GENERIC's flags, and the new entries' presence and argument checks, which need no device.

Test signal (ctcss_ref.signal(seed, rate, L)): n = 80 L + 37 samples, noise 0.01 standard_normal from default_rng(seed),
plus amp sin(2 pi f t / rate) on [5L + L//3, 20L + L//2) and [25L, 27L) at 100.0 Hz, amp 0.1; [30L, 40L) at 103.5 Hz,
amp 0.1; [45L, 55L) at 100.0 Hz, amp 0.012; [60L, 70L) at 100.0 Hz, amp 0.1 with [64L, 66L) at 97.4 Hz, amp 0.3 on top;
float32.  With freq 100.0 and level 0.01 each of the three comparisons of the decision trips.

The fixture was recorded from the reference's gr_ctcss_squelch_ff.cc, gr_squelch_base_ff.cc and gri_goertzel.cc, compiled
unchanged against stub headers for gr_block, gr_io_signature and boost::shared_ptr, on the seed-1 signal at rate 500,
len 250 (20037 samples), in two calls cut at sample 4097: ramp 0 / 64 / 300 with and without gating at 100.0 Hz, and
99.0 Hz (no standard tone) and 67.0 Hz (the first tone) at ramp 64, gated.  It holds SHA-256 over the bit patterns of the
input and of every case's outputs, the input's first 64 items and 64 from the first burst on, every case's first 160
outputs from the first non-zero one on, the produced counts of both calls, unmuted() after each, the final d_mute, and,
in full, |l|, |c|, |r| of all 80 blocks for the three tones as bit patterns (taken from copies of the block's own three
filters, fed and read the way update_state does)."""
import hashlib
import os
import re

import numpy as np
import pytest

import ctcss_ref as ct

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = np.load(os.path.join(HERE, "golden", "ref_ctcss_squelch.npz"))
NAMES = [str(n) for n in FIX["names"]]
RATE, LEN, LEVEL = int(FIX["rate"]), int(FIX["len"]), float(FIX["level"])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint32).tobytes()).hexdigest()


def test_the_signal_is_the_recorded_one():
    x = ct.signal(int(FIX["seed"]), RATE, LEN)
    assert len(x) == int(FIX["n"]) == 80 * LEN + 37 and x.dtype == np.float32
    assert np.array_equal(x.view(np.uint32)[:64], FIX["in_head_bits"])
    a = 5 * LEN + LEN // 3
    assert np.array_equal(x.view(np.uint32)[a:a + 64], FIX["in_burst_bits"])
    assert _sha(x) == str(FIX["in_sha256"])


@pytest.mark.parametrize("k", range(3), ids=["100.0", "99.0", "67.0"])
def test_magnitudes_match_the_compiled_reference_bit_for_bit(k):
    """every block's |l|, |c|, |r|: the recurrence, the double real part, and the magnitude formula, which on these
    values is the host's hypotf"""
    x = ct.signal(int(FIX["seed"]), RATE, LEN)
    freq = float(FIX["mags_freqs"][k])
    got = ct.recurrence(RATE, LEN, ct.guards(freq), x[:80 * LEN])
    assert got.dtype == np.float32 and got.shape == (80, 3)
    assert np.array_equal(got.view(np.uint32), FIX["mags_bits"][k].astype(np.uint32))


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_restatement_matches_the_compiled_reference_bit_for_bit(i):
    m = re.match(r"f=(\S+) r=(\d+) g=(\d)", NAMES[i])
    freq, ramp, gate = float(m.group(1)), int(m.group(2)), int(m.group(3))
    x = ct.signal(int(FIX["seed"]), RATE, LEN)
    blk = ct.CtcssSquelch(RATE, freq, LEVEL, LEN, ramp, bool(gate))
    split = int(FIX["split"])
    a = blk.work(x[:split]); ua = blk.unmuted()
    b = blk.work(x[split:]); ub = blk.unmuted()
    assert [len(a), len(b), int(ua), int(ub)] == FIX["counts"][i].tolist()
    assert int(blk.mute) == int(FIX["mute"][i]) and len(blk.pending) == 37
    out = np.concatenate([a, b]).astype(np.float32)
    win = FIX["first_attack"][i]
    s = int(win[0])
    seg = out[s:s + 160].view(np.uint32)
    assert np.array_equal(seg, win[1:1 + len(seg)].astype(np.uint32))
    assert _sha(out) == str(FIX["out_sha256"][i])


def test_the_fixture_trips_every_comparison():
    m = FIX["mags_bits"][0].astype(np.uint32).view(np.float32)
    l, c, r = m[:, 0], m[:, 1], m[:, 2]
    lev = np.float32(LEVEL)
    assert np.any((c < lev) & (c >= l) & (c >= r))            # the level alone mutes (the weak burst)
    assert np.any((c >= lev) & (c < l) & (c >= r))            # the left guard alone (the strong 97.4 Hz tone on top)
    assert np.any((c < r) & (c >= l) & (r >= lev))            # the right guard (the 103.5 Hz burst)
    d = ct.decide(m, LEVEL)
    assert int(np.count_nonzero(~d)) == 26 and int(np.count_nonzero(d[1:] != d[:-1])) == 8
    assert not ct.decide(m, float("nan"))[(c >= l) & (c >= r)].any()      # a NaN level never mutes


def test_guard_selection():
    f = np.float32
    assert ct.guards(100.0) == (f(97.4), f(100.0), f(103.5))                       # a standard tone: its neighbours
    assert ct.guards(99.0) == (f(99.0 * 0.98), f(99.0), f(99.0 * 1.02))            # no standard tone: 2 % either side
    assert ct.guards(67.0) == (f(67.0 * 0.98), f(67.0), f(71.9))                   # the first: 2 % below
    assert ct.guards(250.3) == (f(241.8), f(250.3), f(float(f(250.3)) * 1.02))     # the last: 2 % above
    assert ct.guards(100.000001)[0] == f(97.4)                                     # the compare is on floats
    assert ct.guards(100.0001)[0] == f(float(f(100.0001)) * 0.98)
    # the product is formed in double and stored to float, not formed in float
    assert any(f(float(f(t)) * 0.98) != f(t) * f(0.98) for t in (99.0, 101.0, 123.4, 88.8, 67.0))


def test_len_defaults_to_a_tenth_of_a_second():
    assert ct.default_len(8000) == 800 and ct.default_len(500) == 50 and ct.default_len(44100) == 4410 and ct.default_len(11025) == 1102
    assert ct.CtcssSquelch(8000, 100.0).len == 800 and ct.CtcssSquelch(8000, 100.0, len=250).len == 250


def test_block_phase_across_calls():
    """however the stream is cut, the flags are those of one call; a call that completes nothing reuses the decision"""
    x = ct.signal(2, RATE, LEN)[:12 * LEN + 37]
    want = ct.CtcssSquelch(RATE, 100.0, LEVEL, LEN).flags(x)
    assert want[:LEN - 1].all() and not want[LEN * 7 - 1:LEN * 8].any()             # d_mute starts true; inside the burst
    for cuts in ([1], [249], [250], [251], [249, 250, 251], list(range(240, 265, 7)), [600, 600], [4097 % len(x)]):
        b = ct.CtcssSquelch(RATE, 100.0, LEVEL, LEN)
        edges = [0] + cuts + [len(x)]
        got = np.concatenate([b.flags(x[a:e]) for a, e in zip(edges[:-1], edges[1:])])
        assert np.array_equal(got, want), cuts
        assert len(b.pending) == 37 and len(b.mags) == 12


CASES = [(500, 250), (8000, 800)]


@pytest.mark.parametrize("rate,L", CASES)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_condition(seed, rate, L):
    """A cap: no comparison of any block comes closer to a tie than 10 x the largest relative deviation between the
    float recurrence and closed_form() on the same blocks (ctcss_ref.condition has the arithmetic).  Under it FAST may
    be required to give GENERIC's flags with no block left out."""
    x = ct.signal(seed, rate, L)
    margin, deviation = ct.condition(rate, L, 100.0, 0.01, x)
    print("seed %d rate %d len %d: margin %.3g, deviation %.3g, ratio %.3g" % (seed, rate, L, margin, deviation, margin / deviation))
    assert margin >= 10 * deviation
    b = ct.CtcssSquelch(rate, 100.0, 0.01, L)
    d = b.flags(x)[L - 1::L]
    assert int(np.count_nonzero(~d)) == 26 and int(np.count_nonzero(d[1:] != d[:-1])) == 8
    cf = ct.decide(ct.closed_form(rate, L, b.tones, x[:80 * L]).astype(np.float32), 0.01)
    assert np.array_equal(cf, d)


OPS = ("create", "destroy", "set_mode", "set_streams", "level", "set_level", "len", "ramp", "set_ramp", "gate", "set_gate",
       "squelch_range", "unmuted", "state", "tones", "work", "work_device")


def test_new_entries_are_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(grhip_ctcss_squelch_ff_[a-z0-9_]+)\s*\(", hdr))
    lib = g.lib()
    for op in OPS:
        assert "grhip_ctcss_squelch_ff_" + op in names, op
    assert not [n for n in names if not hasattr(lib, n)]
    assert g.ctcss_squelch_ff.squelch_range() == [0.0, 1.0, float(np.float32(0.01))]


def test_bad_arguments_are_refused_before_the_device(g):
    for make in (lambda: g.ctcss_squelch_ff(0, 100.0), lambda: g.ctcss_squelch_ff(-8000, 100.0), lambda: g.ctcss_squelch_ff(8000, 100.0, 0.01, -1),
                 lambda: g.ctcss_squelch_ff(8000, float("nan")), lambda: g.ctcss_squelch_ff(8000, float("inf")),
                 lambda: g.ctcss_squelch_ff(8000, 100.0, 0.01, 0, -1), lambda: g.ctcss_squelch_ff(8000, 100.0, 0.01, 0, (1 << 24) + 1)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1, str(e.value)                 # GRHIP_EINVAL
    for make in (lambda: g.ctcss_squelch_ff(8000, 100.0, 0.01, (1 << 20) + 1), lambda: g.ctcss_squelch_ff(9, 100.0)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -2, str(e.value)                 # GRHIP_ERANGE: the effective len outside 1 .. 2^20


def test_new_entry_refuses_to_run_without_a_device(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(g.GrhipError) as e:
        g.ctcss_squelch_ff(8000, 100.0, 0.01, 0, 64, True)
    assert e.value.code == -5 and "no CPU fallback" in str(e.value)
