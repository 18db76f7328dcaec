"""GPU tests of ctcss_squelch_ff against the restatement (ctcss_ref.py, itself held to the compiled reference by
test_ctcss_squelch_cpu.py): outputs, produced counts, the final machine state, d_mute and the length of the unfinished
block bit for bit, in GENERIC and in FAST.

Test signal (ctcss_ref.signal(seed, rate, L)): n = 80 L + 37 samples, noise 0.01, bursts of 100.0 Hz (amp 0.1, 0.012),
103.5 Hz and 97.4 Hz as listed in test_ctcss_squelch_cpu.py; freq 100.0, level 0.01.  At (rate, L) = (500, 250) that is
20037 samples.  FAST evaluates the closed form of the recurrence, so it is held to GENERIC's flags only under the
condition (ctcss_ref.condition): no comparison of any block closer to a tie than 10 x the largest relative deviation
between the float recurrence and the closed form.  The condition is asserted on the restatement before anything is
compared, for every shape used here, and no block is left out."""
import os
import subprocess

import numpy as np
import pytest

import ctcss_ref as ct
import squelch_ref as sq

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "gnuradio-3.5.0-dmr_amd", "host")
RATE, LEN, FREQ, LEVEL = 500, 250, 100.0, 0.01
RAMPS = (0, 1, 64, 300, 600)                 # 300 and 600 outlast one and two blocks: decisions arrive mid-ramp
_SIG, _REF, _COND = {}, {}, {}


def sig(seed, rate=RATE, L=LEN, bursts=True):
    k = (seed, rate, L, bursts)
    if k not in _SIG:
        _SIG[k] = ct.signal(seed, rate, L, bursts)
        _SIG[k].setflags(write=False)
    return _SIG[k]


def cond(x, rate=RATE, L=LEN, level=LEVEL):
    """(margin, deviation) of the condition, asserted; computed once per signal"""
    k = (id(x), rate, L, level)
    if k not in _COND:
        _COND[k] = ct.condition(rate, L, FREQ, level, x)
    margin, deviation = _COND[k]
    assert margin >= 10 * deviation, "margin %.3g, deviation %.3g" % (margin, deviation)
    return margin, deviation


def ref(x, ramp, gate, rate=RATE, L=LEN, level=LEVEL):
    """(outputs, (state, ramped, envelope, d_mute, pending), unmuted) of one call over the whole of x; computed once"""
    k = (id(x), ramp, gate, rate, L, level)
    if k not in _REF:
        b = ct.CtcssSquelch(rate, FREQ, level, L, ramp, gate)
        out = b.work(x)
        out.setflags(write=False)
        _REF[k] = (out, (b.state, b.ramped, b.envelope, b.mute, len(b.pending)), b.unmuted())
    return _REF[k]


def make(g, ramp, gate, mode, rate=RATE, L=LEN, level=LEVEL):
    blk = g.ctcss_squelch_ff(rate, FREQ, level, L, ramp, gate)
    blk.set_mode(mode)
    return blk


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_state(blk, want, unmuted, s=0):
    st, r, env, mute, pending = blk.state(s)
    assert (st, r, mute, pending) == (want[0], want[1], want[3], want[4]), ((st, r, mute, pending), want)
    assert np.float64(env).view(np.uint64) == np.float64(want[2]).view(np.uint64), (env, want[2])
    assert blk.unmuted(s) == unmuted


def run_split(blk, x, cuts):
    """work over x cut at `cuts` (a repeated position is a zero-length call); the outputs joined"""
    parts, edges = [], [0] + list(cuts) + [len(x)]
    for a, b in zip(edges[:-1], edges[1:]):
        parts.append(blk.work(x[a:b]))
        assert len(parts[-1]) <= b - a
    return np.concatenate(parts)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_call_every_ramp_gate_and_mode(gpu, seed):
    g = gpu
    x = sig(seed)
    cond(x)
    for ramp in RAMPS:
        for gate in (False, True):
            want, state, unm = ref(x, ramp, gate)
            for mode in (g.MODE_GENERIC, g.MODE_FAST):
                blk = make(g, ramp, gate, mode)
                got = blk.work(x)
                assert len(got) == len(want), (ramp, gate, mode, len(got), len(want))
                assert same_bits(got, want), (ramp, gate, mode, int(np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[0]))
                check_state(blk, state, unm)
    assert 0 < len(ref(x, 64, True)[0]) < len(x)                        # gating does drop samples
    assert ref(x, 0, False)[1][3:] == (True, 37)                        # the call ends muted, 37 samples into a block


def test_fixture_cases_in_two_calls(gpu):
    """the compiled reference's own outputs (SHA-256 and the first 160 outputs from the first non-zero one on)"""
    import hashlib
    import re
    g = gpu
    fix = np.load(os.path.join(HERE, "golden", "ref_ctcss_squelch.npz"))
    x = sig(int(fix["seed"]))
    split = int(fix["split"])
    for i, name in enumerate(str(n) for n in fix["names"]):
        m = re.match(r"f=(\S+) r=(\d+) g=(\d)", name)
        freq, ramp, gate = float(m.group(1)), int(m.group(2)), int(m.group(3))
        blk = g.ctcss_squelch_ff(RATE, freq, LEVEL, LEN, ramp, bool(gate))
        blk.set_mode(g.MODE_GENERIC)
        a = blk.work(x[:split]); ua = blk.unmuted()
        b = blk.work(x[split:]); ub = blk.unmuted()
        assert [len(a), len(b), int(ua), int(ub)] == fix["counts"][i].tolist(), name
        out = np.concatenate([a, b])
        s = int(fix["first_attack"][i][0])
        seg = out[s:s + 160].view(np.uint32)
        assert np.array_equal(seg, fix["first_attack"][i][1:1 + len(seg)].astype(np.uint32)), name
        assert hashlib.sha256(out.view(np.uint32).tobytes()).hexdigest() == str(fix["out_sha256"][i]), name
        k = [100.0, 99.0, 67.0].index(freq)
        assert blk.tones() == ct.guards(freq)
        tail = blk.last_magnitudes(80)                                  # the blocks the second call completed
        assert np.array_equal(tail.view(np.uint32), fix["mags_bits"][k].astype(np.uint32)[80 - len(tail):]) and len(tail) == 80 - split // LEN


CUTS = {
    "1": [1], "249": [249], "250": [250], "251": [251], "4097": [4097],
    "sevens": list(range(233, 275, 7)),         # calls of 7 samples across the block end at 250: most complete nothing
    "zero-length": [5000, 5000],
}


@pytest.mark.parametrize("name", list(CUTS))
def test_split_calls_give_the_same(gpu, name):
    g = gpu
    x = sig(1)
    cond(x)
    cuts = CUTS[name]
    for ramp, gate in ((64, True), (0, False), (0, True), (300, True), (600, False)):
        want, state, unm = ref(x, ramp, gate)
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            blk = make(g, ramp, gate, mode)
            got = run_split(blk, x, cuts)
            assert same_bits(got, want), (ramp, gate, mode)
            check_state(blk, state, unm)


def test_a_call_that_completes_nothing_keeps_the_decision(gpu):
    g = gpu
    x = sig(1)
    a = 5 * LEN + LEN // 3 + 2 * LEN                                    # inside the first burst, unmuted
    r = ct.CtcssSquelch(RATE, FREQ, LEVEL, LEN, 0, True)
    blk = make(g, 0, True, g.MODE_FAST)
    assert same_bits(blk.work(x[:a]), r.work(x[:a])) and not r.mute and blk.state()[3:] == (False, a % LEN)
    for n in (7, 1, 30):                                                # a % LEN + 38 < LEN: nothing completes
        got, want = blk.work(x[a:a + n]), r.work(x[a:a + n])
        assert len(got) == n and same_bits(got, want) and len(blk.last_magnitudes(4)) == 0
        a += n
        assert blk.state()[3:] == (False, a % LEN)


def test_set_mode_with_a_block_in_progress(gpu):
    """a block in progress is evaluated whole in the mode in force when it completes: its magnitudes are, bit for bit,
    those a handle that ran in that mode all along gives for it"""
    g = gpu
    x = sig(1)
    cond(x)
    cut = 4097                                                          # 97 samples into block 16
    want, state, unm = ref(x, 64, True)
    allfast = make(g, 64, True, g.MODE_FAST)
    allfast.work(x)
    fast_mags = allfast.last_magnitudes(80)
    rec_mags = ct.recurrence(RATE, LEN, ct.guards(FREQ), x[:80 * LEN])
    assert not np.array_equal(fast_mags.view(np.uint32), rec_mags.view(np.uint32))   # the two modes do differ in the last places
    for first, second, mags in ((g.MODE_GENERIC, g.MODE_FAST, fast_mags), (g.MODE_FAST, g.MODE_GENERIC, rec_mags)):
        blk = make(g, 64, True, first)
        a = blk.work(x[:cut])
        assert blk.state()[4] == cut % LEN
        blk.set_mode(second)
        b = blk.work(x[cut:])
        assert same_bits(np.concatenate([a, b]), want)
        check_state(blk, state, unm)
        got = blk.last_magnitudes(80)
        assert np.array_equal(got.view(np.uint32), mags[cut // LEN:].view(np.uint32))


def short_signal(seed, rate, L, n):
    """noise of 0.01 and, in units of L: 100.0 Hz on [1 1/3, 3), 103.5 Hz on [6, 8), 100.0 Hz on [10, 13) and [14 1/2, 40),
    amp 0.1, cut at n"""
    x = 0.01 * np.random.default_rng(seed).standard_normal(n)
    t = np.arange(n)
    for a, b, f in ((L + L // 3, 3 * L, 100.0), (6 * L, 8 * L, 103.5), (10 * L, 13 * L, 100.0), (14 * L + L // 2, 40 * L, 100.0)):
        a, b = min(a, n), min(b, n)
        x[a:b] += 0.1 * np.sin(2 * np.pi * f * t[a:b] / rate)
    return x.astype(np.float32)


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 250, 2047, 2048, 5000])
def test_block_lengths(gpu, L):
    """many decisions per flag word, one per word or so, and blocks longer than the walk's 4096-flag step; 2047 / 2048 is
    where FAST deals a block to a workgroup.  The rate is 2 L, so the tones stay 1.3 and 1.75 bins apart as at (500, 250)
    (below the Nyquist rate from L = 100 down: the aliased tones are as far apart).  L = 1 and 2 resolve nothing: the
    three magnitudes nearly tie, and only GENERIC, which is bit for bit the recurrence, is compared."""
    g = gpu
    rate = 2 * L if L >= 63 else 500
    n = max(4 * L + 37, 1000)
    x = short_signal(L, rate, L, n)
    modes = (g.MODE_GENERIC,)
    if L >= 63:
        cond(x, rate, L)                                                # asserted: none of these shapes is let off
        modes = (g.MODE_GENERIC, g.MODE_FAST)
    for ramp, gate in ((0, False), (64, True), (0, True)):
        want, state, unm = ref(x, ramp, gate, rate, L)
        if L >= 63:
            assert 0 < len(ref(x, 64, True, rate, L)[0]) < n           # something is muted and something is not
        for mode in modes:
            for cuts in ([], [n // 2 + 1]):
                blk = make(g, ramp, gate, mode, rate, L)
                got = run_split(blk, x, cuts)
                assert same_bits(got, want), (L, ramp, gate, mode, cuts)
                check_state(blk, state, unm)


SENT = np.uint32(0x7fc12345)          # a NaN payload no product makes


@pytest.mark.parametrize("device_call", [False, True], ids=["work", "work_device"])
def test_three_streams_gated(gpu, device_call):
    """seeds 1 and 2 and a stream of pure noise (never unmutes); the outputs of stream s start at s * n_in and nothing is
    written behind produced[s].  work_device runs on a stream of the caller's with the counts left on the device."""
    g = gpu
    xs = [sig(1), sig(2), sig(3, bursts=False)]
    for v in xs:
        cond(v)
    x = np.concatenate(xs)
    n = len(xs[0])
    for ramp in (64, 0):
        refs = [ref(v, ramp, True) for v in xs]
        assert len(refs[2][0]) == 0 and not refs[2][2] and 0 < len(refs[0][0]) < n
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            blk = make(g, ramp, True, mode)
            blk.set_streams(3)
            if device_call:
                import torch
                d_in = torch.from_numpy(x.view(np.int32).copy()).cuda()
                d_out = torch.from_numpy(np.full(3 * n, SENT, np.uint32).view(np.int32)).cuda()
                d_p = torch.full((3,), -1, dtype=torch.int32, device="cuda")
                st = torch.cuda.Stream()
                torch.cuda.synchronize()
                blk.work_device(n, d_in, d_out, d_p, st)
                st.synchronize()
                out = d_out.cpu().numpy().view(np.uint32)
                p = d_p.cpu().numpy()
            else:
                o = np.full(3 * n, SENT, np.uint32).view(np.float32)
                p = blk.work_into(n, x, o)
                out = o.view(np.uint32)
            for s in range(3):
                want = refs[s][0]
                assert p[s] == len(want), (s, p, len(want))
                seg = out[s * n:(s + 1) * n]
                assert np.array_equal(seg[:len(want)], want.view(np.uint32)), (ramp, mode, s)
                assert np.all(seg[len(want):] == SENT), (ramp, mode, s)
                check_state(blk, refs[s][1], refs[s][2], s)


def test_setters_between_calls_keep_carry_and_state(gpu):
    g = gpu
    x = sig(1)
    cond(x)
    cond(x, level=0.02)
    f0 = int(np.flatnonzero(~ct.CtcssSquelch(RATE, FREQ, LEVEL, LEN).flags(x))[0])          # the first sample that unmutes
    later = ct.CtcssSquelch(RATE, FREQ, 0.02, LEN).flags(x)
    a = f0 + 11                                                         # ten samples into the attack
    b = a + 3 * LEN + 11
    assert not later[b - 1]
    c = b + int(np.flatnonzero(later[b:])[0]) + 51                      # fifty samples into the decay
    for first in (g.MODE_GENERIC, g.MODE_FAST):
        other = g.MODE_FAST if first == g.MODE_GENERIC else g.MODE_GENERIC
        blk = make(g, 64, False, first)
        r = ct.CtcssSquelch(RATE, FREQ, LEVEL, LEN, 64, False)
        assert blk.ramp() == 64 and not blk.gate() and blk.level() == np.float32(LEVEL) and blk.len() == LEN
        got, want = [blk.work(x[:a])], [r.work(x[:a])]
        assert r.state == sq.ATTACK and blk.state() == (sq.ATTACK, 10, r.envelope, False, a % LEN)
        blk.set_ramp(300); r.set_ramp(300)                              # mid-attack: ramped kept, the new divisor
        blk.set_level(0.02); r.set_level(0.02)
        got.append(blk.work(x[a:b])); want.append(r.work(x[a:b]))
        blk.set_gate(True); r.set_gate(True)
        blk.set_mode(other)
        assert blk.ramp() == 300 and blk.gate() and blk.level() == np.float32(0.02)
        got.append(blk.work(x[b:c])); want.append(r.work(x[b:c]))
        assert r.state == sq.DECAY and r.ramped == 250 and blk.state()[:2] == (sq.DECAY, 250)
        with pytest.raises(g.GrhipError) as e:
            blk.set_ramp(0)                                             # the reference's envelope would be NaN here
        assert e.value.code == -2 and blk.ramp() == 300
        with pytest.raises(g.GrhipError) as e:
            blk.set_ramp(-1)
        assert e.value.code == -1
        with pytest.raises(g.GrhipError) as e:
            blk.set_streams(0)
        assert e.value.code == -1
        got.append(blk.work(x[c:])); want.append(r.work(x[c:]))
        for u, v in zip(got, want):
            assert same_bits(u, v)
        check_state(blk, (r.state, r.ramped, r.envelope, r.mute, len(r.pending)), r.unmuted())
        blk.set_streams(1)                                              # restarts: muted, d_mute true, nothing carried
        assert blk.state() == (sq.MUTED, 0, 0.0, True, 0) and not blk.unmuted()
        fresh = ct.CtcssSquelch(RATE, FREQ, 0.02, LEN, 300, True)
        assert same_bits(blk.work(x[1000:9000]), fresh.work(x[1000:9000]))


def test_a_nan_level_never_mutes_on_the_level(gpu):
    g = gpu
    x = sig(1)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = make(g, 0, True, mode, level=float("nan"))
        r = ct.CtcssSquelch(RATE, FREQ, float("nan"), LEN, 0, True)
        want = r.work(x[:20 * LEN])                                     # noise, then the first burst
        got = blk.work(x[:20 * LEN])
        if mode == g.MODE_GENERIC:
            assert same_bits(got, want)
        assert len(got) >= 14 * LEN                                     # the burst's whole blocks, at the least


@pytest.mark.parametrize("rate,L", [(500, 250), (8000, 800)])
def test_fast_magnitudes_against_the_closed_form(gpu, rate, L):
    """|l|, |c|, |r| of every block in FAST lie within the condition's deviation of closed_form(): FAST is at least as
    close to the exact value as the float recurrence it stands in for.  (8000, 800) is 64037 samples."""
    g = gpu
    for seed in (1, 2, 3):
        x = sig(seed, rate, L)
        margin, deviation = cond(x, rate, L)
        blk = make(g, 0, False, g.MODE_FAST, rate, L)
        blk.work(x)
        got = blk.last_magnitudes(80).astype(np.float64)
        cf = ct.closed_form(rate, L, ct.guards(FREQ), x[:80 * L])
        worst = float(np.max(np.abs(got - cf) / cf))
        print("seed %d rate %d len %d: FAST - closed form %.3g relative, recurrence - closed form %.3g" % (seed, rate, L, worst, deviation))
        assert got.shape == (80, 3) and worst <= deviation
        gen = make(g, 0, False, g.MODE_GENERIC, rate, L)
        gen.work(x)
        rec = ct.recurrence(rate, L, ct.guards(FREQ), x[:80 * L])
        assert np.array_equal(gen.last_magnitudes(80).view(np.uint32), rec.view(np.uint32))


def test_calls_that_are_refused(gpu):
    import torch
    g = gpu
    blk = make(g, 64, True, g.MODE_FAST)
    before = blk.state()
    out = np.full(4, 7, np.float32)
    assert blk.work_into(0, np.zeros(0, np.float32), out).tolist() == [0] and np.all(out == 7)
    with pytest.raises(g.GrhipError) as e:
        blk.work_into(-1, np.zeros(4, np.float32), out)
    assert e.value.code == -1
    d = torch.zeros(600, dtype=torch.float32, device="cuda")
    d_p = torch.zeros(1, dtype=torch.int32, device="cuda")
    for d_out in (d, d[299:]):
        with pytest.raises(g.GrhipError) as e:
            blk.work_device(300, d, d_out, d_p)
        assert e.value.code == -1 and "overlap" in str(e.value)
    assert blk.state() == before


def test_cpp_block(gpu):
    subprocess.check_call(["make", "-C", HOST, "ctcss_squelch_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "ctcss_squelch_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
