"""GPU tests of pwr_squelch_cc / _ff and simple_squelch_cc against the restatement (squelch_ref.py, itself held to the
compiled reference by test_squelch_cpu.py): outputs, produced counts, the final machine state and unmuted() bit for bit
in GENERIC and in FAST.

Test signal (squelch_ref.signal): N = 20000 samples from np.random.default_rng(seed), complex Gaussian noise 0.01 per
component, a unit tone at 0.05 cycles per sample on [3000, 7000), [9000, 9030), [9500, 9900), [12000, 16000),
[16040, 16100), [19990, 20000); _ff takes its real part.  (alpha, dB): (0.01, -20), (0.0001, -40), (0.3, -10), (1.0, -20).
On it the detector stays at least 1e-9 of the threshold away from it (asserted on the restatement before anything is
compared), a million times the FAST form's deviation from the serial recurrence, so FAST is held to the same standard
as GENERIC.  The detector's own value y is the one thing FAST does not reproduce to the bit: it is held to 1e-12."""
import os
import subprocess

import numpy as np
import pytest

import squelch_ref as sq

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "gnuradio-3.5.0-dmr_amd", "host")
RAMPS = (0, 1, 7, 64, 500, 5000)
_SIG, _REF, _GUARD = {}, {}, {}


def sig(seed, cc=True, bursts=sq.BURSTS):
    k = (seed, cc, bursts)
    if k not in _SIG:
        x = sq.signal(seed, bursts=bursts)
        _SIG[k] = x if cc else x.real.astype(np.float32)
        _SIG[k].setflags(write=False)
    return _SIG[k]


def guard(x, alpha, db):
    """the no-exceptions condition, on the restatement, before anything is compared"""
    k = (id(x), alpha, db)
    if k not in _GUARD:
        _GUARD[k] = sq.closest_approach(x, alpha, db)
    assert _GUARD[k] > 1e-9, "the detector comes within %.3g of the threshold" % _GUARD[k]


def ref(x, cc, alpha, db, ramp, gate):
    """(outputs, final (state, ramped, envelope, y), unmuted) of one call over the whole of x; computed once"""
    k = (id(x), cc, alpha, db, ramp, gate)
    if k not in _REF:
        guard(x, alpha, db)
        b = sq.PwrSquelch(db, alpha, ramp, gate, cc)
        out = b.work(x)
        out.setflags(write=False)
        _REF[k] = (out, (b.state, b.ramped, b.envelope, b.y), b.unmuted())
    return _REF[k]


def make(g, cc, db, alpha, ramp, gate, mode):
    blk = (g.pwr_squelch_cc if cc else g.pwr_squelch_ff)(db, alpha, ramp, gate)
    blk.set_mode(mode)
    return blk


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_state(blk, want, unmuted, mode, g, s=0):
    st, r, env, y = blk.state(s)
    assert (st, r) == want[:2] and np.float64(env).view(np.uint64) == np.float64(want[2]).view(np.uint64), ((st, r, env), want)
    assert blk.unmuted(s) == unmuted
    if mode == g.MODE_GENERIC:
        assert y == want[3]
    else:
        assert abs(y - want[3]) <= 1e-12 * abs(want[3])


def run_split(blk, x, cuts):
    """work over x cut at `cuts` (a repeated position is a zero-length call); the outputs joined"""
    parts, edges = [], [0] + list(cuts) + [len(x)]
    for a, b in zip(edges[:-1], edges[1:]):
        parts.append(blk.work(x[a:b]))
        assert len(parts[-1]) <= b - a
    return np.concatenate(parts)


@pytest.mark.parametrize("cc", [True, False], ids=["cc", "ff"])
@pytest.mark.parametrize("pair", sq.PAIRS, ids=lambda p: "alpha%g" % p[0])
def test_one_call_every_ramp_gate_and_mode(gpu, pair, cc):
    g = gpu
    alpha, db = pair
    x = sig(1, cc)
    for ramp in RAMPS:
        for gate in (False, True):
            want, state, unm = ref(x, cc, alpha, db, ramp, gate)
            for mode in (g.MODE_GENERIC, g.MODE_FAST):
                blk = make(g, cc, db, alpha, ramp, gate, mode)
                got = blk.work(x)
                assert len(got) == len(want), (ramp, gate, mode, len(got), len(want))
                assert same_bits(got, want), (ramp, gate, mode, int(np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[0]))
                check_state(blk, state, unm, mode, g)
    assert len(ref(x, cc, alpha, db, 500, True)[0]) < len(x)            # gating does drop samples
    assert not cc or ref(x, cc, alpha, db, 64, False)[2]                # the call ends inside a burst, unmuted


CUTS = {
    "1": [1], "63-65": [63, 64, 65], "255-257": [255, 256, 257], "4095-4097": [4095, 4096, 4097],
    "mid-attack": [3010], "mid-decay": [7020], "one-by-one": list(range(2850, 3150)), "zero-length": [5000, 5000],
}


@pytest.mark.parametrize("name", list(CUTS))
def test_split_calls_give_the_same(gpu, name):
    g = gpu
    alpha, db = 0.3, -10.0
    cuts = CUTS[name]
    for cc, ramp, gate in ((True, 64, True), (False, 64, False), (True, 0, True), (False, 7, True), (True, 5000, True)):
        x = sig(1, cc)
        if name in ("mid-attack", "mid-decay") and ramp == 64:
            b = sq.PwrSquelch(db, alpha, ramp, gate, cc)
            b.work(x[:cuts[0]])
            assert b.state == (sq.ATTACK if name == "mid-attack" else sq.DECAY) and 0 < b.ramped < ramp
        want, state, unm = ref(x, cc, alpha, db, ramp, gate)
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            blk = make(g, cc, db, alpha, ramp, gate, mode)
            got = run_split(blk, x, cuts)
            assert same_bits(got, want), (cc, ramp, gate, mode)
            check_state(blk, state, unm, mode, g)


def test_zero_length_call_is_a_no_op(gpu):
    blk = gpu.pwr_squelch_cc(-20, 0.01, 64, True)
    before = blk.state()
    out = np.full(4, 7 + 7j, np.complex64)
    assert blk.work_into(0, np.zeros(0, np.complex64), out).tolist() == [0] and np.all(out == 7 + 7j)
    assert blk.state() == before
    with pytest.raises(gpu.GrhipError) as e:
        blk.work_into(-1, np.zeros(4, np.complex64), out)
    assert e.value.code == -1


SENT = np.uint32(0x7fc12345)          # a NaN payload no product makes


@pytest.mark.parametrize("device_call", [False, True], ids=["work", "work_device"])
def test_three_streams_gated(gpu, device_call):
    """seeds 1, 2, 3, the third all noise (never unmutes); the outputs of stream s start at s * n_in and nothing is
    written behind produced[s].  work_device runs on a stream of the caller's with the counts left on the device."""
    g = gpu
    alpha, db, n = 0.01, -20.0, sq.N
    for cc in (True, False):
        xs = [sig(1, cc), sig(2, cc), sig(3, cc, bursts=())]
        x = np.concatenate(xs)
        w = 2 if cc else 1
        for ramp in (64, 0):
            refs = [ref(v, cc, alpha, db, ramp, True) for v in xs]
            assert len(refs[2][0]) == 0 and not refs[2][2] and 0 < len(refs[0][0]) < n
            for mode in (g.MODE_GENERIC, g.MODE_FAST):
                blk = make(g, cc, db, alpha, ramp, True, mode)
                blk.set_streams(3)
                if device_call:
                    import torch
                    d_in = torch.from_numpy(x.view(np.uint32).copy().view(np.int32)).cuda()
                    d_out = torch.from_numpy(np.full(3 * n * w, SENT, np.uint32).view(np.int32)).cuda()
                    d_p = torch.full((3,), -1, dtype=torch.int32, device="cuda")
                    st = torch.cuda.Stream()
                    torch.cuda.synchronize()
                    blk.work_device(n, d_in, d_out, d_p, st)
                    st.synchronize()
                    out = d_out.cpu().numpy().view(np.uint32)
                    p = d_p.cpu().numpy()
                else:
                    o = np.full(3 * n * w, SENT, np.uint32).view(x.dtype)
                    p = blk.work_into(n, x, o)
                    out = o.view(np.uint32)
                for s in range(3):
                    want = refs[s][0]
                    assert p[s] == len(want), (s, p, len(want))
                    seg = out[s * n * w:(s + 1) * n * w]
                    assert np.array_equal(seg[:len(want) * w], want.view(np.uint32)), (cc, ramp, mode, s)
                    assert np.all(seg[len(want) * w:] == SENT), (cc, ramp, mode, s)
                    check_state(blk, refs[s][1], refs[s][2], mode, g, s)


def test_setters_between_calls_keep_the_state(gpu):
    g = gpu
    x = sig(1)
    guard(x, 0.3, -10.0)
    for first in (g.MODE_GENERIC, g.MODE_FAST):
        other = g.MODE_FAST if first == g.MODE_GENERIC else g.MODE_GENERIC
        blk = g.pwr_squelch_cc(-10.0, 0.3, 7, False)
        blk.set_mode(first)
        r = sq.PwrSquelch(-10.0, 0.3, 7, False, True)
        assert blk.ramp() == 7 and not blk.gate() and abs(blk.threshold() - r.threshold()) == 0
        got, want = [blk.work(x[:7010])], [r.work(x[:7010])]
        assert r.state == sq.DECAY and blk.state()[:2] == (sq.DECAY, r.ramped)
        blk.set_ramp(64); r.set_ramp(64)                                  # mid-decay: ramped kept, the new divisor
        got.append(blk.work(x[7010:9000])); want.append(r.work(x[7010:9000]))
        blk.set_threshold(-12.0); r.set_threshold(-12.0)
        blk.set_alpha(0.2); r.set_alpha(0.2)
        blk.set_gate(True); r.set_gate(True)
        blk.set_mode(other)
        assert blk.ramp() == 64 and blk.gate() and blk.threshold() == r.threshold()
        got.append(blk.work(x[9000:12005])); want.append(r.work(x[9000:12005]))
        assert r.state == sq.ATTACK and blk.state()[:2] == (sq.ATTACK, r.ramped) and blk.unmuted()
        with pytest.raises(g.GrhipError) as e:
            blk.set_ramp(0)                                               # the reference's envelope would be NaN here
        assert e.value.code == -2 and blk.ramp() == 64
        with pytest.raises(g.GrhipError) as e:
            blk.set_alpha(1.5)
        assert e.value.code == -2
        with pytest.raises(g.GrhipError) as e:
            blk.set_ramp(-1)
        assert e.value.code == -1
        with pytest.raises(g.GrhipError) as e:
            blk.set_streams(0)
        assert e.value.code == -1
        got.append(blk.work(x[12005:])); want.append(r.work(x[12005:]))
        for a, b in zip(got, want):
            assert same_bits(a, b)
        st = blk.state()
        assert st[:3] == (r.state, r.ramped, r.envelope) and abs(st[3] - r.y) <= 1e-12 * r.y
        blk.set_streams(1)                                                # restarts
        assert blk.state() == (sq.MUTED, 0, 0.0, 0.0) and not blk.unmuted()
        fresh = sq.PwrSquelch(-12.0, 0.2, 64, True, True)
        assert same_bits(blk.work(x[2000:8000]), fresh.work(x[2000:8000]))


def test_sign_of_zero_bit_patterns(gpu):
    g = gpu
    fix = np.load(os.path.join(HERE, "golden", "ref_squelch.npz"))
    z = fix["signs_in_bits"].astype(np.uint32).view(np.complex64)
    for ramp in (0, 2):
        want = fix["signs_out_bits_ramp%d" % ramp].astype(np.uint32)
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            blk = make(g, True, -20.0, 1.0, ramp, False, mode)
            got = np.concatenate([blk.work(z[:5]), blk.work(z[5:])])
            assert np.array_equal(got.view(np.uint32), want), (ramp, mode)


@pytest.mark.parametrize("pair", sq.PAIRS, ids=lambda p: "alpha%g" % p[0])
def test_simple_squelch(gpu, pair):
    g = gpu
    alpha, db = pair
    x = sig(1)
    guard(x, alpha, db)
    for cuts in ([], [1], [255, 256, 257], [3010, 4097, 7020, 16050]):
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            blk = g.simple_squelch_cc(db, alpha)
            blk.set_mode(mode)
            r = sq.SimpleSquelch(db, alpha)
            assert blk.threshold() == r.threshold() and not blk.unmuted()
            edges = [0] + cuts + [len(x)]
            for a, b in zip(edges[:-1], edges[1:]):
                got, want = blk.work(x[a:b]), r.work(x[a:b])
                assert same_bits(got, want), (cuts, mode, a)
                assert blk.unmuted() == r.unmuted()


def test_cpp_blocks(gpu):
    subprocess.check_call(["make", "-C", HOST, "squelch_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "squelch_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
