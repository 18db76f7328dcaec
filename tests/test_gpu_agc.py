"""GPU tests of agc_cc / agc_ff / agc2_cc / agc2_ff against the restatement (agc_ref.py, pinned to the reference's own
code by test_agc_cpu.py).  GENERIC of all four blocks and every mode of agc2_* are held to it bit for bit, outputs and
gain; the chunked form of agc_cc / agc_ff (every other mode, calls of more than 256 items) to
    dev_fast <= 2 dev_ref + 4 * 2^-23,
where dev_ref is the serial float restatement's largest deviation of the gain track from the float64 recurrence,
relative to that track's peak gain, recomputed here per case: on gain() directly and on the outputs as
    |out_i - x_i g64_i| <= |x_i| bound peak + 2^-23 |x_i g64_i|."""
import functools
import os
import subprocess

import numpy as np
import pytest

import agc_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "gnuradio-3.5.0-dmr_amd", "host")
SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def sig(seed, block):
    x = R.signal(seed, block)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref(block, pi, seed, gain=None):
    """the serial restatement (cuts do not change it), and for agc_* the float64 track and dev_ref"""
    x = sig(seed, block)
    params = R.sets(block)[pi]
    r = R.serial(block, x, params, gain)
    if block.startswith("agc2"):
        return r, None, None
    g64 = R.exact64(block, x, params, gain)
    return r, g64, R.deviation(r.gains, g64)


def make(g, block, params, mode, streams=1):
    blk = getattr(g, block)(*params)
    blk.set_mode(mode)
    if streams != 1:
        blk.set_streams(streams)
    return blk


def run(blk, xs, cuts=(), empty_between=False):
    """the streams xs (equal lengths) through blk in calls cut at `cuts`; returns every stream's outputs"""
    n = len(xs[0])
    edges = [0] + [c for c in cuts if 0 < c < n] + [n]
    outs = [[] for _ in xs]
    for a, b in zip(edges[:-1], edges[1:]):
        y = blk.work(np.concatenate([x[a:b] for x in xs]), b - a)
        for s in range(len(xs)):
            outs[s].append(y[s * (b - a):(s + 1) * (b - a)])
        if empty_between:
            assert len(blk.work(np.zeros(0, xs[0].dtype), 0)) == 0
    return [np.concatenate(o) for o in outs]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


def check_bound(block, x, out, gain, g64, dev_ref, what):
    """the issue's two inequalities; prints dev_fast as the outputs show it"""
    peak = np.max(np.abs(g64))
    bound = R.bound(dev_ref)
    ideal = x.astype(np.complex128 if R.is_cc(block) else np.float64) * g64[:-1]
    mag = R.mag64(x)
    err = np.abs(out - ideal)
    tol = mag * bound * peak + 2.0 ** -23 * np.abs(ideal)
    nz = mag > 0
    dev_fast = float(np.max(err[nz] / mag[nz]) / peak) if nz.any() else 0.0
    dev_gain = abs(float(gain) - g64[-1]) / peak
    print("%s: dev_ref %.3g bound %.3g dev_fast(outputs) %.3g dev(gain()) %.3g" % (what, dev_ref, bound, dev_fast, dev_gain))
    assert np.all(err <= tol), what
    assert dev_gain <= bound, what


# ---- GENERIC, all four blocks: bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("block", R.BLOCKS)
def test_generic_one_call_and_cut_calls(gpu, block):
    g = gpu
    for pi, params in enumerate(R.sets(block)):
        x = sig(1, block)
        r = ref(block, pi, 1)[0]
        if block.startswith("agc2") and pi == 2:
            assert r.resets > 100                                   # the 10e-5 reset is exercised
        for cuts, empty in (((), False), (R.CUTS, True)):
            blk = make(g, block, params, g.MODE_GENERIC)
            got = run(blk, [x], cuts, empty)[0]
            assert same_bits(got, r.out), (block, pi, cuts)
            assert R.bits(np.array([blk.gain()]))[0] == R.bits(r.gains[-1:])[0], (block, pi, cuts)


@pytest.mark.parametrize("block", R.BLOCKS)
def test_generic_three_streams(gpu, block):
    g = gpu
    for pi, params in enumerate(R.sets(block)):
        blk = make(g, block, params, g.MODE_GENERIC, 3)
        got = run(blk, [sig(s, block) for s in SEEDS], (4097,))
        for k, s in enumerate(SEEDS):
            r = ref(block, pi, s)[0]
            assert same_bits(got[k], r.out), (block, pi, s)
            assert R.bits(np.array([blk.gain(k)]))[0] == R.bits(r.gains[-1:])[0], (block, pi, s)


@pytest.mark.parametrize("block", R.BLOCKS)
def test_generic_setters_between_calls(gpu, block):
    g = gpu
    x = sig(2, block)
    two = block.startswith("agc2")
    params = R.sets(block)[0]
    for mode in (g.MODE_GENERIC,) + ((g.MODE_FAST,) if two else ()):
        blk = make(g, block, params, mode)
        a = R.serial(block, x[:3000], params)
        got = [blk.work(x[:3000])]
        # a new rate, gain and clamp hold from the next call on
        if two:
            blk.set_attack_rate(3e-2)
            blk.set_decay_rate(2e-3)
            p2 = (3e-2, 2e-3, params[2], 0.0, 1.5)
            assert blk.attack_rate() == np.float32(3e-2) and blk.decay_rate() == np.float32(2e-3)
        else:
            blk.set_rate(5e-3)
            p2 = (5e-3, params[1], 0.0, 1.5)
            assert blk.rate() == np.float32(5e-3)
        assert blk.gain() == a.gain
        blk.set_gain(0.25)
        blk.set_max_gain(1.5)
        assert blk.gain() == np.float32(0.25) and blk.max_gain() == np.float32(1.5) and blk.reference() == np.float32(1)
        b = R.serial(block, x[3000:], p2, 0.25)
        assert b.clamped > 0
        got.append(blk.work(x[3000:]))
        assert same_bits(got[0], a.out) and same_bits(got[1], b.out), (block, mode)
        assert blk.gain() == b.gain
        blk.set_reference(0.5)
        c = R.serial(block, x[:500], p2[:-3] + (0.5,) + p2[-2:], b.gain)
        assert same_bits(blk.work(x[:500]), c.out)
        # set_streams restarts every stream from the constructor's gain
        blk.set_streams(2)
        assert blk.gain(0) == blk.gain(1) == np.float32(params[-2])
        with pytest.raises(g.GrhipError):
            blk.gain(2)
        with pytest.raises(g.GrhipError):
            blk.set_streams(0)


# ---- agc2_*: every mode is the serial walk -----------------------------------------------------------------------
@pytest.mark.parametrize("block", ("agc2_cc", "agc2_ff"))
def test_agc2_fast_is_generic(gpu, block):
    g = gpu
    for pi, params in enumerate(R.sets(block)):
        for streams, cuts in ((1, ()), (3, (257, 4097))):
            blk = make(g, block, params, g.MODE_FAST, streams)
            got = run(blk, [sig(s, block) for s in SEEDS[:streams]], cuts)
            for k in range(streams):
                r = ref(block, pi, SEEDS[k])[0]
                assert same_bits(got[k], r.out), (block, pi, streams)
                assert blk.gain(k) == r.gain


# ---- agc_*: the chunked form within the bound --------------------------------------------------------------------
@pytest.mark.parametrize("block", ("agc_cc", "agc_ff"))
@pytest.mark.parametrize("pi", range(len(R.AGC_SETS)))
def test_agc_fast_within_the_bound(gpu, block, pi):
    g = gpu
    params = R.AGC_SETS[pi]
    if pi == 3:
        for s in SEEDS:
            r = ref(block, pi, s)[0]
            assert r.gains.min() < 0 and np.isfinite(r.gains).all()     # the negative-gain branch is exercised
            assert sum(R.chunk_triples(block, sig(s, block), params)[1]) >= 5
    for streams in (1, 3):
        for cuts in ((), R.CUTS):
            blk = make(g, block, params, g.MODE_FAST, streams)
            got = run(blk, [sig(s, block) for s in SEEDS[:streams]], cuts, empty_between=bool(cuts))
            for k in range(streams):
                r, g64, dev_ref = ref(block, pi, SEEDS[k])
                if pi == 3:
                    assert np.isfinite(R.bits(got[k]).view(np.float32)).all()
                check_bound(block, sig(SEEDS[k], block), got[k], blk.gain(k), g64, dev_ref,
                            "%s set %d seed %d S %d cuts %s" % (block, pi, SEEDS[k], streams, cuts))


@pytest.mark.parametrize("block", ("agc_cc", "agc_ff"))
def test_agc_fast_shortest_calls_and_stream_alignment(gpu, block):
    g = gpu
    for pi in (0, 3):
        params = R.AGC_SETS[pi]
        x = sig(1, block)[2400:]                        # silence, then the loud part
        # 256 items: the serial walk, bit for bit; 257: the shortest chunked call
        blk = make(g, block, params, g.MODE_FAST)
        r = R.serial(block, x[:256], params)
        assert same_bits(blk.work(x[:256]), r.out) and blk.gain() == r.gain
        for n in (257, 513):
            blk = make(g, block, params, g.MODE_FAST)
            r = R.serial(block, x[:n], params)
            g64 = R.exact64(block, x[:n], params)
            check_bound(block, x[:n], blk.work(x[:n]), blk.gain(), g64, R.deviation(r.gains, g64), "%s set %d n %d" % (block, pi, n))
    # three streams whose starts are 16-byte aligned (n a multiple of 4) and not (n odd): both load widths
    params = R.AGC_SETS[0]
    for n in (6036, 6037, 1031):
        blk = make(g, block, params, g.MODE_FAST, 3)
        xs = [sig(s, block)[:n] for s in SEEDS]
        got = run(blk, xs)
        for k in range(3):
            r = R.serial(block, xs[k], params)
            g64 = R.exact64(block, xs[k], params)
            check_bound(block, xs[k], got[k], blk.gain(k), g64, R.deviation(r.gains, g64), "%s S 3 n %d stream %d" % (block, n, k))


@pytest.mark.parametrize("block", ("agc_cc", "agc_ff"))
def test_agc_fast_from_a_negative_gain(gpu, block):
    g = gpu
    for pi in (0, 3):
        params = R.AGC_SETS[pi]
        x = sig(3, block)
        r, g64, dev_ref = ref(block, pi, 3, -0.5)
        assert r.gains[0] < 0 and r.gains.max() > 0.5                          # negative at the start, then recovers
        if pi == 0:
            assert r.gains[300] < 0                                             # ... after more than a chunk
        blk = make(g, block, params, g.MODE_FAST)
        blk.set_gain(-0.5)
        got = blk.work(x)
        check_bound(block, x, got, blk.gain(), g64, dev_ref, "%s set %d from -0.5" % (block, pi))


def test_agc_fallbacks_are_the_serial_walk(gpu):
    """rate < 0, reference < 0 or a parameter that is not finite: the serial walk whatever the mode, NaN and all"""
    g = gpu
    x = sig(1, "agc_cc")[:1200]
    for params in ((-1e-4, 1, 1, 0), (1e-3, -1, 1, 0), (1e-3, 1, 1, float("inf"))):
        blk = make(g, "agc_cc", params, g.MODE_FAST)
        r = R.serial("agc_cc", x, params)
        assert same_bits(blk.work(x), r.out), params
        assert R.bits(np.array([blk.gain()]))[0] == R.bits(r.gains[-1:])[0]
    blk = make(g, "agc_cc", (float("nan"), 1, 1, 0), g.MODE_FAST)
    got = blk.work(x)
    assert same_bits(got[:1], x[:1]) and np.isnan(got[1:].real).all() and np.isnan(blk.gain())
    # an infinity and a NaN among the samples of a chunked call: flagged chunks, walked in float
    y = x.copy()
    y[300] = np.inf
    y[700] = complex(np.nan, 1.0)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = make(g, "agc_cc", R.AGC_SETS[0], mode)
        r = R.serial("agc_cc", y, R.AGC_SETS[0])
        got = blk.work(y)
        assert same_bits(got[:301], r.out[:301]) if mode == g.MODE_GENERIC else np.isfinite(got[:300]).all()
        assert np.isnan(blk.gain()) and np.isnan(r.gain)


def test_refusals(gpu):
    g = gpu
    blk = g.agc_cc(1e-3, 1, 1, 0)
    with pytest.raises(g.GrhipError) as e:
        blk.work(np.zeros(4, np.complex64), -1)
    assert e.value.code == -1
    with pytest.raises(g.GrhipError) as e:
        blk.work_device(16, 0, 0)
    assert e.value.code == -1
    assert len(blk.work(np.zeros(0, np.complex64), 0)) == 0 and blk.gain() == np.float32(1)


def test_host_program(gpu):
    subprocess.check_call(["make", "-C", HOST, "agc_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "agc_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "agc_test ok" in r.stdout, r.stdout + r.stderr
