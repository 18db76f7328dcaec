"""GPU tests of costas_loop_cc, pll_freqdet_cf, pll_refout_cc and pll_carriertracking_cc against the restatement
(carrier_ref.py, pinned to the reference's own code by test_carrier_cpu.py) and the recording (ref_carrier.npz).

  * the three PLLs: phase, frequency and pll_freqdet_cf's output bit for bit the restatement's in every mode; the outputs
    that carry a sine or cosine within the CPU test's bounds of the RECORDING (one float ulp of the component for
    pll_refout_cc, 4 * 2^-24 (|re| + |im|) for pll_carriertracking_cc, 2^-19 for the lock signal), squelch decisions the
    reference's;
  * Costas GENERIC: out, freq_out and state bit for bit the restatement with the float-rounded double sine and cosine;
  * Costas in the other modes: outputs within 1e-5 of the input's peak of the float64 recurrence on the same input, the
    frequency output within 1e-5 rad/sample;
  * lengths 1, 63, 64, 65, window - 1, window, window + 1 and 3 window + 37 (a partial group, a partial window, the
    prefetch past the end), 1 and 3 streams, state carried over a cut at 4097, setters between calls, freq_out NULL."""
import functools
import os

import numpy as np
import pytest

import carrier_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "ref_carrier.npz"))
LOCK_DEV = 2.0 ** -19
LENGTHS = (1, 63, 64, 65, R.WIN - 1, R.WIN, R.WIN + 1, 3 * R.WIN + 37)
PLL_BLOCKS = ("pll_freqdet_cf", "pll_refout_cc", "pll_carriertracking_cc")
PLL_IDS = [p[0] for p in R.PLL_SETS]
COSTAS_IDS = [c[0] for c in R.COSTAS_SETS]


def secs(a):
    return np.concatenate([a[s:s + R.SEC_LEN] for s in R.SECTIONS])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fbits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


@functools.lru_cache(maxsize=None)
def pll_sig(pi, seed):
    x = R.pll_signal(seed, R.PLL_SETS[pi])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pll_ref(pi, seed):
    """the restatement's one walk of the whole signal (cuts do not change it)"""
    return R.pll(R.pll_loop(R.PLL_SETS[pi]), pll_sig(pi, seed))


@functools.lru_cache(maxsize=None)
def cos_sig(ci, seed):
    x = R.costas_signal(seed, R.COSTAS_SETS[ci])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def cos_ref(ci, seed):
    cs = R.COSTAS_SETS[ci]
    return R.costas(R.costas_loop(cs), cos_sig(ci, seed), cs[1]), R.costas64(R.costas_loop(cs), cos_sig(ci, seed), cs[1])


def make_pll(g, block, ps, mode, streams=1):
    blk = getattr(g, block)(ps[1], ps[2], ps[3])
    blk.set_mode(mode)
    if streams != 1:
        blk.set_streams(streams)
    return blk


def make_costas(g, cs, mode, streams=1):
    blk = g.costas_loop_cc(cs[2], cs[1])
    blk.set_mode(mode)
    if streams != 1:
        blk.set_streams(streams)
    if cs[6] is not None:
        blk.set_frequency(cs[6])
    return blk


def run(blk, xs, cuts=(), **kw):
    """the streams xs (equal lengths) through blk in calls cut at `cuts`; returns every stream's outputs (a tuple of
    lists where work returns a tuple)"""
    n = len(xs[0])
    edges = [0] + [c for c in cuts if 0 < c < n] + [n]
    outs = None
    for a, b in zip(edges[:-1], edges[1:]):
        y = blk.work(np.concatenate([x[a:b] for x in xs]), b - a, **kw)
        ys = y if isinstance(y, tuple) else (y,)
        if outs is None:
            outs = [[[] for _ in xs] for _ in ys]
        for o, yy in zip(outs, ys):
            for s in range(len(xs)):
                o[s].append(yy[s * (b - a):(s + 1) * (b - a)])
    res = [[np.concatenate(p) for p in o] for o in outs]
    return res if len(res) > 1 else res[0]


def check_pll_output(block, got, r, x, n=None):
    """one stream's output against the restatement's first n items"""
    n = len(got) if n is None else n
    if block == "pll_freqdet_cf":
        assert same_bits(got, r.freqdet[:n])
    elif block == "pll_refout_cc":
        want = r.refout[:n]
        for a, b in ((got.real, want.real), (got.imag, want.imag)):
            assert np.all(np.abs(a.astype(np.float64) - b) <= np.spacing(np.abs(b)))
    else:
        want = r.ct[:n]
        tol = 4 * 2.0 ** -24 * (np.abs(x[:n].real).astype(np.float64) + np.abs(x[:n].imag))
        assert np.all(np.abs(got.real.astype(np.float64) - want.real) <= tol)
        assert np.all(np.abs(got.imag.astype(np.float64) - want.imag) <= tol)


def check_pll_state(blk, k, r, n):
    assert fbits(blk.get_phase(k)) == fbits(r.phases[n]) and fbits(blk.get_frequency(k)) == fbits(r.freqs[n])


# ---- the three PLLs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", range(len(R.PLL_SETS)), ids=PLL_IDS)
@pytest.mark.parametrize("block", PLL_BLOCKS)
def test_pll_three_streams_cut_at_4097(gpu, block, pi):
    g = gpu
    ps = R.PLL_SETS[pi]
    blk = make_pll(g, block, ps, g.MODE_GENERIC, 3)
    got = run(blk, [pll_sig(pi, s) for s in R.SEEDS], (R.CUT,))
    worst = 0.0
    for k, s in enumerate(R.SEEDS):
        r, x = pll_ref(pi, s), pll_sig(pi, s)
        key = "pll_%s_s%d_" % (ps[0], s)
        check_pll_state(blk, k, r, R.N)
        assert [fbits(blk.get_phase(k)), fbits(blk.get_frequency(k))] == FIX[key + "state"].tolist()
        check_pll_output(block, got[k], r, x)
        # and the CPU test's bounds against the recording
        if block == "pll_refout_cc":
            want, mine = FIX[key + "refout_sec"].view(np.complex64), secs(got[k])
            for a, b in ((mine.real, want.real), (mine.imag, want.imag)):
                assert np.all(np.abs(a.astype(np.float64) - b) <= np.spacing(np.abs(b)))
        if block == "pll_carriertracking_cc":
            want, mine, xs = FIX[key + "ct_sec"].view(np.complex64), secs(got[k]), secs(x)
            tol = 4 * 2.0 ** -24 * (np.abs(xs.real).astype(np.float64) + np.abs(xs.imag))
            assert np.all(np.abs(mine.real.astype(np.float64) - want.real) <= tol)
            assert np.all(np.abs(mine.imag.astype(np.float64) - want.imag) <= tol)
            dev = abs(float(blk.locksig(k)) - float(FIX[key + "lock_final"].view(np.float32)[0]))
            worst = max(worst, dev)
            assert dev <= LOCK_DEV
            assert blk.lock_detector(k) == (abs(float(blk.locksig(k))) > 0.0)
    if block == "pll_carriertracking_cc":
        print("%s: final lock signal deviates from the recording by at most %.3g" % (ps[0], worst))


@pytest.mark.parametrize("pi", range(len(R.PLL_SETS)), ids=PLL_IDS)
def test_pll_one_stream_one_call_in_every_mode(gpu, pi):
    g = gpu
    ps, x, r = R.PLL_SETS[pi], pll_sig(pi, 2), pll_ref(pi, 2)
    for mode in (g.MODE_GENERIC, g.MODE_FAST, g.MODE_FAST_VALU, g.MODE_FAST_REFTAPS):
        for block in PLL_BLOCKS if mode in (g.MODE_GENERIC, g.MODE_FAST) else PLL_BLOCKS[:1]:
            blk = make_pll(g, block, ps, mode)
            got = run(blk, [x])[0]
            check_pll_state(blk, 0, r, R.N)
            check_pll_output(block, got, r, x)


@pytest.mark.parametrize("n", LENGTHS)
def test_pll_lengths(gpu, n):
    g = gpu
    pi = 1          # "wrap"
    for block in PLL_BLOCKS:
        blk = make_pll(g, block, R.PLL_SETS[pi], g.MODE_FAST, 3)
        got = run(blk, [pll_sig(pi, s)[:n] for s in R.SEEDS])
        for k, s in enumerate(R.SEEDS):
            check_pll_state(blk, k, pll_ref(pi, s), n)
            check_pll_output(block, got[k], pll_ref(pi, s), pll_sig(pi, s), n)
        # a second call carries on from there
        m = min(70, R.N - n)
        got = run(blk, [pll_sig(pi, s)[n:n + m] for s in R.SEEDS])
        for k, s in enumerate(R.SEEDS):
            check_pll_state(blk, k, pll_ref(pi, s), n + m)
            if block == "pll_freqdet_cf":
                assert same_bits(got[k], pll_ref(pi, s).freqdet[n:n + m])


def test_pll_setters_act_between_calls(gpu):
    g = gpu
    pi = 0
    ps, x = R.PLL_SETS[pi], pll_sig(pi, 3)
    loop = R.pll_loop(ps)
    a = R.pll(loop, x[:2000])
    loop.alpha, loop.beta = R.gains(0.1, 0.5)
    loop.set_frequency(1.5)             # above the maximum: the MINIMUM
    assert loop.freq == np.float32(-1.0)
    loop.set_phase(100.0)
    b = R.pll(loop, x[2000:3100])
    loop.alpha, loop.beta = np.float32(0.25), np.float32(0.0625)
    loop.set_frequency(0.25)
    c = R.pll(loop, x[3100:])
    want = R.join([a, b, c])
    for block in PLL_BLOCKS:
        blk = make_pll(g, block, ps, g.MODE_GENERIC)
        got = [blk.work(x[:2000])]
        blk.set_damping_factor(0.5)
        blk.set_loop_bandwidth(0.1)
        assert fbits(blk.get_alpha()) == fbits(R.gains(0.1, 0.5)[0]) and fbits(blk.get_beta()) == fbits(R.gains(0.1, 0.5)[1])
        assert blk.get_loop_bandwidth() == np.float32(0.1) and blk.get_damping_factor() == np.float32(0.5)
        blk.set_frequency(1.5)
        assert blk.get_frequency() == np.float32(-1.0)
        blk.set_phase(100.0)
        assert fbits(blk.get_phase()) == fbits(b.phases[0])
        got.append(blk.work(x[2000:3100]))
        blk.set_alpha(0.25)
        blk.set_beta(0.0625)
        blk.set_frequency(0.25)
        got.append(blk.work(x[3100:]))
        check_pll_state(blk, 0, want, R.N)
        check_pll_output(block, np.concatenate(got), want, x)
        for bad in (lambda: blk.set_loop_bandwidth(-1.0), lambda: blk.set_damping_factor(1.5), lambda: blk.set_alpha(2.0),
                    lambda: blk.set_beta(-0.5), lambda: blk.set_phase(float("inf")), lambda: blk.set_phase(2.0 ** 21)):
            with pytest.raises(g.GrhipError) as e:
                bad()
            assert e.value.code == -1
        check_pll_state(blk, 0, want, R.N)          # a refusal changes nothing
        assert blk.get_alpha() == np.float32(0.25) and blk.get_beta() == np.float32(0.0625)


@pytest.mark.parametrize("pi", range(len(R.PLL_SETS)), ids=PLL_IDS)
def test_squelch_decisions_are_the_references(gpu, pi):
    g = gpu
    ps, x = R.PLL_SETS[pi], pll_sig(pi, 1)
    key = "pll_%s_s1_" % ps[0]
    thr = FIX[key + "sq_thr"].view(np.float32)[0]
    zero = np.unpackbits(FIX[key + "sq_zero"])[:R.N].astype(bool)
    blk = make_pll(g, "pll_carriertracking_cc", ps, g.MODE_FAST)
    assert blk.set_lock_threshold(thr) == float(thr) and blk.squelch_enable(True) is True
    got = run(blk, [x], (R.CUT,))[0]
    assert np.array_equal(got == 0, zero)
    want, xs = FIX[key + "sq_sec"].view(np.complex64), secs(x)
    tol = 4 * 2.0 ** -24 * (np.abs(xs.real).astype(np.float64) + np.abs(xs.imag))
    assert np.all(np.abs(secs(got).real.astype(np.float64) - want.real) <= tol)
    assert np.all(np.abs(secs(got).imag.astype(np.float64) - want.imag) <= tol)
    full = FIX[key + "lock_full"].view(np.float32)
    assert abs(float(blk.locksig()) - float(full[-1])) <= LOCK_DEV
    assert blk.lock_detector() == bool(abs(full[-1]) > thr)


# ---- Costas ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(R.COSTAS_SETS)), ids=COSTAS_IDS)
def test_costas_generic_is_the_restatement_bit_for_bit(gpu, ci):
    g = gpu
    cs = R.COSTAS_SETS[ci]
    blk = make_costas(g, cs, g.MODE_GENERIC, 3)
    out, freq = run(blk, [cos_sig(ci, s) for s in R.SEEDS], (R.CUT,), freq=True)
    for k, s in enumerate(R.SEEDS):
        r = cos_ref(ci, s)[0]
        diff = np.flatnonzero(out[k].view(np.uint32) != r.out.view(np.uint32))
        assert diff.size == 0, "seed %d: first differing float %d of %d" % (s, diff[0], diff.size)
        assert same_bits(freq[k], r.freq)
        assert fbits(blk.get_phase(k)) == fbits(r.phases[-1]) and fbits(blk.get_frequency(k)) == fbits(r.freq[-1])
    # one stream, one call, no frequency output: the same out
    one = make_costas(g, cs, g.MODE_GENERIC)
    assert same_bits(run(one, [cos_sig(ci, 2)])[0], cos_ref(ci, 2)[0].out)


@pytest.mark.parametrize("ci", range(len(R.COSTAS_SETS)), ids=COSTAS_IDS)
def test_costas_fast_is_within_1e5_of_the_float64_recurrence(gpu, ci):
    g = gpu
    cs = R.COSTAS_SETS[ci]
    worst_o = worst_f = 0.0
    for mode, streams, cuts in ((g.MODE_FAST, 3, (R.CUT,)), (g.MODE_FAST_VALU, 1, ()), (g.MODE_FAST_REFTAPS, 1, ())):
        seeds = R.SEEDS[:streams]
        blk = make_costas(g, cs, mode, streams)
        out, freq = run(blk, [cos_sig(ci, s) for s in seeds], cuts, freq=True)
        for k, s in enumerate(seeds):
            r64 = cos_ref(ci, s)[1]
            peak = float(np.abs(cos_sig(ci, s)).max())
            eo = float(np.abs(out[k] - r64.out).max()) / peak
            ef = float(np.abs(freq[k].astype(np.float64) - r64.freq).max())
            worst_o, worst_f = max(worst_o, eo), max(worst_f, ef)
            assert eo <= 1e-5 and ef <= 1e-5, (cs[0], mode, s, eo, ef)
            assert R.circ([blk.get_phase(k)], [r64.phases[-1]]) <= 1e-5
    print("%s: outputs within %.3g of the peak, frequency within %.3g rad/sample of the float64 recurrence" % (cs[0], worst_o, worst_f))
    # freq_out NULL and non-NULL give the same out
    a, b = make_costas(g, cs, g.MODE_FAST), make_costas(g, cs, g.MODE_FAST)
    assert same_bits(run(a, [cos_sig(ci, 1)], (R.CUT,))[0], run(b, [cos_sig(ci, 1)], (R.CUT,), freq=True)[0][0])


@pytest.mark.parametrize("n", LENGTHS)
def test_costas_lengths(gpu, n):
    g = gpu
    for ci in (1, 2):           # "qpsk", "8psk"
        cs = R.COSTAS_SETS[ci]
        blk = make_costas(g, cs, g.MODE_GENERIC, 3)
        out, freq = run(blk, [cos_sig(ci, s)[:n] for s in R.SEEDS], freq=True)
        m = min(70, R.N - n)
        out2 = run(blk, [cos_sig(ci, s)[n:n + m] for s in R.SEEDS])
        for k, s in enumerate(R.SEEDS):
            r = cos_ref(ci, s)[0]
            assert same_bits(out[k], r.out[:n]) and same_bits(freq[k], r.freq[:n]) and same_bits(out2[k], r.out[n:n + m])
            assert fbits(blk.get_phase(k)) == fbits(r.phases[n + m]) and fbits(blk.get_frequency(k)) == fbits(r.freq[n + m - 1])
        fast = make_costas(g, cs, g.MODE_FAST, 3)
        out = run(fast, [cos_sig(ci, s)[:n] for s in R.SEEDS])
        for k, s in enumerate(R.SEEDS):
            assert np.abs(out[k] - cos_ref(ci, s)[1].out[:n]).max() <= 1e-5 * np.abs(cos_sig(ci, s)).max()


def test_costas_setters_act_between_calls(gpu):
    g = gpu
    ci = 0
    cs, x = R.COSTAS_SETS[ci], cos_sig(ci, 2)
    loop = R.costas_loop(cs)
    a = R.costas(loop, x[:1500], 2)
    loop.alpha, loop.beta = R.gains(0.02)
    loop.set_phase(-7.0)
    loop.set_frequency(-1.5)            # below the minimum: the MAXIMUM
    b = R.costas(loop, x[1500:], 2)
    blk = make_costas(g, cs, g.MODE_GENERIC)
    got = [blk.work(x[:1500])]
    blk.set_loop_bandwidth(0.02)
    blk.set_phase(-7.0)
    blk.set_frequency(-1.5)
    assert blk.get_frequency() == np.float32(1.0) and fbits(blk.get_phase()) == fbits(b.phases[0])
    got.append(blk.work(x[1500:]))
    assert same_bits(np.concatenate(got), np.concatenate([a.out, b.out]))
    assert fbits(blk.get_phase()) == fbits(b.phases[-1]) and fbits(blk.get_frequency()) == fbits(b.freq[-1])
    # set_streams restarts every stream from zero
    blk.set_streams(2)
    assert blk.get_phase(1) == 0 and blk.get_frequency(0) == 0
    with pytest.raises(g.GrhipError):
        blk.get_phase(2)
