"""GPU tests of fll_band_edge_cc against the restatement (fll_ref.py, pinned to the reference's own code by
test_fll_band_edge_cpu.py), the float64 recurrence and the recording (ref_fll_band_edge.npz).

  * GENERIC: out, frq, phs, err and the final state bit for bit the restatement on the library's taps;
  * every mode, three drift-free identities on the device's own outputs:
      (a) given err[n] and the state behind n-1, frq[n] and phs[n] are the restatement's Loop.step bit for bit;
      (b) |out[n] - x[n-2fs+1] expj64(phase before that step)| <= 1e-5 peak(x): the family's bound;
      (c) err[n] within 8 (fs+2) 2^-24 S^2 of the float64 band-edge powers of the device's own d, S = sum|tap| max|d|:
          the dot product's forward-error bound carried through the two squared magnitudes.  The last fs - 1 steps of a
          run have no output yet and are left out; nothing else is;
  * every mode: frequency and error within 2 dev_ref + 4 ulp(max_freq) of the float64 recurrence, dev_ref the recording's
    own deviation (fll_ref.DEV_REF, measured by the CPU test).  The phase, a pure integrator, gets no such bound;
  * the QA (gr-digital/python/qa_fll_band_edge.py) with seeds confirmed on the recording;
  * lengths 1, fs-1, fs, fs+1, 63, 64, 65, window-1, window, window+1, 3 window + 37; filter sizes 1, 2, 45, 55, 63, 64,
    65, 129; sps 2, 2.5, 4; rolloff 0, 0.35, 1; 1 and 3 streams; a cut at 4097 and calls of 7 items; setters between
    calls; a signal that drives frequency_limit and phase_wrap; aux outputs NULL."""
import functools
import math
import os

import numpy as np
import pytest

import fll_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "ref_fll_band_edge.npz"))
FS0 = R.SETS[0][3]
LENGTHS = (1, FS0 - 1, FS0, FS0 + 1, 63, 64, 65, R.WIN - 1, R.WIN, R.WIN + 1, 3 * R.WIN + 37)
# filter size, sps, rolloff: every size with one, two and three taps per lane, every sps and rolloff of the issue
SHAPES = ((1, 2.0, 0.35), (2, 2.5, 0.0), (45, 4.0, 0.35), (55, 4.0, 1.0), (63, 2.5, 0.35), (64, 2.0, 0.0), (65, 4.0, 1.0),
          (129, 2.5, 0.35))
SET_IDS = [s[0] for s in R.SETS]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fbits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def modes(g):
    return (g.MODE_GENERIC, g.MODE_FAST, g.MODE_FAST_VALU, g.MODE_FAST_REFTAPS)


@functools.lru_cache(maxsize=None)
def sig(si, seed):
    x = R.signal(seed, R.SETS[si])
    x.setflags(write=False)
    return x


_TAPS, _REF = {}, {}


def taps_of(g, sps, ro, fs):
    k = (float(sps), float(ro), int(fs))
    if k not in _TAPS:
        _TAPS[k] = g.fll_band_edge_taps(*k)
    return _TAPS[k]


def ref_of(g, si, seed):
    """the restatement's and the float64 recurrence's one walk of a whole signal (cuts do not change them)"""
    if (si, seed) not in _REF:
        fset = R.SETS[si]
        f = R.Fll(fset[1], fset[2], fset[3], fset[4], taps_of(g, fset[1], fset[2], fset[3]))
        _REF[(si, seed)] = (f.work(sig(si, seed)), f.work64(sig(si, seed)), f)
    return _REF[(si, seed)]


def make(g, sps, ro, fs, bw, mode, streams=1):
    blk = g.fll_band_edge_cc(sps, ro, fs, bw)
    blk.set_mode(mode)
    if streams != 1:
        blk.set_streams(streams)
    return blk


def make_set(g, si, mode, streams=1):
    fset = R.SETS[si]
    return make(g, fset[1], fset[2], fset[3], fset[4], mode, streams)


def run(blk, xs, cuts=(), aux=True):
    """the streams xs (equal lengths) through blk in calls cut at `cuts`: per output a list with every stream's"""
    n = len(xs[0])
    edges = [0] + [c for c in cuts if 0 < c < n] + [n]
    outs = [[[] for _ in xs] for _ in range(4 if aux else 1)]
    for a, b in zip(edges[:-1], edges[1:]):
        y = blk.work(np.concatenate([x[a:b] for x in xs]), b - a, aux=aux)
        for o, yy in zip(outs, y if aux else (y,)):
            for s in range(len(xs)):
                o[s].append(yy[s * (b - a):(s + 1) * (b - a)])
    return [[np.concatenate(p) for p in o] for o in outs]


def first_diff(a, b):
    d = np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)
    return int(np.argmax(d)) // (2 if a.dtype == np.complex64 else 1) if d.any() else -1


def check_generic(got, k, r, n0=0, n1=None):
    """stream k's four outputs bit for bit the restatement's items n0 .. n1"""
    for name, y in zip(("out", "frq", "phs", "err"), got):
        want = getattr(r, name)[n0:n1]
        assert y[k].shape == want.shape, (name, k, y[k].shape, want.shape)
        assert same_bits(y[k], want), (name, k, first_diff(y[k], want))


def check_identities(x, taps, loop, out, frq, phs, err, phase0=0.0, freq0=0.0):
    """(a), (b), (c) on one stream's whole run from zero histories and the state (phase0, freq0); `loop` holds the gains
    and limits.  Returns the measured (b) and (c) as fractions of their bounds."""
    n, fs = len(x), len(taps[0])
    # (a) the loop's step
    lp = loop
    bad = []
    for i in range(n):
        lp.phase, lp.freq = (R.f32(phase0), R.f32(freq0)) if i == 0 else (phs[i - 1], frq[i - 1])
        lp.step(err[i])
        if fbits(lp.freq) != fbits(frq[i]) or fbits(lp.phase) != fbits(phs[i]):
            bad.append(i)
    assert not bad, ("loop step", bad[:5], len(bad))
    # (b) output n is x[n - 2 fs + 1] turned by the phase before step n - (fs - 1), which is phs of the step before it
    peak = float(np.max(np.abs(x))) if n else 0.0
    before = np.concatenate([[float(R.f32(phase0))], phs[:-1].astype(np.float64)])           # the phase before step j
    want = np.zeros(n, np.complex128)
    if n > 2 * fs - 1:
        j = np.arange(fs, n - (fs - 1))                     # the steps whose sample is an input (xz[j] = x[j - fs]) and is out already
        want[j + fs - 1] = x[j - fs].astype(np.complex128) * np.exp(1j * before[j])
    b_meas = float(np.max(np.abs(out.astype(np.complex128) - want))) if n else 0.0
    assert b_meas <= 1e-5 * peak, ("output against phase", b_meas, peak)
    assert not np.any(out[:min(n, 2 * fs - 1)].view(np.float32))                             # the delay: zeros
    # (c) err against the float64 band-edge powers of the device's own d; d[j] = out[j + fs - 1]
    c_frac = 0.0
    m = n - (fs - 1)                                        # steps whose whole window is out
    if m > 0:
        dz = out.astype(np.complex128)                      # out[0 .. fs-2] are the zeros before the start
        e64 = R.band_edge_error64(taps[0], taps[1], dz)[:m]
        S = float(np.sum(np.abs(taps[0]).astype(np.float64))) * float(np.max(np.abs(dz)))
        tol = 8 * (fs + 2) * 2.0 ** -24 * S * S
        c_meas = float(np.max(np.abs(err[:m].astype(np.float64) - e64)))
        assert c_meas <= tol, ("error against output", c_meas, tol)
        c_frac = c_meas / tol if tol else 0.0
    return (b_meas / (1e-5 * peak) if peak else 0.0), c_frac


# ---- 3: GENERIC bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(R.SETS)), ids=SET_IDS)
def test_generic_three_streams_cut_at_4097(gpu, si):
    g = gpu
    blk = make_set(g, si, g.MODE_GENERIC, 3)
    got = run(blk, [sig(si, s) for s in R.SEEDS], (R.CUT,))
    for k, s in enumerate(R.SEEDS):
        r, _, f = ref_of(g, si, s)
        check_generic(got, k, r)
        assert fbits(blk.get_phase(k)) == fbits(r.phs[-1]) and fbits(blk.get_frequency(k)) == fbits(r.frq[-1])
    assert blk.history() == R.SETS[si][3] + 1


@pytest.mark.parametrize("si", range(len(R.SETS)), ids=SET_IDS)
def test_generic_one_call_and_aux_null(gpu, si):
    g = gpu
    r, _, f = ref_of(g, si, 2)
    blk = make_set(g, si, g.MODE_GENERIC)
    got = run(blk, [sig(si, 2)])
    check_generic(got, 0, r)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        a, b = make_set(g, si, mode), make_set(g, si, mode)
        with_aux, without = run(a, [sig(si, 2)[:2500]], (1300,)), run(b, [sig(si, 2)[:2500]], (1300,), aux=False)
        assert same_bits(with_aux[0][0], without[0][0])
        assert fbits(a.get_phase()) == fbits(b.get_phase()) and fbits(a.get_frequency()) == fbits(b.get_frequency())


def test_generic_calls_of_seven_items(gpu):
    """fs = 55: the delayed tail of an input spans eight calls and more"""
    g = gpu
    n = 7 * 60
    r, _, f = ref_of(g, 0, 1)
    for streams in (1, 3):
        blk = make_set(g, 0, g.MODE_GENERIC, streams)
        seeds = R.SEEDS[:streams]
        got = run(blk, [sig(0, s)[:n] for s in seeds], tuple(range(7, n, 7)))
        for k, s in enumerate(seeds):
            check_generic(got, k, ref_of(g, 0, s)[0], 0, n)
    # the fast form depends on the concatenated input alone too: calls of 7 items against one call, bit for bit
    xs = [sig(0, s)[:n] for s in R.SEEDS]
    one, sevens = make_set(g, 0, g.MODE_FAST, 3), make_set(g, 0, g.MODE_FAST, 3)
    a, b = run(one, xs), run(sevens, xs, tuple(range(7, n, 7)))
    for q in range(4):
        for k in range(3):
            assert same_bits(a[q][k], b[q][k]), (q, k, first_diff(a[q][k], b[q][k]))


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(gpu, n):
    g = gpu
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = make_set(g, 0, mode, 3)
        m = min(70, R.N - n)
        got = run(blk, [sig(0, s)[:n + m] for s in R.SEEDS], (n,))      # a second call carries on from there
        for k, s in enumerate(R.SEEDS):
            if mode == g.MODE_GENERIC:
                r = ref_of(g, 0, s)[0]
                check_generic(got, k, r, 0, n + m)
                assert fbits(blk.get_phase(k)) == fbits(r.phs[n + m - 1]) and fbits(blk.get_frequency(k)) == fbits(r.frq[n + m - 1])
            else:
                fset = R.SETS[0]
                check_identities(sig(0, s)[:n + m], taps_of(g, fset[1], fset[2], fset[3]), R.Loop(fset[1], fset[4]),
                                 *[got[q][k] for q in range(4)])


@pytest.mark.parametrize("shape", SHAPES, ids=["%d-%g-%g" % s for s in SHAPES])
def test_filter_sizes_sps_and_rolloff(gpu, shape):
    g = gpu
    fs, sps, ro = shape
    bw, n = 2 * math.pi / 100, 1300
    taps = taps_of(g, sps, ro, fs)
    xs = [sig(0, s)[:n] for s in R.SEEDS]
    for mode in modes(g):
        blk = make(g, sps, ro, fs, bw, mode, 3)
        assert blk.get_filter_size() == fs and blk.get_samples_per_symbol() == np.float32(sps) and blk.get_rolloff() == np.float32(ro)
        got = run(blk, xs, (R.WIN + 1,))
        for k, s in enumerate(R.SEEDS):
            if mode == g.MODE_GENERIC:
                f = R.Fll(sps, ro, fs, bw, taps)
                check_generic(got, k, f.work(xs[k]))
                assert fbits(blk.get_phase(k)) == fbits(f.loop.phase) and fbits(blk.get_frequency(k)) == fbits(f.loop.freq)
            elif k == 0 or mode == g.MODE_FAST:
                check_identities(xs[k], taps, R.Loop(sps, bw), *[got[q][k] for q in range(4)])


# ---- 4 and 5: every mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(R.SETS)), ids=SET_IDS)
def test_identities_and_float64_contract_in_every_mode(gpu, si):
    g = gpu
    fset = R.SETS[si]
    taps = taps_of(g, fset[1], fset[2], fset[3])
    x = sig(si, 1)
    _, r64, f = ref_of(g, si, 1)
    df, de = R.DEV_REF["%s_s1" % fset[0]]
    bf, be = R.bound(df, f.loop.max_freq), R.bound(de, f.loop.max_freq)
    for mode in modes(g):
        blk = make_set(g, si, mode)
        out, frq, phs, err = [y[0] for y in run(blk, [x], (R.CUT,))]
        b_frac, c_frac = check_identities(x, taps, R.Loop(fset[1], fset[4]), out, frq, phs, err)
        mf = float(np.max(np.abs(frq.astype(np.float64) - r64.frq)))
        me = float(np.max(np.abs(err.astype(np.float64) - r64.err)))
        print("%s mode %d: frequency %.3g of float64 (bound %.3g), error %.3g (bound %.3g), phase %.3g rad (no bound); identity (b) at "
              "%.3g of its bound, (c) at %.3g" % (fset[0], mode, mf, bf, me, be, R.CR.circ(phs, r64.phs), b_frac, c_frac))
        assert mf <= bf and me <= be, (mode, mf, bf, me, be)
        assert fbits(blk.get_phase()) == fbits(phs[-1]) and fbits(blk.get_frequency()) == fbits(frq[-1])


def test_the_limit_signal_limits_and_wraps_on_the_device(gpu):
    g = gpu
    fset = R.SETS[1]
    blk = make_set(g, 1, g.MODE_FAST)
    out, frq, phs, err = [y[0] for y in run(blk, [sig(1, 1)])]
    lp, n = R.Loop(fset[1], fset[4]), len(frq)
    for i in range(n):                      # the restatement's step from the device's own state and error counts them
        if i:
            lp.phase, lp.freq = phs[i - 1], frq[i - 1]
        lp.step(err[i])
    print("limit signal on the device: frequency_limit on %d, phase_wrap trips on %d of %d steps" % (lp.limits, lp.wraps, n))
    assert 0.02 * n <= lp.limits <= 0.10 * n and lp.wraps >= 0.02 * n and lp.remainders == 0
    assert 0.02 * n <= np.count_nonzero(np.abs(frq) == R.max_freq_of(fset[1])) <= 0.10 * n


# ---- 6: the QA -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.QA_SEEDS)
def test_qa_fll_band_edge(gpu, seed):
    g = gpu
    q = R.QA
    rrc = g.firdes_root_raised_cosine(q["sps"], q["sps"], 1.0, q["rolloff"], q["ntaps"])
    assert same_bits(rrc, FIX["rrc_0"].view(np.float32))
    x = R.qa_signal(seed, rrc)
    taps = taps_of(g, q["sps"], q["rolloff"], q["ntaps"])
    f = R.Fll(q["sps"], q["rolloff"], q["ntaps"], q["bw"], taps)
    r64 = f.work64(x)
    df, de = R.DEV_REF["qa_s%d" % seed]
    for mode in modes(g):
        blk = make(g, q["sps"], q["rolloff"], q["ntaps"], q["bw"], mode)
        out, frq, phs, err = blk.work(x, aux=True)
        worst = float(np.max(np.abs(frq[q["skip"]:].astype(np.float64) - q["expect"])))
        mf, me = float(np.max(np.abs(frq.astype(np.float64) - r64.frq))), float(np.max(np.abs(err.astype(np.float64) - r64.err)))
        print("qa seed %d mode %d: max |frq + 0.2| from 700 on = %.3g; frequency %.3g, error %.3g of float64" % (seed, mode, worst, mf, me))
        assert worst <= q["tol"]
        assert mf <= R.bound(df, f.loop.max_freq) and me <= R.bound(de, f.loop.max_freq)
        check_identities(x, taps, R.Loop(q["sps"], q["bw"]), out, frq, phs, err)


# ---- setters ---------------------------------------------------------------------------------------------------------
def test_setters_act_between_calls(gpu):
    g = gpu
    fset = R.SETS[0]
    sps, ro, fs, bw = fset[1:5]
    x = sig(0, 3)
    f = R.Fll(sps, ro, fs, bw, taps_of(g, sps, ro, fs))
    a = f.work(x[:1000])
    f.loop.set_frequency(4.0)               # above the maximum (pi): the MINIMUM
    assert f.loop.freq == -R.max_freq_of(sps)
    f.loop.set_phase(20.0)
    p20 = f.loop.phase
    b = f.work(x[1000:2000])
    f.set_taps(taps_of(g, sps, 0.5, fs))    # set_rolloff: new taps, the histories stay
    c = f.work(x[2000:3000])
    f.loop.alpha, f.loop.beta = R.gains(0.1, 0.5)
    f.set_taps(taps_of(g, sps, 0.5, 129), True)     # set_filter_size: new taps, the histories zeroed, the loop's state stays
    d = f.work(x[3000:4100])
    blk = make(g, sps, ro, fs, bw, g.MODE_GENERIC, 2)
    xs = [x, x[::-1].copy()]
    got = run(blk, [v[:1000] for v in xs])
    check_generic(got, 0, a)
    blk.set_frequency(4.0)
    assert fbits(blk.get_frequency(0)) == fbits(-R.max_freq_of(sps)) == fbits(blk.get_frequency(1))
    blk.set_phase(20.0)
    assert fbits(blk.get_phase(1)) == fbits(p20) and abs(float(p20) - (20.0 - 3 * R.TWOPI)) < 1e-5
    got = run(blk, [v[1000:2000] for v in xs])
    check_generic(got, 0, b)
    blk.set_rolloff(0.5)
    assert blk.get_rolloff() == np.float32(0.5) and blk.get_filter_size() == fs
    got = run(blk, [v[2000:3000] for v in xs])
    check_generic(got, 0, c)
    blk.set_damping_factor(0.5)
    blk.set_loop_bandwidth(0.1)
    assert fbits(blk.get_alpha()) == fbits(f.loop.alpha) and fbits(blk.get_beta()) == fbits(f.loop.beta)
    ph, fr = blk.get_phase(0), blk.get_frequency(0)
    blk.set_filter_size(129)
    assert blk.get_filter_size() == 129 and blk.history() == 130
    assert fbits(blk.get_phase(0)) == fbits(ph) and fbits(blk.get_frequency(0)) == fbits(fr)
    got = run(blk, [v[3000:4100] for v in xs])
    check_generic(got, 0, d)
    assert not np.any(got[0][1][:2 * 129 - 1].view(np.float32))          # the second stream's histories are zeros too
    # set_samples_per_symbol redesigns and leaves the limits alone; refused values change nothing
    blk.set_samples_per_symbol(2.0)
    assert blk.get_samples_per_symbol() == np.float32(2.0)
    blk.set_frequency(100.0)
    assert fbits(blk.get_frequency(0)) == fbits(-R.max_freq_of(sps))
    for bad in (lambda: blk.set_samples_per_symbol(0.0), lambda: blk.set_rolloff(1.5), lambda: blk.set_filter_size(0),
                lambda: blk.set_filter_size(1025), lambda: blk.set_phase(float("inf")), lambda: blk.set_alpha(2.0)):
        with pytest.raises(g.GrhipError) as e:
            bad()
        assert e.value.code == -1
    assert blk.get_samples_per_symbol() == np.float32(2.0) and blk.get_rolloff() == np.float32(0.5) and blk.get_filter_size() == 129


def test_work_device_refuses_partial_aux_and_overlap(gpu):
    import torch
    g = gpu
    blk = make_set(g, 0, g.MODE_FAST)
    n = 256
    x = torch.zeros(n, dtype=torch.complex64, device="cuda")
    out = torch.zeros(n, dtype=torch.complex64, device="cuda")
    f = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(3)]
    for args in ((x, out, f[0], None, None), (x, out, None, f[1], f[2]), (x, x, None, None, None), (x, out, f[0], f[0], f[2]),
                 (x, out, out, f[1], f[2]), (x.data_ptr() + 4, out, None, None, None), (x, out, f[0].data_ptr() + 2, f[1], f[2])):
        with pytest.raises(g.GrhipError) as e:
            blk.work_device(n, *args)
        assert e.value.code == -1
    assert blk.work_device(0, x, out) == 0 and blk.work_device(n, x, out, *f) == 0
    torch.cuda.synchronize()
    assert not bool(out.abs().max() > 0)
