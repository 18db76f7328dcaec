"""constellation_decoder_cb, diff_decoder_bb, map_bb, constellation_receiver_cb and constellation_demod_cb on the device
against the restatement (constellation_ref.py) and the reference's recording (tests/golden/ref_constellation.npz;
test_constellation_cpu.py says what it holds and shows that the recorded cases meet the decision guard).

  * decoder and byte blocks: byte for byte, lengths 1, 63, 64, 65, 4097, one and three streams, a two-dimensional
    constellation, calls cut at an odd item;
  * receiver, GRHIP_MODE_GENERIC: all four outputs and the final state bit for bit the restatement;
  * receiver, every other mode: the recording's symbols, the phase within the deviation contract
    dev <= 2 dev(recording) + 4 ulp(2 pi) against the float64 recurrence, error and frequency within 1e-5 of it; the
    angle form and the cartesian form each asserted through form();
  * constellation_demod_cb: both engines in both modes, byte for byte the library's own blocks in a row and the
    recorded tail, as one call and as two, bits per symbol 1 .. 5.

Measured on an MI355X (printed by the tests, -s): DESIGN.md 4.23."""
import functools

import numpy as np
import pytest

import constellation_ref as R
import test_constellation_cpu as T

pytestmark = pytest.mark.gpu

FIX = T.FIX
CASES = {c[0]: c for c in R.RX_CASES}
CALCDIST = ("calcdist4", lambda: R.Constellation("calcdist", [1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j], [0, 1, 3, 2], 4, 1), 19, 0.02, 0.01)
LENGTHS = (1, 63, 64, 65, 4097)
ANGLE_CASES = ("bpsk", "qpsk", "dqpsk", "8psk", "psk16", "psk32", "limit")


@functools.lru_cache(maxsize=None)
def runs(name):
    """(constellation, signal, float32 restatement as one call, float64 recurrence), computed once per case"""
    if name != "calcdist4":
        c, x, one, _, r64 = T.rx_runs(CASES[name])
        return c, x, one, r64
    c, x = CALCDIST[1](), R.rx_signal(CALCDIST)
    return c, x, R.receiver(R.rx_loop(), c, x), R.receiver64(R.rx_loop(), c, x)


@functools.lru_cache(maxsize=None)
def segments(name, least, step=None):
    """three streams cut from the case's signal, each started from rest, and their float64 recurrences: back to back,
    of the shortest length from `least` on at which every stream meets the decision guard (an unlocked loop's first
    samples may not); or, with `step`, of length `least` and overlapping, the largest distance up to `step` at which
    they do"""
    c, x, _, _ = runs(name)
    for t in range(64):
        m, d = (least, step - t) if step else (least + t, least + t)
        xs = np.stack([x[s * d:][:m] for s in range(3)])
        refs = [R.receiver64(R.rx_loop(), c, xs[s]) for s in range(3)]
        if all(R.guard(c, r.derot) for r in refs):
            return xs, refs
    raise AssertionError("no guarded segment length for %s from %d" % (name, least))


def receiver_for(g, name, mode, streams=1):
    blk = g.constellation_receiver_cb(T.handle(g, runs(name)[0]), R.LOOP_BW, R.FMIN, R.FMAX)
    blk.set_mode(mode)
    if streams != 1:
        blk.set_streams(streams)
    return blk


# ---- decoder and byte blocks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.KINDS)
def test_decoder_equals_the_host_decisions(gpu, name):
    g = gpu
    r = dict(R.DEC_KINDS)[name]()
    h = T.handle(g, r)
    x = T.samples()
    d = r.dimensionality
    want = FIX["dec_" + (name[:-1] + "g" if name.startswith("psk") and name.endswith("n") else name) + "_dec"]
    for mode in (g.MODE_FAST, g.MODE_GENERIC):
        blk = g.constellation_decoder_cb(h)
        blk.set_mode(mode)
        assert blk.work(x).tolist() == want.tolist()
        for n in LENGTHS[:4]:
            assert blk.work(x[100 * d:(100 + n) * d]).tolist() == want[100:100 + n].tolist(), n
    blk = g.constellation_decoder_cb(h)
    blk.set_streams(3)
    n = 4096 // d // 3
    assert blk.work(x[:3 * n * d]).tolist() == want[:3 * n].tolist()


def test_decoder_on_samples_that_are_not_finite(gpu):
    g = gpu
    v = np.array([np.nan, np.inf, -np.inf, 0.0, 1e38, -1e38, 1.0], np.float32)
    x = np.zeros((7, 7), np.complex64)
    x.real, x.imag = v[:, None], v[None, :]
    x = x.reshape(-1)
    for name, make in R.DEC_KINDS:
        r = make()
        h = T.handle(g, r)
        xs = x[:len(x) // r.dimensionality * r.dimensionality]
        assert g.constellation_decoder_cb(h).work(xs).tolist() == h.decision_maker(xs).tolist(), name


@pytest.mark.parametrize("streams", (1, 3))
def test_diff_decoder_and_map(gpu, streams):
    g = gpu
    b = FIX["bytes_in"]
    for m in (1, 2, 3, 4, 7, 8, 16, 100, 255, 256, 1000):
        want = FIX["bytes_diff_%d" % m]
        if streams == 1:
            for n in LENGTHS:
                assert g.diff_decoder_bb(m).work(b[:n]).tolist() == want[:n].tolist(), (m, n)
            blk = g.diff_decoder_bb(m)          # cut at an odd item: the carry
            assert np.concatenate([blk.work(b[:1001]), blk.work(b[1001:1002]), blk.work(b[1002:])]).tolist() == want.tolist(), m
        else:
            n = 1365
            blk = g.diff_decoder_bb(m)
            blk.set_streams(3)
            x = b[:3 * n].reshape(3, n)
            a, c = blk.work(x[:, :701].copy()).reshape(3, -1), blk.work(x[:, 701:].copy()).reshape(3, -1)
            for s in range(3):
                assert np.concatenate([a[s], c[s]]).tolist() == R.diff_decoder(x[s], m).tolist(), (m, s)
    for tag in ("short", "wide", "empty"):
        blk = g.map_bb(FIX["bytes_map_%s_arg" % tag])
        blk.set_streams(streams)
        for n in LENGTHS:
            n -= n % streams
            assert blk.work(b[:n]).tolist() == FIX["bytes_map_" + tag][:n].tolist(), (tag, n)


# ---- the receiver, GENERIC ---------------------------------------------------------------------------------------------
def check_generic(blk, got, r, a, b, floats):
    assert got[0].tolist() == r.sym[a:b].tolist()
    if floats:
        for name, arr in zip(("err", "phase", "freq"), got[1:]):
            assert R.bits(arr).tolist() == R.bits(getattr(r, name)[a:b]).tolist(), name
    assert R.bits(np.array([blk.get_phase(), blk.get_frequency()], np.float32)).tolist() == R.bits(np.array([r.phase[b - 1], r.freq[b - 1]])).tolist()


@pytest.mark.parametrize("name", list(CASES) + ["calcdist4"])
def test_receiver_generic_is_the_restatement(gpu, name):
    g = gpu
    c, x, one, _ = runs(name)
    for floats in (True, False):
        blk = receiver_for(g, name, g.MODE_GENERIC)
        assert blk.form() == blk.FORM_GENERIC
        for a, b in ((0, R.CUT), (R.CUT, R.N)):
            got = blk.work(x[a:b], floats=floats)
            check_generic(blk, got if floats else (got,), one, a, b, floats)


@pytest.mark.parametrize("n", (1, 63, 64, 65, R.WIN - 1, R.WIN, R.WIN + 1))
@pytest.mark.parametrize("name", ("qpsk", "psk16", "rect16"))
def test_receiver_generic_shapes(gpu, name, n):
    g = gpu
    c, x, one, _ = runs(name)
    for floats in (True, False):
        blk = receiver_for(g, name, g.MODE_GENERIC)
        got = blk.work(x[:n], floats=floats)
        check_generic(blk, got if floats else (got,), one, 0, n, floats)


@pytest.mark.parametrize("name", ("8psk", "rect16"))
def test_receiver_generic_three_streams(gpu, name):
    g = gpu
    c, x, _, _ = runs(name)
    n = R.WIN + 37
    xs = x[:3 * n].reshape(3, n)
    refs = [R.receiver(R.rx_loop(), c, xs[s]) for s in range(3)]
    blk = receiver_for(g, name, g.MODE_GENERIC, streams=3)
    sym, err, ph, fr = [a.reshape(3, n) for a in blk.work(xs, floats=True)]
    for s in range(3):
        assert sym[s].tolist() == refs[s].sym.tolist()
        for got, want in ((err[s], refs[s].err), (ph[s], refs[s].phase), (fr[s], refs[s].freq)):
            assert R.bits(got).tolist() == R.bits(want).tolist()
        assert blk.get_phase(s) == refs[s].phase[-1] and blk.get_frequency(s) == refs[s].freq[-1]


def test_setters_between_calls_take_effect(gpu):
    g = gpu
    c, x, _, _ = runs("qpsk")
    blk = receiver_for(g, "qpsk", g.MODE_GENERIC)
    loop = R.rx_loop()
    a = R.receiver(loop, c, x[:500])
    assert blk.work(x[:500]).tolist() == a.sym.tolist()
    blk.set_alpha(0.2); blk.set_beta(0.02); blk.set_frequency(0.05); blk.set_phase(7.5)
    loop.alpha, loop.beta = np.float32(0.2), np.float32(0.02)
    loop.set_frequency(0.05); loop.set_phase(7.5)
    assert blk.get_alpha() == loop.alpha and blk.get_beta() == loop.beta
    assert blk.get_phase() == loop.phase and blk.get_frequency() == loop.freq
    b = R.receiver(loop, c, x[500:1500])
    sym, err, ph, fr = blk.work(x[500:1500], floats=True)
    assert sym.tolist() == b.sym.tolist() and R.bits(ph).tolist() == R.bits(b.phase).tolist() and R.bits(fr).tolist() == R.bits(b.freq).tolist()
    blk.set_frequency(0.3)              # above the maximum gives the minimum (gri_control_loop.cc:126-135)
    assert blk.get_frequency() == np.float32(R.FMIN)
    for bad in (lambda: blk.set_alpha(1.5), lambda: blk.set_beta(-0.1), lambda: blk.set_loop_bandwidth(-1), lambda: blk.set_damping_factor(2),
                lambda: blk.set_phase(float("inf"))):
        with pytest.raises(g.GrhipError):
            bad()
    blk.set_streams(2)                  # restarts every stream
    assert blk.get_phase(1) == 0 and blk.get_frequency(0) == 0


# ---- the receiver, the fast forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES) + ["calcdist4"])
def test_receiver_fast_forms(gpu, name):
    """symbols: the recording's (the float64 recurrence's for calcdist4, which is not recorded; its guard is asserted
    here).  Phase: the deviation contract.  Error and frequency: within 1e-5 of the float64 recurrence's."""
    g = gpu
    c, x, one, r64 = runs(name)
    if name == "calcdist4":
        assert R.guard(c, r64.derot)
        want_sym, dev_ref = r64.sym, R.circ(one.phase, r64.phase)       # the restatement stands in for the recording
    else:
        want_sym, dev_ref = FIX["rx_%s_sym" % name], R.circ(T.f32(FIX["rx_%s_phase" % name]), r64.phase)
    for cuts in (((0, R.N),), ((0, R.CUT), (R.CUT, R.N))):
        blk = receiver_for(g, name, g.MODE_FAST)
        assert blk.form() == (blk.FORM_ANGLE if name in ANGLE_CASES else blk.FORM_CARTESIAN)
        parts = [blk.work(x[a:b], floats=True) for a, b in cuts]
        sym, err, ph, fr = [np.concatenate([p[i] for p in parts]) for i in range(4)]
        dev = R.circ(ph, r64.phase)
        e_max, f_max = np.abs(err.astype(np.float64) - r64.err).max(), np.abs(fr.astype(np.float64) - r64.freq).max()
        print("%s form %d: dev(recording) %.3g dev(device) %.3g bound %.3g; error within %.3g, frequency within %.3g"
              % (name, blk.form(), dev_ref, dev, R.bound(dev_ref), e_max, f_max))
        assert sym.tolist() == want_sym.tolist()
        assert dev <= R.bound(dev_ref)
        assert e_max <= 1e-5 and f_max <= 1e-5
        assert R.circ([blk.get_phase()], [r64.phase[-1]]) <= R.bound(dev_ref)
        # symbols alone give the same symbols
        blk2 = receiver_for(g, name, g.MODE_FAST)
        assert blk2.work(x).tolist() == want_sym.tolist()


@pytest.mark.parametrize("n", (1, 63, 64, 65, R.WIN - 1, R.WIN, R.WIN + 1))
def test_receiver_fast_shapes_and_streams(gpu, n):
    g = gpu
    for name in ("psk16", "rect16"):
        c, x, one, r64 = runs(name)
        blk = receiver_for(g, name, g.MODE_FAST)
        sym, err, ph, fr = blk.work(x[:n], floats=True)
        assert sym.tolist() == r64.sym[:n].tolist()
        assert R.circ(ph, r64.phase[:n]) <= 1e-5 and np.abs(fr - r64.freq[:n]).max() <= 1e-5 and np.abs(err - r64.err[:n]).max() <= 1e-5
        xs, refs = segments(name, n + 36)
        m = xs.shape[1]
        blk = receiver_for(g, name, g.MODE_FAST, streams=3)
        got = blk.work(xs).reshape(3, m)
        for s in range(3):
            assert got[s].tolist() == refs[s].sym.tolist(), (name, s)


def test_receiver_refusals(gpu):
    g = gpu
    q = g.constellation_qpsk()
    blk = g.constellation_receiver_cb(q, R.LOOP_BW, R.FMIN, R.FMAX)
    x = np.ones(8, np.complex64)
    sym, f = np.zeros(8, np.uint8), np.zeros(8, np.float32)
    p = lambda a: a.ctypes.data
    lib = g.lib()
    for err, ph, fr in ((p(f), None, None), (None, p(f), None), (p(f), p(f), None), (None, p(f), p(f))):
        assert lib.grhip_constellation_receiver_cb_work(blk._h, 8, p(x), p(sym), err, ph, fr) == -1
        assert lib.grhip_constellation_receiver_cb_work_device(blk._h, 8, 256, 512, 1024 if err else None, 2048 if ph else None,
                                                               4096 if fr else None, None) == -1
    assert blk.work(x[:0]).size == 0
    with pytest.raises(g.GrhipError):
        g.constellation_receiver_cb(g.constellation_calcdist([1, 1, -1, -1], [], 1, 2), R.LOOP_BW, R.FMIN, R.FMAX)
    with pytest.raises(g.GrhipError):
        g.constellation_calcdist(np.ones(257), [], 1, 1)
    with pytest.raises(g.GrhipError):
        g.diff_decoder_bb(0)


# ---- constellation_demod_cb ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_demod_both_engines_equal_the_blocks_in_a_row_and_the_recording(gpu, name):
    g = gpu
    c, x, _, _ = runs(name)
    h = T.handle(g, c)
    k = c.bits_per_symbol()
    for d in (0, 1):
        for gr in (0, 1):
            want = np.unpackbits(FIX["rx_%s_tail_d%dg%d" % (name, d, gr)])[:R.N * k]
            for mode in (g.MODE_FAST, g.MODE_GENERIC):
                # the library's own blocks in a row
                y = receiver_for(g, name, mode).work(x)
                if d:
                    y = g.diff_decoder_bb(c.arity).work(y)
                if gr and c.apply_pre_diff_code:
                    y = g.map_bb(R.invert_code(c.pre_diff_code)).work(y)
                row = g.unpack_k_bits_bb(k).work(len(y) * k, y)
                assert row.tolist() == want.tolist(), (d, gr, mode)
                for engine in (0, 1):
                    for cuts in (((0, R.N),), ((0, R.CUT), (R.CUT, R.N))):
                        blk = g.constellation_demod_cb(h, R.LOOP_BW, R.FMIN, R.FMAX, d, gr)
                        assert blk.engine() == 1 and blk.bits_per_symbol() == k
                        blk.set_mode(mode)
                        blk.set_engine(engine)
                        assert blk.engine() == engine
                        got = np.concatenate([blk.work(x[a:b]) for a, b in cuts])
                        assert got.tolist() == want.tolist(), (d, gr, mode, engine, cuts)


def test_demod_streams_shapes_and_engine_switch(gpu):
    g = gpu
    for name in ("8psk", "psk32", "qpsk"):
        c, x, _, _ = runs(name)
        h, k = T.handle(g, c), c.bits_per_symbol()
        for least in (1, 63, 64, 65, R.WIN + 1):
            xs, refs = segments(name, least)
            n = xs.shape[1]
            want = [R.demod_tail(c, refs[s].sym, True, True) for s in range(3)]
            for engine in (0, 1):
                blk = g.constellation_demod_cb(h, R.LOOP_BW, R.FMIN, R.FMAX, True, True)
                blk.set_streams(3)
                blk.set_engine(engine)
                got = blk.work(xs).reshape(3, n * k)
                for s in range(3):
                    assert got[s].tolist() == want[s].tolist(), (name, n, engine, s)
        # the engine changes between calls: the previous symbol is one state
        want = np.unpackbits(FIX["rx_%s_tail_d1g1" % name])[:R.N * k]
        blk = g.constellation_demod_cb(h, R.LOOP_BW, R.FMIN, R.FMAX, True, True)
        parts = []
        for i, (a, b) in enumerate(((0, 999), (999, 1000), (1000, R.CUT), (R.CUT, R.N))):
            blk.set_engine(i % 2)
            parts.append(blk.work(x[a:b]))
        assert np.concatenate(parts).tolist() == want.tolist(), name
