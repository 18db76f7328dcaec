"""trellis_viterbi_X, trellis_encoder_XX, trellis_metrics_X and trellis_constellation_metrics_cf on the device, byte for
byte (floats bit for bit) against the restatement of tests/trellis_ref.py, which tests/test_trellis_cpu.py pins to the
reference's recording.  The shapes are the smallest at which each path of the kernels can go wrong; the sizes that
depend on the handle (trace window, blocks per wavefront, resident blocks) come from its accessors."""
import functools

import numpy as np
import pytest

import trellis_ref as tr

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def extra_fsm(name):
    """restated FSMs beyond the recorded ones: long predecessor lists, and a state that nothing leads to"""
    if name == "radix3":                             # S = 4, Pmax = 8: the predecessor table is walked out of LDS
        return tr.fsm_from_radix(tr.make_fsm("awgn1o2_4"), 3)
    if name == "radix5_64":                          # S = 64, Pmax = 32, O = 1024: the table stays in device memory
        return tr.fsm_from_radix(tr.make_fsm("gen_133_171"), 5)
    assert name == "orphan"                          # nothing leads to state 0
    return tr.Fsm(2, 3, 2, [1, 2, 1, 2, 2, 1], [0, 1, 1, 0, 0, 1])


def ref_fsm(name):
    return tr.make_fsm(name) if name in tr.FSM_SPECS else extra_fsm(name)


def lib_fsm(g, name):
    if name in tr.FSM_SPECS:
        return tr.lib_fsm(g, name)
    return g.fsm(*ref_fsm(name).tables())


@functools.lru_cache(maxsize=None)
def reference(name, K, nblocks, S0, SK, kind, seed, ot):
    f = ref_fsm(name)
    m = tr.viterbi_input(f, kind, K, nblocks, seed)
    m.setflags(write=False)
    out, dead = tr.viterbi(f, K, S0, SK, m, tr.OUT_DTYPES[ot])
    out.setflags(write=False)
    return m, out, dead


def decoder(g, ot):
    return {"b": g.trellis_viterbi_b, "s": g.trellis_viterbi_s, "i": g.trellis_viterbi_i}[ot]


def size_of(blk, spec):
    """a K or a block count given by the handle: "tw-1", "tw", "tw+1", "3tw+5", "g-1", "g+1", "res+1" or a number"""
    if not isinstance(spec, str):
        return spec
    tw, gpw, res = blk.trace_window(), blk.blocks_per_wavefront(), blk.resident_blocks()
    return {"tw-1": tw - 1, "tw": tw, "tw+1": tw + 1, "3tw+5": 3 * tw + 5, "g-1": max(gpw - 1, 1), "g+1": gpw + 1, "res+1": res + 1}[spec]


# (fsm, K, blocks, streams, S0, SK, input, output type)
DECODER_CASES = [
    # S = 1: every lane is its own block
    ("rep2", 63, "g+1", 1, 0, -1, "euclid", "b"), ("nothing", 64, "g-1", 1, -1, -1, "quant", "b"), ("rep2", "tw+1", 3, 1, 0, -1, "quant", "b"),
    # S = 3: 21 blocks per wavefront and a spare lane; Pmax = 3, two decision bits
    ("isi_3_2", 65, "g+1", 1, 0, -1, "euclid", "b"), ("isi_3_2", 64, "g-1", 1, -1, 2, "quant", "b"), ("isi_3_2", "tw-1", 2, 1, 0, -1, "hard", "b"),
    ("isi_3_2", "tw", 2, 1, 0, -1, "quant", "s"), ("isi_3_2", "tw+1", 2, 1, -1, -1, "quant", "b"), ("isi_3_2", "3tw+5", 22, 1, 0, 0, "special", "i"),
    # S = 4, Pmax = 2: the ballot is the decision word
    ("awgn1o2_4", 1, 1, 1, -1, -1, "quant", "b"), ("awgn1o2_4", 2, "g-1", 1, 0, -1, "quant", "b"), ("awgn1o2_4", 63, "g+1", 1, 0, -1, "euclid", "b"),
    ("awgn1o2_4", 64, 17, 3, 0, 0, "hard", "b"), ("awgn1o2_4", 65, 17, 3, 3, 2, "quant", "s"), ("awgn1o2_4", 64, 1, 1, -1, -1, "zeros", "i"),
    ("awgn1o2_4", "tw-1", 2, 1, 0, -1, "quant", "b"), ("awgn1o2_4", "tw", 2, 1, 0, -1, "hard", "b"), ("awgn1o2_4", "tw+1", 2, 1, 3, 2, "quant", "b"),
    ("awgn1o2_4", "3tw+5", 17, 1, 0, -1, "special", "b"), ("awgn1o2_4", 2, "res+1", 1, -1, -1, "quant", "b"),
    # S = 16, Pmax = 4
    ("awgn2o3_16", 65, "g+1", 1, 0, -1, "euclid", "b"), ("awgn2o3_16", "tw+1", 3, 1, -1, -1, "special", "b"), ("awgn2o3_16", 64, 17, 3, 3, 2, "quant", "i"),
    # S = 64: exactly one wavefront
    ("gen_133_171", 64, 1, 1, 0, -1, "euclid", "b"), ("gen_133_171", 65, 3, 1, -1, -1, "quant", "s"), ("gen_133_171", "tw+1", 2, 1, 3, 2, "special", "b"),
    ("gen_133_171", 2, "res+1", 1, 0, -1, "quant", "b"),
    # S = 128: two wavefronts and a barrier
    ("awgn1o2_128", 65, 1, 1, 0, -1, "euclid", "b"), ("awgn1o2_128", 63, 17, 3, -1, -1, "quant", "b"), ("awgn1o2_128", "tw-1", 2, 1, 0, 0, "hard", "b"),
    ("awgn1o2_128", "tw", 2, 1, 3, 2, "quant", "s"), ("awgn1o2_128", "tw+1", 2, 1, 0, -1, "quant", "b"), ("awgn1o2_128", "3tw+5", 3, 1, -1, -1, "special", "i"),
    ("awgn1o2_128", 2, "res+1", 1, 0, -1, "quant", "b"),
    # S = 1024: the largest workgroup; O = 2048 leaves a metric window of two steps
    ("isi_2_11", 32, 2, 1, 0, -1, "quant", "b"), ("isi_2_11", 32, 1, 1, -1, -1, "special", "b"),
    # predecessor lists of 3 and 1 (padded rounds), of 1 everywhere (no decision bit), a disconnected FSM
    ("irregular", 64, "g+1", 1, -1, -1, "quant", "b"), ("irregular", 65, 17, 3, 0, -1, "special", "b"), ("irregular", "tw+1", 2, 1, 1, -1, "hard", "b"),
    ("disconnected", 20, 17, 1, -1, -1, "quant", "b"), ("simple", 20, 17, 3, 1, -1, "zeros", "b"), ("disconnected", 1500, 2, 1, 2, -1, "special", "b"),
    # long lists: the table walked out of LDS, and out of device memory with a one-step window
    ("radix3", 65, "g+1", 1, 0, -1, "quant", "b"), ("radix3", "tw+1", 2, 1, -1, -1, "special", "s"), ("radix5_64", 20, 2, 1, 0, -1, "quant", "i"),
    ("joint", 64, 9, 1, -1, -1, "quant", "b"), ("cpm_2_4_2", 64, 9, 1, 0, -1, "euclid", "b"), ("radix2", 64, 17, 1, 0, -1, "hard", "b"),
    # a state that nothing leads to, as S0: the traceback never stands in it
    ("orphan", 64, 22, 1, 0, -1, "quant", "b"),
]


@pytest.mark.parametrize("case", DECODER_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_viterbi_equals_the_restatement(gpu, case):
    g = gpu
    name, K, blocks, streams, S0, SK, kind, ot = case
    f = lib_fsm(g, name)
    probe = decoder(g, ot)(f, 1, S0, SK)
    K = size_of(probe, K)
    blk = decoder(g, ot)(f, K, S0, SK)
    blocks = size_of(blk, blocks)
    assert (blk.K(), blk.S0(), blk.SK()) == (K, S0, SK)
    tw = blk.trace_window()
    assert (blk.workspace_bytes() > 0) == (K > tw)
    blk.set_streams(streams)
    m, ref, dead = reference(name, K, blocks * streams, S0, SK, kind, 1000 + len(name) + K % 97, ot)
    assert dead == 0
    for mode in (g.MODE_FAST, g.MODE_GENERIC):
        blk.set_mode(mode)
        got = blk.work(m)
        assert got.dtype == ref.dtype and len(got) == len(ref)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, "mode %d: %d of %d symbols differ, the first at %d (block %d, step %d)" % (
            mode, bad.size, len(ref), bad[0], bad[0] // K, bad[0] % K)
    assert blk.dead_ends() == 0


def test_all_zero_metrics_take_the_first_predecessor(gpu):
    """every comparison ties: the first predecessor wins everywhere and the path ends in state 0"""
    g = gpu
    f = tr.make_fsm("awgn1o2_4")
    blk = g.trellis_viterbi_b(tr.lib_fsm(g, "awgn1o2_4"), 33, -1, -1)
    out = blk.work(np.zeros(33 * 4 * 5, np.float32)).reshape(5, 33)
    st, want = 0, np.zeros(33, np.uint8)
    for k in range(32, -1, -1):
        want[k] = f.PI[st][0]
        st = f.PS[st][0]
    assert np.array_equal(out, np.tile(want, (5, 1)))


def test_dead_ends(gpu):
    """where the traceback stands in a state without predecessors: symbol 0, the state stays, the event is counted"""
    g = gpu
    f, lf = extra_fsm("orphan"), lib_fsm(g, "orphan")
    K, nblocks = 16, 22
    # SK on the orphan: every step of every block
    m = tr.viterbi_input(f, "quant", K, nblocks, 5)
    blk = g.trellis_viterbi_b(lf, K, -1, 0)
    ref, dead = tr.viterbi(f, K, -1, 0, m)
    assert dead == K * nblocks
    assert np.array_equal(blk.work(m), ref) and not ref.any() and blk.dead_ends() == dead
    # metrics of 1e9 everywhere: nothing is below INF, every alpha is INF - INF = 0 and the first minimum is state 0
    m = np.full(K * nblocks * f.O, 1e9, np.float32)
    m[:K * f.O] = tr.viterbi_input(f, "quant", K, 1, 6)              # the first block is an ordinary one
    for mode in (g.MODE_FAST, g.MODE_GENERIC):
        blk = g.trellis_viterbi_s(lf, K, -1, -1)
        blk.set_mode(mode)
        ref, dead = tr.viterbi(f, K, -1, -1, m, np.int16)
        assert dead == K * (nblocks - 1) and ref[:K].any()
        assert np.array_equal(blk.work(m), ref) and blk.dead_ends() == dead
        assert np.array_equal(blk.work(m), ref) and blk.dead_ends() == 2 * dead         # it adds up over the handle's life


def test_viterbi_refusals_and_accessors(gpu):
    g = gpu
    f4 = tr.lib_fsm(g, "awgn1o2_4")
    for make in (lambda: g.trellis_viterbi_b(f4, 0, 0, -1), lambda: g.trellis_viterbi_b(f4, -5, 0, -1), lambda: g.trellis_viterbi_b(f4, 8, 4, -1),
                 lambda: g.trellis_viterbi_s(f4, 8, 0, 4), lambda: g.trellis_viterbi_i(g.fsm(2, 12), 8, 0, -1),
                 lambda: g.trellis_viterbi_b(tr.lib_fsm(g, "isi_2_11"), 1 << 20, 0, -1)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1
    blk = g.trellis_viterbi_b(f4, 8, -7, -1)
    assert (blk.S0(), blk.SK()) == (-1, -1) and blk.blocks_per_wavefront() == 16 and blk.resident_blocks() % 16 == 0
    assert blk.trace_window() >= 64 and blk.workspace_bytes() == 0
    with pytest.raises(g.GrhipError):
        blk.work(np.zeros(4 * 12, np.float32), 12)                  # n is no multiple of K
    assert len(blk.work(np.zeros(0, np.float32), 0)) == 0
    assert g.trellis_viterbi_b(tr.lib_fsm(g, "disconnected"), 8, 0, -1).trace_window() == INT_MAX
    long_k = g.trellis_viterbi_b(f4, 4 * blk.trace_window(), 0, -1)
    assert long_k.workspace_bytes() == long_k.resident_blocks() // 16 * 4 * blk.trace_window() * 8     # by the resident blocks


# ---- encoder -----------------------------------------------------------------------------------------------------------
ENCODERS = {"bb": "trellis_encoder_bb", "bs": "trellis_encoder_bs", "bi": "trellis_encoder_bi", "ss": "trellis_encoder_ss",
            "si": "trellis_encoder_si", "ii": "trellis_encoder_ii"}


@pytest.mark.parametrize("case", tr.ENCODER_CASES, ids=lambda c: tr.case_key("enc", c))
def test_encoder_against_the_recording(gpu, case):
    g = gpu
    name, sig, n, st, seed = case
    f = tr.make_fsm(name)
    x = np.random.RandomState(seed).randint(0, f.I, n).astype(tr.OUT_DTYPES[sig[0]])
    for mode in (g.MODE_FAST, g.MODE_GENERIC):
        blk = getattr(g, ENCODERS[sig])(tr.lib_fsm(g, name), st)
        blk.set_mode(mode)
        out = blk.work(x)
        assert out.dtype == tr.OUT_DTYPES[sig[1]] and tr.matches(tr.case_key("enc", case), out)
        assert blk.ST() == int(tr.fixture()[tr.case_key("enc", case) + "_end"])


@pytest.mark.parametrize("name", ("rep2", "awgn1o2_4", "gen_133_171", "awgn1o2_128"))      # S = 1, 4, 64 (chunked), 128 (serial)
def test_encoder_lengths_cuts_and_streams(gpu, name):
    g = gpu
    f = tr.make_fsm(name)
    lf = tr.lib_fsm(g, name)
    r = np.random.RandomState(len(name))
    for n in (1, 255, 256, 257, 3 * 256 + 37):
        x = r.randint(0, f.I, n).astype(np.uint8)
        ref, end = tr.encode(f, f.S - 1, x)
        for mode in (g.MODE_FAST, g.MODE_GENERIC):
            blk = g.trellis_encoder_bb(lf, f.S - 1)
            blk.set_mode(mode)
            assert np.array_equal(blk.work(x), ref) and blk.ST() == end
    n = 3 * 256 + 37
    x = r.randint(0, f.I, n).astype(np.uint8)
    ref, end = tr.encode(f, 0, x)
    for cuts in ([97, n - 97], [7] * (n // 7) + [n % 7], [300, 1, n - 301]):
        blk = g.trellis_encoder_bb(lf, 0)
        got = np.concatenate([blk.work(x[a:a + c]) for a, c in zip(np.cumsum([0] + cuts[:-1]), cuts)])
        assert np.array_equal(got, ref) and blk.ST() == end
    # three streams, each with its own state
    xs = r.randint(0, f.I, (3, n)).astype(np.uint8)
    for mode in (g.MODE_FAST, g.MODE_GENERIC):
        blk = g.trellis_encoder_bb(lf, 0)
        blk.set_mode(mode)
        blk.set_streams(3)
        first = blk.work(xs[:, :400].copy()).reshape(3, -1)
        second = blk.work(xs[:, 400:].copy()).reshape(3, -1)
        for s in range(3):
            ref, end = tr.encode(f, 0, xs[s])
            assert np.array_equal(np.concatenate([first[s], second[s]]), ref) and blk.ST(s) == end
        blk.set_ST(f.S - 1)
        assert [blk.ST(s) for s in range(3)] == [f.S - 1] * 3


def test_encoder_refuses_a_bad_symbol_and_keeps_its_states(gpu):
    g = gpu
    f = tr.make_fsm("awgn1o2_4")
    for sig, bad in (("bb", 2), ("ss", -1), ("ii", 1 << 20), ("si", 2)):
        for n, mode in ((100, g.MODE_FAST), (1000, g.MODE_FAST), (1000, g.MODE_GENERIC)):
            blk = getattr(g, ENCODERS[sig])(tr.lib_fsm(g, "awgn1o2_4"), 0)
            blk.set_mode(mode)
            blk.set_streams(2)
            x = np.random.RandomState(n).randint(0, f.I, (2, n)).astype(tr.OUT_DTYPES[sig[0]])
            blk.work(x[:, :50].copy())
            states = [blk.ST(0), blk.ST(1)]
            assert states == [tr.encode(f, 0, x[s, :50])[1] for s in range(2)]
            y = x.copy()
            y[1, n // 2] = bad
            with pytest.raises(g.GrhipError) as e:
                blk.work(y)
            assert e.value.code == -1 and [blk.ST(0), blk.ST(1)] == states
            out = blk.work(x[:, 50:].copy()).reshape(2, -1)          # and goes on as if the call had not been made
            for s in range(2):
                assert np.array_equal(out[s], tr.encode(f, 0, x[s])[0][50:])
    with pytest.raises(g.GrhipError):
        g.trellis_encoder_bb(tr.lib_fsm(g, "awgn1o2_4"), 4)
    with pytest.raises(g.GrhipError):
        g.trellis_encoder_bb(tr.lib_fsm(g, "awgn1o2_4"), -1)


# ---- metrics -----------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", tr.METRICS_CASES, ids=lambda c: tr.case_key("met", c))
def test_metrics_against_the_recording(gpu, case):
    g = gpu
    t, O, D, ty, steps, seed = case
    tab, x = tr.metrics_input(tr.METRIC_DTYPES[t], O, D, steps, seed)
    blk = getattr(g, "trellis_metrics_" + t)(O, D, tab, ty)
    assert (blk.O(), blk.D(), blk.TYPE()) == (O, D, ty)
    for mode in (g.MODE_FAST, g.MODE_GENERIC):
        blk.set_mode(mode)
        assert tr.matches(tr.case_key("met", case), blk.work(x))
    # three streams, and another table
    blk.set_streams(3)
    xs = np.concatenate([x, x[::-1], x])
    ref = tr.calc_metric(xs, tab, O, D, ty)
    assert same_bits(blk.work(xs), ref)
    tab2 = tab[::-1].copy()
    blk.set_TABLE(tab2)
    assert same_bits(blk.work(xs), tr.calc_metric(xs, tab2, O, D, ty))
    with pytest.raises(g.GrhipError):
        blk.set_TABLE(tab2[:-1])


def test_metrics_ties_wraps_and_refusals(gpu):
    g = gpu
    # a sample midway between two table points: HARD_SYMBOL takes the first
    blk = g.trellis_metrics_f(4, 1, [-3.0, -1.0, 1.0, 3.0], g.TRELLIS_HARD_SYMBOL)
    x = np.array([0.0, 2.0, -2.0, 7.0, np.nan, np.inf], np.float32)
    got = blk.work(x).reshape(-1, 4)
    assert same_bits(got.reshape(-1), tr.calc_metric(x, [-3.0, -1.0, 1.0, 3.0], 4, 1, tr.HARD_SYMBOL))
    assert got[0].tolist() == [1, 0, 1, 1] and got[1].tolist() == [1, 1, 0, 1] and got[2].tolist() == [0, 1, 1, 1]
    assert got[4].tolist() == [0, 1, 1, 1] and got[5].tolist() == [0, 1, 1, 1]       # nothing below FLT_MAX: minmi stays 0
    # short differences beyond the short range wrap before they are squared
    blk = g.trellis_metrics_s(2, 1, np.array([-30000, 30000], np.int16), g.TRELLIS_EUCLIDEAN)
    x = np.array([30000, -30000, 0, 32767, -32768], np.int16)
    got = blk.work(x)
    assert same_bits(got, tr.calc_metric(x, np.array([-30000, 30000], np.int16), 2, 1, tr.EUCLIDEAN))
    assert got[0] == float((60000 - 65536) ** 2) and got[1] == 0.0
    # int products wrap
    blk = g.trellis_metrics_i(1, 1, np.array([0], np.int32), g.TRELLIS_EUCLIDEAN)
    x = np.array([46340, 46341, 65536, -2 ** 31], np.int32)
    assert same_bits(blk.work(x), tr.calc_metric(x, np.array([0], np.int32), 1, 1, tr.EUCLIDEAN))
    for make in (lambda: g.trellis_metrics_f(2, 1, [0.0, 1.0], g.TRELLIS_HARD_BIT), lambda: g.trellis_metrics_f(2, 1, [0.0, 1.0], 0),
                 lambda: g.trellis_metrics_f(2, 1, [0.0], g.TRELLIS_EUCLIDEAN), lambda: g.trellis_metrics_c(0, 1, [], g.TRELLIS_EUCLIDEAN),
                 lambda: g.trellis_metrics_s(2, 0, [], g.TRELLIS_EUCLIDEAN),
                 lambda: g.trellis_constellation_metrics_cf(g.constellation_bpsk(), g.TRELLIS_HARD_BIT)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1


@pytest.mark.parametrize("case", tr.CONSTELLATION_CASES, ids=lambda c: tr.case_key("cmet", c))
def test_constellation_metrics_against_the_recording(gpu, case):
    g = gpu
    kind, dim, ty, steps, seed = case
    c = {"bpsk": g.constellation_bpsk, "qpsk": g.constellation_qpsk, "8psk": g.constellation_8psk,
         "calcdist": lambda: g.constellation_calcdist(tr.CALCDIST_POINTS, [], 1, 2)}[kind]()
    blk = g.trellis_constellation_metrics_cf(c, ty)
    assert (blk.O(), blk.D(), blk.TYPE()) == (c.arity(), dim, ty)
    x = tr.constellation_input(dim, steps, seed)
    assert tr.matches(tr.case_key("cmet", case), blk.work(x))


# ---- viterbi_combined --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tr.COMBINED_CASES, ids=lambda c: tr.case_key("comb", c))
def test_viterbi_combined_against_the_recording(gpu, case):
    """both engines and both modes equal the fixture, and equal metrics followed by Viterbi on the device; set_TABLE
    between calls"""
    g = gpu
    name, K, nblocks, S0, SK, sig, D, ty, seed = case
    f, lf = tr.make_fsm(name), tr.lib_fsm(g, name)
    tab, x = tr.combined_input(f, tr.METRIC_DTYPES[sig[0]], D, K, nblocks, seed)
    blk = getattr(g, "trellis_viterbi_combined_" + sig)(lf, K, S0, SK, D, tab, ty)
    assert (blk.K(), blk.S0(), blk.SK(), blk.D(), blk.TYPE(), blk.engine()) == (K, S0, SK, D, ty, 1)
    met = getattr(g, "trellis_metrics_" + sig[0])(f.O, D, tab, ty)
    va = decoder(g, sig[1])(lf, K, S0, SK)
    two_blocks = va.work(met.work(x))
    assert tr.matches(tr.case_key("comb", case), two_blocks)
    for mode, engine, runs in ((g.MODE_FAST, 1, 1), (g.MODE_FAST, 0, 0), (g.MODE_GENERIC, 1, 0), (g.MODE_GENERIC, 0, 0)):
        blk.set_mode(mode)
        blk.set_engine(engine)
        assert blk.engine() == runs                  # GENERIC runs engine 0 whatever was set
        out = blk.work(x)
        assert out.dtype == tr.OUT_DTYPES[sig[1]] and np.array_equal(out, two_blocks)
    assert blk.dead_ends() == 0
    # another table between calls: three streams, both engines
    tab2 = tab.reshape(f.O, D)[::-1].copy().reshape(-1)
    ref2, _ = tr.viterbi_combined(f, K, S0, SK, D, tab2, ty, x, tr.OUT_DTYPES[sig[1]])
    if nblocks % 3 == 0:
        blk.set_streams(3)
    blk.set_TABLE(tab2)
    for mode, engine in ((g.MODE_FAST, 1), (g.MODE_FAST, 0)):
        blk.set_mode(mode)
        blk.set_engine(engine)
        assert np.array_equal(blk.work(x), ref2)
    with pytest.raises(g.GrhipError):
        blk.set_TABLE(tab2[:-1])


def test_viterbi_combined_windows_and_refusals(gpu):
    """the fused engine across the trace window and with an O too large for the metric window"""
    g = gpu
    f, lf = tr.make_fsm("awgn1o2_4"), tr.lib_fsm(g, "awgn1o2_4")
    probe = g.trellis_viterbi_combined_fb(lf, 1, 0, -1, 1, np.zeros(4, np.float32), g.TRELLIS_EUCLIDEAN)
    K = 2 * probe.trace_window() + 3
    nblocks = probe.blocks_per_wavefront() + 1
    tab, x = tr.combined_input(f, np.float32, 2, K, nblocks, 7)
    ref, _ = tr.viterbi_combined(f, K, 0, -1, 2, tab, tr.HARD_SYMBOL, x)
    blk = g.trellis_viterbi_combined_fb(lf, K, 0, -1, 2, tab, g.TRELLIS_HARD_SYMBOL)
    assert blk.workspace_bytes() > 0
    for engine in (1, 0):
        blk.set_engine(engine)
        assert np.array_equal(blk.work(x), ref)
    # S = 1024, O = 2048: a metric window of two steps
    f, lf = tr.make_fsm("isi_2_11"), tr.lib_fsm(g, "isi_2_11")
    tab, x = tr.combined_input(f, np.float32, 1, 32, 2, 8)
    ref, _ = tr.viterbi_combined(f, 32, 0, -1, 1, tab, tr.EUCLIDEAN, x)
    blk = g.trellis_viterbi_combined_fb(lf, 32, 0, -1, 1, tab, g.TRELLIS_EUCLIDEAN)
    for engine in (1, 0):
        blk.set_engine(engine)
        assert blk.engine() == engine and np.array_equal(blk.work(x), ref)
    # four blocks of O = 4096 floats do not fit the window of one wavefront: engine 0 whatever was set
    big = tr.fsm_from_radix(tr.make_fsm("awgn2o3_16"), 4)           # I = 256, S = 16, O = 4096
    lbig = g.fsm(*big.tables())
    tab, x = tr.combined_input(big, np.float32, 1, 8, 2, 9)
    blk = g.trellis_viterbi_combined_fb(lbig, 8, 0, -1, 1, tab, g.TRELLIS_EUCLIDEAN)
    assert blk.engine() == 0
    assert np.array_equal(blk.work(x), tr.viterbi_combined(big, 8, 0, -1, 1, tab, tr.EUCLIDEAN, x)[0])
    t4 = np.zeros(4, np.float32)
    lf = tr.lib_fsm(g, "awgn1o2_4")
    for make in (lambda: g.trellis_viterbi_combined_fb(lf, 8, 0, -1, 1, t4, g.TRELLIS_HARD_BIT), lambda: g.trellis_viterbi_combined_fb(lf, 8, 0, -1, 1, t4[:3], g.TRELLIS_EUCLIDEAN),
                 lambda: g.trellis_viterbi_combined_fb(lf, 8, 0, -1, 0, t4, g.TRELLIS_EUCLIDEAN), lambda: g.trellis_viterbi_combined_cb(lf, 0, 0, -1, 1, t4, g.TRELLIS_EUCLIDEAN),
                 lambda: g.trellis_viterbi_combined_sb(lf, 8, 4, -1, 1, t4, g.TRELLIS_EUCLIDEAN)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1
    blk = g.trellis_viterbi_combined_fb(lf, 8, 0, -1, 1, t4, g.TRELLIS_EUCLIDEAN)
    with pytest.raises(g.GrhipError):
        blk.set_engine(2)
    with pytest.raises(g.GrhipError):
        blk.work(np.zeros(12, np.float32), 12)
