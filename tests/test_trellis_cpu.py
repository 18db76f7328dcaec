"""gr-trellis without a device: the grhip_fsm_* entries against the reference's recorded tables for every constructor,
their refusals, csrc/trellis_fsm.h under the sanitizers (host/trellis_fsm_test.cc), and the Python restatement
(tests/trellis_ref.py) against every case of tests/golden/ref_trellis.npz, which pins it for the GPU tests."""
import os
import subprocess

import numpy as np
import pytest

import trellis_ref as tr

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnuradio-3.5.0-dmr_amd", "host")


lib_fsm = tr.lib_fsm


@pytest.mark.parametrize("name", sorted(tr.FSM_SPECS))
def test_fsm_entries_against_the_recording(g, name):
    f = lib_fsm(g, name)
    assert [f.I(), f.S(), f.O()] == list(tr.fixture()["fsm_%s_ISO" % name])
    for t in ("NS", "OS", "TMl", "TMi"):
        assert tr.matches("fsm_%s_%s" % (name, t), getattr(f, t)()), t
    ps, pi = f.PS(), f.PI()
    assert tr.matches("fsm_%s_Plen" % name, np.array([len(p) for p in ps], np.int32))
    assert tr.matches("fsm_%s_PS" % name, np.concatenate(ps).astype(np.int32))
    assert tr.matches("fsm_%s_PI" % name, np.concatenate(pi).astype(np.int32))


@pytest.mark.parametrize("name", sorted(tr.FSM_SPECS))
def test_restated_fsm_against_the_recording(name):
    f = tr.make_fsm(name)
    assert [f.I, f.S, f.O] == list(tr.fixture()["fsm_%s_ISO" % name])
    assert tr.matches("fsm_%s_NS" % name, np.array(f.NS, np.int32)) and tr.matches("fsm_%s_OS" % name, np.array(f.OS, np.int32))
    lens, ps = tr.flat_lists(f.PS)
    assert tr.matches("fsm_%s_Plen" % name, lens) and tr.matches("fsm_%s_PS" % name, ps)
    assert tr.matches("fsm_%s_PI" % name, tr.flat_lists(f.PI)[1])
    if f.S <= 128:                                  # find_es is a serial sweep: the large ones are the library's to match
        assert tr.matches("fsm_%s_TMl" % name, np.array(f.TMl, np.int32)) and tr.matches("fsm_%s_TMi" % name, np.array(f.TMi, np.int32))


def test_fsm_constructors_agree(g):
    def same(a, b):
        return (a.I(), a.S(), a.O()) == (b.I(), b.S(), b.O()) and np.array_equal(a.NS(), b.NS()) and np.array_equal(a.OS(), b.OS()) \
            and np.array_equal(a.TMl(), b.TMl()) and np.array_equal(a.TMi(), b.TMi())
    file = lib_fsm(g, "awgn1o2_4")
    assert same(file, g.fsm(1, 2, [5, 7])) and same(file, g.fsm(*tr.QA_FSMS["qa_awgn1o2_4"]))
    assert same(file, g.fsm(text=tr.fsm_file_text("awgn1o2_4"))) and same(file, g.fsm(file))        # qa_trellis.py test_002
    f64 = g.fsm(1, 2, [0o133, 0o171])
    assert (f64.I(), f64.S(), f64.O()) == (2, 64, 4)
    isi = g.fsm(3, 2)
    assert (isi.I(), isi.S(), isi.O()) == (3, 3, 9)
    big = g.fsm(2, 11)
    assert (big.I(), big.S(), big.O()) == (2, 1024, 2048) and big.connected()
    assert lib_fsm(g, "awgn1o2_4").connected() and not lib_fsm(g, "disconnected").connected()
    assert tr.make_fsm("awgn1o2_4").connected and not tr.make_fsm("disconnected").connected
    irr = lib_fsm(g, "irregular")
    assert [len(p) for p in irr.PS()] == [3, 1] and [list(p) for p in irr.PS()] == [[0, 0, 1], [1]] and list(irr.PI()[0]) == [0, 1, 0]


def test_fsm_refusals(g):
    bad = [
        lambda: g.fsm(0, 1, 4, [], []), lambda: g.fsm(2, 0, 4, [], []), lambda: g.fsm(2, 1, 0, [0, 0], [0, 0]),
        lambda: g.fsm(2, 1, 4, [0], [0, 3]), lambda: g.fsm(2, 1, 4, [0, 0], [0, 3, 3]),
        lambda: g.fsm(2, 1, 4, [0, 1], [0, 3]), lambda: g.fsm(2, 1, 4, [0, -1], [0, 3]),
        lambda: g.fsm(2, 1, 4, [0, 0], [0, 4]), lambda: g.fsm(2, 1, 4, [0, 0], [-1, 3]),
        lambda: g.fsm(text=""), lambda: g.fsm(text="2 4 4\n0 2 0 2 1 3 1 3\n0 3 3 0 1 2 2"), lambda: g.fsm(text="2 1 4\n0 x\n0 3"),
        lambda: g.fsm(os.path.join(tr.FSM_DIR, "no_such_file.fsm")),
        lambda: g.fsm(1, 2, [0, 0]), lambda: g.fsm(1, 2, [5]), lambda: g.fsm(1, 2, [1 << 12, 1]),
        lambda: g.fsm(0, 2), lambda: g.fsm(2, 0), lambda: g.fsm(2, 13),
        lambda: g.fsm(0, 2, 1), lambda: g.fsm(2, 2, 0), lambda: g.fsm(3, 2, 11),
        lambda: g.fsm(g.fsm(2, 12), g.fsm(2, 2)), lambda: g.fsm(g.fsm(2, 2), 0), lambda: g.fsm(g.fsm(2, 2), 22),
    ]
    for make in bad:
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1                   # GRHIP_EINVAL
    with pytest.raises(TypeError):
        g.fsm(1, 2, 3, 4)


def test_trellis_fsm_under_the_sanitizers():
    """csrc/trellis_fsm.h under the address and undefined-behaviour sanitizers: no device, its own main"""
    r = subprocess.run(["make", "-C", HOST, "trellis_fsm_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([os.path.join(HOST, "trellis_fsm_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "trellis_fsm_test ok" in r.stdout, r.stdout


# ---- the restatement against every recorded case -----------------------------------------------------------------------
@pytest.mark.parametrize("case", tr.VITERBI_CASES, ids=lambda c: tr.case_key("vit", c))
def test_restated_viterbi(case):
    name, K, nblocks, S0, SK, kind, seed, ot = case
    f = tr.make_fsm(name)
    out, dead = tr.viterbi(f, K, S0, SK, tr.viterbi_input(f, kind, K, nblocks, seed), tr.OUT_DTYPES[ot])
    assert dead == 0 and tr.matches(tr.case_key("vit", case), out)


def test_the_tie_cases_tell_the_first_minimum_from_the_last():
    """a decoder that kept the last minimum instead of the first would give other bytes on these inputs, so the
    recorded cases (and the GPU tests on the same kinds of input) can fail for that reason"""
    differing = 0
    for case in tr.VITERBI_CASES:
        name, K, nblocks, S0, SK, kind, seed, ot = case
        if kind not in ("quant", "hard", "zeros") or max(len(p) for p in tr.make_fsm(name).PS) < 2:
            continue
        f = tr.make_fsm(name)
        m = tr.viterbi_input(f, kind, K, nblocks, seed)
        first, _ = tr.viterbi(f, K, S0, SK, m, tr.OUT_DTYPES[ot])
        last, _ = tr.viterbi(f, K, S0, SK, m, tr.OUT_DTYPES[ot], last_minimum=True)
        assert tr.matches(tr.case_key("vit", case), first)
        if not np.array_equal(first, last):
            differing += 1
            assert not tr.matches(tr.case_key("vit", case), last)
    assert differing >= 5
    # all-zero metrics: every comparison ties, the first predecessor wins everywhere and the path ends in state 0
    f = tr.make_fsm("awgn1o2_4")
    out, _ = tr.viterbi(f, 33, -1, -1, np.zeros(33 * 4, np.float32))
    st = 0
    for k in range(32, -1, -1):
        assert out[k] == f.PI[st][0]
        st = f.PS[st][0]


def test_restated_dead_end_rule():
    """a state without predecessors: as S0 it is never stood in by the traceback; driven there by 1e9 metrics it is"""
    f = tr.Fsm(2, 3, 2, [1, 2, 1, 2, 2, 1], [0, 1, 1, 0, 0, 1])        # nothing leads to state 0
    assert f.PS[0] == []
    m = tr.viterbi_input(f, "quant", 16, 4, 5)
    out, dead = tr.viterbi(f, 16, 0, -1, m)
    assert dead == 0
    out, dead = tr.viterbi(f, 16, -1, 0, m)                            # SK on the state without predecessors
    assert dead == 4 * 16 and not out.any()


@pytest.mark.parametrize("case", tr.ENCODER_CASES, ids=lambda c: tr.case_key("enc", c))
def test_restated_encoder(case):
    name, sig, n, st, seed = case
    f = tr.make_fsm(name)
    x = np.random.RandomState(seed).randint(0, f.I, n).astype(tr.OUT_DTYPES[sig[0]])
    out, end = tr.encode(f, st, x, tr.OUT_DTYPES[sig[1]])
    assert tr.matches(tr.case_key("enc", case), out) and end == int(tr.fixture()[tr.case_key("enc", case) + "_end"])


@pytest.mark.parametrize("case", tr.METRICS_CASES, ids=lambda c: tr.case_key("met", c))
def test_restated_metrics(case):
    t, O, D, ty, steps, seed = case
    tab, x = tr.metrics_input(tr.METRIC_DTYPES[t], O, D, steps, seed)
    assert tr.matches(tr.case_key("met", case), tr.calc_metric(x, tab, O, D, ty))


@pytest.mark.parametrize("case", tr.CONSTELLATION_CASES, ids=lambda c: tr.case_key("cmet", c))
def test_restated_constellation_metrics(case):
    kind, dim, ty, steps, seed = case
    pts = tr.fixture()["cpoints_" + kind]
    x = tr.constellation_input(dim, steps, seed)
    got = tr.calc_metric(x, pts, len(pts) // dim, dim, ty)
    assert tr.matches(tr.case_key("cmet", case), got)
    if ty == tr.HARD_SYMBOL:
        assert np.all((got.reshape(steps, -1) == 0).sum(axis=1) == 1)
    if ty == tr.HARD_SYMBOL and kind in ("bpsk", "qpsk"):
        assert got.reshape(steps, -1)[0, 0] == 0.0      # the sample at the origin ties between the points: the first wins


def test_short_differences_wrap_in_the_recording():
    """the short cases hold steps whose difference leaves the short range, so the truncation is exercised"""
    tab, x = tr.metrics_input(np.int16, 2, 1, 97, 40)
    d = x.astype(np.int32)[:, None] - tab.astype(np.int32)[None, :]
    assert (np.abs(d) > 32767).any()


@pytest.mark.parametrize("name", ("qa_awgn1o2_4", "rep2", "nothing"))
def test_restated_qa_chain_returns_every_bit(name):
    """the chain of tests/test_gpu_trellis_loopback.py (trellis_ref.qa_chain) on the restatement: at N0 = 0.02 every bit comes back"""
    f = tr.make_fsm(name)
    pts = tr.fixture()["cpoints_bpsk" if f.O == 2 else "cpoints_qpsk"]
    sent, noise, rx, metrics = tr.qa_chain(name, pts, tr.QA_K, tr.QA_N0)
    assert np.abs(noise.real).max() < 0.5 and np.abs(noise.imag).max() < 0.5      # no sample crosses a decision border
    dec, dead = tr.viterbi(f, tr.QA_K, 0, -1, metrics)
    assert dead == 0 and np.array_equal(np.packbits(dec), sent)
    dec2, _ = tr.viterbi_combined(f, tr.QA_K, 0, -1, 1, pts, tr.EUCLIDEAN, rx)
    assert np.array_equal(dec2, dec)


@pytest.mark.parametrize("case", tr.COMBINED_CASES, ids=lambda c: tr.case_key("comb", c))
def test_restated_viterbi_combined(case):
    name, K, nblocks, S0, SK, sig, D, ty, seed = case
    f = tr.make_fsm(name)
    tab, x = tr.combined_input(f, tr.METRIC_DTYPES[sig[0]], D, K, nblocks, seed)
    out, dead = tr.viterbi_combined(f, K, S0, SK, D, tab, ty, x, tr.OUT_DTYPES[sig[1]])
    assert dead == 0 and tr.matches(tr.case_key("comb", case), out)
