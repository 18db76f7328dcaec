"""The trellis blocks' work_device on pointers aligned to their item and to nothing more, through the guarded buffers of
tests/device_offsets.py: input and output offsets chosen independently, three streams of an odd number of blocks (the
streams lie back to back, so streams 1 and 2 start at odd item offsets of their own), compared with the restatement
byte for byte, every output item written and nothing written outside the outputs."""
import functools

import numpy as np
import pytest
import torch

import device_offsets as DO
import trellis_ref as tr

pytestmark = pytest.mark.gpu

S = 3
OFFSETS = ((0, 0), (1, 0), (0, 1), (1, 3), (3, 2), (5, 7))
IDS = ["%d-%d" % o for o in OFFSETS]


@functools.lru_cache(maxsize=None)
def viterbi_case(name, K, ot, nblocks):
    """(metrics [S][n * O], the restatement's symbols) of S streams of nblocks blocks, made once"""
    f = tr.make_fsm(name)
    m = tr.viterbi_input(f, "quant", K, S * nblocks, 3).reshape(S, nblocks * K * f.O)
    ref, _ = tr.viterbi(f, K, 0, -1, m, tr.OUT_DTYPES[ot])
    m.setflags(write=False)
    ref.setflags(write=False)
    return m, ref


@functools.lru_cache(maxsize=None)
def combined_case(name, K, sig, D, ty, nblocks):
    f = tr.make_fsm(name)
    tab, x = tr.combined_input(f, tr.METRIC_DTYPES[sig[0]], D, K, S * nblocks, 13)
    ref, _ = tr.viterbi_combined(f, K, 0, -1, D, tab, ty, x, tr.OUT_DTYPES[sig[1]])
    for a in (tab, x, ref):
        a.setflags(write=False)
    return tab, x, ref


def finish(out):
    torch.cuda.synchronize()
    DO.check_guards(out)
    assert not DO.unwritten_items(out).any()
    return out.payload()


@pytest.mark.parametrize("offs", OFFSETS, ids=IDS)
@pytest.mark.parametrize("name,K,ot", (("awgn1o2_4", 65, "b"), ("isi_3_2", 33, "s"), ("awgn1o2_128", 21, "i"), ("awgn1o2_4", 1029, "b")))
def test_viterbi_work_device(gpu, name, K, ot, offs):
    g = gpu
    nblocks = 5                                      # per stream, odd
    n = nblocks * K
    m, ref = viterbi_case(name, K, ot, nblocks)
    blk = {"b": g.trellis_viterbi_b, "s": g.trellis_viterbi_s, "i": g.trellis_viterbi_i}[ot](tr.lib_fsm(g, name), K, 0, -1)
    blk.set_streams(S)
    d_in = DO.guarded(m, offs[0])
    for mode in (g.MODE_FAST, g.MODE_GENERIC):
        blk.set_mode(mode)
        d_out = DO.guarded_output(n, tr.OUT_DTYPES[ot], offs[1], n_streams=S)
        blk.work_device(n, d_in.ptr(), d_out.ptr())
        assert np.array_equal(finish(d_out).reshape(-1), ref)


@pytest.mark.parametrize("offs", OFFSETS, ids=IDS)
@pytest.mark.parametrize("sig", ("bb", "bs", "bi", "ss", "si", "ii"))
def test_encoder_work_device(gpu, sig, offs):
    g = gpu
    f = tr.make_fsm("awgn2o3_16")
    n = 3 * 256 + 37
    x = np.random.RandomState(9).randint(0, f.I, (S, n)).astype(tr.OUT_DTYPES[sig[0]])
    d_in = DO.guarded(x, offs[0])
    for mode in (g.MODE_FAST, g.MODE_GENERIC):
        blk = getattr(g, "trellis_encoder_" + sig)(tr.lib_fsm(g, "awgn2o3_16"), 1)
        blk.set_mode(mode)
        blk.set_streams(S)
        d_out = DO.guarded_output(n, tr.OUT_DTYPES[sig[1]], offs[1], n_streams=S)
        blk.work_device(n, d_in.ptr(), d_out.ptr())
        got = finish(d_out)
        for s in range(S):
            ref, end = tr.encode(f, 1, x[s], tr.OUT_DTYPES[sig[1]])
            assert np.array_equal(got[s], ref) and blk.ST(s) == end


@pytest.mark.parametrize("offs", OFFSETS, ids=IDS)
@pytest.mark.parametrize("t,ty", (("s", tr.EUCLIDEAN), ("i", tr.HARD_SYMBOL), ("f", tr.EUCLIDEAN), ("f", tr.HARD_SYMBOL), ("c", tr.EUCLIDEAN),
                                  ("c", tr.HARD_SYMBOL)))
def test_metrics_work_device(gpu, t, ty, offs):
    g = gpu
    O, D, steps = 9, 3, 35                           # per stream, odd
    tab, x = tr.metrics_input(tr.METRIC_DTYPES[t], O, D, S * steps, 11)
    blk = getattr(g, "trellis_metrics_" + t)(O, D, tab, ty)
    blk.set_streams(S)
    d_in = DO.guarded(x.reshape(S, steps * D), offs[0])
    d_out = DO.guarded_output(steps * O, np.float32, offs[1], n_streams=S)
    blk.work_device(steps, d_in.ptr(), d_out.ptr())
    got = finish(d_out).reshape(-1)
    assert np.array_equal(got.view(np.uint32), tr.calc_metric(x, tab, O, D, ty).view(np.uint32))


@pytest.mark.parametrize("offs", OFFSETS, ids=IDS)
def test_constellation_metrics_work_device(gpu, offs):
    g = gpu
    c = g.constellation_calcdist(tr.CALCDIST_POINTS, [], 1, 2)
    steps = 35
    x = tr.constellation_input(2, S * steps, 12)
    blk = g.trellis_constellation_metrics_cf(c, g.TRELLIS_EUCLIDEAN)
    blk.set_streams(S)
    d_in = DO.guarded(x.reshape(S, steps * 2), offs[0])
    d_out = DO.guarded_output(steps * 4, np.float32, offs[1], n_streams=S)
    blk.work_device(steps, d_in.ptr(), d_out.ptr())
    got = finish(d_out).reshape(-1)
    assert np.array_equal(got.view(np.uint32), tr.calc_metric(x, tr.CALCDIST_POINTS, 4, 2, tr.EUCLIDEAN).view(np.uint32))


@pytest.mark.parametrize("offs", OFFSETS, ids=IDS)
@pytest.mark.parametrize("sig,D,ty", (("fb", 1, tr.EUCLIDEAN), ("cb", 2, tr.HARD_SYMBOL), ("ss", 2, tr.EUCLIDEAN), ("ii", 1, tr.HARD_SYMBOL)))
def test_viterbi_combined_work_device(gpu, sig, D, ty, offs):
    g = gpu
    name, K, nblocks = "awgn1o2_4", 65, 5            # per stream, odd
    n = nblocks * K
    tab, x, ref = combined_case(name, K, sig, D, ty, nblocks)
    blk = getattr(g, "trellis_viterbi_combined_" + sig)(tr.lib_fsm(g, name), K, 0, -1, D, tab, ty)
    blk.set_streams(S)
    d_in = DO.guarded(x.reshape(S, n * D), offs[0])
    for engine in (1, 0):
        blk.set_engine(engine)
        d_out = DO.guarded_output(n, tr.OUT_DTYPES[sig[1]], offs[1], n_streams=S)
        blk.work_device(n, d_in.ptr(), d_out.ptr())
        assert np.array_equal(finish(d_out).reshape(-1), ref)
