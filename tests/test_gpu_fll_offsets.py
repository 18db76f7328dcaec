"""fll_band_edge_cc work_device on pointers aligned to their item and to nothing more, through the guarded buffers of
tests/device_offsets.py: the offsets of the input and of the four outputs chosen independently, three streams of an odd
length (the entry takes no stream stride: the streams lie back to back, so streams 1 and 2 start at odd item offsets of
their own), GENERIC compared bit for bit against the restatement and FAST through the float64 recurrence's bound, every
output item written and nothing written outside the outputs; with the three float outputs NULL they stay untouched."""
import functools

import numpy as np
import pytest
import torch

import device_offsets as DO
import fll_ref as R

pytestmark = pytest.mark.gpu

S = 3
N = 2 * R.WIN + 37          # odd: two whole windows and a partial one
# input, out, frq, phs, err
OFFSETS = ((0, 0, 0, 0, 0), (1, 0, 1, 2, 3), (0, 1, 3, 1, 2), (1, 3, 2, 3, 1), (3, 2, 1, 0, 1))


@functools.lru_cache(maxsize=None)
def case(g):
    fset = R.SETS[0]
    x = np.stack([R.signal(s, fset)[:N] for s in R.SEEDS])
    taps = g.fll_band_edge_taps(fset[1], fset[2], fset[3])
    refs, refs64 = [], []
    for k in range(S):
        f = R.Fll(fset[1], fset[2], fset[3], fset[4], taps)
        refs.append(f.work(x[k]))
        refs64.append(f.work64(x[k]))
    return fset, x, refs, refs64


def finish(out):
    torch.cuda.synchronize()
    DO.check_guards(out)
    assert not DO.unwritten_items(out).any()
    return out.payload()


@pytest.mark.parametrize("offs", OFFSETS, ids=["-".join(map(str, o)) for o in OFFSETS])
@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_fll_work_device(gpu, mode, offs):
    g = gpu
    fset, x, refs, refs64 = case(g)
    d_in = DO.guarded(x, offs[0])
    df, de = R.DEV_REF["qpsk_s1"]
    mx = R.max_freq_of(fset[1])
    for with_aux in (True, False):
        blk = g.fll_band_edge_cc(fset[1], fset[2], fset[3], fset[4])
        blk.set_mode(getattr(g, mode))
        blk.set_streams(S)
        d_out = DO.guarded_output(N, np.complex64, offs[1], n_streams=S)
        d_f = [DO.guarded_output(N, np.float32, o, n_streams=S) for o in offs[2:]]
        blk.work_device(N, d_in.ptr(), d_out.ptr(), *([b.ptr() for b in d_f] if with_aux else [None, None, None]))
        got = finish(d_out)
        if with_aux:
            frq, phs, err = [finish(b) for b in d_f]
        else:
            torch.cuda.synchronize()
            for b in d_f:
                DO.check_guards(b)
                assert DO.unwritten_items(b).all()
        for k in range(S):
            r = refs[k]
            if mode == "MODE_GENERIC":
                assert np.array_equal(got[k].view(np.uint32), r.out.view(np.uint32))
                assert blk.get_phase(k) == r.phs[-1] and blk.get_frequency(k) == r.frq[-1]
                if with_aux:
                    for a, b in ((frq[k], r.frq), (phs[k], r.phs), (err[k], r.err)):
                        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            else:
                assert np.abs(got[k] - refs64[k].out).max() <= 1e-3 * np.abs(x[k]).max()       # the phase random-walks: coarse
                if with_aux:
                    # seed 1's yardstick holds for stream 0; the other seeds get a factor 4 (what is held here is that
                    # every item is the right item, which a misplaced store misses by the signal's own scale)
                    w = 1 if k == 0 else 4
                    assert np.abs(frq[k].astype(np.float64) - refs64[k].frq).max() <= w * R.bound(df, mx)
                    assert np.abs(err[k].astype(np.float64) - refs64[k].err).max() <= w * R.bound(de, mx)
                    assert blk.get_phase(k) == phs[k][-1] and blk.get_frequency(k) == frq[k][-1]
