"""pfb_clock_sync_ccf work_device on pointers aligned to their item and to nothing more, through the guarded buffers of
tests/device_offsets.py: the offsets of the input and of the four outputs chosen independently, three streams of an odd
length (the entry takes no stream stride: the streams lie back to back, so streams 1 and 2 start at odd item offsets of
their own).  GENERIC is compared bit for bit against the restatement, FAST through the replay of its own errors; every
item below produced[s] is written and nothing at or behind it, nor outside the outputs; with the three float outputs
NULL they stay untouched."""
import functools

import numpy as np
import pytest
import torch

import device_offsets as DO
import pfb_clock_sync_ref as R

pytestmark = pytest.mark.gpu

S = 3
N = 2 * R.WIN + 37          # odd: two whole windows and a partial one
RUN = R.run_of("s2_o2")     # two outputs per symbol: the aux copies behind a symbol's slot are in play
# input, out, err, rate, k
OFFSETS = ((0, 0, 0, 0, 0), (1, 0, 1, 2, 3), (0, 1, 3, 1, 2), (1, 3, 2, 3, 1))


@functools.lru_cache(maxsize=None)
def case():
    x = np.stack([R.signal(seed, RUN[1], RUN[5])[:N] for seed in (1, 2, 3)])
    refs = []
    for s in range(S):
        p = R.make(RUN)
        refs.append((p.work(x[s]), p))
    return x, refs


@pytest.mark.parametrize("offs", OFFSETS, ids=["-".join(map(str, o)) for o in OFFSETS])
@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_pfb_clock_sync_work_device(gpu, mode, offs):
    g = gpu
    x, refs = case()
    nf = R.bank_case(RUN[6])[1]
    taps = R.proto(R.bank_case(RUN[6]))
    d_in = DO.guarded(x, offs[0])
    for with_aux in (True, False):
        blk = g.pfb_clock_sync_ccf(RUN[1], R.LOOP_BW, taps, nf, RUN[3], RUN[4], RUN[2])
        blk.set_mode(getattr(g, mode))
        blk.set_streams(S)
        cap = blk.max_produced(N)
        d_out = DO.guarded_output(cap, np.complex64, offs[1], n_streams=S)
        d_f = [DO.guarded_output(cap, np.float32, o, n_streams=S) for o in offs[2:]]
        d_p = torch.full((S,), -1, dtype=torch.int32, device="cuda")
        blk.work_device(N, d_in.ptr(), cap, d_out.ptr(), d_p, *([b.ptr() for b in d_f] if with_aux else []))
        torch.cuda.synchronize()
        prod = d_p.cpu().numpy()
        written = np.arange(cap)[None, :] < prod[:, None]
        for b in [d_out] + d_f:
            DO.check_guards(b)
            un = DO.unwritten_items(b).reshape(S, cap)
            if b is d_out or with_aux:
                assert np.array_equal(~un, written)             # every item below produced[s], nothing at or behind it
            else:
                assert un.all()
        out = d_out.payload()
        aux = [b.payload() for b in d_f]
        for s in range(S):
            t, p = refs[s]
            n = int(prod[s])
            assert n == len(t.out) and n % RUN[2] == 0
            if mode == "MODE_GENERIC":
                assert np.array_equal(out[s, :n].view(np.uint32), t.out.view(np.uint32))
                if with_aux:
                    for a, name in zip(aux, ("err", "rate", "k")):
                        assert np.array_equal(a[s, :n].view(np.uint32), getattr(t, name).view(np.uint32)), name
                assert blk.position(s) == p.pos and blk.k(s) == p.k
            elif with_aux:
                # the scalar chain replayed with the device's own errors gives the device's rate and k bit for bit
                err = aux[0][s, :n]
                q = R.make(RUN)
                u = q.work(x[s], forced_err=np.concatenate([err[::RUN[2]][1:], [blk.error(s)]]).astype(np.float32))
                assert np.array_equal(aux[1][s, :n].view(np.uint32), u.rate.view(np.uint32))
                assert np.array_equal(aux[2][s, :n].view(np.uint32), u.k.view(np.uint32)) and blk.position(s) == q.pos
                assert np.max(np.abs(out[s, :n] - u.out)) <= 1e-4          # the same items through the same arms (a misplaced store misses by the signal's own scale)
