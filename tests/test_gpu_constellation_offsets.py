"""constellation_decoder_cb, diff_decoder_bb, map_bb, constellation_receiver_cb and constellation_demod_cb work_device on
pointers aligned to their item and to nothing more, through the guarded buffers of tests/device_offsets.py: three
streams of an odd length (the entries take no stream stride: the streams lie back to back, so streams 1 and 2 start at
odd offsets of their own), the byte outputs at every offset 0 .. 15, the float outputs at offsets chosen independently;
results compared against the restatement, nothing written outside the outputs.  (A byte output may rightly equal the
pre-fill pattern, so byte payloads are compared whole; the float outputs must all be written.)"""
import functools

import numpy as np
import pytest
import torch

import constellation_ref as R
import device_offsets as DO
import test_constellation_cpu as T
import test_gpu_constellation as G

pytestmark = pytest.mark.gpu

S = 3
BYTE_OFFSETS = tuple(range(16))


def done(out, written=True):
    torch.cuda.synchronize()
    DO.check_guards(out)
    if written:
        assert not DO.unwritten_items(out).any()
    return out.payload()


@functools.lru_cache(maxsize=None)
def rx_case(name):
    xs, refs = G.segments(name, 2 * R.WIN + 37, step=1900)     # odd: two whole windows and a partial one
    c = G.runs(name)[0]
    return c, xs, refs, [R.receiver(R.rx_loop(), c, xs[s]) for s in range(S)]


@pytest.mark.parametrize("off", BYTE_OFFSETS)
def test_byte_blocks_work_device(gpu, off):
    g = gpu
    n = 1365
    b = T.FIX["bytes_in"][:S * n].reshape(S, n)
    d_in = DO.guarded(b, (off * 7 + 3) % 16)
    for blk, want in ((g.diff_decoder_bb(7), [R.diff_decoder(b[s], 7) for s in range(S)]),
                      (g.map_bb(T.FIX["bytes_map_wide_arg"]), [R.map_bb(b[s], T.FIX["bytes_map_wide_arg"].tolist()) for s in range(S)])):
        blk.set_streams(S)
        d_out = DO.guarded_output(n, np.uint8, off, n_streams=S)
        blk.work_device(n, d_in.ptr(), d_out.ptr())
        got = done(d_out, written=False)
        for s in range(S):
            assert got[s].tolist() == want[s].tolist(), s
    # the decoder: complex items at an odd item offset, one and two dimensions
    x = T.samples()
    for name in ("psk16g", "rect16", "calcdist2d", "8psk"):
        r = dict(R.DEC_KINDS)[name]()
        d, m = r.dimensionality, 455
        xs = x[:S * m * d].reshape(S, m * d)
        blk = g.constellation_decoder_cb(T.handle(g, r))
        blk.set_streams(S)
        d_x = DO.guarded(xs, off % 4)
        d_out = DO.guarded_output(m, np.uint8, off, n_streams=S)
        blk.work_device(m, d_x.ptr(), d_out.ptr())
        got = done(d_out, written=False)
        assert got.reshape(-1).tolist() == r.decision_maker(xs.reshape(-1)).tolist(), name


@pytest.mark.parametrize("off", BYTE_OFFSETS)
@pytest.mark.parametrize("name, mode", (("psk16", "MODE_GENERIC"), ("qpsk", "MODE_FAST"), ("rect16", "MODE_FAST")))
def test_receiver_work_device(gpu, name, mode, off):
    g = gpu
    c, xs, refs64, refs = rx_case(name)
    n = xs.shape[1]
    d_in = DO.guarded(xs, off % 3)
    for floats in (True, False):
        blk = g.constellation_receiver_cb(T.handle(g, c), R.LOOP_BW, R.FMIN, R.FMAX)
        blk.set_mode(getattr(g, mode))
        blk.set_streams(S)
        d_sym = DO.guarded_output(n, np.uint8, off, n_streams=S)
        d_f = [DO.guarded_output(n, np.float32, (off + 1 + 2 * i) % 5, n_streams=S) for i in range(3)]
        blk.work_device(n, d_in.ptr(), d_sym.ptr(), *([f.ptr() for f in d_f] if floats else []))
        sym = done(d_sym, written=False)
        fl = [done(f, written=floats) for f in d_f]
        if not floats:
            assert all(DO.unwritten_items(f).all() for f in d_f)
        for s in range(S):
            assert sym[s].tolist() == refs[s].sym.tolist()
            if floats and mode == "MODE_GENERIC":
                for got, want in zip(fl, (refs[s].err, refs[s].phase, refs[s].freq)):
                    assert R.bits(got[s]).tolist() == R.bits(want).tolist()
            elif floats:
                assert np.abs(fl[0][s] - refs64[s].err).max() <= 1e-5 and np.abs(fl[2][s] - refs64[s].freq).max() <= 1e-5
                assert R.circ(fl[1][s], refs64[s].phase) <= 1e-5


@pytest.mark.parametrize("off", BYTE_OFFSETS)
@pytest.mark.parametrize("name", ("bpsk", "dqpsk", "8psk", "psk16", "psk32"))
def test_demod_work_device(gpu, name, off):
    """bits per symbol 1 .. 5: the one-store paths of k = 1, 2, 4 at aligned and unaligned outputs, and the byte path"""
    g = gpu
    c, xs, refs64, _ = rx_case(name)
    n, k = xs.shape[1], c.bits_per_symbol()
    want = [R.demod_tail(c, refs64[s].sym, True, True) for s in range(S)]
    d_in = DO.guarded(xs, off % 2)
    for engine in (1, 0):
        blk = g.constellation_demod_cb(T.handle(g, c), R.LOOP_BW, R.FMIN, R.FMAX, True, True)
        blk.set_streams(S)
        blk.set_engine(engine)
        d_out = DO.guarded_output(n * k, np.uint8, off, n_streams=S)
        blk.work_device(n, d_in.ptr(), d_out.ptr())
        got = done(d_out, written=False)
        for s in range(S):
            assert got[s].tolist() == want[s].tolist(), (engine, s)
