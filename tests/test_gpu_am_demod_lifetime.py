"""Handle lifetime of complex_to_mag and am_demod_cf: rounds of create, work and destroy over both modes, decimations
and filter lengths with every result checked (a handle that came up with a stale delay line or stale taps would show),
handles that never worked, set_streams up and down on a live handle, and a handle destroyed with its work still
queued."""
import gc

import numpy as np
import pytest

import optfir_ref as O

pytestmark = pytest.mark.gpu

ROUNDS = 60
SHAPES = ((1, 83), (2, 37), (1, 1), (5, 130))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(O.bits32(a), O.bits32(b))


def close(got, want64):
    return got.shape == want64.shape and float(np.max(np.abs(got - want64))) <= 1e-5 * float(np.max(np.abs(want64)))


def test_create_work_destroy(gpu, po):
    g = gpu
    x = O.am_signal(9, 5000)
    v = O.am_v(x)
    want = {s: (O.am_fir(po, v, s[0], O.audio_taps(s[1])), O.am_fir64(v, s[0], O.audio_taps(s[1]))) for s in SHAPES}
    m = O.mag(x)
    for i in range(ROUNDS):
        D, ntaps = shape = SHAPES[i % 4]
        blk = g.am_demod_cf.from_taps(D, O.audio_taps(ntaps))
        generic = bool(i & 4)
        blk.set_mode(g.MODE_GENERIC if generic else g.MODE_FAST)
        got = np.concatenate([blk.work(x[:333]), blk.work(x[333:])])
        assert same_bits(got, want[shape][0]) if generic else close(got, want[shape][1]), i
        del blk
        g.am_demod_cf.from_taps(3, np.ones(2, np.float32))              # never used
        c = g.complex_to_mag(1 + i % 3)
        assert same_bits(c.work(999 // (1 + i % 3), x[:999]), m[:999 // (1 + i % 3) * (1 + i % 3)]), i
        del c
    gc.collect()


def test_set_streams_on_a_live_handle(gpu, po):
    g = gpu
    x = O.am_signal(10, 4500)
    v = O.am_v(x)
    taps = O.audio_taps(83)
    want, want64 = O.am_fir(po, v, 1, taps), O.am_fir64(v, 1, taps)
    blk = g.am_demod_cf.from_taps(1, taps)
    c = g.complex_to_mag()
    for S in (1, 5, 64, 2, 1):
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            blk.set_mode(mode)
            blk.set_streams(S)                                          # every stream back at a zero delay line
            y = blk.work(np.tile(x, S), 4500).reshape(S, -1)
            for s in range(S):
                row = np.ascontiguousarray(y[s])
                assert same_bits(row, want) if mode == g.MODE_GENERIC else close(row, want64), (S, s)
        c.set_streams(S)
        assert same_bits(c.work(4500, np.tile(x, S)), np.tile(O.mag(x), S))


def test_destroy_with_work_queued(gpu, po):
    import torch
    g = gpu
    x = O.am_signal(11, 9000)
    v = O.am_v(x)
    taps = O.audio_taps(83)
    want, want64 = O.am_fir(po, v, 1, taps), O.am_fir64(v, 1, taps)
    d_in = torch.from_numpy(np.tile(x, 16).view(np.float32)).cuda()
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        d_out = torch.zeros(16 * len(x), dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        blk = g.am_demod_cf.from_taps(1, taps)
        blk.set_mode(mode)
        blk.set_streams(16)
        blk.work_device(len(x), d_in, d_out, None, st)
        del blk                                                         # no synchronisation before the handle goes
        gc.collect()
        st.synchronize()
        out = d_out.cpu().numpy().reshape(16, len(x))
        for s in range(16):
            row = np.ascontiguousarray(out[s])
            assert same_bits(row, want) if mode == g.MODE_GENERIC else close(row, want64), s
