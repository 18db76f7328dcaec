"""GPU tests of complex_to_mag: the 4096 recorded pairs of tests/golden/ref_complex_to_mag.npz (std::abs of the
reference's loop; tests/test_am_demod_cpu.py says what they hold) bit for bit in both modes, vlen 1 and 3, three
streams, and lengths 1, 63, 64, 65 and 4097 around the wave and the workgroup."""
import os

import numpy as np
import pytest

import optfir_ref as O

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(O.GOLDEN, "ref_complex_to_mag.npz"))


def pairs():
    return np.ascontiguousarray(FIX["pairs"]).view(np.float32).reshape(-1, 2).copy().view(np.complex64).reshape(-1)


def same(got, want_bits):
    want = np.ascontiguousarray(want_bits).view(np.float32)
    return got.dtype == np.float32 and got.shape == want.shape and bool(
        np.all((O.bits32(got) == want_bits) | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_the_recorded_pairs_bit_for_bit(gpu, mode):
    g = gpu
    blk = g.complex_to_mag()
    blk.set_mode(getattr(g, mode))
    got = blk.work(4096, pairs())
    assert same(got, FIX["mag"])
    inf_nan = np.isinf(pairs().real) & np.isnan(pairs().imag)
    assert inf_nan.sum() == 2 and np.all(np.isposinf(got[inf_nan]))


@pytest.mark.parametrize("vlen", (1, 3))
def test_lengths_vlen_and_streams(gpu, vlen):
    g = gpu
    x, want = np.tile(pairs(), 10), np.tile(FIX["mag"], 10)          # 4097 items of 3 on 3 streams fit
    for n in (1, 63, 64, 65, 4097):
        for streams in (1, 3):
            blk = g.complex_to_mag(vlen)
            if streams != 1:
                blk.set_streams(streams)
            k = streams * n * vlen
            got = blk.work(n, x[-k:])                   # the tail of the set: the special values are in it
            assert same(got, want[-k:]), (n, streams)
    blk = g.complex_to_mag(vlen)
    assert len(blk.work(0, x[:0])) == 0
