"""complex_to_mag_work_device and am_demod_cf_work_device on pointers aligned to their item and to nothing more, through
the guarded buffers of tests/device_offsets.py: input and output offsets chosen independently (the fused AM kernel
stores four outputs at a time where the output pointer allows it, so every residue of the output pointer modulo 16
bytes is run), three streams, results equal to the aligned call's, every output item written and nothing written
outside the output.  Neither entry takes a stream stride: the streams lie back to back."""
import numpy as np
import pytest
import torch

import device_offsets as DO
import optfir_ref as O

pytestmark = pytest.mark.gpu

S = 3
IN_OFFSETS = (0, 1)
OUT_OFFSETS = (0, 1, 2, 3)


def signal(n):
    return np.stack([O.am_signal(40 + k, n) for k in range(S)])


def finish(out, want, exact):
    torch.cuda.synchronize()
    DO.check_guards(out)
    assert not DO.unwritten_items(out).any()
    got = out.payload()
    if exact:
        assert np.array_equal(O.bits32(got), O.bits32(want))
    else:
        peak = float(np.max(np.abs(want)))
        assert float(np.max(np.abs(got.astype(np.float64) - want))) <= 1e-5 * peak


@pytest.mark.parametrize("off_out", OUT_OFFSETS)
@pytest.mark.parametrize("off_in", IN_OFFSETS)
def test_complex_to_mag_work_device(gpu, off_in, off_out):
    g = gpu
    n = 3 * 256 + 37
    x = signal(n)
    want = np.stack([O.mag(x[k]) for k in range(S)])
    blk = g.complex_to_mag()
    blk.set_streams(S)
    d_in = DO.guarded(x, off_in)
    d_out = DO.guarded_output(n, np.float32, off_out, n_streams=S)
    assert blk.work_device(n, d_in.ptr(), d_out.ptr()) == n
    finish(d_out, want, True)


@pytest.mark.parametrize("off_out", OUT_OFFSETS)
@pytest.mark.parametrize("off_in", IN_OFFSETS)
@pytest.mark.parametrize("D, mode", ((1, "MODE_FAST"), (2, "MODE_FAST"), (1, "MODE_GENERIC")))
def test_am_demod_cf_work_device(gpu, po, D, mode, off_in, off_out):
    g = gpu
    n = g.am_demod_cf.tile() + 3 * 256 + 37
    taps = O.audio_taps(37)
    x = signal(n)
    v = [O.am_v(x[k]) for k in range(S)]
    exact = mode == "MODE_GENERIC"
    want = np.stack([O.am_fir(po, v[k], D, taps) if exact else O.am_fir64(v[k], D, taps) for k in range(S)])
    blk = g.am_demod_cf.from_taps(D, taps)
    blk.set_mode(getattr(g, mode))
    blk.set_streams(S)
    np_ = blk.produced(n)
    assert np_ == O.am_outputs(n, D)
    d_in = DO.guarded(x, off_in)
    d_out = DO.guarded_output(np_, np.float32, off_out, n_streams=S)
    d_np = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    blk.work_device(n, d_in.ptr(), d_out.ptr(), d_np)
    finish(d_out, want, exact)
    assert int(d_np.cpu()[0]) == np_
