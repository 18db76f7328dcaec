"""costas_loop_cc, pll_freqdet_cf, pll_refout_cc and pll_carriertracking_cc work_device on pointers aligned to their
item and to nothing more, through the guarded buffers of tests/device_offsets.py: input, output and frequency-output
offsets chosen independently, three streams of an odd length (the entries take no stream stride: the streams lie back
to back, so streams 1 and 2 start at odd item offsets of their own), results compared against the restatement, every
output item written and nothing written outside the outputs."""
import functools

import numpy as np
import pytest
import torch

import carrier_ref as R
import device_offsets as DO

pytestmark = pytest.mark.gpu

S = 3
N = 2 * R.WIN + 37          # odd: two whole windows and a partial one
OFFSETS = ((0, 0, 0), (1, 0, 1), (0, 1, 3), (1, 3, 2), (3, 2, 1))


@functools.lru_cache(maxsize=None)
def pll_case():
    ps = R.PLL_SETS[1]
    x = np.stack([R.pll_signal(s, ps)[:N] for s in R.SEEDS])
    return ps, x, [R.pll(R.pll_loop(ps), x[k]) for k in range(S)]


@functools.lru_cache(maxsize=None)
def costas_case(ci):
    cs = R.COSTAS_SETS[ci]
    x = np.stack([R.costas_signal(s, cs)[:N] for s in R.SEEDS])
    return cs, x, [R.costas(R.costas_loop(cs), x[k], cs[1]) for k in range(S)], [R.costas64(R.costas_loop(cs), x[k], cs[1]) for k in range(S)]


def finish(out):
    torch.cuda.synchronize()
    DO.check_guards(out)
    assert not DO.unwritten_items(out).any()
    return out.payload()


@pytest.mark.parametrize("off_in, off_out, _", OFFSETS[:4])
@pytest.mark.parametrize("block", ("pll_freqdet_cf", "pll_refout_cc", "pll_carriertracking_cc"))
def test_pll_work_device(gpu, block, off_in, off_out, _):
    g = gpu
    ps, x, refs = pll_case()
    blk = getattr(g, block)(ps[1], ps[2], ps[3])
    blk.set_streams(S)
    d_in = DO.guarded(x, off_in)
    d_out = DO.guarded_output(N, np.float32 if block == "pll_freqdet_cf" else np.complex64, off_out, n_streams=S)
    blk.work_device(N, d_in.ptr(), d_out.ptr())
    got = finish(d_out)
    for k in range(S):
        r = refs[k]
        assert blk.get_phase(k) == r.phases[-1] and blk.get_frequency(k) == r.freqs[-1]
        if block == "pll_freqdet_cf":
            assert np.array_equal(got[k].view(np.uint32), r.freqdet.view(np.uint32))
        elif block == "pll_refout_cc":
            for a, b in ((got[k].real, r.refout.real), (got[k].imag, r.refout.imag)):
                assert np.all(np.abs(a.astype(np.float64) - b) <= np.spacing(np.abs(b)))
        else:
            tol = 4 * 2.0 ** -24 * (np.abs(x[k].real).astype(np.float64) + np.abs(x[k].imag))
            assert np.all(np.abs(got[k].real.astype(np.float64) - r.ct.real) <= tol)
            assert np.all(np.abs(got[k].imag.astype(np.float64) - r.ct.imag) <= tol)


@pytest.mark.parametrize("off_in, off_out, off_f", OFFSETS)
@pytest.mark.parametrize("ci, mode", ((0, "MODE_GENERIC"), (1, "MODE_GENERIC"), (2, "MODE_FAST")))
def test_costas_work_device(gpu, ci, mode, off_in, off_out, off_f):
    g = gpu
    cs, x, refs, refs64 = costas_case(ci)
    d_in = DO.guarded(x, off_in)
    for with_freq in (True, False):
        blk = g.costas_loop_cc(cs[2], cs[1])
        blk.set_mode(getattr(g, mode))
        blk.set_streams(S)
        d_out = DO.guarded_output(N, np.complex64, off_out, n_streams=S)
        d_f = DO.guarded_output(N, np.float32, off_f, n_streams=S)
        blk.work_device(N, d_in.ptr(), d_out.ptr(), d_f.ptr() if with_freq else None)
        got = finish(d_out)
        if with_freq:
            f = finish(d_f)
        else:
            torch.cuda.synchronize()
            DO.check_guards(d_f)
            assert DO.unwritten_items(d_f).all()
        for k in range(S):
            if mode == "MODE_GENERIC":
                assert np.array_equal(got[k].view(np.uint32), refs[k].out.view(np.uint32))
                assert not with_freq or np.array_equal(f[k].view(np.uint32), refs[k].freq.view(np.uint32))
            else:
                assert np.abs(got[k] - refs64[k].out).max() <= 1e-5 * np.abs(x[k]).max()
                assert not with_freq or np.abs(f[k].astype(np.float64) - refs64[k].freq).max() <= 1e-5
