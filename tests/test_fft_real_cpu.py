"""CPU tests of the real-signal FFT blocks' references (tests/fft_real_ref.py) and of the boundary the blocks add: the
restated overlap-add equals the direct-form FIR, the sizes follow the reference's formula, the library exports the new
symbols and the binding has the classes.  No GPU involved."""
import os
import re

import numpy as np
import pytest

import fft_real_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FFF_SYMBOLS = ["grhip_fft_filter_fff_" + n for n in ("create", "destroy", "set_taps", "nsamples", "decimation", "work",
                                                     "work_device")]
VFC_SYMBOLS = ["grhip_fft_vfc_" + n for n in ("create", "destroy", "set_window", "work", "work_device")]


@pytest.mark.parametrize("decim", [1, 2, 5])
@pytest.mark.parametrize("ntaps", [1, 2, 7, 64, 255, 1000])
def test_restatement_equals_direct_form(ntaps, decim):
    rng = np.random.default_rng(1000 * decim + ntaps)
    taps = rng.standard_normal(ntaps).astype(np.float32)
    ref = fr.FftFilterFff(decim, taps)
    ns = ref.nsamples
    nout = 4 * ns
    x = rng.standard_normal(nout * decim).astype(np.float32)
    # two calls: the tail and the decimation counter cross the seam
    got = np.concatenate([ref.filter(ns, x[:ns * decim]), ref.filter(3 * ns, x[ns * decim:])])
    # the taps the block applies are float32(taps / fftsize) * fftsize: exact, fftsize is a power of two
    want = fr.fir_direct(taps, x, nout, decim)
    assert len(got) == nout
    # float64 rounding: two transforms of fftsize points and one of the taps, a few eps log2(fftsize) of the peak
    tol = 64 * np.finfo(np.float64).eps * np.log2(2 * ref.fftsize) * max(np.abs(want).max(), np.abs(taps).sum() * 1e-3)
    assert np.abs(got - want).max() <= tol


@pytest.mark.parametrize("ntaps,fftsize", [(1, 2), (2, 4), (3, 8), (7, 16), (64, 128), (65, 256), (255, 512), (1000, 2048),
                                           (2049, 8192), (5000, 16384)])
def test_sizes_follow_the_reference_formula(ntaps, fftsize):
    assert fr.sizes(ntaps) == (fftsize, fftsize - ntaps + 1)
    assert fr.FftFilterFff(1, np.ones(ntaps, np.float32)).nsamples == fftsize - ntaps + 1


def test_vfc_reference_is_the_full_spectrum():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(3 * 16).astype(np.float32)
    w = rng.standard_normal(16).astype(np.float32)
    X = fr.fft_vfc(x, 16, w).reshape(3, 16)
    assert X.shape == (3, 16)
    # real input: Hermitian, X[N - k] = conj(X[k]) -- the block emits both halves
    assert np.abs(X[:, 1:] - np.conj(X[:, :0:-1])).max() < 1e-12
    assert np.allclose(X[:, 0], (x.reshape(3, 16) * w).astype(np.float64).sum(axis=1))


def test_library_exports_the_new_symbols(g):
    lib = g.lib()
    missing = [n for n in FFF_SYMBOLS + VFC_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    for n in FFF_SYMBOLS + VFC_SYMBOLS:
        assert re.search(r"GRHIP_API\s+\w+\s+\*?%s\(" % n, hdr), n


def test_binding_has_both_classes(g):
    for name in ("fft_filter_fff", "fft_vfc"):
        assert hasattr(g, name) and name in g.__all__, name
    for m in ("nsamples", "decimation", "history", "set_taps", "work", "work_device"):
        assert callable(getattr(g.fft_filter_fff, m)), m
    for m in ("set_window", "work", "work_device"):
        assert callable(getattr(g.fft_vfc, m)), m
    # history() is the reference's set_history(1) (gr_fft_filter_fff.cc:51): no handle needed to say so
    blk = g.fft_filter_fff.__new__(g.fft_filter_fff)
    blk._h = None
    assert blk.history() == 1
