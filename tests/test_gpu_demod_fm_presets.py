"""GPU tests of the FM presets that design their own audio filter: fm_demod_cf.design, demod_20k0f3e_cf and
demod_200kf3e_cf (blks2impl/fm_demod.py:51-111) over the existing fm_demod_cf handle.

demod_20k0f3e_cf(32e3, 4) has the 61 taps recorded from the reference's remez (tests/golden/ref_remez.npz, lp_fm)
narrowed to float, runs the fused kernel, and equals fm_demod_cf constructed with those taps bit for bit in GENERIC and
in FAST.  demod_200kf3e_cf(320e3, 10) has the 1164 recorded taps (lp_wfm), more than the fused kernel takes
(engine() == 0); over 2 tile() + 3 samples its output is within 1e-5 of the peak of the float64 chain over the
library's own demodulator output (float64 IIR -> float32 -> float64 FIR), measured as tests/test_gpu_fm_demod.py
measures it."""
import math
import os

import numpy as np
import pytest

import iir_ref as R
import optfir_ref as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
FIX = np.load(os.path.join(O.GOLDEN, "ref_remez.npz"))


def recorded(name):
    return FIX[name + "_taps"].view(np.float64).astype(np.float32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


def test_demod_20k0f3e_cf(gpu):
    g = gpu
    n = 2 * g.fm_demod_cf.tile() + 3
    x = R.fm_signal(21, n)
    taps = recorded("lp_fm")
    assert len(taps) == 61
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        rx = g.demod_20k0f3e_cf(32e3, 4)
        assert same_bits(rx.audio_taps, taps) and rx.audio_decim == 4
        assert rx.k == float(np.float32(32e3 / (2 * math.pi * 5000)))
        assert rx.engine() == 1
        ref = g.fm_demod_cf(32e3, 4, 5000, taps)
        rx.set_mode(mode)
        ref.set_mode(mode)
        assert rx.engine() == ref.engine() == (1 if mode == g.MODE_FAST else 0)
        a = np.concatenate([rx.work(x[:255]), rx.work(x[255:])])
        b = np.concatenate([ref.work(x[:255]), ref.work(x[255:])])
        assert len(a) == R.fm_outputs(n, 4) and same_bits(a, b)
    # design() is the constructor the presets go through
    d = g.fm_demod_cf.design(32e3, 4, 5000, 3000, 4500)
    assert isinstance(d, g.fm_demod_cf) and same_bits(d.audio_taps, taps)
    none = g.fm_demod_cf.design(32e3, 4, 5000, 3000, 4500, gain=2.0, tau=None)
    assert same_bits(none.audio_taps, g.optfir_low_pass(2.0, 32e3, 3000, 4500, 0.1, 60).astype(np.float32))


def test_demod_200kf3e_cf(gpu):
    g = gpu
    n = 2 * g.fm_demod_cf.tile() + 3
    x = R.fm_signal(22, n)
    taps = recorded("lp_wfm")
    rx = g.demod_200kf3e_cf(320e3, 10)
    assert len(rx.audio_taps) == 1164 and same_bits(rx.audio_taps, taps) and rx.audio_decim == 10
    assert rx.engine() == 0                             # 1164 taps: above the fused kernel's 1025
    k = float(np.float32(320e3 / (2 * math.pi * 75000)))
    assert rx.k == k
    got = rx.work(x)
    q = g.quadrature_demod_cf(k).work(n, np.concatenate([np.zeros(1, np.complex64), x]))
    y = R.serial(q, *R.deemph_taps(320e3))[0]
    want = R.fm_fir64(y, 10, taps, n)
    assert got.shape == want.shape
    err = float(np.max(np.abs(got.astype(np.float64) - want))) / (float(np.max(np.abs(want))) or 1.0)
    print("demod_200kf3e_cf(320e3, 10), %d samples: %.3g of the peak" % (n, err))
    assert err <= TOL
