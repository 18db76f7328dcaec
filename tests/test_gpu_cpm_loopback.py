"""The frequency-shift receive path closed on the device: the library's own continuous-phase transmitter feeds
quadrature_demod_cf, and what comes back is what was sent.  tests/test_cpm_cpu.py runs the same two loops on the
restatements, which fixes the lag and the settling allowance used here."""
import numpy as np
import pytest
import torch

import cpm_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ("MODE_FAST", "MODE_GENERIC"))
def test_gmsk_bits_come_back(gpu, mode):
    """(a) gmsk_mod(sps 4, bt 0.35) on 512 random bytes -> quadrature_demod_cf(sps / (pi / 2)) -> clock_recovery_mm_ff with
    gmsk.py's defaults -> binary_slicer_fb, on device buffers throughout.  Every bit behind the first LOOP_SETTLE = 300 symbols
    (the allowance of tests/test_gpu_mod_demod_loopback.py; the restated loop passes with it) is returned at the single lag
    LOOP_LAG = 1 <= 16 that the restated loop finds."""
    g = gpu
    sent = R.loop_bytes()
    n = 8 * len(sent) * R.LOOP_SPS
    mod = g.gmsk_mod(R.LOOP_SPS, R.LOOP_BT)
    qd = g.quadrature_demod_cf(R.loop_demod_gain())
    mm = g.clock_recovery_mm_ff(*R.loop_mm_params())
    sl = g.binary_slicer_fb()
    mod.set_mode(getattr(g, mode))         # the three receive blocks have one form
    st = torch.cuda.Stream()            # the entries do not synchronise: one stream orders the blocks
    d_sent = torch.from_numpy(sent).cuda()
    d_x = torch.zeros(n + 1, dtype=torch.complex64, device="cuda")          # item 0: the demodulator's history
    d_y = torch.zeros(n, dtype=torch.float32, device="cuda")
    nout = n // R.LOOP_SPS - 8
    assert mm.forecast(nout) <= n
    d_soft = torch.zeros(nout, dtype=torch.float32, device="cuda")
    d_counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_bits = torch.zeros(nout, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mod.work_device(len(sent), d_sent, d_x[1:], stream=st)
    qd.work_device(n, d_x, d_y, stream=st)
    mm.general_work_device(nout, n, d_y, d_soft, d_counts, stream=st)
    st.synchronize()
    produced = int(d_counts.cpu()[0])
    assert produced > 8 * len(sent) - 16
    sl.work_device(produced, d_soft, d_bits, stream=st)
    st.synchronize()
    bits = d_bits.cpu().numpy()[:produced]
    lags = R.lags_without_error(bits, np.unpackbits(sent), R.LOOP_SETTLE)
    print("%s: %d bits, lags without an error behind %d symbols: %s" % (mode, produced, R.LOOP_SETTLE, lags))
    assert lags == [R.LOOP_LAG] and R.LOOP_LAG <= R.LOOP_MAX_LAG


@pytest.mark.parametrize("mode", ("MODE_FAST", "MODE_GENERIC"))
def test_4fsk_levels_come_back(gpu, mode):
    """(b) cpmmod_bc(LREC, h 0.5, sps 10, L 1) on 1000 symbols from {-3, -1, 1, 3} -> quadrature_demod_cf(sps / (pi h)): every
    sample from the second on, rounded to the nearest level, is the symbol it lies in -- the phase step inside a symbol is
    constant.  This is the benchmark's 4FSK signal, made by the library."""
    g = gpu
    s = R.fsk4_symbols()
    n = len(s) * R.FSK4_SPS
    mod = g.cpmmod_bc(g.CPM_LREC, R.FSK4_H, R.FSK4_SPS, 1)
    qd = g.quadrature_demod_cf(R.FSK4_SPS / (np.pi * R.FSK4_H))
    mod.set_mode(getattr(g, mode))
    st = torch.cuda.Stream()
    d_s = torch.from_numpy(s.view(np.uint8).copy()).cuda()
    d_x = torch.zeros(n + 1, dtype=torch.complex64, device="cuda")
    d_y = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    mod.work_device(len(s), d_s, d_x[1:], stream=st)
    qd.work_device(n, d_x, d_y, stream=st)
    st.synchronize()
    y = d_y.cpu().numpy()
    want = np.repeat(s, R.FSK4_SPS)
    print("%s: largest distance from the level %.4f" % (mode, float(np.abs(y - want)[1:].max())))
    assert np.array_equal(R.fsk4_levels(y[1:]), want[1:])
