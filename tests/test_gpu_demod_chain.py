"""generic_demod's receive chain on the device (gr-digital/python/generic_mod_demod.py:268-313, with its parameters):
agc2_cc -> fll_band_edge_cc -> pfb_clock_sync_ccf -> constellation_demod_cb on device buffers throughout; only the
count of symbols that timing recovery produced comes to the host, to size the last call.  4096 known DQPSK symbols at
2 samples per symbol with a small frequency and clock offset (demod_chain_ref.py): behind the settling prefix the
transmitted bits come back at the fixed lag with no errors.  tests/test_demod_chain_cpu.py holds the same signal against
the four restatements, with margin."""
import numpy as np
import pytest
import torch

import demod_chain_ref as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ("MODE_FAST", "MODE_GENERIC"))
@pytest.mark.parametrize("cut", (None, 4097))
def test_demod_chain_on_device_buffers(gpu, mode, cut):
    g = gpu
    x, v = D.transmit()
    agc = g.agc2_cc(*D.AGC)
    fll = g.fll_band_edge_cc(*D.FLL)
    pcs = g.pfb_clock_sync_ccf(float(D.SPS), 2 * np.pi / 100, g.firdes_root_raised_cosine(*D.PCS_TAPS), 32, 16.0, 1.5, 1)
    rx = g.constellation_demod_cb(g.constellation_dqpsk(), D.RX[0], D.RX[1], D.RX[2], True, True)
    for b in (agc, fll, pcs, rx):
        b.set_mode(getattr(g, mode))
    d_x = torch.from_numpy(x).cuda()
    st = torch.cuda.Stream()            # the entries do not synchronise: one stream orders the four blocks
    bits = []
    edges = [0, len(x)] if cut is None else [0, cut, len(x)]
    for a, b in zip(edges[:-1], edges[1:]):
        n = b - a
        cap = pcs.max_produced(n)
        d_a, d_f = torch.empty(n, dtype=torch.complex64, device="cuda"), torch.empty(n, dtype=torch.complex64, device="cuda")
        d_s = torch.empty(cap, dtype=torch.complex64, device="cuda")
        d_p = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        agc.work_device(n, d_x[a:b], d_a, stream=st)
        fll.work_device(n, d_a, d_f, stream=st)
        pcs.work_device(n, d_f, cap, d_s, d_p, stream=st)
        st.synchronize()
        m = int(d_p.cpu()[0])
        d_b = torch.empty(max(2 * m, 1), dtype=torch.uint8, device="cuda")
        if m:
            rx.work_device(m, d_s, d_b, stream=st)
        st.synchronize()
        bits.append(d_b.cpu().numpy()[:2 * m])
    bits = np.concatenate(bits)
    assert pcs.slips(0) == 0 and len(bits) // 2 > D.NSYM - 100
    errors, compared = D.errors_behind_prefix(bits, v, D.LAG)
    print("%s cut %s: %d bit errors in %d symbols behind the prefix" % (mode, cut, errors, compared))
    assert errors == 0 and compared > D.NSYM - D.PREFIX - 100
