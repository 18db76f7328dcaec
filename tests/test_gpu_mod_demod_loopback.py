"""Modulator into demodulator on the device: dqpsk_mod feeds the receive chain of tests/test_gpu_demod_chain.py (agc2_cc ->
fll_band_edge_cc -> pfb_clock_sync_ccf -> constellation_demod_cb) on device buffers throughout, and unpacked_to_packed_bb
turns the received bits back into bytes there.  Only the produced counts come to the host.  Behind the prefix the bytes
are the sent ones at the lag that tests/modulator_ref.py pins (tests/test_modulator_cpu.py holds the same loop on the
restatements, with noise as margin), and timing recovery never slips."""
import numpy as np
import pytest
import torch

import demod_chain_ref as D
import modulator_ref as MR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ("MODE_FAST", "MODE_GENERIC"))
@pytest.mark.parametrize("cut", (None, (333, 4097)))
def test_dqpsk_bytes_come_back(gpu, mode, cut):
    g = gpu
    sent = MR.loop_bytes()
    mod = g.dqpsk_mod(samples_per_symbol=MR.LOOP_SPS)
    agc = g.agc2_cc(*D.AGC)
    fll = g.fll_band_edge_cc(*D.FLL)
    pcs = g.pfb_clock_sync_ccf(float(D.SPS), 2 * np.pi / 100, g.firdes_root_raised_cosine(*D.PCS_TAPS), 32, 16.0, 1.5, 1)
    rx = g.constellation_demod_cb(g.constellation_dqpsk(), D.RX[0], D.RX[1], D.RX[2], True, True)
    for b in (mod, agc, fll, pcs, rx):
        b.set_mode(getattr(g, mode))
    st = torch.cuda.Stream()            # the entries do not synchronise: one stream orders the blocks
    d_sent = torch.from_numpy(sent).cuda()
    n_samples = mod.max_produced(len(sent))
    d_x = torch.empty(n_samples, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    # the modulator, in one call or cut at a byte
    edges = [0, len(sent)] if cut is None else [0, cut[0], len(sent)]
    done = 0
    for a, b in zip(edges[:-1], edges[1:]):
        done += mod.work_device(b - a, d_sent[a:b], d_x[done:], 0, n_samples - done, stream=st)
    assert done == n_samples == 8 * len(sent)
    # the receiver, in one call or cut at a sample
    d_bits = torch.zeros(2 * (n_samples // 2 + 8), dtype=torch.uint8, device="cuda")
    edges = [0, n_samples] if cut is None else [0, cut[1], n_samples]
    nsym = 0
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
        if m:
            rx.work_device(m, d_s, d_bits[2 * nsym:], stream=st)
        nsym += m
    assert pcs.slips(0) == 0 and nsym > 4 * len(sent) - 100
    # bits back into bytes, from the first symbol behind the prefix that starts a sent byte
    first = MR.LOOP_PREFIX + (MR.LOOP_LAG - MR.LOOP_PREFIX) % 4
    byte0 = (first - MR.LOOP_LAG) // 4
    nbytes = (nsym - first) // 4
    pack = g.unpacked_to_packed_bb(1, g.GR_MSB_FIRST)
    d_back = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    produced, consumed = pack.general_work_device(nbytes, 8 * nbytes, d_bits[2 * first:], d_back, stream=st)
    st.synchronize()
    assert (produced, consumed) == (nbytes, 8 * nbytes)
    back = d_back.cpu().numpy()
    wrong = int(np.count_nonzero(back != sent[byte0:byte0 + nbytes]))
    print("%s cut %s: %d of %d bytes wrong behind the prefix at lag %d" % (mode, cut, wrong, nbytes, MR.LOOP_LAG))
    assert nbytes > len(sent) - MR.LOOP_PREFIX // 4 - 40 and wrong == 0
