"""Packets through the modulator and the receive chain on the device: packet_maker's packets behind a settling prefix go
through dqpsk_mod and the receive chain of tests/test_gpu_mod_demod_loopback.py (agc2_cc -> fll_band_edge_cc ->
pfb_clock_sync_ccf -> constellation_demod_cb, the same blocks and constants), then correlate_access_code_bb ->
framer_sink_1_batch -> its device view -> packet_check.  Three messages come out, all ok, with the sent payloads.
tests/test_packet_cpu.py confirms the same stream on the restated chain."""
import numpy as np
import pytest
import torch

import demod_chain_ref as D
import modulator_ref as MR
import packet_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ("MODE_FAST", "MODE_GENERIC"))
def test_packets_come_back_over_the_air(gpu, mode):
    g = gpu
    stream, payloads, packets = packet_ref.rf_loop_stream()
    # the packets are the library's own
    mk = g.packet_maker(MR.LOOP_SPS, 2, pad_for_usrp=False)
    assert mk.make_packets(payloads, packet_ref.RF_OFFSETS) == packets
    mod = g.dqpsk_mod(samples_per_symbol=MR.LOOP_SPS)
    agc = g.agc2_cc(*D.AGC)
    fll = g.fll_band_edge_cc(*D.FLL)
    pcs = g.pfb_clock_sync_ccf(float(D.SPS), 2 * np.pi / 100, g.firdes_root_raised_cosine(*D.PCS_TAPS), 32, 16.0, 1.5, 1)
    rx = g.constellation_demod_cb(g.constellation_dqpsk(), D.RX[0], D.RX[1], D.RX[2], True, True)
    for b in (mod, agc, fll, pcs, rx):
        b.set_mode(getattr(g, mode))
    st = torch.cuda.Stream()            # the entries do not synchronise: one stream orders the blocks
    d_sent = torch.from_numpy(stream).cuda()
    n = mod.max_produced(len(stream))
    d_x = torch.empty(n, dtype=torch.complex64, device="cuda")
    cap = pcs.max_produced(n)
    d_a, d_f = torch.empty(n, dtype=torch.complex64, device="cuda"), torch.empty(n, dtype=torch.complex64, device="cuda")
    d_s = torch.empty(cap, dtype=torch.complex64, device="cuda")
    d_p = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_bits = torch.zeros(2 * (cap + 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert mod.work_device(len(stream), d_sent, d_x, 0, n, stream=st) == n == 8 * len(stream)
    agc.work_device(n, d_x, d_a, stream=st)
    fll.work_device(n, d_a, d_f, stream=st)
    pcs.work_device(n, d_f, cap, d_s, d_p, stream=st)
    st.synchronize()
    nsym = int(d_p.cpu()[0])
    assert pcs.slips(0) == 0 and nsym > 4 * len(stream) - 100
    # the buffers of the rest of the chain, all there before anything more is queued
    nbits = 2 * nsym
    max_msgs = 5
    ca = g.correlate_access_code_bb(packet_ref.default_access_code(), 12)
    fr = g.framer_sink_1_batch(1, nbits)
    chk = g.packet_check()
    v = fr.device_view()
    d_flagged = torch.zeros(nbits, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(v["pool_stride"], dtype=torch.uint8, device="cuda")
    d_ok = torch.full((max_msgs,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rx.work_device(nsym, d_s, d_bits, stream=st)
    ca.work_device(nbits, d_bits, d_flagged, stream=st)
    fr.run_device(d_flagged, nbits, None, nbits, stream=st)
    chk.work_device(1, max_msgs, v["d_recs"], v["rec_stride"], v["d_counts"], v["count_stride_words"], v["d_pool"],
                    v["pool_stride"], True, d_out, d_ok, stream=st)
    st.synchronize()
    assert list(d_ok.cpu().numpy()) == [1, 1, 1, 0, 0]
    out = d_out.cpu().numpy()
    at = 0
    for p in payloads:
        assert out[at:at + len(p)].tobytes() == p
        at += len(p) + 4
    assert [(o, len(m)) for o, m in fr.messages(st)[0]] == [(o, len(p) + 4) for o, p in zip(packet_ref.RF_OFFSETS, payloads)]
