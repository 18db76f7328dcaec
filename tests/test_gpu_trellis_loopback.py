"""The chain of the reference's QA (gr-trellis/src/python/qa_trellis.py:75-136) on device buffers for its three FSMs:
bits -> packed_to_unpacked_bb -> trellis_encoder_bb(f, 0) -> chunks_to_symbols_bc(constellation points) -> plus seeded
complex Gaussian noise made on the host -> trellis_constellation_metrics_cf -> trellis_viterbi_b(f, K, 0, -1) ->
unpacked_to_packed_bb, and the same chain with trellis_viterbi_combined_cb in place of the last two blocks before the
packer.  K = 2048 steps (the QA's 16384 is a workload, not a corner), N0 = 0.02: the noise has a standard deviation of 0.1
per component, so the uncoded FSMs (rep2, nothing) sit at ten standard deviations from a decision border and the
restatement returns every bit (tests/test_trellis_cpu.py).  The device must equal the restatement byte for byte and return
every bit."""
import numpy as np
import pytest
import torch

import trellis_ref as tr

pytestmark = pytest.mark.gpu

K = tr.QA_K                  # one packet, as in the QA: the encoder starts in state 0 and so does the decoder's block


def constellation_of(g, f):
    return {2: g.constellation_bpsk, 4: g.constellation_qpsk}[f.O]()       # qa_trellis.py:42-44


@pytest.mark.parametrize("name", ("qa_awgn1o2_4", "rep2", "nothing"))
def test_qa_chain_on_the_device(gpu, name):
    g = gpu
    f = tr.make_fsm(name)
    c = constellation_of(g, f)
    pts = c.points()
    sent, noise, rx, metrics = tr.qa_chain(name, pts, K, tr.QA_N0)
    n = K
    dec_ref, dead = tr.viterbi(f, K, 0, -1, metrics)
    assert dead == 0 and np.array_equal(np.packbits(dec_ref), sent)         # the restatement returns every bit

    unpack = g.packed_to_unpacked_bb(1, g.GR_MSB_FIRST)
    enc = g.trellis_encoder_bb(tr.lib_fsm(g, name), 0)
    mod = g.chunks_to_symbols_bc(pts, 1)
    met = g.trellis_constellation_metrics_cf(c, g.TRELLIS_EUCLIDEAN)
    va = g.trellis_viterbi_b(tr.lib_fsm(g, name), K, 0, -1)
    pack = g.unpacked_to_packed_bb(1, g.GR_MSB_FIRST)
    st = torch.cuda.Stream()                         # the entries do not synchronise: one stream orders the blocks
    d_sent = torch.from_numpy(sent).cuda()
    d_noise = torch.from_numpy(noise).cuda()
    d_bits = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_sym = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_x = torch.zeros(n, dtype=torch.complex64, device="cuda")
    d_m = torch.zeros(n * f.O, dtype=torch.float32, device="cuda")
    d_dec = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_back = torch.zeros(n // 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert unpack.general_work_device(n, n // 8, d_sent, d_bits, stream=st) == (n, n // 8)
    enc.work_device(n, d_bits, d_sym, stream=st)
    mod.work_device(n, d_sym, d_x, stream=st)
    with torch.cuda.stream(st):
        d_x += d_noise
    met.work_device(n, d_x, d_m, stream=st)
    va.work_device(n, d_m, d_dec, stream=st)
    assert pack.general_work_device(n // 8, n, d_dec, d_back, stream=st) == (n // 8, n)
    st.synchronize()
    assert np.array_equal(d_m.cpu().numpy().view(np.uint32), metrics.view(np.uint32))
    assert np.array_equal(d_dec.cpu().numpy(), dec_ref)
    assert np.array_equal(d_back.cpu().numpy(), sent)
    assert va.dead_ends() == 0
    # the same chain through viterbi_combined_cb, both engines
    for engine in (1, 0):
        vc = g.trellis_viterbi_combined_cb(tr.lib_fsm(g, name), K, 0, -1, 1, pts, g.TRELLIS_EUCLIDEAN)
        vc.set_engine(engine)
        assert vc.engine() == engine
        d_dec.zero_()
        d_back.zero_()
        torch.cuda.synchronize()
        vc.work_device(n, d_x, d_dec, stream=st)
        assert pack.general_work_device(n // 8, n, d_dec, d_back, stream=st) == (n // 8, n)
        st.synchronize()
        assert np.array_equal(d_x.cpu().numpy().view(np.uint32), rx.view(np.uint32))
        assert np.array_equal(d_dec.cpu().numpy(), dec_ref) and np.array_equal(d_back.cpu().numpy(), sent)
