"""The packet layer on the device: crc32 against the recording of digital_crc32.cc and the restated CRC, packet_maker
byte for byte against tests/packet_ref.py's make_packet, packet_check against unmake_packet, and the bit-level loop
maker -> packed_to_unpacked_bb -> correlate_access_code_bb -> framer_sink_1_batch -> device view -> packet_check with
nothing but the verdicts and payloads coming to the host.  All comparisons are exact."""
import numpy as np
import pytest
import torch

import device_offsets as do
import lfsr_ref
import packet_ref

pytestmark = pytest.mark.gpu

FX = lfsr_ref.fixture()
PASS, LANE = 16384, 64                    # csrc/packet.h: bytes a workgroup takes per pass, bytes a lane takes
BIG = 1 << 20
_RNG = np.random.RandomState(5)
BUF = _RNG.randint(0, 256, BIG).astype(np.uint8)
# one byte either side of every boundary the kernels have: the lane's run, the pass, the pass behind an unaligned head
# (15 + PASS is the first length that can leave the finishing workgroup), two passes, the segment of the knob
CRC_LENGTHS = sorted({0, 1, 3, 4, 5, 15, 16, 17, LANE - 1, LANE, LANE + 1, 255, 256, 257, PASS - 1, PASS, PASS + 1, PASS + 14,
                      PASS + 15, PASS + 16, PASS + 17, 2 * PASS - 1, 2 * PASS, 2 * PASS + 1, 3 * PASS - 1, 3 * PASS, 3 * PASS + 1,
                      3 * PASS + 16, 6 * PASS + 15, 6 * PASS + 16, 6 * PASS + 17, BIG - 1, BIG})
_REF = {}


def ref_crc(n):
    if n not in _REF:
        _REF[n] = packet_ref.crc32_fast(BUF[:n])
    return _REF[n]


def test_crc_recorded_values(gpu):
    c = gpu.crc32()
    for ln, v in zip(FX["crc_lengths"], FX["crc_values"]):
        assert c.crc32(FX["input"][:ln]) == int(v), ln
    assert [c.crc32(s) for s in (100 * b"0", 100 * b"1", 10 * b"0123456789")] == [2943744955, 2326594156, 3774345973]   # qa_crc32.py
    assert c.crc32(b"123456789") == 0xFC891918 and c.crc32(b"") == 0
    assert c.update_crc32(c.update_crc32(0xFFFFFFFF, b"1234"), b"56789") ^ 0xFFFFFFFF == 0xFC891918
    assert c.update_crc32(0x12345678, b"") == 0x12345678


@pytest.mark.parametrize("segment", [0, 3 * PASS])
def test_crc_lengths_and_the_multi_workgroup_combine(gpu, segment):
    """BIG bytes are 64 passes: with the default split as many workgroups of one pass; with the knob workgroups of three
    passes and a last one of one.  The partial CRCs are combined by the finishing workgroup either way."""
    c = gpu.crc32()
    c.set_segment_bytes(segment)
    buf = do.guarded(BUF, 0)
    torch.cuda.synchronize()                                    # the buffer is filled before the handle's stream starts
    for n in CRC_LENGTHS:
        assert c.crc32_device(buf.ptr(), n) == ref_crc(n), n
    # host buffers are staged, never computed on the CPU
    assert c.crc32(BUF[:3 * PASS + 17]) == packet_ref.crc32_fast(BUF[:3 * PASS + 17])
    for init in (0, 0xFFFFFFFF, 0xDEADBEEF):
        for n in (0, 5, 300, PASS + 17):
            assert c.update_crc32_device(init, buf.ptr(), n) == packet_ref.update_crc32(init, BUF[:n].tobytes()), (init, n)


@pytest.mark.parametrize("offset", range(16))
def test_crc_at_every_byte_offset(gpu, offset):
    c = gpu.crc32()
    c.set_segment_bytes(2 * PASS)
    n_max = 5 * PASS + 31
    buf = do.guarded(BUF[:n_max], offset)
    assert buf.ptr() % 16 == offset
    torch.cuda.synchronize()
    for n in (0, 1, 15, 16, 17, 257, PASS - 1, PASS + 14, PASS + 15, PASS + 16, 2 * PASS + 15, 2 * PASS + 16, 2 * PASS + 17, n_max):
        assert c.crc32_device(buf.ptr(), n) == ref_crc(n), (offset, n)


def test_crc_refusals(gpu):
    c = gpu.crc32()
    with pytest.raises(gpu.GrhipError):
        c.crc32_device(0, 5)
    with pytest.raises(gpu.GrhipError):
        c.crc32_device(do.guarded(BUF[:64], 0).ptr(), -1)
    with pytest.raises(gpu.GrhipError):
        c.crc32_device(do.guarded(BUF[:64], 0).ptr(), 1 << 31)
    with pytest.raises(gpu.GrhipError):
        c.set_segment_bytes(-1)
    assert c.crc32_device(0, 0) == 0                            # an empty buffer needs no address


# ---- maker and check -------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4091, 4092]
OFFSETS = [0, 1, 15, 0, 1, 15, 0, 1, 15, 0, 1, 15, 0, 1, 0]       # L + o <= 4096 throughout
CODE13 = "1010110011011"
PAYLOADS = [_RNG.randint(0, 256, n).astype(np.uint8).tobytes() for n in LENGTHS]


@pytest.mark.parametrize("whitening", [True, False])
@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("sps,bps,code", [(2, 1, None), (3, 2, CODE13), (2.9, 2, None)])
def test_maker_matches_make_packet(gpu, sps, bps, code, pad, whitening):
    kw = {} if code is None else {"access_code": code}
    mk = gpu.packet_maker(sps, bps, pad_for_usrp=pad, whitening=whitening, **kw)
    want = [packet_ref.make_packet(p, sps, bps, access_code=code, pad_for_usrp=pad, whitener_offset=o, whitening=whitening)
            for p, o in zip(PAYLOADS, OFFSETS)]
    assert [mk.packet_bytes(n) for n in LENGTHS] == [len(packet_ref.make_packet(bytes(n), sps, bps, access_code=code, pad_for_usrp=pad))
                                                     for n in LENGTHS]
    # host buffers
    assert mk.make_packets(PAYLOADS, OFFSETS) == want
    # device buffers at odd addresses, guards around the output
    jobs, tin, tout = mk.plan(LENGTHS, OFFSETS)
    assert tin == sum(LENGTHS) and tout == sum(len(w) for w in want)
    assert list(jobs["out_offset"]) == list(np.cumsum([0] + [len(w) for w in want[:-1]]))
    d_jobs = torch.from_numpy(jobs.view(np.uint32).reshape(-1).copy().view(np.int32)).cuda()
    d_in = do.guarded(np.frombuffer(b"".join(PAYLOADS), np.uint8), 5)
    d_out = do.guarded_output(tout, np.uint8, 3)
    torch.cuda.synchronize()                                    # the buffers are filled before the handle's stream starts
    mk.work_device(len(LENGTHS), d_jobs, d_in.ptr(), d_out.ptr())
    torch.cuda.synchronize()
    assert d_out.payload().tobytes() == b"".join(want)
    do.check_guards(d_out)


def test_maker_refusals(gpu):
    mk = gpu.packet_maker(2, 1)
    for lengths, offs in (([4093], [0]), ([4092], [1]), ([100], [-1]), ([100], [3993]), ([-1], [0])):
        with pytest.raises(gpu.GrhipError) as e:
            mk.plan(lengths, offs)
        assert e.value.code == -1
    jobs, _, _ = mk.plan([100], [3992])                         # the mask is read from the full offset
    assert int(jobs["whitener_offset"][0]) == 3992
    got = mk.make_packets([PAYLOADS[7]], [3992 - 36])[0]
    body = bytes(np.frombuffer(PAYLOADS[7] + packet_ref.crc32(PAYLOADS[7]).to_bytes(4, "big"), np.uint8) ^ FX["random_mask"][3956:3956 + 68])
    assert got[14:14 + 68] == body and got[10:14] == bytes([0x40, 68, 0x40, 68])          # 3956 & 0xf = 4
    with pytest.raises(gpu.GrhipError):
        mk.packet_bytes(4093)
    # records that plan() never writes, handed to the device entry: nothing is written for them, their neighbours are made
    jobs, _, tout = mk.plan([5, 5, 5, 5], [0, 0, 0, 0])
    size = mk.packet_bytes(5)
    jobs["length"][1] = 4093
    jobs["whitener_offset"][2] = 4090
    d_jobs = torch.from_numpy(jobs.view(np.uint32).reshape(-1).copy().view(np.int32)).cuda()
    d_in = torch.from_numpy(np.frombuffer(PAYLOADS[13], np.uint8).copy()).cuda()
    d_out = do.guarded_output(tout, np.uint8, 1)
    torch.cuda.synchronize()
    mk.work_device(4, d_jobs, d_in, d_out.ptr())
    torch.cuda.synchronize()
    got = d_out.payload()
    for i in (0, 3):
        assert got[i * size:(i + 1) * size].tobytes() == packet_ref.make_packet(PAYLOADS[13][5 * i:5 * i + 5], 2, 1)
    assert do.unwritten_items(d_out)[size:3 * size].all()
    do.check_guards(d_out)


def _check_inputs(dewhitening):
    """two streams of messages as the framer leaves them: records, counts, pools; and what unmake_packet says"""
    msgs = []
    for p, o in zip(PAYLOADS[:-1], OFFSETS[:-1]):               # L = 4096 never reaches a framer: its header says 0
        whole = p + packet_ref.crc32(p).to_bytes(4, "big")
        msgs.append((packet_ref.whiten(whole, o) if dewhitening else whole, o))
    flipped = []
    for k, (m, o) in enumerate(msgs):                           # one flipped bit in each, at a different place each time
        b = bytearray(m)
        b[(k * 37) % len(b)] ^= 1 << (k % 8)
        flipped.append((bytes(b), o))
    msgs = msgs + flipped + [(b"", 0), (b"abc", 2), (b"\0\0\0\0", 0), (b"\xff\xff\xff\xff", 0), (bytes(100), 4000)]
    streams = [msgs[0::2], msgs[1::2]]
    max_msgs = max(len(s) for s in streams) + 1                 # the slot behind a stream's count is not a message
    rec_stride, pool_stride = max_msgs + 3, max(sum(len(m) for m, _ in s) for s in streams) + 21
    recs = np.zeros((2, rec_stride), np.dtype([("o", np.uint32), ("len", np.uint32), ("off", np.uint32), ("pad", np.uint32)]))
    pool = np.full((2, pool_stride), 0xEE, np.uint8)
    counts = np.zeros((2, 5), np.uint32)
    want_ok = np.zeros((2, max_msgs), np.uint8)
    want_payload = {}
    for s, ms in enumerate(streams):
        at = 0
        counts[s, 0] = len(ms)
        for m, (data, o) in enumerate(ms):
            recs[s, m] = (o, len(data), at, 0)
            pool[s, at:at + len(data)] = np.frombuffer(data, np.uint8)
            if len(data) + o > 4096:                            # past the mask's end: the stated deviation, not ok, not touched
                ok, payload = False, None
            else:
                ok, payload = packet_ref.unmake_packet(data, o, dewhitening)
            want_ok[s, m] = ok
            if len(data) >= 4 and payload is not None:
                want_payload[(s, m)] = (at, packet_ref.whiten(data, o) if dewhitening else data)
            at += len(data)
        recs[s, len(ms)] = (0, 8, 0, 0)                         # what a stale slot may hold
    return recs, counts, pool, want_ok, want_payload, max_msgs, rec_stride, pool_stride


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("dewhitening", [True, False])
def test_check_matches_unmake_packet(gpu, dewhitening, in_place):
    recs, counts, pool, want_ok, want_payload, max_msgs, rec_stride, pool_stride = _check_inputs(dewhitening)
    assert want_ok.sum() == len(PAYLOADS) - 1 + (0 if dewhitening else 1)    # the good ones; CRC-32 of nothing is 0: plain b"\0\0\0\0"
    d_recs = torch.from_numpy(recs.view(np.uint32).reshape(-1).copy().view(np.int32)).cuda()
    d_counts = torch.from_numpy(counts.reshape(-1).view(np.int32).copy()).cuda()
    d_pool = do.guarded(pool, 7)
    d_out = d_pool if in_place else do.guarded_output(pool_stride, np.uint8, 9, n_streams=2)
    d_ok = do.guarded_output(2 * max_msgs, np.uint8, 1)
    chk = gpu.packet_check()
    torch.cuda.synchronize()                                    # the buffers are filled before the handle's stream starts
    chk.work_device(2, max_msgs, d_recs, rec_stride, d_counts, 5, d_pool.ptr(), pool_stride, dewhitening, d_out.ptr(), d_ok.ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_ok.payload().reshape(2, max_msgs), want_ok)
    do.check_guards(d_ok)
    got = d_out.payload()
    written = np.zeros(got.shape, bool)
    for (s, m), (at, data) in want_payload.items():
        assert got[s, at:at + len(data)].tobytes() == data, (s, m)
        written[s, at:at + len(data)] = True
    if not in_place:                                            # nothing else is written: short, over-long and stale slots
        assert do.unwritten_items(d_out).reshape(got.shape)[~written].all()
        do.check_guards(d_out)


def test_check_without_counts_and_refusals(gpu):
    recs, counts, pool, want_ok, _, max_msgs, rec_stride, pool_stride = _check_inputs(True)
    n0 = int(counts[0, 0])
    d_recs = torch.from_numpy(recs.view(np.uint32).reshape(-1).copy().view(np.int32)).cuda()
    d_pool = torch.from_numpy(pool.copy()).cuda()
    d_out = torch.zeros_like(d_pool)
    d_ok = torch.full((n0,), 7, dtype=torch.uint8).cuda()
    chk = gpu.packet_check()
    torch.cuda.synchronize()
    chk.work_device(1, n0, d_recs, rec_stride, None, 0, d_pool, pool_stride, True, d_out, d_ok)      # NULL counts: max_msgs each
    torch.cuda.synchronize()
    assert np.array_equal(d_ok.cpu().numpy(), want_ok[0, :n0])
    assert chk.work_device(0, 5, None, 0, None, 0, None, 0, True, None, None) == 0
    for args in ((1, 1, None, 1, None, 0, d_pool, 1, True, d_out, d_ok), (-1, 1, d_recs, 1, None, 0, d_pool, 1, True, d_out, d_ok),
                 (2, 4, d_recs, 3, None, 0, d_pool, 1, True, d_out, d_ok)):
        with pytest.raises(gpu.GrhipError):
            chk.work_device(*args)


# ---- the bit-level loop ----------------------------------------------------------------------------------------------
def test_bit_level_loop_ends_on_the_device(gpu):
    S = 3
    order = [[0, 3, 6, 9, 12], [1, 4, 7, 10, 13], [2, 5, 8, 11]]            # payloads of each stream; L = 4096 stays out
    mk = gpu.packet_maker(2, 1)                                             # pad_for_usrp, whitening, the default access code
    flat = [k for row in order for k in row]
    jobs, tin, tout = mk.plan([LENGTHS[k] for k in flat], [OFFSETS[k] for k in flat])
    sizes = [mk.packet_bytes(LENGTHS[k]) for k in flat]
    # the job records say where a packet goes: lay every stream's packets in a row of its own, 16 zero bytes behind
    # (the correlator's output lags its input by 64 bits)
    nbytes = max(sum(mk.packet_bytes(LENGTHS[k]) for k in row) for row in order) + 16
    at, i = 0, 0
    for s, row in enumerate(order):
        at = s * nbytes
        for k in row:
            jobs["out_offset"][i] = at
            at += sizes[i]
            i += 1
    # every buffer and handle first; then one stream orders the entries, which do not synchronise
    nbits = 8 * nbytes
    max_msgs = 6
    unp = gpu.packed_to_unpacked_bb(1, gpu.GR_MSB_FIRST)
    unp.set_streams(S)
    cas = [gpu.correlate_access_code_bb(packet_ref.default_access_code(), 12) for _ in range(S)]   # a correlator takes one stream
    fr = gpu.framer_sink_1_batch(S, nbits)
    chk = gpu.packet_check()
    v = fr.device_view()                                                    # addresses and strides are the handle's from create on
    assert v["d_recs"] and v["d_counts"] and v["d_pool"] and v["count_stride_words"] > 0 and v["rec_stride"] >= max_msgs
    d_jobs = torch.from_numpy(jobs.view(np.uint32).reshape(-1).copy().view(np.int32)).cuda()
    d_payloads = torch.from_numpy(np.frombuffer(b"".join(PAYLOADS[k] for k in flat) + b"\0", np.uint8).copy()).cuda()
    d_packed = torch.zeros(S * nbytes, dtype=torch.uint8).cuda()
    d_bits = torch.zeros(S * nbits, dtype=torch.uint8).cuda()
    d_flagged = torch.zeros(S * nbits, dtype=torch.uint8).cuda()
    d_out = torch.zeros(S * v["pool_stride"], dtype=torch.uint8).cuda()
    d_ok = torch.full((S * max_msgs,), 9, dtype=torch.uint8).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    mk.work_device(len(flat), d_jobs, d_payloads, d_packed, stream=st)
    assert unp.general_work_device(nbits, nbytes, d_packed, d_bits, stream=st) == (nbits, nbytes)
    for s in range(S):
        cas[s].work_device(nbits, d_bits[s * nbits:], d_flagged[s * nbits:], stream=st)
    fr.run_device(d_flagged, nbits, None, nbits, stream=st)
    assert fr.device_view() == v
    chk.work_device(S, max_msgs, v["d_recs"], v["rec_stride"], v["d_counts"], v["count_stride_words"], v["d_pool"],
                    v["pool_stride"], True, d_out, d_ok, stream=st)
    st.synchronize()
    ok = d_ok.cpu().numpy().reshape(S, max_msgs)
    out = d_out.cpu().numpy().reshape(S, v["pool_stride"])
    for s, row in enumerate(order):
        assert list(ok[s]) == [1] * len(row) + [0] * (max_msgs - len(row)), (s, ok[s])
        at = 0
        for k in row:
            assert out[s, at:at + LENGTHS[k]].tobytes() == PAYLOADS[k], (s, k)
            at += LENGTHS[k] + 4
    # the framer's own host path saw the same messages
    got = fr.messages(st)
    assert [[(o, len(m)) for o, m in ms] for ms in got] == [[(OFFSETS[k], LENGTHS[k] + 4) for k in row] for row in order]
