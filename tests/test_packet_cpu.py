"""CPU tests of the packet layer and the scramblers: the test-only restatements (tests/lfsr_ref.py, tests/packet_ref.py)
against tests/golden/ref_packet.npz -- recorded from gri_lfsr.h and digital_crc32.cc compiled unchanged, plus the 4096
numbers of packet_utils.py:198-454 --, the new entries' declarations, the refusals that need no device, and csrc/gf2.h
under the sanitizers (host/gf2_test.cc)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfsr_ref
import packet_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")
FX = lfsr_ref.fixture()

BLOCK_OPS = ("create", "destroy", "set_mode", "set_streams", "work", "work_device")
ENTRIES = [(b, op) for b in ("scrambler_bb", "descrambler_bb", "additive_scrambler_bb") for op in BLOCK_OPS] + \
          [("crc32", op) for op in ("create", "destroy", "set_segment_bytes", "compute", "update", "compute_device", "update_device")] + \
          [("packet_maker", op) for op in ("create", "destroy", "packet_bytes", "plan", "work", "work_device")] + \
          [("packet_check", op) for op in ("create", "destroy", "work_device")] + [("framer_sink_1_batch", "device_view")]


def test_fixture_shape():
    assert os.path.getsize(lfsr_ref.GOLDEN) < 64 * 1024
    assert len(FX["params"]) >= 12 and FX["input"].shape == (6000,) and FX["input"].max() > 1      # random bytes, not only 0 / 1
    lens = {p[2] for p in FX["params"]}
    assert {0, 1, 30, 31, 7, 14} <= lens
    assert {p[3] for p in FX["params"]} >= {0, 1, 7, 100, 4097}
    assert any(p[1] >> (p[2] + 1) for p in FX["params"] if p[2] < 31) and any(p[0] >> (p[2] + 1) for p in FX["params"] if p[2] < 31)
    assert (0x8a, 0x7f, 7, 0) in FX["params"] and (0x3, 0x3FFF, 14, 0) in FX["params"]
    assert len(FX["crc_lengths"]) >= 40 and FX["crc_lengths"].min() == 0 and FX["crc_lengths"].max() == 5000


@pytest.mark.parametrize("k", range(len(FX["params"])))
@pytest.mark.parametrize("kind", ["scrambler", "descrambler", "additive"])
def test_lfsr_ref_against_the_recording(kind, k):
    """all 6000 recorded items of every set, whole and cut at 7 and 4097 as the recording was: count 4097 resets inside,
    and the GPU tests take this restatement as their reference on inputs the recording does not hold"""
    mask, seed, ln, count = FX["params"][k]
    x = FX["input"]
    whole = lfsr_ref.Block(kind, mask, seed, ln, count).work(x)
    assert np.array_equal(whole, lfsr_ref.expected(kind, k))
    b = lfsr_ref.Block(kind, mask, seed, ln, count)
    cut = np.concatenate([b.work(x[a:e]) for a, e in ((0, 7), (7, 4097), (4097, 6000))])
    assert np.array_equal(cut, whole)


def test_whitening_table_is_the_lfsr():
    assert np.array_equal(lfsr_ref.whitening_table(), FX["random_mask"])
    assert tuple(FX["random_mask"][:8]) == (255, 63, 0, 16, 0, 12, 0, 5) and tuple(FX["random_mask"][-2:]) == (255, 63)


def test_library_whitening_table(g):
    assert np.array_equal(g.random_mask_vec8(), FX["random_mask"])         # host arithmetic: needs no device
    assert g.default_access_code == packet_ref.default_access_code()


def test_crc_ref_against_the_recording():
    for ln, v in zip(FX["crc_lengths"], FX["crc_values"]):
        assert packet_ref.crc32(FX["input"][:ln].tobytes()) == int(v), ln
    qa = [int(v) for v in FX["qa_crc32"]]
    assert [packet_ref.crc32(s) for s in (100 * b"0", 100 * b"1", 10 * b"0123456789")] == qa == [2943744955, 2326594156, 3774345973]
    assert packet_ref.crc32(b"123456789") == 0xFC891918 == packet_ref.crc32_fast(b"123456789")
    assert [packet_ref.crc32_fast(FX["input"][:ln]) for ln in FX["crc_lengths"]] == [int(v) for v in FX["crc_values"]]
    assert packet_ref.update_crc32(packet_ref.update_crc32(0xFFFFFFFF, b"1234"), b"56789") ^ 0xFFFFFFFF == 0xFC891918


def test_packet_ref_round_trip_and_layout():
    payload = FX["input"][:100].tobytes()
    pkt = packet_ref.make_packet(payload, 2, 1, whitener_offset=3)
    assert pkt[:2] == b"\xA4\xF2" and pkt[2:10] == bytes(FX["default_access_code"])
    assert pkt[10:14] == bytes([0x30, 104, 0x30, 104])
    assert len(pkt) == 120 and set(pkt[14 + 104:]) == {0x55}               # sps 2, bps 1: lcm(16, 2) * 1 / 2 = a byte modulus of 8
    ok, back = packet_ref.unmake_packet(pkt[14:14 + 104], 3)
    assert ok and back == payload
    bad = bytearray(pkt[14:14 + 104])
    bad[50] ^= 4
    assert packet_ref.unmake_packet(bytes(bad), 3) == (False, bytes(packet_ref.whiten(bytes(bad), 3))[:-4])
    assert packet_ref.unmake_packet(b"abc", 0) == (False, b"")
    assert packet_ref.make_packet(b"", 3, 2, access_code="1010110011011", pad_for_usrp=False, whitening=False)[:4] == b"\xA4\xF2\x15\x9B"
    with pytest.raises(ValueError):
        packet_ref.make_packet(bytes(4093), 2, 1)
    with pytest.raises(ValueError):
        packet_ref.make_packet(bytes(4092), 2, 1, whitener_offset=1)       # numpy raises past the mask's end


def test_new_entries_are_declared_and_exported(g):
    sig = g.binding.signatures()
    lib = g.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", g.binding.lib_path()], stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r"\bT (grhip_\w+)", nm))
    for n in ["grhip_%s_%s" % e for e in ENTRIES] + ["grhip_whitening_table"]:
        assert n in sig and hasattr(lib, n) and n in exported, n
    p = C.c_void_p
    assert sig["grhip_scrambler_bb_create"] == (C.c_int, [p, C.c_int, C.c_int, C.c_int, C.c_int])
    assert sig["grhip_additive_scrambler_bb_create"] == (C.c_int, [p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int])
    assert sig["grhip_crc32_update_device"] == (C.c_int, [p, C.c_uint, p, C.c_longlong, p, p])
    assert sig["grhip_packet_maker_packet_bytes"] == (C.c_longlong, [p, C.c_int])
    assert sig["grhip_packet_check_work_device"] == (C.c_int, [p, C.c_int, C.c_int, p, C.c_longlong, p, C.c_int, p, C.c_longlong,
                                                               C.c_int, p, p, p])
    assert g.PACKET_JOB.itemsize == 16 and g.PACKET_REC.itemsize == 16
    for name in ("scrambler_bb", "descrambler_bb", "additive_scrambler_bb", "crc32", "packet_maker", "packet_check"):
        assert name in g.binding.__all__ and hasattr(g, name)


def test_each_citation_is_in_the_header():
    src = open(os.path.join(ROOT, "include", "grhip.h")).read()
    for cite in ("digital_crc32.cc:45-134", "packet_utils.py:89-194", "crc.py:26-38", "packet_utils.py:198-454", "gri_lfsr.h:103-147",
                 "gr_scrambler_bb.cc:44-57", "gr_descrambler_bb.cc:44-57", "gr_additive_scrambler_bb.cc:46-65"):
        assert cite in src, cite


def test_refusals_without_a_device(g):
    bad = [lambda: g.scrambler_bb(0x8a, 0x7f, 32), lambda: g.descrambler_bb(0x8a, 0x7f, -1), lambda: g.additive_scrambler_bb(1, 1, 40, 3),
           lambda: g.packet_maker(2, 1, access_code="1" * 65), lambda: g.packet_maker(2, 1, access_code=""),
           lambda: g.packet_maker(2, 1, access_code="0120"), lambda: g.packet_maker(0.5, 1), lambda: g.packet_maker(2, 0)]
    for make in bad:
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1, str(e.value)
    lib = g.lib()
    for name in ("scrambler_bb", "descrambler_bb", "additive_scrambler_bb"):
        assert getattr(lib, "grhip_%s_work" % name)(None, 1, None, None) == -1
        assert getattr(lib, "grhip_%s_set_streams" % name)(None, 2) == -1
    out = C.c_uint(0)
    assert lib.grhip_crc32_compute(None, None, 0, C.byref(out)) == -1
    assert lib.grhip_packet_maker_packet_bytes(None, 0) == -1
    assert lib.grhip_packet_check_work_device(None, 1, 1, None, 0, None, 0, None, 0, 1, None, None, None) == -1
    assert lib.grhip_whitening_table(None, 4096) == -1
    t = np.zeros(4095, np.uint8)
    assert lib.grhip_whitening_table(t.ctypes.data, 4095) == -1


def test_no_cpu_fallback(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    for make in (lambda: g.crc32(), lambda: g.scrambler_bb(0x8a, 0x7f, 7), lambda: g.packet_maker(2, 1), lambda: g.packet_check()):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -5, str(e.value)                 # GRHIP_ENODEV


def test_gf2_test_builds_and_passes():
    """csrc/gf2.h under the address and undefined-behaviour sanitizers: no device, its own main"""
    r = subprocess.run(["make", "-C", HOST, "gf2_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([os.path.join(HOST, "gf2_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "gf2_test ok" in r.stdout, r.stdout


def test_rf_loop_stream_survives_the_restated_chain():
    """the stream of tests/test_gpu_packet_rf_loop.py through the restated modulator and receive chain that
    tests/test_modulator_cpu.py uses: every packet's bits, from the access code on, come back whole, at the pinned lag,
    with the 64 bits behind the last one that the correlator needs"""
    import constellation_ref as KR
    import demod_chain_ref as D
    import fll_ref as FR
    import modulator_ref as MR
    stream, payloads, packets = packet_ref.rf_loop_stream()
    assert [len(p) for p in payloads] == [100, 0, 257] and len(stream) == 128 + sum(len(p) for p in packets) + 32
    x = MR.generic_mod(KR.Constellation("dqpsk"), stream, MR.LOOP_SPS, True)
    got = D.restated_chain(x.astype(np.complex64), FR.design(D.FLL[0], D.FLL[1], D.FLL[2]))
    bits = bytes(np.asarray(got, np.uint8) & 1)
    at = 128
    for p in packets:
        want = bytes(np.unpackbits(np.frombuffer(p[2:], np.uint8)))
        assert bits.find(want) == 8 * (at + 2) + 2 * MR.LOOP_LAG, len(p)
        at += len(p)
    assert len(bits) >= 8 * at + 2 * MR.LOOP_LAG + 64
