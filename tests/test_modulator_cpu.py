"""The modulator's blocks without a device: the restatement (tests/modulator_ref.py) against tests/golden/ref_generic_mod.npz,
which was recorded from the reference's own gr_packed_to_unpacked_XX.cc.t, gr_unpacked_to_packed_XX.cc.t,
gr_chunks_to_symbols_XX.cc.t (expanded for bb / bc), gr_diff_encoder_bb.cc, gr_map_bb.cc and
gr_pfb_arb_resampler_ccf.cc on gr_fir_ccf_generic, compiled unchanged against stub headers; the scan form of the encoder
against its serial loop; the reference's QA vectors; the header's declarations; csrc/modulator_plan.h under the
sanitizers; and the loop through the restated receive chain.

The recording holds, per modulator case, the output's length, its first 512 samples and the SHA-256 of all of it (the
samples of all 56 cases would be 2.6 MB).  The reference gave the same samples whether the symbols reached its
resampler in one piece or cut at 97 bytes' worth; cutting at 4097 bytes is past the recording's 600 bytes."""
import ctypes as C
import hashlib
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import constellation_ref as KR
import demod_chain_ref as D
import fll_ref as FR
import modulator_ref as MR

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "..", "gnuradio-3.5.0-dmr_amd", "host")
FIX = np.load(os.path.join(HERE, "golden", "ref_generic_mod.npz"))
DATA = FIX["data"]
NB = 100                # bytes the byte blocks were recorded on
MODULI = (1, 2, 3, 4, 8, 200, 256, 257, 300, 510, 511, 1000)
CONS = {"bpsk": lambda: KR.Constellation("bpsk"), "dqpsk": lambda: KR.Constellation("dqpsk"),
        "qpsk": lambda: KR.Constellation("qpsk"), "8psk": lambda: KR.Constellation("8psk"),
        "psk16": lambda: KR.psk_constellation(16), "qam16": lambda: KR.qam_constellation(16),
        "qam64": lambda: KR.qam_constellation(64)}


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


@pytest.mark.parametrize("k", range(1, 9))
def test_repackers_equal_the_recording(k):
    for e in (MR.MSB_FIRST, MR.LSB_FIRST):
        for per in (0, 7):              # one call; calls of 7 outputs
            a = MR.run_in_calls(MR.PackedToUnpacked(k, e), DATA[:NB], per or None)
            b = MR.run_in_calls(MR.UnpackedToPacked(k, e), DATA[:NB], per or None)
            assert a.tolist() == FIX["p2u_k%d_e%d_c%d" % (k, e, per)].tolist(), (e, per)
            assert b.tolist() == FIX["u2p_k%d_e%d_c%d" % (k, e, per)].tolist(), (e, per)


def test_encoder_and_symbol_table_equal_the_recording():
    for m in MODULI:
        assert MR.diff_encoder_serial(DATA, m)[0].tolist() == FIX["denc_m%d" % m].tolist(), m
        a, last = MR.diff_encoder_serial(DATA[:257], m)                 # last_out carried over a cut
        b, _ = MR.diff_encoder_serial(DATA[257:], m, last)
        assert np.concatenate([a, b]).tolist() == FIX["denc_m%d" % m].tolist(), m
    for d in (1, 2):
        assert bits(MR.chunks_to_symbols(DATA[:NB], FIX["c2s_table%d" % d], d)).tolist() == bits(FIX["c2s_d%d" % d]).tolist()
    assert not MR.chunks_to_symbols([2, 3], FIX["c2s_table1"][:5], 2)[2:].any()          # 3 * 2 + 2 > 5: zeros, the stated deviation
    assert MR.map_bb([0, 1, 2, 3, 4, 255], [0, 1, 3, 2]).tolist() == [0, 1, 3, 2, 4, 255]


@pytest.mark.parametrize("name", sorted(CONS))
def test_modulator_equals_the_recording(name):
    """bit for bit for the samples: length, head and digest of every recorded case"""
    c = CONS[name]()
    for diff in (0, 1):
        for sps in (2.0, 2.5, 3.0, 4.0):
            key = "mod_%s_d%d_s%s" % (name, diff, ("%g" % sps).replace(".", "p"))
            y = MR.generic_mod(c, DATA, sps, bool(diff))
            head = FIX[key + "_head"]
            assert len(y) == int(FIX[key + "_n"]), key
            assert bits(y[:len(head)]).tolist() == bits(head).tolist(), key
            assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).digest() == FIX[key + "_sha256"].tobytes(), key
    # qpsk's code is applied by the modulator although apply_pre_diff_code() is false: without it the samples differ
    if name == "qpsk":
        assert not c.apply_pre_diff_code and c.pre_diff_code == [0, 2, 3, 1]
        y = MR.generic_mod(c, DATA, 2.0, False, gray_coded=False)
        assert bits(y[:512]).tolist() != bits(FIX["mod_qpsk_d0_s2_head"]).tolist()


def test_fixture_size():
    assert os.path.getsize(os.path.join(HERE, "golden", "ref_generic_mod.npz")) < 300 * 1024


@pytest.mark.parametrize("lo, hi", ((1, 65), (65, 129), (129, 193), (193, 257)))
def test_scan_form_equals_the_serial_loop_up_to_256(lo, hi):
    """the encoder the way the kernels run it (tile sums, carries, lane sums, the lanes' scan) for every modulus up to
    256, on bytes above the modulus, over three tiles plus one item and from a last_out that is not 0"""
    rng = np.random.RandomState(lo)
    x = rng.randint(0, 256, 3 * MR.SCAN_TILE + 1).astype(np.uint8)
    for m in range(lo, hi):
        assert MR.diff_scan_modulus(m) == m
        for last in (0, m - 1):
            want, wl = MR.diff_encoder_serial(x, m, last)
            got, gl = MR.diff_encoder_scan(x, m, last)
            assert got.tolist() == want.tolist() and gl == wl, (m, last)


def test_scan_form_equals_the_serial_loop_above_510():
    rng = np.random.RandomState(5)
    x = rng.randint(0, 256, 3 * MR.SCAN_TILE + 1).astype(np.uint8)
    x[:600] = 255                                                       # in + last_out reaches 510
    for m in (511, 512, 600, 1000, 65536, 2 ** 32 - 1):
        assert MR.diff_scan_modulus(m) == 256
        for last in (0, 255):
            want, wl = MR.diff_encoder_serial(x, m, last)
            got, gl = MR.diff_encoder_scan(x, 256, last)
            assert got.tolist() == want.tolist() and gl == wl, (m, last)
    for n in (1, 2, 7, MR.SCAN_TILE, MR.SCAN_TILE + 1):
        assert MR.diff_encoder_scan(x[:n], 256)[0].tolist() == MR.diff_encoder_serial(x[:n], 511)[0].tolist()


def test_scan_form_fails_between_257_and_510():
    """so the serial route of those moduli cannot be dropped silently: neither the sum modulo the modulus nor the sum
    modulo 256 is the serial loop there"""
    x = np.random.RandomState(9).randint(0, 256, 4000).astype(np.uint8)
    x[:3] = (255, 0, 255)               # 255 + 255: the one sum that 510 reduces, to 0 where the byte store alone gives 254
    for m in (257, 300, 510):
        assert MR.diff_scan_modulus(m) == 0
        want = MR.diff_encoder_serial(x, m)[0]
        assert MR.diff_encoder_scan(x, m)[0].tolist() != want.tolist()
        assert MR.diff_encoder_scan(x, 256)[0].tolist() != want.tolist()
    assert MR.diff_encoder_serial([255, 255, 50, 0, 252], 300)[0].tolist() == [255, 210, 4, 4, 0]     # csrc/modulator_plan.h's example


def test_qa_vectors_and_round_trips():
    with open(os.path.join(HERE, "golden", "ref_qa_modulator.json")) as f:
        cases = json.load(f)["cases"]
    assert [c["test"] for c in cases] == ["%03d" % i for i in range(1, 9)]
    for c in cases:
        cls = MR.PackedToUnpacked if c["block"] == "packed_to_unpacked_bb" else MR.UnpackedToPacked
        blk = cls(c["bits_per_chunk"], MR.MSB_FIRST if c["endianness"] == "MSB" else MR.LSB_FIRST)
        assert MR.run_in_calls(blk, np.asarray(c["src"], np.uint8), None).tolist() == c["expected"], c["test"]
    # qa_packed_to_unpacked.py tests 009-011: through both blocks and back, 3 bits (202 bytes give 201), 7 bits both ways
    # (56 bytes are 64 chunks), and 8 bits; the bytes are seeded here
    for k, e, n, back in ((3, MR.MSB_FIRST, 202, 201), (3, MR.LSB_FIRST, 202, 201), (7, MR.MSB_FIRST, 56, 56), (7, MR.LSB_FIRST, 56, 56),
                          (8, MR.MSB_FIRST, 64, 64), (8, MR.LSB_FIRST, 64, 64)):
        random.seed(0)
        src = np.asarray([random.randint(0, 255) for _ in range(n)], np.uint8)
        for per in (None, 1, 7):
            chunks = MR.run_in_calls(MR.PackedToUnpacked(k, e), src, per)
            assert chunks.max() < 2 ** k
            got = MR.run_in_calls(MR.UnpackedToPacked(k, e), chunks, per)
            assert len(got) >= back - (0 if per is None else 1) and got.tolist() == src[:len(got)].tolist(), (k, e, per)


PACK_OPS = ("create", "destroy", "set_mode", "set_streams", "forecast", "general_work", "general_work_device")
BYTE_OPS = ("create", "destroy", "set_mode", "set_streams", "work", "work_device")
MOD_OPS = ("create", "destroy", "set_mode", "set_streams", "set_engine", "engine", "bits_per_symbol", "samples_per_symbol", "ntaps",
           "taps", "max_produced", "work", "work_device")
ENTRIES = ([(b, op) for b in ("packed_to_unpacked_bb", "unpacked_to_packed_bb") for op in PACK_OPS]
           + [("diff_encoder_bb", op) for op in BYTE_OPS] + [("chunks_to_symbols_bc", op) for op in BYTE_OPS + ("D",)]
           + [("generic_mod", op) for op in MOD_OPS])


def test_new_entries_are_declared_and_exported(g):
    sig = g.binding.signatures()
    lib = g.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", g.binding.lib_path()], stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r"\bT (grhip_\w+)", nm))
    for n in ["grhip_%s_%s" % e for e in ENTRIES]:
        assert n in sig and hasattr(lib, n) and n in exported, n
    for cls in ("packed_to_unpacked_bb", "unpacked_to_packed_bb", "GR_MSB_FIRST", "GR_LSB_FIRST", "diff_encoder_bb", "chunks_to_symbols_bc",
                "generic_mod", "psk_mod", "qam_mod", "bpsk_mod", "dbpsk_mod", "qpsk_mod", "dqpsk_mod"):
        assert hasattr(g, cls) and cls in g.__all__, cls
    assert (g.GR_MSB_FIRST, g.GR_LSB_FIRST) == (0, 1)
    with open(os.path.join(HERE, "..", "include", "grhip.h")) as f:
        text = f.read()
    assert re.search(r"#define GRHIP_MSB_FIRST 0\b", text) and re.search(r"#define GRHIP_LSB_FIRST 1\b", text)
    p = C.c_void_p
    for b in ("packed_to_unpacked_bb", "unpacked_to_packed_bb"):
        assert sig["grhip_%s_create" % b] == (C.c_int, [p, C.c_uint, C.c_int, C.c_int])
        assert sig["grhip_%s_forecast" % b] == (C.c_int, [p, C.c_int])
        assert sig["grhip_%s_general_work" % b] == (C.c_int, [p, C.c_int, C.c_int, p, p, p])
        assert sig["grhip_%s_general_work_device" % b] == (C.c_int, [p, C.c_int, C.c_int, p, p, p, p])
    assert sig["grhip_diff_encoder_bb_create"] == (C.c_int, [p, C.c_uint, C.c_int])
    assert sig["grhip_diff_encoder_bb_work_device"] == (C.c_int, [p, C.c_int, p, p, p])
    assert sig["grhip_chunks_to_symbols_bc_create"] == (C.c_int, [p, p, C.c_size_t, C.c_int, C.c_int])
    assert sig["grhip_generic_mod_create"] == (C.c_int, [p, p, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int])
    assert sig["grhip_generic_mod_max_produced"] == (C.c_longlong, [p, C.c_int])
    assert sig["grhip_generic_mod_samples_per_symbol"] == (C.c_double, [p])
    assert sig["grhip_generic_mod_work"] == (C.c_int, [p, C.c_int, p, p, C.c_longlong, p])
    assert sig["grhip_generic_mod_work_device"] == (C.c_int, [p, C.c_int, p, p, C.c_longlong, C.c_longlong, p, p])


def test_refusals_come_before_the_device(g):
    """refused with GRHIP_EINVAL whether or not a device is there"""
    dq = g.constellation_dqpsk()
    bad = [lambda: g.packed_to_unpacked_bb(0), lambda: g.packed_to_unpacked_bb(9), lambda: g.unpacked_to_packed_bb(0),
           lambda: g.unpacked_to_packed_bb(9), lambda: g.packed_to_unpacked_bb(3, 2), lambda: g.unpacked_to_packed_bb(3, -1),
           lambda: g.diff_encoder_bb(0), lambda: g.chunks_to_symbols_bc([], 1), lambda: g.chunks_to_symbols_bc([1, 2], 0),
           lambda: g.chunks_to_symbols_bc(np.zeros(65537), 1),
           lambda: g.generic_mod(dq, 1.99), lambda: g.generic_mod(dq, 12), lambda: g.generic_mod(dq, float("nan")),
           lambda: g.generic_mod(g.constellation_calcdist([1, 1, -1, -1], [], 1, 2), 2),            # dimensionality 2
           lambda: g.generic_mod(g.constellation_calcdist([1], [], 1, 1), 2),                       # no bits
           lambda: g.generic_mod(dq, 2, excess_bw=float("inf"))]
    for make in bad:
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1, str(e.value)
    lib = g.lib()
    for name in ("packed_to_unpacked_bb", "unpacked_to_packed_bb", "diff_encoder_bb", "chunks_to_symbols_bc", "generic_mod"):
        assert getattr(lib, "grhip_%s_set_mode" % name)(None, 0) == -1 and getattr(lib, "grhip_%s_set_streams" % name)(None, 1) == -1
        getattr(lib, "grhip_%s_destroy" % name)(None)
    assert lib.grhip_generic_mod_max_produced(None, 1) == -1 and lib.grhip_generic_mod_create(None, dq._h, 2.0, 1, 0.35, 1, 0) == -1
    pp = C.c_void_p(0)
    assert lib.grhip_generic_mod_create(C.byref(pp), None, 2.0, 1, 0.35, 1, 0) == -1
    assert lib.grhip_chunks_to_symbols_bc_create(C.byref(pp), None, 4, 1, 0) == -1
    with pytest.raises(ValueError):
        g.qpsk_mod(gray_coded=False)
    for wrapper in (g.bpsk_mod, g.dbpsk_mod, g.qpsk_mod, g.dqpsk_mod):
        with pytest.raises(ValueError):
            wrapper(8)
    with pytest.raises(ValueError):
        g.psk_mod(6)


def test_modulator_plan_test_builds_and_passes():
    """csrc/modulator_plan.h under the address and undefined-behaviour sanitizers: no device, its own main"""
    r = subprocess.run(["make", "-C", HOST, "modulator_plan_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([os.path.join(HOST, "modulator_plan_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "modulator_plan_test ok" in r.stdout, r.stdout


def test_loop_back_on_the_restatements():
    """1024 seeded bytes through the restated modulator (dqpsk, 2 samples per symbol: 4096 symbols, 8192 samples) and the
    restated receive chain: behind the prefix every bit comes back at the pinned lag, clean and with noise of 0.01 and
    0.02 per component, and at no neighbouring lag"""
    sent = MR.loop_bytes()
    x = MR.generic_mod(KR.Constellation("dqpsk"), sent, MR.LOOP_SPS, True)
    assert len(x) == 8 * MR.LOOP_BYTES
    rms, peak = float(np.sqrt((np.abs(x) ** 2).mean())), float(np.abs(x).max())
    assert 0.99 < rms < 1.01 and 1.5 < peak < 1.6
    fll_taps = FR.design(D.FLL[0], D.FLL[1], D.FLL[2])
    for noise in MR.LOOP_NOISE:
        rng = np.random.RandomState(1)
        xx = (x + noise * (rng.randn(len(x)) + 1j * rng.randn(len(x)))).astype(np.complex64)
        got = D.restated_chain(xx, fll_taps)
        assert len(got) // 2 > 4 * MR.LOOP_BYTES - 100
        found = []
        for lag in MR.LOOP_LAGS:
            errors, compared = MR.loop_bit_errors(got, sent, lag)
            assert compared > 2 * (4 * MR.LOOP_BYTES - MR.LOOP_PREFIX - 100)
            if errors == 0:
                found.append(lag)
            else:
                assert errors > compared // 4, (noise, lag, errors)
        print("noise %g: rms %.3f peak %.2f, %d symbols out, no bit error at lag(s) %s" % (noise, rms, peak, len(got) // 2, found))
        assert found == [MR.LOOP_LAG], noise
