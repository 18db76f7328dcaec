"""packed_to_unpacked_bb, unpacked_to_packed_bb, diff_encoder_bb, chunks_to_symbols_bc and generic_mod on the device, against
the restatement (tests/modulator_ref.py, itself held against the reference's recording by tests/test_modulator_cpu.py)
and against tests/golden/ref_generic_mod.npz directly.

Shapes are the smallest at which the kernels can go wrong: one item, around the 256 lanes of a workgroup, three scan
tiles of the encoder plus one item, chunks that straddle calls (calls of 1 and 7 items), 1 and 3 streams of distinct
data; for the fused modulator one byte, fewer symbols than a filter has taps, output counts of one tile of 1024 less
one, exact, plus one, and three tiles plus one, samples_per_symbol 2, 2.5 (acc != 0) and 11.5 (next to the LDS cap)."""
import hashlib
import os

import numpy as np
import pytest
import torch

import constellation_ref as KR
import device_offsets as DO
import modulator_ref as MR
import test_constellation_cpu as T

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_generic_mod.npz"))
DATA = FIX["data"]
MODES = ("MODE_FAST", "MODE_GENERIC", "MODE_FAST_VALU", "MODE_FAST_REFTAPS")
SCAN_TILE = MR.SCAN_TILE
SIZES = (1, 2, 255, 256, 257, 3 * SCAN_TILE + 1)
MOD_TILE = 1024                     # MOD_MAX_TILE of csrc/modulator.h
CONS = {"bpsk": lambda: KR.Constellation("bpsk"), "dqpsk": lambda: KR.Constellation("dqpsk"),
        "qpsk": lambda: KR.Constellation("qpsk"), "8psk": lambda: KR.Constellation("8psk"),
        "psk16": lambda: KR.psk_constellation(16), "qam16": lambda: KR.qam_constellation(16),
        "qam64": lambda: KR.qam_constellation(64)}
SPS = (2.0, 2.5, 3.0, 4.0)


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def streams(n, S, seed=5):
    return np.random.RandomState(seed + 31 * S).randint(0, 256, (S, n)).astype(np.uint8)


# ---- the four blocks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("k", (1, 3, 5, 8))
def test_pack_blocks_equal_the_restatement(gpu, k, S):
    g = gpu
    for cls, ref_cls in ((g.packed_to_unpacked_bb, MR.PackedToUnpacked), (g.unpacked_to_packed_bb, MR.UnpackedToPacked)):
        for e in (g.GR_MSB_FIRST, g.GR_LSB_FIRST):
            for n in SIZES:
                need = ref_cls(k, e).forecast(n)
                x = streams(need, S, seed=n + k)
                want = np.stack([ref_cls(k, e).general_work(n, x[s])[0] for s in range(S)])
                consumed_want = ref_cls(k, e).general_work(n, x[0])[1]
                for mode in MODES if n in (257, SIZES[-1]) else MODES[:1]:
                    blk = cls(k, e)
                    blk.set_mode(getattr(g, mode))
                    blk.set_streams(S)
                    assert blk.forecast(n) == need
                    got, consumed = blk.general_work(n, x)
                    assert consumed == consumed_want
                    assert got.reshape(S, n).tolist() == want.tolist(), (cls.__name__, e, n, mode)
            # calls of 1 and 7 items: chunks straddle the calls, the unconsumed items come again
            x = streams(24, S, seed=k)
            for per in (1, 7):
                blk = cls(k, e)
                blk.set_streams(S)
                pos, outs = 0, []
                while True:                                 # as modulator_ref.run_in_calls: the last calls shrink
                    n = per
                    while n > 0 and blk.forecast(n) > x.shape[1] - pos:
                        n -= 1
                    if n == 0:
                        break
                    y, consumed = blk.general_work(n, np.ascontiguousarray(x[:, pos:pos + blk.forecast(n)]))
                    outs.append(y.reshape(S, n))
                    pos += consumed
                got = np.concatenate(outs, axis=1)
                for s in range(S):
                    assert got[s].tolist() == MR.run_in_calls(ref_cls(k, e), x[s], per).tolist(), (cls.__name__, e, per, s)


def test_pack_blocks_on_the_qa_vectors(gpu):
    import json
    g = gpu
    with open(os.path.join(os.path.dirname(__file__), "golden", "ref_qa_modulator.json")) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        blk = getattr(g, c["block"])(c["bits_per_chunk"], g.GR_MSB_FIRST if c["endianness"] == "MSB" else g.GR_LSB_FIRST)
        n = len(c["expected"])
        got, _ = blk.general_work(n, np.asarray(c["src"], np.uint8))
        assert got.tolist() == c["expected"], c["test"]


@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("modulus", (2, 3, 256, 300, 511))
def test_diff_encoder_equals_the_serial_loop(gpu, modulus, S):
    g = gpu
    for n in SIZES:
        x = streams(2 * n, S, seed=n)                      # bytes above the modulus; two calls, last_out carried
        want = np.stack([MR.diff_encoder_serial(x[s], modulus)[0] for s in range(S)])
        for mode in MODES if n in (257, SIZES[-1]) else MODES[:1]:
            blk = g.diff_encoder_bb(modulus)
            blk.set_mode(getattr(g, mode))
            blk.set_streams(S)
            a = blk.work(np.ascontiguousarray(x[:, :n])).reshape(S, n)
            b = blk.work(np.ascontiguousarray(x[:, n:])).reshape(S, n)
            assert np.concatenate([a, b], axis=1).tolist() == want.tolist(), (n, mode)
    blk = g.diff_encoder_bb(modulus)
    assert blk.work(DATA).tolist() == FIX["denc_m%d" % modulus].tolist()
    blk.set_streams(1)                                      # last_out is 0 again
    assert blk.work(DATA[:7]).tolist() == FIX["denc_m%d" % modulus][:7].tolist()


def test_chunks_to_symbols(gpu):
    g = gpu
    for D, table in ((1, FIX["c2s_table1"]), (2, FIX["c2s_table2"])):
        for mode in MODES:
            blk = g.chunks_to_symbols_bc(table, D)
            blk.set_mode(getattr(g, mode))
            assert blk.D() == D
            assert bits(blk.work(DATA[:100])).tolist() == bits(FIX["c2s_d%d" % D]).tolist()
    rng = np.random.RandomState(3)
    # indices outside the table give zeros: a table in LDS (5 entries, D = 2: bytes 0 and 1 fit) and one read from
    # memory (5000 entries, D = 20: bytes up to 249 fit), 3 streams, sizes around a workgroup
    for ntab, D in ((5, 2), (5000, 20), (4, 1)):
        table = (rng.randn(ntab) + 1j * rng.randn(ntab)).astype(np.complex64)
        for n in (1, 255, 257, 1000):
            x = streams(n, 3, seed=n)
            x[:, ::3] = x[:, ::3] % 3                      # some that fit the small tables
            blk = g.chunks_to_symbols_bc(table, D)
            blk.set_streams(3)
            got = blk.work(x).reshape(3, n * D)
            for s in range(3):
                want = MR.chunks_to_symbols(x[s], table, D)
                assert bits(got[s]).tolist() == bits(want).tolist(), (ntab, D, n, s)
            if ntab == 5:
                assert not got[:, :].reshape(3, n, D)[x > 1].any()


def test_refusals(gpu):
    g = gpu
    E = g.GrhipError
    for cls in (g.packed_to_unpacked_bb, g.unpacked_to_packed_bb):
        for k in (0, 9):
            with pytest.raises(E):
                cls(k, g.GR_MSB_FIRST)
        with pytest.raises(E):
            cls(3, 2)
        blk = cls(3, g.GR_MSB_FIRST)
        with pytest.raises(E):
            blk.set_mode(17)
        with pytest.raises(E):
            blk.set_streams(0)
        short = blk.forecast(5) - 1
        with pytest.raises(E):                              # below what forecast asks for
            blk.general_work(5, np.zeros(short, np.uint8))
        with pytest.raises(E):
            blk.forecast(-1)
        with pytest.raises(E):                              # the bit addresses pass 2^32
            blk.forecast(2 ** 31 - 1)
        assert blk.general_work(0, np.zeros(4, np.uint8))[0].size == 0          # a no-op
        buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
        with pytest.raises(E):                              # the output overlaps the input
            blk.general_work_device(4, 16, buf.data_ptr(), buf.data_ptr() + 8)
    with pytest.raises(E):
        g.diff_encoder_bb(0)
    enc = g.diff_encoder_bb(4)
    assert enc.work(np.zeros(0, np.uint8)).size == 0
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(E):
        enc.work_device(16, buf.data_ptr(), buf.data_ptr() + 15)
    with pytest.raises(E):
        enc.work_device(-1, buf.data_ptr(), buf.data_ptr() + 32)
    for table, D in (([], 1), ([1, 2], 0), (np.zeros(65537), 1)):
        with pytest.raises(E):
            g.chunks_to_symbols_bc(table, D)
    c2s = g.chunks_to_symbols_bc([1, 1j], 1)
    assert c2s.work(np.zeros(0, np.uint8)).size == 0
    big = torch.zeros(64 * 9, dtype=torch.uint8, device="cuda")
    with pytest.raises(E):
        c2s.work_device(16, big.data_ptr() + 8, big.data_ptr())
    with pytest.raises(E):                                  # complex items not aligned to 8
        c2s.work_device(16, big.data_ptr(), big.data_ptr() + 68)
    # generic_mod
    dq = g.constellation_dqpsk()
    for sps in (1.99, 12.0, float("nan"), float("inf")):
        with pytest.raises(E):
            g.generic_mod(dq, sps)
    g.generic_mod(dq, 11.99)
    two_d = g.constellation_calcdist([1, 1j, -1, -1j, 1, -1, 1j, -1j], [], 1, 2)
    one_point = g.constellation_calcdist([1], [], 1, 1)
    for c in (two_d, one_point):
        with pytest.raises(E):
            g.generic_mod(c, 2)
    with pytest.raises(E):
        g.generic_mod(dq, 2, excess_bw=float("nan"))
    m = g.generic_mod(dq, 2)
    with pytest.raises(E):
        m.set_engine(2)
    with pytest.raises(E):
        m.set_mode(9)
    assert m.work(np.zeros(0, np.uint8)).size == 0
    d_in = torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_out = torch.full((1024,), float("nan"), dtype=torch.complex64, device="cuda")
    need = m.max_produced(16)
    with pytest.raises(E):                                  # too little room: refused before anything is written or carried
        m.work_device(16, d_in, d_out, need, need - 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_out.real).all())
    assert m.max_produced(16) == need
    m.set_streams(2)
    with pytest.raises(E):                                  # a stride shorter than what a stream produces
        m.work_device(8, d_in, d_out, m.max_produced(8) - 1, 512)
    assert g.qpsk_mod().bits_per_symbol() == 2 and g.bpsk_mod().bits_per_symbol() == 1
    with pytest.raises(ValueError):
        g.qpsk_mod(gray_coded=False)
    with pytest.raises(ValueError):
        g.bpsk_mod(4)


# ---- generic_mod --------------------------------------------------------------------------------------------------------------
def key_of(name, diff, sps):
    return "mod_%s_d%d_s%s" % (name, diff, ("%g" % sps).replace(".", "p"))


def run_cut(blk, data, cuts):
    """the output of `data` [S][n] given in calls that end at `cuts` (and at the end); produced is max_produced"""
    data = np.atleast_2d(data)
    outs, pos = [], 0
    for end in list(cuts) + [data.shape[1]]:
        end = min(end, data.shape[1])
        if end <= pos:
            continue
        want = blk.max_produced(end - pos)
        y = blk.work(np.ascontiguousarray(data[:, pos:end]))
        assert len(y) == want * data.shape[0]
        outs.append(y.reshape(data.shape[0], want))
        pos = end
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("name", sorted(CONS))
def test_generic_mod_is_the_recording_bit_for_bit(gpu, name):
    """GENERIC, engines 0 and 1: the recorded reference's output of 600 bytes uncut, cut at 97 bytes, cut at 4097 (past
    the recording's 600 bytes: one call) and, for the first 40 bytes, in calls of one byte"""
    g = gpu
    r = CONS[name]()
    c = T.handle(g, r)
    for diff in (0, 1):
        for sps in SPS:
            key = key_of(name, diff, sps)
            n, head, sha = int(FIX[key + "_n"]), FIX[key + "_head"], FIX[key + "_sha256"].tobytes()
            for engine in (0, 1):
                for cuts in ((), (97,), (4097,)):
                    blk = g.generic_mod(c, sps, bool(diff))
                    assert blk.engine() == 1
                    blk.set_engine(engine)
                    blk.set_mode(g.MODE_GENERIC)
                    y = run_cut(blk, DATA, cuts)[0]
                    assert len(y) == n, (key, engine, cuts)
                    assert bits(y[:len(head)]).tolist() == bits(head).tolist(), (key, engine, cuts)
                    assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).digest() == sha, (key, engine, cuts)
                blk = g.generic_mod(c, sps, bool(diff))
                blk.set_engine(engine)
                blk.set_mode(g.MODE_GENERIC)
                y = run_cut(blk, DATA[:40], range(1, 40))[0]
                m = min(len(y), len(head))
                assert m >= 100 and bits(y[:m]).tolist() == bits(head[:m]).tolist(), (key, engine, "bytes")


def test_generic_mod_surface(gpu):
    g = gpu
    blk = g.dqpsk_mod(samples_per_symbol=3, excess_bw=0.5)
    assert (blk.bits_per_symbol(), blk.samples_per_symbol(), blk.ntaps()) == (2, 3.0, 32 * 11 * 3 + 1)
    assert bits(blk.taps().astype(np.complex64)).tolist() == bits(MR.mod_taps(3, 0.5).astype(np.complex64)).tolist()
    # the engine may change between calls: the state is shared
    data = DATA[:300]
    blk = g.generic_mod(T.handle(g, CONS["8psk"]()), 2.5, True)
    blk.set_mode(g.MODE_GENERIC)
    parts = []
    for i, (a, b) in enumerate(((0, 77), (77, 78), (78, 200), (200, 300))):
        blk.set_engine(i % 2)
        parts.append(blk.work(data[a:b]))
    want = MR.generic_mod(CONS["8psk"](), data, 2.5, True)
    assert bits(np.concatenate(parts)).tolist() == bits(want).tolist()
    # the wrappers' defaults (psk.py, qam.py, bpsk.py, qpsk.py)
    for mod, r, diff in ((g.bpsk_mod(), CONS["bpsk"](), False), (g.dbpsk_mod(differential=False), CONS["bpsk"](), True),
                         (g.qpsk_mod(), CONS["qpsk"](), True), (g.dqpsk_mod(differential=False), CONS["dqpsk"](), True),
                         (g.psk_mod(8), KR.psk_constellation(8), True), (g.qam_mod(16, False), KR.qam_constellation(16, False), False),
                         (g.qam_mod(), CONS["qam16"](), True)):
        mod.set_mode(g.MODE_GENERIC)
        assert bits(mod.work(DATA[:50])).tolist() == bits(MR.generic_mod(r, DATA[:50], 2, diff)).tolist()
    # gray_coded=False leaves the map out
    mod = g.generic_mod(g.constellation_dqpsk(), 2, True, 0.35, False)
    mod.set_mode(g.MODE_GENERIC)
    assert bits(mod.work(DATA[:50])).tolist() == bits(MR.generic_mod(CONS["dqpsk"](), DATA[:50], 2, True, 0.35, False)).tolist()


# (constellation, samples_per_symbol, bytes, outputs per stream): the sizes of the fused kernel
FUSED_SIZES = (("dqpsk", 2.0, 1, 8), ("qam16", 2.0, 11, 44),            # one byte; 22 symbols, one fewer than a filter has taps
               ("qam64", 2.5, 307, MOD_TILE - 1), ("bpsk", 2.0, 64, MOD_TILE), ("8psk", 2.5, 154, MOD_TILE + 1),
               ("8psk", 2.5, 461, 3 * MOD_TILE + 1), ("dqpsk", 11.5, 45, 2070), ("bpsk", 11.5, 9, 828))


@pytest.mark.parametrize("name, sps, nbytes, nout", FUSED_SIZES)
def test_generic_mod_sizes_streams_and_modes(gpu, name, sps, nbytes, nout):
    """3 streams of distinct data.  GENERIC: both engines equal the restatement bit for bit, in one call and in two.
    FAST: both engines within 1e-5 of the peak of the float64 evaluation of the same schedule, taps and symbols, the
    FIR family's bound (tests/test_gpu_arb_resampler.py)."""
    g = gpu
    S = 3
    r = CONS[name]()
    c = T.handle(g, r)
    data = streams(nbytes, S, seed=nbytes)
    for diff in (True, False):
        want = [MR.generic_mod(r, data[s], sps, diff) for s in range(S)]
        want64 = [MR.generic_mod(r, data[s], sps, diff, f64=True) for s in range(S)]
        assert len(want[0]) == nout
        got = {}
        for engine in (0, 1):
            for cuts in ((), (nbytes // 3,)):
                blk = g.generic_mod(c, sps, diff)
                blk.set_streams(S)
                blk.set_engine(engine)
                blk.set_mode(g.MODE_GENERIC)
                y = run_cut(blk, data, cuts)
                for s in range(S):
                    assert bits(y[s]).tolist() == bits(want[s]).tolist(), (engine, cuts, s, diff)
            for mode in ("MODE_FAST", "MODE_FAST_VALU"):
                blk = g.generic_mod(c, sps, diff)
                blk.set_streams(S)
                blk.set_engine(engine)
                blk.set_mode(getattr(g, mode))
                y = run_cut(blk, data, (nbytes // 2,))
                peak = max(np.abs(w).max() for w in want64)
                dev = max(np.abs(y[s] - want64[s]).max() for s in range(S)) / peak
                print("generic_mod %s sps %g engine %d %s: max deviation %.3g of the peak" % (name, sps, engine, mode, dev))
                assert dev <= 1e-5
                got[(engine, mode)] = y
        assert bits(got[(0, "MODE_FAST")]).tolist() == bits(got[(0, "MODE_FAST_VALU")]).tolist()
        assert bits(got[(1, "MODE_FAST")]).tolist() == bits(got[(1, "MODE_FAST_VALU")]).tolist()


@pytest.mark.parametrize("off", tuple(range(16)))
def test_work_device_at_unaligned_pointers(gpu, off):
    """byte buffers at every offset 0 .. 15, complex outputs one item past a 256-byte boundary, odd strides; nothing
    written outside the outputs, nothing read outside the inputs (the poison around them would show)"""
    g = gpu
    S, n = 3, 77
    data = streams(n, S, seed=off)

    def done(out, written=True):
        torch.cuda.synchronize()
        DO.check_guards(out)
        if written:
            assert not DO.unwritten_items(out).any()
        return out.payload()

    # generic_mod: 8psk (chunks straddle bytes), sps 2.5, both engines, GENERIC and FAST
    r = CONS["8psk"]()
    want = [MR.generic_mod(r, data[s], 2.5, True) for s in range(S)]
    want64 = [MR.generic_mod(r, data[s], 2.5, True, f64=True) for s in range(S)]
    peak = max(np.abs(w).max() for w in want64)
    nout = len(want[0])
    d_in = DO.guarded(data, off)
    for engine in (0, 1):
        for mode, exact in (("MODE_GENERIC", True), ("MODE_FAST", False)):
            blk = g.generic_mod(T.handle(g, r), 2.5, True)
            blk.set_streams(S)
            blk.set_engine(engine)
            blk.set_mode(getattr(g, mode))
            stride = nout + 3 + 2 * (off % 2)
            d_out = DO.guarded_output(nout, np.complex64, 1 + off % 3, n_streams=S, stride_items=stride)
            assert blk.work_device(n, d_in.ptr(), d_out.ptr(), stride, nout) == nout
            y = done(d_out)
            for s in range(S):
                if exact:
                    assert bits(y[s]).tolist() == bits(want[s]).tolist(), (engine, s)
                else:
                    assert np.abs(y[s] - want64[s]).max() <= 1e-5 * peak
    # the four blocks
    for k, e in ((3, g.GR_MSB_FIRST), (5, g.GR_LSB_FIRST)):
        for cls, ref_cls in ((g.packed_to_unpacked_bb, MR.PackedToUnpacked), (g.unpacked_to_packed_bb, MR.UnpackedToPacked)):
            nn = 41
            need = ref_cls(k, e).forecast(nn)
            blk = cls(k, e)
            blk.set_streams(S)
            x = streams(need, S, seed=off + k)
            d_x = DO.guarded(x, (off * 5 + 1) % 16)
            d_out = DO.guarded_output(nn, np.uint8, off, n_streams=S)
            assert blk.general_work_device(nn, need, d_x.ptr(), d_out.ptr()) == (nn, ref_cls(k, e).general_work(nn, x[0])[1])
            y = done(d_out, written=False)
            for s in range(S):
                assert y[s].tolist() == ref_cls(k, e).general_work(nn, x[s])[0].tolist()
    for modulus in (4, 300):
        blk = g.diff_encoder_bb(modulus)
        blk.set_streams(S)
        d_out = DO.guarded_output(n, np.uint8, (off + 7) % 16, n_streams=S)
        blk.work_device(n, d_in.ptr(), d_out.ptr())
        y = done(d_out, written=False)
        for s in range(S):
            assert y[s].tolist() == MR.diff_encoder_serial(data[s], modulus)[0].tolist()
    table = FIX["c2s_table2"]
    blk = g.chunks_to_symbols_bc(table, 2)
    blk.set_streams(S)
    d_out = DO.guarded_output(2 * n, np.complex64, 1 + off % 2, n_streams=S)
    blk.work_device(n, d_in.ptr(), d_out.ptr())
    y = done(d_out)
    for s in range(S):
        assert bits(y[s]).tolist() == bits(MR.chunks_to_symbols(data[s], table, 2)).tolist()
