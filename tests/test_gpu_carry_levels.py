"""The chunked scans past the first group of their carry pass.

Every recurrence with a parallel form reduces its tiles or chunks, chains the partial results in a carry pass and walks
the tiles again from their start values.  The other GPU tests stop at "three tiles and a bit"; here every call is long
enough for the carry pass itself to enter its second group (tests/carry_levels.py names the thresholds and their csrc/
origin, tests/test_carry_levels_cpu.py holds them to the headers):

  frequency_modulator_fc, cpmmod_bc, gmsk_mod   fm_carry_kernel's second turn of 64 tiles (csrc/cpm.hip)
  agc_cc, agc_ff                                agc_carry_kernel's second turn of 64 chunks, its serial fallback with
                                                base = 64, and agc_chunk_walk_kernel's second workgroup (csrc/agc.hip)
  diff_encoder_bb, generic_mod engine 1         diff_carry_kernel with several tiles per lane (csrc/modulator.hip)
  crc32                                         crc_finish_kernel's second turn over the partial CRCs (csrc/packet.hip)
  trellis_encoder_bb                            enc_walk_kernel's second workgroup, a stream boundary inside a wavefront
  iir_filter_ffd                                one stream over several workgroups of iirffd_chunk_kernel (csrc/iir.hip)

No contract is stated here: the helpers and bounds are those of the blocks' own test files and restatements."""
import functools

import numpy as np
import pytest
import torch

import agc_ref
import carry_levels as CL
import constellation_ref as KR
import cpm_ref
import device_offsets as do
import iir_ref
import modulator_ref as MR
import packet_ref
import test_constellation_cpu as TC
import trellis_ref as tr
from test_gpu_agc import check_bound, make, run, same_bits
from test_gpu_cpm import SENS, make_hier, run_fm, run_hier

pytestmark = pytest.mark.gpu


# ---- frequency_modulator_fc ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_frequency_modulator_past_64_tiles(gpu, mode, S):
    """a random walk of the phase: a tile sum dropped or taken twice is an error of order 1 from there on"""
    T = gpu.frequency_modulator_fc_tile()
    assert T == CL.FM_TILE
    G = CL.FM_GROUP
    rng = np.random.RandomState(21)
    lengths = (G * T, G * T + 1, (G + 1) * T, 2 * G * T + 5)
    for n in lengths:
        x = rng.standard_normal((S, n)).astype(np.float32)
        run_fm(gpu, getattr(gpu, mode), x, SENS, [n])
        if n == lengths[-1]:
            # the second call enters with a wrapped phase that is not zero and still has more than 64 tiles
            assert n - (G * T + 1) > G * T
            run_fm(gpu, getattr(gpu, mode), x, SENS, [G * T + 1, n - (G * T + 1)])


@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_frequency_modulator_equal_tile_sums(gpu, mode):
    """a constant input: every tile sum is the same, and a carry off by whole tiles still shows, since 0.37 * 2048 is no
    multiple of 2 pi"""
    T = gpu.frequency_modulator_fc_tile()
    G = CL.FM_GROUP
    n = 2 * G * T + 5
    assert min(abs(SENS * T * k / (2 * np.pi) - round(SENS * T * k / (2 * np.pi))) for k in range(1, 2 * G + 1)) > 1e-3
    x = np.ones((1, n), np.float32)
    run_fm(gpu, getattr(gpu, mode), x, SENS, [n])
    run_fm(gpu, getattr(gpu, mode), x, SENS, [G * T + 1, n - (G * T + 1)])


# ---- cpmmod_bc, gmsk_mod ---------------------------------------------------------------------------------------------
HIER_LEGS = (("MODE_FAST", None, 1), ("MODE_FAST", 0, 0), ("MODE_GENERIC", None, 0))       # mode, set_engine, engine()


@pytest.mark.parametrize("leg", HIER_LEGS, ids=lambda l: "%s-engine%d" % (l[0], l[2]))
def test_cpmmod_bc_past_64_tiles(gpu, leg):
    mode, engine, want_engine = leg
    T = gpu.cpmmod_bc.tile()
    assert T == CL.FM_TILE
    sps, L, h, beta = 8, 4, 0.5, 0.3
    nsym = CL.FM_GROUP * T // sps + 12
    taps = gpu.cpm_phase_response(cpm_ref.GAUSSIAN, sps, L, beta)
    items = np.random.RandomState(31).randint(-128, 128, (1, nsym)).astype(np.int8).view(np.uint8)
    for chunks in ([nsym], [7, nsym - 7]):
        assert chunks[-1] * sps > CL.FM_GROUP * T
        blk = make_hier(gpu, lambda: gpu.cpmmod_bc(cpm_ref.GAUSSIAN, h, sps, L, beta), getattr(gpu, mode), engine)
        assert blk.engine() == want_engine
        run_hier(gpu, blk, lambda: cpm_ref.Chain(taps, sps, cpm_ref.cpm_sensitivity(h)), items, chunks)


@pytest.mark.parametrize("leg", HIER_LEGS, ids=lambda l: "%s-engine%d" % (l[0], l[2]))
def test_gmsk_mod_past_64_tiles(gpu, leg):
    mode, engine, want_engine = leg
    T = gpu.cpmmod_bc.tile()
    sps, bt = 8, 0.35
    nbytes = CL.FM_GROUP * T // (8 * sps) + 1                    # 2049 bytes, 64 outputs each
    assert nbytes * 8 * sps > CL.FM_GROUP * T
    taps = gpu.gmsk_mod_taps(sps, bt)
    items = np.random.RandomState(32).randint(0, 256, (1, nbytes)).astype(np.uint8)
    blk = make_hier(gpu, lambda: gpu.gmsk_mod(sps, bt), getattr(gpu, mode), engine)
    assert blk.engine() == want_engine
    run_hier(gpu, blk, lambda: cpm_ref.Chain(taps, sps, cpm_ref.gmsk_sensitivity(sps), True), items, [nbytes])


# ---- agc_cc, agc_ff --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def agc_reference(block, pi, first):
    """input, the serial restatement's outputs and gains and the float64 track at the longest length; all are causal,
    so a shorter call's are their fronts"""
    x = CL.agc_input(block, CL.AGC_LENGTHS[-1], first)
    params = agc_ref.AGC_SETS[pi]
    r = agc_ref.serial(block, x, params)
    g64 = agc_ref.exact64(block, x, params)
    for a in (x, r.out, r.gains, g64):
        a.setflags(write=False)
    return x, r.gains, g64, r.out


def check_agc(block, pi, first, n, out, gain, what):
    x, gains, g64, _ = agc_reference(block, pi, first)
    check_bound(block, x[:n], out, gain, g64[:n + 1], agc_ref.deviation(gains[:n + 1], g64[:n + 1]), what)


@pytest.mark.parametrize("pi", CL.AGC_SETS)
@pytest.mark.parametrize("block", ("agc_cc", "agc_ff"))
def test_agc_fast_past_64_chunks(gpu, block, pi):
    assert gpu.agc_cc.chunk() == CL.AGC_CHUNK
    params = agc_ref.AGC_SETS[pi]
    for n in CL.AGC_LENGTHS:
        x = agc_reference(block, pi, 0)[0][:n]
        if pi == 3 and n == CL.AGC_LENGTHS[-1]:
            # flagged chunks behind the first 64: the carry pass walks them serially with base = 64
            assert CL.agc_flagged_behind(block, x, params) >= 5
        blk = make(gpu, block, params, gpu.MODE_FAST)
        got = run(blk, [x])[0]
        check_agc(block, pi, 0, n, got, blk.gain(), "%s set %d n %d" % (block, pi, n))
    # the control: GENERIC, the serial walk, bit for bit at the longest length
    _, gains, _, out = agc_reference(block, pi, 0)
    blk = make(gpu, block, params, gpu.MODE_GENERIC)
    assert same_bits(run(blk, [x])[0], out) and agc_ref.bits(np.array([blk.gain()]))[0] == agc_ref.bits(gains[-1:])[0]


@pytest.mark.parametrize("pi", CL.AGC_SETS)
@pytest.mark.parametrize("block", ("agc_cc", "agc_ff"))
def test_agc_fast_three_streams_past_64_chunks(gpu, block, pi):
    """three streams of distinct data; n odd takes the narrow loads, n a multiple of 4 the 16-byte ones"""
    base = CL.AGC_GROUP * CL.AGC_CHUNK
    for n in (base + 1, base + 4):
        xs = [agc_reference(block, pi, k)[0][:n] for k in range(3)]
        blk = make(gpu, block, agc_ref.AGC_SETS[pi], gpu.MODE_FAST, 3)
        got = run(blk, xs)
        for k in range(3):
            check_agc(block, pi, k, n, got[k], blk.gain(k), "%s set %d S 3 n %d stream %d" % (block, pi, n, k))


# ---- diff_encoder_bb -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 2))
@pytest.mark.parametrize("modulus", (2, 7, 256))
def test_diff_encoder_past_256_tiles(gpu, modulus, S):
    """257 tiles: every lane of the carry pass chains two; 514 tiles: three, and the last lanes have none.  Two calls of
    n items each, last_out carried."""
    assert CL.DIFF_TILE == MR.SCAN_TILE
    for n in (CL.DIFF_THREADS * CL.DIFF_TILE + 1, (2 * CL.DIFF_THREADS + 1) * CL.DIFF_TILE + 1):
        tiles = -(-n // CL.DIFF_TILE)
        per = -(-tiles // CL.DIFF_THREADS)
        assert per == (2 if n < 2 * CL.DIFF_THREADS * CL.DIFF_TILE else 3)
        assert per == 2 or (CL.DIFF_THREADS - 1) * per >= tiles          # per = 3: the last lane starts behind the tiles
        x = np.random.RandomState(modulus + 7 * S).randint(0, 256, (S, 2 * n)).astype(np.uint8)
        blk = gpu.diff_encoder_bb(modulus)
        blk.set_streams(S)
        a = blk.work(np.ascontiguousarray(x[:, :n])).reshape(S, n)
        b = blk.work(np.ascontiguousarray(x[:, n:])).reshape(S, n)
        got = np.concatenate([a, b], axis=1)
        for s in range(S):
            want, _ = CL.diff_encoder_cumsum(x[s], modulus)
            bad = np.flatnonzero(got[s] != want)
            assert bad.size == 0, (modulus, n, s, int(bad[0]), int(bad.size))


# ---- generic_mod -----------------------------------------------------------------------------------------------------
GM_BYTES = 16449


@functools.lru_cache(maxsize=None)
def generic_mod_reference(differential):
    data = np.random.RandomState(41).randint(0, 256, GM_BYTES).astype(np.uint8)
    want = MR.generic_mod(KR.Constellation("bpsk"), data, 2, differential)
    for a in (data, want):
        a.setflags(write=False)
    return data, want


@pytest.mark.parametrize("engine", (0, 1))
def test_generic_mod_differential_past_256_tiles(gpu, engine):
    """dbpsk at 2 samples per symbol, GENERIC: 263184 outputs are more than 256 tiles of the fused kernel, whose symbol
    carries diff_carry_kernel chains; the same data without the encoder is the control"""
    for differential in (True, False):
        data, want = generic_mod_reference(differential)
        assert len(want) == 263184 and len(want) > CL.DIFF_THREADS * CL.MOD_MAX_TILE
        blk = gpu.generic_mod(TC.handle(gpu, KR.Constellation("bpsk")), 2, differential)
        blk.set_engine(engine)
        blk.set_mode(gpu.MODE_GENERIC)
        got = blk.work(data)
        assert len(got) == len(want)
        bad = np.flatnonzero(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
        assert bad.size == 0, (engine, differential, int(bad[0]), int(bad.size))


# ---- crc32 -----------------------------------------------------------------------------------------------------------
CRC_LENGTHS = (CL.CRC_THREADS * CL.CRC_PASS_BYTES + 15, (CL.CRC_THREADS + 1) * CL.CRC_PASS_BYTES + 17,
               (2 * CL.CRC_THREADS + 1) * CL.CRC_PASS_BYTES + 17)


@functools.lru_cache(maxsize=None)
def crc_buffer():
    buf = np.random.RandomState(51).randint(0, 256, CRC_LENGTHS[-1]).astype(np.uint8)
    buf.setflags(write=False)
    return buf


@functools.lru_cache(maxsize=None)
def crc_reference(n):
    return packet_ref.crc32_fast(crc_buffer()[:n])


@pytest.mark.parametrize("offset", (0, 5))
def test_crc_past_256_workgroups(gpu, offset):
    """one pass per workgroup: 256 partial CRCs (one turn of the finishing workgroup, full), 257 and 513 (two and three
    turns), from an aligned buffer and from one with 11 bytes in front of the first 16-byte boundary"""
    c = gpu.crc32()
    c.set_segment_bytes(CL.CRC_PASS_BYTES)
    buf = do.guarded(crc_buffer(), offset)
    assert buf.ptr() % 16 == offset
    torch.cuda.synchronize()                                    # the buffer is filled before the handle's stream starts
    for n in CRC_LENGTHS:
        groups = (n - (16 - offset) % 16) // CL.CRC_PASS_BYTES
        assert groups in (CL.CRC_THREADS, CL.CRC_THREADS + 1, 2 * CL.CRC_THREADS + 1)
        assert c.crc32_device(buf.ptr(), n) == crc_reference(n), (offset, n)
    n = CRC_LENGTHS[1]
    assert c.update_crc32_device(0xDEADBEEF, buf.ptr(), n) == CL.update_crc32_fast(0xDEADBEEF, crc_buffer()[:n]), offset


# ---- trellis_encoder_bb ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 2))
@pytest.mark.parametrize("name", ("awgn1o2_4", "gen_133_171"))
def test_trellis_encoder_past_64_lanes(gpu, name, S):
    """66 chunks per stream: the walk's second workgroup, and with two streams the boundary between them at lane 66,
    inside the second wavefront.  Two calls, the second from the first's end states."""
    f = tr.make_fsm(name)
    lf = tr.lib_fsm(gpu, name)
    n = (CL.WAVE + 1) * CL.ENC_CHUNK + 3
    assert -(-n // CL.ENC_CHUNK) > CL.WAVE and (S == 1 or -(-n // CL.ENC_CHUNK) % CL.WAVE)
    xs = np.random.RandomState(len(name) + S).randint(0, f.I, (S, 2 * n)).astype(np.uint8)
    refs = [tr.encode(f, f.S - 1, xs[s]) for s in range(S)]
    mids = [tr.encode(f, f.S - 1, xs[s, :n])[1] for s in range(S)]
    for mode in (gpu.MODE_FAST, gpu.MODE_GENERIC):
        blk = gpu.trellis_encoder_bb(lf, f.S - 1)
        blk.set_mode(mode)
        if S > 1:
            blk.set_streams(S)
        first = blk.work(np.ascontiguousarray(xs[:, :n])).reshape(S, n)
        assert [blk.ST(s) for s in range(S)] == mids, mode
        second = blk.work(np.ascontiguousarray(xs[:, n:])).reshape(S, n)
        for s in range(S):
            got = np.concatenate([first[s], second[s]])
            bad = np.flatnonzero(got != refs[s][0])
            assert bad.size == 0, (mode, s, int(bad[0]), int(bad.size))
            assert blk.ST(s) == refs[s][1], (mode, s)


# ---- iir_filter_ffd --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("order4", "deemph320k"))
def test_iir_fast_one_stream_past_64_chunks(gpu, name):
    """66 chunks of one stream: two workgroups of iirffd_chunk_kernel.  order4 has five feed-forward taps, whose inputs
    reach back over the chunk edges; deemph320k a pole of 0.96, whose state is carried along many chunks."""
    assert gpu.iir_filter_ffd.chunk() == CL.IIR_CHUNK
    n = (CL.WAVE + 1) * CL.IIR_CHUNK + 3
    x = np.concatenate([iir_ref.signal(s) for s in (1, 2, 3)])[:n]
    ff, fb = iir_ref.TAP_SETS[name]
    ref, _, _ = iir_ref.serial(x, ff, fb)
    blk = gpu.iir_filter_ffd(ff, fb)
    blk.set_mode(gpu.MODE_FAST)
    assert blk.chunked()
    got = blk.work(x)
    diff = int(np.count_nonzero(iir_ref.bits(got) != iir_ref.bits(ref)))
    print("%s n %d: %d of %d outputs differ from GENERIC in bits" % (name, n, diff, n))
    assert iir_ref.within_fast_bound(got, ref), name
    # the control: GENERIC, the serial walk, bit for bit
    blk = gpu.iir_filter_ffd(ff, fb)
    blk.set_mode(gpu.MODE_GENERIC)
    got = blk.work(x)
    assert got.dtype == ref.dtype and np.array_equal(iir_ref.bits(got), iir_ref.bits(ref)), name
