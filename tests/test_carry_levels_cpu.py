"""What tests/test_gpu_carry_levels.py stands on, checked without a device: the prefix-sum reference of diff_encoder_bb
is the serial loop, the agc input flags chunks behind the carry pass's first group, and the thresholds written in
tests/carry_levels.py are the ones in the headers and kernels of csrc/, read as text."""
import os
import re

import numpy as np
import pytest

import agc_ref
import carry_levels as CL
import modulator_ref as MR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnuradio-3.5.0-dmr_amd", "csrc")


def text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constants(name):
    """every `constexpr int NAME = expression;` of a file, the expressions over the names in front of them"""
    vals = {}
    for m in re.finditer(r"^constexpr int (\w+) = ([^;]+);", text(name), re.M):
        expr = m.group(2)
        if re.fullmatch(r"[\w\s+\-*/()]+", expr) and all(w in vals for w in re.findall(r"[A-Za-z_]\w*", expr)):
            vals[m.group(1)] = eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(vals))
    return vals


def kernel(name, kernel_name):
    """the text of one kernel: from its name in front of the argument list to the closing brace in column 0"""
    src = text(name)
    at = src.index(kernel_name + "(")
    return src[at:src.index("\n}\n", at)]


@pytest.mark.parametrize("m", (2, 7, 256))
def test_cumsum_reference_is_the_serial_loop(m):
    x = np.random.RandomState(m).randint(0, 256, 1 << 20).astype(np.uint8)
    cut = 256 * CL.DIFF_TILE + 1
    want, want_last = MR.diff_encoder_serial(x, m)
    a, last = CL.diff_encoder_cumsum(x[:cut], m)
    assert last == int(want[cut - 1])
    b, last = CL.diff_encoder_cumsum(x[cut:], m, last)
    assert np.array_equal(np.concatenate([a, b]), want) and last == want_last


def test_fast_update_crc32_is_update_crc32():
    import packet_ref
    data = np.random.RandomState(9).randint(0, 256, 3001).astype(np.uint8)
    for crc in (0, 0xFFFFFFFF, 0xDEADBEEF, 0x12345678):
        for n in (4, 5, 3001):
            assert CL.update_crc32_fast(crc, data[:n]) == packet_ref.update_crc32(crc, data[:n].tobytes()), (crc, n)


@pytest.mark.parametrize("block", ("agc_cc", "agc_ff"))
def test_agc_input_flags_chunks_behind_the_first_group(block):
    n = CL.AGC_LENGTHS[-1]
    assert n == 2 * 64 * 256 + 37
    x = CL.agc_input(block, n)
    assert np.array_equal(x, np.concatenate([agc_ref.signal(s, block) for s in (1, 2, 3, 1, 2, 3)])[:n])
    count = CL.agc_flagged_behind(block, x, agc_ref.AGC_SETS[3])
    assert count >= 5 and count == CL.AGC_FLAGGED_BEHIND[block]
    # the further streams differ from the first
    assert not np.array_equal(CL.agc_input(block, n, 1), x) and not np.array_equal(CL.agc_input(block, n, 2), x)
    for length in CL.AGC_LENGTHS:
        assert agc_ref.can_chunk(block, agc_ref.AGC_SETS[3], length) and -(-length // CL.AGC_CHUNK) >= CL.AGC_GROUP


def test_constants_are_the_headers():
    assert constants("cpm_blocks.h")["FM_TILE"] == CL.FM_TILE
    assert constants("agc.h")["AGC_CHUNK"] == CL.AGC_CHUNK == agc_ref.CHUNK
    plan = constants("modulator_plan.h")
    assert plan["DIFF_TILE"] == CL.DIFF_TILE == MR.SCAN_TILE and plan["DIFF_THREADS"] == CL.DIFF_THREADS
    assert constants("modulator.h")["MOD_MAX_TILE"] == CL.MOD_MAX_TILE
    packet = constants("packet.h")
    assert packet["CRC_PASS_BYTES"] == CL.CRC_PASS_BYTES and packet["CRC_THREADS"] == CL.CRC_THREADS
    assert constants("trellis.h")["ENC_CHUNK"] == CL.ENC_CHUNK
    assert constants("iir.h")["IIR_CHUNK"] == CL.IIR_CHUNK and constants("spectrum.h")["IIR_CHUNK"] == CL.IIR_CHUNK


def test_group_widths_are_the_kernels():
    fm = kernel("cpm.hip", "fm_carry_kernel")
    assert "for (long long base = 0; base < ntiles; base += %d) {" % CL.FM_GROUP in fm
    assert "carry += __shfl(inc, %d);" % (CL.FM_GROUP - 1) in fm
    agc = kernel("agc.hip", "agc_carry_kernel")
    assert "for (int base = 0; base < nch; base += %d) {" % CL.AGC_GROUP in agc
    assert "const long long i0 = (long long)(base + j) * AGC_CHUNK;" in agc
    walk = kernel("agc.hip", "agc_chunk_walk_kernel")
    assert "const int cbase = blockIdx.x * %d;" % CL.AGC_GROUP in walk
    diff = kernel("modulator.hip", "diff_carry_kernel")
    assert "const long long per = (tiles + DIFF_THREADS - 1) / DIFF_THREADS;" in diff
    assert "__launch_bounds__(DIFF_THREADS)\ndiff_carry_kernel(" in text("modulator.hip")
    assert "for (long long g = tid; g < groups; g += CRC_THREADS) {" in kernel("packet.hip", "crc_finish_kernel")
    # one lane per (stream, chunk) in blocks of a wavefront
    assert "dim3((unsigned)((lanes + %d) / %d)), dim3(%d)" % (CL.WAVE - 1, CL.WAVE, CL.WAVE) in text("trellis.hip")
    assert "const long long q = (long long)blockIdx.x * %d + threadIdx.x;" % CL.WAVE in kernel("iir.hip", "iirffd_chunk_kernel")
