"""What tests/test_gpu_carry_levels.py and tests/test_carry_levels_cpu.py share: the sizes at which the chunked scans'
carry passes enter their second group, the inputs that cross them, and the references that are not a restatement's.

The chunked recurrences reduce every tile or chunk, chain the partial results in a carry pass and walk the tiles again
from their start values.  Several carry passes are grouped themselves (64 tiles per turn of a wavefront, or several
tiles per lane of a workgroup); the sizes below are the smallest that reach the second group.  The constants are written
out with their csrc/ origin; test_carry_levels_cpu.py holds every one of them to the header's text, so that a retuned
tile does not silently turn the GPU tests back into tests of the first group."""
import numpy as np

import agc_ref

FM_TILE = 2048              # csrc/cpm_blocks.h: FM_THREADS * FM_PER (the handle's frequency_modulator_fc_tile())
FM_GROUP = 64               # csrc/cpm.hip, fm_carry_kernel: for (long long base = 0; base < ntiles; base += 64)
AGC_CHUNK = 256             # csrc/agc.h (agc_cc.chunk())
AGC_GROUP = 64              # csrc/agc.hip, agc_carry_kernel: for (int base = 0; base < nch; base += 64)
DIFF_TILE = 2048            # csrc/modulator_plan.h: DIFF_THREADS * DIFF_PER_LANE
DIFF_THREADS = 256          # csrc/modulator_plan.h; csrc/modulator.hip, diff_carry_kernel: per = ceil(tiles / DIFF_THREADS)
MOD_MAX_TILE = 1024         # csrc/modulator.h: outputs of a tile of the fused modulator at most
CRC_THREADS = 256           # csrc/packet.h
CRC_PASS_BYTES = 16384      # csrc/packet.h: CRC_THREADS * CRC_LANE_BYTES
ENC_CHUNK = 256             # csrc/trellis.h
IIR_CHUNK = 256             # csrc/iir.h (iir_filter_ffd.chunk()) and csrc/spectrum.h
WAVE = 64                   # lanes of a wavefront: the block of enc_walk_kernel and iirffd_chunk_kernel

AGC_LENGTHS = (AGC_GROUP * AGC_CHUNK, AGC_GROUP * AGC_CHUNK + 1, 2 * AGC_GROUP * AGC_CHUNK + 37)
AGC_SETS = (0, 3)
# chunks behind the first 64 that agc_ref.chunk_triples flags for set 3 at the longest length: at least 5 are asked
# for, these were counted
AGC_FLAGGED_BEHIND = {"agc_cc": 15, "agc_ff": 12}


def agc_input(block, n, first=0):
    """n items of the test signal's six repeats (seeds 1, 2, 3, 1, 2, 3), rotated by `first` seeds for further streams"""
    seeds = [(first + k) % 3 + 1 for k in range(6)]
    x = np.concatenate([agc_ref.signal(s, block) for s in seeds])
    assert len(x) >= n
    return np.ascontiguousarray(x[:n])


def agc_flagged_behind(block, x, params):
    """how many chunks from AGC_GROUP on are flagged: agc_carry_kernel walks those serially with base >= 64"""
    return int(sum(agc_ref.chunk_triples(block, x, params)[1][AGC_GROUP:]))


def update_crc32_fast(crc, data):
    """packet_ref.update_crc32(crc, data) for long buffers of at least four bytes.  The register is linear over GF(2)
    in (start value, data) together, and a start value acts as if XORed onto the first four bytes (MSB first), so
    update(c, d) = update(0xFFFFFFFF, d ^ pad(c ^ 0xFFFFFFFF)) = crc32(d ^ pad(c ^ 0xFFFFFFFF)) ^ 0xFFFFFFFF;
    tests/test_carry_levels_cpu.py holds it to update_crc32 itself."""
    import packet_ref
    d = np.array(data, np.uint8)
    assert len(d) >= 4
    d[:4] ^= np.frombuffer(((int(crc) ^ 0xFFFFFFFF) & 0xFFFFFFFF).to_bytes(4, "big"), np.uint8)
    return packet_ref.crc32_fast(d) ^ 0xFFFFFFFF


def diff_encoder_cumsum(x, modulus, last_out=0):
    """gr_diff_encoder_bb for a modulus of at most 256, where the byte store changes nothing: a prefix sum modulo the
    modulus from last_out.  Returns (out, last_out)."""
    assert 1 <= modulus <= 256
    x = np.asarray(x, np.uint8)
    out = ((int(last_out) + np.cumsum(x.astype(np.int64))) % modulus).astype(np.uint8)
    return out, (int(out[-1]) if len(out) else int(last_out))
