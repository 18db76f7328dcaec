"""TEST-ONLY restatement of gri_lfsr (gnuradio-core/src/lib/general/gri_lfsr.h:103-147) and of the three blocks on it:
gr_scrambler_bb.cc:44-57, gr_descrambler_bb.cc:44-57, gr_additive_scrambler_bb.cc:46-65.  Serial, one statement of the
reference per line; tests/golden/ref_packet.npz, recorded from gri_lfsr.h compiled unchanged, is what it is held to."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_packet.npz")
M32 = 0xFFFFFFFF


class Lfsr(object):
    def __init__(self, mask, seed, reg_len):
        if reg_len > 31:
            raise ValueError("reg_len must be <= 31")               # :109-110
        self.reg, self.mask, self.seed, self.len = seed & M32, mask & M32, seed & M32, reg_len

    def _shift(self, newbit):
        self.reg = ((self.reg >> 1) | (newbit << self.len)) & M32   # :116

    def next_bit(self):
        out = self.reg & 1
        self._shift(bin(self.reg & self.mask).count("1") % 2)
        return out

    def next_bit_scramble(self, x):
        out = self.reg & 1
        self._shift((bin(self.reg & self.mask).count("1") % 2) ^ (x & 1))
        return out

    def next_bit_descramble(self, x):
        out = (bin(self.reg & self.mask).count("1") % 2) ^ (x & 1)
        self._shift(x & 1)
        return out

    def reset(self):
        self.reg = self.seed


class Block(object):
    """kind 'scrambler' | 'descrambler' | 'additive'; work(bytes) carries the state across calls"""

    def __init__(self, kind, mask, seed, reg_len, count=0):
        self.kind, self.l, self.count, self.bits = kind, Lfsr(mask, seed, reg_len), int(count), 0

    def work(self, x):
        x = np.asarray(x, np.uint8)
        out = np.zeros(len(x), np.uint8)
        l = self.l
        for i, v in enumerate(x.tolist()):
            if self.kind == "scrambler":
                out[i] = l.next_bit_scramble(v)
            elif self.kind == "descrambler":
                out[i] = l.next_bit_descramble(v)
            else:
                out[i] = v ^ l.next_bit()
                if self.count > 0:
                    self.bits += 1
                    if self.bits == self.count:
                        l.reset()
                        self.bits = 0
        return out


def whitening_table():
    """packet_utils.random_mask_tuple (packet_utils.py:198-454) generated: 4094 bytes of gri_lfsr(0x3, 0x3FFF, 14).next_bit(),
    eight to a byte, least significant bit first, then 255, 63; tests/test_packet_cpu.py holds it to the 4096 recorded
    numbers in tests/golden/ref_packet.npz"""
    l = Lfsr(0x3, 0x3FFF, 14)
    bits = np.array([l.next_bit() for _ in range(4094 * 8)], np.uint8)
    return np.concatenate([np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1), np.array([255, 63], np.uint8)])


_FIX = {}


def fixture():
    """the recorded data: params [k][mask, seed, len, count], input (6000 random bytes), and per parameter set the 6000
    outputs of the three blocks on that input (additive as out ^ in, a 0/1 bit)"""
    if not _FIX:
        z = np.load(GOLDEN)
        n = z["input"].shape[0]
        _FIX.update(params=[tuple(int(v) for v in row) for row in z["params"]], input=z["input"].copy(),
                    scrambler=np.unpackbits(z["scrambler"], axis=1)[:, :n], descrambler=np.unpackbits(z["descrambler"], axis=1)[:, :n],
                    additive=np.unpackbits(z["additive_bits"], axis=1)[:, :n] ^ z["input"][None, :],
                    random_mask=z["random_mask"].copy(), crc_lengths=z["crc_lengths"].copy(), crc_values=z["crc_values"].copy(),
                    default_access_code=z["default_access_code"].copy(), preamble=z["preamble"].copy(), qa_crc32=z["qa_crc32"].copy())
    return _FIX


def expected(kind, k, n=None):
    """the recorded output of block `kind` for parameter set k, its first n items"""
    return fixture()[kind][k][:n]
