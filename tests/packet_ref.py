"""TEST-ONLY restatement of gr-digital/python/packet_utils.py:89-194 and crc.py:26-38 in Python 3 (the reference is
Python 2 and does not run under it) over a bitwise CRC-32 (digital_crc32.cc:45-134: polynomial 0x04C11DB7, MSB first, start
and final XOR 0xFFFFFFFF).  The whitening mask is the recorded one of tests/golden/ref_packet.npz."""
import struct
from math import gcd

import numpy as np

import lfsr_ref

POLY = 0x04C11DB7


def _table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ POLY) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
        t.append(c)
    return t


_T = _table()


def update_crc32(crc, data):
    for b in bytes(data):
        crc = (_T[b ^ ((crc >> 24) & 0xff)] ^ (crc << 8)) & 0xFFFFFFFF      # digital_crc32.cc:117
    return crc


def crc32(data):
    return update_crc32(0xFFFFFFFF, data) ^ 0xFFFFFFFF                      # :133


_REV8 = np.array([int("{:08b}".format(i)[::-1], 2) for i in range(256)], np.uint8)


def crc32_fast(data):
    """crc32() for long buffers: the reflected CRC-32 of zlib over bit-reversed bytes, bit-reversed, is the unreflected
    one (the same shift register seen from the other end); tests/test_packet_cpu.py holds it to crc32() on the recording"""
    import zlib
    a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    return int("{:032b}".format(zlib.crc32(_REV8[a].tobytes()) & 0xFFFFFFFF)[::-1], 2)


def random_mask():
    return lfsr_ref.fixture()["random_mask"]


def default_access_code():
    return "".join("{:08b}".format(int(b)) for b in lfsr_ref.fixture()["default_access_code"])


def conv_1_0_string_to_packed_binary_string(s):                             # packet_utils.py:40-69
    if not s or any(ch not in "01" for ch in s):
        raise ValueError("Input must be a string containing only 0's and 1's")
    if len(s) % 8:
        s = "0" * (8 - len(s) % 8) + s
    return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def whiten(s, o):                                                           # :89-92
    sa = np.frombuffer(bytes(s), np.uint8)
    m = random_mask()[o:len(sa) + o]
    if len(m) != len(sa):
        raise ValueError("operands could not be broadcast together")        # what numpy raises past the mask's end
    return (sa ^ m).tobytes()


def make_header(payload_len, whitener_offset=0):                            # :98-102
    val = ((whitener_offset & 0xf) << 12) | (payload_len & 0x0fff)
    return struct.pack("!HH", val, val)


def npadding_bytes(pkt_byte_len, samples_per_symbol, bits_per_symbol):      # :151-172, Python 2's integer division
    lcm = 16 * samples_per_symbol // gcd(16, samples_per_symbol)
    byte_modulus = lcm * bits_per_symbol // samples_per_symbol
    r = pkt_byte_len % byte_modulus
    return 0 if r == 0 else byte_modulus - r


def make_packet(payload, samples_per_symbol, bits_per_symbol, access_code=None, pad_for_usrp=True, whitener_offset=0,
                whitening=True):                                            # :104-149
    access_code = default_access_code() if access_code is None else access_code
    packed_access_code = conv_1_0_string_to_packed_binary_string(access_code)
    packed_preamble = bytes(lfsr_ref.fixture()["preamble"])
    payload_with_crc = bytes(payload) + struct.pack(">I", crc32(payload))   # crc.py:26-28
    L = len(payload_with_crc)
    if L > 4096:
        raise ValueError("len(payload) must be in [0, 4096]")
    body = whiten(payload_with_crc, whitener_offset) if whitening else payload_with_crc
    pkt = packed_preamble + packed_access_code + make_header(L, whitener_offset) + body + b"\x55"
    if pad_for_usrp:
        pkt += npadding_bytes(len(pkt), int(samples_per_symbol), bits_per_symbol) * b"\x55"
    return pkt


def unmake_packet(whitened_payload_with_crc, whitener_offset=0, dewhitening=True):      # :175-194
    s = whiten(whitened_payload_with_crc, whitener_offset) if dewhitening else bytes(whitened_payload_with_crc)
    if len(s) < 4:                                                          # crc.py:31-32
        return False, b""
    msg = s[:-4]
    (expected,) = struct.unpack(">I", s[-4:])
    return crc32(msg) == expected, msg


# ---- the stream of the RF loop tests ---------------------------------------------------------------------------------
RF_PAYLOAD_LENGTHS = (100, 0, 257)
RF_OFFSETS = (0, 5, 15)


def rf_loop_stream():
    """(stream, payloads, packets): the first 128 bytes of modulator_ref.loop_bytes() for the receive loops to settle on,
    three packets without the 0x55 padding (the loops were never tested on such runs) and 32 more random bytes"""
    import modulator_ref as MR
    rng = np.random.RandomState(2011)
    payloads = [rng.randint(0, 256, n).astype(np.uint8).tobytes() for n in RF_PAYLOAD_LENGTHS]
    packets = [make_packet(p, MR.LOOP_SPS, 2, pad_for_usrp=False, whitener_offset=o) for p, o in zip(payloads, RF_OFFSETS)]
    tail = rng.randint(0, 256, 32).astype(np.uint8).tobytes()
    stream = MR.loop_bytes()[:128].tobytes() + b"".join(packets) + tail
    return np.frombuffer(stream, np.uint8).copy(), payloads, packets
