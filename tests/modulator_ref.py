"""Restatement in numpy of the blocks in front of generic_mod's pulse shaper (gr-digital/python/generic_mod_demod.py:114-150):
gr_packed_to_unpacked_bb (gengen/gr_packed_to_unpacked_XX.cc.t:58-137), gr_unpacked_to_packed_bb
(gengen/gr_unpacked_to_packed_XX.cc.t:56-129), gr_diff_encoder_bb (general/gr_diff_encoder_bb.cc:44-62, the serial loop
literally) and gr_chunks_to_symbols_bc (gengen/gr_chunks_to_symbols_XX.cc.t:51-74).  tests/test_modulator_cpu.py holds it
against tests/golden/ref_generic_mod.npz, recorded from the reference's own files; the GPU tests hold the device against
it."""
import numpy as np

MSB_FIRST = 0       # GR_MSB_FIRST, gengen/gr_endianness.h:25
LSB_FIRST = 1

SCAN_TILE = 2048    # DIFF_TILE of csrc/modulator_plan.h
SCAN_LANE = 8       # DIFF_PER_LANE


def _ceil_div(a, b):
    return -(-a // b)


class PackedToUnpacked(object):
    """one stream of gr_packed_to_unpacked_bb; general_work(noutput, bytes) -> (chunks, consumed)"""

    def __init__(self, bits_per_chunk, endianness=MSB_FIRST):
        assert 1 <= bits_per_chunk <= 8
        self.k, self.endianness, self.index = int(bits_per_chunk), endianness, 0

    def forecast(self, noutput):
        return _ceil_div(self.index + noutput * self.k, 8)                  # .cc.t:62

    def general_work(self, noutput, x):
        x = np.asarray(x, np.uint8)
        assert len(x) >= self.forecast(noutput)
        # get_bit_be counts a byte's bits from the top, get_bit_le from the bottom (.cc.t:70-82)
        bits = np.unpackbits(x, bitorder="big" if self.endianness == MSB_FIRST else "little")
        b = bits[self.index:self.index + noutput * self.k].reshape(noutput, self.k).astype(np.uint32)
        out = np.zeros(noutput, np.uint32)
        for j in range(self.k):                                            # x = (x << 1) | bit, for both (:109, :119)
            out = (out << 1) | b[:, j]
        end = self.index + noutput * self.k
        self.index = end & 7                                               # :134
        return out.astype(np.uint8), end >> 3                              # :133


class UnpackedToPacked(object):
    """one stream of gr_unpacked_to_packed_bb; general_work(noutput, chunks) -> (bytes, consumed)"""

    def __init__(self, bits_per_chunk, endianness=MSB_FIRST):
        assert 1 <= bits_per_chunk <= 8
        self.k, self.endianness, self.index = int(bits_per_chunk), endianness, 0

    def forecast(self, noutput):
        return _ceil_div(self.index + noutput * 8, self.k)                 # .cc.t:59

    def general_work(self, noutput, x):
        x = np.asarray(x, np.uint8)
        assert len(x) >= self.forecast(noutput)
        a = self.index + np.arange(noutput * 8)
        c = a // self.k
        bits = ((x[c].astype(np.uint32) >> (self.k - 1 - (a - c * self.k))) & 1).reshape(noutput, 8)    # get_bit_be1, :66-73
        out = np.zeros(noutput, np.uint32)
        for j in range(8):
            if self.endianness == MSB_FIRST:
                out = (out << 1) | bits[:, j]                              # :101
            else:
                out = (out >> 1) | (bits[:, j] << 7)                       # :112
        end = self.index + noutput * 8
        self.index = end % self.k                                          # :126
        return out.astype(np.uint8), end // self.k                         # :125


def run_in_calls(block, x, per_call):
    """a stream through a repacking block in calls of per_call outputs (None: one call), fed as a scheduler would: what
    forecast asks for, the unconsumed items first.  Returns the outputs; leftover bits that fill no output stay."""
    x = np.asarray(x, np.uint8)
    out, pos = [], 0
    while True:
        n = per_call
        if n is None:
            n = (len(x) * 8 - block.index) // block.k if isinstance(block, PackedToUnpacked) else \
                (len(x) * block.k - block.index) // 8
        while n > 0 and block.forecast(n) > len(x) - pos:
            n -= 1
        if n <= 0:
            break
        y, consumed = block.general_work(n, x[pos:pos + block.forecast(n)])
        out.append(y)
        pos += consumed
        if per_call is None:
            break
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def diff_encoder_serial(x, modulus, last_out=0):
    """gr_diff_encoder_bb.cc:52-60 literally; returns (out, last_out)"""
    x = np.asarray(x, np.uint8)
    out = np.zeros(len(x), np.uint8)
    last = int(last_out)
    for i in range(len(x)):
        out[i] = ((int(x[i]) + last) % modulus) & 0xff                     # the store into an unsigned char
        last = int(out[i])
    return out, last


def diff_scan_modulus(modulus):
    """the modulus of the scan form, or 0 where only the serial walk is right (csrc/modulator_plan.h)"""
    if modulus <= 256:
        return modulus
    return 256 if modulus > 510 else 0


def diff_encoder_scan(x, modulus, last_out=0, tile=SCAN_TILE, lane=SCAN_LANE):
    """the encoder the way the kernels run it, with scan modulus m (given as it is, so that a test can show where the
    form fails): the sum of every tile mod m, the tiles' carries from last_out, then inside a tile the sum of every
    lane's `lane` items, the lanes' exclusive scan, and each lane's walk from there"""
    x = np.asarray(x, np.uint8)
    m = int(modulus)
    n = len(x)
    tiles = _ceil_div(n, tile)
    pad = np.zeros(tiles * tile, np.int64)
    pad[:n] = x
    pad = pad.reshape(tiles, tile)
    sums = pad.sum(axis=1) % m                                             # pass 1
    carry = np.zeros(tiles, np.int64)                                      # pass 2
    run = int(last_out) % m
    for t in range(tiles):
        carry[t] = run
        run = (run + int(sums[t])) % m
    lanes = pad.reshape(tiles, tile // lane, lane)                         # pass 3
    ls = lanes.sum(axis=2) % m
    incl = np.cumsum(ls, axis=1) % m
    start = (carry[:, None] + incl + m - ls) % m
    out = np.zeros_like(lanes)
    v = start
    for j in range(lane):
        v = (v + lanes[:, :, j]) % m
        out[:, :, j] = v
    return (out.reshape(-1)[:n] & 0xff).astype(np.uint8), run


def map_bb(x, code):
    """gr_map_bb.cc:36-60: the identity behind the entries given"""
    t = np.arange(256, dtype=np.uint8)
    code = np.asarray(code, np.int64)[:256]
    t[:len(code)] = code.astype(np.uint8)
    return t[np.asarray(x, np.uint8)]


# ---- generic_mod (gr-digital/python/generic_mod_demod.py:76-157) ----------------------------------------------------------
MOD_NFILTS = 32                                                            # :132


def mod_taps(samples_per_symbol, excess_bw):
    """:132-139: root_raised_cosine(nfilts, nfilts, 1.0, excess_bw, nfilts * 11 * int(sps))"""
    import fll_ref as FR
    return FR.root_raised_cosine(float(MOD_NFILTS), float(MOD_NFILTS), 1.0, excess_bw, 11 * int(samples_per_symbol) * MOD_NFILTS)


def generic_mod_symbols(c, data, differential=True, gray_coded=True):
    """the symbol indices in front of chunks_to_symbols: packed_to_unpacked_bb(k, MSB_FIRST) -> map_bb(pre_diff_code) if
    gray_coded (the modulator does not ask apply_pre_diff_code(): an empty code is the identity, and constellation_qpsk's
    is applied although the demodulator skips it) -> diff_encoder_bb(arity) if differential.  `c` has points,
    pre_diff_code and bits_per_symbol() (constellation_ref.Constellation or the library's)."""
    k = c.bits_per_symbol()
    s = run_in_calls(PackedToUnpacked(k, MSB_FIRST), data, None)
    if gray_coded:
        s = map_bb(s, list(c.pre_diff_code() if callable(c.pre_diff_code) else c.pre_diff_code))
    if differential:
        s, _ = diff_encoder_serial(s, 2 ** k)
    return s


def generic_mod(c, data, samples_per_symbol=2, differential=True, excess_bw=0.35, gray_coded=True, f64=False):
    """the hier block's output for the whole of `data`: every output of pfb_arb_resampler_ccf whose count lies below the
    number of symbols, the scheduler's history zeros in front (f64: the same schedule, taps and symbols evaluated in
    float64)"""
    import arb_resampler_ref as AR
    pts = np.asarray(c.points() if callable(c.points) else c.points, np.complex64)
    sym = chunks_to_symbols(generic_mod_symbols(c, data, differential, gray_coded), pts)
    tpf, fwd, dfwd = AR.banks(mod_taps(samples_per_symbol, excess_bw), MOD_NFILTS)
    cs, js, accs = AR.walk_schedule(MOD_NFILTS, samples_per_symbol, n_samples=len(sym))
    buf = np.concatenate([np.zeros(tpf, np.complex64), sym])
    return AR.eval_schedule(fwd, dfwd, buf, cs, js, accs, f64=f64)


# ---- the loop-back through the receive chain of tests/demod_chain_ref.py -----------------------------------------------------
# dqpsk at 2 samples per symbol: LOOP_BYTES seeded bytes are 4096 symbols and 8192 samples, as the receive chain's own
# test signal.  Behind LOOP_PREFIX output symbols the chain gives symbol m - LOOP_LAG of the modulator's input without
# a bit error, clean and with noise of 0.01 and 0.02 per component, and at no other lag in LOOP_LAGS fewer than a
# quarter of the bits are wrong.  The lag is the modulator's 11 symbols of pulse, the FLL's 2 * 55 - 1 samples and the
# matched filter's delay; it was found once by tests/test_modulator_cpu.py's search and is pinned here.
LOOP_BYTES = 1024
LOOP_SEED = 7
LOOP_SPS = 2
LOOP_PREFIX = 300
LOOP_LAG = 73
LOOP_LAGS = range(55, 80)
LOOP_NOISE = (0.0, 0.01, 0.02)


def loop_bytes():
    return np.random.RandomState(LOOP_SEED).randint(0, 256, LOOP_BYTES).astype(np.uint8)


def loop_bit_errors(got_bits, sent_bytes, lag, prefix=LOOP_PREFIX):
    """(bit errors, bits compared) of the receiver's output (one bit per byte, 2 per symbol) behind `prefix` symbols
    against the sent bytes' symbols at `lag`"""
    got = np.asarray(got_bits, np.uint8).reshape(-1, 2)
    sent = np.unpackbits(np.asarray(sent_bytes, np.uint8)).reshape(-1, 2)
    m = np.arange(prefix, len(got))
    m = m[(m - lag >= 0) & (m - lag < len(sent))]
    return int(np.count_nonzero(got[m] != sent[m - lag])), 2 * len(m)


def chunks_to_symbols(x, table, D=1):
    """gr_chunks_to_symbols_bc: table[in * D : in * D + D] per input byte; zeros where that leaves the table (the
    library's stated deviation: the reference asserts)"""
    x = np.asarray(x, np.uint8).astype(np.int64)
    table = np.asarray(table, np.complex64)
    idx = x[:, None] * D + np.arange(D)[None, :]
    ok = (x * D + D <= len(table))[:, None] & np.ones((1, D), bool)
    out = np.zeros(idx.shape, np.complex64)
    out[ok] = table[idx[ok]]
    return out.reshape(-1)
