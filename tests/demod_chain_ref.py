"""The receive chain of gr-digital/python/generic_mod_demod.py:268-313 with its own parameters, for DQPSK at 2 samples per
symbol: agc2_cc(0.6e-1, 1e-3, 1, 1, 100) -> fll_band_edge_cc(2, 0.35, 55, 2 pi / 100) -> pfb_clock_sync_ccf(2, 2 pi / 100,
root_raised_cosine(32, 64, 1.0, 0.35, 704), 32, 16, 1.5) -> constellation_receiver_cb(dqpsk, 2 pi / 100, -0.25, 0.25) ->
diff_decoder_bb(4) -> map_bb(invert_code(pre_diff_code)) -> unpack_k_bits_bb(2); the transmit side restated from
generic_mod (map_bb(pre_diff_code) -> diff_encoder_bb(4) -> chunks_to_symbols -> root raised cosine); and the same chain
on the restatements of the four blocks (agc_ref, fll_ref, pfb_clock_sync_ref, constellation_ref), run on the CPU.

The signal: NSYM known symbols, shaped at 16 samples per symbol and read at 2 (1 + CLOCK) samples per symbol by linear
interpolation, spun by FREQ rad/sample, scaled by 0.4, with noise of NOISE per component.  NOISE, CLOCK, FREQ, PREFIX and
LAG are chosen so that the restatements decode everything behind PREFIX symbols without an error at this noise and at
twice this noise (tests/test_demod_chain_cpu.py asserts both)."""
import math

import numpy as np

import agc_ref as AR
import carrier_ref as CR
import constellation_ref as KR
import fll_ref as FR
import pfb_clock_sync_ref as PR

NSYM = 4096
SPS = 2
NOISE = 0.01
CLOCK = 5e-4            # of the symbol rate
FREQ = 0.004            # rad/sample
PREFIX = 1024           # symbols of the output that the loops may take to settle
LAG = 66                # output symbol m is transmitted symbol m - LAG: the FLL's 2 * 55 - 1 items and the two pulse filters
AGC = (0.6e-1, 1e-3, 1.0, 1.0, 100.0)
FLL = (2.0, 0.35, 55, 2 * math.pi / 100)
PCS_TAPS = (32.0, 64.0, 1.0, 0.35, 704)
RX = (2 * math.pi / 100, -0.25, 0.25)


def transmit(seed=7, noise=NOISE):
    """(x, values): the samples and the 2-bit values behind them"""
    rng = np.random.RandomState(seed)
    c = KR.Constellation("dqpsk")
    v = rng.randint(0, 4, NSYM)
    u = np.asarray(c.pre_diff_code, np.int64)[v]                    # map_bb(pre_diff_code)
    s = np.cumsum(u) % 4                                            # diff_encoder_bb(4)
    pts = np.asarray(c.points, np.complex128)[s]                    # chunks_to_symbols
    L = 16
    t = FR.root_raised_cosine(1.0, L * 1.0, 1.0, 0.35, 11 * L).astype(np.float64)
    up = np.zeros(NSYM * L, complex)
    up[::L] = pts
    y = np.convolve(up, t)
    step = L / SPS * (1 + CLOCK)
    n = int((len(y) - 2 - 4) / step)
    idx = np.arange(n) * step + 2.7
    i0 = idx.astype(int)
    fr = idx - i0
    x = y[i0] * (1 - fr) + y[i0 + 1] * fr
    x = x / np.sqrt((np.abs(x) ** 2).mean()) * 0.4
    x = x * np.exp(1j * FREQ * np.arange(n))
    x = x + (rng.randn(n) + 1j * rng.randn(n)) * noise
    return x.astype(np.complex64), v


def bits_of(values):
    return KR.unpack_k_bits(np.asarray(values, np.uint8), 2)


def restated_chain(x, fll_taps):
    """the bits that the four restatements give for x"""
    a = AR.serial("agc2_cc", x, AGC).out
    f = FR.Fll(FLL[0], FLL[1], FLL[2], FLL[3], fll_taps).work(a).out
    p = PR.Pcs(float(SPS), 2 * math.pi / 100, FR.root_raised_cosine(*PCS_TAPS), 32, 16.0, 1.5, 1)
    sym = p.work(f).out
    assert p.slips == 0
    c = KR.Constellation("dqpsk")
    r = KR.receiver(CR.Loop(RX[0], RX[2], RX[1]), c, sym)
    return KR.demod_tail(c, r.sym, True, True)


def errors_behind_prefix(bits, values, lag):
    """bit errors of output symbols PREFIX .. against the transmitted values at the given lag, and the symbols compared"""
    got = np.asarray(bits, np.uint8).reshape(-1, 2)
    m = np.arange(PREFIX, len(got))
    m = m[(m - lag >= 0) & (m - lag < len(values))]
    want = bits_of(values[m - lag]).reshape(-1, 2)
    return int(np.count_nonzero(got[m] != want)), len(m)
