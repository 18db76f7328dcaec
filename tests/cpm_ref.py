"""Test-only Python restatement of the continuous-phase transmitter: gr_frequency_modulator_fc
(general/gr_frequency_modulator_fc.cc:49-72), gr_bytes_to_syms, gr_char_to_float, gr_chunks_to_symbols_bf,
gr_interp_fir_filter_fff on gr_fir_fff_generic, and the chains of digital_cpmmod_bc and gmsk_mod (gmsk.py:84-120).

tests/golden/ref_cpm.npz was recorded on the CPU from the reference's own files compiled unchanged against stub
headers: gr_frequency_modulator_fc.cc, gr_cpm.cc, gr_firdes.cc (gaussian), gr_bytes_to_syms.cc, gr_char_to_float.cc with
gri_char_to_float.cc, gr_chunks_to_symbols_XX.cc.t expanded for bf, gr_interp_fir_filter_XXX.cc.t expanded for fff on
gr_fir_XXX_generic.cc.t, gr_sincos.c (sincosf).  Boost is not installed: the stubs map boost::math::erf and
boost::math::trunc onto std::erf and std::trunc, and boost::shared_ptr onto std::shared_ptr.  The taps of gmsk_mod are
numpy.convolve of the recorded gaussian taps with sps ones, as gmsk.py:99-107 forms them.  Long outputs are kept as
length, first and last 512 samples and SHA-256 (as ref_generic_mod.npz); every end-of-call phase is kept.  The hier
cases are cut in input items: one call, a cut at 97 symbols (37 bytes for gmsk_mod) since the modulator's 4097 lies
past their 600 symbols, and calls of 7."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cpm.npz")
QA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_qa_cpm.json")
CUTS = ("one", "cut", "seven")
KEEP = 512
LRC, LSRC, LREC, TFM, GAUSSIAN = range(5)
TYPE_NAMES = ("LRC", "LSRC", "LREC", "TFM", "GAUSSIAN")

_FX = None


def fixture():
    global _FX
    if _FX is None:
        with np.load(GOLDEN) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def chunks_of(n, cut, at):
    """the work calls of n items: one call, a cut at `at` (one call where it lies past the end), calls of 7"""
    if cut == "one" or (cut == "cut" and at >= n):
        return [n]
    if cut == "cut":
        return [at, n - at]
    return [7] * (n // 7) + ([n % 7] if n % 7 else [])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ulps(a, b):
    """per float component: how many floats apart (NaN against NaN is 0, NaN against a number is huge)"""
    a = np.ascontiguousarray(a).view(np.float32).astype(np.float32)
    b = np.ascontiguousarray(b).view(np.float32).astype(np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)

    def order(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(order(a) - order(b))
    return np.where(both_nan, 0, np.where(one_nan, 1 << 40, d))


def same_phases(a, b):
    """bit for bit; a non-finite state only has to be non-finite in both (the sign and payload of a NaN are the platform's)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a)
    return a.shape == b.shape and np.array_equal(fin, np.isfinite(b)) and np.array_equal(a[fin].view(np.uint64), b[fin].view(np.uint64))


def within_one_ulp(out, key):
    assert len(out) == int(fixture()[key + "_len"])
    return max(int(ulps(out[:KEEP], fixture()[key + "_head"]).max()), int(ulps(out[-KEEP:], fixture()[key + "_tail"]).max())) <= 1


# ---- gr_frequency_modulator_fc ---------------------------------------------------------------------------------------
def wrap(ph):
    """.cc:66-69 on a float64 scalar"""
    with np.errstate(all="ignore"):
        if np.abs(ph) > 16 * np.pi:
            ii = np.trunc(ph / (2 * np.pi))
            ph = ph - (ii * 2 * np.pi)
    return np.float64(ph)


def call_phases(x, sens, phase):
    """the float64 phases behind every item of one work call: phase += sens * in[i] in the reference's order
    (numpy's cumsum adds one element at a time)"""
    with np.errstate(all="ignore"):
        prod = np.float64(sens) * np.asarray(x, np.float32).astype(np.float64)
        return np.cumsum(np.concatenate(([np.float64(phase)], prod)))[1:]


def rounded_sincos(p64):
    """(cos, sin) of (float)phase, each the float-rounded double function"""
    with np.errstate(all="ignore"):
        pf = p64.astype(np.float32).astype(np.float64)
        out = np.empty(len(p64), np.complex64)
        out.real = np.cos(pf).astype(np.float32)
        out.imag = np.sin(pf).astype(np.float32)
    return out


def freq_mod(x, sens, chunks=None, phase=0.0):
    """GENERIC: (outputs, end-of-call phases) of the work calls `chunks` over x"""
    x = np.asarray(x, np.float32)
    chunks = [len(x)] if chunks is None else chunks
    out, phases, at, ph = [], [], 0, np.float64(phase)
    for m in chunks:
        p = call_phases(x[at:at + m], sens, ph)
        out.append(rounded_sincos(p))
        ph = wrap(p[-1]) if m else ph
        phases.append(ph)
        at += m
    return np.concatenate(out) if out else np.zeros(0, np.complex64), np.array(phases, np.float64)


def fast_reference(x, sens, phase):
    """one work call in float64: (exp(j phi64), the bound 1e-5 + 2^-50 Phi, Phi).  Phi = sum |sens x| + |phase|; behind
    a non-finite product every output is NaN and nothing is bounded, so Phi stops in front of the first one."""
    with np.errstate(all="ignore"):
        p = call_phases(x, sens, phase)
        prod = np.abs(np.float64(sens) * np.asarray(x, np.float32).astype(np.float64))
        bad = np.flatnonzero(~np.isfinite(prod))
        Phi = np.sum(prod[:bad[0]] if len(bad) else prod) + abs(np.float64(phase))
        return np.cos(p) + 1j * np.sin(p), 1e-5 + 2.0 ** -50 * Phi, Phi


# ---- the small blocks ------------------------------------------------------------------------------------------------
def bytes_to_syms(b):
    bits = np.unpackbits(np.asarray(b, np.uint8))                    # MSB first
    return (bits.astype(np.int32) * 2 - 1).astype(np.float32)


def char_to_float(b):
    return np.asarray(b, np.uint8).view(np.int8).astype(np.float32)


def chunks_to_symbols_bf(b, table, D=1):
    table = np.asarray(table, np.float32)
    b = np.asarray(b, np.uint8).astype(np.int64)
    out = np.zeros((len(b), D), np.float32)
    ok = b * D + D <= len(table)
    out[ok] = table[(b[ok] * D)[:, None] + np.arange(D)[None, :]]
    return out.reshape(-1)


# ---- gr_interp_fir_filter_fff on gr_fir_fff_generic ------------------------------------------------------------------
def taps_per_filter(ntaps, sps):
    return (ntaps + sps - 1) // sps


def interp_fir(sym, taps, sps):
    """sym: float32 with the nt - 1 history items in front; out[i * sps + f] = filter f at &sym[i].  Four float
    accumulators over the reversed taps, the rest into the first, ((a0 + a1) + a2) + a3, nothing fused."""
    taps = np.asarray(taps, np.float32)
    nt = taps_per_filter(len(taps), sps)
    padded = np.concatenate((np.zeros(nt * sps - len(taps), np.float32), taps))
    sym = np.asarray(sym, np.float32)
    n = len(sym) - (nt - 1)
    out = np.zeros((n, sps), np.float32)
    for f in range(sps):
        rev = padded[f::sps][::-1]
        acc = [np.zeros(n, np.float32) for _ in range(4)]
        whole = nt // 4 * 4
        for k in range(nt):
            a = k % 4 if k < whole else 0
            acc[a] = acc[a] + rev[k] * sym[k:k + n]
        out[:, f] = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    return out.reshape(-1)


class Chain(object):
    """char_to_float (or bytes_to_syms) -> interp_fir_filter_fff(sps, taps) -> frequency_modulator_fc(sens), one work
    call of every block per work call"""

    def __init__(self, taps, sps, sens, bits=False):
        self.taps, self.sps, self.sens, self.bits = np.asarray(taps, np.float32), int(sps), np.float64(sens), bits
        self.hist = np.zeros(taps_per_filter(len(self.taps), self.sps) - 1, np.float32)
        self.phase = np.float64(0.0)

    def work(self, items):
        sym = np.concatenate((self.hist, bytes_to_syms(items) if self.bits else char_to_float(items)))
        freq = interp_fir(sym, self.taps, self.sps)
        if len(self.hist):
            self.hist = sym[-len(self.hist):]
        out, ph = freq_mod(freq, self.sens, None, self.phase)
        self.phase = ph[-1]
        return out, freq

    def run(self, items, chunks):
        outs, freqs, phases, at = [], [], [], 0
        for m in chunks:
            o, f = self.work(items[at:at + m])
            outs.append(o); freqs.append(f); phases.append(self.phase)
            at += m
        return np.concatenate(outs), np.concatenate(freqs), np.array(phases, np.float64)


def cpm_sensitivity(h):
    return np.pi * np.float64(np.float32(h))                        # M_PI * h, h a float


def gmsk_sensitivity(sps):
    return (np.pi / 2) / sps


# ---- the loops of tests/test_gpu_cpm_loopback.py ---------------------------------------------------------------------------
LOOP_SPS, LOOP_BT, LOOP_BYTES = 4, 0.35, 512
LOOP_GAIN_MU, LOOP_MU, LOOP_OMEGA_LIMIT = 0.175, 0.5, 0.005          # gmsk.py:41-44, :219-220
LOOP_MAX_LAG = 16
FSK4_SPS, FSK4_H, FSK4_SYMBOLS = 10, 0.5, 1000


def loop_bytes():
    return np.random.RandomState(4).randint(0, 256, LOOP_BYTES).astype(np.uint8)


def loop_mm_params():
    """digital.clock_recovery_mm_ff's arguments in gmsk_demod (gmsk.py:218-233) at LOOP_SPS"""
    return (float(LOOP_SPS), .25 * LOOP_GAIN_MU * LOOP_GAIN_MU, LOOP_MU, LOOP_GAIN_MU, LOOP_OMEGA_LIMIT)


def loop_demod_gain():
    return 1.0 / ((np.pi / 2) / LOOP_SPS)                             # gmsk.py:226-227


def lags_without_error(bits, sent_bits, settle):
    """the lags 0 .. LOOP_MAX_LAG at which every received bit behind the first `settle` is the sent one"""
    good = []
    for lag in range(LOOP_MAX_LAG + 1):
        m = min(len(bits), len(sent_bits) + lag)
        if m > settle and np.array_equal(bits[settle:m], sent_bits[settle - lag:m - lag]):
            good.append(lag)
    return good


def fsk4_symbols():
    return (2 * np.random.RandomState(5).randint(0, 4, FSK4_SYMBOLS) - 3).astype(np.int8)


def fsk4_levels(soft):
    """the nearest of -3, -1, 1, 3"""
    return (2 * np.clip(np.rint((np.asarray(soft, np.float64) + 3) / 2), 0, 3) - 3).astype(np.int8)


LOOP_SETTLE = 300       # symbols; the allowance of tests/test_gpu_mod_demod_loopback.py, which the restated loop passes with
LOOP_LAG = 1            # found by the restated loop (tests/test_cpm_cpu.py), the only lag without an error
