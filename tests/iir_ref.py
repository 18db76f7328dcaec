"""Restatement of gr_iir_filter_ffd, filter/gri_iir.h:126-163, in Python floats (IEEE doubles, every product and every
add rounded once, in the reference's order), of the chunked form that iir_filter_ffd runs in every mode but GENERIC
(csrc/iir.hip): every chunk of 256 items walked from zero accumulators, the chunks chained through C^256 in double,
then walked again from their true starts; and of the tap formulas of blks2.fm_deemph (blks2impl/fm_emph.py:55-63).
tests/golden/ref_iir.npz pins serial() to the reference's own code bit for bit (test_iir_cpu.py states how it was
recorded)."""
import hashlib
import math

import numpy as np

N = 6037
CHUNK = 256
MAX_K = 8
MAX_GROWTH = 64.0
CUTS = (1, 255, 256, 257, 4097)


def deemph_taps(fs, tau=75e-6):
    """(btaps, ataps) as fm_emph.py:55-63 writes them"""
    w_p = 1 / tau
    w_pp = math.tan(w_p / (fs * 2))
    a1 = (w_pp - 1) / (w_pp + 1)
    b0 = w_pp / (1 + w_pp)
    b1 = b0
    return [b0, b1], [1, a1]


# (fftaps, fbtaps); the feedback is ADDED, so a pole pair r e^{+-j theta} is fb = [*, 2 r cos theta, -r^2]
TAP_SETS = {
    "deemph32k": deemph_taps(32e3),
    "deemph320k": deemph_taps(320e3),
    # poles 0.71 e^{+-j pi/4}
    "biquad": ([0.2, 0.4, 0.2], [0.0, 1.0040916292848976, -0.5041]),
    # poles 0.9 e^{+-0.3 pi j} and 0.8 e^{+-0.6 pi j}
    "order4": ([0.05, 0.1, 0.15, 0.1, 0.05],
               [-1.0, 0.5635862631265358, -0.9268893798361404, 0.27664258593099733, -0.5184000000000002]),
    "n1m3": ([0.5], [0.0, 0.3, -0.4]),
    "n5m2": ([0.1, 0.2, 0.4, 0.2, 0.1], [0.0, 0.5]),
}
STABLE = tuple(TAP_SETS)
# qa_iir.py test 005: roots 1.30 and -2.30, run over 64 samples only
UNSTABLE = ([2.0, 11.0, 0.0], [0.0, -1.0, 3.0])
UNSTABLE_N = 64
# feedback order 9: stable (the taps' magnitudes sum to 0.45), above the chunked form's K <= 8
K9 = ([1.0, 0.5], [0.0] + [0.05] * 9)
# the latched set_taps: LATCH[0] up to sample 4097, then LATCH[1] from zeroed delay lines
LATCH = ("biquad", "deemph32k")
LATCH_AT = 4097


def signal(seed=1):
    """noise through four levels: 1, silence, 30 and 0.02"""
    rng = np.random.default_rng(seed)
    env = np.empty(N)
    env[:1500] = 1.0
    env[1500:2500] = 0.0
    env[2500:4000] = 30.0
    env[4000:] = 0.02
    return (rng.standard_normal(N) * 0.7 * env).astype(np.float32)


class State(object):
    """xs[k] / ys[k]: the input / the accumulator k + 1 items back; ys in double"""

    def __init__(self, n, m):
        self.xs = [0.0] * max(n - 1, 0)
        self.ys = [0.0] * max(m - 1, 0)

    def copy(self):
        s = State(0, 0)
        s.xs, s.ys = list(self.xs), list(self.ys)
        return s


def serial(x, ff, fb, state=None):
    """filter_n over x from `state` (zero if None).  Returns (out float32, acc float64, state after)."""
    ff = [float(t) for t in ff]
    fb = [float(t) for t in fb]
    n, m = len(ff), len(fb)
    x = np.asarray(x, np.float32)
    out = np.zeros(len(x), np.float32)
    accs = np.zeros(len(x), np.float64)
    st = State(n, m) if state is None else state.copy()
    if n == 0:                                          # gri_iir.h:135-136
        return out, accs, st
    assert m >= 1, "the reference writes past an empty vector"
    xs, ys = st.xs, st.ys
    with np.errstate(all="ignore"):
        for t, xv in enumerate(x.tolist()):             # a float32 as a Python float: the promotion to double
            acc = ff[0] * xv
            for i in range(1, n):
                acc = acc + ff[i] * xs[i - 1]
            for i in range(1, m):
                acc = acc + fb[i] * ys[i - 1]
            if n > 1:
                xs.insert(0, xv)
                xs.pop()
            if m > 1:
                ys.insert(0, acc)
                ys.pop()
            accs[t] = acc
        out[:] = accs.astype(np.float32)
    return out, accs, st


def in_calls(fn, x, ff, fb, cuts=(), state=None):
    """fn (serial or chunked_call) over x cut into calls at `cuts`, the state carried"""
    edges = [0] + [c for c in cuts if 0 < c < len(x)] + [len(x)]
    outs, st = [], state
    for a, b in zip(edges[:-1], edges[1:]):
        o, _, st = fn(x[a:b], ff, fb, st)
        outs.append(o)
    return np.concatenate(outs), st


def companion_powers(fb):
    """C^1 .. C^CHUNK of the K x K companion matrix of fb, built as the library builds them (C times the last)"""
    K = len(fb) - 1
    C = np.zeros((K, K))
    if K:
        C[0, :] = [float(t) for t in fb[1:]]
        for r in range(1, K):
            C[r, r - 1] = 1.0
    P, out = np.eye(K), []
    for _ in range(CHUNK):
        P = C @ P
        out.append(P)
    return out


def can_chunk(ff, fb, n_items=N):
    if len(ff) == 0 or len(fb) == 0 or len(fb) - 1 > MAX_K or n_items <= CHUNK:
        return False
    if not (np.all(np.isfinite(ff)) and np.all(np.isfinite(fb))):
        return False
    with np.errstate(all="ignore"):
        return all(np.abs(P).sum(axis=1).max(initial=0.0) <= MAX_GROWTH for P in companion_powers(fb))


def chunked_call(x, ff, fb, state=None):
    """one work call of the chunked form"""
    if not can_chunk(ff, fb, len(x)):
        return serial(x, ff, fb, state)
    n, m = len(ff), len(fb)
    K = m - 1
    st = State(n, m) if state is None else state.copy()
    CL = companion_powers(fb)[-1]
    x = np.asarray(x, np.float32)

    def front(c0):
        """the n - 1 inputs in front of item c0"""
        h = [float(v) for v in x[max(c0 - (n - 1), 0):c0][::-1]]
        return h + st.xs[:n - 1 - len(h)]

    starts, s = [], np.array(st.ys, np.float64)
    for c0 in range(0, len(x), CHUNK):
        z = State(n, m)
        z.xs = front(c0)
        _, _, e = serial(x[c0:c0 + CHUNK], ff, fb, z)
        starts.append(s)
        s = CL @ s + np.array(e.ys, np.float64) if K else s
    outs, accs = [], []
    for k, c0 in enumerate(range(0, len(x), CHUNK)):
        z = State(n, m)
        z.xs, z.ys = front(c0), [float(v) for v in starts[k]]
        o, a, end = serial(x[c0:c0 + CHUNK], ff, fb, z)
        outs.append(o)
        accs.append(a)
    return np.concatenate(outs), np.concatenate(accs), end


def chunked(x, ff, fb, cuts=()):
    return in_calls(chunked_call, x, ff, fb, cuts)


def fast_bound(ref_out):
    """the FAST contract of include/grhip.h per output: ulp_float(|y|) + 2^-40 peak"""
    ref = np.asarray(ref_out, np.float32)
    peak = float(np.max(np.abs(ref.astype(np.float64)))) if len(ref) else 0.0
    return np.spacing(np.abs(ref)).astype(np.float64) + 2.0 ** -40 * peak


def within_fast_bound(got, ref_out):
    got = np.asarray(got, np.float32).astype(np.float64)
    return bool(np.all(np.abs(got - np.asarray(ref_out, np.float32).astype(np.float64)) <= fast_bound(ref_out)))


# ---- the FM demodulator hier block (blks2impl/fm_demod.py:51-72, nbfm_rx.py:67-88) ---------------------------------
def fm_signal(seed, n):
    """a frequency-modulated carrier with an amplitude that fades to zero and back, complex64"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    audio = 0.6 * np.sin(2 * np.pi * 0.011 * t + seed) + 0.3 * np.sin(2 * np.pi * 0.037 * t) + 0.05 * rng.standard_normal(n)
    phase = np.cumsum(0.9 * audio)
    amp = 0.5 + 0.5 * np.cos(2 * np.pi * t / 3001.0)
    amp[(t % 4000) > 3990] = 0.0                        # a few exact zeros: atan2(0, 0)
    x = amp * np.exp(1j * phase) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (amp > 0)
    return x.astype(np.complex64)


def fm_outputs(n_in, D):
    """outputs of the first n_in items of a stream: the j with j D < n_in"""
    return (n_in + D - 1) // D


def fm_deemphasised(po, x, k, deemph):
    """the reference's first two blocks over a whole stream: quadrature_demod_cf(k) from x[-1] = 0 through the oracle,
    then the restatement of iir_filter_ffd (deemph = (fftaps, fbtaps), or None).  Returns (q, y), float32 both."""
    x = np.asarray(x, np.complex64)
    q = po.quad_demod_cf(k, np.concatenate([np.zeros(1, np.complex64), x]), len(x))
    if deemph is None:
        return q, q
    return q, serial(q, deemph[0], deemph[1])[0]


def fm_fir(po, y, D, taps, n_in=None):
    """fir_filter_fff(D, taps) from a zero delay line over the first n_in de-emphasised samples, through the oracle"""
    taps = np.asarray(taps, np.float32)
    n_in = len(y) if n_in is None else n_in
    padded = np.concatenate([np.zeros(len(taps) - 1, np.float32), y[:n_in]])
    return po.fir_fff(taps, padded, fm_outputs(n_in, D), D)


def fm_fir64(y, D, taps, n_in=None):
    """the same FIR in float64 over the float32 samples"""
    n_in = len(y) if n_in is None else n_in
    full = np.convolve(np.asarray(y[:n_in], np.float64), np.asarray(taps, np.float64))[:n_in]
    return full[::D]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
