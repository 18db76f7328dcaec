"""numpy restatement of gr_ctcss_squelch_ff (general/gr_ctcss_squelch_ff.{h,cc}, filter/gri_goertzel.cc:36-75): guard
selection, three float32 Goertzel recurrences with the real part of the output formed in double, the magnitudes, the
decision c < level || c < l || c < r once per block of len samples, held until the next block ends, and the block phase
across calls.  The four-state machine behind the detector is squelch_ref.PwrSquelch's, run on these flags.
test_ctcss_squelch_cpu.py holds it to outputs recorded from the reference's own sources
(tests/golden/ref_ctcss_squelch.npz); the GPU tests hold the kernels to it.

closed_form() is the float64 evaluation of the per-position tables the FAST kernels multiply by, and condition() the
cap under which FAST may be held to GENERIC's flags.  The test signal of the test files is made here too."""
import math

import numpy as np

import analytic_ref as an
import squelch_ref as sq

f32 = np.float32
# gr_ctcss_squelch_ff.cc:29-34
TONES = (67.0, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0,
         127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 162.2, 167.9, 173.8, 179.9, 186.2, 192.8, 203.5, 210.7, 218.1,
         225.7, 233.6, 241.8, 250.3)


def signal(seed, rate, L, bursts=True):
    """n = 80 L + 37 samples: noise of 0.01, plus amp sin(2 pi f t / rate) on [5L + L//3, 20L + L//2) and [25L, 27L) at
    100.0 Hz, amp 0.1; [30L, 40L) at 103.5 Hz, amp 0.1; [45L, 55L) at 100.0 Hz, amp 0.012; [60L, 70L) at 100.0 Hz,
    amp 0.1, with [64L, 66L) at 97.4 Hz, amp 0.3 on top.  With freq 100.0 and level 0.01 every one of the three
    comparisons trips somewhere."""
    n = 80 * L + 37
    x = 0.01 * np.random.default_rng(seed).standard_normal(n)
    t = np.arange(n)
    spans = ((5 * L + L // 3, 20 * L + L // 2, 100.0, 0.1), (25 * L, 27 * L, 100.0, 0.1), (30 * L, 40 * L, 103.5, 0.1),
             (45 * L, 55 * L, 100.0, 0.012), (60 * L, 70 * L, 100.0, 0.1), (64 * L, 66 * L, 97.4, 0.3))
    for a, b, f, amp in spans if bursts else ():
        x[a:b] += amp * np.sin(2 * np.pi * f * t[a:b] / rate)
    return x.astype(f32)


def default_len(rate):
    return int(rate / 10.0)                                  # gr_ctcss_squelch_ff.cc:60-61


def guards(freq):
    """(f_l, f_c, f_r) as float32: the adjacent standard tones, or 2 % (the product in double, stored to float) for a
    non-standard tone and on the outer side of the first and the last (gr_ctcss_squelch_ff.cc:65-78)"""
    f = f32(freq)
    tones = [f32(t) for t in TONES]
    i = tones.index(f) if f in tones else -1                 # an exact float compare
    f_l = f32(float(f) * 0.98) if i in (-1, 0) else tones[i - 1]
    f_r = f32(float(f) * 1.02) if i in (-1, len(tones) - 1) else tones[i + 1]
    return f_l, f, f_r


def magnitude(z):
    """std::abs of a gr_complex, the host's hypotf on finite values: (float)sqrt((double)re re + (double)im im)"""
    z = np.asarray(z, np.complex64)
    re, im = z.real.astype(np.float64), z.imag.astype(np.float64)
    return np.sqrt(re * re + im * im).astype(f32)


def recurrence(rate, L, freqs, blocks):
    """|output| of the float32 filters (gri_goertzel::input / output) on every row of `blocks`, one column per tone"""
    blocks = np.ascontiguousarray(blocks, f32).reshape(-1, L)
    return np.stack([magnitude(an.goertzel_fc(rate, L, f, blocks.reshape(-1))) for f in freqs], axis=1)


def table(rate, L, freq):
    """the per-position table of one tone in float64: out = sum_n x[n] tab[n] is what the recurrence computes in exact
    arithmetic with the float coefficients (wr, wi): tab[n] = (cos((L - n) w'), wi U_(L-1-n)) / L, w' = acos(wr / 2),
    U_k = sin((k + 1) w') / sin(w')"""
    wr, wi = (float(v) for v in an.goertzel_params(rate, freq))
    wp = math.acos(min(1.0, max(-1.0, 0.5 * wr)))
    n = np.arange(L, dtype=np.float64)
    return (np.cos((L - n) * wp) + 1j * wi * np.sin((L - n) * wp) / math.sin(wp)) / L


def closed_form(rate, L, freqs, blocks):
    """|sum_n x[n] tab[n]| in float64 on every row of `blocks`, one column per tone"""
    blocks = np.asarray(blocks, np.float64).reshape(-1, L)
    return np.stack([np.abs(blocks @ table(rate, L, f)) for f in freqs], axis=1)


def decide(mags, level):
    """d_mute after each block (gr_ctcss_squelch_ff.cc:110), float compares; a NaN level never mutes"""
    m = np.asarray(mags, f32)
    l, c, r = m[:, 0], m[:, 1], m[:, 2]
    return (c < f32(level)) | (c < l) | (c < r)


def _tie(a, b):
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


def condition(rate, L, freq, level, x):
    """(margin, deviation) over the whole blocks of x.  margin: the smallest |a - b| / max(a, b) over the three
    comparisons a < b of every block (float recurrence).  deviation: the largest |recurrence - closed form| / closed
    form over every block and tone.  A comparison a < b whose sides each move by at most d relative changes sides only
    if |a - b| <= d (a + b) <= 2 d max(a, b), so margin >= 10 deviation leaves a factor of 5."""
    fr = guards(freq)
    nb = len(x) // L
    blocks = np.asarray(x[:nb * L], f32).reshape(nb, L)
    rec = recurrence(rate, L, fr, blocks).astype(np.float64)
    cf = closed_form(rate, L, fr, blocks)
    l, c, r = rec[:, 0], rec[:, 1], rec[:, 2]
    lev = np.full(nb, float(f32(level)))
    margin = float(min(_tie(c, lev).min(), _tie(c, l).min(), _tie(c, r).min()))
    deviation = float(np.max(np.abs(rec - cf) / np.maximum(cf, 1e-300)))
    return margin, deviation


class CtcssSquelch(sq.PwrSquelch):
    """gr_ctcss_squelch_ff(rate, freq, level, len, ramp, gate); work(x) may cut the stream anywhere.  A block is
    evaluated when its last sample arrives, which for filters that start every block from zero is what feeding them
    sample by sample gives."""

    def __init__(self, rate, freq, level=0.01, len=0, ramp=0, gate=False):
        sq.PwrSquelch.__init__(self, 0.0, 1.0, ramp, gate, False)
        self.rate = int(rate)
        self.level = f32(level)
        self.len = int(len) if len else default_len(rate)
        self.tones = guards(freq)
        self.mute = True                                     # gr_ctcss_squelch_ff.cc:84
        self.pending = np.zeros(0, f32)                      # the samples the filters hold
        self.mags = []                                       # (|l|, |c|, |r|) of every block so far

    def set_level(self, level):
        self.level = f32(level)

    def flags(self, x):
        """the value of mute() behind every sample of x"""
        x = np.asarray(x, f32)
        p, L = len(self.pending), self.len
        v = np.concatenate([self.pending, x])
        nb = len(v) // L
        dec = np.zeros(nb + 1, bool)
        dec[0] = self.mute
        if nb:
            m = recurrence(self.rate, L, self.tones, v[:nb * L])
            self.mags.extend(m.tolist())
            dec[1:] = decide(m, self.level)
            self.mute = bool(dec[-1])
        self.pending = v[nb * L:]
        return dec[(np.arange(len(x)) + p + 1) // L]

    def work(self, x):
        """squelch_ref.PwrSquelch.work (the machine, the envelope, gating) with these flags as its detector's verdict:
        that work() mutes where detector(...) < thr"""
        x = np.asarray(x, f32)
        mute = self.flags(x)
        saved, self.thr = sq.detector, 0.5
        sq.detector = lambda p, alpha, y: np.where(mute, 0.0, 1.0)
        try:
            return sq.PwrSquelch.work(self, x)
        finally:
            sq.detector = saved
