"""Restatement of gr-digital/lib/digital_fll_band_edge_cc.cc (:34-40 sinc, :148-188 design_filter, :208-259 work) and of
gr_firdes::root_raised_cosine (general/gr_firdes.cc:601-650) in float32 scalars and arrays with every operation rounded
once and double where the reference's expression is double; the same recurrence in float64 (the yardstick of the
deviation contracts); and the test signals.

The contract restated (include/grhip.h): with fs = filter_size and xz = fs zeros followed by the stream, step j forms
d[j] = xz[j] * expj(phase), filters d[j-fs+1 .. j] (tap k on d[j-fs+1+k], zeros before the start), takes error =
norm(lower) - norm(upper) and steps the loop; output n is d[n-(fs-1)].  An Fll object takes the stream in pieces and
keeps the last fs inputs and the last fs - 1 derotated samples, as the device handle does.

Sine and cosine of the NCO are the float-rounded float64 ones, which is what the device's GRHIP_MODE_GENERIC computes and
not the reference's sincosf to the bit; numpy's sine in the designer is not glibc's sincosf either, so the restated taps
are within one float ulp of the reference's and the loops here run on the taps they are given.  phase_wrap is the
device's: the reference's subtract loop for at most WRAP_TRIPS trips each way, beyond that the exact double remainder
(a stated deviation of the library: the error is unbounded here and the reference's loop then never ends)."""
import math
import random

import numpy as np

import carrier_ref as CR

f32 = np.float32
TWOPI = 2.0 * math.pi           # this block's M_TWOPI is (2*M_PI); gri_control_loop's (2.0f*M_PI) is the same double
WRAP_TRIPS = 256                # FLL_WRAP_TRIPS of csrc/fll_band_edge.h
MAX_TAPS = 1024
WIN = 1024                      # FLL_WIN
N = 6037
CUT = 4097
SEEDS = (1, 2, 3)
SECTIONS, SEC_LEN = (0, 1400, 2900, 3960), 256
gains = CR.gains
bits = CR.bits
digest = CR.digest


# ---- the designers ----------------------------------------------------------------------------------------------
def root_raised_cosine(gain, sampling_freq, symbol_rate, alpha, ntaps):
    """gr_firdes.cc:601-650 in Python floats (doubles), every tap narrowed to float32 where the reference stores it"""
    ntaps |= 1
    spb = sampling_freq / symbol_rate
    taps = np.zeros(ntaps, np.float32)
    scale = 0.0
    for i in range(ntaps):
        xindx = float(i - ntaps // 2)
        x1 = math.pi * xindx / spb
        x2 = 4 * alpha * xindx / spb
        x3 = x2 * x2 - 1
        if abs(x3) >= 0.000001:
            if i != ntaps // 2:
                num = math.cos((1 + alpha) * x1) + math.sin((1 - alpha) * x1) / (4 * alpha * xindx / spb)
            else:
                num = math.cos((1 + alpha) * x1) + (1 - alpha) * math.pi / (4 * alpha)
            den = x3 * math.pi
        else:
            if alpha == 1:
                taps[i] = -1
                continue
            x3 = (1 - alpha) * x1
            x2 = (1 + alpha) * x1
            num = (math.sin(x2) * (1 + alpha) * math.pi - math.cos(x3) * ((1 - alpha) * math.pi * spb) / (4 * alpha * xindx)
                   + math.sin(x3) * spb * spb / (4 * alpha * xindx * xindx))
            den = -32 * math.pi * alpha * alpha * xindx / spb
        taps[i] = 4 * alpha * num / den
        scale += float(taps[i])
    return (taps.astype(np.float64) * gain / scale).astype(np.float32)


def _sinc(x):
    x = f32(x)
    if x == 0:
        return f32(1)
    return f32(math.sin(math.pi * float(x)) / (math.pi * float(x)))


def max_freq_of(sps):
    return f32(TWOPI * (2.0 / float(f32(sps))))             # :58


def design(sps, rolloff, filter_size):
    """(lower, upper) as complex64, stored reversed (:148-188); sine and cosine of the float argument are numpy's"""
    sps, rolloff = f32(sps), f32(rolloff)
    M = int(np.rint(float(f32(filter_size) / sps)))
    power = f32(0)
    bb = []
    for i in range(filter_size):
        k = f32(-M + i * 2.0 / float(sps))
        tap = _sinc(float(rolloff * k) - 0.5) + _sinc(float(rolloff * k) + 0.5)
        power = power + tap
        bb.append(tap)
    N_ = int((filter_size - 1.0) / 2.0)
    lower, upper = np.zeros(filter_size, np.complex64), np.zeros(filter_size, np.complex64)
    lo, up = lower.view(np.float32), upper.view(np.float32)
    with np.errstate(all="ignore"):
        for i in range(filter_size):
            tap = bb[i] / power
            k = f32((-N_ + i) / (2.0 * float(sps)))
            a1 = f32(-TWOPI * float(f32(1) + rolloff) * float(k))
            a2 = f32(TWOPI * float(f32(1) + rolloff) * float(k))
            j = filter_size - i - 1
            lo[2 * j], lo[2 * j + 1] = tap * np.cos(a1), tap * np.sin(a1)
            up[2 * j], up[2 * j + 1] = tap * np.cos(a2), tap * np.sin(a2)
    return lower, upper


# (sps, rolloff, filter_size) whose taps tests/golden/ref_fll_band_edge.npz holds
TAP_CASES = ((4.0, 0.35, 45), (4.0, 0.35, 55), (2.0, 0.35, 55), (2.5, 0.35, 55), (4.0, 0.0, 55), (4.0, 1.0, 55), (2.0, 0.5, 1),
             (4.0, 0.35, 2), (4.0, 0.35, 63), (4.0, 0.35, 64), (2.0, 0.35, 65), (2.5, 0.5, 129), (4.0, 0.35, 1024), (2.0, 1.0, 1024))
# (gain, sampling_freq, symbol_rate, alpha, ntaps): the QA's shape, generic_demod's (nfilts = 32, sps = 2, 11 * sps * nfilts
# taps, gr-digital/python/generic_mod_demod.py), alpha == 1 and the |x3| < 1e-6 branch (taps 2 and 4 symbols out), an even
# count, one tap
RRC_CASES = ((4.0, 4.0, 1.0, 0.35, 45), (32.0, 64.0, 1.0, 0.35, 704), (1.0, 4.0, 1.0, 1.0, 45), (1.0, 4.0, 1.0, 0.5, 45),
             (2.0, 4.0, 1.0, 0.25, 44), (1.0, 8.0, 2.0, 0.35, 1))


# ---- the loop ---------------------------------------------------------------------------------------------------
def wrap(phase, loop=None):
    """phase_wrap with the device's bounded trip count"""
    t = 0
    while t < WRAP_TRIPS and float(phase) > TWOPI:
        phase = f32(float(phase) - TWOPI)
        t += 1
    u = 0
    while u < WRAP_TRIPS and float(phase) < -TWOPI:
        phase = f32(float(phase) + TWOPI)
        u += 1
    if loop is not None:
        loop.wraps += t + u
    if float(phase) > TWOPI or float(phase) < -TWOPI:
        phase = f32(math.fmod(float(phase), TWOPI)) if math.isfinite(float(phase)) else f32(np.nan)
        if float(phase) > TWOPI:
            phase = f32(float(phase) - TWOPI)
        elif float(phase) < -TWOPI:
            phase = f32(float(phase) + TWOPI)
        if loop is not None:
            loop.remainders += 1
    return phase


class Loop(CR.Loop):
    """gri_control_loop with this block's limits and the bounded phase_wrap"""

    def __init__(self, sps, bandwidth):
        mx = max_freq_of(sps)
        CR.Loop.__init__(self, bandwidth, mx, -mx)
        self.remainders = 0

    def step(self, error):
        with np.errstate(all="ignore"):
            freq = self.freq + self.beta * error
            phase = wrap(self.phase + freq + self.alpha * error, self)
        if freq > self.max_freq:
            freq = self.max_freq
            self.limits += 1
        elif freq < self.min_freq:
            freq = self.min_freq
            self.limits += 1
        self.phase, self.freq = phase, freq


class Run(object):
    """out, frq, phs, err of one or more calls, and d: every derotated sample the calls formed"""


def _join(runs):
    r = Run()
    for k in vars(runs[0]):
        setattr(r, k, np.concatenate([getattr(q, k) for q in runs]))
    return r


class Fll(object):
    """the block on given taps, in float32 as the reference writes it (work) or in float64 throughout (work64)"""

    def __init__(self, sps, rolloff, filter_size, bandwidth, taps):
        self.loop = Loop(sps, bandwidth)
        self.set_taps(taps, True)
        self.phase64, self.freq64 = 0.0, 0.0

    def set_taps(self, taps, zero_hist=False):
        lower, upper = taps
        self.lower, self.upper = np.asarray(lower, np.complex64), np.asarray(upper, np.complex64)
        fs = len(self.lower)
        if zero_hist:
            self.fs = fs
            self.xq = np.zeros(fs, np.complex64)
            self.dq = np.zeros(fs - 1, np.complex64)
            self.dq64 = np.zeros(fs - 1, np.complex128)
        assert fs == self.fs

    def _xz(self, x):
        x = np.asarray(x, np.complex64)
        full = np.concatenate([self.xq, x])
        self.xq = full[len(full) - self.fs:].copy()
        return full[:len(x)], len(x)

    def work(self, x):
        xz, n = self._xz(x)
        fs, loop = self.fs, self.loop
        ur_t, ui_t = np.ascontiguousarray(self.upper.real), np.ascontiguousarray(self.upper.imag)
        lr_t, li_t = np.ascontiguousarray(self.lower.real), np.ascontiguousarray(self.lower.imag)
        dre = np.concatenate([self.dq.real, np.zeros(n, np.float32)]).astype(np.float32)
        dim = np.concatenate([self.dq.imag, np.zeros(n, np.float32)]).astype(np.float32)
        frq, phs, err = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        xr, xi = xz.real, xz.imag
        seq = lambda p: np.cumsum(p, dtype=np.float32)[-1]           # 0 + p[0] + p[1] + ... in order
        with np.errstate(all="ignore"):
            for i in range(n):
                ang = float(loop.phase)
                sn, cs = f32(math.sin(ang)), f32(math.cos(ang))
                dre[i + fs - 1] = xr[i] * cs - xi[i] * sn           # :236
                dim[i + fs - 1] = xr[i] * sn + xi[i] * cs
                c, d = dre[i:i + fs], dim[i:i + fs]
                u_re, u_im = seq(ur_t * c - ui_t * d), seq(ur_t * d + ui_t * c)     # :241-244
                l_re, l_im = seq(lr_t * c - li_t * d), seq(lr_t * d + li_t * c)
                e = (l_re * l_re + l_im * l_im) - (u_re * u_re + u_im * u_im)       # :245
                loop.step(e)
                frq[i], phs[i], err[i] = loop.freq, loop.phase, e
        r = Run()
        dall = np.zeros(len(dre), np.complex64)
        dv = dall.view(np.float32)
        dv[0::2], dv[1::2] = dre, dim
        self.dq = dall[len(dall) - (fs - 1):].copy() if fs > 1 else dall[:0].copy()
        r.out, r.d, r.frq, r.phs, r.err = dall[:n].copy(), dall[fs - 1:].copy(), frq, phs, err
        return r

    def work64(self, x):
        """float64 throughout, on the same input and taps and the same (float) gains and limits; its own state"""
        x = np.asarray(x, np.complex64)
        if not hasattr(self, "xq64"):
            self.xq64 = np.zeros(self.fs, np.complex64)
        full = np.concatenate([self.xq64, x])
        self.xq64 = full[len(full) - self.fs:].copy()
        n, fs, lp = len(x), self.fs, self.loop
        xz = full[:n].astype(np.complex128)
        up, lo = self.upper.astype(np.complex128), self.lower.astype(np.complex128)
        d = np.concatenate([self.dq64, np.zeros(n, np.complex128)])
        al, be, mx, mn = float(lp.alpha), float(lp.beta), float(lp.max_freq), float(lp.min_freq)
        ph, fq = self.phase64, self.freq64
        frq, phs, err = np.zeros(n), np.zeros(n), np.zeros(n)
        for i in range(n):
            d[i + fs - 1] = xz[i] * complex(math.cos(ph), math.sin(ph))
            w = d[i:i + fs]
            ou, ol = np.dot(up, w), np.dot(lo, w)
            e = (ol.real * ol.real + ol.imag * ol.imag) - (ou.real * ou.real + ou.imag * ou.imag)
            fq = fq + be * e
            ph = ph + fq + al * e
            if ph > TWOPI or ph < -TWOPI:
                ph = math.fmod(ph, TWOPI)
            fq = mx if fq > mx else (mn if fq < mn else fq)
            frq[i], phs[i], err[i] = fq, ph, e
        self.phase64, self.freq64 = ph, fq
        self.dq64 = d[len(d) - (fs - 1):].copy() if fs > 1 else d[:0].copy()
        r = Run()
        r.out, r.d, r.frq, r.phs, r.err = d[:n].copy(), d[fs - 1:].copy(), frq, phs, err
        return r

    def in_calls(self, x, cuts=(), fn="work"):
        edges = [0] + [c for c in cuts if 0 < c < len(x)] + [len(x)]
        return _join([getattr(self, fn)(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])


def band_edge_error64(lower, upper, dz):
    """the float64 band-edge powers' difference at every step of dz = fs - 1 samples before the first step, then one
    sample per step: what identity (c) holds the device's err against"""
    lo, up = np.asarray(lower, np.complex64).astype(np.complex128), np.asarray(upper, np.complex64).astype(np.complex128)
    dz = np.asarray(dz).astype(np.complex128)
    # tap k on d[j - fs + 1 + k]: a correlation
    ol, ou = np.correlate(dz, np.conj(lo), "valid"), np.correlate(dz, np.conj(up), "valid")
    return (ol.real ** 2 + ol.imag ** 2) - (ou.real ** 2 + ou.imag ** 2)


def ulp32(v):
    return float(np.spacing(f32(abs(v))))


def bound(dev_ref, max_freq):
    """how far frequency and error may lie from the float64 recurrence: Costas's form (tests/carrier_ref.py)"""
    return 2.0 * dev_ref + 4.0 * ulp32(max_freq)


# The recording's largest deviation from the float64 recurrence (work64 on the recorded taps), frequency and error, per
# signal: measured by test_fll_band_edge_cpu.py, which asserts these figures to one part in 10^3, and stored in DESIGN.md
# 4.24.  (The phase, a pure integrator, lies 8e-6 .. 3e-5 rad from float64 on these signals and 1e-2 on "limit"; it gets
# no bound.)
DEV_REF = {
    "qpsk_s1": (1.8400e-07, 4.4442e-07),
    "limit_s1": (9.1069e-06, 4.4139e-06),
    "qa_s20111": (2.6678e-07, 1.9970e-06),
    "qa_s1": (1.3847e-07, 1.2881e-06),
    "qa_s3": (1.1825e-07, 1.1773e-06),
}


# ---- test signals -----------------------------------------------------------------------------------------------
# name, sps, rolloff, filter_size, bandwidth, amplitude, the carrier's frequency (rad/sample) before and from item 3000,
# noise
SETS = (
    ("qpsk", 4.0, 0.35, 55, 2 * math.pi / 100, 1.0, (0.15, -0.1), 0.05),
    # a loud signal on a wide loop: the error drives frequency_limit and phase_wrap
    ("limit", 4.0, 0.35, 45, 0.3, 2.0, (0.3, -0.4), 0.05),
)


def signal(seed, fset):
    """seeded QPSK symbols through a root-raised-cosine pulse at sps samples per symbol, spun by a carrier whose
    frequency steps at item 3000, with noise"""
    _, sps, rolloff, _, _, amp, fo, noise = fset
    rng = np.random.default_rng(seed)
    isps = int(math.ceil(sps))
    nsym = N // isps + 20
    pts = np.exp(1j * (math.pi / 4 + math.pi / 2 * rng.integers(0, 4, nsym)))
    t = root_raised_cosine(isps, isps, 1.0, rolloff, 11 * isps).astype(np.float64)
    upz = np.zeros(nsym * isps, np.complex128)
    upz[::isps] = pts
    s = np.convolve(upz, t)[:N]
    th = np.cumsum(np.where(np.arange(N) < 3000, fo[0], fo[1]))
    w = noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return (amp * (s * np.exp(1j * th) + w)).astype(np.complex64)


# gr-digital/python/qa_fll_band_edge.py
QA = dict(sps=4, rolloff=0.35, ntaps=45, bw=2 * math.pi / 100.0, nsym=200, spin=0.2, skip=700, expect=-0.20, tol=5e-5)
QA_SEEDS = (20111, 1, 3)


def qa_signal(seed, rrc_taps):
    """200 symbols 2 * randint(0, 2) - 1 from random.Random(seed), zero-stuffed by 4 through the pulse
    (gr_interp_fir_filter_ccf from a zero delay line), times a complex sinusoid of 0.2 rad/sample"""
    r = random.Random(seed)
    data = np.array([2.0 * r.randint(0, 2) - 1.0 for _ in range(QA["nsym"])])
    sps = QA["sps"]
    up = np.zeros(len(data) * sps)
    up[::sps] = data
    s = np.convolve(up, np.asarray(rrc_taps, np.float64))[:len(up)]
    return (s * np.exp(1j * QA["spin"] * np.arange(len(s)))).astype(np.complex64)
