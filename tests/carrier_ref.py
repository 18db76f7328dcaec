"""Restatement of the reference's four carrier loops, general/gri_control_loop.cc:49-80, gr_pll_freqdet_cf.cc:50-90,
gr_pll_refout_cc.cc:70-93, gr_pll_carriertracking_cc.cc:92-120 and gr-digital/lib/digital_costas_loop_cc.cc:69-153, in
float32 scalars with every operation rounded once and double where the reference's expression is double; the loop-gain
arithmetic; and the test signals.  Sine and cosine are the float-rounded float64 ones (sincos="rounded": what the
device's GRHIP_MODE_GENERIC computes), which is not the reference's sincosf to the bit; the Costas loop can also run in
float64 throughout (costas64), the yardstick of the deviation contract.  tests/golden/ref_carrier.npz pins the PLLs'
state to the reference's own code bit for bit (test_carrier_cpu.py states how it was recorded)."""
import hashlib
import math
import os
import re

import numpy as np

N = 6037
CUT = 4097
SEEDS = (1, 2, 3)
WIN = 1024                      # CARRIER_WIN of csrc/carrier.h
SECTIONS, SEC_LEN = (0, 1400, 2400, 3960), 256      # what the fixture keeps of outputs that are not bit exact
f32 = np.float32
PI = math.pi
TWOPI = 2.0 * math.pi           # (2.0f*M_PI): a double
ULP_2PI = 2.0 ** -21            # ulp of a float in [4, 8)

# ---- loop gains ------------------------------------------------------------------------------------------------
DAMPING0 = f32(np.sqrt(f32(2.0)) / f32(2.0))            # gri_control_loop.cc:38
GAIN_CASES = ((0.0, 0.7071), (math.pi / 100, 0.7071), (2 * math.pi / 100, 0.7071), (0.05, 0.7071), (0.25, 0.7071),
              (1.0, 0.7071), (0.01, 0.0), (0.01, 1.0), (0.3, 0.5), (3.0, 0.25), (1e-4, 0.9), (100.0, 0.7071))


def gains(loop_bw, damping=None):
    """(alpha, beta) of update_gains (:49-54): a float denom from a double expression around the float product bw * bw"""
    d = DAMPING0 if damping is None else f32(damping)
    bw = f32(loop_bw)
    denom = f32(1.0 + 2.0 * float(d) * float(bw) + float(bw * bw))
    return (f32(4) * d * bw) / denom, (f32(4) * bw * bw) / denom


class Loop(object):
    """alpha, beta, max_freq, min_freq as floats, and the state"""

    def __init__(self, loop_bw, max_freq, min_freq, damping=None):
        self.alpha, self.beta = gains(loop_bw, damping)
        self.max_freq, self.min_freq = f32(max_freq), f32(min_freq)
        self.phase, self.freq, self.locksig = f32(0), f32(0), f32(0)
        self.wraps = self.limits = self.mod_up = self.mod_down = self.clips = 0

    def set_frequency(self, freq):          # :126-135
        freq = f32(freq)
        self.freq = self.min_freq if freq > self.max_freq else (self.max_freq if freq < self.min_freq else freq)

    def set_phase(self, phase):             # :137-145
        p = f32(phase)
        while float(p) > TWOPI:
            p = f32(float(p) - TWOPI)
        while float(p) < -TWOPI:
            p = f32(float(p) + TWOPI)
        self.phase = p

    def step(self, error):
        """advance_loop, phase_wrap, frequency_limit (:56-80)"""
        freq = self.freq + self.beta * error
        phase = self.phase + freq + self.alpha * error
        while float(phase) > TWOPI:
            phase = f32(float(phase) - TWOPI)
            self.wraps += 1
        while float(phase) < -TWOPI:
            phase = f32(float(phase) + TWOPI)
            self.wraps += 1
        if freq > self.max_freq:
            freq = self.max_freq
            self.limits += 1
        elif freq < self.min_freq:
            freq = self.min_freq
            self.limits += 1
        self.phase, self.freq = phase, freq


# ---- gr_fast_atan2f (general/gr_fast_atan2f.cc:125-198) for finite input, in float32 arrays -------------------------
def _atan_table():
    txt = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "atan_table.inc")).read()
    w = [int(t, 16) for t in re.findall(r"0x[0-9a-fA-F]+", txt)]
    assert len(w) == 257
    return np.array(w, np.uint32).view(np.float32)


_TAB = None


def fast_atan2f(y, x):
    global _TAB
    if _TAB is None:
        _TAB = _atan_table()
    y, x = np.asarray(y, np.float32), np.asarray(x, np.float32)
    ya, xa = np.abs(y), np.abs(x)
    big = xa > ya
    num, den = np.where(big, ya, xa), np.where(big, xa, ya)
    with np.errstate(all="ignore"):
        z = np.where(den == 0, f32(0), num / np.where(den == 0, f32(1), den)).astype(np.float32)
    alpha = z * f32(256) - f32(0.5)
    idx = np.clip(alpha.astype(np.int32), 0, 255)
    alpha = alpha - idx.astype(np.float32)
    interp = _TAB[idx] + (_TAB[idx + 1] - _TAB[idx]) * alpha
    base = np.where(z < np.array(0x3b808082, np.uint32).view(np.float32), z, interp).astype(np.float32)
    pi_f, hpi_f = f32(3.14159265358979323846), f32(1.57079632679489661923)
    xpos, ypos = x >= 0, y >= 0
    q = np.where(big, np.where(xpos, f32(0), pi_f), hpi_f).astype(np.float32)
    ap = q + np.where(big != xpos, -base, base)
    return np.where(den == 0, f32(0), np.where(ypos, ap, -ap)).astype(np.float32)


def sincos_rounded(phase):
    """(float)sin((double)phase), (float)cos((double)phase) of a float32 array"""
    p = np.asarray(phase, np.float32).astype(np.float64)
    return np.sin(p).astype(np.float32), np.cos(p).astype(np.float32)


# ---- the three PLLs ---------------------------------------------------------------------------------------------
class PllRun(object):
    """phases / freqs / locks: the state in front of every sample and after the last (n + 1 floats; locks[k + 1] is
    the lock signal behind sample k); freqdet, refout, ct: the three blocks' outputs"""


def mod_2pi(v, loop=None):
    if float(v) > PI:
        if loop is not None:
            loop.mod_up += 1
        return f32(float(v) - TWOPI)
    if float(v) < -PI:
        if loop is not None:
            loop.mod_down += 1
        return f32(float(v) + TWOPI)
    return v


def pll(loop, x, squelch=False, threshold=0.0):
    """one work call of all three PLLs on x (they share the state walk) from the state in `loop`, which it advances"""
    x = np.asarray(x, np.complex64)
    n = len(x)
    theta = fast_atan2f(x.imag, x.real)
    phases, freqs = np.zeros(n + 1, np.float32), np.zeros(n + 1, np.float32)
    for i in range(n):
        phases[i], freqs[i] = loop.phase, loop.freq
        loop.step(mod_2pi(theta[i] - loop.phase, loop))
    phases[n], freqs[n] = loop.phase, loop.freq
    r = PllRun()
    r.phases, r.freqs = phases, freqs
    r.freqdet = freqs[:-1].copy()
    t_imag, t_real = sincos_rounded(phases[:-1])
    r.refout = np.zeros(n, np.complex64)
    ro = r.refout.view(np.float32)
    ro[0::2], ro[1::2] = t_real, t_imag
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    r.ct = np.zeros(n, np.complex64)
    co = r.ct.view(np.float32)
    co[0::2] = xr * t_real - xi * (-t_imag)                 # gr_pll_carriertracking_cc.cc:105
    co[1::2] = xr * (-t_imag) + xi * t_real
    c = xr * t_real + xi * t_imag                           # :114
    locks = np.zeros(n + 1, np.float32)
    lock, keep, a = loop.locksig, 1.0 - float(loop.alpha), loop.alpha
    for i in range(n):
        locks[i] = lock
        lock = f32(float(lock) * keep + float(a * c[i]))    # :113-114
    locks[n] = lock
    loop.locksig = lock
    r.locks = locks
    r.open = np.abs(locks[1:]) > f32(threshold)             # :116, after the sample's update
    if squelch:
        r.ct[~r.open] = 0
    return r


def join(runs):
    """the runs of consecutive calls as one"""
    r = runs[0].__class__()
    for k, v in vars(runs[0]).items():
        if k in ("phases", "freqs", "locks"):
            setattr(r, k, np.concatenate([q.__dict__[k][:-1] for q in runs] + [runs[-1].__dict__[k][-1:]]))
        else:
            setattr(r, k, np.concatenate([q.__dict__[k] for q in runs]))
    return r


def in_calls(fn, loop, x, cuts=(), **kw):
    edges = [0] + [c for c in cuts if 0 < c < len(x)] + [len(x)]
    return join([fn(loop, x[a:b], **kw) for a, b in zip(edges[:-1], edges[1:])])


# ---- Costas -----------------------------------------------------------------------------------------------------
K8 = f32(math.sqrt(2.0) - 1)


def _detector(order, re, im):
    """digital_costas_loop_cc.cc:69-108 on Python floats that hold float32 values; orders 4 and 8 in double"""
    if order == 2:
        return None
    a = im if re > 0 else -im
    b = re if im > 0 else -re
    if order == 4:
        return a - b
    k = float(K8)
    return a - b * k if abs(re) >= abs(im) else a * k - b


class CostasRun(object):
    """out, freq (d_freq behind every sample), phases (n + 1: in front of every sample and after the last)"""


def costas(loop, x, order=2):
    """one work call in float32, the NCO's sine and cosine the float-rounded double ones; advances `loop`"""
    x = np.asarray(x, np.complex64)
    n = len(x)
    out = np.zeros(n, np.complex64)
    of = out.view(np.float32)
    fr, phases = np.zeros(n, np.float32), np.zeros(n + 1, np.float32)
    xr, xi = x.real, x.imag
    one = f32(1.0)
    for i in range(n):
        phases[i] = loop.phase
        ang = float(-loop.phase)
        sn, cs = f32(math.sin(ang)), f32(math.cos(ang))
        o_re = xr[i] * cs - xi[i] * sn
        o_im = xr[i] * sn + xi[i] * cs
        of[2 * i], of[2 * i + 1] = o_re, o_im
        e = o_re * o_im if order == 2 else f32(_detector(order, float(o_re), float(o_im)))
        x1 = np.abs(e + one) - np.abs(e - one)              # gr_math.h:63-69
        c = f32(0.5 * float(x1))
        loop.clips += int(abs(e) > one)
        loop.step(c)
        fr[i] = loop.freq
    phases[n] = loop.phase
    r = CostasRun()
    r.out, r.freq, r.phases = out, fr, phases
    return r


def costas64(loop, x, order=2):
    """the same recurrence in float64 throughout, on the same input and the same (float) gains and limits"""
    x = np.asarray(x, np.complex64)
    n = len(x)
    out = np.zeros(n, np.complex128)
    fr, phases = np.zeros(n), np.zeros(n + 1)
    xr, xi = x.real.astype(np.float64), x.imag.astype(np.float64)
    ph, fq = float(loop.phase), float(loop.freq)
    al, be, mx, mn = float(loop.alpha), float(loop.beta), float(loop.max_freq), float(loop.min_freq)
    for i in range(n):
        phases[i] = ph
        sn, cs = math.sin(-ph), math.cos(-ph)
        o_re = xr[i] * cs - xi[i] * sn
        o_im = xr[i] * sn + xi[i] * cs
        out[i] = complex(o_re, o_im)
        e = o_re * o_im if order == 2 else _detector(order, o_re, o_im)
        e = 0.5 * (abs(e + 1.0) - abs(e - 1.0))
        fq = fq + be * e
        ph = ph + fq + al * e
        while ph > TWOPI:
            ph -= TWOPI
        while ph < -TWOPI:
            ph += TWOPI
        fq = mx if fq > mx else (mn if fq < mn else fq)
        fr[i] = fq
    phases[n] = ph
    loop.phase64, loop.freq64 = ph, fq
    r = CostasRun()
    r.out, r.freq, r.phases = out, fr, phases
    return r


def circ(a, b):
    """largest circular difference of two phase tracks"""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.max(np.abs((d + PI) % TWOPI - PI)))


def bound(dev_ref):
    return 2.0 * dev_ref + 4.0 * ULP_2PI


# ---- test signals -----------------------------------------------------------------------------------------------
def envelope():
    env = np.empty(N)
    env[:1500] = 1.0
    env[1500:2500] = 0.0
    env[2500:4000] = 30.0
    env[4000:] = 0.02
    return env


AUDIO = 32e3            # wfm_rcv_pll with demod_rate 256 kHz and audio_decimation 8
# name, loop_bw, max_freq, min_freq, the tone's frequency in rad/sample on [0, 1500), [1500, 4000) and from 4000 on
PLL_SETS = (
    ("limit", 0.05, 1.0, -1.0, (0.7, 0.97, -0.97)),
    ("wrap", 0.2, 2.5, -2.5, (1.9, -2.2, 0.7)),
    ("wfm_demod", 2 * math.pi / 100, 2 * math.pi * 90e3 / 256e3, -2 * math.pi * 90e3 / 256e3, (0.5, -1.5, 2.0)),
    ("wfm_pilot", 2 * math.pi / 100, -2 * math.pi * 18990 / AUDIO, -2 * math.pi * 19010 / AUDIO,
     (-2 * math.pi * 19000 / AUDIO, -2 * math.pi * 19004 / AUDIO, -2 * math.pi * 18995 / AUDIO)),
)


def pll_loop(pset):
    return Loop(pset[1], pset[2], pset[3])


def pll_signal(seed, pset):
    """a complex tone whose frequency steps at 1500 and at 4000, its amplitude 1, 0, 30 and 0.02 in sections, with
    noise of 5 % of the amplitude"""
    rng = np.random.default_rng(seed)
    f = np.empty(N)
    f[:1500], f[1500:4000], f[4000:] = pset[4]
    ph = rng.uniform(-PI, PI) + np.cumsum(f)
    noise = 0.05 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return (envelope() * (np.exp(1j * ph) + noise)).astype(np.complex64)


# name, order, loop_bw, amplitude, frequency offset (rad/sample), noise, set_frequency before the first sample
COSTAS_SETS = (
    ("bpsk", 2, 0.05, 1.0, 2e-3, 0.02, None),
    ("qpsk", 4, 0.05, 1.0, 2e-3, 0.01, None),
    ("8psk", 8, 0.05, 2.0, 1e-3, 0.005, None),
    ("clip", 2, 0.05, 3.0, 2e-3, 0.2, None),
    ("limit", 2, 0.1, 1.0, 0.9995, 0.05, 0.999),
)


def costas_loop(cset):
    loop = Loop(cset[2], 1.0, -1.0)
    if cset[6] is not None:
        loop.set_frequency(cset[6])
    return loop


def constellation(order, amplitude=1.0):
    """the QA's constellations (gr-digital/python/qa_costas_loop_cc.py): +-1, +-1 +-j, and 2 exp(j pi / 8) times the
    eighth roots of unity"""
    if order == 2:
        return amplitude * np.array([1, -1], np.complex128)
    if order == 4:
        return amplitude * np.array([1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j])
    return amplitude * np.exp(1j * PI / 8) * np.exp(2j * PI * np.arange(8) / 8)


def costas_signal(seed, cset):
    """seeded symbols rotated by 0.2 rad plus a frequency offset, with small noise"""
    _, order, _, amp, fo, noise, _ = cset
    rng = np.random.default_rng(seed)
    sym = constellation(order, amp)[rng.integers(0, order, N)]
    rot = np.exp(1j * (0.2 + fo * np.arange(N)))
    w = noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return (sym * rot + w).astype(np.complex64)


def boundary_distance(order, out):
    """distance of every output from the nearest decision boundary of the order's detector, relative to |out|"""
    o = np.asarray(out, np.complex128)
    re, im = np.abs(o.real), np.abs(o.imag)
    d = np.minimum(re, im)
    if order == 8:
        d = np.minimum(d, np.abs(re - im) / math.sqrt(2.0))
    return d / np.abs(o)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
