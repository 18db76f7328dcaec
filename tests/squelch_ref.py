"""numpy / Python restatement of gr_pwr_squelch_cc, gr_pwr_squelch_ff and gr_simple_squelch_cc
(general/gr_squelch_base_cc.cc:42-93, gr_pwr_squelch_cc.{h,cc}, gr_simple_squelch_cc.cc:53-71): float32 power, float64
single-pole recurrence, the four-state ramp machine, gating.  test_squelch_cpu.py holds it to outputs recorded from the
reference's own sources (tests/golden/ref_squelch.npz); the GPU tests hold the kernels to it.

The test signal of both test files is made here too."""
import math

import numpy as np

f32 = np.float32
MUTED, ATTACK, UNMUTED, DECAY = 0, 1, 2, 3          # the reference's enum order (gr_squelch_base_cc.h:37)

N = 20000
BURSTS = ((3000, 7000), (9000, 9030), (9500, 9900), (12000, 16000), (16040, 16100), (19990, 20000))
PAIRS = ((0.01, -20.0), (0.0001, -40.0), (0.3, -10.0), (1.0, -20.0))      # (alpha, threshold in dB)


def signal(seed, n=N, bursts=BURSTS):
    """complex Gaussian noise, 0.01 per component, plus a unit tone at 0.05 cycles per sample on `bursts`"""
    rng = np.random.default_rng(seed)
    x = 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    tone = np.exp(2j * np.pi * 0.05 * np.arange(n))
    for a, b in bursts:
        x[a:b] += tone[a:b]
    return x.astype(np.complex64)


def power(x):
    """the detector's input: re * re + im * im (two rounded float products, one rounded add), or x * x"""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        x = x.astype(np.complex64)
        return x.real * x.real + x.imag * x.imag
    x = x.astype(f32)
    return x * x


def detector(p, alpha, y=0.0):
    """y = alpha * p + (1.0 - alpha) * y in float64 (gr_single_pole_iir<double,double,double>); returns every y"""
    oma = 1.0 - alpha
    out = np.empty(len(p), np.float64)
    for i, v in enumerate(np.asarray(p, np.float64).tolist()):
        y = alpha * v + oma * y
        out[i] = y
    return out


def detector_chunked(p, alpha, y=0.0, chunk=256):
    """the FAST form: every chunk from a zero start, chained by (1 - alpha)^len, walked again from its start"""
    out = np.empty(len(p), np.float64)
    pc = (1.0 - alpha) ** chunk
    for c in range(0, len(p), chunk):
        seg = p[c:c + chunk]
        out[c:c + len(seg)] = detector(seg, alpha, y)
        end0 = detector(seg, alpha, 0.0)[-1]
        y = end0 + pc * y if len(seg) == chunk else out[c + len(seg) - 1]
    return out


def envelope(k, ramp):
    return 0.5 - math.cos((math.pi * k) / ramp) / 2.0


class PwrSquelch(object):
    def __init__(self, db, alpha=0.0001, ramp=0, gate=False, complex_items=True):
        self.cc = bool(complex_items)
        self.alpha = float(alpha)
        self.set_threshold(db)
        self.ramp = int(ramp)
        self.gate = bool(gate)
        self.state = MUTED
        self.envelope = 0.0 if self.ramp else 1.0
        self.ramped = 0
        self.y = 0.0

    def set_threshold(self, db):
        self.thr = math.pow(10.0, db / 10)

    def threshold(self):
        return 10 * math.log10(self.thr)

    def set_alpha(self, alpha):
        self.alpha = float(alpha)

    def set_ramp(self, ramp):
        self.ramp = int(ramp)

    def set_gate(self, gate):
        self.gate = bool(gate)

    def unmuted(self):
        return self.state in (UNMUTED, ATTACK)

    def work(self, x):
        x = np.asarray(x, np.complex64 if self.cc else f32)
        ys = detector(power(x), self.alpha, self.y)
        if len(ys):
            self.y = float(ys[-1])
        mute = (ys < self.thr).tolist()
        out = np.zeros(len(x), x.dtype)
        j = 0
        R = self.ramp
        for i in range(len(x)):
            if self.state == MUTED:
                if not mute[i]:
                    self.state = ATTACK if R else UNMUTED
            elif self.state == UNMUTED:
                if mute[i]:
                    self.state = DECAY if R else MUTED
            elif self.state == ATTACK:
                self.ramped += 1
                self.envelope = envelope(self.ramped, R)
                if self.ramped >= R:
                    self.state = UNMUTED
                    self.envelope = 1.0
            else:
                self.ramped -= 1
                self.envelope = envelope(self.ramped, R)
                if self.ramped == 0:
                    self.state = MUTED
            if self.state != MUTED:
                if self.cc:
                    # in * gr_complex(envelope, 0.0): the full complex product in float
                    e, z = f32(self.envelope), f32(0.0)
                    a, b = x.real[i], x.imag[i]
                    out[j] = complex(f32(a * e) - f32(b * z), f32(a * z) + f32(b * e))
                else:
                    out[j] = f32(float(x[i]) * self.envelope)
                j += 1
            elif not self.gate:
                out[j] = 0
                j += 1
        return out[:j]


class SimpleSquelch(object):
    def __init__(self, db, alpha=0.0001):
        self.alpha = float(alpha)
        self.thr = math.pow(10.0, db / 10)
        self.y = 0.0
        self._unmuted = False

    def set_threshold(self, db):
        self.thr = math.pow(10.0, db / 10)

    def threshold(self):
        return 10 * math.log10(self.thr)

    def set_alpha(self, alpha):
        self.alpha = float(alpha)

    def unmuted(self):
        return self._unmuted

    def work(self, x):
        x = np.asarray(x, np.complex64)
        ys = detector(power(x), self.alpha, self.y)
        if len(ys):
            self.y = float(ys[-1])
        self._unmuted = self.y >= self.thr
        return np.where(ys >= self.thr, x, np.complex64(0))


def closest_approach(x, alpha, db, chunked=False):
    """min |y - threshold| / threshold of the detector over the whole of x"""
    thr = math.pow(10.0, db / 10)
    ys = (detector_chunked if chunked else detector)(power(x), alpha)
    return float(np.min(np.abs(ys - thr)) / thr)
