"""numpy / Python restatement of blks2.logpwrfft on top of spectrum_ref.py.

- blackmanharris: the cosine-sum closure of gnuradio/window.py:166-176, term by term in double.
- window_power / k_of: blks2impl/logpwrfft.py:53-62 (k in double; gr_nlog10_ff receives it as a float).
- decimation_of: blks2impl/stream_to_vector_decimator.py:71-75, max(1, int(round(decim))) with Python 2's round (half away
  from zero; Python 3's rounds half to even, so it is written out).  True division throughout.
- LogPwrFft: the block over whole frames, given a transform function: keep-one countdown, float-windowed transform,
  float32 mag^2, the single-pole IIR (taps 1.0 while averaging is off) and the float64-rounded log of spectrum_ref."""
import math

import numpy as np

import spectrum_ref as sr

f32 = np.float32
COEFFS = (0.35875, 0.48829, 0.14128, 0.01168)


def blackmanharris(fft_size):
    """the four-term cosine sum of window.blackmanharris as doubles: term c is sign_c * COEFFS[c] * cos(angle_c), the angle
    formed as ((2.0 * c) * pi) * (i + 0.5) / (fft_size - 1), the terms added one after the other starting from 0"""
    if fft_size == 1:
        raise ZeroDivisionError("fft_size - 1 is the divisor")
    i = np.arange(fft_size, dtype=np.float64)
    acc = np.zeros(fft_size, np.float64)
    for c, a in enumerate(COEFFS):
        sign = -1.0 if c & 1 else 1.0
        angle = 2.0 * c * math.pi * (i + 0.5) / (fft_size - 1)
        acc = acc + (sign * a) * np.array([math.cos(v) for v in angle])      # libm's cos, one element at a time
    return acc.tolist()


def window_power(fft_window):
    """sum of squares, accumulated left to right from 0"""
    total = 0.0
    for v in fft_window:
        total = total + v * v
    return total


def k_of(fft_size, fft_window, ref_scale):
    return (-20 * math.log10(fft_size)
            - 10 * math.log10(window_power(fft_window) / fft_size)
            - 20 * math.log10(ref_scale / 2))


def round_half_away(x):
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def decimation_of(sample_rate, vec_len, vec_rate):
    return max(1, int(round_half_away(sample_rate / vec_len / vec_rate)))


class LogPwrFft(object):
    def __init__(self, sample_rate, fft_size, ref_scale, frame_rate, avg_alpha, average, win=None, streams=1, fft=None):
        self.N, self.S = fft_size, streams
        w = blackmanharris(fft_size) if win is None else list(win)
        self.k = f32(k_of(fft_size, w, ref_scale))
        self.window = np.asarray(w, np.float64).astype(f32) if len(w) == fft_size else None     # set_window refuses another length
        self._sample_rate, self._vec_rate = sample_rate, frame_rate
        self.keep = sr.KeepOneInN(1)
        self.set_decimation(sample_rate / fft_size / frame_rate)
        self.iir = sr.SinglePoleIir(1.0, fft_size, streams)
        self._avg_alpha, self._average = avg_alpha, average
        self.set_average(average)
        self.fft = fft or (lambda frames: np.fft.fft(frames, axis=-1).astype(np.complex64))

    def set_decimation(self, decim):
        self._decim = max(1, int(round_half_away(decim)))
        self.keep.set_n(self._decim)

    def set_vec_rate(self, r):
        self._vec_rate = r
        self.set_decimation(self._sample_rate / self.N / self._vec_rate)

    def set_sample_rate(self, r):
        self._sample_rate = r
        self.set_decimation(self._sample_rate / self.N / self._vec_rate)

    def set_average(self, average):
        self._average = average
        self.iir.set_taps(self._avg_alpha if average else 1.0)

    def set_avg_alpha(self, a):
        self._avg_alpha = a
        self.set_average(self._average)

    def decimation(self):
        return self._decim

    def frame_rate(self):
        return self._sample_rate / self.N / self._decim

    def work(self, n_frames, x):
        """x: [S][n_frames][N] samples; returns [S][kept][N] dB, flattened"""
        idx = self.keep.kept(n_frames)
        if not idx:
            return np.zeros(0, f32)
        fr = np.asarray(x).reshape(self.S, n_frames, self.N)[:, idx]
        if self.window is not None:
            fr = (fr * self.window).astype(np.complex64 if np.iscomplexobj(fr) else f32)
        p = sr.mag_squared(self.fft(fr).reshape(-1))
        return sr.nlog10(self.iir.work(p.reshape(self.S, -1)), 10, self.k)
