"""numpy restatements of the spectrum-estimate blocks, in the reference's number formats.

- mag_squared: float32 products and add (general/gr_complex_to_xxx.cc:198).
- SinglePoleIir: double taps, float32 state, y = float32(alpha * x + (1 - alpha) * y_prev) with x and y_prev widened
  (filter/gr_single_pole_iir.h:60-97); iir_f64 is the float64 recurrence the FAST mode is judged against.
- nlog10 / nlog10_f64 (general/gr_nlog10_ff.cc:60-61; numpy's float32 log10 is not the device's, so the device is
  judged against the float64 value of the same float input).
- KeepOneInN: the countdown of general/gr_keep_one_in_n.cc:52-90.
- chain_f64: the float64 form of blks2.logpwrfft's chain (blks2impl/logpwrfft.py:54-63) (numpy FFT of the float-windowed input, float64 power and recurrence)."""
import numpy as np

f32 = np.float32


def mag_squared(z):
    z = np.asarray(z, np.complex64)
    re, im = z.real.astype(f32), z.imag.astype(f32)
    return (re * re + im * im).astype(f32)


class SinglePoleIir(object):
    """items of vlen floats; x is [items * vlen] (or [S, items * vlen] for S streams with their own state)"""

    def __init__(self, alpha, vlen=1, streams=1):
        self.vlen, self.streams = vlen, streams
        self.prev = np.zeros((streams, vlen), f32)
        self.set_taps(alpha)

    def set_taps(self, alpha):
        if alpha < 0 or alpha > 1:
            raise IndexError("Alpha must be in [0, 1]")
        self.alpha = float(alpha)
        self.one_minus_alpha = 1.0 - float(alpha)

    def work(self, x):
        x = np.asarray(x, f32).reshape(self.streams, -1, self.vlen)
        out = np.empty_like(x)
        y = self.prev
        for j in range(x.shape[1]):
            y = (self.alpha * x[:, j, :].astype(np.float64) + self.one_minus_alpha * y.astype(np.float64)).astype(f32)
            out[:, j, :] = y
        self.prev = y
        return out.reshape(-1)


def iir_f64(x, alpha, y0=None):
    """float64 recurrence along axis 0; returns (outputs, last output)"""
    x = np.asarray(x, np.float64)
    y = np.zeros(x.shape[1:]) if y0 is None else np.asarray(y0, np.float64)
    out = np.empty_like(x)
    for j in range(x.shape[0]):
        y = alpha * x[j] + (1.0 - alpha) * y
        out[j] = y
    return out, y


def _clamp(x):
    x = np.asarray(x, f32)
    return np.where(x < f32(1e-18), f32(1e-18), x)             # std::max(in, 1e-18f): a NaN stays


def nlog10(x, n=1, k=0):
    # log10 in float64, narrowed: the correctly rounded float log10 (numpy's own float32 log10 is not)
    return (f32(n) * np.log10(_clamp(x).astype(np.float64)).astype(f32) + f32(k)).astype(f32)


def nlog10_f64(x, n=1, k=0):
    return float(f32(n)) * np.log10(_clamp(x).astype(np.float64)) + float(f32(k))


class KeepOneInN(object):
    def __init__(self, n):
        self.set_n(n)

    def set_n(self, n):
        self.n = max(int(n), 1)
        self.count = self.n

    def kept(self, n_in):
        """indices of the kept items among the next n_in; advances the countdown"""
        idx = []
        for i in range(n_in):
            self.count -= 1
            if self.count <= 0:
                idx.append(i)
                self.count = self.n
        return idx


def chain_f64(frames, window, alpha, k, y0=None):
    """frames [F, N] (kept frames of one stream): dB [F, N] in float64, linear averaged power [F, N], last state"""
    w = np.asarray(window, np.float64).astype(f32)
    xw = np.asarray(frames).astype(np.complex128 if np.iscomplexobj(frames) else np.float64) * w.astype(np.float64)
    spec = np.fft.fft(xw, axis=1)
    p, last = iir_f64(spec.real ** 2 + spec.imag ** 2, alpha, y0)
    return 10.0 * np.log10(np.maximum(p, 1e-18)) + float(k), p, last
