"""References for the real-signal FFT blocks, in float64.

FftFilterFff restates gri_fft_filter_fff_generic (filter/gri_fft_filter_fff_generic.cc:34-158) from its description:
compute_sizes (fftsize = 2 * 2^ceil(log2 ntaps), nsamples = fftsize - ntaps + 1), the taps scaled by 1/fftsize and
transformed once, and per block of nsamples inputs: zero-pad to fftsize, real forward transform, product with the
transformed taps, unnormalised real inverse transform, the carried tail added to the first ntaps-1 results, every
decimation-th result emitted through a counter that runs across blocks, the last ntaps-1 results stashed as the next tail.
fir_direct is the function the block stands for, y[n] = sum_k taps[k] x[n D - k] with silence before the stream, and
fft_vfc the transform gr_fft_vfc computes (general/gr_fft_vfc.cc:69-107: float times window, widened, forward FFT)."""
import math

import numpy as np


def sizes(ntaps):
    """(fftsize, nsamples) as gri_fft_filter_fff_generic::compute_sizes"""
    fftsize = int(2 * math.pow(2.0, math.ceil(math.log(float(ntaps)) / math.log(2.0))))
    return fftsize, fftsize - ntaps + 1


class FftFilterFff(object):
    def __init__(self, decimation, taps):
        self.decimation = int(decimation)
        self.set_taps(taps)

    def set_taps(self, taps):
        taps = np.asarray(taps, dtype=np.float32)
        self.ntaps = len(taps)
        self.fftsize, self.nsamples = sizes(self.ntaps)
        self.tail = np.zeros(self.ntaps - 1, dtype=np.float64)
        scale = np.float32(1.0 / self.fftsize)
        padded = np.zeros(self.fftsize, dtype=np.float64)
        padded[:self.ntaps] = (taps * scale).astype(np.float32)         # the product is a float in the reference
        self.xformed = np.fft.rfft(padded)
        return self.nsamples

    def filter(self, nitems, x):
        x = np.asarray(x, dtype=np.float64)
        ninput = nitems * self.decimation
        assert ninput % self.nsamples == 0 and len(x) >= ninput
        out = []
        dec_ctr = 0
        ts = self.ntaps - 1
        for i in range(0, ninput, self.nsamples):
            blk = np.zeros(self.fftsize, dtype=np.float64)
            blk[:self.nsamples] = x[i:i + self.nsamples]
            y = np.fft.irfft(np.fft.rfft(blk) * self.xformed, self.fftsize) * self.fftsize      # FFTW's inverse: unnormalised
            y[:ts] += self.tail
            j = dec_ctr
            picked = y[j:self.nsamples:self.decimation]
            out.append(picked)
            j += len(picked) * self.decimation
            dec_ctr = j - self.nsamples
            self.tail = y[self.nsamples:self.nsamples + ts].copy()
        assert dec_ctr == 0
        return np.concatenate(out) if out else np.zeros(0)


def fir_direct(taps, x, nout, decim=1):
    """y[n] = sum_k taps[k] x[n decim - k], x[m] = 0 for m < 0, in float64"""
    taps = np.asarray(taps, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    full = np.convolve(x[:nout * decim], taps)
    return full[:nout * decim:decim][:nout]


def fft_vfc(x, fft_size, window=None):
    """numpy.fft.fft(x * w) per item of fft_size floats; the product is a float in the reference"""
    v = np.asarray(x, dtype=np.float32).reshape(-1, fft_size)
    if window is not None and len(window):
        v = v * np.asarray(window, dtype=np.float32)[None, :]
    return np.fft.fft(v.astype(np.float64), axis=1).reshape(-1)
