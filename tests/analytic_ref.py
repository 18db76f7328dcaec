"""Restatements for the three real -> complex blocks (a helper, not a test).

firdes_hilbert / window: gr_firdes::hilbert and gr_firdes::window (general/gr_firdes.cc:538-565, 720-780) from their
description.  window() computes in double and narrows each value to float; its WIN_RECTANGULAR case has no break and
runs on into WIN_HAMMING, so a "rectangular" window IS a Hamming window.  hilbert() works in float: 1/(float)i, float
products, the alternating float recurrence gain = taps[h+i] - gain, 2*fabs(gain) and a float division per tap.

hilbert_fc / filter_delay_fc: out[i] = (in0[i + ntaps/2], fir_fff(&in1[i])) (filter/gr_hilbert_fc.cc:57-66,
filter/gr_filter_delay_fc.cc:57-79), the FIR sums through the checker's fir_fff (gr_fir_fff_generic's order).

goertzel: gri_goertzel (filter/gri_goertzel.cc:36-75) in float32, one numpy lane per block: w narrowed to float,
wr = 2 cosf(w), wi = sinf(w) through libm (numpy's float cosine may differ in the last place), y = (x + wr*d1) - d2
with every operation rounded, the real part of the output formed in double, the imaginary part in float.
goertzel64 is the same recurrence in float64 with the same float wr, wi: the yardstick of the FAST kernel.
"""
import ctypes as C
import ctypes.util
import math

import numpy as np

f32 = np.float32
WIN_HAMMING, WIN_HANN, WIN_BLACKMAN, WIN_RECTANGULAR, WIN_KAISER, WIN_BLACKMAN_hARRIS = range(6)
WINDOWS = (WIN_HAMMING, WIN_HANN, WIN_BLACKMAN, WIN_RECTANGULAR, WIN_KAISER, WIN_BLACKMAN_hARRIS)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = C.c_float
_libm.cosf.argtypes = [C.c_float]
_libm.sinf.restype = C.c_float
_libm.sinf.argtypes = [C.c_float]


def _izero(x):
    """Izero of general/gr_firdes.cc:35-49 (double)"""
    s = u = 1.0
    n = 1
    halfx = x / 2.0
    while True:
        t = halfx / float(n)
        n += 1
        t *= t
        u *= t
        s += u
        if not u >= 1e-21 * s:
            return s


def window(wtype, ntaps, beta=6.76):
    M = ntaps - 1
    w = np.zeros(ntaps, dtype=f32)
    pi = math.pi
    if wtype in (WIN_RECTANGULAR, WIN_HAMMING):          # the missing break
        for n in range(ntaps):
            w[n] = 0.54 - 0.46 * math.cos((2 * pi * n) / M)
    elif wtype == WIN_HANN:
        for n in range(ntaps):
            w[n] = 0.5 - 0.5 * math.cos((2 * pi * n) / M)
    elif wtype == WIN_BLACKMAN:
        for n in range(ntaps):
            w[n] = 0.42 - 0.50 * math.cos((2 * pi * n) / (M - 1)) - 0.08 * math.cos((4 * pi * n) / (M - 1))
    elif wtype == WIN_BLACKMAN_hARRIS:
        half = int(ntaps / 2)                            # C's division (ntaps > 0)
        Mf = float(f32(M))
        for n in range(-half, half):                     # an odd length leaves the last value at 0
            w[n + half] = (0.35875 + 0.48829 * math.cos((2 * pi * n) / Mf) + 0.14128 * math.cos((4 * pi * n) / Mf)
                           + 0.01168 * math.cos((6 * pi * n) / Mf))
    elif wtype == WIN_KAISER:
        ib = 1.0 / _izero(beta)
        inm1 = 1.0 / float(ntaps)
        for i in range(ntaps):
            t = i * inm1
            w[i] = _izero(beta * math.sqrt(1.0 - t * t)) * ib
    else:
        raise ValueError("window type out of range")
    return w


def firdes_hilbert(ntaps, wtype=WIN_RECTANGULAR, beta=6.76):
    if not ntaps & 1:
        raise ValueError("Hilbert:  Must have odd number of taps")
    taps = np.zeros(ntaps, dtype=f32)
    w = window(wtype, ntaps, beta)
    h = (ntaps - 1) // 2
    gain = f32(0)
    with np.errstate(all="ignore"):
        for i in range(1, h + 1):
            if i & 1:
                x = f32(1) / f32(i)
                taps[h + i] = x * w[h + i]
                taps[h - i] = -x * w[h - i]
                gain = f32(taps[h + i] - gain)
        gain = f32(2) * f32(abs(gain))
        return (taps / gain).astype(f32)


def filter_delay_fc(po, taps, n, in0, in1=None):
    """n outputs; in0 (and in1) carry len(taps) - 1 history items in front"""
    taps = np.ascontiguousarray(taps, dtype=f32)
    in0 = np.ascontiguousarray(in0, dtype=f32)
    in1 = in0 if in1 is None else np.ascontiguousarray(in1, dtype=f32)
    d = len(taps) // 2
    out = np.zeros(n, dtype=np.complex64)
    out.real = in0[d:d + n]
    out.imag = po.fir_fff(taps, in1, n)
    return out


def hilbert_fc(po, ntaps, n, x, wtype=WIN_RECTANGULAR, beta=6.76):
    return filter_delay_fc(po, firdes_hilbert(ntaps | 1, wtype, beta), n, x)


def filter_delay_fc64(taps, n, in0, in1=None):
    """the same block with the sum in float64 (yardstick of the FAST kernels)"""
    t = np.asarray(taps, dtype=np.float64)
    in0 = np.asarray(in0, dtype=np.float64)
    in1 = in0 if in1 is None else np.asarray(in1, dtype=np.float64)
    d = len(t) // 2
    return in0[d:d + n] + 1j * np.convolve(in1[:n + len(t) - 1], t, mode="valid")[:n]


def goertzel_params(rate, freq):
    """(wr, wi) as gri_setparms computes them"""
    w = f32(2.0 * math.pi * float(f32(freq)) / int(rate))
    wr = f32(2.0 * float(_libm.cosf(C.c_float(float(w)))))
    wi = f32(_libm.sinf(C.c_float(float(w))))
    return wr, wi


def goertzel_fc(rate, length, freq, x, nblocks=None):
    wr, wi = goertzel_params(rate, freq)
    x = np.ascontiguousarray(x, dtype=f32)
    nb = len(x) // length if nblocks is None else nblocks
    xb = x[:nb * length].reshape(nb, length)
    d1 = np.zeros(nb, dtype=f32)
    d2 = np.zeros(nb, dtype=f32)
    for i in range(length):
        y = (xb[:, i] + wr * d1) - d2
        d2 = d1
        d1 = y
    assert d1.dtype == f32
    out = np.zeros(nb, dtype=np.complex64)
    out.real = ((0.5 * float(wr) * d1.astype(np.float64) - d2.astype(np.float64)) / int(length)).astype(f32)
    out.imag = (wi * d1) / f32(length)
    return out


def goertzel64(rate, length, freq, x, nblocks=None):
    wr, wi = (float(v) for v in goertzel_params(rate, freq))
    x = np.asarray(x, dtype=np.float64)
    nb = len(x) // length if nblocks is None else nblocks
    xb = x[:nb * length].reshape(nb, length)
    d1 = np.zeros(nb)
    d2 = np.zeros(nb)
    for i in range(length):
        y = (xb[:, i] + wr * d1) - d2
        d2 = d1
        d1 = y
    return (0.5 * wr * d1 - d2) / length + 1j * (wi * d1) / length
