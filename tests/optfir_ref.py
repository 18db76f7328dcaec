"""Plain-Python restatement of gnuradio/optfir.py (remezord, lporder and the four designers' argument building) and the
CPU restatement of the AM demodulator chain, for the tests of remez / optfir_* / complex_to_mag / am_demod_cf.

What optfir.py hands to gr.remez is (order, band edges, amplitudes, weights); design_args() returns exactly that, so a
test can compare it with what the C ABI derives, and the recorded fixture can be keyed by the designer's arguments."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def stopband_atten_to_dev(atten_db):
    return 10 ** (-atten_db / 20.0)                     # true division: include/grhip.h states the deviation


def passband_ripple_to_dev(ripple_db):
    return (10 ** (ripple_db / 20.0) - 1) / (10 ** (ripple_db / 20.0) + 1)


def lporder(freq1, freq2, delta_p, delta_s):
    df = abs(freq2 - freq1)
    ddp = math.log10(delta_p)
    dds = math.log10(delta_s)
    a1, a2, a3, a4, a5, a6 = 5.309e-3, 7.114e-2, -4.761e-1, -2.66e-3, -5.941e-1, -4.278e-1
    b1, b2 = 11.01217, 0.5124401
    t1 = a1 * ddp * ddp
    t2 = a2 * ddp
    t3 = a4 * ddp * ddp
    t4 = a5 * ddp
    dinf = ((t1 + t2 + a3) * dds) + (t3 + t4 + a6)
    ff = b1 + b2 * (ddp - dds)
    return dinf / df - ff * df + 1


def remezord(fcuts, mags, devs, fsamp=2):
    fcuts = [float(f) / fsamp for f in fcuts]
    mags = list(mags)
    devs = list(devs)
    nbands = len(mags)
    assert len(devs) == nbands and len(fcuts) == 2 * (nbands - 1)
    for i in range(nbands):
        if mags[i] != 0:
            devs[i] = devs[i] / mags[i]
    f1, f2 = fcuts[0::2], fcuts[1::2]
    n, min_delta = 0, 2
    for i in range(len(f1)):
        if f2[i] - f1[i] < min_delta:
            n, min_delta = i, f2[i] - f1[i]
    if nbands == 2:
        l = lporder(f1[n], f2[n], devs[0], devs[1])
    else:
        l = 0
        for i in range(1, nbands - 1):
            l1 = lporder(f1[i - 1], f2[i - 1], devs[i], devs[i - 1])
            l2 = lporder(f1[i], f2[i], devs[i], devs[i + 1])
            l = max(l, l1, l2)
    n = int(math.ceil(l)) - 1
    ff = [0.0] + [2 * f for f in fcuts] + [1.0]
    aa = []
    for a in mags:
        aa += [float(a), float(a)]
    max_dev = max(devs)
    return n, ff, aa, [max_dev / d for d in devs]


def design_args(kind, *args, **kw):
    """(order, bands, ampl, weights) that optfir.<kind>(*args) hands to gr.remez"""
    nextra = kw.get("nextra_taps", 2)
    if kind in ("low_pass", "high_pass"):
        gain, fs, f1, f2, ripple, atten = args
    else:
        gain, fs, f1, f2, f3, f4, ripple, atten = args
    pb, sb = passband_ripple_to_dev(ripple), stopband_atten_to_dev(atten)
    if kind == "low_pass":
        n, fo, ao, w = remezord([f1, f2], (gain, 0), [pb, sb], fs)
    elif kind == "high_pass":
        n, fo, ao, w = remezord([f1, f2], (0, 1), [sb, pb], fs)
    elif kind == "band_pass":
        n, fo, ao, w = remezord([f1, f2, f3, f4], (0, gain, 0), [sb, pb, sb], fs)
    elif kind == "band_reject":
        n, fo, ao, w = remezord([f1, f2, f3, f4], (gain, 0, gain), [pb, sb, pb], fs)
    else:
        raise ValueError(kind)
    if kind in ("high_pass", "band_reject") and (n + nextra) % 2 == 1:
        n += 1
    return n + nextra, fo, ao, w


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the AM demodulator (blks2impl/am_demod.py:42-58) -------------------------------------------------------------
def mag(x):
    """gr_complex_to_mag as the library defines it: (float)sqrt((double)re * re + (double)im * im)"""
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        m = np.sqrt(re * re + im * im).astype(np.float32)
    m[np.isinf(re) | np.isinf(im)] = np.inf             # hypotf: an infinite part wins over a NaN
    return m


def am_v(x):
    """complex_to_mag -> add_const_ff(-1): float32"""
    with np.errstate(invalid="ignore"):
        return (mag(x) + np.float32(-1.0)).astype(np.float32)


def am_outputs(n_in, D):
    return (n_in + D - 1) // D


def am_fir(po, v, D, taps, n_in=None):
    """fir_filter_fff(D, taps) from a zero delay line over the first n_in values of v, through the oracle"""
    taps = np.asarray(taps, np.float32)
    n_in = len(v) if n_in is None else n_in
    padded = np.concatenate([np.zeros(len(taps) - 1, np.float32), v[:n_in]])
    return po.fir_fff(taps, padded, am_outputs(n_in, D), D)


def am_fir64(v, D, taps, n_in=None):
    n_in = len(v) if n_in is None else n_in
    full = np.convolve(np.asarray(v[:n_in], np.float64), np.asarray(taps, np.float64))[:n_in]
    return full[::D]


def audio_taps(ntaps):
    """a windowed low-pass of the given length with a little asymmetry, so that a reversed tap order would show (the
    taps tests/test_gpu_fm_demod.py uses, stated again)"""
    n = np.arange(ntaps)
    h = np.sinc(0.2 * (n - (ntaps - 1) / 2.0)) * np.hamming(ntaps) if ntaps > 2 else np.array([0.75, 0.25][:ntaps])
    h = h * (1.0 + 0.01 * n / max(ntaps, 1))
    return (h / h.sum()).astype(np.float32)


def am_signal(seed, n):
    """carrier 1.0 with 50 % tone modulation plus noise, a stretch at amplitude 30, one at 1e-3, one of exact zeros"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    env = 1.0 + 0.5 * np.sin(2 * np.pi * 0.013 * t + seed)
    x = env * np.exp(1j * (0.31 * t + seed)) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    q = max(n // 8, 1)
    x[2 * q:3 * q] *= 30.0
    x[4 * q:5 * q] *= 1e-3
    x[6 * q:6 * q + max(q // 2, 1)] = 0.0
    return x.astype(np.complex64)
