"""References for the real-input FIR kinds (gr_fir_filter_fcc / _scc / _fsf, gr_freq_xlating_fir_filter_fcf / _fcc /
_scf / _scc / _ccf).

For finite inputs the ccc oracle on widened input is an exact reference of the complex-output kinds:
(tr + j ti)(x + j0) gives tr*x -/+ 0 and +/-0 + ti*x, the accumulators start at +0 so a zero of either sign never
changes a sum, N_UNROLL is 2 in both, and the composite taps of the ?cf kinds, (a*c, a*d), differ from the ccc
oracle's (a*c - 0*d, a*d + 0*c) at most in the sign of zero.  The direct numpy float32 restatements below (one IEEE
operation per numpy operation, no fused multiply-add) pin that equivalence and are the reference for non-finite
inputs, where the ccc product's NaN recovery differs from a real product."""
import numpy as np


def x86_f2s(acc):
    """(short)acc as the reference's x86-64 build converts: cvttss2si to int32 (NaN and |acc| >= 2^31 give
    0x80000000), then the low 16 bits"""
    a = np.asarray(acc, dtype=np.float32)
    out = np.zeros(a.shape, dtype=np.int64)
    ok = np.isfinite(a) & (np.abs(a.astype(np.float64)) < 2.0 ** 31)
    out[ok] = np.trunc(a[ok].astype(np.float64)).astype(np.int64)
    return (out & 0xFFFF).astype(np.uint16).view(np.int16)


def _windows(x, n, decim, i):
    return x[np.arange(n, dtype=np.int64) * decim + i]


def fir_cc_direct(taps_fwd, x, n, decim=1):
    """gr_fir_fcc_generic / gr_fir_scc_generic (taps in forward order, as gr_fir_filter_XXX takes them): complex
    accumulators, N_UNROLL 2, products complex * float, scc's (float) cast"""
    d = np.ascontiguousarray(np.asarray(taps_fwd, np.complex64)[::-1])
    xf = np.asarray(x).astype(np.float32)
    T = len(d)
    z = np.zeros(n, np.float32)
    a0r, a0i, a1r, a1i = z.copy(), z.copy(), z.copy(), z.copy()
    nn = (T // 2) * 2
    for i in range(0, nn, 2):
        x0, x1 = _windows(xf, n, decim, i), _windows(xf, n, decim, i + 1)
        a0r = a0r + np.float32(d[i].real) * x0
        a0i = a0i + np.float32(d[i].imag) * x0
        a1r = a1r + np.float32(d[i + 1].real) * x1
        a1i = a1i + np.float32(d[i + 1].imag) * x1
    for i in range(nn, T):
        x0 = _windows(xf, n, decim, i)
        a0r = a0r + np.float32(d[i].real) * x0
        a0i = a0i + np.float32(d[i].imag) * x0
    out = np.empty(n, np.complex64)
    out.real = a0r + a1r
    out.imag = a0i + a1i
    return out


def fir_fsf_direct(taps_fwd, x, n, decim=1):
    """gr_fir_fsf_generic: float accumulators, N_UNROLL 4, (short) of the sum"""
    d = np.ascontiguousarray(np.asarray(taps_fwd, np.float32)[::-1])
    xf = np.asarray(x, np.float32)
    T = len(d)
    acc = [np.zeros(n, np.float32) for _ in range(4)]
    nn = (T // 4) * 4
    for i in range(0, nn, 4):
        for u in range(4):
            acc[u] = acc[u] + d[i + u] * _windows(xf, n, decim, i + u)
    for i in range(nn, T):
        acc[0] = acc[0] + d[i] * _windows(xf, n, decim, i)
    return x86_f2s(acc[0] + acc[1] + acc[2] + acc[3])


def cmul_ref(a, b):
    """complex<float> product, unfused (gr_rotator.h:43)"""
    ar, ai = a.real.astype(np.float32), a.imag.astype(np.float32)
    br, bi = b.real.astype(np.float32), b.imag.astype(np.float32)
    out = np.empty(len(a), np.complex64)
    out.real = ar * br - ai * bi
    out.imag = ar * bi + ai * br
    return out


def fcc_ref(po, taps_fwd, x, n, decim=1):
    """exact for finite x: the ccc oracle on widened input"""
    return po.fir_ccc(np.asarray(taps_fwd, np.complex64), np.asarray(x).astype(np.float32) + 0j, n, decim)


def fsf_ref(po, taps_fwd, x, n, decim=1):
    return x86_f2s(po.fir_fff(np.asarray(taps_fwd, np.float32), np.asarray(x, np.float32), n, decim))


class XlatingRef(object):
    """gr_freq_xlating_fir_filter_XXX for real (or complex) items, exact for finite input: the ccc oracle on
    widened input with the prototype as complex taps; keeps the rotator across calls"""

    def __init__(self, po, decim, proto, center_freq, sampling_freq):
        self.x = po.Xlating(decim, np.asarray(proto).astype(np.complex64), center_freq, sampling_freq)

    def work(self, x_with_history, nout):
        x = np.asarray(x_with_history)
        if not np.iscomplexobj(x):
            x = x.astype(np.float32) + 0j
        return self.x.work(x.astype(np.complex64), nout)


def xlating_direct(po, decim, proto, center_freq, sampling_freq, x_with_history, nout):
    """direct restatement of a fresh block's first call: composite taps (the oracle's, zero signs aside), gr_fir_fcc
    order over the real items, then the rotator phases with the unfused product"""
    xl = po.Xlating(decim, np.asarray(proto).astype(np.complex64), center_freq, sampling_freq)
    ctaps = xl.ctaps()                                  # d_taps order of the inner FIR
    y = fir_cc_direct(ctaps[::-1], x_with_history, nout, decim)
    _, incr, _ = xl.rot()
    return cmul_ref(y, po.rotator_phases(incr, nout))
