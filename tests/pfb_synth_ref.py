"""Test helper (not a test): restatements of gr_pfb_synthesis_filterbank_ccf and gr_pfb_interpolator_ccf
(gnuradio-core/src/lib/filter/gr_pfb_synthesis_filterbank_ccf.{h,cc}, gr_pfb_interpolator_ccf.{h,cc},
gri_fir_filter_with_buffer_XXX.cc.t).

- end_pad() / bank(): set_taps of both blocks (zeros at the END up to a multiple of M; branch f gets padded[f + q*M]).
- SynthRef: the synthesis block call by call, literally: bin filling with the `(in+i)[n]` offset, the forward DFT in
  float64 rounded to complex64 (the reference's is FFTW in float32; the DFT cannot be pinned bit for bit), the
  with_buffer branches: delay lines that live across calls, ONE float32 accumulator, oldest sample first, a product and
  a sum per term.
- closed_form(): every output of a fresh block over whole streams, in float64:
  out[n*M + f] = sum_q padded[f + q*M] * DFT_M(b_{n-q})[M-1-f],  b_m[i] = x_{s(i)}[m + i - tpf]  (zero before a stream
  starts, and b_m = 0 for m < 0: the delay lines start at zero).
- PfbInterpRef / whole_interp(): the interpolator through the CPU oracle's generic FIR (po.fir_ccf) per branch.
"""
import numpy as np

import resampler_ref as rr

f32 = np.float32
c64 = np.complex64


def end_pad(taps, M):
    taps = np.asarray(taps, dtype=f32)
    tpf = -(-len(taps) // M)
    return np.concatenate([taps, np.zeros(M * tpf - len(taps), dtype=f32)])


def bank(taps, M):
    """(tpf, h): h[f][q] = padded[f + q*M]"""
    p = end_pad(taps, M)
    tpf = len(p) // M
    return tpf, p.reshape(tpf, M).T.copy()


def stream_of_bin(M, numsigs):
    """.cc:139-156: the stream that fills bin i, or -1 for the zero bins around M/2"""
    ndiff = M - numsigs
    nhalf = -(-numsigs // 2)
    return [i if i < nhalf else (-1 if i < nhalf + ndiff else i - ndiff) for i in range(M)]


def in_range(M, tpf, numsigs):
    """bin M-1 reads item n + M - 1; the scheduler provides items up to n + tpf"""
    return numsigs == 1 or M - 1 <= tpf


def fill_bins(M, streams, nvec):
    """B[n, i] = streams[s(i)][n + i]"""
    B = np.zeros((nvec, M), dtype=c64)
    for i, s in enumerate(stream_of_bin(M, len(streams))):
        if s >= 0:
            B[:, i] = np.asarray(streams[s], dtype=c64)[i:i + nvec]
    return B


def branch_fir_literal(x, hrev, n):
    """out[k] = sum_j x[k + j] * hrev[j], j ascending (oldest sample first), one complex float32 accumulator, every
    product and sum a float32 operation (gri_fir_filter_with_buffer_ccf::filter, .cc.t:73-77)"""
    xr = np.ascontiguousarray(x.real, dtype=f32)
    xi = np.ascontiguousarray(x.imag, dtype=f32)
    ar = np.zeros(n, dtype=f32)
    ai = np.zeros(n, dtype=f32)
    for j in range(len(hrev)):
        h = f32(hrev[j])
        ar = ar + xr[j:j + n] * h
        ai = ai + xi[j:j + n] * h
    out = np.empty(n, dtype=c64)
    out.real = ar
    out.imag = ai
    return out


class SynthRef(object):
    """gr_pfb_synthesis_filterbank_ccf, call by call (every stream with history() - 1 = tpf items in front)"""

    def __init__(self, M, taps):
        self.M = M
        self._install(taps)
        self.new = None

    def _install(self, taps):
        self.tpf, self.h = bank(taps, self.M)
        self.delay = np.zeros((self.M, self.tpf - 1), dtype=c64)       # the tpf - 1 older samples of every delay line

    def history(self):
        return self.tpf + 1

    def set_taps(self, taps):
        self.new = taps

    def work(self, noutput_items, streams):
        M = self.M
        assert noutput_items % M == 0 and 1 <= len(streams) <= M
        if self.new is not None:
            self._install(self.new)
            self.new = None
            return np.zeros(0, dtype=c64)
        assert in_range(M, self.tpf, len(streams)), "the reference reads past its input here"
        nvec = noutput_items // M
        B = fill_bins(M, streams, nvec)
        V = np.fft.fft(B.astype(np.complex128), axis=1).astype(c64)     # forward, unnormalised
        out = np.zeros((nvec, M), dtype=c64)
        for f in range(M):
            x = np.concatenate([self.delay[f], V[:, M - 1 - f]])
            out[:, f] = branch_fir_literal(x, self.h[f][::-1], nvec)
            self.delay[f] = x[len(x) - (self.tpf - 1):]
        return out.reshape(-1)


def with_history(x, tpf):
    return np.concatenate([np.zeros(tpf, dtype=c64), np.asarray(x, dtype=c64)])


def whole_literal(M, taps, xs):
    """every output of a fresh SynthRef over whole streams xs (equal lengths N): N vectors"""
    ref = SynthRef(M, taps)
    return ref.work(len(xs[0]) * M, [with_history(x, ref.tpf) for x in xs])


def closed_form(M, taps, xs):
    """the closed form in float64 (complex128 result)"""
    tpf, h = bank(taps, M)
    N = len(xs[0])
    bufs = [np.concatenate([np.zeros(tpf), np.asarray(x, dtype=np.complex128), np.zeros(M)]) for x in xs]
    B = np.zeros((N, M), dtype=np.complex128)
    for i, s in enumerate(stream_of_bin(M, len(xs))):
        if s >= 0:
            B[:, i] = bufs[s][i:i + N]
    V = np.fft.fft(B, axis=1)
    U = np.concatenate([np.zeros((tpf - 1, M), dtype=np.complex128), V[:, ::-1]])      # U[tpf-1 + m, f] = V_m[M-1-f]
    out = np.zeros((N, M), dtype=np.complex128)
    for q in range(tpf):
        out += h[:, q].astype(np.float64)[None, :] * U[tpf - 1 - q:tpf - 1 - q + N, :]
    return out.reshape(-1)


class PfbInterpRef(rr.InterpRef):
    """gr_pfb_interpolator_ccf, call by call (input with history() - 1 = tpf - 1 items in front): the interpolating
    FIR's schedule over the end-padded bank, every branch through gr_fir_ccf_generic (po.fir_ccf)"""

    def __init__(self, po, R, taps):
        self.po, self.I = po, R
        self.nt, self.fwd = bank(taps, R)
        self.new = None

    def work(self, n, x):
        if self.new is not None:
            self.nt, self.fwd = bank(self.new, self.I)
            self.new = None
            return np.zeros(0, dtype=c64)
        return rr.InterpRef.work(self, n, x)


def whole_interp(po, R, taps, x):
    ref = PfbInterpRef(po, R, taps)
    buf = np.concatenate([np.zeros(ref.nt - 1, dtype=c64), np.asarray(x, dtype=c64)])
    return ref.work(R * len(x), buf)
