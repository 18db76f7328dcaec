"""Test helper (not a test): restatements of gr_rational_resampler_base_XXX and gr_interp_fir_filter_XXX
(gnuradio-core/src/lib/filter/gr_rational_resampler_base_XXX.{h,cc}.t, gr_interp_fir_filter_XXX.{h,cc}.t).

- front_pad() / bank(): set_taps (zeros in FRONT up to a multiple of I) and install_taps (filter n gets
  padded[n + k*I], forward order; gr_fir_XXX::set_taps reverses them inside).
- literal_walk() is the reference's ctr loop; closed_form() is the same schedule in closed form.
- RationalRef / InterpRef: the blocks call by call.  Their dot products come from the CPU oracle's generic FIRs
  (po.fir_ccf / fir_fff / fir_ccc), every filter at every offset of the call's input, then gathered by the schedule.
- whole_rational() / whole_interp(): every output of a fresh block over a whole stream.
"""
import numpy as np

f32 = np.float32


def front_pad(taps, I):
    taps = np.asarray(taps)
    n = len(taps) % I
    if n > 0:
        taps = np.concatenate([np.zeros(I - n, dtype=taps.dtype), taps])
    return taps


def bank(taps, I):
    """(nt, fwd): fwd[n] = the forward taps of filter n (install_taps, .cc.t:102-120)"""
    p = front_pad(taps, I)
    nt = len(p) // I
    idx = np.arange(I)[:, None] + np.arange(nt)[None, :] * I
    return nt, p[idx]


def literal_walk(I, D, c0, n):
    """general_work's loop (.cc.t:160-168) from ctr = c0: (filter, input offset) per output, ctr at the end and the
    items consumed"""
    ctr, pos = c0, 0
    fs, offs = [], []
    i = 0
    while i < n:
        fs.append(ctr)
        offs.append(pos)
        i += 1
        ctr += D
        while ctr >= I:
            ctr -= I
            pos += 1
    return np.array(fs, dtype=np.int64), np.array(offs, dtype=np.int64), ctr, pos


def closed_form(I, D, c0, n):
    """output o uses filter (c0 + o*D) % I at (c0 + o*D) // I; ctr and consumed after n outputs"""
    p = c0 + np.arange(n, dtype=np.int64) * D
    return p % I, p // I, (c0 + n * D) % I, (c0 + n * D) // I


def forecast(I, D, nt, n):
    """.cc.t:135-141: max(1, (int)((double)(n+1) * D / I) + history() - 1)"""
    return max(1, int(float(n + 1) * D / I) + nt - 1)


def _fir(po, taps_fwd, x, n):
    x = np.asarray(x)
    if np.iscomplexobj(np.asarray(taps_fwd)):
        return po.fir_ccc(taps_fwd, x, n)
    return po.fir_ccf(taps_fwd, x, n) if np.iscomplexobj(x) else po.fir_fff(taps_fwd, x, n)


def gather(po, fwd, x, filters, offsets):
    """out[k] = filter filters[k] at x[offsets[k]:], each filter run by the oracle over every offset it needs"""
    x = np.asarray(x)
    nt = fwd.shape[1]
    out = np.zeros(len(filters), dtype=np.complex64 if np.iscomplexobj(x) or np.iscomplexobj(fwd) else f32)
    for f in np.unique(filters):
        sel = filters == f
        hi = int(offsets[sel].max()) + 1
        y = _fir(po, fwd[f], x[:hi + nt - 1], hi)
        out[sel] = y[offsets[sel]]
    return out


class RationalRef(object):
    """gr_rational_resampler_base_XXX, call by call"""

    def __init__(self, po, I, D, taps):
        if I == 0 or D == 0:
            raise OverflowError("out of range")
        self.po, self.I, self.D = po, I, D
        self.d_ctr = 0
        self.nt, self.fwd = bank(taps, I)          # the constructor installs them
        self.new = None

    def history(self):
        return self.nt

    def forecast(self, n):
        return forecast(self.I, self.D, self.nt, n)

    def set_taps(self, taps):
        self.new = taps

    def general_work(self, n, x):
        if self.new is not None:
            self.nt, self.fwd = bank(self.new, self.I)
            self.new = None
            return np.zeros(0, dtype=np.asarray(x).dtype), 0
        fs, offs, ctr, consumed = literal_walk(self.I, self.D, self.d_ctr, n)
        assert len(x) >= (offs[-1] + self.nt if n else 0), "the call would read past its input"
        self.d_ctr = ctr
        return gather(self.po, self.fwd, x, fs, offs), consumed


class InterpRef(object):
    """gr_interp_fir_filter_XXX, call by call (input with history()-1 items in front)"""

    def __init__(self, po, I, taps):
        self.po, self.I = po, I
        self.nt, self.fwd = bank(taps, I)
        self.new = None

    def history(self):
        return self.nt

    def set_taps(self, taps):
        self.new = taps

    def work(self, n, x):
        if self.new is not None:
            self.nt, self.fwd = bank(self.new, self.I)
            self.new = None
            return np.zeros(0, dtype=np.asarray(x).dtype)
        ni = n // self.I
        fs = np.tile(np.arange(self.I), ni)
        offs = np.repeat(np.arange(ni), self.I)
        return gather(self.po, self.fwd, x, fs, offs)


def rational_nout(I, D, nt, N):
    """fresh outputs whose window fits a stream of N items: (o*D)//I + nt <= N"""
    return 0 if N < nt else ((N - nt) * I + I - 1) // D + 1


def whole_rational(po, I, D, taps, x):
    nt, fwd = bank(taps, I)
    n = rational_nout(I, D, nt, len(x))
    fs, offs, _, _ = closed_form(I, D, 0, n)
    return gather(po, fwd, x, fs, offs)


def whole_interp(po, I, taps, x):
    nt, fwd = bank(taps, I)
    x = np.asarray(x)
    buf = np.concatenate([np.zeros(nt - 1, dtype=x.dtype), x])
    return InterpRef(po, I, taps).work(I * len(x), buf)
