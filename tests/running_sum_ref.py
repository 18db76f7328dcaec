"""numpy restatements of gr_dc_blocker_ff / _cc (filter/gr_dc_blocker_ff.cc:41-53, 105-138), gr_moving_average_XX
(gengen/gr_moving_average_XX.cc.t:64-93) and gr_integrate_XX (gengen/gr_integrate_XX.cc.t:52-67).

The float32 forms keep the reference's order of operations.  They lean on np.cumsum(dtype=float32) being strictly
sequential (out[i] = out[i-1] + a[i], every step rounded to float32); test_running_sum_cpu.py checks that against a
Python loop.  Complex streams are two float planes: every operation of the three blocks acts on the parts alone,
except moving_average_cc's final product with its complex scale.

The float64 forms are the same difference equations in double: what the filters compute, without the float
recurrence's accumulated rounding.  FAST mode is compared with these.
"""
import numpy as np


def _seq_cumsum(first, terms, dt):
    """first + terms[0] + terms[1] ... in order, every partial sum rounded to dt; returns the partial sums"""
    a = np.concatenate([np.asarray([first], dtype=dt), np.asarray(terms, dtype=dt)])
    return np.cumsum(a, dtype=dt)[1:]


class _Averager(object):
    """moving_averager_f: y = (x - x[n-D]) + y_prev, returned as y / (float)D"""

    def __init__(self, D, dt):
        self.D, self.dt = D, dt
        self.hist = np.zeros(D, dtype=dt)       # the last D inputs: d_delay_line (D - 1) and d_out_d1
        self.y = dt(0)

    def filter(self, x):
        if len(x) == 0:
            return x.copy()
        ext = np.concatenate([self.hist, x])
        d = (ext[self.D:] - ext[:-self.D]).astype(self.dt)
        ys = _seq_cumsum(self.y, d, self.dt)
        self.y = ys[-1]
        self.hist = ext[-self.D:]
        return (ys / self.dt(self.D)).astype(self.dt)


class _DcPlane(object):
    def __init__(self, D, long_form, dt):
        self.gd = (2 * D - 2) if long_form else (D - 1)
        self.ma = [_Averager(D, dt) for _ in range(4 if long_form else 2)]
        self.xh = np.zeros(self.gd, dtype=dt)   # delayed_sig() and, long form, the block's own delay line
        self.dt = dt

    def work(self, x):
        x = np.asarray(x, dtype=self.dt)
        y = x
        for m in self.ma:
            y = m.filter(y)
        ext = np.concatenate([self.xh, x])
        delayed = ext[:len(x)]
        self.xh = ext[len(x):]
        return (delayed - y).astype(self.dt)


class DcBlocker(object):
    """gr_dc_blocker_ff / _cc with its state; dt = np.float32 (the reference) or np.float64 (the filter)"""

    def __init__(self, D=32, long_form=True, complex_=False, dt=np.float32):
        if D < 1:
            raise ValueError("D must be at least 1")
        self.planes = [_DcPlane(D, long_form, dt) for _ in range(2 if complex_ else 1)]
        self.complex_ = complex_
        self.gd = self.planes[0].gd

    def get_group_delay(self):
        return self.gd

    def work(self, x):
        x = np.asarray(x)
        if not self.complex_:
            return self.planes[0].work(x)
        re, im = self.planes[0].work(x.real), self.planes[1].work(x.imag)
        return re + 1j * im if re.dtype == np.float64 else (re + 1j * im).astype(np.complex64)


def dc_blocker_taps(D, long_form):
    """the FIR the block is in exact arithmetic: delta at the group delay minus the D-box convolved 2 or 4 times"""
    box = np.ones(D) / D
    h = box
    for _ in range(3 if long_form else 1):
        h = np.convolve(h, box)
    t = -h
    t[(2 * D - 2) if long_form else (D - 1)] += 1.0
    return t


_INT = {"ss": (np.int16, 16), "ii": (np.int32, 32)}


def _wrap(a, bits):
    a = np.asarray(a, dtype=np.int64) & ((1 << bits) - 1)
    return np.where(a >= (1 << (bits - 1)), a - (1 << bits), a)


def moving_average_work(kind, x, length, scale, noutput_items, max_iter=4096):
    """ONE reference work call: x holds the history (length - 1 items) and then the new items.  Returns the
    min(noutput_items, max_iter) outputs."""
    n = min(noutput_items, max_iter)
    x = np.asarray(x)[:n + length - 1]
    if kind in _INT:
        dt, bits = _INT[kind]
        c = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
        s = _wrap(c[length:length + n] - c[:n], bits)           # wrapping sums are exact in any order
        return _wrap(s * int(scale), bits).astype(dt)
    planes = [x.real, x.imag] if kind == "cc" else [x]
    sums = []
    for p in planes:
        p = np.asarray(p, dtype=np.float32)
        terms = np.empty(length - 1 + 2 * n, dtype=np.float32)
        terms[:length - 1] = p[:length - 1]
        terms[length - 1::2] = p[length - 1:length - 1 + n]     # sum += in[i + length - 1]
        terms[length::2] = -p[:n]                               # sum -= in[i]
        ps = _seq_cumsum(np.float32(0), terms, np.float32)
        sums.append(ps[length - 1::2][:n])
    if kind == "ff":
        return (sums[0] * np.float32(scale)).astype(np.float32)
    z = np.complex64(scale)
    cr, ci = np.float32(z.real), np.float32(z.imag)
    sr, si = sums
    re = (sr * cr).astype(np.float32) - (si * ci).astype(np.float32)
    im = (sr * ci).astype(np.float32) + (si * cr).astype(np.float32)
    return (re.astype(np.float32) + 1j * im.astype(np.float32)).astype(np.complex64)


def moving_average_calls(kind, x, length, scale, n, max_iter=4096):
    """the chunking the device entry defines: successive work calls of exactly max_iter outputs, the last one shorter"""
    out = [moving_average_work(kind, x[o:], length, scale, min(max_iter, n - o), max_iter) for o in range(0, n, max_iter)]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.asarray(x).dtype)


def moving_average_f64(x, length, scale, n):
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    return np.array([x[i:i + length].sum() for i in range(n)]) * scale if n * length <= 1 << 22 else \
        np.convolve(x[:n + length - 1], np.ones(length), "valid") * scale


def integrate(kind, x, decim, n):
    x = np.asarray(x)[:n * decim].reshape(n, decim)
    if kind in _INT:
        dt, bits = _INT[kind]
        return _wrap(x.astype(np.int64).sum(axis=1), bits).astype(dt)
    planes = [x.real, x.imag] if kind == "cc" else [x]
    outs = []
    for p in planes:
        a = np.concatenate([np.zeros((n, 1), dtype=np.float32), np.asarray(p, dtype=np.float32)], axis=1)
        outs.append(np.cumsum(a, axis=1, dtype=np.float32)[:, -1])
    return outs[0] if kind == "ff" else (outs[0] + 1j * outs[1]).astype(np.complex64)


def integrate_f64(x, decim, n):
    x = np.asarray(x)[:n * decim].reshape(n, decim)
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64).sum(axis=1)
