"""Test helper (not a test): restatements of gr_pfb_arb_resampler_ccf / _fff
(gnuradio-core/src/lib/filter/gr_pfb_arb_resampler_ccf.{h,cc}; the _fff files differ only in the item type).

- ArbResamplerRef: general_work line by line, call by call, the state in np.float32 scalars named as in the
  reference.  Its dot products follow gr_fir_XXX_generic.cc.t (2 accumulators for a complex accumulator, 4 for a
  float one: generate_gr_fir_XXX.py:59-64), vectorised over the outputs of a call.
- whole_stream(): fresh state, the tpf history zeros in front, every output with count_k < N; the dot products
  come from the CPU oracle's FIRs (po.fir_ccf / po.fir_fff: forward taps, reversed inside as gr_fir::set_taps
  does), each of the R filters at every offset, then gathered by the schedule.
- closed_form_schedule() / walk_schedule(): the index schedule (count_k, j_k, acc_k) two ways.
"""
import numpy as np

f32 = np.float32
MASK23 = (1 << 23) - 1


def rate_params(R, rate):
    """set_rate (.h:166-170): d_dec_rate = (unsigned)floor(d_int_rate/rate), d_flt_rate = d_int_rate/rate - d_dec_rate,
    in float (an unsigned over a float is a float division)"""
    x = f32(R) / f32(rate)
    D = int(np.floor(x))
    return D, f32(x - f32(D))


def banks(taps, R):
    """create_diff_taps (.cc:126-139) and create_taps (.cc:93-124): (tpf, fwd, dfwd), fwd[i] = the taps filter i is
    given (forward order: taps[i + t*R]); gr_fir_XXX::set_taps stores them reversed"""
    taps = np.asarray(taps, dtype=f32)
    ntaps = len(taps)
    tpf = int(np.ceil(float(ntaps) / float(R)))
    diff = np.empty(ntaps, dtype=f32)
    diff[:-1] = taps[1:] - taps[:-1]
    diff[-1] = diff[-2]
    proto = np.zeros(R * tpf, dtype=f32)
    dproto = np.zeros(R * tpf, dtype=f32)
    proto[:ntaps] = taps
    dproto[:ntaps] = diff
    idx = np.arange(R)[:, None] + np.arange(tpf)[None, :] * R
    return tpf, proto[idx], dproto[idx]


def _parts(x):
    x = np.asarray(x)
    if np.iscomplexobj(x):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        return [x.real.astype(f32), x.imag.astype(f32)], True
    return [np.asarray(x, dtype=f32)], False


def _generic_dot(dt, X):
    """gr_fir_XXX_generic::filter per row: dt (n, ntaps) reversed taps, X (n, ntaps) float32 inputs (one component)"""
    ntaps = dt.shape[1]
    nu = 2 if _generic_dot.complex_acc else 4
    acc = [np.zeros(dt.shape[0], dtype=f32) for _ in range(nu)]
    n = (ntaps // nu) * nu
    for i in range(0, n, nu):
        for q in range(nu):
            acc[q] = acc[q] + dt[:, i + q] * X[:, i + q]
    for i in range(n, ntaps):
        acc[0] = acc[0] + dt[:, i] * X[:, i]
    s = acc[0]
    for q in range(1, nu):
        s = s + acc[q]
    return s


_generic_dot.complex_acc = True


def eval_schedule(fwd, dfwd, buf, counts, js, accs, f64=False):
    """out_k = o0 + o1*acc with o0/o1 the generic-order dot products of filter j_k at buf[count_k:] (float32), or
    the same in float64 (f64=True) for a rounding-free yardstick"""
    tpf = fwd.shape[1]
    counts = np.asarray(counts, dtype=np.int64)
    js = np.asarray(js, dtype=np.int64)
    accs = np.asarray(accs, dtype=f32)
    parts, cplx = _parts(buf)
    if len(counts) == 0:
        return np.zeros(0, dtype=np.complex64 if cplx else f32)
    gidx = counts[:, None] + np.arange(tpf)[None, :]
    dt = fwd[js][:, ::-1]
    ddt = dfwd[js][:, ::-1]
    res = []
    for p in parts:
        X = p[gidx]
        if f64:
            o0 = (dt.astype(np.float64) * X).sum(axis=1)
            o1 = (ddt.astype(np.float64) * X).sum(axis=1)
            res.append(o0 + o1 * accs.astype(np.float64))
        else:
            _generic_dot.complex_acc = cplx
            o0 = _generic_dot(dt, X)
            o1 = _generic_dot(ddt, X)
            res.append(o0 + o1 * accs)
    if f64:
        return res[0] + 1j * res[1] if cplx else res[0]
    if cplx:
        out = np.empty(len(counts), dtype=np.complex64)
        out.real, out.imag = res[0], res[1]
        return out
    return res[0]


class ArbResamplerRef(object):
    """gr_pfb_arb_resampler_{ccf,fff}, call by call"""

    def __init__(self, rate, taps, filter_size=32, complex_items=True):
        self.d_int_rate = int(filter_size)
        self.set_rate(rate)
        self.d_acc = f32(0.0)
        self.d_last_filter = 0
        self.d_start_index = 0
        self.d_taps_per_filter, self.fwd, self.dfwd = banks(taps, self.d_int_rate)
        self.d_updated = True                     # create_taps (.cc:121)
        self.cplx = complex_items

    def set_rate(self, rate):
        self.d_dec_rate, self.d_flt_rate = rate_params(self.d_int_rate, rate)

    def history(self):
        return self.d_taps_per_filter + 1

    def forecast(self, noutput_items):
        return noutput_items + self.history() - 1

    def schedule_call(self, noutput_items, ninput_items):
        """the control flow of general_work (.cc:158-209): [(count, j, acc)] of the outputs, consumed"""
        if self.d_updated:
            self.d_updated = False
            return [], 0
        R = self.d_int_rate
        i = 0
        count = self.d_start_index
        j = self.d_last_filter
        sched = []
        max_input = ninput_items - self.d_taps_per_filter
        while i < noutput_items and count < max_input:
            while j < R and i < noutput_items:
                sched.append((count, j, self.d_acc))
                i += 1
                self.d_acc = f32(self.d_acc + self.d_flt_rate)
                j += self.d_dec_rate + int(np.floor(self.d_acc))
                self.d_acc = f32(np.fmod(self.d_acc, f32(1.0)))
            if i < noutput_items:
                ss = f32(j // R)                   # float ss = (int)(j / d_int_rate)
                count = int(f32(count) + ss)       # count += ss (through a float)
                j = j % R
        self.d_last_filter = j
        self.d_start_index = max(0, count - ninput_items)
        return sched, min(count, ninput_items)

    def general_work(self, noutput_items, in_items):
        """(out, consumed); in_items carries the history in front"""
        sched, consumed = self.schedule_call(noutput_items, len(in_items))
        if not sched:
            return np.zeros(0, dtype=np.complex64 if self.cplx else f32), consumed
        c, j, a = zip(*sched)
        return eval_schedule(self.fwd, self.dfwd, in_items, c, j, a), consumed


def run_calls(blk, x, sizes, rng=None):
    """drive a block (ArbResamplerRef or the product's) the way a scheduler would: the history zeros in front,
    calls of (noutput, ninput-cap) from `sizes` (cycled), until a call with all the input left makes no progress.
    Returns the concatenated output."""
    x = np.asarray(x)
    buf = np.concatenate([np.zeros(blk.history() - 1, dtype=x.dtype), x])
    rd = 0
    outs = []
    k = 0
    idle = 0
    while True:
        nout, ncap = sizes[k % len(sizes)]
        k += 1
        avail = len(buf) - rd
        nin = avail if ncap is None else min(avail, ncap)
        out, consumed = blk.general_work(nout, buf[rd:rd + nin])
        outs.append(np.asarray(out))
        rd += consumed
        if len(out) == 0 and consumed == 0 and nin == avail:
            idle += 1
            if idle >= 3:
                break
        else:
            idle = 0
    return np.concatenate(outs) if outs else np.zeros(0, dtype=x.dtype)


def walk_schedule(R, rate, n_outputs=None, n_samples=None):
    """fresh-state walk of the reference's float32 arithmetic: (count, j, acc) arrays, positions exact; stops after
    n_outputs, or (n_samples) once count_k >= n_samples"""
    D, f = rate_params(R, rate)
    count, j, acc = 0, 0, f32(0.0)
    cs, js, accs = [], [], []
    while True:
        if n_outputs is not None and len(cs) >= n_outputs:
            break
        if j >= R:
            count += j // R
            j %= R
        if n_samples is not None and count >= n_samples:
            break
        cs.append(count); js.append(j); accs.append(acc)
        acc = f32(acc + f)
        j += D + int(np.floor(acc))
        acc = f32(np.fmod(acc, f32(1.0)))
    return np.array(cs, dtype=np.int64), np.array(js, dtype=np.int64), np.array(accs, dtype=f32)


def closed_form_schedule(R, rate, n_outputs, c0=0, j0=0, acc0=0.0):
    """T_k = A0 + k*F, pos_k = j0 + k*D + (T_k >> 23), count_k = c0 + pos_k // R, j_k = pos_k % R,
    acc_k = (T_k & (2^23-1)) * 2^-23; exact when f and acc0 are multiples of 2^-23 (rate <= R from fresh state)"""
    D, f = rate_params(R, rate)
    F = int(np.float64(f) * 2 ** 23)
    A0 = int(np.float64(acc0) * 2 ** 23)
    assert F == np.float64(f) * 2 ** 23 and A0 == np.float64(acc0) * 2 ** 23, "not on the 2^-23 grid"
    k = np.arange(n_outputs, dtype=np.int64)
    T = A0 + k * F
    pos = j0 + k * D + (T >> 23)
    return c0 + pos // R, pos % R, ((T & MASK23).astype(np.float64) * 2.0 ** -23).astype(f32)


def whole_stream_schedule(R, rate, n_samples):
    return walk_schedule(R, rate, n_samples=n_samples)


def whole_stream(po, rate, taps, R, x):
    """every output of a fresh block over x, dot products from the oracle's FIRs (generic order)"""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    tpf, fwd, dfwd = banks(taps, R)
    N = len(x)
    counts, js, accs = whole_stream_schedule(R, rate, N)
    xs = np.concatenate([np.zeros(tpf, dtype=x.dtype), x])
    fir = po.fir_ccf if cplx else po.fir_fff
    Y = np.stack([fir(fwd[i], xs, N) for i in range(R)])
    dY = np.stack([fir(dfwd[i], xs, N) for i in range(R)])
    o0 = Y[js, counts]
    o1 = dY[js, counts]
    if cplx:
        out = np.empty(len(counts), dtype=np.complex64)
        out.real = o0.real + o1.real * accs
        out.imag = o0.imag + o1.imag * accs
        return out
    return (o0 + o1 * accs).astype(f32)
