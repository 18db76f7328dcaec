"""Test helper (not a test): restatements of gr_fractional_interpolator_ff / _cc
(gnuradio-core/src/lib/filter/gr_fractional_interpolator_ff.{h,cc}; the _cc files differ only in the item type) over
gri_mmse_fir_interpolator{,_cc} (filter/gri_mmse_fir_interpolator.cc:61-71).

- walk_step() / walk_schedule(): the walk of general_work (.cc:83-87) in the reference's arithmetic.  d_mu and d_mu_inc
  are floats, so `double s = d_mu + d_mu_inc` is a FLOAT sum widened afterwards; floor and the subtraction are in
  double, and s - f, the fraction of a float, narrows back to float exactly.  The float sum is the one place that
  rounds.  tests/golden/ref_fractional_interp.npz (the reference's own code, compiled) pins this.
- closed_form_ok() / closed_form_schedule(): T_k = A0 + k*F in units of 2^-24, ii_k = T_k >> 24, m_k = T_k mod 2^24,
  imu_k = round-half-even(m_k / 2^17), and when it equals the walk: mu and mu_inc multiples of a power of two g with
  1 + mu_inc <= 2^24 * g, so that every sum is a multiple of g below 2^24 * g and exact.  mu == 1 at the start is the
  same form with A0 = 2^24 except for output 0, which is filter 128 at offset 0.
- whole_stream_schedule(): fresh state, every output with ii_k + 8 <= N.
- eval_schedule(): the 8-tap dot products in gr_fir_XXX_generic's order (float32), or in float64 (f64=True).
- FractionalInterpolatorRef: general_work call by call with the product's input-shortfall rule (include/grhip.h);
  run_calls() drives it, or the product's block, the way a scheduler would.
"""
import os

import numpy as np

f32 = np.float32
NTAPS = 8
NSTEPS = 128
ONE24 = 1 << 24

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_BANK = None


def bank_reversed():
    """[129][8]: row imu multiplies in[ii .. ii + 8) (the taps as gr_fir stores them, reversed)"""
    global _BANK
    if _BANK is None:
        fwd = np.load(os.path.join(_GOLDEN, "ref_mmse_taps.npz"))["taps"].astype(f32)
        assert fwd.shape == (NSTEPS + 1, NTAPS)
        _BANK = np.ascontiguousarray(fwd[:, ::-1])
    return _BANK


def imu_of(mu):
    """int imu = (int) rint(mu * NSTEPS)   (float product, rint in double: round-half-even)"""
    return int(np.rint(np.float64(f32(mu) * f32(NSTEPS))))


def walk_step(mu, mu_inc):
    """(mu', incr) of .cc:83-87"""
    s = np.float64(f32(f32(mu) + f32(mu_inc)))           # float + float, then widened
    f = np.floor(s)
    return f32(s - f), int(f)


def forecast(noutput_items, mu_inc):
    """(int) ceil((noutput_items * d_mu_inc) + d_interp->ntaps()): int * float and + unsigned, both in float"""
    return int(np.ceil(np.float64(f32(f32(noutput_items) * f32(mu_inc)) + f32(NTAPS))))


def walk_schedule(phase, ratio, n_outputs=None, n_samples=None):
    """(ii, imu, mu) arrays of the outputs (mu the value each output is interpolated at), then (ii_end, mu_end);
    stops after n_outputs, or (n_samples) at the first output with ii + 8 > n_samples"""
    mu, inc, ii = f32(phase), f32(ratio), 0
    iis, imus, mus = [], [], []
    while True:
        if n_outputs is not None and len(iis) >= n_outputs:
            break
        if n_samples is not None and ii + NTAPS > n_samples:
            break
        iis.append(ii); imus.append(imu_of(mu)); mus.append(mu)
        mu, incr = walk_step(mu, inc)
        ii += incr
    return (np.array(iis, dtype=np.int64), np.array(imus, dtype=np.int64), np.array(mus, dtype=f32)), (ii, mu)


def _grid(v):
    """v * 2^24 as an int, or None"""
    s = float(f32(v)) * ONE24
    return int(s) if s >= 0 and s == np.floor(s) else None


def closed_form_ok(mu, mu_inc):
    """the walk from (mu, mu_inc) never rounds: both multiples of a power of two g, 1 + mu_inc <= 2^24 * g"""
    A0, F = _grid(mu), _grid(mu_inc)
    if A0 is None or F is None or F == 0 or A0 > ONE24:
        return False
    m = A0 | F
    low = m & -m
    return ONE24 + F <= low * ONE24


def closed_form_schedule(phase, ratio, n_outputs):
    """(ii, imu, mu) as walk_schedule gives them, from integers alone; valid where closed_form_ok()"""
    A0, F = _grid(phase), _grid(ratio)
    assert A0 is not None and F is not None, "not on the 2^-24 grid"
    k = np.arange(n_outputs, dtype=object)
    T = A0 + k * F                                   # Python integers: no overflow at any ratio
    ii = np.array([t >> 24 for t in T], dtype=np.int64)
    m = np.array([t & (ONE24 - 1) for t in T], dtype=np.int64)
    q = m >> 17
    imu = (m + 0xffff + (q & 1)) >> 17               # round-half-even of m / 2^17
    mu = (m.astype(np.float64) * 2.0 ** -24).astype(f32)
    if A0 == ONE24 and n_outputs > 0:                # mu == 1.0f: filter 128 at offset 0, not filter 0 at offset 1
        ii[0], imu[0], mu[0] = 0, NSTEPS, f32(1.0)
    return ii, imu, mu


def schedule(phase, ratio, n_outputs):
    """what the product does: the closed form where it holds, the walk elsewhere"""
    if closed_form_ok(phase, ratio):
        return closed_form_schedule(phase, ratio, n_outputs)
    return walk_schedule(phase, ratio, n_outputs=n_outputs)[0]


def whole_stream_schedule(phase, ratio, n_samples):
    """fresh state over a stream of n_samples items: every output with ii_k + 8 <= n_samples"""
    return walk_schedule(phase, ratio, n_samples=n_samples)[0]


def _parts(x):
    x = np.asarray(x)
    if np.iscomplexobj(x):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        return [x.real.astype(f32), x.imag.astype(f32)], True
    return [np.asarray(x, dtype=f32)], False


def _generic_dot(dt, X, nu):
    """gr_fir_XXX_generic::filter per row (gr_fir_XXX_generic.cc.t:28-78): nu accumulators from 0, then their sum"""
    acc = [np.zeros(dt.shape[0], dtype=f32) for _ in range(nu)]
    for i in range(0, NTAPS, nu):
        for q in range(nu):
            acc[q] = acc[q] + dt[:, i + q] * X[:, i + q]
    s = acc[0]
    for q in range(1, nu):
        s = s + acc[q]
    return s


def eval_schedule(buf, ii, imu, f64=False):
    """out_k = filters[imu_k]->filter(&buf[ii_k]) in the generic order (4 float accumulators for ff, 2 complex ones
    for cc: generate_gr_fir_XXX.py:59-64), or the same sums in float64 (f64=True) for a rounding-free yardstick"""
    ii = np.asarray(ii, dtype=np.int64)
    imu = np.asarray(imu, dtype=np.int64)
    parts, cplx = _parts(buf)
    if len(ii) == 0:
        return np.zeros(0, dtype=(np.complex128 if cplx else np.float64) if f64 else (np.complex64 if cplx else f32))
    gidx = ii[:, None] + np.arange(NTAPS)[None, :]
    dt = bank_reversed()[imu]
    res = []
    for p in parts:
        X = p[gidx]
        if f64:
            res.append((dt.astype(np.float64) * X).sum(axis=1))
        else:
            res.append(_generic_dot(dt, X, 2 if cplx else 4))
    if f64:
        return res[0] + 1j * res[1] if cplx else res[0]
    if cplx:
        out = np.empty(len(ii), dtype=np.complex64)
        out.real, out.imag = res[0], res[1]
        return out
    return res[0]


def whole_stream(phase, ratio, x, f64=False):
    ii, imu, _ = whole_stream_schedule(phase, ratio, len(x))
    return eval_schedule(x, ii, imu, f64=f64)


class FractionalInterpolatorRef(object):
    """gr_fractional_interpolator_{ff,cc}, call by call.  With ninput_items >= forecast(noutput_items) a call is the
    reference's; with less it produces the outputs with ii + 8 <= ninput_items, consumes at most ninput_items and
    carries the rest of ii (d_skip: 0 in the reference) into the next call."""

    def __init__(self, phase_shift, interp_ratio, complex_items=False):
        if not interp_ratio > 0:
            raise IndexError("interpolation ratio must be > 0")
        if phase_shift < 0 or phase_shift > 1:
            raise IndexError("phase shift ratio must be > 0 and < 1")
        self.d_mu = f32(phase_shift)
        self.d_mu_inc = f32(interp_ratio)
        self.d_skip = 0
        self.cplx = complex_items

    def mu(self):
        return float(self.d_mu)

    def interp_ratio(self):
        return float(self.d_mu_inc)

    def set_mu(self, mu):
        self.d_mu = f32(mu)

    def set_interp_ratio(self, r):
        self.d_mu_inc = f32(r)

    def history(self):
        return 1

    def forecast(self, noutput_items):
        return forecast(noutput_items, self.d_mu_inc)

    def schedule_call(self, noutput_items, ninput_items):
        """[(ii, imu)] of the outputs, consumed"""
        ii = self.d_skip
        sched = []
        while len(sched) < noutput_items and ii + NTAPS <= ninput_items:
            sched.append((ii, imu_of(self.d_mu)))
            self.d_mu, incr = walk_step(self.d_mu, self.d_mu_inc)
            ii += incr
        consumed = min(ii, ninput_items)
        self.d_skip = ii - consumed
        return sched, consumed

    def general_work(self, noutput_items, in_items):
        sched, consumed = self.schedule_call(noutput_items, len(in_items))
        if not sched:
            return np.zeros(0, dtype=np.complex64 if self.cplx else f32), consumed
        ii, imu = zip(*sched)
        return eval_schedule(in_items, ii, imu), consumed


def run_calls(blk, x, sizes):
    """drive a block (FractionalInterpolatorRef or the product's) the way a scheduler would: calls of
    (noutput, ninput-cap) from `sizes` (cycled; a cap of None = all the input left, "forecast" = what the block's
    forecast asks for, "forecast-1" = one item less), until a call with all the input left makes no progress.
    Returns the concatenated output and the items consumed in all."""
    x = np.asarray(x)
    rd = 0
    outs = []
    k = 0
    idle = 0
    while True:
        nout, ncap = sizes[k % len(sizes)]
        k += 1
        avail = len(x) - rd
        if ncap == "forecast":
            ncap = blk.forecast(nout)
        elif ncap == "forecast-1":
            ncap = blk.forecast(nout) - 1
        nin = avail if ncap is None else min(avail, ncap)
        out, consumed = blk.general_work(nout, x[rd:rd + nin])
        outs.append(np.asarray(out))
        rd += consumed
        if len(out) or consumed:
            idle = 0
        elif nin == avail:
            idle += 1
            if idle >= 3:
                break
    return (np.concatenate(outs) if outs else np.zeros(0, dtype=x.dtype)), rd
