"""GPU tests of am_demod_cf / demod_10k0a3e_cf, the AM demodulator hier block (complex_to_mag -> add_const_ff(-1) ->
fir_filter_fff) as one handle on new items only.

GRHIP_MODE_GENERIC equals the reference's chain restated in optfir_ref.py (the double-sqrt magnitude, which
tests/test_am_demod_cpu.py pins to the reference's std::abs, a float add of -1, and the oracle's generic-order fir_fff
from a zero delay line) bit for bit, calls cut anywhere equal the single call, and the first ntaps - 1 outputs are
compared on their own: there the delay line's zeros show (a line of |0| - 1 = -1 would not pass).  The other modes are
held to the FIR family's FAST contract of include/grhip.h, 1e-5 of the output's peak, against the float64 FIR over
the CPU's float v; engine() says whether the fused kernel or the three steps ran.

With T = tile() and R = outputs_per_lane(): n_in in {1, T - 1, T, T + 1, 2 T + 3} and 256 R + R + 3 (an output count
that is no multiple of R or of 256 R), audio_decim in {1, 2, 5}, ntaps in {1, 2, 37, 83, max_taps(), max_taps() + 1},
three streams, calls cut at 1, 255 and T + 1 with an empty call in front of each piece.  The signal (optfir_ref.am_signal)
is a carrier of 1.0 with 50 % tone modulation and noise, a stretch at amplitude 30, one at 1e-3 and one of exact
zeros."""
import functools
import os

import numpy as np
import pytest

import optfir_ref as O

pytestmark = pytest.mark.gpu

TOL = 1e-5                          # FAST modes of the FIR family: include/grhip.h
DECIMS = (1, 2, 5)


def T(g):
    return g.am_demod_cf.tile()


def ntaps_set(g):
    return (1, 2, 37, 83, g.am_demod_cf.max_taps(), g.am_demod_cf.max_taps() + 1)


def sizes(g):
    t, r = T(g), g.am_demod_cf.outputs_per_lane()
    return (1, t - 1, t, t + 1, 2 * t + 3, 256 * r + r + 3)


def cuts(g):
    return (1, 255, T(g) + 1)


@functools.lru_cache(maxsize=None)
def stream(k, n):
    x = O.am_signal(5 + k, n)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def v_of(k, n):
    v = O.am_v(stream(k, n))
    v.setflags(write=False)
    return v


_REF = {}


def reference(po, k, n, D, ntaps):
    """(the generic-order FIR through the oracle, the float64 FIR) over stream k's v, once at the longest length; the
    outputs of a shorter call are a prefix"""
    key = (k, n, D, ntaps)
    if key not in _REF:
        taps = O.audio_taps(ntaps)
        _REF[key] = (O.am_fir(po, v_of(k, n), D, taps), O.am_fir64(v_of(k, n), D, taps))
    return _REF[key]


def make(g, D, ntaps, mode, streams=1):
    blk = g.am_demod_cf.from_taps(D, O.audio_taps(ntaps))
    blk.set_mode(mode)
    if streams != 1:
        blk.set_streams(streams)
    return blk


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(O.bits32(a), O.bits32(b))


def in_calls(blk, x, at, streams=1):
    """x ([streams][n]) cut at `at`, an empty call in front of every piece; returns [streams][outputs]"""
    x = x.reshape(streams, -1)
    n, D = x.shape[1], blk.audio_decim
    edges = [0] + [c for c in at if 0 < c < n] + [n]
    outs = []
    for a, b in zip(edges[:-1], edges[1:]):
        assert len(blk.work(x[:, :0])) == 0
        assert blk.produced(b - a) == O.am_outputs(b, D) - O.am_outputs(a, D)
        outs.append(blk.work(np.ascontiguousarray(x[:, a:b])).reshape(streams, -1))
    return np.concatenate(outs, axis=1)


def worst(got, want64):
    assert got.shape == want64.shape
    peak = float(np.max(np.abs(want64))) or 1.0
    return float(np.max(np.abs(got.astype(np.float64) - want64))) / peak if len(want64) else 0.0


@pytest.mark.parametrize("D", DECIMS)
def test_generic_is_the_reference_chain_bit_for_bit(gpu, po, D):
    g = gpu
    nmax = max(sizes(g))
    for ntaps in ntaps_set(g):
        want, _ = reference(po, 0, nmax, D, ntaps)
        for n_in in sizes(g):
            blk = make(g, D, ntaps, g.MODE_GENERIC)
            np_ = O.am_outputs(n_in, D)
            assert blk.engine() == 0 and blk.produced(n_in) == np_
            got = blk.work(stream(0, nmax)[:n_in])
            head = min(ntaps - 1, np_)
            assert same_bits(got[:head], want[:head]), ("the zero delay line", ntaps, n_in)
            assert same_bits(got, want[:np_]), (ntaps, n_in)
        blk = make(g, D, ntaps, g.MODE_GENERIC)
        got = in_calls(blk, stream(0, nmax), cuts(g))[0]
        assert same_bits(got, want), ("cut calls", ntaps)


@pytest.mark.parametrize("D", DECIMS)
def test_fused_kernel_is_within_the_fast_contract(gpu, po, D):
    g = gpu
    nmax = max(sizes(g))
    limit = g.am_demod_cf.max_taps()
    lines = []
    for ntaps in ntaps_set(g):
        _, want64 = reference(po, 0, nmax, D, ntaps)
        for n_in in sizes(g):
            blk = make(g, D, ntaps, g.MODE_FAST)
            assert blk.engine() == (1 if ntaps <= limit else 0), ntaps
            np_ = O.am_outputs(n_in, D)
            assert blk.produced(n_in) == np_
            got = blk.work(stream(0, nmax)[:n_in])
            assert got.shape == (np_,)
            # of the peak of this call's own outputs
            e = float(np.max(np.abs(got.astype(np.float64) - want64[:np_]))) / float(np.max(np.abs(want64[:np_])) or 1.0)
            lines.append("D %d ntaps %4d n_in %5d: %.3g of the peak" % (D, ntaps, n_in, e))
            print(lines[-1])
            head = min(ntaps - 1, np_)
            if head:
                eh = float(np.max(np.abs(got[:head].astype(np.float64) - want64[:head])))
                assert eh <= TOL * float(np.max(np.abs(want64[:np_]))), ("the zero delay line", ntaps, n_in, eh)
            assert e <= TOL, lines[-1]
        blk = make(g, D, ntaps, g.MODE_FAST)
        got = in_calls(blk, stream(0, nmax), cuts(g))[0]
        e = worst(got, want64)
        print("D %d ntaps %4d cut calls: %.3g of the peak" % (D, ntaps, e))
        assert e <= TOL, ("cut calls", ntaps, e)


@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_three_streams_and_cut_calls(gpu, po, mode):
    g = gpu
    n = 2 * T(g) + 3
    x = np.stack([stream(k, n) for k in range(3)])
    for D, ntaps in ((1, 83), (2, 37), (5, g.am_demod_cf.max_taps())):
        refs = [reference(po, k, n, D, ntaps) for k in range(3)]
        one = make(g, D, ntaps, getattr(g, mode), streams=3).work(x).reshape(3, -1)
        cut = in_calls(make(g, D, ntaps, getattr(g, mode), streams=3), x, cuts(g), streams=3)
        for k in range(3):
            if mode == "MODE_GENERIC":
                assert same_bits(one[k], refs[k][0]) and same_bits(cut[k], refs[k][0]), (D, ntaps, k)
            else:
                assert worst(one[k], refs[k][1]) <= TOL and worst(cut[k], refs[k][1]) <= TOL, (D, ntaps, k)
        # set_streams restarts every stream: the same input gives the same output again
        blk = make(g, D, ntaps, getattr(g, mode), streams=3)
        first = blk.work(x[:, :1000].copy())
        blk.set_streams(3)
        assert same_bits(blk.work(x[:, :1000].copy()), first)


def test_special_values_pass_through_v(gpu):
    """v is the same in every mode: with one tap of 1.0 the block's output IS v, infinities and NaNs included"""
    g = gpu
    fix = np.load(os.path.join(O.GOLDEN, "ref_complex_to_mag.npz"))
    x = np.ascontiguousarray(fix["pairs"]).view(np.float32).reshape(-1, 2).copy().view(np.complex64).reshape(-1)
    want = O.am_v(x)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = g.am_demod_cf.from_taps(1, np.ones(1, np.float32))
        blk.set_mode(mode)
        got = blk.work(x)
        assert np.all((O.bits32(got) == O.bits32(want)) | (np.isnan(got) & np.isnan(want)))


@pytest.mark.parametrize("ntaps", (3, 8, 13))
def test_an_infinite_sample_reaches_ntaps_outputs_and_no_more(gpu, ntaps):
    """the blocked step works in blocks of 8 taps: a filter that does not fill its last block must not let a sample
    that is not finite into outputs it does not reach"""
    g = gpu
    n, p = 600, 301
    x = stream(2, 2 * T(g) + 3)[:n].copy()
    x[p] = complex(np.inf, 1.0)
    x[p + 40] = complex(np.nan, 0.0)
    taps = O.audio_taps(ntaps)
    want = O.am_fir64(O.am_v(x), 1, taps)
    hit = np.zeros(n, bool)
    hit[p:p + ntaps] = hit[p + 40:p + 40 + ntaps] = True
    assert np.array_equal(~np.isfinite(want), hit)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = g.am_demod_cf.from_taps(1, taps)
        blk.set_mode(mode)
        got = blk.work(x)
        assert np.array_equal(~np.isfinite(got), hit), mode
        assert np.max(np.abs(got[~hit] - want[~hit])) <= TOL * np.max(np.abs(want[~hit])), mode


def test_demod_10k0a3e_cf_end_to_end(gpu, po):
    g = gpu
    rx = g.demod_10k0a3e_cf(16e3, 1)
    taps = g.optfir_low_pass(0.5, 16e3, 5000, 5500, 0.1, 60).astype(np.float32)
    assert len(rx.audio_taps) == 83 and same_bits(rx.audio_taps, taps) and rx.engine() == 1
    fix = np.load(os.path.join(O.GOLDEN, "ref_remez.npz"))
    assert O.bits64(g.optfir_low_pass(0.5, 16e3, 5000, 5500, 0.1, 60)).tolist() == fix["lp_am_taps"].tolist()
    n = T(g) + 77
    x, v = stream(1, 2 * T(g) + 3)[:n], v_of(1, 2 * T(g) + 3)[:n]
    got = rx.work(x)
    assert worst(got, O.am_fir64(v, 1, taps)) <= TOL
    rx = g.demod_10k0a3e_cf(16e3, 1)
    rx.set_mode(g.MODE_GENERIC)
    assert same_bits(rx.work(x), O.am_fir(po, v, 1, taps))
    am = g.am_demod_cf(16e3, 1, 5000, 5500)
    assert same_bits(am.audio_taps, taps)
