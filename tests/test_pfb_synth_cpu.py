"""CPU tests of the synthesis filterbank's and the PFB interpolator's restatements (tests/pfb_synth_ref.py): the literal
loop against the closed form, state across calls, what the bank computes (a tone per stream, the channeliser's inverse)
and the interpolator's tap layout.  No GPU involved."""
import numpy as np
import pytest

import pfb_synth_ref as sr
import resampler_ref as rr
from conftest import bits_equal

c64 = np.complex64


def _noise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(c64)


def _proto(wl, M, tpf):
    """low-pass prototype for M channels, pass band inside a channel, gain M"""
    return (wl.lowpass_taps(M * tpf, 0.8 / (2 * M), 1.0) * M).astype(np.float32)


@pytest.mark.parametrize("M", list(range(1, 17)) + [32])
def test_literal_equals_closed_form(M):
    rng = np.random.default_rng(100 + M)
    worst = 0.0
    ncases = 0
    for tpf in sorted({max(M - 1, 1), M, 5}):
        for k in (0, 1, M - 1):
            ntaps = M * tpf - k
            if ntaps <= 0 or -(-ntaps // M) != tpf:
                continue
            taps = rng.standard_normal(ntaps).astype(np.float32)
            for ns in sorted({1, max(1, M // 2), max(1, M - 1), M}):
                if not sr.in_range(M, tpf, ns):
                    continue
                xs = [_noise(rng, 150) for _ in range(ns)]
                a = sr.whole_literal(M, taps, xs)
                b = sr.closed_form(M, taps, xs)
                worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
                ncases += 1
    assert ncases >= 3
    print("M=%d: %d cases, worst %.3g of the peak" % (M, ncases, worst))
    assert worst < 1e-6


@pytest.mark.parametrize("M,tpf,ns", [(1, 4, 1), (4, 3, 4), (7, 9, 5), (8, 32, 8), (16, 15, 9), (32, 3, 1)])
def test_call_splits_equal_one_call(M, tpf, ns):
    rng = np.random.default_rng(7 * M + tpf)
    taps = rng.standard_normal(M * tpf - (M > 1)).astype(np.float32)
    N = 700
    xs = [_noise(rng, N) for _ in range(ns)]
    one = sr.whole_literal(M, taps, xs)
    ref = sr.SynthRef(M, taps)
    bufs = [sr.with_history(x, ref.tpf) for x in xs]
    outs, rd = [], 0
    while rd < N:
        n = int(min(N - rd, rng.integers(1, 200)))
        outs.append(ref.work(n * M, [b[rd:rd + n + ref.tpf] for b in bufs]))
        rd += n
    assert bits_equal(np.concatenate(outs), one)


def test_set_taps_clears_the_delay_lines():
    rng = np.random.default_rng(3)
    M = 4
    t1 = rng.standard_normal(M * 6).astype(np.float32)
    t2 = rng.standard_normal(M * 9 - 2).astype(np.float32)
    xs = [_noise(rng, 300) for _ in range(M)]
    ref = sr.SynthRef(M, t1)
    ref.work(100 * M, [sr.with_history(x, 6)[:106] for x in xs])
    assert ref.history() == 7
    ref.set_taps(t2)
    assert len(ref.work(40 * M, [sr.with_history(x, 6)[100:146] for x in xs])) == 0      # installs, produces nothing
    assert ref.history() == 10
    # from here it is a fresh block with the new taps over the items it is given
    seg = [np.concatenate([x[91:100], x[100:300]]) for x in xs]                           # tpf = 9 old items in front
    got = ref.work(200 * M, seg)
    fresh = sr.SynthRef(M, t2).work(200 * M, seg)
    assert bits_equal(got, fresh)


@pytest.mark.parametrize("M,k", [(8, 3), (8, 0), (8, 7), (5, 2), (16, 11)])
def test_dc_on_stream_k_is_a_tone_at_k_over_M(wl, M, k):
    taps = _proto(wl, M, 32)
    xs = [np.zeros(1500, dtype=c64) for _ in range(M)]
    xs[k][:] = 1
    y = sr.closed_form(M, taps, xs)[64 * M:]
    n = 1024 * M                                       # k/M of the output rate is bin 1024 k
    Y = np.abs(np.fft.fft(y[:n]))
    assert int(np.argmax(Y)) == 1024 * k


def test_synth_to_chan(wl, po):
    """gnuradio-examples/python/pfb/synth_to_chan.py: the bank's output through the channeliser with the same
    prototype: stream k's tone comes back in channel k and nowhere else above the prototype's stop band"""
    M, tpf, N = 8, 32, 4000
    taps = _proto(wl, M, tpf)
    fr = [0.01 * (k + 1) - 0.045 for k in range(M)]                  # inside a channel's pass band, all different
    xs = [np.exp(2j * np.pi * fr[k] * np.arange(N)).astype(c64) for k in range(M)]
    y = sr.closed_form(M, taps, xs).astype(c64)
    ch = po.PfbChannelizer(M, taps / M)
    ys = [np.concatenate([np.zeros(ch.taps_per_filter, dtype=c64), y[j::M]]) for j in range(M)]
    out, _ = ch.general_work(N - 1, ys)
    seg = out[1000:3000]
    w = np.hanning(len(seg))
    f = np.fft.fftfreq(len(seg))
    for c in range(M):
        F = np.abs(np.fft.fft(seg[:, c] * w)) / w.sum()
        peak = int(np.argmax(F))
        assert abs(f[peak] - fr[c]) < 1.0 / len(seg), (c, f[peak], fr[c])
        assert abs(F[peak] - 1.0) < 0.02
        # the other streams' tones: below the Hamming prototype's stop band (-53 dB; two filters in a row here)
        for k in range(M):
            if k != c:
                b = int(np.argmin(np.abs(f - fr[k])))
                assert F[b] < 10 ** (-50 / 20.0), (c, k, F[b])


@pytest.mark.parametrize("R,ntaps", [(1, 1), (3, 8), (4, 13), (5, 5), (8, 255)])
def test_interpolator_bank_pads_at_the_end(R, ntaps):
    taps = np.arange(1, ntaps + 1, dtype=np.float32)
    tpf, h = sr.bank(taps, R)
    assert tpf == -(-ntaps // R)
    p = sr.end_pad(taps, R)
    assert len(p) == R * tpf and np.array_equal(p[:ntaps], taps) and not p[ntaps:].any()
    for j in range(R):
        assert np.array_equal(h[j], p[j::R])
    fp = rr.front_pad(taps, R)
    if ntaps % R:
        assert not fp[:R - ntaps % R].any() and np.array_equal(fp[R - ntaps % R:], taps)     # gr_interp_fir_filter: in front
        assert not np.array_equal(fp, p)
    else:
        assert np.array_equal(fp, p)


def test_interpolator_restatement(po):
    rng = np.random.default_rng(5)
    R, taps = 3, rng.standard_normal(10).astype(np.float32)
    x = _noise(rng, 50)
    y = sr.whole_interp(po, R, taps, x)
    # out[n*R + j] = sum_k padded[j + k*R] x[n - k]
    p = sr.end_pad(taps, R).astype(np.float64)
    want = np.zeros(R * len(x), dtype=np.complex128)
    for n in range(len(x)):
        for j in range(R):
            want[n * R + j] = sum(p[j + k * R] * x[n - k] for k in range(len(p) // R) if n - k >= 0)
    assert np.abs(y - want).max() < 1e-5 * np.abs(want).max()
