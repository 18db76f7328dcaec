"""GPU tests of fm_demod_cf / nbfm_rx, the FM demodulator hier block (quadrature_demod_cf -> fm_deemph ->
fir_filter_fff) as one handle on new items only.

GRHIP_MODE_GENERIC equals the reference's chain restated in iir_ref.py (the oracle's quadrature demodulator and
fir_fff around the restatement of iir_filter_ffd, which tests/test_iir_cpu.py pins to the reference's own code) bit for
bit, and calls cut anywhere equal the single call.  The other modes are held to the FIR family's FAST contract of
include/grhip.h, 1e-5 of the output's peak, against the float64 chain over the library's own quadrature_demod_cf
output (float64 IIR -> float32 -> float64 FIR); engine() says whether the fused kernel or the three blocks ran.

With T = tile(): n_in in {1, T - 1, T, T + 1, 2 T + 3}, audio_decim in {1, 4, 5}, ntaps in {1, 2, 37, 150}, three
streams, calls cut at 1, 255 and T + 1 with an empty call between, de-emphasis at 32 kHz, at 320 kHz and none."""
import functools
import math

import numpy as np
import pytest

import iir_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5                          # FAST modes of the FIR family: include/grhip.h, tests/test_gpu_fir.py
DEVIATION = 5e3
DEEMPH = {"32k": 32e3, "320k": 320e3, "none": None}
DECIMS = (1, 4, 5)
NTAPS = (1, 2, 37, 150)


def T(g):
    return g.fm_demod_cf.tile()


def sizes(g):
    t = T(g)
    return (1, t - 1, t, t + 1, 2 * t + 3)


def rate_of(which):
    return DEEMPH[which] or 32e3


def gain_of(which):
    return float(np.float32(rate_of(which) / (2 * math.pi * DEVIATION)))


def audio_taps(ntaps):
    """a windowed low-pass of the given length with a little asymmetry, so that a reversed tap order would show"""
    n = np.arange(ntaps)
    h = np.sinc(0.2 * (n - (ntaps - 1) / 2.0)) * np.hamming(ntaps) if ntaps > 2 else np.array([0.75, 0.25][:ntaps])
    h = h * (1.0 + 0.01 * n / max(ntaps, 1))
    return (h / h.sum()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def stream(k, n):
    x = R.fm_signal(11 + k, n)
    x.setflags(write=False)
    return x


_CHAIN = {}


def chain(po, k, which, n):
    """(q, y) of the reference's first two blocks over stream k, computed once at the longest length"""
    key = (k, which)
    if key not in _CHAIN:
        deemph = None if DEEMPH[which] is None else R.deemph_taps(DEEMPH[which])
        _CHAIN[key] = R.fm_deemphasised(po, stream(k, n), gain_of(which), deemph)
    return _CHAIN[key]


def make(g, which, D, taps, mode, streams=1):
    blk = g.fm_demod_cf(rate_of(which), D, DEVIATION, taps, tau=75e-6 if DEEMPH[which] else None)
    blk.set_mode(mode)
    if streams != 1:
        blk.set_streams(streams)
    return blk


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


def in_calls(blk, x, cuts):
    """x cut at `cuts`, an empty call in front of every piece"""
    edges = [0] + [c for c in cuts if 0 < c < len(x)] + [len(x)]
    outs = []
    for a, b in zip(edges[:-1], edges[1:]):
        assert len(blk.work(x[:0])) == 0
        assert blk.produced(b - a) == R.fm_outputs(b, blk.audio_decim) - R.fm_outputs(a, blk.audio_decim)
        outs.append(blk.work(x[a:b]))
    return np.concatenate(outs)


def deemph64(q, deemph):
    """the float64 IIR over the demodulator output q, narrowed to float32 (a prefix of it is the prefix's result)"""
    return q if deemph is None else R.serial(q, *deemph)[0]


def close(got, y, D, taps, n_in):
    """the error against the float64 FIR over y = deemph64(the library's demodulator output), as a part of the peak"""
    want = R.fm_fir64(y, D, taps, n_in)
    assert got.shape == want.shape
    peak = float(np.max(np.abs(want))) or 1.0
    err = float(np.max(np.abs(got.astype(np.float64) - want))) / peak if len(want) else 0.0
    return err


@pytest.mark.parametrize("ntaps", NTAPS)
@pytest.mark.parametrize("D", DECIMS)
def test_generic_is_the_reference_chain_bit_for_bit(gpu, po, D, ntaps):
    g = gpu
    taps = audio_taps(ntaps)
    nmax = sizes(g)[-1]
    for which in DEEMPH:
        _, y = chain(po, 0, which, nmax)
        for n_in in sizes(g):
            blk = make(g, which, D, taps, g.MODE_GENERIC)
            assert blk.engine() == 0 and blk.produced(n_in) == R.fm_outputs(n_in, D)
            got = blk.work(stream(0, nmax)[:n_in])
            assert same_bits(got, R.fm_fir(po, y, D, taps, n_in)), (which, n_in)
        # cut calls, an empty call between: the same outputs as one call
        blk = make(g, which, D, taps, g.MODE_GENERIC)
        got = in_calls(blk, stream(0, nmax), (1, 255, T(g) + 1))
        assert same_bits(got, R.fm_fir(po, y, D, taps)), which


@pytest.mark.parametrize("ntaps", NTAPS)
@pytest.mark.parametrize("D", DECIMS)
def test_fused_kernel_is_within_the_fast_contract(gpu, D, ntaps):
    g = gpu
    taps = audio_taps(ntaps)
    nmax = sizes(g)[-1]
    lines = []
    for which in DEEMPH:
        x = stream(0, nmax)
        # the library's own demodulator output: quadrature_demod_cf has one form, whatever the mode
        q = g.quadrature_demod_cf(gain_of(which)).work(nmax, np.concatenate([np.zeros(1, np.complex64), x]))
        y = deemph64(q, None if DEEMPH[which] is None else R.deemph_taps(DEEMPH[which]))
        for n_in in sizes(g):
            blk = make(g, which, D, taps, g.MODE_FAST)
            assert blk.engine() == 1
            err = close(blk.work(x[:n_in]), y, D, taps, n_in)
            lines.append("D %d ntaps %d %s n_in %d: %.3g of the peak" % (D, ntaps, which, n_in, err))
            assert err <= TOL, lines[-1]
        blk = make(g, which, D, taps, g.MODE_FAST)
        err = close(in_calls(blk, x, (1, 255, T(g) + 1)), y, D, taps, nmax)
        lines.append("D %d ntaps %d %s cut calls: %.3g of the peak" % (D, ntaps, which, err))
        assert err <= TOL, lines[-1]
    print("\n".join(lines))


@pytest.mark.parametrize("mode_name", ("GENERIC", "FAST"))
def test_three_streams(gpu, po, mode_name):
    g = gpu
    D, taps = 4, audio_taps(37)
    n = T(g) + 1
    x = np.concatenate([stream(k, 2 * T(g) + 3)[:n] for k in range(3)])
    for which in ("32k", "none"):
        blk = make(g, which, D, taps, getattr(g, "MODE_" + mode_name), streams=3)
        # two calls: [3][255] and [3][n - 255]
        a = blk.work(np.concatenate([stream(k, 2 * T(g) + 3)[:255] for k in range(3)]), 255).reshape(3, -1)
        b = blk.work(np.concatenate([stream(k, 2 * T(g) + 3)[255:n] for k in range(3)]), n - 255).reshape(3, -1)
        got = np.concatenate([a, b], axis=1)
        assert got.shape == (3, R.fm_outputs(n, D))
        for k in range(3):
            # the oracle's demodulator equals the library's bit for bit (tests/test_gpu_fir.py), so y serves both
            _, y = chain(po, k, which, 2 * T(g) + 3)
            if mode_name == "GENERIC":
                assert same_bits(np.ascontiguousarray(got[k]), R.fm_fir(po, y, D, taps, n)), (which, k)
            else:
                assert close(np.ascontiguousarray(got[k]), y, D, taps, n) <= TOL, (which, k)
        blk.set_streams(3)                                              # restarts every stream
        got = blk.work(x, n).reshape(3, -1)
        for k in range(3):
            _, y = chain(po, k, which, 2 * T(g) + 3)
            assert close(np.ascontiguousarray(got[k]), y, D, taps, n) <= TOL, (which, k)


def test_shapes_the_fused_kernel_does_not_take(gpu):
    """a pole too close to the circle (W0 > T / 8), a biquad, and more than 1025 audio taps: engine() == 0, the three
    blocks in a row, the same contract"""
    g = gpu
    lib = g.lib()
    import ctypes as C
    n_in = 2 * T(g) + 3
    x = stream(0, n_in)
    k = gain_of("32k")
    q = g.quadrature_demod_cf(k).work(n_in, np.concatenate([np.zeros(1, np.complex64), x]))
    taps = audio_taps(37)
    cases = {"slow pole": ([1e-4, 0.0], [1.0, 0.9999]), "biquad": R.TAP_SETS["biquad"]}
    for name, (ff, fb) in cases.items():
        h = C.c_void_p(0)
        f, b = np.array(ff, np.float64), np.array(fb, np.float64)
        assert lib.grhip_fm_demod_cf_create(C.byref(h), k, f.ctypes.data, len(f), b.ctypes.data, len(b), 4, taps.ctypes.data,
                                            len(taps), 0) == 0
        try:
            assert lib.grhip_fm_demod_cf_set_mode(h, g.MODE_FAST) == 0
            assert lib.grhip_fm_demod_cf_engine(h) == 0, name
            np_ = lib.grhip_fm_demod_cf_produced(h, n_in)
            out = np.zeros(np_, np.float32)
            got = C.c_int(0)
            assert lib.grhip_fm_demod_cf_work(h, n_in, x.ctypes.data, out.ctypes.data, C.byref(got)) == 0
            assert got.value == np_ == R.fm_outputs(n_in, 4)
            assert close(out, deemph64(q, (ff, fb)), 4, taps, n_in) <= TOL, name
        finally:
            lib.grhip_fm_demod_cf_destroy(h)
    long_taps = audio_taps(1100)
    blk = g.fm_demod_cf(32e3, 4, DEVIATION, long_taps)
    assert blk.engine() == 0
    y = deemph64(q, R.deemph_taps(32e3))
    assert close(blk.work(x), y, 4, long_taps, n_in) <= TOL
    blk = g.fm_demod_cf(32e3, 4, DEVIATION, audio_taps(1025))                   # the longest delay line the kernel takes
    assert blk.engine() == 1
    assert close(blk.work(x), y, 4, audio_taps(1025), n_in) <= TOL
    blk.set_mode(g.MODE_GENERIC)
    assert blk.engine() == 0


def test_nbfm_rx_end_to_end(gpu, po):
    g = gpu
    n_in = 2 * T(g) + 3
    x = stream(1, n_in)
    rx = g.nbfm_rx(16000, 32000)
    assert rx.audio_decim == 2 and len(rx.audio_taps) == 211 and rx.engine() == 1
    assert same_bits(rx.audio_taps, g.firdes_low_pass(1.0, 32000, 2.7e3, 0.5e3, g.WIN_HAMMING))
    k = float(np.float32(32000 / (2 * math.pi * 5e3)))
    assert rx.k == k
    q = g.quadrature_demod_cf(k).work(n_in, np.concatenate([np.zeros(1, np.complex64), x]))
    got = rx.work(x)
    assert len(got) == R.fm_outputs(n_in, 2)
    assert close(got, deemph64(q, R.deemph_taps(32e3)), 2, rx.audio_taps, n_in) <= TOL
    # and the bit-exact mode against the reference's chain
    rx = g.nbfm_rx(16000, 32000)
    rx.set_mode(g.MODE_GENERIC)
    _, y = R.fm_deemphasised(po, x, k, R.deemph_taps(32e3))
    assert same_bits(rx.work(x), R.fm_fir(po, y, 2, rx.audio_taps))
    with pytest.raises(ValueError):
        g.nbfm_rx(16000, 40000)


def test_refusals_and_device_entry(gpu):
    import torch
    g = gpu
    taps = audio_taps(37)
    for args in ((32e3, 0, DEVIATION, taps), (32e3, 4, DEVIATION, [])):
        with pytest.raises((g.GrhipError, ValueError)):
            g.fm_demod_cf(*args)
    blk = g.fm_demod_cf(32e3, 4, DEVIATION, taps)
    for bad in (0, 65536):
        with pytest.raises(g.GrhipError):
            blk.set_streams(bad)
    with pytest.raises(g.GrhipError):
        blk.set_mode(99)
    with pytest.raises(g.GrhipError):
        blk.produced(-1)
    # device buffers, the count through d_produced, both engines
    n_in = T(g) + 1
    x = stream(2, 2 * T(g) + 3)[:n_in]
    d_in = torch.from_numpy(np.array(x)).cuda()
    want = None
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = g.fm_demod_cf(32e3, 4, DEVIATION, taps)
        blk.set_mode(mode)
        d_out = torch.full((R.fm_outputs(n_in, 4) + 8,), float("nan"), dtype=torch.float32, device="cuda")
        d_np = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        blk.work_device(n_in, d_in, d_out, d_np)
        torch.cuda.synchronize()
        assert int(d_np.item()) == R.fm_outputs(n_in, 4)
        out = d_out.cpu().numpy()
        assert np.isnan(out[R.fm_outputs(n_in, 4):]).all() and np.isfinite(out[:R.fm_outputs(n_in, 4)]).all()
        host = g.fm_demod_cf(32e3, 4, DEVIATION, taps)
        host.set_mode(mode)
        assert same_bits(out[:R.fm_outputs(n_in, 4)], host.work(x))
        blk.work_device(0, None, None, d_np)
        torch.cuda.synchronize()
        assert int(d_np.item()) == 0
