"""GPU tests of blks2.logpwrfft_c / logpwrfft_f, the fused block.

The yardstick is this library's own five blocks in the reference's order (logpwrfft.py:47-63: keep_one_in_n -> fft_vcc |
fft_vfc -> complex_to_mag_squared -> single_pole_iir_filter_ff -> nlog10_ff), given the same calls and the same setter
calls: the dB output and the IIR's final state must match BIT FOR BIT in both modes, on every dispatch leg (the three
register families, their store sites, the composed path), through the persistent loops with a partial last group, with
averaging off, and across the setters.  Against the float64 chain the bounds are test_chain_behind_the_transform's."""
import math
import os
import subprocess

import numpy as np
import pytest

import logpwrfft_ref as lr
import spectrum_ref as sr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "gnuradio-3.5.0-dmr_amd", "host")
f32 = np.float32


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32).reshape(-1), np.ascontiguousarray(b, f32).reshape(-1)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def _frames(kind, S, F, N, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(S * F * N)
    if kind == "c":
        x = 0.5 * np.exp(2j * np.pi * 0.1234 * t) + 0.05 * (rng.normal(size=t.size) + 1j * rng.normal(size=t.size))
        return x.astype(np.complex64)
    return (0.5 * np.cos(2 * np.pi * 0.1234 * t) + 0.05 * rng.normal(size=t.size)).astype(f32)


def _noise(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "c":
        return rng.standard_normal(2 * n, dtype=f32).view(np.complex64)
    return rng.standard_normal(n, dtype=f32)


def _cut(x, S, N, cuts):
    """x is [S][F] frames; yields (frames, [S][frames][N] flattened) for each cut of the frame axis"""
    x = x.reshape(S, -1, N)
    pos = 0
    for c in cuts:
        c = x.shape[1] - pos if c is None else c
        yield c, np.ascontiguousarray(x[:, pos:pos + c]).reshape(-1)
        pos += c


class Chain(object):
    """the library's five blocks in the reference's order, with the hier block's setters"""

    def __init__(self, g, kind, N, S, decim, alpha, average, win, ref_scale, mode):
        w = lr.blackmanharris(N) if win is None else list(win)
        self.k = f32(lr.k_of(N, w, ref_scale))
        w32 = np.asarray(w, np.float64).astype(f32)
        self.kind, self.N, self.S, self.alpha, self.avg = kind, N, S, alpha, average
        self.keep = g.keep_one_in_n(N * (8 if kind == "c" else 4), decim)
        self.fft = g.fft_vcc(N, True, w32) if kind == "c" else g.fft_vfc(N, True, w32)     # a wrong length: ignored there too
        self.mag, self.iir = g.complex_to_mag_squared(N), g.single_pole_iir_filter_ff(alpha if average else 1.0, N)
        self.log = g.nlog10_ff(10, N, self.k)
        for b in (self.keep, self.mag, self.iir, self.log):
            b.set_streams(S)
        self.set_mode(mode)

    def set_mode(self, mode):
        for b in (self.mag, self.iir, self.log):
            b.set_mode(mode)

    def set_average(self, average):
        self.avg = average
        self.iir.set_taps(self.alpha if average else 1.0)

    def set_avg_alpha(self, alpha):
        self.alpha = alpha
        self.set_average(self.avg)

    def work(self, c, part):
        kept = self.keep.work(c, part)
        n = len(kept) // (self.S * self.N)
        if not n:
            return np.zeros(0, f32)
        spec = self.fft.work(self.S * n, kept)
        return self.log.work(n, self.iir.work(n, self.mag.work(n, spec)))

    def state(self):
        """the IIR's state: with taps 0.0 its next output is (float)(0 * x + 1 * y_prev) = y_prev (changes the taps: last)"""
        self.iir.set_taps(0.0)
        return self.iir.work(1, np.zeros(self.S * self.N, f32))


def _pair(g, kind, N, S, decim, alpha, average, win=None, ref_scale=2.0, mode=None):
    mode = g.MODE_GENERIC if mode is None else mode
    cls = g.logpwrfft_c if kind == "c" else g.logpwrfft_f
    frame_rate = 30.0
    blk = cls(frame_rate * N * decim, N, ref_scale, frame_rate, alpha, average, win)
    assert blk.decimation() == decim
    blk.set_streams(S)
    blk.set_mode(mode)
    return blk, Chain(g, kind, N, S, decim, alpha, average, win, ref_scale, mode)


# ---- every dispatch leg at small sizes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 100])
@pytest.mark.parametrize("kind", ["c", "f"])
def test_every_leg_equals_the_five_blocks(gpu, kind, N):
    """14 frames split 1 / 1 / rest at decimation 3: the first two calls keep nothing and only advance the countdown.
    N = 16 and 100 take the composed path (too small; Bluestein), the others the fused kernels: with averaging on the
    power kind of every size plus the averaging pass, with averaging off the dB kind of every size and its state store.
    With three streams and four kept frames each a group of the 32 ... 2048 family straddles streams."""
    g = gpu
    for S in (1, 3):
        x = _frames(kind, S, 14, N, N + S)
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            for average in (True, False):
                blk, ch = _pair(g, kind, N, S, 3, 0.2, average, mode=mode)
                kept = 0
                for c, part in _cut(x, S, N, (1, 1, None)):
                    want = ch.work(c, part)
                    assert blk.produced(c) == len(want) // (S * N)
                    got = blk.work(c, part)
                    assert _same_bits(got, want), (S, mode, average, c)
                    kept += len(got) // (S * N)
                assert kept == 4
                assert _same_bits(blk.state(), ch.state()), (S, mode, average)


@pytest.mark.parametrize("N,wlen", [(64, 64), (256, 256), (64, 48), (100, 100)])
def test_callers_window_and_wrong_length(gpu, N, wlen):
    """a caller's window (as doubles), and one of the wrong length: the transform runs unwindowed, k from the given values"""
    g = gpu
    win = (np.hamming(wlen) + 0.01).tolist()
    for kind in ("c", "f"):
        x = _frames(kind, 2, 9, N, wlen)
        blk, ch = _pair(g, kind, N, 2, 2, 0.3, True, win=win, ref_scale=0.5)
        assert _same_bits(blk.work(9, x), ch.work(9, x))
        assert _same_bits(blk.state(), ch.state())


# ---- the persistent loops and the partial last group -----------------------------------------------------------------------
@pytest.mark.parametrize("N,kind", [(32, "c"), (256, "f"), (1024, "c"), (4096, "f"), (8192, "c")])
def test_persistent_loop_and_partial_group(gpu, N, kind):
    """4 CUs 4096 / N kept frames plus half a group plus one.  The grids are capped at three workgroups per CU (two for
    8192 points), so that is one full trip of every workgroup, a second trip of about a third of them (at 8192 points a
    second trip of all and a third trip of one), and a partial last group.  FAST mode (the chain's IIR would dominate
    otherwise)."""
    import torch
    g = gpu
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    group = max(4096 // N, 1)
    kept = (4 * cus * 4096) // N + group // 2 + 1
    F = 2 * kept
    x = _noise(kind, F * N, N)
    print("N %d %s: %d frames in (%.1f MB), %d kept, %d CUs" % (N, kind, F, x.nbytes / 1e6, kept, cus))
    blk, ch = _pair(g, kind, N, 1, 2, 0.2, True, mode=g.MODE_FAST)
    want = ch.work(F, x)
    got = blk.work(F, x)
    assert len(got) == kept * N
    assert _same_bits(got, want)
    assert _same_bits(blk.state(), ch.state())


# ---- averaging off ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192])
def test_averaging_off_then_on(gpu, N):
    """off = IIR taps 1.0: dB straight from the transform kernel, the state the power of the last kept frame of every
    stream; set_average(True) then continues from it"""
    g = gpu
    for kind in ("c", "f"):
        S = 3
        x = _frames(kind, S, 11, N, 7 * N)
        blk, ch = _pair(g, kind, N, S, 2, 0.25, False)
        assert not blk.average()
        parts = list(_cut(x, S, N, (1, 6, None)))
        for c, part in parts[:2]:
            assert _same_bits(blk.work(c, part), ch.work(c, part))
        blk.set_average(True)
        ch.set_average(True)
        assert blk.average() and blk.avg_alpha() == 0.25
        c, part = parts[2]
        assert _same_bits(blk.work(c, part), ch.work(c, part))
        assert _same_bits(blk.state(), ch.state())
    # the state after an averaging-off call alone
    blk, ch = _pair(g, "c", N, 2, 3, 0.5, False)
    x = _frames("c", 2, 7, N, N)
    assert _same_bits(blk.work(7, x), ch.work(7, x))
    assert _same_bits(blk.state(), ch.state())


# ---- state and setters --------------------------------------------------------------------------------------------------------
def test_state_and_setters(gpu):
    g = gpu
    N, S = 128, 2
    x = _frames("c", S, 30, N, 5)
    blk, ch = _pair(g, "c", N, S, 3, 0.2, True)
    parts = list(_cut(x, S, N, (4, 5, 4, 6, None)))
    c, part = parts[0]
    assert blk.produced(c) == blk.produced(c) == 1               # asking changes nothing
    assert _same_bits(blk.work(c, part), ch.work(c, part))
    blk.set_avg_alpha(0.7)                                        # new taps, the state kept
    ch.set_avg_alpha(0.7)
    blk.set_mode(g.MODE_FAST)                                     # the state kept
    ch.set_mode(g.MODE_FAST)
    c, part = parts[1]
    assert _same_bits(blk.work(c, part), ch.work(c, part))
    blk.set_decimation(2.5)                                       # rounds half away from zero: 3, and reloads the countdown
    ch.keep.set_n(3)
    assert blk.decimation() == 3
    c, part = parts[2]
    got = blk.work(c, part)
    assert len(got) == S * N and _same_bits(got, ch.work(c, part))    # countdown reloaded: frame 2 of these 4
    blk.set_vec_rate(blk.sample_rate() / N / 2)                   # decimation 2
    ch.keep.set_n(2)
    assert blk.decimation() == 2 and blk.frame_rate() == blk.sample_rate() / N / 2
    c, part = parts[3]
    assert _same_bits(blk.work(c, part), ch.work(c, part))
    blk.set_sample_rate(blk.sample_rate() * 2)                    # decimation 4
    ch.keep.set_n(4)
    assert blk.decimation() == 4
    c, part = parts[4]
    assert _same_bits(blk.work(c, part), ch.work(c, part))
    assert _same_bits(blk.state(), ch.state())
    # set_streams restarts state and countdown
    blk.set_streams(1)
    assert not blk.state().any()
    _, ch2 = _pair(g, "c", N, 1, 3, 0.2, True, mode=g.MODE_FAST)
    blk.set_decimation(3)
    blk.set_avg_alpha(0.2)
    y = _frames("c", 1, 7, N, 9)
    assert _same_bits(blk.work(7, y), ch2.work(7, y))
    for bad in (1.5, -1e-9):
        with pytest.raises(g.GrhipError) as e:
            blk.set_avg_alpha(bad)
        assert e.value.code == -2                                # GRHIP_ERANGE
    assert blk.avg_alpha() == 0.2


# ---- against the float64 chain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 100, 4096])
@pytest.mark.parametrize("kind", ["c", "f"])
def test_against_the_float64_chain(gpu, kind, N):
    """spectrum_ref.chain_f64 with the restated window and k: 2.5e-6 max(log2 N, 1) of the call's peak in linear power,
    0.02 dB over the bins within 40 dB of the peak (the bounds of test_chain_behind_the_transform)."""
    g = gpu
    F, decim, alpha = 14, 3, 0.2
    wd = lr.blackmanharris(N)
    k = f32(lr.k_of(N, wd, 2.0))
    w = np.asarray(wd, np.float64).astype(f32)
    kept_idx = list(range(decim - 1, F, decim))
    for S in (1, 3):
        x = _frames(kind, S, F, N, N + S)
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            blk, _ = _pair(g, kind, N, S, decim, alpha, True, mode=mode)
            out = blk.work(F, x).reshape(S, len(kept_idx), N).astype(np.float64)
            for s in range(S):
                ref_db, p_ref, _ = sr.chain_f64(x.reshape(S, F, N)[s, kept_idx], w, alpha, k)
                e_lin = np.abs(10.0 ** ((out[s] - float(k)) / 10.0) - p_ref).max() / p_ref.max()
                near = p_ref >= p_ref.max() * 1e-4
                e_db = np.abs(out[s] - ref_db)[near].max()
                print("logpwrfft_%s N %d mode %d stream %d/%d: linear %.3g of peak (bound %.3g), %.3g dB within 40 dB of the peak"
                      % (kind, N, mode, s, S, e_lin, 2.5e-6 * max(math.log2(N), 1), e_db))
                assert e_lin <= 2.5e-6 * max(math.log2(N), 1) and e_db <= 0.02


# ---- the C++ blocks -------------------------------------------------------------------------------------------------------------
def test_cpp_blocks(gpu):
    subprocess.check_call(["make", "-C", HOST, "logpwrfft_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "logpwrfft_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
