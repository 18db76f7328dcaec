"""GPU tests of the spectrum-estimate blocks: complex_to_mag_squared, single_pole_iir_filter_ff, nlog10_ff and
keep_one_in_n, the stages of blks2.logpwrfft behind its transform.

- GENERIC: mag^2 and the IIR bit for bit against spectrum_ref.py; keep_one_in_n exact in both modes.
- nlog10_ff (both modes): within 4 float ulps, at the output's magnitude, of the float64 value of the same float input.
- FAST IIR: within 1e-5 of the output's peak of the float64 recurrence.
- The blocks in a row behind fft_vcc / fft_vfc against the float64 chain (numpy FFT of the float-windowed input, float64
  power and recurrence).  The measured errors are printed."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import spectrum_ref as sr
from conftest import bits_equal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "gnuradio-3.5.0-dmr_amd", "host")
QA = json.load(open(os.path.join(HERE, "golden", "ref_qa_spectrum.json")))
f32 = np.float32


def _split(x, S, per_item, cuts):
    """x is [S][n] items of per_item elements; yields (count, [S][count] items flattened) for each cut of the item axis"""
    x = x.reshape(S, -1, per_item)
    pos = 0
    for c in cuts:
        c = x.shape[1] - pos if c is None else c
        yield c, np.ascontiguousarray(x[:, pos:pos + c, :]).reshape(-1)
        pos += c


def _join(parts, S, per_item):
    """the per-call outputs ([S][count] items each, empty ones left out) as one [S][n] array"""
    return np.concatenate([p.reshape(S, -1, per_item) for p in parts if p.size], axis=1).reshape(-1)


# ---- stand-alone blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vlen,n", [(1, 1000 + 37), (4096, 3)])
def test_mag_squared_bit_exact(gpu, vlen, n):
    g = gpu
    rng = np.random.default_rng(vlen)
    z = (rng.normal(size=n * vlen) * 10 ** rng.uniform(-3, 3, n * vlen) + 1j * rng.normal(size=n * vlen)).astype(np.complex64)
    want = sr.mag_squared(z)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        b = g.complex_to_mag_squared(vlen)
        b.set_mode(mode)
        assert bits_equal(b.work(n, z), want)
    c = QA["complex_to_mag_squared"][0]
    got = g.complex_to_mag_squared().work(6, np.array([complex(a, b) for a, b in c["src"]], np.complex64))
    assert got.tolist() == c["expected"]


@pytest.mark.parametrize("vlen", [1, 2, 100, 4096])
def test_iir_generic_bit_exact(gpu, vlen):
    g = gpu
    n = 20
    for S in (1, 3):
        rng = np.random.default_rng(vlen * 10 + S)
        x = (rng.normal(size=S * n * vlen) * 100).astype(f32)
        for alpha in (0.0, 0.125, 1.0):
            b = g.single_pole_iir_filter_ff(alpha, vlen)
            b.set_mode(g.MODE_GENERIC)
            b.set_streams(S)
            ref = sr.SinglePoleIir(alpha, vlen, S)
            got, want = [], []
            for i, (c, part) in enumerate(_split(x, S, vlen, (1, 7, None))):
                if i == 2:                              # new taps, the state kept
                    b.set_taps(0.3)
                    ref.set_taps(0.3)
                got.append(b.work(c, part))
                want.append(ref.work(part.reshape(S, -1)))
            assert bits_equal(_join(got, S, vlen), _join(want, S, vlen)), (S, alpha)


@pytest.mark.parametrize("vlen", [1, 2])
def test_iir_fast_chunked(gpu, vlen):
    g = gpu
    chunk = g.single_pole_iir_filter_ff.chunk()
    n = 3 * chunk + 37
    rng = np.random.default_rng(vlen)
    x = (rng.normal(size=n * vlen) + 2.0).astype(f32)
    for alpha in (0.05, 0.0, 1.0):
        b = g.single_pole_iir_filter_ff(alpha, vlen)
        b.set_mode(g.MODE_FAST)
        cut = chunk + 5
        got = np.concatenate([b.work(cut, x[:cut * vlen]), b.work(n - cut, x[cut * vlen:])])
        want, _ = sr.iir_f64(x.reshape(n, vlen), alpha)
        err = np.abs(got.reshape(n, vlen) - want).max()
        peak = max(np.abs(want).max(), 1e-30)
        print("single_pole_iir FAST vlen %d alpha %g: %.3g of peak" % (vlen, alpha, err / peak))
        assert err <= 1e-5 * peak


def _ulps_from_f64(got, x, n, k):
    want = sr.nlog10_f64(x, n, k)
    return np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(f32)).astype(np.float64)


def test_nlog10(gpu):
    g = gpu
    c = QA["nlog10"][0]
    sweep = np.concatenate([np.array(c["src"], f32), np.logspace(-30, 30, 1201).astype(f32), np.array([0, -1, np.nan], f32)])
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        b = g.nlog10_ff(c["n"], 1, c["k"])
        b.set_mode(mode)
        got = b.work(len(sweep), sweep)
        assert np.isnan(got[-1]) and not np.isnan(got[:-1]).any()
        u = _ulps_from_f64(got[:-1], sweep[:-1], c["n"], c["k"])
        print("nlog10_ff mode %d: max %.2f ulp" % (mode, u.max()))
        assert u.max() <= 4
        # the clamp: zero, negative and tiny inputs give n * -18 + k
        low = got[np.flatnonzero(sweep[:-1] < 1e-18)]
        assert len(low) > 100 and np.all(np.abs(low - (-180.0)) <= 4 * np.spacing(f32(180)))
    v = g.nlog10_ff(20, 5, 0)                       # a vector form is the same element-wise pass
    got = v.work(3, np.arange(1, 16, dtype=f32))
    assert _ulps_from_f64(got, np.arange(1, 16, dtype=f32), 20, 0).max() <= 4


@pytest.mark.parametrize("item_size", [4, 32768])
def test_keep_one_in_n(gpu, item_size):
    g = gpu
    total = 23
    rng = np.random.default_rng(item_size)
    x = rng.integers(0, 256, total * item_size, dtype=np.uint8)
    items = x.reshape(total, item_size)
    for n in (1, 3, 7):
        b = g.keep_one_in_n(item_size, n)
        ref = sr.KeepOneInN(n)
        pos = 0
        for c in (5, 1, total - 6):
            assert b.produced(c) == b.produced(c)                # asking changes nothing
            want = items[[pos + i for i in ref.kept(c)]]
            assert b.produced(c) == len(want)
            got = b.work(c, items[pos:pos + c])
            assert bits_equal(got.reshape(-1, item_size), want)
            pos += c
    b = g.keep_one_in_n(4, 3)
    b.work(4, x[:16])                                            # countdown now 2
    b.set_n(0)                                                   # clamped to 1, countdown reloaded
    assert bits_equal(b.work(3, x[:12]), x[:12])
    b.set_n(3)
    b.set_streams(2)                                             # two streams share the countdown
    got = b.work(4, x[:32])
    assert bits_equal(got, np.concatenate([x[8:12], x[24:28]]))


def test_alpha_out_of_range_is_refused(gpu):
    g = gpu
    b = g.single_pole_iir_filter_ff(0.5)
    for bad in (1.5, -1e-9):
        with pytest.raises(g.GrhipError) as e:
            b.set_taps(bad)
        assert e.value.code == -2                               # GRHIP_ERANGE
    with pytest.raises(g.GrhipError) as e:
        g.single_pole_iir_filter_ff(1.5, 8)
    assert e.value.code == -2


# ---- the blocks in a row: the chain of blks2.logpwrfft behind a transform of this library -----------------------------------
def _frames(kind, S, F, N, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(S * F * N)
    if kind == "c":
        x = 0.5 * np.exp(2j * np.pi * 0.1234 * t) + 0.05 * (rng.normal(size=t.size) + 1j * rng.normal(size=t.size))
        return x.astype(np.complex64)
    return (0.5 * np.cos(2 * np.pi * 0.1234 * t) + 0.05 * rng.normal(size=t.size)).astype(f32)


@pytest.mark.parametrize("N", [64, 100])
@pytest.mark.parametrize("kind", ["c", "f"])
def test_chain_behind_the_transform(gpu, kind, N):
    """fft_vcc | fft_vfc -> keep_one_in_n(3) -> complex_to_mag_squared -> single_pole_iir_filter_ff(0.2) -> nlog10_ff(10),
    frames split 1 / 1 / rest so that the first two calls keep nothing and only advance the countdown.  GENERIC: power
    and average bit for bit the restatement on this library's own spectrum (the log stage has test_nlog10).  Both modes against
    the float64 chain: 2.5e-6 max(log2 N, 1) of the call's peak in linear power (twice the transform's amplitude rule
    plus margin for the averaging), 0.02 dB over the bins within 40 dB of the peak."""
    g = gpu
    F, decim, alpha, k = 14, 3, 0.2, f32(0)
    w = np.blackman(N).astype(f32)
    for S in (1, 3):
        x = _frames(kind, S, F, N, N + S)
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            fft = g.fft_vcc(N, True, w) if kind == "c" else g.fft_vfc(N, True, w)
            keep, mag = g.keep_one_in_n(N * 8, decim), g.complex_to_mag_squared(N)
            iir, log = g.single_pole_iir_filter_ff(alpha, N), g.nlog10_ff(10, N, k)
            for b in (keep, mag, iir, log):
                b.set_streams(S)
            for b in (mag, iir, log):
                b.set_mode(mode)
            ctr, ref_iir = sr.KeepOneInN(decim), sr.SinglePoleIir(alpha, N, S)
            outs, kept_idx, pos = [], [], 0
            for c, part in _split(x, S, N, (1, 1, None)):
                spec = fft.work(S * c, part)
                idx = ctr.kept(c)
                assert keep.produced(c) == len(idx)
                kept = keep.work(c, spec.view(np.uint8)).view(np.complex64)
                assert bits_equal(kept, np.ascontiguousarray(spec.reshape(S, c, N)[:, idx]).reshape(-1))
                kept_idx += [pos + i for i in idx]
                pos += c
                if not idx:
                    continue
                avg = iir.work(len(idx), mag.work(len(idx), kept))
                out = log.work(len(idx), avg)
                if mode == g.MODE_GENERIC:
                    assert bits_equal(avg, ref_iir.work(sr.mag_squared(kept).reshape(S, -1)))
                outs.append(out)
            out = _join(outs, S, N).reshape(S, len(kept_idx), N).astype(np.float64)
            assert len(kept_idx) == 4
            for s in range(S):
                ref_db, p_ref, _ = sr.chain_f64(x.reshape(S, F, N)[s, kept_idx], w, alpha, k)
                e_lin = np.abs(10.0 ** ((out[s] - float(k)) / 10.0) - p_ref).max() / p_ref.max()
                near = p_ref >= p_ref.max() * 1e-4
                e_db = np.abs(out[s] - ref_db)[near].max()
                print("chain %s N %d mode %d stream %d/%d: linear %.3g of peak (bound %.3g), %.3g dB within 40 dB of the peak"
                      % (kind, N, mode, s, S, e_lin, 2.5e-6 * max(math.log2(N), 1), e_db))
                assert e_lin <= 2.5e-6 * max(math.log2(N), 1) and e_db <= 0.02


# ---- the C++ blocks --------------------------------------------------------------------------------------------------------
def test_cpp_blocks(gpu):
    subprocess.check_call(["make", "-C", HOST, "spectrum_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "spectrum_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
