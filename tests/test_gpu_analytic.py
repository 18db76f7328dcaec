"""-m gpu: hilbert_fc, filter_delay_fc and goertzel_fc on the device against tests/analytic_ref.py (itself pinned to the
reference's own outputs by tests/test_analytic_cpu.py).

GENERIC is bit for bit.  FAST of the FIR blocks: the real part bit-equal to the delayed input, the imaginary part
within the project's 1e-5 criterion (rel_err_max and the large-element check).  FAST Goertzel is a different, better
conditioned sum than the reference's float recurrence, so its yardstick is the float64 recurrence with the same float
wr, wi: e_fast <= max(e_ref, (log2(len) + 3) 2^-24 mean|x|), where e_ref is the float32 restatement's distance from
that yardstick (measured here) and the second term the rounding bound of a pairwise float sum of len products.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import analytic_ref as ar
from conftest import bits_equal, rel_err_max

pytestmark = pytest.mark.gpu
f32 = np.float32
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")
HERE = os.path.dirname(os.path.abspath(__file__))


def _close(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if rel_err_max(got, ref) > TOL:
        return False
    big = np.abs(ref) > 0.1 * np.abs(ref).max()
    return bool(np.all(np.abs(got[big] - ref[big]) <= TOL * np.abs(ref[big])))


def _stream(seed, n):
    return np.random.default_rng(seed).standard_normal(n).astype(f32)


def _with_history(x, ntaps):
    return np.concatenate([np.zeros(ntaps - 1, dtype=f32), x])


# ---- hilbert_fc -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaps", [2, 3, 5, 19, 51, 255, 1023])
def test_hilbert_generic_bit_exact(gpu, po, ntaps):
    g, n, nt = gpu, 1100, ntaps | 1
    x = _stream(100 + ntaps, n + nt - 1)
    blk = g.hilbert_fc(ntaps)
    blk.set_mode(g.MODE_GENERIC)
    assert blk.history() == nt and blk.ntaps() == nt and blk.decimation() == 1
    assert bits_equal(blk.taps(), ar.firdes_hilbert(nt)) and blk.is_sparse()
    assert bits_equal(blk.work(n, x), ar.hilbert_fc(po, ntaps, n, x))


@pytest.mark.parametrize("ntaps", [3, 19, 51, 255, 1023])
def test_hilbert_fast(gpu, ntaps):
    g, n = gpu, 20000
    x = _stream(200 + ntaps, n)
    xh = _with_history(x, ntaps)
    blk = g.hilbert_fc(ntaps)
    blk.set_mode(g.MODE_FAST)
    got = blk.work(n, xh)
    assert len(got) == n
    assert bits_equal(np.ascontiguousarray(got.real), xh[ntaps // 2:ntaps // 2 + n])
    ref = ar.filter_delay_fc64(ar.firdes_hilbert(ntaps), n, xh)
    assert _close(got.imag, ref.imag), rel_err_max(got.imag, ref.imag)
    for chunk in (1000, 4096):
        assert bits_equal(g.run_sync_block(blk, x, chunk=chunk, out_dtype=np.complex64), got), chunk


# ---- filter_delay_fc ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True], ids=["one_input", "two_inputs"])
@pytest.mark.parametrize("ntaps", [1, 2, 7, 64, 255])
def test_filter_delay_random_taps(gpu, po, ntaps, two):
    g, n = gpu, 5000
    rng = np.random.default_rng(300 + ntaps)
    taps = rng.standard_normal(ntaps).astype(f32)
    x0 = _stream(301 + ntaps, n + ntaps - 1)
    x1 = _stream(302 + ntaps, n + ntaps - 1) if two else None
    blk = g.filter_delay_fc(taps)
    assert blk.history() == ntaps and not blk.is_sparse() and bits_equal(blk.taps(), taps)
    blk.set_mode(g.MODE_GENERIC)
    assert bits_equal(blk.work(n, x0, x1), ar.filter_delay_fc(po, taps, n, x0, x1))
    blk.set_mode(g.MODE_FAST)
    got = blk.work(n, x0, x1)
    ref = ar.filter_delay_fc64(taps, n, x0, x1)
    assert bits_equal(np.ascontiguousarray(got.real), x0[ntaps // 2:ntaps // 2 + n])
    assert _close(got.imag, ref.imag), rel_err_max(got.imag, ref.imag)


def test_filter_delay_with_hilbert_taps_is_hilbert_fc(gpu):
    g, n, nt = gpu, 5000, 63
    x = _stream(400, n + nt - 1)
    fd, hb = g.filter_delay_fc(g.firdes_hilbert(nt)), g.hilbert_fc(nt)
    assert fd.is_sparse() and hb.is_sparse()
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        fd.set_mode(mode)
        hb.set_mode(mode)
        assert bits_equal(fd.work(n, x), hb.work(n, x)), mode


def test_filter_delay_perturbed_taps_take_the_dense_kernel(gpu, po):
    """one even offset from the centre made non-zero: a structure check that is too lenient would drop that tap"""
    g, n, nt = gpu, 5000, 63
    x = _stream(401, n + nt - 1)
    for off in (0, 2, -4):
        taps = g.firdes_hilbert(nt).copy()
        taps[nt // 2 + off] = f32(1e-3)
        blk = g.filter_delay_fc(taps)
        assert not blk.is_sparse()
        blk.set_mode(g.MODE_FAST)
        got = blk.work(n, x)
        ref = ar.filter_delay_fc64(taps, n, x)
        assert _close(got.imag, ref.imag), off
        # the perturbation is visible at this tolerance: the unperturbed filter does not pass
        assert not _close(got.imag, ar.filter_delay_fc64(g.firdes_hilbert(nt), n, x).imag)
        blk.set_mode(g.MODE_GENERIC)
        assert bits_equal(blk.work(n, x), ar.filter_delay_fc(po, taps, n, x))
    asym = g.firdes_hilbert(nt).copy()
    asym[nt // 2 + 1] = np.nextafter(asym[nt // 2 + 1], f32(1))
    assert not g.filter_delay_fc(asym).is_sparse()


@pytest.mark.parametrize("kernel", ["sparse", "dense", "dense_two"])
def test_work_device_any_float_offset(gpu, kernel):
    import torch
    g, n, nt = gpu, 3000, 31
    taps = g.firdes_hilbert(nt) if kernel == "sparse" else np.random.default_rng(500).standard_normal(nt).astype(f32)
    blk = g.filter_delay_fc(taps)
    assert blk.is_sparse() == (kernel == "sparse")
    x0, x1 = _stream(501, n + nt - 1), _stream(502, n + nt - 1)
    for mode in (g.MODE_FAST, g.MODE_GENERIC):
        blk.set_mode(mode)
        want = blk.work(n, x0, x1 if kernel == "dense_two" else None)
        for off in (0, 1, 2, 3):
            d0 = torch.zeros(len(x0) + 8, dtype=torch.float32, device="cuda")
            d1 = torch.zeros(len(x1) + 8, dtype=torch.float32, device="cuda")
            assert d0.data_ptr() % 16 == 0 and d1.data_ptr() % 16 == 0
            d0[off:off + len(x0)] = torch.from_numpy(x0).cuda()
            d1[3 - off:3 - off + len(x1)] = torch.from_numpy(x1).cuda()
            d_out = torch.zeros(2 * n + 4, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            r = blk.work_device(n, d0[off:].data_ptr(), d1[3 - off:].data_ptr() if kernel == "dense_two" else None,
                                d_out[2 * (off & 1):].data_ptr())
            g.lib().grhip_device_synchronize(0)
            assert r == n
            got = d_out.cpu().numpy()[2 * (off & 1):2 * (off & 1) + 2 * n].view(np.complex64)
            assert bits_equal(got, want), (mode, off)


# ---- goertzel_fc ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def goertzel_fx():
    return np.load(os.path.join(HERE, "golden", "ref_goertzel.npz"))


def test_goertzel_generic_fixture_bit_exact(gpu, goertzel_fx):
    g, d = gpu, goertzel_fx
    for k, (rate, ln, fr, nb) in enumerate(zip(d["rate"], d["len"], d["freq"], d["nblocks"])):
        blk = g.goertzel_fc(int(rate), int(ln), float(fr))
        blk.set_mode(g.MODE_GENERIC)
        assert blk.decimation() == ln and blk.history() == 1
        assert bits_equal(blk.work(int(nb), d["x_%d" % k]), d["out_%d" % k]), k


@pytest.mark.parametrize("length", [1, 2, 31, 32, 33, 64, 4096])
def test_goertzel_generic_block_lengths(gpu, length):
    g = gpu
    for nb in (70, 257):
        x = _stream(600 + length + nb, length * nb)
        blk = g.goertzel_fc(8000, length, 440.0)
        blk.set_mode(g.MODE_GENERIC)
        assert bits_equal(blk.work(nb, x), ar.goertzel_fc(8000, length, 440.0, x)), nb


def test_goertzel_set_freq_and_split_calls(gpu):
    g, ln, nb = gpu, 400, 130
    x = _stream(700, ln * nb)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = g.goertzel_fc(8000, ln, 100.0)
        blk.set_mode(mode)
        whole = blk.work(nb, x)
        a, b = blk.work(67, x[:67 * ln]), blk.work(nb - 67, x[67 * ln:])
        assert bits_equal(np.concatenate([a, b]), whole)
        blk.set_freq(250.0)
        c = blk.work(nb - 67, x[67 * ln:])
        other = g.goertzel_fc(8000, ln, 250.0)
        other.set_mode(mode)
        assert bits_equal(c, other.work(nb - 67, x[67 * ln:])) and not bits_equal(c, b)
        blk.set_rate(16000)
        other = g.goertzel_fc(16000, ln, 250.0)
        other.set_mode(mode)
        assert bits_equal(blk.work(5, x[:5 * ln]), other.work(5, x[:5 * ln]))
    blk = g.goertzel_fc(8000, ln, 250.0)
    blk.set_mode(g.MODE_GENERIC)
    assert bits_equal(blk.work(nb - 67, x[67 * ln:]), ar.goertzel_fc(8000, ln, 250.0, x[67 * ln:]))


FAST_CASES = [(8000, 8000, 100.0, 3), (8000, 400, 100.0, 257), (8000, 64, 1000.0, 257), (48000, 1000, 67.0, 70),
              (8000, 2000, 5.0, 70)] + [(8000, ln, 440.0, nb) for ln in (1, 2, 31, 32, 33, 64, 4096) for nb in (70, 257)]


def test_goertzel_fast_against_float64(gpu):
    g = gpu
    bad = []
    print("\nrate len freq nblocks e_ref e_fast bound")
    for rate, ln, fr, nb in FAST_CASES:
        t = np.arange(ln * nb)
        x = (_stream(800 + ln + nb, ln * nb) + 0.7 * np.cos(2 * np.pi * fr * t / rate + 0.3)).astype(f32)
        y64 = ar.goertzel64(rate, ln, fr, x)
        e_ref = float(np.abs(ar.goertzel_fc(rate, ln, fr, x) - y64).max())
        blk = g.goertzel_fc(rate, ln, fr)
        blk.set_mode(g.MODE_FAST)
        got = blk.work(nb, x)
        e_fast = float(np.abs(got - y64).max())
        bound = (math.log2(ln) + 3) * 2.0 ** -24 * float(np.abs(x).mean())
        print("%d %d %g %d %.3e %.3e %.3e" % (rate, ln, fr, nb, e_ref, e_fast, bound))
        if not (len(got) == nb and e_fast <= max(e_ref, bound)):
            bad.append((rate, ln, fr, nb, e_ref, e_fast, bound))
    assert not bad, bad


def test_goertzel_work_device(gpu):
    import torch
    g, ln, nb = gpu, 333, 100
    x = _stream(900, ln * nb + 3)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = g.goertzel_fc(8000, ln, 300.0)
        blk.set_mode(mode)
        for off in (0, 1, 3):
            want = blk.work(nb, x[off:])
            d_in = torch.from_numpy(x).cuda()
            d_out = torch.zeros(2 * nb, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert blk.work_device(nb, d_in[off:].data_ptr(), d_out.data_ptr()) == nb
            g.lib().grhip_device_synchronize(0)
            assert bits_equal(d_out.cpu().numpy().view(np.complex64), want), (mode, off)


def test_bad_arguments(gpu):
    g = gpu
    for make, code in ((lambda: g.hilbert_fc(1), -1), (lambda: g.hilbert_fc(0), -1), (lambda: g.filter_delay_fc([]), -1),
                       (lambda: g.filter_delay_fc(np.ones(16385, f32)), -1), (lambda: g.goertzel_fc(8000, 0, 1.0), -1),
                       (lambda: g.goertzel_fc(0, 10, 1.0), -1), (lambda: g.hilbert_fc(51).set_mode(9), -1),
                       (lambda: g.goertzel_fc(8000, 10, 1.0).set_rate(0), -1)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == code


# ---- the C++ blocks under the stand-in executor ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def analytic_exe(gpu):
    subprocess.check_call(["make", "-C", HOST, "analytic_test"], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "analytic_test")


def test_cpp_blocks_under_executor(gpu, po, analytic_exe, tmp_path):
    n = 70000                                               # more than one default scheduler call
    x = _stream(1000, n)
    x.tofile(tmp_path / "x.bin")
    taps = np.random.default_rng(1001).standard_normal(24).astype(f32)
    taps.tofile(tmp_path / "t.bin")
    runs = [(["hilbert", "50"], lambda: ar.hilbert_fc(po, 50, n, _with_history(x, 51))),
            (["delay", str(tmp_path / "t.bin")], lambda: ar.filter_delay_fc(po, taps, n, _with_history(x, 24))),
            (["goertzel", "8000", "400", "100.0"], lambda: ar.goertzel_fc(8000, 400, 100.0, x))]
    for args, ref in runs:
        r = subprocess.run([analytic_exe] + args + [str(tmp_path / "x.bin"), str(tmp_path / "y.bin")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert bits_equal(np.fromfile(tmp_path / "y.bin", dtype=np.complex64), ref()), args
    r = subprocess.run([analytic_exe, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
