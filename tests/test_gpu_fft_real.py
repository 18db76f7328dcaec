"""GPU tests of fft_filter_fff and fft_vfc against tests/fft_real_ref.py (float64): parity with the restated
gri_fft_filter_fff_generic and with the direct-form FIR over call lengths that exercise the pairing of engine blocks
(a lone block, a full pair, pair plus lone, the history handed over at odd and even block counts), isolation between
the two blocks that share a transform, set_taps, the device entry, refusals, the C++ blocks under the stand-in
executor; fft_vfc against the float64 transform and value for value against fft_vcc on the widened input."""
import os
import subprocess

import numpy as np
import pytest

import fft_real_ref as fr
from conftest import bits_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")
OLS_N, OLS_MAX_TAPS = 4096, 2049          # csrc/fft_kernels.h

FUSED = [(1, 1), (2, 1), (7, 1), (64, 2), (256, 4), (255, 5), (1000, 1), (2049, 3), (300, 16), (100, 8)]
LONG = [(2500, 1), (5000, 2)]


def _rf(rng, n):
    return rng.standard_normal(n).astype(np.float32)


def _engine_block(ntaps, decim):
    return ((OLS_N - ntaps + 1) // decim) * decim


def _tol_restated(ns, ref):
    return 2e-6 * np.log2(2 * ns) * np.abs(ref).max()


def _tol_direct(direct, taps):
    return 1e-5 * max(np.abs(direct).max(), 1e-3 * np.abs(taps).sum())


def _call_multiples(ntaps, decim, ns):
    """output multiples per call, and the engine blocks each call then covers.  Fused path: the largest call of 1, 2, 3
    and 5 engine blocks.  Where one output multiple already spans more than that many engine blocks ((2049, 3): nine,
    (300, 16): three) the pattern cannot be met in engine blocks; the calls are then 1, 2, 3 and 5 output multiples,
    which still hand the history over at odd and at even block counts (asserted below).  Long path: 1, 2, 3, 5 of the
    reference's own blocks."""
    if ntaps > OLS_MAX_TAPS:
        return [1, 2, 3, 5], None
    L = _engine_block(ntaps, decim)
    ks = [(t * L) // (ns * decim) for t in (1, 2, 3, 5)]
    if min(ks) < 1 or len(set(ks)) < 4:
        ks = [1, 2, 3, 5]
    blocks = [-(-(k * ns * decim) // L) for k in ks]
    return ks, blocks


@pytest.mark.parametrize("ntaps,decim", FUSED + LONG)
def test_fft_filter_fff_vs_restatement_and_direct_form(gpu, ntaps, decim):
    rng = np.random.default_rng(7 * ntaps + decim)
    taps = _rf(rng, ntaps)
    ref_blk = fr.FftFilterFff(decim, taps)
    blk = gpu.fft_filter_fff(decim, taps)
    ns = blk.nsamples()
    assert ns == ref_blk.nsamples and blk.decimation() == decim and blk.history() == 1
    ks, blocks = _call_multiples(ntaps, decim, ns)
    if blocks is not None:
        if ns * decim <= _engine_block(ntaps, decim):
            assert blocks == [1, 2, 3, 5], blocks
        else:
            assert {b & 1 for b in blocks} == {0, 1}, blocks
    nout = sum(ks) * ns
    x = _rf(rng, nout * decim)
    ref = ref_blk.filter(nout, x)
    got, rd = [], 0
    for k in ks:
        got.append(blk.work(k * ns, x[rd * decim:(rd + k * ns) * decim]))
        rd += k * ns
    got = np.concatenate(got)
    assert len(got) == nout
    e1, t1 = np.abs(got - ref).max(), _tol_restated(ns, ref)
    direct = fr.fir_direct(taps, x, nout, decim)
    e2, t2 = np.abs(got - direct).max(), _tol_direct(direct, taps)
    print("ntaps %d decim %d calls %s engine blocks %s: vs restatement %.3g (tol %.3g), vs direct form %.3g (tol %.3g)"
          % (ntaps, decim, ks, blocks, e1, t1, e2, t2))
    assert e1 <= t1
    assert e2 <= t2
    with pytest.raises(gpu.GrhipError):
        blk.work(ns + 1, x)                      # not a multiple of nsamples (the reference asserts)


def test_fft_filter_fff_reference_qa_vectors(gpu):
    """qa_fft_filter.py:174-203: taps (1,) and (2,) on 0..7"""
    src = np.arange(8, dtype=np.float32)
    for tap in (1.0, 2.0):
        blk = gpu.fft_filter_fff(1, [tap])
        assert blk.nsamples() == 2
        got = blk.work(8, src)
        np.testing.assert_almost_equal(got, tap * src, 5)


def test_fft_filter_fff_paired_blocks_are_isolated(gpu):
    """six engine blocks alternately loud (amplitude 1e3) and exactly zero: a quiet block shares its transform with a
    loud one.  More than ntaps-1 samples after a loud stretch ends the convolution is exactly zero; there the output
    must stay within the parity tolerance of the call's peak."""
    ntaps, decim = 64, 1
    rng = np.random.default_rng(11)
    taps = _rf(rng, ntaps)
    blk = gpu.fft_filter_fff(decim, taps)
    ns, L = blk.nsamples(), _engine_block(ntaps, decim)
    nout = -(-6 * L // ns) * ns
    x = np.zeros(nout, np.float32)
    for b in (0, 2, 4):
        x[b * L:(b + 1) * L] = 1e3 * _rf(rng, L)
    direct = fr.fir_direct(taps, x, nout, decim)
    quiet = np.zeros(nout, bool)
    for b in (1, 3, 5):
        quiet[b * L + ntaps - 1:(b + 1) * L] = True
    quiet[6 * L + ntaps - 1:] = True
    assert not direct[quiet].any() and quiet.sum() > 3 * (L - ntaps)
    got = blk.work(nout, x)
    tol = _tol_restated(ns, direct)
    leak = np.abs(got[quiet]).max()
    print("leakage into silent paired blocks %.3g of a peak of %.3g (tol %.3g)" % (leak, np.abs(direct).max(), tol))
    assert leak <= tol
    assert np.abs(got - direct).max() <= _tol_direct(direct, taps)


def test_fft_filter_fff_set_taps(gpu):
    rng = np.random.default_rng(3)
    t1, t2 = _rf(rng, 33), _rf(rng, 200)
    blk = gpu.fft_filter_fff(1, t1)
    ns1 = blk.nsamples()
    x = _rf(rng, 4096)
    blk.work(ns1, x[:ns1])
    blk.set_taps(t2)
    assert blk.nsamples() == ns1                 # latched: nothing changes before the next work
    assert len(blk.work(ns1, x[:ns1])) == 0      # takes effect, produces nothing (gr_fft_filter_fff.cc:83-88)
    ns2 = blk.nsamples()
    assert ns2 == fr.sizes(200)[1] and ns2 != ns1
    got = blk.work(2 * ns2, x[:2 * ns2])         # carried state was cleared by set_taps
    fresh = gpu.fft_filter_fff(1, t2).work(2 * ns2, x[:2 * ns2])
    assert bits_equal(got, fresh)
    ref = fr.FftFilterFff(1, t2).filter(2 * ns2, x[:2 * ns2])
    assert np.abs(got - ref).max() <= _tol_restated(ns2, ref)


@pytest.mark.parametrize("ntaps,decim", [(256, 4), (2500, 1)])
def test_fft_filter_fff_device_entry_equals_host_entry(gpu, ntaps, decim):
    import torch
    rng = np.random.default_rng(ntaps)
    taps = _rf(rng, ntaps)
    a, b = gpu.fft_filter_fff(decim, taps), gpu.fft_filter_fff(decim, taps)
    ns = a.nsamples()
    calls = [3 * ns, 4 * ns] if ntaps > OLS_MAX_TAPS else [7 * ns, 11 * ns]         # (256, 4): two, then three engine blocks
    x = _rf(rng, sum(calls) * decim)
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.full((sum(calls) + 16,), 7.0, dtype=torch.float32, device="cuda")
    want, rd = [], 0
    for n in calls:
        want.append(a.work(n, x[rd * decim:(rd + n) * decim]))
        assert b.work_device(n, d_x[rd * decim:], d_y[rd:]) == n
        rd += n
    torch.cuda.synchronize()
    got = d_y.cpu().numpy()
    assert bits_equal(got[:rd], np.concatenate(want))
    assert (got[rd:] == 7.0).all()               # nothing behind the items produced


def test_fft_filter_fff_refusals(gpu):
    import ctypes as C
    with pytest.raises(gpu.GrhipError):
        gpu.fft_filter_fff(0, [1.0])
    with pytest.raises(gpu.GrhipError):
        gpu.fft_filter_fff(1, [])
    L = gpu.lib()
    buf = np.zeros(8, np.float32)
    assert L.grhip_fft_filter_fff_work(None, 2, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data)) < 0
    assert L.grhip_fft_filter_fff_nsamples(None) < 0


# ---- the C++ blocks under the stand-in executor -------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(gpu):
    subprocess.check_call(["make", "-C", HOST, "fft_real_test"], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "fft_real_test")


def _run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return r.stdout


def test_host_block_errors(host_exe):
    assert "errors test: ok" in _run(host_exe, ["errors"])


@pytest.mark.parametrize("ntaps", [1025, 2500])
def test_host_fft_filter_fff_equals_binding(gpu, host_exe, tmp_path, ntaps):
    """The executor asks for two output multiples per call, the binding is called with four and eight.  Both chunkings
    cut the stream on pair boundaries (1025 taps: nsamples = 3072 = one engine block; 2500 taps: the reference's own
    blocks), so every transform sees the same two blocks and the results are equal bit for bit -- a cut inside a pair
    would change the rounding (never the tolerance)."""
    rng = np.random.default_rng(ntaps)
    taps = _rf(rng, ntaps)
    blk = gpu.fft_filter_fff(1, taps)
    ns = blk.nsamples()
    if ntaps <= OLS_MAX_TAPS:
        assert ns == _engine_block(ntaps, 1)
    x = _rf(rng, 12 * ns)
    want = np.concatenate([blk.work(4 * ns, x[:4 * ns]), blk.work(8 * ns, x[4 * ns:])])
    tp, ip, op = (str(tmp_path / n) for n in ("taps.bin", "in.bin", "out.bin"))
    taps.tofile(tp); x.tofile(ip)
    _run(host_exe, ["filter", 1, 2 * ns, tp, ip, op])
    assert bits_equal(np.fromfile(op, np.float32), want)


def test_host_fft_filter_fff_set_taps_returns_zero_once(gpu, host_exe, tmp_path):
    rng = np.random.default_rng(21)
    t1, t2 = _rf(rng, 33), _rf(rng, 200)
    ns1, ns2 = fr.sizes(33)[1], fr.sizes(200)[1]
    x = _rf(rng, 2 * 6 * ns1 * ns2 // 8)
    half = len(x) // 2
    p = [str(tmp_path / n) for n in ("t1.bin", "t2.bin", "in.bin", "out.bin")]
    t1.tofile(p[0]); t2.tofile(p[1]); x.tofile(p[2])
    out = _run(host_exe, ["retap", 1, 4096, p[0], p[1], p[2], p[3]])
    n1, n2 = (half // ns1) * ns1, ((len(x) - half) // ns2) * ns2
    assert "multiples %d %d first %d" % (ns1, ns2, n1) in out
    got = np.fromfile(p[3], np.float32)
    assert len(got) == n1 + n2
    r1 = fr.FftFilterFff(1, t1).filter(n1, x[:n1])
    r2 = fr.FftFilterFff(1, t2).filter(n2, x[half:half + n2])          # a fresh filter: the carried state was cleared
    assert np.abs(got[:n1] - r1).max() <= _tol_restated(ns1, r1)
    assert np.abs(got[n1:] - r2).max() <= _tol_restated(ns2, r2)


def test_host_fft_vfc_equals_binding(gpu, host_exe, tmp_path):
    rng = np.random.default_rng(8)
    N, nvec = 256, 37
    w, x = _rf(rng, N), _rf(rng, N * nvec)
    want = gpu.fft_vfc(N, True, w).work(nvec, x)
    p = [str(tmp_path / n) for n in ("w.bin", "in.bin", "out.bin")]
    w.tofile(p[0]); x.tofile(p[1])
    _run(host_exe, ["vfc", N, 5, p[0], p[1], p[2]])
    assert bits_equal(np.fromfile(p[2], np.complex64), want)


# ---- fft_vfc --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvec", [1, 3])
@pytest.mark.parametrize("N", [1, 2, 8, 32, 100, 1000, 4096, 8192, 16384])
def test_fft_vfc_vs_float64_and_fft_vcc(gpu, N, nvec):
    """native register kernels (1 ... 8192, real-input load path), direct DFT (100), Bluestein (1000), four-step (16384);
    within 1e-6 max(log2 N, 1) of the spectrum's peak, and value for value what fft_vcc gives on x + 0j"""
    rng = np.random.default_rng(N + nvec)
    x = _rf(rng, N * nvec)
    for window in (None, _rf(rng, N)):
        got = gpu.fft_vfc(N, True, window).work(nvec, x)
        ref = fr.fft_vfc(x, N, window)
        assert got.dtype == np.complex64 and len(got) == N * nvec
        err, tol = np.abs(got - ref).max(), 1e-6 * max(np.log2(N), 1) * np.abs(ref).max()
        print("N %d nvec %d window %s: %.3g (tol %.3g)" % (N, nvec, window is not None, err, tol))
        assert err <= tol
        vcc = gpu.fft_vcc(N, True, window, False).work(nvec, x.astype(np.complex64))
        assert np.array_equal(got, vcc)


def test_fft_vfc_refusals_and_set_window(gpu):
    with pytest.raises(gpu.GrhipError) as e:
        gpu.fft_vfc(64, False, None)
    assert e.value.code == -1                    # GRHIP_EINVAL
    with pytest.raises(gpu.GrhipError) as e:
        gpu.fft_vfc(0, True, None)
    assert e.value.code == -2                    # GRHIP_ERANGE
    rng = np.random.default_rng(2)
    N = 64
    w, x = _rf(rng, N), _rf(rng, N)
    blk = gpu.fft_vfc(N, True, w)
    before = blk.work(1, x)
    assert blk.set_window(_rf(rng, N - 1)) is False
    assert bits_equal(blk.work(1, x), before)    # the old window stays
    assert blk.set_window([]) is True
    ref = fr.fft_vfc(x, N)
    assert np.abs(blk.work(1, x) - ref).max() <= 1e-6 * np.log2(N) * np.abs(ref).max()
