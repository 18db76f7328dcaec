"""GPU tests of the real-input FIR kinds: gr_fir_filter_fcc / _scc / _fsf and gr_freq_xlating_fir_filter_{ccf,fcf,
fcc,scf,scc}.  GENERIC is bit-exact against the references of tests/realin_ref.py, FAST within 1e-5 (fsf: 1 LSB)."""
import numpy as np
import pytest

import realin_ref as rr
from conftest import bits_equal, rel_err_max

TOL = 1e-5
TAPS = [1, 2, 3, 7, 64, 255, 1024]
DECIMS = [1, 2, 3, 4, 8, 10]


def _cls(g, kind):
    return getattr(g, "fir_filter_" + kind)


def _data(kind, ntaps, n_items, seed, full_scale=False):
    rng = np.random.default_rng(seed)
    if kind == "fsf":
        taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    else:
        taps = ((rng.standard_normal(ntaps) + 1j * rng.standard_normal(ntaps)) / np.sqrt(ntaps)).astype(np.complex64)
    if kind == "scc" or kind.startswith("s"):
        if full_scale:
            x = rng.choice(np.array([-32768, 32767], np.int16), n_items)
        else:
            x = rng.integers(-32768, 32768, n_items).astype(np.int16)
    else:
        x = rng.standard_normal(n_items).astype(np.float32)
        if kind == "fsf":
            x *= 3000
    return taps, x


def _ref(po, kind, taps, x, n, decim):
    return rr.fsf_ref(po, taps, x, n, decim) if kind == "fsf" else rr.fcc_ref(po, taps, x, n, decim)


def _close(got, ref, kind):
    if kind == "fsf":
        d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
        return int(d.max()) <= 1
    if rel_err_max(got, ref) > TOL:
        return False
    big = np.abs(ref) > 0.1 * np.abs(ref).max()
    return bool(np.all(np.abs(got[big] - ref[big]) <= TOL * np.abs(ref[big])))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fcc", "scc", "fsf"])
def test_generic_bit_exact(gpu, po, kind):
    for ntaps in TAPS:
        for decim in DECIMS:
            n = 1100
            taps, x = _data(kind, ntaps, n * decim + ntaps - 1, ntaps * 100 + decim)
            blk = _cls(gpu, kind)(decim, taps)
            blk.set_mode(gpu.MODE_GENERIC)
            assert blk.history() == ntaps and blk.decimation() == decim
            got = blk.work(n, x)
            assert bits_equal(got, _ref(po, kind, taps, x, n, decim)), (kind, ntaps, decim)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fcc", "scc", "fsf"])
def test_fast_tolerance_and_chunking(gpu, po, kind):
    for ntaps in [1, 7, 64, 255, 1024]:
        for decim in [1, 2, 4, 8, 3]:
            n = 20000
            taps, x = _data(kind, ntaps, n * decim + ntaps - 1, ntaps * 7 + decim)
            x[:ntaps - 1] = 0                                           # the history run_sync_block puts in front
            if kind == "fsf":
                taps = np.full(ntaps, 1.0 / ntaps, np.float32)          # outputs inside the int16 range
            blk = _cls(gpu, kind)(decim, taps)
            blk.set_mode(gpu.MODE_FAST)
            got = blk.work(n, x)
            ref = _ref(po, kind, taps, x, n, decim)
            assert _close(got, ref, kind), (kind, ntaps, decim)
            raw = x[ntaps - 1:]
            for chunk in (1000, 4096):
                y = gpu.run_sync_block(blk, raw, chunk=chunk)
                # (fsf's float engines may be the overlap-save one, whose blocks follow the calls: 1 LSB)
                assert bits_equal(y, got) if kind != "fsf" else _close(y, ref, kind), (kind, ntaps, decim, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fcc", "scc", "fsf"])
def test_set_taps_returns_zero_once_and_filterNdec(gpu, po, kind):
    taps, x = _data(kind, 40, 4000, 5)
    taps2, _ = _data(kind, 25, 10, 6)
    for mode in (gpu.MODE_GENERIC, gpu.MODE_FAST):
        blk = _cls(gpu, kind)(2, taps)
        blk.set_mode(mode)
        blk.set_taps(taps2)
        assert len(blk.work(100, x)) == 0
        assert blk.history() == 25
        got = blk.work(100, x)
        ref = _ref(po, kind, taps2, x, 100, 2)
        assert bits_equal(got, ref) if mode == gpu.MODE_GENERIC else _close(got, ref, kind)
        # kernel-level seam: another decimation runs the generic order; the handle's own may run FAST
        assert bits_equal(blk.filterNdec(x, 500, 3), _ref(po, kind, taps2, x, 500, 3))
        assert _close(blk.filterNdec(x, 500, 2), _ref(po, kind, taps2, x, 500, 2), kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fcc", "scc"])
@pytest.mark.parametrize("decim", [1, 4, 8])
def test_work_device_unaligned_offsets(gpu, po, kind, decim):
    import torch
    ntaps, n = 129, 30000
    taps, x = _data(kind, ntaps, n * decim + ntaps + 16, 11 + decim)
    dx = torch.from_numpy(x).cuda()
    out = torch.zeros(n, dtype=torch.complex64, device="cuda")
    for mode in (gpu.MODE_FAST, gpu.MODE_GENERIC):
        blk = _cls(gpu, kind)(decim, taps)
        blk.set_mode(mode)
        for off in range(1, 8):
            ref = _ref(po, kind, taps, x[off:], n, decim)
            assert blk.work_device(n, dx[off:].data_ptr(), out.data_ptr()) == n
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert (bits_equal(got, ref) if mode == gpu.MODE_GENERIC else _close(got, ref, kind)), (mode, off)


@pytest.mark.gpu
def test_full_scale_int16(gpu, po):
    for decim in (1, 4):
        taps, x = _data("scc", 64, 5000 * decim + 63, 3, full_scale=True)
        for mode in (gpu.MODE_GENERIC, gpu.MODE_FAST):
            blk = gpu.fir_filter_scc(decim, taps)
            blk.set_mode(mode)
            got, ref = blk.work(5000, x), rr.fcc_ref(po, taps, x, 5000, decim)
            assert bits_equal(got, ref) if mode == gpu.MODE_GENERIC else _close(got, ref, "scc")


@pytest.mark.gpu
@pytest.mark.parametrize("decim", [1, 2, 4, 8, 3])
def test_nan_guarded_tail(gpu, po, decim):
    """exactly the items the scheduler guarantees ((n-1)*decim + ntaps), then NaNs: nothing past them is read"""
    import torch
    ntaps, n = 255, 9000
    taps, x = _data("fcc", ntaps, (n - 1) * decim + ntaps, 21)
    ref = rr.fcc_ref(po, taps, x, n, decim)
    buf = np.concatenate([x, np.full(decim + 64, np.nan, np.float32)])
    dx = torch.from_numpy(buf).cuda()
    out = torch.zeros(n, dtype=torch.complex64, device="cuda")
    blk = gpu.fir_filter_fcc(decim, taps)
    assert blk.work_device(n, dx.data_ptr(), out.data_ptr()) == n
    torch.cuda.synchronize()                            # (the handle's own stream)
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and _close(got, ref, "fcc")
    xl = gpu.freq_xlating_fir_filter_fcc(decim, taps, 1500.0, 48000.0)
    assert xl.work_device(n, dx.data_ptr(), out.data_ptr()) == n
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    xref = rr.XlatingRef(po, decim, taps, 1500.0, 48000.0).work(x, n)
    assert np.isfinite(got).all() and _close(got, xref, "fcc")


# ---- freq_xlating_fir_filter_{ccf,fcf,fcc,scf,scc} ----

XKINDS = ["ccf", "fcf", "fcc", "scf", "scc"]


def _xdata(kind, ntaps, n_items, seed):
    rng = np.random.default_rng(seed)
    proto = (np.sinc(0.05 * (np.arange(ntaps) - (ntaps - 1) / 2)) * 0.05).astype(np.float32)
    if kind.endswith("cc"):
        proto = (proto * np.exp(0.3j * np.arange(ntaps))).astype(np.complex64)
    if kind[0] == "s":
        x = rng.integers(-32768, 32768, n_items).astype(np.int16)
    elif kind[0] == "f":
        x = rng.standard_normal(n_items).astype(np.float32)
    else:
        x = (rng.standard_normal(n_items) + 1j * rng.standard_normal(n_items)).astype(np.complex64)
    return proto, x


@pytest.mark.gpu
@pytest.mark.parametrize("kind", XKINDS)
@pytest.mark.parametrize("decim,ntaps", [(4, 256), (1, 31), (3, 100), (8, 1024), (10, 7)])
def test_xlating_generic_bit_exact_chunked(gpu, po, kind, decim, ntaps):
    fc, fs = 3211.0, 48000.0
    nout = 1700                                        # rotator renormalises every 512 outputs
    proto, x = _xdata(kind, ntaps, nout * decim, decim * 1000 + ntaps)
    xin = np.concatenate([np.zeros(ntaps - 1, x.dtype), x])
    ref = rr.XlatingRef(po, decim, proto, fc, fs).work(xin, nout)
    blk = getattr(gpu, "freq_xlating_fir_filter_" + kind)(decim, proto, fc, fs)
    blk.set_mode(gpu.MODE_GENERIC)
    assert bits_equal(blk.work(nout, xin), ref)
    blk.reset()
    assert bits_equal(gpu.run_sync_block(blk, x, chunk=333), ref)
    blk.reset()
    blk.set_mode(gpu.MODE_FAST)
    got = gpu.run_sync_block(blk, x, chunk=1000)
    assert rel_err_max(got, ref) <= TOL, (kind, decim, ntaps)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", XKINDS)
def test_xlating_fast_tolerance(gpu, po, kind):
    fc, fs = 2500.0, 48000.0
    for decim, ntaps in [(4, 256), (1, 64), (2, 128), (8, 1024)]:
        nout = 200_000 // decim
        proto, x = _xdata(kind, ntaps, nout * decim, 5)
        xin = np.concatenate([np.zeros(ntaps - 1, x.dtype), x])
        ref = rr.XlatingRef(po, decim, proto, fc, fs).work(xin, nout)
        blk = getattr(gpu, "freq_xlating_fir_filter_" + kind)(decim, proto, fc, fs)
        blk.set_mode(gpu.MODE_FAST)
        got = blk.work(nout, xin)
        assert _close(got, ref, kind), (kind, decim, ntaps)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", XKINDS)
def test_xlating_set_center_freq_keeps_phase(gpu, kind):
    """the family handle against the _ccc handle on widened input, through set_center_freq / set_taps"""
    decim, ntaps = 4, 64
    proto, x = _xdata(kind, ntaps, 40000, 9)
    xc = x.astype(np.complex64)
    a = getattr(gpu, "freq_xlating_fir_filter_" + kind)(decim, proto, 1000.0, 48000.0)
    b = gpu.freq_xlating_fir_filter_ccc(decim, np.asarray(proto).astype(np.complex64), 1000.0, 48000.0)
    for blk in (a, b):
        blk.set_mode(gpu.MODE_GENERIC)
    xin, xcin = np.concatenate([np.zeros(ntaps - 1, x.dtype), x]), np.concatenate([np.zeros(ntaps - 1, np.complex64), xc])
    pos = 0
    for step, n in enumerate([777, 1300, 2000, 900]):
        if step == 1:
            a.set_center_freq(-7000.0); b.set_center_freq(-7000.0)
        if step == 3:
            a.set_taps(proto[::-1].copy()); b.set_taps(np.asarray(proto[::-1]).astype(np.complex64))
        if step in (1, 3):
            assert len(a.work(n, xin[pos:])) == 0 and len(b.work(n, xcin[pos:])) == 0
        ya, yb = a.work(n, xin[pos:]), b.work(n, xcin[pos:])
        assert bits_equal(ya, yb), step
        pos += n * decim


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["GENERIC", "FAST"])
def test_xlating_ccc_kind_equals_ccc_handle(gpu, mode):
    class fam_ccc(gpu.binding._freq_xlating_fir_filter):
        _kind = "ccc"
        _tap = np.complex64

    rng = np.random.default_rng(2)
    for decim, ntaps in [(4, 256), (3, 50), (1, 17)]:
        proto = (rng.standard_normal(ntaps) + 1j * rng.standard_normal(ntaps)).astype(np.complex64) / ntaps
        x = (rng.standard_normal(60000) + 1j * rng.standard_normal(60000)).astype(np.complex64)
        a, b = fam_ccc(decim, proto, 1111.0, 48000.0), gpu.freq_xlating_fir_filter_ccc(decim, proto, 1111.0, 48000.0)
        for blk in (a, b):
            blk.set_mode(getattr(gpu, "MODE_" + mode))
        assert bits_equal(gpu.run_sync_block(a, x, chunk=4096), gpu.run_sync_block(b, x, chunk=4096))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fcf", "fcc"])
def test_xlating_generic_nonfinite_positions(gpu, po, kind):
    decim, ntaps, nout = 2, 33, 3000
    proto, x = _xdata(kind, ntaps, nout * decim, 13)
    x[[100, 2000, 4100]] = [np.nan, np.inf, -np.inf]
    xin = np.concatenate([np.zeros(ntaps - 1, x.dtype), x])
    ref = rr.xlating_direct(po, decim, proto, 900.0, 48000.0, xin, nout)
    blk = getattr(gpu, "freq_xlating_fir_filter_" + kind)(decim, proto, 900.0, 48000.0)
    blk.set_mode(gpu.MODE_GENERIC)
    got = blk.work(nout, xin)
    for part in ("real", "imag"):
        g_, r_ = getattr(got, part), getattr(ref, part)
        assert np.array_equal(np.isnan(g_), np.isnan(r_))
        fin = ~np.isnan(r_)
        assert np.array_equal(g_[fin].view(np.uint32), r_[fin].view(np.uint32))
    assert np.isnan(got.real).any()


@pytest.mark.gpu
def test_cpp_blocks_and_seams(gpu):
    """host/xlating_test: every new block under the stand-in executor and the gr_fir_{fcc,scc,fsf}_hip seams,
    GENERIC, against its x86-64 restatement of the reference's generic code"""
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnuradio-3.5.0-dmr_amd", "host")
    r = subprocess.run(["make", "-C", host, "xlating_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([os.path.join(host, "xlating_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0 and "all ok" in r.stdout, r.stdout
