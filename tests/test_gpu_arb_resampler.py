"""-m gpu: gr_pfb_arb_resampler_ccf / _fff on the device against the call-by-call restatement
(tests/arb_resampler_ref.py): GRHIP_MODE_GENERIC bit for bit, FAST within 1e-5 of the output peak, the block
contract (first call, history, forecast, call sizes, set_rate), the device entries, bad arguments, and the C++
block under the stand-in executor."""
import os
import subprocess

import numpy as np
import pytest

import arb_resampler_ref as ar
from conftest import rel_err_max

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")

RATES = [0.0192, 0.3, 0.5, 0.999, 1.0, 1.25, 2.5]


def _blk(g, cplx, rate, taps, R, mode):
    b = (g.pfb_arb_resampler_ccf if cplx else g.pfb_arb_resampler_fff)(rate, taps, R)
    b.set_mode(mode)
    return b


def _signal(rng, n, cplx):
    x = rng.standard_normal(n).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.standard_normal(n)).astype(np.complex64)
    return x


def _whole_ref(rate, taps, R, x, f64=False):
    tpf, fwd, dfwd = ar.banks(taps, R)
    counts, js, accs = ar.whole_stream_schedule(R, rate, len(x))
    buf = np.concatenate([np.zeros(tpf, dtype=x.dtype), x])
    return ar.eval_schedule(fwd, dfwd, buf, counts, js, accs, f64=f64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _n_samples(rate, cap=20000):
    return int(max(64, min(3000, cap / rate)))


def _shapes():
    out = []
    for R in (1, 2, 32, 50, 128):
        for tpf in (1, 5, 64):
            if R * (tpf | 1) > 4096:
                tpf = 4096 // R - (1 if (4096 // R) % 2 == 0 else 0)
            ntaps = max(2, R * tpf - (R // 3))        # mostly not a multiple of R
            for rate in RATES + [R - 0.1]:
                if rate > 0:
                    out.append((R, rate, ntaps))
    out += [(4, 5.3, 13), (1, 1.5, 7), (4, 5.3, 40), (1, 1.5, 1)]     # the rounding regime
    return sorted(set(o for o in out if o[2] >= 2))


@pytest.mark.parametrize("cplx", [True, False], ids=["ccf", "fff"])
def test_generic_bit_exact_sweep(gpu, cplx):
    g = gpu
    rng = np.random.default_rng(1 if cplx else 2)
    bad = []
    for R, rate, ntaps in _shapes():
        taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        x = _signal(rng, _n_samples(rate), cplx)
        ref = _whole_ref(rate, taps, R, x)
        blk = _blk(g, cplx, rate, taps, R, g.MODE_GENERIC)
        got = ar.run_calls(blk, x, [(len(ref) + 16, None)])
        if len(got) != len(ref) or not np.array_equal(_bits(got), _bits(ref)):
            bad.append((R, rate, ntaps, len(got), len(ref)))
    assert not bad, bad


@pytest.mark.parametrize("cplx", [True, False], ids=["ccf", "fff"])
def test_fast_within_tolerance(gpu, cplx):
    g = gpu
    rng = np.random.default_rng(5)
    for R, rate, ntaps in [(32, 0.5, 32 * 16), (32, 1.25, 32 * 16 - 7), (32, 0.0192, 32 * 8), (50, 49.9, 120),
                           (4, 5.3, 13), (128, 0.3, 128 * 31), (1, 1.5, 64)]:
        taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        x = _signal(rng, _n_samples(rate), cplx)
        ref = _whole_ref(rate, taps, R, x)
        ref64 = _whole_ref(rate, taps, R, x, f64=True)
        blk = _blk(g, cplx, rate, taps, R, g.MODE_FAST)
        got = ar.run_calls(blk, x, [(len(ref) + 16, None)])
        assert len(got) == len(ref)
        assert rel_err_max(got, ref) < 1e-5, (R, rate)
        assert rel_err_max(got, ref64) < 1e-5, (R, rate)


def test_fast_modes_are_one_kernel(gpu):
    g = gpu
    rng = np.random.default_rng(6)
    taps = rng.standard_normal(300).astype(np.float32)
    x = _signal(rng, 2000, True)
    outs = []
    for m in (g.MODE_FAST, g.MODE_FAST_VALU, g.MODE_FAST_REFTAPS):
        outs.append(ar.run_calls(_blk(g, True, 0.7, taps, 32, m), x, [(5000, None)]))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(outs[2]))


@pytest.mark.parametrize("cplx", [True, False], ids=["ccf", "fff"])
def test_first_call_history_forecast(gpu, cplx):
    g = gpu
    taps = np.arange(1, 32 * 9 - 4, dtype=np.float32)
    blk = _blk(g, cplx, 0.5, taps, 32, g.MODE_GENERIC)
    tpf = 9
    assert blk.taps_per_filter() == tpf
    assert blk.history() == tpf + 1
    assert blk.forecast(100) == 100 + tpf and blk.forecast(0) == tpf
    x = np.ones(500, np.complex64 if cplx else np.float32)
    out, consumed = blk.general_work(100, x)
    assert len(out) == 0 and consumed == 0
    out, consumed = blk.general_work(100, x)
    assert len(out) == 100 and consumed > 0
    blk.set_rate(0.25)                      # set_rate does not make the next call return 0
    out, consumed = blk.general_work(10, x)
    assert len(out) == 10


@pytest.mark.parametrize("R,rate,ntaps,cplx", [(32, 0.5, 32 * 8 - 5, True), (32, 0.0192, 32 * 16, False),
                                               (32, 1.25, 32 * 4 + 3, True), (4, 5.3, 13, False),
                                               (50, 49.9, 150, True)])
def test_call_sizes_concatenate_to_whole_stream(gpu, R, rate, ntaps, cplx):
    g = gpu
    rng = np.random.default_rng(ntaps)
    taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    N = 70000 if rate < 2 else 1500
    x = _signal(rng, N, cplx)
    ref = _whole_ref(rate, taps, R, x)
    rnd = [(int(a), int(b)) for a, b in zip(rng.integers(1, 5000, 40), rng.integers(1, 9000, 40))]
    rest = [(1 << 20, None)]
    for sizes in ([(1, None)] * 300 + rest, [(7, None)] * 200 + [(1, 40)] * 50 + rest, [(4096, None)],
                  [(65536, None)], rnd + rest):
        got = ar.run_calls(_blk(g, cplx, rate, taps, R, g.MODE_GENERIC), x, sizes)
        assert len(got) == len(ref) and np.array_equal(_bits(got), _bits(ref)), sizes[:3]


@pytest.mark.parametrize("cplx", [True, False], ids=["ccf", "fff"])
def test_set_rate_between_calls(gpu, cplx):
    g = gpu
    rng = np.random.default_rng(21)
    taps = (rng.standard_normal(200) / 14).astype(np.float32)
    x = _signal(rng, 30000, cplx)
    plan = [(0.7, 3000, 5000), (1.9, 2000, 3000), (0.05, 10, 9000), (4.0, 4000, 1000), (33.5, 3000, 200),
            (0.999, 6000, None)]
    outs = []
    for blk in (ar.ArbResamplerRef(0.7, taps, 32, cplx), _blk(g, cplx, 0.7, taps, 32, g.MODE_GENERIC)):
        buf = np.concatenate([np.zeros(blk.history() - 1, dtype=x.dtype), x])
        rd, res = 0, []
        blk.general_work(10, buf)           # the first call's 0
        for rate, nout, ncap in plan:
            blk.set_rate(rate)
            nin = len(buf) - rd if ncap is None else min(ncap, len(buf) - rd)
            out, consumed = blk.general_work(nout, buf[rd:rd + nin])
            res.append(np.asarray(out))
            rd += consumed
        outs.append(np.concatenate(res))
    assert len(outs[0]) > 1000 and len(outs[0]) == len(outs[1])
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("mode", ["FAST", "GENERIC"])
@pytest.mark.parametrize("cplx", [True, False], ids=["ccf", "fff"])
def test_device_entries_equal_host_path(gpu, cplx, mode):
    g = gpu
    torch = _torch()
    m = getattr(g, "MODE_" + mode)
    rng = np.random.default_rng(8)
    taps = (rng.standard_normal(32 * 16) / 22).astype(np.float32)
    dt = np.complex64 if cplx else np.float32
    w = 2 if cplx else 1
    st = torch.cuda.Stream()
    for rate in (0.5, 1.25, 0.0192, 40.3):
        n_streams, N, stride = 3, 50000 if rate < 2 else 800, 60001
        caps = [_signal(rng, N, cplx) for _ in range(n_streams)]
        host = [ar.run_calls(_blk(g, cplx, rate, taps, 32, m), c, [(1 << 20, None)]) for c in caps]
        blk = _blk(g, cplx, rate, taps, 32, m)
        n_out = blk.captures_nout(N)
        assert all(len(h) == n_out for h in host)
        d_in = torch.zeros(n_streams * stride * w, dtype=torch.float32, device="cuda")
        for s, c in enumerate(caps):
            d_in[s * stride * w:(s * stride + N) * w] = torch.from_numpy(c.view(np.float32).copy()).cuda()
        ostride = n_out + 5
        d_out = torch.zeros(n_streams * ostride * w, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert blk.run_captures_device(n_streams, N, d_in, stride, d_out, ostride, stream=st) == n_out
        st.synchronize()
        got = d_out.cpu().numpy().view(dt)
        for s in range(n_streams):
            assert np.array_equal(_bits(got[s * ostride:s * ostride + n_out]), _bits(host[s])), (rate, s)
        # general_work_device on the first capture, history zeros in front, irregular calls, on the torch stream
        tpf = blk.taps_per_filter()
        buf = np.concatenate([np.zeros(tpf, dt), caps[0]])
        d_buf = torch.from_numpy(buf.view(np.float32).copy()).cuda()
        d_o = torch.zeros((n_out + 16) * w, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        blk2 = _blk(g, cplx, rate, taps, 32, m)
        rd, produced, calls = 0, 0, 0
        sizes = [(1000, 7000), (3, 50), (70000, None), (1, None)]
        while True:
            assert calls < 200000
            nout, ncap = sizes[calls % len(sizes)]
            calls += 1
            avail = len(buf) - rd
            nin = avail if ncap is None else min(avail, ncap)
            nout = min(nout, n_out + 16 - produced)
            n, c = blk2.general_work_device(nout, nin, d_buf[rd * w:].data_ptr(), d_o[produced * w:].data_ptr(),
                                            stream=st)
            produced += n
            rd += c
            if calls > 2 and n == 0 and c == 0 and nin == avail:
                break
        st.synchronize()
        assert produced == n_out
        assert np.array_equal(_bits(d_o.cpu().numpy().view(dt)[:n_out]), _bits(host[0])), rate


@pytest.mark.parametrize("mode", ["FAST", "GENERIC"])
def test_capture_past_float_precision(gpu, mode):
    """a capture of more than 2^24 samples: exact 64-bit positions in run_captures_device against host-path calls
    of at most 2^22 items (where the reference's float count is exact)"""
    g = gpu
    torch = _torch()
    m = getattr(g, "MODE_" + mode)
    rng = np.random.default_rng(9)
    taps = (rng.standard_normal(32 * 8) / 16).astype(np.float32)
    N = (1 << 24) + 12345
    x = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)
    host = ar.run_calls(_blk(g, True, 0.5, taps, 32, m), x, [(1 << 21, 1 << 22)])
    blk = _blk(g, True, 0.5, taps, 32, m)
    n_out = blk.captures_nout(N)
    assert len(host) == n_out > (1 << 23)
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_out = torch.zeros(2 * n_out, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    blk.run_captures_device(1, N, d_in, N, d_out, n_out)
    g.lib().grhip_device_synchronize(0)
    got = d_out.cpu().numpy().view(np.complex64)
    assert np.array_equal(_bits(got), _bits(host))
    if mode == "GENERIC":
        tail = slice(n_out - 3000, n_out)
        counts, js, accs = ar.closed_form_schedule(32, 0.5, n_out)
        buf = np.concatenate([np.zeros(8, np.complex64), x])
        ref = ar.eval_schedule(*ar.banks(taps, 32)[1:], buf, counts[tail], js[tail], accs[tail])
        assert counts[-1] < N <= ar.closed_form_schedule(32, 0.5, n_out + 1)[0][-1]
        assert np.array_equal(_bits(got[tail]), _bits(ref))


def test_bad_arguments_einval(gpu):
    g = gpu
    L = g.lib()
    taps = np.ones(64, np.float32)
    blk = g.pfb_arb_resampler_ccf(0.5, taps, 32)
    for rate in (0.0, -2.0, float("nan"), float("inf"), 32 / 2.0 ** 21):
        with pytest.raises(g.GrhipError) as e:
            blk.set_rate(rate)
        assert e.value.code == -1
    with pytest.raises(g.GrhipError) as e:
        blk.set_mode(7)
    assert e.value.code == -1
    with pytest.raises(g.GrhipError) as e:
        blk.forecast(-1)
    assert e.value.code == -1
    x = np.zeros(100, np.complex64)
    out = np.zeros(100, np.complex64)
    assert L.grhip_pfb_arb_resampler_ccf_general_work(blk._h, 10, 100, x.ctypes.data, out.ctypes.data, None) == -1
    with pytest.raises(g.GrhipError) as e:
        blk.general_work(-1, x)
    assert e.value.code == -1
    with pytest.raises(g.GrhipError) as e:          # strides shorter than the capture
        blk.run_captures_device(2, 1000, 1, 10, 1, 10)
    assert e.value.code == -1
    for cls in (g.pfb_arb_resampler_ccf, g.pfb_arb_resampler_fff):
        for args in ((0.5, [], 32), (0.5, [1.0], 32), (0.5, taps, 0), (0.0, taps, 32), (-1.0, taps, 32),
                     (float("nan"), taps, 32), (0.5, np.ones(4097, np.float32), 1)):
            with pytest.raises(g.GrhipError) as e:
                cls(*args)
            assert e.value.code == -1, args
    # the blocks' limits hold exactly at their edges
    g.pfb_arb_resampler_fff(0.5, np.ones(4064, np.float32), 32)            # 32 * (127 | 1) = 4064 pairs
    g.pfb_arb_resampler_fff(0.5, np.ones(4095, np.float32), 1)             # 1 * 4095


@pytest.fixture(scope="module")
def arb_exe(gpu):
    exe = os.path.join(HOST, "arb_resampler_test")
    subprocess.check_call(["make", "-C", HOST, "arb_resampler_test"], stdout=subprocess.DEVNULL)
    return exe


@pytest.mark.parametrize("cplx,rate", [(True, 0.5), (False, 1.25), (True, 0.0192), (False, 5.3)])
def test_cpp_block_under_executor(gpu, arb_exe, tmp_path, cplx, rate):
    g = gpu
    rng = np.random.default_rng(12)
    R = 32 if rate < 5 else 4
    taps = (rng.standard_normal(R * 12 - 3) / 20).astype(np.float32)
    x = _signal(rng, 300_000 if rate < 5 else 20_000, cplx)
    x.tofile(tmp_path / "x.bin")
    taps.tofile(tmp_path / "taps.f32")
    r = subprocess.run([arb_exe, "ccf" if cplx else "fff", repr(rate), str(R), "generic", str(tmp_path / "taps.f32"),
                        str(tmp_path / "x.bin"), str(tmp_path / "y.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(tmp_path / "y.bin", dtype=np.complex64 if cplx else np.float32)
    ref = ar.run_calls(_blk(g, cplx, rate, taps, R, g.MODE_GENERIC), x, [(1 << 16, None)])
    assert len(got) == len(ref) > 0 and np.array_equal(_bits(got), _bits(ref))
    r = subprocess.run([arb_exe, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("mode", ["GENERIC", "FAST"])
def test_walked_schedule_in_small_tiles(gpu, mode):
    """rate > filter_size with 4000 taps per filter: the span of a 1024-output tile (~683 + 4000 items) exceeds the
    4096 complex items of the LDS image, so the walked schedule's tiles are halved down to 128"""
    g = gpu
    torch = _torch()
    m = getattr(g, "MODE_" + mode)
    rng = np.random.default_rng(31)
    taps = (rng.standard_normal(4000) / 64).astype(np.float32)
    x = _signal(rng, 1500, True)
    ref = _whole_ref(1.5, taps, 1, x)
    got = ar.run_calls(_blk(g, True, 1.5, taps, 1, m), x, [(len(ref) + 16, None)])
    assert len(got) == len(ref) > 2000
    if mode == "GENERIC":
        assert np.array_equal(_bits(got), _bits(ref))
    else:
        assert rel_err_max(got, ref) < 1e-5
    blk = _blk(g, True, 1.5, taps, 1, m)
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_out = torch.zeros(2 * len(ref), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert blk.run_captures_device(1, len(x), d_in, len(x), d_out, len(ref)) == len(ref)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_out.cpu().numpy().view(np.complex64)), _bits(got))


def test_acc_off_grid_after_set_rate(gpu):
    """a call at rate > filter_size that leaves acc off the 2^-23 grid: the later calls at rate <= filter_size take the
    walked schedule, here with D = 640 (tiles of 1024 outputs would span 20 K items: halved until they fit)"""
    g = gpu
    rng = np.random.default_rng(41)
    taps = (rng.standard_normal(32 * 64) / 45).astype(np.float32)
    x = _signal(rng, 120000, True)
    nout1 = None
    for n in range(1, 400):                 # a first call length whose end leaves acc off the grid
        r = ar.ArbResamplerRef(33.5, taps, 32, True)
        r.schedule_call(1, 100)
        r.schedule_call(n, 100000)
        a = float(r.d_acc) * 2 ** 23
        if a != np.floor(a):
            nout1 = n
            break
    assert nout1 is not None
    outs = []
    for blk in (ar.ArbResamplerRef(33.5, taps, 32, True), _blk(g, True, 33.5, taps, 32, g.MODE_GENERIC)):
        buf = np.concatenate([np.zeros(blk.history() - 1, np.complex64), x])
        blk.general_work(1, buf[:100])      # the first call's 0
        out, rd = blk.general_work(nout1, buf[:100000])
        res = [np.asarray(out)]
        blk.set_rate(0.05)
        for nout in (3000, 1, 2500):
            out, consumed = blk.general_work(nout, buf[rd:])
            res.append(np.asarray(out))
            rd += consumed
        outs.append(np.concatenate(res))
    assert len(outs[0]) == len(outs[1]) > 5000
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
