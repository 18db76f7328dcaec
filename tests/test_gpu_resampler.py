"""-m gpu: gr_rational_resampler_base_XXX and gr_interp_fir_filter_XXX (ccf, fff, ccc) on the device against the
restatements of tests/resampler_ref.py: GRHIP_MODE_GENERIC bit for bit, FAST within 1e-5 of the output peak, the block
contract (call sizes with ctr carried, set_taps, history, forecast, output_multiple), the device entries, a capture
past 2^32 positions, bad arguments, blks2.rational_resampler_ccf and the C++ blocks under the stand-in executor."""
import os
import subprocess

import numpy as np
import pytest

import resampler_ref as rr
from conftest import rel_err_max

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")

KINDS = ["ccf", "fff", "ccc"]
RATES = [(1, 1), (1, 3), (2, 1), (3, 2), (2, 3), (4, 1), (5, 7), (160, 147)]


def _dt(kind):
    return np.float32 if kind == "fff" else np.complex64


def _taps(rng, kind, n):
    t = (rng.standard_normal(n) / np.sqrt(n)).astype(np.float32)
    if kind == "ccc":
        t = (t + 1j * rng.standard_normal(n) / np.sqrt(n)).astype(np.complex64)
    return t


def _signal(rng, kind, n):
    x = rng.standard_normal(n).astype(np.float32)
    if kind != "fff":
        x = (x + 1j * rng.standard_normal(n)).astype(np.complex64)
    return x


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rs(g, kind, I, D, taps, mode):
    b = getattr(g, "rational_resampler_base_" + kind)(I, D, taps)
    b.set_mode(mode)
    return b


def _ip(g, kind, I, taps, mode):
    b = getattr(g, "interp_fir_filter_" + kind)(I, taps)
    b.set_mode(mode)
    return b


def _tap_counts(I):
    return sorted({1, 3 * I - 1, 101 * I} if I > 1 else {1, 7, 101})


def _n_in(I, D, nt):
    return int(min(6000, max(400, 1500 * D // I))) + nt


@pytest.mark.parametrize("kind", KINDS)
def test_rational_generic_bit_exact(gpu, po, kind):
    g = gpu
    rng = np.random.default_rng(1)
    bad = []
    for I, D in RATES:
        for ntaps in _tap_counts(I):
            taps = _taps(rng, kind, ntaps)
            nt = rr.bank(taps, I)[0]
            x = _signal(rng, kind, _n_in(I, D, nt))
            ref = rr.whole_rational(po, I, D, taps, x)
            n = len(ref)
            while (n * D) // I > len(x):                   # one call may not consume more than it is given
                n -= 1
            out, consumed = _rs(g, kind, I, D, taps, g.MODE_GENERIC).general_work(n, x)
            if len(out) != n or not np.array_equal(_bits(out), _bits(ref[:n])):
                bad.append((I, D, ntaps))
            assert consumed == (n * D) // I
    assert not bad, bad


@pytest.mark.parametrize("kind", KINDS)
def test_interp_generic_bit_exact(gpu, po, kind):
    g = gpu
    rng = np.random.default_rng(2)
    bad = []
    for I in (1, 2, 3, 4, 5, 160):
        for ntaps in _tap_counts(I):
            taps = _taps(rng, kind, ntaps)
            x = _signal(rng, kind, 700)
            ref = rr.whole_interp(po, I, taps, x)
            blk = _ip(g, kind, I, taps, g.MODE_GENERIC)
            buf = np.concatenate([np.zeros(blk.history() - 1, x.dtype), x])
            out = blk.work(I * len(x), buf)
            if len(out) != len(ref) or not np.array_equal(_bits(out), _bits(ref)):
                bad.append((I, ntaps))
    assert not bad, bad


@pytest.mark.parametrize("kind", KINDS)
def test_fast_within_tolerance(gpu, po, kind):
    g = gpu
    rng = np.random.default_rng(3)
    for I, D in RATES:
        taps = _taps(rng, kind, 101 * I)
        x = _signal(rng, kind, _n_in(I, D, 101))
        ref = rr.whole_rational(po, I, D, taps, x)
        out, _ = _rs(g, kind, I, D, taps, g.MODE_FAST).general_work(len(ref), x)
        assert len(out) == len(ref) and rel_err_max(out, ref) < 1e-5, (I, D)
    for I in (1, 4, 5, 160):
        taps = _taps(rng, kind, 16 * I - 3)
        x = _signal(rng, kind, 900)
        ref = rr.whole_interp(po, I, taps, x)
        blk = _ip(g, kind, I, taps, g.MODE_FAST)
        out = blk.work(I * len(x), np.concatenate([np.zeros(blk.history() - 1, x.dtype), x]))
        assert rel_err_max(out, ref) < 1e-5, I
    outs = [_rs(g, kind, 3, 2, taps[:303], m).general_work(500, x)[0]
            for m in (g.MODE_FAST, g.MODE_FAST_VALU, g.MODE_FAST_REFTAPS)]
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(outs[2]))


def _drive_rational(blk, x, sizes):
    """scheduler-style calls: n outputs from `sizes` (cycled), shrunk until the call's reads fit the input left"""
    rd, outs, k = 0, [], 0
    while True:
        n = sizes[k % len(sizes)]
        k += 1
        I, D, nt = blk.interpolation(), blk.decimation(), blk.history()
        ctr = blk._ctr if hasattr(blk, "_ctr") else None
        left = len(x) - rd
        while n > 0 and not _fits(I, D, nt, ctr, n, left):
            n -= 1
        if n == 0:
            break
        out, c = blk.general_work(n, x[rd:])
        blk._ctr = (blk._ctr + n * D) % I
        outs.append(out)
        rd += c
    return np.concatenate(outs) if outs else np.zeros(0, x.dtype)


def _fits(I, D, nt, ctr, n, left):
    return (ctr + (n - 1) * D) // I + nt <= left and (ctr + n * D) // I <= left


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("I,D", [(3, 2), (2, 3), (5, 7), (160, 147), (1, 3)])
def test_call_sizes_concatenate_with_ctr_carried(gpu, po, kind, I, D):
    g = gpu
    rng = np.random.default_rng(I * 100 + D)
    taps = _taps(rng, kind, 7 * I + 1)
    x = _signal(rng, kind, 5000)
    ref = rr.whole_rational(po, I, D, taps, x)
    for sizes in ([1] * 50 + [1 << 20], [int(v) for v in rng.integers(1, 700, 40)], [1 << 20]):
        blk = _rs(g, kind, I, D, taps, g.MODE_GENERIC)
        blk._ctr = 0
        got = _drive_rational(blk, x, sizes)
        assert len(got) == len(ref) and np.array_equal(_bits(got), _bits(ref)), sizes[:3]
    # the interpolator in calls of random multiples of I
    tp = _taps(rng, kind, 5 * I + 2)
    ref = rr.whole_interp(po, I, tp, x[:1500])
    blk = _ip(g, kind, I, tp, g.MODE_GENERIC)
    buf = np.concatenate([np.zeros(blk.history() - 1, x.dtype), x[:1500]])
    rd, outs = 0, []
    while rd < 1500:
        ni = min(1500 - rd, int(rng.integers(1, 300)))
        outs.append(blk.work(ni * I, buf[rd:rd + ni + blk.history() - 1]))
        rd += ni
    assert np.array_equal(_bits(np.concatenate(outs)), _bits(ref))


@pytest.mark.parametrize("kind", KINDS)
def test_set_taps_between_calls(gpu, po, kind):
    g = gpu
    rng = np.random.default_rng(7)
    t1, t2 = _taps(rng, kind, 13), _taps(rng, kind, 40)
    x = _signal(rng, kind, 3000)
    res = []
    for blk in (rr.RationalRef(po, 3, 2, t1), _rs(g, kind, 3, 2, t1, g.MODE_GENERIC)):
        assert blk.history() == 5
        rd, outs = 0, []
        out, c = blk.general_work(301, x)
        outs.append(out); rd += c
        blk.set_taps(t2)
        assert blk.history() == 5                           # latched: nothing changes until the next call
        out, c = blk.general_work(50, x[rd:])
        assert len(out) == 0 and c == 0                     # installs and returns 0, consuming nothing
        assert blk.history() == 14                          # ceil(40/3)
        out, c = blk.general_work(400, x[rd:])
        outs.append(out); rd += c
        res.append(np.concatenate(outs))
    assert len(res[0]) == 701 and np.array_equal(_bits(res[0]), _bits(res[1]))
    res = []
    for blk in (rr.InterpRef(po, 4, t1), _ip(g, kind, 4, t1, g.MODE_GENERIC)):
        assert blk.history() == 4
        o1 = blk.work(400, x[:100 + 3])
        blk.set_taps(t2)
        assert len(blk.work(400, x[97:97 + 103])) == 0
        assert blk.history() == 10
        o2 = blk.work(400, x[100 - 9:100 + 100])
        res.append(np.concatenate([o1, o2]))
    assert len(res[0]) == 800 and np.array_equal(_bits(res[0]), _bits(res[1]))


def test_history_forecast_output_multiple(gpu):
    g = gpu
    taps = np.ones(301, np.float32)
    for kind in KINDS:
        b = getattr(g, "rational_resampler_base_" + kind)(3, 2, taps)
        assert b.history() == 101 and b.interpolation() == 3 and b.decimation() == 2
        assert b.relative_rate() == 1.5
        for n in (0, 1, 2, 99, 1000, 4095):
            assert b.forecast(n) == rr.forecast(3, 2, 101, n)
        b = getattr(g, "rational_resampler_base_" + kind)(160, 147, np.ones(20, np.float32))
        assert b.history() == 1 and b.forecast(0) == 1 and b.forecast(159) == 147
        ip = getattr(g, "interp_fir_filter_" + kind)(4, np.ones(64, np.float32))
        assert ip.history() == 16 and ip.interpolation() == 4 and ip.output_multiple() == 4


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float32).copy()).cuda()


@pytest.mark.parametrize("mode", ["FAST", "GENERIC"])
@pytest.mark.parametrize("kind", KINDS)
def test_device_entries_equal_host_path(gpu, po, kind, mode):
    g = gpu
    torch = _torch()
    m = getattr(g, "MODE_" + mode)
    rng = np.random.default_rng(8)
    dt = _dt(kind)
    w = 1 if kind == "fff" else 2
    st = torch.cuda.Stream()
    for I, D in [(3, 2), (2, 3), (160, 147), (4, 1)]:
        taps = _taps(rng, kind, 11 * I + 2)
        S, N, stride = 3, 4001, 4099
        caps = [_signal(rng, kind, N) for _ in range(S)]
        host = [_rs(g, kind, I, D, taps, m).general_work(rr.rational_nout(I, D, 12, N), c)[0] for c in caps]
        blk = _rs(g, kind, I, D, taps, m)
        n_out = blk.captures_nout(N)
        assert n_out == len(host[0]) == rr.rational_nout(I, D, blk.history(), N)
        d_in = torch.zeros(S * stride * w, dtype=torch.float32, device="cuda")
        for s, c in enumerate(caps):
            d_in[s * stride * w:(s * stride + N) * w] = _to_dev(torch, c)
        ostride = n_out + 7
        d_out = torch.zeros(S * ostride * w, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert blk.run_captures_device(S, N, d_in, stride, d_out, ostride, stream=st) == n_out
        st.synchronize()
        got = d_out.cpu().numpy().view(dt)
        for s in range(S):
            assert np.array_equal(_bits(got[s * ostride:s * ostride + n_out]), _bits(host[s])), (I, D, s)
        # general_work_device in irregular calls on the torch stream
        blk2 = _rs(g, kind, I, D, taps, m)
        d_x = _to_dev(torch, caps[0])
        d_o = torch.zeros((n_out + 16) * w, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rd, produced, ctr, k = 0, 0, 0, 0
        sizes = [1000, 3, 777, 1]
        while True:
            n = sizes[k % 4]
            k += 1
            while n > 0 and not _fits(I, D, 12, ctr, n, N - rd):
                n -= 1
            if n == 0:
                break
            r, c = blk2.general_work_device(n, N - rd, d_x[rd * w:].data_ptr(), d_o[produced * w:].data_ptr(),
                                            stream=st)
            assert r == n and c == (ctr + n * D) // I
            ctr = (ctr + n * D) % I
            produced += r
            rd += c
        st.synchronize()
        assert produced == n_out
        assert np.array_equal(_bits(d_o.cpu().numpy().view(dt)[:n_out]), _bits(host[0])), (I, D)
    # the interpolator: fresh captures (history zeros implied) and work_device
    for I in (4, 3):
        taps = _taps(rng, kind, 16 * I)
        S, N, stride = 2, 3001, 3011
        caps = [_signal(rng, kind, N) for _ in range(S)]
        ref = [rr.whole_interp(po, I, taps, c) for c in caps]
        blk = _ip(g, kind, I, taps, m)
        d_in = torch.zeros(S * stride * w, dtype=torch.float32, device="cuda")
        for s, c in enumerate(caps):
            d_in[s * stride * w:(s * stride + N) * w] = _to_dev(torch, c)
        ostride = I * N + 5
        d_out = torch.zeros(S * ostride * w, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert blk.run_captures_device(S, N, d_in, stride, d_out, ostride, stream=st) == I * N
        st.synchronize()
        got = d_out.cpu().numpy().view(dt)
        for s in range(S):
            o = got[s * ostride:s * ostride + I * N]
            if mode == "GENERIC":
                assert np.array_equal(_bits(o), _bits(ref[s]))
            else:
                assert rel_err_max(o, ref[s]) < 1e-5
        buf = np.concatenate([np.zeros(blk.history() - 1, dt), caps[0]])
        d_b = _to_dev(torch, buf)
        d_o = torch.zeros(I * N * w, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert blk.work_device(I * N, d_b, d_o, stream=st) == I * N
        st.synchronize()
        assert np.array_equal(_bits(d_o.cpu().numpy().view(dt)), _bits(got[:I * N]))


def test_capture_past_2_32_positions(gpu, po):
    """160/147 fff: c0 + o*D passes 2^32 after 29.2 M outputs; run_captures_device keeps 64-bit positions"""
    g = gpu
    torch = _torch()
    rng = np.random.default_rng(9)
    I, D = 160, 147
    taps = _taps(rng, "fff", 2 * I)
    N = 27_500_000
    x = rng.standard_normal(N).astype(np.float32)
    blk = _rs(g, "fff", I, D, taps, g.MODE_GENERIC)
    n_out = blk.captures_nout(N)
    assert n_out == rr.rational_nout(I, D, 2, N) and (n_out - 1) * D > 2 ** 32
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros(n_out, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    blk.run_captures_device(1, N, d_in, N, d_out, n_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    nt, fwd = rr.bank(taps, I)
    for lo in (0, 29_000_000, n_out - 3000):
        p = np.arange(lo, lo + 3000, dtype=np.int64) * D
        fs, offs = p % I, p // I
        base = int(offs[0])
        ref = rr.gather(po, fwd, x[base:], fs, offs - base)
        assert np.array_equal(_bits(got[lo:lo + 3000]), _bits(ref)), lo


def test_bad_arguments(gpu):
    g = gpu
    taps = np.ones(30, np.float32)
    for cls in (g.rational_resampler_base_ccf, g.rational_resampler_base_fff):
        for args, code in (((0, 2, taps), -2), ((3, 0, taps), -2), ((3, 2, []), -1), ((1, 1000, taps), -1)):
            with pytest.raises(g.GrhipError) as e:
                cls(*args)
            assert e.value.code == code, args
    with pytest.raises(g.GrhipError) as e:
        g.interp_fir_filter_ccc(0, np.ones(3, np.complex64))
    assert e.value.code == -2
    with pytest.raises(g.GrhipError) as e:
        g.interp_fir_filter_fff(3, [])
    assert e.value.code == -1
    ip = g.interp_fir_filter_ccf(3, taps)
    with pytest.raises(g.GrhipError) as e:
        ip.work(10, np.zeros(100, np.complex64))            # not a multiple of I
    assert e.value.code == -1
    with pytest.raises(g.GrhipError) as e:
        ip.set_taps([])
    assert e.value.code == -1
    with pytest.raises(g.GrhipError) as e:
        ip.set_mode(9)
    assert e.value.code == -1
    b = g.rational_resampler_base_ccf(3, 2, taps)           # nt = 10
    x = np.zeros(100, np.complex64)
    # 10 outputs from ctr 0 read up to (9*2)//3 + 10 = 16 items and consume 20//3 = 6
    with pytest.raises(g.GrhipError) as e:
        b.general_work(10, x[:15])
    assert e.value.code == -1
    out, c = b.general_work(10, x[:16])
    assert len(out) == 10 and c == 6
    with pytest.raises(g.GrhipError) as e:
        b.forecast(-1)
    assert e.value.code == -1
    with pytest.raises(g.GrhipError) as e:
        b.general_work(-1, x)
    assert e.value.code == -1
    d = g.rational_resampler_base_fff(1, 3, np.ones(1, np.float32))   # consumes more than it reads
    with pytest.raises(g.GrhipError) as e:
        d.general_work(4, np.zeros(10, np.float32))          # reads 10, consumes 12
    assert e.value.code == -1
    with pytest.raises(g.GrhipError) as e:
        b.run_captures_device(2, 1000, 1, 10, 1, 10)         # strides shorter than the capture
    assert e.value.code == -1


@pytest.mark.parametrize("kind", KINDS)
def test_blks2_rational_resampler_designed_taps(gpu, po, kind):
    g = gpu
    rng = np.random.default_rng(11)
    x = _signal(rng, kind, 4000)
    rs = getattr(g, "rational_resampler_" + kind)(6, 4)
    assert rs.interpolation() == 3 and rs.decimation() == 2 and rs.history() == 101
    taps = g.design_filter(3, 2, 0.4)
    ref = rr.whole_rational(po, 3, 2, taps.astype(_dt(kind)) if kind == "ccc" else taps, x)
    rs.set_mode(g.MODE_GENERIC)
    out, _ = rs.general_work(len(ref), x)
    assert np.array_equal(_bits(out), _bits(ref))
    rs2 = getattr(g, "rational_resampler_" + kind)(3, 2)
    rs2.set_mode(g.MODE_FAST)
    assert rel_err_max(rs2.general_work(len(ref), x)[0], ref) < 1e-5


@pytest.fixture(scope="module")
def rs_exe(gpu):
    exe = os.path.join(HOST, "resampler_test")
    subprocess.check_call(["make", "-C", HOST, "resampler_test"], stdout=subprocess.DEVNULL)
    return exe


@pytest.mark.parametrize("which,kind,I,D", [("rational", "ccf", 3, 2), ("rational", "fff", 160, 147),
                                            ("rational", "ccc", 2, 3), ("interp", "ccf", 4, 1),
                                            ("interp", "ccc", 3, 1), ("interp", "fff", 5, 1)])
def test_cpp_blocks_under_executor(gpu, po, rs_exe, tmp_path, which, kind, I, D):
    g = gpu
    rng = np.random.default_rng(12)
    taps = _taps(rng, kind, 9 * I + 1)
    x = _signal(rng, kind, 200_000)
    x.tofile(tmp_path / "x.bin")
    taps.tofile(tmp_path / "taps.bin")
    r = subprocess.run([rs_exe, which, kind, str(I), str(D), "generic", str(tmp_path / "taps.bin"),
                        str(tmp_path / "x.bin"), str(tmp_path / "y.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(tmp_path / "y.bin", dtype=_dt(kind))
    if which == "interp":
        ref = rr.whole_interp(po, I, taps, x)
        assert len(got) == len(ref) and np.array_equal(_bits(got), _bits(ref))
    else:
        # the scheduler stops where forecast (one output more) no longer fits: a prefix of the whole stream
        ref = rr.whole_rational(po, I, D, taps, x)
        assert len(ref) - 4 <= len(got) <= len(ref) and np.array_equal(_bits(got), _bits(ref[:len(got)]))
    r = subprocess.run([rs_exe, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
