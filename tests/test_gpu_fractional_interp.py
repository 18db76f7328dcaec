"""-m gpu: gr_fractional_interpolator_ff / _cc on the device against the restatement (tests/fractional_interp_ref.py,
itself pinned to the reference's own outputs by tests/test_fractional_interp_cpu.py): GRHIP_MODE_GENERIC bit for
bit with the output count, the consumed count and the final mu(), FAST within 1e-5 of the output peak of the float64
evaluation of the same schedule, call splitting around the kernel's tile, the setters, the walked schedule back to
back on one stream, run_captures_device, bad arguments, the C++ block under the stand-in executor, and the block in
front of clock_recovery_mm_ff."""
import os
import re
import subprocess

import numpy as np
import pytest

import fractional_interp_ref as fr
from conftest import rel_err_max

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd")
HOST = os.path.join(PKG, "host")


def _const(name):
    src = open(os.path.join(PKG, "csrc", "frac_interp.h")).read()
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % name, src)
    return int(eval(m.group(1)))


TILE = _const("FRAC_TILE")
SPAN_BYTES = _const("FRAC_SPAN_BYTES")


def on_grid(v):
    return f32(np.round(float(f32(v)) * 2 ** 24) / 2 ** 24)


PHASES = [f32(0.0), f32(2.0 ** -24), f32(0.5), on_grid(0.37), on_grid(0.999), f32(1.0)]
RATIOS = [f32(0.3), f32(0.5), f32(0.75), f32(0.9999), f32(1.0), f32(1.0001), f32(1.3), f32(160.0 / 147.0),
          f32(147.0 / 160.0), f32(2.5), f32(4.8), f32(10.0), f32(1000.7)]
OFF_GRID = [(f32(0.1), f32(1.0)), (f32(0.1), f32(10.0)), (f32(0.0), f32(0.01)), (f32(0.37), f32(0.001))]


def _torch():
    import torch
    return torch


def _blk(g, cplx, phase, ratio, mode):
    b = (g.fractional_interpolator_cc if cplx else g.fractional_interpolator_ff)(phase, ratio)
    b.set_mode(mode)
    return b


def _signal(rng, n, cplx):
    x = rng.standard_normal(n).astype(f32)
    if cplx:
        x = (x + 1j * rng.standard_normal(n)).astype(np.complex64)
    return x


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _n_samples(ratio):
    """at most 3000 input items, and not more than ~3000 outputs (three tiles)"""
    return int(max(40, min(3000, 3000 * float(ratio))))


def _same_mu(blk, ref):
    return f32(blk.mu()).view(np.uint32) == f32(ref.mu()).view(np.uint32)


@pytest.mark.parametrize("cplx", [False, True], ids=["ff", "cc"])
def test_generic_bit_exact_sweep(gpu, cplx):
    g = gpu
    rng = np.random.default_rng(3 if cplx else 4)
    bad = []
    for phase, ratio in [(p, r) for r in RATIOS for p in PHASES] + OFF_GRID:
        x = _signal(rng, _n_samples(ratio), cplx)
        rblk = fr.FractionalInterpolatorRef(phase, ratio, cplx)
        ref, rc = rblk.general_work(1 << 20, x)
        assert len(ref) > 0
        blk = _blk(g, cplx, phase, ratio, g.MODE_GENERIC)
        got, c = blk.general_work(len(ref) + 16, x)
        if len(got) != len(ref) or c != rc or not np.array_equal(_bits(got), _bits(ref)) or not _same_mu(blk, rblk):
            bad.append((float(phase), float(ratio), len(got), len(ref), c, rc, blk.mu(), rblk.mu()))
    assert not bad, bad


@pytest.mark.parametrize("cplx", [False, True], ids=["ff", "cc"])
def test_fast_within_tolerance(gpu, cplx):
    g = gpu
    rng = np.random.default_rng(5)
    for phase, ratio in [(f32(0.0), f32(0.5)), (on_grid(0.37), f32(160.0 / 147.0)), (f32(1.0), f32(1.25)),
                         (f32(0.1), f32(10.0)), (f32(0.0), f32(0.3)), (f32(0.5), f32(1000.7)), (f32(0.0), f32(4.8))]:
        x = _signal(rng, _n_samples(ratio), cplx)
        ii, imu, _mu = fr.whole_stream_schedule(phase, ratio, len(x))
        ref64 = fr.eval_schedule(x, ii, imu, f64=True)
        blk = _blk(g, cplx, phase, ratio, g.MODE_FAST)
        got, _c = blk.general_work(len(ii) + 16, x)
        assert len(got) == len(ii)
        assert rel_err_max(got, ref64) < 1e-5, (phase, ratio)


def test_fast_modes_are_one_kernel(gpu):
    g = gpu
    x = _signal(np.random.default_rng(6), 2000, True)
    outs = [_blk(g, True, 0.25, 1.3, m).general_work(5000, x)[0]
            for m in (g.MODE_FAST, g.MODE_FAST_VALU, g.MODE_FAST_REFTAPS)]
    assert len(outs[0]) > 1000
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(outs[2]))


def test_history_forecast_accessors(gpu):
    g = gpu
    for cls in (g.fractional_interpolator_ff, g.fractional_interpolator_cc):
        blk = cls(1.0, 1.25)
        assert blk.history() == 1 and blk.mu() == 1.0 and blk.interp_ratio() == 1.25
        assert blk.forecast(100) == 133 and blk.forecast(0) == 8
        blk.set_interp_ratio(0.3)
        assert blk.forecast(3) == fr.forecast(3, f32(0.3)) == 9
        assert f32(blk.interp_ratio()) == f32(0.3)


def _shrink_ratios(cplx):
    """a tile of TILE outputs spans up to (TILE - 1) * ratio + 1 + 8 items; the LDS image holds SPAN_BYTES / item.
    The smallest ratios past that: the next float (a walked schedule) and the next multiple of 1/8 (a closed form)."""
    cap = SPAN_BYTES // (8 if cplx else 4)
    edge = (cap - 8) / (TILE - 1.0)
    return [np.nextafter(f32(edge), f32(np.inf)), f32(np.ceil(edge * 8 + 1e-9) / 8)]


@pytest.mark.parametrize("mode", ["GENERIC", "FAST"])
@pytest.mark.parametrize("cplx", [False, True], ids=["ff", "cc"])
def test_call_sizes_concatenate_to_whole_stream(gpu, cplx, mode):
    g = gpu
    m = getattr(g, "MODE_" + mode)
    rng = np.random.default_rng(7)
    cases = [(f32(0.0), f32(1.25), 3000), (on_grid(0.37), f32(147.0 / 160.0), 3000), (f32(1.0), f32(0.75), 3000),
             (f32(0.1), f32(1.0), 3000)]
    for r in _shrink_ratios(cplx):                       # correspondingly more input: three tiles' worth
        cases += [(f32(0.0), r, int(3 * TILE * float(r))), (f32(1.0), r, int(3 * TILE * float(r)))]
    for phase, ratio, N in cases:
        x = _signal(rng, N, cplx)
        whole = fr.whole_stream(phase, ratio, x)
        assert len(whole) > 2 * TILE + 3
        if mode == "FAST":                               # FAST against itself in one call: its sums do not depend
            whole, _ = fr.run_calls(_blk(g, cplx, phase, ratio, m), x, [(1 << 20, None)])      # on the tiling
            assert rel_err_max(whole, fr.whole_stream(phase, ratio, x, f64=True)) < 1e-5
        patterns = [
            [(1, None)] * 3 + [(7, None), (TILE - 1, None), (TILE, None), (TILE + 1, None), (2 * TILE + 3, None)],
            [(TILE + 1, "forecast-1"), (7, "forecast"), (2 * TILE + 3, "forecast-1"), (TILE, "forecast")],
            [(5, 1), (TILE - 1, 100), (65536, 17), (1 << 20, None)],
        ]
        for sizes in patterns:
            blk = _blk(g, cplx, phase, ratio, m)
            got, rd = fr.run_calls(blk, x, sizes)
            assert len(got) == len(whole) and np.array_equal(_bits(got), _bits(whole)), (phase, ratio, sizes)


@pytest.mark.parametrize("cplx", [False, True], ids=["ff", "cc"])
def test_setters_between_calls(gpu, cplx):
    g = gpu
    rng = np.random.default_rng(8)
    x = _signal(rng, 3000, cplx)
    blk = _blk(g, cplx, 0.0, 1.25, g.MODE_GENERIC)
    ref = fr.FractionalInterpolatorRef(0.0, 1.25, cplx)
    rd = 0
    steps = [(None, None), ("ratio", 147.0 / 160.0), ("ratio", 0.75), ("mu", 1.0), ("ratio", 0.01), ("ratio", 2.5),
             ("mu", 0.0)]
    for what, v in steps:
        for b in (blk, ref):
            if what == "ratio":
                b.set_interp_ratio(v)
            elif what == "mu":
                b.set_mu(v)
        nout = 300
        nin = min(len(x) - rd, blk.forecast(nout))
        assert blk.forecast(nout) == ref.forecast(nout)
        got, c = blk.general_work(nout, x[rd:rd + nin])
        want, rc = ref.general_work(nout, x[rd:rd + nin])
        assert len(got) == len(want) == nout and c == rc, (what, v)
        assert np.array_equal(_bits(got), _bits(want)) and _same_mu(blk, ref), (what, v)
        rd += c


@pytest.mark.parametrize("cplx", [False, True], ids=["ff", "cc"])
def test_walked_schedule_back_to_back(gpu, cplx):
    """two general_work_device calls with walked schedules on one stream, no sync in between: the second call's
    upload must not overwrite the entries the first launch still reads"""
    g = gpu
    torch = _torch()
    w = 2 if cplx else 1
    dt = np.complex64 if cplx else f32
    x = _signal(np.random.default_rng(9), 3000, cplx)
    phase, ratio = f32(0.1), f32(147.0 / 160.0)
    assert not fr.closed_form_ok(phase, ratio)
    ref = fr.FractionalInterpolatorRef(phase, ratio, cplx)
    w1, c1 = ref.general_work(1500, x)
    w2, c2 = ref.general_work(1500, x[c1:])
    d_in = torch.from_numpy(x.view(f32).copy()).cuda()
    d_out = torch.zeros(3000 * w, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    blk = _blk(g, cplx, phase, ratio, g.MODE_GENERIC)
    n1, k1 = blk.general_work_device(1500, len(x), d_in.data_ptr(), d_out.data_ptr(), stream=st)
    n2, k2 = blk.general_work_device(1500, len(x) - k1, d_in[k1 * w:].data_ptr(), d_out[n1 * w:].data_ptr(), stream=st)
    st.synchronize()
    assert (n1, k1, n2, k2) == (len(w1), c1, len(w2), c2) and n1 == 1500 and n2 > 1000
    got = d_out.cpu().numpy().view(dt)
    assert np.array_equal(_bits(got[:n1]), _bits(w1)) and np.array_equal(_bits(got[n1:n1 + n2]), _bits(w2))
    assert _same_mu(blk, ref)


@pytest.mark.parametrize("mode", ["GENERIC", "FAST"])
@pytest.mark.parametrize("cplx", [False, True], ids=["ff", "cc"])
def test_run_captures_device(gpu, cplx, mode):
    g = gpu
    torch = _torch()
    m = getattr(g, "MODE_" + mode)
    rng = np.random.default_rng(10)
    dt = np.complex64 if cplx else f32
    w = 2 if cplx else 1
    for phase, ratio in ((0.0, 0.5), (0.25, 160.0 / 147.0), (1.0, 2.0), (0.1, 147.0 / 160.0), (0.0, 4.8)):
        n_streams, N, stride = 3, 3000, 3011
        caps = [_signal(rng, N, cplx) for _ in range(n_streams)]
        host = [_blk(g, cplx, phase, ratio, m).general_work(1 << 20, c)[0] for c in caps]
        blk = _blk(g, cplx, phase, ratio, m)
        blk.set_mu(0.5)                                   # the handle's own mu: not what a capture starts from
        n_out = blk.captures_nout(N)
        assert n_out == len(fr.whole_stream_schedule(phase, ratio, N)[0]) and all(len(h) == n_out for h in host)
        d_in = torch.zeros(n_streams * stride * w, dtype=torch.float32, device="cuda")
        for s, c in enumerate(caps):
            d_in[s * stride * w:(s * stride + N) * w] = torch.from_numpy(c.view(f32).copy()).cuda()
        ostride = n_out + 5
        d_out = torch.zeros(n_streams * ostride * w, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert blk.run_captures_device(n_streams, N, d_in, stride, d_out, ostride) == n_out
        g.lib().grhip_device_synchronize(0)
        got = d_out.cpu().numpy().view(dt)
        for s in range(n_streams):
            assert np.array_equal(_bits(got[s * ostride:s * ostride + n_out]), _bits(host[s])), (ratio, s)
            assert not got[s * ostride + n_out:(s + 1) * ostride].any()
        assert blk.mu() == 0.5
        if mode == "GENERIC":
            assert np.array_equal(_bits(host[0]), _bits(fr.whole_stream(phase, ratio, caps[0])))


def test_bad_arguments(gpu):
    g = gpu
    for cls in (g.fractional_interpolator_ff, g.fractional_interpolator_cc):
        for args, code in (((0.0, 0.0), -2), ((0.0, -1.0), -2), ((0.0, float("nan")), -2), ((-0.1, 1.0), -2),
                           ((1.1, 1.0), -2), ((0.0, 2.0 ** 20), -1)):
            with pytest.raises(g.GrhipError) as e:
                cls(*args)
            assert e.value.code == code, args
        blk = cls(0.0, 1.25)
        blk.set_mode(g.MODE_GENERIC)
        for call, code in ((lambda: blk.set_interp_ratio(0.0), -2), (lambda: blk.set_interp_ratio(-3.0), -2),
                           (lambda: blk.set_interp_ratio(float("nan")), -2), (lambda: blk.set_mu(2.0), -2),
                           (lambda: blk.set_mu(-0.1), -2), (lambda: blk.set_interp_ratio(2.0 ** 21), -1),
                           (lambda: blk.set_mode(7), -1), (lambda: blk.forecast(-1), -1),
                           (lambda: blk.general_work(-1, np.zeros(10, blk._dtype)), -1),
                           (lambda: blk.run_captures_device(2, 1000, 1, 10, 1, 10), -1)):
            with pytest.raises(g.GrhipError) as e:
                call()
            assert e.value.code == code
        # the handle is as it was and still works
        assert blk.mu() == 0.0 and blk.interp_ratio() == 1.25
        x = _signal(np.random.default_rng(11), 500, blk._dtype == np.complex64)
        got, c = blk.general_work(100, x)
        ref, rc = fr.FractionalInterpolatorRef(0.0, 1.25, blk._dtype == np.complex64).general_work(100, x)
        assert c == rc and np.array_equal(_bits(got), _bits(ref))
        cls(1.0, np.nextafter(f32(2.0 ** 20), f32(0)))       # the limits hold exactly at their edges


@pytest.fixture(scope="module")
def frac_exe(gpu):
    exe = os.path.join(HOST, "frac_interp_test")
    subprocess.check_call(["make", "-C", HOST, "frac_interp_test"], stdout=subprocess.DEVNULL)
    return exe


@pytest.mark.parametrize("cplx,phase,ratio", [(False, 0.0, 1.25), (True, 1.0, 160.0 / 147.0), (False, 0.1, 0.3),
                                              (True, 0.5, 52.1)])
def test_cpp_block_under_executor(gpu, frac_exe, tmp_path, cplx, phase, ratio):
    rng = np.random.default_rng(12)
    x = _signal(rng, 100_000, cplx)
    x.tofile(tmp_path / "x.bin")
    r = subprocess.run([frac_exe, "cc" if cplx else "ff", repr(phase), repr(ratio), "generic", str(tmp_path / "x.bin"),
                        str(tmp_path / "y.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(tmp_path / "y.bin", dtype=np.complex64 if cplx else f32)
    ii, imu, _mu = fr.whole_stream_schedule(f32(phase), f32(ratio), len(x))
    # the executor stops once forecast for one more output cannot be met: a prefix of the whole stream, short of it
    # by less than the items one forecast asks for
    assert 0 < len(got) <= len(ii) and len(ii) - len(got) <= 8 / ratio + 2
    assert np.array_equal(_bits(got), _bits(fr.eval_schedule(x, ii[:len(got)], imu[:len(got)])))
    r = subprocess.run([frac_exe, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_pipeline_into_clock_recovery(gpu, po):
    """fractional_interpolator_ff(0, 1.25) brings 12.5 samples per symbol to 10; clock_recovery_mm_ff follows.  Both
    GENERIC bit-exact against the two restatements chained."""
    g = gpu
    rng = np.random.default_rng(13)
    sym = np.repeat(rng.choice([-3.0, -1.0, 1.0, 3.0], 240), 25)[::2]          # 12.5 samples per symbol
    x = (np.convolve(sym, np.ones(5) / 5, mode="same") + rng.normal(0, 0.1, len(sym))).astype(f32)
    assert len(x) == 3000
    mid_ref = fr.whole_stream(f32(0.0), f32(1.25), x)
    omega, gm = 10.0, 0.175
    ref, st = po.chain_mm(omega, 0.25 * gm * gm, 0.5, gm, 0.005, mid_ref)
    fi = _blk(g, False, 0.0, 1.25, g.MODE_GENERIC)
    mid, _c = fi.general_work(len(mid_ref) + 16, x)
    cr = g.clock_recovery_mm_ff(omega, 0.25 * gm * gm, 0.5, gm, 0.005)
    out, consumed = cr.general_work(len(mid), mid)
    assert np.array_equal(_bits(mid), _bits(mid_ref))
    assert len(out) == len(ref) > 200 and np.array_equal(_bits(out), _bits(ref)) and consumed == st["consumed"]
