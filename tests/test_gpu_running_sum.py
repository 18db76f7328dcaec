"""GPU tests of dc_blocker_ff / _cc, moving_average_XX and integrate_XX.

GENERIC is compared bit for bit (uint32 views) with the float32 restatements of running_sum_ref.py, which
test_running_sum_cpu.py pins to the reference's QA vectors.  FAST is compared with the float64 form of the same
filters, within 1e-5 of the output's peak (the project's FAST rule): the float32 recurrence of the reference drifts
from that form (DESIGN 4.14 records by how much), a true window sum does not.

Shapes: the GENERIC dc_blocker kernel walks windows of 256 samples, the FAST kernel tiles of 2304 staged samples;
N = 3 * 2304 + 37 covers three tiles of either plus an odd remainder.  DC 10 makes the reference's drift non-zero.
"""
import os
import subprocess

import numpy as np
import pytest

import running_sum_ref as rr
from conftest import bits_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")
GEN_WIN, FAST_TILE = 256, 2304
N = 3 * FAST_TILE + 37
DS = [1, 2, 3, 32, 33, 100]
FAST_TOL = 1e-5


def _signal(kind, n, seed, dc=10.0):
    rng = np.random.default_rng(seed)
    if kind == "cc":
        return (rng.uniform(-1, 1, n) + dc + 1j * (rng.uniform(-1, 1, n) - dc / 2)).astype(np.complex64)
    return (rng.uniform(-1, 1, n) + dc).astype(f32)


def _splits(n, D, tile):
    sizes = [s for s in (1, D - 2, D, tile + 1) if s > 0]
    edges = np.cumsum([0] + sizes).tolist()
    return list(zip(edges, edges[1:] + [n]))


def _peak_err(got, ref):
    e, p = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    return e / p if p > 0 else e


def _fast_ok(got, ref):
    """the FAST rule: within 1e-5 of the output's peak.  (At D = 1 the filter's output is identically zero, in the
    float64 form too: its inputs are floats, every difference is exact; FAST must then return exactly 0.)"""
    return float(np.abs(got - ref).max()) <= FAST_TOL * float(np.abs(ref).max())


def _blk(g, kind, D, long_form, mode):
    b = (g.dc_blocker_cc if kind == "cc" else g.dc_blocker_ff)(D, long_form)
    b.set_mode(mode)
    return b


@pytest.mark.parametrize("kind", ["ff", "cc"])
@pytest.mark.parametrize("long_form", [True, False])
@pytest.mark.parametrize("D", DS)
def test_dc_blocker_generic_bit_exact(gpu, kind, long_form, D):
    g = gpu
    x = _signal(kind, N, D)
    ref = rr.DcBlocker(D, long_form, kind == "cc").work(x)
    b = _blk(g, kind, D, long_form, g.MODE_GENERIC)
    assert b.get_group_delay() == (2 * D - 2 if long_form else D - 1)
    assert bits_equal(b.work(N, x), ref)
    b = _blk(g, kind, D, long_form, g.MODE_GENERIC)             # the same stream in pieces: the state carries exactly
    got = np.concatenate([b.work(e - s, x[s:e]) for s, e in _splits(N, D, GEN_WIN)])
    assert bits_equal(got, ref)


@pytest.mark.parametrize("kind", ["ff", "cc"])
@pytest.mark.parametrize("mode", ["GENERIC", "FAST"])
def test_dc_blocker_streams(gpu, kind, mode):
    g = gpu
    m = getattr(g, "MODE_" + mode)
    n, D = 2 * FAST_TILE + 11, 33
    xs = [_signal(kind, n, 40 + s, dc=3.0 * s) for s in range(3)]
    b = _blk(g, kind, D, True, m)
    b.set_streams(3)
    b.set_mode(m)
    cut = FAST_TILE + 5
    got = np.concatenate([b.work(cut, np.concatenate([x[:cut] for x in xs])).reshape(3, cut),
                          b.work(n - cut, np.concatenate([x[cut:] for x in xs])).reshape(3, n - cut)], axis=1)
    for s in range(3):
        one = _blk(g, kind, D, True, m).work(n, xs[s])          # a handle of its own
        if mode == "GENERIC":
            assert bits_equal(got[s], one)
        else:
            ref = rr.DcBlocker(D, True, kind == "cc", np.float64).work(xs[s])
            assert _fast_ok(got[s], one.astype(ref.dtype))
            assert _fast_ok(got[s], ref) and _fast_ok(one, ref)


@pytest.mark.parametrize("kind", ["ff", "cc"])
@pytest.mark.parametrize("long_form", [True, False])
@pytest.mark.parametrize("D", DS)
def test_dc_blocker_fast_is_the_float64_filter(gpu, kind, long_form, D):
    g = gpu
    x = _signal(kind, N, D)
    ref = rr.DcBlocker(D, long_form, kind == "cc", np.float64).work(x)
    b = _blk(g, kind, D, long_form, g.MODE_FAST)
    one = b.work(N, x)
    e1 = _peak_err(one, ref)
    b = _blk(g, kind, D, long_form, g.MODE_FAST)
    parts = np.concatenate([b.work(e - s, x[s:e]) for s, e in _splits(N, D, FAST_TILE - (4 if long_form else 2) * (D - 1))])
    e2, e3 = _peak_err(parts, ref), _peak_err(parts, one.astype(ref.dtype))
    gen = _blk(g, kind, D, long_form, g.MODE_GENERIC).work(N, x)
    print("dc_blocker_%s D=%d long=%d: FAST %.2e, in pieces %.2e, pieces vs one call %.2e; GENERIC vs float64 %.2e"
          % (kind, D, long_form, e1, e2, e3, _peak_err(gen, ref)))
    assert _fast_ok(one, ref) and _fast_ok(parts, ref) and _fast_ok(parts, one.astype(ref.dtype))


def test_dc_blocker_fast_error_does_not_grow_with_length(gpu):
    g = gpu
    n = 2_000_000
    x = _signal("ff", n, 77)
    ref = rr.DcBlocker(32, True, False, np.float64).work(x)
    got = _blk(g, "ff", 32, True, g.MODE_FAST).work(n, x)
    tail = slice(n - 100_000, n)
    e, et = _peak_err(got, ref), float(np.abs(got[tail] - ref[tail]).max() / np.abs(ref).max())
    gen = _blk(g, "ff", 32, True, g.MODE_GENERIC).work(n, x)
    print("2 M samples, DC 10: FAST %.2e of peak (last 100 k: %.2e); GENERIC (the reference's recurrence) %.2e, absolute %.2e"
          % (e, et, _peak_err(gen, ref), float(np.abs(gen - ref).max())))
    assert _fast_ok(got, ref)


def test_dc_blocker_largest_D(gpu):
    g = gpu
    D, n = 1024, 9000
    for kind in ("ff", "cc"):
        x = _signal(kind, n, 5)
        ref64 = rr.DcBlocker(D, True, kind == "cc", np.float64).work(x)
        assert _fast_ok(_blk(g, kind, D, True, g.MODE_FAST).work(n, x), ref64)
        assert bits_equal(_blk(g, kind, D, True, g.MODE_GENERIC).work(n, x), rr.DcBlocker(D, True, kind == "cc").work(x))


# ---- moving_average ------------------------------------------------------------------------------------------------------
MA = {"ff": ("moving_average_ff", f32(0.1)), "cc": ("moving_average_cc", np.complex64(0.1 - 0.05j)),
      "ss": ("moving_average_ss", 3), "ii": ("moving_average_ii", 3)}


def _ma_input(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "ss":
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[::5] = 32767
        x[1::7] = -32767
        return x
    if kind == "ii":
        x = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
        x[::5] = 2 ** 31 - 1
        x[1::7] = -2 ** 31
        return x
    return _signal(kind, n, seed, dc=1.0)


def _device_call(g, blk, x, n, dtype):
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).cuda()
    d_out = torch.zeros(max(n, 1) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                    # the block's stream does not wait for the fill
    r = blk.work_device(n, d_in, d_out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return r, d_out.cpu().numpy().view(dtype)[:n]


@pytest.mark.parametrize("kind", ["ff", "cc", "ss", "ii"])
@pytest.mark.parametrize("length", [1, 2, 7, 10, 64, 65, 1000])
def test_moving_average(gpu, kind, length):
    g = gpu
    name, scale = MA[kind]
    for max_iter in (1, 7, 4096):
        for chunks in (1, 2, 2.5):
            n = int(max_iter * chunks) if max_iter > 1 else int(chunks * 2)
            x = _ma_input(kind, n + length - 1, length + max_iter)
            ref = rr.moving_average_calls(kind, x, length, scale, n, max_iter)
            for mode in (g.MODE_GENERIC, g.MODE_FAST):
                b = getattr(g, name)(length, scale, max_iter)
                b.set_mode(mode)
                assert b.history() == length and b.max_iter() == max_iter
                r, got = _device_call(g, b, x, n, x.dtype)          # successive work calls of max_iter outputs
                one = b.work(n, x)                                    # one work call
                assert r == n and len(one) == min(n, max_iter)
                if kind in ("ss", "ii") or mode == g.MODE_GENERIC:
                    assert bits_equal(got, ref), (kind, length, max_iter, n, mode)
                    assert bits_equal(one, ref[:len(one)])
                else:
                    ref64 = rr.moving_average_f64(x, length, complex(scale) if kind == "cc" else float(scale), n)
                    assert _peak_err(got, ref64) <= FAST_TOL, (kind, length, max_iter, n)
                    assert _peak_err(one, ref64[:len(one)]) <= FAST_TOL


@pytest.mark.parametrize("kind", ["ff", "cc", "ii"])
@pytest.mark.parametrize("length", [4096, 8449])
def test_moving_average_long_windows(gpu, kind, length):
    """4096 must work; 8449 is the most the LDS layout carries (R and the tile are at their caps there)"""
    g = gpu
    name, scale = MA[kind]
    n = 12000                                                   # more than one tile at either length, 2.9 work calls
    x = _ma_input(kind, n + length - 1, length)
    ref = rr.moving_average_calls(kind, x, length, scale, n, 4096)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        b = getattr(g, name)(length, scale)
        b.set_mode(mode)
        r, got = _device_call(g, b, x, n, x.dtype)
        assert r == n
        if kind == "ii" or mode == g.MODE_GENERIC:
            assert bits_equal(got, ref), (kind, length, mode)
        else:
            ref64 = rr.moving_average_f64(x, length, complex(scale) if kind == "cc" else float(scale), n)
            e = _peak_err(got, ref64)
            print("moving_average_%s length %d FAST: %.2e of peak" % (kind, length, e))
            assert e <= FAST_TOL
    with pytest.raises(g.GrhipError):
        getattr(g, name)(8450, scale)


@pytest.mark.parametrize("kind", ["ff", "ii"])
def test_moving_average_setter_latches(gpu, kind):
    g = gpu
    name, scale = MA[kind]
    x = _ma_input(kind, 300, 3)
    b = getattr(g, name)(10, scale, 4096)
    b.set_mode(g.MODE_GENERIC)
    assert bits_equal(b.work(100, x), rr.moving_average_work(kind, x, 10, scale, 100))
    b.set_length_and_scale(33, scale)
    assert b.history() == 10                                    # not yet
    assert len(b.work(100, x)) == 0                             # the call that applies it computes nothing
    assert b.history() == 33
    assert bits_equal(b.work(100, x), rr.moving_average_work(kind, x, 33, scale, 100))
    b.set_length_and_scale(5, scale)
    r, _ = _device_call(g, b, x, 100, x.dtype)
    assert r == 0 and b.history() == 5
    with pytest.raises(g.GrhipError):
        b.set_length_and_scale(0, scale)


# ---- integrate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ff", "cc", "ss", "ii"])
@pytest.mark.parametrize("decim", [1, 2, 3, 10, 64, 1000])
def test_integrate(gpu, kind, decim):
    g = gpu
    n = 3 * 256 + 37 if decim < 64 else 67
    x = _ma_input(kind, n * decim, decim)
    ref = rr.integrate(kind, x, decim, n)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        b = getattr(g, "integrate_" + kind)(decim)
        b.set_mode(mode)
        assert b.decimation() == decim and b.history() == 1
        got = b.work(n, x)
        if kind in ("ss", "ii") or mode == g.MODE_GENERIC:
            assert bits_equal(got, ref), (kind, decim, mode)
        else:
            assert _peak_err(got, rr.integrate_f64(x, decim, n)) <= FAST_TOL


def test_bad_arguments(gpu):
    g = gpu
    for make in (lambda: g.dc_blocker_ff(0), lambda: g.dc_blocker_ff(32).set_mode(9), lambda: g.dc_blocker_ff(32).set_streams(0),
                 lambda: g.moving_average_ff(0, 1.0), lambda: g.integrate_ii(0), lambda: g.integrate_ff(3).set_mode(7)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1


# ---- the C++ blocks --------------------------------------------------------------------------------------------------------
def test_cpp_blocks(gpu):
    subprocess.check_call(["make", "-C", HOST, "running_sum_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "running_sum_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
