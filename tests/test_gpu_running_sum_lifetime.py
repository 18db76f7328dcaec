"""Handle lifetime of the running-sum blocks: create, work and destroy a few dozen times for every new handle type,
in both modes, and destroy handles that never worked.  Each result is checked, so a handle that came up with stale
state or buffers would show."""
import gc

import numpy as np
import pytest

import running_sum_ref as rr
from conftest import bits_equal

pytestmark = pytest.mark.gpu

ROUNDS = 32


def _x(kind, n):
    rng = np.random.default_rng(n)
    if kind == "cc":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) + 3).astype(np.complex64)
    if kind == "ff":
        return (rng.uniform(-1, 1, n) + 3).astype(np.float32)
    return rng.integers(-30000, 30000, n).astype(np.int16 if kind == "ss" else np.int32)


@pytest.mark.parametrize("kind", ["ff", "cc"])
def test_dc_blocker_handles(gpu, kind):
    g = gpu
    x = _x(kind, 700)
    ref = rr.DcBlocker(7, True, kind == "cc").work(x)
    make = g.dc_blocker_cc if kind == "cc" else g.dc_blocker_ff
    for i in range(ROUNDS):
        b = make(7, True)
        b.set_mode(g.MODE_GENERIC if i & 1 else g.MODE_FAST)
        got = b.work(700, x)
        if i & 1:
            assert bits_equal(got, ref)
        else:
            assert np.abs(got - ref).max() < 1e-4
        del b
        make(33, False)                                         # never used
    gc.collect()


@pytest.mark.parametrize("kind", ["ff", "cc", "ss", "ii"])
def test_moving_average_and_integrate_handles(gpu, kind):
    g = gpu
    x = _x(kind, 600)
    scale = {"ff": 0.5, "cc": 0.5 - 0.25j, "ss": 2, "ii": 2}[kind]
    ref_ma = rr.moving_average_work(kind, x, 10, scale, 500)
    ref_it = rr.integrate(kind, x, 6, 100)
    for i in range(ROUNDS):
        m = getattr(g, "moving_average_" + kind)(10, scale)
        it = getattr(g, "integrate_" + kind)(6)
        if i & 1:
            m.set_mode(g.MODE_GENERIC)
            it.set_mode(g.MODE_GENERIC)
        got_ma, got_it = m.work(500, x), it.work(100, x)
        if (i & 1) or kind in ("ss", "ii"):
            assert bits_equal(got_ma, ref_ma) and bits_equal(got_it, ref_it)
        else:
            assert np.abs(got_ma - ref_ma).max() < 1e-4 and np.abs(got_it - ref_it).max() < 1e-4
        del m, it
        getattr(g, "moving_average_" + kind)(1000, scale, 7)    # never used
        getattr(g, "integrate_" + kind)(1000)
    gc.collect()
