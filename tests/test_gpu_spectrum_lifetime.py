"""Handle lifetime of the spectrum-estimate blocks: create, work and destroy every new handle type a few dozen times in
both modes, destroy handles that never worked, change set_streams on a live handle (the state is re-sized and starts
from zero), and do the same once in a child process that has to end cleanly.  Each result is checked, so a handle that
came up with stale state or buffers would show."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import spectrum_ref as sr
from conftest import bits_equal

pytestmark = pytest.mark.gpu

ROUNDS = 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_standalone_handles(gpu):
    g = gpu
    rng = np.random.default_rng(1)
    z = (rng.normal(size=300) + 1j * rng.normal(size=300)).astype(np.complex64)
    x = (rng.normal(size=300) + 3).astype(f32)
    ref_iir = sr.SinglePoleIir(0.25, 3).work(x)
    for i in range(ROUNDS):
        mode = g.MODE_GENERIC if i & 1 else g.MODE_FAST
        m, f, l, k = g.complex_to_mag_squared(3), g.single_pole_iir_filter_ff(0.25, 3), g.nlog10_ff(10, 3), g.keep_one_in_n(12, 4)
        for b in (m, f, l):
            b.set_mode(mode)
        assert bits_equal(m.work(100, z), sr.mag_squared(z))
        assert bits_equal(f.work(100, x), ref_iir)
        assert np.abs(l.work(100, x) - sr.nlog10_f64(x, 10)).max() < 1e-4
        assert bits_equal(k.work(100, x), x.reshape(100, 3)[3::4].reshape(-1))
        del m, f, l, k
        g.single_pole_iir_filter_ff(0.5, 4096)                  # never used
        g.keep_one_in_n(32768, 2)
    gc.collect()


def test_set_streams_resizes_the_state(gpu):
    g = gpu
    rng = np.random.default_rng(2)
    f = g.single_pole_iir_filter_ff(0.25, 5)
    f.set_mode(g.MODE_GENERIC)
    for S in (1, 4, 2, 300, 1):
        x = (rng.normal(size=S * 6 * 5) + 1).astype(f32)
        f.set_streams(S)                                        # restarts from zero, whatever ran before
        ref = sr.SinglePoleIir(0.25, 5, S)
        a = f.work(2, np.ascontiguousarray(x.reshape(S, 6, 5)[:, :2]).reshape(-1))
        b = f.work(4, np.ascontiguousarray(x.reshape(S, 6, 5)[:, 2:]).reshape(-1))
        want = ref.work(x.reshape(S, -1)).reshape(S, 6, 5)
        assert bits_equal(a.reshape(S, 2, 5), np.ascontiguousarray(want[:, :2]))
        assert bits_equal(b.reshape(S, 4, 5), np.ascontiguousarray(want[:, 2:]))


CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import grhip_loader
g = grhip_loader.import_grhip()
x = np.ones(4096 * 4, np.complex64)
for vlen in (4096, 12):
    m, f = g.complex_to_mag_squared(vlen), g.single_pole_iir_filter_ff(0.2, vlen)
    f.set_streams(2)
    m.set_streams(2)
    y = f.work(2, m.work(2, x))
    assert len(y) == 2 * 2 * vlen and abs(float(y[-1]) - 0.36) < 1e-6
    del m, f
for b in (g.complex_to_mag_squared(8), g.single_pole_iir_filter_ff(0.5, 8), g.nlog10_ff(10, 8), g.keep_one_in_n(8, 2)):
    del b
print("child ok")
"""


def test_create_and_destroy_in_a_child_process(gpu):
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout
