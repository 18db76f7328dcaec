"""Handle lifetime of iir_filter_ffd: 200 rounds of create, work and destroy over the tap sets and both modes with every
result checked (a handle that came up with a stale delay line, stale taps or stale scratch would show), handles that
never worked, set_streams up and down on a live handle, a handle destroyed with its work still queued, and the same
once in a child process that has to end cleanly."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import iir_ref as R

pytestmark = pytest.mark.gpu

ROUNDS = 200
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("deemph32k", "biquad", "order4", "n1m3")


def piece():
    """900 samples across the step from silence to the loud part"""
    return R.signal(1)[2200:3100]


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(R.bits(a), R.bits(b))


def test_create_work_destroy(gpu):
    g = gpu
    x = piece()
    want = {name: R.serial(x, *R.TAP_SETS[name])[0] for name in NAMES}
    for i in range(ROUNDS):
        name = NAMES[i % 4]
        blk = g.iir_filter_ffd(*R.TAP_SETS[name])
        blk.set_mode(g.MODE_GENERIC if i & 4 else g.MODE_FAST)
        if i & 8:
            # calls of at most 256 items take the serial walk in FAST too: bit for bit in both modes
            parts = (x[:200], x[200:333], x[333:589], x[589:845], x[845:])
            assert same_bits(np.concatenate([blk.work(p) for p in parts]), want[name]), i
        else:
            got = np.concatenate([blk.work(x[:333]), blk.work(x[333:])])
            if i & 4:
                assert same_bits(got, want[name]), i
            else:
                assert R.within_fast_bound(got, want[name]), i
        del blk
        g.iir_filter_ffd([1.0], [0.0])                                  # never used
    gc.collect()


def test_set_streams_on_a_live_handle(gpu):
    g = gpu
    x = R.signal(2)[:700]
    want = R.serial(x, *R.TAP_SETS["order4"])[0]
    blk = g.iir_filter_ffd(*R.TAP_SETS["order4"])
    for S in (1, 5, 64, 2, 1):
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            blk.set_mode(mode)
            blk.set_streams(S)                                          # every stream back at zeroed delay lines
            y = blk.work(np.tile(x, S), 700).reshape(S, 700)
            for s in range(S):
                if mode == g.MODE_GENERIC:
                    assert same_bits(np.ascontiguousarray(y[s]), want), (S, s)
                else:
                    assert R.within_fast_bound(y[s], want), (S, s)


def test_destroy_with_work_queued(gpu):
    import torch
    g = gpu
    x = R.signal(3)[:3000]
    want = R.serial(x, *R.TAP_SETS["biquad"])[0]
    d_in = torch.from_numpy(np.tile(x, 64)).cuda()
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        d_out = torch.zeros(64 * len(x), dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        blk = g.iir_filter_ffd(*R.TAP_SETS["biquad"])
        blk.set_mode(mode)
        blk.set_streams(64)
        blk.work_device(len(x), d_in, d_out, st)
        del blk                                                         # no synchronisation before the handle goes
        gc.collect()
        st.synchronize()
        out = d_out.cpu().numpy().reshape(64, len(x))
        for s in range(64):
            if mode == g.MODE_GENERIC:
                assert same_bits(np.ascontiguousarray(out[s]), want), s
            else:
                assert R.within_fast_bound(out[s], want), s


CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import grhip_loader
g = grhip_loader.import_grhip()
x = (np.arange(2000) %% 7 - 3).astype(np.float32)
for make in (lambda: g.fm_deemph(32e3), lambda: g.iir_filter_ffd([1.0, 0.5], [0.0, 0.25, -0.5])):
    b = make()
    b.set_streams(2)
    y = b.work(np.concatenate([x, 0 * x]))
    assert len(y) == 4000 and not y[2000:].any() and y[:2000].any()
    del b
for b in (g.iir_filter_ffd([], []), g.fm_deemph(320e3, 50e-6)):
    del b
print("child ok")
"""


def test_create_and_destroy_in_a_child_process(gpu):
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout
