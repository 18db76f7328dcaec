"""Handle lifetime of the gain loops: 200 rounds of create, work and destroy over the four blocks and both modes with
every result checked (a handle that came up with a stale gain or stale scratch would show), handles that never worked,
set_streams up and down on a live handle, a handle destroyed with its work still queued, and the same once in a child
process that has to end cleanly."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import agc_ref as R

pytestmark = pytest.mark.gpu

ROUNDS = 200
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def piece(block):
    """900 samples across the step from silence to the loud part"""
    return R.signal(1, block)[2200:3100]


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(R.bits(a), R.bits(b))


def test_create_work_destroy(gpu):
    g = gpu
    want = {}
    for block in R.BLOCKS:
        x = piece(block)
        a = R.serial(block, x[:333], R.sets(block)[0])
        want[block] = (a, R.serial(block, x[333:], R.sets(block)[0], a.gain))
    for i in range(ROUNDS):
        block = R.BLOCKS[i % 4]
        x = piece(block)
        blk = getattr(g, block)(*R.sets(block)[0])
        # calls of at most 256 items in FAST take the serial walk too, so every round is held bit for bit
        blk.set_mode(g.MODE_GENERIC if i & 4 else g.MODE_FAST)
        if i & 4:
            for part, w in zip((x[:333], x[333:]), want[block]):
                assert same_bits(blk.work(part), w.out), i
        else:
            parts = (x[:200], x[200:333], x[333:589], x[589:845], x[845:])
            got = np.concatenate([blk.work(p) for p in parts])
            assert same_bits(got, np.concatenate([w.out for w in want[block]])), i
        assert blk.gain() == want[block][1].gain, i
        del blk
        getattr(g, block)()                                             # never used
    gc.collect()


def test_set_streams_on_a_live_handle(gpu):
    g = gpu
    params = R.AGC_SETS[0]
    x = R.signal(2)
    r = R.serial("agc_cc", x[:700], params)
    g64 = R.exact64("agc_cc", x[:700], params)
    bound = R.bound(R.deviation(r.gains, g64)) * np.max(np.abs(g64))
    blk = g.agc_cc(*params)
    for S in (1, 5, 64, 2, 1):
        blk.set_streams(S)                                              # every stream back at the constructor's gain
        for mode in (g.MODE_GENERIC, g.MODE_FAST):
            blk.set_mode(mode)
            blk.set_gain(params[2])
            y = blk.work(np.tile(x[:700], S), 700).reshape(S, 700)
            for s in range(S):
                if mode == g.MODE_GENERIC:
                    assert same_bits(y[s], r.out) and blk.gain(s) == r.gain, (S, s)
                else:
                    assert np.all(np.abs(y[s] - x[:700] * g64[:-1]) <= R.mag64(x[:700]) * bound + 2.0 ** -23 * np.abs(x[:700] * g64[:-1]))
                    assert abs(float(blk.gain(s)) - g64[-1]) <= bound, (S, s)
        with pytest.raises(g.GrhipError):
            blk.gain(S)


def test_destroy_with_work_queued(gpu):
    import torch
    g = gpu
    x = R.signal(3)[:3000]
    params = R.AGC_SETS[2]
    want = R.serial("agc_cc", x, params)
    g64 = R.exact64("agc_cc", x, params)
    bound = R.bound(R.deviation(want.gains, g64)) * np.max(np.abs(g64))
    d_in = torch.from_numpy(np.tile(x, 64)).cuda()
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        d_out = torch.zeros(64 * len(x), dtype=torch.complex64, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        blk = g.agc_cc(*params)
        blk.set_mode(mode)
        blk.set_streams(64)
        blk.work_device(len(x), d_in, d_out, st)
        del blk                                                         # no synchronisation before the handle goes
        gc.collect()
        st.synchronize()
        out = d_out.cpu().numpy().reshape(64, len(x))
        if mode == g.MODE_GENERIC:
            assert np.array_equal(R.bits(out), np.tile(R.bits(want.out), (64, 1)))
        else:
            ideal = x * g64[:-1]
            assert np.all(np.abs(out - ideal) <= R.mag64(x) * bound + 2.0 ** -23 * np.abs(ideal))


CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import grhip_loader
g = grhip_loader.import_grhip()
x = (np.arange(2000) %% 7 - 3).astype(np.float32)
for make in (g.agc_ff, g.agc2_ff):
    b = make()
    b.set_streams(2)
    y = b.work(np.concatenate([x, 0 * x]))
    assert len(y) == 4000 and not y[2000:].any() and y[:2000].any()
    del b
for b in (g.agc_cc(), g.agc2_cc(0.5, 0.1, 1, 1, 3)):
    del b
print("child ok")
"""


def test_create_and_destroy_in_a_child_process(gpu):
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout
