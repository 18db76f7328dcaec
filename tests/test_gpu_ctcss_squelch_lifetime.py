"""Handle lifetime of ctcss_squelch_ff: 200 rounds of create, work and destroy in both modes with every result checked
(a handle that came up with a stale carry, decision or table would show), handles that never worked, a handle destroyed
with its work still queued, and the same once in a child process that has to end cleanly."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import ctcss_ref as ct

pytestmark = pytest.mark.gpu

ROUNDS = 200
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, LEN = 500, 250


def piece():
    """2000 samples around the start of the first burst, cut so that every call leaves a block unfinished"""
    x = ct.signal(1, RATE, LEN)[4 * LEN:4 * LEN + 2000]
    assert ct.condition(RATE, LEN, 100.0, 0.01, x)[0] >= 10 * ct.condition(RATE, LEN, 100.0, 0.01, x)[1]
    return x


def test_create_work_destroy(gpu):
    g = gpu
    x = piece()
    r = ct.CtcssSquelch(RATE, 100.0, 0.01, LEN, 64, True)
    want = [r.work(x[:777]), r.work(x[777:])]
    assert 0 < len(want[0]) < 777 and len(want[1]) == 2000 - 777       # unmutes inside the first call
    for i in range(ROUNDS):
        blk = g.ctcss_squelch_ff(RATE, 100.0, 0.01, LEN, 64, True)
        blk.set_mode(g.MODE_GENERIC if i & 1 else g.MODE_FAST)
        for a, w in zip((x[:777], x[777:]), want):
            got = blk.work(a)
            assert got.dtype == w.dtype and np.array_equal(got.view(np.uint32), w.view(np.uint32)), i
        assert blk.state()[3:] == (r.mute, 2000 % LEN)
        del blk
        g.ctcss_squelch_ff(8000, 100.0, 0.01, 1 << 20)                  # never used
    gc.collect()


def test_destroy_with_work_queued(gpu):
    import torch
    g = gpu
    x = piece()
    r = ct.CtcssSquelch(RATE, 100.0, 0.01, LEN, 64, False)
    want = r.work(x)
    d_in = torch.from_numpy(np.tile(x, 64)).cuda()
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        d_out = torch.zeros(64 * len(x), dtype=torch.float32, device="cuda")
        d_p = torch.zeros(64, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        blk = g.ctcss_squelch_ff(RATE, 100.0, 0.01, LEN, 64, False)
        blk.set_mode(mode)
        blk.set_streams(64)
        blk.work_device(len(x), d_in, d_out, d_p, st)
        del blk                                                         # no synchronisation before the handle goes
        gc.collect()
        st.synchronize()
        assert d_p.cpu().tolist() == [len(x)] * 64
        out = d_out.cpu().numpy().view(np.uint32).reshape(64, len(x))
        assert np.array_equal(out, np.tile(want.view(np.uint32), (64, 1))), mode


CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import grhip_loader
g = grhip_loader.import_grhip()
x = (0.1 * np.sin(2 * np.pi * 100.0 * np.arange(4000) / 500)).astype(np.float32)
for L in (250, 5000):
    b = g.ctcss_squelch_ff(500, 100.0, 0.01, L, 7, True)
    b.set_streams(2)
    y = b.work(np.concatenate([x, 0 * x]))
    assert len(y[1]) == 0 and (len(y[0]) == 4000 - (L - 1) if L == 250 else len(y[0]) == 0), (L, len(y[0]), len(y[1]))
    del b
for b in (g.ctcss_squelch_ff(8000, 100.0), g.ctcss_squelch_ff(8000, 67.0, 0.5, 1, 3, True)):
    del b
print("child ok")
"""


def test_create_and_destroy_in_a_child_process(gpu):
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout
