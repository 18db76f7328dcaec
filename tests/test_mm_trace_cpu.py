"""The reference traces of tests/mm_trace.py are the reference: the oracle's tracing entry of clock_recovery_mm_cc is
a second writing of its loop, pinned here bit for bit to po.ClockRecoveryMMcc in one whole call on every _cc input
of the GPU tests; the _ff walk (one output per call) is pinned to the one long call; and every case meets, on the
CPU alone, the conditions its GPU test asserts before it looks at a kernel."""
import numpy as np
import pytest

import mm_trace as mt
from conftest import bits_equal


@pytest.mark.parametrize("want_error", [False, True])
@pytest.mark.parametrize("name", sorted(mt.cc_cases()))
def test_cc_trace_is_the_oracle_in_one_call(po, name, want_error):
    params, x, nout, floors = mt.cc_cases()[name]
    ref = po.ClockRecoveryMMcc(*params)
    y, e, c = ref.general_work(nout, x, want_error)
    tr = mt.trace_cc(po, params, x, nout, want_error)
    assert len(y) > 0 and bits_equal(tr.out, y) and tr.consumed == c
    if want_error:
        assert bits_equal(tr.err, e)
    else:
        assert tr.err is None
    assert tr.mu.tobytes() == ref.mu().tobytes() and tr.omega.tobytes() == ref.omega().tobytes()
    assert len(tr.pos) == len(y) + 1 and tr.pos[0] == 0 and max(int(tr.pos[-1]), 0) == c
    mt.assert_conditions(tr.regimes(), floors[want_error])


@pytest.mark.parametrize("name", sorted(mt.ff_cases()))
def test_ff_walk_is_the_oracle_in_one_call(po, name):
    params, x, nout, floor = mt.ff_cases()[name]
    tr = mt.trace_ff(po, params, x, nout)
    reg = tr.regimes()
    mt.assert_conditions(reg, floor)                   # (position never below 0: the one long call is well defined)
    ref = po.ClockRecoveryMM(*params)
    y, c = ref.general_work(nout, x)
    assert len(y) > 0 and bits_equal(tr.out, y) and tr.consumed == c
    assert tr.mu == ref.state["mu"] and tr.omega == ref.state["omega"]
    if name in mt.FF_FORWARD_ONLY:
        assert reg["back"] == 0


def test_ff_case_that_ends_below_zero(po):
    params, x, nout = mt.ff_below_zero_case()
    tr = mt.trace_ff(po, params, x, nout)
    assert tr.below_zero and tr.pos[-1] < 0 and (tr.pos[:-1] >= 0).all()
    assert 2 <= len(tr.out) < 100                      # a few symbols, then the end


def test_regime_counts():
    tr = mt.Trace(np.zeros(6, np.float32), [0, 10, 10, 7, 80, 2200, 4300], 4300, 0, 0, clamps=2)
    r = tr.regimes()
    assert (r["symbols"], r["min_pos"], r["back"], r["zero"], r["clamps"]) == (6, 0, 1, 1, 2)
    assert (r["gt64"], r["gt256"], r["gt512"], r["gt1024"], r["gt2048"]) == (3, 2, 2, 2, 2)
    assert r["first_window"] == 5
    with pytest.raises(AssertionError):
        mt.assert_conditions(r, {"back": 2})
    with pytest.raises(AssertionError):
        mt.assert_conditions(mt.Trace(np.zeros(1, np.float32), [0, -3], -3, 0, 0).regimes(), {})
