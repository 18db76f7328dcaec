"""CPU tests of gr_fractional_interpolator_{ff,cc}: the restatement (tests/fractional_interp_ref.py) against outputs of
the reference's own code (tests/golden/ref_fractional_interp.npz), the index schedule (closed form vs the reference's
walk) and the predicate that chooses between them, the whole-stream rule, and the product's names and refusals
without a GPU.

The walk is the reference's: `double s = d_mu + d_mu_inc` adds two floats, so the sum is rounded to float before it
is widened (the fixture, made by compiling that loop, pins it: test_fixture_needs_the_float_sum).  A closed form on
the 2^-24 grid therefore equals the walk only while no float sum rounds -- mu and mu_inc multiples of a power of two g
with 1 + mu_inc <= 2^24 * g -- not for every mu_inc >= 0.5: 147/160.f from phase 0 rounds within a few outputs (its
last bit is 2^-24 and the sums pass 1), 1.0001f has a last bit of 2^-23 and rounds once a sum passes 2, and every
ratio rounds from a phase of 2^-24; 1.3f, 160/147.f, 4.8f and 1000.7f happen to end in enough zero bits to be exact
from phase 0, 0.5 or 1.  So the closed form is compared with the walk wherever
the predicate admits it, the predicate is checked against the walk itself over the whole list (no sum of the 3000
steps may round where it admits a pair), and what the product schedules is compared with the walk everywhere.
"""
import os
import re

import numpy as np
import pytest

import fractional_interp_ref as fr

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def on_grid(v):
    """v rounded to float, then to the 2^-24 grid"""
    return f32(np.round(float(f32(v)) * 2 ** 24) / 2 ** 24)


PHASES = [f32(0.0), f32(2.0 ** -24), f32(0.5), on_grid(0.37), on_grid(0.999)]
RATIOS = [f32(0.3), f32(0.5), f32(0.75), f32(0.9999), f32(1.0), f32(1.0001), f32(1.3), f32(160.0 / 147.0),
          f32(147.0 / 160.0), f32(2.5), f32(4.8), f32(10.0), f32(1000.7)]
OFF_GRID = [(f32(0.1), f32(1.0)), (f32(0.1), f32(10.0)), (f32(0.0), f32(0.01)), (f32(0.37), f32(0.01)),
            (f32(0.0), f32(0.001)), (f32(0.5), f32(0.001))]
N_OUT = 3000


def _bits(a):
    return np.asarray(a).view(np.uint32 if np.asarray(a).dtype.itemsize % 8 else np.uint64)


def _same(a, b):
    (i1, m1, u1), (i2, m2, u2) = a, b
    return np.array_equal(i1, i2) and np.array_equal(m1, m2) and np.array_equal(u1.view(np.uint32), u2.view(np.uint32))


def _exact_walk(phase, ratio, n):
    """True when none of the first n float sums of the walk rounds"""
    mu, inc = f32(phase), f32(ratio)
    for _ in range(n):
        if float(f32(mu + inc)) != float(mu) + float(inc):
            return False
        mu, _i = fr.walk_step(mu, inc)
    return True


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "ref_fractional_interp.npz"))


def test_restatement_equals_reference_fixture(fixture):
    d = fixture
    assert len(d["phase"]) == 4 and f32(1.0) in d["phase"]
    for i, (ph, ra, n) in enumerate(zip(d["phase"], d["ratio"], d["nout"])):
        (ii, imu, mu), (ii_end, mu_end) = fr.walk_schedule(ph, ra, n_outputs=int(n))
        assert np.array_equal(ii, d["pos_%d" % i]), i
        assert ii_end == int(d["consumed_%d" % i]), i
        assert f32(mu_end).view(np.uint32) == f32(d["mu_end_%d" % i]).view(np.uint32), i
        for kind, x in (("ff", d["x_ff"]), ("cc", d["x_cc"])):
            got = fr.eval_schedule(x, ii, imu)
            ref = d["out_%s_%d" % (kind, i)]
            assert got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref)), (kind, i)
            # the block itself, in one call with all the input and in forecast-sized calls
            blk = fr.FractionalInterpolatorRef(ph, ra, kind == "cc")
            out, consumed = blk.general_work(int(n), x)
            assert np.array_equal(_bits(out), _bits(ref)) and consumed == ii_end and blk.d_skip == 0
            blk = fr.FractionalInterpolatorRef(ph, ra, kind == "cc")
            outs, rd = [], 0
            while sum(map(len, outs)) < int(n):
                nout = min(257, int(n) - sum(map(len, outs)))
                out, consumed = blk.general_work(nout, x[rd:rd + blk.forecast(nout)])
                assert len(out) == nout and blk.d_skip == 0          # forecast honoured: always noutput_items
                outs.append(out); rd += consumed
            assert np.array_equal(_bits(np.concatenate(outs)), _bits(ref)) and rd == ii_end


def test_fixture_needs_the_float_sum(fixture):
    """with the sum taken in double (and the narrowing of s - f rounding instead) the positions of the reference's
    160/147 run are not reproduced: the fixture tells the two readings of .cc:83 apart"""
    d = fixture
    ph, ra, n = d["phase"][0], d["ratio"][0], int(d["nout"][0])
    mu, ii, pos = f32(ph), 0, []
    for _ in range(n):
        pos.append(ii)
        s = float(mu) + float(ra)
        f = np.floor(s)
        mu = f32(s - f)
        ii += int(f)
    assert not fr.closed_form_ok(ph, ra)
    assert not np.array_equal(np.array(pos), d["pos_0"]) or ii != int(d["consumed_0"]) or \
        f32(mu).view(np.uint32) != f32(d["mu_end_0"]).view(np.uint32)


@pytest.mark.parametrize("ratio", RATIOS)
def test_closed_form_equals_walk_where_admitted(ratio):
    for phase in PHASES + [f32(1.0)]:
        walk = fr.walk_schedule(phase, ratio, n_outputs=N_OUT)[0]
        if fr.closed_form_ok(phase, ratio):
            assert _same(fr.closed_form_schedule(phase, ratio, N_OUT), walk), (phase, ratio)
        assert _same(fr.schedule(phase, ratio, N_OUT), walk), (phase, ratio)


@pytest.mark.parametrize("ratio", RATIOS)
def test_phase_one_first_output(ratio):
    (ii, imu, mu), _end = fr.walk_schedule(f32(1.0), ratio, n_outputs=N_OUT)
    assert ii[0] == 0 and imu[0] == 128                 # filter 128 at offset 0, not filter 0 at offset 1
    assert _same(fr.schedule(f32(1.0), ratio, N_OUT), (ii, imu, mu))
    if fr.closed_form_ok(f32(1.0), ratio):
        c = fr.closed_form_schedule(f32(1.0), ratio, N_OUT)
        assert c[0][0] == 0 and c[1][0] == 128 and _same(c, (ii, imu, mu))


def test_grid_predicate():
    # off the 2^-24 grid, or on it with sums that round: the walk
    for phase, ratio in OFF_GRID:
        assert not fr.closed_form_ok(phase, ratio), (phase, ratio)
    # dyadic ratios from dyadic phases: the closed form
    for ratio in (0.5, 0.75, 1.0, 1.25, 2.0, 2.5, 10.0, 4.0, 8.0):
        for phase in (0.0, 0.5, 0.25, 1.0):
            assert fr.closed_form_ok(f32(phase), f32(ratio)), (phase, ratio)
    # over the whole list: where the predicate admits a pair none of the walk's 3000 sums rounds, and where a sum
    # does round it sends the pair to the walk.  (It is a sufficient condition: (0, 1.0001f) stays exact for 3000
    # steps only because mu has not reached 1 - 2^-23 * k yet, and goes to the walk.)
    admitted = rounding = 0
    for ratio in RATIOS:
        for phase in PHASES + [f32(1.0)]:
            ok, exact = fr.closed_form_ok(phase, ratio), _exact_walk(phase, ratio, N_OUT)
            admitted += ok
            rounding += not exact
            assert exact or not ok, (phase, ratio)
    assert admitted >= 12 and rounding >= 12
    # a phase of 2^-24 rounds at the first sum that reaches 1.0, and so does a ratio with an odd last bit such as
    # 147/160.f from 0: mu_inc >= 0.5 alone does not make the sums exact
    assert not fr.closed_form_ok(f32(2.0 ** -24), f32(0.5)) and not _exact_walk(f32(2.0 ** -24), f32(0.5), 10)
    assert not fr.closed_form_ok(f32(0.0), f32(147.0 / 160.0)) and not _exact_walk(f32(0.0), f32(147.0 / 160.0), 10)
    # every ratio of the list keeps phase 0 on the closed form when its own grid is coarse enough for 1 + ratio
    for ratio in (0.5, 0.75, 0.9999, 1.0, 1.3, 160.0 / 147.0, 2.5, 4.8, 10.0, 1000.7):
        assert fr.closed_form_ok(f32(0.0), f32(ratio)), ratio


def test_forecast_is_the_float_expression():
    assert fr.forecast(0, f32(1.0)) == 8
    assert fr.forecast(100, f32(0.5)) == 58
    assert fr.forecast(3, f32(0.3)) == 9                # ceil(0.90000004 + 8) in float: 8.900001 -> 9
    assert fr.forecast(1 << 24, f32(1.0)) == (1 << 24) + 8
    assert fr.forecast((1 << 24) + 1, f32(1.0)) == (1 << 24) + 8     # the int does not fit a float


CASES = [(f32(0.0), f32(1.25), False), (f32(0.37), f32(160.0 / 147.0), True), (f32(1.0), f32(0.75), True),
         (f32(0.1), f32(10.0), False), (f32(0.0), f32(0.3), True), (f32(0.5), f32(1000.7), False),
         (f32(0.0), f32(0.01), False)]


@pytest.mark.parametrize("phase,ratio,cplx", CASES)
def test_whole_stream_rule_independent_of_call_sizes(phase, ratio, cplx):
    rng = np.random.default_rng(int(float(ratio) * 1000))
    N = 3000 if ratio > 0.1 else 60
    x = rng.standard_normal(N).astype(f32)
    if cplx:
        x = (x + 1j * rng.standard_normal(N)).astype(np.complex64)
    ii, imu, _mu = fr.whole_stream_schedule(phase, ratio, N)
    assert len(ii) > 0 and ii[-1] + 8 <= N
    ref = fr.eval_schedule(x, ii, imu)
    whole, rd = fr.run_calls(fr.FractionalInterpolatorRef(phase, ratio, cplx), x, [(1 << 30, None)])
    assert np.array_equal(_bits(whole), _bits(ref))      # exactly the outputs with ii_k + 8 <= N
    patterns = [
        [(1, None)],                                       # one output per call
        [(5, 1), (5, None)],                               # one-input calls in between: no progress, no harm
        [(7, None), (1, None), (3, 40)],
        [(64, "forecast-1"), (64, "forecast")],
        [(4096, 100), (65536, 17), (5, None)],
        [(int(a), int(b)) for a, b in zip(rng.integers(1, 300, 50), rng.integers(1, 400, 50))] + [(1 << 20, None)],
    ]
    for sizes in patterns:
        got, rd2 = fr.run_calls(fr.FractionalInterpolatorRef(phase, ratio, cplx), x, sizes)
        assert np.array_equal(_bits(got), _bits(whole)), sizes
        assert rd2 == rd, sizes


def test_short_call_carries_what_it_could_not_consume():
    blk = fr.FractionalInterpolatorRef(0.0, 1000.5, False)
    sched, consumed = blk.schedule_call(10, 100)          # one output at 0, then a jump of 1000 items
    assert len(sched) == 1 and consumed == 100 and blk.d_skip == 900
    sched, consumed = blk.schedule_call(10, 500)
    assert sched == [] and consumed == 500 and blk.d_skip == 400
    sched, consumed = blk.schedule_call(10, 408)
    assert [s[0] for s in sched] == [400] and consumed == 408


API_NAMES = ["create", "destroy", "set_mu", "set_interp_ratio", "mu", "interp_ratio", "set_mode", "history", "forecast",
             "general_work", "general_work_device", "run_captures_device"]


@pytest.mark.parametrize("suf", ["ff", "cc"])
def test_api_names_in_header_and_library(g, suf):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    L = g.lib()
    for n in API_NAMES:
        name = "grhip_fractional_interpolator_%s_%s" % (suf, n)
        assert re.search(r"GRHIP_API\s+\w+\s+\*?%s\(" % name, hdr), name
        assert getattr(L, name) is not None, name
    assert hasattr(g, "fractional_interpolator_" + suf)


@pytest.mark.parametrize("cls", ["fractional_interpolator_ff", "fractional_interpolator_cc"])
def test_no_cpu_fallback_without_device(g, cls):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(g.GrhipError) as e:
        getattr(g, cls)(0.0, 1.25)
    assert e.value.code == -5      # GRHIP_ENODEV
    assert "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("cls", ["fractional_interpolator_ff", "fractional_interpolator_cc"])
@pytest.mark.parametrize("phase,ratio,code", [(0.0, 0.0, -2), (0.0, -1.0, -2), (0.0, float("nan"), -2),
                                              (0.0, float("inf"), -2), (-0.1, 1.0, -2), (1.1, 1.0, -2),
                                              (float("nan"), 1.0, -2), (0.0, 2.0 ** 20, -1), (0.0, 3e6, -1)])
def test_bad_arguments_refused_before_the_device(g, cls, phase, ratio, code):
    with pytest.raises(g.GrhipError) as e:
        getattr(g, cls)(phase, ratio)
    assert e.value.code == code    # GRHIP_ERANGE / GRHIP_EINVAL, with or without a GPU
