"""CPU tests of dc_blocker / moving_average / integrate: the numpy restatements (running_sum_ref.py) against the
reference's own QA vectors (tests/golden/ref_qa_running_sum.json), the float64 forms against a direct FIR, and the
new entries' argument checks, which need no device.

The reference has no QA for gr_moving_average_XX; that restatement is pinned by a case evaluated by hand in float32
(test_moving_average_hand_case)."""
import json
import os

import numpy as np
import pytest

import running_sum_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
QA = json.load(open(os.path.join(HERE, "golden", "ref_qa_running_sum.json")))
f32 = np.float32


def _cplx(v):
    return np.array([complex(a, b) for a, b in v])


def test_cumsum_float32_is_sequential():
    rng = np.random.default_rng(1)
    a = (rng.uniform(-1, 1, 5000) + 10).astype(f32)
    s, want = f32(0), np.empty(5000, f32)
    for i, v in enumerate(a):
        s = f32(s + v)
        want[i] = s
    assert np.array_equal(np.cumsum(a, dtype=f32).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("case", QA["dc_blocker"], ids=lambda c: c["name"])
def test_dc_blocker_restatement_matches_qa(case):
    cc = case["kind"] == "cc"
    src = np.array([case["src"]["impulse"]] + [0] * case["src"]["zeros"], dtype=np.complex64 if cc else f32)
    blk = rr.DcBlocker(case["D"], case["long_form"], cc)
    got = blk.work(src)[case["slice"][0]:case["slice"][1]]
    want = _cplx(case["expected"]) if cc else np.array(case["expected"])
    # assertFloatTuplesAlmostEqual(places=7): round(|a - b|, 7) == 0
    assert all(round(abs(complex(a) - complex(b)), case["places"]) == 0 for a, b in zip(got, want)), (got, want)
    assert blk.get_group_delay() == (case["slice"][0] + 2)      # the QA looks "around 2D-2" / "around D-1"


@pytest.mark.parametrize("case", QA["integrate"], ids=lambda c: c["name"])
def test_integrate_restatement_matches_qa(case):
    k = case["kind"]
    src = _cplx(case["src"]).astype(np.complex64) if k == "cc" else np.array(case["src"])
    want = _cplx(case["expected"]) if k == "cc" else np.array(case["expected"])
    got = rr.integrate(k, src, case["decim"], len(want))
    assert np.array_equal(got, want)                            # exact: stricter than the QA's 6 places for ff / cc


def test_moving_average_hand_case():
    # length 3, scale 0.5, float32 by hand.  2^24 + 1 is not a float: sum = 0 + 2^24 = 16777216; + 1 -> 16777216 (tie to
    # even); then the loop: + 1 -> 16777216, out 8388608, - 2^24 -> 0; + 3 -> 3, out 1.5, - 1 -> 2; + 0.25 -> 2.25, out 1.125.
    x = np.array([2.0 ** 24, 1.0, 1.0, 3.0, 0.25], dtype=f32)
    got = rr.moving_average_work("ff", x, 3, 0.5, 3)
    assert got.tolist() == [8388608.0, 1.5, 1.125]
    # the float64 filter says (2^24 + 2) / 2, 2.5, 2.125: the recurrence carries its rounding error on
    assert rr.moving_average_f64(x, 3, 0.5, 3).tolist() == [8388609.0, 2.5, 2.125]
    # a new work call starts its sum again: outputs 1 and 2 as calls of their own
    assert rr.moving_average_calls("ff", x, 3, 0.5, 3, max_iter=1).tolist() == [8388608.0, 2.5, 2.125]
    # short wraps in the sum and in the product; int likewise
    s = np.array([32767, 1, 2, -32768], dtype=np.int16)
    # 32767 + 1 -> -32768, * 3 = -98304 -> -32768;  1 + 2 = 3 -> 9;  2 - 32768 = -32766, * 3 = -98298 -> -32762
    assert rr.moving_average_work("ss", s, 2, 3, 3).tolist() == [-32768, 9, -32762]
    i = np.array([2 ** 31 - 1, 1, 5], dtype=np.int32)
    assert rr.moving_average_work("ii", i, 2, 2, 2).tolist() == [0, 12]
    # complex scale: the product of std::complex
    z = np.array([1 + 2j, 3 - 1j], dtype=np.complex64)
    assert rr.moving_average_work("cc", z, 2, 0.5 + 0.5j, 1).tolist() == [(4 + 1j) * (0.5 + 0.5j)]


@pytest.mark.parametrize("long_form", [True, False])
@pytest.mark.parametrize("D", [1, 2, 3, 32, 33])
def test_float64_form_is_the_fir(D, long_form):
    rng = np.random.default_rng(D)
    x = rng.uniform(-1, 1, 700) + 10
    got = rr.DcBlocker(D, long_form, False, np.float64).work(x)
    want = np.convolve(x, rr.dc_blocker_taps(D, long_form))[:len(x)]
    assert np.abs(got - want).max() < 1e-11 * 10
    # in two calls: the state carries
    b = rr.DcBlocker(D, long_form, False, np.float64)
    assert np.array_equal(np.concatenate([b.work(x[:D + 1]), b.work(x[D + 1:])]), got)
    # and the float32 recurrence is that filter up to its drift
    g32 = rr.DcBlocker(D, long_form, False, f32).work(x.astype(f32))
    assert np.abs(g32 - rr.DcBlocker(D, long_form, False, np.float64).work(x.astype(f32))).max() < 1e-4


def test_float64_moving_average_and_integrate_are_the_fir():
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, 300)
    assert np.abs(rr.moving_average_f64(x, 10, 0.1, 291) - np.convolve(x, np.full(10, 0.1), "valid")).max() < 1e-14
    assert np.abs(rr.integrate_f64(x, 10, 30) - x.reshape(30, 10).sum(axis=1)).max() < 1e-14


def test_bad_arguments_are_refused_before_the_device(g):
    # GRHIP_EINVAL (-1), checked before any device is touched: the same answer with and without a GPU
    makes = [lambda: g.dc_blocker_ff(0), lambda: g.dc_blocker_cc(-3, False), lambda: g.dc_blocker_ff(1346),
             lambda: g.moving_average_ff(0, 1.0), lambda: g.moving_average_cc(-1, 1j), lambda: g.moving_average_ss(0, 1),
             lambda: g.moving_average_ii(0, 1), lambda: g.moving_average_ff(8450, 1.0), lambda: g.moving_average_ff(4, 1.0, 0),
             lambda: g.integrate_ff(0), lambda: g.integrate_cc(-1), lambda: g.integrate_ss(0), lambda: g.integrate_ii(0)]
    for make in makes:
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1, str(e.value)


def test_new_entries_refuse_to_run_without_a_device(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    for make in (lambda: g.dc_blocker_ff(32, True), lambda: g.dc_blocker_cc(), lambda: g.moving_average_ff(10, 0.1),
                 lambda: g.moving_average_ii(10, 1), lambda: g.integrate_ff(10), lambda: g.integrate_ss(3)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
