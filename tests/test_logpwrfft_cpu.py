"""CPU tests of blks2.logpwrfft_c / _f: the window, k and the decimation rule against values recorded from the reference's
own closure (tests/golden/ref_logpwrfft.json), the declared entries, the refused arguments, and the fused-versus-composed
addressing predicate (csrc/logpwr_plan.h) as a sanitized program of its own."""
import ctypes as C
import json
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import logpwrfft_ref as lr

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "gnuradio-3.5.0-dmr_amd", "host")
FIX = json.load(open(os.path.join(HERE, "golden", "ref_logpwrfft.json")))


def _d(h):
    return struct.unpack(">d", bytes.fromhex(h))[0]


def _ulps(a, b):
    """distance in double ulps between two doubles of the same sign (or zero)"""
    ia, ib = (struct.unpack("<q", struct.pack("<d", v))[0] for v in (a, b))
    return abs(ia - ib)


def _check_window(w, case):
    want = [_d(h) for h in case["window"]]
    assert len(w) == len(want)
    # libm's cos may differ between hosts: the doubles within 1 ulp, their float narrowing bit for bit
    assert max(_ulps(float(a), b) for a, b in zip(w, want)) <= 1
    got32 = np.asarray(w, np.float64).astype(np.float32).view(np.uint32)
    assert ["%08x" % v for v in got32] == case["window_f32"]


@pytest.mark.parametrize("case", FIX["cases"], ids=lambda c: "N%d" % c["fft_size"])
def test_restatement_equals_the_fixture(case):
    n = case["fft_size"]
    w = lr.blackmanharris(n)
    _check_window(w, case)
    # The window's doubles may each be 1 ulp off (libm's cos), so their squares up to 2 ulps and the sum of n of them,
    # all positive, up to 2 ulps of the sum plus its own n roundings either way: (n + 2) ulps at most.  Where libm agrees
    # with the recording (the usual case) the difference is 0.
    wp, wp_ref = lr.window_power(w), _d(case["window_power"])
    print("N %d: window_power %d ulps from the recording" % (n, _ulps(wp, wp_ref)))
    assert _ulps(wp, wp_ref) <= n + 2
    for e in case["k"]:
        k, k_ref = lr.k_of(n, w, e["ref_scale"]), _d(e["k_f64"])
        assert "%08x" % np.float32(k).view(np.uint32) == e["k_f32"]
        # k moves by 10 / ln 10 times the relative error of window_power, (n + 2) 2^-52 at most, plus one rounding of each
        # of its three terms and two of their sum: 5 ulps of the largest magnitude involved
        bound = 10 / math.log(10) * (n + 2) * 2.0 ** -52 + 5 * np.spacing(max(abs(k_ref), 20 * math.log10(n)))
        assert abs(k - k_ref) <= bound


def test_issue_figures():
    w = lr.blackmanharris(4096)
    assert lr.window_power(w) == pytest.approx(1056.3599385238522, rel=1e-14)
    assert lr.k_of(4096, w, 2.0) == pytest.approx(-66.3617187, abs=1e-6)
    assert lr.k_of(32, lr.blackmanharris(32), 2.0) == pytest.approx(-24.0806969, abs=1e-6)


def test_decimation_rule():
    # max(1, int(round(sample_rate / vec_len / vec_rate))), half away from zero, true division
    assert lr.decimation_of(10e6, 4096, 30) == 81
    assert lr.decimation_of(10e6, 1024, 30) == 326
    assert lr.decimation_of(5, 1, 2) == 3           # 2.5 rounds away from zero (Python 3's round gives 2)
    assert lr.decimation_of(3, 1, 2) == 2           # 1.5
    assert lr.decimation_of(1, 64, 30) == 1         # never below 1


@pytest.mark.parametrize("case", FIX["cases"], ids=lambda c: "N%d" % c["fft_size"])
def test_library_window_equals_the_fixture(g, case):
    _check_window(g.window_blackmanharris(case["fft_size"]), case)


def test_window_refusals(g):
    with pytest.raises(g.GrhipError) as e:
        g.window_blackmanharris(1)
    assert e.value.code == -1                       # GRHIP_EINVAL: the reference divides by fft_size - 1
    assert len(g.window_blackmanharris(0)) == 0


def test_entries_are_declared_and_exported(g):
    src = open(os.path.join(os.path.dirname(HERE), "include", "grhip.h")).read()
    lib = g.lib()
    names = ["grhip_window_blackmanharris"]
    for kind in ("c", "f"):
        for fn in ("create", "destroy", "set_mode", "set_streams", "set_decimation", "set_vec_rate", "set_sample_rate",
                   "set_average", "set_avg_alpha", "sample_rate", "decimation", "frame_rate", "average", "avg_alpha",
                   "produced", "work", "work_device"):
            names.append("grhip_logpwrfft_%s_%s" % (kind, fn))
    for n in names:
        assert n + "(" in src, n
        assert hasattr(lib, n), n


@pytest.mark.parametrize("cls", ["logpwrfft_c", "logpwrfft_f"])
def test_bad_arguments_are_refused_before_any_device_work(g, cls):
    """every refusal below comes back with its own code whether or not a device is visible (without one a valid create
    ends in GRHIP_ENODEV, -5)"""
    mk = getattr(g, cls)
    ok = dict(sample_rate=1e6, fft_size=64, ref_scale=2.0, frame_rate=30, avg_alpha=0.2, average=True)
    for change, code in (({"fft_size": 0}, -2), ({"fft_size": -4}, -2), ({"avg_alpha": 1.5}, -2), ({"avg_alpha": -1e-9}, -2),
                         ({"ref_scale": 0.0}, -1), ({"ref_scale": -1.0}, -1), ({"fft_size": 1}, -1),
                         ({"win": [0.0] * 64}, -1), ({"frame_rate": 0.0}, -1)):
        with pytest.raises(g.GrhipError) as e:
            mk(**dict(ok, **change))
        assert e.value.code == code, (change, e.value.code)
    if g.device_count() == 0:
        with pytest.raises(g.GrhipError) as e:
            mk(**ok)
        assert e.value.code == -5


def test_addressing_predicate():
    r = subprocess.run(["make", "-C", HOST, "logpwr_plan_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([os.path.join(HOST, "logpwr_plan_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
