"""CPU tests of the spectrum-estimate blocks: the numpy restatements (spectrum_ref.py) against the reference's own QA
vectors (tests/golden/ref_qa_spectrum.json) and against outputs recorded from the reference's single-pole IIR header
(tests/golden/ref_single_pole_iir_header.json), the keep-one countdown, and the new entries' presence and argument checks, which need no device."""
import json
import os
import re

import numpy as np
import pytest

import spectrum_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
QA = json.load(open(os.path.join(HERE, "golden", "ref_qa_spectrum.json")))
HDR = json.load(open(os.path.join(HERE, "golden", "ref_single_pole_iir_header.json")))
f32 = np.float32


def _almost(got, want, places):
    # assertFloatTuplesAlmostEqual(places): round(|a - b|, places) == 0
    return len(got) == len(want) and all(round(abs(float(a) - float(b)), places) == 0 for a, b in zip(got, want))


@pytest.mark.parametrize("case", QA["single_pole_iir"], ids=lambda c: c["name"])
def test_iir_restatement_matches_qa(case):
    got = sr.SinglePoleIir(case["alpha"], case["vlen"]).work(np.array(case["src"], f32))
    assert _almost(got, case["expected"], case["places"]), got


def test_nlog10_and_mag_squared_restatements_match_qa():
    c = QA["nlog10"][0]
    assert _almost(sr.nlog10(c["src"], c["n"], c["k"]), c["expected"], c["places"])
    # the float64 form keeps the float clamp's own error (1e-18f is not 1e-18): 6 places
    assert _almost(sr.nlog10_f64(c["src"], c["n"], c["k"]), c["expected"], 6)
    c = QA["complex_to_mag_squared"][0]
    z = np.array([complex(a, b) for a, b in c["src"]], np.complex64)
    assert _almost(sr.mag_squared(z), c["expected"], c["places"])
    assert np.isnan(sr.nlog10([np.nan], 10)[0])


@pytest.mark.parametrize("case", HDR["cases"], ids=lambda c: "alpha=%g" % c["alpha"])
def test_iir_restatement_matches_the_compiled_header_bit_for_bit(case):
    x = np.array(HDR["input_bits"], np.uint32).view(f32)
    want = np.array(case["output_bits"], np.uint32)
    blk = sr.SinglePoleIir(case["alpha"])
    got = np.concatenate([blk.work(x[:11]), blk.work(x[11:])])             # the state carries across calls
    assert np.array_equal(got.view(np.uint32), want)


def test_keep_one_counter_across_calls_and_set_n():
    k = sr.KeepOneInN(3)
    assert k.kept(4) == [2] and k.kept(1) == [] and k.kept(5) == [0, 3]
    k.set_n(2)                                                  # reloads the countdown
    assert k.kept(3) == [1] and k.kept(2) == [0]
    k.set_n(0)                                                  # clamped to 1
    assert k.kept(3) == [0, 1, 2]
    whole = sr.KeepOneInN(7).kept(100)
    parts = sr.KeepOneInN(7)
    assert [i for i in parts.kept(5)] + [5 + i for i in parts.kept(1)] + [6 + i for i in parts.kept(94)] == whole


NEW = ["grhip_complex_to_mag_squared", "grhip_single_pole_iir_filter_ff", "grhip_nlog10_ff", "grhip_keep_one_in_n"]


def test_new_entries_are_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(n for n in re.findall(r"\b(grhip_[a-z0-9_]+)\s*\(", hdr) if any(n.startswith(p + "_") for p in NEW)))
    for p in NEW:
        for op in ("create", "destroy", "work", "work_device", "set_streams"):
            assert "%s_%s" % (p, op) in names
    for extra in ("grhip_keep_one_in_n_produced", "grhip_keep_one_in_n_set_n", "grhip_single_pole_iir_filter_ff_set_taps",
                  "grhip_single_pole_iir_filter_ff_chunk"):
        assert extra in names
    lib = g.lib()
    assert not [n for n in names if not hasattr(lib, n)]


def test_bad_arguments_are_refused_before_the_device(g):
    for make in (lambda: g.single_pole_iir_filter_ff(1.5), lambda: g.single_pole_iir_filter_ff(-0.1, 4)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -2, str(e.value)                 # GRHIP_ERANGE
    for make in (lambda: g.complex_to_mag_squared(0), lambda: g.nlog10_ff(10, 0), lambda: g.keep_one_in_n(0, 3)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -1, str(e.value)                 # GRHIP_EINVAL


def test_new_entries_refuse_to_run_without_a_device(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    for make in (lambda: g.complex_to_mag_squared(), lambda: g.single_pole_iir_filter_ff(0.5), lambda: g.nlog10_ff(10),
                 lambda: g.keep_one_in_n(8, 3)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
