"""CPU tests of agc_cc / agc_ff / agc2_cc / agc2_ff: the restatement (agc_ref.py) against outputs recorded from the
reference's own code (tests/golden/ref_agc.npz), the QA vectors of gr/qa_agc.py, the chunked form of agc_cc / agc_ff in
numpy against the float64 recurrence and the serial float one, the composition rule, and the new entries' presence and
argument checks, which need no device.

Test signal (agc_ref.signal(seed)): n = 6037, (standard_normal + j standard_normal) * 0.7 * env from default_rng(seed) as
complex64, env = 1 on [0, 1500), 0 on [1500, 2500), 30 on [2500, 4000) and 0.02 from 4000 on; the _ff blocks take the
real part.  Parameter sets: agc_ref.AGC_SETS and AGC2_SETS.

The fixture was recorded by a throw-away program from the reference's gri_agc_cc.h, gri_agc_ff.h, gri_agc2_cc.h and
gri_agc2_ff.h, compiled unchanged with g++ -O2 against a one-line stub gr_core_api.h (an empty GR_CORE_API).  It holds
  * the input of gr/qa_agc.py test_001 .. 004, 50 samples of a 100-amplitude tone at 0.1 cycles per sample, with the
    four blocks' outputs, all as bit patterns (qa_in_c, qa_in_f, qa_out_<block>).  The tone comes from the reference's
    gr_fxpt_nco.h / gr_fxpt.cc (against a three-line stub gr_types.h), the oscillator that gr_sig_source_c / _f use
    (gengen/gr_sig_source_X.h.t:51): its first sample is 100.000244, as in the QA's expected tuples, where gr_nco.h
    gives 100.0 and misses the QA's 4 places by 2.4e-4;
  * per block, parameter set p, seed s = 1 .. 3 and cut (`one` call, or `two` calls cut at 4097), under the key
    <block>_p<p>_s<s>_<cut>_: gain (the final gain's bits), sha (SHA-256 over the output's bytes), head (the first 64
    outputs' bits) and mid (64 outputs from sample 2490 on).
tests/golden/ref_qa_agc.json holds the four expected_result tuples of qa_agc.py."""
import json
import os
import re

import numpy as np
import pytest

import agc_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = np.load(os.path.join(HERE, "golden", "ref_agc.npz"))
QA = json.load(open(os.path.join(HERE, "golden", "ref_qa_agc.json")))
SEEDS = (1, 2, 3)


def _qa_in(block):
    return FIX["qa_in_c"].view(np.complex64) if R.is_cc(block) else FIX["qa_in_f"].view(np.float32)


def _qa_expected(block):
    e = np.array(QA[block], np.float64)
    return e[:, 0] + 1j * e[:, 1] if e.ndim == 2 else e


@pytest.mark.parametrize("block", R.BLOCKS)
def test_restatement_equals_the_reference_bit_for_bit(block):
    for pi, params in enumerate(R.sets(block)):
        for seed in SEEDS:
            x = R.signal(seed, block)
            assert len(x) == R.N == 6037
            for tag, cuts in (("one", ()), ("two", (4097,))):
                key = "%s_p%d_s%d_%s_" % (block, pi, seed, tag)
                r = R.in_calls(R.serial, block, x, params, cuts)
                assert R.bits(r.out[:64]).tolist() == FIX[key + "head"].tolist(), key
                assert R.bits(r.out[2490:2490 + 64]).tolist() == FIX[key + "mid"].tolist(), key
                assert R.digest(r.out) == bytes(FIX[key + "sha"]).hex(), key
                assert R.bits(r.gains[-1:])[0] == FIX[key + "gain"][0], key


@pytest.mark.parametrize("block", R.BLOCKS)
def test_qa_vectors(block):
    """the recorded outputs equal qa_agc.py's expected tuples to its 4 places, and the restatement equals them bit for bit"""
    x = _qa_in(block)
    got = FIX["qa_out_" + block].view(x.dtype)
    exp = _qa_expected(block)
    assert len(x) == len(got) == len(exp) == 50
    for a, b in zip(got, exp):
        assert round(abs(complex(a) - complex(b)), 4) == 0       # assertComplexTuplesAlmostEqual(..., 4)
    params = (1e-2, 1e-3, 1, 1, 1000) if block.startswith("agc2") else (1e-3, 1, 1, 1000)
    assert R.bits(R.serial(block, x, params).out).tolist() == FIX["qa_out_" + block].tolist()


def test_the_signal_exercises_the_clamp_the_flags_and_the_negative_gain():
    for block in ("agc_cc", "agc_ff"):
        for seed in SEEDS:
            x = R.signal(seed, block)
            runs = [R.serial(block, x, p) for p in R.AGC_SETS]
            assert runs[0].clamped == 0 and runs[1].clamped == 0
            # the third set clamps a few per cent of the samples (2 % of the complex ones), the fifth a quarter or more
            assert 0.02 <= runs[2].clamped / R.N <= 0.10, (block, seed, runs[2].clamped)
            if block == "agc_cc":
                assert 0.02 <= runs[2].clamped / R.N <= 0.03
                assert 0.24 <= runs[4].clamped / R.N <= 0.26
            assert runs[4].clamped / R.N >= 0.24
            # the fourth: rate |x| reaches 1.4 .. 1.7 (to one decimal), 5 .. 7 chunks are flagged, the gain goes negative and stays finite
            rate = float(np.float32(R.AGC_SETS[3][0]))
            peak = rate * R.mag64(x).max()
            assert 1.35 <= peak <= 1.75, (block, seed, peak)
            _, flags = R.chunk_triples(block, x, R.AGC_SETS[3])
            assert 5 <= sum(flags) <= 7, (block, seed, sum(flags))
            assert -0.035 <= runs[3].gains.min() <= -0.005, (block, seed, runs[3].gains.min())
            assert np.isfinite(runs[3].gains).all() and np.isfinite(R.bits(runs[3].out).view(np.float32)).all()
            for k in (0, 1, 2, 4):
                assert runs[k].gains.min() > 0 and not any(R.chunk_triples(block, x, R.AGC_SETS[k])[1])


def test_agc2_reset_fires():
    for block in ("agc2_cc", "agc2_ff"):
        for seed in SEEDS:
            x = R.signal(seed, block)
            assert R.serial(block, x, R.AGC2_SETS[0]).resets == 0
            assert R.serial(block, x, R.AGC2_SETS[2]).resets > 100


def test_the_two_agc2_rate_tests_differ():
    # tmp = -0.9 against a gain of 0.5: agc2_cc compares tmp, agc2_ff its magnitude (gri_agc2_cc.h:60, gri_agc2_ff.h:60)
    p = (0.5, 0.125, 1.0, 0.5, 0.0)
    cc = R.serial("agc2_cc", np.array([0.2], np.complex64), p)
    ff = R.serial("agc2_ff", np.array([0.2], np.float32), p)
    assert abs(cc.gain - (0.5 + 0.9 * 0.125)) < 1e-6 and abs(ff.gain - (0.5 + 0.9 * 0.5)) < 1e-6      # decay, attack


def test_composition_rule_against_a_walk():
    rng = np.random.default_rng(7)
    for _ in range(200):
        k = int(rng.integers(1, 40))
        maps = [(float(rng.uniform(0, 1.2)), float(rng.uniform(0, 0.5)), float(rng.choice([np.inf, rng.uniform(0.1, 3)])))
                for _ in range(k)]
        t = (1.0, 0.0, np.inf)
        for m in maps:
            t = R.compose(t, m)
        # associativity: the same product from the right
        u = maps[-1]
        for m in maps[-2::-1]:
            u = R.compose(m, u)
        for g in rng.uniform(0, 4, 5):
            w = float(g)
            for m in maps:
                w = R.apply(m, w)
            assert abs(R.apply(t, float(g)) - w) <= 1e-12 * max(1.0, abs(w))
            assert abs(R.apply(u, float(g)) - w) <= 1e-12 * max(1.0, abs(w))
    # a zero factor behind an unclamped map: no 0 * inf
    assert R.compose((0.5, 1.0, np.inf), (0.0, 0.25, 2.0)) == (0.0, 0.25, 2.0)


@pytest.mark.parametrize("block", ("agc_cc", "agc_ff"))
def test_chunked_form_is_as_close_to_float64_as_the_serial_float_walk(block):
    """dev_fast <= 2 dev_ref + 4 * 2^-23 on the gain track, and the outputs within the bound that follows from it.
    Ratios dev_fast / dev_ref measured on this numpy form, seeds 1 .. 3: 0.27 .. 1.08."""
    lines = []
    for pi, params in enumerate(R.AGC_SETS):
        for seed in SEEDS:
            x = R.signal(seed, block)
            g64 = R.exact64(block, x, params)
            dev_ref = R.deviation(R.serial(block, x, params).gains, g64)
            for cuts in ((), (257, 4097)):
                f = R.chunked(block, x, params, cuts)
                dev_fast = R.deviation(f.gains, g64)
                lines.append("%s set %d seed %d cuts %s: dev_ref %.3g dev_fast %.3g ratio %.3g"
                             % (block, pi, seed, cuts, dev_ref, dev_fast, dev_fast / dev_ref if dev_ref else 0.0))
                assert dev_fast <= R.bound(dev_ref), lines[-1]
                peak = np.max(np.abs(g64))
                ideal = x.astype(np.complex128 if R.is_cc(block) else np.float64) * g64[:-1]
                tol = R.mag64(x) * R.bound(dev_ref) * peak + 2.0 ** -23 * np.abs(ideal)
                assert np.all(np.abs(f.out - ideal) <= tol), lines[-1]
    print("\n".join(lines))


def test_chunked_falls_back_to_the_serial_walk():
    x = R.signal(1)
    # at most one chunk, a negative rate, a negative reference, a parameter that is not finite
    assert not R.can_chunk("agc_cc", R.AGC_SETS[0], 256) and R.can_chunk("agc_cc", R.AGC_SETS[0], 257)
    for params in ((-1e-3, 1, 1, 0), (1e-3, -1, 1, 0), (float("nan"), 1, 1, 0), (1e-3, 1, 1, float("inf"))):
        assert not R.can_chunk("agc_cc", params, R.N)
    assert not R.can_chunk("agc2_cc", R.AGC2_SETS[0], R.N)
    a, b = R.chunked("agc_cc", x[:256], R.AGC_SETS[0]), R.serial("agc_cc", x[:256], R.AGC_SETS[0])
    assert R.bits(a.out).tolist() == R.bits(b.out).tolist() and a.gain == b.gain


OPS1 = ("create", "destroy", "set_mode", "set_streams", "rate", "reference", "max_gain", "gain", "set_rate",
        "set_reference", "set_max_gain", "set_gain", "work", "work_device")
OPS2 = tuple(o for o in OPS1 if o not in ("rate", "set_rate")) + ("attack_rate", "decay_rate", "set_attack_rate", "set_decay_rate")


def test_new_entries_are_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = g.lib()
    for block in R.BLOCKS:
        names = set(re.findall(r"\b(grhip_%s_[a-z0-9_]+)\s*\(" % block, hdr))
        for op in (OPS2 if block.startswith("agc2") else OPS1):
            assert "grhip_%s_%s" % (block, op) in names, (block, op)
        assert not [n for n in names if not hasattr(lib, n)]
        assert hasattr(g, block) and block in g.__all__
    assert g.agc_cc.chunk() == R.CHUNK == 256


def test_null_arguments_are_refused_before_the_device(g):
    import ctypes as C
    lib = g.lib()
    for block in R.BLOCKS:
        for op, args in (("set_mode", (None, 0)), ("set_streams", (None, 1)), ("set_gain", (None, C.c_float(1))),
                         ("gain", (None, 0, None)), ("work", (None, 0, None, None)), ("work_device", (None, 0, None, None, None))):
            f = getattr(lib, "grhip_%s_%s" % (block, op))
            assert f(*args) == -1, (block, op)                      # GRHIP_EINVAL
    assert lib.grhip_agc_cc_create(None, 1e-3, 1.0, 1.0, 0.0, 0) == -1


def test_new_entries_refuse_to_run_without_a_device(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    for make in (lambda: g.agc_cc(1e-3, 1, 1, 1000), lambda: g.agc_ff(), lambda: g.agc2_cc(), lambda: g.agc2_ff(1e-2, 1e-3, 1, 1, 0)):
        with pytest.raises(g.GrhipError) as e:
            make()
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
