"""tests/float_range.py proven without a GPU.  First the class table and the scale set, on the references alone: for
every row, variant and scale of tests/test_gpu_float_range.py the reference the GPU case compares with is finite and
has its class property bit for bit against the reference at amplitude 1.  Then the comparison functions: each kind of
wrong result the GPU cases rely on them to show is shown."""
import numpy as np
import pytest

import float_range as fr
import test_gpu_device_offsets as tdo
from conftest import bits_equal

CASES = fr.cases(tdo.ROWS)


def test_every_row_has_a_class():
    for row in tdo.ROWS:
        for variant in row.variants:
            cls, reason = fr.classify(row.id, variant)                  # KeyError: a row the table does not know
            assert cls in (fr.LINEAR, fr.QUADRATIC, fr.INVARIANT, fr.REFERENCE_ONLY, fr.SKIP) and reason
    known = {r.id for r in tdo.ROWS}
    assert {e[0] for e in fr.CLASSES} == known
    assert {e[0] for e in fr.EXEMPT} <= known and {e[0] for e in fr.SLACK} <= known
    for rid, word, reason in fr.EXEMPT:                                  # an exemption names code, and matches something
        assert ":" in reason
        assert any(fr.exempt(row.id, v) for row in tdo.ROWS if row.id == rid for v in row.variants), (rid, word)
    for rid, need, n, why in fr.SLACK:                                   # never more than a tile; matches a variant
        assert 0 < n <= fr.TILE[rid] and why
        assert any(fr.slack(rid, v) == n and all(w in v.split("-") for w in need)
                   for row in tdo.ROWS if row.id == rid for v in row.variants), (rid, need)
    for row, variant, _cls in CASES:                                     # bit-exact variants have none
        if "GENERIC" in variant.split("-"):
            assert fr.slack(row.id, variant) == 0


def _refs(g, po, wl, row, variant, k):
    """(the references, the inputs) of the case at amplitude 2^k"""
    with tdo.amplitude(2.0 ** k):
        spec = row.build(g, po, wl, variant, max(row.sizes))
    return (fr.flatten(spec.cpu_ref if spec.cpu_ref is not None else spec.ref),
            [np.asarray(i["arr"]) for i in spec.ins])


@pytest.mark.parametrize("row,variant,cls", [pytest.param(r, v, c, id=fr.case_id(r, v)) for r, v, c in CASES])
def test_reference_over_the_scales(g, po, wl, row, variant, cls):
    base, x_1 = _refs(g, po, wl, row, variant, 0)
    for k in fr.scales(row.id, variant):
        at_k, x_k = _refs(g, po, wl, row, variant, k)
        if variant == "nlog10_ff":                                       # fewer decades under a scale, all of them normal
            assert all(np.abs(x).min() >= np.finfo(np.float32).tiny and np.isfinite(x).all() for x in x_k)
            assert x_k[0].max() > x_1[0].max() * 2.0 ** (k - 20) and x_k[0].min() < x_1[0].min() * 2.0 ** (k + 20)
        else:                                                            # the knob reaches this builder's input
            head = 4 if row.id == "quadrature_demod_cf" else 0           # its first items are 0, 0, 1, 1j at any scale
            fr.assert_property(fr.LINEAR, k, [x[..., head:] for x in x_k], [x[..., head:] for x in x_1], "input")
        for a in at_k:
            assert not fr.bad(a).any(), "the reference at 2^%d is not finite" % k
        if k == fr.SUBNORMAL:
            # the products x[i] conj(x[i-1]) are subnormal: the quotient is formed from a few bits
            assert not all(bits_equal(a, b) for a, b in zip(at_k, base))
        elif cls != fr.REFERENCE_ONLY:
            fr.assert_property(cls, k, at_k, base, "reference")


# ---------------------------------------------------------------------------------------------------------------
# the comparison functions reject what they are there to reject
# ---------------------------------------------------------------------------------------------------------------
def _result(n=300, cplx=True, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    return (x + 1j * rng.uniform(-1, 1, n)).astype(np.complex64) if cplx else x


def test_scaled_is_exact_and_the_property_passes():
    for cplx in (False, True):
        base = _result(cplx=cplx)
        for k in fr.SCALES:
            f = np.float32(2.0) ** np.float32(k)
            fr.assert_property(fr.LINEAR, k, [base * f], [base])
            fr.assert_property(fr.QUADRATIC, k, [base * f * f], [base])
            fr.assert_property(fr.INVARIANT, k, [base.copy()], [base])
            assert bits_equal(fr.scaled(fr.scaled(base, fr.LINEAR, k), fr.LINEAR, -k), base)
    counts = np.array([5, 7], np.int32)
    fr.assert_property(fr.LINEAR, 15, [counts.copy()], [counts])         # integer outputs do not scale
    with pytest.raises(AssertionError):
        fr.assert_property(fr.LINEAR, 15, [counts + 1], [counts])


def test_items_behind_a_short_result_keep_their_pattern():
    base = _result(cplx=False)
    base[250:] = np.frombuffer(np.uint32(0x7FC54321).tobytes(), np.float32)[0]
    at_k = base * np.float32(2.0 ** 15)
    at_k[250:] = base[250:]
    fr.assert_property(fr.LINEAR, 15, [at_k], [base])


@pytest.mark.parametrize("cplx", [False, True])
def test_one_ulp_in_one_item_is_caught(cplx):
    base = _result(cplx=cplx)
    at_k = base * np.float32(2.0 ** -16)
    w = at_k.view(np.uint32)
    w[123] += 1
    with pytest.raises(AssertionError, match="1 of 300 item"):
        fr.assert_property(fr.LINEAR, -16, [at_k], [base])
    with pytest.raises(AssertionError, match="1 item"):
        tdo.exact(at_k, base * np.float32(2.0 ** -16))


@pytest.mark.parametrize("cplx", [False, True])
def test_flushed_subnormals_are_caught(cplx):
    """values of a few bits around 2^-100, times 2^-40: exact, and subnormal"""
    base = (np.round(_result(cplx=cplx) * 8) / 8).astype(np.complex64 if cplx else np.float32) * np.float32(2.0 ** -100)
    base[0] = 2.0 ** -100
    at_k = base * np.float32(2.0 ** -40)
    assert (np.abs(at_k.view(np.float32)) < np.finfo(np.float32).tiny).all() and at_k.view(np.float32).any()
    fr.assert_property(fr.LINEAR, -40, [at_k], [base])
    flushed = fr.flush_subnormals(at_k)
    assert not flushed.view(np.float32).any()
    with pytest.raises(AssertionError):
        fr.assert_property(fr.LINEAR, -40, [flushed], [base])
    with pytest.raises(AssertionError):
        tdo.exact(flushed, at_k)
    keep = fr.flush_subnormals(base)                                     # normal values are left alone
    assert bits_equal(keep, base)


def _poisoned(n=400, lo=190, hi=199):
    ref = _result(n)
    ref[lo:hi + 1] = np.nan
    return ref


def test_non_finite_sets():
    ref = _poisoned()
    fr.assert_local(ref.copy(), ref, 0, tdo.exact)
    got = ref.copy()
    got[187:190] = np.inf                                                # three more on one side: inside a slack of 3
    got[200] = complex(0, np.nan)
    fr.assert_local(got, ref, 3, tdo.peak(1e-5))
    with pytest.raises(AssertionError, match="more than 2 away"):
        fr.assert_local(got, ref, 2, tdo.peak(1e-5))
    got[203] = np.nan                                                    # slack + 1
    with pytest.raises(AssertionError, match="more than 3 away"):
        fr.assert_local(got, ref, 3, tdo.peak(1e-5))


def test_a_hidden_non_finite_output_is_caught():
    ref = _poisoned()
    got = ref.copy()
    got[195] = 0.25
    with pytest.raises(AssertionError, match="1 non-finite output"):
        fr.assert_local(got, ref, 3, tdo.peak(1e-5))


def test_outputs_outside_the_support_are_compared():
    ref = _poisoned()
    got = ref.copy()
    got[20] += np.float32(1e-3)
    with pytest.raises(AssertionError):
        fr.assert_local(got, ref, 3, tdo.peak(1e-5))
    with pytest.raises(AssertionError, match="tests nothing"):
        fr.assert_local(_result(400), _result(400), 3, tdo.exact)


def test_a_short_result_in_a_longer_buffer():
    ref = _poisoned()
    got = np.concatenate([ref, np.full(16, np.nan, np.complex64)])       # the pre-fill behind the produced items
    fr.assert_local(got, ref, 0, lambda g, r: tdo.exact(g[:r.size], r))
