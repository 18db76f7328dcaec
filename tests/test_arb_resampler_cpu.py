"""CPU tests of gr_pfb_arb_resampler_{ccf,fff}: the index schedule (closed form vs the reference's float walk), the
call-by-call restatement against the whole-stream rule, and the product's refusals without a GPU."""
import numpy as np
import pytest

import arb_resampler_ref as ar


def _rates(R, rng, n):
    fixed = [0.0192, 0.3, 0.5, 0.999, 1.0, 1.25, 2.5, R - 0.1 if R > 0.1 else 0.05, float(R)]
    rnd = list(np.exp(rng.uniform(np.log(1e-3), np.log(R), n)))
    return [r for r in fixed + rnd if 0 < r <= R and R / np.float32(r) < 2 ** 20 - 1]


@pytest.mark.parametrize("R", [1, 2, 3, 7, 8, 16, 31, 32, 50, 64, 100, 127, 128, 200, 256])
def test_closed_form_equals_float_walk(R):
    rng = np.random.default_rng(R)
    for rate in _rates(R, rng, 12):
        c, j, a = ar.walk_schedule(R, rate, n_outputs=400)
        c2, j2, a2 = ar.closed_form_schedule(R, rate, 400)
        assert np.array_equal(c, c2) and np.array_equal(j, j2), (R, rate)
        assert np.array_equal(a.view(np.uint32), a2.view(np.uint32)), (R, rate)


def test_rounding_regime_is_not_the_closed_form():
    # rate > R: f is no multiple of 2^-23 and the float sums round; the walk is the schedule there
    D, f = ar.rate_params(4, 5.3)
    assert D == 0 and float(f) * 2 ** 23 != np.floor(float(f) * 2 ** 23)
    c, j, a = ar.walk_schedule(4, 5.3, n_outputs=2000)
    assert np.all(np.diff(c) >= 0) and np.all((j >= 0) & (j < 4)) and np.all((a >= 0) & (a < 1))


CASES = [
    # (R, rate, ntaps, complex)
    (32, 0.5, 32 * 8 - 5, True),
    (32, 1.25, 32 * 4 + 3, False),
    (32, 0.0192, 32 * 16, True),        # strong decimation: count overshoots the call's input (d_start_index)
    (5, 0.037, 23, False),
    (4, 5.3, 13, True),                 # the rounding regime
    (1, 1.5, 7, False),
    (50, 49.9, 50 * 3, True),
]


@pytest.mark.parametrize("R,rate,ntaps,cplx", CASES)
def test_restatement_independent_of_call_sizes(R, rate, ntaps, cplx):
    rng = np.random.default_rng(ntaps)
    taps = rng.standard_normal(ntaps).astype(np.float32) / ntaps
    N = 3000
    x = rng.standard_normal(N).astype(np.float32)
    if cplx:
        x = (x + 1j * rng.standard_normal(N)).astype(np.complex64)
    whole = ar.run_calls(ar.ArbResamplerRef(rate, taps, R, cplx), x, [(1 << 30, None)])
    counts, js, accs = ar.whole_stream_schedule(R, rate, N)
    assert len(whole) == len(counts) > 0          # exactly the outputs with count_k < N
    tpf = ar.banks(taps, R)[0]
    buf = np.concatenate([np.zeros(tpf, dtype=x.dtype), x])
    ref = ar.eval_schedule(*ar.banks(taps, R)[1:], buf, counts, js, accs)
    assert np.array_equal(whole.view(np.uint32), ref.view(np.uint32))
    patterns = [
        [(1, None)],
        [(7, None), (1, None), (3, 40)],
        [(4096, 100), (65536, 17), (5, None)],
        [(int(a), int(b)) for a, b in zip(rng.integers(1, 300, 50), rng.integers(1, 400, 50))] + [(1 << 20, None)],
    ]
    for sizes in patterns:
        got = ar.run_calls(ar.ArbResamplerRef(rate, taps, R, cplx), x, sizes)
        assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), sizes


def test_strong_decimation_carries_the_overshoot():
    blk = ar.ArbResamplerRef(0.0192, np.ones(64, np.float32), 32, False)     # tpf 2, D 1666
    assert blk.schedule_call(10, 100) == ([], 0)      # the first call after create
    sched, consumed = blk.schedule_call(10, 10)       # one output at count 0, then a jump of 1666 // 32 = 52 inputs
    assert len(sched) == 1 and consumed == 10 and blk.d_start_index == 42


def test_whole_stream_oracle_form_matches_restatement(po):
    rng = np.random.default_rng(3)
    for R, rate, ntaps, cplx in CASES:
        taps = rng.standard_normal(ntaps).astype(np.float32)
        x = rng.standard_normal(1500).astype(np.float32)
        if cplx:
            x = (x + 1j * rng.standard_normal(1500)).astype(np.complex64)
        a = ar.whole_stream(po, rate, taps, R, x)
        b = ar.run_calls(ar.ArbResamplerRef(rate, taps, R, cplx), x, [(97, None)])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (R, rate)


def test_set_rate_between_calls_restatement():
    rng = np.random.default_rng(11)
    taps = rng.standard_normal(100).astype(np.float32)
    x = rng.standard_normal(4000).astype(np.float32)
    blk = ar.ArbResamplerRef(0.7, taps, 16, False)
    buf = np.concatenate([np.zeros(blk.history() - 1, np.float32), x])
    out, c = blk.general_work(500, buf)
    assert len(out) == 0 and c == 0
    out, c = blk.general_work(500, buf)
    blk.set_rate(1.9)
    out2, c2 = blk.general_work(500, buf[c:])
    assert len(out) == 500 and len(out2) == 500 and c2 > 0


@pytest.mark.parametrize("cls", ["pfb_arb_resampler_ccf", "pfb_arb_resampler_fff"])
def test_no_cpu_fallback_without_device(g, cls):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(g.GrhipError) as e:
        getattr(g, cls)(0.5, np.ones(64, np.float32), 32)
    assert e.value.code == -5      # GRHIP_ENODEV
    assert "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("cls", ["pfb_arb_resampler_ccf", "pfb_arb_resampler_fff"])
@pytest.mark.parametrize("rate,ntaps,R", [(0.5, 0, 32), (0.5, 1, 32), (0.5, 64, 0), (0.0, 64, 32), (-1.0, 64, 32),
                                          (float("nan"), 64, 32), (float("inf"), 64, 32), (0.5, 8192, 1)])
def test_bad_arguments_refused_before_the_device(g, cls, rate, ntaps, R):
    with pytest.raises(g.GrhipError) as e:
        getattr(g, cls)(rate, np.ones(ntaps, np.float32), R)
    assert e.value.code == -1      # GRHIP_EINVAL, with or without a GPU
