"""GPU tests of iir_filter_ffd: GRHIP_MODE_GENERIC against the restatement of the reference (iir_ref.py, pinned to the
reference's own code by tests/test_iir_cpu.py) bit for bit -- every tap set, one call, calls cut at 1 / 255 / 256 / 257 /
4097, three streams, the vectors of qa_iir.py; the chunked form of every other mode within the bound include/grhip.h
states, ulp_float(|y|) + 2^-40 peak of GENERIC's output; the cases that run the serial walk whatever the mode; the
latched set_taps; the refusals; and the device entry on pointers aligned to a float and nothing more."""
import functools
import json
import os

import numpy as np
import pytest

import device_offsets as do
import iir_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
QA = json.load(open(os.path.join(HERE, "golden", "ref_qa_iir.json")))
EINVAL = -1


@functools.lru_cache(maxsize=None)
def stream(k):
    """three different streams of the test signal's length"""
    x = R.signal(1)
    return (x, np.ascontiguousarray(x[::-1]), R.signal(2))[k]


@functools.lru_cache(maxsize=None)
def ref(name, k=0):
    """the restatement's output for a tap set over stream k, computed once"""
    out, _, _ = R.serial(stream(k), *taps(name))
    out.setflags(write=False)
    return out


def taps(name):
    return {"unstable": R.UNSTABLE, "k9": R.K9}.get(name) or R.TAP_SETS[name]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


def in_calls(blk, x, cuts):
    edges = [0] + [c for c in cuts if 0 < c < len(x)] + [len(x)]
    return np.concatenate([blk.work(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])


@pytest.mark.parametrize("name", R.STABLE + ("k9",))
def test_generic_is_the_reference_bit_for_bit(gpu, name):
    g = gpu
    x = stream(0)
    for cuts in ((),) + tuple((c,) for c in R.CUTS) + (R.CUTS,):
        blk = g.iir_filter_ffd(*taps(name))
        blk.set_mode(g.MODE_GENERIC)
        assert same_bits(in_calls(blk, x, cuts), ref(name)), (name, cuts)


def test_generic_unstable_taps(gpu):
    g = gpu
    x = stream(0)[:R.UNSTABLE_N]
    want, _, _ = R.serial(x, *R.UNSTABLE)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        for cuts in ((), (1,), (33,)):
            blk = g.iir_filter_ffd(*R.UNSTABLE)
            blk.set_mode(mode)
            assert not blk.chunked()
            assert same_bits(in_calls(blk, x, cuts), want), (mode, cuts)


@pytest.mark.parametrize("name", ("deemph320k", "order4", "n5m2"))
def test_three_streams(gpu, name):
    g = gpu
    n = R.N
    x = np.concatenate([stream(k) for k in range(3)])
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = g.iir_filter_ffd(*taps(name))
        blk.set_mode(mode)
        blk.set_streams(3)
        # two calls: [3][4097] and [3][n - 4097]
        a = blk.work(np.concatenate([stream(k)[:4097] for k in range(3)]), 4097).reshape(3, 4097)
        b = blk.work(np.concatenate([stream(k)[4097:] for k in range(3)]), n - 4097).reshape(3, n - 4097)
        got = np.concatenate([a, b], axis=1)
        for k in range(3):
            if mode == g.MODE_GENERIC:
                assert same_bits(got[k], ref(name, k)), (name, k)
            else:
                assert R.within_fast_bound(got[k], ref(name, k)), (name, k)
        # set_streams zeroes the delay lines: one call again equals the reference from the start
        blk.set_streams(3)
        got = blk.work(x, n).reshape(3, n)
        for k in range(3):
            assert R.within_fast_bound(got[k], ref(name, k)), (name, k)


@pytest.mark.parametrize("case", sorted(QA))
def test_qa_vectors(gpu, case):
    g = gpu
    q = QA[case]
    x = np.array(q["src"], np.float32)
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = g.iir_filter_ffd(*q["taps"][0])
        blk.set_mode(mode)
        for ff, fb in q["taps"][1:]:
            blk.set_taps(ff, fb)                                        # qa_iir.py test 006 .. 008
        got = blk.work(x)
        assert got.dtype == np.float32 and got.tolist() == [float(v) for v in q["expected"]], (case, mode)


@pytest.mark.parametrize("name", R.STABLE)
def test_fast_is_within_the_stated_bound_of_generic(gpu, name):
    g = gpu
    x = stream(0)
    for cuts in ((), (257,), (1, 4097), (300, 557, 4097)):
        blk = g.iir_filter_ffd(*taps(name))
        blk.set_mode(g.MODE_FAST)
        assert blk.chunked()
        got = in_calls(blk, x, cuts)
        diff = int(np.count_nonzero(R.bits(got) != R.bits(ref(name))))
        print("%s cuts %s: %d of %d outputs differ from GENERIC in bits" % (name, cuts, diff, len(got)))
        assert R.within_fast_bound(got, ref(name)), (name, cuts)
    # GENERIC on the same handle type reports no chunked form
    blk.set_mode(g.MODE_GENERIC)
    assert not blk.chunked()


def test_serial_walk_whatever_the_mode(gpu):
    g = gpu
    x = stream(0)
    # feedback order 9: above the chunked form's limit
    blk = g.iir_filter_ffd(*R.K9)
    blk.set_mode(g.MODE_FAST)
    assert not blk.chunked()
    assert same_bits(blk.work(x), ref("k9"))
    # a call of exactly one chunk, then the rest in pieces of at most one chunk: chunked() holds, the walk runs
    blk = g.iir_filter_ffd(*taps("biquad"))
    blk.set_mode(g.MODE_FAST)
    assert blk.chunked()
    got = np.concatenate([blk.work(x[a:a + 256]) for a in range(0, 1024, 256)])
    assert same_bits(got, ref("biquad")[:1024])
    # taps that are not finite are accepted and run serially
    blk = g.iir_filter_ffd([1.0, float("inf")], [0.0, 0.5])
    blk.set_mode(g.MODE_FAST)
    assert not blk.chunked()
    want, _, _ = R.serial(x[:600], [1.0, float("inf")], [0.0, 0.5])
    got = blk.work(x[:600])
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got).any()    # a NaN's sign and payload are the machine's


def test_latched_set_taps(gpu):
    g = gpu
    x = stream(0)
    a, _, _ = R.serial(x[:R.LATCH_AT], *taps(R.LATCH[0]))
    b, _, _ = R.serial(x[R.LATCH_AT:], *taps(R.LATCH[1]))
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = g.iir_filter_ffd(*taps(R.LATCH[0]))
        blk.set_mode(mode)
        got_a = blk.work(x[:R.LATCH_AT])
        blk.set_taps(*taps(R.LATCH[1]))                                 # holds from the next call, from zeroed delay lines
        got_b = blk.work(x[R.LATCH_AT:])
        if mode == g.MODE_GENERIC:
            assert same_bits(got_a, a) and same_bits(got_b, b)
        else:
            assert R.within_fast_bound(got_a, a) and R.within_fast_bound(got_b, b)
    # chunked() counts the latched taps; the last set_taps before a call wins
    blk = g.iir_filter_ffd(*taps("biquad"))
    assert blk.chunked()
    blk.set_taps(*R.UNSTABLE)
    assert not blk.chunked()
    blk.set_taps(*R.K9)
    blk.set_taps(*taps("n1m3"))
    assert blk.chunked()
    blk.set_mode(g.MODE_GENERIC)
    assert same_bits(blk.work(x), ref("n1m3"))


def test_no_feed_forward_taps_give_zeros_and_touch_no_state(gpu):
    g = gpu
    x = stream(0)[:700]
    blk = g.iir_filter_ffd([], [])
    got = blk.work(x)
    assert got.dtype == np.float32 and len(got) == 700 and not got.any()
    blk = g.iir_filter_ffd([], [0.0, 0.5])                             # gri_iir.h:135: n == 0 decides, whatever m
    assert not blk.work(x).any()
    # a biquad whose taps become empty and come back: set_taps zeroed the delay lines, the empty call left them so
    blk = g.iir_filter_ffd(*taps("biquad"))
    blk.set_mode(g.MODE_GENERIC)
    blk.work(x)
    blk.set_taps([], [])
    assert not blk.work(x).any()
    blk.set_taps(*taps("biquad"))
    assert same_bits(blk.work(x), ref("biquad")[:700])


def test_refusals(gpu):
    import torch
    g = gpu
    for ff, fb in (([1.0], []), ([0.0] * 65, [0.0]), ([1.0], [0.0] * 65)):
        with pytest.raises(g.GrhipError) as e:
            g.iir_filter_ffd(ff, fb)
        assert e.value.code == EINVAL
    g.iir_filter_ffd([0.0] * 64, [0.0] * 64)                            # 64 on both sides is taken
    blk = g.iir_filter_ffd(*taps("biquad"))
    for ff, fb in (([1.0], []), ([0.0] * 65, [0.0])):
        with pytest.raises(g.GrhipError) as e:
            blk.set_taps(ff, fb)
        assert e.value.code == EINVAL
    for bad in (0, -1, 65536):
        with pytest.raises(g.GrhipError):
            blk.set_streams(bad)
    with pytest.raises(g.GrhipError):
        blk.set_mode(99)
    d = torch.zeros(4096, dtype=torch.float32, device="cuda")
    for a, b, n in ((0, 0, 1000), (0, 999 * 4, 1000), (1000 * 4, 4, 1000)):     # overlapping by all, by one item
        with pytest.raises(g.GrhipError) as e:
            blk.work_device(n, d.data_ptr() + a, d.data_ptr() + b)
        assert e.value.code == EINVAL, (a, b)
    with pytest.raises(g.GrhipError):
        blk.work_device(-1, d, d)
    with pytest.raises(g.GrhipError):
        blk.work_device(10, d.data_ptr() + 2, d.data_ptr() + 2048)                # not aligned to a float
    assert blk.work_device(0, None, None) == 0
    # the refused set_taps latched nothing
    blk.set_mode(g.MODE_GENERIC)
    assert same_bits(blk.work(stream(0)[:500]), ref("biquad")[:500])


@pytest.mark.parametrize("mode_name", ("GENERIC", "FAST"))
@pytest.mark.parametrize("in_off,out_off", ((1, 3), (3, 0), (0, 1)))
def test_device_entry_on_float_aligned_pointers(gpu, mode_name, in_off, out_off):
    """three streams of 3 * 256 + 37 items, packed (an odd stride), `in_off` / `out_off` floats past a 256-byte boundary,
    guards poisoned: outputs as from the host entry, no byte outside the payload written, nothing read from the guards"""
    import torch
    g = gpu
    n = 3 * 256 + 37
    name = "order4"
    xs = np.stack([stream(k)[:n] for k in range(3)])
    outs = []
    for poison in (do.POISON, do.POISON2):
        d_in = do.guarded(xs, in_off)
        if poison != do.POISON:
            d_in.repoison(poison)
        d_out = do.guarded_output(n, np.float32, out_off, n_streams=3)
        blk = g.iir_filter_ffd(*taps(name))
        blk.set_mode(getattr(g, "MODE_" + mode_name))
        blk.set_streams(3)
        blk.work_device(n, d_in.ptr(), d_out.ptr())
        torch.cuda.synchronize()
        got = d_out.payload()
        assert not do.unwritten_items(d_out).any()
        do.check_guards(d_out)
        for k in range(3):
            if mode_name == "GENERIC":
                assert same_bits(np.ascontiguousarray(got[k]), ref(name, k)[:n]), k
            else:
                assert R.within_fast_bound(got[k], ref(name, k)[:n]), k
        outs.append(got)
    assert same_bits(outs[0], outs[1]), "the result depends on what the input's guards hold"
