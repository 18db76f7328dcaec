"""Every device entry on pointers that are aligned to their item and to nothing more, and on odd stream strides
(include/grhip.h, "semantics common to all blocks").  Table driven: one Row per device entry.  Every pointer is a
view into a guarded allocation of tests/device_offsets.py, every result is compared with the CPU reference the
block's own test file uses (never with the same block at offset 0), under that file's tolerance or bit for bit where
the mode is documented bit exact.  Each case: run, synchronise, compare, check the output guards; then refill the
input guards with another poison and require a bit-identical result from a fresh handle.

Sizes per row: three of the kernel's tiles plus an odd remainder, and one call shorter than a vector chunk."""
import contextlib

import numpy as np
import pytest

import arb_resampler_ref
import device_offsets as do
import fft_real_ref
import fractional_interp_ref
import logpwrfft_ref
import pfb_synth_ref
import resampler_ref
import running_sum_ref
import spectrum_ref
from conftest import bits_equal, demod_close, rel_err_max
import agc_ref
import ctcss_ref
import squelch_ref
from test_gpu_arb_resampler import _whole_ref as arb_whole_ref
from test_gpu_digital import _fsk_soft                      # soft FSK symbols for the clock recovery
from test_gpu_logpwrfft import Chain as LogpwrChain          # the five blocks behind blks2.logpwrfft, host entries
from test_gpu_framer import make_stream                     # correlator-style items with headers and stray flags

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # FAST modes of the FIR family: tests/test_gpu_fir.py:11, tests/test_gpu_realin.py:9
EINVAL = -1

# offsets in items from a 16-byte boundary, by item size in bytes
OFFSETS = {16: [0, 1], 8: [0, 1], 4: [0, 1, 2, 3], 2: [0, 1, 3, 7], 1: [0, 1, 7, 8, 15]}

# (entry, condition) pairs that answer GRHIP_EINVAL instead of a result; each one is a sentence at the entry in
# include/grhip.h.  An entry is a row id, or a row id and the variant's first words.  Conditions: "in", "out" (that
# pointer off the 16-byte grid), "odd_stride".
REFUSALS = {
    # grhip_xlating_demod_run_captures_device: "GRHIP_MODE_GENERIC ... an even in_stride_items"
    ("xlating_demod_run_captures-GENERIC", "odd_stride"),
}


def _refusals(row, variant, conditions):
    name = row.id + "-" + variant
    return {c for c in conditions for e, rc in REFUSALS if rc == c and (e == row.id or name.startswith(e + "-"))}


def offset_pairs(in_size, out_size):
    """(0, 0), every (a, 0), every (0, b), and every a paired with a b != a where the types allow it"""
    a, b = OFFSETS[in_size][1:], (OFFSETS[out_size][1:] if out_size else [])
    if not out_size:
        return [(0, 0)] + [(x, 0) for x in a]
    pairs = [(0, 0)] + [(x, 0) for x in a] + [(0, y) for y in b]
    for i, x in enumerate(a):
        y = b[(i + 1) % len(b)]
        pairs.append((x, y))
    return pairs


# every float or complex input the builders generate is multiplied by AMPLITUDE (tests/test_gpu_float_range.py sets
# powers of two); at 1 nothing is touched, so the cases of this file are byte for byte what they were without it.
# Taps and parameters are never scaled.
AMPLITUDE = 1.0
_POISON = []                    # one value: it replaces the middle sample of the next input _amp() sees


@contextlib.contextmanager
def amplitude(a, poison=None):
    """builders called inside see their input times `a`; with `poison`, the middle sample of the first input they
    generate is that value (an inf or a NaN)"""
    global AMPLITUDE
    before, AMPLITUDE = AMPLITUDE, a
    _POISON[:] = [] if poison is None else [poison]
    try:
        yield
    finally:
        AMPLITUDE = before
        del _POISON[:]


def _amp(x):
    if AMPLITUDE != 1:
        x = x * np.float32(AMPLITUDE)
    if _POISON:
        x = x.copy()
        x[tuple(s // 2 for s in x.shape)] = _POISON.pop()
    return x


def _rc(rng, n, scaled=True):
    x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    return _amp(x) if scaled else x


def _rf(rng, n, scaled=True):
    x = rng.uniform(-1, 1, n).astype(np.float32)
    return _amp(x) if scaled else x


class Deferred(object):
    """a reference that the library itself computes on the device: formed when it is first compared, so that the
    builder touches no device"""

    def __init__(self, fn):
        self.fn, self.value = fn, None

    def __array__(self, dtype=None, copy=None):
        if self.value is None:
            self.value = self.fn()
        return self.value


class Spec(object):
    """one call, independent of offsets and strides: how to make the handle, the host inputs, the outputs' shapes, the
    call itself, the reference and the comparison"""

    def __init__(self, make, ins, outs, call, ref, check, ret=None, post=None, ref_post=None, cpu_ref=None):
        self.make, self.ins, self.outs, self.call, self.ref, self.check = make, ins, outs, call, ref, check
        self.ret, self.post, self.ref_post = ret, post, ref_post
        self.cpu_ref = cpu_ref          # where `ref` is Deferred: the CPU form of it, for tests that have no device


class Out(object):
    """packed: the streams lie back to back (the entry takes no stride)"""

    def __init__(self, n, dtype, n_streams=None, itemsize=None, packed=False):
        self.n, self.dtype, self.n_streams, self.itemsize, self.packed = n, dtype, n_streams, itemsize, packed


class Row(object):
    """items: (bytes per input item, bytes per output item; 0: no output), or a function of the variant that
    returns them; sizes: the values of n"""

    def __init__(self, rid, items, sizes, build, variants=("",), strided=False):
        self.id, self.items, self.sizes = rid, items, sizes
        self.build, self.variants, self.strided = build, variants, strided

    def item_sizes(self, variant):
        return self.items(variant) if callable(self.items) else self.items


def exact(got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    if not bits_equal(got, ref):
        bad = np.flatnonzero(got.reshape(-1) != ref.reshape(-1))
        raise AssertionError("%d item(s) differ from the reference, the first at %s" % (bad.size, bad[:4]))


def fir_fast(bound):
    def check(got, ref):                                                # tests/test_gpu_fir.py:117, :691
        assert got.shape == ref.shape
        err = np.abs(got - ref).max()
        assert err <= TOL * max(np.abs(ref).max(), 1e-3 * bound), err
    return check


def rel(tol):
    def check(got, ref):
        assert got.shape == ref.shape
        e = rel_err_max(got, ref)
        assert e <= tol, e
    return check


def _stride(kind, n_items, itemsize):
    """a stride that keeps every stream 16-byte aligned, or one that is odd in items"""
    if kind == "aligned":
        q = max(16 // itemsize, 1)
        return -(-(n_items + 1) // q) * q
    s = n_items + 3
    return s if s % 2 else s + 1


# ---------------------------------------------------------------------------------------------------------------
# the rows.  build(gpu, po, wl, variant, n) -> Spec; `n` counts output items of the first output.
# ---------------------------------------------------------------------------------------------------------------
def _simple(gpu, make, x, n_out, out_dtype, ref, check, out_itemsize=None):
    def call(blk, ins, outs, strides):
        return blk.work_device(n_out, ins[0].ptr(), outs[0].ptr())
    return Spec(make, [dict(arr=x)], [Out(n_out, out_dtype, itemsize=out_itemsize)], call, [ref], check, ret=n_out)


def build_fir(gpu, po, wl, variant, n):
    kind, mode, ntaps, decim = variant.split("-")
    ntaps, decim = int(ntaps[1:]), int(decim[1:])
    rng = np.random.default_rng(ntaps * 10 + decim)
    nin = n * decim + ntaps - 1
    if kind == "fff":
        x, taps = _rf(rng, nin), _rf(rng, ntaps, scaled=False)
    else:
        x = _rc(rng, nin)
        taps = _rf(rng, ntaps, scaled=False) if kind == "ccf" else _rc(rng, ntaps, scaled=False)
    bound = np.abs(taps).sum() * (np.sqrt(2) if kind == "ccc" else 1.0)
    ref = getattr(po, "fir_" + kind)(taps, x, n, decim)

    def make():
        blk = getattr(gpu, "fir_filter_" + kind)(decim, taps)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk
    if AMPLITUDE != 1:                                                  # the absolute term follows the input
        bound = bound * AMPLITUDE
    return _simple(gpu, make, x, n, ref.dtype, ref, exact if mode == "GENERIC" else fir_fast(bound))


FIR_VARIANTS = ["%s-%s-t%d-d%d" % (k, m, t, d) for k in ("ccf", "ccc", "fff") for m in ("GENERIC", "FAST")
                for t in (9, 64) for d in (1, 2, 3)]


def build_xlating(gpu, po, wl, variant, n):
    mode, ntaps, decim = variant.split("-")
    ntaps, decim = int(ntaps[1:]), int(decim[1:])
    c = wl.CFG2
    rng = np.random.default_rng(ntaps + decim)
    taps = (wl.lowpass_taps(ntaps, 0.4 / decim, 1.0) * np.exp(0.02j * np.arange(ntaps))).astype(np.complex64)
    x = _rc(rng, n * decim + ntaps - 1)
    ref = po.Xlating(decim, taps, c["center_freq"], c["fs"]).work(x, n)

    def make():
        blk = gpu.freq_xlating_fir_filter_ccc(decim, taps, c["center_freq"], c["fs"])
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk
    # FAST: tests/test_gpu_fir.py:298
    return _simple(gpu, make, x, n, np.complex64, ref, exact if mode == "GENERIC" else rel(TOL))


XL_VARIANTS = ["%s-t%d-d%d" % (m, t, d) for m in ("GENERIC", "FAST_VALU") for t, d in ((64, 4), (40, 3), (9, 1))]


def build_xlating_demod(gpu, po, wl, variant, n):
    mode, ntaps, decim = variant.split("-")
    ntaps, decim = int(ntaps[1:]), int(decim[1:])
    c = wl.CFG2
    gain = 3.0
    x = _amp(wl.fsk4_capture(n * decim, stream_id=17))
    proto = wl.lowpass_taps(ntaps, 100e3, 10e6).astype(np.complex64)
    ref = po.chain_xlating_demod(decim, proto, c["center_freq"], c["fs"], gain, x)
    xin = wl.with_history(x, ntaps - 1)

    def make():
        blk = gpu.xlating_demod(decim, proto, c["center_freq"], c["fs"], gain)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk

    def close(got, ref):                                                # tests/test_gpu_fir.py:312
        ok, worst = demod_close(got, ref, skip=max(64, ntaps // decim + 1), gain=gain)
        assert ok, worst
    return _simple(gpu, make, xin, n, np.float32, ref, exact if mode == "GENERIC" else close)


XD_VARIANTS = ["%s-t%d-d%d" % (m, t, d) for m in ("GENERIC", "FAST") for t, d in ((64, 4), (33, 1), (100, 2))]


def build_quad_demod(gpu, po, wl, variant, n):
    rng = np.random.default_rng(n)
    x = _rc(rng, n + 1)
    x[:4] = [0, 0, 1, 1j]
    ref = po.quad_demod_cf(4.9, x, n)
    return _simple(gpu, lambda: gpu.quadrature_demod_cf(4.9), x, n, np.float32, ref, exact)


def build_pager_slicer(gpu, po, wl, variant, n):
    rng = np.random.default_rng(n)
    x = _amp((rng.integers(0, 4, n) * 2.0 - 3.0 + 0.7 + 0.3 * rng.standard_normal(n)).astype(np.float32))
    ref = po.PagerSlicer(0.002).work(x)
    return _simple(gpu, lambda: gpu.pager_slicer_fb(0.002), x, n, np.uint8, ref, exact)


def build_unpack(gpu, po, wl, variant, n):
    k = int(variant[1:])
    rng = np.random.default_rng(k + n)
    x = rng.integers(0, 256, n).astype(np.uint8)
    ref = po.unpack_k_bits_bb(k, x)

    def call(blk, ins, outs, strides):
        return blk.work_device(n * k, ins[0].ptr(), outs[0].ptr())
    return Spec(lambda: gpu.unpack_k_bits_bb(k), [dict(arr=x)], [Out(n * k, np.uint8)], call, [ref], exact, ret=n * k)


def build_framer(gpu, po, wl, variant, n):
    rng = np.random.default_rng(n)
    x = make_stream(rng, n, gap=40, maxlen=6)
    ref = po.FramerSink1().work(x)
    assert n < 200 or len(ref) > 3

    def make():
        blk = gpu.framer_sink_1()
        if variant == "segments":
            blk.set_segment_items(64)
        return blk

    def call(blk, ins, outs, strides):
        return blk.work_device(n, ins[0].ptr())
    return Spec(make, [dict(arr=x)], [], call, [], exact, ret=n, post=lambda blk, outs: blk.messages(), ref_post=ref)


def build_adapter(gpu, po, wl, variant, n):
    """gr_stream_to_streams / gr_vector_to_streams / gr_streams_to_stream: a pure re-ordering, against numpy reshapes
    (tests/test_gpu_digital.py:244-248)"""
    which, size = variant.split("-")
    size, nstreams = int(size[1:]), 3
    rng = np.random.default_rng(size + n)
    single = rng.integers(0, 255, n * nstreams * size, dtype=np.uint8)
    streams = np.ascontiguousarray(single.reshape(n, nstreams, size).transpose(1, 0, 2)).reshape(nstreams, n * size)
    cls = getattr(gpu, which)
    if which == "streams_to_stream":
        def call(blk, ins, outs, strides):
            return blk.work_device(n, outs[0].ptr(), ins[0].ptr(), strides[0])
        return Spec(lambda: cls(size, nstreams), [dict(arr=streams, itemsize=size)],
                    [Out(n * nstreams, np.uint8, itemsize=size)], call, [single.reshape(n * nstreams, size)], exact)

    def call(blk, ins, outs, strides):
        return blk.work_device(n, ins[0].ptr(), outs[0].ptr(), strides[1])
    return Spec(lambda: cls(size, nstreams), [dict(arr=single, itemsize=size)],
                [Out(n, np.uint8, n_streams=nstreams, itemsize=size)], call, [streams.reshape(nstreams, n, size)],
                exact)


def build_fft_vcc(gpu, po, wl, variant, n):
    N = int(variant[1:])
    rng = np.random.default_rng(N + n)
    x = _rc(rng, N * n)
    w = np.hamming(N).astype(np.float32)
    ref = po.fft_vcc(N, True, w, True, x)

    def call(blk, ins, outs, strides):
        return blk.work_device(n, ins[0].ptr(), outs[0].ptr())
    # tests/test_gpu_fft_pfb.py:54
    return Spec(lambda: gpu.fft_vcc(N, True, w, True), [dict(arr=x)], [Out(N * n, np.complex64)], call, [ref],
                rel(1e-5), ret=n)


def build_fft_filter_ccc(gpu, po, wl, variant, n):
    ntaps, decim = (int(v[1:]) for v in variant.split("-"))
    rng = np.random.default_rng(ntaps + decim)
    taps = _rc(rng, ntaps, scaled=False)
    ref_blk = po.FftFilterCcc(decim, taps)
    ns = ref_blk.nsamples
    nout = n * ns
    x = _rc(rng, nout * decim)
    ref = ref_blk.filter(nout, x)
    scale = np.abs(ref).max()

    def check(got, ref):                                                # tests/test_gpu_fft_pfb.py:311
        assert np.abs(got - ref).max() <= 2e-6 * np.log2(2 * ns) * scale

    def make():
        blk = gpu.fft_filter_ccc(decim, taps)
        assert blk.nsamples() == ns
        return blk
    return _simple(gpu, make, x, nout, np.complex64, ref, check)


def build_pfb_channelizer(gpu, po, wl, variant, n):
    M, osr = {"M8": (8, 1.0), "M5": (5, 1.0), "M8os2": (8, 2.0)}[variant]
    rng = np.random.default_rng(M * 10 + int(osr))
    taps = _rf(rng, 5 * M - M // 2, scaled=False)
    o = po.PfbChannelizer(M, taps, osr)
    tpf = o.taps_per_filter
    nout = max(n - n % o.output_multiple, o.output_multiple)
    nin = int(round(nout / osr))
    per = tpf + nin + 4
    ins = np.zeros((M, per), np.complex64)
    ins[:, tpf:] = _amp(_rc(rng, M * (nin + 4), scaled=False).reshape(M, nin + 4))
    ref, _used = o.general_work(nout, [ins[j] for j in range(M)])
    scale = np.abs(ref[np.isfinite(ref)]).max()

    def check(got, ref):                                                # tests/test_gpu_fft_pfb.py:209
        err = np.abs(got.reshape(nout, M) - ref).max()
        assert err <= 1e-5 * scale, err

    def call(blk, ins_, outs, strides):
        # d_updated from the constructor's set_taps: the first call produces nothing
        assert blk.general_work_device(nout, ins_[0].ptr(), strides[0], outs[0].ptr()) == 0
        return blk.general_work_device(nout, ins_[0].ptr(), strides[0], outs[0].ptr())
    return Spec(lambda: gpu.pfb_channelizer_ccf(M, taps, osr), [dict(arr=ins)], [Out(nout * M, np.complex64)], call,
                [ref], check, ret=nout)


def build_pfb_hier(gpu, po, wl, variant, n):
    """the one-call hierarchical entry: one interleaved stream in, M streams out"""
    M, osr = {"M8": (8, 1.0), "M5": (5, 1.0), "M8os2": (8, 2.0)}[variant]
    rng = np.random.default_rng(M * 10 + int(osr) + 1)
    taps = _rf(rng, 5 * M - M // 2, scaled=False)
    o = po.PfbChannelizer(M, taps, osr)
    tpf = o.taps_per_filter
    nout = max(n - n % o.output_multiple, o.output_multiple)
    tc = int(np.rint(nout / osr))
    x = _rc(rng, (tc + 4) * M)
    xil = np.concatenate([np.zeros(tpf * M, np.complex64), x])
    streams = [np.concatenate([np.zeros(tpf, np.complex64), x[j::M]]) for j in range(M)]
    ref, _used = o.general_work(nout, streams)
    scale = np.abs(ref).max()

    def check(got, ref):                                                # tests/test_gpu_fft_pfb.py:209
        err = np.abs(got - ref).max()
        assert err <= 1e-5 * scale, err

    def call(blk, ins_, outs, strides):
        assert blk.hier_work_device(nout, ins_[0].ptr(), outs[0].ptr(), strides[1]) == 0
        return blk.hier_work_device(nout, ins_[0].ptr(), outs[0].ptr(), strides[1])
    return Spec(lambda: gpu.pfb_channelizer_ccf(M, taps, osr), [dict(arr=xil)],
                [Out(nout, np.complex64, n_streams=M)], call, [np.ascontiguousarray(ref.T)], check, ret=nout)


def peak(tol):
    """within tol of the reference's peak"""
    def check(got, ref):
        assert got.shape == ref.shape
        err = float(np.abs(got - ref).max())
        assert err <= tol * float(np.abs(ref).max()), err
    return check


def first(p, check):
    """the first p items against the reference, the items behind them as they were pre-filled: a call that produces
    fewer items than the buffer holds writes nothing behind them"""
    def wrapped(got, ref):
        check(got[:p], ref)
        rest = np.ascontiguousarray(got[p:])
        pat = do.pattern(rest.dtype, do.UNWRITTEN)
        assert (rest.view(np.uint8).reshape(-1, rest.dtype.itemsize) == pat).all(), "items written behind the produced"
    return wrapped


def _sig(rng, n, cplx):
    x = rng.standard_normal(n).astype(np.float32)
    return _amp((x + 1j * rng.standard_normal(n)).astype(np.complex64) if cplx else x)


def build_fft_vfc(gpu, po, wl, variant, n):
    N = int(variant[1:])
    rng = np.random.default_rng(N + n)
    x = _amp(rng.standard_normal(N * n).astype(np.float32))
    w = np.hamming(N).astype(np.float32)
    ref = fft_real_ref.fft_vfc(x, N, w).astype(np.complex64).reshape(-1)
    tol = 1e-6 * max(np.log2(N), 1) * np.abs(ref).max()                  # tests/test_gpu_fft_real.py:261

    def check(got, ref):
        assert np.abs(got - ref).max() <= tol

    def call(blk, ins, outs, strides):
        return blk.work_device(n, ins[0].ptr(), outs[0].ptr())
    return Spec(lambda: gpu.fft_vfc(N, True, w), [dict(arr=x)], [Out(N * n, np.complex64)], call, [ref], check, ret=n)


def build_fft_filter_fff(gpu, po, wl, variant, n):
    ntaps, decim = (int(v[1:]) for v in variant.split("-"))
    rng = np.random.default_rng(7 * ntaps + decim)
    taps = rng.standard_normal(ntaps).astype(np.float32)
    ref_blk = fft_real_ref.FftFilterFff(decim, taps)
    ns = ref_blk.nsamples
    nout = n * ns
    x = _amp(rng.standard_normal(nout * decim).astype(np.float32))
    ref = np.asarray(ref_blk.filter(nout, x), np.float32)
    tol = 2e-6 * np.log2(2 * ns) * np.abs(ref).max()                     # tests/test_gpu_fft_real.py:33

    def check(got, ref):
        assert np.abs(got - ref).max() <= tol

    def make():
        blk = gpu.fft_filter_fff(decim, taps)
        assert blk.nsamples() == ns
        return blk
    return _simple(gpu, make, x, nout, np.float32, ref, check)


def build_pfb_decimator(gpu, po, wl, variant, n):
    M, ntaps, chan = 8, 8 * 7 - 3, 3                                    # 7 taps per filter: not a multiple of 4
    rng = np.random.default_rng(n)
    taps = wl.lowpass_taps(ntaps, 0.4 / M, 1.0)
    tpf = -(-ntaps // M)
    xs = np.stack([_sig(rng, n + tpf - 1, True) for _ in range(M)])
    ref = po.pfb_decimator_ccf(M, taps, chan, [xs[j] for j in range(M)], n)

    def call(blk, ins, outs, strides):
        assert blk.work_device(n, ins[0].ptr(), strides[0], outs[0].ptr()) == 0          # d_updated: 0 once
        return blk.work_device(n, ins[0].ptr(), strides[0], outs[0].ptr())
    # tests/test_gpu_pfbdec.py:75
    return Spec(lambda: gpu.pfb_decimator_ccf(M, taps, chan), [dict(arr=xs)], [Out(n, np.complex64)], call, [ref],
                peak(1e-5), ret=n)


def build_pfb_synth(gpu, po, wl, variant, n):
    mode, shape = variant.split("-")
    M, tpf, ns = {"M8": (8, 9, 8), "M5": (5, 6, 3), "M32": (32, 31, 32)}[shape]
    rng = np.random.default_rng(M + n)
    taps = (rng.standard_normal(M * tpf - 2) / np.sqrt(M * tpf)).astype(np.float32)
    xs = [_sig(rng, n, True) for _ in range(ns)]
    bufs = np.stack([pfb_synth_ref.with_history(x, tpf) for x in xs])
    ref = pfb_synth_ref.whole_literal(M, taps, xs)

    def make():
        blk = gpu.pfb_synthesis_filterbank_ccf(M, taps)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk

    def check(got, ref):                                                # tests/test_gpu_pfb_synth.py:62
        e = rel_err_max(got, ref)
        assert e < 1e-5, e

    def call(blk, ins, outs, strides):
        return blk.work_device(n * M, ins[0].ptr(), strides[0], ns, outs[0].ptr())
    return Spec(make, [dict(arr=bufs)], [Out(n * M, np.complex64)], call, [ref.astype(np.complex64)], check, ret=n * M)


def build_pfb_interp(gpu, po, wl, variant, n):
    mode, R, ntaps = variant.split("-")
    R, ntaps = int(R[1:]), int(ntaps[1:])
    rng = np.random.default_rng(R + ntaps)
    taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    x = _sig(rng, n, True)
    buf = np.concatenate([np.zeros(-(-ntaps // R) - 1, np.complex64), x])
    ref = pfb_synth_ref.whole_interp(po, R, taps, x)

    def make():
        blk = gpu.pfb_interpolator_ccf(R, taps)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk

    def fast(got, ref):                                                 # tests/test_gpu_pfb_synth.py:311
        assert rel_err_max(got, ref) < 1e-5
    return _simple(gpu, make, buf, R * n, np.complex64, ref, exact if mode == "GENERIC" else fast)


def _rs_taps(rng, kind, n):
    t = (rng.standard_normal(n) / np.sqrt(n)).astype(np.float32)
    return (t + 1j * rng.standard_normal(n) / np.sqrt(n)).astype(np.complex64) if kind == "ccc" else t


def _lt(tol):
    def check(got, ref):                                                # tests/test_gpu_resampler.py:112, :119
        assert got.shape == ref.shape and rel_err_max(got, ref) < tol
    return check


def build_interp_fir(gpu, po, wl, variant, n):
    kind, mode, I, ntaps = variant.split("-")
    I, ntaps = int(I[1:]), int(ntaps[1:])
    rng = np.random.default_rng(I + ntaps)
    taps = _rs_taps(rng, kind, ntaps)
    x = _sig(rng, n, kind != "fff")
    nt = resampler_ref.bank(taps, I)[0]
    buf = np.concatenate([np.zeros(nt - 1, x.dtype), x])
    ref = resampler_ref.whole_interp(po, I, taps, x)

    def make():
        blk = getattr(gpu, "interp_fir_filter_" + kind)(I, taps)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        assert blk.history() == nt
        return blk
    return _simple(gpu, make, buf, I * n, x.dtype, ref, exact if mode == "GENERIC" else _lt(1e-5))


def build_rational(gpu, po, wl, variant, n):
    kind, mode, I, D, ntaps = variant.split("-")
    I, D, ntaps = int(I[1:]), int(D[1:]), int(ntaps[1:])
    rng = np.random.default_rng(I * 10 + D)
    taps = _rs_taps(rng, kind, ntaps)
    nt = resampler_ref.bank(taps, I)[0]
    x = _sig(rng, max(n * D // I, 2) + nt, kind != "fff")
    ref = resampler_ref.whole_rational(po, I, D, taps, x)
    p = len(ref)
    while (p * D) // I > len(x):                                        # one call may not consume more than it is given
        p -= 1
    ref = ref[:p]

    def make():
        blk = getattr(gpu, "rational_resampler_base_" + kind)(I, D, taps)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk

    def call(blk, ins, outs, strides):
        return blk.general_work_device(p, len(x), ins[0].ptr(), outs[0].ptr())
    return Spec(make, [dict(arr=x)], [Out(p, x.dtype)], call, [ref], exact if mode == "GENERIC" else _lt(1e-5),
                ret=(p, (p * D) // I))


def build_arb(gpu, po, wl, variant, n):
    kind, mode, rate = variant.split("-")
    cplx, rate, R = kind == "ccf", float(rate[1:]), 32
    rng = np.random.default_rng(int(rate * 100))
    ntaps = R * 8 - 7
    taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    x = _sig(rng, max(int(n / rate), 12), cplx)
    ref_blk = arb_resampler_ref.ArbResamplerRef(rate, taps, R, cplx)
    buf = np.concatenate([np.zeros(ref_blk.history() - 1, x.dtype), x])
    assert ref_blk.general_work(10, buf)[1] == 0                        # the first call's 0
    ref, consumed = ref_blk.general_work(1 << 20, buf)
    ref = np.asarray(ref, x.dtype)
    p = len(ref)
    if mode == "GENERIC":
        check = exact
    else:                                                               # tests/test_gpu_arb_resampler.py:92
        ref = arb_whole_ref(rate, taps, R, x).astype(x.dtype)
        assert len(ref) == p
        check = _lt(1e-5)

    def make():
        blk = (gpu.pfb_arb_resampler_ccf if cplx else gpu.pfb_arb_resampler_fff)(rate, taps, R)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk

    def call(blk, ins, outs, strides):
        assert blk.general_work_device(p + 16, len(buf), ins[0].ptr(), outs[0].ptr()) == (0, 0)
        return blk.general_work_device(p + 16, len(buf), ins[0].ptr(), outs[0].ptr())
    return Spec(make, [dict(arr=buf)], [Out(p + 16, x.dtype)], call, [ref], first(p, check), ret=(p, consumed))


def build_frac(gpu, po, wl, variant, n):
    kind, mode, ratio = variant.split("-")
    cplx, ratio, phase = kind == "cc", np.float32(float(ratio[1:])), np.float32(0.5)
    rng = np.random.default_rng(int(ratio * 100))
    x = _sig(rng, max(int(n * float(ratio)), 12) + 8, cplx)
    ref, consumed = fractional_interp_ref.FractionalInterpolatorRef(phase, ratio, cplx).general_work(1 << 20, x)
    ref = np.asarray(ref, x.dtype)
    p = len(ref)
    assert p > 0
    if mode == "GENERIC":
        check = exact
    else:                                                               # tests/test_gpu_fractional_interp.py:104
        ii, imu, _mu = fractional_interp_ref.whole_stream_schedule(phase, ratio, len(x))
        ref = fractional_interp_ref.eval_schedule(x, ii, imu, f64=True)
        assert len(ref) == p
        check = _lt(1e-5)

    def make():
        blk = (gpu.fractional_interpolator_cc if cplx else gpu.fractional_interpolator_ff)(phase, ratio)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk

    def call(blk, ins, outs, strides):
        return blk.general_work_device(p + 16, len(x), ins[0].ptr(), outs[0].ptr())
    return Spec(make, [dict(arr=x)], [Out(p + 16, x.dtype)], call, [ref], first(p, check), ret=(p, consumed))


RS_DTYPE = {"ff": np.float32, "cc": np.complex64, "ss": np.int16, "ii": np.int32}
# tests/test_gpu_running_sum.py:143
MA_SCALE = {"ff": np.float32(0.1), "cc": np.complex64(0.1 - 0.05j), "ss": 3, "ii": 3}


def _rs_input(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "ss":
        return rng.integers(-32768, 32768, n).astype(np.int16)
    if kind == "ii":
        return rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    x = rng.uniform(-1, 1, n) + 1.0
    return _amp((x + 1j * (rng.uniform(-1, 1, n) - 0.5)).astype(np.complex64) if kind == "cc" else x.astype(np.float32))


def build_runsum(gpu, po, wl, variant, n):
    """GENERIC (and the integer kinds) bit for bit, FAST within 1e-5 of the float64 form's peak
    (tests/test_gpu_running_sum.py:52, :194, :259)"""
    name, mode = variant.split("-")
    what, kind = name.rsplit("_", 1)
    is_exact = mode == "GENERIC" or kind in ("ss", "ii")
    R = running_sum_ref
    if what == "dc_blocker":
        D = 33
        x = _rs_input(kind, n, 1)
        ref = R.DcBlocker(D, True, kind == "cc").work(x) if is_exact else \
            R.DcBlocker(D, True, kind == "cc", np.float64).work(x)
        make0 = lambda: getattr(gpu, name)(D, True)
    elif what == "moving_average":
        length, scale = 10, MA_SCALE[kind]
        x = _rs_input(kind, n + length - 1, 2)
        ref = R.moving_average_calls(kind, x, length, scale, n, 4096) if is_exact else \
            R.moving_average_f64(x, length, complex(scale) if kind == "cc" else float(scale), n)
        make0 = lambda: getattr(gpu, name)(length, scale, 4096)
    else:
        decim = 3
        x = _rs_input(kind, n * decim, 3)
        ref = R.integrate(kind, x, decim, n) if is_exact else R.integrate_f64(x, decim, n)
        make0 = lambda: getattr(gpu, name)(decim)

    def make():
        blk = make0()
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk
    return _simple(gpu, make, x, n, RS_DTYPE[kind], np.asarray(ref), exact if is_exact else peak(1e-5))


RUNSUM_VARIANTS = ["%s-%s" % (b, m)
                   for b in ("dc_blocker_ff", "dc_blocker_cc", "moving_average_ff", "moving_average_cc",
                             "moving_average_ss", "moving_average_ii", "integrate_ff", "integrate_ss")
                   for m in ("GENERIC", "FAST")]


def build_spectrum(gpu, po, wl, variant, n):
    S = spectrum_ref
    rng = np.random.default_rng(n)
    if variant == "complex_to_mag_squared":
        z = _amp((rng.normal(size=n) * 10 ** rng.uniform(-3, 3, n) + 1j * rng.normal(size=n)).astype(np.complex64))
        return _simple(gpu, lambda: gpu.complex_to_mag_squared(1), z, n, np.float32, S.mag_squared(z), exact)
    if variant.startswith("single_pole_iir_filter_ff"):
        mode = variant.rsplit("-", 1)[1]
        x = _amp((rng.normal(size=n) + 2.0).astype(np.float32))

        def make():
            blk = gpu.single_pole_iir_filter_ff(0.125, 1)
            blk.set_mode(getattr(gpu, "MODE_" + mode))
            return blk
        if mode == "GENERIC":                                           # tests/test_gpu_spectrum.py:78
            return _simple(gpu, make, x, n, np.float32, S.SinglePoleIir(0.125, 1, 1).work(x.reshape(1, -1)).reshape(-1),
                           exact)
        want, _ = S.iir_f64(x.reshape(n, 1), 0.125)                     # tests/test_gpu_spectrum.py:97
        return _simple(gpu, make, x, n, np.float32, want.reshape(-1), peak(1e-5))
    # 60 decades at amplitude 1; 50 where a scale of up to 2^40 comes on top, so that every input stays a normal float
    decades = 30 if AMPLITUDE == 1 else 25
    x = _amp(np.logspace(-decades, decades, n).astype(np.float32))
    want = S.nlog10_f64(x, 10, 0)                                      # n and k of tests/golden/ref_qa_spectrum.json

    def ulps(got, ref):                                                 # tests/test_gpu_spectrum.py:102, :116
        u = np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert u.max() <= 4, u.max()
    return _simple(gpu, lambda: gpu.nlog10_ff(10, 1, 0), x, n, np.float32, want, ulps)


def build_keep_one_in_n(gpu, po, wl, variant, n):
    size, k = int(variant[1:]), 3
    rng = np.random.default_rng(size + n)
    items = rng.integers(0, 256, (n, size), dtype=np.uint8)
    kept = spectrum_ref.KeepOneInN(k).kept(n)
    want = items[list(kept)]
    p = len(want)

    def call(blk, ins, outs, strides):
        assert blk.produced(n) == p
        return blk.work_device(n, ins[0].ptr(), outs[0].ptr())
    return Spec(lambda: gpu.keep_one_in_n(size, k), [dict(arr=items.reshape(-1), itemsize=size)],
                [Out(p, np.uint8, itemsize=size)], call, [want], exact, ret=p)


def per_stream(counts, check):
    """stream s: its first counts[s] items against the reference's, nothing written behind them"""
    def wrapped(got, ref):
        assert len(got) == len(ref) == len(counts)
        for s, p in enumerate(counts):
            first(p, check)(got[s], np.asarray(ref[s]))
    return wrapped


def build_logpwrfft(gpu, po, wl, variant, n):
    """in each mode bit for bit against the library's five blocks in the reference's order on host buffers
    (tests/test_gpu_logpwrfft.py:128), and against the float64 chain of spectrum_ref.py within the bounds of
    tests/test_gpu_logpwrfft.py:268"""
    kind, N, mode = variant.split("-")
    N, mode = int(N), getattr(gpu, "MODE_" + mode)
    alpha = 0.2
    rng = np.random.default_rng(N + n)
    t = np.arange(n * N)
    if kind == "c":
        x = (0.5 * np.exp(2j * np.pi * 0.1234 * t) + 0.05 * (rng.normal(size=t.size) + 1j * rng.normal(size=t.size))
             ).astype(np.complex64)
    else:
        x = (0.5 * np.cos(2 * np.pi * 0.1234 * t) + 0.05 * rng.normal(size=t.size)).astype(np.float32)
    x = _amp(x)
    ref = Deferred(lambda: np.asarray(LogpwrChain(gpu, kind, N, 1, 1, alpha, True, None, 2.0, mode).work(n, x),
                                      np.float32))
    wd = logpwrfft_ref.blackmanharris(N)
    k = np.float32(logpwrfft_ref.k_of(N, wd, 2.0))
    ref_db, p_ref, _ = spectrum_ref.chain_f64(x.reshape(n, N), np.asarray(wd, np.float64).astype(np.float32), alpha, k)

    def check(got, ref):
        exact(got, ref)
        out = got.reshape(n, N).astype(np.float64)
        # what the logarithm sees: gr_nlog10_ff takes max(p, 1e-18), so a spectrum below -180 dB reads -180 dB (no
        # power of this file's amplitude-1 signal is that small)
        p_lin = np.maximum(p_ref, 1e-18)
        e_lin = np.abs(10.0 ** ((out - float(k)) / 10.0) - p_lin).max() / p_lin.max()
        near = p_ref >= p_ref.max() * 1e-4
        e_db = np.abs(out - ref_db)[near].max()
        assert e_lin <= 2.5e-6 * max(np.log2(N), 1) and e_db <= 0.02, (e_lin, e_db)

    def make():
        blk = (gpu.logpwrfft_c if kind == "c" else gpu.logpwrfft_f)(30.0 * N, N, 2.0, 30.0, alpha, True, None)
        assert blk.decimation() == 1
        blk.set_mode(mode)
        return blk

    def call(blk, ins, outs, strides):
        return blk.work_device(n, ins[0].ptr(), outs[0].ptr())
    return Spec(make, [dict(arr=x)], [Out(n * N, np.float32)], call, [ref], check, ret=n,
                cpu_ref=[ref_db.astype(np.float32).reshape(-1)])


def _sq_bursts(n):
    return ((n // 8, n // 2), (5 * n // 8, 7 * n // 8))


def build_squelch(gpu, po, wl, variant, n):
    """two streams back to back (the entries take no stride: an odd n puts the second stream on an odd item), gate on,
    the produced counts checked; outputs bit for bit in both modes (tests/test_gpu_squelch.py)"""
    name, mode = variant.split("-")
    cc = name != "pwr_squelch_ff"
    alpha, db = 0.3, -10.0
    xs = []
    for seed in (1, 2):
        x = squelch_ref.signal(seed, n=n, bursts=_sq_bursts(n))
        x = _amp(x if cc else x.real.astype(np.float32))
        if n > 100:                                                     # the no-exceptions condition of that file
            assert squelch_ref.closest_approach(x, alpha, db) > 1e-9
        xs.append(x)
    if name == "simple_squelch_cc":
        refs = [squelch_ref.SimpleSquelch(db, alpha).work(x) for x in xs]
        make0 = lambda: gpu.simple_squelch_cc(db, alpha)
    else:
        refs = [squelch_ref.PwrSquelch(db, alpha, 7, True, cc).work(x) for x in xs]
        make0 = lambda: getattr(gpu, name)(db, alpha, 7, True)
    return _two_streams(gpu, make0, mode, xs, refs, n)


def _two_streams(gpu, make0, mode, xs, refs, n, with_counts=True):
    counts = [len(r) for r in refs]

    def make():
        blk = make0()
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        blk.set_streams(2)
        return blk

    def call(blk, ins, outs, strides):
        if with_counts:
            return blk.work_device(n, ins[0].ptr(), outs[0].ptr(), outs[1].ptr())
        return blk.work_device(n, ins[0].ptr(), outs[0].ptr())
    outs = [Out(n, xs[0].dtype, n_streams=2, packed=True)]
    ref, check = [refs], [per_stream(counts, exact)]
    if with_counts:
        outs.append(Out(2, np.int32))
        ref.append(np.array(counts, np.int32))
        check.append(exact)
    return Spec(make, [dict(arr=np.stack(xs), packed=True)], outs, call, ref, check)


def build_ctcss(gpu, po, wl, variant, n):
    """tests/test_gpu_ctcss_squelch.py's signal, shape and condition; two streams, gate on"""
    rate, L, freq, level = 500, 250, 100.0, 0.01
    xs = []
    for seed in (1, 2):
        x = ctcss_ref.signal(seed, rate, L, True)
        margin, deviation = ctcss_ref.condition(rate, L, freq, level, x)
        assert margin >= 10 * deviation
        xs.append(_amp(np.ascontiguousarray(x[:n], np.float32)))
    refs = [ctcss_ref.CtcssSquelch(rate, freq, level, L, 64, True).work(x) for x in xs]
    return _two_streams(gpu, lambda: gpu.ctcss_squelch_ff(rate, freq, level, L, 64, True), variant, xs, refs, n)


def build_agc2(gpu, po, wl, variant, n):
    """every mode of agc2_cc is the reference's recurrence bit for bit (tests/test_gpu_agc.py)"""
    params = agc_ref.sets("agc2_cc")[0]
    xs = [_amp(np.ascontiguousarray(agc_ref.signal(seed, "agc2_cc")[1400:1400 + n])) for seed in (1, 2)]
    refs = [agc_ref.serial("agc2_cc", x, params).out for x in xs]
    return _two_streams(gpu, lambda: gpu.agc2_cc(*params), variant, xs, refs, n, with_counts=False)


def build_mm_ff(gpu, po, wl, variant, n):
    omega, gm = 4.3, 0.3
    go = 0.25 * gm * gm
    rng = np.random.default_rng(n)
    x = _amp(_fsk_soft(rng, max(n // 4, 8), sps=4)[:n])
    n = len(x)
    ref, st = po.chain_mm(omega, go, 0.5, gm, 0.005, x)
    p = len(ref)

    def call(blk, ins, outs, strides):
        return blk.general_work_device(n, n, ins[0].ptr(), outs[0].ptr(), outs[1].ptr())
    return Spec(lambda: gpu.clock_recovery_mm_ff(omega, go, 0.5, gm, 0.005), [dict(arr=x)],
                [Out(n, np.float32), Out(2, np.int32)], call, [ref, np.array([p, st["consumed"]], np.int32)],
                [first(p, exact), exact])


def build_run_captures(gpu, po, wl, variant, n):
    mode, ntaps, decim = variant.split("-")
    ntaps, decim = int(ntaps[1:]), int(decim[1:])
    c = wl.CFG2
    gain = c["demod_gain"]
    proto = wl.cfg2_proto_taps() if ntaps == 256 else wl.lowpass_taps(ntaps, 100e3, 10e6).astype(np.complex64)
    xs = np.stack([_amp(wl.fsk4_capture(n, stream_id=70 + s)) for s in range(2)])
    nout = n // decim
    refs = np.stack([po.chain_xlating_demod(decim, proto, c["center_freq"], c["fs"], gain, x[:nout * decim])
                     for x in xs])

    def make():
        blk = gpu.xlating_demod(decim, proto, c["center_freq"], c["fs"], gain)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        return blk

    def close(got, ref):                                                # tests/test_gpu_fir.py:476
        for s in range(2):
            ok, worst = demod_close(got[s], ref[s], gain=gain)
            assert ok, (s, worst)

    def call(blk, ins, outs, strides):
        return blk.run_captures_device(2, n, ins[0].ptr(), strides[0], outs[0].ptr(), strides[1])
    return Spec(make, [dict(arr=xs)], [Out(nout, np.float32, n_streams=2)], call, [refs],
                exact if mode == "GENERIC" else close)


def _fetch(gpu, ptr, count, dtype):
    """`count` items at a device address the handle owns"""
    import ctypes
    a = np.empty(count, dtype)
    gpu.lib().grhip_memcpy_d2h(a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), a.nbytes)
    return a


def build_dmr_chain(gpu, po, wl, variant, n):
    """GENERIC: every stage bit exact, decisions included.  FAST (the batched matrix-core FIR, or what takes its place
    on an odd capture stride): the criteria of tests/test_gpu_chain.py:70-104 and :602-614 -- the demodulator's output
    within demod_close, as many symbols as the reference, the soft symbols within that file's quantiles, the tail
    exact on the symbols the chain produced, decisions that differ from the reference's only where its own soft
    symbol is within float noise of a threshold"""
    tail, mode = variant.split("-")
    c, c4 = wl.CFG2, wl.CFG4
    code, thr = wl.access_code_string(), c4["threshold"]
    xs = np.stack([_amp(wl.fsk4_capture(n, stream_id=40 + s)) for s in range(2)])
    four, alpha, generic = tail == "four_level", 0.002, mode == "GENERIC"
    per = 2 if four else 1                                              # items per symbol (tests/test_gpu_chain.py:578)
    n_dem = n // c["decim"]

    decided = {}

    def decide(soft):
        """the tail behind the clock recovery, on the CPU: (slicer symbols or bits, the correlator's output); computed
        once per distinct run of soft symbols"""
        key = soft.tobytes()
        if key not in decided:
            sym = po.PagerSlicer(alpha).work(soft) if four else po.binary_slicer_fb(soft)
            decided[key] = sym, po.CorrelateAccessCode(code, thr).work(po.unpack_k_bits_bb(2, sym) if four else sym)
        return decided[key]

    dems, softs, refs = [], [], []
    for x in xs:
        dem = po.chain_xlating_demod(c["decim"], wl.cfg2_proto_taps(), c["center_freq"], c["fs"], c["demod_gain"], x)
        soft, _ = po.chain_mm(c4["omega"], c4["gain_omega"], c4["mu"], c4["gain_mu"], c4["omega_relative_limit"], dem)
        dems.append(dem)
        softs.append(soft)
        refs.append(decide(soft)[1])
    counts = [len(r) for r in refs]
    nout = per * n_dem

    def make():
        blk = gpu.dmr_chain(c["decim"], wl.cfg2_proto_taps(), c["center_freq"], c["fs"], c["demod_gain"],
                            c4["omega"], c4["gain_omega"], c4["mu"], c4["gain_mu"], c4["omega_relative_limit"],
                            code, thr, 2, n)
        blk.set_mode(getattr(gpu, "MODE_" + mode))
        if four:
            blk.set_four_level(True, alpha)
        return blk

    def bits(got, ref):
        for s, p in enumerate(counts):
            exact(got[s][:p], np.asarray(ref[s]))

    def call(blk, ins, outs, strides):
        return blk.run_device(ins[0].ptr(), n, strides[0], outs[0].ptr(), strides[1], outs[1].ptr())

    def fast_stages(blk, outs):
        """the intermediate products of a FAST run against the reference's; returns them, for the re-run to equal"""
        got_bits, nb = outs[0].payload(), outs[1].payload()
        (p_dem, s_dem), (p_soft, s_soft) = blk.intermediate(0), blk.intermediate(1)
        kept = []
        for s in range(2):
            nsym = len(softs[s])
            assert nb[s] == per * nsym, (nb[s], per * nsym)
            dem = _fetch(gpu, p_dem + 4 * s * s_dem, n_dem, np.float32)
            ok, worst = demod_close(dem, dems[s])
            assert ok, worst
            soft = _fetch(gpu, p_soft + 4 * s * s_soft, nsym, np.float32)
            e = np.abs(soft - softs[s])
            assert np.median(e) <= 2e-5 and np.quantile(e, 0.99) <= 5e-3 and e.max() <= 0.1
            sym, mine = decide(soft)
            assert np.array_equal(got_bits[s][:nb[s]], mine)
            ref_sym = decide(softs[s])[0]
            if four:
                p_sym, s_sym = blk.intermediate(2)
                assert np.array_equal(_fetch(gpu, p_sym + s * s_sym, nsym, np.uint8), sym)
                assert (ref_sym != sym).mean() <= 1e-4
            else:
                flips = sym != ref_sym
                assert np.all(np.abs(softs[s][flips]) < 1e-2) and flips.sum() <= 8
                mine_pos, ref_pos = np.nonzero(mine & 2)[0], np.nonzero(refs[s] & 2)[0]
                planted = ref_pos[np.isin(ref_pos, mine_pos)]
                assert len(planted) >= len(ref_pos) - 1 and len(planted) >= len(mine_pos) - 1
            kept += [dem.tobytes(), soft.tobytes()]
        return kept

    outs = [Out(nout, np.uint8, n_streams=2), Out(2, np.int32)]
    if generic:
        return Spec(make, [dict(arr=xs)], outs, call, [refs, np.array(counts, np.int32)], [bits, exact])
    return Spec(make, [dict(arr=xs)], outs, call, [], [], post=fast_stages)


def _by_kind(variant):
    """rows whose variant starts with the signature (ccf, fff, cc, ff, ...): complex or float items in and out"""
    s = 8 if variant[0] == "c" else 4
    return s, s


def _by_suffix(variant):
    """the stream adapters and keep_one_in_n: the item size is the variant's last number"""
    s = int(variant.rsplit("s", 1)[1])
    return s, s


def _runsum_items(variant):
    s = np.dtype(RS_DTYPE[variant.split("-")[0][-2:]]).itemsize
    return s, s


ROWS = [
    Row("fir_filter", _by_kind, (3 * 1024 + 29, 3), build_fir, FIR_VARIANTS),                        # GT_NT = 1024
    Row("freq_xlating_fir_filter_ccc", (8, 8), (3 * 1024 + 29, 3), build_xlating, XL_VARIANTS),
    Row("xlating_demod", (8, 4), (3 * 1020 + 29, 3), build_xlating_demod, XD_VARIANTS),   # 1020 new outputs per tile
    Row("quadrature_demod_cf", (8, 4), (3 * 1024 + 29, 3), build_quad_demod),
    Row("pager_slicer_fb", (4, 1), (3 * 1024 + 29, 3), build_pager_slicer),
    Row("unpack_k_bits_bb", (1, 1), (3 * 4096 + 29, 5), build_unpack, ("k2", "k3")),      # 16 items per lane x 256
    Row("framer_sink_1", (1, 0), (3 * 2048 + 29, 21), build_framer, ("wave", "segments")),   # 32 items per word x 64
    Row("stream_to_streams", _by_suffix, (3 * 1024 + 29, 3), build_adapter,
        ["stream_to_streams-s%d" % s for s in (1, 2, 4, 8, 16)], strided=True),
    Row("streams_to_stream", _by_suffix, (3 * 1024 + 29, 3), build_adapter,
        ["streams_to_stream-s%d" % s for s in (1, 2, 4, 8, 16)], strided=True),
    Row("vector_to_streams", _by_suffix, (3 * 1024 + 29, 3), build_adapter,
        ["vector_to_streams-s%d" % s for s in (1, 2, 4, 8, 16)], strided=True),
    Row("fft_vcc", (8, 8), (3, 1), build_fft_vcc, ("N32", "N1024", "N4096", "N240")),    # one FFT per tile
    Row("fft_filter_ccc", (8, 8), (3, 1), build_fft_filter_ccc, ("t64-d2", "t255-d1")),
    Row("pfb_channelizer_ccf", (8, 8), (3 * 512 + 29, 3), build_pfb_channelizer, ("M8", "M5", "M8os2"), strided=True),
    Row("pfb_channelizer_hier", (8, 8), (3 * 512 + 29, 3), build_pfb_hier, ("M8", "M5", "M8os2"), strided=True),
    Row("fft_vfc", (4, 8), (3, 1), build_fft_vfc, ("N32", "N1024", "N4096", "N240")),
    Row("fft_filter_fff", (4, 4), (3, 1), build_fft_filter_fff, ("t64-d2", "t255-d1")),
    Row("pfb_decimator_ccf", (8, 8), (3 * 1024 + 29, 3), build_pfb_decimator, strided=True),       # PFBDEC_TILE
    Row("pfb_synthesis_filterbank_ccf", (8, 8), (3 * 512 + 29, 3), build_pfb_synth,
        ["%s-%s" % (m, sh) for m in ("GENERIC", "FAST") for sh in ("M8", "M5", "M32")], strided=True),
    Row("pfb_interpolator_ccf", (8, 8), (3 * 512 + 29, 3), build_pfb_interp,
        ["%s-%s" % (m, sh) for m in ("GENERIC", "FAST") for sh in ("R3-t13", "R4-t128")]),
    Row("interp_fir_filter", _by_kind, (3 * 512 + 29, 3), build_interp_fir,
        ["%s-%s-%s" % (k, m, sh) for k in ("ccf", "fff") for m in ("GENERIC", "FAST") for sh in ("I3-t14", "I4-t61")]),
    Row("rational_resampler_base", _by_kind, (3 * 1024 + 29, 3), build_rational,
        ["%s-%s-%s" % (k, m, sh) for k in ("ccf", "fff") for m in ("GENERIC", "FAST")
         for sh in ("I3-D2-t303", "I2-D3-t17")]),
    Row("pfb_arb_resampler", _by_kind, (3 * 1024 + 29, 3), build_arb,
        ["%s-%s-%s" % (k, m, r) for k in ("ccf", "fff") for m in ("GENERIC", "FAST") for r in ("r0.7", "r1.25")]),
    Row("fractional_interpolator", _by_kind, (3 * 1024 + 29, 3), build_frac,
        ["%s-%s-%s" % (k, m, r) for k in ("cc", "ff") for m in ("GENERIC", "FAST") for r in ("r0.75", "r1.3")]),
    Row("runsum", _runsum_items, (3 * 2304 + 37, 3), build_runsum, RUNSUM_VARIANTS),      # FAST tile 2304, GENERIC 256
    Row("spectrum", lambda v: (8 if v == "complex_to_mag_squared" else 4, 4), (3 * 256 + 37, 3), build_spectrum,
        ("complex_to_mag_squared", "single_pole_iir_filter_ff-GENERIC", "single_pole_iir_filter_ff-FAST", "nlog10_ff")),
    Row("keep_one_in_n", _by_suffix, (3 * 256 + 37, 4), build_keep_one_in_n, ("s1", "s2", "s4", "s8")),
    Row("logpwrfft", lambda v: (8 if v[0] == "c" else 4, 4), (3, 1), build_logpwrfft,       # one frame per tile
        ["%s-%s" % (sh, m) for sh in ("c-64", "c-1024", "f-64", "f-1024", "c-100") for m in ("GENERIC", "FAST")]),
    Row("squelch", lambda v: (4, 4) if v.startswith("pwr_squelch_ff") else (8, 8), (3 * 256 + 37, 4), build_squelch,
        ["%s-%s" % (b, m) for b in ("pwr_squelch_cc", "pwr_squelch_ff", "simple_squelch_cc")
         for m in ("GENERIC", "FAST")]),                                                   # 256-item detector chunks
    Row("ctcss_squelch_ff", (4, 4), (80 * 250 + 37, 7), build_ctcss, ("GENERIC", "FAST")),          # blocks of 250
    Row("agc2_cc", (8, 8), (3 * 256 + 37, 4), build_agc2, ("GENERIC", "FAST")),
    Row("clock_recovery_mm_ff", (4, 4), (3 * 4096 + 37, 30), build_mm_ff),                # 4096-float window refills
    Row("xlating_demod_run_captures", (8, 4), (3 * 4080 + 61, 9), build_run_captures,
        ("GENERIC-t256-d4", "FAST-t256-d4", "GENERIC-t33-d1"), strided=True),
    # the short capture is 4000 samples, not less than a chunk: the chain's criteria need symbols to judge (about 100
    # here, at 10 demodulator outputs per symbol) and demod_close a stretch behind the FIR's 64-output start-up
    Row("dmr_chain", (8, 1), (3 * 8000 + 43, 4000), build_dmr_chain,           # tiles of 2000 FIR outputs, decimation 4
        ["%s-%s" % (t, m) for t in ("two_level", "four_level") for m in ("GENERIC", "FAST")], strided=True),
]


def _params():
    out = []
    for row in ROWS:
        for variant in row.variants:
            si, so = row.item_sizes(variant)
            for a, b in offset_pairs(si, so):
                for stride in (("aligned", "odd") if row.strided else ("",)):
                    rid = "-".join(p for p in (row.id if not variant.startswith(row.id) else "", variant,
                                               "in%d" % a, "out%d" % b, stride) if p)
                    out.append(pytest.param(row, variant, a, b, stride, id=rid))
    return out


_SPECS = {}


def _spec(gpu, po, wl, row, variant, n):
    key = (row.id, variant, n)
    if key not in _SPECS:
        _SPECS[key] = row.build(gpu, po, wl, variant, n)
    return _SPECS[key]


def _run_once(gpu, spec, item_sizes, in_off, out_off, stride_kind, poison):
    import torch
    ins, outs, strides = [], [], []
    for i in spec.ins:
        arr = np.asarray(i["arr"])
        itemsize = i.get("itemsize") or arr.dtype.itemsize
        stride = None
        if arr.ndim == 2 and not i.get("packed"):
            stride = _stride(stride_kind or "aligned", arr.shape[1] * arr.dtype.itemsize // itemsize, itemsize)
        g = do.guarded(arr, in_off, stride_items=stride, itemsize=itemsize)
        if poison != do.POISON:
            g.repoison(poison)
        ins.append(g)
        strides.append(g.stride_items)
    for o in spec.outs:
        itemsize = o.itemsize or np.dtype(o.dtype).itemsize
        stride = _stride(stride_kind or "aligned", o.n, itemsize) if o.n_streams and not o.packed else None
        g = do.guarded_output(o.n, o.dtype, out_off, n_streams=o.n_streams, stride_items=stride, itemsize=o.itemsize)
        outs.append(g)
        strides.append(g.stride_items)
    assert ins[0].itemsize == item_sizes[0] and (outs[0].itemsize if outs else 0) == item_sizes[1], \
        "the row's item sizes are not those of its buffers"
    blk = spec.make()
    try:
        ret = spec.call(blk, ins, outs, strides)
    except gpu.GrhipError as e:
        ret = e
    torch.cuda.synchronize()
    post = spec.post(blk, outs) if spec.post and not isinstance(ret, Exception) else None
    return ret, outs, post


def _conditions(in_off, out_off, si, so, stride_kind):
    c = set()
    if (in_off * si) % 16:
        c.add("in")
    if so and (out_off * so) % 16:
        c.add("out")
    if stride_kind == "odd":
        c.add("odd_stride")
    return c


@pytest.mark.parametrize("row,variant,in_off,out_off,stride_kind", _params())
def test_device_entry_at_offset(gpu, po, wl, row, variant, in_off, out_off, stride_kind):
    si, so = row.item_sizes(variant)
    may_refuse = _refusals(row, variant, _conditions(in_off, out_off, si, so, stride_kind))
    for n in row.sizes:
        spec = _spec(gpu, po, wl, row, variant, n)
        ret, outs, post = _run_once(gpu, spec, (si, so), in_off, out_off, stride_kind, do.POISON)
        if isinstance(ret, Exception):
            assert ret.code == EINVAL and may_refuse, "a refusal that include/grhip.h does not state: %s" % ret
            for o in outs:                                           # and no output byte changed
                assert do.unwritten_items(o).all()
                do.check_guards(o)
            continue
        assert not may_refuse, "listed as a refusal, but the entry answered"
        if spec.ret is not None:
            assert ret == spec.ret, (ret, spec.ret)
        got = [o.payload() for o in outs]
        for k, (g_, r_) in enumerate(zip(got, spec.ref)):
            check = spec.check[k] if isinstance(spec.check, list) else spec.check
            if isinstance(r_, list):                                 # per stream, of unequal lengths
                check(g_, r_)
            else:
                check(g_.reshape(np.shape(r_)) if g_.size == np.size(r_) else g_, np.asarray(r_))
        for o in outs:
            do.check_guards(o)
        if spec.ref_post is not None:
            assert post == spec.ref_post
        # input guards under another poison, fresh handle: bit-identical
        _ret2, outs2, post2 = _run_once(gpu, spec, (si, so), in_off, out_off, stride_kind, do.POISON2)
        for o, o2 in zip(outs, outs2):
            assert bits_equal(o2.payload(), o.payload()), "the result depends on what the input's guards hold"
            do.check_guards(o2)
        assert post2 == post
