"""CPU tests of the binding's one host work() path for the blocks that take streams x n steps back to back
(_Block._work_in / _work_out / _stream_work, _stream_block.work): the item arithmetic, the short-input check, the
buffers handed to C and what comes back.  The C entry is replaced by a recorder: no library and no device needed."""
import ast
import collections
import ctypes as C

import numpy as np
import pytest

MARK = 7

# how a family's work is called and what it hands back:
#   "items"    work(input_items, n=None[, flag])        -> the output, or the tuple of it and the optional outputs
#   "count"    work(noutput_items, input_items)         -> the output
#   "general"  general_work(noutput_items, input_items, ninput_items=None) -> (output, consumed)
#   "squelch"  work(input_items, n_in=None)             -> every stream's produced items
Spec = collections.namedtuple("Spec", "cls style in_dtype views per_in per_out out_dtype flag optional want attrs answers")


def _spec(cls, in_dtype, out_dtype, style="items", views=False, per_in=1, per_out=1, flag=None, optional=0, want=False, attrs=(),
          answers=()):
    return Spec(cls, style, in_dtype, views, per_in, per_out, out_dtype, flag, optional, want, dict(attrs), dict(answers))


SPECS = [
    _spec("agc_cc", np.complex64, np.complex64),
    _spec("costas_loop_cc", np.complex64, np.complex64, flag="freq", optional=1),
    _spec("costas_loop_cc", np.complex64, np.complex64, flag="freq", optional=1, want=True),
    _spec("fll_band_edge_cc", np.complex64, np.complex64, flag="aux", optional=3),
    _spec("fll_band_edge_cc", np.complex64, np.complex64, flag="aux", optional=3, want=True),
    _spec("constellation_receiver_cb", np.complex64, np.uint8, flag="floats", optional=3, want=True),
    _spec("constellation_demod_cb", np.complex64, np.uint8, per_out=3, answers={"bits_per_symbol": 3}),
    _spec("constellation_decoder_cb", np.complex64, np.uint8, per_in=2, attrs={"_per_in": 2}),
    _spec("scrambler_bb", np.uint8, np.uint8),
    _spec("unpacked_to_packed_bb", np.uint8, np.uint8, style="general"),
    _spec("chunks_to_symbols_bc", np.uint8, np.complex64, per_out=2, answers={"D": 2}),
    _spec("frequency_modulator_fc", np.float32, np.complex64),
    _spec("bytes_to_syms", np.int8, np.float32, views=True, per_out=8),
    _spec("chunks_to_symbols_bf", np.int8, np.float32, views=True, per_out=3, answers={"D": 3}),
    _spec("gmsk_mod", np.int8, np.complex64, views=True, per_out=16, flag="want_freq", optional=1,
          answers={"samples_per_symbol": 2}),
    _spec("gmsk_mod", np.int8, np.complex64, views=True, per_out=16, flag="want_freq", optional=1, want=True,
          answers={"samples_per_symbol": 2}),
    _spec("trellis_encoder_bs", np.uint8, np.int16),
    _spec("trellis_metrics_c", np.complex64, np.float32, per_in=2, per_out=4, attrs={"_per_in": 2, "_per_out": 4}),
    _spec("trellis_viterbi_combined_cs", np.complex64, np.int16, per_in=2, attrs={"_per_in": 2}),
    _spec("complex_to_mag", np.complex64, np.float32, style="count", per_in=3, per_out=3, attrs={"_per_in": 3, "_per_out": 3}),
    _spec("dc_blocker_ff", np.float32, np.float32, style="count"),
    _spec("iir_filter_ffd", np.float32, np.float32),
    _spec("pwr_squelch_cc", np.complex64, np.complex64, style="squelch"),
    _spec("ctcss_squelch_ff", np.float32, np.float32, style="squelch"),
]
IDS = ["%s%s" % (s.cls, "-" + s.flag if s.want else "") for s in SPECS]


class Recorder(object):
    """stands in for _Block._call: answers the getters a block asks while it sizes its buffers, and for the work entry
    notes every argument and fills the output arrays.  _ptr is wrapped so that a pointer leads back to its array."""

    def __init__(self, binding, monkeypatch, spec, streams):
        self.spec, self.streams, self.arrays, self.calls = spec, streams, {}, []
        ptr = binding._ptr

        def noting_ptr(a):
            p = ptr(a)
            self.arrays[p.value] = a
            return p
        monkeypatch.setattr(binding, "_ptr", noting_ptr)

    def __call__(self, name, *args):
        if name in self.spec.answers:
            return self.spec.answers[name]
        assert name in ("work", "general_work"), name
        n_scalars = 2 if name == "general_work" else 1
        assert all(type(a) is int for a in args[:n_scalars])
        bufs = [self.arrays.get(a.value) if isinstance(a, C.c_void_p) else a for a in args[n_scalars:]]
        self.calls.append((args[:n_scalars], bufs[0].copy(), bufs[1:]))
        for b in bufs[1:]:
            if isinstance(b, np.ndarray):
                b[...] = MARK
        if self.spec.style == "squelch":
            bufs[2][...] = args[0]                  # every stream produced all of its items
        return args[0]


def _block(g, monkeypatch, spec, streams):
    blk = object.__new__(getattr(g.binding, spec.cls))
    blk._h, blk._streams = C.c_void_p(0), streams
    for k, v in spec.attrs.items():
        setattr(blk, k, v)
    blk._call = Recorder(g.binding, monkeypatch, spec, streams)
    return blk


def _items(spec, count):
    """`count` input items with negative values among them, in the dtype the caller would hold them in"""
    v = (np.arange(count) % 5 - 2).astype(np.int8 if spec.views else np.int64)
    if spec.views or np.dtype(spec.in_dtype).kind in "iu":
        return v if spec.views else v + 2
    return v.astype(spec.in_dtype)


def _run(spec, blk, x, n):
    """call the block's host entry; n None: leave the count to it (general_work takes (noutput_items, ninput_items or
    None)).  Returns the list of arrays it handed back."""
    kw = {spec.flag: True} if spec.want else {}
    if spec.style == "count":
        return [blk.work(n, x)]
    if spec.style == "general":
        out, consumed = blk.general_work(n[0], x) if n[1] is None else blk.general_work(n[0], x, n[1])
        assert consumed == 0
        return [out]
    res = blk.work(x, **kw) if n is None else blk.work(x, n, **kw)
    if spec.style == "squelch":
        return [res] if blk._streams == 1 else res
    return list(res) if spec.want else [res]


@pytest.mark.parametrize("n", [0, 1, 5])
@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_work_buffers_and_returns(g, monkeypatch, spec, streams, n):
    need, m = streams * n * spec.per_in, streams * n * spec.per_out
    x = _items(spec, need)
    for explicit in (False, True):
        if spec.style == "count" and not explicit:
            continue                                # the count comes first and has no default
        blk = _block(g, monkeypatch, spec, streams)
        given = np.concatenate([x, x[:2]]) if explicit else x      # an explicit count may leave items unused
        count = (n, n if explicit else None) if spec.style == "general" else (n if explicit else None)
        got = _run(spec, blk, given, count)
        (scalars, x_seen, bufs), = blk._call.calls                  # one C call per work
        assert scalars == ((n, n) if spec.style == "general" else (n,))
        # the input reaches C as its own bytes (viewing blocks) or as the cast to the declared dtype
        want_in = given.view(np.uint8) if spec.views else given.astype(spec.in_dtype)
        assert x_seen.dtype == want_in.dtype and x_seen.tobytes() == want_in.tobytes()
        # the outputs: valid buffers even for no items, the optional ones only where asked for
        if spec.style == "squelch":
            out, produced = bufs
            assert out.dtype == spec.out_dtype and out.size >= max(m, 1)
            assert produced.dtype == np.int32 and produced.size == streams
            assert len(got) == streams
            for a in got:
                assert a.dtype == spec.out_dtype and len(a) == n and np.all(a == MARK)
            continue
        if spec.style == "general":
            bufs = bufs[:1]                         # the consumed count follows the output
        assert len(bufs) == 1 + spec.optional
        if not spec.want:
            assert all(b is None for b in bufs[1:])                 # null pointers
            bufs = bufs[:1]
        dtypes = [spec.out_dtype] + [np.float32] * (len(bufs) - 1)
        for b, d in zip(bufs, dtypes):
            assert isinstance(b, np.ndarray) and b.dtype == d and b.size >= max(m, 1)
        assert len(got) == len(bufs)
        for a, d in zip(got, dtypes):
            assert isinstance(a, np.ndarray) and a.dtype == d and a.shape == (m,) and np.all(a == MARK)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_short_input_is_refused_before_c(g, monkeypatch, spec, streams, n):
    need = streams * n * spec.per_in
    blk = _block(g, monkeypatch, spec, streams)
    x = _items(spec, need - 1)
    with pytest.raises(ValueError) as e:
        _run(spec, blk, x, (n, n) if spec.style == "general" else n)
    assert str(need) in str(e.value).split() and str(need - 1) in str(e.value).split()
    assert blk._call.calls == []


def test_a_count_left_out_is_the_whole_steps_the_input_holds(g, monkeypatch):
    spec = [s for s in SPECS if s.cls == "trellis_metrics_c"][0]
    blk = _block(g, monkeypatch, spec, 3)
    out = blk.work(_items(spec, 3 * 2 * 5 + 5))                     # five items short of a sixth step
    assert blk._call.calls[0][0] == (5,) and out.shape == (3 * 5 * 4,)


def test_stream_value_keeps_each_getters_type(g):
    seen = []

    def call(name, stream, ref):
        seen.append((name, stream))
        ref._obj.value = 3
        return 0

    for cls, getter, kind in (("costas_loop_cc", "get_frequency", np.float32), ("agc_ff", "gain", np.float32),
                              ("pll_carriertracking_cc", "locksig", np.float32), ("pll_carriertracking_cc", "lock_detector", bool),
                              ("pfb_clock_sync_ccf", "k", np.float32), ("pfb_clock_sync_ccf", "slips", int),
                              ("pfb_clock_sync_ccf", "position", int), ("frequency_modulator_fc", "phase", float),
                              ("gmskmod_bc", "phase", float), ("trellis_encoder_bi", "ST", int)):
        blk = object.__new__(getattr(g.binding, cls))
        blk._h, blk._streams, blk._call = C.c_void_p(0), 3, call
        v = getattr(blk, getter)(2)
        assert type(v) is kind and v == kind(3) and seen[-1] == (getter, 2)


# ---- the source itself: the contract is written once ----
def _functions(g):
    tree = ast.parse(open(g.binding.__file__).read())
    return [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]


def test_the_count_is_inferred_in_one_function(g):
    def infers(fn):
        for e in ast.walk(fn):
            if isinstance(e, ast.BinOp) and isinstance(e.op, ast.FloorDiv) and isinstance(e.left, ast.Call) \
                    and getattr(e.left.func, "id", None) == "len" \
                    and any(isinstance(a, ast.Attribute) and a.attr == "_streams" for a in ast.walk(e.right)):
                return True
        return False

    assert [f.name for f in _functions(g) if infers(f)] == ["_work_in"]


def test_one_wording_of_the_short_input_error_and_no_family_helpers(g):
    fns = _functions(g)
    holders = [f.name for f in fns
               if any(isinstance(e, ast.Constant) and e.value == "work needs %d items, got %d" for e in ast.walk(f))]
    assert holders == ["_work_in"]
    defs = [f.name for f in fns]
    assert "_items" not in defs and "_stream_float" not in defs
    assert defs.count("_stream_value") == 1 and defs.count("_work_in") == 1 and defs.count("_work_out") == 1
