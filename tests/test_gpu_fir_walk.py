"""-m gpu tests of the persistent tile WALK of the four FIR kernels on the vector pipes -- fir_tiled_kernel
(csrc/fir_tiled.hip), fir_hidec_kernel and fir_generic_tiled_kernel (csrc/fir_kernels.hip), fir_realin_kernel
(csrc/fir_realin.hip): launches sized from the device's CU count so that every persistent workgroup takes at least
three tiles and one a fourth, on every route that reaches one of them.  What crosses a loop trip is exercised there
and nowhere else in the suite: the next tile's samples prefetched into registers under the MAC loop, its rotator phases
fetched a tile early, the out-of-range offsets of a tile past the end of the launch, the tiled kernel's two static tiles
and then its tile queue (ticket, hand-over through LDS, re-arming by the last workgroup out), the pre-mix phasors rebuilt
at a change of alignment parity, the demodulator's carry taken by tile 0 and left by a tile late in the walk.

WALK_CASES is the one table of cases; tests/test_fir_walk_shapes_cpu.py checks it against the tile constants in the
sources and host/fir_plan_test.cc pins every row's engine ("walk <id>" in its ROWS), both without a GPU.

Out of scope: fir_generic_win_kernel (bit-exact mode at decimation 1 / 2 / 4) launches one workgroup per tile and
strides only beyond 2^20 tiles (a billion outputs)."""
import collections

import numpy as np
import pytest

import realin_ref as rr
from conftest import bits_equal, demod_close

pytestmark = pytest.mark.gpu
TOL = 1e-5
TAIL = 91                       # outputs missing from the last tile
GUARD = 64                      # output items behind n_out that must stay untouched
SENTINEL = 0x7FC0DEAD           # a quiet NaN no kernel produces
SECOND_CALL = 100               # demodulating single-stream cases: outputs of the call that follows the long one
# a centre frequency whose rotator phase does not repeat at any tile period (CFG2's 1.25 MHz of 10 MHz advances the
# phase by pi per output at decimation 4: tile t + 1's phases would equal tile t's)
CENTER, FS = 1.2345e6, 10e6

# kernel: tiled / hidec / realin / gtiled (the launcher whose grid rule applies)
# block:  fir (fir_filter_<kind>), xlating (freq_xlating_fir_filter_<kind>), demod (xlating_demod.work_device),
#         captures (xlating_demod.run_captures_device, 3 captures; stride: even / odd items between captures)
# proto:  xlating / demod / captures: "real" or "complex" prototype taps
# engine / epilogue: what host/fir_plan_test.cc pins for the row
# per_tile: new output items per tile; wg_per_cu: the largest grid the launcher can choose, in workgroups per CU
# queue: tiled kernel only -- the tile queue is on (Tq * decimation >= 128, launch_fir_tiled)
Case = collections.namedtuple("Case", "id kernel block kind proto ntaps decim mode engine epilogue per_tile wg_per_cu queue stride")


def _c(id, kernel, block, kind, proto, ntaps, decim, mode, engine, epilogue, per_tile, wg_per_cu, queue=False, stride=None):
    return Case(id, kernel, block, kind, proto, ntaps, decim, mode, engine, epilogue, per_tile, wg_per_cu, queue, stride)


WALK_CASES = [
    # ---- fir_tiled_kernel, static split.  Grid: tiled_wg_per_cu() x CUs (launch_tiled_inst, fir_tiled.hip): 2 per CU
    # (TILED_WG_PER_CU), 4 for a plain decimation-1 filter; tiles of TILED_NT = 2048 outputs
    _c("tiled-ccf-32/1", "tiled", "fir", "ccf", None, 32, 1, "FAST", "tiled", "none", 2048, 4),
    _c("tiled-ccc-80/2", "tiled", "fir", "ccc", None, 80, 2, "FAST", "tiled", "none", 2048, 2),
    _c("tiled-ccf-92/4", "tiled", "fir", "ccf", None, 92, 4, "FAST", "tiled", "none", 2048, 2),     # 23 taps per phase: under the matrix cores' 24
    # ---- queue on
    _c("tiled-ccc-104/4", "tiled", "fir", "ccc", None, 104, 4, "FAST", "tiled", "none", 2048, 2, True),
    _c("tiled-ccf-120/2", "tiled", "fir", "ccf", None, 120, 2, "FAST_VALU", "tiled", "none", 2048, 2, True),
    _c("tiled-ccf-112/4", "tiled", "fir", "ccf", None, 112, 4, "FAST_VALU", "tiled", "none", 2048, 2, True),
    # (float data: the kernel runs at twice the decimation on overlapped pairs, a tile is 2048 pairs = 4096 floats)
    _c("tiled-fff-128/1", "tiled", "fir", "fff", None, 128, 1, "FAST", "tiled", "none", 4096, 2, True),
    _c("tiled-fff-176/2", "tiled", "fir", "fff", None, 176, 2, "FAST", "tiled", "none", 4096, 2, True),
    # ---- epilogues
    _c("tiled-xlating-real-256/4", "tiled", "xlating", "ccc", "real", 256, 4, "FAST_VALU", "tiled", "rotate", 2048, 2, True),
    _c("tiled-xlating-complex-200/4", "tiled", "xlating", "ccc", "complex", 200, 4, "FAST", "tiled", "rotate", 2048, 2, True),
    # (fused demodulator: lane 0 of every wave overlaps, 2048 - 4 x 8 new outputs per tile)
    _c("tiled-demod-256/4", "tiled", "demod", None, "real", 256, 4, "FAST_VALU", "tiled", "demod", 2016, 2, True),
    # ---- batched: tile ids run over (tile, capture) pairs
    _c("tiled-captures-even", "tiled", "captures", None, "real", 256, 4, "FAST_VALU", "tiled", "demod", 2016, 2, True, "even"),
    _c("tiled-captures-odd", "tiled", "captures", None, "real", 256, 4, "FAST", "tiled", "demod", 2016, 2, True, "odd"),
    # ---- fir_hidec_kernel.  Grid: up to 3 per CU (launch_fir_hidec / launch_fir_hidec_demod: per_cu by LDS size); tiles of
    # 2 * (256 / G) outputs, G = hidec_groups(); the demodulating form overlaps one output pair
    _c("hidec-ccf-64/8", "hidec", "fir", "ccf", None, 64, 8, "FAST", "hidec", "none", 512, 3),
    _c("hidec-ccc-128/64", "hidec", "fir", "ccc", None, 128, 64, "FAST", "hidec", "none", 84, 3),   # G = 6: lanes 252..255 idle
    _c("hidec-xlating-real-64/8", "hidec", "xlating", "ccc", "real", 64, 8, "FAST", "hidec", "rotate", 512, 3),
    # (96/3 with a complex prototype is 64 MACs per input sample: the overlap-save engine.  48/3 is the longest complex
    # prototype at decimation 3 that stays on this kernel; 96/3 with a real prototype adds the pre-mix form + rotate)
    _c("hidec-xlating-complex-48/3", "hidec", "xlating", "ccc", "complex", 48, 3, "FAST", "hidec", "rotate", 512, 3),
    _c("hidec-xlating-real-96/3", "hidec", "xlating", "ccc", "real", 96, 3, "FAST", "hidec", "rotate", 512, 3),
    _c("hidec-demod-64/8", "hidec", "demod", None, "real", 64, 8, "FAST", "hidec", "demod", 510, 3),
    _c("hidec-captures-200/5", "hidec", "captures", None, "real", 200, 5, "FAST", "hidec", "demod", 510, 3, False, "odd"),
    # ---- fir_realin_kernel.  Grid: 2 per CU (launch_realin_inst: per_cu), tiles of RI_T * RI_R = 2048 outputs
    _c("realin-fcc-64/8", "realin", "fir", "fcc", None, 64, 8, "FAST", "realin", "none", 2048, 2),
    _c("realin-scc-64/4", "realin", "fir", "scc", None, 64, 4, "FAST", "realin", "none", 2048, 2),
    _c("realin-xlating-fcf-64/4", "realin", "xlating", "fcf", "real", 64, 4, "FAST", "realin", "rotate", 2048, 2),   # the ROT instantiation
    # ---- fir_generic_tiled_kernel (bit-exact mode, decimations other than 1 / 2 / 4).  Grid: min(8, 160 KiB / (LDS + 512))
    # per CU (launch_generic_tiled: per_cu) -- the tile of 64/16 fills LDS (1 per CU), that of 33/3 fits 6 times; tiles of
    # GT_R * GT_T = 1024 outputs
    _c("gtiled-ccf-64/16", "gtiled", "fir", "ccf", None, 64, 16, "GENERIC", "generic", "none", 1024, 1),
    _c("gtiled-ccc-33/3", "gtiled", "fir", "ccc", None, 33, 3, "GENERIC", "generic", "none", 1024, 6),
]
CAPTURES = 3


def walk_tiles(case, cus):
    """tiles of the long launch (all captures together): three for every workgroup of the largest grid, and one more"""
    return 3 * case.wg_per_cu * cus + 1


def walk_sizes(case, cus):
    """(streams, tiles per stream, outputs per stream, input items per stream) of the long launch: per stream
    n_out = tiles * per_tile - TAIL, the last tile partial (a tile smaller than TAIL: as many tiles more as TAIL takes away)"""
    streams = CAPTURES if case.block == "captures" else 1
    tps = -(-walk_tiles(case, cus) // streams)
    n_out = (tps + TAIL // case.per_tile) * case.per_tile - TAIL
    extra = SECOND_CALL if case.block == "demod" else 0
    n_in = (n_out + extra) * case.decim + case.ntaps - 1
    return streams, tps, n_out, n_in


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rand_c(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)


def _sentinel_tensor(shape, dev):
    import torch
    t = torch.full(shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    torch.cuda.current_stream(dev).synchronize()       # the fill is done before a launch on another stream can write
    return t


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _per_tile_report(case, got, ref, taps, cus, n_tiles_launch):
    """|got - ref| <= TOL * max(|ref|_inf of the tile, 1e-3 * sum|h|) for every tile; returns (worst error / bound,
    text naming the first bad tiles: index, tile % grid and the visit number of the workgroup that took it)"""
    pt = case.per_tile
    n = len(ref)
    tiles = -(-n // pt)
    pad = tiles * pt - n
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.complex128 if np.iscomplexobj(ref) else np.float64) - ref)
    err = np.concatenate([err, np.zeros(pad)]).reshape(tiles, pt)
    mag = np.concatenate([np.abs(ref), np.zeros(pad)]).reshape(tiles, pt).max(axis=1)
    bound = TOL * np.maximum(mag, 1e-3 * float(np.abs(taps).sum()))
    with np.errstate(invalid="ignore"):
        terr = np.where(np.isnan(err).any(axis=1), np.inf, err.max(axis=1))
    bad = np.nonzero(~(terr <= bound))[0]
    grid = min(case.wg_per_cu * cus, n_tiles_launch)
    lines = []
    for t in bad[:12]:
        visit = "%d" % (t // grid) if not case.queue or t < 2 * grid else "queue (>= 2)"
        lines.append("tile %d (tile %% grid %d, visit %s): error %.3g, bound %.3g" % (t, t % grid, visit, terr[t], bound[t]))
    text = "%d of %d tiles off (grid taken as %d):\n  %s" % (len(bad), tiles, grid, "\n  ".join(lines))
    return float((terr / bound).max()), text


def _make(gpu, po, wl, case, n_in):
    """(block, input items as the device entry reads them, taps for the error floor, reference function of n_out)"""
    rng = np.random.default_rng(sum(map(ord, case.id)))
    mode = getattr(gpu, "MODE_" + case.mode)
    T, D = case.ntaps, case.decim
    if case.block == "fir":
        cplx_taps = case.kind in ("ccc", "fcc", "scc")
        taps = _rand_c(rng, T) if cplx_taps else rng.uniform(-1, 1, T).astype(np.float32)
        if case.kind == "fff":
            x = rng.uniform(-1, 1, n_in).astype(np.float32)
            ref = lambda n: po.fir_fff(taps, x, n, D)
        elif case.kind == "fcc":
            x = rng.uniform(-1, 1, n_in).astype(np.float32)
            ref = lambda n: rr.fcc_ref(po, taps, x, n, D)
        elif case.kind == "scc":
            x = rng.integers(-32768, 32768, n_in).astype(np.int16)
            ref = lambda n: rr.fcc_ref(po, taps, x, n, D)
        else:
            x = _rand_c(rng, n_in)
            ref = lambda n: (po.fir_ccc if cplx_taps else po.fir_ccf)(taps, x, n, D)
        blk = getattr(gpu, "fir_filter_" + case.kind)(D, taps)
        blk.set_mode(mode)
        scale = 32768.0 if case.kind == "scc" else 1.0
        return blk, x, taps * scale, ref
    # prototypes of the translating blocks: a low-pass (the pre-mix forms keep the exact tap angles, the reference
    # rounds them to float: random taps at the filter's ends would measure that, not the walk)
    proto = wl.cfg2_proto_taps() if T == 256 else wl.lowpass_taps(T, 200e3, FS).astype(np.complex64)
    if case.proto == "complex":
        proto = (proto * np.exp(1j * 0.013 * np.arange(T))).astype(np.complex64)
    if case.block == "xlating":
        if case.kind == "fcf":
            x = rng.uniform(-1, 1, n_in).astype(np.float32)
            blk = gpu.freq_xlating_fir_filter_fcf(D, proto.real.astype(np.float32), CENTER, FS)
            ref = lambda n: rr.XlatingRef(po, D, proto, CENTER, FS).work(x, n)
        else:
            x = _rand_c(rng, n_in)
            blk = gpu.freq_xlating_fir_filter_ccc(D, proto, CENTER, FS)
            ref = lambda n: po.Xlating(D, proto, CENTER, FS).work(x, n)
        blk.set_mode(mode)
        return blk, x, proto, ref
    raise AssertionError(case.block)


def _single_stream(gpu, po, wl, case):
    """fir / xlating rows: one stream through work_device"""
    import torch
    cus = _cus()
    _streams, tiles, n_out, n_in = walk_sizes(case, cus)
    assert tiles >= 3 * case.wg_per_cu * cus + 1
    blk, x, taps, ref_of = _make(gpu, po, wl, case, n_in)
    ref = ref_of(n_out)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    d_in = torch.from_numpy(x).to(dev)
    out_f32 = 1 if ref.dtype == np.float32 else 2
    np_out = np.float32 if out_f32 == 1 else np.complex64

    def launch(n):
        d_out = _sentinel_tensor((n + GUARD, out_f32), dev)
        if hasattr(blk, "reset"):
            blk.reset()                                            # the rotator starts over: launches are comparable
        assert blk.work_device(n, d_in, d_out, st) == n
        st.synchronize()
        raw = d_out.cpu().numpy()
        assert (_words(raw[n:]) == SENTINEL).all(), "%s: wrote behind n_out = %d" % (case.id, n)
        got = raw[:n].reshape(-1).view(np_out)
        inside = np.nonzero((_words(raw[:n]) == SENTINEL).reshape(n, -1).any(axis=1))[0]
        assert len(inside) == 0, "%s: %d outputs never written, first %d = tile %d, last %d = tile %d" % (
            case.id, len(inside), inside[0], inside[0] // case.per_tile, inside[-1], inside[-1] // case.per_tile)
        return got

    def check(got, n, n_tiles):
        if case.mode == "GENERIC":
            if not bits_equal(got, ref[:n]):
                first = int(np.nonzero(_words(got).reshape(n, -1) != _words(ref[:n]).reshape(n, -1))[0][0])
                raise AssertionError("%s: not bit-exact from output %d = tile %d" % (case.id, first, first // case.per_tile))
            return 0.0
        worst, text = _per_tile_report(case, got, ref[:n], taps, cus, n_tiles)
        print("walk %s: %d tiles, worst per-tile error / bound %.3g" % (case.id, n_tiles, worst))
        assert worst <= 1.0, case.id + ": " + text
        return worst

    got = launch(n_out)
    check(got, n_out, tiles)
    again = launch(n_out)                                          # the queue re-armed itself
    assert bits_equal(again, got), case.id + ": second launch differs"
    short_tiles = max(1, cus // 2)                                 # a grid below the cap: the re-arm compares against another G
    n_short = max(short_tiles * case.per_tile - TAIL, case.per_tile // 2)
    check(launch(n_short), n_short, short_tiles)
    assert bits_equal(launch(n_out), got), case.id + ": long launch after a short one differs"


def _demod_taps(wl, case):
    return wl.cfg2_proto_taps() if case.ntaps == 256 else wl.lowpass_taps(case.ntaps, 100e3, FS).astype(np.complex64)


def _demod_stream(gpu, po, wl, case):
    """xlating_demod.work_device: the long call, then a call of SECOND_CALL outputs; the carry y_last comes from a tile
    late in the walk and goes into tile 0 of the second call"""
    import torch
    c = wl.CFG2
    cus = _cus()
    _streams, tiles, n_out, _n_in = walk_sizes(case, cus)
    D, T, gain = case.decim, case.ntaps, c["demod_gain"]
    n_all = n_out + SECOND_CALL
    x = wl.fsk4_capture(n_all * D, stream_id=sum(map(ord, case.id)) % 1000)
    proto = _demod_taps(wl, case)
    ref = po.chain_xlating_demod(D, proto, c["center_freq"], c["fs"], gain, x)
    xin = wl.with_history(x, T - 1)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    d_in = torch.from_numpy(xin.view(np.float32).reshape(-1, 2)).to(dev)
    blk = gpu.xlating_demod(D, proto, c["center_freq"], c["fs"], gain)
    blk.set_mode(getattr(gpu, "MODE_" + case.mode))

    def launch(n, first=0, reset=True):
        d_out = _sentinel_tensor((n + GUARD,), dev)
        if reset:
            blk.reset()
        assert blk.work_device(n, d_in[first * D:], d_out, st) == n
        st.synchronize()
        raw = d_out.cpu().numpy()
        assert (_words(raw[n:]) == SENTINEL).all(), "%s: wrote behind n_out = %d" % (case.id, n)
        inside = np.nonzero(_words(raw[:n]) == SENTINEL)[0]
        assert len(inside) == 0, "%s: %d outputs never written, first %d = tile %d, last %d = tile %d" % (
            case.id, len(inside), inside[0], inside[0] // case.per_tile, inside[-1], inside[-1] // case.per_tile)
        return raw[:n].copy()

    got = launch(n_out)
    tail = launch(SECOND_CALL, first=n_out, reset=False)
    ok, worst = demod_close(np.concatenate([got, tail]), ref, gain=gain)
    print("walk %s: %d tiles, demod_close worst %.3g of the output range" % (case.id, tiles, worst))
    assert ok, (case.id, worst, _first_bad_tile(case, np.concatenate([got, tail]), ref))
    assert bits_equal(launch(n_out), got), case.id + ": second launch differs"
    short_tiles = max(1, cus // 2)
    n_short = short_tiles * case.per_tile - TAIL
    ok, worst = demod_close(launch(n_short), ref[:n_short], gain=gain)
    assert ok, (case.id, "short launch", worst)
    assert bits_equal(launch(n_out), got), case.id + ": long launch after a short one differs"


def _first_bad_tile(case, got, ref):
    with np.errstate(invalid="ignore"):
        bad = np.nonzero(~(np.abs(got - ref) <= TOL * np.abs(ref).max()))[0]
    bad = bad[bad >= 64]
    return None if len(bad) == 0 else "first output off: %d = tile %d; %d off" % (bad[0], bad[0] // case.per_tile, len(bad))


def _demod_captures(gpu, po, wl, case):
    """xlating_demod.run_captures_device over CAPTURES captures: 3 x tiles-per-capture meets the bound"""
    import torch
    c = wl.CFG2
    cus = _cus()
    S, tpc, n_out, _n_in = walk_sizes(case, cus)
    assert S * tpc >= 3 * case.wg_per_cu * cus + 1
    D, gain = case.decim, c["demod_gain"]
    n = n_out * D
    xs = [wl.fsk4_capture(n, stream_id=sum(map(ord, case.id)) % 1000 + s) for s in range(S)]
    proto = _demod_taps(wl, case)
    refs = [po.chain_xlating_demod(D, proto, c["center_freq"], c["fs"], gain, xs[s]) for s in range(S)]
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    stride = n + 64
    stride += (stride & 1) ^ (1 if case.stride == "odd" else 0)
    assert (stride & 1) == (case.stride == "odd")
    d_in = torch.zeros((S * stride + 8, 2), dtype=torch.float32, device=dev)
    for s in range(S):
        d_in[s * stride: s * stride + n] = torch.from_numpy(xs[s].view(np.float32).reshape(-1, 2))
    ostride = ((n_out + GUARD + 3) // 4) * 4
    blk = gpu.xlating_demod(D, proto, c["center_freq"], c["fs"], gain)
    blk.set_mode(getattr(gpu, "MODE_" + case.mode))

    def launch(n_samples):
        m = n_samples // D
        d_out = _sentinel_tensor((S, ostride), dev)
        blk.run_captures_device(S, n_samples, d_in, stride, d_out, ostride, st)
        st.synchronize()
        raw = d_out.cpu().numpy()
        for s in range(S):
            assert (_words(raw[s, m:]) == SENTINEL).all(), "%s: capture %d wrote behind n_out = %d" % (case.id, s, m)
            inside = np.nonzero(_words(raw[s, :m]) == SENTINEL)[0]
            assert len(inside) == 0, "%s: capture %d, %d outputs never written, first %d = tile %d, last %d = tile %d" % (
                case.id, s, len(inside), inside[0], inside[0] // case.per_tile, inside[-1], inside[-1] // case.per_tile)
        return raw[:, :m].copy()

    def check(got, m, what):
        worst_all = 0.0
        for s in range(S):
            ok, worst = demod_close(got[s], refs[s][:m], gain=gain)
            assert ok, (case.id, what, s, worst, _first_bad_tile(case, got[s], refs[s][:m]))
            worst_all = max(worst_all, worst)
        return worst_all

    got = launch(n)
    print("walk %s: %d tiles, demod_close worst %.3g of the output range" % (case.id, S * tpc, check(got, n_out, "long launch")))
    assert bits_equal(launch(n), got), case.id + ": second launch differs"
    short_tpc = max(1, cus // 2 // S)
    m = short_tpc * case.per_tile - TAIL
    check(launch(m * D), m, "short launch")
    assert bits_equal(launch(n), got), case.id + ": long launch after a short one differs"


@pytest.mark.parametrize("case", WALK_CASES, ids=[k.id for k in WALK_CASES])
def test_every_workgroup_walks_three_tiles(gpu, po, wl, case):
    """One row of WALK_CASES.  The output is pre-filled with a NaN sentinel: none may remain inside [0, n_out), all must
    remain in the guard behind it.  Against the CPU oracle of the same operation: FAST routes per tile, |got - ref| <=
    1e-5 * max(|ref|_inf of the tile, 1e-3 * sum|h|), a failure naming tile, tile % grid and visit; demodulating routes
    demod_close (the single-stream ones over the long call plus a second call of 100 outputs: the carry); GENERIC routes
    bit for bit.  Then on the same handle and stream: the same launch again (bit-identical: the queue re-armed itself),
    a launch of CUs // 2 tiles (a smaller grid) against the oracle, and the long launch once more (bit-identical)."""
    if case.block == "demod":
        _demod_stream(gpu, po, wl, case)
    elif case.block == "captures":
        _demod_captures(gpu, po, wl, case)
    else:
        _single_stream(gpu, po, wl, case)
