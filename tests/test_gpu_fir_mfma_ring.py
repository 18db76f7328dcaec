"""-m gpu tests of the matrix-core FIR engine's tile LOOP (csrc/fir_mfma.hip): launches in which every persistent
workgroup walks at least three tiles, so that what crosses a loop trip is exercised -- the next tile's loads requested
from the first chunk steps of the matrix phase, its block-floating-point maxima taken at the end of the tile before
(between the last demodulator and the output stores), the operand ring, the tile queue.  (The every-block test of
test_gpu_fir_mfma.py has fewer tiles than workgroups: no workgroup takes a second one there.)"""
import numpy as np
import pytest

from conftest import demod_close, rel_err_max

pytestmark = pytest.mark.gpu
TOL = 1e-5
NTE = 1984                      # new outputs per tile (mfma_tables.h)
WGS_PER_CU = 2                  # persistent workgroups per CU
CAPTURES = 7


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _tiles_per_capture():
    # 7 captures x (ceil(3 * 2 * CUs / 7) + 1) tiles: at least three tiles for every one of the 2 * CUs workgroups
    return -(-3 * WGS_PER_CU * _cus() // CAPTURES) + 1


def _rand_c(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)


def _per_element(got, ref, floor=0.1):
    big = np.abs(ref) > floor * np.abs(ref).max()
    return float((np.abs(got[big] - ref[big]) / np.abs(ref[big])).max())


def test_captures_three_tiles_per_workgroup(gpu, po, wl):
    """7 captures of (ceil(6 CUs / 7) + 1) tiles minus 91 outputs (the last tile of every capture is partial) in one
    launch against the oracle per capture; nothing written behind a capture's outputs; a second launch on the same
    handle (the queue re-arms itself) bit-identical"""
    import torch
    c = wl.CFG2
    decim = c["decim"]
    nout = _tiles_per_capture() * NTE - 91
    n = nout * decim
    S = CAPTURES
    assert S * _tiles_per_capture() >= 3 * WGS_PER_CU * _cus()
    proto = wl.cfg2_proto_taps()
    xs = [wl.fsk4_capture(n, stream_id=40 + s) for s in range(S)]
    dev = torch.device("cuda", 0)
    row = ((n + 63) // 64) * 64
    orow = ((nout + 63) // 64) * 64 + 64
    d_in = torch.zeros((S, row, 2), dtype=torch.float32, device=dev)
    for s in range(S):
        d_in[s, :n] = torch.from_numpy(xs[s].view(np.float32).reshape(-1, 2))
    d_out = torch.zeros((S, orow), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    blk = gpu.xlating_demod(decim, proto, c["center_freq"], c["fs"], c["demod_gain"])
    blk.run_captures_device(S, n, d_in, row, d_out, orow, st)
    st.synchronize()
    got = d_out.cpu().numpy()
    for s in range(S):
        ref = po.chain_xlating_demod(decim, proto, c["center_freq"], c["fs"], c["demod_gain"], xs[s])
        ok, worst = demod_close(got[s, :nout], ref, gain=c["demod_gain"])
        assert ok, (s, worst)
        assert not got[s, nout:].any(), s                           # nothing beyond nout
    d_out.zero_()
    blk.run_captures_device(S, n, d_in, row, d_out, orow, st)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), got.view(np.uint32))


@pytest.fixture(scope="module")
def long_stream(wl):
    """one stream as long as the seven captures together: every workgroup walks three tiles of it"""
    nout = CAPTURES * _tiles_per_capture() * NTE - 91
    x = wl.fsk4_capture(nout * 4, stream_id=47)
    proto = wl.cfg2_proto_taps()
    return nout, x, proto, wl.with_history(x, len(proto) - 1)


def test_one_stream_no_epilogue(gpu, po, long_stream):
    nout, _x, proto, xin = long_stream
    taps = proto.real.astype(np.float32)
    ref = po.fir_ccf(taps, xin, nout, 4)
    got = gpu.fir_filter_ccf(4, taps).work(nout, xin)
    bad = np.nonzero(np.abs(got - ref) > TOL * np.abs(ref).max())[0]
    assert len(bad) == 0, (len(bad), bad[:20])


def test_one_stream_rotate_epilogue(gpu, po, wl, long_stream):
    c = wl.CFG2
    nout, _x, proto, xin = long_stream
    ref = po.Xlating(4, proto, c["center_freq"], c["fs"]).work(xin, nout)
    got = gpu.freq_xlating_fir_filter_ccc(4, proto, c["center_freq"], c["fs"]).work(nout, xin)
    bad = np.nonzero(np.abs(got - ref) > TOL * np.abs(ref).max())[0]
    assert len(bad) == 0, (len(bad), bad[:20])


def test_one_stream_reference_taps_demod(gpu, po, wl, long_stream):
    c = wl.CFG2
    nout, x, proto, xin = long_stream
    ref = po.chain_xlating_demod(4, proto, c["center_freq"], c["fs"], c["demod_gain"], x)
    blk = gpu.xlating_demod(4, proto, c["center_freq"], c["fs"], c["demod_gain"])
    blk.set_mode(gpu.MODE_FAST_REFTAPS)
    got = blk.work(nout, xin)
    ok, worst = demod_close(got, ref, gain=c["demod_gain"])
    assert ok, worst


def test_one_stream_decimation_two_short_band(gpu, po):
    """D = 2 with 130 taps: the six-k-step instantiation at decimation 2 (one chunk between block starts: every chunk
    but the first and last three feeds all four blocks; nine loads over nine chunk steps)"""
    rng = np.random.default_rng(130)
    ntaps, decim = 130, 2
    nout = CAPTURES * _tiles_per_capture() * NTE - 91
    x = _rand_c(rng, nout * decim + ntaps - 1)
    taps = rng.uniform(-1, 1, ntaps).astype(np.float32)
    ref = po.fir_ccf(taps, x, nout, decim)
    got = gpu.fir_filter_ccf(decim, taps).work(nout, x)
    bad = np.nonzero(np.abs(got - ref) > TOL * np.abs(ref).max())[0]
    assert len(bad) == 0, (len(bad), bad[:20])


# ---- the maxima of a workgroup's SECOND tile: they are taken at the end of its first one ----
NTAPS, DECIM = 256, 4
TILE_IN = 8256                  # samples staged per tile (mfma_tables.h: tile_samples(4, 10))


def _second_tile_of_workgroup_0():
    """first and last input sample (index into the history-prefixed stream) of tile 2 * CUs: the second tile of
    workgroup 0 of a one-stream launch (tiles b, b + grid, then the queue); the tile starts one 16-output block early"""
    tile = WGS_PER_CU * _cus()
    first = (tile * NTE - 16) * DECIM
    return tile, first, first + TILE_IN - 1


@pytest.fixture(scope="module")
def second_tile_case(po):
    tile, first, last = _second_tile_of_workgroup_0()
    rng = np.random.default_rng(2 * tile + 1)
    n = (tile + 3) * NTE - 91
    nin = n * DECIM + NTAPS - 1
    x = _rand_c(rng, nin)
    taps = (rng.uniform(-1, 1, NTAPS) / 16).astype(np.float32)
    clean = po.fir_ccf(taps, x, n, DECIM)
    return n, x, taps, clean, first, last


@pytest.mark.parametrize("edge", ["first", "last"])
def test_amplitude_step_at_the_ends_of_a_second_tile(gpu, po, second_tile_case, edge):
    """a 60 dB step at the first / at the last sample of a workgroup's second tile: with `first` the tile is loud and
    the one before it (same stretch of the stream, another workgroup) quiet; with `last` one loud sample, the last one
    loaded, sets the tile's scale.  A scale taken from the wrong tile shows exactly here.  Bounds: those of
    test_amplitude_step_inside_a_tile."""
    n, x0, taps, _clean, first, last = second_tile_case
    where = first if edge == "first" else last
    x = x0.copy()
    x[:where] *= np.float32(1e-3)                      # quiet, then loud
    ref = po.fir_ccf(taps, x, n, DECIM)
    got = gpu.fir_filter_ccf(DECIM, taps).work(n, x)
    assert rel_err_max(got, ref) <= TOL
    quiet = np.arange(n) < (where - NTAPS) // DECIM - 1           # outputs whose whole window is quiet
    assert quiet.sum() > 100
    bound = 2.0 ** -21 * np.abs(taps).sum() * np.abs(x).max()     # grhip.h: FAST-mode error of this engine
    assert np.abs(got[quiet] - ref[quiet]).max() <= bound
    loud = np.arange(n) > where // DECIM + 1
    assert _per_element(got[loud], ref[loud]) <= TOL


@pytest.mark.parametrize("edge", ["first", "last"])
def test_one_inf_at_the_ends_of_a_second_tile(gpu, second_tile_case, edge):
    """one Inf there, as in test_one_non_finite_sample_stays_local: the scale of the tile comes from its finite samples"""
    n, x0, taps, clean, first, last = second_tile_case
    pos = first if edge == "first" else last
    x = x0.copy()
    x[pos] = np.complex64(complex(np.inf, 1.0))
    got = gpu.fir_filter_ccf(DECIM, taps).work(n, x)
    idx = np.arange(n)
    lo, hi = (pos - NTAPS + 1 + DECIM - 1) // DECIM, pos // DECIM      # outputs whose window holds the sample
    far = (idx < lo - 32) | (idx > hi + 32)
    assert np.isfinite(got[far]).all()
    assert np.abs(got[far] - clean[far]).max() <= TOL * np.abs(clean).max()
    hit = (idx >= max(lo, 0)) & (idx <= min(hi, n - 1))
    assert hit.any() and not np.isfinite(got[hit]).any()                # as in the reference
