"""scrambler_bb, descrambler_bb and additive_scrambler_bb on the device, bit for bit against tests/golden/ref_packet.npz
(recorded from gri_lfsr.h compiled unchanged) and, for inputs the recording does not hold, against tests/lfsr_ref.py,
which tests/test_packet_cpu.py holds to the recording.  MODE_GENERIC (one lane per stream, the reference's statements)
and the parallel form must give the same bytes."""
import numpy as np
import pytest

import lfsr_ref

pytestmark = pytest.mark.gpu

FX = lfsr_ref.fixture()
KINDS = ("scrambler", "descrambler", "additive")
WALK, CHUNK, TILE = 16, 32, 4096            # csrc/packet.h: items a lane walks (descrambler, additive; scrambler), items of a scan tile
# 1, the lanes' runs +- 1 (the scrambler's start behind its 32 serial items), the tile +- 1 (for the scrambler behind 32
# more), two tiles (the recording's length)
COUNTS = (1, WALK - 1, WALK, WALK + 1, 31, 32, 33, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, TILE - 1, TILE, TILE + 1, TILE + 31, TILE + 32,
          TILE + 33, 6000)


def make(gpu, kind, k, mode=None, streams=1):
    mask, seed, ln, count = FX["params"][k]
    blk = getattr(gpu, kind + "_bb" if kind != "additive" else "additive_scrambler_bb")(*((mask, seed, ln) + ((count,) if kind == "additive" else ())))
    if mode is not None:
        blk.set_mode(mode)
    if streams != 1:
        blk.set_streams(streams)
    return blk


_REFS = {}


def ref(kind, k, x, key):
    """the serial restatement on an input the recording does not hold, computed once"""
    if (kind, k, key) not in _REFS:
        mask, seed, ln, count = FX["params"][k]
        _REFS[(kind, k, key)] = lfsr_ref.Block(kind, mask, seed, ln, count).work(x)
    return _REFS[(kind, k, key)]


@pytest.mark.parametrize("k", range(len(FX["params"])))
@pytest.mark.parametrize("kind", KINDS)
def test_against_the_recording_whole_and_cut(gpu, kind, k):
    x = FX["input"]
    want = lfsr_ref.expected(kind, k)
    for n in COUNTS:
        got = make(gpu, kind, k).work(x[:n])
        assert np.array_equal(got, want[:n]), (n, int(np.flatnonzero(got != want[:n])[0]))
    for n in (33, 6000):
        assert np.array_equal(make(gpu, kind, k, gpu.MODE_GENERIC).work(x[:n]), want[:n]), n
    for mode in (gpu.MODE_FAST, gpu.MODE_GENERIC):
        for cuts in ((0, 7, 4097, 6000), tuple(range(41)) + (57, 4200, 6000)):         # the second: the start item by item
            blk = make(gpu, kind, k, mode)
            got = np.concatenate([blk.work(x[a:e]) for a, e in zip(cuts[:-1], cuts[1:])])
            assert np.array_equal(got, want), (mode, cuts[:3], int(np.flatnonzero(got != want)[0]))
    # the mode may change between calls: the state is the same
    blk = make(gpu, kind, k, gpu.MODE_GENERIC)
    a = blk.work(x[:100])
    blk.set_mode(gpu.MODE_FAST)
    b = blk.work(x[100:5000])
    blk.set_mode(gpu.MODE_GENERIC)
    c = blk.work(x[5000:])
    assert np.array_equal(np.concatenate([a, b, c]), want)


@pytest.mark.parametrize("k", range(len(FX["params"])))
@pytest.mark.parametrize("kind", KINDS)
def test_three_streams(gpu, kind, k):
    """every parameter set and every count with S = 3: stream 0 is the recording's input, streams 1 and 2 other bytes
    (their reference the restatement, computed once); every stream has its own register and its own row of tile carries"""
    x0 = FX["input"]
    xs = [x0, x0[::-1].copy(), np.roll(x0, 1234) ^ np.uint8(0x5A)]
    wants = [lfsr_ref.expected(kind, k), ref(kind, k, xs[1], "rev"), ref(kind, k, xs[2], "roll")]
    for n in COUNTS:
        for mode in (gpu.MODE_FAST,) + ((gpu.MODE_GENERIC,) if n in (1, 33, TILE + 1, 6000) else ()):
            got = make(gpu, kind, k, mode, 3).work(np.concatenate([x[:n] for x in xs])).reshape(3, n)
            for s in range(3):
                assert np.array_equal(got[s], wants[s][:n]), (n, mode, s)
    for mode in (gpu.MODE_FAST, gpu.MODE_GENERIC):
        blk = make(gpu, kind, k, mode, 3)
        parts = [blk.work(np.concatenate([x[a:e] for x in xs])).reshape(3, e - a) for a, e in ((0, 7), (7, 4097), (4097, 6000))]
        got = np.concatenate(parts, axis=1)
        for s in range(3):
            assert np.array_equal(got[s], wants[s]), (mode, s)
    blk.set_streams(3)                                          # restarts every stream from the seed
    assert np.array_equal(blk.work(np.concatenate([x[:50] for x in xs])).reshape(3, 50)[1], wants[1][:50])


@pytest.mark.parametrize("k", [0, 6, 8, 14])
@pytest.mark.parametrize("kind", KINDS)
def test_more_tiles_than_two(gpu, kind, k):
    """three whole tiles and a partial one behind the serial start: the carry pass runs along four tiles"""
    n = 32 + 3 * TILE + 5
    rng = np.random.RandomState(77)
    x = rng.randint(0, 256, 2 * n).astype(np.uint8)
    xs = [x[:n], x[n:]]
    wants = [ref(kind, k, xs[0], "long0"), ref(kind, k, xs[1], "long1")]
    fast = make(gpu, kind, k, gpu.MODE_FAST, 2).work(np.concatenate(xs)).reshape(2, n)
    generic = make(gpu, kind, k, gpu.MODE_GENERIC, 2).work(np.concatenate(xs)).reshape(2, n)
    for s in range(2):
        assert np.array_equal(fast[s], wants[s]) and np.array_equal(generic[s], wants[s]), s
    blk = make(gpu, kind, k, streams=2)                         # and cut in the middle of a tile
    cut = 32 + TILE + 100
    got = np.concatenate([blk.work(np.concatenate([v[:cut] for v in xs])).reshape(2, cut),
                          blk.work(np.concatenate([v[cut:] for v in xs])).reshape(2, n - cut)], axis=1)
    assert np.array_equal(got, np.stack(wants))


def test_qa_scrambler(gpu):
    """gnuradio-core/src/python/gnuradio/gr/qa_scrambler.py:33-61"""
    src = np.ones(1000, np.uint8)
    for mode in (gpu.MODE_FAST, gpu.MODE_GENERIC):
        s, d = gpu.scrambler_bb(0x8a, 0x7F, 7), gpu.descrambler_bb(0x8a, 0x7F, 7)          # CCSDS 7-bit scrambler
        s.set_mode(mode)
        d.set_mode(mode)
        dst = d.work(s.work(src))
        assert np.array_equal(src[:-8], dst[8:])                # skip garbage during synchronization
        for count in (0, 100):
            a, b = gpu.additive_scrambler_bb(0x8a, 0x7f, 7, count), gpu.additive_scrambler_bb(0x8a, 0x7f, 7, count)
            a.set_mode(mode)
            b.set_mode(mode)
            mid = a.work(src)
            assert np.array_equal(b.work(mid), src) and not np.array_equal(mid, src)


def test_device_entry_and_refusals(gpu):
    import torch
    x = FX["input"]
    blk = make(gpu, "scrambler", 0)
    d_in = torch.from_numpy(x.copy()).cuda()
    d_out = torch.zeros(6000, dtype=torch.uint8).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()                                    # the buffers are filled before the stream starts
    assert blk.work_device(0, d_in, d_out, stream=st) == 0      # a successful no-op
    blk.work_device(6000, d_in, d_out, stream=st)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), lfsr_ref.expected("scrambler", 0))
    for kind in KINDS:
        b = make(gpu, kind, 0)
        with pytest.raises(gpu.GrhipError):
            b.work_device(100, d_in, d_in[50:])                 # the output may not overlap the input
        with pytest.raises(gpu.GrhipError):
            b.work_device(-1, d_in, d_out)
        with pytest.raises(gpu.GrhipError):
            b.work_device(10, None, d_out)
        with pytest.raises(gpu.GrhipError):
            b.set_streams(0)
