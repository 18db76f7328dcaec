"""The guarded-buffer harness of tests/device_offsets.py, proven on the CPU: stand-in numpy "kernels" copy between
the CPU twins of the device buffers, and every kind of misaddressed access the GPU tests rely on the harness to
show is shown.  Without this a guard that nobody compares would make tests/test_gpu_device_offsets.py vacuous."""
import numpy as np
import pytest

import device_offsets as do
from conftest import bits_equal

DTYPES = [np.uint8, np.int16, np.int32, np.float32, np.complex64]
OFFSETS = {1: [0, 1, 7, 8, 15], 2: [0, 1, 3, 7], 4: [0, 1, 2, 3], 8: [0, 1]}


def _data(dtype, shape, seed=0):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    if dtype.kind == "f":
        return rng.standard_normal(shape).astype(dtype)
    return rng.integers(0, 2, shape).astype(dtype)              # bits, as the framer and the correlator take them


def _items(buf):
    """the whole CPU allocation as a writable array of items, and the index of the payload's first item"""
    lead = buf.start % buf.itemsize
    a = buf.raw.numpy()[lead:]
    a = a[:a.size // buf.itemsize * buf.itemsize].view(buf.dtype)
    return a, (buf.start - lead) // buf.itemsize


def copy_kernel(src, dst, n, rd=0, wr=0, skip=None):
    """the stand-in: dst[i + wr] = src[i + rd] for i < n on every stream, item `skip` left out"""
    s, s0 = _items(src)
    d, d0 = _items(dst)
    for k in range(src.n_streams):
        for i in range(n):
            if i != skip:
                d[d0 + k * dst.stride_items + i + wr] = s[s0 + k * src.stride_items + i + rd]


def _case(dtype, n=37, n_streams=None, in_off=1, out_off=3, in_stride=None, out_stride=None):
    shape = (n,) if n_streams is None else (n_streams, n)
    x = _data(dtype, shape)
    src = do.guarded(x, in_off, guard_items=16, stride_items=in_stride, device="cpu")
    dst = do.guarded_output(n, dtype, out_off, n_streams=n_streams, guard_items=16, stride_items=out_stride,
                            device="cpu")
    return x, src, dst


def _verdict(x, dst):
    """what a GPU case asserts: payload equal to the reference, guards intact"""
    assert bits_equal(dst.payload(), x), "payload differs from the reference"
    do.check_guards(dst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_and_correct_copy_pass_at_every_offset(dtype):
    size = np.dtype(dtype).itemsize
    for in_off in OFFSETS[size]:
        for out_off in OFFSETS[size]:
            x, src, dst = _case(dtype, in_off=in_off, out_off=out_off)
            assert src.ptr() % do.BASE_ALIGN == in_off * size and dst.ptr() % do.BASE_ALIGN == out_off * size
            assert src.view.data_ptr() == src.raw.data_ptr() + src.start
            assert bits_equal(src.payload(), x)
            assert do.unwritten_items(dst).all()
            copy_kernel(src, dst, len(x))
            _verdict(x, dst)
            assert not do.unwritten_items(dst).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strides", [(None, None), (48, 41), (37, 53)])
def test_strided_streams_correct_copy_passes(dtype, strides):
    x, src, dst = _case(dtype, n_streams=3, in_stride=strides[0], out_stride=strides[1])
    copy_kernel(src, dst, x.shape[1])
    _verdict(x, dst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_store_one_item_before_the_payload_is_caught(dtype):
    x, src, dst = _case(dtype)
    copy_kernel(src, dst, len(x))
    copy_kernel(src, dst, 1, wr=-1)
    with pytest.raises(AssertionError, match="before the payload"):
        do.check_guards(dst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_store_one_item_behind_the_payload_is_caught(dtype):
    x, src, dst = _case(dtype)
    copy_kernel(src, dst, len(x))
    copy_kernel(src, dst, 1, wr=len(x))
    with pytest.raises(AssertionError, match="past the payload's end"):
        do.check_guards(dst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_one_item_too_wide_is_caught(dtype):
    """it carries the input's guard item into the output's guard: the two poisons differ"""
    x, src, dst = _case(dtype)
    copy_kernel(src, dst, len(x) + 1)
    with pytest.raises(AssertionError, match="past the payload's end"):
        do.check_guards(dst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_store_into_the_gap_between_streams_is_caught(dtype):
    x, src, dst = _case(dtype, n_streams=2, in_stride=50, out_stride=45)
    copy_kernel(src, dst, x.shape[1])
    copy_kernel(src, dst, 1, wr=x.shape[1])
    with pytest.raises(AssertionError, match="gap between streams"):
        do.check_guards(dst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwritten_output_item_is_caught(dtype):
    """also where the reference's item is zero: the pre-fill is not zero"""
    x, src, dst = _case(dtype)
    x[11] = 0
    src = do.guarded(x, 1, guard_items=16, device="cpu")
    copy_kernel(src, dst, len(x), skip=11)
    assert do.unwritten_items(dst)[11] and do.unwritten_items(dst).sum() == 1
    with pytest.raises(AssertionError, match="payload differs"):
        _verdict(x, dst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rd", [-1, 1], ids=["early", "late"])
def test_input_read_one_item_off_reaches_the_output(dtype, rd):
    x, src, dst = _case(dtype)
    copy_kernel(src, dst, len(x), rd=rd)
    got = dst.payload()
    edge = got[0] if rd < 0 else got[-1]
    assert bits_equal(np.array([edge]), do.pattern(dtype, do.POISON).view(dtype))
    if np.dtype(dtype).kind in "fc":
        assert np.isnan(edge)
    else:
        assert int(edge) & 3 == 3                                  # a data bit and a flag for the integer blocks
    with pytest.raises(AssertionError, match="payload differs"):
        _verdict(x, dst)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
def test_masked_guard_read_shows_in_the_second_run(dtype):
    """a kernel that reads a guard item and keeps one bit of it: the first poison may agree with the reference by
    chance, the re-run under the second poison then differs from the first"""
    x, src, dst = _case(dtype)

    def leaky(src, dst):
        copy_kernel(src, dst, len(x))
        s, s0 = _items(src)
        d, d0 = _items(dst)
        d[d0] = (int(d[d0]) & ~4) | (int(s[s0 - 1]) & 4)

    leaky(src, dst)
    first = dst.payload().copy()
    src.repoison(do.POISON2)
    assert bits_equal(src.payload(), x)
    dst2 = do.guarded_output(len(x), dtype, 3, guard_items=16, device="cpu")
    leaky(src, dst2)
    assert not bits_equal(dst2.payload(), first)


def test_vector_items_and_patterns():
    x = np.arange(5 * 16, dtype=np.uint8)
    buf = do.guarded(x, 1, guard_items=4, itemsize=16, device="cpu")
    assert buf.n_items == 5 and buf.ptr() % do.BASE_ALIGN == 16 and buf.payload().shape == (5, 16)
    for dtype in DTYPES:
        pats = [do.pattern(dtype, w).tobytes() for w in range(4)]
        assert len(set(pats)) == 4
    assert np.isnan(do.pattern(np.float32, do.POISON).view(np.float32)[0])
    assert np.isnan(do.pattern(np.complex64, do.UNWRITTEN).view(np.complex64)[0])
    assert all(b & 3 == 3 for w in range(4) for b in do.pattern(np.uint8, w, 16))
