"""Guarded device buffers for calling a *_work_device entry on a pointer that is aligned to its item and to nothing
more.  One allocation holds

    [ guard | offset pad | stream 0 | gap | stream 1 | ... | stream S-1 | guard ]

with the allocation's base on a 256-byte boundary and the front guard a multiple of 256 bytes, so `offset_items`
alone decides the alignment of the payload pointer.  Guards, pad and gaps hold a poison (NaN for float and complex
items, an odd bit pattern for integers and bytes); an access that rounds its address down or is one lane too wide
stays inside the allocation and shows in the comparison or in check_guards(), not as a memory fault.

No GPU code beyond torch copies: the same functions run on device="cpu", which is how tests/test_device_offsets_cpu.py
proves that each kind of misaddressed access is caught."""
import numpy as np
import torch

BASE_ALIGN = 256

# (input guard poison, second poison for the re-run, pre-fill of an output payload, output guard poison), one 32-bit
# word each (an output's guard differs from an input's, or a copy one item too wide would carry the one into the
# other unseen); wider items
# repeat the word, narrower ones take its low bytes (little endian).  Every integer pattern has bits 0 and 1 set in
# every byte, so a guard byte read as a framer / correlator item carries a data bit and a flag.
_FLOAT_WORDS = (0x7FC12345, 0x7F800000, 0x7FC54321, 0x7FC0BEEF)        # NaN, +inf, two more NaNs
_INT_WORDS = (0xA7A7A7A7, 0x5B5B5B5B, 0xC3C3C3C3, 0x9F9F9F9F)
POISON, POISON2, UNWRITTEN, OUT_GUARD = 0, 1, 2, 3


def pattern(dtype, which, itemsize=None):
    """the `itemsize` bytes of pattern `which` for items of `dtype`"""
    dtype = np.dtype(dtype)
    itemsize = itemsize or dtype.itemsize
    word = (_FLOAT_WORDS if dtype.kind in "fc" else _INT_WORDS)[which]
    b = np.frombuffer(np.uint32(word).tobytes(), np.uint8)
    return np.resize(b, itemsize).copy() if itemsize >= 4 else b[:itemsize].copy()


class Guarded(object):
    """what guarded() returns.  `raw` is the whole allocation as a uint8 tensor, `view` the uint8 tensor that starts
    at the payload (view.data_ptr() == ptr()); positions below are bytes from raw's start."""

    def __init__(self, raw, dtype, itemsize, n_streams, n_items, stride_items, start, is_output, squeeze):
        self.raw, self.dtype, self.itemsize = raw, np.dtype(dtype), itemsize
        self.n_streams, self.n_items, self.stride_items = n_streams, n_items, stride_items
        self.start, self.is_output, self._squeeze = start, is_output, squeeze
        self.view = raw[start:]
        self.which = POISON
        mask = np.zeros(raw.numel(), bool)
        for s in range(n_streams):
            b = start + s * stride_items * itemsize
            mask[b:b + n_items * itemsize] = True
        self.payload_mask = mask

    def ptr(self):
        return self.view.data_ptr()

    def host(self):
        """the whole allocation, copied to the host, as bytes"""
        return self.raw.cpu().numpy().copy()

    def payload(self):
        """the payload as a host array: [n_items] for one stream given as 1-D, else [n_streams, n_items]; items
        wider than the dtype (vectors) come back as [..., n_items, itemsize // dtype.itemsize]"""
        h = self.host()
        rows = [h[self.start + s * self.stride_items * self.itemsize:][:self.n_items * self.itemsize]
                for s in range(self.n_streams)]
        a = np.stack(rows).view(self.dtype)
        per = self.itemsize // self.dtype.itemsize
        a = a.reshape(self.n_streams, self.n_items, per) if per > 1 else a.reshape(self.n_streams, self.n_items)
        return a[0] if self._squeeze else a

    def expected_outside(self, which=None):
        """the bytes every position outside the payload was filled with"""
        which = self.which if which is None else which
        n = self.raw.numel()
        pat = pattern(self.dtype, which, self.itemsize)
        # the pattern is laid from the payload's start, so that items in the gaps and guards are whole poison items
        idx = (np.arange(n) - self.start) % self.itemsize
        return pat[idx]

    def repoison(self, which=POISON2):
        """fill everything outside the payload with another poison (the payload stays)"""
        h = self.host()
        exp = self.expected_outside(which)
        h[~self.payload_mask] = exp[~self.payload_mask]
        self.raw.copy_(torch.from_numpy(h))
        self.which = which


def _aligned_bytes(nbytes, device):
    t = torch.empty(nbytes + BASE_ALIGN, dtype=torch.uint8, device=device)
    skip = (-t.data_ptr()) % BASE_ALIGN
    t = t[skip:skip + nbytes]
    assert t.data_ptr() % BASE_ALIGN == 0
    return t


def guarded(arr, offset_items, guard_items=1024, poison=POISON, stride_items=None, itemsize=None, device="cuda",
            is_output=False):
    """arr: host array, [n_items] (one stream) or [n_streams, n_items]; with `itemsize` a multiple of the dtype's,
    the last axis holds n_items * (itemsize // dtype.itemsize) scalars (vector items).  Returns a Guarded whose
    payload holds arr, `offset_items` items past a 256-byte boundary, streams `stride_items` items apart (default:
    n_items, packed), everything else poisoned."""
    arr = np.ascontiguousarray(arr)
    squeeze = arr.ndim == 1
    a2 = arr.reshape(1, -1) if squeeze else arr
    assert a2.ndim == 2
    itemsize = itemsize or arr.dtype.itemsize
    assert itemsize % arr.dtype.itemsize == 0
    n_streams = a2.shape[0]
    row_bytes = a2.shape[1] * arr.dtype.itemsize
    assert row_bytes % itemsize == 0
    n_items = row_bytes // itemsize
    stride_items = n_items if stride_items is None else int(stride_items)
    assert stride_items >= n_items or n_streams == 1
    front = -(-guard_items * itemsize // BASE_ALIGN) * BASE_ALIGN
    start = front + offset_items * itemsize
    total = start + ((n_streams - 1) * stride_items + n_items) * itemsize + guard_items * itemsize
    raw = _aligned_bytes(total, device)
    g = Guarded(raw, arr.dtype, itemsize, n_streams, n_items, stride_items, start, is_output, squeeze)
    h = g.expected_outside(poison)
    rows = a2.view(np.uint8).reshape(n_streams, row_bytes)
    for s in range(n_streams):
        b = start + s * stride_items * itemsize
        h[b:b + row_bytes] = rows[s]
    raw.copy_(torch.from_numpy(h))
    g.which = poison
    assert g.ptr() % BASE_ALIGN == (offset_items * itemsize) % BASE_ALIGN
    return g


def guarded_output(n_items, dtype, offset_items, n_streams=None, guard_items=1024, stride_items=None, itemsize=None,
                   device="cuda"):
    """an output buffer: payload pre-filled with the UNWRITTEN pattern (so "not written" and "written as zero"
    differ; for float items it reads as NaN), everything else poisoned.  n_streams=None: one stream, 1-D payload."""
    dtype = np.dtype(dtype)
    itemsize = itemsize or dtype.itemsize
    per = itemsize // dtype.itemsize
    pat = pattern(dtype, UNWRITTEN, itemsize)
    shape = (n_items * per,) if n_streams is None else (n_streams, n_items * per)
    rows = np.resize(pat, int(np.prod(shape)) * dtype.itemsize).view(dtype).reshape(shape)
    return guarded(rows, offset_items, guard_items, OUT_GUARD, stride_items, itemsize, device, is_output=True)


def unwritten_items(buf):
    """bool per payload item: still holds the pre-fill pattern"""
    p = np.ascontiguousarray(buf.payload())
    items = p.view(np.uint8).reshape(-1, buf.itemsize)
    return (items == pattern(buf.dtype, UNWRITTEN, buf.itemsize)).all(axis=1)


def check_guards(buf):
    """every byte outside the payload of an output buffer still equals the pattern it was filled with"""
    assert buf.is_output, "check_guards is for output buffers"
    h, exp = buf.host(), buf.expected_outside()
    bad = np.flatnonzero((h != exp) & ~buf.payload_mask)
    if bad.size:
        first = int(bad[0])
        end = buf.start + ((buf.n_streams - 1) * buf.stride_items + buf.n_items) * buf.itemsize
        where = ("%d byte(s) before the payload" % (buf.start - first) if first < buf.start else
                 "%d byte(s) past the payload's end" % (first - end + 1) if first >= end else
                 "in a gap between streams, byte %d of the payload area" % (first - buf.start))
        raise AssertionError("%d guard byte(s) overwritten, the first %s" % (bad.size, where))
