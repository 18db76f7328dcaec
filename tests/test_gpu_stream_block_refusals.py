"""What the stream blocks refuse and what a refusal leaves alone, one handle of every family, S = 2 streams of n = 16
items, every device buffer a slice of one small torch tensor.

Per handle: a negative count is GRHIP_EINVAL and a zero count returns 0 (work and work_device); a null input or output,
a misaligned one (base + 2 bytes) and an output that overlaps the input (input + one item) are refused by work_device,
each where the table says the handle refuses it -- byte items have no alignment, keep_one_in_n copies items of any
size, the element-wise spectrum blocks, keep_one_in_n and map_bb take in-place calls, and dc_blocker checks no
overlap; set_streams(0),
set_streams(65536), set_mode(99) and a state getter at stream index S are refused.  Every one of these returns before
anything is launched.  Then one valid call gives, byte for byte, what a fresh handle gives (a refusal touched no
state), and after set_streams(3) every stream reads and computes as a fresh handle's does.  am_demod_cf and
fm_demod_cf zero *d_produced on a zero count."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -1         # GRHIP_EINVAL (include/grhip.h)
S, N = 2, 16
IN, OUT, EXTRA, END = 0, 1024, 2048, 4096      # byte offsets of the input, the output and the further outputs
STEP = 512                                      # between two further outputs


class Spec(object):
    """make(g) builds the handle; in_dt / out_dt are the item types; n_out(n) is every stream's output items of a call of
    n from a fresh handle; dev_extra further device outputs between d_out and stream; host_extra(S) their host twins;
    align_in / align_out / overlap say what work_device refuses (overlap False: in-place calls are taken and give the
    same output; None: dc_blocker makes no overlap check and promises nothing, so none is tried); getters read one
    stream's state"""

    def __init__(self, name, make, in_dt, out_dt, n_out=lambda n: n, dev_extra=0, host_extra=lambda s: [],
                 align_in=True, align_out=True, overlap=True, has_mode=True, getters=()):
        self.name, self.make, self.in_dt, self.out_dt, self.n_out = name, make, np.dtype(in_dt), np.dtype(out_dt), n_out
        self.dev_extra, self.host_extra, self.align_in, self.align_out = dev_extra, host_extra, align_in, align_out
        self.overlap, self.has_mode, self.getters = overlap, has_mode, getters


def _floats(k):
    return lambda s: [np.zeros(s * N, np.float32) for _ in range(k)]


def _ints(s):
    return [np.zeros(s, np.int32)]


LOOP = (lambda b, s: b.get_frequency(s), lambda b, s: b.get_phase(s))
SPECS = [
    Spec("agc_cc", lambda g: g.agc_cc(1e-2, 1.0, 2.0, 0.0), np.complex64, np.complex64, getters=(lambda b, s: b.gain(s),)),
    Spec("agc2_ff", lambda g: g.agc2_ff(1e-1, 1e-2, 1.0, 2.0, 0.0), np.float32, np.float32, getters=(lambda b, s: b.gain(s),)),
    Spec("costas_loop_cc", lambda g: g.costas_loop_cc(0.1, 2), np.complex64, np.complex64, dev_extra=1, host_extra=_floats(1),
         getters=LOOP),
    Spec("pll_carriertracking_cc", lambda g: g.pll_carriertracking_cc(0.1, 0.5, -0.5), np.complex64, np.complex64,
         getters=LOOP + (lambda b, s: b.locksig(s),)),
    Spec("iir_filter_ffd", lambda g: g.iir_filter_ffd([1.0], [0.0, 0.5]), np.float32, np.float32),
    Spec("fm_demod_cf", lambda g: g.fm_demod_cf(8000, 3, 1000, [1.0, 0.5], tau=None), np.complex64, np.float32,
         n_out=lambda n: (n + 2) // 3, dev_extra=1, host_extra=lambda s: [np.zeros(1, np.int32)]),
    Spec("am_demod_cf", lambda g: g.am_demod_cf.from_taps(3, [1.0, 0.5]), np.complex64, np.float32,
         n_out=lambda n: (n + 2) // 3, dev_extra=1, host_extra=lambda s: [np.zeros(1, np.int32)]),
    Spec("complex_to_mag", lambda g: g.complex_to_mag(1), np.complex64, np.float32, overlap=False),
    Spec("single_pole_iir_filter_ff", lambda g: g.single_pole_iir_filter_ff(0.5, 1), np.float32, np.float32, overlap=False),
    Spec("keep_one_in_n", lambda g: g.keep_one_in_n(4, 2), np.float32, np.float32, n_out=lambda n: n // 2,
         align_in=False, align_out=False, overlap=False, has_mode=False),
    Spec("dc_blocker_ff", lambda g: g.dc_blocker_ff(2, False), np.float32, np.float32, overlap=None),
    Spec("pwr_squelch_cc", lambda g: g.pwr_squelch_cc(-10.0, 0.5, 2, False), np.complex64, np.complex64, dev_extra=1,
         host_extra=_ints, getters=(lambda b, s: b.state(s),)),
    Spec("ctcss_squelch_ff", lambda g: g.ctcss_squelch_ff(1000, 100.0, 0.01, 4, 2, False), np.float32, np.float32, dev_extra=1,
         host_extra=_ints, getters=(lambda b, s: b.state(s),)),
    Spec("constellation_decoder_cb", lambda g: g.constellation_decoder_cb(g.constellation_qpsk()), np.complex64, np.uint8,
         align_out=False),
    Spec("diff_decoder_bb", lambda g: g.diff_decoder_bb(4), np.uint8, np.uint8, align_in=False, align_out=False),
    Spec("map_bb", lambda g: g.map_bb([3, 2, 1, 0]), np.uint8, np.uint8, align_in=False, align_out=False, overlap=False),
    Spec("constellation_receiver_cb", lambda g: g.constellation_receiver_cb(g.constellation_qpsk(), 0.1, -0.25, 0.25),
         np.complex64, np.uint8, dev_extra=3, host_extra=_floats(3), align_out=False, getters=LOOP),
]


def signal(dt, streams):
    """streams x N items of no particular shape, the same every time"""
    r = np.random.RandomState(5)
    if dt == np.uint8:
        return r.randint(0, 4, streams * N).astype(np.uint8)
    x = r.standard_normal(2 * streams * N).astype(np.float32)
    return (x[0::2] + 1j * x[1::2]).astype(np.complex64) if dt == np.complex64 else x[:streams * N].copy()


class Device(object):
    """the one tensor and the calls on slices of it"""

    def __init__(self, spec):
        self.spec = spec
        self.buf = torch.zeros(END, dtype=torch.uint8, device="cuda")
        self.base = self.buf.data_ptr()
        assert self.base % 256 == 0

    def args(self, d_in, d_out):
        extra = [self.base + EXTRA + k * STEP for k in range(self.spec.dev_extra)]
        return [C.c_void_p(p) for p in [d_in, d_out] + extra + [0]]        # stream NULL: the handle's own

    def call(self, blk, n, d_in=None, d_out=None):
        rc = blk._call("work_device", int(n), *self.args(self.base + IN if d_in is None else d_in,
                                                         self.base + OUT if d_out is None else d_out))
        torch.cuda.synchronize()
        return rc

    def load(self, x):
        self.buf.zero_()
        raw = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy())
        self.buf[IN:IN + len(raw)] = raw.cuda()
        torch.cuda.synchronize()

    def run(self, blk, x, streams=S):
        """one valid call of N items per stream; returns every stream's output bytes and everything behind d_out"""
        self.load(x)
        self.call(blk, N)
        got = self.buf.cpu().numpy()
        per = self.spec.n_out(N) * self.spec.out_dt.itemsize
        return [got[OUT + s * per:OUT + (s + 1) * per].copy() for s in range(streams)], got[OUT:].copy()


def refused(fn, *a):
    with pytest.raises(Exception) as e:
        fn(*a)
    assert getattr(e.value, "code", None) == EINVAL, "%r" % (e.value,)


def states(spec, blk, streams):
    return [tuple(get(blk, s) for get in spec.getters) for s in range(streams)]


def make(g, spec, streams=S):
    blk = spec.make(g)
    blk.set_streams(streams)
    return blk


@pytest.mark.parametrize("spec", SPECS, ids=[s.name for s in SPECS])
def test_refusals_touch_nothing(gpu, spec):
    g = gpu
    dev = Device(spec)
    x = signal(spec.in_dt, S)
    fresh_state = states(spec, make(g, spec), S)
    ref = make(g, spec)
    ref_streams, ref_all = dev.run(ref, x)
    ref_state = states(spec, ref, S)
    assert ref_all.any()                                # the comparison below compares something

    blk = make(g, spec)
    dev.load(x)
    d_in, d_out = dev.base + IN, dev.base + OUT
    host_in, host_out = x.copy(), np.zeros(S * N, spec.out_dt)
    host = [C.c_void_p(a.ctypes.data) for a in [host_in, host_out] + spec.host_extra(S)]

    # the item count
    refused(dev.call, blk, -1)
    refused(blk._call, "work", -1, *host)
    if spec.name in ("am_demod_cf", "fm_demod_cf"):
        dev.buf[EXTRA:EXTRA + 4] = 7
        torch.cuda.synchronize()
    assert dev.call(blk, 0) == 0
    if spec.name in ("am_demod_cf", "fm_demod_cf"):
        assert not dev.buf[EXTRA:EXTRA + 4].cpu().numpy().any()             # *d_produced = 0
    assert blk._call("work", 0, *host) == 0
    # the buffers
    a = dev.args(d_in, d_out)
    refused(blk._call, "work_device", N, C.c_void_p(0), *a[1:])
    refused(blk._call, "work_device", N, a[0], C.c_void_p(0), *a[2:])
    if spec.align_in:
        refused(dev.call, blk, N, d_in + 2, d_out)
    if spec.align_out:
        refused(dev.call, blk, N, d_in, d_out + 2)
    if spec.overlap:
        refused(dev.call, blk, N, d_in, d_in + spec.in_dt.itemsize)
    # the setters and the getters
    refused(blk.set_streams, 0)
    refused(blk.set_streams, 65536)
    if spec.has_mode:
        refused(blk.set_mode, 99)
    for get in spec.getters:
        refused(get, blk, S)

    # nothing of that touched the handle
    got_streams, got_all = dev.run(blk, x)
    assert np.array_equal(got_all, ref_all)
    assert states(spec, blk, S) == ref_state

    # set_streams restarts every stream from the constructor's values
    blk.set_streams(3)
    assert states(spec, blk, 3) == [fresh_state[0]] * 3
    per = N * spec.in_dt.itemsize
    raw = x.view(np.uint8)
    x3 = np.concatenate([raw[:per], raw[per:], raw[:per]])
    got3, _ = dev.run(blk, x3, 3)
    for s, r in enumerate((0, 1, 0)):
        assert np.array_equal(got3[s], ref_streams[r]), "stream %d" % s


IN_PLACE = [s for s in SPECS if s.overlap is False]


@pytest.mark.parametrize("spec", IN_PLACE, ids=[s.name for s in IN_PLACE])
def test_in_place_calls_stay_allowed(gpu, spec):
    g = gpu
    dev = Device(spec)
    x = signal(spec.in_dt, S)
    ref_streams, _ = dev.run(make(g, spec), x)
    # the output on the input: what the separate buffers gave (S * N items: one wave reads them all before it writes)
    blk = make(g, spec)
    dev.load(x)
    dev.call(blk, N, dev.base + IN, dev.base + IN)
    got = dev.buf.cpu().numpy()
    per = spec.n_out(N) * spec.out_dt.itemsize
    for s in range(S):
        assert np.array_equal(got[IN + s * per:IN + (s + 1) * per], ref_streams[s]), "stream %d" % s
    # the output one item behind the input is taken as well
    blk = make(g, spec)
    dev.load(x)
    assert dev.call(blk, N, dev.base + IN, dev.base + IN + spec.in_dt.itemsize) >= 0
