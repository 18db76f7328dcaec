"""CPU tests of the real-input FIR kinds (fir_filter_fcc / _scc / _fsf, freq_xlating_fir_filter_{ccf,fcf,fcc,scf,scc}):
the references of tests/realin_ref.py against each other, the x86 float -> short conversion, and the product's
classes and refusals that need no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import realin_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("ntaps", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("decim", [1, 3, 4])
def test_widened_ccc_equals_direct_restatement(po, ntaps, decim):
    rng = np.random.default_rng(ntaps * 10 + decim)
    taps = (rng.standard_normal(ntaps) + 1j * rng.standard_normal(ntaps)).astype(np.complex64)
    taps[::3] = 0                                      # zero taps, both parts
    if ntaps > 1:
        taps[1] = complex(0.0, 0.5)                    # real part zero only
    n = 300
    xf = rng.standard_normal((n - 1) * decim + ntaps).astype(np.float32)
    xf[::5] = 0
    xs = rng.integers(-32768, 32768, (n - 1) * decim + ntaps).astype(np.int16)
    for x in (xf, xs):
        assert np.array_equal(_bits(rr.fir_cc_direct(taps, x, n, decim)), _bits(rr.fcc_ref(po, taps, x, n, decim)))
    tf = rng.standard_normal(ntaps).astype(np.float32)
    tf[::2] = 0
    assert np.array_equal(rr.fir_fsf_direct(tf * 100, xf * 100, n, decim), rr.fsf_ref(po, tf * 100, xf * 100, n, decim))


@pytest.mark.parametrize("complex_proto", [False, True])
def test_xlating_widened_equals_direct(po, complex_proto):
    rng = np.random.default_rng(7)
    ntaps, decim, nout = 33, 4, 1500                   # past three renormalisations of the rotator (every 512)
    proto = rng.standard_normal(ntaps).astype(np.float32)
    proto[5] = 0
    if complex_proto:
        proto = (proto + 1j * rng.standard_normal(ntaps)).astype(np.complex64)
    x = rng.standard_normal((nout - 1) * decim + ntaps).astype(np.float32)
    ref = rr.XlatingRef(po, decim, proto, 1234.5, 48000.0).work(x, nout)
    got = rr.xlating_direct(po, decim, proto, 1234.5, 48000.0, x, nout)
    assert np.array_equal(_bits(got), _bits(ref))


def test_x86_short_conversion():
    a = np.array([2.0 ** 31, -2.0 ** 31, np.nan, 40000.7, -40000.7, -32768.9, 32767.9, 65535.0, -0.9, 1e20, -np.inf,
                  70000.0, 2147483520.0], np.float32)
    want = np.array([0, 0, 0, 40000 - 65536, -40000 + 65536, -32768, 32767, -1, 0, 0, 0, 70000 - 65536,
                     2147483520 & 0xFFFF], np.int64)
    want = (want & 0xFFFF).astype(np.uint16).view(np.int16)
    assert np.array_equal(rr.x86_f2s(a), want)
    # in-range values agree with numpy's int32 -> int16 narrowing
    b = np.array([40000.7, -40000.7, -32768.9, 123456.0, -2.0 ** 30], np.float32)
    assert np.array_equal(rr.x86_f2s(b), b.astype(np.int32).astype(np.int16))


CLASSES = [("fir_filter_fcc", (1, [1 + 1j, 2])), ("fir_filter_scc", (2, [1 + 1j, 2])), ("fir_filter_fsf", (1, [1.0, 2.0])),
           ("freq_xlating_fir_filter_ccf", (4, [1.0, 2.0], 1000.0, 48000.0)),
           ("freq_xlating_fir_filter_fcf", (4, [1.0, 2.0], 1000.0, 48000.0)),
           ("freq_xlating_fir_filter_fcc", (4, [1 + 1j, 2], 1000.0, 48000.0)),
           ("freq_xlating_fir_filter_scf", (4, [1.0, 2.0], 1000.0, 48000.0)),
           ("freq_xlating_fir_filter_scc", (4, [1 + 1j, 2], 1000.0, 48000.0))]


@pytest.mark.parametrize("name,args", CLASSES)
def test_classes_exist_and_need_a_device(g, name, args):
    cls = getattr(g, name)
    assert name in g.binding.__all__
    if g.device_count() > 0:
        pytest.skip("a device is visible: the GPU tests cover construction")
    with pytest.raises(g.GrhipError) as e:
        cls(*args)
    assert e.value.code == -5                         # GRHIP_ENODEV


def test_dtypes_follow_the_signatures(g):
    assert g.fir_filter_scc._in == np.int16 and g.fir_filter_scc._tap == np.complex64
    assert g.fir_filter_fsf._out == np.int16 and g.fir_filter_fsf._in == np.float32
    assert g.fir_filter_fcc._in == np.float32 and g.fir_filter_fcc._out == np.complex64
    assert g.freq_xlating_fir_filter_scf._in == np.int16 and g.freq_xlating_fir_filter_scf._tap == np.float32
    assert g.freq_xlating_fir_filter_fcc._tap == np.complex64 and g.freq_xlating_fir_filter_ccf._in == np.complex64


def test_create_refusals_before_any_device(g):
    L = g.lib()
    h = C.c_void_p(0)
    taps = np.ones(16, np.float32)
    fc, xc = L.grhip_fir_filter_create, L.grhip_freq_xlating_fir_filter_create
    for k in (b"fcc", b"scc", b"fsf"):
        assert fc(C.byref(h), k, 0, taps.ctypes.data, 8, 0) == -1
        assert fc(C.byref(h), k, 1, None, 8, 0) == -1
    assert fc(C.byref(h), b"ssf", 1, taps.ctypes.data, 8, 0) == -1
    for k in (b"ccf", b"fcf", b"fcc", b"scf", b"scc", b"ccc"):
        assert xc(C.byref(h), k, 0, taps.ctypes.data, 8, 0.0, 1.0, 0) == -1
        assert xc(C.byref(h), k, 1, None, 8, 0.0, 1.0, 0) == -1
    assert xc(C.byref(h), b"sfc", 1, taps.ctypes.data, 8, 0.0, 1.0, 0) == -1
    assert xc(C.byref(h), None, 1, taps.ctypes.data, 8, 0.0, 1.0, 0) == -1
    assert not h.value


def test_xlating_test_compiles():
    r = subprocess.run(["make", "-C", os.path.join(PKG, "host"), "xlating_test"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
