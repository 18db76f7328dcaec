"""-m gpu: the lifetime of block handles (csrc/grhip_internal.h: owners free themselves, make_handle, destroy_handle).

1. a create that fails leaves no handle and the error of the step that failed; the next create works
2. create / work / destroy cycles do not lose device memory
3. the latched set_taps of fft_filter_ccc / _fff (one body for both)
4. fft_vcc.set_window (one body with fft_vfc)
"""
import numpy as np
import pytest

from conftest import bits_equal, rel_err_max

pytestmark = pytest.mark.gpu

NC = 1 << 19            # complex64 items in 4 MiB
NF = 1 << 20            # float32 items in 4 MiB
NB = 1 << 22            # bytes in 4 MiB
S_BYTES = 4 << 20       # what one handle owns at least once used
K = 32                  # cycles between the two readings of the free memory

_cache = {}


def _z(n, dtype):
    """n zero items, made once (the cycles only need the buffers to exist)"""
    key = (int(n), np.dtype(dtype).str)
    if key not in _cache:
        _cache[key] = np.zeros(int(n), dtype=dtype)
    return _cache[key]


def _dev(name, make):
    """a device tensor shared by the cycles of one case, allocated before the free memory is read"""
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _lp(g, n):
    return g.workload.lowpass_taps(n, 200e3, 10e6)


def _mm_args(g):
    c4 = g.workload.CFG4
    return (c4["omega"], c4["gain_omega"], c4["mu"], c4["gain_mu"], c4["omega_relative_limit"])


def _chain(g, dev, taps=None, S=8, n=600_000):
    wl = g.workload
    c, c4 = wl.CFG2, wl.CFG4
    taps = wl.cfg2_proto_taps() if taps is None else taps
    return g.dmr_chain(c["decim"], taps, c["center_freq"], c["fs"], c["demod_gain"], c4["omega"], c4["gain_omega"],
                       c4["mu"], c4["gain_mu"], c4["omega_relative_limit"], wl.access_code_string(), c4["threshold"],
                       S, n, device=dev)


def _chain_use(g, ch, S=8, n=600_000):
    import torch
    dev = torch.device("cuda", 0)
    stride = n + 64
    d_in = _dev("chain_in", lambda: torch.zeros((S, stride, 2), dtype=torch.float32, device=dev))
    d_bits = _dev("chain_bits", lambda: torch.zeros((S, n // 4), dtype=torch.uint8, device=dev))
    d_n = _dev("chain_n", lambda: torch.zeros(S, dtype=torch.int32, device=dev))
    ch.run_device(d_in, n, stride, d_bits, n // 4, d_n, None)
    torch.cuda.synchronize()


def _framer_batch_use(g, b, S=8, n=NB):
    import torch
    dev = torch.device("cuda", 0)
    d_in = _dev("fb_in", lambda: torch.zeros((S, n), dtype=torch.uint8, device=dev))
    d_n = _dev("fb_n", lambda: torch.full((S,), 4096, dtype=torch.int32, device=dev))
    b.run_device(d_in, n, d_n, 4096, None)
    torch.cuda.synchronize()


def _xl(kind):
    def make(g, dev):
        cls = getattr(g, "freq_xlating_fir_filter_" + kind)
        tap = np.complex64 if kind in ("ccc", "fcc", "scc") else np.float32
        return cls(4, _lp(g, 64).astype(tap), 1.25e6, 10e6, device=dev)
    return make


def _xl_use(items):
    return lambda g, b: b.work(items // 4, _z(items + 63, b._in))


def _fir(kind):
    def make(g, dev):
        cls = getattr(g, "fir_filter_" + kind)
        return cls(1, _lp(g, 16).astype(cls._tap), device=dev)
    return make


def _fir_use(n):
    return lambda g, b: b.work(n, _z(n + 15, b._in))


# name -> (make(g, device), use(g, handle)); used once, a handle owns at least S_BYTES of device memory.
# Where nothing else is named the 4 MiB are the staging buffers of one host-buffer call (device memory above
# StageBuf::MAPPED_MAX = 2 MiB); the comment names a larger buffer of the handle's own.
CASES = {
    "fir_filter_ccf": (_fir("ccf"), _fir_use(NC)),
    "fir_filter_fff": (_fir("fff"), _fir_use(NF)),
    "fir_filter_ccc": (_fir("ccc"), _fir_use(NC)),
    "fir_filter_fcc": (_fir("fcc"), _fir_use(NF)),
    "fir_filter_scc": (_fir("scc"), _fir_use(NC)),             # 4 MiB of outputs
    "fir_filter_fsf": (_fir("fsf"), _fir_use(NF)),             # + d_scratch, 4 MiB of floats
    "fir_filter_with_buffer_ccf": (lambda g, d: g.fir_filter_with_buffer("ccf", _lp(g, 16), device=d),
                                   lambda g, b: b.filterNdec(_z(NC, np.complex64), NC)),
    "fir_filter_with_buffer_fff": (lambda g, d: g.fir_filter_with_buffer("fff", _lp(g, 16), device=d),
                                   lambda g, b: b.filterNdec(_z(NF, np.float32), NF)),
    "fir_filter_with_buffer_ccc": (lambda g, d: g.fir_filter_with_buffer("ccc", _lp(g, 16).astype(np.complex64), device=d),
                                   lambda g, b: b.filterNdec(_z(NC, np.complex64), NC)),
    "freq_xlating_fir_filter_ccc": (_xl("ccc"), _xl_use(NC)),
    "freq_xlating_fir_filter_ccf": (_xl("ccf"), _xl_use(NC)),
    "freq_xlating_fir_filter_fcf": (_xl("fcf"), _xl_use(NF)),
    "freq_xlating_fir_filter_fcc": (_xl("fcc"), _xl_use(NF)),
    "freq_xlating_fir_filter_scf": (_xl("scf"), _xl_use(2 * NF)),
    "freq_xlating_fir_filter_scc": (_xl("scc"), _xl_use(2 * NF)),
    "quadrature_demod_cf": (lambda g, d: g.quadrature_demod_cf(1.0, device=d),
                            lambda g, b: b.work(NC, _z(NC + 1, np.complex64))),
    "xlating_demod": (lambda g, d: g.xlating_demod(4, g.workload.cfg2_proto_taps(), 1.25e6, 10e6, 1.0, device=d),
                      lambda g, b: b.work(NC // 4, _z(NC + 255, np.complex64))),
    "clock_recovery_mm_ff": (lambda g, d: g.clock_recovery_mm_ff(*_mm_args(g), device=d),
                             lambda g, b: b.general_work(NF // 16, _z(NF, np.float32))),
    "clock_recovery_mm_cc": (lambda g, d: g.clock_recovery_mm_cc(*_mm_args(g), device=d),
                             lambda g, b: b.general_work(NC // 16, _z(NC, np.complex64))),
    "binary_slicer_fb": (lambda g, d: g.binary_slicer_fb(device=d), lambda g, b: b.work(NF, _z(NF, np.float32))),
    "pager_slicer_fb": (lambda g, d: g.pager_slicer_fb(0.001, device=d), lambda g, b: b.work(NF, _z(NF, np.float32))),
    "unpack_k_bits_bb": (lambda g, d: g.unpack_k_bits_bb(8, device=d), lambda g, b: b.work(NB, _z(NB // 8, np.uint8))),
    "stream_to_vector": (lambda g, d: g.stream_to_vector(8, 16, device=d),
                         lambda g, b: b.work(1024, _z(16 * 1024, np.complex64))),
    "head": (lambda g, d: g.head(8, 1 << 30, device=d), lambda g, b: b.work(1024, _z(1024, np.complex64))),
    # d_pool: 8 streams x (4 Mi / 8 + 4 KiB) = 4.03 MiB, d_F + d_D 1 MiB each
    "framer_sink_1_batch": (lambda g, d: g.framer_sink_1_batch(8, NB, device=d), _framer_batch_use),
    "framer_sink_1": (lambda g, d: g.framer_sink_1(device=d), lambda g, b: b.work(NB, _z(NB, np.uint8))),
    "stream_to_streams": (lambda g, d: g.stream_to_streams(8, 4, device=d),
                          lambda g, b: b.work(NC // 4, _z(NC, np.complex64))),
    "vector_to_streams": (lambda g, d: g.vector_to_streams(8, 4, device=d),
                          lambda g, b: b.work(NC // 4, _z(NC, np.complex64))),
    "streams_to_stream": (lambda g, d: g.streams_to_stream(8, 4, device=d),
                          lambda g, b: b.work(NC, [_z(NC // 4, np.complex64)] * 4)),
    "correlate_access_code_bb": (lambda g, d: g.correlate_access_code_bb(g.workload.access_code_string(), 4, device=d),
                                 lambda g, b: b.work(NB, _z(NB, np.uint8))),
    # d_window: 2^20 floats = 4 MiB
    "fft_vcc": (lambda g, d: g.fft_vcc(1 << 20, True, np.ones(1 << 20, np.float32), False, device=d),
                lambda g, b: b.work(1, _z(1 << 20, np.complex64))),
    "fft_vfc": (lambda g, d: g.fft_vfc(1 << 20, True, np.ones(1 << 20, np.float32), device=d),
                lambda g, b: b.work(1, _z(1 << 20, np.float32))),
    # 3000 taps: above OLS_MAX_TAPS, fftsize 8192; d_a and d_b hold 64 transforms = 4 MiB each
    "fft_filter_ccc": (lambda g, d: g.fft_filter_ccc(1, _lp(g, 3000).astype(np.complex64), device=d),
                       lambda g, b: b.work(64 * b.nsamples(), _z(64 * 5193, np.complex64))),
    "fft_filter_fff": (lambda g, d: g.fft_filter_fff(1, _lp(g, 3000), device=d),
                       lambda g, b: b.work(128 * b.nsamples(), _z(128 * 5193, np.float32))),
    "pfb_channelizer_ccf": (lambda g, d: g.pfb_channelizer_ccf(64, _lp(g, 64 * 16), 1, device=d),
                            lambda g, b: b.general_work(8192, [_z(8192 + 32, np.complex64)] * 64)),
    "pfb_decimator_ccf": (lambda g, d: g.pfb_decimator_ccf(8, _lp(g, 8 * 16), 0, device=d),
                          lambda g, b: b.work(NC // 8, [_z(NC // 8 + 32, np.complex64)] * 8)),
    "pfb_arb_resampler_ccf": (lambda g, d: g.pfb_arb_resampler_ccf(1.25, _lp(g, 32 * 16), 32, device=d),
                              lambda g, b: b.general_work(NC, _z(NC, np.complex64))),
    "pfb_arb_resampler_fff": (lambda g, d: g.pfb_arb_resampler_fff(1.25, _lp(g, 32 * 16), 32, device=d),
                              lambda g, b: b.general_work(NF, _z(NF, np.float32))),
    "fractional_interpolator_ff": (lambda g, d: g.fractional_interpolator_ff(0.0, 1.5, device=d),
                                   lambda g, b: b.general_work(NF // 2, _z(NF, np.float32))),
    "fractional_interpolator_cc": (lambda g, d: g.fractional_interpolator_cc(0.0, 1.5, device=d),
                                   lambda g, b: b.general_work(NC // 2, _z(NC, np.complex64))),
    "hilbert_fc": (lambda g, d: g.hilbert_fc(31, device=d), lambda g, b: b.work(NF, _z(NF + 30, np.float32))),
    "filter_delay_fc": (lambda g, d: g.filter_delay_fc(g.firdes_hilbert(31), device=d),
                        lambda g, b: b.work(NF, _z(NF + 30, np.float32))),
    "goertzel_fc": (lambda g, d: g.goertzel_fc(8000, 64, 1000.0, device=d),
                    lambda g, b: b.work(NF // 64, _z(NF, np.float32))),
    "interp_fir_filter_ccf": (lambda g, d: g.interp_fir_filter_ccf(4, _lp(g, 32), device=d),
                              lambda g, b: b.work(NC, _z(NC // 4 + 32, np.complex64))),
    "interp_fir_filter_fff": (lambda g, d: g.interp_fir_filter_fff(4, _lp(g, 32), device=d),
                              lambda g, b: b.work(NF, _z(NF // 4 + 32, np.float32))),
    "interp_fir_filter_ccc": (lambda g, d: g.interp_fir_filter_ccc(4, _lp(g, 32).astype(np.complex64), device=d),
                              lambda g, b: b.work(NC, _z(NC // 4 + 32, np.complex64))),
    "rational_resampler_base_ccf": (lambda g, d: g.rational_resampler_base_ccf(3, 2, _lp(g, 24), device=d),
                                    lambda g, b: b.general_work(NC, _z(NC, np.complex64))),
    "rational_resampler_base_fff": (lambda g, d: g.rational_resampler_base_fff(3, 2, _lp(g, 24), device=d),
                                    lambda g, b: b.general_work(NF, _z(NF, np.float32))),
    "rational_resampler_base_ccc": (lambda g, d: g.rational_resampler_base_ccc(3, 2, _lp(g, 24).astype(np.complex64), device=d),
                                    lambda g, b: b.general_work(NC, _z(NC, np.complex64))),
    "pfb_interpolator_ccf": (lambda g, d: g.pfb_interpolator_ccf(4, _lp(g, 32), device=d),
                             lambda g, b: b.work(NC, _z(NC // 4 + 32, np.complex64))),
    "pfb_synthesis_filterbank_ccf": (lambda g, d: g.pfb_synthesis_filterbank_ccf(4, _lp(g, 32), device=d),
                                     lambda g, b: b.work(NC, [_z(NC // 4 + 32, np.complex64)] * 4)),
    # d_demod and d_soft: 8 captures x 150 064 floats = 4.6 MiB each
    "dmr_chain": (lambda g, d: _chain(g, d), _chain_use),
}
# the copy adapters own a stream and nothing on the device (their host entry is a memcpy): no buffer to lose
OWNS_NOTHING = ("stream_to_vector", "head")


def _drop(g, b):
    """destroy now, not when the garbage collector gets to it"""
    b.__del__()
    assert not b._h


def _failed_create(g, make, dev):
    """run make(g, dev), which must fail: the error, and the handle the constructor was filling"""
    seen = []
    blk = g.binding._Block
    orig = blk.__init__

    def spy(self):
        orig(self)
        seen.append(self)
    blk.__init__ = spy
    try:
        with pytest.raises(g.GrhipError) as ei:
            make(g, dev)
    finally:
        blk.__init__ = orig
    assert seen, "the constructor made no handle object"
    return ei.value, seen[-1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_failed_create_leaves_nothing(gpu, name):
    make, use = CASES[name]
    ndev = gpu.device_count()
    err, obj = _failed_create(gpu, make, ndev)
    assert err.code < 0
    assert not obj._h, "a failed create handed out a handle"
    assert "out of range [0,%d)" % ndev in str(err), str(err)
    b = make(gpu, 0)                    # the same type still works
    assert b._h
    _drop(gpu, b)


def test_failed_create_after_the_stream_dmr_chain(gpu):
    """no taps: the argument checks pass, init_device makes the stream, and the FIR engines then refuse the shape"""
    err, obj = _failed_create(gpu, lambda g, d: _chain(g, d, taps=np.zeros(0, np.complex64), S=2, n=4096), 0)
    assert err.code < 0
    assert not obj._h
    b = _chain(gpu, 0, S=2, n=4096)
    assert b._h
    _drop(gpu, b)


def test_failed_create_after_the_stream_pfb_decimator(gpu):
    """1025 taps for one filter: init_device makes the stream, the rotators are allocated and uploaded, and set_taps
    then refuses more than 1024 taps per filter; destroy_handle takes down a handle with a stream and a buffer"""
    err, obj = _failed_create(gpu, lambda g, d: g.pfb_decimator_ccf(1, np.ones(1025, np.float32), 0, device=d), 0)
    assert err.code < 0
    assert not obj._h
    assert "more than 1024 taps per filter" in str(err), str(err)
    b = gpu.pfb_decimator_ccf(1, np.ones(1024, np.float32), 0, device=0)
    assert b._h
    _drop(gpu, b)


def test_failed_create_after_the_stream_hilbert_fc(gpu):
    """16384 taps pass the entry's check, the block designs ntaps | 1 = 16385 of them (64 KiB), and install, which runs
    after init_device has made the stream, refuses more than 16384"""
    err, obj = _failed_create(gpu, lambda g, d: g.hilbert_fc(16384, device=d), 0)
    assert err.code < 0
    assert not obj._h
    assert "at most 16384 taps" in str(err), str(err)
    b = gpu.hilbert_fc(16383, device=0)
    assert b._h
    _drop(gpu, b)


@pytest.mark.parametrize("name", sorted(set(CASES) - set(OWNS_NOTHING)))
def test_no_leak_per_cycle(gpu, name):
    """K cycles of create, one work call, destroy.  A handle owns S bytes once used; losing them once per cycle would
    lower the free device memory by K S = 128 MiB.  The bound is a quarter of that."""
    import torch
    make, use = CASES[name]
    bound = K * S_BYTES // 4

    def cycle():
        b = make(gpu, 0)
        use(gpu, b)
        _drop(gpu, b)

    cycle()                             # warm-up: tables per device, the cached inputs, the runtime's own pools
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(K):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    drift = free0 - free1
    print("%s: free memory fell by %d bytes over %d cycles (bound %d)" % (name, drift, K, bound))
    assert drift <= bound


@pytest.mark.parametrize("kind", ["ccc", "fff"])
def test_fft_filter_latched_update(gpu, kind):
    """5 taps -> 9 taps at decimation 2: the work call after set_taps installs them and returns 0; from then on the
    filter is a fresh filter with the new taps, bit for bit"""
    import torch
    rng = np.random.default_rng(0x4C41)
    cplx = kind == "ccc"
    cls = getattr(gpu, "fft_filter_" + kind)

    def rnd(n):
        v = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        return v.view(np.complex64).reshape(n) if cplx else v[:, 0].copy()

    t5, t9 = rnd(5), rnd(9)
    n = 2400                                        # a multiple of both nsamples: 12 (5 taps) and 24 (9 taps)
    x = rnd(2 * n)
    dev = torch.device("cuda", 0)
    tdt = torch.complex64 if cplx else torch.float32
    d_in = torch.from_numpy(x).to(dev)
    d_out = torch.zeros(n, dtype=tdt, device=dev)
    d_ref = torch.zeros(n, dtype=tdt, device=dev)
    st = torch.cuda.Stream(device=dev)
    f = cls(2, t5)
    assert f.nsamples() == 12
    assert f.work_device(n, d_in, d_out, st) == n   # a launch with the old taps is queued on the caller's stream
    f.set_taps(t9)
    assert f.work_device(n, d_in, d_out, st) == 0
    assert f.nsamples() == 24
    assert f.work_device(n, d_in, d_out, st) == n
    fresh = cls(2, t9)
    assert fresh.work_device(n, d_in, d_ref, st) == n
    st.synchronize()
    assert bits_equal(d_out.cpu().numpy(), d_ref.cpu().numpy())


def test_fft_vcc_set_window(gpu):
    N, nvec = 64, 4
    rng = np.random.default_rng(0x57494E)
    xr = rng.uniform(-1, 1, size=nvec * N).astype(np.float32)
    w = (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(N) / (N - 1))).astype(np.float32)
    f = gpu.fft_vcc(N, True, None, False)
    y0 = f.work(nvec, xr.astype(np.complex64)).copy()
    assert f.set_window(np.zeros(0, np.float32)) is True            # length 0: accepted, still no window
    assert bits_equal(f.work(nvec, xr.astype(np.complex64)), y0)
    assert f.set_window(w) is True                                  # length N: accepted and applied
    y1 = f.work(nvec, xr.astype(np.complex64)).copy()
    assert not bits_equal(y1, y0)
    # ... as fft_vfc applies it to the floats: one body, so value for value (as
    # tests/test_gpu_fft_real.py compares the two), and within the 1e-6 log2(N) of the exact transform that
    # tests/test_gpu_fft_pfb.py asks
    ref = gpu.fft_vfc(N, True, w).work(nvec, xr)
    assert np.array_equal(y1, ref)
    exact = np.fft.fft((xr.astype(np.float64) * np.tile(w.astype(np.float64), nvec)).reshape(nvec, N), axis=1).reshape(-1)
    assert rel_err_max(y1, exact) <= 1e-6 * np.log2(N)
    assert f.set_window(np.ones(3, np.float32)) is False            # any other length: refused, nothing changes
    assert bits_equal(f.work(nvec, xr.astype(np.complex64)), y1)
