"""GPU tests of pfb_synthesis_filterbank_ccf and pfb_interpolator_ccf against tests/pfb_synth_ref.py: parity in both
modes, GENERIC pinned exactly where the DFT is exact, the call contract (splits, set_taps, history), the device entry,
refusals, the round trip through the channeliser on the device, and the C++ blocks under the stand-in executor."""
import os
import subprocess

import numpy as np
import pytest

import pfb_synth_ref as sr
from conftest import bits_equal, rel_err_max

pytestmark = pytest.mark.gpu
c64 = np.complex64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")
TOL = 1e-5          # the project's PFB tolerance (test_pfb_vs_oracle): of the reference's peak
MAX_CHANS = 256     # include/grhip.h


def _noise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(c64)


def _taps(rng, n):
    return (rng.standard_normal(n) / np.sqrt(n)).astype(np.float32)


def _shapes():
    """(M, tpf, ntaps, numsigs): the whole grid, without what the in-range rule excludes"""
    out = []
    for M in (1, 2, 3, 4, 5, 7, 8, 12, 16, 32, 64):
        for tpf in sorted({max(M - 1, 1), 16, 32, 33, 64, 128}):
            for ns in sorted({1, max(1, M // 2), max(1, M - 1), M} | ({5} if M == 7 else set())):
                if sr.in_range(M, tpf, ns):
                    ragged = M * tpf - ((tpf + ns) % M if tpf > 1 else 0)
                    out.append((M, tpf, ragged, ns))
    return out


@pytest.mark.parametrize("mode", ["generic", "fast"])
def test_parity(gpu, mode):
    g = gpu
    rng = np.random.default_rng(11)
    shapes = _shapes()
    assert {s[0] for s in shapes} == {1, 2, 3, 4, 5, 7, 8, 12, 16, 32, 64}
    worst = (0.0, None)
    for idx, (M, tpf, ntaps, ns) in enumerate(shapes):
        taps = _taps(rng, ntaps)
        assert -(-ntaps // M) == tpf
        blk = g.pfb_synthesis_filterbank_ccf(M, taps)
        blk.set_mode(g.MODE_GENERIC if mode == "generic" else g.MODE_FAST)
        assert blk.taps_per_filter() == tpf and blk.history() == tpf + 1
        nvec = (37, 512, 700, 1500)[idx % 4]            # below, at and above one 512-vector tile
        xs = [_noise(rng, nvec) for _ in range(ns)]
        got = blk.work(nvec * M, [sr.with_history(x, tpf) for x in xs])
        ref = sr.whole_literal(M, taps, xs)
        assert got.shape == ref.shape
        e = rel_err_max(got, ref)
        if e > worst[0]:
            worst = (e, (M, tpf, ntaps, ns, nvec))
        assert e < TOL, (M, tpf, ntaps, ns, nvec, e)
    print("%s: %d shapes, worst %.3g of the peak at %s" % (mode, len(shapes), worst[0], worst[1]))


@pytest.mark.parametrize("mode", ["generic", "fast"])
def test_parity_2_20_vectors(gpu, mode):
    g = gpu
    rng = np.random.default_rng(12)
    M, tpf, nvec = 8, 32, 1 << 20
    taps = _taps(rng, M * tpf - 3)
    xs = [_noise(rng, nvec) for _ in range(M)]
    blk = g.pfb_synthesis_filterbank_ccf(M, taps)
    blk.set_mode(g.MODE_GENERIC if mode == "generic" else g.MODE_FAST)
    got = blk.work(nvec * M, [sr.with_history(x, tpf) for x in xs])
    ref = sr.whole_literal(M, taps, xs)
    e = rel_err_max(got, ref)
    print("2^20 vectors, %s: %.3g of the peak" % (mode, e))
    assert e < TOL


@pytest.mark.parametrize("M,tpf", [(1, 7), (2, 16), (3, 5), (4, 33), (7, 16), (8, 32), (12, 9), (16, 128), (32, 16), (64, 3)])
def test_generic_exact_with_one_stream(gpu, M, tpf):
    """one connected stream: every other bin is zero, each DFT output is b[0] exactly, so GENERIC must equal the literal
    loop: this pins the accumulation order (direct, radix-2 and general DFT paths)"""
    g = gpu
    rng = np.random.default_rng(13 * M + tpf)
    taps = _taps(rng, M * tpf - (M - 1))
    x = _noise(rng, 1300)
    blk = g.pfb_synthesis_filterbank_ccf(M, taps)
    blk.set_mode(g.MODE_GENERIC)
    got = blk.work(len(x) * M, [sr.with_history(x, tpf)])
    ref = sr.whole_literal(M, taps, [x])
    assert np.array_equal(got, ref), int(np.count_nonzero(got != ref))


@pytest.mark.parametrize("M", [1, 2, 4])
def test_exact_dft_sizes_integer_data(gpu, M):
    """M = 1, 2, 4: only exact twiddles; integer samples and taps small enough that every sum is exact (|sum| <=
    4 * 8 * 20 * 8 < 2^24): GENERIC and FAST both equal the literal loop"""
    g = gpu
    rng = np.random.default_rng(14 + M)
    tpf = 20
    taps = rng.integers(-8, 9, M * tpf - (M - 1)).astype(np.float32)
    xs = [(rng.integers(-8, 9, 900) + 1j * rng.integers(-8, 9, 900)).astype(c64) for _ in range(M)]
    ref = sr.whole_literal(M, taps, xs)
    assert np.array_equal(ref, sr.closed_form(M, taps, xs).astype(c64))
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        blk = g.pfb_synthesis_filterbank_ccf(M, taps)
        blk.set_mode(mode)
        got = blk.work(len(xs[0]) * M, [sr.with_history(x, tpf) for x in xs])
        assert np.array_equal(got, ref), mode


@pytest.mark.parametrize("M,tpf,ns", [(8, 32, 8), (7, 16, 5), (3, 700, 3), (16, 700, 16), (32, 33, 17), (1, 9, 1),
                                      (16, 15, 16), (4, 513, 4)])
def test_call_splits(gpu, M, tpf, ns):
    """a stream cut at random multiples of M equals one call: bit for bit in GENERIC, within tolerance in FAST
    ((3, 700), (16, 700): branches too long for the fused kernel, and (32, ..), (1, ..): the general path)"""
    g = gpu
    rng = np.random.default_rng(15 * M + tpf)
    taps = _taps(rng, M * tpf - 1 if M > 1 else tpf)
    N = 4000
    xs = [_noise(rng, N) for _ in range(ns)]
    bufs = [sr.with_history(x, tpf) for x in xs]
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        one = g.pfb_synthesis_filterbank_ccf(M, taps)
        one.set_mode(mode)
        whole = one.work(N * M, bufs)
        blk = g.pfb_synthesis_filterbank_ccf(M, taps)
        blk.set_mode(mode)
        outs, rd = [], 0
        r2 = np.random.default_rng(99)
        while rd < N:
            n = int(min(N - rd, r2.choice([1, 3, 17, 100, 511, 512, 513, 1200])))
            outs.append(blk.work(n * M, [b[rd:rd + n + tpf] for b in bufs]))
            assert len(outs[-1]) == n * M
            rd += n
        cut = np.concatenate(outs)
        if mode == g.MODE_GENERIC:
            assert bits_equal(cut, whole)
        else:
            assert rel_err_max(cut, whole) < TOL
        assert rel_err_max(whole, sr.whole_literal(M, taps, xs)) < TOL


@pytest.mark.parametrize("M,tpf,ns", [(8, 32, 8), (5, 16, 3), (32, 31, 32), (1, 4, 1)])
def test_device_entry_equals_host_entry(gpu, M, tpf, ns):
    import torch
    g = gpu
    rng = np.random.default_rng(16 * M)
    taps = _taps(rng, M * tpf)
    N = 3000
    xs = [_noise(rng, N) for _ in range(ns)]
    bufs = np.stack([sr.with_history(x, tpf) for x in xs])              # [ns][N + tpf]
    for mode in (g.MODE_GENERIC, g.MODE_FAST):
        host = g.pfb_synthesis_filterbank_ccf(M, taps)
        host.set_mode(mode)
        dev = g.pfb_synthesis_filterbank_ccf(M, taps)
        dev.set_mode(mode)
        stride = N + tpf + 5
        d_in = torch.zeros((ns, stride), dtype=torch.complex64, device="cuda")
        d_in[:, :N + tpf] = torch.from_numpy(bufs).cuda()
        d_out = torch.zeros(N * M, dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        h_out, rd = [], 0
        s = torch.cuda.Stream()
        for n in (1000, 7, 1993):
            h_out.append(host.work(n * M, [b[rd:rd + n + tpf] for b in bufs]))
            r = dev.work_device(n * M, d_in.data_ptr() + 8 * rd, stride, ns, d_out.data_ptr() + 8 * rd * M, s)
            assert r == n * M
            rd += n
        s.synchronize()
        assert bits_equal(d_out.cpu().numpy(), np.concatenate(h_out))


def test_set_taps_between_calls(gpu):
    g = gpu
    rng = np.random.default_rng(17)
    M = 4
    t1, t2 = _taps(rng, M * 6), _taps(rng, M * 9 - 2)
    xs = [_noise(rng, 300) for _ in range(M)]
    blk = g.pfb_synthesis_filterbank_ccf(M, t1)
    blk.set_mode(g.MODE_GENERIC)
    ref = sr.SynthRef(M, t1)
    a = [sr.with_history(x, 6)[:106] for x in xs]
    assert rel_err_max(blk.work(100 * M, a), ref.work(100 * M, a)) < TOL
    assert blk.history() == 7
    blk.set_taps(t2)
    ref.set_taps(t2)
    assert blk.history() == 7                                   # latched: nothing changes until the next call
    b = [sr.with_history(x, 6)[100:146] for x in xs]
    assert len(blk.work(40 * M, b)) == 0 and len(ref.work(40 * M, b)) == 0        # returns 0 once
    assert blk.history() == 10 and blk.taps_per_filter() == 9
    seg = [x[91:300] for x in xs]                               # tpf = 9 old items in front of 200 new ones
    got = blk.work(200 * M, seg)
    assert len(got) == 200 * M
    assert rel_err_max(got, ref.work(200 * M, seg)) < TOL
    # zero delay lines: the same as a fresh block with the new taps
    fresh = g.pfb_synthesis_filterbank_ccf(M, t2)
    fresh.set_mode(g.MODE_GENERIC)
    assert bits_equal(got, fresh.work(200 * M, seg))


def test_refusals(gpu):
    g = gpu
    rng = np.random.default_rng(18)
    EINVAL = -1

    def refused(fn):
        with pytest.raises(g.GrhipError) as e:
            fn()
        assert e.value.code == EINVAL, e.value

    refused(lambda: g.pfb_synthesis_filterbank_ccf(4, []))                      # no taps
    refused(lambda: g.pfb_synthesis_filterbank_ccf(0, [1.0]))
    refused(lambda: g.pfb_synthesis_filterbank_ccf(MAX_CHANS + 1, np.ones(4 * (MAX_CHANS + 1))))
    g.pfb_synthesis_filterbank_ccf(MAX_CHANS, np.ones(MAX_CHANS, dtype=np.float32))
    M, tpf = 8, 4                                                               # M - 1 > tpf
    blk = g.pfb_synthesis_filterbank_ccf(M, _taps(rng, M * tpf))
    xs = [sr.with_history(_noise(rng, 64), tpf + M) for _ in range(M + 1)]
    refused(lambda: blk.work(64 * M, xs[:2]))                                   # reads past its input
    refused(lambda: blk.work(64 * M, xs[:M]))
    refused(lambda: blk.work(64 * M, []))                                       # numsigs 0
    refused(lambda: blk.work(64 * M, xs[:M + 1]))                               # numsigs M + 1
    refused(lambda: blk.work(64 * M - 3, xs[:1]))                               # not a multiple of M
    refused(lambda: blk.set_taps([]))
    # nothing was computed or latched: the block still behaves as fresh with one stream
    blk.set_mode(g.MODE_GENERIC)
    x = _noise(rng, 64)
    got = blk.work(64 * M, [sr.with_history(x, tpf)])
    assert np.array_equal(got, sr.SynthRef(M, _taps(np.random.default_rng(18), M * tpf)).work(64 * M, [sr.with_history(x, tpf)]))
    # the device entry refuses the same, and leaves the output alone
    import torch
    d_in = torch.zeros((M, 64 + tpf + M), dtype=torch.complex64, device="cuda")
    d_out = torch.full((64 * M,), 7.0, dtype=torch.complex64, device="cuda")
    refused(lambda: blk.work_device(64 * M, d_in, d_in.shape[1], M, d_out))
    refused(lambda: blk.work_device(64 * M, d_in, d_in.shape[1], 0, d_out))
    refused(lambda: blk.work_device(64 * M + 1, d_in, d_in.shape[1], 1, d_out))
    torch.cuda.synchronize()
    assert bool((d_out == 7.0).all())


def test_round_trip_through_the_channeliser_on_the_device(gpu, wl):
    """synthesis (M = 8, 256 taps) into g.pfb_channelizer_ccf: each input tone comes back in its own channel"""
    import torch
    g = gpu
    M, tpf, N = 8, 32, 4096
    taps = (wl.lowpass_taps(M * tpf, 0.8 / (2 * M), 1.0) * M).astype(np.float32)
    fr = [0.01 * (k + 1) - 0.045 for k in range(M)]
    xs = np.stack([sr.with_history(np.exp(2j * np.pi * fr[k] * np.arange(N)).astype(c64), tpf) for k in range(M)])
    syn = g.pfb_synthesis_filterbank_ccf(M, taps)
    ch = g.pfb_channelizer_ccf(M, taps / M)
    assert ch.history() == tpf + 1
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(xs).cuda()
    # the bank's output, tpf*M zeros in front: de-interleaved it is the channeliser's M streams with their history
    d_y = torch.zeros((tpf + N) * M, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    assert syn.work_device(N * M, d_x, N + tpf, M, d_y.data_ptr() + 8 * tpf * M, s) == N * M
    s.synchronize()
    d_s = d_y.view(tpf + N, M).t().contiguous()                         # stream j item m = y[m*M + j]
    d_o = torch.zeros((N - 1, M), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    assert ch.general_work_device(N - 1, d_s, tpf + N, d_o, s) == 0          # d_updated from the constructor's set_taps
    assert ch.general_work_device(N - 1, d_s, tpf + N, d_o, s) == N - 1
    s.synchronize()
    out = d_o.cpu().numpy()
    seg = out[1000:3000]
    w = np.hanning(len(seg))
    f = np.fft.fftfreq(len(seg))
    for c in range(M):
        F = np.abs(np.fft.fft(seg[:, c] * w)) / w.sum()
        peak = int(np.argmax(F))
        assert abs(f[peak] - fr[c]) < 1.0 / len(seg), (c, f[peak], fr[c])
        assert abs(F[peak] - 1.0) < 0.02
        for k in range(M):
            if k != c:
                assert F[int(np.argmin(np.abs(f - fr[k])))] < 10 ** (-50 / 20.0), (c, k)


# ---- pfb_interpolator_ccf ------------------------------------------------------------------------------------------
def _interp_cases():
    return [(R, n) for R in (1, 2, 3, 4, 5, 8, 32) for n in sorted({1, max(3 * R - 1, 1), 32 * R})]


def test_interpolator_generic_bit_exact(gpu, po):
    g = gpu
    rng = np.random.default_rng(21)
    for R, ntaps in _interp_cases():
        taps = _taps(rng, ntaps)
        x = _noise(rng, 2100)
        blk = g.pfb_interpolator_ccf(R, taps)
        blk.set_mode(g.MODE_GENERIC)
        assert blk.history() == -(-ntaps // R) == blk.taps_per_filter() and blk.interpolation() == R
        buf = np.concatenate([np.zeros(blk.history() - 1, dtype=c64), x])
        got = blk.work(R * len(x), buf)
        assert bits_equal(got, sr.whole_interp(po, R, taps, x)), (R, ntaps)


def test_interpolator_fast_within_tolerance(gpu, po):
    g = gpu
    rng = np.random.default_rng(22)
    for R, ntaps in _interp_cases():
        taps = _taps(rng, ntaps)
        x = _noise(rng, 2100)
        blk = g.pfb_interpolator_ccf(R, taps)
        blk.set_mode(g.MODE_FAST)
        buf = np.concatenate([np.zeros(blk.history() - 1, dtype=c64), x])
        got = blk.work(R * len(x), buf)
        assert rel_err_max(got, sr.whole_interp(po, R, taps, x)) < TOL, (R, ntaps)


def test_interpolator_set_taps_history_output_multiple(gpu, po):
    g = gpu
    rng = np.random.default_rng(23)
    R = 3
    t1, t2 = _taps(rng, 13), _taps(rng, 40)
    x = _noise(rng, 1500)
    blk = g.pfb_interpolator_ccf(R, t1)
    blk.set_mode(g.MODE_GENERIC)
    ref = sr.PfbInterpRef(po, R, t1)
    assert blk.history() == 5 and blk.output_multiple() == 3 and blk.interpolation() == 3
    buf = np.concatenate([np.zeros(4, dtype=c64), x])
    assert bits_equal(blk.work(R * 500, buf[:504]), ref.work(R * 500, buf[:504]))
    blk.set_taps(t2)
    ref.set_taps(t2)
    assert blk.history() == 5                                   # latched: nothing changes until the next call
    assert len(blk.work(R * 10, buf[500:514])) == 0 and len(ref.work(R * 10, buf[500:514])) == 0
    assert blk.history() == 14                                  # ceil(40/3)
    seg = buf[504 - 13:]
    n = len(seg) - 13
    assert bits_equal(blk.work(R * n, seg), ref.work(R * n, seg))
    with pytest.raises(g.GrhipError) as e:
        blk.work(R * 10 + 1, seg)
    assert e.value.code == -1
    with pytest.raises(g.GrhipError):
        g.pfb_interpolator_ccf(4, [])
    # the device entry
    import torch
    d_in = torch.from_numpy(seg).cuda()
    d_out = torch.zeros(R * n, dtype=torch.complex64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    dev = g.pfb_interpolator_ccf(R, t2)
    dev.set_mode(g.MODE_GENERIC)
    assert dev.work_device(R * n, d_in, d_out, s) == R * n
    s.synchronize()
    assert bits_equal(d_out.cpu().numpy(), ref.work(R * n, seg))


# ---- the C++ blocks ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth_exe():
    subprocess.check_call(["make", "-C", HOST, "pfb_synth_test"], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "pfb_synth_test")


def test_cpp_block_properties(gpu, synth_exe):
    r = subprocess.run([synth_exe, "errors"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "errors test: ok" in r.stdout, r.stdout


@pytest.mark.parametrize("M,tpf,ns,mode", [(8, 32, 8, "generic"), (8, 32, 8, "fast"), (7, 16, 5, "generic"),
                                           (4, 9, 1, "generic"), (32, 31, 32, "fast")])
def test_cpp_synthesis_block(gpu, synth_exe, tmp_path, M, tpf, ns, mode):
    """the block driven in 4096-item calls (scheduler-sized), history tpf + 1 in front of every stream"""
    rng = np.random.default_rng(31 * M + tpf)
    taps = _taps(rng, M * tpf - 1)
    N = 5000
    xs = [_noise(rng, N) for _ in range(ns)]
    tp, ip, op = [str(tmp_path / n) for n in ("taps.bin", "in.bin", "out.bin")]
    taps.tofile(tp)
    np.stack(xs).tofile(ip)                                                 # [ns][N]
    r = subprocess.run([synth_exe, "synth", str(M), str(ns), mode, tp, ip, op], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = np.fromfile(op, dtype=c64)
    ref = sr.whole_literal(M, taps, xs)
    # calls of 4096 outputs: whole multiples of M; what is left below one call's worth is still a multiple of M
    assert len(got) == len(ref)
    assert rel_err_max(got, ref) < TOL
    if ns == 1 and mode == "generic":
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("R,ntaps,mode", [(4, 61, "generic"), (3, 40, "fast"), (32, 1024, "generic")])
def test_cpp_interpolator_block(gpu, po, synth_exe, tmp_path, R, ntaps, mode):
    rng = np.random.default_rng(32 * R)
    taps = _taps(rng, ntaps)
    x = _noise(rng, 9000)
    tp, ip, op = [str(tmp_path / n) for n in ("taps.bin", "in.bin", "out.bin")]
    taps.tofile(tp)
    x.tofile(ip)
    r = subprocess.run([synth_exe, "interp", str(R), "1", mode, tp, ip, op], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = np.fromfile(op, dtype=c64)
    ref = sr.whole_interp(po, R, taps, x)
    assert len(got) == len(ref)
    if mode == "generic":
        assert bits_equal(got, ref)
    else:
        assert rel_err_max(got, ref) < TOL
