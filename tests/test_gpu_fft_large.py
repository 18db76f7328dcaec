"""-m gpu parity tests: gr_fft_vcc above 2^20 points, every register kernel as an in-place leg of the four-step and
Bluestein forms, the chunk loops of FftPlan, and gr_fft_filter_ccc above fftsize 32768.

Reference: test_gpu_fft_pfb._dft64 (np.fft on complex128 with the reference block's window and shift rules), one vector at
a time so that host memory stays bounded.  Bound: the project's 1e-6 * log2 N of the vector's spectral peak, per vector.
Every case prints the worst vector's error and its share of the bound (pytest -s shows them; DESIGN.md 4.5 has the table)."""
import numpy as np
import pytest

from test_gpu_fft_pfb import _dft64, _rc

pytestmark = pytest.mark.gpu

# (forward, shift, window) as test_fft_any_size_window_and_shift
COMBOS = [(True, True, False), (False, True, False), (True, False, True), (False, True, True), (True, True, True)]
BOTH = (True, False)
FWD = (True,)


def _inputs(seed, N, nvec):
    rng = np.random.default_rng(seed)
    x = np.empty(N * nvec, np.complex64)
    for v in range(nvec):                                  # (per vector: _rc's float64 temporaries stay N long)
        x[v * N:(v + 1) * N] = _rc(rng, N)
    return x


def _check_vectors(what, got, x, N, nvec, forward, w=None, shift=False):
    """every vector on its own against _dft64: max|got - ref| / max|ref| <= 1e-6 log2 N; the message names the worst vector"""
    assert got.shape == (N * nvec,)
    err = np.empty(nvec)
    for v in range(nvec):
        ref = _dft64(x[v * N:(v + 1) * N], N, forward, w, shift)
        err[v] = np.abs(got[v * N:(v + 1) * N] - ref).max() / np.abs(ref).max()
    bound = 1e-6 * np.log2(N)
    print("\nfft_large %s N=%d nvec=%d forward=%d shift=%d window=%d: worst vector %d, error %.3g = %.3f of the bound %.3g"
          % (what, N, nvec, forward, shift, w is not None, int(err.argmax()), err.max(), err.max() / bound, bound))
    assert err.max() <= bound, (int(err.argmax()), float(err.max()), [int(i) for i in np.flatnonzero(err > bound)[:8]])


def _case_list(rows):
    return [pytest.param(N, nvec, f, id="%d-%d-%s" % (N, nvec, "fwd" if f else "bwd")) for N, nvec, dirs in rows for f in dirs]


# ---- 1. four-step legs: N = N1 N2, N1 = 2^ceil(lg / 2); both row transforms run in place (S1 -> S1, S2 -> S2) -------------
FOURSTEP = [
    (1 << 17, 3, BOTH),     # 512 x 256: fft16x_kernel<512> and <256> in place
    (1 << 18, 2, BOTH),     # 512 x 512: fft16x_kernel<512> in place, both legs
    (1 << 19, 2, BOTH),     # 1024 x 512: fft16x_kernel<1024> and <512> in place
    (1 << 21, 2, BOTH),     # 2048 x 1024: fft16x_kernel<2048> and <1024> in place
    (1 << 22, 1, BOTH),     # 2048 x 2048: fft16x_kernel<2048> in place, both legs
    (1 << 23, 2, BOTH),     # 4096 x 2048: fft4096_kernel in place, 2 * 2048 row vectors on at most 4 per CU: persistent walk
                            # with the next vector's points in flight; fft16x_kernel<2048> in place
    (1 << 24, 1, FWD),      # 4096 x 4096: fft4096_kernel in place, both legs; thi has 2048 entries
    (1 << 25, 1, BOTH),     # 8192 x 4096: fft8192_kernel and fft4096_kernel in place; chunk == 1
    (1 << 26, 1, FWD),      # 8192 x 8192: fft8192_kernel in place, both legs; chunk = 2^25 / N = 0 clamped to 1; m = r c up to 2^26
]


@pytest.mark.parametrize("N,nvec,forward", _case_list(FOURSTEP))
def test_fft_four_step_legs(gpu, N, nvec, forward):
    x = _inputs(N + 3 * int(forward), N, nvec)
    got = gpu.fft_vcc(N, forward, [], False).work(nvec, x)
    _check_vectors("four-step", got, x, N, nvec, forward)


# ---- 2. the chunk loop of FftPlan::exec_pow2 ----------------------------------------------------------------------------
def test_fft_four_step_chunk_seam(gpu):
    """N = 2^21 (2048 x 1024): chunk = 2^25 / N = 16 vectors per pass, so the 17th goes through a second, short pass whose
    v0 offsets on in and out nothing else exercises; a wrong offset shows as vector 16 (or 0) in the message"""
    N, nvec = 1 << 21, 17
    x = _inputs(21017, N, nvec)
    got = gpu.fft_vcc(N, True, [], False).work(nvec, x)
    _check_vectors("chunk seam", got, x, N, nvec, True)


# ---- 3. window and shift in the transposes at large N ---------------------------------------------------------------------
@pytest.mark.parametrize("N,nvec,forward,shift,win",
                         [(1 << 17, 2) + c for c in COMBOS] +      # 512 x 256: window[n], both N / 2 shifts, thi of 16 entries
                         [(1 << 23, 1) + c for c in COMBOS[:2]])   # 4096 x 2048: the first size where the shifts (MODE 0 backward,
                                                                   # MODE 2 forward) meet the fft4096_kernel leg
def test_fft_four_step_window_and_shift(gpu, N, nvec, forward, shift, win):
    x = _inputs(17 + N + int(forward) + 2 * int(win), N, nvec)
    w = np.hamming(N).astype(np.float32) if win else None
    blk = gpu.fft_vcc(N, forward, w if win else [], shift)
    got = blk.work(nvec, x)
    _check_vectors("four-step window/shift", got, x, N, nvec, forward, w, shift)
    assert blk.set_window(np.ones(N - 1, np.float32)) is False
    assert blk.set_window(np.ones(N, np.float32)) is True


# ---- 4. Bluestein legs: L = the power of two >= 2 N - 1; the sub-plan runs S -> S --------------------------------------------
BLUESTEIN = [
    (300, 9, BOTH),            # L = 1024: fft16x_kernel<1024> in place
    (1500, 7, BOTH),           # L = 4096: fft4096_kernel in place on the scratch buffer
    (3000, 5, BOTH),           # L = 8192: fft8192_kernel in place on the scratch buffer
    (40000, 3, BOTH),          # L = 2^17: four-step sub-plan, 512 x 256
    ((1 << 20) + 1, 2, BOTH),  # L = 2^22: four-step sub-plan, 2048 x 2048
    (3_000_001, 1, FWD),       # L = 2^23: four-step sub-plan S -> S, 4096 x 2048 through fft4096_kernel in place
]


@pytest.mark.parametrize("N,nvec,forward", _case_list(BLUESTEIN))
def test_fft_bluestein_legs(gpu, N, nvec, forward):
    x = _inputs(N + 3 * int(forward), N, nvec)
    got = gpu.fft_vcc(N, forward, [], False).work(nvec, x)
    _check_vectors("Bluestein", got, x, N, nvec, forward)


@pytest.mark.parametrize("forward,shift,win", COMBOS)
@pytest.mark.parametrize("N", [1501,      # L = 4096, fft4096_kernel in place; odd N: the shifts are floor(N/2) in, ceil(N/2) out
                               3001])     # L = 8192, fft8192_kernel in place
def test_fft_bluestein_window_and_shift(gpu, N, forward, shift, win):
    nvec = 3
    x = _inputs(17 + N + int(forward) + 2 * int(win), N, nvec)
    w = np.hamming(N).astype(np.float32) if win else None
    blk = gpu.fft_vcc(N, forward, w if win else [], shift)
    got = blk.work(nvec, x)
    _check_vectors("Bluestein window/shift", got, x, N, nvec, forward, w, shift)
    assert blk.set_window(np.ones(N - 1, np.float32)) is False
    assert blk.set_window(np.ones(N, np.float32)) is True


def test_fft_bluestein_chunk_seam_four_step_sub_plan(gpu):
    """N = 12000: L = 32768 (four-step sub-plan, 256 x 128), chunk = 2^25 / L = 1024 vectors per pass; the 1025th vector goes
    through a second pass of one vector (v0 offsets on in and out, the scratch buffer from its start again)"""
    N, nvec = 12000, 1025
    x = _inputs(12000 + 1025, N, nvec)
    got = gpu.fft_vcc(N, True, [], False).work(nvec, x)
    _check_vectors("Bluestein chunk seam", got, x, N, nvec, True)


# ---- 5. gr_fft_filter_ccc, batched overlap-add above fftsize 32768 ---------------------------------------------------------------
def _fast_len(n):
    """smallest 2^a 3^b 5^c >= n"""
    best = 1 << int(n - 1).bit_length()
    p5 = 1
    while p5 < best:
        p35 = p5
        while p35 < best:
            m = p35
            while m < n:
                m *= 2
            best = min(best, m)
            p35 *= 3
        p5 *= 5
    return best


def _convolve64(taps, x, nout, decim):
    """y[n] = sum_k taps[k] x[n decim - k], zeros before the stream: one zero-padded float64 np.fft product (no wrap-around
    into the outputs kept: the transform is at least len(x) + len(taps) - 1 long), then decimated"""
    m = _fast_len(len(x) + len(taps) - 1)
    X = np.fft.fft(x.astype(np.complex128), m)
    X *= np.fft.fft(taps.astype(np.complex128), m)
    y = np.fft.ifft(X)[:len(x):decim]
    assert len(y) >= nout
    return y[:nout]


@pytest.mark.parametrize("ntaps,decim", [((1 << 17) + 1, 3),      # fftsize 2^19 (1024 x 512), 3 then 6 blocks per call
                                         ((1 << 21) + 1, 1)])     # fftsize 2^23 (4096 x 2048), 1 then 2 blocks per call
def test_fft_filter_ccc_large_fftsize(gpu, ntaps, decim):
    """fftfilt_pack / _mul / _ola / _tail with block offsets b * fftsize beyond 2^19 items and the host's double radix-2
    transform of the taps at these lengths; two calls of ns and 2 ns outputs: the tail crosses a call and blocks inside a call.
    The O(N ntaps) direct form is out of reach here: the same linear convolution by one float64 FFT product"""
    rng = np.random.default_rng(ntaps)
    taps = (_rc(rng, ntaps) / np.sqrt(ntaps)).astype(np.complex64)
    blk = gpu.fft_filter_ccc(decim, taps)
    fftsize = int(2 * 2 ** np.ceil(np.log2(ntaps)))
    ns = blk.nsamples()
    assert ns == fftsize - ntaps + 1 and blk.decimation() == decim
    nout = 3 * ns
    x = _rc(rng, nout * decim)
    got = np.concatenate([blk.work(ns, x[: ns * decim]), blk.work(2 * ns, x[ns * decim:])])
    assert got.shape == (nout,)
    ref = _convolve64(taps, x, nout, decim)
    err = np.abs(got - ref)
    bound = 1e-5 * max(np.abs(ref).max(), 1e-3 * np.abs(taps).sum())
    print("\nfft_large fft_filter_ccc ntaps=%d decim=%d fftsize=%d: worst output %d, error %.3g = %.3f of the bound %.3g"
          % (ntaps, decim, fftsize, int(err.argmax()), err.max(), err.max() / bound, bound))
    assert err.max() <= bound, (int(err.argmax()), float(err.max()))
