"""The continuous-phase transmitter on the device: frequency_modulator_fc, bytes_to_syms, char_to_float,
chunks_to_symbols_bf, cpmmod_bc, gmskmod_bc and gmsk_mod against tests/cpm_ref.py, which tests/test_cpm_cpu.py holds to
tests/golden/ref_cpm.npz, and against the recording itself.

The two contracts of include/grhip.h:
  GENERIC  the phase state equals the restatement's bit for bit across cuts, and so do the outputs (the restatement's
           (float)cos((double)(float)phase)); against the recording, made with glibc's sincosf, one float ulp per component.
  FAST     per work call, from the handle's own entry phase: every output within 1e-5 + 2^-50 Phi of exp(j phi) in
           float64, Phi = sum |sensitivity x| + |entry phase|, and the state within n 2^-53 Phi of GENERIC's from that
           entry phase.
The hier handles' frequency samples are gr_fir_fff_generic's floats in both engines and every mode, so the same two
contracts hold for them with x the restated interpolator's output."""
import numpy as np
import pytest
import torch

import cpm_ref as R
from cpm_ref import same_phases, within_one_ulp

pytestmark = pytest.mark.gpu

FX = R.fixture()
SENS = 0.37


def tile(gpu):
    return gpu.frequency_modulator_fc_tile()


def split(x, chunks):
    """x [S][n] -> per work call the [S][m] block, streams back to back"""
    at, out = 0, []
    for m in chunks:
        out.append(np.ascontiguousarray(x[:, at:at + m]))
        at += m
    return out


def cut_list(n, T):
    return [[n]] + ([[7, n - 7]] if n > 7 else []) + ([[T + 1, n - T - 1]] if n > T + 1 else [])


def check_fast_call(blk, S, x, sens, got, what):
    """one work call already made: x, got [S][m]; entry[s] the phase before it"""
    for s in range(S):
        want, bound, Phi = R.fast_reference(x[s], sens, what["entry"][s])
        err = np.abs(got[s] - want)
        fin = np.isfinite(want)
        assert np.isnan(got[s][~fin].view(np.float32)).all(), what
        assert not fin.any() or err[fin].max() <= bound, (what, s, float(err[fin].max()), bound)
        state = blk.phase(s)
        generic = R.wrap(R.call_phases(x[s], sens, what["entry"][s])[-1])
        if np.isfinite(generic):
            assert abs(state - generic) <= len(x[s]) * 2.0 ** -53 * Phi, (what, s, state, generic)
        else:
            assert not np.isfinite(state), (what, s)


def run_fm(gpu, mode, x, sens, chunks):
    """x [S][n]; returns out [S][n]; checks the contract of `mode` on the way"""
    S, n = x.shape
    blk = gpu.frequency_modulator_fc(sens)
    blk.set_mode(mode)
    if S > 1:
        blk.set_streams(S)
    outs = []
    for part in split(x, chunks):
        entry = [blk.phase(s) for s in range(S)]
        got = blk.work(part).reshape(S, -1)
        if mode != gpu.MODE_GENERIC:
            check_fast_call(blk, S, part, sens, got, dict(n=n, chunks=chunks, entry=entry))
        outs.append(got)
    out = np.concatenate(outs, axis=1)
    if mode == gpu.MODE_GENERIC:
        for s in range(S):
            want, ph = R.freq_mod(x[s], sens, chunks)
            assert int(R.ulps(out[s], want).max()) == 0, (n, chunks, s, int(R.ulps(out[s], want).max()))      # NaN for NaN
            assert same_phases([blk.phase(s)], ph[-1:]), (n, chunks, s)
    return out


@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_frequency_modulator_counts_and_cuts(gpu, mode, S):
    T = tile(gpu)
    rng = np.random.RandomState(11)
    for n in (1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5):
        x = rng.standard_normal((S, n)).astype(np.float32)
        for chunks in cut_list(n, T):
            run_fm(gpu, getattr(gpu, mode), x, SENS, chunks)


@pytest.mark.parametrize("name", ("small", "wrap_pos", "wrap_neg", "const_2p40", "qa"))
def test_frequency_modulator_against_the_recording(gpu, name):
    x, sens = FX["fm_%s_in" % name], float(FX["fm_%s_sens" % name])
    for cut in R.CUTS:
        chunks = R.chunks_of(len(x), cut, 4097)
        if cut == "seven":
            chunks, x1 = chunks[:60], x[:420]          # calls of 7 through the first wraps; the recording keeps every call's phase
        else:
            x1 = x
        blk = gpu.frequency_modulator_fc(sens)
        blk.set_mode(gpu.MODE_GENERIC)
        outs, phases = [], []
        for part in split(x1[None, :], chunks):
            outs.append(blk.work(part))
            phases.append(blk.phase())
        out = np.concatenate(outs)
        key = "fm_%s_%s" % (name, cut)
        assert same_phases(phases, FX[key + "_phases"][:len(phases)]), key
        m = min(len(out), R.KEEP)
        assert int(R.ulps(out[:m], FX[key + "_head"][:m]).max()) <= 1, key
        if cut != "seven":
            assert within_one_ulp(out, key), key
        run_fm(gpu, gpu.MODE_FAST, x1[None, :], sens, chunks)


@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_non_finite_input_stays_in_its_stream(gpu, mode):
    T = tile(gpu)
    for n, at in ((300, 150), (2 * T + 100, T + 37)):
        for bad in (np.nan, np.inf):
            x = np.random.RandomState(3).standard_normal((3, n)).astype(np.float32)
            x[1, at] = bad
            out = run_fm(gpu, getattr(gpu, mode), x, SENS, [n])
            assert np.isfinite(out[0].view(np.float32)).all() and np.isfinite(out[2].view(np.float32)).all()
            assert np.isfinite(out[1, :at].view(np.float32)).all() and np.isnan(out[1, at:].view(np.float32)).all(), (n, bad)


def test_set_sensitivity_between_calls(gpu):
    x = FX["fm_wrap_pos_in"]
    blk = gpu.frequency_modulator_fc(0.1)
    blk.set_mode(gpu.MODE_GENERIC)
    a = blk.work(x[:4097])
    p0 = blk.phase()
    blk.set_sensitivity(0.3)
    assert blk.sensitivity() == float(np.float32(0.3))              # the float of .h:52
    b = blk.work(x[4097:])
    assert same_phases([p0, blk.phase()], FX["fm_setsens_phases"]) and within_one_ulp(np.concatenate((a, b)), "fm_setsens")
    fast = gpu.frequency_modulator_fc(0.1)
    fast.work(x[:4097])
    fast.set_sensitivity(0.3)
    entry = fast.phase()
    got = fast.work(x[4097:])
    check_fast_call(fast, 1, x[None, 4097:], np.float64(np.float32(0.3)), got[None, :], dict(entry=[entry]))
    fast.set_phase(1.25)
    assert fast.phase() == 1.25


@pytest.mark.parametrize("scale", (2.0 ** -40, 2.0 ** 15))
def test_frequency_modulator_over_the_float_range(gpu, scale):
    T = tile(gpu)
    x = (scale * np.random.RandomState(5).standard_normal((1, T + 300))).astype(np.float32)
    for mode in (gpu.MODE_GENERIC, gpu.MODE_FAST):
        run_fm(gpu, mode, x, SENS, [T + 300])
        run_fm(gpu, mode, x, SENS, [100, T + 200])


@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_pointers_one_item_off_a_16_byte_boundary(gpu, mode):
    T = tile(gpu)
    n = T + 77
    x = np.random.RandomState(6).standard_normal(n).astype(np.float32)
    want = None
    for off_in in (0, 1):
        for off_out in (0, 1):
            d_in = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
            d_out = torch.full((n + 8,), float("nan"), dtype=torch.complex64, device="cuda")
            assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
            d_in[off_in:off_in + n] = torch.from_numpy(x)
            blk = gpu.frequency_modulator_fc(SENS)
            blk.set_mode(getattr(gpu, mode))
            torch.cuda.synchronize()
            blk.work_device(n, d_in[off_in:], d_out[off_out:])
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert np.isnan(got[:off_out].real).all() and np.isnan(got[off_out + n:].real).all()       # the guards are (nan, 0)
            if want is None:
                want = run_fm(gpu, getattr(gpu, mode), x[None, :], SENS, [n])[0]
            assert np.array_equal(got[off_out:off_out + n].view(np.uint32), want.view(np.uint32)), (off_in, off_out)


@pytest.mark.parametrize("S", (1, 3))
def test_small_blocks(gpu, S):
    b = FX["small_in"]
    for n in (1, 7, 257):
        x = np.stack([np.roll(b, 31 * s)[:n] for s in range(S)])
        for mode in (gpu.MODE_FAST, gpu.MODE_GENERIC):
            for blk, ref in ((gpu.bytes_to_syms(), R.bytes_to_syms), (gpu.char_to_float(), R.char_to_float)):
                blk.set_mode(mode)
                blk.set_streams(S)
                assert np.array_equal(blk.work(x).view(np.uint32), np.concatenate([ref(r) for r in x]).view(np.uint32)), (n, blk._name)
    assert np.array_equal(gpu.bytes_to_syms().work(b).view(np.uint32), FX["b2s_out"].view(np.uint32))
    assert np.array_equal(gpu.char_to_float().work(b).view(np.uint32), FX["c2f_out"].view(np.uint32))
    for D in (1, 2, 3):
        blk = gpu.chunks_to_symbols_bf(FX["c2s_table"], D)
        blk.set_streams(S)
        for n in (1, 7, 257):
            x = np.stack([np.roll(FX["c2s_in_D%d" % D], 5 * s)[:n] for s in range(S)])
            want = np.concatenate([R.chunks_to_symbols_bf(r, FX["c2s_table"], D) for r in x])
            assert np.array_equal(blk.work(x).view(np.uint32), want.view(np.uint32)), (D, n)
        assert np.array_equal(gpu.chunks_to_symbols_bf(FX["c2s_table"], D).work(FX["c2s_in_D%d" % D]).view(np.uint32), FX["c2s_out_D%d" % D].view(np.uint32))
    # an index whose D entries do not lie inside the table gives zeros
    got = gpu.chunks_to_symbols_bf(FX["c2s_table"], 5).work(np.array([0, 1, 2, 3, 255], np.uint8))
    assert np.array_equal(got[:10], FX["c2s_table"][:10]) and not got[10:].any()


# ---- the hier handles --------------------------------------------------------------------------------------------------------
def run_hier(gpu, blk, restated, items, chunks, S=1):
    """items [S][n] bytes; runs the handle and the restated chain call by call; returns (out, freq) [S][..] of the handle"""
    outs, freqs = [], []
    chains = [restated() for _ in range(S)]
    generic = blk.engine() == 0 and blk._generic
    for part in split(items, chunks):
        entry = [blk.phase(s) for s in range(S)]
        out, freq = blk.work(part, want_freq=True)
        out, freq = out.reshape(S, -1), freq.reshape(S, -1)
        for s in range(S):
            w_out, w_freq = chains[s].work(part[s])
            assert np.array_equal(freq[s].view(np.uint32), w_freq.view(np.uint32)), ("freq", chunks, s)
            if generic:
                assert np.array_equal(out[s].view(np.uint32), w_out.view(np.uint32)), ("out", chunks, s)
                assert same_phases([blk.phase(s)], [chains[s].phase]), ("phase", chunks, s)
        if not generic:
            check_fast_call(blk, S, freq, chains[0].sens, out, dict(chunks=chunks, entry=entry))
            for s in range(S):
                chains[s].phase = np.float64(blk.phase(s))         # the next call is judged from the handle's own entry phase
        outs.append(out)
        freqs.append(freq)
    return np.concatenate(outs, axis=1), np.concatenate(freqs, axis=1)


def make_hier(gpu, ctor, mode, engine=None, S=1):
    blk = ctor()
    blk.set_mode(mode)
    blk._generic = mode == gpu.MODE_GENERIC
    if engine is not None:
        blk.set_engine(engine)
    if S > 1:
        blk.set_streams(S)
    return blk


@pytest.mark.parametrize("shape", ((2, 1), (3, 5), (8, 4), (10, 1)))
@pytest.mark.parametrize("type", range(5))
def test_cpmmod_bc_tile_edges(gpu, type, shape):
    sps, L = shape
    T = gpu.cpmmod_bc.tile()
    h, beta = 0.5, 0.3
    taps = gpu.cpm_phase_response(type, sps, L, beta)
    restated = lambda: R.Chain(taps, sps, R.cpm_sensitivity(h))
    ctor = lambda: gpu.cpmmod_bc(type, h, sps, L, beta)
    rng = np.random.RandomState(100 * type + sps)
    for nsym in range(-(-T // sps) - 1, -(-T // sps) + 2):
        sym = rng.randint(-128, 128, (1, nsym)).astype(np.int8)
        sym[0, :2] = (127, -128)
        items = sym.view(np.uint8)
        e1 = make_hier(gpu, ctor, gpu.MODE_FAST)
        assert e1.engine() == 1
        out1, _ = run_hier(gpu, e1, restated, items, [nsym])
        e0 = make_hier(gpu, ctor, gpu.MODE_FAST, 0)
        assert e0.engine() == 0
        out0, freq0 = run_hier(gpu, e0, restated, items, [nsym])
        bound = R.fast_reference(freq0[0], R.cpm_sensitivity(h), 0.0)[1]
        assert np.abs(out0 - out1).max() <= bound, (nsym, float(np.abs(out0 - out1).max()), bound)
        gen = make_hier(gpu, ctor, gpu.MODE_GENERIC)
        assert gen.engine() == 0
        run_hier(gpu, gen, restated, items, [nsym])
    # cuts that leave tile edges inside symbols and calls shorter than the history, both engines and GENERIC
    nsym = 2 * (-(-T // sps)) + 3
    items = rng.randint(-128, 128, (1, nsym)).astype(np.int8).view(np.uint8)
    for chunks in ([1, 2, L, nsym - 3 - L], [nsym - 5, 5]):
        run_hier(gpu, make_hier(gpu, ctor, gpu.MODE_FAST), restated, items, chunks)
        run_hier(gpu, make_hier(gpu, ctor, gpu.MODE_FAST, 0), restated, items, chunks)
        run_hier(gpu, make_hier(gpu, ctor, gpu.MODE_GENERIC), restated, items, chunks)


def test_cpmmod_bc_is_the_composition_of_the_blocks(gpu):
    """GENERIC: the handle against char_to_float -> interp_fir_filter_fff -> frequency_modulator_fc run one after the other
    on the device, bit for bit, whatever the cuts"""
    sym = FX["mod_symbols"]
    for type, sps, L in ((R.GAUSSIAN, 3, 5), (R.LRC, 8, 4)):
        taps = gpu.cpm_phase_response(type, sps, L, 0.3)
        for cut in R.CUTS:
            chunks = R.chunks_of(len(sym), cut, 97)
            blk = make_hier(gpu, lambda: gpu.cpmmod_bc(type, 0.25, sps, L, 0.3), gpu.MODE_GENERIC)
            c2f, fir, fm = gpu.char_to_float(), gpu.interp_fir_filter_fff(sps, taps), gpu.frequency_modulator_fc(R.cpm_sensitivity(0.25))
            for b in (c2f, fir, fm):
                b.set_mode(gpu.MODE_GENERIC)
            hist = np.zeros(L - 1, np.float32)
            at = 0
            for m in chunks:
                got, freq = blk.work(sym[at:at + m], want_freq=True)
                x = np.concatenate((hist, c2f.work(sym[at:at + m])))
                f = fir.work(m * sps, x)
                want = fm.work(f)
                hist = x[len(x) - (L - 1):]
                assert np.array_equal(freq.view(np.uint32), f.view(np.uint32)) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (type, cut, at)
                assert blk.phase() == fm.phase()
                at += m


@pytest.mark.parametrize("cut", R.CUTS)
def test_hier_against_the_recording(gpu, cut):
    for i, (t, sps, L, beta, h) in enumerate(FX["cpm_cases"]):
        blk = make_hier(gpu, lambda: gpu.cpmmod_bc(int(t), h, int(sps), int(L), beta), gpu.MODE_GENERIC)
        outs, freqs, phases, at = [], [], [], 0
        for m in R.chunks_of(600, cut, 97):
            o, f = blk.work(FX["mod_symbols"][at:at + m], want_freq=True)
            outs.append(o); freqs.append(f); phases.append(blk.phase())
            at += m
        key = "cpm_%d_%s" % (i, cut)
        assert R.digest(np.concatenate(freqs)) == str(FX[key + "_freq_sha"]) and same_phases(phases, FX[key + "_phases"]), key
        assert within_one_ulp(np.concatenate(outs), key), key
    for i, (sps, bt) in enumerate(FX["gmsk_cases"]):
        blk = make_hier(gpu, lambda: gpu.gmsk_mod(int(sps), bt), gpu.MODE_GENERIC)
        outs, freqs, phases, at = [], [], [], 0
        for m in R.chunks_of(75, cut, 37):
            o, f = blk.work(FX["mod_bytes"][at:at + m], want_freq=True)
            outs.append(o); freqs.append(f); phases.append(blk.phase())
            at += m
        key = "gmsk_%d_%s" % (i, cut)
        assert R.digest(np.concatenate(freqs)) == str(FX[key + "_freq_sha"]) and same_phases(phases, FX[key + "_phases"]), key
        assert within_one_ulp(np.concatenate(outs), key), key


@pytest.mark.parametrize("sps", (2, 4))
def test_gmskmod_bc_and_gmsk_mod(gpu, sps):
    T = gpu.cpmmod_bc.tile()
    rng = np.random.RandomState(sps)
    S = 3
    # gmskmod_bc: symbols, three streams
    taps = gpu.cpm_phase_response(R.GAUSSIAN, sps, 4, 0.3)
    assert np.array_equal(gpu.gmskmod_bc(sps).taps(), taps)
    nsym = T // sps + 5
    items = (2 * rng.randint(0, 2, (S, nsym)) - 1).astype(np.int8).view(np.uint8)
    for mode, engine in ((gpu.MODE_FAST, None), (gpu.MODE_FAST, 0), (gpu.MODE_GENERIC, None)):
        for chunks in ([nsym], [7, nsym - 7]):
            run_hier(gpu, make_hier(gpu, lambda: gpu.gmskmod_bc(sps, 0.3, 4), mode, engine, S), lambda: R.Chain(taps, sps, R.cpm_sensitivity(0.5)), items, chunks, S)
    # gmsk_mod: bytes
    taps = gpu.gmsk_mod_taps(sps, 0.35)
    assert np.array_equal(gpu.gmsk_mod(sps).taps(), taps) and gpu.gmsk_mod(sps).items_out() == 8 * sps
    nbytes = T // (8 * sps) + 3
    items = rng.randint(0, 256, (S, nbytes)).astype(np.uint8)
    for mode, engine in ((gpu.MODE_FAST, None), (gpu.MODE_FAST, 0), (gpu.MODE_GENERIC, None)):
        for chunks in ([nbytes], [1, 1, nbytes - 2]):
            blk = make_hier(gpu, lambda: gpu.gmsk_mod(sps, 0.35), mode, engine, S)
            assert blk.engine() == (1 if mode == gpu.MODE_FAST and engine is None else 0)
            run_hier(gpu, blk, lambda: R.Chain(taps, sps, R.gmsk_sensitivity(sps), True), items, chunks, S)


def test_engine_limits_and_device_output(gpu):
    big = gpu.cpmmod_bc(R.LREC, 0.5, 2, 17)                         # 17 taps per filter: engine 0 only
    assert big.engine() == 0
    with pytest.raises(gpu.GrhipError):
        big.set_engine(1)
    sym = FX["mod_symbols"][:100]
    restated = R.Chain(gpu.cpm_phase_response(R.LREC, 2, 17), 2, R.cpm_sensitivity(0.5))
    out, freq = big.work(sym, want_freq=True)
    w_out, w_freq = restated.work(sym)
    assert np.array_equal(freq.view(np.uint32), w_freq.view(np.uint32))
    assert np.abs(out - R.fast_reference(w_freq, restated.sens, 0.0)[0]).max() <= R.fast_reference(w_freq, restated.sens, 0.0)[1]
    # device buffers, without the optional frequency output
    blk = gpu.cpmmod_bc(R.GAUSSIAN, 0.5, 4, 4)
    d_in = torch.from_numpy(sym.copy()).cuda()
    d_out = torch.full((400 + 2,), float("nan"), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    blk.work_device(100, d_in, d_out[1:])
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.isnan(got[0].real) and np.isnan(got[-1].real)
    assert np.array_equal(got[1:-1].view(np.uint32), gpu.cpmmod_bc(R.GAUSSIAN, 0.5, 4, 4).work(sym).view(np.uint32))
