"""-m gpu: the Mueller & Mueller clock recovery off its steady path.  On a clean signal at unit amplitude every step
of the loop is omega +/- 1 samples forward; a demodulator gain set too high (or noise in front of the loop) makes it
step back, stand still and jump, and a large omega makes every step longer than a kernel's window, ring or FIFO.
These are the regimes in which mm_kernel re-windows, mm_rows_kernel re-seeds its ring, mm_pairs_kernel restarts its
register FIFO and mmcc_kernel runs into its output-buffer limit and its clamp at 0.

Every case compares bit for bit with the oracle (tests/mm_trace.py: its outputs and the sample position before every
symbol), and asserts on that reference trace, before it looks at the GPU's result, that the input drives the regime
the case exists for: the position never below 0 (unless the case is about the end there) and the regime's count at
least half of what the CPU run of the reference recorded.  Recorded counts (CPU oracle; chain cases: the sum over
the eight checked captures, on the oracle's own demodulator output):

  stand-alone _ff (omega, gain_mu, limit; input)             symbols  back  zero  >64  >512 >2048  omega at low/high limit
    g30        10, 0.175, 0.005; x30 after 2000 quiet           8000    733   406    0     0     0   3781 / 3616
    g100       10, 0.175, 0.005; x100 after 2000 quiet          7931   2153    64    9     0     0   3772 / 3893
    g100_wide  10, 0.175, 0.3;   x100 after 2000 quiet          7781   2139    53    9     0     0   2751 / 2847
    omega1.0   1.0, 0.05; unit amplitude (2039 symbols in the first window)   11989  0  33
    omega1.3   1.3, 0.05; unit amplitude (1566 symbols in the first window)    9213  0   0
    omega700.5                                                   120      0     0  120   120     0
    omega2100.5                                                   50      0     0   50    50    50
    below zero 10, 0.175; x100 from the first sample: 7 symbols, then position -6
  stand-alone _cc (without / with the error output)
    omega1.3   nout 4096: 1568 / 1569 symbols in the first 2048 samples (> MMC_OUT = 1024), forward only
    loud       (2.0, 0.01, 0.5, 3.0, 0.01), x40 from the first sample: back 3120 / 2724, clamps at 0: 1 / 1368
    omega2500.5  40 symbols, every step > 2048
  chain, 37 captures, n_out 40 000: sums over captures 0, 1, 2, 7, 9, 31, 32, 36 (gain factor, omega)
                                symbols   back  zero   >64  >256  >512 >1024
    x30_omega10                   32250   2844   450   161     0     0     0   (the long steps: the capture of noise)
    x100_omega10                  30308   7158   297   856    61    10     0
    x100_omega3.3                 78058  21312   918   950    97     7     0
    x1_omega300.5                  1072      0     0  1072  1072     0     0   (every step 300 / 301)
    x1_omega700.5                   464      0     0   464   464   464     0
    x1_omega1100.5                  296      0     0   296   296   296   296
    x30_omega10_max1003            8024    670   115    39     0     0     0   (1003 symbols per capture)
    x100_omega10_sliced           53922  13006   543  1532   124     4     0   (n_out 72 000: eight time slices)
  chain, 1600 captures, n_out 24 000, x30, omega 10: sums over the five originals
                                  12192   1046   260     3     0     0     0
  The position is never below 0 in any of them (8000 silent input samples, 2000 demodulator outputs, in front).
"""
import ctypes

import numpy as np
import pytest

import mm_trace as mt
from conftest import bits_equal

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


# ---------------------------------------------------------------------------------------------------------------
# 2. the stand-alone _ff block
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ff_refs(po):
    """the reference trace of every _ff case, computed once"""
    return {name: mt.trace_ff(po, case[0], case[1], case[2]) for name, case in mt.ff_cases().items()}


@pytest.mark.parametrize("name", sorted(mt.ff_cases()))
def test_ff_bit_exact_in_one_call(gpu, po, ff_refs, name):
    params, x, nout, floor = mt.ff_cases()[name]
    tr = ff_refs[name]
    mt.assert_conditions(tr.regimes(), floor)
    ref = po.ClockRecoveryMM(*params)
    yr, cr = ref.general_work(nout, x)                  # (the position never goes below 0: the long call is defined)
    assert bits_equal(yr, tr.out) and cr == tr.consumed
    blk = gpu.clock_recovery_mm_ff(*params)
    y, c = blk.general_work(nout, x)
    assert len(y) == len(yr) and c == cr, (len(y), len(yr), c, cr)
    assert bits_equal(y, yr)
    assert np.float32(blk.mu()) == ref.state["mu"] and np.float32(blk.omega()) == ref.state["omega"]


@pytest.mark.parametrize("name", mt.FF_FORWARD_ONLY)
def test_ff_chunked_like_scheduler(gpu, po, ff_refs, name):
    """300 outputs at a time from windows of 4096 items: the same symbols as the one call, for loops that never step
    back (a step back behind the start of a call's window has no meaning for a scheduler)"""
    params, x, nout, floor = mt.ff_cases()[name]
    tr = ff_refs[name]
    reg = tr.regimes()
    mt.assert_conditions(reg, floor)
    assert reg["back"] == 0
    # the oracle driven the same way: it ends where 4096 items no longer hold a symbol's eight taps after a step
    ref, blk = po.ClockRecoveryMM(*params), gpu.clock_recovery_mm_ff(*params)
    pos = 0
    total = 0
    while True:
        yr, cr = ref.general_work(300, x[pos:pos + 4096])
        y, c = blk.general_work(300, x[pos:pos + 4096])
        assert len(y) == len(yr) and c == cr, (pos, len(y), len(yr), c, cr)
        if len(yr) == 0:
            break
        assert bits_equal(y, yr), pos
        assert bits_equal(yr, tr.out[total:total + len(yr)]), pos
        total += len(yr)
        pos += cr
    assert total >= min(len(tr.out), 40)
    assert np.float32(blk.mu()) == ref.state["mu"] and np.float32(blk.omega()) == ref.state["omega"]


def test_ff_ends_where_the_reference_would_read_before_its_buffer(gpu, po):
    """the documented deviation (grhip.h): the symbols up to the step below 0 are the reference's, the call reports
    the negative position, and the handle produces nothing more.  (The oracle is not called past that point.)"""
    params, x, nout = mt.ff_below_zero_case()
    tr = mt.trace_ff(po, params, x, nout)
    assert tr.below_zero and 2 <= len(tr.out) < 100
    blk = gpu.clock_recovery_mm_ff(*params)
    y, c = blk.general_work(nout, x)
    assert len(y) == len(tr.out) and bits_equal(y, tr.out)
    assert c == tr.consumed and c < 0
    assert np.float32(blk.mu()) == tr.mu and np.float32(blk.omega()) == tr.omega
    y2, c2 = blk.general_work(nout, x)
    assert len(y2) == 0 and c2 == 0


# ---------------------------------------------------------------------------------------------------------------
# 3. the stand-alone _cc block: host entry and device entry
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cc_refs(po):
    return {(name, we): mt.trace_cc(po, case[0], case[1], case[2], we)
            for name, case in mt.cc_cases().items() for we in (False, True)}


def _cc_device(gpu, blk, x, nout, want_error, shift):
    """general_work_device on buffers `shift` complex items behind a 16-byte boundary; sentinels around the outputs"""
    torch = _torch()
    dev = torch.device("cuda", 0)
    d_x = torch.zeros((len(x) + 4, 2), dtype=torch.float32, device=dev)
    assert d_x.data_ptr() % 16 == 0
    d_x[shift:shift + len(x)] = torch.from_numpy(np.ascontiguousarray(x).view(np.float32).reshape(-1, 2))
    d_y = torch.full((nout + 2, 2), 7.5, dtype=torch.float32, device=dev)
    d_e = torch.full((nout + 2,), 7.5, dtype=torch.float32, device=dev)
    n, c = blk.general_work_device(nout, len(x), d_x[shift:], d_y[1:], d_e[1:] if want_error else None)
    torch.cuda.synchronize()
    y = d_y.cpu().numpy().view(np.complex64).reshape(-1)
    e = d_e.cpu().numpy()
    guard = np.float32(7.5)
    assert y[0] == guard + 1j * guard and (y[1 + n:] == guard + 1j * guard).all()
    assert e[0] == guard and (e[1 + n:] == guard).all()
    if not want_error:
        assert (e == guard).all()
    return y[1:1 + n].copy(), e[1:1 + n].copy(), c


@pytest.mark.parametrize("want_error", [False, True])
@pytest.mark.parametrize("name", sorted(mt.cc_cases()))
def test_cc_bit_exact_host_and_device_entries(gpu, po, cc_refs, name, want_error):
    params, x, nout, floors = mt.cc_cases()[name]
    tr = cc_refs[(name, want_error)]
    mt.assert_conditions(tr.regimes(), floors[want_error])
    ref = po.ClockRecoveryMMcc(*params)
    yr, er, cr = ref.general_work(nout, x, want_error)
    assert bits_equal(yr, tr.out) and cr == tr.consumed
    # host entry
    blk = gpu.clock_recovery_mm_cc(*params)
    y, e, c = blk.general_work(nout, x, want_error)
    assert len(y) == len(yr) and c == cr, (len(y), len(yr), c, cr)
    assert bits_equal(np.array(y), yr)
    if want_error:
        assert bits_equal(np.array(e), er)
    assert blk.mu().tobytes() == ref.mu().tobytes() and blk.omega().tobytes() == ref.omega().tobytes()
    # device entry: input 16-byte aligned, and 8 bytes behind a 16-byte boundary
    for shift in (0, 1):
        blk = gpu.clock_recovery_mm_cc(*params)
        y, e, c = _cc_device(gpu, blk, x, nout, want_error, shift)
        assert len(y) == len(yr) and c == cr, (shift, len(y), len(yr), c, cr)
        assert bits_equal(y, yr), shift
        if want_error:
            assert bits_equal(e, er), shift
        assert blk.mu().tobytes() == ref.mu().tobytes() and blk.omega().tobytes() == ref.omega().tobytes()


# ---------------------------------------------------------------------------------------------------------------
# 4. the three forms of the loop in the chain
# ---------------------------------------------------------------------------------------------------------------
S37, N_OUT, LEAD = 37, 40_000, 8000
CHECKED = (0, 1, 2, 7, 9, 31, 32, 36)
NOISE, THIRD, SILENT = 7, 9, 31
BIG_S, BIG_K, BIG_N_OUT = 1600, 5, 24_000

# name -> (demodulator gain factor, omega, set_max_symbols or 0, floors = half of the recorded sums[, n_out])
CHAIN_CASES = {
    "x30_omega10": (30.0, 10.0, 0, {"back": 1422, "zero": 225}),
    "x100_omega10": (100.0, 10.0, 0, {"back": 3579, "gt64": 428, "gt256": 30}),
    "x100_omega3.3": (100.0, 3.3, 0, {"back": 10656, "gt64": 475}),
    "x1_omega300.5": (1.0, 300.5, 0, {"gt256": 536}),          # (and none > 512: runs of accepts, no restart)
    "x1_omega700.5": (1.0, 700.5, 0, {"gt512": 232}),
    "x1_omega1100.5": (1.0, 1100.5, 0, {"gt1024": 148}),
    "x30_omega10_max1003": (30.0, 10.0, 1003, {"back": 335, "symbols": 8 * 1003}),
    # n_out 40 000 is ONE time slice (the chain slices from 65 536 outputs on): the loop resumed slice by slice, with steps
    # back behind the point a resumed launch started from, needs a longer capture
    "x100_omega10_sliced": (100.0, 10.0, 0, {"back": 6503, "gt64": 766, "gt256": 62}, 72_000),
}
BIG_FLOOR = {"back": 523, "zero": 130}

_cache = {}


def chain_captures(wl, n):
    """37 captures at 39 / 40 / 41 samples per symbol, each behind LEAD silent samples (the loop of a loud capture would
    step before its buffer otherwise); one of noise only, one that goes silent after a third, one silent throughout
    (it stays on the steady path beside neighbours that jump)"""
    key = ("c37", n)
    if key not in _cache:
        c = wl.CFG2
        xs = []
        for s in range(S37):
            cfg = dict(c)
            cfg["sym_rate"] = c["fs"] / (39 + s % 3)
            x = wl.fsk4_capture(n, stream_id=300 + s, cfg=cfg)
            if s == NOISE:
                rng = np.random.default_rng(7)
                x = (rng.normal(0, 0.5, n) + 1j * rng.normal(0, 0.5, n)).astype(np.complex64)
            if s == THIRD:
                x[n // 3:] = 0
            if s == SILENT:
                x[:] = 0
            x[:LEAD] = 0
            xs.append(x)
        _cache[key] = xs
    return _cache[key]


def big_batch_captures(wl, n):
    key = ("big", n)
    if key not in _cache:
        xs = []
        for k in range(BIG_K):
            x = wl.fsk4_capture(n, stream_id=380 + k)
            x[:LEAD] = 0
            xs.append(x)
        _cache[key] = xs
    return _cache[key]


def _fetch(gpu, ptr, stride, s, count):
    a = np.empty(int(count), np.float32)
    if count:
        gpu.lib().grhip_memcpy_d2h(a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr + 4 * s * stride), int(count) * 4)
    return a


def _mm_params(wl, omega):
    c4 = wl.CFG4
    return (omega, c4["gain_omega"], c4["mu"], c4["gain_mu"], c4["omega_relative_limit"])


def _sum_regimes(traces):
    tot = {}
    for tr in traces:
        for k, v in tr.regimes().items():
            tot[k] = min(tot.get(k, v), v) if k == "min_pos" else tot.get(k, 0) + v
    return tot


@pytest.mark.parametrize("name", list(CHAIN_CASES))
def test_chain_forms_off_the_steady_path(gpu, po, wl, name):
    """the chain with 8, 32 and 1 captures per wave on 37 captures (one full wave of pairs and five pairs; four full waves
    of eight and five groups): symbols, counts and correlator output of eight captures against the trace of the chain's own
    demodulator output, every capture of the 8 and 32 forms against the one-capture form.  FAST, GENERIC on rows of even
    stride (its time-sliced route) and GENERIC on rows of odd stride (one launch over the whole capture)."""
    torch = _torch()
    G, omega, maxsym, floor = CHAIN_CASES[name][:4]
    c, c4 = wl.CFG2, wl.CFG4
    S, n_out = S37, (CHAIN_CASES[name][4:] or (N_OUT,))[0]
    n = n_out * 4 + 1
    xs = chain_captures(wl, n)
    dev = torch.device("cuda", 0)
    d_bits = torch.zeros((S, n_out), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(S, dtype=torch.int32, device=dev)
    ch = gpu.dmr_chain(4, wl.cfg2_proto_taps(), c["center_freq"], c["fs"], c["demod_gain"] * G, omega, c4["gain_omega"],
                       c4["mu"], c4["gain_mu"], c4["omega_relative_limit"], wl.access_code_string(), c4["threshold"], S, n)
    if maxsym:
        ch.set_max_symbols(maxsym)
    st = torch.cuda.Stream(device=dev)
    routes = [(gpu.MODE_GENERIC, n + 7), (gpu.MODE_GENERIC, n + 8)]
    if not maxsym:
        routes.insert(0, (gpu.MODE_FAST, n + 7))
    d_ins = {}
    for stride in (n + 7, n + 8):
        d_in = torch.zeros((S, stride, 2), dtype=torch.float32, device=dev)
        for s in range(S):
            d_in[s, :n] = torch.from_numpy(xs[s].view(np.float32).reshape(-1, 2))
        d_ins[stride] = d_in
    traces = {}                                        # mode -> (demodulator outputs, traces) of the checked captures
    for mode, stride in routes:
        ch.set_mode(mode)
        got = {}
        for cpw in (1, 8, 32):
            ch.set_captures_per_wave(cpw)
            d_bits.zero_(); d_n.zero_()
            torch.cuda.synchronize()
            ch.run_device(d_ins[stride], n, stride, d_bits, n_out, d_n, st)
            st.synchronize()
            nb = d_n.cpu().numpy()
            bits = d_bits.cpu().numpy()
            p_dem, s_dem = ch.intermediate(0)
            p_soft, s_soft = ch.intermediate(1)
            if cpw == 1:
                dems = {s: _fetch(gpu, p_dem, s_dem, s, n_out) for s in CHECKED}
                if mode not in traces:
                    trs = {s: mt.trace_ff(po, _mm_params(wl, omega), dems[s], maxsym or n_out) for s in CHECKED}
                    # the conditions, on the reference alone
                    reg = _sum_regimes(trs.values())
                    mt.assert_conditions(reg, floor)
                    if name == "x1_omega300.5":
                        assert reg["gt512"] == 0
                    assert trs[SILENT].regimes()["back"] == 0 and not np.any(dems[SILENT])
                    traces[mode] = (dems, trs)
                else:
                    for s in CHECKED:
                        assert bits_equal(dems[s], traces[mode][0][s]), (mode, stride, s)
                trs = traces[mode][1]
                for s in CHECKED:
                    assert nb[s] == len(trs[s].out), (mode, stride, s, nb[s], len(trs[s].out))
                    soft = _fetch(gpu, p_soft, s_soft, s, nb[s])
                    assert bits_equal(soft, trs[s].out), (mode, stride, s)
                    mine = po.CorrelateAccessCode(wl.access_code_string(), c4["threshold"]).work(po.binary_slicer_fb(soft))
                    assert np.array_equal(bits[s, :nb[s]], mine), (mode, stride, s)
            if maxsym:
                assert (nb <= maxsym).all() and nb[0] == maxsym
            got[cpw] = (nb.copy(), [_fetch(gpu, p_soft, s_soft, s, nb[s]) for s in range(S)], bits.copy())
        for cpw in (8, 32):
            assert np.array_equal(got[cpw][0], got[1][0]), (mode, stride, cpw, got[cpw][0], got[1][0])
            for s in range(S):
                assert bits_equal(got[cpw][1][s], got[1][1][s]), (mode, stride, cpw, s)
            assert np.array_equal(got[cpw][2], got[1][2]), (mode, stride, cpw)


def test_chain_big_batch_off_the_steady_path(gpu, po, wl):
    """1600 captures (the library's own choice of the eight-captures form with the ring of 1024), demodulator gain x 30:
    five distinct captures repeated; the originals against the trace of their own demodulator output, every copy like its
    original, and one wave per capture reproduces the batch"""
    torch = _torch()
    c, c4 = wl.CFG2, wl.CFG4
    S, K, n_out = BIG_S, BIG_K, BIG_N_OUT
    n = n_out * 4
    xs = big_batch_captures(wl, n)
    dev = torch.device("cuda", 0)
    d_in = torch.empty((S, n, 2), dtype=torch.float32, device=dev)
    src = [torch.from_numpy(x.view(np.float32).reshape(-1, 2)).to(dev) for x in xs]
    for s in range(S):
        d_in[s] = src[s % K]
    d_bits = torch.zeros((S, n_out), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(S, dtype=torch.int32, device=dev)
    ch = gpu.dmr_chain(4, wl.cfg2_proto_taps(), c["center_freq"], c["fs"], c["demod_gain"] * 30.0, 10.0, c4["gain_omega"],
                       c4["mu"], c4["gain_mu"], c4["omega_relative_limit"], wl.access_code_string(), c4["threshold"], S, n)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ch.run_device(d_in, n, n, d_bits, n_out, d_n, st)
    st.synchronize()
    nb = d_n.cpu().numpy()
    bits = d_bits.cpu().numpy()
    p_dem, s_dem = ch.intermediate(0)
    p_soft, s_soft = ch.intermediate(1)
    trs = [mt.trace_ff(po, _mm_params(wl, 10.0), _fetch(gpu, p_dem, s_dem, k, n_out), n_out) for k in range(K)]
    mt.assert_conditions(_sum_regimes(trs), BIG_FLOOR)
    for k in range(K):
        assert nb[k] == len(trs[k].out), (k, nb[k], len(trs[k].out))
        soft = _fetch(gpu, p_soft, s_soft, k, nb[k])
        assert bits_equal(soft, trs[k].out), k
        mine = po.CorrelateAccessCode(wl.access_code_string(), c4["threshold"]).work(po.binary_slicer_fb(soft))
        assert np.array_equal(bits[k, :nb[k]], mine), k
    nbv = nb.reshape(-1, K)
    assert (nbv == nbv[0]).all()
    bv = bits.reshape(S // K, K, n_out)
    assert (bv == bv[0]).all()                          # every copy like its original
    first = bits.copy()
    ch.set_captures_per_wave(1)
    d_bits.zero_()
    torch.cuda.synchronize()
    ch.run_device(d_in, n, n, d_bits, n_out, d_n, st)
    st.synchronize()
    assert np.array_equal(d_n.cpu().numpy(), nb) and np.array_equal(d_bits.cpu().numpy(), first)


# ---------------------------------------------------------------------------------------------------------------
# 5. unpack_k_bits_bb on device buffers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 5])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_unpack_k_bits_device_entry(gpu, po, k, offset):
    torch = _torch()
    n_in = 10_007
    x = np.random.default_rng(100 * k + offset).integers(0, 256, n_in).astype(np.uint8)
    ref = po.unpack_k_bits_bb(k, x)
    dev = torch.device("cuda", 0)
    d_x = torch.zeros(n_in + 32, dtype=torch.uint8, device=dev)
    d_y = torch.full((n_in * k + 64,), 0xA5, dtype=torch.uint8, device=dev)
    assert d_x.data_ptr() % 16 == 0 and d_y.data_ptr() % 16 == 0
    d_x[offset:offset + n_in] = torch.from_numpy(x)
    o0 = 16 + offset                                   # output `offset` bytes behind a 16-byte boundary, sentinels in front
    blk = gpu.unpack_k_bits_bb(k)
    assert blk.work_device(n_in * k, d_x[offset:], d_y[o0:]) == n_in * k
    torch.cuda.synchronize()
    y = d_y.cpu().numpy()
    assert np.array_equal(y[o0:o0 + n_in * k], ref)
    assert (y[:o0] == 0xA5).all() and (y[o0 + n_in * k:] == 0xA5).all()
