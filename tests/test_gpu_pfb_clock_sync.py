"""GPU tests of pfb_clock_sync_ccf against the restatement (pfb_clock_sync_ref.py, pinned to the reference's own code bit
for bit by test_pfb_clock_sync_cpu.py).

  * GENERIC: out, err, rate, k, produced and the final state bit for bit the restatement: every recorded shape as one
    call, cut at 4097 and in calls of 7; calls of 0 items and calls shorter than an arm; 1 and 3 streams; arms of 1 tap,
    64 arms, 71 and 141 taps per arm (a lane owns two and three taps);
  * every other mode, step by step on the device's own outputs and the state at the start of the call:
      (a) the scalar chain (wraps, positions, k, rate, the clip) replayed in float32 with the device's own errors equals
          the device's rate, k and final state bit for bit;
      (b) each component of out lies within gamma sum |t_j| |x_j| of the float64 arm output at the position and arm
          which that chain implies, gamma = (tpf + 2) 2^-24: the forward-error bound of a dot product of tpf terms in any
          order, fused or not (tpf - 1 sums and tpf products, each within 2^-24 relative, to first order tpf 2^-24; the
          + 2 covers the second-order terms for every tpf <= 256).  err = (o.im d.im + o.re d.re) / 2 is formed from the
          device's float32 arm outputs: with Bo, Bd the bounds of the two arm outputs, it lies within
          sum over re, im of (|o64| Bd + |d64| Bo + Bo Bd) / 2 of the float64 value, plus three roundings (two products,
          one sum; the halving is exact), each within half an ulp of a magnitude at most twice the larger product: 4 ulps
          of the larger product;
    and, as a lock check only, the timing index pos nfilters + k at the end of each run within 4 arms of GENERIC's
    (LOCK_ARMS; the largest measured on the device is written next to it);
  * setters between calls act on the next symbol; set_streams restarts every stream; aux outputs NULL leave out as it is."""
import functools
import math

import numpy as np
import pytest

import pfb_clock_sync_ref as R

pytestmark = pytest.mark.gpu

LOCK_ARMS = 4.0             # ten times the CPU sketch's 0.41 of an arm between float32 and float64; measured on an MI355X: 0.099 at the most (s4_o2)
# further shapes, not recorded: name, nfilters, root_raised_cosine arguments
EXTRA_BANKS = (("one_tap8", 8, (8.0, 16.0, 1.0, 0.35, 7)),          # 8 arms of 1 tap
               ("tpf71", 8, (8.0, 16.0, 1.0, 0.35, 560)),           # 71 taps per arm: two taps in some lanes
               ("tpf141", 4, (4.0, 8.0, 1.0, 0.35, 560)))           # 141 taps per arm: three taps in some lanes
EXTRA_RUNS = (("x_one_tap", 2.0, 1, 3.0, 1.5, 2e-3, "one_tap8"), ("x_tpf71", 2.0, 2, 4.0, 1.5, -2e-3, "tpf71"),
              ("x_tpf141", 2.0, 1, 1.5, 1.5, 3e-3, "tpf141"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_of(name):
    return R.run_of(name) if name in R.RUN_IDS else [r for r in EXTRA_RUNS if r[0] == name][0]


@functools.lru_cache(maxsize=None)
def taps_of(bc):
    for c in R.BANK_CASES + EXTRA_BANKS:
        if c[0] == bc:
            t = R.proto(c)
            t.setflags(write=False)
            return c[1], t
    raise KeyError(bc)


def fresh_ref(name):
    run = run_of(name)
    nf, t = taps_of(run[6])
    return R.Pcs(run[1], R.LOOP_BW, t, nf, run[3], run[4], run[2])


@functools.lru_cache(maxsize=None)
def ref_of(name, seed=1):
    """the restatement's one walk of the whole signal (cuts do not change it), and the object behind it"""
    run = run_of(name)
    p = fresh_ref(name)
    t = p.work(R.signal(seed, run[1], run[5]))
    return t, p


def make(g, name, mode, streams=1):
    run = run_of(name)
    nf, t = taps_of(run[6])
    blk = g.pfb_clock_sync_ccf(run[1], R.LOOP_BW, t, nf, run[3], run[4], run[2])
    blk.set_mode(mode)
    if streams != 1:
        blk.set_streams(streams)
    return blk


def feed(blk, xs, sizes=(), aux=True):
    """the streams xs (equal lengths) through blk in calls of the given sizes, then the rest: per stream (out, err, rate, k)"""
    n, S = len(xs[0]), len(xs)
    parts = [[[] for _ in range(4 if aux else 1)] for _ in xs]
    i = 0
    for size in list(sizes) + [None]:
        m = n - i if size is None else min(size, n - i)
        y = blk.work(np.concatenate([x[i:i + m] for x in xs]), m, aux=aux)
        i += m
        rows = [y] if S == 1 else y
        for s in range(S):
            for q, a in zip(parts[s], rows[s] if aux else (rows[s],)):
                q.append(a)
    return [tuple(np.concatenate(q) for q in p) for p in parts]


def check_generic(blk, got, s, t, p):
    for name, y in zip(("out", "err", "rate", "k"), got):
        assert same_bits(y, getattr(t, name)), (s, name, len(y), len(getattr(t, name)))
    assert same_bits(np.array([blk.k(s), blk.get_clock_rate(s), blk.error(s)], np.float32), p.state()[0])
    assert blk.position(s) == p.pos and blk.slips(s) == p.slips == 0


CUTS = {"one": (), "cut4097": (R.CUT,), "sevens": (7,) * (R.N // 7)}


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("name", R.RUN_IDS)
def test_generic_is_the_restatement_bit_for_bit(gpu, name, cut):
    run = run_of(name)
    t, p = ref_of(name)
    blk = make(gpu, name, gpu.MODE_GENERIC)
    got = feed(blk, [R.run_signal(run)], CUTS[cut])
    assert R.N > 2 * R.WIN and len(got[0][0]) == len(t.out)                         # two whole windows and a partial one
    check_generic(blk, got[0], 0, t, p)


def test_generic_calls_of_nothing_and_calls_shorter_than_an_arm(gpu):
    name = "s4_o2"
    t, p = ref_of(name)
    tpf = p.tpf
    blk = make(gpu, name, gpu.MODE_GENERIC)
    got = feed(blk, [R.run_signal(run_of(name))], (0, 100, 0, tpf - 1, 1, 0, 3000, 2) + (tpf - 1,) * 30 + (0,))
    check_generic(blk, got[0], 0, t, p)


@pytest.mark.parametrize("name", ["s2_o1", "s4_o2", "x_one_tap", "x_tpf71", "x_tpf141"])
def test_generic_three_streams_and_further_shapes(gpu, name):
    run = run_of(name)
    xs = [R.signal(seed, run[1], run[5]) for seed in (1, 2, 3)]
    blk = make(gpu, name, gpu.MODE_GENERIC, streams=3)
    got = feed(blk, xs, (R.CUT,))
    for s in range(3):
        t, p = ref_of(name, s + 1)
        check_generic(blk, got[s], s, t, p)
    if name == "x_tpf141":
        assert ref_of(name)[1].tpf == 141 and ref_of("x_tpf71")[1].tpf == 71 and ref_of("x_one_tap")[1].tpf == 1


def arm64(rev, xz, pos, arm):
    """float64 arm outputs at the given positions, and sum |t_j| |x_j| per component"""
    tpf = rev.shape[1]
    idx = pos[:, None] + np.arange(tpf)[None, :]
    seg = xz[idx].astype(np.complex128)
    tt = rev[arm].astype(np.float64)
    o = np.sum(tt * seg, axis=1)
    return o, np.sum(np.abs(tt) * np.abs(seg.real), axis=1), np.sum(np.abs(tt) * np.abs(seg.imag), axis=1)


def replay(blk, s, name, x, got):
    """(a): the scalar chain in float32 with the device's own errors (the error of symbol m stands in symbol m + 1's slot,
    the last one in the state) equals the device's rate, k and final state bit for bit"""
    out, err, rate, k = got
    osps = run_of(name)[2]
    nsym = len(out) // osps
    assert nsym > 0 and len(out) == nsym * osps and blk.slips(s) == 0
    errs = np.concatenate([err[::osps][1:], [blk.error(s)]]).astype(np.float32)
    p = fresh_ref(name)
    t = p.work(x, forced_err=errs)
    assert p.symbols == nsym and len(t.out) == len(out)
    assert same_bits(t.rate, rate) and same_bits(t.k, k) and same_bits(t.err[osps:], err[osps:]) and not err[:osps].any()
    assert same_bits(np.array([blk.k(s), blk.get_clock_rate(s)], np.float32), p.state()[0][:2]) and blk.position(s) == p.pos
    return p, t, errs


@pytest.mark.parametrize("mode", ("MODE_FAST", "MODE_FAST_VALU"))
@pytest.mark.parametrize("name", tuple(R.RUN_IDS) + ("x_tpf141",))
def test_fast_step_by_step(gpu, name, mode):
    run = run_of(name)
    osps = run[2]
    x = R.run_signal(run)
    blk = make(gpu, name, getattr(gpu, mode))
    out, err, rate, k = feed(blk, [x])[0]
    nsym = len(out) // osps
    p, t, errs = replay(blk, 0, name, x, (out, err, rate, k))
    # (b) the arm outputs in float64 at the positions and arms of that chain
    xz = np.concatenate([np.zeros(p.tpf + p.isps - 1, np.complex64), x])
    pos, arm = t.pos.reshape(nsym, osps + 1), t.arm.reshape(nsym, osps + 1)
    gamma = (p.tpf + 2) * 2.0 ** -24
    o64, br, bi = arm64(p.rev, xz, pos[:, :osps].reshape(-1), arm[:, :osps].reshape(-1))
    worst = max(np.max(np.abs(out.real - o64.real) / np.maximum(gamma * br, 1e-300)), np.max(np.abs(out.imag - o64.imag) / np.maximum(gamma * bi, 1e-300)))
    assert np.all(np.abs(out.real - o64.real) <= gamma * br) and np.all(np.abs(out.imag - o64.imag) <= gamma * bi)
    d64, dr, di = arm64(p.drev, xz, pos[:, osps], arm[:, osps])
    f64, fr, fi = o64[::osps], gamma * br[::osps], gamma * bi[::osps]
    dr, di = gamma * dr, gamma * di
    e64 = (f64.imag * d64.imag + f64.real * d64.real) / 2.0
    big = np.maximum(np.abs(f64.imag * d64.imag), np.abs(f64.real * d64.real)).astype(np.float32)
    bound = (np.abs(f64.real) * dr + np.abs(d64.real) * fr + fr * dr + np.abs(f64.imag) * di + np.abs(d64.imag) * fi + fi * di) / 2.0
    bound = bound + 4 * np.spacing(big).astype(np.float64)
    worst_e = np.max(np.abs(errs.astype(np.float64) - e64) / bound)
    assert np.all(np.abs(errs.astype(np.float64) - e64) <= bound)
    # the lock check
    tg, pg = ref_of(name)
    lock = abs((blk.position(0) - pg.pos) * p.nf + float(blk.k(0)) - float(pg.k))
    print("%s %s: out uses %.3f of its bound, err %.3f of its; timing index %.4f arms from GENERIC's at the end" % (name, mode, worst, worst_e, lock))
    assert lock <= LOCK_ARMS


def test_fast_three_streams(gpu):
    """every stream of a FAST handle walks its own signal, across a cut: the chain replayed from its own errors"""
    name = "s2_o1"
    run = run_of(name)
    xs = [R.signal(seed, run[1], run[5]) for seed in (1, 2, 3)]
    blk = make(gpu, name, gpu.MODE_FAST, streams=3)
    got = feed(blk, xs, (R.CUT,))
    for s in range(3):
        replay(blk, s, name, xs[s], got[s])
        tg, pg = ref_of(name, s + 1)
        assert abs((blk.position(s) - pg.pos) * pg.nf + float(blk.k(s)) - float(pg.k)) <= LOCK_ARMS


def test_setters_between_calls_act_on_the_next_symbol(gpu):
    name = "s2_o1"
    x = R.run_signal(run_of(name))
    p = fresh_ref(name)
    blk = make(gpu, name, gpu.MODE_GENERIC)
    want, got = [], []
    steps = ((1500, None), (1000, ("set_loop_bandwidth", 0.1)), (700, ("set_damping_factor", 0.5)), (800, ("set_alpha", 0.02)),
             (900, ("set_beta", 0.001)), (len(x) - 4900, ("set_max_rate_deviation", 0.05)))
    i = 0
    for n, setter in steps:
        if setter:
            getattr(blk, setter[0])(setter[1])
            if setter[0] == "set_loop_bandwidth":
                p.alpha, p.beta = R.gains(setter[1])
            elif setter[0] == "set_damping_factor":
                p.alpha, p.beta = R.gains(0.1, setter[1])
            else:
                setattr(p, {"set_alpha": "alpha", "set_beta": "beta", "set_max_rate_deviation": "max_dev"}[setter[0]], np.float32(setter[1]))
        want.append(p.work(x[i:i + n]))
        got.append(blk.work(x[i:i + n], n, aux=True))
        i += n
    for w, y in zip(want, got):
        for name_, a in zip(("out", "err", "rate", "k"), y):
            assert same_bits(a, getattr(w, name_)), name_
    assert blk.get_alpha() == p.alpha and blk.get_beta() == p.beta and blk.get_max_rate_deviation() == p.max_dev
    # the first slot holds the rate from before the new limit's first clip; gr_branchless_clip rounds x + c and x - c once each,
    # so it lands within an ulp of |x| + c of the limit
    assert np.max(np.abs(want[-1].rate[1:])) <= 0.05 + np.spacing(np.float32(0.25))
    # a refused setter changes nothing
    before = (blk.get_loop_bandwidth(), blk.get_damping_factor(), blk.get_alpha(), blk.get_beta(), blk.get_max_rate_deviation())
    for setter, v in (("set_loop_bandwidth", -1.0), ("set_loop_bandwidth", float("nan")), ("set_damping_factor", 1.5), ("set_damping_factor", -0.1),
                      ("set_alpha", 1.5), ("set_alpha", -0.5), ("set_beta", 2.0), ("set_beta", float("nan")), ("set_max_rate_deviation", float("inf"))):
        with pytest.raises(gpu.GrhipError) as e:
            getattr(blk, setter)(v)
        assert e.value.code == -1
    assert before == (blk.get_loop_bandwidth(), blk.get_damping_factor(), blk.get_alpha(), blk.get_beta(), blk.get_max_rate_deviation())


def test_gains_through_the_handle_are_the_recording_bit_for_bit(gpu):
    """GAIN_CASES through the constructor and through set_damping_factor / set_loop_bandwidth, read back with the getters"""
    import os
    fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pfb_clock_sync.npz"))["gains"]
    nf, t = taps_of("demod")
    walked = gpu.pfb_clock_sync_ccf(2.0, R.LOOP_BW, t, nf, 16.0, 1.5, 1)
    for i, (bw, df) in enumerate(R.GAIN_CASES):
        if df is None:
            made = gpu.pfb_clock_sync_ccf(2.0, bw, t, nf, 16.0, 1.5, 1)          # the constructor's damping
            assert same_bits(np.array([made.get_alpha(), made.get_beta()], np.float32), fix[i].view(np.float32)), (bw, df)
            assert made.get_loop_bandwidth() == np.float32(bw) and made.get_damping_factor() == np.float32(math.sqrt(2.0)) / np.float32(2)
        walked.set_damping_factor(float(np.float32(math.sqrt(2.0)) / np.float32(2)) if df is None else df)
        walked.set_loop_bandwidth(bw)
        assert same_bits(np.array([walked.get_alpha(), walked.get_beta()], np.float32), fix[i].view(np.float32)), (bw, df)


def test_set_streams_restarts_every_stream_and_getters(gpu):
    name = "s2_o2"
    run = run_of(name)
    t, p = ref_of(name)
    x = R.run_signal(run)
    blk = make(gpu, name, gpu.MODE_GENERIC, streams=2)
    feed(blk, [x[:1000], x[1000:2000]])
    assert blk.position(0) > 0 and blk.position(1) > 0
    blk.set_streams(2)
    q = fresh_ref(name)
    for s in range(2):
        assert blk.position(s) == 0 and blk.slips(s) == 0
        assert same_bits(np.array([blk.k(s), blk.get_clock_rate(s), blk.error(s)], np.float32), q.state()[0])
    got = feed(blk, [x, x])
    for s in range(2):
        check_generic(blk, got[s], s, t, p)
    nf, taps = taps_of(run[6])
    assert same_bits(blk.get_taps(), q.bank) and same_bits(blk.get_diff_taps(), q.dbank)
    assert blk.max_produced(100) == run[2] * (100 + int(run[1]))
    with pytest.raises(gpu.GrhipError):
        blk.k(2)


@pytest.mark.parametrize("mode", ("MODE_GENERIC", "MODE_FAST"))
def test_aux_outputs_null_leave_out_unchanged(gpu, mode):
    name = "s2p5_o1"
    x = R.run_signal(run_of(name))
    with_aux = feed(make(gpu, name, getattr(gpu, mode)), [x], (R.CUT,))[0]
    without = feed(make(gpu, name, getattr(gpu, mode)), [x], (R.CUT,), aux=False)[0]
    assert same_bits(with_aux[0], without[0])


def test_work_device_refusals(gpu):
    import torch
    name = "s2_o1"
    blk = make(gpu, name, gpu.MODE_GENERIC)
    n = 256
    cap = blk.max_produced(n)
    d_in = torch.zeros(n, dtype=torch.complex64, device="cuda")
    d_out = torch.zeros(cap, dtype=torch.complex64, device="cuda")
    d_f = [torch.zeros(cap, dtype=torch.float32, device="cuda") for _ in range(3)]
    d_p = torch.zeros(1, dtype=torch.int32, device="cuda")
    bad = [lambda: blk.work_device(n, d_in, cap - 1, d_out, d_p),                       # an out_cap that may not suffice
           lambda: blk.work_device(n, d_in, 2 ** 31, d_out, d_p),                       # byte counts would leave their range
           lambda: blk.work_device(-1, d_in, cap, d_out, d_p),
           lambda: blk.work_device(n, d_in, cap, d_out, None),
           lambda: blk.work_device(n, None, cap, d_out, d_p),
           lambda: blk.work_device(n, d_in, cap, d_out, d_p, d_f[0], d_f[1], None),      # all three or none
           lambda: blk.work_device(n, d_in, cap, d_out, d_p, d_f[0], d_f[0], d_f[1]),    # overlapping
           lambda: blk.work_device(n, d_in, cap, d_in, d_p)]
    for call in bad:
        with pytest.raises(gpu.GrhipError) as e:
            call()
        assert e.value.code == -1
    assert blk.position(0) == 0                                                         # nothing ran
    blk.work_device(n, d_in, cap, d_out, d_p, *d_f)
    torch.cuda.synchronize()
    assert int(d_p.cpu()[0]) == (23 + 2 - 1 + n - (1 * R.CARRY + 1 + 23)) // 2 + 1       # zeros in: k stays, a symbol every 2 items
