"""CPU checks of pfb_clock_sync_ccf: the restatement (pfb_clock_sync_ref.py) against tracks recorded from the reference's
own code, bit for bit; its independence of where calls cut the stream; the tap partition and the gains through the
library against the recording; every refusal; the sanitizer program.

The fixture, tests/golden/ref_pfb_clock_sync.npz, was recorded once by a throw-away program compiled from the reference's
own files -- filter/gr_pfb_clock_sync_ccf.cc, gr_fir_ccf.cc and gr_fir_ccf_generic.cc (expanded from gr_fir_XXX.cc.t and
gr_fir_XXX_generic.cc.t for ccf: complex accumulators, N_UNROLL 2), general/gr_reverse.cc and general/gr_math.h,
unchanged, with g++ -O2 -- against stub headers for gr_block, gr_io_signature, gr_core_api.h and gr_fir_util (which
hands out gr_fir_ccf_generic).  general_work got one linear, fully populated input buffer that starts with
tpf + floor(sps) - 1 zeros (history = tpf + sps), the pointers advanced by what each call consumed and produced; the
first call returns 0 (d_updated) and is not counted.  Every signal ran as one call, as two calls cut at 4097 new items and
in calls of 7 new items, each repeated while it made progress, and the program required the three to agree bit for bit
in all four outputs wherever each produced: all three produced the same counts and consumed the same items, which is the
evidence that the block's observable behaviour is a linear stream (include/grhip.h).  The fixture holds, as bit patterns:
  * proto_<c>, bank_<c>, dbank_<c> for pfb_clock_sync_ref.BANK_CASES: the prototype, get_taps() and get_diff_taps();
  * gains: (alpha, beta) for pfb_clock_sync_ref.GAIN_CASES;
  * per run <r> of pfb_clock_sync_ref.RUNS: err, rate and k in full, out in full for s2_o1 and otherwise its first 256
    items and SHA-256; produced and consumed per cut pattern; the final (d_k, d_error, d_rate_f, alpha, beta); the SHA-256
    of the input signal, which pfb_clock_sync_ref.signal regenerates.
The reference's input test, count < ninput - tpf - osps, allows for no carry and so lets it produce a few symbols more
from the same items than the library's rule (pos + osps 8 + osps + tpf <= arrived); the comparison runs on what both
produced, and the final state is compared after the restatement got need() zeros more and stopped at the reference's count."""
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_clock_sync_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")
FIX = np.load(os.path.join(HERE, "golden", "ref_pfb_clock_sync.npz"))
BANK_IDS = [c[0] for c in R.BANK_CASES]


def recorded_banks(name):
    return FIX["bank_" + name].view(np.float32), FIX["dbank_" + name].view(np.float32)


_ONE = {}


def one_call(name):
    """(track, object) of the run as one call, on the recorded banks"""
    if name not in _ONE:
        run = R.run_of(name)
        p = R.make(run, banks=recorded_banks(run[6]))
        _ONE[name] = (p.work(R.run_signal(run)), p)
    return _ONE[name]


# ---- 1: the designer and the gains ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.BANK_CASES, ids=BANK_IDS)
def test_banks_bit_for_bit(g, case):
    name, nf, _ = case
    t = R.proto(case)
    assert np.array_equal(R.bits(t), FIX["proto_" + name])
    for got in (g.pfb_clock_sync_taps(t, nf), R.design(t, nf)[:2]):         # the library, and the restatement
        assert got[0].shape == FIX["bank_" + name].shape
        assert np.array_equal(R.bits(got[0]), FIX["bank_" + name]) and np.array_equal(R.bits(got[1]), FIX["dbank_" + name])


def test_bank_shapes_are_the_ones_asked_for():
    assert FIX["bank_demod"].shape == (32, 23) and len(FIX["proto_demod"]) == 705
    assert FIX["bank_one_tap"].shape == (8, 1) and FIX["bank_arms64"].shape[0] == 64
    assert len(FIX["proto_ragged"]) % FIX["bank_ragged"].shape[0] != 0 and FIX["bank_two"].shape == (1, 2)
    assert not np.any(FIX["dbank_two"]) and np.any(FIX["dbank_demod"])


def test_gains_bit_for_bit():
    """update_gains of the restatement, and of csrc/pfb_clock_sync.h (the text the library compiles: pcs_gains itself and
    the way a handle's setters reach it, PcsLoop::init, set_damping_factor, set_loop_bandwidth), against the recording;
    tests/test_gpu_pfb_clock_sync.py walks the same cases through a handle's setters and getters"""
    for i, (bw, df) in enumerate(R.GAIN_CASES):
        a, b = R.gains(bw, df)
        assert np.array_equal(R.bits(np.array([a, b], np.float32)), FIX["gains"][i]), (bw, df)
    r = subprocess.run(["make", "-C", HOST, "pfb_clock_sync_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    args = []
    for bw, df in R.GAIN_CASES:
        args += ["%08x" % R.bits(np.array([bw], np.float32))[0], "-" if df is None else "%08x" % R.bits(np.array([df], np.float32))[0]]
    r = subprocess.run([os.path.join(HOST, "pfb_clock_sync_test"), "gains"] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = np.array([int(w, 16) for w in r.stdout.split()], np.uint32).reshape(len(R.GAIN_CASES), 4)
    assert np.array_equal(got[:, :2], FIX["gains"]) and np.array_equal(got[:, 2:], FIX["gains"])


def test_sanitizer_program_builds_and_passes():
    r = subprocess.run(["make", "-C", HOST, "pfb_clock_sync_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    exe = os.path.join(HOST, "pfb_clock_sync_test")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "pfb_clock_sync_test ok" in r.stdout, r.stdout
    # csrc/pfb_clock_sync.h, the text the library compiles, against the recording
    for name in ("ragged", "one_tap", "sps4"):
        case = R.bank_case(name)
        args = ["%08x" % v for v in FIX["proto_" + name]]
        r = subprocess.run([exe, "taps", str(case[1])] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        got = np.array([int(t, 16) for t in r.stdout.split()], np.uint32)
        assert np.array_equal(got, np.concatenate([FIX["bank_" + name].reshape(-1), FIX["dbank_" + name].reshape(-1)]))


# ---- 2: the restatement against the recording ---------------------------------------------------------------------------
def aux_equal(got, want_bits, osps):
    """slot i of a symbol holds what the reference wrote there; the osps - 1 slots behind it repeat it here and were left
    as they were (zero) by the reference"""
    g = R.bits(got).reshape(-1, osps)
    w = want_bits.reshape(-1, osps)
    return np.array_equal(g[:, 0], w[:, 0]) and np.all(g == g[:, :1]) and not np.any(w[:, 1:])


@pytest.mark.parametrize("name", R.RUN_IDS)
def test_restatement_is_the_recording_bit_for_bit(name):
    run = R.run_of(name)
    x = R.run_signal(run)
    assert R.digest(x) == bytes(FIX[name + "_x_sha"]).hex()
    t, p = one_call(name)
    n_ref = int(FIX[name + "_produced"][0])
    assert np.all(FIX[name + "_produced"] == n_ref) and len(set(FIX[name + "_consumed"])) == 1      # the three cut patterns
    n = len(t.out)
    print("%s: the reference produced %d, the restatement %d; carries %d forward, %d back; slips %d" % (name, n_ref, n, p.fwd, p.back, p.slips))
    assert n_ref - run[2] * (R.CARRY + 2) <= n <= n_ref
    for k in ("err", "rate", "k"):
        assert aux_equal(getattr(t, k), FIX["%s_%s" % (name, k)][:n], run[2]), k
    head = FIX[name + "_out_head"]
    assert np.array_equal(R.bits(t.out)[:len(head)], head)
    if name + "_out" in FIX:
        assert np.array_equal(R.bits(t.out), FIX[name + "_out"][:2 * n])
    # the whole of what the reference produced, and its final state: the items behind the stream are read by later symbols only
    q = R.make(run, banks=recorded_banks(run[6]))
    u = q.work(np.concatenate([x, np.zeros(q.need(), np.complex64)]), max_symbols=n_ref // run[2])
    assert len(u.out) == n_ref and R.digest(R.bits(u.out)) == bytes(FIX[name + "_out_sha"]).hex()
    for k in ("err", "rate", "k"):
        assert aux_equal(getattr(u, k), FIX["%s_%s" % (name, k)], run[2]), k
    st = FIX[name + "_state"]
    assert np.array_equal(R.bits(np.array([q.k, q.error, q.rate_f, q.alpha, q.beta], np.float32)), st)
    assert q.pos == int(FIX[name + "_consumed"][0])


def test_every_run_carries_and_none_slips():
    fwd = back = 0
    for name in R.RUN_IDS:
        t, p = one_call(name)
        assert p.slips == 0 and p.remainders == 0, name
        assert p.fwd + p.back >= 2, name
        fwd += p.fwd
        back += p.back
        assert np.all(np.diff(t.pos.reshape(-1, p.osps + 1)[:, 0]) >= 1)
    assert fwd >= 2 and back >= 2
    assert one_call("s2p5_o1")[1].fwd > 1000                   # sps 2.5: a carry every other symbol
    assert not np.any(one_call("s2_dev0")[0].rate)              # max_dev 0 pins the rate


@pytest.mark.parametrize("name", ["s2_o1", "s4_o2", "s2p5_o1"])
def test_cuts_do_not_change_the_restatement(name):
    run = R.run_of(name)
    x = R.run_signal(run)
    one, p = one_call(name)
    tpf = p.tpf
    for sizes in ((R.CUT,), (7,) * (len(x) // 7), (0, 100, 0, tpf - 1, 1, 0, 3000, 2), (tpf - 1,) * 40 + (0,)):
        q = R.make(run, banks=recorded_banks(run[6]))
        two = q.in_calls(x, sizes)
        for k in ("out", "err", "rate", "k", "pos", "arm"):
            assert np.array_equal(getattr(one, k).view(np.uint8), getattr(two, k).view(np.uint8)), (sizes[0], k)
        assert np.array_equal(R.bits(q.state()[0]), R.bits(p.state()[0])) and q.pos == p.pos
        assert len(q.held) <= q.hist()


def test_deviations_of_the_restatement():
    """the three deviations on states that no signal reaches (the device is never given these)"""
    class St(object):
        slips = fwd = back = remainders = 0
    for k, nf in ((1e30, 32), (-1e30, 32), (float("inf"), 32), (float("nan"), 5), (-0.0, 32), (2.0 ** 29, 7), (65 * 32.0, 32), (-70 * 32.0, 32)):
        st = St()
        fn, k2, pos = R.wrap(np.float32(k), 1000, 999, nf, st)
        assert 0 <= fn < nf and 999 <= pos <= 1000 + R.CARRY and 0 <= float(k2) <= nf
        if abs(k) >= 65 * 32.0 or k != k:
            assert st.slips >= 1
    st = St()
    assert R.wrap(np.float32(-1e-10), 10, 9, 32, st) == (31, np.float32(32.0), 9) and st.slips == 0     # the reference's own rounding


# ---- 3: the library's entries, which need no device ------------------------------------------------------------------------
def test_designer_refuses(g):
    t = np.ones(64, np.float32)
    bad = [(t[:1], 4), (t[:0], 4), (t, 0), (t, -1), (t, 257), (np.ones(4097, np.float32), 64), (np.ones(300, np.float32), 1)]
    for v in (np.nan, np.inf):
        u = t.copy()
        u[5] = v
        bad.append((u, 4))
    u = t.copy()
    u[7], u[9] = 3e38, -3e38
    bad.append((u, 4))
    for taps, nf in bad:
        with pytest.raises(g.GrhipError) as e:
            g.pfb_clock_sync_taps(taps, nf)
        assert e.value.code == -1
    import ctypes as C
    tpf = C.c_int(0)
    assert g.lib().grhip_pfb_clock_sync_taps(C.c_void_p(t.ctypes.data), 64, 4, None, None, None) == -1
    assert g.lib().grhip_pfb_clock_sync_taps(None, 64, 4, None, None, C.byref(tpf)) == -1
    assert g.lib().grhip_pfb_clock_sync_taps(C.c_void_p(t.ctypes.data), 64, 5, None, None, C.byref(tpf)) == 0 and tpf.value == 13


def test_block_refuses_before_the_device(g):
    """refused with GRHIP_EINVAL whether or not a device is there: the checks come first"""
    nan, inf = float("nan"), float("inf")
    t = R.proto(R.bank_case("demod"))
    ok = dict(sps=2.0, loop_bw=0.06, taps=t, filter_size=32, init_phase=16.0, max_rate_deviation=1.5, osps=1)
    for k, vals in (("sps", (0.99, 0.0, -2.0, 256.0, nan, inf)), ("loop_bw", (-0.01, nan, inf, 3e38)), ("filter_size", (0, -1, 257, 2)),
                    ("init_phase", (nan, inf)), ("max_rate_deviation", (nan, inf)), ("osps", (0, -1, 9)),
                    ("taps", (t[:1], np.full(8, nan, np.float32), np.ones(4100, np.float32)))):
        for v in vals:
            a = dict(ok)
            a[k] = v
            with pytest.raises(g.GrhipError) as e:
                g.pfb_clock_sync_ccf(**a)
            assert e.value.code == -1, (k, v)


OPS = ("create", "destroy", "set_mode", "set_streams", "set_loop_bandwidth", "set_damping_factor", "set_alpha", "set_beta",
       "set_max_rate_deviation", "get_loop_bandwidth", "get_damping_factor", "get_alpha", "get_beta", "get_max_rate_deviation",
       "get_clock_rate", "k", "error", "slips", "position", "get_taps", "get_diff_taps", "max_produced", "work", "work_device")


def test_new_entries_are_declared_and_exported(g):
    hdr = open(os.path.join(ROOT, "include", "grhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = g.lib()
    names = set(re.findall(r"\b(grhip_pfb_clock_sync_ccf_[a-z0-9_]+)\s*\(", hdr))
    assert names == set("grhip_pfb_clock_sync_ccf_" + op for op in OPS)
    for n in sorted(names) + ["grhip_pfb_clock_sync_taps"]:
        assert hasattr(lib, n), n
    for n in ("pfb_clock_sync_ccf", "pfb_clock_sync_taps"):
        assert hasattr(g, n) and n in g.__all__
    import ctypes as C
    sig = g.binding.signatures()
    assert sig["grhip_pfb_clock_sync_ccf_create"][1] == [C.c_void_p, C.c_double, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float,
                                                         C.c_int, C.c_int]
    assert sig["grhip_pfb_clock_sync_ccf_work_device"][1] == [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong] + [C.c_void_p] * 6
    assert sig["grhip_pfb_clock_sync_ccf_get_beta"][0] is C.c_float
    one = C.c_float(1)
    for op, args in (("set_mode", (None, 0)), ("set_streams", (None, 1)), ("set_loop_bandwidth", (None, one)), ("set_damping_factor", (None, one)),
                     ("set_alpha", (None, one)), ("set_beta", (None, one)), ("set_max_rate_deviation", (None, one)),
                     ("get_clock_rate", (None, 0, None)), ("k", (None, 0, None)), ("error", (None, 0, None)), ("slips", (None, 0, None)),
                     ("position", (None, 0, None)), ("get_taps", (None, None, 0, None, None)), ("get_diff_taps", (None, None, 0, None, None)),
                     ("max_produced", (None, 5)), ("work", (None, 0, None, 0) + (None,) * 5), ("work_device", (None, 0, None, 0) + (None,) * 6)):
        assert getattr(lib, "grhip_pfb_clock_sync_ccf_" + op)(*args) == -1, op
    assert lib.grhip_pfb_clock_sync_ccf_get_alpha(None) == -1.0
    assert lib.grhip_pfb_clock_sync_ccf_create(None, 2.0, 0.06, None, 0, 32, 0.0, 1.5, 1, 0) == -1


def test_block_refuses_to_run_without_a_device(g):
    if g.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(g.GrhipError) as e:
        g.pfb_clock_sync_ccf(2.0, 0.06, R.proto(R.bank_case("demod")), 32, 16.0, 1.5, 1)
    assert e.value.code == -5 and "no CPU fallback" in str(e.value)
