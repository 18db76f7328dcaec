"""Reference traces of the Mueller & Mueller loops: the oracle's outputs together with the sample position `ii` before
every symbol, and the counts that tell which regime of the loop an input drives (steps back, steps of zero, long
steps, clamps at 0).  The GPU tests assert these counts on the reference before they look at a kernel's result, so a
case cannot quietly stop exercising the branch it exists for.  CPU only; pinned by tests/test_mm_trace_cpu.py."""
import numpy as np

STEP_BINS = (64, 256, 512, 1024, 2048)


class Trace(object):
    """out[k]: symbol k; pos[k]: its sample position, pos[n]: where the walk ended; err: the _cc error output or None;
    consumed / mu / omega as the reference leaves them; below_zero: the _ff walk stopped at a negative position"""

    def __init__(self, out, pos, consumed, mu, omega, err=None, clamps=0, below_zero=False, omegas=None, limits=None):
        self.out, self.pos, self.consumed, self.mu, self.omega = out, np.asarray(pos, np.int64), consumed, mu, omega
        self.err, self.clamps, self.below_zero = err, clamps, below_zero
        self.omegas, self.limits = omegas, limits          # _ff: omega after every symbol, (lowest, highest) it can take

    def regimes(self):
        d = np.diff(self.pos)
        r = {"symbols": len(self.out), "min_pos": int(self.pos.min()), "back": int((d < 0).sum()),
             "zero": int((d == 0).sum()), "clamps": int(self.clamps)}
        for b in STEP_BINS:
            r["gt%d" % b] = int((d > b).sum())
        # symbols before the position first leaves the 2048 samples a one-capture kernel stages at the stream's start
        beyond = np.nonzero(self.pos[:len(self.out)] > 2048 - 8)[0]
        r["first_window"] = int(beyond[0]) if len(beyond) else len(self.out)
        if self.omegas is not None:                        # symbols that leave omega within 0.1 % of the range of a limit
            lo, hi = self.limits
            tol = 1e-3 * (hi - lo)
            r["omega_low"] = int((self.omegas <= lo + tol).sum())
            r["omega_high"] = int((self.omegas >= hi - tol).sum())
        return r


def trace_ff(po, params, x, nout):
    """digital_clock_recovery_mm_ff, one output per call.  The block's `consumed` is the raw position, so the walk is
    the one long call -- up to the first negative position, where the long call would read before its buffer and the
    walk stops (below_zero)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    blk = po.ClockRecoveryMM(*params)
    mid, rel = float(blk.state["omega_mid"]), float(np.float32(params[4]))
    out, pos, p, om = [], [0], 0, []
    while len(out) < nout:
        y, c = blk.general_work(1, x[p:])
        if len(y) == 0:
            break
        out.append(y[0])
        om.append(blk.s.omega)
        p += c
        pos.append(p)
        if p < 0:
            break
    st = blk.state
    # (the loop clips omega - omega_mid to +/- omega_relative_limit, taken as an absolute figure as the reference does)
    return Trace(np.array(out, np.float32), pos, p, st["mu"], st["omega"], below_zero=p < 0,
                 omegas=np.array(om, np.float64), limits=(mid - rel, mid + rel))


def trace_cc(po, params, x, nout, want_error):
    """digital_clock_recovery_mm_cc in one call of the oracle's tracing entry (stepping one output per call is another
    computation there: `consumed` and the loop's position are clamped at 0 per call)"""
    blk = po.ClockRecoveryMMcc(*params)
    y, e, c, pos, clamps = blk.general_work_trace(nout, x, want_error)
    return Trace(y, pos, c, blk.mu(), blk.omega(), err=e, clamps=clamps)


def assert_conditions(reg, floor, allow_negative=False):
    """the conditions of a case on its reference trace: the position stays at or above 0 unless the case is about the
    loop's end there, and every regime count named in `floor` (half of what the CPU run recorded) is reached"""
    if not allow_negative:
        assert reg["min_pos"] >= 0, reg
    for k, v in floor.items():
        assert reg[k] >= v, (k, v, reg)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def fsk_soft(rng, nsym, sps=10, noise=0.15):
    """four-level soft symbols at unit spacing, as the demodulator of the chain delivers them (tests/test_gpu_digital.py)"""
    x = np.repeat(rng.choice([-3.0, -1.0, 1.0, 3.0], nsym), sps)
    x = np.convolve(x, np.ones(4) / 4, mode="same")
    return (x + rng.normal(0, noise, len(x))).astype(np.float32)


def loud_fsk(seed, nsym, sps, gain, quiet):
    """fsk_soft with its first `quiet` samples silent and the rest scaled by `gain`: a demodulator gain set too high"""
    x = fsk_soft(np.random.default_rng(seed), nsym, sps)
    x[:quiet] = 0
    x[quiet:] *= np.float32(gain)
    return x


def qpsk(rng, nsym, sps, noise=0.1):
    sym = (rng.integers(0, 2, nsym) * 2 - 1) + 1j * (rng.integers(0, 2, nsym) * 2 - 1)
    x = np.repeat(sym, sps).astype(np.complex64)
    x = np.convolve(x, np.ones(sps) / sps)[:len(x)]
    x = x + noise * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    return x.astype(np.complex64)


def _mm(omega, gain_mu, rel=0.005):
    return (omega, 0.25 * gain_mu * gain_mu, 0.5, gain_mu, rel)


# _ff cases: name -> (parameters, input, outputs asked for, floor of the regime counts = half the recorded ones)
def ff_cases():
    return {
        "g30": (_mm(10.0, 0.175), loud_fsk(30, 8200, 10, 30.0, 2000), 8000, {"back": 366, "zero": 203}),
        "g100": (_mm(10.0, 0.175), loud_fsk(100, 8200, 10, 100.0, 2000), 8000, {"back": 1076, "gt64": 4}),
        "g100_wide": (_mm(10.0, 0.175, 0.3), loud_fsk(101, 8200, 10, 100.0, 2000), 8000,
                      {"back": 1069, "gt64": 4, "omega_low": 1375, "omega_high": 1423}),
        "omega1.0": (_mm(1.0, 0.05), fsk_soft(np.random.default_rng(10), 6000, 2), 12000, {"first_window": 1019, "zero": 16}),
        "omega1.3": (_mm(1.3, 0.05), fsk_soft(np.random.default_rng(13), 6000, 2), 12000, {"first_window": 783}),
        "omega700.5": (_mm(700.5, 0.175), fsk_soft(np.random.default_rng(700), 120, 700), 200, {"gt512": 60}),
        "omega2100.5": (_mm(2100.5, 0.175), fsk_soft(np.random.default_rng(2100), 50, 2100), 200, {"gt2048": 25}),
    }


FF_FORWARD_ONLY = ("omega1.0", "omega1.3", "omega700.5", "omega2100.5")


def ff_below_zero_case():
    """loud from the first sample: the loop steps before its buffer after a few symbols"""
    return _mm(10.0, 0.175), loud_fsk(7, 3000, 10, 100.0, 0), 3000


# _cc cases: name -> (parameters, input with its two history items, noutput_items, floors without / with error output)
def cc_cases():
    z = np.zeros(2, np.complex64)
    loud = 40 * qpsk(np.random.default_rng(2), 6000, 2)
    return {
        "omega1.3": ((1.3, 0.001, 0.5, 0.01, 0.005), np.concatenate([z, qpsk(np.random.default_rng(1), 6000, 2)]), 4096,
                     ({"first_window": 1025}, {"first_window": 1025})),
        "loud": ((2.0, 0.01, 0.5, 3.0, 0.01), np.concatenate([z, loud]).astype(np.complex64), 4096,
                 ({"back": 1560, "clamps": 1}, {"back": 1362, "clamps": 684})),
        "omega2500.5": ((2500.5, 0.01, 0.5, 0.1, 0.01), np.concatenate([z, qpsk(np.random.default_rng(3), 40, 2500)]),
                        100, ({"gt2048": 20}, {"gt2048": 20})),
    }
