"""Restatement of gnuradio-core/src/lib/filter/gr_pfb_clock_sync_ccf.cc (:200-205 update_gains, :208-248 set_taps,
:250-274 create_diff_taps, :351-427 general_work), of gr_fir_ccf_generic::filter (gr_fir_XXX_generic.cc.t:59-79) and of
gr_branchless_clip (gr_math.h:63-69) in float32 scalars and arrays with every operation rounded once and double where
the reference's expression is double; and the test signals.

The contract restated (include/grhip.h): with isps = floor(sps), xz is tpf + isps - 1 zeros followed by the stream and
`pos` an absolute index into it; an evaluation at pos reads xz[pos .. pos + tpf - 1], tap j of arm f on
xz[pos + tpf - 1 - j].  A Pcs object takes the stream in pieces and keeps, as the device handle does, k, rate_f, error,
pos, the slips and the last hist() items of xz.  A symbol starts once pos + need() items of xz have arrived.

The three deviations are the library's (csrc/pfb_clock_sync.h): the backward limit `lo`, at most CARRY forward carries
per evaluation, the wrap loops bounded by WRAP_TRIPS with the exact remainder beyond."""
import math

import numpy as np

import carrier_ref as CR
import fll_ref as FR

f32 = np.float32
bits = CR.bits
digest = CR.digest
root_raised_cosine = FR.root_raised_cosine

CARRY = 8                       # PCS_CARRY
WRAP_TRIPS = 64                 # PCS_WRAP_TRIPS
MAX_FILTERS, MAX_TPF, MAX_BANK, MAX_OSPS, MAX_SPS = 256, 256, 4096, 8, 256
WIN = 2048                      # PCS_WIN of csrc/pfb_clock_sync_launch.h
N = 6037
CUT = 4097
LOOP_BW = 2 * math.pi / 100     # generic_demod's timing_bw


# ---- the designer -----------------------------------------------------------------------------------------------
def diff_taps(taps):
    """create_diff_taps: pwr gathers |the partial sums|, and the taps are multiplied by it"""
    t = np.asarray(taps, np.float32)
    d = [f32(0)]
    pwr = f32(0)
    for i in range(len(t) - 2):
        tap = f32(0)
        for j, c in enumerate((f32(-1), f32(0), f32(1))):
            tap = tap + c * t[i + j]
            pwr = pwr + abs(tap)
        d.append(tap)
    d.append(f32(0))
    return np.array(d, np.float32) * pwr


def partition(taps, nf):
    """set_taps: arm f's tap j is taps[f + j nf]; [nf][tpf]"""
    tpf = -(-len(taps) // nf)
    t = np.zeros(nf * tpf, np.float32)
    t[:len(taps)] = taps
    return np.ascontiguousarray(t.reshape(tpf, nf).T), tpf


def design(taps, nf):
    """(bank, diff_bank, tpf)"""
    b, tpf = partition(np.asarray(taps, np.float32), nf)
    d, _ = partition(diff_taps(taps), nf)
    return b, d, tpf


def gains(loop_bw, damping=None):
    """update_gains: the same mix of float and double as gri_control_loop's"""
    return CR.gains(loop_bw, damping)


def clip(x, c):
    x1 = abs(x + c)
    x2 = abs(x - c)
    x1 = x1 - x2
    return f32(0.5 * float(x1))


def fir_generic(rev, seg):
    """gr_fir_ccf_generic::filter: two complex accumulators over the even and the odd taps (the tail of an odd count
    goes to the first), every product and sum rounded once, then acc0 + acc1"""
    pr = rev * seg.real
    pi = rev * seg.imag
    z = np.zeros(1, np.float32)
    re = np.cumsum(np.concatenate([z, pr[0::2]]), dtype=np.float32)[-1] + np.cumsum(np.concatenate([z, pr[1::2]]), dtype=np.float32)[-1]
    im = np.cumsum(np.concatenate([z, pi[0::2]]), dtype=np.float32)[-1] + np.cumsum(np.concatenate([z, pi[1::2]]), dtype=np.float32)[-1]
    return f32(re), f32(im)


def fir64(rev, seg):
    s = np.sum(rev.astype(np.float64) * seg.astype(np.complex128))
    return s.real, s.imag


def wrap(k, pos, lo, nf, st):
    """pcs_wrap of csrc/pfb_clock_sync.h: (arm, k, pos); counts in st"""
    if not np.isfinite(k):
        k = f32(0)
        st.slips += 1
    carry = 0
    far = True
    fn = 0
    if abs(k) < f32(2.0 ** 29):
        fn = int(math.floor(float(k)))
        t = 0
        while fn >= nf and t < WRAP_TRIPS:
            k = k - f32(nf)
            fn -= nf
            carry += 1
            t += 1
        while fn < 0 and t < WRAP_TRIPS:
            k = k + f32(nf)
            fn += nf
            carry -= 1
            t += 1
        far = fn >= nf or fn < 0
    if far:
        r = math.fmod(float(k), float(nf))
        if r < 0:
            r += float(nf)
        c = (float(k) - r) / float(nf)
        carry += int(max(-1e12, min(1e12, c)))
        fn = min(int(r), nf - 1)
        k = f32(r)
        st.remainders += 1
    if carry > 0:
        st.fwd += carry
    else:
        st.back -= carry
    if carry > CARRY:
        carry = CARRY
        st.slips += 1
    pos += carry
    if pos < lo:
        pos = lo
        st.slips += 1
    return fn, k, pos


class Track(object):
    """what a piece of the stream gave: the four outputs, and per evaluation its position and arm"""
    def __init__(self):
        self.out, self.err, self.rate, self.k = [], [], [], []
        self.pos, self.arm = [], []

    def arrays(self):
        self.out = np.array(self.out, np.complex64).reshape(-1)
        for n in ("err", "rate", "k"):
            setattr(self, n, np.array(getattr(self, n), np.float32))
        self.pos = np.array(self.pos, np.int64)
        self.arm = np.array(self.arm, np.int64)
        return self


class Pcs(object):
    def __init__(self, sps, loop_bw, taps, nf, init_phase, max_dev, osps, banks=None):
        self.nf, self.osps = int(nf), int(osps)
        self.isps = int(math.floor(sps))
        if banks is None:
            self.bank, self.dbank, self.tpf = design(taps, nf)
        else:
            self.bank, self.dbank = banks
            self.tpf = self.bank.shape[1]
        self.rev, self.drev = np.ascontiguousarray(self.bank[:, ::-1]), np.ascontiguousarray(self.dbank[:, ::-1])
        self.alpha, self.beta = gains(loop_bw)
        self.max_dev = f32(max_dev)
        rate = f32((sps - math.floor(sps)) * float(nf))
        self.rate_i = f32(int(math.floor(float(rate))))
        self.rate_f = rate - self.rate_i
        self.k = f32(init_phase)
        self.error = f32(0)
        self.pos = 0
        self.slips = self.fwd = self.back = self.remainders = 0
        self.symbols = 0
        # the items of xz that are kept: xz[self.h0 .. self.h0 + len(self.held))
        self.h0 = 0
        self.held = np.zeros(self.tpf + self.isps - 1, np.complex64)

    def need(self):
        return self.osps * CARRY + self.osps + self.tpf

    def hist(self):
        return self.need() + self.isps

    def state(self):
        return np.array([self.k, self.rate_f, self.error], np.float32), self.pos

    def seg(self, pos):
        return self.held[pos - self.h0:pos - self.h0 + self.tpf]

    def work(self, x, max_symbols=None, forced_err=None, fir=fir_generic):
        """takes the new items x; forced_err: the errors to step with, one per symbol (the device's own, for the
        step-by-step check), in place of the ones computed here"""
        self.held = np.concatenate([self.held, np.asarray(x, np.complex64).reshape(-1)])
        arrived = self.h0 + len(self.held)
        t = Track()
        m = 0
        while self.pos + self.need() <= arrived and (max_symbols is None or self.symbols < max_symbols):
            lo = max(self.pos - self.isps + 1, 0)
            first = None
            for kk in range(self.osps):
                fn, self.k, self.pos = wrap(self.k, self.pos, lo, self.nf, self)
                o = fir(self.rev[fn], self.seg(self.pos + kk))
                t.pos.append(self.pos + kk)
                t.arm.append(fn)
                t.out.append(complex(float(o[0]), float(o[1])))
                if kk == 0:
                    first = o
                self.k = (self.k + self.rate_i) + self.rate_f
            for kk in range(self.osps):
                t.err.append(self.error)
                t.rate.append(self.rate_f)
                t.k.append(self.k)
            d = fir(self.drev[fn], self.seg(self.pos))
            t.pos.append(self.pos)
            t.arm.append(fn)
            if forced_err is not None:
                self.error = f32(forced_err[m])
            else:
                er = f32(first[0]) * f32(d[0])
                ei = f32(first[1]) * f32(d[1])
                self.error = f32(float(ei + er) / 2.0)
            with np.errstate(all="ignore"):
                self.rate_f = self.rate_f + self.beta * self.error
                self.k = self.k + self.alpha * self.error
                self.rate_f = clip(self.rate_f, self.max_dev)
            self.pos += self.isps
            self.symbols += 1
            m += 1
        # keep what a later symbol may read, hist() items at the most
        keep = max(self.pos - self.isps + 1, 0)
        assert max_symbols is not None or arrived - keep <= self.hist()
        if keep > self.h0:
            self.held = self.held[keep - self.h0:]
            self.h0 = keep
        return t.arrays()

    def in_calls(self, x, sizes):
        """x in calls of the given sizes, then the rest; the concatenated track"""
        parts, i = [], 0
        for n in list(sizes) + [None]:
            piece = x[i:] if n is None else x[i:i + n]
            i += len(piece)
            parts.append(self.work(piece))
        t = Track()
        for n in ("out", "err", "rate", "k", "pos", "arm"):
            setattr(t, n, np.concatenate([getattr(p, n) for p in parts]))
        return t


# ---- the shapes and the signals whose recordings tests/golden/ref_pfb_clock_sync.npz holds --------------------------
# (nfilters, taps as (gain, fs, symbol_rate, alpha, ntaps) of root_raised_cosine, or a count of ramp taps)
BANK_CASES = (("demod", 32, (32.0, 64.0, 1.0, 0.35, 704)),      # generic_demod's own: 705 taps, tpf 23 with padding
              ("one_tap", 8, 8),                                # 8 arms of 1 tap
              ("arms64", 64, (64.0, 128.0, 1.0, 0.35, 1408)),   # 64 arms of 23
              ("ragged", 5, 13),                                # a count that is no multiple of the arm count
              ("two", 1, 2),                                    # the smallest prototype
              ("sps2p5", 32, (32.0, 80.0, 1.0, 0.35, 704)),
              ("sps4", 32, (32.0, 128.0, 1.0, 0.35, 1408)))     # tpf 45
GAIN_CASES = ((LOOP_BW, None), (0.0, None), (0.05, 0.5), (0.3, 1.0), (1.0, 0.0), (2.0, None))


def proto(case):
    name, nf, spec = case
    if isinstance(spec, tuple):
        return root_raised_cosine(*spec)
    # a ramp with a bump: taps of both signs, differences of both signs
    i = np.arange(spec, dtype=np.float64)
    return (np.sin(0.9 * i + 0.3) * (1.0 + 0.1 * i)).astype(np.float32)


def bank_case(name):
    return [c for c in BANK_CASES if c[0] == name][0]


# name, sps, osps, init_phase, max_dev, clock offset (of the symbol rate), bank case
RUNS = (("s2_o1", 2.0, 1, 16.0, 1.5, 2e-3, "demod"),
        ("s2_o2", 2.0, 2, 0.0, 1.5, -2e-3, "demod"),
        ("s2p5_o1", 2.5, 1, 0.0, 1.5, 3e-3, "sps2p5"),
        ("s4_o2", 4.0, 2, 31.5, 1.5, -3e-3, "sps4"),
        ("s2_dev0", 2.0, 1, 16.0, 0.0, 2e-3, "demod"),
        ("s2_a64", 2.0, 1, 16.0, 1.5, -3e-3, "arms64"))
RUN_IDS = [r[0] for r in RUNS]


def run_of(name):
    return RUNS[RUN_IDS.index(name)]


_SIG = {}


def signal(seed, sps, drift, n=N, noise=0.01):
    """QPSK shaped with a root raised cosine at 16 samples per symbol, resampled to sps (1 + drift) samples per symbol by
    linear interpolation, a little noise, scaled to unit power: n complex64 items"""
    key = (seed, sps, drift, n, noise)
    if key not in _SIG:
        rng = np.random.RandomState(seed)
        nsym = int(n / sps) + 40
        sym = ((rng.randint(0, 2, nsym) * 2 - 1) + 1j * (rng.randint(0, 2, nsym) * 2 - 1)) / math.sqrt(2)
        L = 16
        t = root_raised_cosine(1.0, L * 1.0, 1.0, 0.35, 11 * L).astype(np.float64)
        up = np.zeros(nsym * L, complex)
        up[::L] = sym
        y = np.convolve(up, t)
        step = L / sps * (1 + drift)
        idx = np.arange(n) * step + 3.3 + 5 * L
        i0 = idx.astype(int)
        fr = idx - i0
        x = y[i0] * (1 - fr) + y[i0 + 1] * fr
        x = x + (rng.randn(n) + 1j * rng.randn(n)) * noise
        x = x / np.sqrt((np.abs(x) ** 2).mean())
        _SIG[key] = x.astype(np.complex64)
        _SIG[key].setflags(write=False)
    return _SIG[key]


def run_signal(run, seed=1):
    return signal(seed, run[1], run[5])


def make(run, taps=None, banks=None):
    name, sps, osps, init, md, drift, bc = run
    case = bank_case(bc)
    return Pcs(sps, LOOP_BW, proto(case) if (taps is None and banks is None) else taps, case[1], init, md, osps, banks=banks)
