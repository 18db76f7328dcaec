"""Restatement of the reference's constellation objects (gr-digital/lib/digital_constellation.cc), of
digital_constellation_receiver_cb.cc:80-122, digital_constellation_decoder_cb.cc:63-78, gr_diff_decoder_bb.cc:48-61,
gr_map_bb.cc:36-60 and gr_unpack_k_bits_bb.cc, and of the Python helpers that build constellations (gr-digital/python/
psk.py, qam.py, utils/gray_code.py, utils/mod_codes.py), in float32 with every operation rounded once and double where
the reference's expression is double.  arg, cos and sin of a float are the float-rounded float64 functions (what
csrc/constellation.h and the device's GRHIP_MODE_GENERIC compute), which is glibc's atan2f / sincosf to within an ulp
but not to the bit; the receiver can also run in float64 throughout (receiver64), the yardstick of the deviation
contract.  tests/golden/ref_constellation.npz pins all of it to the reference's own code (test_constellation_cpu.py
states how it was recorded).  The loop arithmetic is carrier_ref.Loop's."""
import math

import numpy as np

import carrier_ref as CR
from carrier_ref import bits, bound, circ, digest, in_calls  # noqa: F401  (the tests take them from here)

N = 6037
CUT = 4097
WIN = CR.WIN
f32 = np.float32
TWOPI = 2 * math.pi             # digital_constellation.cc:38 (2*M_PI)
SQRT_TWO = f32(0.707107)        # :39
MAX_SECTORS = 16384


# ---- utils/gray_code.py, utils/mod_codes.py ------------------------------------------------------------------------
def gray_code(length):
    gcs, lp2, np2, i = [0, 1], 2, 4, 2
    while len(gcs) < length:
        gcs.append(i + i // 2 if i == lp2 else gcs[2 * lp2 - 1 - i] + lp2)
        i += 1
        if i == np2:
            lp2, np2 = i, i * 2
    return gcs[:length]


def invert_code(code):
    return [a for (b, a) in sorted((b, a) for (a, b) in enumerate(code))]


# ---- float32 arithmetic on arrays ------------------------------------------------------------------------------------
def arg_f(im, re):
    return np.arctan2(np.asarray(im, np.float32).astype(np.float64), np.asarray(re, np.float32).astype(np.float64)).astype(np.float32)


def cmul(a_re, a_im, b_re, b_im):
    """(a_re + j a_im)(b_re + j b_im) as g++ forms it for finite operands: ac - bd, ad + bc"""
    return a_re * b_re - a_im * b_im, a_re * b_im + a_im * b_re


class Constellation(object):
    """kind: bpsk, qpsk, dqpsk, 8psk, calcdist, psk or rect; points: complex64, arity * dim of them"""

    def __init__(self, kind, points=(), pre_diff_code=(), rotational_symmetry=0, dimensionality=1, n_sectors=0,
                 real_sectors=0, imag_sectors=0, width_real=0.0, width_imag=0.0):
        s = SQRT_TWO
        self.kind = kind
        if kind == "bpsk":                                          # :383-391
            points, pre_diff_code, rotational_symmetry = [-1, 1], [], 2
        elif kind == "qpsk":                                        # :406-431; d_apply_pre_diff_code stays false (:62)
            points, pre_diff_code, rotational_symmetry = [complex(-s, -s), complex(s, -s), complex(-s, s), complex(s, s)], [0, 2, 3, 1], 4
        elif kind == "dqpsk":                                       # :468-490
            points, pre_diff_code, rotational_symmetry = [complex(s, s), complex(-s, s), complex(-s, -s), complex(s, -s)], [0, 1, 3, 2], 4
        elif kind == "8psk":                                        # :520-536
            angle = f32(math.pi / 8.0)
            a = [float(f32(m) * angle) for m in (1, 7, 15, 9, 3, 5, 13, 11)]
            points, pre_diff_code, rotational_symmetry = [complex(f32(math.cos(t)), f32(math.sin(t))) for t in a], [], 8
        elif kind == "psk":
            rotational_symmetry = len(points)
        # the base constructor (:52-57) for the kinds that take a code; of the fixed ones only dqpsk sets it (:485)
        self.apply_pre_diff_code = kind == "dqpsk" or (kind in ("calcdist", "psk", "rect") and len(pre_diff_code) != 0)
        if len(pre_diff_code) not in (0, len(points)):
            raise ValueError("The constellation and pre-diff code must be of the same length.")
        if dimensionality < 1 or len(points) % dimensionality or len(points) == 0:
            raise ValueError("Constellation vector size must be a multiple of the dimensionality.")
        self.points = np.asarray(points, np.complex64)
        self.pre_diff_code = [int(c) for c in pre_diff_code]
        self.rotational_symmetry, self.dimensionality = int(rotational_symmetry), int(dimensionality)
        self.arity = len(self.points) // self.dimensionality
        if self.arity > 256:
            raise ValueError("at most 256 points")
        self.n_real, self.n_imag = int(real_sectors), int(imag_sectors)
        self.w_real, self.w_imag = f32(width_real), f32(width_imag)
        self.n_sectors = int(n_sectors) if kind == "psk" else self.n_real * self.n_imag
        self.sector_values = None
        if kind in ("psk", "rect"):
            if not 1 <= self.n_sectors <= MAX_SECTORS:
                raise ValueError("1 .. 16384 sectors")
            sec = np.arange(self.n_sectors)
            if kind == "psk":                                       # :368-374
                ph = (sec * TWOPI / self.n_sectors).astype(np.float32).astype(np.float64)
                c = (np.cos(ph).astype(np.float32) + 1j * np.sin(ph).astype(np.float32)).astype(np.complex64)
            else:                                                   # :322-333
                rs = (sec.astype(np.float32) / f32(self.n_imag)).astype(np.uint32).astype(np.int64)
                im = sec - rs * self.n_imag
                c = (((rs + 0.5 - self.n_real / 2.0) * float(self.w_real)).astype(np.float32)
                     + 1j * ((im + 0.5 - self.n_imag / 2.0) * float(self.w_imag)).astype(np.float32)).astype(np.complex64)
            self.sector_values = self.closest(c).astype(np.uint32)

    def bits_per_symbol(self):
        return int(math.floor(math.log(float(len(self.points))) / self.dimensionality / math.log(2.0)))

    def closest(self, x):
        """get_closest_point (:96-113) of items of `dimensionality` samples: float norm, first strict minimum"""
        d = self.dimensionality
        x = np.asarray(x, np.complex64).reshape(-1, d)
        p = self.points.reshape(self.arity, d)
        best = np.zeros(len(x), np.int64)
        best_d = None
        for j in range(self.arity):
            dist = np.zeros(len(x), np.float32)
            for i in range(d):
                dr, di = x[:, i].real - p[j, i].real, x[:, i].imag - p[j, i].imag
                dist = dist + (dr * dr + di * di)
            if best_d is None:
                best_d = dist
            else:
                lt = dist < best_d
                best[lt], best_d = j, np.where(lt, dist, best_d)
        return best

    def sector(self, x):
        x = np.asarray(x, np.complex64)
        if self.kind == "psk":                                      # :355-365
            phase = arg_f(x.imag, x.real)
            width = f32(TWOPI / self.n_sectors)
            s = np.floor((phase / width).astype(np.float64) + 0.5)
            s = np.where(s < 0, s + self.n_sectors, s)
            return np.clip(np.nan_to_num(s, nan=0.0), 0, self.n_sectors - 1).astype(np.int64)

        def axis(v, w, n):                                          # :305-309
            with np.errstate(all="ignore"):
                t = np.trunc((v / w).astype(np.float64) + n / 2.0)
            return np.clip(np.nan_to_num(t, nan=0.0), 0, n - 1).astype(np.int64)
        return axis(x.real, self.w_real, self.n_real) * self.n_imag + axis(x.imag, self.w_imag, self.n_imag)

    def decision_maker(self, x):
        """one decision per item of `dimensionality` samples"""
        x = np.asarray(x, np.complex64)
        re, im = x.real, x.imag
        k = self.kind
        if k == "bpsk":
            return (re > 0).astype(np.int64)
        if k == "qpsk":
            return 2 * (im > 0).astype(np.int64) + (re > 0)
        if k == "dqpsk":
            return np.where(re > 0, np.where(im > 0, 0, 3), np.where(im > 0, 1, 2)).astype(np.int64)
        if k == "8psk":
            return (np.where(np.abs(re) <= np.abs(im), 4, 0) | np.where(re <= 0, 1, 0) | np.where(im <= 0, 2, 0)).astype(np.int64)
        if k in ("psk", "rect"):
            return self.sector_values[self.sector(x)].astype(np.int64)
        return self.closest(x)

    def decision_maker_pe(self, x):
        """(index, phase error) per item: :115-123, d_constellation[index + d] as the reference has it"""
        d = self.dimensionality
        x = np.asarray(x, np.complex64).reshape(-1, d)
        idx = self.decision_maker(x.reshape(-1))
        pe = np.zeros(len(x), np.float32)
        for i in range(d):
            p = self.points[idx + i]
            zr, zi = cmul(x[:, i].real, x[:, i].imag, p.real, -p.imag)
            pe = pe + (-arg_f(zi, zr))
        return idx, pe


def psk_constellation(m=4, gray=True):
    """psk.py psk_constellation(m, mod_code): mod_code GRAY_CODE or NO_CODE"""
    k = math.log(m) / math.log(2.0)
    if k != int(k):
        raise ValueError("Number of constellation points must be a power of two.")
    pts = [complex(np.exp(2 * math.pi * 1j * i / m)) for i in range(m)]
    return Constellation("psk", pts, gray_code(m) if gray else [], n_sectors=m)


def _get_bits(x, n, k):
    return (x >> n) % (2 ** k)


def qam_points(m=16, differential=True, gray=False):
    """qam.py make_differential_constellation / make_non_differential_constellation"""
    k = int(math.log(m) / math.log(2.0))
    if m < 4 or 4 ** (k // 2) != m:
        raise ValueError("m must be a power of 4 integer.")
    if differential:
        side = int(pow(m, 0.5) / 2)
        i_gcs = dict((v, key) for key, v in enumerate(gray_code(side))) if gray else dict((i, i) for i in range(side))
        step = 1 / (side - 0.5)
        g = [(i_gcs[gc] + 0.5) * step for gc in range(side)]
        quad = (lambda x, y: complex(g[x], g[y]), lambda x, y: complex(-g[y], g[x]), lambda x, y: complex(-g[x], -g[y]),
                lambda x, y: complex(g[y], -g[x]))
        h = (k - 2) // 2
        return [quad[_get_bits(i, k - 2, 2)](_get_bits(i, h, h), _get_bits(i, 0, h)) for i in range(m)]
    side = int(pow(m, 0.5))
    i_gcs = invert_code(gray_code(side)) if gray else list(range(side))
    step = 2.0 / (side - 1)
    g = [-1 + i_gcs[gc] * step for gc in range(side)]
    return [complex(g[_get_bits(i, k // 2, k // 2)], g[_get_bits(i, 0, k // 2)]) for i in range(m)]


def qam_constellation(m=16, differential=True, gray=False):
    side = int(math.sqrt(m))
    width = 2.0 / (side - 1)
    return Constellation("rect", qam_points(m, differential, gray), [], 4, real_sectors=side, imag_sectors=side,
                         width_real=width, width_imag=width)


# ---- the byte blocks ----------------------------------------------------------------------------------------------------
def diff_decoder(x, modulus, prev=0):
    """gr_diff_decoder_bb.cc:56-58: the int difference converted to unsigned, % modulus, narrowed to a byte"""
    x = np.asarray(x, np.uint8).astype(np.int64)
    d = x - np.concatenate(([int(prev)], x[:-1]))
    return (((d + (1 << 32)) % (1 << 32)) % int(modulus)).astype(np.uint8)


def map_table(m):
    t = np.arange(256)
    m = np.asarray(m[:256], np.int64)
    t[:len(m)] = m
    return t.astype(np.uint8)          # `d_map[i] = map[i]`: an int narrowed to a byte


def map_bb(x, m):
    return map_table(m)[np.asarray(x, np.uint8)]


def unpack_k_bits(x, k):
    x = np.asarray(x, np.uint8)
    return np.stack([(x >> (k - 1 - j)) & 1 for j in range(k)], axis=1).reshape(-1).astype(np.uint8)


def demod_tail(c, sym, differential, gray_coded, prev=0):
    """generic_mod_demod.py:296-313 behind the receiver"""
    y = np.asarray(sym, np.uint8)
    if differential:
        y = diff_decoder(y, c.arity, prev)
    if gray_coded and c.apply_pre_diff_code:
        y = map_bb(y, invert_code(c.pre_diff_code))
    return unpack_k_bits(y, c.bits_per_symbol())


# ---- the receiver -------------------------------------------------------------------------------------------------------
class Run(object):
    """sym, err, phase, freq: the four outputs (phase and freq AFTER the update); phases: n + 1, in front of every
    sample and after the last; derot: the derotated samples"""


def receiver(loop, c, x):
    """one general_work call in float32; advances `loop` (a carrier_ref.Loop)"""
    assert c.dimensionality == 1
    x = np.asarray(x, np.complex64)
    n = len(x)
    r = Run()
    r.sym, r.err, r.phase, r.freq = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    r.phases, r.derot = np.zeros(n + 1, np.float32), np.zeros(n, np.complex64)
    xr, xi = x.real, x.imag
    pts = c.points
    one = np.zeros(1, np.complex64)
    for i in range(n):
        r.phases[i] = loop.phase
        ang = float(loop.phase)
        cs, sn = f32(math.cos(ang)), f32(math.sin(ang))             # gr_expj(d_phase), :104
        s_re, s_im = cmul(cs, sn, xr[i], xi[i])                     # nco * sample, :105
        one[0] = complex(s_re, s_im)
        k = int(c.decision_maker(one)[0])
        p = pts[k]
        z_re, z_im = cmul(s_re, s_im, p.real, -p.imag)
        e = f32(0) + (-f32(math.atan2(float(z_im), float(z_re))))   # `*phase_error = 0; *phase_error += -arg(...)`
        loop.step(e)
        r.sym[i], r.err[i], r.phase[i], r.freq[i], r.derot[i] = k, e, loop.phase, loop.freq, one[0]
    r.phases[n] = loop.phase
    return r


def receiver64(loop, c, x):
    """the same recurrence in float64 throughout, on the same input and the same (float) gains, limits and points"""
    x = np.asarray(x, np.complex64)
    n = len(x)
    r = Run()
    r.sym, r.err, r.phase, r.freq = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n), np.zeros(n)
    r.phases, r.derot = np.zeros(n + 1), np.zeros(n, np.complex128)
    ph, fq = float(loop.phase), float(loop.freq)
    al, be, mx, mn = float(loop.alpha), float(loop.beta), float(loop.max_freq), float(loop.min_freq)
    pts = c.points.astype(np.complex128)
    for i in range(n):
        r.phases[i] = ph
        s = complex(math.cos(ph), math.sin(ph)) * complex(x[i])
        k = decide64(c, s)
        z = s * pts[k].conjugate()
        e = -math.atan2(z.imag, z.real)
        fq = fq + be * e
        ph = ph + fq + al * e
        while ph > TWOPI:
            ph -= TWOPI
        while ph < -TWOPI:
            ph += TWOPI
        fq = mx if fq > mx else (mn if fq < mn else fq)
        r.sym[i], r.err[i], r.phase[i], r.freq[i], r.derot[i] = k, e, ph, fq, s
    r.phases[n] = ph
    return r


def decide64(c, s):
    """the decision on a float64 sample: the same rules without float32 rounding"""
    re, im, k = s.real, s.imag, c.kind
    if k == "bpsk":
        return int(re > 0)
    if k == "qpsk":
        return 2 * int(im > 0) + int(re > 0)
    if k == "dqpsk":
        return (0 if im > 0 else 3) if re > 0 else (1 if im > 0 else 2)
    if k == "8psk":
        return (4 if abs(re) <= abs(im) else 0) | (1 if re <= 0 else 0) | (2 if im <= 0 else 0)
    if k == "psk":
        sec = int(math.floor(math.atan2(im, re) / (TWOPI / c.n_sectors) + 0.5))
        return int(c.sector_values[sec % c.n_sectors])
    if k == "rect":
        a = min(max(int(re / float(c.w_real) + c.n_real / 2.0), 0), c.n_real - 1)
        b = min(max(int(im / float(c.w_imag) + c.n_imag / 2.0), 0), c.n_imag - 1)
        return int(c.sector_values[a * c.n_imag + b])
    return int(np.argmin(np.abs(s - c.points.astype(np.complex128)) ** 2))


def guard(c, derot64, rel=1e-3):
    """the decision guard: every float64 derotated sample keeps its decision when moved by rel * |s| in eight directions"""
    for s in derot64:
        k = decide64(c, complex(s))
        for j in range(8):
            if decide64(c, complex(s) + rel * abs(s) * complex(math.cos(j * math.pi / 4), math.sin(j * math.pi / 4))) != k:
                return False
    return True


# ---- the recorded cases -------------------------------------------------------------------------------------------------
LOOP_BW, FMAX, FMIN = 2 * math.pi / 100, 0.25, -0.25
# name, constellation, seed, noise, frequency offset
RX_CASES = (
    ("bpsk", lambda: Constellation("bpsk"), 11, 0.02, 0.01),
    ("qpsk", lambda: Constellation("qpsk"), 12, 0.02, 0.01),
    ("dqpsk", lambda: Constellation("dqpsk"), 13, 0.02, 0.01),
    ("8psk", lambda: Constellation("8psk"), 14, 0.02, 0.01),
    ("psk16", lambda: psk_constellation(16, True), 15, 0.02, 0.01),
    ("psk32", lambda: psk_constellation(32, True), 16, 0.008, 0.01),
    ("rect16", lambda: qam_constellation(16, True, False), 17, 0.02, 0.01),
    ("limit", lambda: Constellation("qpsk"), 18, 0.02, 0.3),        # the offset exceeds fmax: frequency_limit acts
)
DEC_KINDS = (
    [("bpsk", lambda: Constellation("bpsk")), ("qpsk", lambda: Constellation("qpsk")), ("dqpsk", lambda: Constellation("dqpsk")),
     ("8psk", lambda: Constellation("8psk"))]
    + [("psk%d%s" % (m, "g" if gr else "n"), lambda m=m, gr=gr: psk_constellation(m, gr)) for m in (2, 4, 8, 16, 32) for gr in (True, False)]
    + [("rect16", lambda: qam_constellation(16, True, False)),
       ("calcdist4", lambda: Constellation("calcdist", [1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j], [0, 1, 3, 2], 4, 1)),
       ("calcdist2d", lambda: Constellation("calcdist", [1, 1, 1, -1, -1, 1, -1, -1, 1j, 0.5], [], 1, 2))])


RX_FULL = ("qpsk", "rect16")                # the fixture keeps these cases' error and frequency tracks whole
SECTIONS, SEC_LEN = (0, 1400, 4000, 5781), 256      # ... and these sections of the others'


def secs(a):
    return np.concatenate([a[s:s + SEC_LEN] for s in SECTIONS])


def rx_loop():
    return CR.Loop(LOOP_BW, FMAX, FMIN)


def rx_signal(case):
    """6037 random symbols of the case's constellation, rotated by 0.15 rad + offset rad/sample, plus noise, on a grid
    of 2^-13 (so the samples do not hang on the last bit of this machine's exp)"""
    name, make, seed, noise, offset = case
    c = make()
    rng = np.random.RandomState(seed)
    sy = rng.randint(0, c.arity, N)
    w = rng.standard_normal(2 * N).reshape(N, 2)
    x = c.points[sy].astype(np.complex128) * np.exp(-1j * (0.15 + offset * np.arange(N))) + noise * (w[:, 0] + 1j * w[:, 1])
    q = 8192.0
    return (np.round(x.real * q) / q + 1j * np.round(x.imag * q) / q).astype(np.complex64)


def decision_samples():
    """4096 samples: random ones, points on the axes, on |re| = |im|, zeros of both signs, denormals, tiny and huge
    magnitudes, and points beside the borders of the 16-point grid"""
    rng = np.random.RandomState(4096)
    x = (1.2 * (rng.standard_normal(4096) + 1j * rng.standard_normal(4096))).astype(np.complex64)
    v = x.view(np.float32).reshape(-1, 2)
    v[3000:3064, 1] = 0.0
    v[3064:3128, 1] = -0.0
    v[3128:3192, 0] = 0.0
    v[3192:3256, 0] = -0.0
    sg = np.array([1, -1], np.float32)
    v[3256:3512, 1] = np.abs(v[3256:3512, 0]) * sg[rng.randint(0, 2, 256)]
    v[3512:3520] = [[0, 0], [-0.0, 0], [0, -0.0], [-0.0, -0.0], [0, 1e-45], [1e-45, 0], [-1e-45, 1e-45], [1e-45, -1e-45]]
    v[3520:3584] *= f32(1e-41)                                      # denormals
    v[3584:3616] *= f32(1e-30)
    v[3616:3648] *= f32(1e8)                                        # the grid's `int(re / width + 2)` is still defined
    g = np.array([-2 / 3.0, 0.0, 2 / 3.0])                          # the grid's inner borders, and a step to each side
    t = (g[rng.randint(0, 3, 192)] + 1e-6 * rng.randint(-3, 4, 192)).astype(np.float32)
    v[3648:3744, 0] = t[:96]
    v[3744:3840, 1] = t[96:]
    return x
