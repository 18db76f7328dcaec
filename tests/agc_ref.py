"""numpy restatement of the reference's four gain loops, general/gri_agc_cc.h:53-61, gri_agc_ff.h:51-57,
gri_agc2_cc.h:54-76 and gri_agc2_ff.h:55-75, in float32 scalars with every operation rounded once, and of the chunked
form that agc_cc / agc_ff run in every mode but GENERIC (csrc/agc.hip): clamp-affine triples per chunk of 256 samples
in double, a carry along the chunks with a serial fallback for flagged chunks and negative gains, then the float steps
again from every chunk's start.  tests/golden/ref_agc.npz pins serial() to the reference's own code bit for bit
(test_agc_cpu.py states how it was recorded)."""
import hashlib

import numpy as np

N = 6037
CHUNK = 256
CUTS = (1, 255, 256, 257, 4097)
BLOCKS = ("agc_cc", "agc_ff", "agc2_cc", "agc2_ff")
# (rate, reference, gain, max_gain)
AGC_SETS = ((1e-3, 1, 1, 1000), (1e-2, 1, 1, 0), (1e-3, 1, 1, 2.0), (2e-2, 1, 1, 1.0), (1 / 16000, 1, 1, 1))
# (attack_rate, decay_rate, reference, gain, max_gain); the third is fast enough for the 10e-5 reset to fire
AGC2_SETS = ((1e-2, 1e-3, 1, 1, 1000), (0.6e-1, 1e-3, 1, 1, 100), (0.5, 0.1, 1, 1, 1000))

f32 = np.float32


def sets(block):
    return AGC2_SETS if block.startswith("agc2") else AGC_SETS


def is_cc(block):
    return block.endswith("_cc")


def signal(seed, block="agc_cc"):
    """complex noise through four levels: 1, silence, 30 and 0.02; the _ff blocks take the real part"""
    rng = np.random.default_rng(seed)
    env = np.empty(N)
    env[:1500] = 1.0
    env[1500:2500] = 0.0
    env[2500:4000] = 30.0
    env[4000:] = 0.02
    x = ((rng.standard_normal(N) + 1j * rng.standard_normal(N)) * 0.7 * env).astype(np.complex64)
    return x if is_cc(block) else np.ascontiguousarray(x.real)


class Run(object):
    """out: the outputs; gains: the gain in front of every sample and after the last (n + 1 floats); gain: the last;
    clamped / resets: how often the max_gain clamp and agc2's 10e-5 reset fired"""

    def __init__(self, out, gains, clamped=0, resets=0):
        self.out, self.gains, self.gain, self.clamped, self.resets = out, gains, gains[-1], clamped, resets


def _step(block, p, g, xr, xi):
    """one scale(): (out_re, out_im, gain after, clamped, reset) in float32"""
    o_re = xr * g
    if is_cc(block):
        o_im = xi * g
        m = np.sqrt(o_re * o_re + o_im * o_im)
    else:
        o_im = f32(0)
        m = np.abs(o_re)
    reset = False
    if block == "agc_cc":
        rate, ref, mx = p
        g = g + rate * (ref - m)
    elif block == "agc_ff":
        rate, ref, mx = p
        g = g + (ref - m) * rate
    else:
        att, dec, ref, mx = p
        if block == "agc2_cc":
            tmp = -ref + m
            r = att if tmp > g else dec
        else:
            tmp = m - ref
            r = att if np.abs(tmp) > g else dec
        g = g - tmp * r
        if g < 0.0:
            g = f32(10e-5)
            reset = True
    clamped = bool(mx > 0.0 and g > mx)
    if clamped:
        g = mx
    return o_re, o_im, g, clamped, reset


def _params(block, params):
    """the parameters as float32 without the gain, and the gain"""
    v = [f32(t) for t in params]
    if block.startswith("agc2"):
        return (v[0], v[1], v[2], v[4]), v[3]
    return (v[0], v[1], v[3]), v[2]


def serial(block, x, params, gain=None):
    """scaleN over x; `gain` overrides the parameter set's start gain"""
    p, g0 = _params(block, params)
    g = g0 if gain is None else f32(gain)
    cc = is_cc(block)
    x = np.asarray(x, np.complex64 if cc else np.float32)
    n = len(x)
    out = np.zeros(n, x.dtype)
    outf = out.view(np.float32)         # the parts are stored as they are: a sum would lose a zero's sign
    gains = np.zeros(n + 1, np.float32)
    xr = x.real if cc else x
    xi = x.imag if cc else np.zeros(n, np.float32)
    clamped = resets = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            gains[i] = g
            o_re, o_im, g, c, r = _step(block, p, g, xr[i], xi[i])
            if cc:
                outf[2 * i], outf[2 * i + 1] = o_re, o_im
            else:
                outf[i] = o_re
            clamped += c
            resets += r
    gains[n] = g
    return Run(out, gains, clamped, resets)


def mag64(x):
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return np.sqrt(x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2)
    return np.abs(x.astype(np.float64))


def exact64(block, x, params, gain=None):
    """the recurrence of agc_cc / agc_ff in float64: g += rate (reference - |x| |g|), then the clamp.  Returns the n + 1
    gains."""
    p, g0 = _params(block, params)
    rate, ref, mx = (float(t) for t in p)
    g = float(g0 if gain is None else f32(gain))
    m = mag64(x)
    gains = np.zeros(len(m) + 1)
    with np.errstate(all="ignore"):
        for i in range(len(m)):
            gains[i] = g
            g = g + rate * (ref - m[i] * abs(g))
            if mx > 0.0 and g > mx:
                g = mx
    gains[-1] = g
    return gains


def compose(f, s):
    """clamp-affine maps g -> min(A g + B, C), `f` first and then `s`; C = inf means no clamp"""
    c = np.inf if f[2] == np.inf else s[0] * f[2] + s[1]
    return (s[0] * f[0], s[0] * f[1] + s[1], min(c, s[2]))


def apply(t, g):
    v = t[0] * g + t[1]
    return t[2] if v > t[2] else v


def can_chunk(block, params, n):
    p, _ = _params(block, params)
    return (not block.startswith("agc2") and n > CHUNK and all(np.isfinite(t) for t in p) and p[0] >= 0 and p[1] >= 0)


def chunk_triples(block, x, params):
    """per chunk of one call: the composed triple from the identity and the flag (some sample with !(a >= 0))"""
    p, _ = _params(block, params)
    rate, ref, mx = (float(t) for t in p)
    b = rate * ref
    M = mx if mx > 0.0 else np.inf
    with np.errstate(all="ignore"):
        a = 1.0 - rate * mag64(x)
    tri, flags = [], []
    for c0 in range(0, len(a), CHUNK):
        t = (1.0, 0.0, np.inf)
        for ai in a[c0:c0 + CHUNK]:
            t = compose(t, (ai, b, M))
        tri.append(t)
        flags.append(bool(np.any(~(a[c0:c0 + CHUNK] >= 0.0))))
    return tri, flags


def chunked_call(block, x, params, gain):
    """one work call of the chunked form from `gain`"""
    if not can_chunk(block, params, len(x)):
        return serial(block, x, params, gain)
    tri, flags = chunk_triples(block, x, params)
    g = float(f32(gain))
    starts = []
    for k, (t, fl) in enumerate(zip(tri, flags)):
        starts.append(f32(g))
        if not fl and g >= 0.0:
            g = apply(t, g)
        else:
            g = float(serial(block, x[k * CHUNK:(k + 1) * CHUNK], params, f32(g)).gain)
    outs, gains, clamped = [], [], 0
    for k, s in enumerate(starts):
        r = serial(block, x[k * CHUNK:(k + 1) * CHUNK], params, s)
        outs.append(r.out)
        gains.append(r.gains[:-1])
        clamped += r.clamped
    gains.append(r.gains[-1:])
    return Run(np.concatenate(outs), np.concatenate(gains), clamped)


def in_calls(fn, block, x, params, cuts=(), gain=None):
    """fn (serial or chunked_call) over x cut into calls at `cuts`, the gain carried from call to call"""
    _, g0 = _params(block, params)
    g = g0 if gain is None else f32(gain)
    edges = [0] + [c for c in cuts if 0 < c < len(x)] + [len(x)]
    outs, gains, clamped, resets = [], [], 0, 0
    for a, b in zip(edges[:-1], edges[1:]):
        r = fn(block, x[a:b], params, g)
        g = r.gain
        outs.append(r.out)
        gains.append(r.gains[:-1])
        clamped += r.clamped
        resets += r.resets
    gains.append(np.array([g], np.float32))
    return Run(np.concatenate(outs), np.concatenate(gains), clamped, resets)


def chunked(block, x, params, cuts=(), gain=None):
    return in_calls(chunked_call, block, x, params, cuts, gain)


def deviation(gains, g64):
    """largest deviation of a gain track from the float64 recurrence's, relative to that track's peak gain"""
    return float(np.max(np.abs(gains.astype(np.float64) - g64)) / np.max(np.abs(g64)))


def bound(dev_ref):
    return 2.0 * dev_ref + 4.0 * 2.0 ** -23


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
