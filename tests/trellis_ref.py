"""Test-only Python restatement of gr-trellis' coding layer: fsm (gr-trellis/src/lib/fsm.cc:34-452, base.cc),
trellis_encoder_XX (trellis_encoder_XX.cc.t:50-75), calc_metric (calc_metric.cc:29-72, :212-250),
digital_constellation::calc_metric (digital_constellation.cc:160-201) and viterbi_algorithm (core_algorithms.cc:45-109).
Every float is a float32 numpy value, so every add, subtract and multiply rounds once, as the reference's do.  The decoder
runs all blocks and all states of a step as arrays: within a step no state depends on another, and the predecessors of
a state are still tried one after the other in PS[j] order.

tests/golden/ref_trellis.npz was recorded on the CPU from the reference's own files compiled unchanged with g++ -O2:
fsm.cc, base.cc, core_algorithms.cc, calc_metric.cc, interleaver.cc and quicksort_index.cc (core_algorithms.h includes
the interleaver) against gruel/attributes.h for the export macros, and digital_constellation.cc with gr_fast_atan2f.cc
against stubs that map boost::shared_ptr and boost::enable_shared_from_this onto std and leave gr_io_signature.h empty.
The work loops of trellis_encoder_XX.cc.t, trellis_metrics_X.cc.t and trellis_viterbi_X.cc.t were expanded by hand around
those calls.  The driver and the stubs are not in the repository.  The inputs of every case are made by the functions
below from a seed; the fixture holds what the reference answered: every table of every FSM (PS, PI, TMl, TMi included)
and the outputs of the encoder, metrics, decoder and combined-decoder cases (viterbi_algorithm_combined through the
expanded loop of trellis_viterbi_combined_XX.cc.t).  Arrays above KEEP * 4 items are kept as length, first and last KEEP
items and SHA-256.  The .fsm files under tests/golden/fsm/ are the reference's data files.

The decoder cases never reach a state without predecessors in the traceback (the reference indexes an empty vector
there); the handle's rule for it -- symbol 0, stay, count -- is restated here and tested on the device only."""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_trellis.npz")
FSM_DIR = os.path.join(HERE, "golden", "fsm")
KEEP = 512
INF = np.float32(1.0e9)
FLT_MAX = np.finfo(np.float32).max
EUCLIDEAN, HARD_SYMBOL, HARD_BIT = 200, 201, 202
F32 = np.float32

_FX = None


def fixture():
    global _FX
    if _FX is None:
        with np.load(GOLDEN) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pack(store, key, a):
    """an array into the fixture: whole, or as length, head, tail and digest"""
    a = np.ascontiguousarray(a)
    if a.size <= 4 * KEEP:
        store[key] = a
    else:
        store[key + "_len"] = np.int64(a.size)
        store[key + "_head"] = a.reshape(-1)[:KEEP].copy()
        store[key + "_tail"] = a.reshape(-1)[-KEEP:].copy()
        store[key + "_sha"] = np.array(digest(a))


def matches(key, a, fx=None):
    """is `a` what the fixture keeps under `key`?  Floats are compared as bit patterns, NaN against NaN as equal."""
    fx = fixture() if fx is None else fx
    a = np.ascontiguousarray(a).reshape(-1)

    def same(x, y):
        x, y = np.ascontiguousarray(x).reshape(-1), np.ascontiguousarray(y).reshape(-1)
        if x.dtype != y.dtype or x.shape != y.shape:
            return False
        if x.dtype.kind in "fc":
            xf, yf = x.view(np.float32), y.view(np.float32)
            nan = np.isnan(xf) & np.isnan(yf)
            return bool(np.all(nan | (xf.view(np.uint32) == yf.view(np.uint32))))
        return bool(np.array_equal(x, y))
    if key in fx:
        return same(a, fx[key])
    if int(fx[key + "_len"]) != a.size or not same(a[:KEEP], fx[key + "_head"]) or not same(a[-KEEP:], fx[key + "_tail"]):
        return False
    if a.dtype.kind in "fc" and np.isnan(a.view(np.float32)).any():
        return True                                 # the payload of a NaN is the platform's: head and tail only
    return digest(a) == str(fx[key + "_sha"])


# ---- base.cc -----------------------------------------------------------------------------------------------------------
def dec2base(num, base, l):
    s = [0] * l
    n = num
    for i in range(l):
        s[l - i - 1] = n % base
        n //= base
    return s


def base2dec(s, base):
    num = 0
    for d in s:
        num = num * base + d
    return num


def dec2bases(num, bases):
    l = len(bases)
    s = [0] * l
    n = num
    for i in range(l):
        s[l - i - 1] = n % bases[l - i - 1]
        n //= bases[l - i - 1]
    return s


def bases2dec(s, bases):
    num = 0
    for d, b in zip(s, bases):
        num = num * b + d
    return num


# ---- fsm ---------------------------------------------------------------------------------------------------------------
class Fsm(object):
    """fsm(I, S, O, NS, OS) with PS, PI made at once and TMl, TMi on first use (find_es is a serial sweep)"""

    def __init__(self, I, S, O, NS, OS):
        self.I, self.S, self.O = int(I), int(S), int(O)
        self.NS = [int(v) for v in NS]
        self.OS = [int(v) for v in OS]
        assert len(self.NS) == len(self.OS) == self.I * self.S
        self.PS = [[] for _ in range(self.S)]       # generate_PS_PI, fsm.cc:377-395: ascending (state, input)
        self.PI = [[] for _ in range(self.S)]
        for ii in range(self.S):
            for jj in range(self.I):
                i = self.NS[ii * self.I + jj]
                self.PS[i].append(ii)
                self.PI[i].append(jj)
        self._tm = None

    def tables(self):
        return self.I, self.S, self.O, self.NS, self.OS

    def _generate_TM(self):                          # fsm.cc:401-452
        S, I, NS = self.S, self.I, self.NS
        TMi = [-1] * (S * S)
        TMl = [S] * (S * S)
        for i in range(S):
            TMl[i * S + i] = 0
        connected = True
        for es in range(S):
            done = False
            attempts = 0
            while not done and attempts < S - 1:
                done = True                          # find_es(es)
                for s in range(S):
                    if TMl[s * S + es] < S:
                        continue
                    minl, mini = S, -1
                    for i in range(I):
                        c = 1 + TMl[NS[s * I + i] * S + es]
                        if c < minl:
                            minl, mini = c, i
                    if mini != -1:
                        TMl[s * S + es] = minl
                        TMi[s * S + es] = mini
                    else:
                        done = False
                attempts += 1
            if not done and S > 1:
                connected = False
        self._tm = (TMl, TMi, connected)

    @property
    def TMl(self):
        if self._tm is None:
            self._generate_TM()
        return self._tm[0]

    @property
    def TMi(self):
        if self._tm is None:
            self._generate_TM()
        return self._tm[1]

    @property
    def connected(self):
        if self._tm is None:
            self._generate_TM()
        return self._tm[2]


def fsm_from_text(text):
    """fsm(const char *name), fsm.cc:82-117, on the file's text"""
    tok = text.split()
    I, S, O = int(tok[0]), int(tok[1]), int(tok[2])
    n = I * S
    return Fsm(I, S, O, [int(t) for t in tok[3:3 + n]], [int(t) for t in tok[3 + n:3 + 2 * n]])


def fsm_file_text(name):
    with open(os.path.join(FSM_DIR, name + ".fsm")) as f:
        return f.read()


def fsm_from_generator(k, n, G):
    """fsm.cc:125-224"""
    max_mem_x = [-1] * k
    max_mem = -1
    for i in range(k):
        for j in range(n):
            mem = -1
            if G[i * n + j] != 0:
                mem = int(np.log(float(G[i * n + j])) / np.log(2.0))
            max_mem_x[i] = max(max_mem_x[i], mem)
            max_mem = max(max_mem, mem)
    I, S, O = 1 << k, 1 << sum(max_mem_x), 1 << n
    Gb = [dec2base(G[j], 2, max_mem + 1) for j in range(k * n)]
    bases_x = [1 << m for m in max_mem_x]
    NS, OS = [0] * (I * S), [0] * (I * S)
    for s in range(S):
        sx = dec2bases(s, bases_x)
        for i in range(I):
            inb = dec2base(i, 2, k)
            nsx = [(inb[j] * bases_x[j] + sx[j]) // 2 for j in range(k)]
            NS[s * I + i] = bases2dec(nsx, bases_x)
            tb = [dec2base(inb[j] * bases_x[j] + sx[j], 2, max_mem + 1) for j in range(k)]
            outb = [0] * n
            for nn in range(n):
                for j in range(k):
                    for m in range(max_mem + 1):
                        outb[nn] = (outb[nn] + Gb[j * n + nn][m] * tb[j][m]) % 2
            OS[s * I + i] = base2dec(outb, 2)
    return Fsm(I, S, O, NS, OS)


def fsm_from_isi(mod_size, ch_length):
    """fsm.cc:234-253"""
    I = mod_size
    S = int(pow(1.0 * I, 1.0 * ch_length - 1) + 0.5)
    O = S * I
    NS, OS = [0] * (I * S), [0] * (I * S)
    for s in range(S):
        for i in range(I):
            t = i * S + s
            NS[s * I + i] = t // I
            OS[s * I + i] = t
    return Fsm(I, S, O, NS, OS)


def fsm_from_cpm(P, M, L):
    """fsm.cc:267-292"""
    I = M
    S = int(pow(1.0 * M, 1.0 * L - 1) + 0.5) * P
    O = int(pow(1.0 * M, 1.0 * L) + 0.5) * P
    NS, OS = [0] * (I * S), [0] * (I * S)
    for s in range(S):
        for i in range(I):
            s1, v = s // P, s % P
            ns1 = (i * int(pow(1.0 * M, 1.0 * (L - 1)) + 0.5) + s1) // M
            nv = (i + v) % P if L == 1 else (s1 % M + v) % P
            NS[s * I + i] = ns1 * P + nv
            OS[s * I + i] = i * S + s
    return Fsm(I, S, O, NS, OS)


def fsm_from_joint(f1, f2):
    """fsm.cc:307-329"""
    I, S, O = f1.I * f2.I, f1.S * f2.S, f1.O * f2.O
    NS, OS = [0] * (I * S), [0] * (I * S)
    for s in range(S):
        for i in range(I):
            s1, s2, i1, i2 = s // f2.S, s % f2.S, i // f2.I, i % f2.I
            NS[s * I + i] = f1.NS[s1 * f1.I + i1] * f2.S + f2.NS[s2 * f2.I + i2]
            OS[s * I + i] = f1.OS[s1 * f1.I + i1] * f2.O + f2.OS[s2 * f2.I + i2]
    return Fsm(I, S, O, NS, OS)


def fsm_from_radix(f, n):
    """fsm.cc:338-364"""
    I, S, O = int(pow(1.0 * f.I, 1.0 * n) + 0.5), f.S, int(pow(1.0 * f.O, 1.0 * n) + 0.5)
    NS, OS = [0] * (I * S), [0] * (I * S)
    for s in range(S):
        for i in range(I):
            ii = dec2base(i, f.I, n)
            oo = [0] * n
            ns = s
            for k in range(n):
                oo[k] = f.OS[ns * f.I + ii[k]]
                ns = f.NS[ns * f.I + ii[k]]
            NS[s * I + i] = ns
            OS[s * I + i] = base2dec(oo, f.O)
    return Fsm(I, S, O, NS, OS)


QA_FSMS = {"qa_awgn1o2_4": (2, 4, 4, (0, 2, 0, 2, 1, 3, 1, 3), (0, 3, 3, 0, 1, 2, 2, 1)),      # qa_trellis.py:34-40
           "rep2": (2, 1, 4, (0, 0), (0, 3)),
           "nothing": (2, 1, 2, (0, 0), (0, 1))}
FSM_FILES = ("awgn1o2_4", "awgn1o2_128", "awgn2o3_16", "irregular", "disconnected", "simple")
# name -> how to make it (the recorder and both sides of every test go through this table)
FSM_SPECS = dict([(n, ("file", n)) for n in FSM_FILES] + [(n, ("tables",) + a) for n, a in QA_FSMS.items()] + [
    ("gen_5_7", ("generator", 1, 2, (5, 7))),
    ("gen_133_171", ("generator", 1, 2, (0o133, 0o171))),
    ("gen_2o3", ("generator", 2, 3, (1, 0, 2, 0, 1, 6))),
    ("isi_3_2", ("isi", 3, 2)),
    ("isi_2_11", ("isi", 2, 11)),
    ("cpm_2_4_2", ("cpm", 2, 4, 2)),
    ("cpm_3_2_1", ("cpm", 3, 2, 1)),
    ("joint", ("joint", "awgn1o2_4", "irregular")),
    ("radix2", ("radix", "awgn1o2_4", 2)),
])

_FSMS = {}


def make_fsm(name):
    """the restatement's FSM of FSM_SPECS[name], made once"""
    if name not in _FSMS:
        spec = FSM_SPECS[name]
        kind = spec[0]
        if kind == "file":
            f = fsm_from_text(fsm_file_text(spec[1]))
        elif kind == "tables":
            f = Fsm(*spec[1:])
        elif kind == "generator":
            f = fsm_from_generator(spec[1], spec[2], list(spec[3]))
        elif kind == "isi":
            f = fsm_from_isi(spec[1], spec[2])
        elif kind == "cpm":
            f = fsm_from_cpm(spec[1], spec[2], spec[3])
        elif kind == "joint":
            f = fsm_from_joint(make_fsm(spec[1]), make_fsm(spec[2]))
        else:
            f = fsm_from_radix(make_fsm(spec[1]), spec[2])
        _FSMS[name] = f
    return _FSMS[name]


def lib_fsm(g, name):
    """the library's FSM of FSM_SPECS[name], through the constructor of its kind"""
    spec = FSM_SPECS[name]
    kind = spec[0]
    if kind == "file":
        return g.fsm(os.path.join(FSM_DIR, spec[1] + ".fsm"))
    if kind == "tables":
        return g.fsm(*spec[1:])
    if kind == "generator":
        return g.fsm(spec[1], spec[2], list(spec[3]))
    if kind in ("isi", "cpm"):
        return g.fsm(*spec[1:])
    if kind == "joint":
        return g.fsm(lib_fsm(g, spec[1]), lib_fsm(g, spec[2]))
    return g.fsm(lib_fsm(g, spec[1]), spec[2])


def flat_lists(ll):
    """PS or PI as (lengths, entries back to back)"""
    return np.array([len(l) for l in ll], np.int32), np.array([v for l in ll for v in l], np.int32)


# ---- trellis_encoder_XX ------------------------------------------------------------------------------------------------
def encode(f, st, x, out_dtype=np.uint8):
    """(outputs, end state) of one stream from state st"""
    out = np.zeros(len(x), out_dtype)
    for i, v in enumerate(x):
        out[i] = f.OS[st * f.I + int(v)]
        st = f.NS[st * f.I + int(v)]
    return out, st


# ---- calc_metric -------------------------------------------------------------------------------------------------------
def _sums(x, table, O, D):
    """metric[step][o] = sum over d of s * s, s = x[step][d] - TABLE[o][d], in the item's type; float32 adds in d order"""
    x = np.ascontiguousarray(x)
    t = np.ascontiguousarray(table, x.dtype).reshape(O, D)
    x = x.reshape(-1, 1, D)
    m = np.zeros((x.shape[0], O), F32)
    with np.errstate(all="ignore"):
        for d in range(D):
            if x.dtype == np.complex64:
                re = x[:, :, d].real.astype(F32) - t[None, :, d].real.astype(F32)
                im = x[:, :, d].imag.astype(F32) - t[None, :, d].imag.astype(F32)
                term = (re * re).astype(F32) + (im * im).astype(F32)
            elif x.dtype == np.float32:
                s = x[:, :, d] - t[None, :, d]
                term = s * s
            elif x.dtype == np.int16:
                s = (x[:, :, d].astype(np.int32) - t[None, :, d].astype(np.int32)).astype(np.int16)     # truncated to short
                term = (s.astype(np.int32) * s.astype(np.int32)).astype(F32)
            else:
                s = (x[:, :, d].astype(np.int64) - t[None, :, d].astype(np.int64)).astype(np.int32)     # the wrap
                term = (s.astype(np.int64) * s.astype(np.int64)).astype(np.int32).astype(F32)
            m = (m + term.astype(F32)).astype(F32)
    return m


def calc_metric(x, table, O, D, type):
    """steps * D items -> steps * O float32"""
    m = _sums(x, table, O, D)
    if type == EUCLIDEAN:
        return m.reshape(-1)
    assert type == HARD_SYMBOL
    m2 = np.where(np.isnan(m), np.inf, m)           # a NaN never passes metric[o] < minm
    idx = np.argmin(m2, axis=1)                     # the first minimum in o order ...
    idx = np.where(m2[np.arange(len(idx)), idx] < FLT_MAX, idx, 0)      # ... below FLT_MAX, else minmi stays 0
    out = np.ones(m.shape, F32)
    out[np.arange(len(idx)), idx] = 0.0
    return out.reshape(-1)


# ---- viterbi_algorithm -------------------------------------------------------------------------------------------------
def viterbi(f, K, S0, SK, metrics, out_dtype=np.uint8, last_minimum=False):
    """every block of K steps of `metrics` (nblocks * K * O float32) -> (nblocks * K symbols, dead ends).
    last_minimum flips the comparisons to <=, the rule that a wrong tie-break would follow (for the tests only)."""
    S, O, I = f.S, f.O, f.I
    m = np.ascontiguousarray(metrics, F32).reshape(-1, K, O)
    nb = m.shape[0]
    cnt = np.array([len(p) for p in f.PS])
    pmax = max(1, int(cnt.max()))
    ps = np.zeros((pmax, S), np.int64)
    mi = np.zeros((pmax, S), np.int64)
    for j in range(S):
        for i in range(cnt[j]):
            ps[i, j] = f.PS[j][i]
            mi[i, j] = f.OS[f.PS[j][i] * I + f.PI[j][i]]
    alpha = np.zeros((nb, S), F32) if S0 < 0 else np.full((nb, S), INF, F32)
    if S0 >= 0:
        alpha[:, S0] = 0.0
    trace = np.zeros((K, nb, S), np.int32)
    less = (lambda a, b: a <= b) if last_minimum else (lambda a, b: a < b)
    with np.errstate(all="ignore"):
        for k in range(K):
            minm = np.full((nb, S), INF, F32)
            minmi = np.zeros((nb, S), np.int32)
            for i in range(pmax):
                mm = (alpha[:, ps[i]] + m[:, k, mi[i]]).astype(F32)
                win = less(mm, minm) & (i < cnt)[None, :]
                minm = np.where(win, mm, minm)
                minmi = np.where(win, i, minmi)
            trace[k] = minmi
            low = minm.min(axis=1)                   # no minm is a NaN: a NaN never passed the comparison
            norm = np.where(low < INF, low, INF).astype(F32)
            alpha = (minm - norm[:, None]).astype(F32)
    out = np.zeros((nb, K), out_dtype)
    dead = 0
    for b in range(nb):
        if SK < 0:
            st, best = 0, INF
            for i in range(S):
                if less(alpha[b, i], best):
                    best, st = alpha[b, i], i
        else:
            st = SK
        for k in range(K - 1, -1, -1):
            if cnt[st] == 0:                          # the handle's rule where the reference indexes an empty vector
                dead += 1
                continue
            i0 = trace[k, b, st]
            out[b, k] = f.PI[st][i0]
            st = f.PS[st][i0]
    return out.reshape(-1), dead


# ---- the inputs of the cases -------------------------------------------------------------------------------------------
def pam_table(O):
    """one real sample per step: output symbol o is sent as o - (O - 1) / 2"""
    return (np.arange(O) - (O - 1) / 2.0).astype(F32)


def viterbi_input(f, kind, K, nblocks, seed):
    """nblocks * K * O float32 metrics of `kind`"""
    r = np.random.RandomState(seed)
    n = nblocks * K
    if kind == "zeros":
        return np.zeros(n * f.O, F32)
    if kind in ("euclid", "hard"):
        sent, st = np.zeros(n, np.int64), 0
        x = r.randint(0, f.I, n)
        for i in range(n):
            if i % K == 0:
                st = 0
            sent[i] = f.OS[st * f.I + x[i]]
            st = f.NS[st * f.I + x[i]]
        tab = pam_table(f.O)
        rx = (tab[sent] + r.normal(0, 0.6, n)).astype(F32)
        return calc_metric(rx, tab, f.O, 1, EUCLIDEAN if kind == "euclid" else HARD_SYMBOL)
    if kind == "quant":                              # small whole numbers: ties at most steps, no two paths alike
        return r.randint(0, 3, n * f.O).astype(F32)
    assert kind == "special"
    m = r.uniform(0, 4, n * f.O).astype(F32)
    pos = r.rand(n * f.O) < 0.03
    vals = np.array([1e9, np.inf, -np.inf, np.nan, -0.0], F32)
    m[pos] = vals[r.randint(0, len(vals), int(pos.sum()))]
    return m


def metrics_input(dtype, O, D, steps, seed):
    """(TABLE of O * D items, steps * D inputs) of a metrics case"""
    r = np.random.RandomState(seed)
    if dtype == np.float32:
        return r.normal(0, 1, O * D).astype(F32), r.normal(0, 1.5, steps * D).astype(F32)
    if dtype == np.complex64:
        return ((r.normal(0, 1, O * D) + 1j * r.normal(0, 1, O * D)).astype(np.complex64),
                (r.normal(0, 1.5, steps * D) + 1j * r.normal(0, 1.5, steps * D)).astype(np.complex64))
    if dtype == np.int16:                            # differences beyond 32767 wrap
        return r.randint(-30000, 30000, O * D).astype(np.int16), r.randint(-32768, 32768, steps * D).astype(np.int16)
    return r.randint(-40000, 40000, O * D).astype(np.int32), r.randint(-40000, 40000, steps * D).astype(np.int32)


METRIC_DTYPES = {"s": np.int16, "i": np.int32, "f": np.float32, "c": np.complex64}
OUT_DTYPES = {"b": np.uint8, "s": np.int16, "i": np.int32}

# (fsm, K, nblocks, S0, SK, input kind, seed, output type)
VITERBI_CASES = [
    ("awgn1o2_4", 64, 5, 0, -1, "euclid", 1, "b"),
    ("awgn1o2_4", 64, 5, -1, -1, "hard", 2, "b"),
    ("awgn1o2_4", 33, 3, 0, 0, "zeros", 3, "b"),
    ("awgn1o2_4", 65, 4, 3, 2, "quant", 4, "s"),
    ("awgn1o2_4", 1500, 2, 0, -1, "special", 5, "i"),
    ("awgn1o2_4", 1, 7, -1, -1, "quant", 6, "b"),
    ("awgn1o2_4", 2, 7, 0, -1, "quant", 7, "b"),
    ("rep2", 40, 3, 0, -1, "euclid", 8, "b"),
    ("nothing", 40, 3, -1, -1, "quant", 9, "b"),
    ("isi_3_2", 50, 4, 0, -1, "euclid", 10, "b"),
    ("isi_3_2", 50, 4, -1, 2, "quant", 11, "b"),
    ("awgn2o3_16", 70, 3, 0, -1, "euclid", 12, "b"),
    ("awgn2o3_16", 70, 3, -1, -1, "special", 13, "b"),
    ("gen_133_171", 96, 2, 0, -1, "euclid", 14, "b"),
    ("gen_133_171", 96, 2, -1, -1, "quant", 15, "s"),
    ("awgn1o2_128", 80, 2, 0, -1, "euclid", 16, "b"),
    ("awgn1o2_128", 80, 2, 3, 2, "special", 17, "i"),
    ("isi_2_11", 32, 1, 0, -1, "quant", 18, "b"),
    ("irregular", 64, 3, -1, -1, "quant", 19, "b"),
    ("irregular", 64, 3, 0, -1, "special", 20, "b"),
    ("disconnected", 20, 3, -1, -1, "quant", 21, "b"),
    ("simple", 20, 3, 1, -1, "zeros", 22, "b"),
    ("radix2", 48, 3, 0, -1, "hard", 23, "b"),
    ("cpm_2_4_2", 48, 3, 0, -1, "euclid", 24, "b"),
    ("joint", 48, 3, -1, -1, "quant", 25, "b"),
]

# (fsm, signature, n, start state, seed)
ENCODER_CASES = [
    ("awgn1o2_4", "bb", 1000, 0, 31), ("awgn1o2_4", "bs", 257, 2, 32), ("awgn1o2_4", "bi", 256, 0, 33),
    ("awgn2o3_16", "ss", 805, 5, 34), ("gen_133_171", "si", 805, 0, 35), ("awgn1o2_128", "ii", 805, 100, 36),
    ("rep2", "bb", 255, 0, 37), ("isi_3_2", "bb", 1, 1, 38), ("cpm_2_4_2", "bs", 300, 3, 39),
]

# (item type, O, D, metric type, steps, seed)
METRICS_CASES = [(t, O, D, ty, 97, 40 + n) for n, (t, O, D, ty) in enumerate(
    [(t, O, D, ty) for t in "sifc" for (O, D) in ((2, 1), (4, 2), (9, 3)) for ty in (EUCLIDEAN, HARD_SYMBOL)])]

# (kind, dimensionality, metric type, steps, seed); calcdist takes CALCDIST_POINTS, 4 points of 2 samples
CONSTELLATION_CASES = [(k, 2 if k == "calcdist" else 1, ty, 97, 80 + n) for n, (k, ty) in enumerate(
    [(k, ty) for k in ("bpsk", "qpsk", "8psk", "calcdist") for ty in (EUCLIDEAN, HARD_SYMBOL)])]
CALCDIST_POINTS = np.array([1 + 1j, -1 + 0.5j, -1 - 1j, 0.25 - 1j, 1 - 1j, 0.5 + 0.5j, -0.5 + 1j, 2 + 0j], np.complex64)


# (fsm, K, blocks, S0, SK, signature, D, metric type, seed): viterbi_algorithm_combined (core_algorithms.cc:147-217)
COMBINED_CASES = [(name, K, nb, S0, SK, sig, D, ty, 100 + n) for n, (name, K, nb, S0, SK, sig, D, ty) in enumerate([
    ("awgn1o2_4", 65, 5, 0, -1, "fb", 1, EUCLIDEAN), ("awgn1o2_4", 65, 5, 0, -1, "fb", 2, HARD_SYMBOL),
    ("awgn1o2_4", 64, 3, -1, -1, "cb", 1, EUCLIDEAN), ("awgn1o2_4", 64, 3, 3, 2, "cb", 2, HARD_SYMBOL),
    ("awgn2o3_16", 70, 3, 0, -1, "sb", 1, EUCLIDEAN), ("awgn2o3_16", 70, 3, 0, -1, "sb", 2, HARD_SYMBOL),
    ("isi_3_2", 50, 4, 0, -1, "ib", 1, HARD_SYMBOL), ("isi_3_2", 50, 4, -1, 2, "ib", 2, EUCLIDEAN),
    ("gen_133_171", 96, 2, 0, -1, "fs", 1, EUCLIDEAN), ("gen_133_171", 96, 2, 0, 0, "fs", 2, HARD_SYMBOL),
    ("awgn1o2_128", 80, 2, 0, -1, "fi", 1, HARD_SYMBOL), ("awgn1o2_128", 80, 2, -1, -1, "fi", 2, EUCLIDEAN),
    ("awgn1o2_4", 1500, 2, 0, -1, "ci", 2, EUCLIDEAN), ("rep2", 40, 3, 0, -1, "ss", 1, EUCLIDEAN),
])]


def combined_input(f, dtype, D, K, nblocks, seed):
    """(TABLE of O * D items, nblocks * K * D raw items): every block is a coded sequence from state 0, sent as the rows
    of TABLE, plus noise of a fifth of the points' spread (rounded for the integer types)"""
    r = np.random.RandomState(seed)
    n = nblocks * K
    sym, st = np.zeros(n, np.int64), 0
    x = r.randint(0, f.I, n)
    for i in range(n):
        if i % K == 0:
            st = 0
        sym[i] = f.OS[st * f.I + x[i]]
        st = f.NS[st * f.I + x[i]]
    if dtype in (np.float32, np.complex64):
        tab = r.normal(0, 1, (f.O, D)) + (1j * r.normal(0, 1, (f.O, D)) if dtype == np.complex64 else 0)
        noise = 0.2 * (r.normal(0, 1, (n, D)) + (1j * r.normal(0, 1, (n, D)) if dtype == np.complex64 else 0))
        return tab.astype(dtype).reshape(-1), (tab[sym] + noise).astype(dtype).reshape(-1)
    tab = r.randint(-1000, 1000, (f.O, D))
    rx = tab[sym] + np.rint(200 * r.normal(0, 1, (n, D))).astype(np.int64)
    return tab.astype(dtype).reshape(-1), rx.astype(dtype).reshape(-1)


def viterbi_combined(f, K, S0, SK, D, table, type, x, out_dtype=np.uint8):
    """calc_metric of every step's D items, then viterbi_algorithm on them: what the reference does step by step"""
    return viterbi(f, K, S0, SK, calc_metric(x, table, f.O, D, type), out_dtype)


def qa_chain(name, points, K, N0):
    """the restated chain of qa_trellis.py:75-136 for one packet of K steps: (bytes sent, noise, received samples,
    metrics).  bits -> encoder from state 0 -> points -> plus seeded complex Gaussian noise -> Euclidean metrics"""
    f = make_fsm(name)
    pts = np.array(points, np.complex64)
    r = np.random.RandomState(666)
    sent = r.randint(0, 256, K // 8).astype(np.uint8)
    bits = np.unpackbits(sent)                       # packed_to_unpacked_bb(1, GR_MSB_FIRST)
    sym, _ = encode(f, 0, bits)
    noise = (np.sqrt(N0 / 2) * (r.normal(0, 1, len(bits)) + 1j * r.normal(0, 1, len(bits)))).astype(np.complex64)
    rx = (pts[sym] + noise).astype(np.complex64)
    return sent, noise, rx, calc_metric(rx, pts, len(pts), 1, EUCLIDEAN)


QA_K = 2048          # the QA's 16384 is a workload, not a corner
QA_N0 = 0.02         # a standard deviation of 0.1 per component: the uncoded FSMs sit ten of them from a decision border


def constellation_input(dim, steps, seed):
    r = np.random.RandomState(seed)
    x = (r.normal(0, 1, steps * dim) + 1j * r.normal(0, 1, steps * dim)).astype(np.complex64)
    x[::7] = 0                                       # midway between the points: HARD_SYMBOL ties
    return x


def case_key(prefix, case):
    return prefix + "_" + "_".join(str(c) for c in case)
