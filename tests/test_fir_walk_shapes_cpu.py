"""The table of tests/test_gpu_fir_walk.py against the sources, without a GPU: the tile sizes and grid rules of the four
persistent FIR kernels are read out of csrc/ by name, so that a change of tile size or of a grid rule cannot silently
leave a walk case with fewer than three tiles per workgroup; the sizing arithmetic over a range of CU counts; and the
rows of host/fir_plan_test.cc that pin every case's engine."""
import os
import re

import pytest

import test_gpu_fir_walk as walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd")
CU_COUNTS = [1, 8, 64, 256, 304]
IDS = [k.id for k in walk.WALK_CASES]


def _src(name):
    with open(os.path.join(PKG, name)) as f:
        return f.read()


def _squash(text):
    return re.sub(r"\s+", " ", text)


def _int(text, pattern):
    m = re.search(pattern, text)
    assert m, "not found in the source: " + pattern
    return int(m.group(1))


def _has(text, snippet):
    assert _squash(snippet) in _squash(text), "the source no longer says: " + snippet


@pytest.fixture(scope="module")
def K():
    """the constants, and the rules the table relies on (their text: a changed rule must be looked at)"""
    tiled, kern, realin = _src("csrc/fir_tiled.hip"), _src("csrc/fir_kernels.hip"), _src("csrc/fir_realin.hip")
    k = {
        "TILED_R": _int(tiled, r"#define GRHIP_TILED_R (\d+)"),
        "TILED_THREADS": _int(tiled, r"#define GRHIP_TILED_THREADS (\d+)"),
        "QUEUE_MIN": _int(tiled, r"if \(a\.Tq \* decim < (\d+)\) a\.sched = nullptr;"),
        "GT_R": _int(kern, r"constexpr int GT_R = (\d+)"),
        "GT_T": _int(kern, r"constexpr int GT_R = \d+, GT_T = (\d+)"),
        "GT_CAP": _int(kern, r"if \(per_cu > (\d+)\) per_cu = \1;"),
        "HIDEC_LDS_SAMPLES": _int(kern, r"constexpr int HIDEC_LDS_SAMPLES = (\d+);"),
        "HIDEC_G_MAX": _int(kern, r"for \(int G = 1; G <= (\d+); \+\+G\)"),
        "RI_R": _int(realin, r"constexpr int RI_R = (\d+);"),
        "RI_T": _int(realin, r"constexpr int RI_T = (\d+);"),
    }
    _has(tiled, "constexpr int TILED_NT = TILED_THREADS * TILED_R;")
    _has(tiled, "constexpr int TILED_WG_PER_CU = (TILED_R == 8 ? 2 : 3) * 256 / TILED_THREADS;")
    _has(tiled, "return (D == 1 && !premix && epi == 0) ? 2 * TILED_WG_PER_CU : TILED_WG_PER_CU;")
    _has(tiled, "constexpr int NEW_PER_TILE = EPI == EPI_DEMOD ? TILED_NT - TILED_R * (TILED_THREADS / 64) : TILED_NT;")
    _has(tiled, "long long grid = (long long)wgs * device_cus();")
    _has(tiled, "if ((a_in.n_in - a_in.n_lo) * item >= (1ll << 31) - (1ll << 20))")
    _has(kern, "GT_NT = GT_R * GT_T;")
    _has(kern, "long long per_cu = (long long)(160 * 1024) / (long long)(lds + 512);")
    _has(kern, "const size_t lds = (((size_t)decim * per_row * 8 + 15) & ~(size_t)15) + (size_t)(ntaps + 1) * (KIND == FIR_CCC ? 8 : 4);")
    _has(kern, "const int per_row = GT_NT + (ntaps + decim - 1) / decim + 2;")
    _has(kern, "const int tn_max = (HIDEC_LDS_SAMPLES - ntaps - 64) / D;")
    _has(kern, "if (2 * (256 / G) <= tn_max) return G;")
    _has(kern, "const long long per_cu = lds <= 53 * 1024 ? 3 : (lds <= 80 * 1024 ? 2 : 1);")
    _has(kern, "long long per_cu = lds <= 53 * 1024 ? 3 : (lds <= 80 * 1024 ? 2 : 1);")
    _has(kern, "const long long ntiles = (n_out + (Tn - 2) - 1) / (Tn - 2);")
    _has(kern, "if (n_in * 8 > 0x7fffffffLL || n_out * 8 > 0x7fffffffLL)")
    _has(kern, "((n_out - 1) * decim + ntaps) * 8 < 0x7ffffff0ll;")
    _has(realin, "constexpr int RI_NT = RI_T * RI_R;")
    _has(realin, "const int per_cu = lds * 2 <= 160 * 1024 ? 2 : 1;")
    _has(realin, "if ((n_in + 8) * (in_short ? 2 : 4) >= 0x7fffffffll)")
    return k


def _hidec_groups(K, D, ntaps):
    tn_max = (K["HIDEC_LDS_SAMPLES"] - ntaps - 64) // D
    for G in range(1, K["HIDEC_G_MAX"] + 1):
        if 2 * (256 // G) <= tn_max:
            return G
    return 0


def _expected(K, c):
    """(new outputs per tile, largest workgroups per CU, queue on) of a row, from the constants"""
    if c.kernel == "tiled":
        R, TH = K["TILED_R"], K["TILED_THREADS"]
        base = (2 if R == 8 else 3) * 256 // TH
        dk = 2 * c.decim if c.kind == "fff" else c.decim              # float data: pairs at twice the decimation
        assert dk in (1, 2, 4)
        plain = c.block == "fir"
        per_tile = R * TH
        if c.kind == "fff":
            per_tile *= 2                                              # a pair is two float outputs
        if c.epilogue == "demod":
            per_tile -= R * (TH // 64)
        per = -(-c.ntaps // dk)
        Tq = -(-per // R) * R
        return per_tile, base * (2 if dk == 1 and plain else 1), Tq * dk >= K["QUEUE_MIN"]
    if c.kernel == "hidec":
        G = _hidec_groups(K, c.decim, c.ntaps)
        assert G > 0
        return 2 * (256 // G) - (2 if c.epilogue == "demod" else 0), 3, False
    if c.kernel == "realin":
        return K["RI_R"] * K["RI_T"], 2, False
    assert c.kernel == "gtiled"
    nt = K["GT_R"] * K["GT_T"]
    per_row = nt + -(-c.ntaps // c.decim) + 2
    lds = ((c.decim * per_row * 8 + 15) & ~15) + (c.ntaps + 1) * (8 if c.kind == "ccc" else 4)
    # generic_tiled_ok, and not the window kernel's decimations
    assert c.decim not in (1, 2, 4) and c.decim <= 16 and c.ntaps >= 8
    assert c.decim * (nt + c.ntaps // c.decim + 3) * 8 + c.ntaps * 8 + 64 <= 150 * 1024
    return nt, max(1, min(K["GT_CAP"], 160 * 1024 // (lds + 512))), False


@pytest.mark.parametrize("case", walk.WALK_CASES, ids=IDS)
def test_table_agrees_with_the_tile_constants(K, case):
    per_tile, wg, queue = _expected(K, case)
    assert case.per_tile == per_tile
    assert case.wg_per_cu >= wg, "the launcher can choose a larger grid than the table assumes"
    assert case.wg_per_cu == wg
    assert case.queue == queue


def test_hidec_case_with_idle_lanes(K):
    G = _hidec_groups(K, 64, 128)
    assert G == 6 and 256 % G != 0


def test_tiled_cases_cover_both_sides_of_the_queue_threshold():
    tiled = [k for k in walk.WALK_CASES if k.kernel == "tiled"]
    assert any(k.queue for k in tiled) and any(not k.queue for k in tiled)
    assert {k.id for k in tiled if not k.queue} >= {"tiled-ccf-32/1", "tiled-ccc-80/2", "tiled-ccf-92/4"}


@pytest.mark.parametrize("cus", CU_COUNTS)
@pytest.mark.parametrize("case", walk.WALK_CASES, ids=IDS)
def test_sizing_arithmetic(K, case, cus):
    _per_tile, wg, _queue = _expected(K, case)
    streams, tps, n_out, n_in = walk.walk_sizes(case, cus)
    grid_max = wg * cus
    assert streams * tps >= 3 * grid_max + 1                          # three tiles for every workgroup, one a fourth
    assert -(-n_out // case.per_tile) == tps and n_out % case.per_tile != 0      # the last tile is partial
    assert n_out + walk.GUARD < 2 ** 31
    item = {"fff": 4, "fcc": 4, "fcf": 4, "scc": 2}.get(case.kind, 8)
    if case.kernel == "tiled":
        assert n_in * item < (1 << 31) - (1 << 20)
    elif case.kernel == "hidec":
        assert n_in * 8 <= 0x7FFFFFFF and n_out * 8 <= 0x7FFFFFFF
    elif case.kernel == "realin":
        assert (n_in + 8) * item < 0x7FFFFFFF
    else:
        assert ((n_out - 1) * case.decim + case.ntaps) * 8 < 0x7FFFFFF0
        assert n_out >= 2 * K["GT_R"] * K["GT_T"]


def test_every_case_has_its_engine_pinned():
    """host/fir_plan_test.cc holds one row "walk <id>" per case with the same shape, mode, engine and epilogue
    (tests/test_fir_plan_cpu.py runs that program)"""
    text = _src("host/fir_plan_test.cc")
    rows = {}
    for m in re.finditer(r'\{"walk ([^"]+)", ([^}]*)\}', text):
        rows[m.group(1)] = [f.strip() for f in m.group(2).split(",")]
    assert set(rows) == set(IDS)
    engines = {"tiled": "ENG_TILED", "hidec": "ENG_HIDEC", "realin": "ENG_REALIN", "generic": "ENG_GENERIC"}
    epilogues = {"none": "EPILOGUE_NONE", "rotate": "EPILOGUE_ROTATE", "demod": "EPILOGUE_DEMOD_FUSED"}
    modes = {"FAST": "FAST", "FAST_VALU": "VALU", "GENERIC": "GEN"}
    for c in walk.WALK_CASES:
        f = rows[c.id]
        xlating = c.block != "fir"
        assert f[0] == ("true" if xlating else "false"), c.id
        if xlating:
            assert f[1] == ("1" if c.kind == "fcf" else "0"), c.id
            assert f[2] == ("true" if c.proto == "real" else "false"), c.id
            assert f[3] == ("true" if c.block in ("demod", "captures") else "false"), c.id
        else:
            assert f[1] == "FIR_" + c.kind.upper(), c.id
        assert (int(f[4]), int(f[5])) == (c.ntaps, c.decim), c.id
        assert f[6] == modes[c.mode], c.id
        assert f[7] == ("true" if c.epilogue == "demod" else "false"), c.id
        assert f[9] == engines[c.engine] and f[10] == epilogues[c.epilogue], c.id
        batched = c.block == "captures"
        assert f[11:] == (["true", "true" if c.stride == "odd" else "false"] if batched else []), c.id
