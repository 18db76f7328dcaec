"""CPU check of the matrix phase's schedule (csrc/mfma_tables.h, the constexpr helpers fir_mfma.hip unrolls from): the
chunk-major walk with a bounded operand ring and two accumulator tiles per block.  The header is plain C++; a small g++
program prints the schedule and the properties are checked here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "csrc")

PROG = r"""
#include <cstdio>
#include <cstdlib>
#include "mfma_tables.h"
using namespace grhip;
int main(int argc, char **argv)
{
    int D = atoi(argv[1]), KS = atoi(argv[2]);
    std::vector<mf::SchedRead> reads;
    std::vector<mf::SchedMfma> mfmas;
    mf::build_schedule(D, KS, reads, mfmas);
    const int NCH = mf::chunks_per_seg(D, KS), NI = mf::rounds(D, KS);
    printf("H %d %d %d %d %d %d %d %d %d\n", NCH, mf::sched_cb(D), mf::RING, mf::READ_AHEAD, mf::NBLK, NI, mf::ACC_EDGE, mf::ACC_MID, mf::PASSES);
    for (auto &r : reads) printf("R %d %d %d\n", r.step, r.chunk, r.slot);
    for (auto &m : mfmas) printf("M %d %d %d %d %d %d %d\n", m.step, m.chunk, m.block, m.k, m.pass, m.acc, m.slot);
    for (int c = 0; c <= NCH; ++c) printf("L %d %d\n", c, mf::loads_begin(NI, NCH, c));
    for (int b = 0; b < mf::NBLK; ++b) printf("E %d %d\n", b, mf::sched_last_chunk(D, KS, b));
    return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("mfma_sched")
    src = d / "s.cc"
    src.write_text(PROG)
    exe = d / "s"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", HDR, str(src), "-o", str(exe)])
    return str(exe)


def _schedule(prog, D, KS):
    out = subprocess.check_output([prog, str(D), str(KS)], text=True).split("\n")
    rows = {"H": [], "R": [], "M": [], "L": [], "E": []}
    for line in out:
        if line.strip():
            f = line.split()
            rows[f[0]].append(tuple(int(v) for v in f[1:]))
    return rows


SHAPES = [(4, 10), (4, 6), (2, 10), (2, 6)]


@pytest.mark.parametrize("D,KS", SHAPES)
def test_every_block_and_k_step_once_from_its_chunk(prog, D, KS):
    s = _schedule(prog, D, KS)
    NCH, CB, R, AHEAD, NBLK = s["H"][0][:5]
    PASSES = s["H"][0][8]
    assert PASSES == 3                                                      # Ah Xh, Ah Xl, Al Xh
    assert CB == 16 * D // 32 and NCH == (NBLK - 1) * CB + KS
    for p in range(PASSES):
        pairs = [(b, k) for (_st, _c, b, k, ps, _a, _sl) in s["M"] if ps == p]
        assert sorted(pairs) == [(b, k) for b in range(NBLK) for k in range(KS)]      # each exactly once
    for step, c, b, k, _ps, _acc, slot in s["M"]:
        assert c == CB * b + k and step == c and slot == c % R
    # the walk is one sweep: steps (= chunks) never go back
    steps = [m[0] for m in s["M"]]
    assert steps == sorted(steps)
    # a block's tiles are added behind its last chunk
    assert s["E"] == [(b, CB * b + KS - 1) for b in range(NBLK)]


@pytest.mark.parametrize("D,KS", SHAPES)
def test_every_chunk_read_once_two_steps_ahead_into_a_bounded_ring(prog, D, KS):
    s = _schedule(prog, D, KS)
    NCH, CB, R, AHEAD, NBLK = s["H"][0][:5]
    assert R == 3 and AHEAD == R - 1
    read_at = {}
    for step, c, slot in s["R"]:
        assert c not in read_at, "chunk %d read twice" % c
        read_at[c] = step
        assert slot == c % R
    assert sorted(read_at) == list(range(NCH))
    first_use = {}
    last_use = {}
    for step, c, *_rest in s["M"]:
        first_use.setdefault(c, step)
        last_use[c] = step
    assert sorted(first_use) == list(range(NCH))                     # every chunk is used
    for c in range(NCH):
        assert read_at[c] <= first_use[c] - 2, (c, read_at[c], first_use[c])
    # reads are issued in chunk order (LDS answers in order: the waits count on it)
    assert [c for (_s, c, _sl) in s["R"]] == list(range(NCH))
    # residency at the MFMAs of every step: read (at that step's top or before) and still to be used
    for step in range(NCH):
        resident = [c for c in range(NCH) if read_at[c] <= step and last_use[c] >= step]
        assert len(resident) <= R, (step, resident)
        assert len({c % R for c in resident}) == len(resident)       # no two of them in one slot
    # a slot is overwritten only behind its chunk's last use
    for step, c, slot in s["R"]:
        if c >= R:
            assert last_use[c - R] < step, (c, step)


@pytest.mark.parametrize("D,KS", SHAPES)
def test_middle_k_steps_go_to_the_middle_accumulator(prog, D, KS):
    """the high-half product of the two middle k-steps (and of their two neighbours: the main lobe's shoulders) goes to
    the middle tile in every block; everything else -- the outer k-steps and all low-half products -- to the edge tile,
    whose first product is k-step 0"""
    s = _schedule(prog, D, KS)
    EDGE, MID = s["H"][0][6:8]
    assert EDGE != MID
    mids = {KS // 2 - 2, KS // 2 - 1, KS // 2, KS // 2 + 1}
    assert min(mids) >= 1 and max(mids) < KS
    for _step, _c, b, k, ps, acc, _slot in s["M"]:
        assert acc == (MID if (k in mids and ps == 0) else EDGE), (b, k, ps)
    for b in range(s["H"][0][4]):
        in_mid = sorted(k for (_st, _c, bb, k, ps, acc, _sl) in s["M"] if bb == b and acc == MID)
        assert KS // 2 - 1 in in_mid and KS // 2 in in_mid and len(in_mid) == 4


@pytest.mark.parametrize("D,KS", SHAPES)
def test_next_tile_loads_spread_over_the_chunk_steps(prog, D, KS):
    s = _schedule(prog, D, KS)
    NCH, NI = s["H"][0][0], s["H"][0][5]
    lb = dict(s["L"])
    assert lb[0] == 0 and lb[NCH] == NI
    per_step = [lb[c + 1] - lb[c] for c in range(NCH)]
    assert min(per_step) >= 0 and sum(per_step) == NI
    assert max(per_step) <= (NI + NCH - 1) // NCH              # no burst: 17 loads over 16 steps = one step with two
    if NI >= NCH:
        assert per_step[0] >= 1                                                   # the first load goes out with chunk 0
