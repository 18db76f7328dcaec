// trellis_fsm_test.cc -- csrc/trellis_fsm.h on the host, under the address and undefined-behaviour sanitizers (no device,
// no library):
//   * every constructor: tables, text, file, generator matrix, ISI, CPM, joint, radix-n, against what the reference's
//     statements imply (fsm(1, 2, [5, 7]) is awgn1o2_4.fsm; PS / PI in ascending (state, input) order; TMl / TMi of a
//     shift register; the disconnected FSM is accepted and says so);
//   * every refusal: sizes below 1, table lengths, entries out of range, a text that ends early or holds no number, a
//     missing file, a generator matrix with an all-zero row, sizes above the caps;
//   * the largest accepted sizes: S = FSM_MAX_S states, I * S = FSM_MAX_IS entries.
#include <cstdio>
#include <string>
#include <vector>

#include "../csrc/trellis_fsm.h"

using namespace grhip;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static const char *AWGN1O2_4 = "2 4 4\n\n0 2\n0 2\n1 3\n1 3\n\n0 3\n3 0\n1 2\n2 1\n\nAWGN CC from Proakis-Salehi pg 779\nGM1o2_4=[5, 7]\n";

static bool same_tables(const Fsm &a, const Fsm &b)
{
    return a.I == b.I && a.S == b.S && a.O == b.O && a.NS == b.NS && a.OS == b.OS && a.PS == b.PS && a.PI == b.PI && a.TMl == b.TMl &&
           a.TMi == b.TMi;
}

// what every accepted FSM must satisfy
static void check_consistent(const Fsm &f)
{
    CHECK(f.NS.size() == (size_t)f.I * f.S && f.OS.size() == f.NS.size());
    CHECK(f.PS.size() == (size_t)f.S && f.PI.size() == (size_t)f.S);
    CHECK(f.TMl.size() == (size_t)f.S * f.S && f.TMi.size() == f.TMl.size());
    size_t edges = 0;
    for (int j = 0; j < f.S; ++j) {
        CHECK(f.PS[j].size() == f.PI[j].size());
        edges += f.PS[j].size();
        for (size_t i = 0; i < f.PS[j].size(); ++i) {
            CHECK(f.NS[(size_t)f.PS[j][i] * f.I + f.PI[j][i]] == j);
            if (i) CHECK(f.PS[j][i - 1] < f.PS[j][i] || (f.PS[j][i - 1] == f.PS[j][i] && f.PI[j][i - 1] < f.PI[j][i]));
        }
        CHECK(f.TMl[(size_t)j * f.S + j] == 0);
    }
    CHECK(edges == f.NS.size());
    // following TMi from s reaches es in TMl steps
    for (int s = 0; s < f.S && s < 8; ++s)
        for (int es = 0; es < f.S && es < 8; ++es) {
            const int l = f.TMl[(size_t)s * f.S + es];
            if (l >= f.S) continue;
            int st = s;
            for (int k = 0; k < l; ++k) st = f.NS[(size_t)st * f.I + f.TMi[(size_t)st * f.S + es]];
            CHECK(st == es);
        }
}

static void test_constructors()
{
    Fsm file, gen, tab;
    CHECK(fsm_from_text(AWGN1O2_4, file));
    check_consistent(file);
    CHECK(file.I == 2 && file.S == 4 && file.O == 4 && file.connected);
    CHECK(fsm_from_generator(1, 2, {5, 7}, gen) && same_tables(file, gen));
    CHECK(fsm_from_tables(2, 4, 4, {0, 2, 0, 2, 1, 3, 1, 3}, {0, 3, 3, 0, 1, 2, 2, 1}, tab) && same_tables(file, tab));     // qa_trellis.py:34-37
    CHECK((file.PS[0] == std::vector<int>{0, 1}) && (file.PI[0] == std::vector<int>{0, 0}) && (file.PS[3] == std::vector<int>{2, 3}) &&
          (file.PI[3] == std::vector<int>{1, 1}));
    CHECK(file.TMl[0 * 4 + 3] == 2 && file.TMi[0 * 4 + 3] == 1 && file.TMl[3 * 4 + 0] == 2 && file.TMi[3 * 4 + 0] == 0);

    Fsm f;
    CHECK(fsm_from_tables(2, 1, 4, {0, 0}, {0, 3}, f) && f.connected && f.PS[0].size() == 2);      // rep2: a single state
    check_consistent(f);
    CHECK(fsm_from_generator(1, 2, {0133, 0171}, f) && f.I == 2 && f.S == 64 && f.O == 4);
    check_consistent(f);
    CHECK(fsm_from_generator(2, 3, {1, 0, 2, 0, 1, 6}, f) && f.I == 4 && f.S == 8 && f.O == 8);
    check_consistent(f);
    CHECK(fsm_from_isi(3, 2, f) && f.I == 3 && f.S == 3 && f.O == 9);
    check_consistent(f);
    CHECK(fsm_from_isi(2, 11, f) && f.S == 1024 && f.O == 2048);
    check_consistent(f);
    CHECK(fsm_from_isi(5, 1, f) && f.S == 1 && f.O == 5);
    CHECK(fsm_from_cpm(2, 4, 2, f) && f.I == 4 && f.S == 8 && f.O == 32);
    check_consistent(f);
    CHECK(fsm_from_cpm(3, 2, 1, f) && f.I == 2 && f.S == 3 && f.O == 6);
    check_consistent(f);
    Fsm irr, joint, radix;
    CHECK(fsm_from_text("2 2 2\n\n0 0\n0 1\n\n0 1\n0 1\n", irr) && irr.PS[0].size() == 3 && irr.PS[1].size() == 1 && !irr.connected);
    CHECK(fsm_from_joint(file, irr, joint) && joint.I == 4 && joint.S == 8 && joint.O == 8);
    check_consistent(joint);
    CHECK(fsm_from_radix(file, 2, radix) && radix.I == 4 && radix.S == 4 && radix.O == 16);
    check_consistent(radix);
    CHECK(fsm_from_radix(file, 1, radix) && same_tables(radix, file));
    // disconnected.fsm: accepted, and reported
    CHECK(fsm_from_text("1 4 1\n\n1\n0\n3\n2\n\n0\n0\n0\n0\n", f) && !f.connected && f.TMl[0 * 4 + 2] == 4 && f.TMi[0 * 4 + 2] == -1);
    check_consistent(f);
    // a state without predecessors
    CHECK(fsm_from_tables(1, 2, 1, {1, 1}, {0, 0}, f) && f.PS[0].empty() && f.PS[1].size() == 2);
    // a file
    const char *path = "trellis_fsm_test.tmp.fsm";
    FILE *fp = std::fopen(path, "w");
    CHECK(fp != nullptr);
    if (fp) {
        std::fputs(AWGN1O2_4, fp);
        std::fclose(fp);
        CHECK(fsm_from_file(path, f) && same_tables(f, file));
        std::remove(path);
    }
}

static void test_refusals()
{
    Fsm f;
    CHECK(fsm_from_tables(2, 1, 4, {0, 0}, {0, 3}, f));
    const Fsm keep = f;
    CHECK(!fsm_from_tables(0, 1, 4, {}, {}, f) && !fsm_from_tables(2, 0, 4, {}, {}, f) && !fsm_from_tables(2, 1, 0, {0, 0}, {0, 0}, f));
    CHECK(!fsm_from_tables(-1, 1, 4, {0}, {0}, f) && !fsm_from_tables(2, -3, 4, {0}, {0}, f));
    CHECK(!fsm_from_tables(2, 1, 4, {0}, {0, 3}, f) && !fsm_from_tables(2, 1, 4, {0, 0}, {0, 3, 1}, f));
    CHECK(!fsm_from_tables(2, 1, 4, {0, 1}, {0, 3}, f) && !fsm_from_tables(2, 1, 4, {0, -1}, {0, 3}, f));
    CHECK(!fsm_from_tables(2, 1, 4, {0, 0}, {0, 4}, f) && !fsm_from_tables(2, 1, 4, {0, 0}, {-1, 3}, f));
    CHECK(!fsm_from_tables(FSM_MAX_I + 1, 1, 1, {}, {}, f) && !fsm_from_tables(1, FSM_MAX_S + 1, 1, {}, {}, f) &&
          !fsm_from_tables(1, 1, FSM_MAX_O + 1, {0}, {0}, f) && !fsm_from_tables(FSM_MAX_I, 4, 1, {}, {}, f));
    CHECK(!fsm_from_tables(0x7fffffff, 0x7fffffff, 0x7fffffff, {}, {}, f));
    CHECK(!fsm_from_text(nullptr, f) && !fsm_from_text("", f) && !fsm_from_text("2 4", f) && !fsm_from_text("2 4 4\n0 2 0 2 1 3 1 3\n0 3 3 0 1 2 2", f));
    CHECK(!fsm_from_text("2 1 4\n0 x\n0 3\n", f) && !fsm_from_text("2 1 4\n0 0\n0 99999999999\n", f) && !fsm_from_text("comment first", f));
    CHECK(!fsm_from_file(nullptr, f) && !fsm_from_file("no/such/file.fsm", f));
    CHECK(!fsm_from_generator(0, 2, {}, f) && !fsm_from_generator(1, 0, {}, f) && !fsm_from_generator(1, 2, {5}, f) && !fsm_from_generator(1, 2, {5, -7}, f));
    CHECK(!fsm_from_generator(1, 2, {0, 0}, f) && !fsm_from_generator(2, 2, {5, 7, 0, 0}, f));       // an all-zero row
    CHECK(!fsm_from_generator(1, 2, {1 << 12, 1}, f) && !fsm_from_generator(22, 1, std::vector<int>(22, 1), f) &&
          !fsm_from_generator(1, 25, std::vector<int>(25, 1), f));
    CHECK(!fsm_from_isi(0, 2, f) && !fsm_from_isi(2, 0, f) && !fsm_from_isi(2, 13, f) && !fsm_from_isi(2, 65, f) && !fsm_from_isi(1 << 20, 3, f));
    CHECK(!fsm_from_cpm(0, 2, 1, f) && !fsm_from_cpm(2, 0, 1, f) && !fsm_from_cpm(2, 2, 0, f) && !fsm_from_cpm(2, 2, 13, f) &&
          !fsm_from_cpm(FSM_MAX_S + 1, 2, 1, f) && !fsm_from_cpm(3, 2, 11, f));
    Fsm big;
    CHECK(fsm_from_isi(2, 12, big) && big.S == FSM_MAX_S);
    CHECK(!fsm_from_joint(big, big, f));
    CHECK(!fsm_from_radix(keep, 0, f) && !fsm_from_radix(keep, 65, f) && !fsm_from_radix(keep, 22, f));
    CHECK(!fsm_from_radix(Fsm(), 2, f));
    f = keep;
    CHECK(!fsm_from_tables(2, 1, 4, {0, 1}, {0, 3}, f) && same_tables(f, keep));                        // a refusal leaves `out` alone
}

static void test_largest()
{
    Fsm f;
    CHECK(fsm_from_isi(2, 12, f) && f.S == FSM_MAX_S && f.connected);
    CHECK(f.TMl[(size_t)0 * f.S + (f.S - 1)] == 11);
    CHECK(fsm_from_generator(1, 2, {1 << 11, 1}, f) && f.S == FSM_MAX_S);
    // I * S = FSM_MAX_IS: every input of the single state leads back to it
    std::vector<int> ns((size_t)FSM_MAX_I, 0), os((size_t)FSM_MAX_I, 0);
    for (size_t i = 0; i < os.size(); ++i) os[i] = (int)(i % 7);
    CHECK(fsm_from_tables(FSM_MAX_I, 1, 7, ns, os, f) && f.PS[0].size() == (size_t)FSM_MAX_I && f.PI[0].back() == FSM_MAX_I - 1);
    std::vector<int> ns2((size_t)FSM_MAX_IS), os2((size_t)FSM_MAX_IS, 0);
    for (size_t i = 0; i < ns2.size(); ++i) ns2[i] = (int)(i % 2);
    CHECK(FSM_MAX_IS == 2LL * FSM_MAX_I && fsm_from_tables(FSM_MAX_I, 2, 1, ns2, os2, f) && f.connected && f.PS[1].size() == (size_t)FSM_MAX_I);
    CHECK(!fsm_from_tables(FSM_MAX_I, 3, 1, ns2, os2, f));
}

int main()
{
    test_constructors();
    test_refusals();
    test_largest();
    if (failures) {
        std::printf("trellis_fsm_test: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("trellis_fsm_test ok\n");
    return 0;
}
