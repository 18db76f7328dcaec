// trellis_test.cc -- the host blocks of gr-trellis (host/grhip_blocks.h) on a device: the chain of qa_trellis.py:75-136 as
// work() calls for its three FSMs -- trellis_encoder_bb(f, 0) -> constellation points plus a small seeded disturbance ->
// trellis_constellation_metrics_cf -> trellis_viterbi_b(f, K, 0, -1) returns every input symbol, and so does
// trellis_metrics_c(O, 1, points) in its place -- the factory signatures of trellis_encoder_XX.h, trellis_metrics_X.h,
// trellis_constellation_metrics_cf.h and trellis_viterbi_X.h, their forecast / output multiple / relative rate, the fsm
// class' constructors (qa_trellis.py test_001 .. test_004) and the refusals; the same chain through
// trellis_viterbi_combined_cb in both engines.
#include <cstdio>
#include <type_traits>
#include <vector>

#include "grhip_blocks.h"

static_assert(std::is_same<decltype(&trellis_make_encoder_bb), grhip_trellis_encoder_bb_sptr (*)(const fsm &, int, int)>::value, "");
static_assert(std::is_same<decltype(&trellis_make_encoder_si), grhip_trellis_encoder_si_sptr (*)(const fsm &, int, int)>::value, "");
static_assert(std::is_same<decltype(&trellis_make_metrics_f),
                           grhip_trellis_metrics_f_sptr (*)(int, int, const std::vector<float> &, trellis_metric_type_t, int)>::value, "");
static_assert(std::is_same<decltype(&trellis_make_metrics_c),
                           grhip_trellis_metrics_c_sptr (*)(int, int, const std::vector<gr_complex> &, trellis_metric_type_t, int)>::value, "");
static_assert(std::is_same<decltype(&trellis_make_constellation_metrics_cf),
                           grhip_trellis_constellation_metrics_cf_sptr (*)(grhip_constellation_sptr, trellis_metric_type_t, int)>::value, "");
static_assert(std::is_same<decltype(&trellis_make_viterbi_b), grhip_trellis_viterbi_b_sptr (*)(const fsm &, int, int, int, int)>::value, "");
static_assert(std::is_same<decltype(&trellis_make_viterbi_combined_cb),
                           grhip_trellis_viterbi_combined_cb_sptr (*)(const fsm &, int, int, int, int, const std::vector<gr_complex> &,
                                                                      trellis_metric_type_t, int)>::value, "");
static_assert(std::is_same<decltype(&trellis_make_viterbi_combined_si),
                           grhip_trellis_viterbi_combined_si_sptr (*)(const fsm &, int, int, int, int, const std::vector<short> &,
                                                                      trellis_metric_type_t, int)>::value, "");
static_assert(std::is_default_constructible<fsm>::value, "");
static_assert(std::is_base_of<gr_sync_block, grhip_trellis_encoder_bb_blk>::value && std::is_base_of<gr_block, grhip_trellis_viterbi_s_blk>::value, "");
static_assert(!std::is_copy_constructible<grhip_trellis_viterbi_b_blk>::value, "");
static_assert(TRELLIS_EUCLIDEAN == 200 && TRELLIS_HARD_SYMBOL == 201 && TRELLIS_HARD_BIT == 202, "");

template <class F> static bool throws(F f)
{
    try { f(); } catch (const std::exception &) { return true; }
    return false;
}

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

struct qa_fsm {
    const char *name;
    int I, S, O;
    std::vector<int> NS, OS;
};

int main()
{
    const qa_fsm specs[] = {{"awgn1o2_4", 2, 4, 4, {0, 2, 0, 2, 1, 3, 1, 3}, {0, 3, 3, 0, 1, 2, 2, 1}},       // qa_trellis.py:34-40
                            {"rep2", 2, 1, 4, {0, 0}, {0, 3}},
                            {"nothing", 2, 1, 2, {0, 0}, {0, 1}}};
    {   // test_001 .. test_004, and fsm(1, 2, [5, 7]) is awgn1o2_4
        const fsm f(specs[0].I, specs[0].S, specs[0].O, specs[0].NS, specs[0].OS);
        CHECK(f.I() == 2 && f.S() == 4 && f.O() == 4 && f.NS() == specs[0].NS && f.OS() == specs[0].OS && f.connected());
        const fsm none, none2(none);                                                       // fsm.cc:34-45
        CHECK(none.I() == 0 && none.S() == 0 && none.O() == 0 && none.NS().empty() && none.PS().empty() && none2.S() == 0);
        CHECK(throws([&] { trellis_make_encoder_bb(none, 0); }) && throws([&] { trellis_make_viterbi_b(none, 8, 0, -1); }));
        const fsm g(f);
        CHECK(g.I() == f.I() && g.S() == f.S() && g.O() == f.O() && g.NS() == f.NS() && g.OS() == f.OS());
        const fsm c(1, 2, std::vector<int>{5, 7});
        CHECK(c.NS() == f.NS() && c.OS() == f.OS() && c.PS() == f.PS() && c.PI() == f.PI() && c.TMl() == f.TMl() && c.TMi() == f.TMi());
        CHECK((f.PS()[3] == std::vector<int>{2, 3}) && (f.PI()[3] == std::vector<int>{1, 1}));
        const fsm isi(3, 2), cpm(2, 4, 2), joint(f, isi), radix(f, 2), one(specs[1].I, specs[1].S, specs[1].O, specs[1].NS, specs[1].OS);
        CHECK(isi.S() == 3 && isi.O() == 9 && cpm.S() == 8 && cpm.O() == 32 && joint.S() == 12 && joint.I() == 6 && radix.I() == 4 && radix.O() == 16 && one.S() == 1);
        CHECK(throws([] { fsm(2, 1, 4, {0, 1}, {0, 3}); }) && throws([] { fsm(2, 1, 4, {0}, {0, 3}); }) && throws([] { fsm("no/such/file.fsm"); }) &&
              throws([] { fsm(0, 2); }) && throws([] { fsm(1, 2, std::vector<int>{0, 0}); }));
        CHECK(throws([&] { trellis_make_encoder_bb(f, 4); }) && throws([&] { trellis_make_viterbi_b(f, 0, 0, -1); }) &&
              throws([&] { trellis_make_viterbi_b(f, 8, 4, -1); }) && throws([&] { trellis_make_viterbi_b(fsm(2, 12), 8, 0, -1); }) &&
              throws([&] { trellis_make_viterbi_combined_fb(f, 8, 0, -1, 1, {0.f, 1.f, 2.f}, TRELLIS_EUCLIDEAN); }) &&
              throws([&] { trellis_make_viterbi_combined_fb(f, 8, 0, -1, 1, {0.f, 1.f, 2.f, 3.f}, TRELLIS_HARD_BIT); }) &&
              throws([] { trellis_make_metrics_f(2, 1, {0.f, 1.f}, TRELLIS_HARD_BIT); }) && throws([] { trellis_make_metrics_f(2, 1, {0.f}, TRELLIS_EUCLIDEAN); }));
    }
    const int K = 2048;
    for (const qa_fsm &q : specs)
        for (int mode : {GRHIP_MODE_FAST, GRHIP_MODE_GENERIC}) {
            const fsm f(q.I, q.S, q.O, q.NS, q.OS);
            grhip_constellation_sptr con = q.O == 2 ? digital_make_constellation_bpsk() : digital_make_constellation_qpsk();    // qa_trellis.py:42-44
            const std::vector<gr_complex> pts = con->points();
            CHECK((int)pts.size() == q.O);
            std::vector<unsigned char> bits(K), sym(K), dec(K), dec2(K);
            unsigned lcg = 12345u + (unsigned)q.O;
            auto next = [&] { lcg = lcg * 1664525u + 1013904223u; return lcg >> 8; };
            for (int i = 0; i < K; ++i) bits[i] = (unsigned char)(next() & 1u);
            auto enc = trellis_make_encoder_bb(f, 0);
            enc->set_mode(mode);
            {   // cut at 97 and 1000: the state is the handle's
                const int cuts[] = {0, 97, 1000, K};
                for (int c = 0; c < 3; ++c) {
                    gr_vector_const_void_star in{bits.data() + cuts[c]};
                    gr_vector_void_star out{sym.data() + cuts[c]};
                    CHECK(enc->work(cuts[c + 1] - cuts[c], in, out) == cuts[c + 1] - cuts[c]);
                }
            }
            int st = 0;
            for (int i = 0; i < K; ++i) {
                CHECK(sym[i] == q.OS[st * q.I + bits[i]]);
                st = q.NS[st * q.I + bits[i]];
            }
            CHECK(enc->ST() == st);
            const unsigned char bit5 = bits[5];
            bits[5] = 2;                                                                      // an input symbol outside [0, I)
            {
                gr_vector_const_void_star in{bits.data()};
                gr_vector_void_star out{dec.data()};
                CHECK(throws([&] { enc->work(16, in, out); }) && enc->ST() == st);
            }
            bits[5] = bit5;
            std::vector<gr_complex> x(K);
            for (int i = 0; i < K; ++i)         // a disturbance of at most 0.1 per component: no decision comes near a border
                x[i] = pts[sym[i]] + gr_complex(((int)(next() % 201u) - 100) * 1e-3f, ((int)(next() % 201u) - 100) * 1e-3f);
            std::vector<float> m((size_t)K * q.O), m2((size_t)K * q.O);
            auto met = trellis_make_constellation_metrics_cf(con, TRELLIS_EUCLIDEAN);
            auto metc = trellis_make_metrics_c(q.O, 1, pts, TRELLIS_EUCLIDEAN);
            CHECK(met->O() == q.O && met->D() == 1 && met->TYPE() == TRELLIS_EUCLIDEAN && met->output_multiple() == q.O && met->relative_rate() == (double)q.O);
            gr_vector_int req(1, 0), none;
            met->forecast(K * q.O, req);
            CHECK(req[0] == K);
            {
                gr_vector_const_void_star in{x.data()};
                gr_vector_void_star out{m.data()}, out2{m2.data()};
                CHECK(met->general_work(K * q.O, none, in, out) == K * q.O && metc->general_work(K * q.O, none, in, out2) == K * q.O);
                CHECK(m == m2);                                                              // get_distance's sum is calc_metric's
            }
            auto va = trellis_make_viterbi_b(f, K, 0, -1);
            va->set_mode(mode);
            CHECK(va->K() == K && va->S0() == 0 && va->SK() == -1 && va->output_multiple() == K && va->relative_rate() == 1.0 / q.O);
            va->forecast(K, req);
            CHECK(req[0] == K * q.O);
            {
                gr_vector_const_void_star in{m.data()};
                gr_vector_void_star out{dec.data()};
                CHECK(va->general_work(K, none, in, out) == K);
                CHECK(throws([&] { va->general_work(K - 1, none, in, out); }));              // no multiple of K
            }
            CHECK(dec == bits && va->dead_ends() == 0);
            for (int engine : {1, 0}) {                                                      // the same through viterbi_combined_cb
                auto vc = trellis_make_viterbi_combined_cb(f, K, 0, -1, 1, pts, TRELLIS_EUCLIDEAN);
                vc->set_mode(mode);
                vc->set_engine(engine);
                CHECK(vc->engine() == (mode == GRHIP_MODE_GENERIC ? 0 : engine));
                CHECK(vc->K() == K && vc->D() == 1 && vc->TYPE() == TRELLIS_EUCLIDEAN && vc->TABLE() == pts && vc->output_multiple() == K &&
                      vc->relative_rate() == 1.0);
                vc->forecast(K, req);
                CHECK(req[0] == K);
                std::vector<unsigned char> dec3(K);
                gr_vector_const_void_star in{x.data()};
                gr_vector_void_star out{dec3.data()};
                CHECK(vc->general_work(K, none, in, out) == K && dec3 == bits);
                vc->set_TABLE(pts);
                CHECK(throws([&] { vc->set_TABLE(std::vector<gr_complex>(1)); }));
            }
            auto hard = trellis_make_constellation_metrics_cf(con, TRELLIS_HARD_SYMBOL);     // hard decisions decode as well here
            {
                gr_vector_const_void_star in{x.data()};
                gr_vector_void_star out{m2.data()};
                CHECK(hard->general_work(K * q.O, none, in, out) == K * q.O);
                gr_vector_const_void_star in2{m2.data()};
                gr_vector_void_star out2{dec2.data()};
                CHECK(va->general_work(K, none, in2, out2) == K && dec2 == bits);
            }
        }
    std::printf("trellis_test ok\n");
    return 0;
}
