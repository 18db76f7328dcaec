// constellation_test.cc -- csrc/constellation.h on its own, built with -fsanitize=address,undefined: every kind, the
// refused arguments, tables at the sector cap, and samples that are not finite (whose sector the reference leaves to
// an undefined conversion).  Prints "constellation_test ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../csrc/constellation.h"

using namespace grhip;

static int failures = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            ++failures;                                               \
        }                                                             \
    } while (0)

static std::vector<cfloat> circle(unsigned m)
{
    std::vector<cfloat> p(m);
    for (unsigned i = 0; i < m; ++i) p[i] = cfloat{(float)std::cos(2 * M_PI * i / m), (float)std::sin(2 * M_PI * i / m)};
    return p;
}

// every sample of `xs` (items of c.dim samples) decides for a symbol below the arity and gives an error that is NaN or
// within [-dim pi, dim pi]
static void sweep(const Constellation &c, const std::vector<cfloat> &xs)
{
    for (size_t i = 0; i + c.dim <= xs.size(); ++i) {
        float pe = 0;
        const unsigned k = c.decision_maker_pe(&xs[i], &pe);
        CHECK(k < c.arity);
        CHECK(k == c.decision_maker(&xs[i]));
        CHECK(pe != pe || std::fabs(pe) <= c.dim * 3.1415928f);
    }
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float den = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
    std::vector<cfloat> odd;
    const float vals[] = {0.f, -0.f, den, -den, 1e-30f, 0.3f, -0.3f, 1.f, -1.f, 2.5f, 1e8f, -1e8f, big, -big, inf, -inf, nan};
    for (float a : vals)
        for (float b : vals) odd.push_back(cfloat{a, b});

    // the closed forms, on the points themselves and on the QA's samples (qa_constellation_decoder_cb.py)
    Constellation bpsk, qpsk, dqpsk, psk8;
    bpsk.make_bpsk(); qpsk.make_qpsk(); dqpsk.make_dqpsk(); psk8.make_8psk();
    for (Constellation *c : {&bpsk, &qpsk, &dqpsk, &psk8}) {
        CHECK(c->dim == 1 && c->arity == c->points.size() && c->rot_sym == c->arity);
        CHECK(c->bits_per_symbol() == (c->arity == 2 ? 1u : c->arity == 4 ? 2u : 3u));
        for (unsigned k = 0; k < c->arity; ++k) {
            float pe = 1;
            CHECK(c->decision_maker_pe(&c->points[k], &pe) == k);
            CHECK(std::fabs(pe) < 1e-6f);
        }
        sweep(*c, odd);
    }
    CHECK(!bpsk.apply_pre_diff && !qpsk.apply_pre_diff && dqpsk.apply_pre_diff && !psk8.apply_pre_diff);
    CHECK(qpsk.pre_diff.size() == 4 && qpsk.pre_diff[1] == 2 && dqpsk.pre_diff[2] == 3);
    const cfloat qa[7] = {{0.5f, 0.5f}, {0.1f, -1.2f}, {-0.8f, -0.1f}, {-0.45f, 0.8f}, {0.8f, 1.0f}, {-0.5f, 0.1f}, {0.1f, -1.2f}};
    const unsigned qa_bpsk[7] = {1, 1, 0, 0, 1, 0, 1}, qa_qpsk[7] = {3, 1, 0, 2, 3, 2, 1};
    for (int i = 0; i < 7; ++i) CHECK(bpsk.decision_maker(&qa[i]) == qa_bpsk[i] && qpsk.decision_maker(&qa[i]) == qa_qpsk[i]);
    // 0 + -0 is +0: `*phase_error = 0; *phase_error += -arg(...)`
    float pe = -1;
    const cfloat one = {1.f, 0.f};
    bpsk.decision_maker_pe(&one, &pe);
    CHECK(pe == 0.f && !std::signbit(pe));

    // calcdist: one and two dimensions, the first of equal distances wins
    Constellation cd, cd2;
    const std::vector<cfloat> sq = {{1, 1}, {-1, 1}, {-1, -1}, {1, -1}};
    const unsigned code4[4] = {0, 1, 3, 2};
    CHECK(cd.make_calcdist(sq.data(), 4, code4, 4, 4, 1) && cd.arity == 4 && cd.apply_pre_diff && cd.bits_per_symbol() == 2);
    const cfloat origin = {0, 0};
    CHECK(cd.decision_maker(&origin) == 0);
    const std::vector<cfloat> p2 = {{1, 0}, {1, 0}, {1, 0}, {-1, 0}, {-1, 0}, {1, 0}, {-1, 0}, {-1, 0}, {0, 1}, {0.5f, 0}};
    CHECK(cd2.make_calcdist(p2.data(), p2.size(), nullptr, 0, 1, 2) && cd2.arity == 5 && cd2.dim == 2 && cd2.bits_per_symbol() == 1);
    const cfloat s2[2] = {{-0.9f, 0.1f}, {1.1f, 0}};
    CHECK(cd2.decision_maker(s2) == 2);
    sweep(cd, odd);
    sweep(cd2, odd);

    // psk and rect, their tables, and the tables at the cap
    for (unsigned m : {2u, 4u, 8u, 16u, 32u, 256u}) {
        Constellation c;
        const std::vector<cfloat> p = circle(m);
        CHECK(c.make_psk(p.data(), m, nullptr, 0, m) && c.rot_sym == m && c.sector_values.size() == m);
        for (unsigned k = 0; k < m; ++k) CHECK(c.sector_values[k] == k && c.decision_maker(&p[k]) == k);
        sweep(c, odd);
    }
    {
        Constellation c, r;
        const std::vector<cfloat> p = circle(256);
        CHECK(c.make_psk(p.data(), 256, nullptr, 0, CONST_MAX_SECTORS) && c.sector_values.size() == CONST_MAX_SECTORS);
        for (unsigned v : c.sector_values) CHECK(v < 256);
        sweep(c, odd);
        for (unsigned k = 0; k < 256; ++k) CHECK(c.decision_maker(&p[k]) == k);
        std::vector<cfloat> grid;
        for (int a = 0; a < 16; ++a)
            for (int b = 0; b < 16; ++b) grid.push_back(cfloat{-1 + a * (2 / 15.f), -1 + b * (2 / 15.f)});
        CHECK(r.make_rect(grid.data(), grid.size(), nullptr, 0, 4, 128, 128, 2 / 127.f, 2 / 127.f) && r.sector_values.size() == CONST_MAX_SECTORS);
        for (unsigned v : r.sector_values) CHECK(v < 256);
        for (unsigned k = 0; k < 256; ++k) CHECK(r.decision_maker(&grid[k]) == k);
        sweep(r, odd);
        Constellation q;
        CHECK(q.make_rect(sq.data(), 4, nullptr, 0, 4, 2, 2, 1.f, 1.f));
        CHECK(q.sector_values[0] == 2 && q.sector_values[1] == 1 && q.sector_values[2] == 3 && q.sector_values[3] == 0);
        sweep(q, odd);
    }

    // refusals
    {
        Constellation c;
        const std::vector<cfloat> many = circle(258);
        const unsigned code3[3] = {0, 1, 2};
        CHECK(!c.make_calcdist(sq.data(), 4, code3, 3, 4, 1));              // the code's length
        CHECK(!c.make_calcdist(sq.data(), 3, nullptr, 0, 4, 2));            // no multiple of the dimensionality
        CHECK(!c.make_calcdist(sq.data(), 4, nullptr, 0, 4, 0));
        CHECK(!c.make_calcdist(sq.data(), 0, nullptr, 0, 4, 1));
        CHECK(!c.make_calcdist(nullptr, 4, nullptr, 0, 4, 1));
        CHECK(!c.make_calcdist(many.data(), 257, nullptr, 0, 1, 1));        // arity 257
        CHECK(c.make_calcdist(many.data(), 256, nullptr, 0, 1, 1));
        CHECK(c.make_calcdist(many.data(), 258, nullptr, 0, 1, 2) && c.arity == 129);
        CHECK(!c.make_psk(sq.data(), 4, nullptr, 0, 0) && !c.make_psk(sq.data(), 4, nullptr, 0, CONST_MAX_SECTORS + 1));
        CHECK(!c.make_rect(sq.data(), 4, nullptr, 0, 4, 0, 2, 1.f, 1.f) && !c.make_rect(sq.data(), 4, nullptr, 0, 4, 129, 128, 1.f, 1.f));
        CHECK(!c.make_rect(sq.data(), 4, nullptr, 0, 4, 65536, 65536, 1.f, 1.f));
        CHECK(!c.make_rect(sq.data(), 4, nullptr, 0, 4, 2, 2, 0.f, 1.f) && !c.make_rect(sq.data(), 4, nullptr, 0, 4, 2, 2, 1.f, nan));
        CHECK(!c.make_rect(sq.data(), 4, nullptr, 0, 4, 2, 2, inf, 1.f));
        const std::vector<cfloat> bad = {{1, 1}, {nan, 1}};
        CHECK(!c.make_rect(bad.data(), 2, nullptr, 0, 4, 2, 2, 1.f, 1.f));
    }

    // the complex product's Annex G recovery, and invert_code
    {
        const cfloat r = cmul(cfloat{inf, nan}, cfloat{1.f, 0.f});
        CHECK(std::isinf(r.re) && r.re > 0);
        const cfloat n = cmul(cfloat{nan, nan}, cfloat{1.f, 1.f});
        CHECK(n.re != n.re && n.im != n.im);
        const cfloat f = cmul(cfloat{1.f, 2.f}, cfloat{3.f, -4.f});
        CHECK(f.re == 11.f && f.im == 2.f);
        const std::vector<int> inv = invert_code({0, 1, 3, 2});
        CHECK(inv.size() == 4 && inv[0] == 0 && inv[1] == 1 && inv[2] == 3 && inv[3] == 2);
        const std::vector<int> inv8 = invert_code({0, 1, 3, 2, 6, 7, 5, 4});
        CHECK(inv8[4] == 7 && inv8[7] == 5 && inv8[6] == 4);
    }
    if (failures) return 1;
    std::printf("constellation_test ok\n");
    return 0;
}
