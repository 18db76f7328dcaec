// cpm_taps_test.cc -- csrc/cpm.h on the host, under the address and undefined-behaviour sanitizers (no device, no library):
//   * every designer at its smallest and largest accepted size: all taps finite, the closed forms that the reference's
//     statements imply (LREC is flat and sums to 1, LRC starts at 0 and sums to 1, LSRC and TFM are normalised, the
//     gaussian taps sum to the gain, the gmsk taps to sps);
//   * every refusal: samples_per_sym * L == 0, more than CPM_MAX_TAPS taps, ntaps < 1, sps < 2, non-finite arguments;
//   * a type outside the enum gives LREC with L = 1 (gr_cpm.cc:214);
//   * cpm_filter_rows against the interpolator's own indexing (zeros in FRONT, filter f = padded[f + k I], reversed),
//     and cpm_fused_fits at its edges.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../csrc/cpm.h"

using namespace grhip;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static double sum(const std::vector<float> &t)
{
    double s = 0;
    for (float v : t) s += v;
    return s;
}
static bool finite(const std::vector<float> &t)
{
    for (float v : t)
        if (!std::isfinite(v)) return false;
    return true;
}

static void test_phase_response()
{
    const unsigned shapes[][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 5}, {8, 4}, {CPM_MAX_TAPS, 1}, {1, CPM_MAX_TAPS}, {64, 64}};
    for (int type = CPM_LRC; type <= CPM_GAUSSIAN; ++type)
        for (const auto &s : shapes)
            for (double beta : {0.0, 0.3, 0.5, 1.0}) {
                std::vector<float> t;
                CHECK(cpm_phase_response(type, s[0], s[1], beta, t));
                CHECK(t.size() == (size_t)s[0] * s[1] && t.size() == cpm_phase_response_ntaps(type, s[0], s[1], beta));
                CHECK(finite(t));
                if (type == CPM_LREC) {
                    for (float v : t) CHECK(v == (float)(1.0 / s[1] / s[0]));
                    CHECK(std::fabs(sum(t) - 1.0) < 1e-3);
                }
                if (type == CPM_LRC) {
                    CHECK(t[0] == 0.0f);
                    if (t.size() > 1) CHECK(std::fabs(sum(t) - 1.0) < 1e-3);
                }
                if ((type == CPM_LSRC || type == CPM_TFM) && t.size() > 1) CHECK(std::fabs(sum(t) - 1.0) < 1e-3);
            }
    std::vector<float> t, u;
    CHECK(cpm_phase_response(CPM_LREC, 2, 4, 0.3, t) && sum(t) == 1.0);                     // qa_cpm.py:82-84
    // gr_cpm.cc:214
    CHECK(cpm_phase_response(999, 4, 3, 0.3, t) && cpm_phase_response(CPM_LREC, 4, 1, 0.3, u) && t == u && t.size() == 4);
    CHECK(cpm_phase_response(-1, 4, CPM_MAX_TAPS, 0.3, t) && t.size() == 4);                // L is not used there
    // the refusals
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int type = CPM_LRC; type <= CPM_GAUSSIAN; ++type) {
        t.assign(3, 7.0f);
        CHECK(!cpm_phase_response(type, 0, 4, 0.3, t) && !cpm_phase_response(type, 4, 0, 0.3, t) && !cpm_phase_response(type, 0, 0, 0.3, t));
        CHECK(!cpm_phase_response(type, CPM_MAX_TAPS + 1, 1, 0.3, t) && !cpm_phase_response(type, 65, 64, 0.3, t));
        CHECK(!cpm_phase_response(type, 0x10000u, 0x10000u, 0.3, t));                       // the product wraps 32 bits
        CHECK(!cpm_phase_response(type, 2, 4, inf, t) && !cpm_phase_response(type, 2, 4, -inf, t) && !cpm_phase_response(type, 2, 4, nan, t));
        CHECK(t.size() == 3 && t[0] == 7.0f);                                               // a refusal leaves the vector alone
    }
    CHECK(!cpm_phase_response(999, 0, 1, 0.3, t) && !cpm_phase_response(999, CPM_MAX_TAPS + 1, 1, 0.3, t));
}

static void test_gaussian()
{
    std::vector<float> t;
    for (int n : {1, 2, 8, 16, (int)CPM_MAX_TAPS})
        for (double bt : {0.25, 0.35, 1.0}) {
            CHECK(firdes_gaussian(1.0, 2.0, bt, n, t) && (int)t.size() == n && finite(t));
            CHECK(std::fabs(sum(t) - 1.0) < 1e-4);
            CHECK(firdes_gaussian(2.5, 8.0, bt, n, t) && std::fabs(sum(t) - 2.5) < 1e-3);
        }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(!firdes_gaussian(1, 2, 0.3, 0, t) && !firdes_gaussian(1, 2, 0.3, -1, t) && !firdes_gaussian(1, 2, 0.3, CPM_MAX_TAPS + 1, t));
    CHECK(!firdes_gaussian(inf, 2, 0.3, 8, t) && !firdes_gaussian(1, nan, 0.3, 8, t) && !firdes_gaussian(1, 2, -inf, 8, t));
    for (unsigned sps : {2u, 3u, 4u, 8u, GMSK_MAX_SPS}) {
        CHECK(gmsk_mod_taps(sps, 0.35, t) && t.size() == 5 * (size_t)sps - 1 && finite(t));
        CHECK(std::fabs(sum(t) - sps) < 1e-3 * sps);
        CHECK(cpm_taps_per_filter(t.size(), sps) == 5);
    }
    CHECK(5 * GMSK_MAX_SPS - 1 <= CPM_MAX_TAPS && 5 * (GMSK_MAX_SPS + 1) - 1 > CPM_MAX_TAPS);
    CHECK(!gmsk_mod_taps(0, 0.35, t) && !gmsk_mod_taps(1, 0.35, t) && !gmsk_mod_taps(GMSK_MAX_SPS + 1, 0.35, t) && !gmsk_mod_taps(0xffffffffu, 0.35, t));
    CHECK(!gmsk_mod_taps(4, nan, t) && !gmsk_mod_taps(4, inf, t));
}

static void test_rows()
{
    for (unsigned I : {1u, 2u, 3u, 4u, 10u})
        for (size_t n : {(size_t)1, (size_t)2, (size_t)7, (size_t)19, (size_t)40}) {
            std::vector<float> taps(n);
            for (size_t i = 0; i < n; ++i) taps[i] = (float)(i + 1);
            const unsigned nt = cpm_taps_per_filter(n, I);
            const std::vector<float> rows = cpm_filter_rows(taps, I);
            CHECK(rows.size() == (size_t)nt * I);
            // gr_interp_fir_filter_XXX.cc.t:77-100: xtaps[i % I][i / I] = padded[i], then gr_reverse
            std::vector<float> padded((size_t)nt * I - n, 0.0f);
            padded.insert(padded.end(), taps.begin(), taps.end());
            for (size_t i = 0; i < padded.size(); ++i) CHECK(rows[(i % I) * nt + (nt - 1 - i / I)] == padded[i]);
        }
    CHECK(cpm_fused_fits(1, 1) && cpm_fused_fits(64, 16) && cpm_fused_fits(1024, 1) && cpm_fused_fits(204, 5));
    CHECK(!cpm_fused_fits(1, 0) && !cpm_fused_fits(2, 17) && !cpm_fused_fits(65, 16) && !cpm_fused_fits(1025, 1) && !cpm_fused_fits(0xffffffffu, 16));
}

int main()
{
    test_phase_response();
    test_gaussian();
    test_rows();
    if (failures) {
        std::printf("cpm_taps_test: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("cpm_taps_test ok\n");
    return 0;
}
