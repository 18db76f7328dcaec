// fll_taps_test.cc -- csrc/fll_taps.h (gr_firdes::root_raised_cosine and digital_fll_band_edge_cc::design_filter) under
// the address and undefined-behaviour sanitizers: host arithmetic only, needs neither libgrhip.so nor HIP.
//
//   fll_taps_test                                  the checks below; prints "fll_taps_test ok"
//   fll_taps_test taps SPS ROLLOFF SIZE            the lower, then the upper taps as hex bit patterns (re im re im ...)
//   fll_taps_test rrc GAIN FS SYMRATE ALPHA NTAPS  the taps as hex bit patterns
// (tests/test_fll_band_edge_cpu.py holds the printed taps against the reference's.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#include "../csrc/fll_taps.h"

using namespace grhip;
typedef std::vector<std::complex<float>> cvec;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

static bool finite_taps(const cvec &t)
{
    for (const auto &c : t) if (!std::isfinite(c.real()) || !std::isfinite(c.imag())) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc == 5 && std::string(argv[1]) == "taps") {
        cvec lo, up;
        if (const char *e = fll_design((float)atof(argv[2]), (float)atof(argv[3]), atoi(argv[4]), lo, up)) { printf("%s\n", e); return 1; }
        for (const cvec *t : {&lo, &up})
            for (const auto &c : *t) printf("%08x %08x\n", bits(c.real()), bits(c.imag()));
        return 0;
    }
    if (argc == 7 && std::string(argv[1]) == "rrc") {
        std::vector<float> t;
        if (const char *e = rrc_design(atof(argv[2]), atof(argv[3]), atof(argv[4]), atof(argv[5]), atoi(argv[6]), t)) { printf("%s\n", e); return 1; }
        for (float v : t) printf("%08x\n", bits(v));
        return 0;
    }
    const float nanf_ = std::numeric_limits<float>::quiet_NaN(), inff = std::numeric_limits<float>::infinity();
    const double nan_ = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    cvec lo, up;
    // ---- design_filter: size 1, size 1024, rolloff 0 and 1, fractional sps
    CHECK(!fll_design(2.0f, 0.5f, 1, lo, up) && lo.size() == 1 && up.size() == 1 && finite_taps(lo) && finite_taps(up));
    CHECK(lo[0].real() == 1.0f && lo[0].imag() == 0.0f && up[0].real() == 1.0f);           // tap / power, expj(0)
    CHECK(!fll_design(4.0f, 0.35f, 1024, lo, up) && lo.size() == 1024 && up.size() == 1024 && finite_taps(lo) && finite_taps(up));
    CHECK(!fll_design(2.0f, 1.0f, 1024, lo, up) && lo.size() == 1024 && finite_taps(lo));
    CHECK(!fll_design(4.0f, 0.0f, 55, lo, up) && lo.size() == 55 && finite_taps(lo) && finite_taps(up));
    CHECK(!fll_design(4.0f, 1.0f, 55, lo, up) && lo.size() == 55 && finite_taps(lo) && finite_taps(up));
    CHECK(!fll_design(2.5f, 0.35f, 129, lo, up) && lo.size() == 129);
    // the upper taps are the lower ones' conjugates: cos is even and sin odd in sincosf
    for (size_t i = 0; i < lo.size(); ++i) CHECK(lo[i].real() == up[i].real() && lo[i].imag() == -up[i].imag());
    // the smallest sps inside the 1024 rad/sample bound, with the largest filter: M = rint(size / sps) stays an int
    CHECK(!fll_check(0.0123f, 0.35f, 1024));
    (void)fll_design(0.0123f, 0.35f, 1024, lo, up);             // may be refused for its taps; must not trip a sanitizer
    // ---- every refusal; a refused design leaves the vectors alone
    CHECK(!fll_design(4.0f, 0.35f, 45, lo, up) && lo.size() == 45);
    const cvec keep = lo;
    CHECK(fll_design(0.0f, 0.35f, 45, lo, up) && fll_design(-1.0f, 0.35f, 45, lo, up) && fll_design(nanf_, 0.35f, 45, lo, up));
    CHECK(fll_design(inff, 0.35f, 45, lo, up));
    CHECK(fll_design(4.0f, -0.01f, 45, lo, up) && fll_design(4.0f, 1.01f, 45, lo, up) && fll_design(4.0f, nanf_, 45, lo, up));
    CHECK(fll_design(4.0f, 0.35f, 0, lo, up) && fll_design(4.0f, 0.35f, -3, lo, up) && fll_design(4.0f, 0.35f, 1025, lo, up));
    CHECK(fll_design(0.012f, 0.35f, 45, lo, up));               // 2 pi 2 / sps = 1047 rad/sample
    CHECK(fll_design(1e-30f, 0.35f, 45, lo, up));
    CHECK(lo == keep);
    CHECK(fll_max_freq_of(4.0f) == (float)M_PI && fll_max_freq_of(2.0f) == (float)(2 * M_PI));
    // ---- root_raised_cosine
    std::vector<float> t;
    CHECK(!rrc_design(4, 4, 1.0, 0.35, 45, t) && t.size() == 45);
    CHECK(!rrc_design(4, 4, 1.0, 0.35, 44, t) && t.size() == 45);           // ntaps |= 1
    CHECK(!rrc_design(32, 64, 1.0, 0.35, 704, t) && t.size() == 705);
    CHECK(!rrc_design(1, 8, 2.0, 0.35, 1, t) && t.size() == 1 && t[0] == 1.0f);
    // alpha == 1: the taps one symbol out are -1 before the scaling and stay out of the scale
    CHECK(!rrc_design(1, 4, 1.0, 1.0, 45, t) && t.size() == 45 && t[22 - 1] == t[22 + 1]);
    double sum = 0;
    for (float v : t) sum += v;
    CHECK(fabs(sum - (1.0 + 2.0 * t[21])) < 1e-5);              // the other taps sum to the gain
    // the |x3| < 1e-6 branch with alpha != 1: 4 alpha xindx / spb == +-1 at xindx = +-2 (alpha 0.5) and +-4 (alpha 0.25)
    CHECK(!rrc_design(1, 4, 1.0, 0.5, 45, t) && std::isfinite(t[22 + 2]) && t[22 + 2] == t[22 - 2] && t[24] > t[25] && t[24] < t[23]);
    CHECK(!rrc_design(2, 4, 1.0, 0.25, 44, t) && std::isfinite(t[22 + 4]) && t[22 + 4] == t[22 - 4] && t[26] > t[27] && t[26] < t[25]);
    // refusals
    const std::vector<float> keep_t = t;
    CHECK(rrc_design(nan_, 4, 1, 0.35, 45, t) && rrc_design(1, inf, 1, 0.35, 45, t) && rrc_design(1, 4, -inf, 0.35, 45, t));
    CHECK(rrc_design(1, 4, 1, nan_, 45, t) && rrc_design(1, 4, 1, 0.35, 0, t) && rrc_design(1, 4, 1, 0.35, -5, t));
    CHECK(rrc_design(1, 4, 1, 0.35, 1 << 24, t) && rrc_design(1, 4, 1, 0.35, std::numeric_limits<int>::max(), t));
    CHECK(t == keep_t);
    CHECK(!rrc_design(1, 4, 0.0, 0.35, 5, t) && t.size() == 5);             // spb infinite: taps not finite, as in the reference
    if (fails) return 1;
    printf("fll_taps_test ok\n");
    return 0;
}
