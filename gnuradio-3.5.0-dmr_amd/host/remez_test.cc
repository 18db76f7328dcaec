// remez_test -- the host arithmetic of csrc/remez.h (gr_remez and the optfir designers) under the address and
// undefined-behaviour sanitizers: the designs of remez_test_vectors.inc (taken from tests/golden/ref_remez.npz, the
// reference's own taps) come back bit for bit, the failing designs fail with the reference's words, every refused
// argument is refused, and one design at the 4096-tap cap runs to its end.  Needs neither libgrhip.so nor HIP.
//
// For tests/test_optfir_cpu.py; no arguments.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../csrc/remez.h"

using namespace grhip;

namespace {

struct Case {
    const char *name;
    int kind;                       // -1: gr_remez itself; else the optfir designer
    int order, type, density;       // gr_remez
    std::vector<double> a, b, c;    // gr_remez: bands, response, weights; optfir: the designer's arguments in a
    const char *message;            // "" for a design that succeeds
    std::vector<uint64_t> taps;
};

#include "remez_test_vectors.inc"

int fails = 0;

void expect(bool ok, const std::string &what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what.c_str());
        ++fails;
    }
}

int design(const Case &c, std::vector<double> &taps, const char **msg)
{
    if (c.kind < 0)
        return remez_design(c.order, c.a.data(), c.a.size(), c.b.data(), c.b.size(), c.c.data(), c.c.size(), c.type, c.density, taps, msg);
    const size_t nf = c.kind <= OPTFIR_HIGH_PASS ? 2 : 4;
    return optfir_design(c.kind, c.a[0], c.a[1], c.a.data() + 2, c.a[2 + nf], c.a[3 + nf], 2, taps, msg);
}

void recorded()
{
    for (const Case &c : CASES) {
        std::vector<double> taps;
        const char *msg = "";
        const int rc = design(c, taps, &msg);
        if (c.message[0]) {
            expect(rc == REMEZ_EFAILED && std::string(msg) == c.message && taps.empty(), std::string(c.name) + ": " + msg);
            continue;
        }
        expect(rc == 0 && taps.size() == c.taps.size(), std::string(c.name) + ": status or tap count, " + msg);
        if (rc || taps.size() != c.taps.size()) continue;
        bool same = true, symmetric = true;
        for (size_t i = 0; i < taps.size(); ++i) {
            uint64_t u;
            std::memcpy(&u, &taps[i], 8);
            same = same && u == c.taps[i];
            symmetric = symmetric && (c.kind < 0 || taps[i] == taps[taps.size() - 1 - i]);
        }
        expect(same, std::string(c.name) + ": not the recorded taps bit for bit");
        expect(symmetric, std::string(c.name) + ": not symmetric");
    }
}

void refused()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double b[4] = {0, .3, .4, 1}, r[4] = {1, 1, 0, 0}, w[2] = {1, 2};
    std::vector<double> t;
    const char *m;
    auto rz = [&](int order, const double *bb, size_t nb, const double *rr, size_t nr, const double *ww, size_t nw, int type, int dens) {
        return remez_design(order, bb, nb, rr, nr, ww, nw, type, dens, t, &m);
    };
    expect(rz(15, b, 4, r, 4, w, 2, 1, 16) == 0 && t.size() == 16, "the accepted call");
    expect(rz(2, b, 4, r, 4, w, 2, 1, 16) == REMEZ_EINVAL, "fewer than 4 taps");
    expect(rz(-7, b, 4, r, 4, w, 2, 1, 16) == REMEZ_EINVAL, "a negative order");
    expect(rz(15, b, 3, r, 3, w, 1, 1, 16) == REMEZ_EINVAL, "an odd number of band edges");
    expect(rz(15, b, 0, r, 0, w, 0, 1, 16) == REMEZ_EINVAL, "no bands");
    const double dec[4] = {0, .4, .3, 1}, low[4] = {-.1, .3, .4, 1}, high[4] = {0, .3, .4, 1.1};
    expect(rz(15, dec, 4, r, 4, w, 2, 1, 16) == REMEZ_EINVAL, "decreasing edges");
    expect(rz(15, low, 4, r, 4, w, 2, 1, 16) == REMEZ_EINVAL, "an edge below 0");
    expect(rz(15, high, 4, r, 4, w, 2, 1, 16) == REMEZ_EINVAL, "an edge above 1");
    expect(rz(15, b, 4, r, 2, w, 2, 1, 16) == REMEZ_EINVAL, "the response count");
    expect(rz(15, b, 4, r, 4, w, 1, 1, 16) == REMEZ_EINVAL, "the weight count");
    expect(rz(15, b, 4, r, 4, w, 2, 1, 15) == REMEZ_EINVAL, "grid density below 16");
    expect(rz(15, b, 4, r, 4, w, 2, 0, 16) == REMEZ_EINVAL && rz(15, b, 4, r, 4, w, 2, 4, 16) == REMEZ_EINVAL, "an unknown type");
    const double bn[4] = {0, nan, .4, 1}, rn[4] = {1, inf, 0, 0}, wn[2] = {1, nan};
    expect(rz(15, bn, 4, r, 4, w, 2, 1, 16) == REMEZ_EINVAL && rz(15, b, 4, rn, 4, w, 2, 1, 16) == REMEZ_EINVAL &&
               rz(15, b, 4, r, 4, wn, 2, 1, 16) == REMEZ_EINVAL, "arguments that are not finite");
    expect(rz(REMEZ_MAX_TAPS, b, 4, r, 4, w, 2, 1, 16) == REMEZ_ERANGE, "4097 taps");
    expect(rz(54321, b, 4, r, 4, w, 2, 1, 16) == REMEZ_ERANGE, "an order the reference dies of");
    // bands that leave the dense grid fewer than two points, and an empty first band
    const double thin[2] = {0.5, 0.5001}, one[2] = {1, 1}, empty_first[4] = {0, 0, .4, 1};
    expect(rz(3, thin, 2, one, 2, w, 0, 1, 16) == REMEZ_EINVAL, "a grid of fewer than two points");
    rz(15, empty_first, 4, r, 4, w, 2, 1, 16);
    rz(15, empty_first, 4, r, 4, w, 2, 3, 16);
    // a hilbert transformer that starts above the first grid step: the reference writes one point past its grid
    const double hb[2] = {0.1, 0.9};
    expect(rz(30, hb, 2, one, 2, w, 0, 3, 16) == 0 && t.size() == 31, "hilbert, 31 taps from 0.1");
    expect(rz(31, hb, 2, one, 2, w, 0, 3, 16) == 0 && t.size() == 32, "hilbert, 32 taps from 0.1");
    // the designers
    const double f2[2] = {3000, 4500}, fn[2] = {3000, nan};
    expect(optfir_design(OPTFIR_LOW_PASS, 1, 32e3, fn, 0.1, 60, 2, t, &m) == REMEZ_EINVAL, "optfir: not finite");
    expect(optfir_design(OPTFIR_LOW_PASS, 1, 0.0, f2, 0.1, 60, 2, t, &m) == REMEZ_EINVAL, "optfir: fs == 0");
    expect(optfir_design(7, 1, 32e3, f2, 0.1, 60, 2, t, &m) == REMEZ_EINVAL, "optfir: unknown designer");
    expect(optfir_design(OPTFIR_LOW_PASS, 1, 32e3, f2, 0.1, 60, -200, t, &m) == REMEZ_EINVAL, "optfir: an order below 3");
    const double f0[2] = {3000, 3000};
    expect(optfir_design(OPTFIR_LOW_PASS, 1, 32e3, f0, 0.1, 60, 2, t, &m) != 0, "optfir: no transition band");
    const double narrow[2] = {3000, 3001};
    expect(optfir_design(OPTFIR_LOW_PASS, 1, 32e3, narrow, 0.1, 60, 2, t, &m) == REMEZ_ERANGE, "optfir: more than 4096 taps");
}

void at_the_cap()
{
    // (at this length the exchange gives up after a few rounds, as the reference's does: what counts here is that
    // every array is walked at its largest size)
    const double b[4] = {0, .45, .55, 1}, r[4] = {1, 1, 0, 0};
    std::vector<double> t;
    const char *m = "";
    const int rc = remez_design(REMEZ_MAX_TAPS - 1, b, 4, r, 4, nullptr, 0, 1, 16, t, &m);
    std::printf("4096 taps: status %d %s\n", rc, m);
    expect((rc == 0 && t.size() == (size_t)REMEZ_MAX_TAPS) || (rc == REMEZ_EFAILED && t.empty()), "the design at the cap");
}

}  // namespace

int main()
{
    recorded();
    refused();
    at_the_cap();
    if (!fails) std::printf("remez_test ok\n");
    return fails ? 1 : 0;
}
