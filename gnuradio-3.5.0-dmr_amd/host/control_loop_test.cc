// control_loop_test -- the loop parameters of gri_control_loop as csrc/control_loop.h restates them, on the CPU under the
// address and undefined-behaviour sanitizers: the constructor's damping and gains, every setter with the reference's
// range checks (general/gri_control_loop.cc:86-145), set_frequency's swapped limits, set_phase's wrap loops, and the
// caps that keep the device walk finite.  Prints alpha and beta as bit patterns for the bandwidths given as arguments
// ("control_loop_test bw damping ..."), which tests/test_carrier_cpu.py compares with the recorded reference.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../csrc/control_loop.h"

using namespace grhip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static unsigned bits(float f)
{
    unsigned u;
    memcpy(&u, &f, sizeof u);
    return u;
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        for (int i = 1; i + 1 < argc; i += 2) {
            ControlLoop c;
            if (!c.init(0.f, 1.f, -1.f) || !c.set_damping_factor((float)atof(argv[i + 1])) || !c.set_loop_bandwidth((float)atof(argv[i]))) {
                printf("refused\n");
                continue;
            }
            printf("%08x %08x\n", bits(c.alpha), bits(c.beta));
        }
        return 0;
    }
    ControlLoop c;
    CHECK(c.init(0.05f, 1.f, -1.f));
    CHECK(c.damping == sqrtf(2.0f) / 2.0f && c.loop_bw == 0.05f && c.max_freq == 1.f && c.min_freq == -1.f);
    {   // gri_control_loop.cc:49-54 spelled out once more
        const float d = c.damping, bw = 0.05f;
        const float denom = (1.0 + 2.0 * d * bw + bw * bw);
        CHECK(bits(c.alpha) == bits((4 * d * bw) / denom) && bits(c.beta) == bits((4 * bw * bw) / denom));
    }
    // the setters and their refusals; a refusal leaves everything as it was
    const ControlLoop before = c;
    CHECK(!c.set_loop_bandwidth(-1e-3f) && !c.set_damping_factor(-0.1f) && !c.set_damping_factor(1.5f));
    CHECK(!c.set_alpha(-0.1f) && !c.set_alpha(1.1f) && !c.set_beta(-0.1f) && !c.set_beta(1.1f));
    CHECK(!c.set_alpha(NAN) && !c.set_beta(NAN) && !c.set_loop_bandwidth(NAN) && !c.set_damping_factor(NAN));
    CHECK(!c.set_loop_bandwidth(INFINITY) && !c.set_loop_bandwidth(1e19f) && !c.set_loop_bandwidth(1.5e19f) && !c.set_loop_bandwidth(3e38f));
    CHECK(!memcmp(&before, &c, sizeof c));
    CHECK(c.set_loop_bandwidth(0.f) && c.alpha == 0.f && c.beta == 0.f);
    CHECK(c.set_damping_factor(0.f) && c.set_damping_factor(1.f) && c.damping == 1.f);
    CHECK(c.set_loop_bandwidth(0.25f) && c.loop_bw == 0.25f);
    CHECK(c.set_alpha(0.f) && c.set_alpha(1.f) && c.alpha == 1.f && c.set_beta(0.f) && c.set_beta(1.f) && c.beta == 1.f);
    // every bandwidth that is accepted leaves finite gains below the bounds the walk's trip count rests on
    for (int e = -149; e <= 127; ++e)
        for (float m : {1.0f, 1.3f, 1.999f})
            for (float d : {0.f, 0.3f, sqrtf(2.0f) / 2.0f, 1.f}) {
                ControlLoop t;
                CHECK(t.init(0.f, 1.f, -1.f) && t.set_damping_factor(d));
                if (t.set_loop_bandwidth(ldexpf(m, e)))
                    CHECK(std::isfinite(t.alpha) && std::isfinite(t.beta) && t.alpha >= 0.f && t.alpha <= 1.0001f && t.beta >= 0.f && t.beta <= 4.0001f);
            }
    // set_frequency: above the maximum gives the minimum, below the minimum the maximum
    CHECK(c.set_frequency(0.5f) == 0.5f && c.set_frequency(1.f) == 1.f && c.set_frequency(-1.f) == -1.f);
    CHECK(c.set_frequency(1.5f) == -1.f && c.set_frequency(-1.5f) == 1.f && std::isnan(c.set_frequency(NAN)));
    // set_phase: (float)((double)phase -+ 2 pi) until within [-2 pi, 2 pi]; float(2 pi) lies above the double 2 pi
    CHECK(ControlLoop::set_phase(1.f) == 1.f && ControlLoop::set_phase(-6.f) == -6.f);
    const float tp = (float)CL_TWOPI;
    CHECK((double)tp > CL_TWOPI && ControlLoop::set_phase(tp) == (float)((double)tp - CL_TWOPI));
    CHECK(ControlLoop::set_phase(nextafterf(tp, 0.f)) == nextafterf(tp, 0.f));
    CHECK(ControlLoop::set_phase(7.f) == (float)(7.0 - CL_TWOPI) && ControlLoop::set_phase(-7.f) == (float)(-7.0 + CL_TWOPI));
    {
        float p = 100.f;
        int trips = 0;
        while (p > CL_TWOPI) { p = (float)(p - CL_TWOPI); trips++; }
        CHECK(trips == 15 && ControlLoop::set_phase(100.f) == p && ControlLoop::set_phase(-100.f) == -p);
    }
    CHECK(std::fabs(ControlLoop::set_phase(CL_PHASE_CAP)) <= tp && std::fabs(ControlLoop::set_phase(-CL_PHASE_CAP)) <= tp);
    // the caps
    CHECK(ControlLoop::phase_ok(CL_PHASE_CAP) && ControlLoop::phase_ok(-CL_PHASE_CAP) && !ControlLoop::phase_ok(nextafterf(CL_PHASE_CAP, INFINITY)));
    CHECK(!ControlLoop::phase_ok(NAN) && !ControlLoop::phase_ok(INFINITY) && !ControlLoop::phase_ok(-INFINITY));
    CHECK(ControlLoop::limits_ok(CL_FREQ_CAP, -CL_FREQ_CAP) && ControlLoop::limits_ok(-0.1f, -0.2f));
    CHECK(!ControlLoop::limits_ok(1025.f, 0.f) && !ControlLoop::limits_ok(0.f, -1025.f) && !ControlLoop::limits_ok(NAN, 0.f) &&
          !ControlLoop::limits_ok(0.f, INFINITY));
    ControlLoop r;
    CHECK(!r.init(0.1f, 2000.f, -1.f) && !r.init(-0.1f, 1.f, -1.f) && r.init(0.1f, -1.f, 1.f));      // max < min is not checked
    if (!fails) printf("control_loop_test ok\n");
    return fails ? 1 : 0;
}
