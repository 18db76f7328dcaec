// sched_plan_test.cc -- the closed-form schedules of csrc/sched_plan.h against the walks of the reference's float
// arithmetic, on the CPU: wherever the block's own predicate says the closed form holds, both must give the same number
// of outputs, the same end state bit for bit and the same place for every output.  Exits non-zero with the first
// disagreeing case printed.  Links nothing of HIP.
#include <cstdio>
#include <cstring>

#include "../csrc/sched_plan.h"

using namespace grhip;

namespace {

unsigned bits(float v)
{
    unsigned u;
    memcpy(&u, &v, sizeof u);
    return u;
}

const long long NOUTS[] = {1, 7, 1000, 1 << 20};
long long compared = 0, outputs = 0;

// ---- pfb_arb_resampler ------------------------------------------------------------------------------------------------

bool arb_case(const ArbState &s, const ArbRate &r, float rate, unsigned tpf, long long max_input, long long nout)
{
    unsigned long long Fq = 0, A0 = 0;
    if (!(arb_on_grid(r.f, &Fq) && arb_on_grid(s.acc, &A0))) {   // every rate here is <= R: always on the grid
        printf("arb: off the 2^-23 grid: rate %.9g R %u f %.9g, state count %lld j %u acc %.9g\n", rate, r.R, r.f, s.count,
               s.j, s.acc);
        return false;
    }
    if (s.count >= max_input) return true;                       // neither loop runs
    const unsigned F = (unsigned)Fq;
    ArbPlan c, w;
    c.end = w.end = s;
    arb_plan_closed(s, r, A0, F, max_input, nout, &c);
    arb_plan_walked(s, r, max_input, nout, &w);
    const char *what = nullptr;
    long long at = -1;
    if (c.too_many || w.too_many) what = "too_many";
    else if (c.n != w.n) what = "n";
    else if (c.end.count != w.end.count || c.end.j != w.end.j || bits(c.end.acc) != bits(w.end.acc)) what = "end state";
    for (long long k = 0; !what && k < c.n; ++k) {
        const long long pos = arb_cf_pos(s, A0, F, r.D, k);
        const float acc = (float)((A0 + (unsigned long long)k * F) & 0x7fffffull) * (1.0f / 8388608.0f);
        const ArbStep &st = w.steps[(size_t)k];
        if (s.count + pos / (long long)r.R != st.count || (int)(pos % (long long)r.R) != st.j || bits(acc) != bits(st.acc)) {
            what = "output";
            at = k;
        }
    }
    ++compared;
    outputs += c.n;
    if (!what) return true;
    printf("arb: %s differs (output %lld): rate %.9g R %u tpf %u D %u f %.9g, state count %lld j %u acc %.9g, "
           "max_input %lld nout %lld: closed n %lld end (%lld, %u, %.9g), walked n %lld end (%lld, %u, %.9g)\n",
           what, at, rate, r.R, tpf, r.D, r.f, s.count, s.j, s.acc, max_input, nout, c.n, c.end.count, c.end.j, c.end.acc,
           w.n, w.end.count, w.end.j, w.end.acc);
    return false;
}

bool arb_cases()
{
    const float rates[] = {0.0192f, 0.5f, 1.0f, 1.25f, 5.3f, 31.999f, 32.0f};
    const long long extra[] = {1, 100, 4097};                   // ninput - tpf
    for (unsigned tpf : {8u, 16u})
        for (float rate : rates) {
            ArbRate r;
            if (const char *bad = arb_rate_params(32, rate, &r)) { printf("arb: rate %.9g refused: %s\n", rate, bad); return false; }
            // fresh; left by a call stopped by noutput_items; left by a call stopped by the input
            ArbState starts[3];
            int consumed;
            ArbPlan a, b;
            arb_plan_walked(ArbState(), r, 4097, 7, &a);
            if (a.n != 7) { printf("arb: rate %.9g: the 7-output call was not stopped by noutput_items\n", rate); return false; }
            starts[1] = arb_carry(a.end, 4097 + tpf, &consumed);
            arb_plan_walked(ArbState(), r, 100, 1 << 20, &b);
            if (b.n >= 1 << 20) { printf("arb: rate %.9g: the long call was not stopped by the input\n", rate); return false; }
            starts[2] = arb_carry(b.end, 100 + tpf, &consumed);
            for (const ArbState &s : starts)
                for (long long e : extra)
                    for (long long nout : NOUTS)
                        if (!arb_case(s, r, rate, tpf, e, nout)) return false;
        }
    return true;
}

// ---- fractional_interpolator ------------------------------------------------------------------------------------------

bool frac_case(const FracState &s, float ratio, long long ninput, long long nout)
{
    unsigned long long A0 = 0, F = 0;
    if (!frac_closed_form(s.mu, ratio, &A0, &F)) {               // a walk from a closed-form pair stays on its grid
        printf("frac: closed_form is false for ratio %.9g from state mu %.9g skip %lld\n", ratio, s.mu, s.skip);
        return false;
    }
    if (s.skip + FRAC_NTAPS > ninput) return true;               // no output fits
    FracPlan c, w;
    c.end = w.end = s;
    frac_plan_closed(s, A0, F, ninput, nout, &c);
    frac_plan_walked(s, ratio, ninput, nout, &w);
    const char *what = nullptr;
    long long at = -1;
    if (c.too_many || w.too_many) what = "too_many";
    else if (c.n != w.n) what = "n";
    else if (bits(c.end.mu) != bits(w.end.mu) || c.end.skip != w.end.skip) what = "end state";
    for (long long k = 0; !what && k < c.n; ++k) {
        const long long ii = frac_cf_ii(c.sc, k);
        const int imu = c.sc.first_one && k == 0 ? FRAC_NSTEPS
                                                 : frac_imu_of((unsigned)((A0 + (unsigned long long)k * F) & (FRAC_ONE - 1)));
        const unsigned long long st = w.steps[(size_t)k];
        if (ii != (long long)(st >> 8) || imu != (int)(st & 0xffu)) {
            what = "output";
            at = k;
        }
    }
    ++compared;
    outputs += c.n;
    if (!what) return true;
    printf("frac: %s differs (output %lld): ratio %.9g, state mu %.9g skip %lld, ninput %lld nout %lld: closed n %lld end "
           "(%.9g, %lld), walked n %lld end (%.9g, %lld)\n",
           what, at, ratio, s.mu, s.skip, ninput, nout, c.n, c.end.mu, c.end.skip, w.n, w.end.mu, w.end.skip);
    return false;
}

bool frac_cases()
{
    const float closed[][2] = {{0.f, 0.5f},          {0.f, 0.75f}, {0.5f, 1.25f}, {1.0f, 160 / 147.f},
                               {0.f, 2.5f},          {0.f, 10.f},  {0.25f, 1.3f}, {0.f, 4.8f}};
    const float walked[][2] = {{0.f, 1.0001f}, {0.f, 147 / 160.f}, {0.f, 0.3f}, {0.f, 0.01f}, {ldexpf(1.f, -24), 0.5f},
                               {0.1f, 0.5f}};
    unsigned long long A0, F;
    for (const auto &c : walked)
        if (frac_closed_form(c[0], c[1], &A0, &F)) {
            printf("frac: closed_form(mu %.9g, ratio %.9g) is true, the float sums round\n", c[0], c[1]);
            return false;
        }
    for (const auto &c : closed) {
        const float mu = c[0], ratio = c[1];
        if (!frac_closed_form(mu, ratio, &A0, &F)) {
            printf("frac: closed_form(mu %.9g, ratio %.9g) is false\n", mu, ratio);
            return false;
        }
        // fresh; left by a call stopped by noutput_items; left by a call stopped by the input
        FracState starts[3];
        int consumed;
        FracPlan a, b;
        starts[0] = FracState{mu, 0};
        frac_plan_walked(starts[0], ratio, 4097, 7, &a);
        if (a.n != 7) { printf("frac: ratio %.9g: the 7-output call was not stopped by noutput_items\n", ratio); return false; }
        starts[1] = frac_carry(a.end, 4097, &consumed);
        frac_plan_walked(starts[0], ratio, 100, 1 << 20, &b);
        if (b.n >= 1 << 20) { printf("frac: ratio %.9g: the long call was not stopped by the input\n", ratio); return false; }
        starts[2] = frac_carry(b.end, 100, &consumed);
        for (const FracState &s : starts)
            for (long long ninput : {8LL, 9LL, 100LL, 4097LL})
                for (long long nout : NOUTS)
                    if (!frac_case(s, ratio, ninput, nout)) return false;
    }
    return true;
}

}  // namespace

int main()
{
    if (!arb_cases() || !frac_cases()) return 1;
    printf("sched_plan_test: %lld cases, %lld outputs agree\n", compared, outputs);
    return 0;
}
