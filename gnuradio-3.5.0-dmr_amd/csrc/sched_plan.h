// sched_plan.h -- the data-independent index schedules of pfb_arb_resampler and fractional_interpolator as plain host
// arithmetic: which outputs one general_work produces, where each reads its input, and the state it leaves.  Used by
// csrc/capi_arbresamp.hip and csrc/capi_fracinterp.hip, whose handles keep only state and locking, and by
// host/sched_plan_test.cc, which runs the closed forms against the walks on a CPU.  Includes no HIP header.  Not part
// of the ABI.
//
// Both blocks produce outputs whose place in the input does not depend on the data.  Each has a closed form, valid when
// the float sums of the reference's loop never round (arb_on_grid / frac_closed_form say when), and a walk of the
// reference's float arithmetic that lists one step per output when they do.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

// frac_imu_of is the one function here that a kernel calls too.  A HIP file includes <hip/hip_runtime.h> before this
// header (frac_interp.h and arb_resampler.h do), which is where __host__ and __device__ come from.
#ifdef __HIPCC__
#define GRHIP_HOST_DEVICE __host__ __device__
#else
#define GRHIP_HOST_DEVICE
#endif

namespace grhip {

// ---- shared by both schedules ----------------------------------------------------------------------------------------

// n = the first k in [0, nout] that does not fit (fits(k) is true up to some k and false from there on), searched by
// doubling and then bisecting.  fits is only asked for k < 2 * kmax; *too_many (and 0) when the doubling reaches kmax
// with outputs still fitting and nout beyond it.
template <class Fits>
long long first_not(long long nout, long long kmax, Fits fits, bool *too_many)
{
    long long hi = 1;
    while (hi < nout && hi < kmax && fits(hi)) hi *= 2;
    if (hi >= kmax && hi < nout) { *too_many = true; return 0; }
    long long lo = 0;
    hi = std::min(hi, nout);
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (!fits(mid)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Walked schedule of n steps, pos(k) the first input item step k reads and `tail` the items it reads from there: the
// largest tile (max_tile halved until it fits) whose input span fits `cap` LDS items, and the span that tile needs at
// most: LDS is sized to it, not to the cap, so short spans leave room for more workgroups per CU.
template <class Pos>
int walked_tile(size_t n, int max_tile, long long tail, long long cap, Pos pos, int *span)
{
    for (int tile = max_tile;; tile /= 2) {
        long long worst = 0;
        for (size_t k0 = 0; k0 < n; k0 += tile) {
            const size_t kl = std::min(n, k0 + tile) - 1;
            worst = std::max(worst, pos(kl) - pos(k0) + tail);
        }
        if (worst <= cap || tile == 1) { *span = (int)std::min(worst, cap); return tile; }
    }
}

// ---- gr_pfb_arb_resampler_ccf / _fff (filter/gr_pfb_arb_resampler_ccf.cc:158-209) --------------------------------------
//
// The schedule (count_k, j_k, acc_k) of the outputs does not depend on the data.  When acc and the fractional rate
// f are multiples of 2^-23 (always, from fresh state, when rate <= filter_size: then R/rate >= 1 and f is a float
// below 1 with an exponent >= -23), every acc + f of the reference is exact and its walk equals the closed form of
// ArbSched; produced and consumed follow on the host from a binary search.  Otherwise (rate > filter_size: the sums
// round) the host walks the reference's float32 arithmetic and hands the kernel one ArbStep per output.

// the per-output position inside a tile is 32-bit: dec_rate + 1 <= ARB_MAX_DEC, i.e. filter_size / rate < 2^20
constexpr unsigned ARB_MAX_DEC = 1u << 20;
constexpr long long ARB_MAX_OUT = 1LL << 40;          // closed form: k * F stays below 2^64
constexpr long long ARB_MAX_STEPS = 1LL << 28;        // walked schedule: 4 GB of steps

// One output's place in the schedule when it has to come from a float walk (rate > filter_size): the
// first input item the two filters read, the filter index j and the interpolation weight acc.
struct ArbStep {
    long long count;
    int j;
    float acc;
};

// The index schedule of one call.  Closed form (steps == nullptr), output k of the launch:
//   T_k = A0 + k*F,  pos_k = j0 + k*D + (T_k >> 23),  count_k = c0 + pos_k / R,  j_k = pos_k % R,
//   acc_k = (T_k & (2^23 - 1)) * 2^-23.
// count_k indexes the logical input: `lead` zeros, then the n_phys items at `in`.
struct ArbSched {
    long long c0 = 0;
    unsigned long long j0 = 0, A0 = 0;
    unsigned F = 0, D = 0;
    const ArbStep *steps = nullptr;         // device array of nout entries, or nullptr for the closed form
};

// the reference's state between general_work calls
struct ArbState {
    long long count = 0;        // d_start_index (at entry) / count (at exit)
    unsigned j = 0;             // d_last_filter (may be >= R: the last call ended before wrapping it)
    float acc = 0.f;            // d_acc
};

// what set_rate derives from the rate (.h:166-170)
struct ArbRate {
    unsigned R = 0;             // filter_size
    unsigned D = 0;             // d_dec_rate
    float f = 0.f;              // d_flt_rate
};

// what one run of the loop of general_work does (.cc:172-201), from state `s`, inputs limited by
// count < max_input, at most nout outputs
struct ArbPlan {
    long long n = 0;            // outputs produced
    ArbState end;               // count, j, acc at the loop's exit
    bool closed = true;         // schedule by the closed form (sc) or by steps
    ArbSched sc;
    std::vector<ArbStep> steps;
    bool too_many = false;      // more outputs than a launch takes (ARB_MAX_OUT)
    unsigned D = 0;             // dec_rate and mode the plan was made with: tiles and the kernel follow the plan,
    int mode = 0;               // not the handle's current values
};

// set_rate (.h:166-170): the float arithmetic of the reference.  Returns what is wrong with the rate, or nullptr.
inline const char *arb_rate_params(unsigned R, float rate, ArbRate *r)
{
    if (!(rate > 0.f) || !std::isfinite(rate)) return "pfb_arb_resampler: rate must be finite and > 0";
    const float x = (float)R / rate;
    const float fl = floorf(x);
    if (!(fl + 1.f <= (float)ARB_MAX_DEC)) return "pfb_arb_resampler: filter_size / rate must be below 2^20";
    r->R = R;
    r->D = (unsigned)fl;
    r->f = x - (float)r->D;
    return nullptr;
}

// v * 2^23 as an integer, if v is a multiple of 2^-23 in [0, 1)
inline bool arb_on_grid(float v, unsigned long long *q)
{
    const float s = v * 8388608.0f;                   // exact: a power-of-two scaling
    if (!(s >= 0.f) || s >= 8388608.0f || s != floorf(s)) return false;
    *q = (unsigned long long)s;
    return true;
}

// pos_k of the closed form from state s (A0 = acc * 2^23); count_k = s.count + pos_k / R
inline long long arb_cf_pos(const ArbState &s, unsigned long long A0, unsigned F, unsigned D, long long k)
{
    const unsigned long long T = A0 + (unsigned long long)k * F;
    return (long long)((unsigned long long)s.j + (unsigned long long)k * D + (T >> 23));
}

// the closed form, for A0 = s.acc * 2^23 and F = r.f * 2^23 from arb_on_grid; the outer loop runs (nout > 0 and
// s.count < max_input)
inline void arb_plan_closed(const ArbState &s, const ArbRate &r, unsigned long long A0, unsigned F, long long max_input,
                            long long nout, ArbPlan *p)
{
    const unsigned D = r.D;
    const long long R = r.R;
    // n = the first k with count_k >= max_input, at most nout (count_k does not decrease)
    p->n = first_not(nout, ARB_MAX_OUT,
                     [&](long long k) { return s.count + arb_cf_pos(s, A0, F, D, k) / R < max_input; }, &p->too_many);
    if (p->too_many) return;
    const long long posn = arb_cf_pos(s, A0, F, D, p->n);
    if (p->n == nout) {         // stopped by noutput_items: j not wrapped (.cc:194)
        const long long prev = arb_cf_pos(s, A0, F, D, p->n - 1) / R;
        p->end.count = s.count + prev;
        p->end.j = (unsigned)(posn - prev * R);
    } else {                    // stopped by the input: the wrap that ran past it has happened
        p->end.count = s.count + posn / R;
        p->end.j = (unsigned)(posn % R);
    }
    p->end.acc = (float)((A0 + (unsigned long long)p->n * F) & 0x7fffffull) * (1.0f / 8388608.0f);
    p->sc.c0 = s.count; p->sc.j0 = s.j; p->sc.A0 = A0; p->sc.F = F; p->sc.D = D;
}

// the reference's loop in float32 (.cc:172-201), positions kept exact in 64 bits
inline void arb_plan_walked(const ArbState &s, const ArbRate &r, long long max_input, long long nout, ArbPlan *p)
{
    const unsigned R = r.R;
    long long count = s.count, i = 0;
    unsigned j = s.j;
    float acc = s.acc;
    while (i < nout && count < max_input) {
        while (j < R && i < nout) {
            if (i >= ARB_MAX_STEPS) { p->too_many = true; return; }
            p->steps.push_back(ArbStep{count, (int)j, acc});
            ++i;
            acc += r.f;
            j += r.D + (int)floorf(acc);
            acc = fmodf(acc, 1.0f);
        }
        if (i < nout) {
            count += j / R;
            j = j % R;
        }
    }
    p->n = i;
    p->end.count = count; p->end.j = j; p->end.acc = acc;
}

inline ArbPlan arb_plan(const ArbState &s, const ArbRate &r, long long max_input, long long nout)
{
    ArbPlan p;
    p.end = s;
    p.D = r.D;
    unsigned long long Fq = 0, A0 = 0;
    p.closed = arb_on_grid(r.f, &Fq) && arb_on_grid(s.acc, &A0);
    if (nout <= 0 || s.count >= max_input) return p;          // the outer loop never runs (.cc:175)
    if (p.closed) arb_plan_closed(s, r, A0, (unsigned)Fq, max_input, nout, &p);
    else arb_plan_walked(s, r, max_input, nout, &p);
    return p;
}

// Closed-form schedule: the largest tile (at most max_tile outputs) whose input span fits `cap` LDS items, and the span
// that tile needs at most.  pos_k - pos_0 <= k*(D+1) and pos_0 % R < R: count_k - count_0 <= (R-1 + k*(D+1)) / R.
inline int arb_closed_tile(unsigned R, unsigned D, unsigned tpf, long long cap, int max_tile, int *span)
{
    const long long t = 1 + (cap - (long long)tpf) * R / ((long long)D + 1);
    const int tile = (int)std::min<long long>(max_tile, std::max<long long>(1, t));
    *span = (int)(((long long)R - 1 + (long long)(tile - 1) * ((long long)D + 1)) / R + tpf);
    return tile;
}

// create_diff_taps (.cc:130-138), then create_taps (.cc:93-124) for both banks, as the kernel reads them: R rows of S
// (h, dh) pairs, S >= tpf, filter i's taps proto[i + t*R] zero padded to R*tpf and reversed as gr_fir_XXX::set_taps
// stores them.  ntaps >= 2.
inline std::vector<float> arb_tap_pairs(const float *taps, size_t ntaps, unsigned R, unsigned tpf, unsigned S)
{
    std::vector<float> proto((size_t)R * tpf, 0.f), diff((size_t)R * tpf, 0.f);
    for (size_t i = 0; i < ntaps; ++i) proto[i] = taps[i];
    for (size_t i = 0; i + 1 < ntaps; ++i) diff[i] = taps[i + 1] - taps[i];
    diff[ntaps - 1] = diff[ntaps - 2];
    std::vector<float> pairs(2 * (size_t)R * S, 0.f);
    for (unsigned i = 0; i < R; ++i)
        for (unsigned k = 0; k < tpf; ++k) {
            const size_t src = i + (size_t)(tpf - 1 - k) * R;
            pairs[2 * ((size_t)i * S + k)] = proto[src];
            pairs[2 * ((size_t)i * S + k) + 1] = diff[src];
        }
    return pairs;
}

// the state the next call starts from and what this one consumed (.cc:204-207)
inline ArbState arb_carry(const ArbState &end, long long ninput, int *consumed)
{
    ArbState st = end;
    st.count = std::max(0LL, end.count - ninput);               // .cc:204
    *consumed = (int)std::min(end.count, ninput);               // .cc:207
    return st;
}

// ---- gr_fractional_interpolator_ff / _cc (filter/gr_fractional_interpolator_ff.cc:67-93) -------------------------------
//
// The walk of general_work (.cc:83-87) is
//     double s = d_mu + d_mu_inc;  double f = floor(s);  d_mu = s - f;  ii += (int) f;
// d_mu and d_mu_inc are floats, so the sum is a FLOAT sum, widened afterwards; s - f is the fraction of a float and
// narrows back exactly.  The float sum is the one place that rounds.  It is exact when mu and mu_inc are multiples of
// a power of two g with 1 + mu_inc <= 2^24 * g: every s is then a multiple of g below 2^24 * g.  With positions in
// units of 2^-24 (A0 = mu * 2^24, F = mu_inc * 2^24) that reads 2^24 + F <= 2^24 * lowbit(A0 | F), the walk equals the
// closed form of FracSched, and produced and consumed follow on the host from a binary search.
// A float ratio in [2^e, 2^(e+1)) is a multiple of 2^(e-23), so from a phase on its grid it needs one or two more
// trailing zero bits than it is sure to have: 0.5, 0.75, 1.25, 2.5 and 10 have them, and so do 1.3f, 160/147.f and
// 4.8f as it happens.  Otherwise (1.0001f, 147/160.f, 0.3f, 0.01f; a phase of 2^-24 or 0.1f) a sum rounds sooner or
// later, the host walks the reference's arithmetic and hands the kernel one (ii, imu) per output.

constexpr int FRAC_NTAPS = 8;
constexpr int FRAC_NSTEPS = 128;
constexpr long long FRAC_MAX_STEPS = 1LL << 28;        // walked schedule: 2 GB of steps
constexpr unsigned long long FRAC_ONE = 1ull << 24;

// The index schedule of one call.  Closed form (steps == nullptr), output k of the launch:
//   T_k = A0 + k*F,  ii_k = ii0 + (T_k >> 24),  m_k = T_k mod 2^24,  imu_k = round-half-even(m_k / 2^17);
//   with first_one (mu == 1.0f at the start) output 0 is ii0 with filter 128 instead.
// Walked: steps[k] = ((ii_k - 0) << 8) | imu_k, ii_k counted from the start of `in` as in the closed form.
struct FracSched {
    long long ii0 = 0;
    unsigned long long A0 = 0, F = 0;
    int first_one = 0;
    const unsigned long long *steps = nullptr;  // device array of nout entries, or nullptr for the closed form
};

// the state between general_work calls: d_mu, and the items a short call could not consume (0 while forecast is
// honoured: the reference has no such state)
struct FracState {
    float mu = 0.f;
    long long skip = 0;
};

struct FracPlan {
    long long n = 0;            // outputs produced
    FracState end;              // mu after the last output, ii after it (as skip)
    bool closed = true;
    FracSched sc;
    std::vector<unsigned long long> steps;
    bool too_many = false;
    int mode = 0;               // the mode the plan was made with
};

// imu = (int) rint(mu * NSTEPS) for mu = m * 2^-24: round-half-even of m / 2^17
GRHIP_HOST_DEVICE inline int frac_imu_of(unsigned m) { return (int)((m + 0xffffu + ((m >> 17) & 1u)) >> 17); }

// v * 2^24 as an integer, if it is one (v >= 0, below 2^20: the product is exact, a power-of-two scaling)
inline bool frac_on_grid(float v, unsigned long long *q)
{
    const float s = v * 16777216.0f;
    if (!(s >= 0.f) || s != floorf(s) || s >= 17592186044416.0f) return false;      // 2^44
    *q = (unsigned long long)s;
    return true;
}

// the closed form holds from (mu, mu_inc): see the head of this section
inline bool frac_closed_form(float mu, float inc, unsigned long long *A0, unsigned long long *F)
{
    if (!frac_on_grid(mu, A0) || !frac_on_grid(inc, F) || *F == 0) return false;
    const unsigned long long m = *A0 | *F, low = m & (~m + 1);
    return FRAC_ONE + *F <= low * FRAC_ONE;            // low < 2^44: no overflow
}

// ii_k (from the start of the input) of the closed form
inline long long frac_cf_ii(const FracSched &sc, long long k)
{
    if (sc.first_one && k == 0) return sc.ii0;
    return sc.ii0 + (long long)((sc.A0 + (unsigned long long)k * sc.F) >> 24);
}

// the closed form, for A0 and F from frac_closed_form; nout > 0 and the first output fits
inline void frac_plan_closed(const FracState &s, unsigned long long A0, unsigned long long F, long long ninput,
                             long long nout, FracPlan *p)
{
    p->sc.ii0 = s.skip; p->sc.A0 = A0; p->sc.F = F; p->sc.first_one = A0 == FRAC_ONE;
    // ii_k <= ninput - 8 bounds k * F by ninput * 2^24; cap the search so that k * F stays below 2^62
    const long long kmax = (long long)std::min<unsigned long long>((1ull << 62) / F, 1ull << 62);
    // n = the first k that does not fit, at most nout (ii_k does not decrease)
    p->n = first_not(nout, kmax, [&](long long k) { return frac_cf_ii(p->sc, k) + FRAC_NTAPS <= ninput; }, &p->too_many);
    if (p->too_many) return;
    const unsigned long long Tn = A0 + (unsigned long long)p->n * F;
    p->end.mu = (float)(Tn & (FRAC_ONE - 1)) * (1.0f / 16777216.0f);
    p->end.skip = s.skip + (long long)(Tn >> 24);
}

// the reference's loop (.cc:79-88), positions kept in 64 bits
inline void frac_plan_walked(const FracState &s, float mu_inc, long long ninput, long long nout, FracPlan *p)
{
    float mu = s.mu;
    long long ii = s.skip, i = 0;
    while (i < nout && ii + FRAC_NTAPS <= ninput) {
        if (i >= FRAC_MAX_STEPS) { p->too_many = true; return; }
        int imu = (int)rint(mu * (float)FRAC_NSTEPS);            // gri_mmse_fir_interpolator.cc:64
        imu = imu < 0 ? 0 : (imu > FRAC_NSTEPS ? FRAC_NSTEPS : imu);
        p->steps.push_back(((unsigned long long)ii << 8) | (unsigned)imu);
        ++i;
        const float sf = mu + mu_inc;                           // float + float
        const double sd = sf, f = floor(sd);
        mu = (float)(sd - f);
        ii += (long long)f;
    }
    p->n = i;
    p->end.mu = mu; p->end.skip = ii;
}

// what one general_work does from state s: the outputs k < nout with ii_k + 8 <= ninput
inline FracPlan frac_plan(const FracState &s, float mu_inc, long long ninput, long long nout)
{
    FracPlan p;
    p.end = s;
    unsigned long long A0 = 0, F = 0;
    p.closed = frac_closed_form(s.mu, mu_inc, &A0, &F);
    if (nout <= 0 || s.skip + FRAC_NTAPS > ninput) return p;
    if (p.closed) frac_plan_closed(s, A0, F, ninput, nout, &p);
    else frac_plan_walked(s, mu_inc, ninput, nout, &p);
    return p;
}

// the state the next call starts from and what this one consumed
inline FracState frac_carry(const FracState &end, long long ninput, int *consumed)
{
    const long long c = std::min(end.skip, ninput);
    *consumed = (int)c;
    return FracState{end.mu, end.skip - c};
}

}  // namespace grhip
