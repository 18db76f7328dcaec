// capi_fracinterp.hip -- gr_fractional_interpolator_ff / _cc: handle, index schedule and C ABI.
//
// Reference: gnuradio-core/src/lib/filter/gr_fractional_interpolator_ff.cc:38-50 (constructor), 57-65 (forecast),
// 67-93 (general_work); gr_fractional_interpolator_ff.h:51-54 (accessors); gri_mmse_fir_interpolator.cc:61-71.  The
// _cc files differ only in the item type.
//
// The walk of general_work (.cc:83-87) is
//     double s = d_mu + d_mu_inc;  double f = floor(s);  d_mu = s - f;  ii += (int) f;
// d_mu and d_mu_inc are floats, so the sum is a FLOAT sum, widened afterwards; s - f is the fraction of a float and
// narrows back exactly.  The float sum is the one place that rounds.  It is exact when mu and mu_inc are multiples of
// a power of two g with 1 + mu_inc <= 2^24 * g: every s is then a multiple of g below 2^24 * g.  With positions in
// units of 2^-24 (A0 = mu * 2^24, F = mu_inc * 2^24) that reads 2^24 + F <= 2^24 * lowbit(A0 | F), the walk equals the
// closed form of FracSched (frac_interp.h), and produced and consumed follow on the host from a binary search.
// A float ratio in [2^e, 2^(e+1)) is a multiple of 2^(e-23), so from a phase on its grid it needs one or two more
// trailing zero bits than it is sure to have: 0.5, 0.75, 1.25, 2.5 and 10 have them, and so do 1.3f, 160/147.f and
// 4.8f as it happens.  Otherwise (1.0001f, 147/160.f, 0.3f, 0.01f; a phase of 2^-24 or 0.1f) a sum rounds sooner or
// later, the host walks the reference's arithmetic and hands the kernel one (ii, imu) per output.
#include <cmath>
#include <limits>
#include <vector>

#include "frac_interp.h"
#include "grhip_internal.h"

using namespace grhip;

namespace {

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
    int mode = GRHIP_MODE_FAST;
};

constexpr long long FRAC_MAX_STEPS = 1LL << 28;        // walked schedule: 2 GB of steps
constexpr unsigned long long ONE24 = 1ull << 24;

// v * 2^24 as an integer, if it is one (v >= 0, below 2^20: the product is exact, a power-of-two scaling)
bool on_grid(float v, unsigned long long *q)
{
    const float s = v * 16777216.0f;
    if (!(s >= 0.f) || s != floorf(s) || s >= 17592186044416.0f) return false;      // 2^44
    *q = (unsigned long long)s;
    return true;
}

}  // namespace

struct grhip_fractional_interpolator_base : HandleBase {
    bool cplx = true;
    float phase0 = 0.f;         // the constructor's phase_shift: the fresh state of run_captures_device
    float mu_inc = 1.f;         // d_mu_inc
    FracState st;
    int mode = GRHIP_MODE_FAST;
    const DeviceTables *tabs = nullptr;
    DevBuf d_steps;
    std::vector<unsigned long long> h_steps;   // source of the last upload to d_steps, kept until steps_ev has passed
    hipEvent_t steps_ev = nullptr;             // recorded after the last launch that read d_steps
    bool steps_busy = false;

    size_t item() const { return cplx ? 8 : 4; }
    int span_cap() const { return FRAC_SPAN_BYTES / (int)item(); }

    static int check_ratio(float r)
    {
        if (!std::isfinite(r) || !(r > 0.f))
            return fail(GRHIP_ERANGE, "fractional_interpolator: interpolation ratio must be finite and > 0");
        if (!(r < FRAC_MAX_RATIO)) return fail(GRHIP_EINVAL, "fractional_interpolator: interp_ratio must be below 2^20");
        return GRHIP_OK;
    }
    static int check_mu(float m)
    {
        if (!std::isfinite(m) || m < 0.f || m > 1.f)
            return fail(GRHIP_ERANGE, "fractional_interpolator: phase shift must be in [0, 1]");
        return GRHIP_OK;
    }

    // the closed form holds from (mu, mu_inc): see the head of this file
    static bool closed_form(float mu, float inc, unsigned long long *A0, unsigned long long *F)
    {
        if (!on_grid(mu, A0) || !on_grid(inc, F) || *F == 0) return false;
        const unsigned long long m = *A0 | *F, low = m & (~m + 1);
        return ONE24 + *F <= low * ONE24;            // low < 2^44: no overflow
    }

    // ii_k (from the start of the input) of the closed form
    static long long cf_ii(const FracSched &sc, long long k)
    {
        if (sc.first_one && k == 0) return sc.ii0;
        return sc.ii0 + (long long)((sc.A0 + (unsigned long long)k * sc.F) >> 24);
    }

    // what one general_work does from state s: the outputs k < nout with ii_k + 8 <= ninput
    FracPlan plan(const FracState &s, long long ninput, long long nout) const
    {
        FracPlan p;
        p.end = s;
        p.mode = mode;
        unsigned long long A0 = 0, F = 0;
        p.closed = closed_form(s.mu, mu_inc, &A0, &F);
        if (nout <= 0 || s.skip + FRAC_NTAPS > ninput) return p;
        if (p.closed) {
            p.sc.ii0 = s.skip; p.sc.A0 = A0; p.sc.F = F; p.sc.first_one = A0 == ONE24;
            // ii_k <= ninput - 8 bounds k * F by ninput * 2^24; cap the search so that k * F stays below 2^62
            const long long kmax = (long long)std::min<unsigned long long>((1ull << 62) / F, 1ull << 62);
            auto fits = [&](long long k) { return cf_ii(p.sc, k) + FRAC_NTAPS <= ninput; };
            // n = the first k that does not fit, at most nout (ii_k does not decrease)
            long long hi = 1;
            while (hi < nout && hi < kmax && fits(hi)) hi *= 2;
            if (hi >= kmax && hi < nout) { p.too_many = true; return p; }
            long long lo = 0;
            hi = std::min(hi, nout);
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (!fits(mid)) hi = mid; else lo = mid + 1;
            }
            p.n = lo;
            const unsigned long long Tn = A0 + (unsigned long long)p.n * F;
            p.end.mu = (float)(Tn & (ONE24 - 1)) * (1.0f / 16777216.0f);
            p.end.skip = s.skip + (long long)(Tn >> 24);
            return p;
        }
        // the reference's loop (.cc:79-88), positions kept in 64 bits
        float mu = s.mu;
        long long ii = s.skip, i = 0;
        while (i < nout && ii + FRAC_NTAPS <= ninput) {
            if (i >= FRAC_MAX_STEPS) { p.too_many = true; return p; }
            int imu = (int)rint(mu * (float)FRAC_NSTEPS);            // gri_mmse_fir_interpolator.cc:64
            imu = imu < 0 ? 0 : (imu > FRAC_NSTEPS ? FRAC_NSTEPS : imu);
            p.steps.push_back(((unsigned long long)ii << 8) | (unsigned)imu);
            ++i;
            const float sf = mu + mu_inc;                           // float + float
            const double sd = sf, f = floor(sd);
            mu = (float)(sd - f);
            ii += (long long)f;
        }
        p.n = i;
        p.end.mu = mu; p.end.skip = ii;
        return p;
    }

    // largest tile whose input span fits the LDS image, and the span (LDS items) that tile needs at most
    int tile_for(const FracPlan &p, int *span) const
    {
        const long long cap = span_cap();
        if (p.closed) {
            // ii_(k+n) - ii_k <= (2^24 - 1 + n*F) >> 24, one more where the mu == 1 output leads
            const long long room = cap - FRAC_NTAPS - p.sc.first_one;
            const unsigned long long nmax = ((unsigned long long)room << 24) / p.sc.F;
            const int tile = (int)std::min<unsigned long long>(FRAC_TILE, 1 + nmax);
            *span = (int)((ONE24 - 1 + (unsigned long long)(tile - 1) * p.sc.F) >> 24) + FRAC_NTAPS + p.sc.first_one;
            return tile;
        }
        for (int tile = FRAC_TILE;; tile /= 2) {
            long long worst = 0;
            for (size_t k0 = 0; k0 < p.steps.size(); k0 += tile) {
                const size_t kl = std::min(p.steps.size(), k0 + tile) - 1;
                worst = std::max(worst, (long long)(p.steps[kl] >> 8) - (long long)(p.steps[k0] >> 8) + FRAC_NTAPS);
            }
            if (worst <= cap || tile == 1) { *span = (int)std::min(worst, cap); return tile; }
        }
    }

    int launch(FracPlan &p, const void *d_in, long long in_stride, long long n_phys, void *d_out, long long out_stride,
               int n_streams, hipStream_t stream)
    {
        if (p.n <= 0) return GRHIP_OK;
        FracLaunch a;
        a.in = d_in; a.in_stride = in_stride; a.n_phys = n_phys;
        a.out = d_out; a.out_stride = out_stride; a.nout = p.n; a.n_streams = n_streams;
        a.taps = tabs->mmse_rev;
        a.tile = tile_for(p, &a.span_cap);
        a.sc = p.sc;
        if (p.closed) return frac_interp_launch(cplx, !mode_fast(p.mode), a, stream);
        // the walked schedule: d_steps and its host source are rewritten, so the handle's last launch that read them
        // (on whatever stream) must be done -- that launch only, nothing else on the device
        if (!steps_ev) GRHIP_HIP(hipEventCreateWithFlags(&steps_ev, hipEventDisableTiming));
        if (steps_busy) { GRHIP_HIP(hipEventSynchronize(steps_ev)); steps_busy = false; }
        h_steps.swap(p.steps);
        const size_t bytes = h_steps.size() * sizeof(unsigned long long);
        int rc = d_steps.reserve(bytes);
        if (rc) return rc;
        GRHIP_HIP(hipMemcpyAsync(d_steps.p, h_steps.data(), bytes, hipMemcpyHostToDevice, stream));
        a.sc.steps = d_steps.as<unsigned long long>();
        rc = frac_interp_launch(cplx, !mode_fast(p.mode), a, stream);
        GRHIP_HIP(hipEventRecord(steps_ev, stream));       // after the copy, whether or not the kernel was launched
        steps_busy = true;
        return rc;
    }

    int init(float phase_shift, float interp_ratio, int dev)
    {
        int rc = check_ratio(interp_ratio);                 // .cc:44-47, in the reference's order
        if (rc) return rc;
        if ((rc = check_mu(phase_shift))) return rc;
        phase0 = phase_shift; st.mu = phase_shift; mu_inc = interp_ratio;
        if ((rc = init_device(dev))) return rc;
        mode = default_mode();
        return get_device_tables(device, &tabs);
    }

    int general_work_device(int noutput_items, int ninput_items, const void *d_in, void *d_out, int *consumed,
                            void *stream)
    {
        if (!consumed) return fail(GRHIP_EINVAL, "null consumed");
        *consumed = 0;
        if (noutput_items < 0 || ninput_items < 0) return fail(GRHIP_EINVAL, "negative item count");
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        FracPlan p = plan(st, ninput_items, noutput_items);
        if (p.too_many) return fail(GRHIP_EINVAL, "fractional_interpolator: too many outputs for one call");
        if (p.n > 0 && (!d_in || !d_out)) return fail(GRHIP_EINVAL, "null buffer");
        if ((rc = launch(p, d_in, 0, ninput_items, d_out, 0, 1, pick(stream)))) return rc;
        const long long c = std::min<long long>(p.end.skip, ninput_items);
        st.mu = p.end.mu;
        st.skip = p.end.skip - c;
        *consumed = (int)c;
        return (int)p.n;
    }

    int general_work(int noutput_items, int ninput_items, const void *in, void *out, int *consumed)
    {
        if (!consumed) return fail(GRHIP_EINVAL, "null consumed");
        *consumed = 0;
        if (noutput_items < 0 || ninput_items < 0) return fail(GRHIP_EINVAL, "negative item count");
        if ((!in && ninput_items) || (!out && noutput_items)) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        return (int)host_call(in, (size_t)ninput_items * item(), (size_t)ninput_items * item() + 16,
                              (size_t)noutput_items * item() + 16, out, item(), [&](void *d_in, void *d_out, hipStream_t s) {
                                  return general_work_device(noutput_items, ninput_items, d_in, d_out, consumed, s);
                              });
    }

    // n_streams captures from the constructor's phase_shift: the outputs with ii_k + 8 <= n_samples
    int run_captures_device(int n_streams, size_t n_samples, const void *d_in, size_t in_stride, void *d_out,
                            size_t out_stride, size_t *n_out, void *stream)
    {
        if (!n_out) return fail(GRHIP_EINVAL, "null n_out");
        if (n_streams < 0) return fail(GRHIP_EINVAL, "negative n_streams");
        if (n_samples > (size_t)1 << 38) return fail(GRHIP_EINVAL, "n_samples too large");
        int rc = bind();
        if (rc) return rc;
        FracState fresh;
        fresh.mu = phase0;
        std::lock_guard<std::mutex> lk(setter_mutex);               // plan and launch under one lock
        FracPlan p = plan(fresh, (long long)n_samples, std::numeric_limits<long long>::max() / 4);
        if (p.too_many) return fail(GRHIP_EINVAL, "fractional_interpolator: too many outputs per capture");
        *n_out = (size_t)p.n;
        if (!d_out || n_streams == 0 || p.n == 0) return GRHIP_OK;   // a query, or nothing to do
        if (!d_in) return fail(GRHIP_EINVAL, "null buffer");
        if (n_streams > 1 && (in_stride < n_samples || out_stride < (size_t)p.n))
            return fail(GRHIP_EINVAL, "fractional_interpolator: strides shorter than n_samples / n_out");
        return launch(p, d_in, (long long)in_stride, (long long)n_samples, d_out, (long long)out_stride, n_streams,
                      pick(stream));
    }

    int set_mu(float m)
    {
        int rc = check_mu(m);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        st.mu = m;
        return GRHIP_OK;
    }

    int set_interp_ratio(float r)
    {
        int rc = check_ratio(r);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        mu_inc = r;
        return GRHIP_OK;
    }

    int set_mode(int m)
    {
        if (!mode_valid(m)) return fail(GRHIP_EINVAL, "bad mode %d", m);
        std::lock_guard<std::mutex> lk(setter_mutex);
        mode = m;
        return GRHIP_OK;
    }

    // .cc:63-64: (int) ceil((noutput_items * d_mu_inc) + d_interp->ntaps()) -- int * float, + unsigned, all in float
    int forecast(int noutput_items)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        float inc;
        {
            std::lock_guard<std::mutex> lk(setter_mutex);
            inc = mu_inc;
        }
        const float v = ((float)noutput_items * inc) + (float)(unsigned)FRAC_NTAPS;
        const double c = ceil((double)v);
        if (!(c < 2147483648.0)) return fail(GRHIP_EINVAL, "fractional_interpolator: forecast does not fit an int");
        return (int)c;
    }

    void destroy()
    {
        (void)bind();
        if (steps_ev) {
            if (steps_busy) (void)hipEventSynchronize(steps_ev);
            (void)hipEventDestroy(steps_ev);
            steps_ev = nullptr; steps_busy = false;
        }
        d_steps.release();
        destroy_base();
    }
};

struct grhip_fractional_interpolator_ff : grhip_fractional_interpolator_base {};
struct grhip_fractional_interpolator_cc : grhip_fractional_interpolator_base {};

namespace {

template <class H>
int create_t(H **h, bool cplx, float phase_shift, float interp_ratio, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    auto *b = new (std::nothrow) H();
    if (!b) return fail(GRHIP_ENOMEM, "alloc");
    b->cplx = cplx;
    int rc = b->init(phase_shift, interp_ratio, device);
    if (rc) {
        if (b->own_stream) b->destroy();
        delete b;
        return rc;
    }
    *h = b;
    return GRHIP_OK;
}

}  // namespace

extern "C" {

#define GRHIP_FRAC_ENTRIES(SUF, CPLX)                                                                                  \
    int grhip_fractional_interpolator_##SUF##_create(grhip_fractional_interpolator_##SUF **h, float phase_shift,      \
                                                     float interp_ratio, int device)                                 \
    {                                                                                                                  \
        return create_t(h, CPLX, phase_shift, interp_ratio, device);                                                   \
    }                                                                                                                  \
    void grhip_fractional_interpolator_##SUF##_destroy(grhip_fractional_interpolator_##SUF *h)                         \
    {                                                                                                                  \
        if (!h) return;                                                                                                \
        h->destroy();                                                                                                  \
        delete h;                                                                                                      \
    }                                                                                                                  \
    int grhip_fractional_interpolator_##SUF##_set_mu(grhip_fractional_interpolator_##SUF *h, float mu)                \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->set_mu(mu);                                                                                          \
    }                                                                                                                  \
    int grhip_fractional_interpolator_##SUF##_set_interp_ratio(grhip_fractional_interpolator_##SUF *h,                \
                                                               float interp_ratio)                                   \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->set_interp_ratio(interp_ratio);                                                                      \
    }                                                                                                                  \
    float grhip_fractional_interpolator_##SUF##_mu(grhip_fractional_interpolator_##SUF *h)                            \
    {                                                                                                                  \
        if (!h) return 0.f;                                                                                            \
        std::lock_guard<std::mutex> lk(h->setter_mutex);                                                               \
        return h->st.mu;                                                                                               \
    }                                                                                                                  \
    float grhip_fractional_interpolator_##SUF##_interp_ratio(grhip_fractional_interpolator_##SUF *h)                  \
    {                                                                                                                  \
        if (!h) return 0.f;                                                                                            \
        std::lock_guard<std::mutex> lk(h->setter_mutex);                                                               \
        return h->mu_inc;                                                                                              \
    }                                                                                                                  \
    int grhip_fractional_interpolator_##SUF##_set_mode(grhip_fractional_interpolator_##SUF *h, int mode)              \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->set_mode(mode);                                                                                      \
    }                                                                                                                  \
    int grhip_fractional_interpolator_##SUF##_history(const grhip_fractional_interpolator_##SUF *h)                   \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return 1;                                                                                                      \
    }                                                                                                                  \
    int grhip_fractional_interpolator_##SUF##_forecast(grhip_fractional_interpolator_##SUF *h, int noutput_items)     \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->forecast(noutput_items);                                                                             \
    }                                                                                                                  \
    int grhip_fractional_interpolator_##SUF##_general_work(grhip_fractional_interpolator_##SUF *h, int noutput_items, \
                                                           int ninput_items, const void *in, void *out,              \
                                                           int *consumed)                                            \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->general_work(noutput_items, ninput_items, in, out, consumed);                                        \
    }                                                                                                                  \
    int grhip_fractional_interpolator_##SUF##_general_work_device(grhip_fractional_interpolator_##SUF *h,             \
                                                                  int noutput_items, int ninput_items,               \
                                                                  const void *d_in, void *d_out, int *consumed,      \
                                                                  void *stream)                                      \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->general_work_device(noutput_items, ninput_items, d_in, d_out, consumed, stream);                     \
    }                                                                                                                  \
    int grhip_fractional_interpolator_##SUF##_run_captures_device(grhip_fractional_interpolator_##SUF *h,             \
                                                                  int n_streams, size_t n_samples, const void *d_in, \
                                                                  size_t in_stride, void *d_out, size_t out_stride,  \
                                                                  size_t *n_out, void *stream)                       \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->run_captures_device(n_streams, n_samples, d_in, in_stride, d_out, out_stride, n_out, stream);        \
    }

GRHIP_FRAC_ENTRIES(ff, false)
GRHIP_FRAC_ENTRIES(cc, true)

#undef GRHIP_FRAC_ENTRIES

}  // extern "C"
