// capi_fracinterp.hip -- gr_fractional_interpolator_ff / _cc: handle and C ABI.
//
// Reference: gnuradio-core/src/lib/filter/gr_fractional_interpolator_ff.cc:38-50 (constructor), 57-65 (forecast),
// 67-93 (general_work); gr_fractional_interpolator_ff.h:51-54 (accessors); gri_mmse_fir_interpolator.cc:61-71.  The
// _cc files differ only in the item type.
//
// Where output k reads its input, (ii_k, imu_k), does not depend on the data; csrc/sched_plan.h works it out on the
// host, by a closed form when the float sums of the reference's walk (.cc:83-87) never round, else by walking them.
// The handle keeps the state and the lock.
#include <cmath>
#include <limits>
#include <vector>

#include "frac_interp.h"
#include "sched_block.h"

using namespace grhip;

struct grhip_fractional_interpolator_base : SchedBlock<grhip_fractional_interpolator_base> {
    float phase0 = 0.f;         // the constructor's phase_shift: the fresh state of run_captures_device
    float mu_inc = 1.f;         // d_mu_inc
    FracState st;
    const DeviceTables *tabs = nullptr;
    WalkedSteps<unsigned long long> walked;

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

    FracPlan plan(const FracState &s, long long ninput, long long nout) const
    {
        FracPlan p = frac_plan(s, mu_inc, ninput, nout);
        p.mode = mode;
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
            *span = (int)((FRAC_ONE - 1 + (unsigned long long)(tile - 1) * p.sc.F) >> 24) + FRAC_NTAPS + p.sc.first_one;
            return tile;
        }
        return walked_tile(p.steps.size(), FRAC_TILE, FRAC_NTAPS, cap,
                           [&](size_t k) { return (long long)(p.steps[k] >> 8); }, span);
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
        int rc = walked.upload(p.steps, stream, &a.sc.steps);
        if (rc) return rc;
        rc = frac_interp_launch(cplx, !mode_fast(p.mode), a, stream);
        const int rc_ev = walked.mark_read(stream);
        return rc_ev ? rc_ev : rc;
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
        st = frac_carry(p.end, ninput_items, consumed);
        return (int)p.n;
    }

    // n_streams captures from the constructor's phase_shift: the outputs with ii_k + 8 <= n_samples
    int run_captures_device(int n_streams, size_t n_samples, const void *d_in, size_t in_stride, void *d_out,
                            size_t out_stride, size_t *n_out, void *stream)
    {
        return run_captures(
            "fractional_interpolator", (size_t)1 << 38, n_streams, n_samples, d_in, in_stride, d_out, out_stride, n_out,
            [&] { return plan(FracState{phase0, 0}, (long long)n_samples, std::numeric_limits<long long>::max() / 4); },
            [&](FracPlan &p) {
                return launch(p, d_in, (long long)in_stride, (long long)n_samples, d_out, (long long)out_stride, n_streams,
                              pick(stream));
            });
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
};

struct grhip_fractional_interpolator_ff : grhip_fractional_interpolator_base {};
struct grhip_fractional_interpolator_cc : grhip_fractional_interpolator_base {};

extern "C" {

#define GRHIP_FRAC_ENTRIES(SUF, CPLX)                                                                                  \
    int grhip_fractional_interpolator_##SUF##_create(grhip_fractional_interpolator_##SUF **h, float phase_shift,      \
                                                     float interp_ratio, int device)                                 \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null argument");                                                            \
        return make_handle(h, [&](grhip_fractional_interpolator_##SUF *b) {                                            \
            b->cplx = CPLX;                                                                                            \
            return b->init(phase_shift, interp_ratio, device);                                                         \
        });                                                                                                            \
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
    GRHIP_SCHED_ENTRIES(fractional_interpolator_##SUF)

GRHIP_FRAC_ENTRIES(ff, false)
GRHIP_FRAC_ENTRIES(cc, true)

#undef GRHIP_FRAC_ENTRIES

}  // extern "C"
