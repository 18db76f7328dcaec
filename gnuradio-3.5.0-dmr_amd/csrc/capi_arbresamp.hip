// capi_arbresamp.hip -- gr_pfb_arb_resampler_ccf / _fff: handle, index schedule and C ABI.
//
// Reference: gnuradio-core/src/lib/filter/gr_pfb_arb_resampler_ccf.cc:42-83 (constructor), 93-124 (create_taps),
// 126-139 (create_diff_taps), 158-209 (general_work); gr_pfb_arb_resampler_ccf.h:166-170 (set_rate).  The _fff
// files differ only in the item type.
//
// The schedule (count_k, j_k, acc_k) of the outputs does not depend on the data.  When acc and the fractional rate
// f are multiples of 2^-23 (always, from fresh state, when rate <= filter_size: then R/rate >= 1 and f is a float
// below 1 with an exponent >= -23), every acc + f of the reference is exact and its walk equals the closed form of
// ArbSched (arb_resampler.h); produced and consumed follow on the host from a binary search.  Otherwise
// (rate > filter_size: the sums round) the host walks the reference's float32 arithmetic and hands the kernel one
// ArbStep per output.
#include <cmath>
#include <limits>
#include <vector>

#include "arb_resampler.h"
#include "grhip_internal.h"

using namespace grhip;

namespace {

// the reference's state between general_work calls
struct ArbState {
    long long count = 0;        // d_start_index (at entry) / count (at exit)
    unsigned j = 0;             // d_last_filter (may be >= R: the last call ended before wrapping it)
    float acc = 0.f;            // d_acc
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
    int mode = GRHIP_MODE_FAST; // not the handle's current values
};

constexpr long long ARB_MAX_OUT = 1LL << 40;          // closed form: k * F stays below 2^64
constexpr long long ARB_MAX_STEPS = 1LL << 28;        // walked schedule: 4 GB of steps

bool on_grid(float v, unsigned long long *q)
{
    const float s = v * 8388608.0f;                   // exact: a power-of-two scaling
    if (!(s >= 0.f) || s >= 8388608.0f || s != floorf(s)) return false;
    *q = (unsigned long long)s;
    return true;
}

}  // namespace

struct grhip_pfb_arb_resampler_base : HandleBase {
    bool cplx = true;
    unsigned R = 0, tpf = 0, S = 0;
    float rate = 1.f;
    unsigned dec_rate = 0;      // d_dec_rate
    float flt_rate = 0.f;       // d_flt_rate
    ArbState st;
    bool updated = true;        // create_taps sets d_updated (.cc:121)
    int mode = GRHIP_MODE_FAST;
    DevBuf d_taps, d_steps;
    std::vector<ArbStep> h_steps;   // source of the last upload to d_steps, kept until steps_ev has passed
    hipEvent_t steps_ev = nullptr;  // recorded after the last launch that read d_steps
    bool steps_busy = false;

    size_t item() const { return cplx ? 8 : 4; }
    int span_cap() const { return ARB_SPAN_BYTES / (int)item(); }

    // set_rate (.h:166-170): the float arithmetic of the reference
    static int rate_params(unsigned R, float rate, unsigned *D, float *f)
    {
        if (!(rate > 0.f) || !std::isfinite(rate))
            return fail(GRHIP_EINVAL, "pfb_arb_resampler: rate must be finite and > 0");
        const float x = (float)R / rate;
        const float fl = floorf(x);
        if (!(fl + 1.f <= (float)ARB_MAX_DEC))
            return fail(GRHIP_EINVAL, "pfb_arb_resampler: filter_size / rate must be below 2^20");
        *D = (unsigned)fl;
        *f = x - (float)*D;
        return GRHIP_OK;
    }

    // count_k, pos_k of the closed form from state s (A0 = acc * 2^23)
    static long long cf_pos(const ArbState &s, unsigned long long A0, unsigned F, unsigned D, long long k)
    {
        const unsigned long long T = A0 + (unsigned long long)k * F;
        return (long long)((unsigned long long)s.j + (unsigned long long)k * D + (T >> 23));
    }

    ArbPlan plan(const ArbState &s, long long max_input, long long nout) const
    {
        ArbPlan p;
        p.end = s;
        const unsigned D = dec_rate;
        p.D = D;
        p.mode = mode;
        unsigned long long Fq = 0, A0 = 0;
        p.closed = on_grid(flt_rate, &Fq) && on_grid(s.acc, &A0);
        if (nout <= 0 || s.count >= max_input) return p;          // the outer loop never runs (.cc:175)
        if (p.closed) {
            const unsigned F = (unsigned)Fq;
            auto count_of = [&](long long k) { return s.count + cf_pos(s, A0, F, D, k) / (long long)R; };
            // n = the first k with count_k >= max_input, at most nout (count_k does not decrease)
            long long hi = 1;
            while (hi < nout && hi < ARB_MAX_OUT && count_of(hi) < max_input) hi *= 2;
            if (hi >= ARB_MAX_OUT && hi < nout) { p.too_many = true; return p; }
            long long lo = 0;
            hi = std::min(hi, nout);
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (count_of(mid) >= max_input) hi = mid; else lo = mid + 1;
            }
            p.n = lo;
            const long long posn = cf_pos(s, A0, F, D, p.n);
            if (p.n == nout) {          // stopped by noutput_items: j not wrapped (.cc:194)
                const long long prev = cf_pos(s, A0, F, D, p.n - 1) / (long long)R;
                p.end.count = s.count + prev;
                p.end.j = (unsigned)(posn - prev * (long long)R);
            } else {                    // stopped by the input: the wrap that ran past it has happened
                p.end.count = s.count + posn / (long long)R;
                p.end.j = (unsigned)(posn % (long long)R);
            }
            p.end.acc = (float)((A0 + (unsigned long long)p.n * F) & 0x7fffffull) * (1.0f / 8388608.0f);
            p.sc.c0 = s.count; p.sc.j0 = s.j; p.sc.A0 = A0; p.sc.F = F; p.sc.D = D;
            return p;
        }
        // the reference's loop in float32 (.cc:172-201), positions kept exact in 64 bits
        long long count = s.count, i = 0;
        unsigned j = s.j;
        float acc = s.acc;
        while (i < nout && count < max_input) {
            while (j < R && i < nout) {
                if (i >= ARB_MAX_STEPS) { p.too_many = true; return p; }
                p.steps.push_back(ArbStep{count, (int)j, acc});
                ++i;
                acc += flt_rate;
                j += D + (int)floorf(acc);
                acc = fmodf(acc, 1.0f);
            }
            if (i < nout) {
                count += j / R;
                j = j % R;
            }
        }
        p.n = i;
        p.end.count = count; p.end.j = j; p.end.acc = acc;
        return p;
    }

    // largest tile whose input span fits the LDS image, and the span (LDS items) that tile needs at most: LDS is
    // sized to it, not to the cap, so short spans leave room for more workgroups per CU
    int tile_for(const ArbPlan &p, int *span) const
    {
        const long long cap = span_cap();
        if (p.closed) {
            // pos_k - pos_0 <= k*(D+1) and pos_0 % R < R: count_k - count_0 <= (R-1 + k*(D+1)) / R
            const long long t = 1 + (cap - (long long)tpf) * (long long)R / ((long long)p.D + 1);
            const int tile = (int)std::min<long long>(ARB_MAX_TILE, std::max<long long>(1, t));
            *span = (int)(((long long)R - 1 + (long long)(tile - 1) * ((long long)p.D + 1)) / R + tpf);
            return tile;
        }
        for (int tile = ARB_MAX_TILE;; tile /= 2) {
            long long worst = 0;
            for (size_t k0 = 0; k0 < p.steps.size(); k0 += tile) {
                const size_t kl = std::min(p.steps.size(), k0 + tile) - 1;
                worst = std::max(worst, p.steps[kl].count - p.steps[k0].count + (long long)tpf);
            }
            if (worst <= cap || tile == 1) { *span = (int)std::min(worst, cap); return tile; }
        }
    }

    // launches the outputs of plan p; sc.steps is filled in here
    int launch(ArbPlan &p, const void *d_in, long long in_stride, long long lead, long long n_phys, void *d_out,
               long long out_stride, int n_streams, hipStream_t stream)
    {
        if (p.n <= 0) return GRHIP_OK;
        ArbLaunch a;
        a.in = d_in; a.in_stride = in_stride; a.lead = lead; a.n_phys = n_phys;
        a.out = d_out; a.out_stride = out_stride; a.nout = p.n; a.n_streams = n_streams;
        a.taps = d_taps.as<float2>(); a.R = (int)R; a.tpf = (int)tpf; a.S = (int)S;
        a.tile = tile_for(p, &a.span_cap);
        a.sc = p.sc;
        if (p.closed) return arb_resampler_launch(cplx, !mode_fast(p.mode), a, stream);
        // the walked schedule: d_steps and its host source are rewritten, so the handle's last launch that read them
        // (on whatever stream) must be done -- that launch only, nothing else on the device
        if (!steps_ev) GRHIP_HIP(hipEventCreateWithFlags(&steps_ev, hipEventDisableTiming));
        if (steps_busy) { GRHIP_HIP(hipEventSynchronize(steps_ev)); steps_busy = false; }
        h_steps.swap(p.steps);
        const size_t bytes = h_steps.size() * sizeof(ArbStep);
        int rc = d_steps.reserve(bytes);
        if (rc) return rc;
        GRHIP_HIP(hipMemcpyAsync(d_steps.p, h_steps.data(), bytes, hipMemcpyHostToDevice, stream));
        a.sc.steps = d_steps.as<ArbStep>();
        rc = arb_resampler_launch(cplx, !mode_fast(p.mode), a, stream);
        GRHIP_HIP(hipEventRecord(steps_ev, stream));       // after the copy, whether or not the kernel was launched
        steps_busy = true;
        return rc;
    }

    int init(float r, const float *taps, size_t ntaps, unsigned filter_size, int device)
    {
        if (filter_size == 0) return fail(GRHIP_EINVAL, "pfb_arb_resampler: filter_size must be > 0 (.cc:100 divides by it)");
        if (ntaps < 2)
            return fail(GRHIP_EINVAL, "pfb_arb_resampler: at least 2 taps (create_diff_taps, .cc:130-138, underflows "
                                      "size()-1 for none and repeats an unset difference for one)");
        R = filter_size;
        const unsigned long long t = (ntaps + R - 1) / R;               // ceil(ntaps / R), .cc:100
        const unsigned long long s = t | 1ull;
        if ((unsigned long long)R * s > (unsigned long long)ARB_MAX_TAP_PAIRS)
            return fail(GRHIP_EINVAL, "pfb_arb_resampler: filter_size * (taps_per_filter | 1) must be <= %d", ARB_MAX_TAP_PAIRS);
        tpf = (unsigned)t; S = (unsigned)s;
        int rc = rate_params(R, r, &dec_rate, &flt_rate);
        if (rc) return rc;
        rate = r;
        if ((rc = init_device(device))) return rc;
        mode = default_mode();
        // create_diff_taps (.cc:130-138), then create_taps (.cc:93-124) for both banks: filter i gets
        // proto[i + t*R], zero padded to R*tpf, reversed by gr_fir_XXX::set_taps
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
        if ((rc = d_taps.reserve(pairs.size() * 4))) return rc;
        GRHIP_HIP(hipMemcpy(d_taps.p, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));
        return GRHIP_OK;
    }

    // general_work (.cc:158-209) on device buffers; the kernel is enqueued, produced / consumed are known now
    int general_work_device(int noutput_items, int ninput_items, const void *d_in, void *d_out, int *consumed,
                            void *stream)
    {
        if (!consumed) return fail(GRHIP_EINVAL, "null consumed");
        *consumed = 0;
        if (noutput_items < 0 || ninput_items < 0) return fail(GRHIP_EINVAL, "negative item count");
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if (updated) { updated = false; return 0; }                         // .cc:166-169
        ArbPlan p = plan(st, (long long)ninput_items - (long long)tpf, noutput_items);
        if (p.too_many) return fail(GRHIP_EINVAL, "pfb_arb_resampler: too many outputs for one call");
        if (p.n > 0 && (!d_in || !d_out)) return fail(GRHIP_EINVAL, "null buffer");
        if ((rc = launch(p, d_in, 0, 0, ninput_items, d_out, 0, 1, pick(stream)))) return rc;
        st.j = p.end.j; st.acc = p.end.acc;
        st.count = std::max(0LL, p.end.count - (long long)ninput_items);   // .cc:204
        *consumed = (int)std::min<long long>(p.end.count, ninput_items);   // .cc:207
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

    // n_streams fresh-state captures: tpf history zeros in front of each (the scheduler's, .cc:123), outputs while
    // count_k < n_samples
    int run_captures_device(int n_streams, size_t n_samples, const void *d_in, size_t in_stride, void *d_out,
                            size_t out_stride, size_t *n_out, void *stream)
    {
        if (!n_out) return fail(GRHIP_EINVAL, "null n_out");
        if (n_streams < 0) return fail(GRHIP_EINVAL, "negative n_streams");
        if (n_samples > (size_t)std::numeric_limits<long long>::max() / 2) return fail(GRHIP_EINVAL, "n_samples too large");
        int rc = bind();
        if (rc) return rc;
        ArbState fresh;
        std::lock_guard<std::mutex> lk(setter_mutex);               // plan and launch under one lock
        ArbPlan p = plan(fresh, (long long)n_samples, std::numeric_limits<long long>::max() / 4);
        if (p.too_many) return fail(GRHIP_EINVAL, "pfb_arb_resampler: too many outputs per capture");
        *n_out = (size_t)p.n;
        if (!d_out || n_streams == 0 || p.n == 0) return GRHIP_OK;   // a query, or nothing to do
        if (!d_in) return fail(GRHIP_EINVAL, "null buffer");
        if (n_streams > 1 && (in_stride < n_samples || out_stride < (size_t)p.n))
            return fail(GRHIP_EINVAL, "pfb_arb_resampler: strides shorter than n_samples / n_out");
        return launch(p, d_in, (long long)in_stride, tpf, (long long)n_samples, d_out, (long long)out_stride, n_streams,
                      pick(stream));
    }

    int set_rate(float r)
    {
        unsigned D;
        float f;
        int rc = rate_params(R, r, &D, &f);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        dec_rate = D; flt_rate = f; rate = r;
        return GRHIP_OK;
    }

    int set_mode(int m)
    {
        if (!mode_valid(m)) return fail(GRHIP_EINVAL, "bad mode %d", m);
        std::lock_guard<std::mutex> lk(setter_mutex);
        mode = m;
        return GRHIP_OK;
    }

    void destroy()
    {
        (void)bind();
        if (steps_ev) {
            if (steps_busy) (void)hipEventSynchronize(steps_ev);
            (void)hipEventDestroy(steps_ev);
            steps_ev = nullptr; steps_busy = false;
        }
        d_taps.release(); d_steps.release();
        destroy_base();
    }
};

struct grhip_pfb_arb_resampler_ccf : grhip_pfb_arb_resampler_base {};
struct grhip_pfb_arb_resampler_fff : grhip_pfb_arb_resampler_base {};

namespace {

template <class H>
int create_t(H **h, bool cplx, float rate, const float *taps, size_t ntaps, unsigned filter_size, int device)
{
    if (!h || (!taps && ntaps)) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    auto *b = new (std::nothrow) H();
    if (!b) return fail(GRHIP_ENOMEM, "alloc");
    b->cplx = cplx;
    int rc = b->init(rate, taps, ntaps, filter_size, device);
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

#define GRHIP_ARB_ENTRIES(SUF, CPLX)                                                                                   \
    int grhip_pfb_arb_resampler_##SUF##_create(grhip_pfb_arb_resampler_##SUF **h, float rate, const float *taps,      \
                                               size_t ntaps, unsigned filter_size, int device)                       \
    {                                                                                                                  \
        return create_t(h, CPLX, rate, taps, ntaps, filter_size, device);                                              \
    }                                                                                                                  \
    void grhip_pfb_arb_resampler_##SUF##_destroy(grhip_pfb_arb_resampler_##SUF *h)                                     \
    {                                                                                                                  \
        if (!h) return;                                                                                                \
        h->destroy();                                                                                                  \
        delete h;                                                                                                      \
    }                                                                                                                  \
    int grhip_pfb_arb_resampler_##SUF##_set_rate(grhip_pfb_arb_resampler_##SUF *h, float rate)                        \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->set_rate(rate);                                                                                      \
    }                                                                                                                  \
    int grhip_pfb_arb_resampler_##SUF##_set_mode(grhip_pfb_arb_resampler_##SUF *h, int mode)                          \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->set_mode(mode);                                                                                      \
    }                                                                                                                  \
    int grhip_pfb_arb_resampler_##SUF##_history(const grhip_pfb_arb_resampler_##SUF *h)                               \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return (int)h->tpf + 1;                                                                                        \
    }                                                                                                                  \
    int grhip_pfb_arb_resampler_##SUF##_taps_per_filter(const grhip_pfb_arb_resampler_##SUF *h)                       \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return (int)h->tpf;                                                                                            \
    }                                                                                                                  \
    int grhip_pfb_arb_resampler_##SUF##_forecast(const grhip_pfb_arb_resampler_##SUF *h, int noutput_items)           \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");                                    \
        return noutput_items + (int)h->tpf;                                                                            \
    }                                                                                                                  \
    int grhip_pfb_arb_resampler_##SUF##_general_work(grhip_pfb_arb_resampler_##SUF *h, int noutput_items,             \
                                                     int ninput_items, const void *in, void *out, int *consumed)      \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->general_work(noutput_items, ninput_items, in, out, consumed);                                        \
    }                                                                                                                  \
    int grhip_pfb_arb_resampler_##SUF##_general_work_device(grhip_pfb_arb_resampler_##SUF *h, int noutput_items,      \
                                                            int ninput_items, const void *d_in, void *d_out,          \
                                                            int *consumed, void *stream)                             \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->general_work_device(noutput_items, ninput_items, d_in, d_out, consumed, stream);                     \
    }                                                                                                                  \
    int grhip_pfb_arb_resampler_##SUF##_run_captures_device(grhip_pfb_arb_resampler_##SUF *h, int n_streams,          \
                                                            size_t n_samples, const void *d_in, size_t in_stride,     \
                                                            void *d_out, size_t out_stride, size_t *n_out,           \
                                                            void *stream)                                            \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->run_captures_device(n_streams, n_samples, d_in, in_stride, d_out, out_stride, n_out, stream);        \
    }

GRHIP_ARB_ENTRIES(ccf, true)
GRHIP_ARB_ENTRIES(fff, false)

#undef GRHIP_ARB_ENTRIES

}  // extern "C"
