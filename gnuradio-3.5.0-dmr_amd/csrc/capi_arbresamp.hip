// capi_arbresamp.hip -- gr_pfb_arb_resampler_ccf / _fff: handle and C ABI.
//
// Reference: gnuradio-core/src/lib/filter/gr_pfb_arb_resampler_ccf.cc:42-83 (constructor), 93-124 (create_taps),
// 126-139 (create_diff_taps), 158-209 (general_work); gr_pfb_arb_resampler_ccf.h:166-170 (set_rate).  The _fff
// files differ only in the item type.
//
// The schedule (count_k, j_k, acc_k) of the outputs does not depend on the data; csrc/sched_plan.h works it out on the
// host, by a closed form or by walking the reference's float32 arithmetic.  The handle keeps the state and the lock.
#include <cmath>
#include <limits>
#include <vector>

#include "arb_resampler.h"
#include "sched_block.h"

using namespace grhip;

struct grhip_pfb_arb_resampler_base : SchedBlock<grhip_pfb_arb_resampler_base> {
    unsigned tpf = 0, S = 0;
    float rate = 1.f;
    ArbRate rp;                 // filter_size, d_dec_rate, d_flt_rate
    ArbState st;
    bool updated = true;        // create_taps sets d_updated (.cc:121)
    DevBuf d_taps;
    WalkedSteps<ArbStep> walked;

    int span_cap() const { return ARB_SPAN_BYTES / (int)item(); }

    ArbPlan plan(const ArbState &s, long long max_input, long long nout) const
    {
        ArbPlan p = arb_plan(s, rp, max_input, nout);
        p.mode = mode;
        return p;
    }

    // largest tile whose input span fits the LDS image, and the span (LDS items) that tile needs at most: LDS is
    // sized to it, not to the cap, so short spans leave room for more workgroups per CU
    int tile_for(const ArbPlan &p, int *span) const
    {
        const long long cap = span_cap();
        if (p.closed) return arb_closed_tile(rp.R, p.D, tpf, cap, ARB_MAX_TILE, span);
        return walked_tile(p.steps.size(), ARB_MAX_TILE, tpf, cap, [&](size_t k) { return p.steps[k].count; }, span);
    }

    // launches the outputs of plan p; sc.steps is filled in here
    int launch(ArbPlan &p, const void *d_in, long long in_stride, long long lead, long long n_phys, void *d_out,
               long long out_stride, int n_streams, hipStream_t stream)
    {
        if (p.n <= 0) return GRHIP_OK;
        ArbLaunch a;
        a.in = d_in; a.in_stride = in_stride; a.lead = lead; a.n_phys = n_phys;
        a.out = d_out; a.out_stride = out_stride; a.nout = p.n; a.n_streams = n_streams;
        a.taps = d_taps.as<float2>(); a.R = (int)rp.R; a.tpf = (int)tpf; a.S = (int)S;
        a.tile = tile_for(p, &a.span_cap);
        a.sc = p.sc;
        if (p.closed) return arb_resampler_launch(cplx, !mode_fast(p.mode), a, stream);
        int rc = walked.upload(p.steps, stream, &a.sc.steps);
        if (rc) return rc;
        rc = arb_resampler_launch(cplx, !mode_fast(p.mode), a, stream);
        const int rc_ev = walked.mark_read(stream);
        return rc_ev ? rc_ev : rc;
    }

    int init(float r, const float *taps, size_t ntaps, unsigned filter_size, int device)
    {
        if (filter_size == 0) return fail(GRHIP_EINVAL, "pfb_arb_resampler: filter_size must be > 0 (.cc:100 divides by it)");
        if (ntaps < 2)
            return fail(GRHIP_EINVAL, "pfb_arb_resampler: at least 2 taps (create_diff_taps, .cc:130-138, underflows "
                                      "size()-1 for none and repeats an unset difference for one)");
        const unsigned R = filter_size;
        const unsigned long long t = (ntaps + R - 1) / R;               // ceil(ntaps / R), .cc:100
        const unsigned long long s = t | 1ull;
        if ((unsigned long long)R * s > (unsigned long long)ARB_MAX_TAP_PAIRS)
            return fail(GRHIP_EINVAL, "pfb_arb_resampler: filter_size * (taps_per_filter | 1) must be <= %d", ARB_MAX_TAP_PAIRS);
        tpf = (unsigned)t; S = (unsigned)s;
        if (const char *bad = arb_rate_params(R, r, &rp)) return fail(GRHIP_EINVAL, "%s", bad);
        rate = r;
        int rc = init_device(device);
        if (rc) return rc;
        mode = default_mode();
        const std::vector<float> pairs = arb_tap_pairs(taps, ntaps, R, tpf, S);        // sched_plan.h
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
        st = arb_carry(p.end, ninput_items, consumed);
        return (int)p.n;
    }

    // n_streams fresh-state captures: tpf history zeros in front of each (the scheduler's, .cc:123), outputs while
    // count_k < n_samples
    int run_captures_device(int n_streams, size_t n_samples, const void *d_in, size_t in_stride, void *d_out,
                            size_t out_stride, size_t *n_out, void *stream)
    {
        return run_captures(
            "pfb_arb_resampler", (size_t)std::numeric_limits<long long>::max() / 2, n_streams, n_samples, d_in, in_stride,
            d_out, out_stride, n_out,
            [&] { return plan(ArbState(), (long long)n_samples, std::numeric_limits<long long>::max() / 4); },
            [&](ArbPlan &p) {
                return launch(p, d_in, (long long)in_stride, tpf, (long long)n_samples, d_out, (long long)out_stride,
                              n_streams, pick(stream));
            });
    }

    int set_rate(float r)
    {
        ArbRate n;
        if (const char *bad = arb_rate_params(rp.R, r, &n)) return fail(GRHIP_EINVAL, "%s", bad);
        std::lock_guard<std::mutex> lk(setter_mutex);
        rp = n; rate = r;
        return GRHIP_OK;
    }
};

struct grhip_pfb_arb_resampler_ccf : grhip_pfb_arb_resampler_base {};
struct grhip_pfb_arb_resampler_fff : grhip_pfb_arb_resampler_base {};

extern "C" {

#define GRHIP_ARB_ENTRIES(SUF, CPLX)                                                                                   \
    int grhip_pfb_arb_resampler_##SUF##_create(grhip_pfb_arb_resampler_##SUF **h, float rate, const float *taps,      \
                                               size_t ntaps, unsigned filter_size, int device)                       \
    {                                                                                                                  \
        if (!h || (!taps && ntaps)) return fail(GRHIP_EINVAL, "null argument");                                        \
        return make_handle(h, [&](grhip_pfb_arb_resampler_##SUF *b) {                                                  \
            b->cplx = CPLX;                                                                                            \
            return b->init(rate, taps, ntaps, filter_size, device);                                                    \
        });                                                                                                            \
    }                                                                                                                  \
    int grhip_pfb_arb_resampler_##SUF##_set_rate(grhip_pfb_arb_resampler_##SUF *h, float rate)                        \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->set_rate(rate);                                                                                      \
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
    GRHIP_SCHED_ENTRIES(pfb_arb_resampler_##SUF)

GRHIP_ARB_ENTRIES(ccf, true)
GRHIP_ARB_ENTRIES(fff, false)

#undef GRHIP_ARB_ENTRIES

}  // extern "C"
