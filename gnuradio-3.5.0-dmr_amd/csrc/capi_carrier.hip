// capi_carrier.hip -- C ABI of digital_costas_loop_cc, gr_pll_freqdet_cf, gr_pll_refout_cc and gr_pll_carriertracking_cc.
//
// Reference: general/gri_control_loop.{h,cc} (the parameters, their setters and getters), general/gr_pll_freqdet_cf.cc,
// gr_pll_refout_cc.cc, gr_pll_carriertracking_cc.cc and gr-digital/lib/digital_costas_loop_cc.cc (work).
//
// A handle takes S streams back to back ([S][n_in]).  What a stream remembers is its phase, its frequency and, for
// carrier tracking, its lock signal: one CarrierState on the device.  The loop gains and limits are kernel arguments: a
// setter holds from the next work call, launches already queued keep theirs.
#include <cmath>
#include <vector>

#include "carrier.h"
#include "control_loop.h"
#include "grhip_internal.h"
#include "loop_block.h"

using namespace grhip;

namespace {

enum { CARRIER_COSTAS = -1 };       // otherwise a PLL_* kind

struct CarrierBlock : LoopBlock {
    int kind = PLL_FREQDET;
    int order = 2;
    float lock_threshold = 0.f;         // gr_pll_carriertracking_cc.cc:50
    int squelch = 0;
    const DeviceTables *tabs = nullptr;

    size_t out_item() const { return kind == PLL_FREQDET ? sizeof(float) : 2 * sizeof(float); }

    int restart() { return zero_loop_state(); }

    int init(int which, int ord, float loop_bw, float max_freq, float min_freq, int dev)
    {
        kind = which; order = ord;
        if (which == CARRIER_COSTAS && ord != 2 && ord != 4 && ord != 8)
            return fail(GRHIP_EINVAL, "costas_loop_cc: order must be 2, 4, or 8");          // digital_costas_loop_cc.cc:63-65
        if (!ControlLoop::limits_ok(max_freq, min_freq))
            return fail(GRHIP_EINVAL, "control loop: max_freq and min_freq must be finite and within +-%g rad/sample", (double)CL_FREQ_CAP);
        if (!cl.init(loop_bw, max_freq, min_freq))
            return fail(GRHIP_EINVAL, "gri_control_loop: invalid bandwidth. Must be >= 0 (and leave finite gains).");
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        if (which != CARRIER_COSTAS && (rc = get_device_tables(dev, &tabs))) return rc;
        return restart();
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
    }

    int lock_detector(int s, int *locked)   // gr_pll_carriertracking_cc.cc:74-78
    {
        if (!locked) return fail(GRHIP_EINVAL, "null argument");
        CarrierState t;
        int rc = read_state(d_state, s, &t);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        *locked = fabsf(t.locksig) > lock_threshold ? 1 : 0;
        return GRHIP_OK;
    }

    int squelch_enable(int on)              // gr_pll_carriertracking_cc.cc:80-84
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        squelch = on ? 1 : 0;
        return GRHIP_OK;
    }

    int set_lock_threshold(float thr)       // :86-90
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        lock_threshold = thr;
        return GRHIP_OK;
    }

    int work_device(int n_in, const void *d_in, void *d_out, void *d_freq, void *stream)
    {
        const int c = check_count(n_in);
        if (c <= 0) return c;
        int rc = check_io(d_in, 8, d_out, out_item());
        if (rc) return rc;
        if (!aligned(d_freq, 4)) return fail(GRHIP_EINVAL, "items not naturally aligned");
        const size_t items = (size_t)nstreams * (size_t)n_in;
        const size_t in_bytes = items * 8, out_bytes = items * out_item(), f_bytes = items * 4;
        if ((rc = check_apart("carrier loop", d_in, in_bytes, d_out, out_bytes))) return rc;
        if (overlap(d_in, in_bytes, d_freq, f_bytes) || overlap(d_out, out_bytes, d_freq, f_bytes))
            return fail(GRHIP_EINVAL, "carrier loop: the frequency output may not overlap the other buffers");
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        CarrierLaunch l;
        l.in = (const float2 *)d_in; l.out = d_out; l.freq_out = (float *)d_freq; l.n = n_in; l.nstreams = nstreams;
        l.p = CarrierParams{cl.alpha, cl.beta, cl.max_freq, cl.min_freq, lock_threshold, squelch};
        l.state = d_state.as<CarrierState>();
        if (kind == CARRIER_COSTAS) return costas_launch(order, mode_fast(mode), l, st);
        return pll_launch(kind, l, tabs->atan_tab, st);
    }

    int work(int n_in, const void *in, void *out, void *freq_out)
    {
        // the frequencies are staged behind the output, 16-byte aligned
        const size_t items = (size_t)nstreams * (size_t)n_in, out_bytes = items * out_item();
        const size_t f_off = (out_bytes + 15) & ~(size_t)15, f_bytes = freq_out ? items * 4 : 0;
        int rc = host_work(n_in, 8, in, (size_t)n_in, out_item(), out, f_off - out_bytes + f_bytes, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n_in, d_in, d_out, freq_out ? (char *)d_out + f_off : nullptr, st);
        });
        if (rc || n_in == 0 || !freq_out) return rc;
        // host_work has synchronised; the staged frequencies are still there
        GRHIP_D2H(this, freq_out, (char *)stage_out.p + f_off, f_bytes, own_stream);
        GRHIP_HIP(hipStreamSynchronize(own_stream));
        return GRHIP_OK;
    }
};

}  // namespace

struct grhip_costas_loop_cc : CarrierBlock {};
struct grhip_pll_freqdet_cf : CarrierBlock {};
struct grhip_pll_refout_cc : CarrierBlock {};
struct grhip_pll_carriertracking_cc : CarrierBlock {};

extern "C" {

// gr_pll_freqdet_cf.h:33-34 and its two siblings
#define GRHIP_CL_PLL(NAME, KIND)                                                                                      \
    int grhip_##NAME##_create(grhip_##NAME **h, float loop_bw, float max_freq, float min_freq, int device)            \
    {                                                                                                                 \
        if (!h) return fail(GRHIP_EINVAL, "null argument");                                                           \
        return make_handle(h, [&](grhip_##NAME *b) { return b->init(KIND, 0, loop_bw, max_freq, min_freq, device); }); \
    }                                                                                                                 \
    int grhip_##NAME##_work(grhip_##NAME *h, int n_in, const void *in, void *out)                                     \
    {                                                                                                                 \
        GRHIP_CL_NULL(h);                                                                                             \
        return h->work(n_in, in, out, nullptr);                                                                       \
    }                                                                                                                 \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n_in, const void *d_in, void *d_out, void *stream)            \
    {                                                                                                                 \
        GRHIP_CL_NULL(h);                                                                                             \
        return h->work_device(n_in, d_in, d_out, nullptr, stream);                                                    \
    }                                                                                                                 \
    GRHIP_CL_COMMON(NAME)

GRHIP_CL_PLL(pll_freqdet_cf, PLL_FREQDET)
GRHIP_CL_PLL(pll_refout_cc, PLL_REFOUT)
GRHIP_CL_PLL(pll_carriertracking_cc, PLL_CARRIERTRACKING)

// gr_pll_carriertracking_cc.h:84-90
int grhip_pll_carriertracking_cc_locksig(grhip_pll_carriertracking_cc *h, int s, float *locksig)
{
    GRHIP_CL_NULL(h);
    return h->get_float(s, &CarrierState::locksig, locksig);
}
int grhip_pll_carriertracking_cc_lock_detector(grhip_pll_carriertracking_cc *h, int s, int *locked)
{
    GRHIP_CL_NULL(h);
    return h->lock_detector(s, locked);
}
int grhip_pll_carriertracking_cc_squelch_enable(grhip_pll_carriertracking_cc *h, int enable)
{
    GRHIP_CL_NULL(h);
    return h->squelch_enable(enable);
}
int grhip_pll_carriertracking_cc_set_lock_threshold(grhip_pll_carriertracking_cc *h, float threshold)
{
    GRHIP_CL_NULL(h);
    return h->set_lock_threshold(threshold);
}

// digital_costas_loop_cc.h:61-63; the loop's limits are +-1.0 (digital_costas_loop_cc.cc:46)
int grhip_costas_loop_cc_create(grhip_costas_loop_cc **h, float loop_bw, int order, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_costas_loop_cc *b) { return b->init(CARRIER_COSTAS, order, loop_bw, 1.0f, -1.0f, device); });
}
int grhip_costas_loop_cc_work(grhip_costas_loop_cc *h, int n_in, const void *in, void *out, void *freq_out)
{
    GRHIP_CL_NULL(h);
    return h->work(n_in, in, out, freq_out);
}
int grhip_costas_loop_cc_work_device(grhip_costas_loop_cc *h, int n_in, const void *d_in, void *d_out, void *d_freq_out, void *stream)
{
    GRHIP_CL_NULL(h);
    return h->work_device(n_in, d_in, d_out, d_freq_out, stream);
}
GRHIP_CL_COMMON(costas_loop_cc)

#undef GRHIP_CL_PLL

}  // extern "C"
