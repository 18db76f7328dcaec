// capi_fll.hip -- C ABI of digital_fll_band_edge_cc, of its filter designer and of gr_firdes::root_raised_cosine.
//
// Reference: gr-digital/lib/digital_fll_band_edge_cc.{h,cc}, general/gri_control_loop.{h,cc}, general/gr_firdes.cc:601-650.
//
// A handle takes S streams back to back ([S][n_in]) and works on new items only.  What a stream remembers on the
// device is its phase and frequency (a CarrierState), its last filter_size inputs and its last filter_size - 1
// derotated samples, so the result depends on the concatenated input alone (include/grhip.h).  The two tap sets are
// designed on the host (fll_taps.h) and live on the device; the loop gains and limits are kernel arguments.
#include <complex>
#include <cstring>
#include <vector>

#include "fll_band_edge.h"
#include "fll_taps.h"
#include "loop_block.h"

using namespace grhip;

namespace {

struct FllBlock : LoopBlock {
    float sps = 0.f, rolloff = 0.f;
    int fs = 0;
    DevBuf d_lower, d_upper, d_xh, d_dh;

    // the two histories back at zeros, sized for fs; streams drained, under setter_mutex
    int zero_hist()
    {
        const size_t bytes = (size_t)nstreams * (size_t)fs * sizeof(float2);
        int rc;
        if ((rc = d_xh.reserve(bytes)) || (rc = d_dh.reserve(bytes))) return rc;
        if ((rc = zero_device(d_xh.p, bytes))) return rc;
        return zero_device(d_dh.p, bytes);
    }

    int restart()
    {
        int rc = zero_loop_state();
        return rc ? rc : zero_hist();
    }

    // design_filter for (sps_, rolloff_, fs_) onto the device; nothing changes where the design is refused.  Streams
    // drained, under setter_mutex.
    int design(float sps_, float rolloff_, int fs_)
    {
        std::vector<std::complex<float>> lo, up;
        if (const char *e = fll_design(sps_, rolloff_, fs_, lo, up)) return fail(GRHIP_EINVAL, "%s", e);
        const size_t bytes = (size_t)fs_ * sizeof(float2);
        int rc;
        if ((rc = d_lower.reserve(bytes)) || (rc = d_upper.reserve(bytes))) return rc;
        GRHIP_HIP(hipMemcpy(d_lower.p, lo.data(), bytes, hipMemcpyHostToDevice));
        GRHIP_HIP(hipMemcpy(d_upper.p, up.data(), bytes, hipMemcpyHostToDevice));
        sps = sps_; rolloff = rolloff_; fs = fs_;
        return GRHIP_OK;
    }

    int init(float sps_, float rolloff_, int fs_, float bandwidth, int dev)
    {
        if (const char *e = fll_check(sps_, rolloff_, fs_)) return fail(GRHIP_EINVAL, "%s", e);
        const float max_freq = fll_max_freq_of(sps_);           // digital_fll_band_edge_cc.cc:58
        if (!cl.init(bandwidth, max_freq, -max_freq))
            return fail(GRHIP_EINVAL, "gri_control_loop: invalid bandwidth. Must be >= 0 (and leave finite gains).");
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        if ((rc = design(sps_, rolloff_, fs_))) return rc;
        return restart();
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
    }

    // set_samples_per_symbol, set_rolloff, set_filter_size (:92-120): a new design; a new size also zeroes the histories.
    // The device is idle while the taps are rewritten: a launch on a caller's stream may still read them.
    // A null argument keeps the value.
    int redesign(const float *sps_, const float *rolloff_, const int *fs_)
    {
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        GRHIP_HIP(hipDeviceSynchronize());
        if ((rc = design(sps_ ? *sps_ : sps, rolloff_ ? *rolloff_ : rolloff, fs_ ? *fs_ : fs))) return rc;
        return fs_ ? zero_hist() : GRHIP_OK;
    }

    int set_sps(float v) { return redesign(&v, nullptr, nullptr); }
    int set_rolloff(float v) { return redesign(nullptr, &v, nullptr); }
    int set_filter_size(int v) { return redesign(nullptr, nullptr, &v); }

    template <class T>
    T get(T FllBlock::*which)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return this->*which;
    }

    int work_device(int n_in, const void *d_in, void *d_out, void *d_frq, void *d_phs, void *d_err, void *stream)
    {
        const int c = check_count(n_in);
        if (c <= 0) return c;
        int rc = check_io(d_in, 8, d_out, 8);
        if (rc) return rc;
        const void *aux[3] = {d_frq, d_phs, d_err};
        const int given = (d_frq != nullptr) + (d_phs != nullptr) + (d_err != nullptr);
        if (given != 0 && given != 3) return fail(GRHIP_EINVAL, "fll_band_edge_cc: frq, phs and err are given together or not at all");
        const size_t items = (size_t)nstreams * (size_t)n_in, c_bytes = items * 8, f_bytes = items * 4;
        if ((rc = check_apart("fll_band_edge_cc", d_in, c_bytes, d_out, c_bytes))) return rc;
        for (int i = 0; i < 3; ++i) {
            if (!aligned(aux[i], 4)) return fail(GRHIP_EINVAL, "items not naturally aligned");
            bool hit = overlap(d_in, c_bytes, aux[i], f_bytes) || overlap(d_out, c_bytes, aux[i], f_bytes);
            for (int k = 0; k < i; ++k) hit = hit || overlap(aux[k], f_bytes, aux[i], f_bytes);
            if (hit) return fail(GRHIP_EINVAL, "fll_band_edge_cc: frq, phs and err may not overlap another buffer");
        }
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        FllLaunch l;
        l.in = (const float2 *)d_in; l.out = (float2 *)d_out;
        l.frq = (float *)d_frq; l.phs = (float *)d_phs; l.err = (float *)d_err;
        l.n = n_in; l.nstreams = nstreams; l.fs = fs;
        l.lower = d_lower.as<float2>(); l.upper = d_upper.as<float2>();
        l.p = CarrierParams{cl.alpha, cl.beta, cl.max_freq, cl.min_freq, 0.f, 0};
        l.state = d_state.as<CarrierState>();
        l.xh = d_xh.as<float2>(); l.dh = d_dh.as<float2>();
        return fll_band_edge_launch(!mode_fast(mode), l, st);
    }

    int work(int n_in, const void *in, void *out, void *frq, void *phs, void *err)
    {
        const int given = (frq != nullptr) + (phs != nullptr) + (err != nullptr);
        if (given != 0 && given != 3) return fail(GRHIP_EINVAL, "fll_band_edge_cc: frq, phs and err are given together or not at all");
        // the three float outputs are staged behind the output, 16-byte aligned
        const size_t items = (size_t)nstreams * (size_t)(n_in > 0 ? n_in : 0), out_bytes = items * 8;
        const size_t f_row = (items * 4 + 15) & ~(size_t)15, f_off = (out_bytes + 15) & ~(size_t)15;
        int rc = host_work(n_in, 8, in, (size_t)n_in, 8, out, f_off - out_bytes + (given ? 3 * f_row : 0), [&](void *d_in, void *d_out, hipStream_t st) {
            char *f = (char *)d_out + f_off;
            return work_device(n_in, d_in, d_out, given ? f : nullptr, given ? f + f_row : nullptr, given ? f + 2 * f_row : nullptr, st);
        });
        if (rc || n_in == 0 || !given) return rc;
        // host_work has synchronised; the staged floats are still there
        void *dst[3] = {frq, phs, err};
        for (int i = 0; i < 3; ++i) GRHIP_D2H(this, dst[i], (char *)stage_out.p + f_off + (size_t)i * f_row, items * 4, own_stream);
        GRHIP_HIP(hipStreamSynchronize(own_stream));
        return GRHIP_OK;
    }
};

// the size query of grhip_firdes_low_pass: *ntaps always, the taps where they fit
template <class T>
int hand_out(const char *who, const std::vector<T> &t, T *out, size_t cap, size_t *ntaps_out)
{
    *ntaps_out = t.size();
    if (cap < t.size() || !out) return fail(GRHIP_ERANGE, "%s: %zu taps, room for %zu", who, t.size(), out ? cap : (size_t)0);
    memcpy(out, t.data(), t.size() * sizeof(T));
    return GRHIP_OK;
}

}  // namespace

struct grhip_fll_band_edge_cc : FllBlock {};

extern "C" {

int grhip_firdes_root_raised_cosine(double gain, double fs, double symbol_rate, double alpha, int ntaps, float *out, size_t cap,
                                    size_t *ntaps_out)
{
    if (!ntaps_out) return fail(GRHIP_EINVAL, "null argument");
    std::vector<float> t;
    if (const char *e = rrc_design(gain, fs, symbol_rate, alpha, ntaps, t)) return fail(GRHIP_EINVAL, "%s", e);
    return hand_out("firdes_root_raised_cosine", t, out, cap, ntaps_out);
}

int grhip_fll_band_edge_taps(float sps, float rolloff, int filter_size, void *lower, void *upper)
{
    if (!lower || !upper) return fail(GRHIP_EINVAL, "null argument");
    std::vector<std::complex<float>> lo, up;
    if (const char *e = fll_design(sps, rolloff, filter_size, lo, up)) return fail(GRHIP_EINVAL, "%s", e);
    memcpy(lower, lo.data(), lo.size() * sizeof(lo[0]));
    memcpy(upper, up.data(), up.size() * sizeof(up[0]));
    return GRHIP_OK;
}

int grhip_fll_band_edge_cc_create(grhip_fll_band_edge_cc **h, float samps_per_sym, float rolloff, int filter_size, float bandwidth,
                                  int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_fll_band_edge_cc *b) { return b->init(samps_per_sym, rolloff, filter_size, bandwidth, device); });
}

int grhip_fll_band_edge_cc_work(grhip_fll_band_edge_cc *h, int n_in, const void *in, void *out, void *frq, void *phs, void *err)
{
    GRHIP_CL_NULL(h);
    return h->work(n_in, in, out, frq, phs, err);
}

int grhip_fll_band_edge_cc_work_device(grhip_fll_band_edge_cc *h, int n_in, const void *d_in, void *d_out, void *d_frq, void *d_phs,
                                       void *d_err, void *stream)
{
    GRHIP_CL_NULL(h);
    return h->work_device(n_in, d_in, d_out, d_frq, d_phs, d_err, stream);
}

GRHIP_CL_COMMON(fll_band_edge_cc)

// digital_fll_band_edge_cc.cc:92-142
int grhip_fll_band_edge_cc_set_samples_per_symbol(grhip_fll_band_edge_cc *h, float sps) { GRHIP_CL_NULL(h); return h->set_sps(sps); }
int grhip_fll_band_edge_cc_set_rolloff(grhip_fll_band_edge_cc *h, float rolloff) { GRHIP_CL_NULL(h); return h->set_rolloff(rolloff); }
int grhip_fll_band_edge_cc_set_filter_size(grhip_fll_band_edge_cc *h, int filter_size) { GRHIP_CL_NULL(h); return h->set_filter_size(filter_size); }
float grhip_fll_band_edge_cc_get_samples_per_symbol(grhip_fll_band_edge_cc *h)
{
    if (!h) return (float)fail(GRHIP_EINVAL, "null handle");
    return h->get(&FllBlock::sps);
}
float grhip_fll_band_edge_cc_get_rolloff(grhip_fll_band_edge_cc *h)
{
    if (!h) return (float)fail(GRHIP_EINVAL, "null handle");
    return h->get(&FllBlock::rolloff);
}
int grhip_fll_band_edge_cc_get_filter_size(grhip_fll_band_edge_cc *h)
{
    GRHIP_CL_NULL(h);
    return h->get(&FllBlock::fs);
}

}  // extern "C"
