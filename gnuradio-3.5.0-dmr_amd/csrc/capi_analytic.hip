// capi_analytic.hip -- C ABI of the real -> complex blocks: gr_firdes::hilbert, gr_hilbert_fc, gr_filter_delay_fc,
// gr_goertzel_fc.
//
// Reference: general/gr_firdes.cc:538-565 (hilbert), 720-780 (window; its WIN_RECTANGULAR case has no break and runs
// on into WIN_HAMMING, so hilbert_fc's default "rectangular" window is a Hamming window -- reproduced, not repaired);
// filter/gr_hilbert_fc.cc:39-67; filter/gr_filter_delay_fc.cc:38-80; filter/gr_goertzel_fc.cc:38-78;
// filter/gri_goertzel.cc:36-75.
//
// hilbert_fc and filter_delay_fc are one handle: taps, delay = ntaps / 2, history = ntaps.  At creation the host looks
// at the taps EXACTLY: odd length >= 3, t[h + i] == 0 for every even i (the centre included) and t[h - i] == -t[h + i]
// for every odd i.  Then (and with one input) FAST runs the sparse kernel; otherwise the dense one.  gr_firdes::hilbert
// produced such taps for every length tried, but nothing in its float arithmetic guarantees it, hence the check.
//
// goertzel_fc keeps no state between blocks (gri_goertzel::batch clears d_d1 / d_d2), so set_freq / set_rate simply
// change what the next call computes.  FAST evaluates the recurrence in closed form: with cos w' = wr / 2 (w' derived
// in double from the FLOAT wr the reference would use) and U_k = sin((k + 1) w') / sin w',
//     d1 = sum_n x[n] U_(len-1-n),   0.5 wr d1 - d2 = sum_n x[n] cos((len - n) w'),
// so out = sum_n x[n] (cos((len - n) w'), wi U_(len-1-n)) / len.  The per-position table is built in double (no
// recurrence: its error does not grow with len) and rounded to float once.
#include <cmath>
#include <vector>

#include "analytic.h"
#include "grhip_internal.h"
#include "stream_block.h"

using namespace grhip;

namespace {

enum { WIN_HAMMING = 0, WIN_HANN = 1, WIN_BLACKMAN = 2, WIN_RECTANGULAR = 3, WIN_KAISER = 4, WIN_BLACKMAN_hARRIS = 5 };

// Izero of general/gr_firdes.cc:35-49
double izero(double x)
{
    double sum, u, halfx, temp;
    int n;
    sum = u = n = 1;
    halfx = x / 2.0;
    do {
        temp = halfx / (double)n;
        n += 1;
        temp *= temp;
        u *= temp;
        sum += u;
    } while (u >= 1E-21 * sum);
    return sum;
}

// gr_firdes::window: every value computed in double, narrowed to float
bool firdes_window(int type, int ntaps, double beta, std::vector<float> &w)
{
    w.assign((size_t)ntaps, 0.f);
    const int M = ntaps - 1;
    switch (type) {
    case WIN_RECTANGULAR:                       // no break in the reference: the ones are overwritten below
    case WIN_HAMMING:
        for (int n = 0; n < ntaps; n++) w[n] = (float)(0.54 - 0.46 * cos((2 * M_PI * n) / M));
        return true;
    case WIN_HANN:
        for (int n = 0; n < ntaps; n++) w[n] = (float)(0.5 - 0.5 * cos((2 * M_PI * n) / M));
        return true;
    case WIN_BLACKMAN:
        for (int n = 0; n < ntaps; n++)
            w[n] = (float)(0.42 - 0.50 * cos((2 * M_PI * n) / (M - 1)) - 0.08 * cos((4 * M_PI * n) / (M - 1)));
        return true;
    case WIN_BLACKMAN_hARRIS:
        for (int n = -ntaps / 2; n < ntaps / 2; n++)        // an odd length leaves the last value at 0
            w[n + ntaps / 2] = (float)(0.35875 + 0.48829 * cos((2 * M_PI * n) / (float)M) +
                                       0.14128 * cos((4 * M_PI * n) / (float)M) + 0.01168 * cos((6 * M_PI * n) / (float)M));
        return true;
    case WIN_KAISER: {
        const double IBeta = 1.0 / izero(beta);
        const double inm1 = 1.0 / ((double)(ntaps));
        for (int i = 0; i < ntaps; i++) {
            const double temp = i * inm1;
            w[i] = (float)(izero(beta * sqrt(1.0 - temp * temp)) * IBeta);
        }
        return true;
    }
    default: return false;
    }
}

int firdes_hilbert(unsigned ntaps, int window_type, double beta, std::vector<float> &taps)
{
    if (!(ntaps & 1)) return fail(GRHIP_ERANGE, "Hilbert:  Must have odd number of taps");
    if (ntaps > (1u << 24)) return fail(GRHIP_EINVAL, "firdes_hilbert: too many taps");
    std::vector<float> w;
    if (!firdes_window(window_type, (int)ntaps, beta, w)) return fail(GRHIP_ERANGE, "gr_firdes:window: type out of range");
    taps.assign(ntaps, 0.f);
    const unsigned h = (ntaps - 1) / 2;
    volatile float gain = 0;                    // volatile: every step rounds to float, whatever the host compiler
    for (unsigned i = 1; i <= h; i++) {
        if (i & 1) {
            const float x = 1 / (float)i;
            taps[h + i] = x * w[h + i];
            taps[h - i] = -x * w[h - i];
            gain = taps[h + i] - gain;
        } else
            taps[h + i] = taps[h - i] = 0;
    }
    const float g2 = 2 * fabsf(gain);
    for (unsigned i = 0; i < ntaps; i++) taps[i] /= g2;
    return GRHIP_OK;
}

}  // namespace

struct grhip_analytic_base : ModeBlock {
    std::vector<float> taps;                    // forward order, as given
    int ntaps = 0, delay = 0, nodd = 0;
    bool sparse = false;
    DevBuf d_rev, d_odd;

    int install(const float *t, size_t n)
    {
        if (!t || n < 1) return fail(GRHIP_EINVAL, "filter_delay_fc needs at least one tap");
        if (n > (size_t)AN_MAX_TAPS) return fail(GRHIP_EINVAL, "filter_delay_fc: at most %d taps", AN_MAX_TAPS);
        taps.assign(t, t + n);
        ntaps = (int)n;
        delay = ntaps / 2;
        std::vector<float> rev(taps.rbegin(), taps.rend()), odd;
        const int h = ntaps / 2;
        sparse = (ntaps & 1) && ntaps >= 3;
        for (int i = 0; sparse && i <= h; ++i) {
            if (i & 1) sparse = taps[h - i] == -taps[h + i];
            else sparse = taps[h + i] == 0.f && taps[h - i] == 0.f;
        }
        nodd = 0;
        if (sparse) {
            for (int i = 1; i <= h; i += 2) odd.push_back(taps[h + i]);
            nodd = (int)odd.size();
        }
        int rc = d_rev.reserve(rev.size() * sizeof(float));
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(d_rev.p, rev.data(), rev.size() * sizeof(float), hipMemcpyHostToDevice));
        if (sparse) {
            if ((rc = d_odd.reserve(odd.size() * sizeof(float)))) return rc;
            GRHIP_HIP(hipMemcpy(d_odd.p, odd.data(), odd.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        return GRHIP_OK;
    }

    int work_device(int noutput_items, const void *d_in0, const void *d_in1, void *d_out, void *stream)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        if (noutput_items == 0) return 0;
        if (!d_in0 || !d_out) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        int m;
        {
            std::lock_guard<std::mutex> lk(setter_mutex);
            m = mode;
        }
        AnalyticLaunch a;
        a.in0 = (const float *)d_in0;
        a.in1 = d_in1 ? (const float *)d_in1 : a.in0;
        a.out = (float2 *)d_out;
        a.n_out = noutput_items;
        a.taps_rev = d_rev.as<float>();
        a.odd = sparse ? d_odd.as<float>() : nullptr;
        a.ntaps = ntaps; a.delay = delay; a.nodd = nodd;
        const int form = !mode_fast(m) ? AN_GENERIC : (sparse && a.in1 == a.in0) ? AN_SPARSE : AN_DENSE;
        if ((rc = analytic_launch(form, a, pick(stream)))) return rc;
        return noutput_items;
    }

    int work(int noutput_items, const void *in0, const void *in1, void *out)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        if (noutput_items == 0) return 0;
        if (!in0 || !out) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        const size_t bytes = ((size_t)noutput_items + ntaps - 1) * sizeof(float), slot = (bytes + 15) & ~(size_t)15;
        return (int)host_call(in0, bytes, slot * (in1 ? 2 : 1) + 16, (size_t)noutput_items * 8 + 16, out, 8,
                              [&](void *d_in, void *d_out, hipStream_t s) -> long long {
                                  void *d_in1 = nullptr;
                                  if (in1) {
                                      d_in1 = (char *)d_in + slot;
                                      GRHIP_H2D(this, d_in1, in1, bytes, s);
                                  }
                                  return work_device(noutput_items, d_in, d_in1, d_out, s);
                              });
    }

    int read_taps(float *out, size_t cap) const
    {
        if (!out || cap < (size_t)ntaps) return fail(GRHIP_EINVAL, "taps: room for %d floats needed", ntaps);
        memcpy(out, taps.data(), (size_t)ntaps * sizeof(float));
        return ntaps;
    }
};

struct grhip_hilbert_fc : grhip_analytic_base {};
struct grhip_filter_delay_fc : grhip_analytic_base {};

struct grhip_goertzel_fc : ModeBlock {
    int rate = 1, len = 1;
    float freq = 0.f, wr = 0.f, wi = 0.f;
    DevBuf d_tab;
    bool tab_valid = false;

    // gri_goertzel::gri_setparms (gri_goertzel.cc:41-52)
    void setparms()
    {
        goertzel_setparms(rate, freq, &wr, &wi);
        tab_valid = false;
    }

    int build_tab(hipStream_t st)
    {
        std::vector<float2> tab((size_t)len);
        goertzel_build_table(len, wr, wi, tab.data());
        int rc = drain(st);                                         // a launch may still read the old table
        if (rc) return rc;
        if ((rc = d_tab.reserve(tab.size() * sizeof(float2)))) return rc;
        GRHIP_HIP(hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice));
        tab_valid = true;
        return GRHIP_OK;
    }

    int work_device(int noutput_items, const void *d_in, void *d_out, void *stream)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        if (noutput_items == 0) return 0;
        if (!d_in || !d_out) return fail(GRHIP_EINVAL, "null buffer");
        if (!aligned(d_in, 4) || !aligned(d_out, 8)) return fail(GRHIP_EINVAL, "goertzel: items not naturally aligned");
        int rc = bind();
        if (rc) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        if (mode_fast(mode)) {
            if (!tab_valid && (rc = build_tab(st))) return rc;
            rc = goertzel_launch_fast((const float *)d_in, (float2 *)d_out, noutput_items, len, d_tab.as<float2>(), st);
        } else
            rc = goertzel_launch_generic((const float *)d_in, (float2 *)d_out, noutput_items, len, wr, wi, st);
        return rc ? rc : noutput_items;
    }

    int work(int noutput_items, const void *in, void *out)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        if (noutput_items == 0) return 0;
        if (!in || !out) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        const size_t bytes = (size_t)noutput_items * (size_t)len * sizeof(float);
        return (int)host_call(in, bytes, bytes + 16, (size_t)noutput_items * 8 + 16, out, 8,
                              [&](void *d_in, void *d_out, hipStream_t s) -> long long {
                                  return work_device(noutput_items, d_in, d_out, s);
                              });
    }
};

namespace {

template <class H>
int create_analytic(H **h, const float *taps, size_t ntaps, int device)
{
    return make_handle(h, [&](H *b) {
        int rc = b->init_device(device);
        if (rc) return rc;
        b->mode = default_mode();
        return b->install(taps, ntaps);
    });
}

}  // namespace

extern "C" {

int grhip_firdes_hilbert(unsigned ntaps, int window_type, double beta, float *out)
{
    if (!out) return fail(GRHIP_EINVAL, "null argument");
    std::vector<float> t;
    int rc = firdes_hilbert(ntaps, window_type, beta, t);
    if (rc) return rc;
    memcpy(out, t.data(), t.size() * sizeof(float));
    return GRHIP_OK;
}

// general/gr_firdes.cc:104-148, compute_ntaps :680-695, sanity_check_1f :783-796
int grhip_firdes_low_pass(double gain, double fs, double cutoff, double transition, int window_type, double beta, float *out,
                          size_t cap, size_t *ntaps_out)
{
    static const float width_factor[5] = {3.3, 3.1, 5.5, 2.0, 10.0};
    if (!ntaps_out) return fail(GRHIP_EINVAL, "null argument");
    if (!std::isfinite(gain) || !std::isfinite(fs) || !std::isfinite(cutoff) || !std::isfinite(transition) || !std::isfinite(beta))
        return fail(GRHIP_EINVAL, "firdes_low_pass: an argument is not finite");
    if (fs <= 0.0) return fail(GRHIP_EINVAL, "gr_firdes check failed: sampling_freq > 0");
    if (cutoff <= 0.0 || cutoff > fs / 2) return fail(GRHIP_EINVAL, "gr_firdes check failed: 0 < fa <= sampling_freq / 2");
    if (transition <= 0) return fail(GRHIP_EINVAL, "gr_firdes check failed: transition_width > 0");
    if (window_type < 0 || window_type > WIN_KAISER) return fail(GRHIP_EINVAL, "firdes_low_pass: window type outside 0 .. 4");
    const double delta_f = transition / fs;
    const double want = width_factor[window_type] / delta_f + 0.5;
    if (!(want < (double)(1 << 24))) return fail(GRHIP_EINVAL, "firdes_low_pass: too many taps");
    int ntaps = (int)want;
    if ((ntaps & 1) == 0) ntaps++;
    *ntaps_out = (size_t)ntaps;
    if (cap < (size_t)ntaps || !out) return fail(GRHIP_ERANGE, "firdes_low_pass: %d taps, room for %zu", ntaps, out ? cap : (size_t)0);
    std::vector<float> w;
    firdes_window(window_type, ntaps, beta, w);
    std::vector<float> taps((size_t)ntaps);
    const int M = (ntaps - 1) / 2;
    const double fwT0 = 2 * M_PI * cutoff / fs;
    for (int n = -M; n <= M; n++) {
        if (n == 0) taps[n + M] = (float)(fwT0 / M_PI * w[n + M]);
        else taps[n + M] = (float)(sin(n * fwT0) / (n * M_PI) * w[n + M]);
    }
    double fmax = taps[0 + M];
    for (int n = 1; n <= M; n++) fmax += 2 * taps[n + M];
    gain /= fmax;
    for (int i = 0; i < ntaps; i++) taps[i] = (float)(taps[i] * gain);
    memcpy(out, taps.data(), taps.size() * sizeof(float));
    return GRHIP_OK;
}

// blks2impl/fm_emph.py:55-63
int grhip_fm_deemph_taps(double fs, double tau, double *b, double *a)
{
    if (!b || !a) return fail(GRHIP_EINVAL, "null argument");
    if (!std::isfinite(fs) || !std::isfinite(tau) || fs == 0.0 || tau == 0.0)
        return fail(GRHIP_EINVAL, "fm_deemph: fs and tau must be finite and not zero");
    const double w_p = 1 / tau;
    const double w_pp = tan(w_p / (fs * 2));
    a[0] = 1;
    a[1] = (w_pp - 1) / (w_pp + 1);
    b[0] = w_pp / (1 + w_pp);
    b[1] = b[0];
    return GRHIP_OK;
}

int grhip_hilbert_fc_create(grhip_hilbert_fc **h, unsigned ntaps, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (ntaps <= 1) return fail(GRHIP_EINVAL, "hilbert_fc: ntaps must be at least 2 (one tap divides 0 by 0)");
    if (ntaps > (unsigned)AN_MAX_TAPS) return fail(GRHIP_EINVAL, "hilbert_fc: at most %d taps", AN_MAX_TAPS);
    std::vector<float> t;
    int rc = firdes_hilbert(ntaps | 1u, WIN_RECTANGULAR, 6.76, t);       // d_ntaps = ntaps | 0x1, gr_firdes::hilbert's defaults
    if (rc) return rc;
    return create_analytic(h, t.data(), t.size(), device);
}

int grhip_filter_delay_fc_create(grhip_filter_delay_fc **h, const float *taps, size_t ntaps, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (!taps || ntaps < 1) return fail(GRHIP_EINVAL, "filter_delay_fc needs at least one tap");
    if (ntaps > (size_t)AN_MAX_TAPS) return fail(GRHIP_EINVAL, "filter_delay_fc: at most %d taps", AN_MAX_TAPS);
    return create_analytic(h, taps, ntaps, device);
}

#define GRHIP_ANALYTIC_COMMON(NAME)                                                                                    \
    void grhip_##NAME##_destroy(grhip_##NAME *h)                                                                       \
    {                                                                                                                  \
        destroy_handle(h);                                                                                             \
    }                                                                                                                  \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode)                                                             \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->set_mode(mode);                                                                                      \
    }                                                                                                                  \
    int grhip_##NAME##_history(const grhip_##NAME *h) { return h ? h->ntaps : fail(GRHIP_EINVAL, "null handle"); }    \
    int grhip_##NAME##_ntaps(const grhip_##NAME *h) { return h ? h->ntaps : fail(GRHIP_EINVAL, "null handle"); }      \
    int grhip_##NAME##_taps(const grhip_##NAME *h, float *out, size_t capacity)                                       \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->read_taps(out, capacity);                                                                            \
    }                                                                                                                  \
    int grhip_##NAME##_is_sparse(const grhip_##NAME *h) { return h ? (h->sparse ? 1 : 0) : fail(GRHIP_EINVAL, "null handle"); }

GRHIP_ANALYTIC_COMMON(hilbert_fc)
GRHIP_ANALYTIC_COMMON(filter_delay_fc)
#undef GRHIP_ANALYTIC_COMMON

int grhip_hilbert_fc_work(grhip_hilbert_fc *h, int noutput_items, const void *in, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work(noutput_items, in, nullptr, out);
}

int grhip_hilbert_fc_work_device(grhip_hilbert_fc *h, int noutput_items, const void *d_in, void *d_out, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work_device(noutput_items, d_in, nullptr, d_out, stream);
}

int grhip_filter_delay_fc_work(grhip_filter_delay_fc *h, int noutput_items, const void *in0, const void *in1, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work(noutput_items, in0, in1, out);
}

int grhip_filter_delay_fc_work_device(grhip_filter_delay_fc *h, int noutput_items, const void *d_in0, const void *d_in1,
                                      void *d_out, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work_device(noutput_items, d_in0, d_in1, d_out, stream);
}

int grhip_goertzel_fc_create(grhip_goertzel_fc **h, int rate, int len, float freq, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (len < 1 || len > (1 << 24)) return fail(GRHIP_EINVAL, "goertzel_fc: len must be in [1, 2^24]");
    if (rate == 0) return fail(GRHIP_EINVAL, "goertzel_fc: rate must not be 0");
    return make_handle(h, [&](grhip_goertzel_fc *g) {
        g->rate = rate; g->len = len; g->freq = freq;
        g->setparms();
        g->mode = default_mode();
        return g->init_device(device);
    });
}

void grhip_goertzel_fc_destroy(grhip_goertzel_fc *h)
{
    destroy_handle(h);
}

int grhip_goertzel_fc_set_freq(grhip_goertzel_fc *h, float freq)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    h->freq = freq;
    h->setparms();
    return GRHIP_OK;
}

int grhip_goertzel_fc_set_rate(grhip_goertzel_fc *h, int rate)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (rate == 0) return fail(GRHIP_EINVAL, "goertzel_fc: rate must not be 0");
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    h->rate = rate;
    h->setparms();
    return GRHIP_OK;
}

int grhip_goertzel_fc_set_mode(grhip_goertzel_fc *h, int mode)
{
    return h ? h->set_mode(mode) : fail(GRHIP_EINVAL, "null handle");
}

int grhip_goertzel_fc_decimation(const grhip_goertzel_fc *h) { return h ? h->len : fail(GRHIP_EINVAL, "null handle"); }

int grhip_goertzel_fc_work(grhip_goertzel_fc *h, int noutput_items, const void *in, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work(noutput_items, in, out);
}

int grhip_goertzel_fc_work_device(grhip_goertzel_fc *h, int noutput_items, const void *d_in, void *d_out, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work_device(noutput_items, d_in, d_out, stream);
}

}  // extern "C"
