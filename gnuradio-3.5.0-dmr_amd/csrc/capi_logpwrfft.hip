// capi_logpwrfft.hip -- C ABI of blks2.logpwrfft_c / logpwrfft_f: the windowed forward transform of every kept frame,
// |X|^2, the averaging single-pole IIR and 10 log10 + k, fused into the register FFT kernels.
//
// Reference: gnuradio-core/src/python/gnuradio/blks2impl/logpwrfft.py:26-154 (the hier block),
// blks2impl/stream_to_vector_decimator.py:24-93 (the decimation rule), gnuradio/window.py:166-176 (the default
// window), general/gr_keep_one_in_n.cc:52-105 (the countdown).
//
// The block is the reference's six in a row: stream_to_vector -> keep_one_in_n -> fft_vcc | fft_vfc ->
// complex_to_mag_squared -> single_pole_iir_filter_ff -> nlog10_ff.  Its arithmetic is instruction for instruction that
// of this library's own blocks run one after the other (the same kernel templates, spectrum_math.h), so the results are
// bit for bit theirs in every mode; what changes is the HBM traffic:
//   averaging off (IIR taps exactly 1.0): the transform kernel stores dB directly, 8 B in + 4 B out per kept complex
//     sample (4 + 4 for float input), and the lanes that transform the last kept frame of a stream leave its power in
//     the IIR's state.  The reference computes (float)(1.0 x + 0.0 y_prev), which is x for every finite y_prev; after a
//     NON-FINITE state (0 * inf = NaN there) the shortcut differs from the reference.  Non-finite input is out of scope.
//   averaging on: the kernel stores the power into `out`, one more pass runs the recurrence along the frame axis in place
//     and writes the log of every average: 20 B (16 B) per kept sample, no scratch buffer for the power.
// Frames that are not kept are never read.
// Composed path (same results): sizes outside 32 ... 8192 powers of two, a transform that runs unwindowed (a window of
// the wrong length), and kept-frame addressing out of the kernels' reach (logpwr_plan.h) run keep_one_in_n, the
// transform (FftPlan), mag^2 and the IIR-plus-log pass one after the other through buffers the handle owns.
//
// All arithmetic on rates is true division (Python 3's); Python 2's integer division of all-integer arguments is not
// reproduced.
#include <cmath>

#include "fft_kernels.h"
#include "grhip_internal.h"
#include "logpwr_plan.h"
#include "spectrum.h"
#include "stream_block.h"

using namespace grhip;

namespace {

// window.py:166-176 with the coefficients of line 176: window[i] = sum_c (-1)**c * coeff_c * cos(2.0*c*pi*(i+0.5)/(fft_size-1)),
// accumulated from 0 in coefficient order
int blackmanharris(int fft_size, std::vector<double> &w)
{
    static const double coeffs[4] = {0.35875, 0.48829, 0.14128, 0.01168};
    if (fft_size < 0) return fail(GRHIP_EINVAL, "window: negative fft_size");
    if (fft_size == 1) return fail(GRHIP_EINVAL, "window: fft_size 1 divides by fft_size - 1 = 0");      // ZeroDivisionError there
    w.assign((size_t)fft_size, 0.0);
    for (int i = 0; i < fft_size; ++i)
        for (int c = 0; c < 4; ++c) {
            const double sign = (c & 1) ? -1.0 : 1.0;
            w[i] += sign * coeffs[c] * cos(2.0 * c * M_PI * (i + 0.5) / (fft_size - 1));
        }
    return GRHIP_OK;
}

// stream_to_vector_decimator.py:71: max(1, int(round(decim))), Python 2's round (half away from zero, as C's)
int decimation_of(double decim, int *out)
{
    if (!std::isfinite(decim)) return fail(GRHIP_EINVAL, "logpwrfft: decimation is not finite (a rate of 0?)");
    const double r = round(decim);
    if (r > 2147483647.0) return fail(GRHIP_EINVAL, "logpwrfft: decimation past 2^31 - 1");
    *out = r < 1.0 ? 1 : (int)r;
    return GRHIP_OK;
}

}  // namespace

struct LogPwrFft : StreamBlock {
    bool real_in = false;
    int N = 0;
    double sample_rate = 0, vec_rate = 0, avg_alpha = 1.0;
    bool average = false;
    int decim = 1;
    KeepOne ctr;
    float k = 0.f;
    bool has_window = false;
    FftPlan plan;
    DevBuf d_window, d_state, d_scratch, d_keep, d_spec;

    size_t item() const { return real_in ? 4 : 8; }

    int restart()       // under setter_mutex (or before the handle is handed out): zero state, countdown reloaded
    {
        const size_t b = (size_t)nstreams * N * sizeof(float);
        int rc = d_state.reserve(b);
        if (rc) return rc;
        ctr.set_n(decim);
        return zero_device(d_state.p, b);
    }

    int set_decim(double d)
    {
        int v = 1;
        if (int rc = decimation_of(d, &v)) return rc;
        decim = v;
        ctr.set_n(v);                       // gr_keep_one_in_n.cc:52-65: set_n reloads the countdown
        return GRHIP_OK;
    }
    int update_decimator() { return set_decim(sample_rate / N / vec_rate); }      // stream_to_vector_decimator.py:74-75

    int work_device(int n_frames, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n_frames);
        if (c <= 0) return c;
        int rc = check_io(d_in, item(), d_out, 4);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        return run(n_frames, d_in, d_out, pick(stream));
    }

    // under setter_mutex: what the countdown keeps of the next n_frames, transformed; advances the countdown
    int run(int n_frames, const void *d_in, void *d_out, hipStream_t st)
    {
        const long long p = ctr.produced(n_frames);
        if (p > 0)
            if (int rc = launch(n_frames, p, d_in, (float *)d_out, st)) return rc;
        ctr.advance(n_frames);
        return (int)p;
    }

    int launch(long long n_frames, long long p, const void *d_in, float *out, hipStream_t st)
    {
        const double alpha = average ? avg_alpha : 1.0;                     // logpwrfft.py:91-100
        const float *w = has_window ? d_window.as<float>() : nullptr;
        IirLaunch a;
        a.in = out; a.out = out; a.n = p; a.nstreams = nstreams; a.vlen = N; a.alpha = alpha; a.state = d_state.as<float>();
        a.log = true; a.log_n = 10.f; a.log_k = k;
        int rc;
        if (plan.kind == FftPlan::NATIVE && w && logpwr_fused_ok(N, (int)item(), nstreams, n_frames, p, ctr.n)) {
            FftFrames fr;
            fr.n_frames = n_frames; fr.n_out = (int)p; fr.first = ctr.first(); fr.n = ctr.n; fr.k = k;
            fr.state = d_state.as<float>();
            const bool db = alpha == 1.0;
            if ((rc = launch_fft_power(N, real_in, db, w, plan.d_tw.as<float2>(), d_in, out, nstreams, fr, st))) return rc;
            return db ? GRHIP_OK : single_pole_iir_launch(mode_fast(mode), a, d_scratch, st);
        }
        // the blocks one after the other
        const size_t frames = (size_t)nstreams * (size_t)p;
        if ((rc = d_keep.reserve(frames * N * item()))) return rc;
        if ((rc = d_spec.reserve(frames * N * sizeof(float2)))) return rc;
        if ((rc = keep_one_launch(d_in, d_keep.p, (size_t)N * item(), n_frames, p, ctr.first(), ctr.n, nstreams, st))) return rc;
        rc = real_in ? plan.exec_real(w, d_keep.as<float>(), d_spec.as<float2>(), (long long)frames, st)
                     : plan.exec(0, w, d_keep.as<float2>(), d_spec.as<float2>(), (long long)frames, st);
        if (rc) return rc;
        if ((rc = mag_squared_launch(d_spec.as<float2>(), out, (long long)frames * N, st))) return rc;
        return single_pole_iir_launch(mode_fast(mode), a, d_scratch, st);
    }

    int work(int n_frames, const void *in, void *out)
    {
        const int c = check_count(n_frames);
        if (c <= 0) return c;
        if (!in || !out) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        // not host_work: one lock over the count that sizes the staging buffers and the launch that fills them: a setter cannot change
        // the decimation in between
        std::lock_guard<std::mutex> lk(setter_mutex);
        const long long p = ctr.produced(n_frames);
        const size_t in_bytes = (size_t)nstreams * (size_t)n_frames * N * item();
        const size_t out_bytes = (size_t)nstreams * (size_t)p * N * sizeof(float);
        return (int)host_call(in, in_bytes, in_bytes + 16, out_bytes + 16, out, (size_t)nstreams * N * sizeof(float),
                              [&](void *d_in, void *d_out, hipStream_t s) -> long long {
                                  return run(n_frames, d_in, d_out, s);
                              });
    }
};
struct grhip_logpwrfft_c : LogPwrFft {};
struct grhip_logpwrfft_f : LogPwrFft {};

namespace {

int check_alpha(double alpha)
{
    // gr_single_pole_iir.h:62-63 (a NaN passes there; it is refused here)
    return (alpha >= 0.0 && alpha <= 1.0) ? GRHIP_OK : fail(GRHIP_ERANGE, "Alpha must be in [0, 1]");
}

template <class H>
int logpwrfft_create(H **h, bool real_in, double sample_rate, int fft_size, double ref_scale, double frame_rate,
                     double avg_alpha, int average, const double *window, size_t window_len, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (fft_size <= 0) return fail(GRHIP_ERANGE, "gri_fftw: invalid fft_size");      // gri_fft.cc:104-105
    if (!FftPlan::size_ok(fft_size))
        return fail(GRHIP_EINVAL, "fft_size %d: more than 2^26 points (2^25 when not a power of two)", fft_size);
    if (window_len && !window) return fail(GRHIP_EINVAL, "window is NULL");
    if (int rc = check_alpha(avg_alpha)) return rc;
    if (!(ref_scale > 0)) return fail(GRHIP_EINVAL, "logpwrfft: ref_scale must be positive (log10 of ref_scale / 2)");
    // logpwrfft.py:52-55: win(fft_size) in double, window_power the sum of squares in order
    std::vector<double> wd;
    if (window_len) wd.assign(window, window + window_len);
    else if (int rc = blackmanharris(fft_size, wd)) return rc;
    double window_power = 0.0;
    for (double x : wd) window_power += x * x;
    if (!(window_power > 0)) return fail(GRHIP_EINVAL, "logpwrfft: window power is zero");
    // logpwrfft.py:59-62, in double; gr_nlog10_ff takes a float k
    const double kd = -20 * log10((double)fft_size) - 10 * log10(window_power / fft_size) - 20 * log10(ref_scale / 2);
    int decim = 1;
    if (int rc = decimation_of(sample_rate / fft_size / frame_rate, &decim)) return rc;
    return make_handle(h, [&](H *b) {
        b->real_in = real_in; b->N = fft_size; b->mode = default_mode();
        b->sample_rate = sample_rate; b->vec_rate = frame_rate; b->avg_alpha = avg_alpha; b->average = average != 0;
        b->decim = decim; b->k = (float)kd;
        int rc = b->init_device(device);
        if (!rc) rc = b->plan.build(fft_size, 1);
        // gr_fft_vcc.cc:55-64: set_window accepts only length 0 or fft_size and the constructor ignores a refusal -- a
        // window of another length leaves the transform unwindowed while k comes from the given values
        if (!rc && wd.size() == (size_t)fft_size) {
            std::vector<float> wf(wd.begin(), wd.end());
            if (!(rc = b->d_window.reserve(wf.size() * 4))) {
                GRHIP_HIP(hipMemcpy(b->d_window.p, wf.data(), wf.size() * 4, hipMemcpyHostToDevice));
                b->has_window = true;
            }
        }
        return rc ? rc : b->restart();
    });
}

}  // namespace

extern "C" {

// window.py:166-176
int grhip_window_blackmanharris(int fft_size, double *out)
{
    if (fft_size > 0 && !out) return fail(GRHIP_EINVAL, "null argument");
    std::vector<double> w;
    if (int rc = blackmanharris(fft_size, w)) return rc;
    if (!w.empty()) memcpy(out, w.data(), w.size() * sizeof(double));
    return GRHIP_OK;
}

int grhip_logpwrfft_c_create(grhip_logpwrfft_c **h, double sample_rate, int fft_size, double ref_scale, double frame_rate,
                             double avg_alpha, int average, const double *window, size_t window_len, int device)
{
    return logpwrfft_create(h, false, sample_rate, fft_size, ref_scale, frame_rate, avg_alpha, average, window, window_len, device);
}
int grhip_logpwrfft_f_create(grhip_logpwrfft_f **h, double sample_rate, int fft_size, double ref_scale, double frame_rate,
                             double avg_alpha, int average, const double *window, size_t window_len, int device)
{
    return logpwrfft_create(h, true, sample_rate, fft_size, ref_scale, frame_rate, avg_alpha, average, window, window_len, device);
}

#define GRHIP_LOGPWRFFT_SETTER(NAME, FN, ARGS, BODY)                                                                    \
    int grhip_##NAME##_##FN ARGS                                                                                        \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        std::lock_guard<std::mutex> lk(h->setter_mutex);                                                               \
        BODY                                                                                                           \
    }

#define GRHIP_LOGPWRFFT_ENTRIES(NAME)                                                                                  \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { return h ? h->set_mode(mode) : fail(GRHIP_EINVAL, "null handle"); } \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams)                                                      \
    {                                                                                                                  \
        return h ? h->set_streams(nstreams, [&] { return h->restart(); }) : fail(GRHIP_EINVAL, "null handle");         \
    }                                                                                                                  \
    /* logpwrfft.py:70-108 */                                                                                          \
    GRHIP_LOGPWRFFT_SETTER(NAME, set_decimation, (grhip_##NAME *h, double decim), return h->set_decim(decim);)         \
    GRHIP_LOGPWRFFT_SETTER(NAME, set_vec_rate, (grhip_##NAME *h, double vec_rate),                                     \
        const double old = h->vec_rate; h->vec_rate = vec_rate;                                                        \
        int rc = h->update_decimator(); if (rc) h->vec_rate = old; return rc;)                                         \
    GRHIP_LOGPWRFFT_SETTER(NAME, set_sample_rate, (grhip_##NAME *h, double sample_rate),                               \
        const double old = h->sample_rate; h->sample_rate = sample_rate;                                               \
        int rc = h->update_decimator(); if (rc) h->sample_rate = old; return rc;)                                      \
    GRHIP_LOGPWRFFT_SETTER(NAME, set_average, (grhip_##NAME *h, int average), h->average = average != 0; return GRHIP_OK;) \
    GRHIP_LOGPWRFFT_SETTER(NAME, set_avg_alpha, (grhip_##NAME *h, double avg_alpha),                                   \
        if (int rc = check_alpha(avg_alpha)) return rc;                                                                \
        h->avg_alpha = avg_alpha; return GRHIP_OK;)                                                                    \
    /* logpwrfft.py:110-138, stream_to_vector_decimator.py:77-93 */                                                    \
    double grhip_##NAME##_sample_rate(grhip_##NAME *h) { return h ? h->sample_rate : NAN; }                            \
    int grhip_##NAME##_decimation(grhip_##NAME *h) { return h ? h->decim : fail(GRHIP_EINVAL, "null handle"); }        \
    double grhip_##NAME##_frame_rate(grhip_##NAME *h) { return h ? h->sample_rate / h->N / h->decim : NAN; }           \
    int grhip_##NAME##_average(grhip_##NAME *h) { return h ? (h->average ? 1 : 0) : fail(GRHIP_EINVAL, "null handle"); } \
    double grhip_##NAME##_avg_alpha(grhip_##NAME *h) { return h ? h->avg_alpha : NAN; }                                \
    int grhip_##NAME##_produced(grhip_##NAME *h, int n_frames)                                                         \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        if (n_frames < 0) return fail(GRHIP_EINVAL, "negative frame count");                                           \
        std::lock_guard<std::mutex> lk(h->setter_mutex);                                                               \
        return (int)h->ctr.produced(n_frames);                                                                         \
    }                                                                                                                  \
    int grhip_##NAME##_state(grhip_##NAME *h, float *out)                                                              \
    {                                                                                                                  \
        if (!h || !out) return fail(GRHIP_EINVAL, "null argument");                                                    \
        int rc = h->bind();                                                                                            \
        if (rc) return rc;                                                                                             \
        std::lock_guard<std::mutex> lk(h->setter_mutex);                                                               \
        if ((rc = h->drain(h->own_stream))) return rc;                                                                 \
        GRHIP_HIP(hipMemcpy(out, h->d_state.p, (size_t)h->nstreams * h->N * sizeof(float), hipMemcpyDeviceToHost));    \
        return GRHIP_OK;                                                                                               \
    }                                                                                                                  \
    int grhip_##NAME##_work(grhip_##NAME *h, int n_frames, const void *in, void *out)                                  \
    {                                                                                                                  \
        return h ? h->work(n_frames, in, out) : fail(GRHIP_EINVAL, "null handle");                                     \
    }                                                                                                                  \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n_frames, const void *d_in, void *d_out, void *stream)         \
    {                                                                                                                  \
        return h ? h->work_device(n_frames, d_in, d_out, stream) : fail(GRHIP_EINVAL, "null handle");                  \
    }

GRHIP_LOGPWRFFT_ENTRIES(logpwrfft_c)
GRHIP_LOGPWRFFT_ENTRIES(logpwrfft_f)

#undef GRHIP_LOGPWRFFT_ENTRIES
#undef GRHIP_LOGPWRFFT_SETTER

}  // extern "C"
