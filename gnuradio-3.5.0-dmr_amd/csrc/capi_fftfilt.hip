// capi_fftfilt.hip -- C ABI for gr_fft_filter_ccc and gr_fft_filter_fff.
// filter/gr_fft_filter_ccc.cc:46-128, filter/gri_fft_filter_ccc_generic.cc:63-170,
// filter/gr_fft_filter_fff.cc:44-97, filter/gri_fft_filter_fff_generic.cc:34-158:
// overlap-ADD fast convolution with the reference's sizes, taps pre-scaled by 1/fftsize,
// tail carried between blocks and calls.  All blocks of a call are transformed in one
// batched launch of the FFT kernels (fft_kernels.hip); the overlap-add + decimation is a
// gather over the inverse transforms.  Up to OLS_MAX_TAPS taps the fused overlap-save kernel on
// 4096-point blocks runs instead (fftfilt4096_kernel, fftfilt4096_pair_kernel).
//
// The reference's fff runs a real-to-complex transform per block; here TWO consecutive real blocks
// share one complex transform (block 2p in the real plane, block 2p+1 in the imaginary one): the
// transformed taps of a real filter are Hermitian, so z = x_a + j x_b comes out as y_a + j y_b with
// nothing to untangle.  One handle template serves both; the traits below are all that differs.
#include <cmath>
#include <complex>
#include <vector>

#include "fft_kernels.h"
#include "grhip_internal.h"

using namespace grhip;

struct FftFiltCcc {
    using item = float2;
    using tap = std::complex<float>;
    static constexpr const char *name = "fft_filter_ccc";
    static std::complex<float> cplx(tap t) { return t; }
    static constexpr int blocks_per_xform = 1;
    // a fused ccc handle still builds the overlap-add plan and spectrum it never runs
    static constexpr bool fused_needs_ola = true;
    static constexpr auto fused = launch_fftfilt4096;
    static constexpr auto pack = launch_fftfilt_pack;
    static constexpr auto ola = launch_fftfilt_ola;
    static constexpr auto tail = launch_fftfilt_tail;
};

struct FftFiltFff {
    using item = float;
    using tap = float;
    static constexpr const char *name = "fft_filter_fff";
    static std::complex<float> cplx(tap t) { return {t, 0.f}; }      // imaginary parts zero: H Hermitian
    static constexpr int blocks_per_xform = 2;
    // a fused fff handle has no overlap-add plan and no spectrum
    static constexpr bool fused_needs_ola = false;
    static constexpr auto fused = launch_fftfilt4096_pair;
    static constexpr auto pack = launch_fftfilt_pack_real;
    static constexpr auto ola = launch_fftfilt_ola_real;
    static constexpr auto tail = launch_fftfilt_tail_real;
};

template <class T>
struct FftFilter : HandleBase {
    using item = typename T::item;
    using tap = typename T::tap;
    int decim = 1, ntaps = 0, fftsize = 0, nsamples = 0;
    std::vector<tap> new_taps;
    bool updated = false;
    DevBuf d_xformed, d_tail, d_a, d_b;
    FftPlan plan;              // the fftsize-point transform, both directions (four-step form above 8192 points)
    // fused overlap-save path (ntaps <= OLS_MAX_TAPS): 4096-point blocks
    bool fused = false;
    int L = 0, fold = 0;             // full-rate outputs per block (a multiple of the decimation); folded inverse
    DevBuf d_tw4096, d_H4096, d_hist[2];
    int hist_cur = 0;

    int install(const tap *taps, size_t n)
    {
        // compute_sizes + set_taps (gri_fft_filter_ccc_generic.cc:63-118, gri_fft_filter_fff_generic.cc:51-105)
        ntaps = (int)n;
        fftsize = (int)(2 * pow(2.0, ceil(log((double)ntaps) / log(2.0))));
        nsamples = fftsize - ntaps + 1;
        if (ntaps > (1 << 25) || !FftPlan::size_ok(fftsize))
            return fail(GRHIP_EINVAL, "%s: %d taps need an FFT of more than 2^26 points", T::name, ntaps);
        fused = ntaps <= OLS_MAX_TAPS && ((OLS_N - (ntaps - 1)) / decim) >= 1;
        const bool ola = !fused || T::fused_needs_ola;
        int rc;
        if (ola && (rc = plan.build(fftsize, 1))) return rc;
        std::vector<std::complex<float>> tc((size_t)ntaps);
        for (int i = 0; i < ntaps; ++i) tc[(size_t)i] = T::cplx(taps[i]);
        const size_t hl = (size_t)(ntaps > 1 ? ntaps - 1 : 1);                          // history / tail items
        if (fused) {
            rc = ols_build((const float *)tc.data(), ntaps, decim, d_tw4096, d_H4096, &L, &fold);
            if (!rc) rc = d_hist[0].reserve(hl * sizeof(item));
            if (!rc) rc = d_hist[1].reserve(hl * sizeof(item));
            if (rc) return rc;
            if ((rc = zero_device(d_hist[0].p, hl * sizeof(item)))) return rc;          // a fresh filter starts from silence
            if ((rc = zero_device(d_hist[1].p, hl * sizeof(item)))) return rc;
            hist_cur = 0;
        }
        if (!ola) return GRHIP_OK;
        // forward transform of the scaled, zero-padded taps (double, rounded once)
        const float scale = 1.0 / fftsize;                                              // ccc :76, fff :63
        std::vector<std::complex<double>> t((size_t)fftsize, std::complex<double>(0, 0));
        for (int i = 0; i < ntaps; ++i)
            t[i] = std::complex<double>((double)(tc[i].real() * scale), (double)(tc[i].imag() * scale));
        host_fft_pow2(t, -1);
        std::vector<float2> H((size_t)fftsize);
        for (int k = 0; k < fftsize; ++k) H[k] = make_float2((float)t[k].real(), (float)t[k].imag());
        rc = d_xformed.reserve(H.size() * sizeof(float2));
        if (!rc) rc = d_tail.reserve(hl * sizeof(item));
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(d_xformed.p, H.data(), H.size() * sizeof(float2), hipMemcpyHostToDevice));
        return zero_device(d_tail.p, hl * sizeof(item));                                // tail cleared (ccc :69-71, fff :56-58)
    }

    int set_taps(const tap *taps, size_t n)
    {
        new_taps.assign(taps, taps + n);
        updated = true;                                  // gr_fft_filter_ccc.cc:88-93, gr_fft_filter_fff.cc:69-73
        return GRHIP_OK;
    }

    int work_device(int noutput_items, const void *d_in, void *d_out, void *stream)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        int rc = bind();
        if (rc) return rc;
        hipStream_t st = pick(stream);
        if (updated) {                                   // ccc .cc:113-118, fff .cc:83-88: new sizes, produce nothing this call
            if ((rc = drain(st))) return rc;
            rc = install(new_taps.data(), new_taps.size());
            if (rc) return rc;
            updated = false;
            return 0;
        }
        if (noutput_items == 0) return 0;
        if (noutput_items % nsamples)
            return fail(GRHIP_EINVAL, "noutput_items must be a multiple of nsamples (%d)", nsamples);
        const long long nin = (long long)noutput_items * decim;
        if (fused) {
            if ((rc = T::fused((const item *)d_in, nin, d_hist[hist_cur].as<item>(), ntaps, d_tw4096.as<float2>(),
                               d_H4096.as<float2>(), (item *)d_out, noutput_items, decim, L, fold, st,
                               d_hist[hist_cur ^ 1].as<item>())))
                return rc;
            hist_cur ^= 1;
            return noutput_items;
        }
        // nblk blocks of the stream, T::blocks_per_xform of them per complex transform
        const long long nblk = nin / nsamples, ncb = (nblk + T::blocks_per_xform - 1) / T::blocks_per_xform;
        const size_t bytes = (size_t)ncb * fftsize * sizeof(float2);
        if ((rc = d_a.reserve(bytes))) return rc;
        if ((rc = d_b.reserve(bytes))) return rc;
        float2 *A = d_a.as<float2>(), *B = d_b.as<float2>();
        const int tailsize = ntaps - 1;
        if ((rc = T::pack((const item *)d_in, A, nsamples, fftsize, nblk, st))) return rc;
        if ((rc = plan.exec_pow2(1, 0, nullptr, A, B, ncb, st))) return rc;
        if ((rc = launch_fftfilt_mul(B, d_xformed.as<float2>(), fftsize, ncb, st))) return rc;
        if ((rc = plan.exec_pow2(0, 0, nullptr, B, A, ncb, st))) return rc;
        if ((rc = T::ola(A, d_tail.as<item>(), (item *)d_out, noutput_items, decim, nsamples, fftsize, tailsize, st)))
            return rc;
        if ((rc = T::tail(A, d_tail.as<item>(), nblk, nsamples, fftsize, tailsize, st))) return rc;
        return noutput_items;
    }

    int work(int noutput_items, const void *in, void *out)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        int rc = bind();
        if (rc) return rc;
        if (updated || noutput_items == 0) return work_device(noutput_items, nullptr, nullptr, own_stream);
        const size_t nin = (size_t)noutput_items * decim, sz = sizeof(item);
        return (int)host_call(in, nin * sz, nin * sz, (size_t)noutput_items * sz, out, sz, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(noutput_items, d_in, d_out, st);
        });
    }
};
struct grhip_fft_filter_ccc : FftFilter<FftFiltCcc> {};
struct grhip_fft_filter_fff : FftFilter<FftFiltFff> {};

template <class H>
static int fftfilt_create(H **h, const char *name, int decimation, const float *taps, size_t ntaps, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (decimation < 1) return fail(GRHIP_EINVAL, "decimation must be >= 1");
    if (!taps || ntaps < 1) return fail(GRHIP_EINVAL, "%s needs at least one tap", name);
    return make_handle(h, [&](H *f) {
        f->decim = decimation;
        int rc = f->init_device(device);
        if (!rc) rc = f->install((const typename H::tap *)taps, ntaps);
        return rc;
    });
}

extern "C" {

// `taps` holds ntaps taps of the block's tap type (ccc: interleaved complex floats)
#define GRHIP_FFTFILT_ENTRIES(NAME)                                                                                    \
    int grhip_##NAME##_create(grhip_##NAME **h, int decimation, const float *taps, size_t ntaps, int device)          \
    {                                                                                                                  \
        return fftfilt_create(h, #NAME, decimation, taps, ntaps, device);                                             \
    }                                                                                                                  \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                                \
    int grhip_##NAME##_set_taps(grhip_##NAME *h, const float *taps, size_t ntaps)                                     \
    {                                                                                                                  \
        if (!h || !taps || ntaps < 1) return fail(GRHIP_EINVAL, "bad argument");                                      \
        return h->set_taps((const grhip_##NAME::tap *)taps, ntaps);                                                   \
    }                                                                                                                  \
    int grhip_##NAME##_nsamples(const grhip_##NAME *h) { return h ? h->nsamples : GRHIP_EINVAL; }                      \
    int grhip_##NAME##_decimation(const grhip_##NAME *h) { return h ? h->decim : GRHIP_EINVAL; }                       \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int noutput_items, const void *d_in, void *d_out, void *stream)   \
    {                                                                                                                  \
        return h ? h->work_device(noutput_items, d_in, d_out, stream) : fail(GRHIP_EINVAL, "null handle");            \
    }                                                                                                                  \
    int grhip_##NAME##_work(grhip_##NAME *h, int noutput_items, const void *in, void *out)                            \
    {                                                                                                                  \
        return h ? h->work(noutput_items, in, out) : fail(GRHIP_EINVAL, "null handle");                               \
    }
GRHIP_FFTFILT_ENTRIES(fft_filter_ccc)
GRHIP_FFTFILT_ENTRIES(fft_filter_fff)

}  // extern "C"
