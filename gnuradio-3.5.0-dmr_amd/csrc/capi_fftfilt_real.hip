// capi_fftfilt_real.hip -- C ABI for gr_fft_filter_fff.
// filter/gr_fft_filter_fff.cc:44-97, filter/gri_fft_filter_fff_generic.cc:34-158:
// overlap-ADD fast convolution of a float stream with float taps, the reference's sizes, taps
// pre-scaled by 1/fftsize, tail carried between blocks and calls.  The reference runs a
// real-to-complex transform per block; here TWO consecutive real blocks share one complex
// transform (block 2p in the real plane, block 2p+1 in the imaginary one): the transformed taps of
// a real filter are Hermitian, so z = x_a + j x_b comes out as y_a + j y_b with nothing to untangle.
// Up to OLS_MAX_TAPS taps that is the fused overlap-save kernel (fftfilt4096_pair_kernel), beyond it
// the batched overlap-add of capi_fftfilt.hip on packed block pairs.
#include <cmath>
#include <complex>
#include <vector>

#include "fft_kernels.h"
#include "grhip_internal.h"

using namespace grhip;

struct grhip_fft_filter_fff : HandleBase {
    int decim = 1, ntaps = 0, fftsize = 0, nsamples = 0;
    std::vector<float> new_taps;
    bool updated = false;
    DevBuf d_xformed, d_tail, d_a, d_b;
    FftPlan plan;              // the fftsize-point transform, both directions (four-step form above 8192 points)
    // fused overlap-save path (ntaps <= OLS_MAX_TAPS): 4096-point blocks in pairs, see fftfilt4096_pair_kernel
    bool fused = false;
    int L = 0, fold = 0;             // full-rate outputs per block (a multiple of the decimation); folded inverse
    DevBuf d_tw4096, d_H4096, d_hist[2];
    int hist_cur = 0;

    int install(const float *taps, size_t n)
    {
        // compute_sizes + set_taps (gri_fft_filter_fff_generic.cc:51-105)
        ntaps = (int)n;
        fftsize = (int)(2 * pow(2.0, ceil(log((double)ntaps) / log(2.0))));              // :89
        nsamples = fftsize - ntaps + 1;                                                  // :90
        if (ntaps > (1 << 25) || !FftPlan::size_ok(fftsize))
            return fail(GRHIP_EINVAL, "fft_filter_fff: %d taps need an FFT of more than 2^26 points", ntaps);
        fused = ntaps <= OLS_MAX_TAPS && ((OLS_N - (ntaps - 1)) / decim) >= 1;
        const size_t hl = (size_t)(ntaps > 1 ? ntaps - 1 : 1);
        if (fused) {
            std::vector<float> tc(2 * (size_t)ntaps, 0.f);                               // imaginary parts zero: H Hermitian
            for (int i = 0; i < ntaps; ++i) tc[2 * (size_t)i] = taps[i];
            int rc = ols_build(tc.data(), ntaps, decim, d_tw4096, d_H4096, &L, &fold);
            if (!rc) rc = d_hist[0].reserve(hl * sizeof(float));
            if (!rc) rc = d_hist[1].reserve(hl * sizeof(float));
            if (rc) return rc;
            if ((rc = zero_device(d_hist[0].p, hl * sizeof(float)))) return rc;          // a fresh filter starts from silence
            if ((rc = zero_device(d_hist[1].p, hl * sizeof(float)))) return rc;
            hist_cur = 0;
            return GRHIP_OK;
        }
        int rc = plan.build(fftsize, 1);
        if (rc) return rc;
        // forward transform of the scaled, zero-padded taps (double, rounded once): the full Hermitian spectrum
        const float scale = 1.0 / fftsize;                                               // :63
        std::vector<std::complex<double>> t((size_t)fftsize, std::complex<double>(0, 0));
        for (int i = 0; i < ntaps; ++i) t[i] = std::complex<double>((double)(taps[i] * scale), 0.0);
        host_fft_pow2(t, -1);
        std::vector<float2> H((size_t)fftsize);
        for (int k = 0; k < fftsize; ++k) H[k] = make_float2((float)t[k].real(), (float)t[k].imag());
        rc = d_xformed.reserve(H.size() * sizeof(float2));
        if (!rc) rc = d_tail.reserve(hl * sizeof(float));
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(d_xformed.p, H.data(), H.size() * sizeof(float2), hipMemcpyHostToDevice));
        return zero_device(d_tail.p, hl * sizeof(float));                                // tail cleared (:56-58)
    }
    void release_all()
    {
        plan.release(); d_xformed.release(); d_tail.release(); d_a.release(); d_b.release();
        d_tw4096.release(); d_H4096.release(); d_hist[0].release(); d_hist[1].release();
    }
};

extern "C" {

int grhip_fft_filter_fff_create(grhip_fft_filter_fff **h, int decimation, const float *taps, size_t ntaps, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (decimation < 1) return fail(GRHIP_EINVAL, "decimation must be >= 1");
    if (!taps || ntaps < 1) return fail(GRHIP_EINVAL, "fft_filter_fff needs at least one tap");
    auto *f = new (std::nothrow) grhip_fft_filter_fff();
    if (!f) return fail(GRHIP_ENOMEM, "alloc");
    f->decim = decimation;
    int rc = f->init_device(device);
    if (!rc) rc = f->install(taps, ntaps);
    if (rc) { f->release_all(); f->destroy_base(); delete f; return rc; }
    *h = f;
    return GRHIP_OK;
}

void grhip_fft_filter_fff_destroy(grhip_fft_filter_fff *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    h->release_all();
    h->destroy_base();
    delete h;
}

int grhip_fft_filter_fff_set_taps(grhip_fft_filter_fff *h, const float *taps, size_t ntaps)
{
    if (!h || !taps || ntaps < 1) return fail(GRHIP_EINVAL, "bad argument");
    h->new_taps.assign(taps, taps + ntaps);
    h->updated = true;                                   // gr_fft_filter_fff.cc:69-73
    return GRHIP_OK;
}

int grhip_fft_filter_fff_nsamples(const grhip_fft_filter_fff *h) { return h ? h->nsamples : GRHIP_EINVAL; }
int grhip_fft_filter_fff_decimation(const grhip_fft_filter_fff *h) { return h ? h->decim : GRHIP_EINVAL; }

int grhip_fft_filter_fff_work_device(grhip_fft_filter_fff *h, int noutput_items, const void *d_in, void *d_out,
                                     void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    int rc = h->bind();
    if (rc) return rc;
    hipStream_t st = h->pick(stream);
    if (h->updated) {                                    // .cc:83-88: new sizes, produce nothing this call
        if ((rc = h->drain(st))) return rc;
        rc = h->install(h->new_taps.data(), h->new_taps.size());
        if (rc) return rc;
        h->updated = false;
        return 0;
    }
    if (noutput_items == 0) return 0;
    if (noutput_items % h->nsamples)                     // .cc:90
        return fail(GRHIP_EINVAL, "noutput_items must be a multiple of nsamples (%d)", h->nsamples);
    const long long nin = (long long)noutput_items * h->decim;
    if (h->fused) {
        const float *hist = h->d_hist[h->hist_cur].as<float>();
        float *hist_new = h->d_hist[h->hist_cur ^ 1].as<float>();
        if ((rc = launch_fftfilt4096_pair((const float *)d_in, nin, hist, h->ntaps, h->d_tw4096.as<float2>(),
                                          h->d_H4096.as<float2>(), (float *)d_out, noutput_items, h->decim, h->L, h->fold,
                                          st, hist_new)))
            return rc;
        h->hist_cur ^= 1;
        return noutput_items;
    }
    const long long nblk = nin / h->nsamples, ncb = (nblk + 1) / 2;       // real blocks, complex blocks
    const size_t bytes = (size_t)ncb * h->fftsize * sizeof(float2);
    if ((rc = h->d_a.reserve(bytes))) return rc;
    if ((rc = h->d_b.reserve(bytes))) return rc;
    float2 *A = h->d_a.as<float2>(), *B = h->d_b.as<float2>();
    const int tailsize = h->ntaps - 1;
    if ((rc = launch_fftfilt_pack_real((const float *)d_in, A, h->nsamples, h->fftsize, nblk, st))) return rc;
    if ((rc = h->plan.exec_pow2(1, 0, nullptr, A, B, ncb, st))) return rc;
    if ((rc = launch_fftfilt_mul(B, h->d_xformed.as<float2>(), h->fftsize, ncb, st))) return rc;
    if ((rc = h->plan.exec_pow2(0, 0, nullptr, B, A, ncb, st))) return rc;
    if ((rc = launch_fftfilt_ola_real(A, h->d_tail.as<float>(), (float *)d_out, noutput_items, h->decim, h->nsamples,
                                      h->fftsize, tailsize, st)))
        return rc;
    if ((rc = launch_fftfilt_tail_real(A, h->d_tail.as<float>(), nblk, h->nsamples, h->fftsize, tailsize, st))) return rc;
    return noutput_items;
}

int grhip_fft_filter_fff_work(grhip_fft_filter_fff *h, int noutput_items, const void *in, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    int rc = h->bind();
    if (rc) return rc;
    if (h->updated || noutput_items == 0)
        return grhip_fft_filter_fff_work_device(h, noutput_items, nullptr, nullptr, h->own_stream);
    const size_t nin = (size_t)noutput_items * h->decim;
    return (int)h->host_call(in, nin * 4, nin * 4, (size_t)noutput_items * 4, out, 4, [&](void *d_in, void *d_out, hipStream_t st) {
        return grhip_fft_filter_fff_work_device(h, noutput_items, d_in, d_out, st);
    });
}

}  // extern "C"
