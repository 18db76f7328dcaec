// capi_spectrum.hip -- C ABI of the spectrum-estimate blocks: gr_complex_to_mag_squared, gr_single_pole_iir_filter_ff,
// gr_nlog10_ff and gr_keep_one_in_n, the stages of blks2.logpwrfft behind its transform.
//
// Reference: general/gr_complex_to_xxx.cc:180-203; filter/gr_single_pole_iir.h:60-97,
// filter/gr_single_pole_iir_filter_ff.cc:53-81; general/gr_nlog10_ff.cc:49-64; general/gr_keep_one_in_n.cc:52-105.
//
// Every block takes S streams back to back ([S][items]); what a block remembers (the IIR's outputs, the keep-one
// countdown) is kept per handle, the IIR's per (stream, element).  set_streams restarts a block from the reference's
// initial state; set_mode and the tap setters keep the state.
#include <cmath>

#include "grhip_internal.h"
#include "spectrum.h"
#include "stream_block.h"

using namespace grhip;

namespace {

int check_alpha(double alpha)
{
    // gr_single_pole_iir.h:62-63 (a NaN passes there; it is refused here)
    return (alpha >= 0.0 && alpha <= 1.0) ? GRHIP_OK : fail(GRHIP_ERANGE, "Alpha must be in [0, 1]");
}

}  // namespace

// ---- the element-wise blocks and the IIR: items of vlen floats (mag^2: vlen complex in); in-place calls are allowed ---
struct SpectrumBlock : StreamBlock {
    int vlen = 1;
    virtual ~SpectrumBlock() = default;
    virtual size_t in_elem() const { return 4; }
    virtual int launch(int n, const void *d_in, void *d_out, hipStream_t st) = 0;     // under setter_mutex

    int work_device(int noutput_items, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(noutput_items);
        if (c <= 0) return c;
        int rc = check_io(d_in, in_elem(), d_out, 4);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = launch(noutput_items, d_in, d_out, pick(stream)))) return rc;
        return noutput_items;
    }

    int work(int noutput_items, const void *in, void *out)
    {
        const size_t in_item = (size_t)vlen * in_elem(), out_item = (size_t)vlen * 4;
        const int rc = host_work(noutput_items, in_item, in, (size_t)noutput_items, out_item, out, 0, [&](void *d_in, void *d_out, hipStream_t s) {
            const int r = work_device(noutput_items, d_in, d_out, s);
            return r < 0 ? r : GRHIP_OK;
        });
        return rc ? rc : noutput_items;
    }

    virtual int restart() { return GRHIP_OK; }      // after nstreams changed, under setter_mutex, streams drained

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
    }
};

struct grhip_complex_to_mag_squared : SpectrumBlock {
    size_t in_elem() const override { return 8; }
    int launch(int n, const void *d_in, void *d_out, hipStream_t st) override
    {
        return mag_squared_launch((const float2 *)d_in, (float *)d_out, (long long)nstreams * n * vlen, st);
    }
};

struct grhip_complex_to_mag : SpectrumBlock {
    size_t in_elem() const override { return 8; }
    int launch(int n, const void *d_in, void *d_out, hipStream_t st) override
    {
        return mag_launch((const float2 *)d_in, (float *)d_out, (long long)nstreams * n * vlen, st);
    }
};

struct grhip_nlog10_ff : SpectrumBlock {
    float n = 1.f, k = 0.f;
    int launch(int count, const void *d_in, void *d_out, hipStream_t st) override
    {
        return nlog10_launch((const float *)d_in, (float *)d_out, (long long)nstreams * count * vlen, n, k, st);
    }
};

struct grhip_single_pole_iir_filter_ff : SpectrumBlock {
    double alpha = 1.0;
    DevBuf d_state, d_scratch;

    int restart() override
    {
        const size_t b = (size_t)nstreams * vlen * sizeof(float);
        int rc = d_state.reserve(b);
        return rc ? rc : zero_device(d_state.p, b);
    }

    int launch(int n, const void *d_in, void *d_out, hipStream_t st) override
    {
        IirLaunch a;
        a.in = (const float *)d_in; a.out = (float *)d_out; a.n = n;
        a.nstreams = nstreams; a.vlen = vlen; a.alpha = alpha; a.state = d_state.as<float>();
        return single_pole_iir_launch(mode_fast(mode), a, d_scratch, st);
    }

    int set_taps(double a)
    {
        if (int rc = check_alpha(a)) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        alpha = a;                                      // a kernel argument: launches already queued keep theirs
        return GRHIP_OK;
    }
};

// items of any size at any address (the launcher picks the word it copies by), in place or not; the mode is not used
struct grhip_keep_one_in_n : StreamBlock {
    size_t item_size = 4;
    KeepOne ctr;

    int work_device(int n_in, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n_in);
        if (c <= 0) return c;
        int rc = check_io(d_in, 1, d_out, 1);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        const long long p = ctr.produced(n_in);
        if ((rc = keep_one_launch(d_in, d_out, item_size, n_in, p, ctr.first(), ctr.n, nstreams, pick(stream)))) return rc;
        ctr.advance(n_in);
        return (int)p;
    }

    int work(int n_in, const void *in, void *out)
    {
        // not host_work: the call returns the count that work_device reports, known only under its lock
        const int c = check_count(n_in);
        if (c <= 0) return c;
        if (!in || !out) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        const size_t bytes = (size_t)nstreams * (size_t)n_in * item_size;
        return (int)host_call(in, bytes, bytes + 16, bytes + 16, out, item_size * nstreams,
                              [&](void *d_in, void *d_out, hipStream_t s) -> long long {
                                  return work_device(n_in, d_in, d_out, s);
                              });
    }
};

namespace {

template <class H, class Set>
int create_vlen(H **h, int vlen, int device, Set &&set)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (vlen < 1) return fail(GRHIP_EINVAL, "vlen must be at least 1");
    return make_handle(h, [&](H *b) {
        b->vlen = vlen;
        b->mode = default_mode();
        set(b);
        int rc = b->init_device(device);
        return rc ? rc : b->restart();
    });
}

}  // namespace

extern "C" {

#define GRHIP_SPECTRUM_COMMON(NAME)                                                                                    \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_work(grhip_##NAME *h, int noutput_items, const void *in, void *out)                             \
    {                                                                                                                  \
        return h ? h->work(noutput_items, in, out) : fail(GRHIP_EINVAL, "null handle");                                \
    }                                                                                                                  \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int noutput_items, const void *d_in, void *d_out, void *stream)    \
    {                                                                                                                  \
        return h ? h->work_device(noutput_items, d_in, d_out, stream) : fail(GRHIP_EINVAL, "null handle");             \
    }

#define GRHIP_SPECTRUM_VLEN(NAME)                                                                                      \
    GRHIP_SPECTRUM_COMMON(NAME)                                                                                        \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { return h ? h->set_mode(mode) : fail(GRHIP_EINVAL, "null handle"); } \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams)                                                      \
    {                                                                                                                  \
        return h ? h->set_streams(nstreams) : fail(GRHIP_EINVAL, "null handle");                                       \
    }

// ---- gr_complex_to_mag_squared (gr_complex_to_xxx.cc:180-203) -----------------------------------------------------------
int grhip_complex_to_mag_squared_create(grhip_complex_to_mag_squared **h, int vlen, int device)
{
    return create_vlen(h, vlen, device, [](grhip_complex_to_mag_squared *) {});
}
GRHIP_SPECTRUM_VLEN(complex_to_mag_squared)

// ---- gr_complex_to_mag (gr_complex_to_xxx.cc, the std::abs loop) --------------------------------------------------------
int grhip_complex_to_mag_create(grhip_complex_to_mag **h, int vlen, int device)
{
    return create_vlen(h, vlen, device, [](grhip_complex_to_mag *) {});
}
GRHIP_SPECTRUM_VLEN(complex_to_mag)

// ---- gr_single_pole_iir_filter_ff (gr_single_pole_iir_filter_ff.cc:32-81) ----------------------------------------------
int grhip_single_pole_iir_filter_ff_create(grhip_single_pole_iir_filter_ff **h, double alpha, int vlen, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (int rc = check_alpha(alpha)) return rc;
    return create_vlen(h, vlen, device, [&](grhip_single_pole_iir_filter_ff *b) { b->alpha = alpha; });
}
GRHIP_SPECTRUM_VLEN(single_pole_iir_filter_ff)
int grhip_single_pole_iir_filter_ff_set_taps(grhip_single_pole_iir_filter_ff *h, double alpha)
{
    return h ? h->set_taps(alpha) : fail(GRHIP_EINVAL, "null handle");
}
int grhip_single_pole_iir_filter_ff_chunk(void) { return IIR_CHUNK; }

// ---- gr_nlog10_ff (gr_nlog10_ff.cc:31-64) --------------------------------------------------------------------------------
int grhip_nlog10_ff_create(grhip_nlog10_ff **h, float n, int vlen, float k, int device)
{
    return create_vlen(h, vlen, device, [&](grhip_nlog10_ff *b) { b->n = n; b->k = k; });
}
GRHIP_SPECTRUM_VLEN(nlog10_ff)

// ---- gr_keep_one_in_n (gr_keep_one_in_n.cc:31-105) -----------------------------------------------------------------------
int grhip_keep_one_in_n_create(grhip_keep_one_in_n **h, size_t item_size, int n, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (item_size < 1) return fail(GRHIP_EINVAL, "keep_one_in_n: item_size must be at least 1");
    return make_handle(h, [&](grhip_keep_one_in_n *b) {
        b->item_size = item_size;
        b->ctr.set_n(n);
        return b->init_device(device);
    });
}
GRHIP_SPECTRUM_COMMON(keep_one_in_n)
int grhip_keep_one_in_n_set_n(grhip_keep_one_in_n *h, int n)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    h->ctr.set_n(n);
    return GRHIP_OK;
}
int grhip_keep_one_in_n_set_streams(grhip_keep_one_in_n *h, int nstreams)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (int rc = check_streams(nstreams)) return rc;
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    h->nstreams = nstreams;
    h->ctr.set_n(h->ctr.n);
    return GRHIP_OK;
}
int grhip_keep_one_in_n_produced(grhip_keep_one_in_n *h, int n_in)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (n_in < 0) return fail(GRHIP_EINVAL, "negative item count");
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    return (int)h->ctr.produced(n_in);
}

#undef GRHIP_SPECTRUM_VLEN
#undef GRHIP_SPECTRUM_COMMON

}  // extern "C"
