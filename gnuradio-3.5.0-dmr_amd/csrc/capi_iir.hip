// capi_iir.hip -- C ABI of gr_iir_filter_ffd.
//
// Reference: filter/gr_iir_filter_ffd.cc:56-82 (work applies a pending set_taps first), filter/gri_iir.h:90-163
// (set_taps zeroes both delay lines; filter() is the recurrence).
//
// A handle takes S streams back to back ([S][n_in]).  What a stream remembers is its delay lines on the device: the
// last n - 1 inputs as float and the last m - 1 accumulators as double.  The taps live on the device too; set_taps is
// latched and applied, with the delay lines zeroed, at the start of the next work call.
#include <cmath>
#include <vector>

#include "grhip_internal.h"
#include "stream_block.h"
#include "iir.h"

using namespace grhip;

namespace {

struct IirBlock : StreamBlock {
    std::vector<double> ff, fb;             // the taps in force
    std::vector<double> new_ff, new_fb;     // latched by set_taps
    bool updated = false;
    bool can_chunk = false;                 // of the taps in force
    IirCarry carry = {};
    DevBuf d_taps, d_x, d_y, d_scratch;

    static int check_taps(const double *fft, size_t n, const double *fbt, size_t m)
    {
        if ((n && !fft) || (m && !fbt)) return fail(GRHIP_EINVAL, "null taps");
        if (n > (size_t)IIR_MAX_TAPS || m > (size_t)IIR_MAX_TAPS)
            return fail(GRHIP_EINVAL, "iir_filter_ffd: at most %d taps on either side", IIR_MAX_TAPS);
        if (n > 0 && m == 0)
            return fail(GRHIP_EINVAL, "iir_filter_ffd: feed-forward taps need at least one feedback tap (fbtaps[0] is never read)");
        return GRHIP_OK;
    }

    int zero_state()
    {
        int rc;
        if ((rc = d_x.reserve((size_t)nstreams * IIR_HIST * sizeof(float)))) return rc;
        if ((rc = d_y.reserve((size_t)nstreams * IIR_HIST * sizeof(double)))) return rc;
        if ((rc = zero_device(d_x.p, (size_t)nstreams * IIR_HIST * sizeof(float)))) return rc;
        return zero_device(d_y.p, (size_t)nstreams * IIR_HIST * sizeof(double));
    }

    // gri_iir.h:90-111: the taps and two zeroed delay lines; streams drained, under setter_mutex
    int install(const std::vector<double> &f, const std::vector<double> &b)
    {
        ff = f; fb = b;
        can_chunk = iir_plan(ff, fb, &carry);
        int rc = d_taps.reserve(2 * IIR_MAX_TAPS * sizeof(double));
        if (rc) return rc;
        std::vector<double> t(2 * IIR_MAX_TAPS, 0.0);
        std::copy(ff.begin(), ff.end(), t.begin());
        std::copy(fb.begin(), fb.end(), t.begin() + IIR_MAX_TAPS);
        GRHIP_HIP(hipMemcpy(d_taps.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
        return zero_state();
    }

    int init(const double *fft, size_t n, const double *fbt, size_t m, int dev)
    {
        int rc = check_taps(fft, n, fbt, m);
        if (rc) return rc;
        mode = default_mode();
        if ((rc = init_device(dev))) return rc;
        return install(std::vector<double>(fft, fft + n), std::vector<double>(fbt, fbt + m));
    }

    int set_taps(const double *fft, size_t n, const double *fbt, size_t m)
    {
        int rc = check_taps(fft, n, fbt, m);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        new_ff.assign(fft, fft + n);
        new_fb.assign(fbt, fbt + m);
        updated = true;
        return GRHIP_OK;
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return zero_state(); });
    }

    int chunked()
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        if (!mode_fast(mode)) return 0;
        return (updated ? iir_plan(new_ff, new_fb, nullptr) : can_chunk) ? 1 : 0;
    }

    int work_device(int n_in, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n_in);
        if (c <= 0) return c;
        const size_t bytes = (size_t)nstreams * (size_t)n_in * sizeof(float);
        int rc;
        if ((rc = check_io(d_in, sizeof(float), d_out, sizeof(float))) || (rc = check_apart("iir_filter_ffd", d_in, bytes, d_out, bytes)))
            return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        if (updated) {                                                  // gr_iir_filter_ffd.cc:66-69
            if ((rc = drain(st))) return rc;
            if ((rc = install(new_ff, new_fb))) return rc;
            updated = false;
        }
        if (ff.empty()) {                                               // gri_iir.h:135-136: zeros, no state touched
            GRHIP_HIP(hipMemsetAsync(d_out, 0, bytes, st));
            return GRHIP_OK;
        }
        IirLaunch l;
        l.in = (const float *)d_in; l.out = (float *)d_out; l.in_stride = l.out_stride = n_in; l.n_items = n_in; l.nstreams = nstreams;
        l.n = (int)ff.size(); l.m = (int)fb.size();
        l.taps = d_taps.as<double>(); l.xstate = d_x.as<float>(); l.ystate = d_y.as<double>();
        if (mode_fast(mode) && can_chunk && n_in > IIR_CHUNK) {
            if ((rc = d_scratch.reserve(iir_scratch_bytes(l)))) return rc;
            return iir_chunked_launch(l, carry, d_scratch.p, st);
        }
        return iir_walk_launch(l, st);
    }

    int work(int n_in, const void *in, void *out)
    {
        return host_work(n_in, sizeof(float), in, (size_t)n_in, sizeof(float), out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n_in, d_in, d_out, st);
        });
    }
};

}  // namespace

struct grhip_iir_filter_ffd : IirBlock {};

extern "C" {

#define GRHIP_IIR_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")

int grhip_iir_filter_ffd_create(grhip_iir_filter_ffd **h, const double *fftaps, size_t n, const double *fbtaps, size_t m,
                                int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    int rc = IirBlock::check_taps(fftaps, n, fbtaps, m);
    if (rc) return rc;
    return make_handle(h, [&](grhip_iir_filter_ffd *b) { return b->init(fftaps, n, fbtaps, m, device); });
}

void grhip_iir_filter_ffd_destroy(grhip_iir_filter_ffd *h) { destroy_handle(h); }

int grhip_iir_filter_ffd_set_taps(grhip_iir_filter_ffd *h, const double *fftaps, size_t n, const double *fbtaps, size_t m)
{
    GRHIP_IIR_NULL(h);
    return h->set_taps(fftaps, n, fbtaps, m);
}

int grhip_iir_filter_ffd_set_mode(grhip_iir_filter_ffd *h, int mode) { GRHIP_IIR_NULL(h); return h->set_mode(mode); }
int grhip_iir_filter_ffd_set_streams(grhip_iir_filter_ffd *h, int nstreams) { GRHIP_IIR_NULL(h); return h->set_streams(nstreams); }
int grhip_iir_filter_ffd_chunked(grhip_iir_filter_ffd *h) { GRHIP_IIR_NULL(h); return h->chunked(); }

int grhip_iir_filter_ffd_work(grhip_iir_filter_ffd *h, int n_in, const void *in, void *out)
{
    GRHIP_IIR_NULL(h);
    return h->work(n_in, in, out);
}

int grhip_iir_filter_ffd_work_device(grhip_iir_filter_ffd *h, int n_in, const void *d_in, void *d_out, void *stream)
{
    GRHIP_IIR_NULL(h);
    return h->work_device(n_in, d_in, d_out, stream);
}

int grhip_iir_filter_ffd_chunk(void) { return IIR_CHUNK; }

#undef GRHIP_IIR_NULL

}  // extern "C"
