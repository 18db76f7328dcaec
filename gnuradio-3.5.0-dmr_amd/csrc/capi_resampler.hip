// capi_resampler.hip -- gr_rational_resampler_base_XXX and gr_interp_fir_filter_XXX (ccf, fff, ccc), and
// gr_pfb_interpolator_ccf: handles and C ABI.
//
// Reference (gnuradio-core/src/lib/filter/):
//   gr_rational_resampler_base_XXX.cc.t:49-72 (constructor: I or D == 0 throws std::out_of_range), 83-120 (set_taps:
//   zeros in FRONT of the taps up to a multiple of I; install_taps: nt = len/I, filter n gets taps[n + k*I]),
//   135-141 (forecast), 144-172 (general_work: the ctr walk, consume_each(in - in0)); .h.t:51,72-73 (its own
//   d_history / history() / set_history(), which hide gr_block's: the scheduler sees history 1, no zeros in front).
//   gr_interp_fir_filter_XXX.cc.t:72-109 (the same bank; set_history(nt)), 112-145 (work: out[i*I + nf] =
//   firs[nf]->filter(&in[i])); runtime/gr_sync_interpolator.h:48-53 (output_multiple I).
//   gr_pfb_interpolator_ccf.cc:69-104 (set_taps: tpf = ceil(ntaps/R), zeros at the END of the taps, filter j gets
//   padded[j + k*R] through gr_fir_ccf; set_history(tpf)), 122-148 (work: out[n*R + j] = filters[j]->filter(&in[n])):
//   the interpolator's schedule with another bank.
//
// Both run the closed form of resampler.h: output o of a call that starts at c0 = ctr uses filter (c0 + o*D) % I at
// input (c0 + o*D) / I; a call of n outputs consumes (c0 + n*D) / I items and leaves ctr = (c0 + n*D) % I.  The
// interpolator is D = 1, c0 = 0 on its input with the nt - 1 history items in front.  Nothing depends on the data:
// produced, consumed and ctr are known on the host before the kernel runs.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "grhip_internal.h"
#include "resampler.h"
#include "stream_block.h"

using namespace grhip;

namespace {

constexpr unsigned long long RS_MAX_ID = 1ull << 20;        // I, D: c0 + o*D stays far inside 64 bits
constexpr long long RS_MAX_CAPTURE = 1LL << 40;             // run_captures_device: items per capture

unsigned long long gcd_ull(unsigned long long a, unsigned long long b)
{
    while (b) { const unsigned long long t = a % b; a = b; b = t; }
    return a;
}

int kind_of(const char *kind, RsKind *k)
{
    if (!kind) return fail(GRHIP_EINVAL, "null kind");
    if (!strcmp(kind, "ccf")) *k = RS_CCF;
    else if (!strcmp(kind, "fff")) *k = RS_FFF;
    else if (!strcmp(kind, "ccc")) *k = RS_CCC;
    else return fail(GRHIP_EINVAL, "unknown resampler kind '%s' (ccf, fff or ccc)", kind);
    return GRHIP_OK;
}

}  // namespace

// what both blocks share: the polyphase bank, the latch of set_taps and the launch
struct grhip_rs_core : ModeBlock {
    RsKind kind = RS_CCF;
    bool interp = false;
    bool pad_end = false;               // gr_pfb_interpolator_ccf: the zeros go behind the taps
    unsigned long long I = 1, D = 1, P = 1, Dp = 1;
    int nt = 1, WP = 0;
    unsigned long long ctr = 0;         // d_ctr (rational resampler)
    std::vector<float> new_taps;        // d_new_taps, front padded (floats; x2 for ccc)
    bool updated = false;
    DevBuf d_bank;

    int tw() const { return kind == RS_CCC ? 2 : 1; }
    size_t item() const { return kind == RS_FFF ? 4 : 8; }

    // set_taps (.cc.t:83-99): the taps, zeros in front up to a multiple of I (behind them for the pfb interpolator,
    // gr_pfb_interpolator_ccf.cc:82-87); refuses what the kernel cannot take
    int pad_taps(const float *taps, size_t ntaps, std::vector<float> *out) const
    {
        if (ntaps == 0)
            return fail(GRHIP_EINVAL, "%s: no taps (install_taps would make filters of 0 taps: outside the "
                                      "reference's defined behaviour)", name());
        if (!taps) return fail(GRHIP_EINVAL, "null taps");
        const unsigned long long padded = (ntaps + I - 1) / I * I;
        if (padded / I > (unsigned long long)std::numeric_limits<int>::max() / 4)
            return fail(GRHIP_EINVAL, "%s: too many taps", name());
        const int nt_new = (int)(padded / I);
        RsConfig c;
        int rc = rs_config(kind, true, I, D, nt_new, 0, &c);
        if (!rc) rc = rs_config(kind, false, I, D, nt_new, 0, &c);
        if (rc) return rc;
        out->assign((size_t)(pad_end ? 0 : (padded - ntaps) * tw()), 0.f);
        out->insert(out->end(), taps, taps + ntaps * tw());
        out->resize((size_t)(padded * tw()), 0.f);
        return GRHIP_OK;
    }

    const char *name() const { return pad_end ? "pfb_interpolator" : interp ? "interp_fir_filter" : "rational_resampler_base"; }

    // install_taps (.cc.t:102-120): the bank of resampler.h's rs_bank
    int install(const std::vector<float> &padded)
    {
        const std::vector<float> bank = rs_bank(padded, tw(), I, D, P, &nt, &WP);
        int rc = d_bank.reserve(bank.size() * sizeof(float));
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(d_bank.p, bank.data(), bank.size() * sizeof(float), hipMemcpyHostToDevice));
        return GRHIP_OK;
    }

    int init(RsKind k, bool is_interp, unsigned long long i, unsigned long long d, const float *taps, size_t ntaps,
             int device, bool zeros_behind = false)
    {
        kind = k; interp = is_interp; pad_end = zeros_behind;
        if (i == 0) return fail(GRHIP_ERANGE, "%s: interpolation must be > 0", name());
        if (d == 0) return fail(GRHIP_ERANGE, "%s: decimation must be > 0", name());
        if (i > RS_MAX_ID || d > RS_MAX_ID) return fail(GRHIP_EINVAL, "%s: interpolation and decimation must be <= 2^20", name());
        I = i; D = d;
        const unsigned long long g = gcd_ull(I, D);
        P = I / g; Dp = D / g;
        std::vector<float> padded;
        int rc = pad_taps(taps, ntaps, &padded);
        if (rc) return rc;
        if ((rc = init_device(device))) return rc;
        if ((rc = rs_prepare_device(kind))) return rc;
        mode = default_mode();
        return install(padded);                         // the constructor installs the taps (.cc.t:70-71)
    }

    int set_taps(const float *taps, size_t ntaps)
    {
        std::vector<float> padded;
        int rc = pad_taps(taps, ntaps, &padded);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        new_taps.swap(padded);
        updated = true;
        return GRHIP_OK;
    }

    // a latched set_taps: install the new bank and report it (the work call then returns 0).  The bank is rewritten
    // by a blocking copy, so the launches that may still read it (on `st` and the handle's stream) are waited for.
    int apply_update(hipStream_t st, bool *did)
    {
        *did = false;
        if (!updated) return GRHIP_OK;
        int rc = drain(st);
        if (!rc) rc = install(new_taps);
        if (rc) return rc;
        updated = false;
        *did = true;
        return GRHIP_OK;
    }

    int launch(unsigned long long c0, long long nout, const void *d_in, long long in_stride, long long lead,
               long long n_phys, void *d_out, long long out_stride, int n_streams, hipStream_t st)
    {
        RsLaunch a;
        a.in = d_in; a.in_stride = in_stride; a.lead = lead; a.n_phys = n_phys;
        a.out = d_out; a.out_stride = out_stride; a.nout = nout; a.n_streams = n_streams;
        a.bank = d_bank.p;
        a.I = I; a.D = D; a.c0 = c0;
        a.P = (int)P; a.Dp = (int)Dp; a.nt = nt; a.WP = WP; a.RS = nt + 2 * WP;
        return rs_launch(kind, !mode_fast(mode), a, st);
    }

    // ---- gr_rational_resampler_base_XXX ----
    int forecast(int n) const
    {
        // .cc.t:137: max(1, (int)((double)(n+1) * D / I) + nt - 1)
        const long long r = (long long)(int)((double)((long long)n + 1) * (double)D / (double)I) + nt - 1;
        return (int)std::max(1LL, std::min<long long>(r, std::numeric_limits<int>::max()));
    }

    int general_work_device(int noutput_items, int ninput_items, const void *d_in, void *d_out, int *consumed,
                            void *stream)
    {
        if (!consumed) return fail(GRHIP_EINVAL, "null consumed");
        *consumed = 0;
        if (noutput_items < 0 || ninput_items < 0) return fail(GRHIP_EINVAL, "negative item count");
        int rc = bind();
        if (rc) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        bool did;
        if ((rc = apply_update(st, &did))) return rc;
        if (did) return 0;                                                  // .cc.t:152-155
        if (noutput_items == 0) return 0;
        const unsigned long long n = (unsigned long long)noutput_items;
        const unsigned long long reads = (ctr + (n - 1) * D) / I + (unsigned long long)nt;   // last window's end
        const unsigned long long eaten = (ctr + n * D) / I;                                  // in - in0
        if (reads > (unsigned long long)ninput_items || eaten > (unsigned long long)ninput_items)
            return fail(GRHIP_EINVAL, "rational_resampler_base: %d outputs from ctr %llu need %llu input items, got %d",
                        noutput_items, ctr, std::max(reads, eaten), ninput_items);
        if (!d_in || !d_out) return fail(GRHIP_EINVAL, "null buffer");
        if ((rc = launch(ctr, noutput_items, d_in, 0, 0, ninput_items, d_out, 0, 1, st))) return rc;
        ctr = (ctr + n * D) % I;
        *consumed = (int)eaten;
        return noutput_items;
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

    // ---- gr_interp_fir_filter_XXX ----
    int work_device(int noutput_items, const void *d_in, void *d_out, void *stream)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        if ((unsigned long long)noutput_items % I)
            return fail(GRHIP_EINVAL, "%s: noutput_items %d is not a multiple of the interpolation %llu "
                                      "(output_multiple)", name(), noutput_items, I);
        int rc = bind();
        if (rc) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        bool did;
        if ((rc = apply_update(st, &did))) return rc;
        if (did) return 0;                                                  // .cc.t:127-130
        if (noutput_items == 0) return 0;
        if (!d_in || !d_out) return fail(GRHIP_EINVAL, "null buffer");
        const long long ni = noutput_items / (long long)I;
        if ((rc = launch(0, noutput_items, d_in, 0, 0, ni + nt - 1, d_out, 0, 1, st))) return rc;
        return noutput_items;
    }

    int work(int noutput_items, const void *in, void *out)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        if ((unsigned long long)noutput_items % I)
            return fail(GRHIP_EINVAL, "%s: noutput_items %d is not a multiple of the interpolation %llu "
                                      "(output_multiple)", name(), noutput_items, I);
        if ((!in || !out) && noutput_items) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        // the items this call reads: n/I + nt - 1, history in front (gr_sync_interpolator with set_history(nt)); a call
        // that installs new taps reads nothing
        size_t nin;
        {
            std::lock_guard<std::mutex> lk(setter_mutex);
            nin = updated || noutput_items == 0 ? 0 : (size_t)(noutput_items / (long long)I) + nt - 1;
        }
        return (int)host_call(in, nin * item(), nin * item() + 16, (size_t)noutput_items * item() + 16, out, item(),
                              [&](void *d_in, void *d_out, hipStream_t s) { return work_device(noutput_items, d_in, d_out, s); });
    }

    // ---- both: fresh captures ----
    int run_captures_device(int n_streams, size_t n_samples, const void *d_in, size_t in_stride, void *d_out,
                            size_t out_stride, size_t *n_out, void *stream)
    {
        if (!n_out) return fail(GRHIP_EINVAL, "null n_out");
        *n_out = 0;
        if (n_streams < 0) return fail(GRHIP_EINVAL, "negative n_streams");
        if (n_samples > (size_t)RS_MAX_CAPTURE) return fail(GRHIP_EINVAL, "%s: n_samples above 2^40", name());
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        const long long N = (long long)n_samples;
        long long nout, lead;
        if (interp) {                       // the nt - 1 history zeros in front, I outputs per input item
            nout = N * (long long)I;
            lead = nt - 1;
        } else {                            // no zeros in front; every o with (o*D)/I + nt <= N
            nout = N < nt ? 0 : (long long)((((unsigned long long)(N - nt) * I + I - 1) / D) + 1);
            lead = 0;
        }
        *n_out = (size_t)nout;
        if (!d_out || n_streams == 0 || nout == 0) return GRHIP_OK;     // a query, or nothing to do
        if (!d_in) return fail(GRHIP_EINVAL, "null buffer");
        if (n_streams > 1 && (in_stride < n_samples || out_stride < (size_t)nout))
            return fail(GRHIP_EINVAL, "%s: strides shorter than n_samples / n_out", name());
        return launch(0, nout, d_in, (long long)in_stride, lead, N, d_out, (long long)out_stride, n_streams,
                      pick(stream));
    }

    ~grhip_rs_core() { if (own_stream) (void)hipStreamSynchronize(own_stream); }     // then the bank is freed
};

struct grhip_interp_fir_filter : grhip_rs_core {};
struct grhip_pfb_interpolator_ccf : grhip_rs_core {};
struct grhip_rational_resampler_base : grhip_rs_core {};

namespace {

template <class H>
int create_t(H **h, const char *kind, bool interp, long long I, long long D, const float *taps, size_t ntaps, int device,
             bool zeros_behind = false)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle pointer");
    *h = nullptr;
    RsKind k;
    int rc = kind_of(kind, &k);
    if (rc) return rc;
    if (I < 0 || D < 0) return fail(GRHIP_ERANGE, "interpolation and decimation must be > 0");
    return make_handle(h, [&](H *b) {
        return b->init(k, interp, (unsigned long long)I, (unsigned long long)D, taps, ntaps, device, zeros_behind);
    });
}

}  // namespace

extern "C" {

// ---- gr_interp_fir_filter_XXX ----
int grhip_interp_fir_filter_create(grhip_interp_fir_filter **h, const char *kind, unsigned interpolation,
                                   const float *taps, size_t ntaps, int device)
{
    return create_t(h, kind, true, interpolation, 1, taps, ntaps, device);
}

void grhip_interp_fir_filter_destroy(grhip_interp_fir_filter *h)
{
    destroy_handle(h);
}

int grhip_interp_fir_filter_set_taps(grhip_interp_fir_filter *h, const float *taps, size_t ntaps)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->set_taps(taps, ntaps);
}

int grhip_interp_fir_filter_set_mode(grhip_interp_fir_filter *h, int mode)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->set_mode(mode);
}

int grhip_interp_fir_filter_history(const grhip_interp_fir_filter *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->nt;
}

int grhip_interp_fir_filter_interpolation(const grhip_interp_fir_filter *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return (int)h->I;
}

int grhip_interp_fir_filter_work(grhip_interp_fir_filter *h, int noutput_items, const void *in, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work(noutput_items, in, out);
}

int grhip_interp_fir_filter_work_device(grhip_interp_fir_filter *h, int noutput_items, const void *d_in, void *d_out,
                                        void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work_device(noutput_items, d_in, d_out, stream);
}

int grhip_interp_fir_filter_run_captures_device(grhip_interp_fir_filter *h, int n_streams, size_t n_samples,
                                                const void *d_in, size_t in_stride_items, void *d_out,
                                                size_t out_stride_items, size_t *n_out, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->run_captures_device(n_streams, n_samples, d_in, in_stride_items, d_out, out_stride_items, n_out, stream);
}

// ---- gr_pfb_interpolator_ccf ----
int grhip_pfb_interpolator_ccf_create(grhip_pfb_interpolator_ccf **h, unsigned interp, const float *taps, size_t ntaps,
                                      int device)
{
    return create_t(h, "ccf", true, interp, 1, taps, ntaps, device, true);
}

void grhip_pfb_interpolator_ccf_destroy(grhip_pfb_interpolator_ccf *h)
{
    destroy_handle(h);
}

int grhip_pfb_interpolator_ccf_set_taps(grhip_pfb_interpolator_ccf *h, const float *taps, size_t ntaps)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->set_taps(taps, ntaps);
}

int grhip_pfb_interpolator_ccf_set_mode(grhip_pfb_interpolator_ccf *h, int mode)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->set_mode(mode);
}

int grhip_pfb_interpolator_ccf_history(const grhip_pfb_interpolator_ccf *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->nt;                                        // set_history(d_taps_per_filter), .cc:101
}

int grhip_pfb_interpolator_ccf_interpolation(const grhip_pfb_interpolator_ccf *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return (int)h->I;
}

int grhip_pfb_interpolator_ccf_work(grhip_pfb_interpolator_ccf *h, int noutput_items, const void *in, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work(noutput_items, in, out);
}

int grhip_pfb_interpolator_ccf_work_device(grhip_pfb_interpolator_ccf *h, int noutput_items, const void *d_in,
                                           void *d_out, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work_device(noutput_items, d_in, d_out, stream);
}

// ---- gr_rational_resampler_base_XXX ----
int grhip_rational_resampler_base_create(grhip_rational_resampler_base **h, const char *kind, unsigned interpolation,
                                         unsigned decimation, const float *taps, size_t ntaps, int device)
{
    return create_t(h, kind, false, interpolation, decimation, taps, ntaps, device);
}

void grhip_rational_resampler_base_destroy(grhip_rational_resampler_base *h)
{
    destroy_handle(h);
}

int grhip_rational_resampler_base_set_taps(grhip_rational_resampler_base *h, const float *taps, size_t ntaps)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->set_taps(taps, ntaps);
}

int grhip_rational_resampler_base_set_mode(grhip_rational_resampler_base *h, int mode)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->set_mode(mode);
}

int grhip_rational_resampler_base_history(const grhip_rational_resampler_base *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->nt;
}

int grhip_rational_resampler_base_interpolation(const grhip_rational_resampler_base *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return (int)h->I;
}

int grhip_rational_resampler_base_decimation(const grhip_rational_resampler_base *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return (int)h->D;
}

int grhip_rational_resampler_base_forecast(const grhip_rational_resampler_base *h, int noutput_items)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    return h->forecast(noutput_items);
}

int grhip_rational_resampler_base_general_work(grhip_rational_resampler_base *h, int noutput_items, int ninput_items,
                                               const void *in, void *out, int *consumed)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->general_work(noutput_items, ninput_items, in, out, consumed);
}

int grhip_rational_resampler_base_general_work_device(grhip_rational_resampler_base *h, int noutput_items,
                                                      int ninput_items, const void *d_in, void *d_out, int *consumed,
                                                      void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->general_work_device(noutput_items, ninput_items, d_in, d_out, consumed, stream);
}

int grhip_rational_resampler_base_run_captures_device(grhip_rational_resampler_base *h, int n_streams,
                                                      size_t n_samples, const void *d_in, size_t in_stride_items,
                                                      void *d_out, size_t out_stride_items, size_t *n_out,
                                                      void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->run_captures_device(n_streams, n_samples, d_in, in_stride_items, d_out, out_stride_items, n_out, stream);
}

}  // extern "C"
