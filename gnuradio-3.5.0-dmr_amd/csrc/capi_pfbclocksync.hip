// capi_pfbclocksync.hip -- C ABI of gr_pfb_clock_sync_ccf and of its tap partition.
//
// Reference: gnuradio-core/src/lib/filter/gr_pfb_clock_sync_ccf.{h,cc}, gr_fir_XXX_generic.cc.t, general/gr_math.h:63-69.
//
// A handle takes S streams back to back ([S][n_in]) and works on new items only.  What a stream remembers on the
// device is a PcsState (k, rate_f, error, the slips, pos) and the last pcs_hist() items of xz, so the result depends on
// the concatenated input alone (include/grhip.h).  The two banks are laid out on the host (pfb_clock_sync.h) and live
// on the device with every arm's taps reversed; the gains and the limit are kernel arguments.  This loop is not
// gri_control_loop, so the handle is a StreamBlock and not a LoopBlock.
#include <climits>
#include <cstring>
#include <vector>

#include "pfb_clock_sync_launch.h"
#include "stream_block.h"

using namespace grhip;

namespace {

struct PcsBlock : StreamBlock {
    PcsLoop loop;
    PcsParams p{};
    float init_phase = 0.f, rate_f0 = 0.f;
    long long arrived = 0;                  // items of xz that the calls so far have brought, the zeros in front included
    std::vector<float> bank, dbank;         // [nfilters][tpf], as the reference's get_taps hands them out
    DevBuf d_bank, d_dbank, d_state, d_hist, d_prod;

    int hist() const { return pcs_hist(p.tpf, p.isps, p.osps); }

    // every stream back at the constructor's values; streams drained, under setter_mutex (or not handed out yet)
    int restart()
    {
        const size_t bytes = (size_t)nstreams * (size_t)hist() * sizeof(float2);
        int rc;
        if ((rc = d_hist.reserve(bytes)) || (rc = d_prod.reserve((size_t)nstreams * sizeof(int)))) return rc;
        if ((rc = zero_device(d_hist.p, bytes))) return rc;
        arrived = p.tpf + p.isps - 1;
        return fill_state(d_state, PcsState{init_phase, rate_f0, 0.f, 0, 0});
    }

    int init(double sps, float loop_bw, const float *taps, int ntaps, int nfilters, float init_phase_, float max_dev, int osps, int dev)
    {
        if (const char *e = pcs_check_args(sps, loop_bw, init_phase_, max_dev, osps)) return fail(GRHIP_EINVAL, "%s", e);
        int tpf = 0;
        if (const char *e = pcs_design(taps, ntaps, nfilters, bank, dbank, tpf)) return fail(GRHIP_EINVAL, "%s", e);
        if (!loop.init(loop_bw, max_dev)) return fail(GRHIP_EINVAL, "gr_pfb_clock_sync_cc: invalid bandwidth (the gains must be finite).");
        p.nfilters = nfilters; p.tpf = tpf; p.isps = (int)floor(sps); p.osps = osps;
        pcs_rate(sps, nfilters, p.rate_i, rate_f0);
        init_phase = init_phase_;
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        // the device's copy: an arm's taps reversed, so that tap j of a row works on xz[pos + j]
        std::vector<float> rb(bank.size()), rd(bank.size());
        for (int f = 0; f < nfilters; ++f)
            for (int j = 0; j < tpf; ++j) {
                rb[(size_t)f * tpf + j] = bank[(size_t)f * tpf + (tpf - 1 - j)];
                rd[(size_t)f * tpf + j] = dbank[(size_t)f * tpf + (tpf - 1 - j)];
            }
        const size_t bytes = rb.size() * sizeof(float);
        if ((rc = d_bank.reserve(bytes)) || (rc = d_dbank.reserve(bytes))) return rc;
        GRHIP_HIP(hipMemcpy(d_bank.p, rb.data(), bytes, hipMemcpyHostToDevice));
        GRHIP_HIP(hipMemcpy(d_dbank.p, rd.data(), bytes, hipMemcpyHostToDevice));
        return restart();
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
    }

    // the setters act on the next symbol: the gains travel as kernel arguments
    int set_param(bool (PcsLoop::*set)(float), float v, const char *what)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        if (!(loop.*set)(v)) return fail(GRHIP_EINVAL, "gr_pfb_clock_sync_cc: invalid %s", what);
        return GRHIP_OK;
    }

    float get_param(float PcsLoop::*which)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return loop.*which;
    }

    template <class T>
    int get_state(int s, T PcsState::*which, T *out)
    {
        if (!out) return fail(GRHIP_EINVAL, "null argument");
        PcsState st;
        int rc = read_state(d_state, s, &st);
        if (rc) return rc;
        *out = st.*which;
        return GRHIP_OK;
    }

    int hand_out(const std::vector<float> &b, float *out, size_t cap, int *nfilters, int *tpf)
    {
        if (!nfilters || !tpf) return fail(GRHIP_EINVAL, "null argument");
        *nfilters = p.nfilters;
        *tpf = p.tpf;
        if (!out || cap < b.size()) return fail(GRHIP_ERANGE, "pfb_clock_sync_ccf: %zu taps, room for %zu", b.size(), out ? cap : (size_t)0);
        memcpy(out, b.data(), b.size() * sizeof(float));
        return GRHIP_OK;
    }

    // an out_cap that always suffices: a symbol moves its base by at least one item, and the first call may find
    // isps - 1 of the zeros in front still unspent
    long long max_produced(long long n_in) const { return (long long)p.osps * (n_in + p.isps); }

    int check_sizes(int n_in, long long out_cap) const
    {
        if (n_in < 0) return fail(GRHIP_EINVAL, "negative item count");
        if (max_produced(n_in) > INT_MAX) return fail(GRHIP_EINVAL, "pfb_clock_sync_ccf: too many items for one call");
        if (out_cap > INT_MAX) return fail(GRHIP_EINVAL, "pfb_clock_sync_ccf: out_cap above 2^31 - 1 items");      // the byte counts below stay exact
        if (out_cap < max_produced(n_in)) return fail(GRHIP_EINVAL, "pfb_clock_sync_ccf: out_cap below grhip_pfb_clock_sync_ccf_max_produced");
        return GRHIP_OK;
    }

    int work_device(int n_in, const void *d_in, long long out_cap, void *d_out, void *d_err, void *d_rate, void *d_k, int *d_produced,
                    void *stream)
    {
        int rc = check_sizes(n_in, out_cap);
        if (rc) return rc;
        if (!d_out || !d_produced || (n_in > 0 && !d_in)) return fail(GRHIP_EINVAL, "null buffer");
        const void *aux[3] = {d_err, d_rate, d_k};
        const int given = (d_err != nullptr) + (d_rate != nullptr) + (d_k != nullptr);
        if (given != 0 && given != 3) return fail(GRHIP_EINVAL, "pfb_clock_sync_ccf: err, rate and k are given together or not at all");
        if (!aligned(d_in, 8) || !aligned(d_out, 8) || !aligned(d_produced, 4)) return fail(GRHIP_EINVAL, "items not naturally aligned");
        const size_t in_bytes = (size_t)nstreams * (size_t)n_in * 8, c_bytes = (size_t)nstreams * (size_t)out_cap * 8, f_bytes = c_bytes / 2;
        const size_t p_bytes = (size_t)nstreams * sizeof(int);
        if ((rc = check_apart("pfb_clock_sync_ccf", d_in, in_bytes, d_out, c_bytes))) return rc;
        bool hit = overlap(d_in, in_bytes, d_produced, p_bytes) || overlap(d_out, c_bytes, d_produced, p_bytes);
        for (int i = 0; i < 3; ++i) {
            if (!aligned(aux[i], 4)) return fail(GRHIP_EINVAL, "items not naturally aligned");
            hit = hit || overlap(d_in, in_bytes, aux[i], f_bytes) || overlap(d_out, c_bytes, aux[i], f_bytes) ||
                  overlap(d_produced, p_bytes, aux[i], f_bytes);
            for (int k = 0; k < i; ++k) hit = hit || overlap(aux[k], f_bytes, aux[i], f_bytes);
        }
        if (hit) return fail(GRHIP_EINVAL, "pfb_clock_sync_ccf: no buffer may overlap another");
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        PcsLaunch l;
        l.in = (const float2 *)d_in; l.out = (float2 *)d_out;
        l.err = (float *)d_err; l.rate = (float *)d_rate; l.k = (float *)d_k;
        l.produced = d_produced;
        l.n = n_in; l.nstreams = nstreams; l.out_cap = out_cap; l.arrived = arrived;
        l.bank = d_bank.as<float>(); l.dbank = d_dbank.as<float>();
        l.p = p;
        l.p.alpha = loop.alpha; l.p.beta = loop.beta; l.p.max_dev = loop.max_dev;
        l.state = d_state.as<PcsState>();
        l.hist = d_hist.as<float2>();
        if ((rc = pfb_clock_sync_launch(!mode_fast(mode), l, st))) return rc;
        arrived += n_in;
        return GRHIP_OK;
    }

    // host buffers: out (and err, rate, k) hold out_cap items per stream; produced[s] of them are written
    int work(int n_in, const void *in, long long out_cap, void *out, void *err, void *rate, void *k, int *produced)
    {
        int rc = check_sizes(n_in, out_cap);
        if (rc) return rc;
        if (!out || !produced || (n_in > 0 && !in)) return fail(GRHIP_EINVAL, "null buffer");
        void *aux[3] = {err, rate, k};
        const int given = (err != nullptr) + (rate != nullptr) + (k != nullptr);
        if (given != 0 && given != 3) return fail(GRHIP_EINVAL, "pfb_clock_sync_ccf: err, rate and k are given together or not at all");
        if ((rc = bind())) return rc;
        const size_t cap = (size_t)max_produced(n_in);           // the device's rows are as short as they may be
        const size_t in_bytes = (size_t)nstreams * (size_t)n_in * 8, c_bytes = (size_t)nstreams * cap * 8;
        const size_t f_row = (c_bytes / 2 + 15) & ~(size_t)15, f_off = (c_bytes + 15) & ~(size_t)15;
        if ((rc = stage_in.reserve(in_bytes + 16))) return rc;
        if ((rc = stage_out.reserve(f_off + 3 * f_row + 16))) return rc;
        hipStream_t st = own_stream;
        if (n_in > 0) GRHIP_H2D(this, stage_in.p, in, in_bytes, st);
        char *so = (char *)stage_out.p, *f = so + f_off;
        if ((rc = work_device(n_in, stage_in.p, (long long)cap, so, given ? f : nullptr, given ? f + f_row : nullptr, given ? f + 2 * f_row : nullptr,
                              d_prod.as<int>(), st)))
            return rc;
        GRHIP_D2H(this, produced, d_prod.p, (size_t)nstreams * sizeof(int), st);
        GRHIP_HIP(hipStreamSynchronize(st));
        for (int s = 0; s < nstreams; ++s) {
            const size_t m = (size_t)produced[s];
            if (!m) continue;
            GRHIP_D2H(this, (char *)out + (size_t)s * (size_t)out_cap * 8, so + (size_t)s * cap * 8, m * 8, st);
            for (int i = 0; given && i < 3; ++i)
                GRHIP_D2H(this, (char *)aux[i] + (size_t)s * (size_t)out_cap * 4, f + (size_t)i * f_row + (size_t)s * cap * 4, m * 4, st);
        }
        GRHIP_HIP(hipStreamSynchronize(st));
        return GRHIP_OK;
    }
};

}  // namespace

struct grhip_pfb_clock_sync_ccf : PcsBlock {};

#define PCS_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")
#define PCS_GET(ENTRY, FIELD)                                                                                         \
    float grhip_pfb_clock_sync_ccf_##ENTRY(grhip_pfb_clock_sync_ccf *h)                                               \
    {                                                                                                                 \
        if (!h) return (float)fail(GRHIP_EINVAL, "null handle");                                                      \
        return h->get_param(&PcsLoop::FIELD);                                                                         \
    }

extern "C" {

int grhip_pfb_clock_sync_taps(const float *taps, int ntaps, int nfilters, float *bank, float *diff_bank, int *tpf)
{
    if (!tpf) return fail(GRHIP_EINVAL, "null argument");
    std::vector<float> b, d;
    int t = 0;
    if (const char *e = pcs_design(taps, ntaps, nfilters, b, d, t)) return fail(GRHIP_EINVAL, "%s", e);
    *tpf = t;
    if (bank) memcpy(bank, b.data(), b.size() * sizeof(float));
    if (diff_bank) memcpy(diff_bank, d.data(), d.size() * sizeof(float));
    return GRHIP_OK;
}

int grhip_pfb_clock_sync_ccf_create(grhip_pfb_clock_sync_ccf **h, double sps, float loop_bw, const float *taps, int ntaps, int filter_size,
                                    float init_phase, float max_rate_deviation, int osps, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_pfb_clock_sync_ccf *b) {
        return b->init(sps, loop_bw, taps, ntaps, filter_size, init_phase, max_rate_deviation, osps, device);
    });
}

void grhip_pfb_clock_sync_ccf_destroy(grhip_pfb_clock_sync_ccf *h) { destroy_handle(h); }
int grhip_pfb_clock_sync_ccf_set_mode(grhip_pfb_clock_sync_ccf *h, int mode) { PCS_NULL(h); return h->set_mode(mode); }
int grhip_pfb_clock_sync_ccf_set_streams(grhip_pfb_clock_sync_ccf *h, int nstreams) { PCS_NULL(h); return h->set_streams(nstreams); }

// gr_pfb_clock_sync_ccf.cc:121-159
int grhip_pfb_clock_sync_ccf_set_loop_bandwidth(grhip_pfb_clock_sync_ccf *h, float bw)
{
    PCS_NULL(h);
    return h->set_param(&PcsLoop::set_loop_bandwidth, bw, "bandwidth. Must be >= 0 (and leave finite gains).");
}
int grhip_pfb_clock_sync_ccf_set_damping_factor(grhip_pfb_clock_sync_ccf *h, float df)
{
    PCS_NULL(h);
    return h->set_param(&PcsLoop::set_damping_factor, df, "damping factor. Must be in [0,1].");
}
int grhip_pfb_clock_sync_ccf_set_alpha(grhip_pfb_clock_sync_ccf *h, float alpha)
{
    PCS_NULL(h);
    return h->set_param(&PcsLoop::set_alpha, alpha, "alpha. Must be in [0,1].");
}
int grhip_pfb_clock_sync_ccf_set_beta(grhip_pfb_clock_sync_ccf *h, float beta)
{
    PCS_NULL(h);
    return h->set_param(&PcsLoop::set_beta, beta, "beta. Must be in [0,1].");
}
int grhip_pfb_clock_sync_ccf_set_max_rate_deviation(grhip_pfb_clock_sync_ccf *h, float m)
{
    PCS_NULL(h);
    return h->set_param(&PcsLoop::set_max_dev, m, "max_rate_deviation. Must be finite.");
}
PCS_GET(get_loop_bandwidth, loop_bw)
PCS_GET(get_damping_factor, damping)
PCS_GET(get_alpha, alpha)
PCS_GET(get_beta, beta)
PCS_GET(get_max_rate_deviation, max_dev)

int grhip_pfb_clock_sync_ccf_get_clock_rate(grhip_pfb_clock_sync_ccf *h, int s, float *rate) { PCS_NULL(h); return h->get_state(s, &PcsState::rate_f, rate); }
int grhip_pfb_clock_sync_ccf_k(grhip_pfb_clock_sync_ccf *h, int s, float *k) { PCS_NULL(h); return h->get_state(s, &PcsState::k, k); }
int grhip_pfb_clock_sync_ccf_error(grhip_pfb_clock_sync_ccf *h, int s, float *error) { PCS_NULL(h); return h->get_state(s, &PcsState::error, error); }
int grhip_pfb_clock_sync_ccf_slips(grhip_pfb_clock_sync_ccf *h, int s, int *slips) { PCS_NULL(h); return h->get_state(s, &PcsState::slips, slips); }
int grhip_pfb_clock_sync_ccf_position(grhip_pfb_clock_sync_ccf *h, int s, long long *pos) { PCS_NULL(h); return h->get_state(s, &PcsState::pos, pos); }

int grhip_pfb_clock_sync_ccf_get_taps(grhip_pfb_clock_sync_ccf *h, float *bank, size_t cap, int *nfilters, int *tpf)
{
    PCS_NULL(h);
    return h->hand_out(h->bank, bank, cap, nfilters, tpf);
}
int grhip_pfb_clock_sync_ccf_get_diff_taps(grhip_pfb_clock_sync_ccf *h, float *bank, size_t cap, int *nfilters, int *tpf)
{
    PCS_NULL(h);
    return h->hand_out(h->dbank, bank, cap, nfilters, tpf);
}

int grhip_pfb_clock_sync_ccf_max_produced(grhip_pfb_clock_sync_ccf *h, int n_in)
{
    PCS_NULL(h);
    if (n_in < 0 || h->max_produced(n_in) > INT_MAX) return fail(GRHIP_EINVAL, "pfb_clock_sync_ccf: item count out of range");
    return (int)h->max_produced(n_in);
}

int grhip_pfb_clock_sync_ccf_work(grhip_pfb_clock_sync_ccf *h, int n_in, const void *in, long long out_cap, void *out, void *err, void *rate,
                                  void *k, int *produced)
{
    PCS_NULL(h);
    return h->work(n_in, in, out_cap, out, err, rate, k, produced);
}

int grhip_pfb_clock_sync_ccf_work_device(grhip_pfb_clock_sync_ccf *h, int n_in, const void *d_in, long long out_cap, void *d_out, void *d_err,
                                         void *d_rate, void *d_k, int *d_produced, void *stream)
{
    PCS_NULL(h);
    return h->work_device(n_in, d_in, out_cap, d_out, d_err, d_rate, d_k, d_produced, stream);
}

}  // extern "C"
