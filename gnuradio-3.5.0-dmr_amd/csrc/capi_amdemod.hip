// capi_amdemod.hip -- C ABI of the AM demodulator hier block, blks2.am_demod_cf and blks2.demod_10k0a3e_cf
// (blks2impl/am_demod.py:42-58, :60-76): gr_complex_to_mag -> gr_add_const_ff(-1) -> gr_fir_filter_fff(audio_decim,
// audio_taps).
//
// The handle is the hier block as the scheduler runs it: new items only, the FIR from a zero delay line.  Per stream
// the device keeps the FIR's last ntaps - 1 input floats (values of |x| - 1, zeros at the start); the stream position
// modulo the decimation is the same for every stream and kept on the host.
#include <vector>

#include "am_demod.h"
#include "fir_kernels.h"
#include "grhip_internal.h"
#include "stream_block.h"

using namespace grhip;

namespace {

constexpr int AMD_MAX_DECIM = 1 << 16;
constexpr int AMD_MAX_TAPS = 1 << 16;

struct AmDemodBlock : StreamBlock {
    int D = 1;
    std::vector<float> taps;            // forward order
    int pos = 0;                        // items taken so far, modulo D
    int cur = 0;                        // which copy of the state is current
    bool fused_ok = false;
    DevBuf d_fwd, d_rev, d_hist, d_row;

    int H() const { return (int)taps.size() - 1; }
    size_t hist_row() const { return (size_t)(H() > 0 ? H() : 1); }

    AmdState state(int which) const
    {
        AmdState s;
        s.hist = d_hist.as<float>() + (size_t)which * nstreams * hist_row();
        return s;
    }

    // the FIR back at a zero delay line; streams drained, under setter_mutex
    int zero_state()
    {
        const size_t bytes = 2 * (size_t)nstreams * hist_row() * sizeof(float);
        int rc = d_hist.reserve(bytes);
        if (rc) return rc;
        if ((rc = zero_device(d_hist.p, bytes))) return rc;
        pos = 0; cur = 0;
        return GRHIP_OK;
    }

    static int check(int decim, const float *at, size_t ntaps)
    {
        if (!at) return fail(GRHIP_EINVAL, "null taps");
        if (decim < 1 || decim > AMD_MAX_DECIM) return fail(GRHIP_EINVAL, "am_demod_cf: audio_decim 1 .. %d", AMD_MAX_DECIM);
        if (ntaps < 1 || ntaps > (size_t)AMD_MAX_TAPS) return fail(GRHIP_EINVAL, "am_demod_cf: 1 .. %d audio taps", AMD_MAX_TAPS);
        return GRHIP_OK;
    }

    int init(int decim, const float *at, size_t ntaps, int dev)
    {
        int rc = check(decim, at, ntaps);
        if (rc) return rc;
        D = decim;
        taps.assign(at, at + ntaps);
        mode = default_mode();
        if ((rc = init_device(dev))) return rc;
        fused_ok = H() <= AMD_MAX_HIST;
        // forward taps zero-padded to a multiple of AMD_R: the blocked step loads them 8 at a time
        std::vector<float> fwd(taps);
        fwd.resize((taps.size() + AMD_R - 1) / AMD_R * AMD_R, 0.f);
        std::vector<float> rev(taps.rbegin(), taps.rend());
        if ((rc = d_fwd.reserve(fwd.size() * sizeof(float)))) return rc;
        if ((rc = d_rev.reserve(rev.size() * sizeof(float)))) return rc;
        GRHIP_HIP(hipMemcpy(d_fwd.p, fwd.data(), fwd.size() * sizeof(float), hipMemcpyHostToDevice));
        GRHIP_HIP(hipMemcpy(d_rev.p, rev.data(), rev.size() * sizeof(float), hipMemcpyHostToDevice));
        return zero_state();
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return zero_state(); });
    }

    int engine()
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return mode_fast(mode) && fused_ok ? 1 : 0;
    }

    // outputs of a call of n_in items at the current position, and the call's item of the first of them
    int produced_of(int n_in, int *o0_out) const
    {
        const int o0 = (D - pos) % D;
        if (o0_out) *o0_out = o0;
        return n_in > o0 ? (int)(((long long)n_in - o0 + D - 1) / D) : 0;
    }

    int produced(int n_in)
    {
        if (n_in < 0) return fail(GRHIP_EINVAL, "negative item count");
        std::lock_guard<std::mutex> lk(setter_mutex);
        return produced_of(n_in, nullptr);
    }

    int composed(int n_in, const float2 *in, float *out, int *d_produced, int np, int o0, hipStream_t st)
    {
        int rc;
        const int Hh = H();
        const long long row_stride = (long long)Hh + n_in;
        if ((rc = d_row.reserve((size_t)nstreams * (size_t)row_stride * sizeof(float)))) return rc;
        float *row = d_row.as<float>();
        const AmdState s = state(cur);
        if ((rc = amd_v_launch(in, n_in, nstreams, s.hist, Hh, row, row_stride, st))) return rc;
        // gr_fir_fff_generic over every stream's row: output j reads row items o0 + j D .. o0 + j D + ntaps - 1
        if (np > 0)
            for (int sidx = 0; sidx < nstreams; ++sidx)
                if ((rc = launch_fir_generic(FIR_FFF, d_rev.as<float>(), (int)taps.size(), row + (long long)sidx * row_stride + o0,
                                             out + (long long)sidx * np, np, D, nullptr, st)))
                    return rc;
        return amd_tail_launch(n_in, nstreams, row, row_stride, Hh, s.hist, d_produced, np, st);
    }

    int work_device(int n_in, const void *d_in, void *d_out, int *d_produced, void *stream)
    {
        const int c = check_count(n_in);
        if (c < 0) return c;
        int rc = bind();
        if (rc) return rc;
        hipStream_t st = pick(stream);
        if (c == 0) {       // nothing but the count, on the caller's stream
            if (d_produced) GRHIP_HIP(hipMemsetAsync(d_produced, 0, sizeof(int), st));
            return GRHIP_OK;
        }
        if ((rc = check_io(d_in, sizeof(float2), d_out, sizeof(float)))) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        int o0;
        const int np = produced_of(n_in, &o0);      // depends on the position: under the lock
        const size_t in_bytes = (size_t)nstreams * (size_t)n_in * sizeof(float2), out_bytes = (size_t)nstreams * (size_t)np * sizeof(float);
        if ((rc = check_apart("am_demod_cf", d_in, in_bytes, d_out, out_bytes))) return rc;
        if (mode_fast(mode) && fused_ok) {
            AmdFused f;
            f.in = (const float2 *)d_in; f.out = (float *)d_out; f.n_in = n_in; f.nstreams = nstreams;
            f.produced = np; f.o0 = o0; f.D = D; f.ntaps = (int)taps.size(); f.taps = d_fwd.as<float>();
            f.rd = state(cur); f.wr = state(cur ^ 1); f.d_produced = d_produced;
            if ((rc = amd_fused_launch(f, st))) return rc;
            cur ^= 1;
        } else {
            if ((rc = composed(n_in, (const float2 *)d_in, (float *)d_out, d_produced, np, o0, st))) return rc;
        }
        pos = (int)(((long long)pos + n_in) % D);
        return GRHIP_OK;
    }

    int work(int n_in, const void *in, void *out, int *produced_out)
    {
        const int c = check_count(n_in);
        if (c < 0) return c;
        if (produced_out) *produced_out = 0;
        if (c == 0) return GRHIP_OK;
        int np;
        {
            std::lock_guard<std::mutex> lk(setter_mutex);
            np = produced_of(n_in, nullptr);
        }
        const int rc = host_work(n_in, sizeof(float2), in, (size_t)np, sizeof(float), out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n_in, d_in, d_out, nullptr, st);
        });
        if (!rc && produced_out) *produced_out = np;
        return rc;
    }
};

}  // namespace

struct grhip_am_demod_cf : AmDemodBlock {};

extern "C" {

#define GRHIP_AMD_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")

int grhip_am_demod_cf_create(grhip_am_demod_cf **h, int audio_decim, const float *audio_taps, size_t ntaps, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    int rc = AmDemodBlock::check(audio_decim, audio_taps, ntaps);
    if (rc) return rc;
    return make_handle(h, [&](grhip_am_demod_cf *b) { return b->init(audio_decim, audio_taps, ntaps, device); });
}

void grhip_am_demod_cf_destroy(grhip_am_demod_cf *h) { destroy_handle(h); }
int grhip_am_demod_cf_set_mode(grhip_am_demod_cf *h, int mode) { GRHIP_AMD_NULL(h); return h->set_mode(mode); }
int grhip_am_demod_cf_set_streams(grhip_am_demod_cf *h, int nstreams) { GRHIP_AMD_NULL(h); return h->set_streams(nstreams); }
int grhip_am_demod_cf_produced(grhip_am_demod_cf *h, int n_in) { GRHIP_AMD_NULL(h); return h->produced(n_in); }
int grhip_am_demod_cf_engine(grhip_am_demod_cf *h) { GRHIP_AMD_NULL(h); return h->engine(); }
int grhip_am_demod_cf_tile(void) { return AMD_TILE; }
int grhip_am_demod_cf_outputs_per_lane(void) { return AMD_R; }
int grhip_am_demod_cf_max_taps(void) { return AMD_MAX_HIST + 1; }

int grhip_am_demod_cf_work(grhip_am_demod_cf *h, int n_in, const void *in, void *out, int *produced)
{
    GRHIP_AMD_NULL(h);
    return h->work(n_in, in, out, produced);
}

int grhip_am_demod_cf_work_device(grhip_am_demod_cf *h, int n_in, const void *d_in, void *d_out, int *d_produced, void *stream)
{
    GRHIP_AMD_NULL(h);
    return h->work_device(n_in, d_in, d_out, d_produced, stream);
}

#undef GRHIP_AMD_NULL

}  // extern "C"
