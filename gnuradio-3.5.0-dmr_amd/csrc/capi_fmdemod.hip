// capi_fmdemod.hip -- C ABI of the FM demodulator hier block, blks2.fm_demod_cf and blks2.nbfm_rx
// (blks2impl/fm_demod.py:51-72, nbfm_rx.py:67-88): gr_quadrature_demod_cf(k) -> fm_deemph, one gr_iir_filter_ffd
// (fm_emph.py:44-72) -> gr_fir_filter_fff(audio_decim, audio_taps).
//
// The handle is the hier block as the scheduler runs it: new items only, every inner block from a zero history.  Per
// stream the device keeps the last complex sample, the IIR's delay lines and the FIR's ntaps - 1 de-emphasised floats;
// the stream position modulo the decimation is the same for every stream and kept on the host.
#include <cmath>
#include <vector>

#include "fir_kernels.h"
#include "fm_demod.h"
#include "grhip_internal.h"
#include "iir.h"
#include "stream_block.h"

using namespace grhip;

namespace {

constexpr int FMD_MAX_DECIM = 1 << 16;
constexpr int FMD_MAX_TAPS = 1 << 16;

struct FmDemodBlock : StreamBlock {
    float k = 1.f;
    std::vector<double> ff, fb;         // the de-emphasis taps; both empty: none
    int D = 1;
    std::vector<float> taps;            // forward order
    int pos = 0;                        // items taken so far, modulo D
    int cur = 0;                        // which copy of the state is current
    bool deemph = false, fused_ok = false, iir_chunk = false;
    int W0 = 0;
    double b0 = 0, b1 = 0, a1 = 0;
    IirCarry carry = {};
    const DeviceTables *tabs = nullptr;
    DevBuf d_iirtaps, d_fwd, d_rev, d_last, d_xs, d_ys, d_hist, d_q, d_row, d_scratch;

    int H() const { return (int)taps.size() - 1; }
    size_t hist_row() const { return (size_t)(H() > 0 ? H() : 1); }

    FmdState state(int which) const
    {
        FmdState s;
        s.last = d_last.as<float2>() + (size_t)which * nstreams;
        s.xs = d_xs.as<float>() + (size_t)which * nstreams * IIR_HIST;
        s.ys = d_ys.as<double>() + (size_t)which * nstreams * IIR_HIST;
        s.hist = d_hist.as<float>() + (size_t)which * nstreams * hist_row();
        return s;
    }

    // every inner block back at a zero history; streams drained, under setter_mutex
    int zero_state()
    {
        int rc;
        const size_t S = (size_t)nstreams;
        const size_t sizes[4] = {2 * S * sizeof(float2), 2 * S * IIR_HIST * sizeof(float), 2 * S * IIR_HIST * sizeof(double),
                                 2 * S * hist_row() * sizeof(float)};
        DevBuf *bufs[4] = {&d_last, &d_xs, &d_ys, &d_hist};
        for (int i = 0; i < 4; ++i) {
            if ((rc = bufs[i]->reserve(sizes[i]))) return rc;
            if ((rc = zero_device(bufs[i]->p, sizes[i]))) return rc;
        }
        pos = 0; cur = 0;
        return GRHIP_OK;
    }

    static int check(const double *fft, size_t n, const double *fbt, size_t m, int decim, const float *at, size_t ntaps)
    {
        if ((n && !fft) || (m && !fbt) || !at) return fail(GRHIP_EINVAL, "null taps");
        if (n > (size_t)IIR_MAX_TAPS || m > (size_t)IIR_MAX_TAPS)
            return fail(GRHIP_EINVAL, "fm_demod_cf: at most %d de-emphasis taps on either side", IIR_MAX_TAPS);
        if ((n == 0) != (m == 0))
            return fail(GRHIP_EINVAL, "fm_demod_cf: de-emphasis needs taps on both sides (none on both: no de-emphasis)");
        if (decim < 1 || decim > FMD_MAX_DECIM) return fail(GRHIP_EINVAL, "fm_demod_cf: audio_decim 1 .. %d", FMD_MAX_DECIM);
        if (ntaps < 1 || ntaps > (size_t)FMD_MAX_TAPS) return fail(GRHIP_EINVAL, "fm_demod_cf: 1 .. %d audio taps", FMD_MAX_TAPS);
        return GRHIP_OK;
    }

    int init(float gain, const double *fft, size_t n, const double *fbt, size_t m, int decim, const float *at, size_t ntaps, int dev)
    {
        int rc = check(fft, n, fbt, m, decim, at, ntaps);
        if (rc) return rc;
        k = gain; D = decim;
        ff.assign(fft, fft + n); fb.assign(fbt, fbt + m);
        taps.assign(at, at + ntaps);
        deemph = n > 0;
        mode = default_mode();
        if ((rc = init_device(dev))) return rc;
        if ((rc = get_device_tables(dev, &tabs))) return rc;
        // the fused kernel's conditions (include/grhip.h)
        fused_ok = H() <= FMD_MAX_HIST;
        if (deemph) {
            b0 = ff[0]; b1 = n > 1 ? ff[1] : 0.0; a1 = m > 1 ? fb[1] : 0.0;
            bool ok = n <= 2 && m <= 2 && std::isfinite(b0) && std::isfinite(b1) && std::isfinite(a1) && std::fabs(a1) < 1.0;
            if (ok) {
                const double w = a1 == 0.0 ? 1.0 : std::ceil(60.0 * std::log(2.0) / -std::log(std::fabs(a1)));
                ok = w <= FMD_TILE / 8;
                W0 = ok ? (w < 1.0 ? 1 : (int)w) : 0;
            }
            fused_ok = fused_ok && ok;
            // the composed path's IIR: the chunked form where iir_filter_ffd would take it
            iir_chunk = iir_plan(ff, fb, &carry);
            std::vector<double> t(2 * IIR_MAX_TAPS, 0.0);
            std::copy(ff.begin(), ff.end(), t.begin());
            std::copy(fb.begin(), fb.end(), t.begin() + IIR_MAX_TAPS);
            if ((rc = d_iirtaps.reserve(t.size() * sizeof(double)))) return rc;
            GRHIP_HIP(hipMemcpy(d_iirtaps.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        std::vector<float> rev(taps.rbegin(), taps.rend());
        if ((rc = d_fwd.reserve(taps.size() * sizeof(float)))) return rc;
        if ((rc = d_rev.reserve(taps.size() * sizeof(float)))) return rc;
        GRHIP_HIP(hipMemcpy(d_fwd.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
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

    int composed(int n_in, const float2 *in, float *out, int *d_produced, int np, int o0, bool fast, hipStream_t st)
    {
        int rc;
        const int Hh = H();
        const long long row_stride = (long long)Hh + n_in;
        const size_t S = (size_t)nstreams;
        if ((rc = d_row.reserve(S * (size_t)row_stride * sizeof(float)))) return rc;
        float *row = d_row.as<float>();
        const FmdState s = state(cur);
        if ((rc = fmd_hist_in_launch(s.hist, Hh, nstreams, row, row_stride, st))) return rc;
        if (!deemph) {
            if ((rc = fmd_demod_launch(in, n_in, nstreams, k, tabs->atan_tab, s.last, row + Hh, row_stride, st))) return rc;
        } else {
            if ((rc = d_q.reserve(S * (size_t)n_in * sizeof(float)))) return rc;
            if ((rc = fmd_demod_launch(in, n_in, nstreams, k, tabs->atan_tab, s.last, d_q.as<float>(), n_in, st))) return rc;
            IirLaunch l;
            l.in = d_q.as<float>(); l.out = row + Hh; l.in_stride = n_in; l.out_stride = row_stride;
            l.n_items = n_in; l.nstreams = nstreams; l.n = (int)ff.size(); l.m = (int)fb.size();
            l.taps = d_iirtaps.as<double>(); l.xstate = s.xs; l.ystate = s.ys;
            if (fast && iir_chunk && n_in > IIR_CHUNK) {
                if ((rc = d_scratch.reserve(iir_scratch_bytes(l)))) return rc;
                rc = iir_chunked_launch(l, carry, d_scratch.p, st);
            } else {
                rc = iir_walk_launch(l, st);
            }
            if (rc) return rc;
        }
        // gr_fir_fff_generic over every stream's row: output j reads row items o0 + j D .. o0 + j D + ntaps - 1
        if (np > 0)
            for (int sidx = 0; sidx < nstreams; ++sidx)
                if ((rc = launch_fir_generic(FIR_FFF, d_rev.as<float>(), (int)taps.size(), row + (long long)sidx * row_stride + o0,
                                             out + (long long)sidx * np, np, D, nullptr, st)))
                    return rc;
        return fmd_tail_launch(in, n_in, nstreams, row, row_stride, Hh, s.last, s.hist, d_produced, np, st);
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
        if ((rc = check_apart("fm_demod_cf", d_in, in_bytes, d_out, out_bytes))) return rc;
        const bool fast = mode_fast(mode);
        if (fast && fused_ok) {
            FmdFused f;
            f.in = (const float2 *)d_in; f.out = (float *)d_out; f.n_in = n_in; f.nstreams = nstreams;
            f.produced = np; f.o0 = o0; f.D = D; f.ntaps = (int)taps.size(); f.taps = d_fwd.as<float>();
            f.gain = k; f.atan_tab = tabs->atan_tab; f.deemph = deemph ? 1 : 0; f.b0 = b0; f.b1 = b1; f.a1 = a1; f.W0 = W0;
            f.rd = state(cur); f.wr = state(cur ^ 1); f.d_produced = d_produced;
            if ((rc = fmd_fused_launch(f, st))) return rc;
            cur ^= 1;
        } else {
            if ((rc = composed(n_in, (const float2 *)d_in, (float *)d_out, d_produced, np, o0, fast, st))) return rc;
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

struct grhip_fm_demod_cf : FmDemodBlock {};

extern "C" {

#define GRHIP_FMD_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")

int grhip_fm_demod_cf_create(grhip_fm_demod_cf **h, float k, const double *fftaps, size_t n, const double *fbtaps, size_t m,
                             int audio_decim, const float *audio_taps, size_t ntaps, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    int rc = FmDemodBlock::check(fftaps, n, fbtaps, m, audio_decim, audio_taps, ntaps);
    if (rc) return rc;
    return make_handle(h, [&](grhip_fm_demod_cf *b) { return b->init(k, fftaps, n, fbtaps, m, audio_decim, audio_taps, ntaps, device); });
}

void grhip_fm_demod_cf_destroy(grhip_fm_demod_cf *h) { destroy_handle(h); }
int grhip_fm_demod_cf_set_mode(grhip_fm_demod_cf *h, int mode) { GRHIP_FMD_NULL(h); return h->set_mode(mode); }
int grhip_fm_demod_cf_set_streams(grhip_fm_demod_cf *h, int nstreams) { GRHIP_FMD_NULL(h); return h->set_streams(nstreams); }
int grhip_fm_demod_cf_produced(grhip_fm_demod_cf *h, int n_in) { GRHIP_FMD_NULL(h); return h->produced(n_in); }
int grhip_fm_demod_cf_engine(grhip_fm_demod_cf *h) { GRHIP_FMD_NULL(h); return h->engine(); }
int grhip_fm_demod_cf_tile(void) { return FMD_TILE; }

int grhip_fm_demod_cf_work(grhip_fm_demod_cf *h, int n_in, const void *in, void *out, int *produced)
{
    GRHIP_FMD_NULL(h);
    return h->work(n_in, in, out, produced);
}

int grhip_fm_demod_cf_work_device(grhip_fm_demod_cf *h, int n_in, const void *d_in, void *d_out, int *d_produced, void *stream)
{
    GRHIP_FMD_NULL(h);
    return h->work_device(n_in, d_in, d_out, d_produced, stream);
}

#undef GRHIP_FMD_NULL

}  // extern "C"
