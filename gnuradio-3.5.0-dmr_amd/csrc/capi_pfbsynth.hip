// capi_pfbsynth.hip -- gr_pfb_synthesis_filterbank_ccf: handle and C ABI.
//
// Reference (gnuradio-core/src/lib/filter/):
//   gr_pfb_synthesis_filterbank_ccf.cc:41-62 (constructor: a gr_sync_interpolator by numchans, 1..numchans inputs, a
//   FORWARD gri_fft_complex(numchans, true)), 71-106 (set_taps: tpf = ceil(ntaps/numchans), zeros at the END, branch i
//   gets tmp[i + j*numchans], set_history(tpf + 1)), 122-169 (work: bin filling with the `(in+i)[n]` offset, the DFT,
//   out[M-1-i] = filters[M-1-i]->filter(outbuf[i])); gri_fir_filter_with_buffer_XXX.cc.t:41-78 (set_taps reverses the
//   taps and zeroes the delay line; filter(x): one accumulator, oldest sample first).
//
// The delay lines live across work calls: the handle keeps, per branch, the last tpf - 1 DFT outputs in device memory
// (two buffers, swapped by every call: a launch reads one and writes the other).  Nothing depends on the data, so the
// device entry never waits for the device.
#include <cmath>
#include <cstring>
#include <vector>

#include "grhip_internal.h"
#include "pfb_synth.h"
#include "stream_block.h"

using namespace grhip;

struct grhip_pfb_synthesis_filterbank_ccf : ModeBlock {
    int M = 1, tpf = 1;
    std::vector<float> new_taps;        // latched by set_taps
    bool updated = false;
    DevBuf d_taps, d_tw, d_state[2], d_scratch;
    int cur = 0;                        // d_state[cur] holds the delay lines

    static int check_taps(int M, const float *taps, size_t ntaps)
    {
        if (ntaps == 0)
            return fail(GRHIP_EINVAL, "pfb_synthesis_filterbank: no taps (branches of 0 taps: outside the reference's "
                                      "defined behaviour)");
        if (!taps) return fail(GRHIP_EINVAL, "null taps");
        if ((ntaps + M - 1) / M > (size_t)SY_MAX_TPF)
            return fail(GRHIP_EINVAL, "pfb_synthesis_filterbank: more than %d taps per filter", SY_MAX_TPF);
        return GRHIP_OK;
    }

    // set_taps (.cc:71-106) as the filters see it: reversed branches (with_buffer's set_taps), zero delay lines
    int install(const std::vector<float> &taps)
    {
        const size_t ntaps = taps.size();
        tpf = (int)((ntaps + M - 1) / M);
        std::vector<float> padded((size_t)M * tpf, 0.f);
        memcpy(padded.data(), taps.data(), ntaps * sizeof(float));
        // [M][tpf] reversed branches, then the same as [tpf][M] (pfb_synth.h)
        std::vector<float> bank(2 * (size_t)M * tpf);
        float *rev = bank.data(), *tr = bank.data() + (size_t)M * tpf;
        for (int f = 0; f < M; ++f)
            for (int k = 0; k < tpf; ++k) {
                const float h = padded[(size_t)f + (size_t)(tpf - 1 - k) * M];
                rev[(size_t)f * tpf + k] = h;
                tr[(size_t)k * M + f] = h;
            }
        int rc = d_taps.reserve(bank.size() * sizeof(float));
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(d_taps.p, bank.data(), bank.size() * sizeof(float), hipMemcpyHostToDevice));
        const size_t sb = (size_t)(tpf - 1) * M * sizeof(float2);
        for (DevBuf &s : d_state) {
            if ((rc = s.reserve(sb + 16))) return rc;
            if ((rc = zero_device(s.p, sb + 16))) return rc;
        }
        cur = 0;
        return GRHIP_OK;
    }

    int init(unsigned numchans, const float *taps, size_t ntaps, int dev)
    {
        if (numchans == 0) return fail(GRHIP_EINVAL, "pfb_synthesis_filterbank: numchans must be > 0");
        if (numchans > (unsigned)SY_MAX_CHANS)
            return fail(GRHIP_EINVAL, "pfb_synthesis_filterbank: numchans %u above the kernels' limit %d", numchans, SY_MAX_CHANS);
        M = (int)numchans;
        int rc = check_taps(M, taps, ntaps);
        if (rc) return rc;
        if ((rc = init_device(dev))) return rc;
        mode = default_mode();
        // e^{-2 pi j k/M}; the quarter turns exact, so that M = 1, 2, 4 transform without rounding
        std::vector<float2> tw((size_t)M);
        for (int k = 0; k < M; ++k) {
            if ((4 * k) % M == 0) {
                static const float2 q[4] = {{1.f, 0.f}, {0.f, -1.f}, {-1.f, 0.f}, {0.f, 1.f}};
                tw[k] = q[4 * k / M];
            } else {
                const double ang = -2.0 * M_PI * (double)k / (double)M;
                tw[k] = make_float2((float)cos(ang), (float)sin(ang));
            }
        }
        if ((rc = d_tw.reserve(tw.size() * sizeof(float2)))) return rc;
        GRHIP_HIP(hipMemcpy(d_tw.p, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
        return install(std::vector<float>(taps, taps + ntaps));      // the constructor installs the taps (.cc:58)
    }

    int set_taps(const float *taps, size_t ntaps)
    {
        int rc = check_taps(M, taps, ntaps);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        new_taps.assign(taps, taps + ntaps);
        updated = true;
        return GRHIP_OK;
    }

    int check_call(int noutput_items, int numsigs) const
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        if (numsigs < 1 || numsigs > M)
            return fail(GRHIP_EINVAL, "pfb_synthesis_filterbank: %d input streams, the block takes 1 to %d", numsigs, M);
        if (noutput_items % M)
            return fail(GRHIP_EINVAL, "pfb_synthesis_filterbank: noutput_items %d is not a multiple of numchans %d "
                                      "(output_multiple)", noutput_items, M);
        return GRHIP_OK;
    }

    // bin M-1 reads item n + M - 1 of its stream; the scheduler provides items up to n + tpf
    int check_range(int numsigs) const
    {
        if (numsigs >= 2 && M - 1 > tpf)
            return fail(GRHIP_EINVAL, "pfb_synthesis_filterbank: %d streams into %d channels with %d taps per filter: "
                                      "the reference reads past its input (needs taps per filter >= numchans - 1)",
                        numsigs, M, tpf);
        return GRHIP_OK;
    }

    int work_device(int noutput_items, const void *d_in, size_t stride, int numsigs, void *d_out, void *stream)
    {
        int rc = check_call(noutput_items, numsigs);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        if (updated) {                                   // .cc:133-136; the new filters start from zero delay lines
            if ((rc = drain(st))) return rc;
            if ((rc = install(new_taps))) return rc;
            updated = false;
            return 0;
        }
        if ((rc = check_range(numsigs))) return rc;
        if (noutput_items == 0) return 0;
        if (!d_in || !d_out) return fail(GRHIP_EINVAL, "null buffer");
        const long long nvec = noutput_items / M;
        if (numsigs > 1 && stride < (size_t)(nvec + tpf))
            return fail(GRHIP_EINVAL, "pfb_synthesis_filterbank: stream_stride_items below the %lld items a stream holds",
                        nvec + tpf);
        PfbSynthArgs a;
        a.M = M; a.tpf = tpf; a.numsigs = numsigs;
        a.in = (const float2 *)d_in; a.stride = (long long)stride; a.in_items = nvec + tpf;
        a.out = (float2 *)d_out; a.nvec = nvec;
        a.taps_rev = d_taps.as<float>(); a.taps_t = d_taps.as<float>() + (size_t)M * tpf;
        a.tw = d_tw.as<float2>();
        a.state_old = d_state[cur].as<float2>(); a.state_new = d_state[cur ^ 1].as<float2>();
        if (!pfb_synth_fused(M, tpf)) {
            if ((rc = d_scratch.reserve((size_t)(nvec + tpf - 1) * M * sizeof(float2)))) return rc;
            a.scratch = d_scratch.as<float2>();
        }
        if ((rc = launch_pfb_synth(a, !mode_fast(mode), st))) return rc;
        cur ^= 1;
        return noutput_items;
    }

    int work(int noutput_items, const void *const *ins, int numsigs, void *out)
    {
        int rc = check_call(noutput_items, numsigs);
        if (rc) return rc;
        if (!ins || (!out && noutput_items)) return fail(GRHIP_EINVAL, "null buffer");
        if ((rc = bind())) return rc;
        // every stream holds noutput_items/M + tpf items (history tpf + 1); a call that installs new taps reads nothing
        size_t per;
        {
            std::lock_guard<std::mutex> lk(setter_mutex);
            if (!updated && (rc = check_range(numsigs))) return rc;
            per = updated || noutput_items == 0 ? 0 : (size_t)(noutput_items / M) + tpf;
        }
        if ((rc = stage_in.reserve(per * numsigs * sizeof(float2) + 16))) return rc;
        if ((rc = stage_out.reserve((size_t)noutput_items * sizeof(float2) + 16))) return rc;
        hipStream_t st = own_stream;
        if (per)
            for (int s = 0; s < numsigs; ++s) {
                if (!ins[s]) return fail(GRHIP_EINVAL, "null input stream %d", s);
                GRHIP_H2D(this, stage_in.as<float2>() + (size_t)s * per, ins[s], per * sizeof(float2), st);
            }
        const int n = work_device(noutput_items, stage_in.p, per, numsigs, stage_out.p, st);
        if (n < 0) return n;
        GRHIP_D2H(this, out, stage_out.p, (size_t)n * sizeof(float2), st);
        GRHIP_HIP(hipStreamSynchronize(st));
        return n;
    }

    ~grhip_pfb_synthesis_filterbank_ccf() { if (own_stream) (void)hipStreamSynchronize(own_stream); }   // then the buffers go
};

extern "C" {

int grhip_pfb_synthesis_filterbank_ccf_create(grhip_pfb_synthesis_filterbank_ccf **h, unsigned numchans,
                                              const float *taps, size_t ntaps, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle pointer");
    *h = nullptr;
    return make_handle(h, [&](grhip_pfb_synthesis_filterbank_ccf *b) { return b->init(numchans, taps, ntaps, device); });
}

void grhip_pfb_synthesis_filterbank_ccf_destroy(grhip_pfb_synthesis_filterbank_ccf *h)
{
    destroy_handle(h);
}

int grhip_pfb_synthesis_filterbank_ccf_set_taps(grhip_pfb_synthesis_filterbank_ccf *h, const float *taps, size_t ntaps)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->set_taps(taps, ntaps);
}

int grhip_pfb_synthesis_filterbank_ccf_set_mode(grhip_pfb_synthesis_filterbank_ccf *h, int mode)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->set_mode(mode);
}

int grhip_pfb_synthesis_filterbank_ccf_history(const grhip_pfb_synthesis_filterbank_ccf *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->tpf + 1;                                   // .cc:103
}

int grhip_pfb_synthesis_filterbank_ccf_taps_per_filter(const grhip_pfb_synthesis_filterbank_ccf *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->tpf;
}

int grhip_pfb_synthesis_filterbank_ccf_numchans(const grhip_pfb_synthesis_filterbank_ccf *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->M;
}

int grhip_pfb_synthesis_filterbank_ccf_work(grhip_pfb_synthesis_filterbank_ccf *h, int noutput_items,
                                            const void *const *ins, int numsigs, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work(noutput_items, ins, numsigs, out);
}

int grhip_pfb_synthesis_filterbank_ccf_work_device(grhip_pfb_synthesis_filterbank_ccf *h, int noutput_items,
                                                   const void *d_in, size_t stream_stride_items, int numsigs,
                                                   void *d_out, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    return h->work_device(noutput_items, d_in, stream_stride_items, numsigs, d_out, stream);
}

}  // extern "C"
