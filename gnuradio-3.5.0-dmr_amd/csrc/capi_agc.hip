// capi_agc.hip -- C ABI of gr_agc_cc, gr_agc_ff, gr_agc2_cc and gr_agc2_ff.
//
// Reference: general/gri_agc_cc.h, gri_agc_ff.h, gri_agc2_cc.h, gri_agc2_ff.h (scale(), the accessors), around them
// general/gr_agc_cc.cc:47-56 and its three siblings (work is one scaleN).
//
// A handle takes S streams back to back ([S][n_in]).  What a stream remembers is its gain, one float on the device.  The
// parameters are kernel arguments: a setter holds from the next work call, launches already queued keep theirs.
#include <cmath>
#include <vector>

#include "agc.h"
#include "grhip_internal.h"
#include "stream_block.h"

using namespace grhip;

namespace {

struct AgcBlock : StreamBlock {
    bool cc = true;
    int law = AGC_LAW_AGC;
    AgcParams p = {1e-4f, 1e-2f, 1.0f, 0.0f};
    float gain0 = 1.0f;                 // the constructor's gain: what set_streams restarts every stream from
    DevBuf d_gain, d_scratch;           // d_gain: every stream's gain, one float

    size_t item() const { return cc ? 2 * sizeof(float) : sizeof(float); }

    int init(bool is_cc, int which, float rate, float decay, float reference, float gain, float max_gain, int dev)
    {
        cc = is_cc; law = which;
        p.rate = rate; p.decay = decay; p.reference = reference; p.max_gain = max_gain;
        gain0 = gain;
        mode = default_mode();
        int rc = init_device(dev);
        return rc ? rc : fill_state(d_gain, gain0);
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return fill_state(d_gain, gain0); });
    }

    // gri_agc_cc.h:50: the one gain of the reference's block; here every stream's
    int set_gain(float v)
    {
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        return fill_state(d_gain, v);
    }

    int get_gain(int s, float *v)
    {
        if (!v) return fail(GRHIP_EINVAL, "null argument");
        return read_state(d_gain, s, v);
    }

    int set_param(float AgcParams::*which, float v)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        p.*which = v;
        return GRHIP_OK;
    }

    float get_param(float AgcParams::*which)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return p.*which;
    }

    int work_device(int n_in, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n_in);
        if (c <= 0) return c;
        const size_t bytes = (size_t)nstreams * (size_t)n_in * item();
        int rc;
        if ((rc = check_io(d_in, item(), d_out, item())) || (rc = check_apart("agc", d_in, bytes, d_out, bytes))) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        AgcLaunch l;
        l.in = d_in; l.out = d_out; l.n = n_in; l.nstreams = nstreams; l.cc = cc; l.law = law; l.p = p;
        l.gain = d_gain.as<float>();
        const bool chunked = mode_fast(mode) && agc_can_chunk(l);
        if (chunked && (rc = d_scratch.reserve(agc_scratch_bytes(l)))) return rc;
        return agc_launch(chunked, l, d_scratch.p, st);
    }

    int work(int n_in, const void *in, void *out)
    {
        return host_work(n_in, item(), in, (size_t)n_in, item(), out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n_in, d_in, d_out, st);
        });
    }
};

}  // namespace

struct grhip_agc_cc : AgcBlock {};
struct grhip_agc_ff : AgcBlock {};
struct grhip_agc2_cc : AgcBlock {};
struct grhip_agc2_ff : AgcBlock {};

extern "C" {

#define GRHIP_AGC_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")

// what the four blocks share; NAME is agc_cc, agc_ff, agc2_cc or agc2_ff
#define GRHIP_AGC_COMMON(NAME)                                                                                        \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { GRHIP_AGC_NULL(h); return h->set_mode(mode); }           \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams) { GRHIP_AGC_NULL(h); return h->set_streams(nstreams); } \
    float grhip_##NAME##_reference(grhip_##NAME *h)                                                                   \
    {                                                                                                                 \
        if (!h) return (float)fail(GRHIP_EINVAL, "null handle");                                                      \
        return h->get_param(&AgcParams::reference);                                                                   \
    }                                                                                                                 \
    float grhip_##NAME##_max_gain(grhip_##NAME *h)                                                                    \
    {                                                                                                                 \
        if (!h) return (float)fail(GRHIP_EINVAL, "null handle");                                                      \
        return h->get_param(&AgcParams::max_gain);                                                                    \
    }                                                                                                                 \
    int grhip_##NAME##_gain(grhip_##NAME *h, int s, float *gain) { GRHIP_AGC_NULL(h); return h->get_gain(s, gain); }  \
    int grhip_##NAME##_set_reference(grhip_##NAME *h, float v) { GRHIP_AGC_NULL(h); return h->set_param(&AgcParams::reference, v); } \
    int grhip_##NAME##_set_max_gain(grhip_##NAME *h, float v) { GRHIP_AGC_NULL(h); return h->set_param(&AgcParams::max_gain, v); } \
    int grhip_##NAME##_set_gain(grhip_##NAME *h, float v) { GRHIP_AGC_NULL(h); return h->set_gain(v); }               \
    int grhip_##NAME##_work(grhip_##NAME *h, int n_in, const void *in, void *out)                                     \
    {                                                                                                                 \
        GRHIP_AGC_NULL(h);                                                                                            \
        return h->work(n_in, in, out);                                                                                \
    }                                                                                                                 \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n_in, const void *d_in, void *d_out, void *stream)            \
    {                                                                                                                 \
        GRHIP_AGC_NULL(h);                                                                                            \
        return h->work_device(n_in, d_in, d_out, stream);                                                             \
    }

// gri_agc_cc.h:38-51 / gri_agc_ff.h:37-49: one rate
#define GRHIP_AGC_ONE_RATE(NAME, CC)                                                                                  \
    int grhip_##NAME##_create(grhip_##NAME **h, float rate, float reference, float gain, float max_gain, int device)  \
    {                                                                                                                 \
        if (!h) return fail(GRHIP_EINVAL, "null argument");                                                           \
        return make_handle(h, [&](grhip_##NAME *b) {                                                                  \
            return b->init(CC, AGC_LAW_AGC, rate, 0.f, reference, gain, max_gain, device);                            \
        });                                                                                                           \
    }                                                                                                                 \
    float grhip_##NAME##_rate(grhip_##NAME *h)                                                                        \
    {                                                                                                                 \
        if (!h) return (float)fail(GRHIP_EINVAL, "null handle");                                                      \
        return h->get_param(&AgcParams::rate);                                                                        \
    }                                                                                                                 \
    int grhip_##NAME##_set_rate(grhip_##NAME *h, float v) { GRHIP_AGC_NULL(h); return h->set_param(&AgcParams::rate, v); } \
    GRHIP_AGC_COMMON(NAME)

// gri_agc2_cc.h:37-52 / gri_agc2_ff.h:38-53: attack and decay
#define GRHIP_AGC_TWO_RATES(NAME, CC)                                                                                 \
    int grhip_##NAME##_create(grhip_##NAME **h, float attack_rate, float decay_rate, float reference, float gain,     \
                              float max_gain, int device)                                                             \
    {                                                                                                                 \
        if (!h) return fail(GRHIP_EINVAL, "null argument");                                                           \
        return make_handle(h, [&](grhip_##NAME *b) {                                                                  \
            return b->init(CC, AGC_LAW_AGC2, attack_rate, decay_rate, reference, gain, max_gain, device);             \
        });                                                                                                           \
    }                                                                                                                 \
    float grhip_##NAME##_attack_rate(grhip_##NAME *h)                                                                 \
    {                                                                                                                 \
        if (!h) return (float)fail(GRHIP_EINVAL, "null handle");                                                      \
        return h->get_param(&AgcParams::rate);                                                                        \
    }                                                                                                                 \
    float grhip_##NAME##_decay_rate(grhip_##NAME *h)                                                                  \
    {                                                                                                                 \
        if (!h) return (float)fail(GRHIP_EINVAL, "null handle");                                                      \
        return h->get_param(&AgcParams::decay);                                                                       \
    }                                                                                                                 \
    int grhip_##NAME##_set_attack_rate(grhip_##NAME *h, float v) { GRHIP_AGC_NULL(h); return h->set_param(&AgcParams::rate, v); } \
    int grhip_##NAME##_set_decay_rate(grhip_##NAME *h, float v) { GRHIP_AGC_NULL(h); return h->set_param(&AgcParams::decay, v); } \
    GRHIP_AGC_COMMON(NAME)

GRHIP_AGC_ONE_RATE(agc_cc, true)
GRHIP_AGC_ONE_RATE(agc_ff, false)
GRHIP_AGC_TWO_RATES(agc2_cc, true)
GRHIP_AGC_TWO_RATES(agc2_ff, false)

int grhip_agc_chunk(void) { return AGC_CHUNK; }

#undef GRHIP_AGC_ONE_RATE
#undef GRHIP_AGC_TWO_RATES
#undef GRHIP_AGC_COMMON
#undef GRHIP_AGC_NULL

}  // extern "C"
