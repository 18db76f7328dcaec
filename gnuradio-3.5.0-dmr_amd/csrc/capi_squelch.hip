// capi_squelch.hip -- C ABI of the power squelch blocks: gr_pwr_squelch_cc, gr_pwr_squelch_ff, gr_simple_squelch_cc.
//
// Reference: general/gr_squelch_base_cc.{h,cc}, gr_squelch_base_ff.{h,cc} (the machine, general_work),
// general/gr_pwr_squelch_cc.{h,cc}, gr_pwr_squelch_ff.{h,cc} (detector, threshold), general/gr_simple_squelch_cc.{h,cc}.
//
// A handle takes S streams back to back ([S][n_in]); what a stream remembers (detector output, machine state, ramp
// position, envelope) is a SquelchState on the device and carries across calls.  set_streams restarts every stream from
// the reference's initial state; the other setters keep the state and hold from the next work call.
#include <cmath>
#include <vector>

#include "grhip_internal.h"
#include "squelch.h"

using namespace grhip;

namespace {

int check_streams(int S)
{
    return (S < 1 || S > 65535) ? fail(GRHIP_EINVAL, "1 .. 65535 streams") : GRHIP_OK;
}

int check_alpha(double alpha)
{
    // gr_single_pole_iir.h:62-63 (a NaN passes there; it is refused here)
    return (alpha >= 0.0 && alpha <= 1.0) ? GRHIP_OK : fail(GRHIP_ERANGE, "Alpha must be in [0, 1]");
}

int check_ramp(int ramp)
{
    return (ramp < 0 || ramp > SQ_MAX_RAMP) ? fail(GRHIP_EINVAL, "ramp must be 0 .. %d", SQ_MAX_RAMP) : GRHIP_OK;
}

bool aligned(const void *p, size_t a) { return !((uintptr_t)p & (a - 1)); }

}  // namespace

struct SquelchBlock : HandleBase {
    bool cc = true, simple = false, gate = false;
    int nstreams = 1, ramp = 0;
    int mode = GRHIP_MODE_FAST;
    double alpha = 0.0001, threshold = 1.0;
    DevBuf d_state, d_table, d_scratch, d_prod;

    size_t item() const { return cc ? 8 : 4; }

    // the envelope of every ramp position a stream can be at: 0.5 - cos(M_PI * k / ramp) / 2.0 in the host's double
    // arithmetic (gr_squelch_base_cc.cc:69, its "FIXME: precalculate").  An attack that starts at or past the ramp's
    // end takes one more step, hence the spare entries.  Streams drained, under setter_mutex.
    int build_table(int max_ramped)
    {
        if (ramp == 0) return GRHIP_OK;
        const size_t len = (size_t)(max_ramped > ramp ? max_ramped : ramp) + 2;
        std::vector<double> t(len);
        for (size_t k = 0; k < len; ++k) t[k] = 0.5 - std::cos(M_PI * (int)k / ramp) / 2.0;
        int rc = d_table.reserve(len * sizeof(double));
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(d_table.p, t.data(), len * sizeof(double), hipMemcpyHostToDevice));
        return GRHIP_OK;
    }

    int read_states(std::vector<SquelchState> &v)
    {
        v.resize(nstreams);
        GRHIP_HIP(hipMemcpy(v.data(), d_state.p, v.size() * sizeof(SquelchState), hipMemcpyDeviceToHost));
        return GRHIP_OK;
    }

    // gr_squelch_base_cc.cc:36-39: muted, nothing ramped, the envelope 0 with a ramp and 1 without
    int restart()
    {
        std::vector<SquelchState> v(nstreams, SquelchState{0.0, ramp ? 0.0 : 1.0, SQ_MUTED, 0});
        int rc = d_state.reserve(v.size() * sizeof(SquelchState));
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(d_state.p, v.data(), v.size() * sizeof(SquelchState), hipMemcpyHostToDevice));
        if ((rc = d_prod.reserve((size_t)nstreams * sizeof(int)))) return rc;
        return build_table(0);
    }

    int work_device(int n_in, const void *d_in, void *d_out, int *d_produced, void *stream)
    {
        if (n_in < 0) return fail(GRHIP_EINVAL, "negative item count");
        if (n_in == 0) return GRHIP_OK;
        if (!d_in || !d_out || !d_produced) return fail(GRHIP_EINVAL, "null buffer");
        if (!aligned(d_in, item()) || !aligned(d_out, item()) || !aligned(d_produced, 4))
            return fail(GRHIP_EINVAL, "items not naturally aligned");
        const char *a = (const char *)d_in, *b = (const char *)d_out;
        const size_t bytes = (size_t)nstreams * (size_t)n_in * item();
        if (a < b + bytes && b < a + bytes) return fail(GRHIP_EINVAL, "squelch: the output may not overlap the input");
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        SquelchLaunch l;
        l.in = d_in; l.out = d_out; l.produced = d_produced; l.n = n_in; l.nstreams = nstreams;
        l.cc = cc; l.simple = simple; l.gate = gate; l.ramp = ramp; l.alpha = alpha; l.threshold = threshold;
        l.state = d_state.as<SquelchState>(); l.table = d_table.as<double>();
        if ((rc = d_scratch.reserve(squelch_scratch_bytes(mode_fast(mode), l)))) return rc;
        return squelch_launch(mode_fast(mode), l, d_scratch.p, pick(stream));
    }

    // every stream's produced[s] items, from out + s * n_in; what lies behind them in `out` stays as it was
    int work(int n_in, const void *in, void *out, int *produced)
    {
        if (n_in < 0) return fail(GRHIP_EINVAL, "negative item count");
        if (n_in == 0) return GRHIP_OK;
        if (!in || !out || !produced) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        const size_t per = (size_t)n_in * item(), bytes = (size_t)nstreams * per;
        if ((rc = stage_in.reserve(bytes + 16))) return rc;
        if ((rc = stage_out.reserve(bytes + 16))) return rc;
        hipStream_t st = own_stream;
        GRHIP_H2D(this, stage_in.p, in, bytes, st);
        if ((rc = work_device(n_in, stage_in.p, stage_out.p, d_prod.as<int>(), st))) return rc;
        GRHIP_D2H(this, produced, d_prod.p, (size_t)nstreams * sizeof(int), st);
        GRHIP_HIP(hipStreamSynchronize(st));
        bool whole = true;
        for (int s = 0; s < nstreams; ++s) whole = whole && produced[s] == n_in;
        if (whole) GRHIP_D2H(this, out, stage_out.p, bytes, st);
        else
            for (int s = 0; s < nstreams; ++s)
                GRHIP_D2H(this, (char *)out + s * per, (const char *)stage_out.p + s * per, (size_t)produced[s] * item(), st);
        GRHIP_HIP(hipStreamSynchronize(st));
        return GRHIP_OK;
    }

    int set_mode(int m)
    {
        if (!mode_valid(m)) return fail(GRHIP_EINVAL, "bad mode %d", m);
        std::lock_guard<std::mutex> lk(setter_mutex);
        mode = m;
        return GRHIP_OK;
    }

    int set_streams(int S)
    {
        if (int rc = check_streams(S)) return rc;
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        nstreams = S;
        return restart();
    }

    int set_alpha(double a)
    {
        if (int rc = check_alpha(a)) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        alpha = a;                                          // kernel arguments: launches already queued keep theirs
        return GRHIP_OK;
    }

    int set_threshold(double db)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        threshold = std::pow(10.0, db / 10);                // gr_pwr_squelch_cc.h:58
        return GRHIP_OK;
    }

    int set_gate(int g)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        gate = g != 0;
        return GRHIP_OK;
    }

    // The reference keeps d_ramped and divides by the new ramp from the next sample on (gr_squelch_base_cc.h:47).
    // Ramp 0 while a stream is inside a ramp would divide by zero there (a NaN envelope): refused here.
    int set_ramp(int r)
    {
        if (int rc = check_ramp(r)) return rc;
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        std::vector<SquelchState> v;
        if ((rc = read_states(v))) return rc;
        int max_ramped = 0;
        for (const SquelchState &s : v) {
            if (r == 0 && (s.state == SQ_ATTACK || s.state == SQ_DECAY))
                return fail(GRHIP_ERANGE, "set_ramp(0) while a stream is inside a ramp");
            if (s.ramped > max_ramped) max_ramped = s.ramped;
        }
        ramp = r;
        return build_table(max_ramped);
    }

    int get_state(int s, SquelchState *out)
    {
        if (s < 0 || s >= nstreams) return fail(GRHIP_EINVAL, "stream %d of %d", s, nstreams);
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        GRHIP_HIP(hipMemcpy(out, d_state.as<SquelchState>() + s, sizeof(SquelchState), hipMemcpyDeviceToHost));
        return GRHIP_OK;
    }
};

struct grhip_pwr_squelch_cc : SquelchBlock {};
struct grhip_pwr_squelch_ff : SquelchBlock {};
struct grhip_simple_squelch_cc : SquelchBlock {};

namespace {

template <class H>
int create(H **h, bool cc, bool simple, double db, double alpha, int ramp, int gate, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (int rc = check_alpha(alpha)) return rc;
    if (int rc = check_ramp(ramp)) return rc;
    return make_handle(h, [&](H *b) {
        b->cc = cc; b->simple = simple; b->alpha = alpha; b->ramp = ramp; b->gate = gate != 0;
        b->threshold = std::pow(10.0, db / 10);
        b->mode = default_mode();
        int rc = b->init_device(device);
        return rc ? rc : b->restart();
    });
}

}  // namespace

extern "C" {

#define GRHIP_SQUELCH_COMMON(NAME)                                                                                     \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { return h ? h->set_mode(mode) : fail(GRHIP_EINVAL, "null handle"); } \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams)                                                      \
    {                                                                                                                  \
        return h ? h->set_streams(nstreams) : fail(GRHIP_EINVAL, "null handle");                                       \
    }                                                                                                                  \
    int grhip_##NAME##_set_threshold(grhip_##NAME *h, double db)                                                       \
    {                                                                                                                  \
        return h ? h->set_threshold(db) : fail(GRHIP_EINVAL, "null handle");                                           \
    }                                                                                                                  \
    int grhip_##NAME##_set_alpha(grhip_##NAME *h, double alpha)                                                        \
    {                                                                                                                  \
        return h ? h->set_alpha(alpha) : fail(GRHIP_EINVAL, "null handle");                                            \
    }                                                                                                                  \
    double grhip_##NAME##_threshold(grhip_##NAME *h)                                                                   \
    {                                                                                                                  \
        if (!h) return (double)fail(GRHIP_EINVAL, "null handle");                                                      \
        std::lock_guard<std::mutex> lk(h->setter_mutex);                                                               \
        return 10 * std::log10(h->threshold);                                                                          \
    }                                                                                                                  \
    int grhip_##NAME##_unmuted(grhip_##NAME *h, int s)                                                                 \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        SquelchState v;                                                                                                \
        if (int rc = h->get_state(s, &v)) return rc;                                                                   \
        return v.state == SQ_UNMUTED || v.state == SQ_ATTACK;                                                          \
    }                                                                                                                  \
    int grhip_##NAME##_state(grhip_##NAME *h, int s, int *state, int *ramped, double *envelope, double *y)             \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        SquelchState v;                                                                                                \
        if (int rc = h->get_state(s, &v)) return rc;                                                                   \
        if (state) *state = v.state;                                                                                   \
        if (ramped) *ramped = v.ramped;                                                                                \
        if (envelope) *envelope = v.envelope;                                                                          \
        if (y) *y = v.y;                                                                                               \
        return GRHIP_OK;                                                                                               \
    }                                                                                                                  \
    int grhip_##NAME##_work(grhip_##NAME *h, int n_in, const void *in, void *out, int *produced)                       \
    {                                                                                                                  \
        return h ? h->work(n_in, in, out, produced) : fail(GRHIP_EINVAL, "null handle");                               \
    }                                                                                                                  \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n_in, const void *d_in, void *d_out, int *d_produced,          \
                                   void *stream)                                                                       \
    {                                                                                                                  \
        return h ? h->work_device(n_in, d_in, d_out, d_produced, stream) : fail(GRHIP_EINVAL, "null handle");          \
    }

#define GRHIP_SQUELCH_RAMP(NAME)                                                                                       \
    GRHIP_SQUELCH_COMMON(NAME)                                                                                         \
    int grhip_##NAME##_set_ramp(grhip_##NAME *h, int ramp) { return h ? h->set_ramp(ramp) : fail(GRHIP_EINVAL, "null handle"); } \
    int grhip_##NAME##_set_gate(grhip_##NAME *h, int gate) { return h ? h->set_gate(gate) : fail(GRHIP_EINVAL, "null handle"); } \
    int grhip_##NAME##_ramp(grhip_##NAME *h)                                                                           \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        std::lock_guard<std::mutex> lk(h->setter_mutex);                                                               \
        return h->ramp;                                                                                                \
    }                                                                                                                  \
    int grhip_##NAME##_gate(grhip_##NAME *h)                                                                           \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        std::lock_guard<std::mutex> lk(h->setter_mutex);                                                               \
        return h->gate ? 1 : 0;                                                                                        \
    }

// ---- gr_pwr_squelch_cc (gr_pwr_squelch_cc.cc:29-56, gr_squelch_base_cc.cc:30-93) ----------------------------------------
int grhip_pwr_squelch_cc_create(grhip_pwr_squelch_cc **h, double db, double alpha, int ramp, int gate, int device)
{
    return create(h, true, false, db, alpha, ramp, gate, device);
}
GRHIP_SQUELCH_RAMP(pwr_squelch_cc)

// ---- gr_pwr_squelch_ff (gr_pwr_squelch_ff.cc:29-56, gr_squelch_base_ff.cc:30-93) ----------------------------------------
int grhip_pwr_squelch_ff_create(grhip_pwr_squelch_ff **h, double db, double alpha, int ramp, int gate, int device)
{
    return create(h, false, false, db, alpha, ramp, gate, device);
}
GRHIP_SQUELCH_RAMP(pwr_squelch_ff)

// ---- gr_simple_squelch_cc (gr_simple_squelch_cc.cc:31-108) ---------------------------------------------------------------
int grhip_simple_squelch_cc_create(grhip_simple_squelch_cc **h, double threshold_db, double alpha, int device)
{
    return create(h, true, true, threshold_db, alpha, 0, 0, device);
}
GRHIP_SQUELCH_COMMON(simple_squelch_cc)

int grhip_pwr_squelch_chunk(void) { return SQ_CHUNK; }

#undef GRHIP_SQUELCH_RAMP
#undef GRHIP_SQUELCH_COMMON

}  // extern "C"
