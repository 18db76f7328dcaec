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
#include "squelch_block.h"

using namespace grhip;

namespace {

int check_alpha(double alpha)
{
    // gr_single_pole_iir.h:62-63 (a NaN passes there; it is refused here)
    return (alpha >= 0.0 && alpha <= 1.0) ? GRHIP_OK : fail(GRHIP_ERANGE, "Alpha must be in [0, 1]");
}

}  // namespace

// the machine, the envelope table and their setters are SquelchMachine's (squelch_block.h)
struct SquelchBlock : SquelchMachine {
    bool cc = true, simple = false;
    double alpha = 0.0001, threshold = 1.0;

    size_t item() const { return cc ? 8 : 4; }

    int restart() { return restart_machine(); }

    int work_device(int n_in, const void *d_in, void *d_out, int *d_produced, void *stream)
    {
        const int c = check_count(n_in);
        if (c <= 0) return c;
        int rc = check_work(n_in, d_in, d_out, d_produced, item());
        if (rc) return rc;
        if ((rc = bind())) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        SquelchLaunch l;
        l.in = d_in; l.out = d_out; l.produced = d_produced; l.n = n_in; l.nstreams = nstreams;
        l.cc = cc; l.simple = simple; l.gate = gate; l.ramp = ramp; l.alpha = alpha; l.threshold = threshold;
        l.state = d_state.as<SquelchState>(); l.table = d_table.as<double>();
        if ((rc = d_scratch.reserve(squelch_scratch_bytes(mode_fast(mode), l)))) return rc;
        return squelch_launch(mode_fast(mode), l, d_scratch.p, pick(stream));
    }

    int work(int n_in, const void *in, void *out, int *produced)
    {
        return host_work(n_in, in, out, produced, item(), [&](int n, const void *d_in, void *d_out, int *d_p, hipStream_t st) {
            return work_device(n, d_in, d_out, d_p, st);
        });
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
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
    if (int rc = squelch_check_ramp(ramp)) return rc;
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
