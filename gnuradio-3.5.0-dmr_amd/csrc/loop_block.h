// loop_block.h -- what the handles built on gri_control_loop share (capi_carrier.hip, capi_fll.hip): the loop's
// parameters on the host, every stream's phase and frequency on the device, gri_control_loop's setters and getters, and
// the macro that gives a block their C entries.  Not part of the ABI.
#pragma once
#include "carrier.h"
#include "control_loop.h"
#include "grhip_internal.h"
#include "stream_block.h"

namespace grhip {

struct LoopBlock : StreamBlock {
    ControlLoop cl;
    DevBuf d_state;                     // every stream's CarrierState

    int zero_loop_state() { return fill_state(d_state, CarrierState{0.f, 0.f, 0.f, 0.f}); }     // gri_control_loop.cc:35

    // a setter of the loop's parameters (control_loop.h): false is the reference's std::out_of_range
    int set_param(bool (ControlLoop::*set)(float), float v, const char *what)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        if (!(cl.*set)(v)) return fail(GRHIP_EINVAL, "gri_control_loop: invalid %s", what);
        return GRHIP_OK;
    }

    float get_param(float ControlLoop::*which)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return cl.*which;
    }

    // one float of every stream's state = v
    int set_state(float CarrierState::*which, float v)
    {
        return edit_states<CarrierState>(d_state, [&](CarrierState &e) { e.*which = v; });
    }

    int set_frequency(float f)              // gri_control_loop.cc:126-135
    {
        float v;
        {
            std::lock_guard<std::mutex> lk(setter_mutex);
            v = cl.set_frequency(f);
        }
        return set_state(&CarrierState::freq, v);
    }

    int set_phase(float ph)                 // gri_control_loop.cc:137-145
    {
        if (!ControlLoop::phase_ok(ph)) return fail(GRHIP_EINVAL, "control loop: the phase must be finite and within +-2^20 rad");
        return set_state(&CarrierState::phase, ControlLoop::set_phase(ph));
    }

    int get_float(int s, float CarrierState::*which, float *v)
    {
        if (!v) return fail(GRHIP_EINVAL, "null argument");
        CarrierState t;
        int rc = read_state(d_state, s, &t);
        if (!rc) *v = t.*which;
        return rc;
    }
};

}  // namespace grhip

#define GRHIP_CL_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")
#define GRHIP_CL_GET(NAME, ENTRY, FIELD)                                                                              \
    float grhip_##NAME##_##ENTRY(grhip_##NAME *h)                                                                     \
    {                                                                                                                 \
        if (!h) return (float)fail(GRHIP_EINVAL, "null handle");                                                      \
        return h->get_param(&ControlLoop::FIELD);                                                                     \
    }

// what the blocks share: gri_control_loop.h:99-200
#define GRHIP_CL_COMMON(NAME)                                                                                         \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { GRHIP_CL_NULL(h); return h->set_mode(mode); }            \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams) { GRHIP_CL_NULL(h); return h->set_streams(nstreams); } \
    int grhip_##NAME##_set_loop_bandwidth(grhip_##NAME *h, float bw)                                                  \
    {                                                                                                                 \
        GRHIP_CL_NULL(h);                                                                                             \
        return h->set_param(&ControlLoop::set_loop_bandwidth, bw, "bandwidth. Must be >= 0 (and leave finite gains).");  \
    }                                                                                                                 \
    int grhip_##NAME##_set_damping_factor(grhip_##NAME *h, float df)                                                  \
    {                                                                                                                 \
        GRHIP_CL_NULL(h);                                                                                             \
        return h->set_param(&ControlLoop::set_damping_factor, df, "damping factor. Must be in [0,1].");               \
    }                                                                                                                 \
    int grhip_##NAME##_set_alpha(grhip_##NAME *h, float alpha)                                                        \
    {                                                                                                                 \
        GRHIP_CL_NULL(h);                                                                                             \
        return h->set_param(&ControlLoop::set_alpha, alpha, "alpha. Must be in [0,1].");                              \
    }                                                                                                                 \
    int grhip_##NAME##_set_beta(grhip_##NAME *h, float beta)                                                          \
    {                                                                                                                 \
        GRHIP_CL_NULL(h);                                                                                             \
        return h->set_param(&ControlLoop::set_beta, beta, "beta. Must be in [0,1].");                                 \
    }                                                                                                                 \
    int grhip_##NAME##_set_frequency(grhip_##NAME *h, float freq) { GRHIP_CL_NULL(h); return h->set_frequency(freq); } \
    int grhip_##NAME##_set_phase(grhip_##NAME *h, float phase) { GRHIP_CL_NULL(h); return h->set_phase(phase); }      \
    GRHIP_CL_GET(NAME, get_loop_bandwidth, loop_bw)                                                                   \
    GRHIP_CL_GET(NAME, get_damping_factor, damping)                                                                   \
    GRHIP_CL_GET(NAME, get_alpha, alpha)                                                                              \
    GRHIP_CL_GET(NAME, get_beta, beta)                                                                                \
    int grhip_##NAME##_get_frequency(grhip_##NAME *h, int s, float *freq)                                             \
    {                                                                                                                 \
        GRHIP_CL_NULL(h);                                                                                             \
        return h->get_float(s, &CarrierState::freq, freq);                                                            \
    }                                                                                                                 \
    int grhip_##NAME##_get_phase(grhip_##NAME *h, int s, float *phase)                                                \
    {                                                                                                                 \
        GRHIP_CL_NULL(h);                                                                                             \
        return h->get_float(s, &CarrierState::phase, phase);                                                          \
    }
