// squelch_block.h -- what the squelch handles share (internal): the streams' machine state on the device, the envelope
// table and the setters of gr_squelch_base_cc / _ff (general/gr_squelch_base_cc.h:40-50).  capi_squelch.hip puts the
// power detector on it, capi_ctcss.hip the tone detector.
#pragma once
#include <cmath>
#include <vector>

#include "grhip_internal.h"
#include "squelch.h"
#include "stream_block.h"

namespace grhip {

inline int squelch_check_ramp(int ramp)
{
    return (ramp < 0 || ramp > SQ_MAX_RAMP) ? fail(GRHIP_EINVAL, "ramp must be 0 .. %d", SQ_MAX_RAMP) : GRHIP_OK;
}

struct SquelchMachine : StreamBlock {
    bool gate = false;
    int ramp = 0;
    DevBuf d_state, d_table, d_scratch, d_prod;     // d_state: every stream's SquelchState

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

    // gr_squelch_base_cc.cc:36-39: muted, nothing ramped, the envelope 0 with a ramp and 1 without
    int restart_machine()
    {
        int rc = fill_state(d_state, SquelchState{0.0, ramp ? 0.0 : 1.0, SQ_MUTED, 0});
        if (rc) return rc;
        if ((rc = d_prod.reserve((size_t)nstreams * sizeof(int)))) return rc;
        return build_table(0);
    }

    // the checks every work_device makes before it binds the device; `item` is the size of one item
    int check_work(int n_in, const void *d_in, void *d_out, const int *d_produced, size_t item) const
    {
        if (!d_produced) return fail(GRHIP_EINVAL, "null buffer");
        if (int rc = check_io(d_in, item, d_out, item)) return rc;
        if (!aligned(d_produced, 4)) return fail(GRHIP_EINVAL, "items not naturally aligned");
        const size_t bytes = (size_t)nstreams * (size_t)n_in * item;
        return check_apart("squelch", d_in, bytes, d_out, bytes);
    }

    // The host-buffer call around work_device(n_in, d_in, d_out, d_produced, stream): every stream's produced[s] items,
    // from out + s * n_in; what lies behind them in `out` stays as it was.
    template <class WorkDevice>
    int host_work(int n_in, const void *in, void *out, int *produced, size_t item, WorkDevice &&work_device)
    {
        const int c = check_count(n_in);
        if (c <= 0) return c;
        if (!in || !out || !produced) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        const size_t per = (size_t)n_in * item, bytes = (size_t)nstreams * per;
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
                GRHIP_D2H(this, (char *)out + s * per, (const char *)stage_out.p + s * per, (size_t)produced[s] * item, st);
        GRHIP_HIP(hipStreamSynchronize(st));
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
        if (int rc = squelch_check_ramp(r)) return rc;
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        std::vector<SquelchState> v;
        if ((rc = read_states(d_state, v))) return rc;
        int max_ramped = 0;
        for (const SquelchState &s : v) {
            if (r == 0 && (s.state == SQ_ATTACK || s.state == SQ_DECAY))
                return fail(GRHIP_ERANGE, "set_ramp(0) while a stream is inside a ramp");
            if (s.ramped > max_ramped) max_ramped = s.ramped;
        }
        ramp = r;
        return build_table(max_ramped);
    }

    int get_state(int s, SquelchState *out) { return read_state(d_state, s, out); }
};

}  // namespace grhip
