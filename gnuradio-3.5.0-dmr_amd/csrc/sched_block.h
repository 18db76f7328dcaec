// sched_block.h -- what the handles of the schedule-driven blocks (csrc/capi_arbresamp.hip, csrc/capi_fracinterp.hip)
// have in common: the device copy of a walked schedule, the mode, the host-buffer general_work, the argument checks of
// run_captures_device and the C entry points that only forward.  Not part of the ABI.
#pragma once
#include <vector>

#include "grhip_internal.h"
#include "stream_block.h"

namespace grhip {

// The steps of a walked schedule on the device, with the host copy they were uploaded from.
template <class Step>
struct WalkedSteps {
    DevBuf d_steps;
    std::vector<Step> h_steps;      // source of the last upload to d_steps, kept until ev has passed
    hipEvent_t ev = nullptr;        // recorded after the last launch that read d_steps
    bool busy = false;

    // takes `steps` (swapped out of the plan) and queues their copy on `stream`; *dev is what the kernel reads
    int upload(std::vector<Step> &steps, hipStream_t stream, const Step **dev)
    {
        // d_steps and its host source are rewritten, so the handle's last launch that read them (on whatever stream)
        // must be done -- that launch only, nothing else on the device
        if (!ev) GRHIP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (busy) { GRHIP_HIP(hipEventSynchronize(ev)); busy = false; }
        h_steps.swap(steps);
        const size_t bytes = h_steps.size() * sizeof(Step);
        int rc = d_steps.reserve(bytes);
        if (rc) return rc;
        GRHIP_HIP(hipMemcpyAsync(d_steps.p, h_steps.data(), bytes, hipMemcpyHostToDevice, stream));
        *dev = d_steps.as<Step>();
        return GRHIP_OK;
    }

    // after the copy of upload(), whether or not the kernel was launched
    int mark_read(hipStream_t stream)
    {
        GRHIP_HIP(hipEventRecord(ev, stream));
        busy = true;
        return GRHIP_OK;
    }

    WalkedSteps() = default;
    WalkedSteps(const WalkedSteps &) = delete;
    WalkedSteps &operator=(const WalkedSteps &) = delete;
    ~WalkedSteps()                  // the event first, then (as a member) d_steps
    {
        if (!ev) return;
        if (busy) (void)hipEventSynchronize(ev);
        (void)hipEventDestroy(ev);
    }
};

// Base of a schedule-driven handle D, which supplies general_work_device(noutput_items, ninput_items, d_in, d_out,
// consumed, stream).
template <class D>
struct SchedBlock : ModeBlock {
    bool cplx = true;

    size_t item() const { return cplx ? 8 : 4; }

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
                                  return static_cast<D *>(this)->general_work_device(noutput_items, ninput_items, d_in,
                                                                                     d_out, consumed, s);
                              });
    }

    // n_streams captures of n_samples items from a fresh state: plan_fresh() is the plan of one capture and
    // launch(plan) enqueues it for all of them, both under the setters' lock.  d_out == NULL only reports *n_out.
    template <class PlanFresh, class Launch>
    int run_captures(const char *name, size_t max_samples, int n_streams, size_t n_samples, const void *d_in,
                     size_t in_stride, void *d_out, size_t out_stride, size_t *n_out, PlanFresh plan_fresh, Launch launch)
    {
        if (!n_out) return fail(GRHIP_EINVAL, "null n_out");
        if (n_streams < 0) return fail(GRHIP_EINVAL, "negative n_streams");
        if (n_samples > max_samples) return fail(GRHIP_EINVAL, "n_samples too large");
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);               // plan and launch under one lock
        auto p = plan_fresh();
        if (p.too_many) return fail(GRHIP_EINVAL, "%s: too many outputs per capture", name);
        *n_out = (size_t)p.n;
        if (!d_out || n_streams == 0 || p.n == 0) return GRHIP_OK;   // a query, or nothing to do
        if (!d_in) return fail(GRHIP_EINVAL, "null buffer");
        if (n_streams > 1 && (in_stride < n_samples || out_stride < (size_t)p.n))
            return fail(GRHIP_EINVAL, "%s: strides shorter than n_samples / n_out", name);
        return launch(p);
    }
};

}  // namespace grhip

// The C entry points of grhip_<NAME> that only forward to the handle (inside extern "C").
#define GRHIP_SCHED_ENTRIES(NAME)                                                                                      \
    void grhip_##NAME##_destroy(grhip_##NAME *h)                                                                       \
    {                                                                                                                  \
        destroy_handle(h);                                                                                             \
    }                                                                                                                  \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode)                                                             \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->set_mode(mode);                                                                                      \
    }                                                                                                                  \
    int grhip_##NAME##_general_work(grhip_##NAME *h, int noutput_items, int ninput_items, const void *in, void *out,   \
                                    int *consumed)                                                                     \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->general_work(noutput_items, ninput_items, in, out, consumed);                                        \
    }                                                                                                                  \
    int grhip_##NAME##_general_work_device(grhip_##NAME *h, int noutput_items, int ninput_items, const void *d_in,     \
                                           void *d_out, int *consumed, void *stream)                                   \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->general_work_device(noutput_items, ninput_items, d_in, d_out, consumed, stream);                     \
    }                                                                                                                  \
    int grhip_##NAME##_run_captures_device(grhip_##NAME *h, int n_streams, size_t n_samples, const void *d_in,         \
                                           size_t in_stride, void *d_out, size_t out_stride, size_t *n_out,            \
                                           void *stream)                                                               \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->run_captures_device(n_streams, n_samples, d_in, in_stride, d_out, out_stride, n_out, stream);        \
    }
