// stream_block.h -- what the handles with a mode, and those that take S streams back to back ([S][n]) with a little
// state per stream on the device, have in common: the mode and stream-count setters, the per-stream state on a DevBuf,
// the argument checks of work_device and the host-buffer work around it.  Not part of the ABI.
#pragma once
#include <vector>

#include "grhip_internal.h"

namespace grhip {

inline int check_streams(int S)
{
    return (S < 1 || S > 65535) ? fail(GRHIP_EINVAL, "1 .. 65535 streams") : GRHIP_OK;
}

// `a` a power of two; a null pointer is aligned
inline bool aligned(const void *p, size_t a) { return !((uintptr_t)p & (a - 1)); }

// do the na bytes at a and the nb bytes at b share a byte?  A null buffer overlaps nothing.
inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    return a && b && (const char *)a < (const char *)b + nb && (const char *)b < (const char *)a + na;
}

// ---- the first rungs of every work / work_device, to be composed as the entry needs them ---------------------------
// an item count: a negative one is refused (the error code), 0 leaves nothing to do, 1 says go on
inline int check_count(int n) { return n < 0 ? fail(GRHIP_EINVAL, "negative item count") : n > 0; }

// an input and an output buffer: neither null, each aligned to its item (item size 1: any address)
inline int check_io(const void *in, size_t in_item, const void *out, size_t out_item)
{
    if (!in || !out) return fail(GRHIP_EINVAL, "null buffer");
    if (!aligned(in, in_item) || !aligned(out, out_item)) return fail(GRHIP_EINVAL, "items not naturally aligned");
    return GRHIP_OK;
}

// for the blocks that cannot run in place: the out_bytes at `out` away from the in_bytes at `in`
inline int check_apart(const char *block, const void *in, size_t in_bytes, const void *out, size_t out_bytes)
{
    return overlap(in, in_bytes, out, out_bytes) ? fail(GRHIP_EINVAL, "%s: the output may not overlap the input", block) : GRHIP_OK;
}

// ---- a handle with a mode ------------------------------------------------------------------------------------------
struct ModeBlock : HandleBase {
    int mode = GRHIP_MODE_FAST;

    int set_mode(int m)
    {
        if (!mode_valid(m)) return fail(GRHIP_EINVAL, "bad mode %d", m);
        std::lock_guard<std::mutex> lk(setter_mutex);
        mode = m;
        return GRHIP_OK;
    }
};

// ---- a handle of S streams back to back ----------------------------------------------------------------------------
struct StreamBlock : ModeBlock {
    int nstreams = 1;

    // `restart` rebuilds what the handle keeps per stream, from the constructor's values; it runs under setter_mutex
    // with the handle's stream drained
    template <class Restart>
    int set_streams(int S, Restart &&restart)
    {
        if (int rc = check_streams(S)) return rc;
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        nstreams = S;
        return restart();
    }

    // Per-stream state: one T per stream in `d`.  fill_state and read_states are for callers that hold setter_mutex
    // and have drained the streams (or whose handle is not handed out yet); read_state and edit_states bind, take
    // setter_mutex and drain themselves.
    template <class T>
    int fill_state(DevBuf &d, const T &v)                           // every stream's T = v; streams drained, under setter_mutex
    {
        int rc = d.reserve((size_t)nstreams * sizeof(T));
        if (rc) return rc;
        std::vector<T> t((size_t)nstreams, v);
        GRHIP_HIP(hipMemcpy(d.p, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice));
        return GRHIP_OK;
    }

    template <class T>
    int read_states(const DevBuf &d, std::vector<T> &v)             // every stream's T; streams drained, under setter_mutex
    {
        v.resize((size_t)nstreams);
        GRHIP_HIP(hipMemcpy(v.data(), d.p, v.size() * sizeof(T), hipMemcpyDeviceToHost));
        return GRHIP_OK;
    }

    template <class T>
    int read_state(const DevBuf &d, int s, T *out)                  // stream s's T; takes setter_mutex and drains
    {
        if (s < 0 || s >= nstreams) return fail(GRHIP_EINVAL, "stream %d of %d", s, nstreams);
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        GRHIP_HIP(hipMemcpy(out, d.as<T>() + s, sizeof(T), hipMemcpyDeviceToHost));
        return GRHIP_OK;
    }

    template <class T, class Edit>
    int edit_states(DevBuf &d, Edit &&edit)                         // edit(T &) on every stream's T; takes setter_mutex and drains
    {
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        std::vector<T> t;
        if ((rc = read_states(d, t))) return rc;
        for (T &e : t) edit(e);
        GRHIP_HIP(hipMemcpy(d.p, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice));
        return GRHIP_OK;
    }

    // The host-buffer work of a block that turns [S][n_in items of in_item bytes] into [S][n_out items of out_item
    // bytes]: work_device(d_in, d_out, stream) runs on staged copies and returns its status.  out_more further bytes
    // are reserved behind the staged output, for a caller that has work_device put more there and fetches it itself.
    template <class WorkDevice>
    int host_work(int n_in, size_t in_item, const void *in, size_t n_out, size_t out_item, void *out, size_t out_more,
                  WorkDevice &&work_device)
    {
        const int c = check_count(n_in);
        if (c <= 0) return c;
        if (!in || !out) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        const size_t in_bytes = (size_t)nstreams * (size_t)n_in * in_item, out_items = (size_t)nstreams * n_out;
        const long long r = host_call(in, in_bytes, in_bytes + 16, out_items * out_item + out_more + 16, out, out_item,
                                      [&](void *d_in, void *d_out, hipStream_t st) {
                                          const int e = work_device(d_in, d_out, st);
                                          return e ? (long long)e : (long long)out_items;
                                      });
        return r < 0 ? (int)r : GRHIP_OK;
    }
};

}  // namespace grhip
