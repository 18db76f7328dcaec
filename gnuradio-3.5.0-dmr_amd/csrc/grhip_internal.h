// grhip_internal.h -- shared plumbing of libgrhip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/grhip.h"
#include "fir_plan.h"

namespace grhip {

// ---- thread-local error detail -------------------------------------------
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

#define GRHIP_HIP(call)                                                                     \
    do {                                                                                    \
        hipError_t e__ = (call);                                                            \
        if (e__ != hipSuccess)                                                              \
            return ::grhip::fail(e__ == hipErrorOutOfMemory ? GRHIP_ENOMEM : GRHIP_ERUNTIME, \
                                 "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),    \
                                 __FILE__, __LINE__);                                       \
    } while (0)

// Zero device memory and return once it is zero.  hipMemset is queued on the null stream, which the handles'
// non-blocking streams do not wait for, and it may return before it has run: a kernel on a handle's stream could
// read the buffer's previous contents.
inline int zero_device(void *p, size_t bytes)
{
    GRHIP_HIP(hipMemset(p, 0, bytes));
    GRHIP_HIP(hipStreamSynchronize(nullptr));
    return GRHIP_OK;
}

// ---- device buffer that only ever grows -----------------------------------
// The owners below (DevBuf, StageBuf, SchedBuf and the structs built from them) free what they hold when they are
// destroyed and cannot be copied; release() is for a live handle that drops a buffer it is about to rebuild.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return GRHIP_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        GRHIP_HIP(hipMalloc(&p, want));
        cap = want;
        return GRHIP_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// Staging buffer of the host-buffer entry points.  Scheduler-sized calls (<= MAPPED_MAX bytes) get host memory that is
// pinned AND mapped into the device's address space: the caller's items are copied into it by the CPU, the kernels read
// and write it in place over the host link, and no copy engine is involved (a 32 KB call spent more time submitting its
// two DMA transfers than moving them: 45 -> 26 us per 1024-output call of the fused block, 61 -> 34 at 8192;
// tools/bench_small_calls.py).  Once a call needs more than MAPPED_MAX, the buffer becomes device memory for good.
struct StageBuf : DevBuf {
#ifndef GRHIP_MAPPED_MAX
#define GRHIP_MAPPED_MAX (2 * 1024 * 1024)
#endif
    static constexpr size_t MAPPED_MAX = GRHIP_MAPPED_MAX;
    void *host = nullptr;       // host address of a mapped buffer (p is its device address); null: device memory
    ~StageBuf() { release(); }  // a mapped buffer goes back to the host allocator; ~DevBuf then finds nothing
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return GRHIP_OK;
        if (bytes <= MAPPED_MAX && (cap == 0 || host)) {
            size_t want = 64 * 1024;
            while (want < bytes) want *= 2;
            release();
            GRHIP_HIP(hipHostMalloc(&host, want, hipHostMallocMapped));
            if (hipHostGetDevicePointer(&p, host, 0) != hipSuccess) { (void)hipHostFree(host); host = nullptr; p = nullptr; }
            else { cap = want; return GRHIP_OK; }
        }
        release();
        return DevBuf::reserve(bytes);
    }
    void release()
    {
        if (host) { (void)hipHostFree(host); host = nullptr; p = nullptr; cap = 0; }
        else DevBuf::release();
    }
    // host address of a device address inside a mapped buffer, or null
    void *host_of(const void *dev) const
    {
        if (!host || (const char *)dev < (const char *)p || (const char *)dev >= (const char *)p + cap) return nullptr;
        return (char *)host + ((const char *)dev - (const char *)p);
    }
};

// the two counters of the tiled kernel's tile queue: zeroed once, re-armed by every launch
struct SchedBuf {
    DevBuf b;
    unsigned *get()
    {
        if (!b.p) {
            if (b.reserve(2 * sizeof(unsigned)) != GRHIP_OK) return nullptr;
            if (zero_device(b.p, 2 * sizeof(unsigned)) != GRHIP_OK) { b.release(); return nullptr; }
        }
        return b.as<unsigned>();
    }
};

// ---- base of every block handle -------------------------------------------
#define GRHIP_H2D(h, dst, src, bytes, st) do { int rc__ = (h)->h2d((dst), (src), (bytes), (st)); if (rc__) return rc__; } while (0)
#define GRHIP_D2H(h, dst, src, bytes, st) do { int rc__ = (h)->d2h((dst), (src), (bytes), (st)); if (rc__) return rc__; } while (0)

struct HandleBase {
    int device = 0;
    hipStream_t own_stream = nullptr;
    std::mutex setter_mutex;   // setters vs. the work thread
    StageBuf stage_in, stage_out;
    // Pinned staging of the host-buffer entry points (SURVEY 8b "Ownership": the handle owns it, the caller owns its I/O
    // buffers).  Scheduler-sized transfers (<= PIN_MAX) go caller buffer -> pinned slot -> DMA and back: no page pinning or
    // runtime staging per call; two slots per direction, so a call split in chunks copies one while the other is in flight.
    // Larger transfers are left to the runtime: measured (tools/bench_small_calls.py) its own staging wins from a few hundred KB.
    static constexpr size_t PIN_SLOT = 32 * 1024, PIN_MAX = 64 * 1024;
    struct PinRing {
        void *buf[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
        bool busy[2] = {false, false};
        int next = 0;
    } pin_up, pin_down;
    int pin_init(PinRing &r);
    void pin_release(PinRing &r);
    int h2d(void *dst_dev, const void *src_host, size_t bytes, hipStream_t st);
    int d2h(void *dst_host, const void *src_dev, size_t bytes, hipStream_t st);     // complete on return (<= PIN_MAX) or queued

    int init_device(int dev);
    HandleBase() = default;
    HandleBase(const HandleBase &) = delete;
    HandleBase &operator=(const HandleBase &) = delete;
    // Pin rings, then staging, then the stream.  A derived handle's members are destroyed before this runs, so its
    // buffers are freed while the stream still exists.  Never binds a device (destroy_handle does): after a failed
    // init_device there is no stream, nothing allocated, and `device` may be out of range.
    ~HandleBase();
    hipStream_t pick(void *stream) const { return stream ? (hipStream_t)stream : own_stream; }
    int bind() const;          // hipSetDevice for the calling thread

    // Wait for the launches that may still read a handle's tap buffers (on `st`, the stream of the coming work call,
    // and on the handle's own stream) before a latched update rewrites them with blocking copies on the null stream,
    // which does not wait for the handles' non-blocking streams.
    int drain(hipStream_t st)
    {
        GRHIP_HIP(hipStreamSynchronize(st));
        if (st != own_stream) GRHIP_HIP(hipStreamSynchronize(own_stream));
        return GRHIP_OK;
    }

    // The body of a host-buffer entry point: reserve the staging buffers, stage in_bytes of `in`, run
    // work(d_in, d_out, stream) on the handle's own stream, copy the n * out_item bytes of the n items it reports back to
    // `out` and return n (or work's negative error code).  The call ends with a synchronisation, which every host-buffer
    // entry needs: h2d writes straight into mapped staging memory, so nothing of this call may still be in flight when
    // the next call's h2d runs.
    template <class Work>
    long long host_call(const void *in, size_t in_bytes, size_t in_reserve, size_t out_reserve, void *out,
                        size_t out_item, Work &&work)
    {
        int rc;
        if ((rc = stage_in.reserve(in_reserve))) return rc;
        if ((rc = stage_out.reserve(out_reserve))) return rc;
        hipStream_t st = own_stream;
        GRHIP_H2D(this, stage_in.p, in, in_bytes, st);
        const long long n = work(stage_in.p, stage_out.p, st);
        if (n < 0) return n;
        GRHIP_D2H(this, out, stage_out.p, (size_t)n * out_item, st);
        GRHIP_HIP(hipStreamSynchronize(st));
        return n;
    }
};

// The body of every destroy entry point: bind the handle's device (only a handle that init_device gave a stream has
// one) and delete it; the members' destructors free what it owns.
template <class H>
void destroy_handle(H *h)
{
    if (!h) return;
    if (h->own_stream) (void)hipSetDevice(h->device);
    delete h;
}

// The tail of a create entry point: allocate a handle H, run init(handle) and hand it out in *h.  When init fails
// the handle is destroyed again and *h stays null.
template <class H, class Init>
int make_handle(H **h, Init &&init)
{
    *h = nullptr;
    auto *b = new (std::nothrow) H();
    if (!b) return fail(GRHIP_ENOMEM, "alloc");
    int rc = init(b);
    if (rc) {
        destroy_handle(b);
        return rc;
    }
    *h = b;
    return GRHIP_OK;
}

int default_mode();
// (mode_valid / mode_fast / mode_matrix: fir_plan.h)

// shared read-only device tables (per device, created on first use)
struct DeviceTables {
    float *atan_tab = nullptr;       // 257 floats   (gr_fast_atan2f table)
    float *mmse_rev = nullptr;       // [8][129] floats, tap-major, reversed taps
};
int get_device_tables(int device, const DeviceTables **out);

// launch limits of the calling thread's current device (cached per device; launchers run with the handle's device bound)
int allow_lds(const void *kernel, size_t bytes);   // let `kernel` launch with `bytes` of dynamic LDS here
int device_cus();                                  // the device's CU count (256 when the runtime cannot say)

}  // namespace grhip
