// capi_runsum.hip -- C ABI of the sliding / running sum blocks: gr_dc_blocker_ff / _cc, gr_moving_average_XX,
// gr_integrate_XX.
//
// Reference: filter/gr_dc_blocker_ff.cc:31-53 (moving_averager_f), 63-80 (constructor), 96-103 (get_group_delay),
// 105-138 (work); filter/gr_dc_blocker_cc.cc likewise; gengen/gr_moving_average_XX.cc.t:38-50 (constructor), 56-62
// (set_length_and_scale), 64-93 (work); gengen/gr_integrate_XX.cc.t:38-46, 52-67.
//
// dc_blocker keeps two states, one per mode: GENERIC the reference's own (every stage's delay line and running sum),
// FAST only the last 2 (D - 1) or 4 (D - 1) inputs.  set_mode and set_streams clear both: the filter restarts from
// the reference's initial state (all zeros).
#include "grhip_internal.h"
#include "running_sum.h"
#include "stream_block.h"

using namespace grhip;

namespace {

bool aligned_items(const void *a, const void *b, int type)
{
    const size_t item = rsum_item(type);            // the kernels load whole items: gr_complex as one float2
    return aligned(a, item) && aligned(b, item);
}

}  // namespace

struct grhip_dc_blocker : StreamBlock {
    int type = RSUM_F, D = 32, stages = 4;
    DevBuf d_state, d_hist[2];
    int cur = 0;                                    // d_hist[cur]: the last inputs before the next call

    int halo() const { return stages * (D - 1); }

    int clear()
    {
        const size_t item = rsum_item(type);
        const size_t sb = (size_t)nstreams * dc_state_elems(D, stages) * item, hb = (size_t)nstreams * halo() * item + 16;
        int rc;
        if ((rc = d_state.reserve(sb)) || (rc = d_hist[0].reserve(hb)) || (rc = d_hist[1].reserve(hb))) return rc;
        if ((rc = zero_device(d_state.p, sb)) || (rc = zero_device(d_hist[0].p, hb)) || (rc = zero_device(d_hist[1].p, hb))) return rc;
        cur = 0;
        return GRHIP_OK;
    }

    int work_device(int noutput_items, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(noutput_items);
        if (c <= 0) return c;
        int rc = check_io(d_in, rsum_item(type), d_out, rsum_item(type));
        if (rc) return rc;
        if ((rc = bind())) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        DcLaunch a;
        a.in = d_in; a.out = d_out; a.n = noutput_items;
        a.nstreams = nstreams; a.D = D; a.stages = stages;
        a.state = d_state.p;
        a.hist_old = d_hist[cur].p; a.hist_new = d_hist[cur ^ 1].p;
        if ((rc = dc_blocker_launch(type, mode_fast(mode), a, pick(stream)))) return rc;
        if (mode_fast(mode) && halo() > 0) cur ^= 1;
        return noutput_items;
    }

    int work(int noutput_items, const void *in, void *out)
    {
        const size_t item = rsum_item(type);
        const int rc = host_work(noutput_items, item, in, (size_t)noutput_items, item, out, 0, [&](void *d_in, void *d_out, hipStream_t s) {
            const int r = work_device(noutput_items, d_in, d_out, s);
            return r < 0 ? r : GRHIP_OK;
        });
        return rc ? rc : noutput_items;
    }

    // not ModeBlock's: each mode keeps a state of its own, so a change of mode restarts the filter
    int set_mode(int m)
    {
        if (!mode_valid(m)) return fail(GRHIP_EINVAL, "bad mode %d", m);
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        mode = m;
        return clear();
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return clear(); });
    }
};
struct grhip_dc_blocker_ff : grhip_dc_blocker {};
struct grhip_dc_blocker_cc : grhip_dc_blocker {};

struct grhip_moving_average : ModeBlock {
    int type = RSUM_F, length = 1, max_iter = 4096, new_length = 1;
    float2 scale = {0.f, 0.f}, new_scale = {0.f, 0.f};
    int iscale = 0, new_iscale = 0;
    bool updated = false;

    static int check_length(int length)
    {
        if (length < 1) return fail(GRHIP_EINVAL, "moving_average: length must be at least 1");
        if (length > RSUM_MA_MAX_LEN) return fail(GRHIP_EINVAL, "moving_average: length at most %d (the window kernel's LDS layout)", RSUM_MA_MAX_LEN);
        return GRHIP_OK;
    }

    int latch(int len, float2 sc, int isc)
    {
        if (int rc = check_length(len)) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        new_length = len; new_scale = sc; new_iscale = isc;
        updated = true;
        return GRHIP_OK;
    }

    // Under the lock: apply a latched update and say so (.cc.t:69-75: the call then returns 0, the history may have
    // changed), or copy out what this call computes with.
    bool take_update(MaLaunch &a, bool &fast)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        if (updated) {
            length = new_length; scale = new_scale; iscale = new_iscale;
            updated = false;
            return true;
        }
        a.length = length; a.max_iter = max_iter; a.scale = scale; a.iscale = iscale;
        fast = mode_fast(mode);
        return false;
    }

    int run(MaLaunch &a, bool fast, int n, const void *d_in, void *d_out, hipStream_t st)
    {
        if (n == 0) return 0;
        if (!d_in || !d_out) return fail(GRHIP_EINVAL, "null buffer");
        if (!aligned_items(d_in, d_out, type)) return fail(GRHIP_EINVAL, "moving_average: items not naturally aligned");
        a.in = d_in; a.out = d_out; a.n = n;
        if (int rc = moving_average_launch(type, fast, a, st)) return rc;
        return n;
    }

    // one launch = the reference's successive work calls of max_iter outputs (the last one shorter)
    int work_device(int noutput_items, const void *d_in, void *d_out, void *stream)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        int rc = bind();
        if (rc) return rc;
        MaLaunch a;
        bool fast;
        if (take_update(a, fast)) return 0;
        return run(a, fast, noutput_items, d_in, d_out, pick(stream));
    }

    // one reference work call: min(noutput_items, max_iter) outputs
    int work(int noutput_items, const void *in, void *out)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        int rc = bind();
        if (rc) return rc;
        MaLaunch a;
        bool fast;
        if (take_update(a, fast)) return 0;
        if (noutput_items == 0) return 0;
        if (!in || !out) return fail(GRHIP_EINVAL, "null buffer");
        const int num = noutput_items > a.max_iter ? a.max_iter : noutput_items;
        const size_t item = rsum_item(type), bytes = ((size_t)num + a.length - 1) * item;
        return (int)host_call(in, bytes, bytes + 16, (size_t)num * item + 16, out, item,
                              [&](void *d_in, void *d_out, hipStream_t s) -> long long {
                                  return run(a, fast, num, d_in, d_out, s);
                              });
    }
};
struct grhip_moving_average_ff : grhip_moving_average {};
struct grhip_moving_average_cc : grhip_moving_average {};
struct grhip_moving_average_ss : grhip_moving_average {};
struct grhip_moving_average_ii : grhip_moving_average {};

struct grhip_integrate : ModeBlock {
    int type = RSUM_F, decim = 1;

    int work_device(int noutput_items, const void *d_in, void *d_out, void *stream)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        if (noutput_items == 0) return 0;
        if (!d_in || !d_out) return fail(GRHIP_EINVAL, "null buffer");
        if (!aligned_items(d_in, d_out, type)) return fail(GRHIP_EINVAL, "integrate: items not naturally aligned");
        int rc = bind();
        if (rc) return rc;
        bool fast;
        {
            std::lock_guard<std::mutex> lk(setter_mutex);
            fast = mode_fast(mode);
        }
        if ((rc = integrate_launch(type, fast, d_in, d_out, noutput_items, decim, pick(stream)))) return rc;
        return noutput_items;
    }

    int work(int noutput_items, const void *in, void *out)
    {
        if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        if (noutput_items == 0) return 0;
        if (!in || !out) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        const size_t item = rsum_item(type), bytes = (size_t)noutput_items * (size_t)decim * item;
        return (int)host_call(in, bytes, bytes + 16, (size_t)noutput_items * item + 16, out, item,
                              [&](void *d_in, void *d_out, hipStream_t s) -> long long {
                                  return work_device(noutput_items, d_in, d_out, s);
                              });
    }
};
struct grhip_integrate_ff : grhip_integrate {};
struct grhip_integrate_cc : grhip_integrate {};
struct grhip_integrate_ss : grhip_integrate {};
struct grhip_integrate_ii : grhip_integrate {};

namespace {

template <class H>
int create_dc(H **h, int type, int D, int long_form, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (D < 1) return fail(GRHIP_EINVAL, "dc_blocker: D must be at least 1 (the reference's deque(D - 1) throws)");
    if (D > RSUM_DC_MAX_D) return fail(GRHIP_EINVAL, "dc_blocker: D at most %d (the window kernel's LDS layout)", RSUM_DC_MAX_D);
    return make_handle(h, [&](H *b) {
        int rc = b->init_device(device);
        if (rc) return rc;
        b->type = type; b->D = D; b->stages = long_form ? 4 : 2;
        b->mode = default_mode();
        return b->clear();
    });
}

template <class H>
int create_ma(H **h, int type, int length, float2 scale, int iscale, int max_iter, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (int rc = grhip_moving_average::check_length(length)) return rc;
    if (max_iter < 1) return fail(GRHIP_EINVAL, "moving_average: max_iter must be at least 1");
    return make_handle(h, [&](H *b) {
        b->type = type; b->length = b->new_length = length; b->max_iter = max_iter;
        b->scale = b->new_scale = scale; b->iscale = b->new_iscale = iscale;
        b->mode = default_mode();
        return b->init_device(device);
    });
}

template <class H>
int create_integrate(H **h, int type, int decim, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (decim < 1) return fail(GRHIP_EINVAL, "integrate: decim must be at least 1");
    return make_handle(h, [&](H *b) {
        b->type = type; b->decim = decim;
        b->mode = default_mode();
        return b->init_device(device);
    });
}

template <class H>
int set_plain_mode(H *h, int mode)
{
    return h ? h->set_mode(mode) : fail(GRHIP_EINVAL, "null handle");
}

}  // namespace

extern "C" {

#define GRHIP_RUNSUM_COMMON(NAME)                                                                                      \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_work(grhip_##NAME *h, int noutput_items, const void *in, void *out)                             \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->work(noutput_items, in, out);                                                                        \
    }                                                                                                                  \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int noutput_items, const void *d_in, void *d_out, void *stream)    \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->work_device(noutput_items, d_in, d_out, stream);                                                     \
    }

// ---- gr_dc_blocker_ff / _cc  (gr_dc_blocker_ff.cc:57-103) ------------------------------------------------------------
#define GRHIP_DC_BLOCKER(SFX, TYPE)                                                                                    \
    int grhip_dc_blocker_##SFX##_create(grhip_dc_blocker_##SFX **h, int D, int long_form, int device)                  \
    {                                                                                                                  \
        return create_dc(h, TYPE, D, long_form, device);                                                               \
    }                                                                                                                  \
    GRHIP_RUNSUM_COMMON(dc_blocker_##SFX)                                                                              \
    int grhip_dc_blocker_##SFX##_set_mode(grhip_dc_blocker_##SFX *h, int mode)                                         \
    {                                                                                                                  \
        return h ? h->set_mode(mode) : fail(GRHIP_EINVAL, "null handle");                                              \
    }                                                                                                                  \
    int grhip_dc_blocker_##SFX##_set_streams(grhip_dc_blocker_##SFX *h, int nstreams)                                  \
    {                                                                                                                  \
        return h ? h->set_streams(nstreams) : fail(GRHIP_EINVAL, "null handle");                                       \
    }                                                                                                                  \
    int grhip_dc_blocker_##SFX##_group_delay(const grhip_dc_blocker_##SFX *h)                                          \
    {                                                                                                                  \
        if (!h) return fail(GRHIP_EINVAL, "null handle");                                                              \
        return h->stages == 4 ? 2 * h->D - 2 : h->D - 1;                                                               \
    }

GRHIP_DC_BLOCKER(ff, RSUM_F)
GRHIP_DC_BLOCKER(cc, RSUM_C)
#undef GRHIP_DC_BLOCKER

// ---- gr_moving_average_XX  (gr_moving_average_XX.cc.t:32-62) ----------------------------------------------------------
#define GRHIP_MOVING_AVERAGE(SFX)                                                                                      \
    GRHIP_RUNSUM_COMMON(moving_average_##SFX)                                                                          \
    int grhip_moving_average_##SFX##_set_mode(grhip_moving_average_##SFX *h, int mode) { return set_plain_mode(h, mode); } \
    int grhip_moving_average_##SFX##_history(const grhip_moving_average_##SFX *h)                                      \
    {                                                                                                                  \
        return h ? h->length : fail(GRHIP_EINVAL, "null handle");                                                      \
    }                                                                                                                  \
    int grhip_moving_average_##SFX##_max_iter(const grhip_moving_average_##SFX *h)                                     \
    {                                                                                                                  \
        return h ? h->max_iter : fail(GRHIP_EINVAL, "null handle");                                                    \
    }

GRHIP_MOVING_AVERAGE(ff)
GRHIP_MOVING_AVERAGE(cc)
GRHIP_MOVING_AVERAGE(ss)
GRHIP_MOVING_AVERAGE(ii)
#undef GRHIP_MOVING_AVERAGE

int grhip_moving_average_ff_create(grhip_moving_average_ff **h, int length, float scale, int max_iter, int device)
{
    return create_ma(h, RSUM_F, length, make_float2(scale, 0.f), 0, max_iter, device);
}
int grhip_moving_average_cc_create(grhip_moving_average_cc **h, int length, float scale_re, float scale_im, int max_iter, int device)
{
    return create_ma(h, RSUM_C, length, make_float2(scale_re, scale_im), 0, max_iter, device);
}
int grhip_moving_average_ss_create(grhip_moving_average_ss **h, int length, short scale, int max_iter, int device)
{
    return create_ma(h, RSUM_S, length, make_float2(0.f, 0.f), (int)scale, max_iter, device);
}
int grhip_moving_average_ii_create(grhip_moving_average_ii **h, int length, int scale, int max_iter, int device)
{
    return create_ma(h, RSUM_I, length, make_float2(0.f, 0.f), scale, max_iter, device);
}
int grhip_moving_average_ff_set_length_and_scale(grhip_moving_average_ff *h, int length, float scale)
{
    return h ? h->latch(length, make_float2(scale, 0.f), 0) : fail(GRHIP_EINVAL, "null handle");
}
int grhip_moving_average_cc_set_length_and_scale(grhip_moving_average_cc *h, int length, float scale_re, float scale_im)
{
    return h ? h->latch(length, make_float2(scale_re, scale_im), 0) : fail(GRHIP_EINVAL, "null handle");
}
int grhip_moving_average_ss_set_length_and_scale(grhip_moving_average_ss *h, int length, short scale)
{
    return h ? h->latch(length, make_float2(0.f, 0.f), (int)scale) : fail(GRHIP_EINVAL, "null handle");
}
int grhip_moving_average_ii_set_length_and_scale(grhip_moving_average_ii *h, int length, int scale)
{
    return h ? h->latch(length, make_float2(0.f, 0.f), scale) : fail(GRHIP_EINVAL, "null handle");
}

// ---- gr_integrate_XX  (gr_integrate_XX.cc.t:32-46) ---------------------------------------------------------------------
#define GRHIP_INTEGRATE(SFX, TYPE)                                                                                     \
    int grhip_integrate_##SFX##_create(grhip_integrate_##SFX **h, int decim, int device)                               \
    {                                                                                                                  \
        return create_integrate(h, TYPE, decim, device);                                                               \
    }                                                                                                                  \
    GRHIP_RUNSUM_COMMON(integrate_##SFX)                                                                               \
    int grhip_integrate_##SFX##_set_mode(grhip_integrate_##SFX *h, int mode) { return set_plain_mode(h, mode); }       \
    int grhip_integrate_##SFX##_decimation(const grhip_integrate_##SFX *h)                                             \
    {                                                                                                                  \
        return h ? h->decim : fail(GRHIP_EINVAL, "null handle");                                                       \
    }

GRHIP_INTEGRATE(ff, RSUM_F)
GRHIP_INTEGRATE(cc, RSUM_C)
GRHIP_INTEGRATE(ss, RSUM_S)
GRHIP_INTEGRATE(ii, RSUM_I)
#undef GRHIP_INTEGRATE
#undef GRHIP_RUNSUM_COMMON

}  // extern "C"
