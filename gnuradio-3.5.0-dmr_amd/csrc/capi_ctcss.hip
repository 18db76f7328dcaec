// capi_ctcss.hip -- C ABI of gr_ctcss_squelch_ff.
//
// Reference: general/gr_ctcss_squelch_ff.{h,cc} (tones, guards, the decision), filter/gri_goertzel.{h,cc} (the filters),
// general/gr_squelch_base_ff.{h,cc} (the machine, general_work).
//
// A handle takes S streams back to back ([S][n_in]) like the power squelch and shares its machine (squelch_block.h).
// What a stream remembers besides the machine is the raw samples of its unfinished block and its last decision, on the
// device; how many samples that block holds is the same for every stream and is kept by the host.  set_streams restarts
// every stream; the other setters keep everything and hold from the next work call.
#include <cmath>
#include <vector>

#include "analytic.h"
#include "ctcss.h"
#include "grhip_internal.h"
#include "squelch_block.h"

using namespace grhip;

namespace {

// gr_ctcss_squelch_ff.cc:29-36
const float ctcss_tones[] = {67.0,  71.9,  74.4,  77.0,  79.7,  82.5,  85.4,  88.5,  91.5,  94.8,  97.4,  100.0, 103.5,
                             107.2, 110.9, 114.8, 118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 162.2,
                             167.9, 173.8, 179.9, 186.2, 192.8, 203.5, 210.7, 218.1, 225.7, 233.6, 241.8, 250.3};
const int max_tone_index = 37;

// gr_ctcss_squelch_ff.cc:44-51: an exact compare
int find_tone(float freq)
{
    for (int i = 0; i <= max_tone_index; i++)
        if (ctcss_tones[i] == freq) return i;
    return -1;
}

}  // namespace

struct grhip_ctcss_squelch_ff : SquelchMachine {
    int rate = 1, len = 1;
    float freq = 0.f, level = 0.01f;
    float f_l = 0.f, f_r = 0.f;
    float wr[3] = {0.f, 0.f, 0.f}, wi[3] = {0.f, 0.f, 0.f};
    int pending = 0;                    // samples of the unfinished block, every stream
    size_t mags_off = 0;                // where the last call's magnitudes lie in d_scratch
    long long mags_blocks = 0;          // ... and how many blocks per stream it completed
    DevBuf d_carry, d_mute, d_tab;
    bool tab_valid = false;

    // gr_ctcss_squelch_ff.cc:65-82: the guards are the adjacent standard tones; a non-standard tone, and the first and
    // the last on their outer side, get 2 % (the product in double, stored to float)
    void set_tones()
    {
        const int i = find_tone(freq);
        f_l = (i == -1 || i == 0) ? (float)(freq * 0.98) : ctcss_tones[i - 1];
        f_r = (i == -1 || i == max_tone_index) ? (float)(freq * 1.02) : ctcss_tones[i + 1];
        goertzel_setparms(rate, f_l, &wr[0], &wi[0]);
        goertzel_setparms(rate, freq, &wr[1], &wi[1]);
        goertzel_setparms(rate, f_r, &wr[2], &wi[2]);
    }

    int build_tab(hipStream_t st)
    {
        std::vector<float2> tab((size_t)3 * len);
        for (int f = 0; f < 3; ++f) goertzel_build_table(len, wr[f], wi[f], tab.data() + (size_t)f * len);
        int rc = drain(st);
        if (rc) return rc;
        if ((rc = d_tab.reserve(tab.size() * sizeof(float2)))) return rc;
        GRHIP_HIP(hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice));
        tab_valid = true;
        return GRHIP_OK;
    }

    // the machine's initial state, d_mute true (gr_ctcss_squelch_ff.cc:84), the filters empty
    int restart()
    {
        int rc = restart_machine();
        if (rc) return rc;
        if ((rc = d_carry.reserve((size_t)nstreams * len * sizeof(float)))) return rc;
        if ((rc = d_mute.reserve((size_t)nstreams))) return rc;
        std::vector<unsigned char> m((size_t)nstreams, 1);
        GRHIP_HIP(hipMemcpy(d_mute.p, m.data(), m.size(), hipMemcpyHostToDevice));
        pending = 0;
        mags_blocks = 0;
        return GRHIP_OK;
    }

    int work_device(int n_in, const void *d_in, void *d_out, int *d_produced, void *stream)
    {
        const int c0 = check_count(n_in);
        if (c0 <= 0) return c0;
        int rc = check_work(n_in, d_in, d_out, d_produced, sizeof(float));
        if (rc) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const bool fast = mode_fast(mode);
        if (fast && !tab_valid && (rc = build_tab(st))) return rc;
        SquelchLaunch l;
        l.in = d_in; l.out = d_out; l.produced = d_produced; l.n = n_in; l.nstreams = nstreams;
        l.cc = false; l.simple = false; l.gate = gate; l.ramp = ramp; l.alpha = 0.0; l.threshold = 0.0;
        l.state = d_state.as<SquelchState>(); l.table = d_table.as<double>();
        CtcssLaunch c;
        c.len = len; c.pending = pending; c.level = level;
        for (int f = 0; f < 3; ++f) { c.wr[f] = wr[f]; c.wi[f] = wi[f]; }
        c.tab = d_tab.as<float2>(); c.carry = d_carry.as<float>(); c.mute = d_mute.as<unsigned char>();
        if ((rc = d_scratch.reserve(ctcss_scratch_bytes(c, l)))) return rc;
        if ((rc = ctcss_launch(fast, c, l, d_scratch.p, st))) return rc;
        mags_off = ctcss_magnitudes_offset(c, l);
        mags_blocks = ctcss_blocks(c, n_in);
        pending = (int)(((long long)pending + n_in) % len);
        return GRHIP_OK;
    }

    int work(int n_in, const void *in, void *out, int *produced)
    {
        return host_work(n_in, in, out, produced, sizeof(float), [&](int n, const void *d_in, void *d_out, int *d_p, hipStream_t st) {
            return work_device(n, d_in, d_out, d_p, st);
        });
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
    }

    int set_level(float v)
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        level = v;                                          // a kernel argument: launches already queued keep theirs
        return GRHIP_OK;
    }

    int get_ctcss(int s, int *mute, int *pend)
    {
        unsigned char m = 0;                // d_mute: every stream's decision, one byte
        if (int rc = read_state(d_mute, s, &m)) return rc;
        if (mute) *mute = m;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if (pend) *pend = pending;
        return GRHIP_OK;
    }

    // |l|, |c|, |r| of the blocks of stream s that the last work call completed, in order; returns how many blocks
    int last_magnitudes(int s, float *out, int cap)
    {
        if (s < 0 || s >= nstreams) return fail(GRHIP_EINVAL, "stream %d of %d", s, nstreams);
        if (cap < 0 || (cap > 0 && !out)) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        if (mags_blocks > cap) return fail(GRHIP_EINVAL, "magnitudes: room for %lld blocks needed", mags_blocks);
        if (mags_blocks)
            GRHIP_HIP(hipMemcpy(out, (const char *)d_scratch.p + mags_off + (size_t)s * mags_blocks * 3 * sizeof(float),
                                (size_t)mags_blocks * 3 * sizeof(float), hipMemcpyDeviceToHost));
        return (int)mags_blocks;
    }
};

extern "C" {

#define GRHIP_CTCSS_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")

// gr_make_ctcss_squelch_ff / the constructor (gr_ctcss_squelch_ff.cc:38-85).  rate <= 0 would give the default len a
// value below 1 and every filter a meaningless w; len < 1 makes gri_goertzel::ready() unreachable (the block never
// decides); a non-finite freq gives NaN coefficients: all refused here.
int grhip_ctcss_squelch_ff_create(grhip_ctcss_squelch_ff **h, int rate, float freq, float level, int len, int ramp, int gate,
                                  int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (rate <= 0) return fail(GRHIP_EINVAL, "ctcss_squelch_ff: rate must be positive");
    if (!std::isfinite(freq)) return fail(GRHIP_EINVAL, "ctcss_squelch_ff: freq must be finite");
    if (len < 0) return fail(GRHIP_EINVAL, "ctcss_squelch_ff: len must not be negative");
    const int eff = len == 0 ? (int)(rate / 10.0) : len;                // gr_ctcss_squelch_ff.cc:60-63: 100 ms
    if (eff < 1 || eff > CTCSS_MAX_LEN) return fail(GRHIP_ERANGE, "ctcss_squelch_ff: len %d outside 1 .. %d", eff, CTCSS_MAX_LEN);
    if (int rc = squelch_check_ramp(ramp)) return rc;
    return make_handle(h, [&](grhip_ctcss_squelch_ff *b) {
        b->rate = rate; b->freq = freq; b->level = level; b->len = eff; b->ramp = ramp; b->gate = gate != 0;
        b->set_tones();
        b->mode = default_mode();
        int rc = b->init_device(device);
        return rc ? rc : b->restart();
    });
}

void grhip_ctcss_squelch_ff_destroy(grhip_ctcss_squelch_ff *h) { destroy_handle(h); }

int grhip_ctcss_squelch_ff_set_mode(grhip_ctcss_squelch_ff *h, int mode)
{
    GRHIP_CTCSS_NULL(h);
    return h->set_mode(mode);
}

int grhip_ctcss_squelch_ff_set_streams(grhip_ctcss_squelch_ff *h, int nstreams)
{
    GRHIP_CTCSS_NULL(h);
    return h->set_streams(nstreams);
}

// gr_ctcss_squelch_ff.h:63-65
float grhip_ctcss_squelch_ff_level(grhip_ctcss_squelch_ff *h)
{
    if (!h) return (float)fail(GRHIP_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    return h->level;
}

int grhip_ctcss_squelch_ff_set_level(grhip_ctcss_squelch_ff *h, float level)
{
    GRHIP_CTCSS_NULL(h);
    return h->set_level(level);
}

int grhip_ctcss_squelch_ff_len(grhip_ctcss_squelch_ff *h)
{
    GRHIP_CTCSS_NULL(h);
    return h->len;
}

// gr_squelch_base_ff.h:44-48
int grhip_ctcss_squelch_ff_ramp(grhip_ctcss_squelch_ff *h)
{
    GRHIP_CTCSS_NULL(h);
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    return h->ramp;
}

int grhip_ctcss_squelch_ff_set_ramp(grhip_ctcss_squelch_ff *h, int ramp)
{
    GRHIP_CTCSS_NULL(h);
    return h->set_ramp(ramp);
}

int grhip_ctcss_squelch_ff_gate(grhip_ctcss_squelch_ff *h)
{
    GRHIP_CTCSS_NULL(h);
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    return h->gate ? 1 : 0;
}

int grhip_ctcss_squelch_ff_set_gate(grhip_ctcss_squelch_ff *h, int gate)
{
    GRHIP_CTCSS_NULL(h);
    return h->set_gate(gate);
}

// gr_ctcss_squelch_ff.cc:87-95
int grhip_ctcss_squelch_ff_squelch_range(float *range)
{
    if (!range) return fail(GRHIP_EINVAL, "null argument");
    range[0] = 0.0;
    range[1] = 1.0;
    range[2] = (range[1] - range[0]) / 100;
    return GRHIP_OK;
}

// gr_squelch_base_ff.h:49
int grhip_ctcss_squelch_ff_unmuted(grhip_ctcss_squelch_ff *h, int s)
{
    GRHIP_CTCSS_NULL(h);
    SquelchState v;
    if (int rc = h->get_state(s, &v)) return rc;
    return v.state == SQ_UNMUTED || v.state == SQ_ATTACK;
}

int grhip_ctcss_squelch_ff_state(grhip_ctcss_squelch_ff *h, int s, int *state, int *ramped, double *envelope, int *mute,
                                 int *pending)
{
    GRHIP_CTCSS_NULL(h);
    SquelchState v;
    if (int rc = h->get_state(s, &v)) return rc;
    if (int rc = h->get_ctcss(s, mute, pending)) return rc;
    if (state) *state = v.state;
    if (ramped) *ramped = v.ramped;
    if (envelope) *envelope = v.envelope;
    return GRHIP_OK;
}

// gr_ctcss_squelch_ff.cc:65-82
int grhip_ctcss_squelch_ff_tones(grhip_ctcss_squelch_ff *h, float *f_l, float *f_c, float *f_r)
{
    GRHIP_CTCSS_NULL(h);
    if (f_l) *f_l = h->f_l;
    if (f_c) *f_c = h->freq;
    if (f_r) *f_r = h->f_r;
    return GRHIP_OK;
}

int grhip_ctcss_squelch_ff_last_magnitudes(grhip_ctcss_squelch_ff *h, int s, float *out, int cap_blocks)
{
    GRHIP_CTCSS_NULL(h);
    return h->last_magnitudes(s, out, cap_blocks);
}

// gr_squelch_base_ff.cc:42-93 around gr_ctcss_squelch_ff.cc:97-112
int grhip_ctcss_squelch_ff_work(grhip_ctcss_squelch_ff *h, int n_in, const void *in, void *out, int *produced)
{
    GRHIP_CTCSS_NULL(h);
    return h->work(n_in, in, out, produced);
}

int grhip_ctcss_squelch_ff_work_device(grhip_ctcss_squelch_ff *h, int n_in, const void *d_in, void *d_out, int *d_produced,
                                       void *stream)
{
    GRHIP_CTCSS_NULL(h);
    return h->work_device(n_in, d_in, d_out, d_produced, stream);
}

#undef GRHIP_CTCSS_NULL

}  // extern "C"
