// capi_constellation.hip -- C ABI of the constellation objects (digital_constellation.h), digital_constellation_decoder_cb,
// digital_constellation_receiver_cb, gr_diff_decoder_bb, gr_map_bb and constellation_demod_cb, the tail of
// gr-digital/python/generic_mod_demod.py:296-313 behind timing recovery as one handle.
//
// A grhip_constellation lives on the host (csrc/constellation.h) and needs no device.  A block copies the
// constellation it is created from, so the constellation handle may be destroyed first.  The blocks take S streams back
// to back as the carrier loops do; what a stream remembers (phase, frequency, the previous symbol) is on the device.
#include <cmath>
#include <vector>

#include "constellation_blocks.h"
#include "control_loop.h"
#include "digital_kernels.h"
#include "grhip_internal.h"
#include "stream_block.h"

using namespace grhip;

namespace {

// a constellation's tables on the device: points | angles | sector values
struct ConstOnDevice {
    DevBuf buf;
    ConstDev dev{};

    int upload(const Constellation &c)
    {
        const bool angle_kind = c.kind != CONST_RECT && c.kind != CONST_CALCDIST;
        const size_t n_ang = !angle_kind ? 0 : (c.kind == CONST_PSK ? c.n_sectors : c.arity);
        const size_t pts_b = c.points.size() * sizeof(cfloat), ang_b = n_ang * sizeof(float), val_b = c.sector_values.size();
        std::vector<unsigned char> img(pts_b + ang_b + val_b + 4);
        memcpy(img.data(), c.points.data(), pts_b);
        float *ang = (float *)(img.data() + pts_b);
        for (size_t i = 0; i < n_ang; ++i) {        // the angle of the point that index i decides for, from double
            const cfloat p = c.points[c.kind == CONST_PSK ? c.sector_values[i] : i];
            ang[i] = (float)atan2((double)p.im, (double)p.re);
        }
        for (size_t i = 0; i < val_b; ++i) img[pts_b + ang_b + i] = (unsigned char)c.sector_values[i];
        int rc = buf.reserve(img.size());
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(buf.p, img.data(), img.size(), hipMemcpyHostToDevice));
        dev.kind = c.kind; dev.arity = c.arity; dev.dim = c.dim; dev.n_sectors = (unsigned)val_b;
        dev.n_real = c.n_real; dev.n_imag = c.n_imag; dev.n_ang = (unsigned)n_ang; dev.w_real = c.w_real; dev.w_imag = c.w_imag;
        dev.points = (const cfloat *)buf.p;
        dev.ang = n_ang ? (const float *)((const char *)buf.p + pts_b) : nullptr;
        dev.sval = val_b ? (const unsigned char *)buf.p + pts_b + ang_b : nullptr;
        return GRHIP_OK;
    }
};

// ---- constellation_decoder_cb ------------------------------------------------------------------------------------------
struct DecoderBlock : StreamBlock {
    ConstOnDevice tab;

    int init(const grhip_constellation *c, int dev)
    {
        if (!c) return fail(GRHIP_EINVAL, "null constellation");
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        return tab.upload(c->c);
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [] { return GRHIP_OK; });        // nothing kept per stream
    }
    int work_device(int n_out, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n_out);
        if (c <= 0) return c;
        int rc = check_io(d_in, 8, d_out, 1);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n_out;
        if ((rc = check_apart("constellation_decoder_cb", d_in, items * tab.dev.dim * 8, d_out, items))) return rc;
        return decoder_launch(tab.dev, (const float2 *)d_in, (unsigned char *)d_out, n_out, nstreams, st);
    }
    int work(int n_out, const void *in, void *out)      // every output item takes dim complex items
    {
        return host_work(n_out, (size_t)tab.dev.dim * 8, in, (size_t)n_out, 1, out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n_out, d_in, d_out, st);
        });
    }
};

// ---- diff_decoder_bb and map_bb --------------------------------------------------------------------------------------
struct ByteBlock : StreamBlock {
    bool is_map = false;
    unsigned modulus = 1;
    DevBuf d_aux;           // diff: one unsigned per stream, the byte in front of the next call; map: the 256 bytes

    int reset_prev()
    {
        int rc = d_aux.reserve((size_t)nstreams * sizeof(unsigned));
        if (rc) return rc;
        return zero_device(d_aux.p, (size_t)nstreams * sizeof(unsigned));
    }
    int init_diff(unsigned m, int dev)
    {
        if (m == 0) return fail(GRHIP_EINVAL, "diff_decoder_bb: the modulus must not be 0");
        modulus = m;
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        return reset_prev();
    }
    int init_map(const int *map, size_t n, int dev)
    {
        if (n && !map) return fail(GRHIP_EINVAL, "null argument");
        is_map = true;
        unsigned char t[256];
        for (int i = 0; i < 256; ++i) t[i] = (unsigned char)i;                          // gr_map_bb.cc:41-46
        for (size_t i = 0; i < (n < 256 ? n : 256); ++i) t[i] = (unsigned char)map[i];
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        if ((rc = d_aux.reserve(256))) return rc;
        GRHIP_HIP(hipMemcpy(d_aux.p, t, 256, hipMemcpyHostToDevice));
        return GRHIP_OK;
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return is_map ? GRHIP_OK : reset_prev(); });
    }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        int rc = check_io(d_in, 1, d_out, 1);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        // map_bb runs in place; diff_decoder_bb reads the byte in front of the one it writes
        if (is_map) return map_launch((const unsigned char *)d_in, (unsigned char *)d_out, (long long)items, d_aux.as<unsigned char>(), st);
        if ((rc = check_apart("diff_decoder_bb", d_in, items, d_out, items))) return rc;
        return diff_decoder_launch((const unsigned char *)d_in, (unsigned char *)d_out, n, nstreams, modulus, d_aux.as<unsigned>(), 1, st);
    }
    int work(int n, const void *in, void *out)
    {
        return host_work(n, 1, in, (size_t)n, 1, out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

// ---- constellation_receiver_cb and constellation_demod_cb ------------------------------------------------------------
struct ReceiverBlock : StreamBlock {
    Constellation c;
    ConstOnDevice tab;
    ControlLoop cl;
    DevBuf d_state;
    // constellation_demod_cb
    bool demod = false, differential = false, use_map = false;
    unsigned k = 0;
    int engine = 1;
    DevBuf d_map, d_a, d_b;

    int restart() { return fill_state(d_state, ConstState{}); }                 // gri_control_loop.cc:35

    int init(const grhip_constellation *cons, float loop_bw, float fmin, float fmax, int dev)
    {
        if (!cons) return fail(GRHIP_EINVAL, "null constellation");
        c = cons->c;
        if (c.dim != 1)                                          // digital_constellation_receiver_cb.cc:61-62
            return fail(GRHIP_EINVAL, "constellation_receiver_cb: This receiver only works with constellations of dimension 1.");
        if (!ControlLoop::limits_ok(fmax, fmin))
            return fail(GRHIP_EINVAL, "control loop: max_freq and min_freq must be finite and within +-%g rad/sample", (double)CL_FREQ_CAP);
        if (!cl.init(loop_bw, fmax, fmin))                       // :57 gri_control_loop(loop_bw, fmax, fmin)
            return fail(GRHIP_EINVAL, "gri_control_loop: invalid bandwidth. Must be >= 0 (and leave finite gains).");
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        if ((rc = tab.upload(c))) return rc;
        return restart();
    }

    int init_demod(const grhip_constellation *cons, float loop_bw, float fmin, float fmax, int diff, int gray_coded, int dev)
    {
        if (!cons) return fail(GRHIP_EINVAL, "null constellation");
        demod = true;
        differential = diff != 0;
        k = cons->c.bits_per_symbol();
        if (k < 1 || k > 8) return fail(GRHIP_EINVAL, "constellation_demod_cb: 1 .. 8 bits per symbol");
        use_map = gray_coded && cons->c.apply_pre_diff;          // generic_mod_demod.py:305-307
        int rc = init(cons, loop_bw, fmin, fmax, dev);
        if (rc) return rc;
        if (use_map) {
            unsigned char t[256];
            for (int i = 0; i < 256; ++i) t[i] = (unsigned char)i;
            const std::vector<int> inv = invert_code(c.pre_diff);
            for (size_t i = 0; i < inv.size() && i < 256; ++i) t[i] = (unsigned char)inv[i];
            if ((rc = d_map.reserve(256))) return rc;
            GRHIP_HIP(hipMemcpy(d_map.p, t, 256, hipMemcpyHostToDevice));
        }
        return GRHIP_OK;
    }

    int form_of(int m) const
    {
        if (!mode_fast(m)) return RX_FORM_GENERIC;
        return (c.kind == CONST_RECT || c.kind == CONST_CALCDIST) ? RX_FORM_CARTESIAN : RX_FORM_ANGLE;
    }
    int form()
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return form_of(mode);
    }
    int set_engine(int e)
    {
        if (e != 0 && e != 1) return fail(GRHIP_EINVAL, "constellation_demod_cb: engine 0 or 1");
        std::lock_guard<std::mutex> lk(setter_mutex);
        engine = e;
        return GRHIP_OK;
    }
    int get_engine()
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return engine;
    }

    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
    }

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
    int set_state(float ConstState::*which, float v)
    {
        return edit_states<ConstState>(d_state, [&](ConstState &e) { e.*which = v; });
    }
    int set_frequency(float f)              // gri_control_loop.cc:126-135
    {
        float v;
        {
            std::lock_guard<std::mutex> lk(setter_mutex);
            v = cl.set_frequency(f);
        }
        return set_state(&ConstState::freq, v);
    }
    int set_phase(float ph)                 // gri_control_loop.cc:137-145
    {
        if (!ControlLoop::phase_ok(ph)) return fail(GRHIP_EINVAL, "control loop: the phase must be finite and within +-2^20 rad");
        return set_state(&ConstState::phase, ControlLoop::set_phase(ph));
    }
    int get_float(int s, float ConstState::*which, float *v)
    {
        if (!v) return fail(GRHIP_EINVAL, "null argument");
        ConstState t;
        int rc = read_state(d_state, s, &t);
        if (!rc) *v = t.*which;
        return rc;
    }

    ReceiverLaunch launch_of(int n, const void *d_in, void *d_sym)
    {
        ReceiverLaunch l{};
        l.in = (const float2 *)d_in; l.sym = (unsigned char *)d_sym; l.n = n; l.nstreams = nstreams;
        l.p = CarrierParams{cl.alpha, cl.beta, cl.max_freq, cl.min_freq, 0.f, 0};
        l.state = d_state.as<ConstState>();
        return l;
    }

    // the receiver: symbols and, all three or none, error, phase and frequency
    int work_device(int n, const void *d_in, void *d_sym, void *d_err, void *d_phase, void *d_freq, void *stream)
    {
        const int go = check_count(n);
        if (go < 0) return go;
        const int given = (d_err != nullptr) + (d_phase != nullptr) + (d_freq != nullptr);
        if (given != 0 && given != 3)
            return fail(GRHIP_EINVAL, "constellation_receiver_cb: the error, phase and frequency outputs come all three or not at all");
        if (go == 0) return GRHIP_OK;
        int rc = check_io(d_in, 8, d_sym, 1);
        if (rc) return rc;
        if (!aligned(d_err, 4) || !aligned(d_phase, 4) || !aligned(d_freq, 4)) return fail(GRHIP_EINVAL, "items not naturally aligned");
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        const void *b[5] = {d_in, d_sym, d_err, d_phase, d_freq};
        const size_t nb[5] = {items * 8, items, items * 4, items * 4, items * 4};
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j)
                if (overlap(b[i], nb[i], b[j], nb[j])) return fail(GRHIP_EINVAL, "constellation_receiver_cb: the buffers may not overlap");
        ReceiverLaunch l = launch_of(n, d_in, d_sym);
        l.err = (float *)d_err; l.phase = (float *)d_phase; l.freq = (float *)d_freq;
        return receiver_launch(form_of(mode), tab.dev, l, st);
    }

    int work(int n, const void *in, void *sym, void *err, void *phase, void *freq)
    {
        const int go = check_count(n);
        if (go < 0) return go;
        const int given = (err != nullptr) + (phase != nullptr) + (freq != nullptr);
        if (given != 0 && given != 3)
            return fail(GRHIP_EINVAL, "constellation_receiver_cb: the error, phase and frequency outputs come all three or not at all");
        // the three float outputs are staged behind the symbols, each 16-byte aligned
        const size_t items = (size_t)nstreams * (size_t)n;
        const size_t f_off = (items + 15) & ~(size_t)15, f_bytes = items * 4, f_step = (f_bytes + 15) & ~(size_t)15;
        int rc = host_work(n, 8, in, (size_t)n, 1, sym, f_off - items + (given ? 3 * f_step : 0), [&](void *d_in, void *d_out, hipStream_t st) {
            char *f = (char *)d_out + f_off;
            return work_device(n, d_in, d_out, given ? f : nullptr, given ? f + f_step : nullptr, given ? f + 2 * f_step : nullptr, st);
        });
        if (rc || go == 0 || !given) return rc;
        // host_work has synchronised; the staged floats are still there
        void *dst[3] = {err, phase, freq};
        for (int i = 0; i < 3; ++i) GRHIP_D2H(this, dst[i], (char *)stage_out.p + f_off + i * f_step, f_bytes, own_stream);
        GRHIP_HIP(hipStreamSynchronize(own_stream));
        return GRHIP_OK;
    }

    // constellation_demod_cb: n complex items in, n * k bytes out per stream
    int demod_device(int n, const void *d_in, void *d_bits, void *stream)
    {
        const int go = check_count(n);
        if (go <= 0) return go;
        int rc = check_io(d_in, 8, d_bits, 1);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart("constellation_demod_cb", d_in, items * 8, d_bits, items * k))) return rc;
        const unsigned char *map = use_map ? d_map.as<unsigned char>() : nullptr;
        if (engine == 1) {
            ReceiverLaunch l = launch_of(n, d_in, d_bits);
            l.tail = true; l.differential = differential; l.map = map; l.k = k;
            return receiver_launch(form_of(mode), tab.dev, l, st);
        }
        // engine 0: the blocks in a row
        if ((rc = d_a.reserve(items)) || (rc = d_b.reserve(items))) return rc;
        unsigned char *cur = d_a.as<unsigned char>(), *other = d_b.as<unsigned char>();
        if ((rc = receiver_launch(form_of(mode), tab.dev, launch_of(n, d_in, cur), st))) return rc;
        if (differential) {
            if ((rc = diff_decoder_launch(cur, other, n, nstreams, c.arity, &d_state.as<ConstState>()->prev, sizeof(ConstState) / sizeof(unsigned), st))) return rc;
            std::swap(cur, other);
        } else {
            // the previous symbol is kept up to date in both engines, so that they may be switched between calls
            if ((rc = diff_decoder_launch(cur, other, n, nstreams, 1, &d_state.as<ConstState>()->prev, sizeof(ConstState) / sizeof(unsigned), st))) return rc;
        }
        if (map) {
            if ((rc = map_launch(cur, other, (long long)items, map, st))) return rc;
            std::swap(cur, other);
        }
        return launch_unpack_k_bits(k, cur, (unsigned char *)d_bits, (long long)(items * k), st);
    }

    int demod_work(int n, const void *in, void *bits)
    {
        return host_work(n, 8, in, (size_t)n * k, 1, bits, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return demod_device(n, d_in, d_out, st);
        });
    }
};

template <class F>
int make_constellation(grhip_constellation **h, F &&build)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    auto *b = new (std::nothrow) grhip_constellation();
    if (!b) return fail(GRHIP_ENOMEM, "alloc");
    if (!build(b->c)) {
        const int rc = fail(GRHIP_EINVAL, "constellation: %s", b->c.why);
        delete b;
        return rc;
    }
    *h = b;
    return GRHIP_OK;
}

}  // namespace

struct grhip_constellation_decoder_cb : DecoderBlock {};
struct grhip_diff_decoder_bb : ByteBlock {};
struct grhip_map_bb : ByteBlock {};
struct grhip_constellation_receiver_cb : ReceiverBlock {};
struct grhip_constellation_demod_cb : ReceiverBlock {};

extern "C" {

#define GRHIP_CN_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")

// ---- the constellation objects (host) ----------------------------------------------------------------------------------
int grhip_constellation_create_bpsk(grhip_constellation **h) { return make_constellation(h, [](Constellation &c) { c.make_bpsk(); return true; }); }
int grhip_constellation_create_qpsk(grhip_constellation **h) { return make_constellation(h, [](Constellation &c) { c.make_qpsk(); return true; }); }
int grhip_constellation_create_dqpsk(grhip_constellation **h) { return make_constellation(h, [](Constellation &c) { c.make_dqpsk(); return true; }); }
int grhip_constellation_create_8psk(grhip_constellation **h) { return make_constellation(h, [](Constellation &c) { c.make_8psk(); return true; }); }
int grhip_constellation_create_calcdist(grhip_constellation **h, const float *points_re_im, size_t npoints, const unsigned *pre_diff_code,
                                        size_t ncode, unsigned rotational_symmetry, unsigned dimensionality)
{
    return make_constellation(h, [&](Constellation &c) {
        return c.make_calcdist((const cfloat *)points_re_im, npoints, pre_diff_code, ncode, rotational_symmetry, dimensionality);
    });
}
int grhip_constellation_create_psk(grhip_constellation **h, const float *points_re_im, size_t npoints, const unsigned *pre_diff_code,
                                   size_t ncode, unsigned n_sectors)
{
    return make_constellation(h, [&](Constellation &c) { return c.make_psk((const cfloat *)points_re_im, npoints, pre_diff_code, ncode, n_sectors); });
}
int grhip_constellation_create_rect(grhip_constellation **h, const float *points_re_im, size_t npoints, const unsigned *pre_diff_code,
                                    size_t ncode, unsigned rotational_symmetry, unsigned real_sectors, unsigned imag_sectors,
                                    float width_real_sectors, float width_imag_sectors)
{
    return make_constellation(h, [&](Constellation &c) {
        return c.make_rect((const cfloat *)points_re_im, npoints, pre_diff_code, ncode, rotational_symmetry, real_sectors, imag_sectors,
                           width_real_sectors, width_imag_sectors);
    });
}
void grhip_constellation_destroy(grhip_constellation *h) { delete h; }
int grhip_constellation_arity(const grhip_constellation *h) { GRHIP_CN_NULL(h); return (int)h->c.arity; }
int grhip_constellation_dimensionality(const grhip_constellation *h) { GRHIP_CN_NULL(h); return (int)h->c.dim; }
int grhip_constellation_rotational_symmetry(const grhip_constellation *h) { GRHIP_CN_NULL(h); return (int)h->c.rot_sym; }
int grhip_constellation_bits_per_symbol(const grhip_constellation *h) { GRHIP_CN_NULL(h); return (int)h->c.bits_per_symbol(); }
int grhip_constellation_apply_pre_diff_code(const grhip_constellation *h) { GRHIP_CN_NULL(h); return h->c.apply_pre_diff ? 1 : 0; }
int grhip_constellation_n_sectors(const grhip_constellation *h) { GRHIP_CN_NULL(h); return (int)h->c.sector_values.size(); }
int grhip_constellation_points(const grhip_constellation *h, float *points_re_im, size_t capacity)
{
    GRHIP_CN_NULL(h);
    if (capacity && !points_re_im) return fail(GRHIP_EINVAL, "null argument");
    for (size_t i = 0; i < h->c.points.size() && i < capacity; ++i) {
        points_re_im[2 * i] = h->c.points[i].re;
        points_re_im[2 * i + 1] = h->c.points[i].im;
    }
    return (int)h->c.points.size();
}
int grhip_constellation_pre_diff_code(const grhip_constellation *h, unsigned *code, size_t capacity)
{
    GRHIP_CN_NULL(h);
    if (capacity && !code) return fail(GRHIP_EINVAL, "null argument");
    for (size_t i = 0; i < h->c.pre_diff.size() && i < capacity; ++i) code[i] = h->c.pre_diff[i];
    return (int)h->c.pre_diff.size();
}
int grhip_constellation_sector_values(const grhip_constellation *h, unsigned *values, size_t capacity)
{
    GRHIP_CN_NULL(h);
    if (capacity && !values) return fail(GRHIP_EINVAL, "null argument");
    for (size_t i = 0; i < h->c.sector_values.size() && i < capacity; ++i) values[i] = h->c.sector_values[i];
    return (int)h->c.sector_values.size();
}
int grhip_constellation_decision_maker(const grhip_constellation *h, const float *sample_re_im, unsigned *index)
{
    GRHIP_CN_NULL(h);
    if (!sample_re_im || !index) return fail(GRHIP_EINVAL, "null argument");
    *index = h->c.decision_maker((const cfloat *)sample_re_im);
    return GRHIP_OK;
}
int grhip_constellation_decision_maker_pe(const grhip_constellation *h, const float *sample_re_im, unsigned *index, float *phase_error)
{
    GRHIP_CN_NULL(h);
    if (!sample_re_im || !index || !phase_error) return fail(GRHIP_EINVAL, "null argument");
    *index = h->c.decision_maker_pe((const cfloat *)sample_re_im, phase_error);
    return GRHIP_OK;
}

// ---- constellation_decoder_cb, diff_decoder_bb, map_bb -------------------------------------------------------------------
#define GRHIP_CN_STREAM_BLOCK(NAME)                                                                                   \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { GRHIP_CN_NULL(h); return h->set_mode(mode); }            \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams) { GRHIP_CN_NULL(h); return h->set_streams(nstreams); }
#define GRHIP_CN_BYTE_WORK(NAME)                                                                                      \
    int grhip_##NAME##_work(grhip_##NAME *h, int n, const void *in, void *out) { GRHIP_CN_NULL(h); return h->work(n, in, out); } \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n, const void *d_in, void *d_out, void *stream)               \
    {                                                                                                                 \
        GRHIP_CN_NULL(h);                                                                                             \
        return h->work_device(n, d_in, d_out, stream);                                                                \
    }

int grhip_constellation_decoder_cb_create(grhip_constellation_decoder_cb **h, const grhip_constellation *constellation, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_constellation_decoder_cb *b) { return b->init(constellation, device); });
}
GRHIP_CN_STREAM_BLOCK(constellation_decoder_cb)
GRHIP_CN_BYTE_WORK(constellation_decoder_cb)

int grhip_diff_decoder_bb_create(grhip_diff_decoder_bb **h, unsigned modulus, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_diff_decoder_bb *b) { return b->init_diff(modulus, device); });
}
GRHIP_CN_STREAM_BLOCK(diff_decoder_bb)
GRHIP_CN_BYTE_WORK(diff_decoder_bb)

int grhip_map_bb_create(grhip_map_bb **h, const int *map, size_t nmap, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_map_bb *b) { return b->init_map(map, nmap, device); });
}
GRHIP_CN_STREAM_BLOCK(map_bb)
GRHIP_CN_BYTE_WORK(map_bb)

// ---- constellation_receiver_cb and constellation_demod_cb: gri_control_loop.h:99-200 ---------------------------------
#define GRHIP_CN_GET(NAME, ENTRY, FIELD)                                                                              \
    float grhip_##NAME##_##ENTRY(grhip_##NAME *h)                                                                     \
    {                                                                                                                 \
        if (!h) return (float)fail(GRHIP_EINVAL, "null handle");                                                      \
        return h->get_param(&ControlLoop::FIELD);                                                                     \
    }
#define GRHIP_CN_LOOP(NAME)                                                                                           \
    GRHIP_CN_STREAM_BLOCK(NAME)                                                                                       \
    int grhip_##NAME##_form(grhip_##NAME *h) { GRHIP_CN_NULL(h); return h->form(); }                                  \
    int grhip_##NAME##_set_loop_bandwidth(grhip_##NAME *h, float bw)                                                  \
    {                                                                                                                 \
        GRHIP_CN_NULL(h);                                                                                             \
        return h->set_param(&ControlLoop::set_loop_bandwidth, bw, "bandwidth. Must be >= 0 (and leave finite gains).");  \
    }                                                                                                                 \
    int grhip_##NAME##_set_damping_factor(grhip_##NAME *h, float df)                                                  \
    {                                                                                                                 \
        GRHIP_CN_NULL(h);                                                                                             \
        return h->set_param(&ControlLoop::set_damping_factor, df, "damping factor. Must be in [0,1].");               \
    }                                                                                                                 \
    int grhip_##NAME##_set_alpha(grhip_##NAME *h, float alpha)                                                        \
    {                                                                                                                 \
        GRHIP_CN_NULL(h);                                                                                             \
        return h->set_param(&ControlLoop::set_alpha, alpha, "alpha. Must be in [0,1].");                              \
    }                                                                                                                 \
    int grhip_##NAME##_set_beta(grhip_##NAME *h, float beta)                                                          \
    {                                                                                                                 \
        GRHIP_CN_NULL(h);                                                                                             \
        return h->set_param(&ControlLoop::set_beta, beta, "beta. Must be in [0,1].");                                 \
    }                                                                                                                 \
    int grhip_##NAME##_set_frequency(grhip_##NAME *h, float freq) { GRHIP_CN_NULL(h); return h->set_frequency(freq); } \
    int grhip_##NAME##_set_phase(grhip_##NAME *h, float phase) { GRHIP_CN_NULL(h); return h->set_phase(phase); }      \
    GRHIP_CN_GET(NAME, get_loop_bandwidth, loop_bw)                                                                   \
    GRHIP_CN_GET(NAME, get_damping_factor, damping)                                                                   \
    GRHIP_CN_GET(NAME, get_alpha, alpha)                                                                              \
    GRHIP_CN_GET(NAME, get_beta, beta)                                                                                \
    int grhip_##NAME##_get_frequency(grhip_##NAME *h, int s, float *freq)                                             \
    {                                                                                                                 \
        GRHIP_CN_NULL(h);                                                                                             \
        return h->get_float(s, &ConstState::freq, freq);                                                              \
    }                                                                                                                 \
    int grhip_##NAME##_get_phase(grhip_##NAME *h, int s, float *phase)                                                \
    {                                                                                                                 \
        GRHIP_CN_NULL(h);                                                                                             \
        return h->get_float(s, &ConstState::phase, phase);                                                            \
    }

int grhip_constellation_receiver_cb_create(grhip_constellation_receiver_cb **h, const grhip_constellation *constellation, float loop_bw,
                                           float fmin, float fmax, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_constellation_receiver_cb *b) { return b->init(constellation, loop_bw, fmin, fmax, device); });
}
GRHIP_CN_LOOP(constellation_receiver_cb)
int grhip_constellation_receiver_cb_work(grhip_constellation_receiver_cb *h, int n_in, const void *in, void *symbols, void *error,
                                         void *phase, void *freq)
{
    GRHIP_CN_NULL(h);
    return h->work(n_in, in, symbols, error, phase, freq);
}
int grhip_constellation_receiver_cb_work_device(grhip_constellation_receiver_cb *h, int n_in, const void *d_in, void *d_symbols,
                                                void *d_error, void *d_phase, void *d_freq, void *stream)
{
    GRHIP_CN_NULL(h);
    return h->work_device(n_in, d_in, d_symbols, d_error, d_phase, d_freq, stream);
}

int grhip_constellation_demod_cb_create(grhip_constellation_demod_cb **h, const grhip_constellation *constellation, float loop_bw,
                                        float fmin, float fmax, int differential, int gray_coded, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_constellation_demod_cb *b) {
        return b->init_demod(constellation, loop_bw, fmin, fmax, differential, gray_coded, device);
    });
}
GRHIP_CN_LOOP(constellation_demod_cb)
int grhip_constellation_demod_cb_set_engine(grhip_constellation_demod_cb *h, int engine) { GRHIP_CN_NULL(h); return h->set_engine(engine); }
int grhip_constellation_demod_cb_engine(grhip_constellation_demod_cb *h) { GRHIP_CN_NULL(h); return h->get_engine(); }
int grhip_constellation_demod_cb_bits_per_symbol(grhip_constellation_demod_cb *h) { GRHIP_CN_NULL(h); return (int)h->k; }
int grhip_constellation_demod_cb_work(grhip_constellation_demod_cb *h, int n_in, const void *in, void *bits)
{
    GRHIP_CN_NULL(h);
    return h->demod_work(n_in, in, bits);
}
int grhip_constellation_demod_cb_work_device(grhip_constellation_demod_cb *h, int n_in, const void *d_in, void *d_bits, void *stream)
{
    GRHIP_CN_NULL(h);
    return h->demod_device(n_in, d_in, d_bits, stream);
}

#undef GRHIP_CN_LOOP
#undef GRHIP_CN_GET
#undef GRHIP_CN_BYTE_WORK
#undef GRHIP_CN_STREAM_BLOCK
#undef GRHIP_CN_NULL

}  // extern "C"
