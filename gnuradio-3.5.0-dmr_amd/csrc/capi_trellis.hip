// capi_trellis.hip -- C ABI of gr-trellis' coding layer: fsm (gr-trellis/src/lib/fsm.cc), trellis_encoder_XX
// (trellis_encoder_XX.cc.t), trellis_metrics_X (trellis_metrics_X.cc.t, calc_metric.cc), trellis_constellation_metrics_cf
// (trellis_constellation_metrics_cf.cc, digital_constellation.cc:160-201), trellis_viterbi_X (trellis_viterbi_X.cc.t,
// core_algorithms.cc:45-109) and trellis_viterbi_combined_XX (trellis_viterbi_combined_XX.cc.t, core_algorithms.cc:147-217).
//
// A grhip_fsm lives on the host (csrc/trellis_fsm.h) and needs no device.  A block copies the FSM it is created from, so
// the fsm handle may be destroyed first.  The blocks take S streams back to back, as every stream block does.
#include <vector>

#include "constellation_blocks.h"
#include "stream_block.h"
#include "trellis.h"

using namespace grhip;

struct grhip_fsm {
    Fsm f;
};

namespace {

int upload_ints(DevBuf &d, const std::vector<int> &v)
{
    int rc = d.reserve(v.size() * sizeof(int) + 4);
    if (rc) return rc;
    if (!v.empty()) GRHIP_HIP(hipMemcpy(d.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return GRHIP_OK;
}

// do the byte counts of `items` items of `size` bytes on `streams` streams fit an int?
bool fits_int(long long streams, long long items, long long size)
{
    return streams * items <= 0x7fffffffLL / size;
}

// ---- trellis_encoder_XX ------------------------------------------------------------------------------------------------
struct EncoderBlock : StreamBlock {
    Fsm f;
    int st0 = 0, tin = TR_B, tout = TR_B;
    DevBuf d_ns, d_os, d_state, d_backup, d_flag, d_maps, d_starts;

    int restart() { return fill_state(d_state, st0); }
    int init(const grhip_fsm *fsm, int ST, int ti, int to, int dev)
    {
        if (!fsm) return fail(GRHIP_EINVAL, "null fsm");
        if (ST < 0 || ST >= fsm->f.S) return fail(GRHIP_EINVAL, "trellis_encoder: the state %d is outside [0, %d)", ST, fsm->f.S);
        f = fsm->f; st0 = ST; tin = ti; tout = to;
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        if ((rc = upload_ints(d_ns, f.NS)) || (rc = upload_ints(d_os, f.OS))) return rc;
        if ((rc = d_flag.reserve(sizeof(unsigned))) || (rc = zero_device(d_flag.p, sizeof(unsigned)))) return rc;
        return restart();
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
    }
    int set_ST(int ST)
    {
        if (ST < 0 || ST >= f.S) return fail(GRHIP_EINVAL, "trellis_encoder: the state %d is outside [0, %d)", ST, f.S);
        const int rc = edit_states<int>(d_state, [&](int &s) { s = ST; });
        if (!rc) st0 = ST;
        return rc;
    }
    int ST(int stream, int *out)
    {
        if (!out) return fail(GRHIP_EINVAL, "null argument");
        return read_state(d_state, stream, out);
    }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        const size_t isz = tr_item_size(tin), osz = tr_item_size(tout);
        int rc = check_io(d_in, isz, d_out, osz);
        if (rc) return rc;
        if (!fits_int(nstreams, n, (long long)osz)) return fail(GRHIP_EINVAL, "trellis_encoder: the call's byte count does not fit an int");
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart("trellis_encoder", d_in, items * isz, d_out, items * osz))) return rc;
        const size_t state_bytes = (size_t)nstreams * sizeof(int);
        if ((rc = d_backup.reserve(state_bytes))) return rc;
        GRHIP_HIP(hipMemcpyAsync(d_backup.p, d_state.p, state_bytes, hipMemcpyDeviceToDevice, st));
        if (mode_fast(mode) && f.S <= ENC_MAX_S && n > ENC_CHUNK) {
            const size_t chunks = ((size_t)n + ENC_CHUNK - 1) / ENC_CHUNK;
            if ((rc = d_maps.reserve((size_t)nstreams * chunks * f.S)) || (rc = d_starts.reserve((size_t)nstreams * chunks * sizeof(int))))
                return rc;
            rc = encoder_chunked_launch(tin, tout, d_in, d_out, n, nstreams, f.I, f.S, d_ns.as<int>(), d_os.as<int>(), d_state.as<int>(),
                                        d_flag.as<unsigned>(), d_maps.as<unsigned char>(), d_starts.as<int>(), st);
        } else {
            rc = encoder_serial_launch(tin, tout, d_in, d_out, n, nstreams, f.I, d_ns.as<int>(), d_os.as<int>(), d_state.as<int>(),
                                       d_flag.as<unsigned>(), st);
        }
        if (rc) return rc;
        // the flag word of the kernels, read after the call: an input outside [0, I) leaves every state as it was
        unsigned flag = 0;
        GRHIP_HIP(hipMemcpyAsync(&flag, d_flag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
        GRHIP_HIP(hipStreamSynchronize(st));
        if (flag) {
            GRHIP_HIP(hipMemcpyAsync(d_state.p, d_backup.p, state_bytes, hipMemcpyDeviceToDevice, st));
            GRHIP_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(unsigned), st));
            GRHIP_HIP(hipStreamSynchronize(st));
            return fail(GRHIP_EINVAL, "trellis_encoder: an input symbol outside [0, %d)", f.I);
        }
        return GRHIP_OK;
    }
    int work(int n, const void *in, void *out)
    {
        return host_work(n, tr_item_size(tin), in, (size_t)n, tr_item_size(tout), out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

// ---- trellis_metrics_X, trellis_constellation_metrics_cf ---------------------------------------------------------------
struct MetricsBlock : StreamBlock {
    int t = TR_F, O = 0, D = 0, type = TRELLIS_EUCLIDEAN;
    DevBuf d_table;

    static int check_type(int type)
    {
        // calc_metric.cc:66-70 throws in work for HARD_BIT and for anything else
        if (type != TRELLIS_EUCLIDEAN && type != TRELLIS_HARD_SYMBOL) return fail(GRHIP_EINVAL, "trellis_metrics: metric type %d is not built", type);
        return GRHIP_OK;
    }
    int load_table(const void *table, long long n)
    {
        if (!table || n != (long long)O * D) return fail(GRHIP_EINVAL, "trellis_metrics: TABLE needs O * D = %lld items", (long long)O * D);
        int rc = d_table.reserve((size_t)n * tr_item_size(t));
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(d_table.p, table, (size_t)n * tr_item_size(t), hipMemcpyHostToDevice));
        return GRHIP_OK;
    }
    int init(int item, int o, int d, const void *table, long long n, int ty, int dev)
    {
        if (o < 1 || d < 1 || (long long)o * d > (1 << 24)) return fail(GRHIP_EINVAL, "trellis_metrics: O and D must be at least 1, O * D at most 2^24");
        int rc = check_type(ty);
        if (rc) return rc;
        t = item; O = o; D = d; type = ty;
        mode = default_mode();
        if ((rc = init_device(dev))) return rc;
        return load_table(table, n);
    }
    int set_TABLE(const void *table, long long n)
    {
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        return load_table(table, n);
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [] { return GRHIP_OK; });        // nothing kept per stream
    }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        const size_t isz = tr_item_size(t);
        int rc = check_io(d_in, isz, d_out, 4);
        if (rc) return rc;
        if (!fits_int(nstreams, (long long)n * O, 4) || !fits_int(nstreams, (long long)n * D, (long long)isz))
            return fail(GRHIP_EINVAL, "trellis_metrics: the call's byte count does not fit an int");
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t steps = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart("trellis_metrics", d_in, steps * D * isz, d_out, steps * O * 4))) return rc;
        return metrics_launch(t, type, d_in, (float *)d_out, (long long)steps, O, D, d_table.p, st);
    }
    int work(int n, const void *in, void *out)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        if (!fits_int(nstreams, (long long)n * O, 4) || !fits_int(nstreams, (long long)n * D, (long long)tr_item_size(t)))
            return fail(GRHIP_EINVAL, "trellis_metrics: the call's byte count does not fit an int");
        return host_work(n * D, tr_item_size(t), in, (size_t)n * O, 4, out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

// ---- trellis_viterbi_X -------------------------------------------------------------------------------------------------
struct ViterbiBlock : StreamBlock {
    Fsm f;
    int K = 0, S0 = -1, SK = -1, tout = TR_B, Pmax = 0;
    VitPlan fast{}, generic{};
    DevBuf d_tab, d_cnt, d_ws, d_dead;

    const VitPlan &plan() const { return mode_fast(mode) ? fast : generic; }
    int init(const grhip_fsm *fsm, int k, int s0, int sk, int to, int dev)
    {
        if (!fsm) return fail(GRHIP_EINVAL, "null fsm");
        f = fsm->f; K = k; S0 = s0 < 0 ? -1 : s0; SK = sk < 0 ? -1 : sk; tout = to;
        if (K < 1) return fail(GRHIP_EINVAL, "trellis_viterbi: K must be at least 1");
        if (f.S > VIT_MAX_S) return fail(GRHIP_EINVAL, "trellis_viterbi: at most %d states", VIT_MAX_S);
        if (S0 >= f.S || SK >= f.S) return fail(GRHIP_EINVAL, "trellis_viterbi: S0 and SK must be below S = %d", f.S);
        if (!fits_int(1, (long long)K * f.O, 4)) return fail(GRHIP_EINVAL, "trellis_viterbi: K * O floats do not fit an int of bytes");
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        Pmax = 0;
        std::vector<int> cnt((size_t)f.S);
        for (int j = 0; j < f.S; ++j) {
            cnt[j] = (int)f.PS[j].size();
            if (cnt[j] > Pmax) Pmax = cnt[j];
        }
        const int pm = Pmax < 1 ? 1 : Pmax;
        if ((long long)f.S * pm > (1 << 24)) return fail(GRHIP_EINVAL, "trellis_viterbi: S * Pmax above 2^24");
        // per next state its predecessors, padded to Pmax: {ps | pi << 10, OS[ps * I + pi]}; a padded round never runs
        std::vector<int> tab((size_t)f.S * pm * 2, 0);
        for (int j = 0; j < f.S; ++j)
            for (int i = 0; i < cnt[j]; ++i) {
                const int ps = f.PS[j][i], pi = f.PI[j][i];
                tab[((size_t)j * pm + i) * 2] = ps | (pi << 10);
                tab[((size_t)j * pm + i) * 2 + 1] = f.OS[(size_t)ps * f.I + pi];
            }
        const int cus = device_cus();
        if (!viterbi_plan(f.S, f.O, K, S0, SK, Pmax, tr_item_size(tout), cus, false, fast) ||
            !viterbi_plan(f.S, f.O, K, S0, SK, Pmax, tr_item_size(tout), cus, true, generic))
            return fail(GRHIP_EINVAL, "trellis_viterbi: the trace of one block of K = %d steps is above the workspace cap", K);
        if ((rc = upload_ints(d_tab, tab)) || (rc = upload_ints(d_cnt, cnt))) return rc;
        if (fast.ws_words && (rc = d_ws.reserve((size_t)fast.max_groups * fast.ws_words * 8))) return rc;
        if ((rc = d_dead.reserve(sizeof(unsigned long long)))) return rc;
        return zero_device(d_dead.p, sizeof(unsigned long long));
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [] { return GRHIP_OK; });        // stateless between calls
    }
    int dead_ends(long long *out)
    {
        if (!out) return fail(GRHIP_EINVAL, "null argument");
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        unsigned long long v = 0;
        GRHIP_HIP(hipMemcpy(&v, d_dead.p, sizeof(v), hipMemcpyDeviceToHost));
        *out = (long long)v;
        return GRHIP_OK;
    }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        if (n % K) return fail(GRHIP_EINVAL, "trellis_viterbi: n = %d is no multiple of K = %d", n, K);
        const size_t osz = tr_item_size(tout);
        int rc = check_io(d_in, 4, d_out, osz);
        if (rc) return rc;
        if (!fits_int(nstreams, (long long)n * f.O, 4) || !fits_int(nstreams, n, (long long)osz))
            return fail(GRHIP_EINVAL, "trellis_viterbi: the call's byte count does not fit an int");
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart("trellis_viterbi", d_in, items * f.O * 4, d_out, items * osz))) return rc;
        return viterbi_launch(plan(), tout, (const float *)d_in, d_out, (long long)(items / K), (const int2 *)d_tab.p, d_cnt.as<int>(),
                              d_ws.as<unsigned long long>(), d_dead.as<unsigned long long>(), VitRaw{}, st);
    }
    int work(int n, const void *in, void *out)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        if (n % K) return fail(GRHIP_EINVAL, "trellis_viterbi: n = %d is no multiple of K = %d", n, K);
        if (!fits_int(nstreams, (long long)n * f.O, 4)) return fail(GRHIP_EINVAL, "trellis_viterbi: the call's byte count does not fit an int");
        return host_work(n * f.O, 4, in, (size_t)n, tr_item_size(tout), out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

// ---- trellis_viterbi_combined_XX ---------------------------------------------------------------------------------------
// viterbi_algorithm_combined (core_algorithms.cc:147-217): the decoder on calc_metric of D raw items per step.  Engine 0
// runs the metrics kernel into a scratch buffer and then the decoder; engine 1 forms the metrics inside the decoder's
// LDS window.  GENERIC, and an O too large for the window, take engine 0.
struct CombinedBlock : ViterbiBlock {
    int tin = TR_F, D = 1, type = TRELLIS_EUCLIDEAN, want_engine = 1;
    DevBuf d_table, d_metrics;

    int load_table(const void *table, long long n)
    {
        if (!table || n != (long long)f.O * D) return fail(GRHIP_EINVAL, "trellis_viterbi_combined: TABLE needs O * D = %lld items", (long long)f.O * D);
        int rc = d_table.reserve((size_t)n * tr_item_size(tin));
        if (rc) return rc;
        GRHIP_HIP(hipMemcpy(d_table.p, table, (size_t)n * tr_item_size(tin), hipMemcpyHostToDevice));
        return GRHIP_OK;
    }
    int init(const grhip_fsm *fsm, int k, int s0, int sk, int d, const void *table, long long n, int ty, int ti, int to, int dev)
    {
        if (d < 1 || d > (1 << 16)) return fail(GRHIP_EINVAL, "trellis_viterbi_combined: D must be 1 .. 65536");
        int rc = MetricsBlock::check_type(ty);
        if (rc) return rc;
        tin = ti; D = d; type = ty;
        if ((rc = ViterbiBlock::init(fsm, k, s0, sk, to, dev))) return rc;
        if (!fits_int(1, (long long)K * D, (long long)tr_item_size(tin))) return fail(GRHIP_EINVAL, "trellis_viterbi_combined: K * D items do not fit an int of bytes");
        return load_table(table, n);
    }
    int set_TABLE(const void *table, long long n)
    {
        int rc = bind();
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = drain(own_stream))) return rc;
        return load_table(table, n);
    }
    int set_engine(int e)
    {
        if (e != 0 && e != 1) return fail(GRHIP_EINVAL, "trellis_viterbi_combined: engine 0 or 1");
        std::lock_guard<std::mutex> lk(setter_mutex);
        want_engine = e;
        return GRHIP_OK;
    }
    int engine() const { return want_engine == 1 && mode_fast(mode) && fast.W > 0 ? 1 : 0; }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        if (n % K) return fail(GRHIP_EINVAL, "trellis_viterbi_combined: n = %d is no multiple of K = %d", n, K);
        const size_t isz = tr_item_size(tin), osz = tr_item_size(tout);
        int rc = check_io(d_in, isz, d_out, osz);
        if (rc) return rc;
        if (!fits_int(nstreams, (long long)n * f.O, 4) || !fits_int(nstreams, (long long)n * D, (long long)isz) || !fits_int(nstreams, n, (long long)osz))
            return fail(GRHIP_EINVAL, "trellis_viterbi_combined: the call's byte count does not fit an int");
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart("trellis_viterbi_combined", d_in, items * D * isz, d_out, items * osz))) return rc;
        if (engine() == 1) {
            VitRaw raw;
            raw.in = d_in; raw.table = d_table.p; raw.t = tin; raw.D = D; raw.type = type; raw.item_bytes = (int)isz;
            return viterbi_launch(fast, tout, nullptr, d_out, (long long)(items / K), (const int2 *)d_tab.p, d_cnt.as<int>(),
                                  d_ws.as<unsigned long long>(), d_dead.as<unsigned long long>(), raw, st);
        }
        if ((rc = d_metrics.reserve(items * f.O * 4))) return rc;
        if ((rc = metrics_launch(tin, type, d_in, d_metrics.as<float>(), (long long)items, f.O, D, d_table.p, st))) return rc;
        return viterbi_launch(plan(), tout, d_metrics.as<float>(), d_out, (long long)(items / K), (const int2 *)d_tab.p, d_cnt.as<int>(),
                              d_ws.as<unsigned long long>(), d_dead.as<unsigned long long>(), VitRaw{}, st);
    }
    int work(int n, const void *in, void *out)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        if (n % K) return fail(GRHIP_EINVAL, "trellis_viterbi_combined: n = %d is no multiple of K = %d", n, K);
        if (!fits_int(nstreams, (long long)n * D, (long long)tr_item_size(tin))) return fail(GRHIP_EINVAL, "trellis_viterbi_combined: the call's byte count does not fit an int");
        return host_work(n * D, tr_item_size(tin), in, (size_t)n, tr_item_size(tout), out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

int fsm_out(grhip_fsm **h, Fsm &f, bool ok, const char *what)
{
    if (!ok) return fail(GRHIP_EINVAL, "fsm: %s refused (sizes below 1 or above the caps, table lengths, entries out of range, or a text that ends early)", what);
    auto *b = new (std::nothrow) grhip_fsm();
    if (!b) return fail(GRHIP_ENOMEM, "alloc");
    b->f = std::move(f);
    *h = b;
    return GRHIP_OK;
}

int copy_ints(const std::vector<int> &v, int *out, int cap)
{
    if (v.size() > 0x7fffffffu) return fail(GRHIP_ERANGE, "fsm: the table does not fit an int count");
    if (out) {
        if (cap < (int)v.size()) return fail(GRHIP_EINVAL, "fsm: room for %d of %d entries", cap, (int)v.size());
        if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(int));
    }
    return (int)v.size();
}

}  // namespace

struct grhip_trellis_encoder_bb : EncoderBlock {};
struct grhip_trellis_encoder_bs : EncoderBlock {};
struct grhip_trellis_encoder_bi : EncoderBlock {};
struct grhip_trellis_encoder_ss : EncoderBlock {};
struct grhip_trellis_encoder_si : EncoderBlock {};
struct grhip_trellis_encoder_ii : EncoderBlock {};
struct grhip_trellis_metrics_s : MetricsBlock {};
struct grhip_trellis_metrics_i : MetricsBlock {};
struct grhip_trellis_metrics_f : MetricsBlock {};
struct grhip_trellis_metrics_c : MetricsBlock {};
struct grhip_trellis_constellation_metrics_cf : MetricsBlock {};
struct grhip_trellis_viterbi_b : ViterbiBlock {};
struct grhip_trellis_viterbi_s : ViterbiBlock {};
struct grhip_trellis_viterbi_i : ViterbiBlock {};
struct grhip_trellis_viterbi_combined_sb : CombinedBlock {};
struct grhip_trellis_viterbi_combined_ss : CombinedBlock {};
struct grhip_trellis_viterbi_combined_si : CombinedBlock {};
struct grhip_trellis_viterbi_combined_ib : CombinedBlock {};
struct grhip_trellis_viterbi_combined_is : CombinedBlock {};
struct grhip_trellis_viterbi_combined_ii : CombinedBlock {};
struct grhip_trellis_viterbi_combined_fb : CombinedBlock {};
struct grhip_trellis_viterbi_combined_fs : CombinedBlock {};
struct grhip_trellis_viterbi_combined_fi : CombinedBlock {};
struct grhip_trellis_viterbi_combined_cb : CombinedBlock {};
struct grhip_trellis_viterbi_combined_cs : CombinedBlock {};
struct grhip_trellis_viterbi_combined_ci : CombinedBlock {};

extern "C" {

#define GRHIP_TR_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")

// ---- fsm (host) --------------------------------------------------------------------------------------------------------
int grhip_fsm_create(grhip_fsm **h, int I, int S, int O, const int *NS, int n_NS, const int *OS, int n_OS)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (!NS || !OS || n_NS < 0 || n_OS < 0) return fail(GRHIP_EINVAL, "fsm: null table");
    Fsm f;
    const bool ok = fsm_from_tables(I, S, O, std::vector<int>(NS, NS + n_NS), std::vector<int>(OS, OS + n_OS), f);
    return fsm_out(h, f, ok, "(I, S, O, NS, OS)");
}
int grhip_fsm_create_text(grhip_fsm **h, const char *text)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    Fsm f;
    const bool ok = fsm_from_text(text, f);
    return fsm_out(h, f, ok, "the text");
}
int grhip_fsm_create_file(grhip_fsm **h, const char *path)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    Fsm f;
    const bool ok = fsm_from_file(path, f);
    return fsm_out(h, f, ok, "the file (or it cannot be opened)");
}
int grhip_fsm_create_generator(grhip_fsm **h, int k, int n, const int *G, int n_G)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (!G || n_G < 0) return fail(GRHIP_EINVAL, "fsm: null generator matrix");
    Fsm f;
    const bool ok = fsm_from_generator(k, n, std::vector<int>(G, G + n_G), f);
    return fsm_out(h, f, ok, "(k, n, G)");
}
int grhip_fsm_create_isi(grhip_fsm **h, int mod_size, int ch_length)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    Fsm f;
    const bool ok = fsm_from_isi(mod_size, ch_length, f);
    return fsm_out(h, f, ok, "(mod_size, ch_length)");
}
int grhip_fsm_create_cpm(grhip_fsm **h, int P, int M, int L)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    Fsm f;
    const bool ok = fsm_from_cpm(P, M, L, f);
    return fsm_out(h, f, ok, "(P, M, L)");
}
int grhip_fsm_create_joint(grhip_fsm **h, const grhip_fsm *fsm1, const grhip_fsm *fsm2)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (!fsm1 || !fsm2) return fail(GRHIP_EINVAL, "null fsm");
    Fsm f;
    const bool ok = fsm_from_joint(fsm1->f, fsm2->f, f);
    return fsm_out(h, f, ok, "(FSM1, FSM2)");
}
int grhip_fsm_create_radix(grhip_fsm **h, const grhip_fsm *fsm, int n)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (!fsm) return fail(GRHIP_EINVAL, "null fsm");
    Fsm f;
    const bool ok = fsm_from_radix(fsm->f, n, f);
    return fsm_out(h, f, ok, "(FSM, n)");
}
void grhip_fsm_destroy(grhip_fsm *h) { delete h; }
int grhip_fsm_I(const grhip_fsm *h) { GRHIP_TR_NULL(h); return h->f.I; }
int grhip_fsm_S(const grhip_fsm *h) { GRHIP_TR_NULL(h); return h->f.S; }
int grhip_fsm_O(const grhip_fsm *h) { GRHIP_TR_NULL(h); return h->f.O; }
int grhip_fsm_connected(const grhip_fsm *h) { GRHIP_TR_NULL(h); return h->f.connected ? 1 : 0; }
int grhip_fsm_NS(const grhip_fsm *h, int *out, int cap) { GRHIP_TR_NULL(h); return copy_ints(h->f.NS, out, cap); }
int grhip_fsm_OS(const grhip_fsm *h, int *out, int cap) { GRHIP_TR_NULL(h); return copy_ints(h->f.OS, out, cap); }
int grhip_fsm_TMl(const grhip_fsm *h, int *out, int cap) { GRHIP_TR_NULL(h); return copy_ints(h->f.TMl, out, cap); }
int grhip_fsm_TMi(const grhip_fsm *h, int *out, int cap) { GRHIP_TR_NULL(h); return copy_ints(h->f.TMi, out, cap); }
int grhip_fsm_PS(const grhip_fsm *h, int state, int *out, int cap)
{
    GRHIP_TR_NULL(h);
    if (state < 0 || state >= h->f.S) return fail(GRHIP_EINVAL, "fsm: state %d of %d", state, h->f.S);
    return copy_ints(h->f.PS[state], out, cap);
}
int grhip_fsm_PI(const grhip_fsm *h, int state, int *out, int cap)
{
    GRHIP_TR_NULL(h);
    if (state < 0 || state >= h->f.S) return fail(GRHIP_EINVAL, "fsm: state %d of %d", state, h->f.S);
    return copy_ints(h->f.PI[state], out, cap);
}

// ---- what every block has ----------------------------------------------------------------------------------------------
#define GRHIP_TR_BLOCK(NAME)                                                                                          \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { GRHIP_TR_NULL(h); return h->set_mode(mode); }            \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams) { GRHIP_TR_NULL(h); return h->set_streams(nstreams); } \
    int grhip_##NAME##_work(grhip_##NAME *h, int n, const void *in, void *out) { GRHIP_TR_NULL(h); return h->work(n, in, out); } \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n, const void *d_in, void *d_out, void *stream)               \
    {                                                                                                                 \
        GRHIP_TR_NULL(h);                                                                                             \
        return h->work_device(n, d_in, d_out, stream);                                                                \
    }

#define GRHIP_TR_ENCODER(NAME, TI, TO)                                                                                \
    int grhip_##NAME##_create(grhip_##NAME **h, const grhip_fsm *fsm, int ST, int device)                             \
    {                                                                                                                 \
        if (!h) return fail(GRHIP_EINVAL, "null argument");                                                           \
        return make_handle(h, [&](grhip_##NAME *b) { return b->init(fsm, ST, TI, TO, device); });                     \
    }                                                                                                                 \
    GRHIP_TR_BLOCK(NAME)                                                                                              \
    int grhip_##NAME##_ST(grhip_##NAME *h, int stream, int *ST) { GRHIP_TR_NULL(h); return h->ST(stream, ST); }       \
    int grhip_##NAME##_set_ST(grhip_##NAME *h, int ST) { GRHIP_TR_NULL(h); return h->set_ST(ST); }

GRHIP_TR_ENCODER(trellis_encoder_bb, TR_B, TR_B)
GRHIP_TR_ENCODER(trellis_encoder_bs, TR_B, TR_S)
GRHIP_TR_ENCODER(trellis_encoder_bi, TR_B, TR_I)
GRHIP_TR_ENCODER(trellis_encoder_ss, TR_S, TR_S)
GRHIP_TR_ENCODER(trellis_encoder_si, TR_S, TR_I)
GRHIP_TR_ENCODER(trellis_encoder_ii, TR_I, TR_I)

#define GRHIP_TR_METRICS_TAIL(NAME)                                                                                   \
    GRHIP_TR_BLOCK(NAME)                                                                                              \
    int grhip_##NAME##_O(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->O; }                                          \
    int grhip_##NAME##_D(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->D; }                                          \
    int grhip_##NAME##_TYPE(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->type; }

#define GRHIP_TR_METRICS(NAME, T)                                                                                     \
    int grhip_##NAME##_create(grhip_##NAME **h, int O, int D, const void *TABLE, int n_TABLE, int TYPE, int device)   \
    {                                                                                                                 \
        if (!h) return fail(GRHIP_EINVAL, "null argument");                                                           \
        return make_handle(h, [&](grhip_##NAME *b) { return b->init(T, O, D, TABLE, n_TABLE, TYPE, device); });       \
    }                                                                                                                 \
    GRHIP_TR_METRICS_TAIL(NAME)                                                                                       \
    int grhip_##NAME##_set_TABLE(grhip_##NAME *h, const void *TABLE, int n_TABLE)                                     \
    {                                                                                                                 \
        GRHIP_TR_NULL(h);                                                                                             \
        return h->set_TABLE(TABLE, n_TABLE);                                                                          \
    }

GRHIP_TR_METRICS(trellis_metrics_s, TR_S)
GRHIP_TR_METRICS(trellis_metrics_i, TR_I)
GRHIP_TR_METRICS(trellis_metrics_f, TR_F)
GRHIP_TR_METRICS(trellis_metrics_c, TR_C)

int grhip_trellis_constellation_metrics_cf_create(grhip_trellis_constellation_metrics_cf **h, const grhip_constellation *constellation,
                                                  int TYPE, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    if (!constellation) return fail(GRHIP_EINVAL, "null constellation");
    const Constellation &c = constellation->c;
    return make_handle(h, [&](grhip_trellis_constellation_metrics_cf *b) {
        return b->init(TR_C, (int)c.arity, (int)c.dim, c.points.data(), (long long)c.points.size(), TYPE, device);
    });
}
GRHIP_TR_METRICS_TAIL(trellis_constellation_metrics_cf)

// what the decoder handles report
#define GRHIP_TR_DECODER_GETTERS(NAME)                                                                                \
    int grhip_##NAME##_K(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->K; }                                          \
    int grhip_##NAME##_S0(grhip_##NAME *h, int *S0) { GRHIP_TR_NULL(h); if (!S0) return fail(GRHIP_EINVAL, "null argument"); *S0 = h->S0; return GRHIP_OK; } \
    int grhip_##NAME##_SK(grhip_##NAME *h, int *SK) { GRHIP_TR_NULL(h); if (!SK) return fail(GRHIP_EINVAL, "null argument"); *SK = h->SK; return GRHIP_OK; } \
    int grhip_##NAME##_trace_window(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->fast.TW; }                         \
    int grhip_##NAME##_resident_blocks(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->fast.max_groups * h->fast.G; }  \
    int grhip_##NAME##_blocks_per_wavefront(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->fast.G; }                  \
    int grhip_##NAME##_workspace_bytes(grhip_##NAME *h, unsigned long long *bytes)                                    \
    {                                                                                                                 \
        GRHIP_TR_NULL(h);                                                                                             \
        if (!bytes) return fail(GRHIP_EINVAL, "null argument");                                                       \
        *bytes = (unsigned long long)h->fast.max_groups * h->fast.ws_words * 8;                                       \
        return GRHIP_OK;                                                                                              \
    }                                                                                                                 \
    int grhip_##NAME##_dead_ends(grhip_##NAME *h, long long *count) { GRHIP_TR_NULL(h); return h->dead_ends(count); }

#define GRHIP_TR_VITERBI(NAME, TO)                                                                                    \
    int grhip_##NAME##_create(grhip_##NAME **h, const grhip_fsm *fsm, int K, int S0, int SK, int device)              \
    {                                                                                                                 \
        if (!h) return fail(GRHIP_EINVAL, "null argument");                                                           \
        return make_handle(h, [&](grhip_##NAME *b) { return b->init(fsm, K, S0, SK, TO, device); });                  \
    }                                                                                                                 \
    GRHIP_TR_BLOCK(NAME)                                                                                              \
    GRHIP_TR_DECODER_GETTERS(NAME)

GRHIP_TR_VITERBI(trellis_viterbi_b, TR_B)
GRHIP_TR_VITERBI(trellis_viterbi_s, TR_S)
GRHIP_TR_VITERBI(trellis_viterbi_i, TR_I)

#define GRHIP_TR_COMBINED(NAME, TI, TO)                                                                               \
    int grhip_##NAME##_create(grhip_##NAME **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE, int n_TABLE, \
                              int TYPE, int device)                                                                   \
    {                                                                                                                 \
        if (!h) return fail(GRHIP_EINVAL, "null argument");                                                           \
        return make_handle(h, [&](grhip_##NAME *b) { return b->init(fsm, K, S0, SK, D, TABLE, n_TABLE, TYPE, TI, TO, device); }); \
    }                                                                                                                 \
    GRHIP_TR_BLOCK(NAME)                                                                                              \
    int grhip_##NAME##_set_TABLE(grhip_##NAME *h, const void *TABLE, int n_TABLE) { GRHIP_TR_NULL(h); return h->set_TABLE(TABLE, n_TABLE); } \
    int grhip_##NAME##_set_engine(grhip_##NAME *h, int engine) { GRHIP_TR_NULL(h); return h->set_engine(engine); }    \
    int grhip_##NAME##_engine(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->engine(); }                              \
    int grhip_##NAME##_D(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->D; }                                          \
    int grhip_##NAME##_TYPE(grhip_##NAME *h) { GRHIP_TR_NULL(h); return h->type; }                                    \
    GRHIP_TR_DECODER_GETTERS(NAME)

GRHIP_TR_COMBINED(trellis_viterbi_combined_sb, TR_S, TR_B)
GRHIP_TR_COMBINED(trellis_viterbi_combined_ss, TR_S, TR_S)
GRHIP_TR_COMBINED(trellis_viterbi_combined_si, TR_S, TR_I)
GRHIP_TR_COMBINED(trellis_viterbi_combined_ib, TR_I, TR_B)
GRHIP_TR_COMBINED(trellis_viterbi_combined_is, TR_I, TR_S)
GRHIP_TR_COMBINED(trellis_viterbi_combined_ii, TR_I, TR_I)
GRHIP_TR_COMBINED(trellis_viterbi_combined_fb, TR_F, TR_B)
GRHIP_TR_COMBINED(trellis_viterbi_combined_fs, TR_F, TR_S)
GRHIP_TR_COMBINED(trellis_viterbi_combined_fi, TR_F, TR_I)
GRHIP_TR_COMBINED(trellis_viterbi_combined_cb, TR_C, TR_B)
GRHIP_TR_COMBINED(trellis_viterbi_combined_cs, TR_C, TR_S)
GRHIP_TR_COMBINED(trellis_viterbi_combined_ci, TR_C, TR_I)
#undef GRHIP_TR_COMBINED

#undef GRHIP_TR_VITERBI
#undef GRHIP_TR_DECODER_GETTERS
#undef GRHIP_TR_METRICS
#undef GRHIP_TR_METRICS_TAIL
#undef GRHIP_TR_ENCODER
#undef GRHIP_TR_BLOCK
#undef GRHIP_TR_NULL

}  // extern "C"
