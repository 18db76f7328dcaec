// capi_cpm.hip -- C ABI of the continuous-phase transmitter: gr_frequency_modulator_fc
// (general/gr_frequency_modulator_fc.cc:30-72, .h:42-52), gr_bytes_to_syms (general/gr_bytes_to_syms.cc:45-71),
// gr_char_to_float (general/gr_char_to_float.cc:42-53), gr_chunks_to_symbols_bf (gengen/gr_chunks_to_symbols_XX.cc.t:51-74),
// the designers of csrc/cpm.h, and the hier blocks digital_cpmmod_bc (gr-digital/lib/digital_cpmmod_bc.cc:44-72),
// digital_gmskmod_bc (gr-digital/lib/digital_gmskmod_bc.cc:41-45) and gmsk_mod (gr-digital/python/gmsk.py:55-120), each
// as one handle that takes new items only.
//
// All take S streams back to back.  The modulator's phase is one double per stream on the device; the hier handles
// also keep each stream's last nt - 1 symbols there (nt taps per filter of their interpolator).
#include <climits>
#include <cmath>
#include <vector>

#include "cpm.h"
#include "cpm_blocks.h"
#include "grhip_internal.h"
#include "resampler.h"
#include "stream_block.h"

using namespace grhip;

namespace {

// the tail of the entries that hand taps out: the count, and the floats where `out` is given and has room
int hand_out(const std::vector<float> &taps, float *out, size_t capacity)
{
    if (capacity && !out) return fail(GRHIP_EINVAL, "null argument");
    if (out && capacity < taps.size()) return fail(GRHIP_EINVAL, "%zu taps, room for %zu", taps.size(), capacity);
    if (out) std::copy(taps.begin(), taps.end(), out);
    return (int)taps.size();
}

// ---- frequency_modulator_fc --------------------------------------------------------------------------------------------
struct FreqModBlock : StreamBlock {
    double sens = 0.0;                  // d_sensitivity
    DevBuf d_phase, d_scratch;          // d_phase per stream; the scan's tile sums

    int init(double sensitivity, int dev)
    {
        sens = sensitivity;
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        return fill_state(d_phase, 0.0);                                                    // d_phase (0), .cc:40
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return fill_state(d_phase, 0.0); });
    }
    int set_sensitivity(float v)                                                            // .h:51: the float widens
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        sens = v;
        return GRHIP_OK;
    }
    float sensitivity()                                                                     // .h:52
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return (float)sens;
    }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        int rc = check_io(d_in, 4, d_out, 8);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart("frequency_modulator_fc", d_in, items * 4, d_out, items * 8))) return rc;
        if (!mode_fast(mode)) return fm_walk_launch((const float *)d_in, (float2 *)d_out, n, nstreams, sens, d_phase.as<double>(), st);
        if ((rc = d_scratch.reserve((size_t)nstreams * (size_t)fm_tiles(n) * sizeof(double)))) return rc;
        return fm_scan_launch((const float *)d_in, (float2 *)d_out, n, nstreams, sens, d_phase.as<double>(), d_scratch.as<double>(), st);
    }
    int work(int n, const void *in, void *out)
    {
        return host_work(n, 4, in, (size_t)n, 8, out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

// ---- bytes_to_syms and char_to_float ------------------------------------------------------------------------------------
struct ByteToFloatBlock : StreamBlock {
    bool bits = false;                  // bytes_to_syms: eight floats per byte

    const char *name() const { return bits ? "bytes_to_syms" : "char_to_float"; }
    int per() const { return bits ? 8 : 1; }
    int init(bool eight, int dev)
    {
        bits = eight;
        mode = default_mode();
        return init_device(dev);
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [] { return GRHIP_OK; });        // nothing kept per stream
    }
    int check_outputs(int n) const
    {
        return (long long)n * per() > INT_MAX ? fail(GRHIP_EINVAL, "%s: the outputs must fit an int", name()) : GRHIP_OK;
    }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        int rc = check_outputs(n);
        if (rc) return rc;
        if ((rc = check_io(d_in, 1, d_out, 4))) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart(name(), d_in, items, d_out, items * per() * 4))) return rc;
        // the block keeps no state, so the streams run as one
        if (bits) return bytes_to_syms_launch((const unsigned char *)d_in, 0, (float *)d_out, 0, (long long)items, 1, st);
        return char_to_float_launch((const unsigned char *)d_in, 0, (float *)d_out, 0, (long long)items, 1, st);
    }
    int work(int n, const void *in, void *out)
    {
        if (n > 0)
            if (int rc = check_outputs(n)) return rc;
        return host_work(n, 1, in, (size_t)n * per(), 4, out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

// ---- chunks_to_symbols_bf ------------------------------------------------------------------------------------------------
constexpr size_t C2S_BF_MAX_ENTRIES = 65536;

struct ChunksBfBlock : StreamBlock {
    DevBuf d_table;
    unsigned table_size = 0, D = 1;

    int init(const float *table, size_t n, int d, int dev)
    {
        if (n == 0) return fail(GRHIP_EINVAL, "chunks_to_symbols_bf: empty symbol table");
        if (!table) return fail(GRHIP_EINVAL, "null argument");
        if (n > C2S_BF_MAX_ENTRIES) return fail(GRHIP_EINVAL, "chunks_to_symbols_bf: at most %zu table entries", C2S_BF_MAX_ENTRIES);
        if (d < 1) return fail(GRHIP_EINVAL, "chunks_to_symbols_bf: D must be at least 1");
        table_size = (unsigned)n;
        D = (unsigned)d;
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        if ((rc = d_table.reserve(n * sizeof(float)))) return rc;
        GRHIP_HIP(hipMemcpy(d_table.p, table, n * sizeof(float), hipMemcpyHostToDevice));
        return GRHIP_OK;
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [] { return GRHIP_OK; });
    }
    int check_outputs(int n) const      // n * D is the reference's noutput_items, an int
    {
        return (long long)n * (long long)D > INT_MAX ? fail(GRHIP_EINVAL, "chunks_to_symbols_bf: n * D must fit an int") : GRHIP_OK;
    }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        int rc = check_outputs(n);
        if (rc) return rc;
        if ((rc = check_io(d_in, 1, d_out, 4))) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart("chunks_to_symbols_bf", d_in, items, d_out, items * D * sizeof(float)))) return rc;
        return chunks_to_symbols_bf_launch((const unsigned char *)d_in, (float *)d_out, (long long)items, d_table.as<float>(), table_size, D, st);
    }
    int work(int n, const void *in, void *out)
    {
        if (n > 0)
            if (int rc = check_outputs(n)) return rc;
        return host_work(n, 1, in, (size_t)n * D, sizeof(float), out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

// ---- cpmmod_bc, gmskmod_bc, gmsk_mod ---------------------------------------------------------------------------------------
// char_to_float (or bytes_to_syms) -> interp_fir_filter_fff(sps, taps) -> frequency_modulator_fc(sensitivity) on new
// items only.  A work call of the handle is a work call of every inner block: the modulator's end-of-call wrap falls
// where the handle's calls end.
//
// The phase integrates the frequency samples, so a rounding difference in one of them stays in every later output:
// both engines form them in gr_fir_fff_generic's order in every mode, and differ only in where the samples live.
struct CpmModBlock : StreamBlock {
    const char *label = "cpmmod_bc";
    bool bits = false;                  // gmsk_mod: bytes of eight symbols
    unsigned sps = 1, nt = 1;
    double sens = 0.0;
    std::vector<float> taps;
    bool fits = false;                  // engine 1 can run: cpm_fused_fits(sps, nt)
    int want = 1;
    int rs_nt = 1, rs_wp = 0;
    DevBuf d_rows, d_bank, d_hist, d_phase, d_sym, d_freq, d_scratch;

    size_t hist_bytes() const { return (size_t)nstreams * (nt - 1) * sizeof(float); }
    int restart()
    {
        int rc = fill_state(d_phase, 0.0);
        if (rc || nt == 1) return rc;
        if ((rc = d_hist.reserve(hist_bytes()))) return rc;
        return zero_device(d_hist.p, hist_bytes());                                         // the scheduler's history zeros
    }
    // taps, sps, sens, bits and label are set
    int init(int dev)
    {
        nt = cpm_taps_per_filter(taps.size(), sps);
        fits = cpm_fused_fits(sps, nt);
        RsConfig c;
        int rc = rs_config(RS_FFF, true, sps, 1, (int)nt, 0, &c);
        if (rc) return rc;
        mode = default_mode();
        if ((rc = init_device(dev)) || (rc = rs_prepare_device(RS_FFF))) return rc;
        std::vector<float> padded((size_t)nt * sps - taps.size(), 0.f);                     // gr_interp_fir_filter_XXX.cc.t:77-83
        padded.insert(padded.end(), taps.begin(), taps.end());
        const std::vector<float> bank = rs_bank(padded, 1, sps, 1, sps, &rs_nt, &rs_wp);
        const std::vector<float> rows = cpm_filter_rows(taps, sps);
        if ((rc = d_bank.reserve(bank.size() * sizeof(float))) || (rc = d_rows.reserve(rows.size() * sizeof(float)))) return rc;
        GRHIP_HIP(hipMemcpy(d_bank.p, bank.data(), bank.size() * sizeof(float), hipMemcpyHostToDevice));
        GRHIP_HIP(hipMemcpy(d_rows.p, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
        return restart();
    }
    int init_cpm(int type, float h, unsigned samples_per_sym, unsigned L, double beta, int dev)
    {
        if (!cpm_type_valid(type)) return fail(GRHIP_EINVAL, "%s: invalid CPM type %d", label, type);      // digital_cpmmod_bc.cc:64-65 throws
        if (!cpm_phase_response(type, samples_per_sym, L, beta, taps))
            return fail(GRHIP_EINVAL, "%s: samples_per_sym * L must be 1 .. %u and beta finite", label, CPM_MAX_TAPS);
        sps = samples_per_sym;
        sens = CPM_PI * h;                                                                  // M_PI * h with h a float, :51
        return init(dev);
    }
    int init_gmsk(int samples_per_symbol, double bt, int dev)
    {
        label = "gmsk_mod";
        bits = true;
        if (samples_per_symbol < 2 || !gmsk_mod_taps((unsigned)samples_per_symbol, bt, taps))              // gmsk.py:87-88 raises
            return fail(GRHIP_EINVAL, "gmsk_mod: samples_per_symbol must be an integer 2 .. %u and bt finite", GMSK_MAX_SPS);
        sps = (unsigned)samples_per_symbol;
        sens = (CPM_PI / 2) / samples_per_symbol;                                           // gmsk.py:91
        return init(dev);
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
    }
    int set_engine(int e)
    {
        if (e != 0 && e != 1) return fail(GRHIP_EINVAL, "%s: engine 0 or 1", label);
        if (e == 1 && !fits)
            return fail(GRHIP_EINVAL, "%s: engine 1 takes at most %u taps per filter and %u taps", label, CPM_FUSED_MAX_NT, CPM_FUSED_MAX_ROWS);
        std::lock_guard<std::mutex> lk(setter_mutex);
        want = e;
        return GRHIP_OK;
    }
    int running() const { return want == 1 && fits && mode_fast(mode); }     // under setter_mutex
    int get_engine()
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return running();
    }
    long long outputs(int n) const { return (long long)n * (bits ? 8 : 1) * sps; }
    int check_outputs(int n) const
    {
        return outputs(n) > INT_MAX ? fail(GRHIP_EINVAL, "%s: the outputs must fit an int", label) : GRHIP_OK;
    }

    // engine 0: the library's blocks in a row, history carried through the interpolator's input buffer
    int run_blocks(int n, const void *d_in, void *d_out, float *freq, hipStream_t st)
    {
        const long long nsym = (long long)n * (bits ? 8 : 1), nout = nsym * sps, row = nsym + nt - 1;
        const size_t S = (size_t)nstreams, hw = (nt - 1) * sizeof(float);
        int rc = d_sym.reserve(S * (size_t)row * sizeof(float));
        if (rc) return rc;
        if (!freq) {
            if ((rc = d_freq.reserve(S * (size_t)nout * sizeof(float)))) return rc;
            freq = d_freq.as<float>();
        }
        float *sym = d_sym.as<float>();
        if (hw) GRHIP_HIP(hipMemcpy2DAsync(sym, (size_t)row * sizeof(float), d_hist.p, hw, hw, S, hipMemcpyDeviceToDevice, st));
        rc = bits ? bytes_to_syms_launch((const unsigned char *)d_in, n, sym + nt - 1, row, n, nstreams, st)
                  : char_to_float_launch((const unsigned char *)d_in, n, sym + nt - 1, row, n, nstreams, st);
        if (rc) return rc;
        RsLaunch a;
        a.in = sym; a.in_stride = row; a.lead = 0; a.n_phys = row;
        a.out = freq; a.out_stride = nout; a.nout = nout; a.n_streams = nstreams;
        a.bank = d_bank.p;
        a.I = sps; a.D = 1; a.c0 = 0;
        a.P = (int)sps; a.Dp = 1; a.nt = rs_nt; a.WP = rs_wp; a.RS = rs_nt + 2 * rs_wp;
        if ((rc = rs_launch(RS_FFF, true, a, st))) return rc;
        rc = mode_fast(mode) ? fm_scan_launch(freq, (float2 *)d_out, nout, nstreams, sens, d_phase.as<double>(), d_scratch.as<double>(), st)
                             : fm_walk_launch(freq, (float2 *)d_out, nout, nstreams, sens, d_phase.as<double>(), st);
        if (rc) return rc;
        if (hw) GRHIP_HIP(hipMemcpy2DAsync(d_hist.p, hw, sym + nsym, (size_t)row * sizeof(float), hw, S, hipMemcpyDeviceToDevice, st));
        return GRHIP_OK;
    }

    // engine 1: the fused kernel behind its carry pre-pass, then the history
    int run_fused(int n, const void *d_in, void *d_out, float *freq, hipStream_t st)
    {
        const long long nsym = (long long)n * (bits ? 8 : 1);
        CpmFused a;
        a.in = (const unsigned char *)d_in; a.n_in = n; a.bits = bits;
        a.hist = d_hist.as<float>(); a.rows = d_rows.as<float>();
        a.sps = (int)sps; a.nt = (int)nt; a.freq = freq;
        if (int rc = cpm_fused_launch(a, (float2 *)d_out, nsym * sps, nstreams, sens, d_phase.as<double>(), d_scratch.as<double>(), st)) return rc;
        return cpm_history_launch(a, nsym, nstreams, st);
    }

    // n input items per stream (symbols; gmsk_mod: bytes); out [S][outputs(n)]; d_freq null or [S][outputs(n)] floats
    int work_device(int n, const void *d_in, void *d_out, void *d_freq_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        int rc = check_outputs(n);
        if (rc) return rc;
        if ((rc = check_io(d_in, 1, d_out, 8))) return rc;
        if (!aligned(d_freq_out, 4)) return fail(GRHIP_EINVAL, "items not naturally aligned");
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t in_bytes = (size_t)nstreams * (size_t)n, items = (size_t)nstreams * (size_t)outputs(n);
        if ((rc = check_apart(label, d_in, in_bytes, d_out, items * 8)) || (rc = check_apart(label, d_in, in_bytes, d_freq_out, items * 4))) return rc;
        if (overlap(d_out, items * 8, d_freq_out, items * 4)) return fail(GRHIP_EINVAL, "%s: the two outputs may not overlap", label);
        if ((rc = d_scratch.reserve((size_t)nstreams * (size_t)fm_tiles(outputs(n)) * sizeof(double)))) return rc;
        return running() ? run_fused(n, d_in, d_out, (float *)d_freq_out, st) : run_blocks(n, d_in, d_out, (float *)d_freq_out, st);
    }
    int work(int n, const void *in, void *out, void *freq_out)
    {
        if (n > 0)
            if (int rc = check_outputs(n)) return rc;
        const size_t items = (size_t)nstreams * (size_t)outputs(n > 0 ? n : 0);
        return host_work(n, 1, in, (size_t)outputs(n > 0 ? n : 0), 8, out, freq_out ? items * 4 : 0, [&](void *d_in, void *d_out, hipStream_t st) -> int {
            float *d_f = freq_out ? (float *)((char *)d_out + items * 8) : nullptr;
            int rc = work_device(n, d_in, d_out, d_f, st);
            if (rc || !d_f) return rc;
            GRHIP_D2H(this, freq_out, d_f, items * 4, st);
            return GRHIP_OK;
        });
    }
};

}  // namespace

struct grhip_frequency_modulator_fc : FreqModBlock {};
struct grhip_bytes_to_syms : ByteToFloatBlock {};
struct grhip_char_to_float : ByteToFloatBlock {};
struct grhip_chunks_to_symbols_bf : ChunksBfBlock {};
struct grhip_cpmmod_bc : CpmModBlock {};
struct grhip_gmskmod_bc : CpmModBlock {};
struct grhip_gmsk_mod : CpmModBlock {};

extern "C" {

#define GRHIP_CPM_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")
#define GRHIP_CPM_STREAM_BLOCK(NAME)                                                                                  \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { GRHIP_CPM_NULL(h); return h->set_mode(mode); }           \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams) { GRHIP_CPM_NULL(h); return h->set_streams(nstreams); }
#define GRHIP_CPM_WORK(NAME)                                                                                          \
    int grhip_##NAME##_work(grhip_##NAME *h, int n, const void *in, void *out) { GRHIP_CPM_NULL(h); return h->work(n, in, out); } \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n, const void *d_in, void *d_out, void *stream)               \
    {                                                                                                                 \
        GRHIP_CPM_NULL(h);                                                                                            \
        return h->work_device(n, d_in, d_out, stream);                                                                \
    }
#define GRHIP_CPM_HIER(NAME)                                                                                          \
    GRHIP_CPM_STREAM_BLOCK(NAME)                                                                                      \
    int grhip_##NAME##_set_engine(grhip_##NAME *h, int engine) { GRHIP_CPM_NULL(h); return h->set_engine(engine); }   \
    int grhip_##NAME##_engine(grhip_##NAME *h) { GRHIP_CPM_NULL(h); return h->get_engine(); }                         \
    int grhip_##NAME##_samples_per_symbol(grhip_##NAME *h) { GRHIP_CPM_NULL(h); return (int)h->sps; }                 \
    int grhip_##NAME##_filter_taps(grhip_##NAME *h, float *taps, size_t capacity) { GRHIP_CPM_NULL(h); return hand_out(h->taps, taps, capacity); } \
    int grhip_##NAME##_phase(grhip_##NAME *h, int stream, double *phase)                                              \
    {                                                                                                                 \
        GRHIP_CPM_NULL(h);                                                                                            \
        if (!phase) return fail(GRHIP_EINVAL, "null argument");                                                       \
        return h->read_state(h->d_phase, stream, phase);                                                              \
    }                                                                                                                 \
    int grhip_##NAME##_work(grhip_##NAME *h, int n, const void *in, void *out, void *freq_out)                        \
    {                                                                                                                 \
        GRHIP_CPM_NULL(h);                                                                                            \
        return h->work(n, in, out, freq_out);                                                                         \
    }                                                                                                                 \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n, const void *d_in, void *d_out, void *d_freq_out, void *stream) \
    {                                                                                                                 \
        GRHIP_CPM_NULL(h);                                                                                            \
        return h->work_device(n, d_in, d_out, d_freq_out, stream);                                                    \
    }

// ---- the designers: host arithmetic, no device ---------------------------------------------------------------------------
int grhip_cpm_phase_response(int type, unsigned samples_per_sym, unsigned L, double beta, float *taps, size_t capacity)
{
    std::vector<float> t;
    if (!cpm_phase_response(type, samples_per_sym, L, beta, t))
        return fail(GRHIP_EINVAL, "cpm_phase_response: samples_per_sym * L must be 1 .. %u and beta finite", CPM_MAX_TAPS);
    return hand_out(t, taps, capacity);
}

int grhip_firdes_gaussian(double gain, double spb, double bt, int ntaps, float *taps, size_t capacity)
{
    std::vector<float> t;
    if (!firdes_gaussian(gain, spb, bt, ntaps, t))
        return fail(GRHIP_EINVAL, "firdes_gaussian: ntaps must be 1 .. %u and gain, spb and bt finite", CPM_MAX_TAPS);
    return hand_out(t, taps, capacity);
}

int grhip_gmsk_mod_taps(int samples_per_symbol, double bt, float *taps, size_t capacity)
{
    std::vector<float> t;
    if (samples_per_symbol < 2 || !gmsk_mod_taps((unsigned)samples_per_symbol, bt, t))
        return fail(GRHIP_EINVAL, "gmsk_mod_taps: samples_per_symbol must be 2 .. %u and bt finite", GMSK_MAX_SPS);
    return hand_out(t, taps, capacity);
}

// ---- frequency_modulator_fc --------------------------------------------------------------------------------------------
int grhip_frequency_modulator_fc_tile(void) { return FM_TILE; }

int grhip_frequency_modulator_fc_create(grhip_frequency_modulator_fc **h, double sensitivity, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_frequency_modulator_fc *b) { return b->init(sensitivity, device); });
}
GRHIP_CPM_STREAM_BLOCK(frequency_modulator_fc)
GRHIP_CPM_WORK(frequency_modulator_fc)
int grhip_frequency_modulator_fc_set_sensitivity(grhip_frequency_modulator_fc *h, float sensitivity)
{
    GRHIP_CPM_NULL(h);
    return h->set_sensitivity(sensitivity);
}
float grhip_frequency_modulator_fc_sensitivity(grhip_frequency_modulator_fc *h)
{
    if (!h) return (float)fail(GRHIP_EINVAL, "null handle");
    return h->sensitivity();
}
int grhip_frequency_modulator_fc_phase(grhip_frequency_modulator_fc *h, int stream, double *phase)
{
    GRHIP_CPM_NULL(h);
    if (!phase) return fail(GRHIP_EINVAL, "null argument");
    return h->read_state(h->d_phase, stream, phase);
}
int grhip_frequency_modulator_fc_set_phase(grhip_frequency_modulator_fc *h, double phase)
{
    GRHIP_CPM_NULL(h);
    return h->edit_states<double>(h->d_phase, [&](double &p) { p = phase; });
}

// ---- the small blocks -----------------------------------------------------------------------------------------------------
int grhip_bytes_to_syms_create(grhip_bytes_to_syms **h, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_bytes_to_syms *b) { return b->init(true, device); });
}
GRHIP_CPM_STREAM_BLOCK(bytes_to_syms)
GRHIP_CPM_WORK(bytes_to_syms)

int grhip_char_to_float_create(grhip_char_to_float **h, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_char_to_float *b) { return b->init(false, device); });
}
GRHIP_CPM_STREAM_BLOCK(char_to_float)
GRHIP_CPM_WORK(char_to_float)

int grhip_chunks_to_symbols_bf_create(grhip_chunks_to_symbols_bf **h, const float *symbol_table, size_t nsymbols, int D, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_chunks_to_symbols_bf *b) { return b->init(symbol_table, nsymbols, D, device); });
}
GRHIP_CPM_STREAM_BLOCK(chunks_to_symbols_bf)
GRHIP_CPM_WORK(chunks_to_symbols_bf)
int grhip_chunks_to_symbols_bf_D(grhip_chunks_to_symbols_bf *h) { GRHIP_CPM_NULL(h); return (int)h->D; }

// ---- the hier blocks --------------------------------------------------------------------------------------------------------
int grhip_cpmmod_bc_tile(void) { return FM_TILE; }

int grhip_cpmmod_bc_create(grhip_cpmmod_bc **h, int type, float h_index, unsigned samples_per_sym, unsigned L, double beta, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_cpmmod_bc *b) { return b->init_cpm(type, h_index, samples_per_sym, L, beta, device); });
}
GRHIP_CPM_HIER(cpmmod_bc)

int grhip_gmskmod_bc_create(grhip_gmskmod_bc **h, unsigned samples_per_sym, double bt, unsigned L, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_gmskmod_bc *b) {                                       // digital_gmskmod_bc.cc:43
        b->label = "gmskmod_bc";
        return b->init_cpm(CPM_GAUSSIAN, 0.5f, samples_per_sym, L, bt, device);
    });
}
GRHIP_CPM_HIER(gmskmod_bc)

int grhip_gmsk_mod_create(grhip_gmsk_mod **h, int samples_per_symbol, double bt, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_gmsk_mod *b) { return b->init_gmsk(samples_per_symbol, bt, device); });
}
GRHIP_CPM_HIER(gmsk_mod)

#undef GRHIP_CPM_HIER
#undef GRHIP_CPM_WORK
#undef GRHIP_CPM_STREAM_BLOCK
#undef GRHIP_CPM_NULL

}  // extern "C"
