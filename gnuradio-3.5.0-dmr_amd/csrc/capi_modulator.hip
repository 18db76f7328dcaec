// capi_modulator.hip -- C ABI of the blocks in front of the pulse shaper of gr-digital/python/generic_mod_demod.py:114-150:
// gr_packed_to_unpacked_bb (gengen/gr_packed_to_unpacked_XX.cc.t:58-137), gr_unpacked_to_packed_bb
// (gengen/gr_unpacked_to_packed_XX.cc.t:56-129), gr_diff_encoder_bb (general/gr_diff_encoder_bb.cc:44-62) and
// gr_chunks_to_symbols_bc (gengen/gr_chunks_to_symbols_XX.cc.t:51-74), and of generic_mod, the hier block that chains
// them into pfb_arb_resampler_ccf (:76-157), as one handle.
//
// The blocks take S streams back to back as diff_decoder_bb and map_bb do (csrc/capi_constellation.hip).  What a call
// of the two repackers needs, consumes and carries does not depend on the data: csrc/modulator_plan.h works it out on
// the host, and the handle keeps the bit index, one value for all streams as in the reference.  The encoder's last_out
// is per stream and lives on the device.
#include <climits>
#include <cmath>
#include <vector>

#include "arb_resampler.h"
#include "constellation_blocks.h"
#include "fll_taps.h"
#include "grhip_internal.h"
#include "modulator.h"
#include "stream_block.h"

using namespace grhip;

namespace {

// ---- packed_to_unpacked_bb and unpacked_to_packed_bb -------------------------------------------------------------------
struct PackBlock : StreamBlock {
    bool unpack = true;         // packed_to_unpacked; false: unpacked_to_packed
    unsigned k = 1;
    bool lsb_first = false;
    unsigned index = 0;         // d_index

    const char *name() const { return unpack ? "packed_to_unpacked_bb" : "unpacked_to_packed_bb"; }
    PackPlan plan(long long noutput) const { return unpack ? p2u_plan(index, noutput, k) : u2p_plan(index, noutput, k); }

    int init(bool unpacking, unsigned bits_per_chunk, int endianness, int dev)
    {
        unpack = unpacking;
        if (!pack_k_ok(bits_per_chunk))                                      // the reference asserts (.cc.t:52-53)
            return fail(GRHIP_EINVAL, "%s: bits_per_chunk must be 1 .. 8", name());
        if (endianness != GRHIP_MSB_FIRST && endianness != GRHIP_LSB_FIRST)  // assert(0) in general_work
            return fail(GRHIP_EINVAL, "%s: endianness must be GRHIP_MSB_FIRST or GRHIP_LSB_FIRST", name());
        k = bits_per_chunk;
        lsb_first = endianness == GRHIP_LSB_FIRST;
        mode = default_mode();
        return init_device(dev);
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { index = 0; return GRHIP_OK; });
    }
    int forecast(int noutput)
    {
        if (noutput < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
        std::lock_guard<std::mutex> lk(setter_mutex);
        const PackPlan p = plan(noutput);
        if (!p.ok || p.needed > INT_MAX) return fail(GRHIP_EINVAL, "%s: the call's bit addresses pass 2^32 or its input an int", name());
        return (int)p.needed;
    }
    int general_work_device(int noutput, int ninput, const void *d_in, void *d_out, int *consumed, void *stream)
    {
        if (!consumed) return fail(GRHIP_EINVAL, "null consumed");
        *consumed = 0;
        if (noutput < 0 || ninput < 0) return fail(GRHIP_EINVAL, "negative item count");
        if (noutput == 0) return 0;                                          // d_index >> 3 (or / k) is 0: nothing consumed
        int rc = check_io(d_in, 1, d_out, 1);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const PackPlan p = plan(noutput);
        if (!p.ok) return fail(GRHIP_EINVAL, "%s: the call's bit addresses pass 2^32", name());
        if (ninput < p.needed)                                               // the reference only asserts (.cc.t:129)
            return fail(GRHIP_EINVAL, "%s: %d input items, forecast asks for %lld", name(), ninput, p.needed);
        if ((rc = check_apart(name(), d_in, (size_t)nstreams * (size_t)ninput, d_out, (size_t)nstreams * (size_t)noutput))) return rc;
        rc = unpack ? packed_to_unpacked_launch((const unsigned char *)d_in, ninput, (unsigned char *)d_out, noutput, nstreams, k, lsb_first, index, st)
                    : unpacked_to_packed_launch((const unsigned char *)d_in, ninput, (unsigned char *)d_out, noutput, nstreams, k, lsb_first, index, st);
        if (rc) return rc;
        index = p.index_after;
        *consumed = (int)p.consumed;
        return noutput;
    }
    int general_work(int noutput, int ninput, const void *in, void *out, int *consumed)
    {
        if (!consumed) return fail(GRHIP_EINVAL, "null consumed");
        *consumed = 0;
        if (noutput < 0 || ninput < 0) return fail(GRHIP_EINVAL, "negative item count");
        if (noutput == 0) return 0;
        if (ninput == 0) return fail(GRHIP_EINVAL, "%s: no input items, forecast asks for some", name());
        int produced = 0;
        const int rc = host_work(ninput, 1, in, (size_t)noutput, 1, out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            produced = general_work_device(noutput, ninput, d_in, d_out, consumed, st);
            return produced < 0 ? produced : GRHIP_OK;
        });
        return rc ? rc : produced;
    }
};

// ---- diff_encoder_bb ---------------------------------------------------------------------------------------------------
struct DiffEncBlock : StreamBlock {
    unsigned modulus = 1;
    DevBuf d_last, d_scratch;   // last_out per stream; the scan's tile sums / carries

    int reset_last()
    {
        int rc = d_last.reserve((size_t)nstreams * sizeof(unsigned));
        if (rc) return rc;
        return zero_device(d_last.p, (size_t)nstreams * sizeof(unsigned));                // d_last_out(0), .cc:40
    }
    int init(unsigned m, int dev)
    {
        if (m == 0) return fail(GRHIP_EINVAL, "diff_encoder_bb: the modulus must not be 0");   // the reference divides by it
        modulus = m;
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        return reset_last();
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return reset_last(); });
    }
    // Moduli up to 256 and above 510 run as a scan (tile sums, a carry pass, the tiles again); 257 .. 510 walk
    // serially, one lane per stream, because the byte store between two steps breaks the sum's associativity
    // (modulator_plan.h).  The bytes are the serial loop's either way.
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
        if ((rc = check_apart("diff_encoder_bb", d_in, items, d_out, items))) return rc;
        if (diff_scan_modulus(modulus) && (rc = d_scratch.reserve((size_t)nstreams * (size_t)diff_tiles(n) * sizeof(unsigned)))) return rc;
        return diff_encoder_launch((const unsigned char *)d_in, (unsigned char *)d_out, n, nstreams, modulus, d_last.as<unsigned>(),
                                   d_scratch.as<unsigned>(), st);
    }
    int work(int n, const void *in, void *out)
    {
        return host_work(n, 1, in, (size_t)n, 1, out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

// ---- chunks_to_symbols_bc ----------------------------------------------------------------------------------------------
struct ChunksBlock : StreamBlock {
    DevBuf d_table;
    unsigned table_size = 0, D = 1;

    int init(const float *table_re_im, size_t n, int d, int dev)
    {
        if (n == 0) return fail(GRHIP_EINVAL, "chunks_to_symbols_bc: empty symbol table");
        if (!table_re_im) return fail(GRHIP_EINVAL, "null argument");
        if (n > (size_t)C2S_MAX_ENTRIES) return fail(GRHIP_EINVAL, "chunks_to_symbols_bc: at most %d table entries", C2S_MAX_ENTRIES);
        if (d < 1) return fail(GRHIP_EINVAL, "chunks_to_symbols_bc: D must be at least 1");
        table_size = (unsigned)n;
        D = (unsigned)d;
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        if ((rc = d_table.reserve(n * sizeof(float2)))) return rc;
        GRHIP_HIP(hipMemcpy(d_table.p, table_re_im, n * sizeof(float2), hipMemcpyHostToDevice));
        return GRHIP_OK;
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [] { return GRHIP_OK; });        // nothing kept per stream
    }
    int check_outputs(int n) const      // n * D is the reference's noutput_items, an int
    {
        return (long long)n * (long long)D > INT_MAX ? fail(GRHIP_EINVAL, "chunks_to_symbols_bc: n * D must fit an int") : GRHIP_OK;
    }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        int rc = check_outputs(n);
        if (rc) return rc;
        if ((rc = check_io(d_in, 1, d_out, 8))) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart("chunks_to_symbols_bc", d_in, items, d_out, items * D * sizeof(float2)))) return rc;
        return chunks_to_symbols_launch((const unsigned char *)d_in, 0, (float2 *)d_out, 0, (long long)items, 1, d_table.as<float2>(), table_size, D, st);
    }
    int work(int n, const void *in, void *out)
    {
        if (n > 0)
            if (int rc = check_outputs(n)) return rc;
        return host_work(n, 1, in, (size_t)n * D, sizeof(float2), out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

// ---- generic_mod ---------------------------------------------------------------------------------------------------------
// gr-digital/python/generic_mod_demod.py:114-150 as one handle that takes new bytes only.  The constellation is asked
// for pre_diff_code() but not for apply_pre_diff_code() (:123-124): an empty code is the identity, and
// constellation_qpsk's code is applied here although generic_demod skips it (:305-307).  That asymmetry is the
// reference's.
struct GenericModBlock : StreamBlock {
    Constellation c;
    unsigned k = 1, npoints = 0;
    bool differential = false, use_map = false;
    double sps = 2.0;                       // the rate of the resampler is (float)sps
    int engine = 1;
    std::vector<float> taps;                // the root raised cosine (:134-139)
    unsigned tpf = 0, S = 0;
    ArbRate rp;
    // between calls: for all streams the unread bits of the last byte and the resampler's (count overshoot, j, acc);
    // per stream, on the device, the last byte, the encoder's last_out and the last tpf symbols
    unsigned pending = 0;
    ArbState st;
    DevBuf d_taps, d_points, d_map, d_carry_byte, d_last, d_hist, d_carries;
    DevBuf d_staged, d_a, d_b, d_sym, d_scratch;        // engine 0's buffers between its blocks

    int restart()
    {
        pending = 0;
        st = ArbState();
        int rc;
        if ((rc = d_carry_byte.reserve((size_t)nstreams)) || (rc = d_last.reserve((size_t)nstreams * sizeof(unsigned))) ||
            (rc = d_hist.reserve((size_t)nstreams * tpf * sizeof(float2))))
            return rc;
        if ((rc = zero_device(d_carry_byte.p, (size_t)nstreams)) || (rc = zero_device(d_last.p, (size_t)nstreams * sizeof(unsigned)))) return rc;
        return zero_device(d_hist.p, (size_t)nstreams * tpf * sizeof(float2));      // the scheduler's history zeros
    }

    int init(const grhip_constellation *cons, double samples_per_symbol, int diff, double excess_bw, int gray_coded, int dev)
    {
        if (!cons) return fail(GRHIP_EINVAL, "null constellation");
        c = cons->c;
        if (!std::isfinite(samples_per_symbol) || samples_per_symbol < (double)MOD_MIN_SPS)      // :114-115 raises
            return fail(GRHIP_EINVAL, "generic_mod: sbp must be >= 2, is %f", samples_per_symbol);
        if ((int)samples_per_symbol > MOD_MAX_INT_SPS)
            return fail(GRHIP_EINVAL, "generic_mod: samples_per_symbol must be below %d (the resampler keeps 32 * (11 * int(sps) + 1) tap pairs in LDS)",
                        MOD_MAX_INT_SPS + 1);
        if (c.dim != 1) return fail(GRHIP_EINVAL, "generic_mod: a constellation of dimensionality 1 (chunks_to_symbols_bc runs with D = 1)");
        if (c.arity < 2) return fail(GRHIP_EINVAL, "generic_mod: a constellation of fewer than 2 points has no bits");
        k = c.bits_per_symbol();
        if (k < 1 || k > 8) return fail(GRHIP_EINVAL, "generic_mod: 1 .. 8 bits per symbol");
        npoints = (unsigned)c.points.size();
        differential = diff != 0;
        use_map = gray_coded && !c.pre_diff.empty();
        sps = samples_per_symbol;
        if (const char *bad = rrc_design((double)MOD_NFILTS, (double)MOD_NFILTS, 1.0, excess_bw, mod_ntaps(sps), taps))
            return fail(GRHIP_EINVAL, "generic_mod: %s", bad);
        for (float t : taps)
            if (!std::isfinite(t)) return fail(GRHIP_EINVAL, "generic_mod: excess_bw %g leaves no finite taps", excess_bw);
        tpf = (unsigned)((taps.size() + MOD_NFILTS - 1) / MOD_NFILTS);
        S = tpf | 1u;
        if ((unsigned long long)MOD_NFILTS * S > (unsigned long long)ARB_MAX_TAP_PAIRS || tpf > 127)
            return fail(GRHIP_EINVAL, "generic_mod: too many taps per filter");
        if (const char *bad = arb_rate_params(MOD_NFILTS, (float)sps, &rp)) return fail(GRHIP_EINVAL, "%s", bad);
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        const std::vector<float> pairs = arb_tap_pairs(taps.data(), taps.size(), MOD_NFILTS, tpf, S);
        if ((rc = d_taps.reserve(pairs.size() * 4)) || (rc = d_points.reserve((size_t)npoints * sizeof(float2))) || (rc = d_map.reserve(256)))
            return rc;
        GRHIP_HIP(hipMemcpy(d_taps.p, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));
        GRHIP_HIP(hipMemcpy(d_points.p, c.points.data(), (size_t)npoints * sizeof(float2), hipMemcpyHostToDevice));
        unsigned char t[256];
        for (int i = 0; i < 256; ++i) t[i] = (unsigned char)i;                          // gr_map_bb.cc:41-46
        for (size_t i = 0; i < c.pre_diff.size() && i < 256; ++i) t[i] = (unsigned char)c.pre_diff[i];
        GRHIP_HIP(hipMemcpy(d_map.p, t, 256, hipMemcpyHostToDevice));
        return restart();
    }
    int set_streams(int n)
    {
        return StreamBlock::set_streams(n, [&] { return restart(); });
    }
    int set_engine(int e)
    {
        if (e != 0 && e != 1) return fail(GRHIP_EINVAL, "generic_mod: engine 0 or 1");
        std::lock_guard<std::mutex> lk(setter_mutex);
        engine = e;
        return GRHIP_OK;
    }
    int get_engine()
    {
        std::lock_guard<std::mutex> lk(setter_mutex);
        return engine;
    }

    // what the next call of n_bytes does, under setter_mutex
    int plan_call(long long n_bytes, ModCall *mc, ArbPlan *p) const
    {
        *mc = mod_call(pending, n_bytes, k);
        *p = mod_outputs(st, rp, mc->nsym);
        if (p->too_many) return fail(GRHIP_EINVAL, "generic_mod: too many outputs for one call");
        // sps <= 32: the schedule is the closed form; sps >= 2: an output never passes a whole symbol, so a call ends
        // exactly at its last symbol and every symbol brings outputs
        if (!p->closed || st.count != 0 || (mc->nsym > 0 && p->n == 0)) return fail(GRHIP_ERUNTIME, "generic_mod: schedule off its closed form");
        return GRHIP_OK;
    }
    long long max_produced(int n_bytes)
    {
        if (n_bytes < 0) return fail(GRHIP_EINVAL, "negative item count");
        std::lock_guard<std::mutex> lk(setter_mutex);
        ModCall mc;
        ArbPlan p;
        if (int rc = plan_call(n_bytes, &mc, &p)) return rc;
        return p.n;
    }

    // engine 0: the library's own five blocks in a row
    int run_blocks(const ModCall &mc, ArbPlan &p, long long n_bytes, const void *d_in, void *d_out, long long out_stride, hipStream_t s)
    {
        const size_t ns = (size_t)nstreams, nsym = (size_t)mc.nsym;
        const long long row = (long long)tpf + mc.nsym;
        int rc;
        if ((rc = d_staged.reserve(ns * ((size_t)n_bytes + 1))) || (rc = d_a.reserve(ns * nsym)) || (rc = d_b.reserve(ns * nsym)) ||
            (rc = d_scratch.reserve(ns * (size_t)diff_tiles(mc.nsym) * sizeof(unsigned))) || (rc = d_sym.reserve(ns * (size_t)row * sizeof(float2))))
            return rc;
        unsigned char *cur = d_a.as<unsigned char>();
        if ((rc = mod_stage_bytes_launch((const unsigned char *)d_in, n_bytes, nstreams, d_carry_byte.as<unsigned char>(), d_staged.as<unsigned char>(), s)))
            return rc;
        if ((rc = packed_to_unpacked_launch(d_staged.as<unsigned char>(), n_bytes + 1, cur, mc.nsym, nstreams, k, false, mc.base, s))) return rc;
        if (use_map && (rc = map_launch(cur, cur, (long long)(ns * nsym), d_map.as<unsigned char>(), s))) return rc;
        if (differential) {
            if ((rc = diff_encoder_launch(cur, d_b.as<unsigned char>(), mc.nsym, nstreams, 1u << k, d_last.as<unsigned>(), d_scratch.as<unsigned>(), s)))
                return rc;
            cur = d_b.as<unsigned char>();
        }
        float2 *sym = d_sym.as<float2>();
        if ((rc = mod_copy_items_launch(d_hist.as<float2>(), tpf, sym, row, (int)tpf, nstreams, s))) return rc;
        if ((rc = chunks_to_symbols_launch(cur, mc.nsym, sym + tpf, row, mc.nsym, nstreams, d_points.as<float2>(), npoints, 1, s))) return rc;
        ArbLaunch a;
        a.in = sym; a.in_stride = row; a.lead = 0; a.n_phys = row;
        a.out = d_out; a.out_stride = out_stride; a.nout = p.n; a.n_streams = nstreams;
        a.taps = d_taps.as<float2>(); a.R = (int)MOD_NFILTS; a.tpf = (int)tpf; a.S = (int)S;
        a.tile = arb_closed_tile(MOD_NFILTS, p.D, tpf, ARB_SPAN_BYTES / (int)sizeof(float2), ARB_MAX_TILE, &a.span_cap);
        a.sc = p.sc;
        if ((rc = arb_resampler_launch(true, !mode_fast(mode), a, s))) return rc;
        return mod_copy_items_launch(sym + mc.nsym, row, d_hist.as<float2>(), tpf, (int)tpf, nstreams, s);
    }

    // engine 1: the fused kernel behind its carry pre-pass
    int run_fused(const ModCall &mc, ArbPlan &p, long long n_bytes, const void *d_in, void *d_out, long long out_stride, hipStream_t s)
    {
        ModLaunch a;
        a.in = (const unsigned char *)d_in; a.n_bytes = n_bytes; a.nsym = mc.nsym; a.base = mc.base; a.k = k;
        a.carry_byte = d_carry_byte.as<unsigned char>();
        a.map = use_map ? d_map.as<unsigned char>() : nullptr;
        a.differential = differential; a.mask = (1u << k) - 1u;
        a.last_out = d_last.as<unsigned>();
        a.points = d_points.as<float2>(); a.npoints = npoints;
        a.hist = d_hist.as<float2>();
        a.out = (float2 *)d_out; a.out_stride = out_stride; a.nout = p.n; a.n_streams = nstreams;
        a.taps = d_taps.as<float2>(); a.R = (int)MOD_NFILTS; a.tpf = (int)tpf; a.S = (int)S;
        a.tile = arb_closed_tile(MOD_NFILTS, p.D, tpf, MOD_SPAN_ITEMS, MOD_MAX_TILE, &a.span_cap);
        a.ntiles = (p.n + a.tile - 1) / a.tile;
        a.sc = p.sc;
        if (int rc = d_carries.reserve((size_t)nstreams * (size_t)a.ntiles * sizeof(unsigned))) return rc;
        a.carries = d_carries.as<unsigned>();
        return modulator_fused_launch(!mode_fast(mode), a, s);
    }

    int work_device(int n_bytes, const void *d_in, void *d_out, long long out_stride, long long out_capacity, long long *produced, void *stream)
    {
        if (!produced) return fail(GRHIP_EINVAL, "null produced");
        *produced = 0;
        const int go = check_count(n_bytes);
        if (go <= 0) return go;
        if (out_capacity < 0 || out_stride < 0) return fail(GRHIP_EINVAL, "negative capacity or stride");
        int rc = bind();
        if (rc) return rc;
        hipStream_t s = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        ModCall mc;
        ArbPlan p;
        if ((rc = plan_call(n_bytes, &mc, &p))) return rc;
        if (out_capacity < p.n)             // before anything is written or carried
            return fail(GRHIP_EINVAL, "generic_mod: the call produces %lld items per stream, out_capacity is %lld", p.n, out_capacity);
        if (nstreams > 1 && out_stride < p.n) return fail(GRHIP_EINVAL, "generic_mod: out_stride_items shorter than the %lld items produced", p.n);
        if ((rc = check_io(d_in, 1, d_out, 8))) return rc;
        const size_t out_items = (size_t)(nstreams - 1) * (size_t)out_stride + (size_t)p.n;
        if ((rc = check_apart("generic_mod", d_in, (size_t)nstreams * (size_t)n_bytes, d_out, out_items * sizeof(float2)))) return rc;
        rc = engine == 1 ? run_fused(mc, p, n_bytes, d_in, d_out, out_stride, s) : run_blocks(mc, p, n_bytes, d_in, d_out, out_stride, s);
        if (rc) return rc;
        pending = mc.pending_after;
        st = mod_next_state(p, mc.nsym);
        *produced = p.n;
        return GRHIP_OK;
    }

    // host buffers: in [S][n_bytes], out [S][*produced] back to back, room for S * out_capacity items
    int work(int n_bytes, const void *in, void *out, long long out_capacity, long long *produced)
    {
        if (!produced) return fail(GRHIP_EINVAL, "null produced");
        *produced = 0;
        const int go = check_count(n_bytes);
        if (go <= 0) return go;
        const long long q = max_produced(n_bytes);
        if (q < 0) return (int)q;
        if (out_capacity < q) return fail(GRHIP_EINVAL, "generic_mod: the call produces %lld items per stream, out_capacity is %lld", q, out_capacity);
        return host_work(n_bytes, 1, in, (size_t)q, sizeof(float2), out, 0, [&](void *d_in, void *d_out, hipStream_t s) {
            const int rc = work_device(n_bytes, d_in, d_out, q, q, produced, s);
            if (!rc && *produced != q) return fail(GRHIP_ERUNTIME, "generic_mod: the handle was reset during work");
            return rc;
        });
    }
};

}  // namespace

struct grhip_generic_mod : GenericModBlock {};
struct grhip_packed_to_unpacked_bb : PackBlock {};
struct grhip_unpacked_to_packed_bb : PackBlock {};
struct grhip_diff_encoder_bb : DiffEncBlock {};
struct grhip_chunks_to_symbols_bc : ChunksBlock {};

extern "C" {

#define GRHIP_MD_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")
#define GRHIP_MD_STREAM_BLOCK(NAME)                                                                                   \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { GRHIP_MD_NULL(h); return h->set_mode(mode); }            \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams) { GRHIP_MD_NULL(h); return h->set_streams(nstreams); }
#define GRHIP_MD_WORK(NAME)                                                                                           \
    int grhip_##NAME##_work(grhip_##NAME *h, int n, const void *in, void *out) { GRHIP_MD_NULL(h); return h->work(n, in, out); } \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n, const void *d_in, void *d_out, void *stream)               \
    {                                                                                                                 \
        GRHIP_MD_NULL(h);                                                                                             \
        return h->work_device(n, d_in, d_out, stream);                                                                \
    }
#define GRHIP_MD_PACK(NAME, UNPACK)                                                                                   \
    int grhip_##NAME##_create(grhip_##NAME **h, unsigned bits_per_chunk, int endianness, int device)                  \
    {                                                                                                                 \
        if (!h) return fail(GRHIP_EINVAL, "null argument");                                                           \
        return make_handle(h, [&](grhip_##NAME *b) { return b->init(UNPACK, bits_per_chunk, endianness, device); });  \
    }                                                                                                                 \
    GRHIP_MD_STREAM_BLOCK(NAME)                                                                                       \
    int grhip_##NAME##_forecast(grhip_##NAME *h, int noutput_items) { GRHIP_MD_NULL(h); return h->forecast(noutput_items); } \
    int grhip_##NAME##_general_work(grhip_##NAME *h, int noutput_items, int ninput_items, const void *in, void *out,  \
                                    int *consumed)                                                                    \
    {                                                                                                                 \
        GRHIP_MD_NULL(h);                                                                                             \
        return h->general_work(noutput_items, ninput_items, in, out, consumed);                                       \
    }                                                                                                                 \
    int grhip_##NAME##_general_work_device(grhip_##NAME *h, int noutput_items, int ninput_items, const void *d_in,    \
                                           void *d_out, int *consumed, void *stream)                                  \
    {                                                                                                                 \
        GRHIP_MD_NULL(h);                                                                                             \
        return h->general_work_device(noutput_items, ninput_items, d_in, d_out, consumed, stream);                    \
    }

GRHIP_MD_PACK(packed_to_unpacked_bb, true)
GRHIP_MD_PACK(unpacked_to_packed_bb, false)

int grhip_diff_encoder_bb_create(grhip_diff_encoder_bb **h, unsigned modulus, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_diff_encoder_bb *b) { return b->init(modulus, device); });
}
GRHIP_MD_STREAM_BLOCK(diff_encoder_bb)
GRHIP_MD_WORK(diff_encoder_bb)

int grhip_chunks_to_symbols_bc_create(grhip_chunks_to_symbols_bc **h, const float *symbol_table_re_im, size_t nsymbols, int D, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_chunks_to_symbols_bc *b) { return b->init(symbol_table_re_im, nsymbols, D, device); });
}
GRHIP_MD_STREAM_BLOCK(chunks_to_symbols_bc)
GRHIP_MD_WORK(chunks_to_symbols_bc)
int grhip_chunks_to_symbols_bc_D(grhip_chunks_to_symbols_bc *h) { GRHIP_MD_NULL(h); return (int)h->D; }

int grhip_generic_mod_create(grhip_generic_mod **h, const grhip_constellation *constellation, double samples_per_symbol, int differential,
                             double excess_bw, int gray_coded, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_generic_mod *b) { return b->init(constellation, samples_per_symbol, differential, excess_bw, gray_coded, device); });
}
GRHIP_MD_STREAM_BLOCK(generic_mod)
int grhip_generic_mod_set_engine(grhip_generic_mod *h, int engine) { GRHIP_MD_NULL(h); return h->set_engine(engine); }
int grhip_generic_mod_engine(grhip_generic_mod *h) { GRHIP_MD_NULL(h); return h->get_engine(); }
int grhip_generic_mod_bits_per_symbol(grhip_generic_mod *h) { GRHIP_MD_NULL(h); return (int)h->k; }
double grhip_generic_mod_samples_per_symbol(grhip_generic_mod *h)
{
    if (!h) return (double)fail(GRHIP_EINVAL, "null handle");
    return h->sps;
}
int grhip_generic_mod_ntaps(grhip_generic_mod *h) { GRHIP_MD_NULL(h); return (int)h->taps.size(); }
int grhip_generic_mod_taps(grhip_generic_mod *h, float *taps, size_t capacity)
{
    GRHIP_MD_NULL(h);
    if (capacity && !taps) return fail(GRHIP_EINVAL, "null argument");
    for (size_t i = 0; i < h->taps.size() && i < capacity; ++i) taps[i] = h->taps[i];
    return (int)h->taps.size();
}
long long grhip_generic_mod_max_produced(grhip_generic_mod *h, int n_bytes)
{
    GRHIP_MD_NULL(h);
    return h->max_produced(n_bytes);
}
int grhip_generic_mod_work(grhip_generic_mod *h, int n_bytes, const void *in, void *out, long long out_capacity, long long *produced)
{
    GRHIP_MD_NULL(h);
    return h->work(n_bytes, in, out, out_capacity, produced);
}
int grhip_generic_mod_work_device(grhip_generic_mod *h, int n_bytes, const void *d_in, void *d_out, long long out_stride_items,
                                  long long out_capacity, long long *produced, void *stream)
{
    GRHIP_MD_NULL(h);
    return h->work_device(n_bytes, d_in, d_out, out_stride_items, out_capacity, produced, stream);
}

#undef GRHIP_MD_PACK
#undef GRHIP_MD_WORK
#undef GRHIP_MD_STREAM_BLOCK
#undef GRHIP_MD_NULL

}  // extern "C"
