// fir_plan_test.cc -- csrc/fir_plan.h on the CPU: which engine a call of the FIR family takes.  Properties that must hold
// for every shape, capability set, mode and call, then the shapes whose tests or documents name their engine.  Exits
// non-zero with the first failing case printed.  Links nothing of HIP.
#include <cstdio>
#include <vector>

#include "../csrc/fir_plan.h"
#include "../csrc/mfma_tables.h"

using namespace grhip;

namespace {

const int MODES[] = {GRHIP_MODE_FAST, GRHIP_MODE_GENERIC, GRHIP_MODE_FAST_VALU, GRHIP_MODE_FAST_REFTAPS};
const char *const ENGINES[] = {"EINVAL", "generic", "generic+demod", "real-input", "tiled", "matrix-core", "high-decimation", "overlap-save"};
const char *const EPILOGUES[] = {"none", "rotate", "fused demod", "second-kernel demod"};
long long routes = 0;

struct Shape {
    bool xlating;
    int kind;               // plain: FirKind; xlating: in_kind
    bool real_proto, for_demod;
    int D, T;
    FirCaps caps;
};

FirPlan plan_of(const Shape &s)
{
    return s.xlating ? fir_plan_xlating(s.kind, s.real_proto, s.for_demod, s.D, s.T, s.caps)
                     : fir_plan_plain((FirKind)s.kind, s.D, s.T, s.caps);
}

bool fail_at(const char *what, const Shape &s, const FirCall &c, const FirRoute &r)
{
    printf("FAIL %s: %s kind %d real_proto %d for_demod %d decim %d taps %d caps tiled %d/%d mfma %d hidec %d realin %d | mode %d demod %d "
           "batched %d same_decim %d aligned %d/%d odd_stride %d generic_fused %d n %lld -> %s, %s, rot %d\n",
           what, s.xlating ? "xlating" : "plain", s.kind, s.real_proto, s.for_demod, s.D, s.T, s.caps.tiled_real, s.caps.tiled_cplx,
           s.caps.mfma, s.caps.hidec, s.caps.realin, c.mode, c.demod, c.batched, c.same_decim, c.in_aligned, c.out_aligned,
           c.odd_stride_multi, c.generic_fused, c.n, ENGINES[r.engine], EPILOGUES[r.epilogue], r.need_rot);
    return false;
}

bool fast_engine(FirEngine e) { return e == ENG_REALIN || e == ENG_TILED || e == ENG_MFMA || e == ENG_HIDEC || e == ENG_OLS; }

// every call of one shape
bool check_shape(const Shape &s)
{
    const FirPlan p = plan_of(s);
    const bool ctaps = s.xlating ? !p.premix : s.kind == FIR_CCC;
    // the facts a call of this family can differ in: gr_fir_filter has neither demodulator nor batches (one call of each,
    // refused), freq_xlating has one decimation, and only real items care about the pointers' alignment
    const int vary = !s.xlating ? (4 | 8 | 16 | 128) : s.kind != 0 ? (1 | 2 | 8 | 16) : (1 | 2 | 8 | 16 | 32 | 64 | 128);
    for (int mode : MODES) {
        bool fused_base[2];
        for (int d = 0; d < 2; ++d) {
            FirCall b;
            b.mode = mode; b.demod = d;
            fused_base[d] = fir_route(p, b).epilogue == EPILOGUE_DEMOD_FUSED;
        }
        for (int f = 0; f < 256; ++f) {
            if ((f & ~vary) && !(!s.xlating && (f == 1 || f == 2))) continue;
            FirCall c;
            c.mode = mode;
            c.demod = f & 1; c.batched = f & 2; c.same_decim = !(f & 4); c.in_aligned = !(f & 8); c.out_aligned = !(f & 16);
            c.odd_stride_multi = (f & 32) && c.batched; c.generic_fused = !(f & 64); c.n = (f & 128) ? 1 : 1500;
            const FirRoute r = fir_route(p, c);
            ++routes;
#define NEED(cond, what) do { if (!(cond)) return fail_at(what, s, c, r); } while (0)
            // an engine is named only where the kernel takes the shape and the plan built it
            if (r.engine == ENG_TILED) NEED(p.use_tiled && (ctaps ? s.caps.tiled_cplx : s.caps.tiled_real), "tiled without capability");
            if (r.engine == ENG_MFMA) NEED(p.use_mfma && s.caps.mfma, "matrix cores without capability");
            if (r.engine == ENG_HIDEC) NEED(p.use_hidec && s.caps.hidec, "high-decimation kernel without capability");
            if (r.engine == ENG_REALIN) NEED(p.use_realin && s.caps.realin, "real-input kernel without capability");
            if (r.engine == ENG_OLS) NEED(p.use_ols && ols_in_range(s.T, s.D), "overlap-save outside its range");
            if (mode == GRHIP_MODE_GENERIC) NEED(!fast_engine(r.engine), "GENERIC mode on a fast engine");
            if (mode == GRHIP_MODE_FAST_VALU) NEED(r.engine != ENG_MFMA, "FAST_VALU on the matrix cores");
            if (c.odd_stride_multi) NEED(r.engine != ENG_MFMA, "matrix cores with an odd stride between streams");
            if (!c.in_aligned || !c.out_aligned) NEED(r.engine != ENG_REALIN, "real-input kernel on a misaligned pointer");
            if (!s.xlating && !c.same_decim && !c.demod && !c.batched) NEED(r.engine == ENG_GENERIC, "another decimation off the generic kernel");
            if (!s.xlating) NEED(r.epilogue == EPILOGUE_NONE && !r.need_rot, "gr_fir_filter with an epilogue");
            if (r.epilogue == EPILOGUE_DEMOD_FUSED) NEED(c.demod && !r.need_rot, "fused demodulator reading rotator phases");
            if (r.epilogue == EPILOGUE_DEMOD_SECOND) NEED(c.demod, "demodulator without demod");
            if (!c.batched) {
                // the carry frame is chosen before pointers and lengths are known
                NEED(fused_base[c.demod] == (r.epilogue == EPILOGUE_DEMOD_FUSED),
                     "fused-demodulator answer depends on alignment, n or the generic kernel's refusal");
            } else {
                NEED(r.engine == ENG_EINVAL || r.engine == ENG_GENERIC_DEMOD || r.engine == ENG_TILED || r.engine == ENG_MFMA ||
                         (r.engine == ENG_HIDEC && r.epilogue == EPILOGUE_DEMOD_FUSED),
                     "batch on an engine that takes one stream");
                if (c.demod && !c.odd_stride_multi)
                    NEED(fir_has_batched_engine(p, mode) == fast_engine(r.engine), "fir_has_batched_engine disagrees with the route");
            }
#undef NEED
        }
    }
    return true;
}

bool sweep()
{
    std::vector<int> decims;
    for (int d = 1; d <= 20; ++d) decims.push_back(d);
    for (int d : {25, 32, 64, 256, 300}) decims.push_back(d);
    for (int D : decims) {
        std::vector<int> taps = {0, 1, 2, 47, 48, 512, 513, 1024, 1025, 2048, 2049, 2050};
        for (int per : {16, 24, 26, 28, 40, 48, 56, 60, 120, 176})
            for (int e = -1; e <= 1; ++e) taps.push_back(per * D + e);
        for (int T : taps)
            for (int cb = 0; cb < 32; ++cb) {
                Shape s{};
                s.D = D; s.T = T;
                s.caps.tiled_real = cb & 1; s.caps.tiled_cplx = cb & 2; s.caps.mfma = cb & 4; s.caps.hidec = cb & 8; s.caps.realin = cb & 16;
                for (int k = 0; k < 6; ++k) {
                    s.xlating = false; s.kind = k;
                    if (!check_shape(s)) return false;
                }
                for (int x = 0; x < 12; ++x) {
                    s.xlating = true; s.kind = x % 3; s.real_proto = (x / 3) & 1; s.for_demod = x >= 6;
                    if (!check_shape(s)) return false;
                }
            }
    }
    return true;
}

// ---- the shapes whose engine a test or a document names -------------------------------------------------------------------
// Capabilities as the kernels document them (fir_kernels.h): tiled -- decimation 1 / 2 / 4, up to 1024 taps; matrix cores --
// mf::supported (decimation 2 / 4, up to ~260 taps); high-decimation -- decimation 3..256, up to 2048 taps, the tile in
// 6144 samples of LDS; real-input -- decimation 1 / 2 / 4 / 8, up to 1024 taps.
FirCaps documented(int D, int T)
{
    FirCaps c;
    c.tiled_real = c.tiled_cplx = (D == 1 || D == 2 || D == 4) && T >= 1 && T <= 1024;
    c.mfma = mf::supported(D, T);
    c.hidec = D >= 3 && D <= 256 && T >= 1 && T <= 2048 && (6144 - T - 64) / D >= 64;
    c.realin = (D == 1 || D == 2 || D == 4 || D == 8) && T >= 1 && T <= 1024;
    return c;
}

struct Row {
    const char *what;
    bool xlating;
    int kind;
    bool real_proto, for_demod;
    int T, D, mode;
    bool demod;
    long long n;
    FirEngine engine;
    FirEpilogue epilogue;
    bool batched = false, odd_stride = false;       // xlating: several captures in one launch, an odd number of items apart
};

const int FAST = GRHIP_MODE_FAST, VALU = GRHIP_MODE_FAST_VALU, GEN = GRHIP_MODE_GENERIC;
// The expected values are those of the dispatch this header replaced (gr_fir_filter's install / run_engines and
// XlatingCore's build / run before fir_plan.h existed), worked out by hand from that code.
const Row ROWS[] = {
    // test_overlap_save_engine_persistent_walk
    {"ccc 1100/1", false, FIR_CCC, false, false, 1100, 1, FAST, false, 1500, ENG_OLS, EPILOGUE_NONE},
    {"ccc 600/4", false, FIR_CCC, false, false, 600, 4, FAST, false, 1500, ENG_OLS, EPILOGUE_NONE},
    {"ccc 200/3", false, FIR_CCC, false, false, 200, 3, FAST, false, 1500, ENG_OLS, EPILOGUE_NONE},
    // test_fused_demod_other_decimations...
    {"demod 200/10", true, 0, true, true, 200, 10, FAST, true, 1500, ENG_HIDEC, EPILOGUE_DEMOD_FUSED},
    {"demod 400/20", true, 0, true, true, 400, 20, FAST, true, 1500, ENG_HIDEC, EPILOGUE_DEMOD_FUSED},
    {"demod 64/8", true, 0, true, true, 64, 8, FAST, true, 1500, ENG_HIDEC, EPILOGUE_DEMOD_FUSED},
    // CFG2, the benchmark's shape
    {"CFG2 FAST", true, 0, true, true, 256, 4, FAST, true, 1500, ENG_MFMA, EPILOGUE_DEMOD_FUSED},
    {"CFG2 FAST_VALU", true, 0, true, true, 256, 4, VALU, true, 1500, ENG_TILED, EPILOGUE_DEMOD_FUSED},
    {"CFG2 GENERIC", true, 0, true, true, 256, 4, GEN, true, 1500, ENG_GENERIC_DEMOD, EPILOGUE_ROTATE},
    // gr_fir_filter
    {"ccf 256/4", false, FIR_CCF, false, false, 256, 4, FAST, false, 1500, ENG_MFMA, EPILOGUE_NONE},
    {"ccf 256/4 FAST_VALU", false, FIR_CCF, false, false, 256, 4, VALU, false, 1500, ENG_OLS, EPILOGUE_NONE},     // 64 per phase > 28
    {"ccf 32/1", false, FIR_CCF, false, false, 32, 1, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    // (64 taps at decimation 1 are past the measured crossover of 48 taps per phase: the engine, not the tiled kernel)
    {"ccf 64/1", false, FIR_CCF, false, false, 64, 1, FAST, false, 1500, ENG_OLS, EPILOGUE_NONE},
    {"ccf 48/1", false, FIR_CCF, false, false, 48, 1, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    // float data: the float-pair mode up to 176 taps per phase, a single output has no pair
    {"fff 128/1", false, FIR_FFF, false, false, 128, 1, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"fff 128/1 n=1", false, FIR_FFF, false, false, 128, 1, FAST, false, 1, ENG_GENERIC, EPILOGUE_NONE},
    {"fff 176/1", false, FIR_FFF, false, false, 176, 1, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    // (256 taps are past the 176: the real-data engine, whatever n)
    {"fff 256/1", false, FIR_FFF, false, false, 256, 1, FAST, false, 1500, ENG_OLS, EPILOGUE_NONE},
    {"fff 256/1 n=1", false, FIR_FFF, false, false, 256, 1, FAST, false, 1, ENG_OLS, EPILOGUE_NONE},
    {"fsf 128/1", false, FIR_FSF, false, false, 128, 1, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"fcc 64/8", false, FIR_FCC, false, false, 64, 8, FAST, false, 1500, ENG_REALIN, EPILOGUE_NONE},
    {"fcc 64/3", false, FIR_FCC, false, false, 64, 3, FAST, false, 1500, ENG_GENERIC, EPILOGUE_NONE},
    {"fcc 64/8 GENERIC", false, FIR_FCC, false, false, 64, 8, GEN, false, 1500, ENG_GENERIC, EPILOGUE_NONE},
    // tests/test_gpu_fir_walk.py: one row per case of its WALK_CASES, by id -- the kernel whose tile walk the case is there for
    {"walk tiled-ccf-32/1", false, FIR_CCF, false, false, 32, 1, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"walk tiled-ccc-80/2", false, FIR_CCC, false, false, 80, 2, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"walk tiled-ccf-92/4", false, FIR_CCF, false, false, 92, 4, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"walk tiled-ccc-104/4", false, FIR_CCC, false, false, 104, 4, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"walk tiled-ccf-120/2", false, FIR_CCF, false, false, 120, 2, VALU, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"walk tiled-ccf-112/4", false, FIR_CCF, false, false, 112, 4, VALU, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"walk tiled-fff-128/1", false, FIR_FFF, false, false, 128, 1, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"walk tiled-fff-176/2", false, FIR_FFF, false, false, 176, 2, FAST, false, 1500, ENG_TILED, EPILOGUE_NONE},
    {"walk tiled-xlating-real-256/4", true, 0, true, false, 256, 4, VALU, false, 1500, ENG_TILED, EPILOGUE_ROTATE},
    {"walk tiled-xlating-complex-200/4", true, 0, false, false, 200, 4, FAST, false, 1500, ENG_TILED, EPILOGUE_ROTATE},
    {"walk tiled-demod-256/4", true, 0, true, true, 256, 4, VALU, true, 1500, ENG_TILED, EPILOGUE_DEMOD_FUSED},
    {"walk tiled-captures-even", true, 0, true, true, 256, 4, VALU, true, 1500, ENG_TILED, EPILOGUE_DEMOD_FUSED, true, false},
    {"walk tiled-captures-odd", true, 0, true, true, 256, 4, FAST, true, 1500, ENG_TILED, EPILOGUE_DEMOD_FUSED, true, true},
    {"walk hidec-ccf-64/8", false, FIR_CCF, false, false, 64, 8, FAST, false, 1500, ENG_HIDEC, EPILOGUE_NONE},
    {"walk hidec-ccc-128/64", false, FIR_CCC, false, false, 128, 64, FAST, false, 1500, ENG_HIDEC, EPILOGUE_NONE},
    {"walk hidec-xlating-real-64/8", true, 0, true, false, 64, 8, FAST, false, 1500, ENG_HIDEC, EPILOGUE_ROTATE},
    {"walk hidec-xlating-complex-48/3", true, 0, false, false, 48, 3, FAST, false, 1500, ENG_HIDEC, EPILOGUE_ROTATE},
    {"walk hidec-xlating-real-96/3", true, 0, true, false, 96, 3, FAST, false, 1500, ENG_HIDEC, EPILOGUE_ROTATE},
    {"walk hidec-demod-64/8", true, 0, true, true, 64, 8, FAST, true, 1500, ENG_HIDEC, EPILOGUE_DEMOD_FUSED},
    {"walk hidec-captures-200/5", true, 0, true, true, 200, 5, FAST, true, 1500, ENG_HIDEC, EPILOGUE_DEMOD_FUSED, true, true},
    {"walk realin-fcc-64/8", false, FIR_FCC, false, false, 64, 8, FAST, false, 1500, ENG_REALIN, EPILOGUE_NONE},
    {"walk realin-scc-64/4", false, FIR_SCC, false, false, 64, 4, FAST, false, 1500, ENG_REALIN, EPILOGUE_NONE},
    {"walk realin-xlating-fcf-64/4", true, 1, true, false, 64, 4, FAST, false, 1500, ENG_REALIN, EPILOGUE_ROTATE},
    {"walk gtiled-ccf-64/16", false, FIR_CCF, false, false, 64, 16, GEN, false, 1500, ENG_GENERIC, EPILOGUE_NONE},
    {"walk gtiled-ccc-33/3", false, FIR_CCC, false, false, 33, 3, GEN, false, 1500, ENG_GENERIC, EPILOGUE_NONE},
};

bool table()
{
    for (const Row &w : ROWS) {
        Shape s{w.xlating, w.kind, w.real_proto, w.for_demod, w.D, w.T, documented(w.D, w.T)};
        if (!w.xlating) {       // gr_fir_fff's float-pair mode runs the tiled kernel at twice the decimation
            const int dk = fir_tiled_decim((FirKind)w.kind, w.D);
            s.caps.tiled_real = s.caps.tiled_cplx = dk != 0 && documented(dk, w.T).tiled_real;
        }
        FirCall c;
        c.mode = w.mode; c.demod = w.demod; c.n = w.n; c.batched = w.batched; c.odd_stride_multi = w.odd_stride;
        const FirRoute r = fir_route(plan_of(s), c);
        if (r.engine != w.engine || r.epilogue != w.epilogue) {
            printf("FAIL %s: routed to %s (%s), expected %s (%s)\n", w.what, ENGINES[r.engine], EPILOGUES[r.epilogue], ENGINES[w.engine],
                   EPILOGUES[w.epilogue]);
            return false;
        }
    }
    return true;
}

bool kinds()
{
    const char *const names[] = {"fff", "ccf", "ccc", "fcc", "scc", "fsf"};
    FirKind k;
    for (int i = 0; i < 6; ++i)
        if (!fir_kind_parse(names[i], &k) || k != (FirKind)i) { printf("FAIL kind '%s'\n", names[i]); return false; }
    for (const char *bad : {"", "cc", "ccfx", "xyz", "CCF"})
        if (fir_kind_parse(bad, &k)) { printf("FAIL kind '%s' accepted\n", bad); return false; }
    return true;
}

}  // namespace

int main()
{
    if (!kinds() || !table() || !sweep()) return 1;
    printf("fir_plan: %zu named shapes, %lld routes checked\n", sizeof(ROWS) / sizeof(ROWS[0]), routes);
    return 0;
}
