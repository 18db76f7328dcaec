// trellis.h -- what the trellis handles (capi_trellis.hip) and their kernels (trellis.hip, trellis_viterbi.hip) share:
// the metric types, the decoder's launch plan and the launchers.  Not part of the ABI.
#pragma once
#include <climits>

#include "grhip_internal.h"
#include "trellis_fsm.h"

namespace grhip {

enum { TRELLIS_EUCLIDEAN = 200, TRELLIS_HARD_SYMBOL = 201, TRELLIS_HARD_BIT = 202 };    // gr-digital/include/digital_metric_type.h:26-28

enum { TR_B = 0, TR_S = 1, TR_I = 2, TR_F = 3, TR_C = 4 };       // item types: byte, short, int, float, complex
inline size_t tr_item_size(int t) { return t == TR_B ? 1 : t == TR_S ? 2 : t == TR_C ? 8 : 4; }

// ---- encoder -----------------------------------------------------------------------------------------------------------
constexpr int ENC_CHUNK = 256;          // items per chunk of the parallel form
constexpr int ENC_WIN = 1024;           // items of the serial form's LDS window
constexpr int ENC_MAX_S = 64;           // the parallel form: one lane per start state

// out[i] = OS[st * I + in[i]], st = NS[st * I + in[i]] on `streams` streams of n items back to back, each from its own
// state[stream]; *flag becomes nonzero where an input is outside [0, I), and then no state is written.
int encoder_serial_launch(int tin, int tout, const void *in, void *out, int n, int streams, int I, const int *NS, const int *OS,
                          int *state, unsigned *flag, hipStream_t st);
// the same bytes in three launches: end-state maps per chunk, the chain along the stream, the walk per chunk.
// maps: streams * chunks * S bytes, starts: streams * chunks ints
int encoder_chunked_launch(int tin, int tout, const void *in, void *out, int n, int streams, int I, int S, const int *NS,
                           const int *OS, int *state, unsigned *flag, unsigned char *maps, int *starts, hipStream_t st);

// ---- metrics -----------------------------------------------------------------------------------------------------------
// steps * D items of type t in, steps * O floats out; table: O * D items
int metrics_launch(int t, int type, const void *in, float *out, long long steps, int O, int D, const void *table, hipStream_t st);

// ---- decoder -----------------------------------------------------------------------------------------------------------
constexpr int VIT_MAX_S = 1024;
constexpr int VIT_LARGE_WAVES_PER_SIMD = 7;                 // what the large form's 63 - 69 VGPRs leave
constexpr size_t VIT_MAX_WORKSPACE = (size_t)1 << 30;       // bytes of trace a handle may keep in device memory

struct VitPlan {
    int S, O, K, S0, SK;
    int G;              // blocks a workgroup decodes side by side
    int T;              // lanes of a workgroup
    int nwaves;
    int Pmax, nb;       // the longest predecessor list; bits of a decision
    int preg;           // predecessor entries held in registers (0: read from the table)
    int small;          // S <= 64: one wavefront, lanes = (block, state)
    int W;              // steps of the metric window in LDS (0: metrics are read from device memory)
    int TW;             // steps whose trace fits in LDS
    int OC;             // steps of output collected in LDS before they are stored
    int tab_lds;        // the predecessor table fits in LDS
    int max_groups;     // workgroups resident at once: the grid, and what the workspace is sized by
    unsigned off_alpha, off_wmin, off_win, off_trace, off_out, off_cnt, off_tab, lds_bytes;
    size_t ws_words;    // 64-bit words of workspace per workgroup (0: the trace stays in LDS)
};

// the plan of a decoder over an FSM with these sizes; `generic`: metrics read from device memory, table walked
inline bool viterbi_plan(int S, int O, int K, int S0, int SK, int Pmax, size_t out_item, int cus, bool generic, VitPlan &p)
{
    if (S < 1 || S > VIT_MAX_S || O < 1 || K < 1 || S0 >= S || SK >= S || Pmax < 0) return false;
    p = VitPlan{};
    p.S = S; p.O = O; p.K = K; p.S0 = S0; p.SK = SK; p.Pmax = Pmax < 1 ? 1 : Pmax;
    p.small = S <= 64;
    p.G = p.small ? 64 / S : 1;
    p.nwaves = p.small ? 1 : (S + 63) / 64;
    p.T = 64 * p.nwaves;
    p.nb = 0;
    while ((1 << p.nb) < p.Pmax) ++p.nb;
    p.preg = generic ? 0 : p.Pmax <= 1 ? 1 : p.Pmax <= 2 ? 2 : p.Pmax <= 4 ? 4 : 0;
    const long long wf = (long long)p.T * (p.small ? 16 : 4);           // floats of the metric window
    const long long w = generic ? 0 : wf / ((long long)p.G * O);
    p.W = (int)(w > K ? K : w);
    const int nbw = p.nwaves * p.nb;
    p.TW = nbw ? (8 * 1024) / (nbw * 8) : INT_MAX;
    if (p.TW < 1) return false;
    const long long oc = 2048 / ((long long)p.G * (long long)out_item);
    p.OC = (int)(oc > K ? K : oc);
    const size_t tab_bytes = (size_t)S * p.Pmax * 8;
    p.tab_lds = tab_bytes <= (p.small ? (size_t)8 * 1024 : (size_t)16 * 1024);
    unsigned o = 0;
    p.off_alpha = o; o += 2u * p.T * 4u;
    p.off_wmin = o;  o += 3u * 16u * 4u;
    p.off_win = o;   o += (unsigned)(p.W ? wf * 4 : 0);
    p.off_trace = o; o += nbw ? (unsigned)((size_t)(K < p.TW ? K : p.TW) * nbw * 8) : 0u;
    p.off_out = o;   o += (unsigned)((size_t)p.G * p.OC * out_item + 7) & ~7u;
    p.off_cnt = o;   o += (unsigned)S * 4u;
    o = (o + 7u) & ~7u;
    p.off_tab = o;   o += p.tab_lds ? (unsigned)tab_bytes : 0u;
    p.lds_bytes = o;
    // resident workgroups per CU: the small form runs at 2 waves per SIMD (its registers), the large form at up to
    // VIT_LARGE_WAVES_PER_SIMD, a workgroup taking ceil(nwaves / 4) of them, and at most two for their LDS
    const int wg_waves_per_simd = (p.nwaves + 3) / 4;
    const int large_per_cu = VIT_LARGE_WAVES_PER_SIMD / wg_waves_per_simd < 2 ? VIT_LARGE_WAVES_PER_SIMD / wg_waves_per_simd : 2;
    p.max_groups = (cus < 1 ? 1 : cus) * (p.small ? 8 : (large_per_cu < 1 ? 1 : large_per_cu));
    p.ws_words = K > p.TW ? (size_t)K * nbw : 0;
    if (p.ws_words) {
        if (p.ws_words * 8 > VIT_MAX_WORKSPACE) return false;
        const size_t fit = VIT_MAX_WORKSPACE / (p.ws_words * 8);
        if ((size_t)p.max_groups > fit) p.max_groups = (int)fit;
    }
    return true;
}

// the raw inputs of the combined decoder: nblocks * K * D items of type t (in == nullptr: the metrics come in `in`)
struct VitRaw {
    const void *in = nullptr, *table = nullptr;     // table: O * D items
    int t = TR_F, D = 1, type = TRELLIS_EUCLIDEAN, item_bytes = 4;
};

// in: nblocks * K * O floats, out: nblocks * K items of out_type; tab: S * Pmax entries {ps | pi << 10, OS index},
// cnt: S list lengths; ws: max_groups * ws_words words; *dead counts the dead ends of the traceback.  With raw.in the
// step's metrics are formed from the raw items inside the kernel (the plan must have a metric window, W > 0).
int viterbi_launch(const VitPlan &p, int out_type, const float *in, void *out, long long nblocks, const int2 *tab, const int *cnt,
                   unsigned long long *ws, unsigned long long *dead, const VitRaw &raw, hipStream_t st);

}  // namespace grhip
