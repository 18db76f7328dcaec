// trellis_viterbi.hip -- viterbi_algorithm (gr-trellis/src/lib/core_algorithms.cc:45-109) with the lanes of a wavefront as
// the states of the recurrence.
//
// A call is nblocks independent problems of K steps (trellis_viterbi_X.cc.t:163-183).  For S <= 64 a workgroup is one
// wavefront that decodes G = 64 / S blocks side by side, lane = block * S + state; for larger S a workgroup of S lanes
// (rounded up to wavefronts) decodes one block.  Workgroups are persistent: workgroup g takes the block groups g,
// g + gridDim.x, ...
//
// Per step every lane does the add-compare-select of its next state with the reference's statements: the predecessors in
// PS[j] order, mm = alpha[ps] + in[k * O + OS[ps * I + pi]], a strict <, minm from INF = 1e9 and minmi from 0.  The
// reference then subtracts the step's norm from every alpha; here a lane stores its raw minimum and the reader subtracts
// the norm before it adds the metric, (raw - norm) + metric, which is the same two roundings in the same order, so that a
// step needs one barrier.  The norm is a minimum of values none of which is a NaN (a NaN never passes the strict <), so
// its order does not matter, except for the sign of a zero, which no comparison and no sum with a non-zero sees.
//
// The decision of a step is nb = ceil(log2 Pmax) bit planes, each the ballot of a wavefront; for Pmax = 2 the ballot is
// the decision word.  TW steps of trace fit in LDS; a longer block flushes every full window to the handle's workspace
// and the traceback reads the windows back, so that the dependent chain of the traceback (decision word, then table entry)
// runs on LDS.  One lane per block traces back; outputs are collected in LDS and stored side by side.
//
// COMB is viterbi_algorithm_combined (core_algorithms.cc:147-217): the step's O metrics are calc_metric of the step's D raw
// inputs.  The window is then filled from the raw items: the lane that would have loaded metric (block, step, o) forms it
// with calc_metric's statements (csrc/trellis_metric.h), so a step moves D * sizeof(item) bytes instead of 4 * O.
#include "trellis_metric.h"

namespace grhip {

namespace {

constexpr float VIT_INF = 1.0e9f;       // core_algorithms.cc:30

template <class To, int PREG, bool SMALL, bool COMB>
__global__ void __launch_bounds__(SMALL ? 64 : 1024)
viterbi_kernel(const VitPlan p, const float *__restrict__ in, To *__restrict__ out, const long long NB,
               const int2 *__restrict__ tab, const int *__restrict__ cnt, unsigned long long *__restrict__ ws,
               unsigned long long *__restrict__ dead, const VitRaw raw)
{
    extern __shared__ __align__(16) unsigned char vit_lds[];
    constexpr int R = SMALL ? 16 : 4;               // floats of the metric window a lane carries
    constexpr int NREG = PREG > 0 ? PREG : 1;
    const int tid = threadIdx.x, T = p.T, S = p.S, O = p.O, K = p.K, G = p.G, Pmax = p.Pmax, nb = p.nb, W = p.W, TW = p.TW,
              OC = p.OC;
    const int b = SMALL ? tid / S : 0;
    const int s = SMALL ? tid - b * S : tid;
    const bool lane_valid = SMALL ? b < G : tid < S;
    const int base = b * S;
    float *alpha = (float *)(vit_lds + p.off_alpha);
    float *wmin = (float *)(vit_lds + p.off_wmin);
    int *widx = (int *)(wmin + 32);
    float *win = (float *)(vit_lds + p.off_win);
    unsigned long long *tr = (unsigned long long *)(vit_lds + p.off_trace);
    To *ob = (To *)(vit_lds + p.off_out);
    int *lcnt = (int *)(vit_lds + p.off_cnt);
    int2 *ltab = (int2 *)(vit_lds + p.off_tab);
    const int2 *tb = p.tab_lds ? (const int2 *)ltab : tab;

    if (p.tab_lds)
        for (int i = tid; i < S * Pmax; i += T) ltab[i] = tab[i];
    for (int i = tid; i < S; i += T) lcnt[i] = cnt[i];
    const int mycnt = lane_valid ? cnt[s] : 0;
    int rps[NREG], rmi[NREG];
#pragma unroll
    for (int i = 0; i < NREG; ++i) {
        int2 e = make_int2(0, 0);
        if (PREG > 0 && lane_valid && i < Pmax) e = tab[s * Pmax + i];
        rps[i] = e.x & 1023;
        rmi[i] = e.y;
    }
    __syncthreads();

    const int nbw = p.nwaves * nb;
    const bool ring = K > TW;
    const size_t slot = (size_t)blockIdx.x * p.ws_words;
    const long long ngroups = (NB + G - 1) / G;
    const int wlen = W * O;                          // floats of one block in the metric window
    const long long block_floats = (long long)K * O;
    unsigned long long ndead = 0;

    for (long long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long blk = grp * G + b;
        const bool active = lane_valid && blk < NB;
        const float *bin = in + (active ? blk : 0) * block_floats;
        int cur = 0;
        alpha[tid] = p.S0 < 0 ? 0.0f : (s == p.S0 ? 0.0f : VIT_INF);
        float norm = 0.0f;                           // what the readers of alpha[cur] still have to subtract
        if (!SMALL && tid < 16) wmin[tid] = 0.0f;

        float pre[R];
        auto issue = [&](int w0) {                   // the window that starts at step w0, into registers
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int e = tid + i * T;
                pre[i] = 0.0f;
                if (e < G * wlen) {
                    const int bb = SMALL ? e / wlen : 0;
                    const int r = e - bb * wlen;
                    const long long blk2 = grp * G + bb, off = (long long)w0 * O + r;
                    if (blk2 < NB && off < block_floats) {
                        if (COMB) {                  // metric (step, o) of the block's raw items
                            const long long step = off / O;
                            const int o = (int)(off - step * O);
                            const char *x = (const char *)raw.in + (size_t)(blk2 * K + step) * raw.D * raw.item_bytes;
                            pre[i] = metric_entry_any(raw.t, x, raw.table, o, O, raw.D, raw.type);
                        } else {
                            pre[i] = in[blk2 * block_floats + off];
                        }
                    }
                }
            }
        };
        if (W > 0) issue(0);
        __syncthreads();

        int wk = 0, wbase = 0, tk = 0, tbase = 0;
        for (int k = 0; k < K; ++k) {
            if (W > 0) {
                if (wk == W) { wk = 0; wbase += W; }
                if (wk == 0) {                       // every lane is past the barrier behind the last read of the window
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const int e = tid + i * T;
                        if (e < G * wlen) win[e] = pre[i];
                    }
                    __syncthreads();
                    if (wbase + W < K) issue(wbase + W);    // in flight through this window's steps
                }
            }
            if (!SMALL) {
                float n = VIT_INF;
                for (int w = 0; w < p.nwaves; ++w) {
                    const float v = wmin[cur * 16 + w];
                    if (v < n) n = v;
                }
                norm = n;
            }
            const float *a_cur = alpha + cur * T + base;
            const float *m_cur = W > 0 ? win + b * wlen + wk * O : nullptr;
            float minm = VIT_INF;
            int minmi = 0;
            if (PREG > 0) {
#pragma unroll
                for (int i = 0; i < NREG; ++i)
                    if (i < mycnt) {
                        const float m = W > 0 ? m_cur[rmi[i]] : bin[(long long)k * O + rmi[i]];
                        const float mm = __fadd_rn(__fsub_rn(a_cur[rps[i]], norm), m);
                        if (mm < minm) { minm = mm; minmi = i; }
                    }
            } else {
                for (int i = 0; i < mycnt; ++i) {
                    const int2 e = tb[s * Pmax + i];
                    const float m = W > 0 ? m_cur[e.y] : (active ? bin[(long long)k * O + e.y] : 0.0f);
                    const float mm = __fadd_rn(__fsub_rn(a_cur[e.x & 1023], norm), m);
                    if (mm < minm) { minm = mm; minmi = i; }
                }
            }
            // the step's norm: the minimum of minm over the block's states, from INF
            float v = minm;
            if (SMALL) {
                for (int off = 1; off < S; off <<= 1) {
                    int sp = s + off;
                    if (sp >= S) sp -= S;
                    const float o = __shfl(v, lane_valid ? base + sp : tid);
                    v = o < v ? o : v;
                }
            } else {
                for (int m = 32; m >= 1; m >>= 1) {
                    const float o = __shfl_xor(v, m);
                    v = o < v ? o : v;
                }
                if ((tid & 63) == 0) wmin[(cur ^ 1) * 16 + (tid >> 6)] = v;
            }
            alpha[(cur ^ 1) * T + tid] = minm;
            for (int bit = 0; bit < nb; ++bit) {
                const unsigned long long word = __ballot((minmi >> bit) & 1);
                if ((tid & 63) == 0) tr[(size_t)tk * nbw + (tid >> 6) * nb + bit] = word;
            }
            if (SMALL) norm = v;
            cur ^= 1;
            ++wk;
            ++tk;
            __syncthreads();
            if (ring && (tk == TW || k == K - 1)) {  // a full window of trace, in whole lines, to the workspace
                for (int i = tid; i < tk * nbw; i += T) ws[slot + (size_t)tbase * nbw + i] = tr[i];
                tbase += tk;
                tk = 0;
                __syncthreads();
            }
        }

        // the last alpha as the reference leaves it: raw - norm
        if (!SMALL) {
            float n = VIT_INF;
            for (int w = 0; w < p.nwaves; ++w) {
                const float x = wmin[cur * 16 + w];
                if (x < n) n = x;
            }
            norm = n;
        }
        const float fin = __fsub_rn(alpha[cur * T + tid], norm);
        __syncthreads();
        alpha[cur * T + tid] = fin;
        __syncthreads();

        // the final state: SK, or the first minimum below INF in state order (core_algorithms.cc:92-101)
        const bool tracer = SMALL ? (tid < G && grp * G + tid < NB) : tid == 0;
        const int tslot = SMALL ? tid : 0;
        int st = p.SK < 0 ? 0 : p.SK;
        if (p.SK < 0) {
            if (SMALL) {
                if (tracer) {
                    float best = VIT_INF;
                    for (int i = 0; i < S; ++i) {
                        const float x = alpha[cur * T + tid * S + i];
                        if (x < best) { best = x; st = i; }
                    }
                }
            } else {
                float x = lane_valid ? fin : VIT_INF;
                int xi = tid;
                if (!(x < VIT_INF)) { x = VIT_INF; xi = INT_MAX; }
                for (int m = 32; m >= 1; m >>= 1) {
                    const float o = __shfl_xor(x, m);
                    const int oi = __shfl_xor(xi, m);
                    if (o < x || (o == x && oi < xi)) { x = o; xi = oi; }
                }
                if ((tid & 63) == 0) { wmin[tid >> 6] = x; widx[tid >> 6] = xi; }
                __syncthreads();
                if (tracer) {
                    float best = VIT_INF;
                    for (int w = 0; w < p.nwaves; ++w)
                        if (wmin[w] < best) { best = wmin[w]; st = widx[w]; }
                }
                __syncthreads();
            }
        }

        // traceback (core_algorithms.cc:103-107), window by window from the end, OC steps of output at a time
        int kend = K;
        while (kend > 0) {
            int wstart = 0;
            if (ring) {
                wstart = ((kend - 1) / TW) * TW;
                for (int i = tid; i < (kend - wstart) * nbw; i += T) tr[i] = ws[slot + (size_t)wstart * nbw + i];
                __syncthreads();
            }
            int chi = kend;
            while (chi > wstart) {
                const int clo = chi - OC > wstart ? chi - OC : wstart;
                if (tracer)
                    for (int kk = chi - 1; kk >= clo; --kk) {
                        int o = 0;
                        if (lcnt[st] == 0) {
                            ++ndead;                 // no predecessor: symbol 0, and the state stays
                        } else {
                            const int pos = tslot * S + st;
                            const unsigned long long *w = tr + (size_t)(kk - wstart) * nbw + (pos >> 6) * nb;
                            int i0 = 0;
                            for (int bit = 0; bit < nb; ++bit) i0 |= (int)((w[bit] >> (pos & 63)) & 1ull) << bit;
                            const int2 e = tb[st * Pmax + i0];
                            o = e.x >> 10;
                            st = e.x & 1023;
                        }
                        ob[tslot * OC + (kk - clo)] = (To)o;
                    }
                __syncthreads();
                const int len = chi - clo;
                for (int e = tid; e < G * len; e += T) {
                    const int bb = e / len, r = e - bb * len;
                    const long long blk2 = grp * G + bb;
                    if (blk2 < NB) out[blk2 * K + clo + r] = ob[bb * OC + r];
                }
                __syncthreads();
                chi = clo;
            }
            kend = wstart;
        }
    }
    if (ndead) atomicAdd(dead, ndead);
}

template <class To, int PREG, bool SMALL, bool COMB>
int launch_comb(const VitPlan &p, const float *in, void *out, long long nblocks, const int2 *tab, const int *cnt,
                unsigned long long *ws, unsigned long long *dead, const VitRaw &raw, hipStream_t st)
{
    const void *kernel = (const void *)viterbi_kernel<To, PREG, SMALL, COMB>;
    int rc = allow_lds(kernel, p.lds_bytes);
    if (rc) return rc;
    const long long ngroups = (nblocks + p.G - 1) / p.G;
    const unsigned grid = (unsigned)(ngroups < p.max_groups ? ngroups : p.max_groups);
    hipLaunchKernelGGL((viterbi_kernel<To, PREG, SMALL, COMB>), dim3(grid), dim3(p.T), p.lds_bytes, st, p, in, (To *)out, nblocks,
                       tab, cnt, ws, dead, raw);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <class To, int PREG, bool SMALL>
int launch_one(const VitPlan &p, const float *in, void *out, long long nblocks, const int2 *tab, const int *cnt,
               unsigned long long *ws, unsigned long long *dead, const VitRaw &raw, hipStream_t st)
{
    return raw.in ? launch_comb<To, PREG, SMALL, true>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st)
                  : launch_comb<To, PREG, SMALL, false>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st);
}

template <class To, bool SMALL>
int launch_preg(const VitPlan &p, const float *in, void *out, long long nblocks, const int2 *tab, const int *cnt,
                unsigned long long *ws, unsigned long long *dead, const VitRaw &raw, hipStream_t st)
{
    switch (p.preg) {
    case 1: return launch_one<To, 1, SMALL>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st);
    case 2: return launch_one<To, 2, SMALL>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st);
    case 4: return launch_one<To, 4, SMALL>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st);
    default: return launch_one<To, 0, SMALL>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st);
    }
}

template <class To>
int launch_out(const VitPlan &p, const float *in, void *out, long long nblocks, const int2 *tab, const int *cnt,
               unsigned long long *ws, unsigned long long *dead, const VitRaw &raw, hipStream_t st)
{
    return p.small ? launch_preg<To, true>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st)
                   : launch_preg<To, false>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st);
}

}  // namespace

int viterbi_launch(const VitPlan &p, int out_type, const float *in, void *out, long long nblocks, const int2 *tab, const int *cnt,
                   unsigned long long *ws, unsigned long long *dead, const VitRaw &raw, hipStream_t st)
{
    if (nblocks < 1) return GRHIP_OK;
    if (raw.in && p.W < 1) return fail(GRHIP_EINVAL, "viterbi: the fused metrics need the metric window");
    switch (out_type) {
    case TR_B: return launch_out<unsigned char>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st);
    case TR_S: return launch_out<short>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st);
    case TR_I: return launch_out<int>(p, in, out, nblocks, tab, cnt, ws, dead, raw, st);
    }
    return fail(GRHIP_EINVAL, "viterbi: bad output type");
}

}  // namespace grhip
