// squelch.hip -- kernels of the power squelch blocks: gr_pwr_squelch_cc, gr_pwr_squelch_ff (general/gr_squelch_base_cc.cc:42-93,
// gr_pwr_squelch_cc.{h,cc} and the _ff twins) and gr_simple_squelch_cc (general/gr_simple_squelch_cc.cc:53-71).
//
// Three steps per call:
//   detect  the power in float, the single-pole recurrence in double, and what leaves the walk is one mute bit per sample
//           (y < threshold), 64 to a word.  GENERIC: one lane per stream.  FAST: chunks of SQ_CHUNK samples, every chunk
//           first from a zero start, the chunks chained by (1 - alpha)^SQ_CHUNK, then walked again from their starts.
//   walk    (ramp > 0) one wavefront per stream moves the four-state machine from event to event over 4096 flags at a
//           time and leaves, per flag word, the machine as it stands in front of the word and the output offset.
//           (ramp == 0 with gating: the state is the flag, the offsets a prefix sum of popcounts.)
//   emit    one lane per sample: from its word's entry it steps over the (few) events in front of it, multiplies by
//           the envelope and writes to its place.
// Every arithmetic step of the detector and of the output product is written with the round-to-nearest intrinsics, so
// none can be contracted whatever the flags.
#include <cmath>

#include "squelch.h"

namespace grhip {

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr long long MAX_BLOCKS_X = 4096;          // emit: grid-stride along the samples from here on
typedef unsigned long long u64;

template <bool CC>
__device__ inline float load_power(const void *in, long long idx)
{
    if (CC) {
        const float2 v = ((const float2 *)in)[idx];
        return __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y));     // gr_pwr_squelch_cc.cc:54, in float
    }
    const float v = ((const float *)in)[idx];
    return __fmul_rn(v, v);                                             // gr_pwr_squelch_ff.cc:54
}

// One lane per (chunk, stream) walks its chunk in order, y in a double register; the loads of the next four samples
// are issued before the four dependent double chains of the current ones.
//   ENDS: start from 0 and write only the value after the chunk (ends[chunk][stream]).
//   else: start from start[chunk][stream] (the stream's state when start is null: one chunk) and write the mute bits,
//         a 64-bit word every 64 samples; the last chunk stores y.  `finish` (no ramp, no gating): the state is the last
//         flag and every sample produces an item, so the same lane stores both.
template <bool CC, bool ENDS>
__global__ void __launch_bounds__(THREADS)
sq_detect_kernel(const void *in, int n, int S, int chunk, int nchunks, double alpha, double oma, double thr,
                 const double *start, double *ends, SquelchState *state, u64 *flags, int nwords, int finish, int *produced)
{
    const long long id = blockIdx.x * (long long)THREADS + threadIdx.x;
    if (id >= (long long)S * nchunks) return;
    const int c = (int)(id / S), s = (int)(id - (long long)c * S);
    const long long j0 = (long long)c * chunk, j1 = j0 + chunk < n ? j0 + chunk : n;
    const long long base = (long long)s * n;
    double y = ENDS ? 0.0 : start ? start[id] : state[s].y;
    u64 bits = 0;
    bool last = false;
    float xa[4], xb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xa[i] = j0 + i < j1 ? load_power<CC>(in, base + j0 + i) : 0.f;
    for (long long j = j0; j < j1; j += 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) xb[i] = j + 4 + i < j1 ? load_power<CC>(in, base + j + 4 + i) : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (j + i < j1) {
                y = __dadd_rn(__dmul_rn(alpha, (double)xa[i]), __dmul_rn(oma, y));     // gr_single_pole_iir.h:93
                if (!ENDS) {
                    last = y < thr;                                                     // gr_pwr_squelch_cc.h:52
                    bits |= (u64)last << (int)((j + i) & 63);
                }
            }
        }
        if (!ENDS && ((((j + 4) & 63) == 0) || j + 4 >= j1)) {
            flags[(long long)s * nwords + (j >> 6)] = bits;
            bits = 0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) xa[i] = xb[i];
    }
    if (ENDS) ends[id] = y;
    else if (c == nchunks - 1) {
        state[s].y = y;
        if (finish) {
            state[s].state = last ? SQ_MUTED : SQ_UNMUTED;
            produced[s] = n;
        }
    }
}

// After a chunk of len samples y = local_end + (1 - alpha)^len * y_start: one lane per stream chains the chunks' local
// ends into every chunk's start value, eight ends loaded ahead of the dependent chain.
__global__ void __launch_bounds__(THREADS)
sq_carry_kernel(const double *__restrict__ ends, double *__restrict__ start, const SquelchState *__restrict__ state, int S,
                int nchunks, double p_chunk)
{
    const int s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= S) return;
    double y = state[s].y;
    for (int c = 0; c < nchunks; c += 8) {
        double e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = c + i < nchunks ? ends[(long long)(c + i) * S + s] : 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (c + i < nchunks) {
                start[(long long)(c + i) * S + s] = y;
                y = __dadd_rn(e[i], __dmul_rn(p_chunk, y));
            }
        }
    }
}

// first sample at or after pos whose bit is set in the wave's 64 words (lane l holds the word that starts at sample ws),
// or -1: a masked ballot and two find-firsts
__device__ inline long long sq_find(u64 m, long long ws, long long pos, long long wbase, int lane)
{
    if (ws + 64 <= pos) m = 0;
    else if (ws < pos) m &= ~0ull << (int)(pos - ws);
    const u64 b = __ballot(m != 0);
    if (!b) return -1;
    const int fl = __ffsll((long long)b) - 1;
    const u64 mw = __shfl(m, fl);
    return (wbase + fl) * 64 + (__ffsll((long long)mw) - 1);
}

// ramp > 0.  One wavefront per stream; the machine (st, r, env, off) is the same in every lane.  A piece [pos, np) of
// the stream is a stable run up to and including the sample that ends it, or the ramp that follows (ramps ignore the
// flags); a lane whose word starts inside the piece takes its entry from it.  Lane 0 stores the state and the count.
__global__ void __launch_bounds__(WAVE)
sq_walk_kernel(const u64 *flags, SquelchEntry *entries, SquelchState *state, int *produced, int n, int nwords, int R, int gate,
               const double *__restrict__ table)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const u64 *F = flags + (long long)s * nwords;
    SquelchEntry *E = entries + (long long)s * nwords;
    int st = state[s].state, r = state[s].ramped, off = 0;
    double env = state[s].envelope;
    long long pos = 0;
    u64 next = lane < nwords ? F[lane] : 0;
    for (long long wbase = 0; wbase < nwords; wbase += WAVE) {
        const u64 w = next;
        next = wbase + WAVE + lane < nwords ? F[wbase + WAVE + lane] : 0;          // in flight under this window's walk
        const long long ws = (wbase + lane) * 64;
        const long long wend = (wbase + WAVE) * 64 < n ? (wbase + WAVE) * 64 : n;
        SquelchEntry e = {0.0, 0, 0, 0, 0};
        while (pos < wend) {
            long long np;
            const int d0 = (int)(ws - pos);
            if (st == SQ_MUTED || st == SQ_UNMUTED) {
                long long q = sq_find(st == SQ_MUTED ? ~w : w, ws, pos, wbase, lane);
                if (q >= wend) q = -1;
                np = q < 0 ? wend : q + 1;
                if (ws >= pos && ws < np) {
                    e.envelope = env; e.state = st; e.ramped = r;
                    e.off = st == SQ_UNMUTED ? off + d0 : off;
                }
                if (st == SQ_UNMUTED) {
                    off += (int)(np - pos);                      // the sample that starts the decay goes out too
                    if (q >= 0) {
                        st = SQ_DECAY;
                        if (r <= 0) r = R;                       // unmuted without a ramp behind it: a whole decay
                    }
                } else if (q >= 0) {
                    off += 1;                                    // the sample that starts the attack, old envelope
                    st = SQ_ATTACK;
                }
            } else if (st == SQ_ATTACK) {
                const long long k = R - r > 1 ? R - r : 1;
                const long long d = k < wend - pos ? k : wend - pos;
                np = pos + d;
                if (ws >= pos && ws < np) { e.envelope = env; e.state = st; e.ramped = r + d0; e.off = off + d0; }
                r += (int)d;
                off += (int)d;
                if (d == k) { st = SQ_UNMUTED; env = 1.0; }
                else env = table[r];
            } else {
                const long long k = r > 0 ? r : 1;
                const long long d = k < wend - pos ? k : wend - pos;
                np = pos + d;
                if (ws >= pos && ws < np) { e.envelope = env; e.state = st; e.ramped = r - d0; e.off = off + d0; }
                r -= (int)d;
                if (d == k) { off += (int)d - 1; st = SQ_MUTED; env = 0.0; }      // 0.5 - cos(0) / 2.0
                else { off += (int)d; env = table[r]; }
            }
            pos = np;
        }
        if (wbase + lane < nwords) E[wbase + lane] = e;
    }
    if (lane == 0) {
        state[s].state = st;
        state[s].ramped = r;
        state[s].envelope = env;
        produced[s] = gate ? off : n;
    }
}

// ramp == 0 with gating: the state after a sample is its flag, so the offset of a word is the number of clear flags in
// front of it.  One wavefront per stream, 64 words a step.
__global__ void __launch_bounds__(WAVE)
sq_scan_kernel(const u64 *flags, SquelchEntry *entries, SquelchState *state, int *produced, int n, int nwords)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const u64 *F = flags + (long long)s * nwords;
    SquelchEntry *E = entries + (long long)s * nwords;
    int off = 0;
    for (long long wbase = 0; wbase < nwords; wbase += WAVE) {
        const long long wi = wbase + lane;
        int cnt = 0;
        if (wi < nwords) {
            const long long left = n - wi * 64;
            const u64 valid = left >= 64 ? ~0ull : (1ull << (int)left) - 1;
            cnt = __popcll(~F[wi] & valid);
        }
        int x = cnt;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const int t = __shfl_up(x, d);
            if (lane >= d) x += t;
        }
        if (wi < nwords) E[wi].off = off + x - cnt;
        off += __shfl(x, WAVE - 1);
    }
    if (lane == 0) {
        const bool mute = (F[nwords - 1] >> ((n - 1) & 63)) & 1;
        state[s].state = mute ? SQ_MUTED : SQ_UNMUTED;
        produced[s] = off;
    }
}

enum { EMIT_CC = 0, EMIT_FF = 1, EMIT_COPY = 2 };

template <int MODE>
__device__ inline void sq_store(const void *in, void *out, long long src, long long dst, double env)
{
    if (MODE == EMIT_FF) {
        // in * d_envelope: the product in double (gr_squelch_base_ff.cc:85)
        ((float *)out)[dst] = (float)__dmul_rn((double)((const float *)in)[src], env);
    } else if (MODE == EMIT_COPY) {
        ((float2 *)out)[dst] = ((const float2 *)in)[src];                          // gr_simple_squelch_cc.cc:64
    } else {
        // in * gr_complex(d_envelope, 0.0): the whole complex product in float (gr_squelch_base_cc.cc:85)
        const float2 v = ((const float2 *)in)[src];
        const float e = (float)env;
        float2 o;
        o.x = __fsub_rn(__fmul_rn(v.x, e), __fmul_rn(v.y, 0.f));
        o.y = __fadd_rn(__fmul_rn(v.x, 0.f), __fmul_rn(v.y, e));
        ((float2 *)out)[dst] = o;
    }
}

template <int MODE>
__device__ inline void sq_store_zero(void *out, long long dst)
{
    if (MODE == EMIT_FF) ((float *)out)[dst] = 0.f;
    else ((float2 *)out)[dst] = make_float2(0.f, 0.f);
}

// One lane per sample, blockIdx.y the stream.  RAMP: the lane starts from its word's entry and steps over the events
// in front of its own bit (a run per step, not a sample per step).  Without a ramp the state is the lane's own flag.
template <int MODE, bool RAMP>
__global__ void __launch_bounds__(THREADS)
sq_emit_kernel(const void *in, void *out, const u64 *__restrict__ flags, const SquelchEntry *__restrict__ entries,
               const SquelchState *state, int n, int nwords, int R, int gate, const double *__restrict__ table)
{
    const int s = blockIdx.y;
    const long long base = (long long)s * n;
    const u64 *F = flags + (long long)s * nwords;
    const SquelchEntry *E = entries + (long long)s * nwords;
    for (long long i = blockIdx.x * (long long)THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * THREADS) {
        const long long wi = i >> 6;
        const int b = (int)(i & 63);
        const u64 w = F[wi];
        bool emit;
        double env;
        int off = 0;
        if (!RAMP) {
            emit = !((w >> b) & 1);
            env = MODE == EMIT_COPY ? 1.0 : state[s].envelope;
            if (gate) off = E[wi].off + __popcll(~w & ((1ull << b) - 1));
        } else {
            const SquelchEntry e = E[wi];
            int st = e.state, r = e.ramped, pos = 0;
            off = e.off;
            env = e.envelope;
            for (;;) {
                if (st == SQ_MUTED) {
                    const u64 c = ~w >> pos;
                    const int q = c ? pos + __ffsll((long long)c) - 1 : 64;
                    if (q >= b) { emit = q == b; break; }
                    off += 1; pos = q + 1; st = SQ_ATTACK;
                } else if (st == SQ_UNMUTED) {
                    const u64 c = w >> pos;
                    const int q = c ? pos + __ffsll((long long)c) - 1 : 64;
                    if (q >= b) { emit = true; off += b - pos; break; }
                    off += q - pos + 1; pos = q + 1; st = SQ_DECAY;
                    if (r <= 0) r = R;
                } else if (st == SQ_ATTACK) {
                    const int k = R - r > 1 ? R - r : 1;
                    if (b - pos < k) {
                        const int ri = r + (b - pos + 1);
                        env = ri >= R ? 1.0 : table[ri];
                        off += b - pos; emit = true; break;
                    }
                    r += k; off += k; pos += k; env = 1.0; st = SQ_UNMUTED;
                } else {
                    const int k = r > 0 ? r : 1;
                    if (b - pos < k) {
                        const int ri = r - (b - pos + 1);
                        emit = ri != 0;
                        if (emit) env = table[ri > 0 ? ri : 0];
                        off += b - pos; break;
                    }
                    r -= k; off += k - 1; pos += k; env = 0.0; st = SQ_MUTED;
                }
            }
        }
        if (emit) sq_store<MODE>(in, out, base + i, base + (gate ? off : i), env);
        else if (!gate) sq_store_zero<MODE>(out, base + i);
    }
}

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Plan {
    int nwords, nchunks;
    bool chunked, ramp_path, entries;
    size_t flags_off, entries_off, ends_off, start_off, total;
};

Plan plan(bool fast, const SquelchLaunch &a)
{
    Plan p;
    p.nwords = (int)(((long long)a.n + 63) / 64);
    p.chunked = fast && a.n > SQ_CHUNK;
    p.nchunks = p.chunked ? (int)(((long long)a.n + SQ_CHUNK - 1) / SQ_CHUNK) : 1;
    p.ramp_path = !a.simple && a.ramp > 0;
    p.entries = p.ramp_path || a.gate;
    const size_t S = (size_t)a.nstreams;
    p.flags_off = 0;
    p.entries_off = align_up(S * p.nwords * sizeof(u64));
    p.ends_off = p.entries_off + align_up(p.entries ? S * p.nwords * sizeof(SquelchEntry) : 0);
    p.start_off = p.ends_off + align_up(p.chunked ? S * p.nchunks * sizeof(double) : 0);
    p.total = p.start_off + align_up(p.chunked ? S * p.nchunks * sizeof(double) : 0);
    return p;
}

template <bool CC, bool ENDS>
int detect(const SquelchLaunch &a, const Plan &p, const double *start, double *ends, u64 *flags, int finish, hipStream_t st)
{
    const long long blocks = ((long long)a.nstreams * p.nchunks + THREADS - 1) / THREADS;
    if (blocks > 0x7fffffffLL) return fail(GRHIP_EINVAL, "squelch: too many items in one call");
    hipLaunchKernelGGL((sq_detect_kernel<CC, ENDS>), dim3((unsigned)blocks), dim3(THREADS), 0, st, a.in, a.n, a.nstreams,
                       p.chunked ? SQ_CHUNK : a.n, p.nchunks, a.alpha, 1.0 - a.alpha, a.threshold, start, ends, a.state, flags,
                       p.nwords, finish, a.produced);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <int MODE, bool RAMP>
int emit(const SquelchLaunch &a, const Plan &p, const u64 *flags, const SquelchEntry *entries, hipStream_t st)
{
    long long bx = ((long long)a.n + THREADS - 1) / THREADS;
    if (bx > MAX_BLOCKS_X) bx = MAX_BLOCKS_X;
    hipLaunchKernelGGL((sq_emit_kernel<MODE, RAMP>), dim3((unsigned)bx, (unsigned)a.nstreams), dim3(THREADS), 0, st, a.in, a.out,
                       flags, entries, a.state, a.n, p.nwords, a.ramp, a.gate ? 1 : 0, a.table);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

size_t squelch_scratch_bytes(bool fast, const SquelchLaunch &a) { return a.n > 0 ? plan(fast, a).total : 0; }
size_t squelch_tail_scratch_bytes(const SquelchLaunch &a) { return squelch_scratch_bytes(false, a); }

int squelch_launch(bool fast, const SquelchLaunch &a, void *scratch, hipStream_t st)
{
    if (a.n <= 0) return GRHIP_OK;
    const Plan p = plan(fast, a);
    char *sc = (char *)scratch;
    u64 *flags = (u64 *)(sc + p.flags_off);
    double *ends = (double *)(sc + p.ends_off), *start = (double *)(sc + p.start_off);
    const int finish = !p.ramp_path && !a.gate;
    int rc;
    if (p.chunked) {
        if ((rc = a.cc ? detect<true, true>(a, p, nullptr, ends, flags, 0, st) : detect<false, true>(a, p, nullptr, ends, flags, 0, st)))
            return rc;
        hipLaunchKernelGGL(sq_carry_kernel, dim3((a.nstreams + THREADS - 1) / THREADS), dim3(THREADS), 0, st, ends, start, a.state,
                           a.nstreams, p.nchunks, std::pow(1.0 - a.alpha, (double)SQ_CHUNK));
        GRHIP_HIP(hipGetLastError());
    }
    const double *from = p.chunked ? start : nullptr;
    if ((rc = a.cc ? detect<true, false>(a, p, from, nullptr, flags, finish, st) : detect<false, false>(a, p, from, nullptr, flags, finish, st)))
        return rc;
    return squelch_tail_launch(a, scratch, st);
}

// From the flag words at the head of `scratch` to the outputs.  Without a ramp and without gating there is nothing to
// walk: the detector that wrote the flags has stored the state (the last flag) and produced[s] = n itself.
int squelch_tail_launch(const SquelchLaunch &a, void *scratch, hipStream_t st)
{
    if (a.n <= 0) return GRHIP_OK;
    const Plan p = plan(false, a);
    char *sc = (char *)scratch;
    u64 *flags = (u64 *)(sc + p.flags_off);
    SquelchEntry *entries = (SquelchEntry *)(sc + p.entries_off);
    if (p.ramp_path) {
        hipLaunchKernelGGL(sq_walk_kernel, dim3(a.nstreams), dim3(WAVE), 0, st, flags, entries, a.state, a.produced, a.n, p.nwords,
                           a.ramp, a.gate ? 1 : 0, a.table);
        GRHIP_HIP(hipGetLastError());
        return a.cc ? emit<EMIT_CC, true>(a, p, flags, entries, st) : emit<EMIT_FF, true>(a, p, flags, entries, st);
    }
    if (a.gate) {
        hipLaunchKernelGGL(sq_scan_kernel, dim3(a.nstreams), dim3(WAVE), 0, st, flags, entries, a.state, a.produced, a.n, p.nwords);
        GRHIP_HIP(hipGetLastError());
    }
    if (a.simple) return emit<EMIT_COPY, false>(a, p, flags, entries, st);
    return a.cc ? emit<EMIT_CC, false>(a, p, flags, entries, st) : emit<EMIT_FF, false>(a, p, flags, entries, st);
}

}  // namespace grhip
