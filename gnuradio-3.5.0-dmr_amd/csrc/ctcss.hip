// ctcss.hip -- the detector of gr_ctcss_squelch_ff (general/gr_ctcss_squelch_ff.cc:97-112, filter/gri_goertzel.cc:60-75).
// The machine behind it is squelch.hip's (gr_squelch_base_ff.cc:42-93), reached through squelch_tail_launch.
//
// Per call, with p samples of an unfinished block carried per stream and n new ones:
//   detect  every block that completes in the call, (p + n) / len of them per stream, is evaluated whole and from a zero
//           start: sample v of the stream's carry followed by its new samples is carry[v] for v < p and in[v - p] from
//           there on (only the first block reaches into the carry).  The three filters share every sample load.
//             GENERIC  one lane per (stream, block) runs the three float recurrences y = (x + wr d1) - d2 in the
//                      reference's order; GZ_ROWS blocks per workgroup, GZ_CH samples of each staged into LDS per pass with
//                      coalesced loads, the row stride odd (analytic.hip's goertzel_generic_kernel, three filters wide).
//             FAST     the closed form out = sum_n x[n] tab[n] against the three tables (analytic.h), a block dealt to a
//                      wave (four blocks at a time, so a table entry is loaded once for four samples), from GZ_WG_LEN
//                      samples on to a workgroup; the reduction order is fixed.
//           Then |l|, |c|, |r| as (float)sqrt((double)re re + (double)im im) and the decision c < level || c < l || c < r,
//           one byte per block.
//   flags   one lane per 64-bit word expands the decisions: sample i takes that of completed block (i + p + 1) / len,
//           counted from 1, or the carried one for 0.  The same grid stores the new tail of every stream into the carry.
//   finish  one lane per stream keeps the last decision; without ramp and gating it also stores the state and the count.
// Every step of GENERIC and of the decision is written with the round-to-nearest intrinsics: none can be contracted.
#include "analytic.h"
#include "ctcss.h"

namespace grhip {

namespace {

constexpr int THREADS = 256;
constexpr long long MAX_GRID = 65536;             // flags: grid-stride from here on
typedef unsigned long long u64;
typedef unsigned char u8;

struct DetectArgs {
    const float *in;            // [S][n]
    const float *carry;         // [S][len]
    const float2 *tab;          // [3][len] (FAST)
    u8 *dec;                    // [S][nb]
    float *mags;                // [S][nb][3]
    long long nb;               // blocks that complete per stream
    int n, len, p;
    float level;
    float wr[3], wi[3];
};

// std::abs(gr_complex) is hypotf, which (finite arguments) is this: the squares are exact in double
__device__ inline float ctcss_abs(float re, float im)
{
    const double x = (double)re, y = (double)im;
    return (float)__dsqrt_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)));
}

// gr_ctcss_squelch_ff.cc:105-110; a NaN level compares false and never mutes
__device__ inline void ctcss_decide(const DetectArgs &k, int s, long long b, const float re[3], const float im[3])
{
    const float l = ctcss_abs(re[0], im[0]), c = ctcss_abs(re[1], im[1]), r = ctcss_abs(re[2], im[2]);
    const long long at = (long long)s * k.nb + b;
    k.dec[at] = (c < k.level || c < l || c < r) ? 1 : 0;
    k.mags[at * 3 + 0] = l;
    k.mags[at * 3 + 1] = c;
    k.mags[at * 3 + 2] = r;
}

__global__ void __launch_bounds__(GZ_ROWS) ctcss_generic_kernel(DetectArgs k)
{
    __shared__ float rows[GZ_ROWS * (GZ_CH + 1)];
    const int t = threadIdx.x, s = blockIdx.y;
    const long long b0 = (long long)blockIdx.x * GZ_ROWS;
    const int nrows = (int)(k.nb - b0 < GZ_ROWS ? k.nb - b0 : GZ_ROWS);
    const float *in = k.in + (long long)s * k.n, *carry = k.carry + (long long)s * k.len;
    float d1[3] = {0.f, 0.f, 0.f}, d2[3] = {0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < k.len; i0 += GZ_CH) {
        const int cols = k.len - i0 < GZ_CH ? k.len - i0 : GZ_CH;
        const int total = nrows * cols;
        for (int e = t; e < total; e += GZ_ROWS) {
            const int row = e / cols, col = e - row * cols;
            const long long v = (b0 + row) * k.len + i0 + col;
            rows[row * (GZ_CH + 1) + col] = v < k.p ? carry[v] : in[v - k.p];
        }
        __syncthreads();
        if (t < nrows) {
            const float *x = rows + t * (GZ_CH + 1);
            for (int i = 0; i < cols; ++i) {
                const float xi = x[i];
#pragma unroll
                for (int f = 0; f < 3; ++f) {
                    const float y = __fsub_rn(__fadd_rn(xi, __fmul_rn(k.wr[f], d1[f])), d2[f]);     // gri_goertzel.cc:62
                    d2[f] = d1[f];
                    d1[f] = y;
                }
            }
        }
        __syncthreads();
    }
    if (t < nrows) {
        float re[3], im[3];
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            // gri_goertzel.cc:70: (0.5*d_wr*d_d1-d_d2)/d_len in double, (d_wi*d_d1)/d_len in float, both stored to float
            re[f] = (float)__ddiv_rn(__dsub_rn(__dmul_rn(__dmul_rn(0.5, (double)k.wr[f]), (double)d1[f]), (double)d2[f]), (double)k.len);
            im[f] = __fdiv_rn(__fmul_rn(k.wi[f], d1[f]), (float)k.len);
        }
        ctcss_decide(k, s, b0 + t, re, im);
    }
}

__device__ __forceinline__ float wave_sum_xor(float v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// goertzel_fast_kernel (analytic.hip) three tones wide.  A table entry is three float2, six times the bytes of the sample
// it multiplies, so a wave takes FAST_NB consecutive blocks of a stream at once and every entry it loads meets FAST_NB
// samples (a workgroup: one block, as few long blocks have to fill the device).  A lane sums its positions n = first,
// first + step, ... of a block in that order into one accumulator per tone and part, whatever else the wave carries.
constexpr int FAST_NB = 4;

template <bool WG>
__global__ void __launch_bounds__(256) ctcss_fast_kernel(DetectArgs k)
{
    constexpr int NB = WG ? 1 : FAST_NB;
    __shared__ float part[4][6];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, s = blockIdx.y;
    const long long b0 = WG ? (long long)blockIdx.x : ((long long)blockIdx.x * 4 + wave) * NB;
    float acc[NB][6];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[j][c] = 0.f;
    if (b0 < k.nb) {                                         // wave-uniform
        const float *in = k.in + (long long)s * k.n, *carry = k.carry + (long long)s * k.len;
        const int len = k.len, step = WG ? 256 : 64;
#pragma unroll 2
        for (int n = WG ? t : lane; n < len; n += step) {
            float x[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const long long v = (b0 + j) * len + n;
                x[j] = b0 + j < k.nb ? (v < k.p ? carry[v] : in[v - k.p]) : 0.f;
            }
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                const float2 p = k.tab[(long long)f * len + n];
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    acc[j][2 * f] = __builtin_fmaf(x[j], p.x, acc[j][2 * f]);
                    acc[j][2 * f + 1] = __builtin_fmaf(x[j], p.y, acc[j][2 * f + 1]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[j][c] = wave_sum_xor(acc[j][c]);
    if (!WG) {
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (b0 + j < k.nb) {
                    const float re[3] = {acc[j][0], acc[j][2], acc[j][4]}, im[3] = {acc[j][1], acc[j][3], acc[j][5]};
                    ctcss_decide(k, s, b0 + j, re, im);
                }
            }
        }
        return;
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) part[wave][c] = acc[0][c];
    }
    __syncthreads();
    if (t == 0) {
        float v[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
        const float re[3] = {v[0], v[2], v[4]}, im[3] = {v[1], v[3], v[5]};
        ctcss_decide(k, s, b0, re, im);
    }
}

// Flag words, then the carry.  With nb > 0 the new tail is in[nb len - p, n), stored from carry[0]; with nb == 0 the
// call's n samples are appended at carry[p] (p + n < len).  The detector ran in the kernel before: nobody reads the
// carry here.
__global__ void __launch_bounds__(THREADS)
ctcss_flags_kernel(const float *in, float *carry, const u8 *mute, const u8 *dec, u64 *flags, int n, int S, int len, int p,
                   long long nb, int nwords)
{
    const long long id = blockIdx.x * (long long)THREADS + threadIdx.x, stride = (long long)gridDim.x * THREADS;
    for (long long w = id; w < (long long)S * nwords; w += stride) {
        const int s = (int)(w / nwords);
        const long long first = (w - (long long)s * nwords) * 64, end = first + 64 < n ? first + 64 : n;
        const bool carried = mute[s] != 0;
        u64 bits = 0;
        for (long long i = first; i < end;) {
            const long long blk = (i + p + 1) / len;                 // blocks complete once sample i has gone in
            long long e = (blk + 1) * len - p - 1;                   // the first sample that sees the next decision
            if (e > end) e = end;
            if (blk ? dec[(long long)s * nb + blk - 1] != 0 : carried) {
                const int cnt = (int)(e - i);
                bits |= (cnt == 64 ? ~0ull : (1ull << cnt) - 1) << (int)(i - first);
            }
            i = e;
        }
        flags[w] = bits;
    }
    const long long src = nb ? nb * len - p : 0, dst = nb ? 0 : p, cnt = n - src;
    for (long long e = id; e < (long long)S * cnt; e += stride) {
        const long long s = e / cnt, j = e - s * cnt;
        carry[s * len + dst + j] = in[s * n + src + j];
    }
}

// the last decision of the call is d_mute from here on; `finish` (no ramp, no gating): the state is the last flag and
// every sample produces an item (what sq_detect_kernel's finish does for the power squelch)
__global__ void __launch_bounds__(THREADS)
ctcss_finish_kernel(u8 *mute, const u8 *dec, long long nb, SquelchState *state, int *produced, int n, int S, int finish)
{
    const int s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= S) return;
    if (nb) mute[s] = dec[(long long)s * nb + nb - 1];
    if (finish) {
        state[s].state = mute[s] ? SQ_MUTED : SQ_UNMUTED;
        produced[s] = n;
    }
}

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

size_t ctcss_magnitudes_offset(const CtcssLaunch &c, const SquelchLaunch &a)
{
    return align_up(squelch_tail_scratch_bytes(a)) + align_up((size_t)a.nstreams * (size_t)ctcss_blocks(c, a.n));
}

size_t ctcss_scratch_bytes(const CtcssLaunch &c, const SquelchLaunch &a)
{
    return ctcss_magnitudes_offset(c, a) + (size_t)a.nstreams * (size_t)ctcss_blocks(c, a.n) * 3 * sizeof(float);
}

int ctcss_launch(bool fast, const CtcssLaunch &c, const SquelchLaunch &a, void *scratch, hipStream_t st)
{
    if (a.n <= 0) return GRHIP_OK;
    if (c.len < 1 || c.len > CTCSS_MAX_LEN || c.pending < 0 || c.pending >= c.len || a.nstreams < 1 || a.nstreams > 65535)
        return fail(GRHIP_EINVAL, "ctcss: bad launch");
    const long long nb = ctcss_blocks(c, a.n);
    const int S = a.nstreams, nwords = (int)(((long long)a.n + 63) / 64);
    char *sc = (char *)scratch;
    u64 *flags = (u64 *)sc;
    u8 *dec = (u8 *)(sc + align_up(squelch_tail_scratch_bytes(a)));
    float *mags = (float *)(sc + ctcss_magnitudes_offset(c, a));
    if (nb > 0) {
        DetectArgs k;
        k.in = (const float *)a.in; k.carry = c.carry; k.tab = c.tab; k.dec = dec; k.mags = mags; k.nb = nb;
        k.n = a.n; k.len = c.len; k.p = c.pending; k.level = c.level;
        for (int f = 0; f < 3; ++f) { k.wr[f] = c.wr[f]; k.wi[f] = c.wi[f]; }
        if (!fast) {
            hipLaunchKernelGGL(ctcss_generic_kernel, dim3((unsigned)((nb + GZ_ROWS - 1) / GZ_ROWS), S), dim3(GZ_ROWS), 0, st, k);
        } else {
            if (!c.tab) return fail(GRHIP_EINVAL, "ctcss: no tables");
            if (c.len >= GZ_WG_LEN) hipLaunchKernelGGL(ctcss_fast_kernel<true>, dim3((unsigned)nb, S), dim3(256), 0, st, k);
            else hipLaunchKernelGGL(ctcss_fast_kernel<false>, dim3((unsigned)((nb + 4 * FAST_NB - 1) / (4 * FAST_NB)), S), dim3(256), 0, st, k);
        }
        GRHIP_HIP(hipGetLastError());
    }
    const long long tail = nb ? ((long long)c.pending + a.n) % c.len : a.n;
    const long long most = (long long)S * (nwords > tail ? nwords : tail);
    long long blocks = (most + THREADS - 1) / THREADS;
    if (blocks > MAX_GRID) blocks = MAX_GRID;
    hipLaunchKernelGGL(ctcss_flags_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, (const float *)a.in, c.carry, c.mute, dec, flags,
                       a.n, S, c.len, c.pending, nb, nwords);
    GRHIP_HIP(hipGetLastError());
    const int finish = a.ramp == 0 && !a.gate;
    if (nb > 0 || finish) {
        hipLaunchKernelGGL(ctcss_finish_kernel, dim3((S + THREADS - 1) / THREADS), dim3(THREADS), 0, st, c.mute, dec, nb, a.state,
                           a.produced, a.n, S, finish);
        GRHIP_HIP(hipGetLastError());
    }
    return squelch_tail_launch(a, scratch, st);
}

}  // namespace grhip
