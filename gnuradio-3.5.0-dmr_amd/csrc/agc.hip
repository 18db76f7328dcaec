// agc.hip -- the gain loops gr_agc_cc, gr_agc_ff, gr_agc2_cc, gr_agc2_ff (general/gri_agc_cc.h:53-61,
// gri_agc_ff.h:51-57, gri_agc2_cc.h:54-76, gri_agc2_ff.h:55-75).
//
// Every block is out = in * g followed by an update of g from |out|: a serial recurrence over the samples.
//
// agc_walk_kernel<LAW, CC>: the recurrence as the reference writes it, every float operation rounded once, bit for bit.
//           One wavefront per stream (the form of pager_slicer_fb): the wave loads a window of samples
//           coalesced into LDS with the next window's loads in flight, every lane walks the recurrence out of LDS,
//           lane l keeps the gain in front of sample l of each group of 64 and forms that sample's output itself (the
//           same two products the walk formed), so the stores are coalesced.  This is GRHIP_MODE_GENERIC of all four
//           blocks and every mode of agc2_*, whose rate switches on a comparison with the gain.
//
// The chunked form of agc_cc / agc_ff (every other mode, calls longer than one chunk).  With g >= 0 a step is
// g' = min(a g + b, M), a = 1 - rate |x|, b = rate reference, and maps g -> min(A g + B, C) with A >= 0 compose:
//     min(a2 min(a1 g + b1, c1) + b2, c2) = min(a2 a1 g + a2 b1 + b2, min(a2 c1 + b2, c2)).
//   agc_ends_kernel   the triple (A, B, C) of every chunk of AGC_CHUNK samples from the identity, in double: a lane
//                     composes four consecutive samples of a coalesced load, an ordered tree over the wave finishes the
//                     chunk.  One flag per chunk: some sample with !(a >= 0) (rate |x| > 1, an infinity, a NaN).
//   agc_carry_kernel  one wavefront per stream over the chunks, 64 triples at a time through LDS: an unflagged chunk
//                     entered with g >= 0 is one application of its triple; a flagged one, or one entered with a
//                     negative (or NaN) gain, is walked sample by sample in the reference's float arithmetic.  Leaves
//                     every chunk's start gain, rounded to float.
//   agc_chunk_walk_kernel   one lane per chunk runs the reference's float steps from the chunk's start gain and writes
//                     the outputs; the lane of the last chunk writes the stream's gain.  A wavefront owns 64 consecutive
//                     chunks and moves them through LDS in pieces of 128 bytes per chunk, so that global loads and
//                     stores use whole lines (eight lanes to a line) while a lane reads and writes its own row; rows
//                     are padded by 16 bytes, which spreads the 64 rows' b128 accesses over all banks.
#include <cmath>

#include "agc.h"

namespace grhip {

namespace {

constexpr double AGC_INF = __builtin_huge_val();

template <bool CC>
__device__ __forceinline__ float agc_mag(float o_re, float o_im)
{
    if (CC) return sqrtf(__fadd_rn(__fmul_rn(o_re, o_re), __fmul_rn(o_im, o_im)));      // gri_agc_cc.h:56-57
    return fabsf(o_re);                                                                  // gri_agc_ff.h:53
}

// one scale() of the reference on the gain; (x_re, x_im) is the input sample
template <int LAW, bool CC>
__device__ __forceinline__ void agc_step(float &g, float x_re, float x_im, const AgcParams &p)
{
    const float m = agc_mag<CC>(__fmul_rn(x_re, g), CC ? __fmul_rn(x_im, g) : 0.f);
    if (LAW == AGC_LAW_AGC) {
        g = __fadd_rn(g, __fmul_rn(p.rate, __fsub_rn(p.reference, m)));                  // gri_agc_cc.h:56, gri_agc_ff.h:53
    } else {
        float tmp;
        bool attack;
        if (CC) {
            tmp = __fadd_rn(-p.reference, m);                                            // gri_agc2_cc.h:57
            attack = tmp > g;                                                            // :60
        } else {
            tmp = __fsub_rn(m, p.reference);                                             // gri_agc2_ff.h:58
            attack = fabsf(tmp) > g;                                                     // :60
        }
        g = __fsub_rn(g, __fmul_rn(tmp, attack ? p.rate : p.decay));                     // gri_agc2_cc.h:62
        if (g < 0.0f) g = (float)10e-5;                                                  // :70-71
    }
    if (p.max_gain > 0.0f && g > p.max_gain) g = p.max_gain;                             // gri_agc_cc.h:58-59
}

// ---- the serial walk ---------------------------------------------------------------------------------------------
constexpr int AGC_WIN = 1024;

template <int LAW, bool CC>
__global__ void __launch_bounds__(64)
agc_walk_kernel(const float *__restrict__ in, float *__restrict__ out, long long n, float *__restrict__ gain, AgcParams p)
{
    constexpr int F = CC ? 2 : 1;
    __shared__ float s_x[AGC_WIN * F];
    const int s = blockIdx.x, lane = threadIdx.x;
    const float *__restrict__ x = in + (long long)s * n * F;
    float *__restrict__ y = out + (long long)s * n * F;
    float g = gain[s];
    float v[AGC_WIN / 64][F];
#pragma unroll
    for (int q = 0; q < AGC_WIN / 64; ++q) {
        const long long i = lane + 64 * q;
#pragma unroll
        for (int e = 0; e < F; ++e) v[q][e] = i < n ? x[i * F + e] : 0.f;
    }
    for (long long base = 0; base < n; base += AGC_WIN) {
        const int m = (int)(n - base < AGC_WIN ? n - base : AGC_WIN);
#pragma unroll
        for (int q = 0; q < AGC_WIN / 64; ++q)
#pragma unroll
            for (int e = 0; e < F; ++e) s_x[(lane + 64 * q) * F + e] = v[q][e];
        __syncthreads();
        // the next window's loads, in flight while this one is walked
#pragma unroll
        for (int q = 0; q < AGC_WIN / 64; ++q) {
            const long long i = base + AGC_WIN + lane + 64 * q;
#pragma unroll
            for (int e = 0; e < F; ++e) v[q][e] = i < n ? x[i * F + e] : 0.f;
        }
        for (int g0 = 0; g0 < m; g0 += 64) {
            const int cnt = m - g0 < 64 ? m - g0 : 64;
            float kg = g;
            if (cnt == 64) {
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    kg = lane == j ? g : kg;
                    agc_step<LAW, CC>(g, s_x[(g0 + j) * F], CC ? s_x[(g0 + j) * F + F - 1] : 0.f, p);
                }
            } else {
                for (int j = 0; j < cnt; ++j) {
                    kg = lane == j ? g : kg;
                    agc_step<LAW, CC>(g, s_x[(g0 + j) * F], CC ? s_x[(g0 + j) * F + F - 1] : 0.f, p);
                }
            }
            if (lane < cnt) {
                const long long i = base + g0 + lane;
#pragma unroll
                for (int e = 0; e < F; ++e) y[i * F + e] = __fmul_rn(s_x[(g0 + lane) * F + e], kg);   // gri_agc_cc.h:54
            }
        }
        __syncthreads();
    }
    if (lane == 0) gain[s] = g;
}

// ---- the chunked form --------------------------------------------------------------------------------------------
// NF floats from p + fo in units of UF floats (UF = 4 needs p + fo 16-byte aligned), zeros at and past nf
template <int UF, int NF>
__device__ __forceinline__ void agc_load(float (&d)[NF], const float *__restrict__ p, long long fo, long long nf)
{
    static_assert(NF % UF == 0, "whole units");
#pragma unroll
    for (int u = 0; u < NF; u += UF) {
        if (fo + u + UF <= nf) {
            if (UF == 4) {
                const float4 t = *reinterpret_cast<const float4 *>(p + fo + u);
                d[u] = t.x; d[u + 1] = t.y; d[u + 2] = t.z; d[u + 3] = t.w;
            } else if (UF == 2) {
                const float2 t = *reinterpret_cast<const float2 *>(p + fo + u);
                d[u] = t.x; d[u + 1] = t.y;
            } else {
                d[u] = p[fo + u];
            }
        } else {
#pragma unroll
            for (int e = 0; e < UF; ++e) d[u + e] = fo + u + e < nf ? p[fo + u + e] : 0.f;
        }
    }
}

template <int UF, int NF>
__device__ __forceinline__ void agc_store(const float (&d)[NF], float *__restrict__ p, long long fo, long long nf)
{
#pragma unroll
    for (int u = 0; u < NF; u += UF) {
        if (fo + u + UF <= nf) {
            if (UF == 4) *reinterpret_cast<float4 *>(p + fo + u) = make_float4(d[u], d[u + 1], d[u + 2], d[u + 3]);
            else if (UF == 2) *reinterpret_cast<float2 *>(p + fo + u) = make_float2(d[u], d[u + 1]);
            else p[fo + u] = d[u];
        } else {
#pragma unroll
            for (int e = 0; e < UF; ++e)
                if (fo + u + e < nf) p[fo + u + e] = d[u + e];
        }
    }
}

struct AgcTriple {
    double A, B, C;         // g -> min(A g + B, C); C = +inf: no clamp
};

// `f` first, then `s`
__device__ __forceinline__ AgcTriple agc_compose(const AgcTriple &f, const AgcTriple &s)
{
    AgcTriple r;
    r.A = s.A * f.A;
    r.B = s.A * f.B + s.B;
    const double c = f.C == AGC_INF ? AGC_INF : s.A * f.C + s.B;      // 0 * inf never formed
    r.C = c < s.C ? c : s.C;
    return r;
}

// One wavefront per chunk at a time.  tri = [3][total] doubles, flag = [total] bytes, total = S * nch.
template <bool CC, int UF>
__global__ void __launch_bounds__(256)
agc_ends_kernel(const float *__restrict__ in, long long n, int nch, long long total, double rate, double b, double M,
                double *__restrict__ tri, unsigned char *__restrict__ flag)
{
    constexpr int F = CC ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const long long nw = (long long)gridDim.x * 4;
    for (long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); q < total; q += nw) {
        const long long s = q / nch;
        const int c = (int)(q - s * nch);
        const long long i0 = (long long)c * AGC_CHUNK + lane * 4;
        float f[4 * F];
        agc_load<UF, 4 * F>(f, in + s * n * F, i0 * F, n * F);
        AgcTriple t = {1.0, 0.0, AGC_INF};
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < n) {
                const double re = f[k * F], im = CC ? f[k * F + F - 1] : 0.0;
                const double mag = CC ? sqrt(re * re + im * im) : fabs(re);
                const double a = 1.0 - rate * mag;
                bad = bad || !(a >= 0.0);
                const AgcTriple st = {a, b, M};
                t = agc_compose(t, st);
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d *= 2) {
            AgcTriple o;
            o.A = __shfl_down(t.A, d);
            o.B = __shfl_down(t.B, d);
            o.C = __shfl_down(t.C, d);
            if (!(lane & (2 * d - 1))) t = agc_compose(t, o);
        }
        const bool any = __any(bad);
        if (lane == 0) {
            tri[q] = t.A;
            tri[total + q] = t.B;
            tri[2 * total + q] = t.C;
            flag[q] = any ? 1 : 0;
        }
    }
}

template <bool CC>
__global__ void __launch_bounds__(64)
agc_carry_kernel(const float *__restrict__ in, long long n, int nch, long long total, const double *__restrict__ tri,
                 const unsigned char *__restrict__ flag, const float *__restrict__ gain, float *__restrict__ start,
                 AgcParams p)
{
    constexpr int F = CC ? 2 : 1;
    __shared__ double s_A[64], s_B[64], s_C[64];
    __shared__ int s_f[64];
    const int s = blockIdx.x, lane = threadIdx.x;
    const long long o = (long long)s * nch;
    const float *__restrict__ x = in + (long long)s * n * F;
    double g = (double)gain[s];
    double a = 1.0, b = 0.0, c = AGC_INF;
    int f = 0;
    if (lane < nch) { a = tri[o + lane]; b = tri[total + o + lane]; c = tri[2 * total + o + lane]; f = flag[o + lane]; }
    for (int base = 0; base < nch; base += 64) {
        s_A[lane] = a; s_B[lane] = b; s_C[lane] = c; s_f[lane] = f;
        __syncthreads();
        if ((long long)base + 64 + lane < nch) {
            const long long k = o + base + 64 + lane;
            a = tri[k]; b = tri[total + k]; c = tri[2 * total + k]; f = flag[k];
        }
        const int cnt = nch - base < 64 ? nch - base : 64;
        float kg = 0.f;
        for (int j = 0; j < cnt; ++j) {
            kg = lane == j ? (float)g : kg;
            if (!s_f[j] && g >= 0.0) {
                const double t = s_A[j] * g + s_B[j];
                g = t > s_C[j] ? s_C[j] : t;
            } else {
                float gf = (float)g;
                const long long i0 = (long long)(base + j) * AGC_CHUNK;
                const long long i1 = i0 + AGC_CHUNK < n ? i0 + AGC_CHUNK : n;
                for (long long i = i0; i < i1; ++i) agc_step<AGC_LAW_AGC, CC>(gf, x[i * F], CC ? x[i * F + F - 1] : 0.f, p);
                g = (double)gf;
            }
        }
        if (lane < cnt) start[o + base + lane] = kg;
        __syncthreads();
    }
}

constexpr int AGC_ROW = 32;             // floats of one chunk in one piece: 128 bytes
constexpr int AGC_ROW_PAD = AGC_ROW + 4;

// One wavefront per 64 consecutive chunks of a stream: grid (ceil(nch / 64), S).
template <bool CC, int UF>
__global__ void __launch_bounds__(64)
agc_chunk_walk_kernel(const float *__restrict__ in, float *__restrict__ out, long long n, int nch,
                      const float *__restrict__ start, float *__restrict__ gain, AgcParams p)
{
    constexpr int F = CC ? 2 : 1;
    constexpr int IPP = AGC_ROW / F;                    // items of a chunk per piece
    constexpr int PIECES = AGC_CHUNK / IPP;
    constexpr int UR = AGC_ROW / UF;                    // load units per row, and per lane and piece
    __shared__ __attribute__((aligned(16))) float s_row[64 * AGC_ROW_PAD];
    const int lane = threadIdx.x, s = blockIdx.y;
    const int cbase = blockIdx.x * 64;
    const int c = cbase + lane;
    const float *__restrict__ x = in + (long long)s * n * F;
    float *__restrict__ y = out + (long long)s * n * F;
    const long long nf = n * F;
    // items of this lane's chunk (0: no such chunk)
    long long left = n - (long long)c * AGC_CHUNK;
    const int mine = c < nch ? (int)(left < AGC_CHUNK ? left : AGC_CHUNK) : 0;
    float g = c < nch ? start[(long long)s * nch + c] : 0.f;

    // unit k of this lane in a piece: row (k * 64 + lane) / UR, unit (k * 64 + lane) % UR of that row
    float v[UR][UF];
    auto fetch = [&](int piece) {
#pragma unroll
        for (int k = 0; k < UR; ++k) {
            const int t = k * 64 + lane, row = t / UR, col = t % UR;
            const long long fo = ((long long)(cbase + row) * AGC_CHUNK + (long long)piece * IPP) * F + col * UF;
            agc_load<UF, UF>(v[k], x, fo, nf);
        }
    };
    fetch(0);
    for (int piece = 0; piece < PIECES; ++piece) {
#pragma unroll
        for (int k = 0; k < UR; ++k) {
            const int t = k * 64 + lane, row = t / UR, col = t % UR;
#pragma unroll
            for (int e = 0; e < UF; ++e) s_row[row * AGC_ROW_PAD + col * UF + e] = v[k][e];
        }
        __syncthreads();
        if (piece + 1 < PIECES) fetch(piece + 1);
        {   // this lane's row: IPP items in order
            float r[AGC_ROW];
#pragma unroll
            for (int u = 0; u < AGC_ROW; u += 4) {
                const float4 t = *reinterpret_cast<const float4 *>(&s_row[lane * AGC_ROW_PAD + u]);
                r[u] = t.x; r[u + 1] = t.y; r[u + 2] = t.z; r[u + 3] = t.w;
            }
            const int valid = mine - piece * IPP;
#pragma unroll
            for (int j = 0; j < IPP; ++j) {
                const float x_re = r[j * F], x_im = CC ? r[j * F + F - 1] : 0.f;
                r[j * F] = __fmul_rn(x_re, g);                                              // gri_agc_cc.h:54
                if (CC) r[j * F + F - 1] = __fmul_rn(x_im, g);
                float gn = g;
                agc_step<AGC_LAW_AGC, CC>(gn, x_re, x_im, p);
                g = j < valid ? gn : g;
            }
#pragma unroll
            for (int u = 0; u < AGC_ROW; u += 4)
                *reinterpret_cast<float4 *>(&s_row[lane * AGC_ROW_PAD + u]) = make_float4(r[u], r[u + 1], r[u + 2], r[u + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < UR; ++k) {
            const int t = k * 64 + lane, row = t / UR, col = t % UR;
            const long long fo = ((long long)(cbase + row) * AGC_CHUNK + (long long)piece * IPP) * F + col * UF;
            float w[UF];
#pragma unroll
            for (int e = 0; e < UF; ++e) w[e] = s_row[row * AGC_ROW_PAD + col * UF + e];
            agc_store<UF, UF>(w, y, fo, nf);
        }
        __syncthreads();
    }
    if (c == nch - 1) gain[s] = g;
}

inline int agc_chunks(int n) { return (n + AGC_CHUNK - 1) / AGC_CHUNK; }

template <int LAW, bool CC>
int walk_launch(const AgcLaunch &a, hipStream_t st)
{
    hipLaunchKernelGGL((agc_walk_kernel<LAW, CC>), dim3(a.nstreams), dim3(64), 0, st, (const float *)a.in, (float *)a.out,
                       (long long)a.n, a.gain, a.p);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <bool CC, int UF>
int chunked_launch(const AgcLaunch &a, void *scratch, hipStream_t st)
{
    const int nch = agc_chunks(a.n);
    const long long total = (long long)a.nstreams * nch;
    double *tri = (double *)scratch;
    float *start = (float *)(tri + 3 * total);
    unsigned char *flag = (unsigned char *)(start + total);
    const float *in = (const float *)a.in;
    const double M = a.p.max_gain > 0.0f ? (double)a.p.max_gain : AGC_INF;
    const double b = (double)a.p.rate * (double)a.p.reference;
    long long blocks = (total + 3) / 4;
    const long long cap = (long long)device_cus() * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((agc_ends_kernel<CC, UF>), dim3((unsigned)blocks), dim3(256), 0, st, in, (long long)a.n, nch, total,
                       (double)a.p.rate, b, M, tri, flag);
    GRHIP_HIP(hipGetLastError());
    hipLaunchKernelGGL((agc_carry_kernel<CC>), dim3(a.nstreams), dim3(64), 0, st, in, (long long)a.n, nch, total, tri, flag,
                       a.gain, start, a.p);
    GRHIP_HIP(hipGetLastError());
    hipLaunchKernelGGL((agc_chunk_walk_kernel<CC, UF>), dim3((nch + 63) / 64, a.nstreams), dim3(64), 0, st, in,
                       (float *)a.out, (long long)a.n, nch, start, a.gain, a.p);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

inline bool aligned16(const void *p) { return !((uintptr_t)p & 15); }

}  // namespace

bool agc_can_chunk(const AgcLaunch &a)
{
    return a.law == AGC_LAW_AGC && a.n > AGC_CHUNK && std::isfinite(a.p.rate) && std::isfinite(a.p.reference) &&
           std::isfinite(a.p.max_gain) && a.p.rate >= 0.0f && a.p.reference >= 0.0f;
}

size_t agc_scratch_bytes(const AgcLaunch &a)
{
    const size_t total = (size_t)a.nstreams * agc_chunks(a.n);
    return total * (3 * sizeof(double) + sizeof(float) + 1);
}

int agc_launch(bool chunked, const AgcLaunch &a, void *scratch, hipStream_t st)
{
    if (a.n <= 0 || a.nstreams <= 0) return GRHIP_OK;
    if (chunked) {
        if (!agc_can_chunk(a) || !scratch) return fail(GRHIP_EINVAL, "agc: the chunked form cannot take this call");
        // 16-byte units where every stream starts on a 16-byte boundary, else one item at a time
        const int fpi = a.cc ? 2 : 1;
        const bool wide = aligned16(a.in) && aligned16(a.out) && (a.nstreams == 1 || ((long long)a.n * fpi) % 4 == 0);
        if (a.cc) return wide ? chunked_launch<true, 4>(a, scratch, st) : chunked_launch<true, 2>(a, scratch, st);
        return wide ? chunked_launch<false, 4>(a, scratch, st) : chunked_launch<false, 1>(a, scratch, st);
    }
    if (a.law == AGC_LAW_AGC) return a.cc ? walk_launch<AGC_LAW_AGC, true>(a, st) : walk_launch<AGC_LAW_AGC, false>(a, st);
    return a.cc ? walk_launch<AGC_LAW_AGC2, true>(a, st) : walk_launch<AGC_LAW_AGC2, false>(a, st);
}

}  // namespace grhip
