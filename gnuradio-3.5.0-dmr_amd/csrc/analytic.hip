// analytic.hip -- kernels of gr_hilbert_fc / gr_filter_delay_fc (filter/gr_hilbert_fc.cc:57-66,
// filter/gr_filter_delay_fc.cc:57-79) and gr_goertzel_fc (filter/gr_goertzel_fc.cc:48-60, filter/gri_goertzel.cc:36-75).
//
// analytic_generic_kernel: one output per lane, the taps in LDS.  The imaginary part is fir_fff_generic_sum
//   (device_math.h) -- gr_fir_fff_generic's order over ALL taps, zeros included, the code fir_filter_fff's generic
//   kernel runs -- the real part a copy of in0[n + delay]; one packed float2 store.  Bit-exact.
//
// analytic_tile_kernel<SPARSE, TWO_IN>: FAST.  One workgroup = AN_NT consecutive outputs, AN_R per lane.  The tile's
//   input and its halo are staged into LDS once with 16-byte loads that are aligned in memory, not to the stream (items
//   are only 4-byte aligned; the chunk at either end that reaches outside the stream is read item by item), one pad
//   slot per 8 samples: the lane stride is 9 slots, conflict-free.  Each lane slides a 16-sample register window over
//   its samples, so one LDS read feeds 8 FMAs (dense) or 4 subtract-FMA pairs (sparse).  The taps are wave-uniform
//   and come through scalar loads.
//     SPARSE: taps of odd length, zero at even distance from the centre and exactly antisymmetric (the host checks):
//             imag[n] = sum over odd i of t[h + i] (x[c - i] - x[c + i]), c = n + h -- a quarter of the multiplies.
//             The real part x[c] is taken from the same staged tile: every input is read from HBM once.
//     dense : imag[n] = sum_k taps_rev[k] in1[n + k], every tap; the delayed sample is joined in the epilogue, from
//             the staged tile (one input) or from in0 (TWO_IN).  No float plane in HBM, no second kernel.
//
// goertzel_generic_kernel: one lane per block.  A workgroup (one wave) owns GZ_ROWS consecutive blocks and brings
//   GZ_CH samples of each into LDS per pass with coalesced loads (consecutive lanes read consecutive floats of a row);
//   each lane then walks its own row.  The row stride is GZ_CH + 1 slots (odd), so the lanes sit on different banks
//   whatever the block length.  y = (x + wr d1) - d2 unfused, the real part of the result formed in double, the
//   imaginary part in float, as gri_goertzel::output does.  Bit-exact.
// goertzel_fast_kernel<WG>: the recurrence in closed form, out = sum_n x[n] tab[n] (analytic.h), the samples of a
//   block dealt to the lanes of a wave (WG = false) or of the whole workgroup (WG = true, long blocks: few blocks
//   still fill the device).  Fixed reduction order: the result does not depend on the launch.
#include <cstdint>

#include "analytic.h"
#include "device_math.h"
#include "grhip_internal.h"

namespace grhip {

namespace {

constexpr int AN_PADL = 8;                      // logical samples in front of the tile (the sparse window looks back)
constexpr int AN_SLACK = 24;                    // ... and behind its halo (the windows are refilled 16 at a time)
__host__ __device__ constexpr int an_slot(int m) { return m + (m >> 3); }
__host__ __device__ constexpr int an_staged(int ntaps) { return AN_PADL + AN_NT + (ntaps - 1) + AN_SLACK; }

__global__ void __launch_bounds__(256) analytic_generic_kernel(AnalyticLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) float an_taps[];
    for (int i = threadIdx.x; i < a.ntaps; i += blockDim.x) an_taps[i] = a.taps_rev[i];
    __syncthreads();
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.n_out) return;
    const float im = fir_fff_generic_sum(an_taps, a.in1 + n, a.ntaps);
    a.out[n] = make_float2(a.in0[n + a.delay], im);
}

template <bool SPARSE, bool TWO_IN>
__global__ void __launch_bounds__(AN_THREADS) analytic_tile_kernel(AnalyticLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * AN_NT;
    const long long n_in = a.n_out + a.ntaps - 1;            // readable items of in1
    const int S = an_staged(a.ntaps);

    // ---- stage logical sample m <-> in1[t0 - AN_PADL + m]; what lies outside the stream is zero -------------------
    {
        const long long g0 = t0 - AN_PADL;                                        // item of logical sample 0
        const long long unit = (long long)(((uintptr_t)a.in1) >> 2) + g0;         // its address in 4-byte units
        const int lead = (int)(unit & 3);
        const int nch = (S + lead + 3) >> 2;
        for (int c = tid; c < nch; c += AN_THREADS) {
            const int m0 = 4 * c - lead;
            const long long gi = g0 + m0;
            float v[4];
            if (gi >= 0 && gi + 4 <= n_in) {
                const float4 f = *reinterpret_cast<const float4 *>(a.in1 + gi);   // 16-byte aligned by construction
                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (gi + e >= 0 && gi + e < n_in) ? a.in1[gi + e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = m0 + e;
                if (m >= 0 && m < S) xs[an_slot(m)] = v[e];
            }
        }
    }
    __syncthreads();

    const int o = tid * AN_R;
    float acc[AN_R], re[AN_R];
#pragma unroll
    for (int r = 0; r < AN_R; ++r) acc[r] = 0.f;

    if (SPARSE) {
        const int h = a.ntaps >> 1;
        const int A = AN_PADL + o + h;                       // logical place of the centre of output o
        float wl[16], wr[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            wl[j] = xs[an_slot(A - 8 + j)];
            wr[j] = xs[an_slot(A + j)];
        }
#pragma unroll
        for (int r = 0; r < AN_R; ++r) re[r] = wr[r];        // x[c]: the delayed sample
        const int G = (a.nodd + 3) >> 2;
        for (int g = 0; g < G; ++g) {
            // odd distances i = 8g + 2q + 1: x[c_r - i] = wl[r + 7 - 2q], x[c_r + i] = wr[r + 2q + 1]
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = 4 * g + q;
                if (m < a.nodd) {
                    const float c = a.odd[m];
#pragma unroll
                    for (int r = 0; r < AN_R; ++r) acc[r] = __builtin_fmaf(c, wl[r + 7 - 2 * q] - wr[r + 2 * q + 1], acc[r]);
                }
            }
            if (g + 1 < G) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    wl[j + 8] = wl[j];
                    wr[j] = wr[j + 8];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    wl[j] = xs[an_slot(A - 8 * (g + 1) - 8 + j)];
                    wr[j + 8] = xs[an_slot(A + 8 * (g + 1) + 8 + j)];
                }
            }
        }
    } else {
        float w[16];
        const int B = AN_PADL + o;
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = xs[an_slot(B + j)];
        const int nb = (a.ntaps + 7) >> 3;
        for (int b = 0; b < nb; ++b) {
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const int k = 8 * b + kk;
                if (k < a.ntaps) {
                    const float c = a.taps_rev[k];
#pragma unroll
                    for (int r = 0; r < AN_R; ++r) acc[r] = __builtin_fmaf(c, w[r + kk], acc[r]);
                }
            }
            if (b + 1 < nb) {
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = w[j + 8];
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j + 8] = xs[an_slot(B + 8 * (b + 1) + 8 + j)];
            }
        }
#pragma unroll
        for (int r = 0; r < AN_R; ++r) {
            if (TWO_IN) re[r] = (t0 + o + r < a.n_out) ? a.in0[t0 + o + r + a.delay] : 0.f;
            else re[r] = xs[an_slot(B + r + a.delay)];
        }
    }

    float2 *out = a.out + t0 + o;
    const long long left = a.n_out - (t0 + o);
    if (left >= AN_R && (((uintptr_t)out) & 15) == 0) {
#pragma unroll
        for (int r = 0; r < AN_R; r += 2)
            *reinterpret_cast<float4 *>(out + r) = make_float4(re[r], acc[r], re[r + 1], acc[r + 1]);
    } else {
#pragma unroll
        for (int r = 0; r < AN_R; ++r)
            if (r < left) out[r] = make_float2(re[r], acc[r]);
    }
}

template <bool SPARSE, bool TWO_IN>
int launch_tile(const AnalyticLaunch &a, hipStream_t st)
{
    const size_t lds = (size_t)(an_slot(an_staged(a.ntaps)) + 1) * sizeof(float);
    if (int rc = allow_lds((const void *)analytic_tile_kernel<SPARSE, TWO_IN>, lds)) return rc;
    const long long tiles = (a.n_out + AN_NT - 1) / AN_NT;
    if (tiles > 0x7fffffffLL) return fail(GRHIP_EINVAL, "analytic: too many outputs for one call");
    hipLaunchKernelGGL((analytic_tile_kernel<SPARSE, TWO_IN>), dim3((unsigned)tiles), dim3(AN_THREADS), lds, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

// ---- Goertzel ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GZ_ROWS)
goertzel_generic_kernel(const float *__restrict__ in, float2 *__restrict__ out, long long nblocks, int len, float wr, float wi)
{
    __shared__ float rows[GZ_ROWS * (GZ_CH + 1)];
    const int t = threadIdx.x;
    const long long b0 = (long long)blockIdx.x * GZ_ROWS;
    const int nrows = (int)(nblocks - b0 < GZ_ROWS ? nblocks - b0 : GZ_ROWS);
    const float *base = in + b0 * len;
    float d1 = 0.f, d2 = 0.f;
    for (int i0 = 0; i0 < len; i0 += GZ_CH) {
        const int cols = len - i0 < GZ_CH ? len - i0 : GZ_CH;
        const int total = nrows * cols;
        for (int e = t; e < total; e += GZ_ROWS) {
            const int row = e / cols, col = e - row * cols;
            rows[row * (GZ_CH + 1) + col] = base[(long long)row * len + i0 + col];
        }
        __syncthreads();
        if (t < nrows) {
            const float *x = rows + t * (GZ_CH + 1);
            for (int i = 0; i < cols; ++i) {
                const float y = (x[i] + wr * d1) - d2;       // gri_goertzel::input, unfused
                d2 = d1;
                d1 = y;
            }
        }
        __syncthreads();
    }
    if (t < nrows) {
        // gri_goertzel::output: gr_complex((0.5*d_wr*d_d1-d_d2)/d_len, (d_wi*d_d1)/d_len) -- 0.5 makes the first a double
        const double re = (0.5 * (double)wr * (double)d1 - (double)d2) / (double)len;
        const float im = (wi * d1) / (float)len;
        out[b0 + t] = make_float2((float)re, im);
    }
}

__device__ __forceinline__ float wave_sum_xor(float v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

template <bool WG>
__global__ void __launch_bounds__(256)
goertzel_fast_kernel(const float *__restrict__ in, float2 *__restrict__ out, long long nblocks, int len,
                     const float2 *__restrict__ tab)
{
    __shared__ float2 part[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long b = WG ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + wave;
    const bool live = b < nblocks;                           // wave-uniform
    float ar0 = 0.f, ai0 = 0.f, ar1 = 0.f, ai1 = 0.f;
    if (live) {
        const float *x = in + b * len;
        const int first = WG ? t : lane, step = WG ? 256 : 64;
        int n = first;
        for (; n + step < len; n += 2 * step) {
            const float x0 = x[n], x1 = x[n + step];
            const float2 p0 = tab[n], p1 = tab[n + step];
            ar0 = __builtin_fmaf(x0, p0.x, ar0); ai0 = __builtin_fmaf(x0, p0.y, ai0);
            ar1 = __builtin_fmaf(x1, p1.x, ar1); ai1 = __builtin_fmaf(x1, p1.y, ai1);
        }
        if (n < len) {
            const float x0 = x[n];
            const float2 p0 = tab[n];
            ar0 = __builtin_fmaf(x0, p0.x, ar0); ai0 = __builtin_fmaf(x0, p0.y, ai0);
        }
    }
    const float sr = wave_sum_xor(ar0 + ar1), si = wave_sum_xor(ai0 + ai1);
    if (!WG) {
        if (live && lane == 0) out[b] = make_float2(sr, si);
        return;
    }
    if (lane == 0) part[wave] = make_float2(sr, si);
    __syncthreads();
    if (t == 0)
        out[b] = make_float2((part[0].x + part[1].x) + (part[2].x + part[3].x), (part[0].y + part[1].y) + (part[2].y + part[3].y));
}

}  // namespace

int analytic_launch(int form, const AnalyticLaunch &a, hipStream_t st)
{
    if (a.n_out <= 0) return GRHIP_OK;
    if (a.ntaps < 1 || a.ntaps > AN_MAX_TAPS) return fail(GRHIP_EINVAL, "analytic: %d taps (1 .. %d)", a.ntaps, AN_MAX_TAPS);
    if ((((uintptr_t)a.in0) & 3) || (((uintptr_t)a.in1) & 3) || (((uintptr_t)a.out) & 7))
        return fail(GRHIP_EINVAL, "analytic: items not naturally aligned");
    if (form == AN_GENERIC || a.ntaps > AN_FAST_MAX_TAPS) {
        const size_t sh = (size_t)a.ntaps * sizeof(float);
        if (int rc = allow_lds((const void *)analytic_generic_kernel, sh)) return rc;
        const long long blocks = (a.n_out + 255) / 256;
        if (blocks > 0x7fffffffLL) return fail(GRHIP_EINVAL, "analytic: too many outputs for one call");
        hipLaunchKernelGGL(analytic_generic_kernel, dim3((unsigned)blocks), dim3(256), sh, st, a);
        GRHIP_HIP(hipGetLastError());
        return GRHIP_OK;
    }
    if (form == AN_SPARSE) {
        if (a.in1 != a.in0 || !a.odd || !(a.ntaps & 1) || a.nodd != (a.ntaps / 2 + 1) / 2 || a.delay != a.ntaps / 2)
            return fail(GRHIP_EINVAL, "analytic: not a sparse launch");
        return launch_tile<true, false>(a, st);
    }
    return a.in1 != a.in0 ? launch_tile<false, true>(a, st) : launch_tile<false, false>(a, st);
}

int goertzel_launch_generic(const float *in, float2 *out, long long nblocks, int len, float wr, float wi, hipStream_t st)
{
    if (nblocks <= 0) return GRHIP_OK;
    const long long wgs = (nblocks + GZ_ROWS - 1) / GZ_ROWS;
    if (len < 1 || wgs > 0x7fffffffLL) return fail(GRHIP_EINVAL, "goertzel: bad launch");
    hipLaunchKernelGGL(goertzel_generic_kernel, dim3((unsigned)wgs), dim3(GZ_ROWS), 0, st, in, out, nblocks, len, wr, wi);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int goertzel_launch_fast(const float *in, float2 *out, long long nblocks, int len, const float2 *tab, hipStream_t st)
{
    if (nblocks <= 0) return GRHIP_OK;
    const bool wg = len >= GZ_WG_LEN;
    const long long wgs = wg ? nblocks : (nblocks + 3) / 4;
    if (len < 1 || !tab || wgs > 0x7fffffffLL) return fail(GRHIP_EINVAL, "goertzel: bad launch");
    if (wg) hipLaunchKernelGGL(goertzel_fast_kernel<true>, dim3((unsigned)wgs), dim3(256), 0, st, in, out, nblocks, len, tab);
    else hipLaunchKernelGGL(goertzel_fast_kernel<false>, dim3((unsigned)wgs), dim3(256), 0, st, in, out, nblocks, len, tab);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
