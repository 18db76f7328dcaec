// pfb_synth.hip -- gr_pfb_synthesis_filterbank_ccf (filter/gr_pfb_synthesis_filterbank_ccf.cc:122-169): the mirror
// image of the channeliser.  Per output vector n: M bins gathered from the input streams (bin i reads item n + i of its
// stream), a FORWARD unnormalised M-point DFT, and M real-tap FIR branches along n, branch f fed by DFT output M-1-f;
// the M branch outputs of a vector are adjacent in memory.
//
// Fused kernel (2 <= M <= 16, tpf <= 513 so that the halo is no longer than the tile, and the tile fits the LDS): a 256-lane workgroup owns a tile of 512 output vectors.
//   1. every lane gathers the bins of one vector at a time (neighbouring lanes read neighbouring items of each
//      stream), runs the DFT in registers (radix-2 for powers of two, the direct M x M sum otherwise) and stores the
//      result in LDS as [branch][time] rows, one pad slot per 8 samples (conflict-free ds_read_b64 in step 2).  The
//      tpf - 1 vectors in front of the tile are recomputed (or, in front of the call, read from the handle's state),
//      so tiles are independent: (tpf-1)/512 extra gather and DFT work, no second pass;
//   2. wave w runs the FIR of branches w, w+4, ...: 8 outputs per lane, an 8-deep register window over the row, the
//      branch's (wave-uniform) taps by scalar loads, one packed FMA per tap and output.  GENERIC: one accumulator,
//      oldest sample first, a multiply and an add per term (gri_fir_filter_with_buffer_ccf::filter, .cc.t:73-77);
//   3. the outputs go back to LDS as [time][branch] and leave as contiguous 16-byte stores.
// 8*numsigs/M + 8 bytes of HBM traffic per output sample.
//
// General path (M = 1, M > 16, tpf > 513 or a tile beyond the LDS): the direct DFT into a [time][branch] scratch
// buffer in HBM, a FIR pass over it (lanes along the branches, so both passes are coalesced), and a copy of the last
// tpf - 1 rows into the state.  Correct for every shape the block accepts; three passes instead of one.
#include "grhip_internal.h"
#include "pfb_synth.h"

namespace grhip {

namespace {

typedef const float __attribute__((address_space(4))) *sy_cfloat_p;
typedef float sy_f32x2 __attribute__((ext_vector_type(2)));

constexpr int SY_R = 8, SY_T = 64 * SY_R, SY_THREADS = 256, SY_WAVES = SY_THREADS / 64;

__host__ __device__ constexpr int sy_slot(int m) { return m + (m >> 3); }
// slots of one [branch] row: the tile, the halo (taps padded to a multiple of 8) and the window's read-ahead
__host__ __device__ constexpr int sy_row(int tpf) { return sy_slot(SY_T + (tpf + SY_R - 1) / SY_R * SY_R + SY_R) + 1; }

// bin i of output vector m (.cc:139-156): the first ceil(numsigs/2) bins and the last floor(numsigs/2) carry streams,
// the ones between are zero; the item is m + i, the reference's `(in+i)[n]`.  Items past what the caller provides read
// as zero (the host refuses the shapes that would need them).
__device__ __forceinline__ float2 sy_bin(const PfbSynthArgs &a, int i, int nhalf, int ndiff, long long m)
{
    int s = i;
    if (i >= nhalf) {
        if (i < nhalf + ndiff) return make_float2(0.f, 0.f);
        s = i - ndiff;
    }
    const long long item = m + i;
    return item < a.in_items ? a.in[(long long)s * a.stride + item] : make_float2(0.f, 0.f);
}

// V[k] = sum_i b[i] e^{-2 pi j i k / M}; tw[k] = e^{-2 pi j k / M} (wave-uniform table, scalar loads)
template <int M>
__device__ __forceinline__ void sy_dft(const float2 (&b)[M], float2 (&v)[M], sy_cfloat_p tw)
{
    constexpr bool POW2 = (M & (M - 1)) == 0;
    if constexpr (M == 1) {
        v[0] = b[0];
    } else if constexpr (POW2) {
        constexpr int LOGM = M == 2 ? 1 : M == 4 ? 2 : M == 8 ? 3 : 4;
        // bit-reversed load, then radix-2 decimation-in-time stages (canonical loop bounds: everything unrolls)
#pragma unroll
        for (int s = 0; s < M; ++s) {
            int rv = 0;
#pragma unroll
            for (int bit = 0; bit < LOGM; ++bit)
                if (s & (1 << bit)) rv |= (M >> 1) >> bit;
            v[rv] = b[s];
        }
#pragma unroll
        for (int stg = 0; stg < LOGM; ++stg) {
            const int len = 2 << stg;
            const int half = len >> 1, step = M / len;
#pragma unroll
            for (int s0 = 0; s0 < M; s0 += len) {
#pragma unroll
                for (int k = 0; k < half; ++k) {
                    const float wr = tw[2 * (k * step)], wi = tw[2 * (k * step) + 1];
                    const float2 u = v[s0 + k], q = v[s0 + k + half];
                    const float2 p = (k == 0) ? q : make_float2(__builtin_fmaf(q.x, wr, -(q.y * wi)),
                                                                __builtin_fmaf(q.x, wi, q.y * wr));
                    v[s0 + k] = make_float2(u.x + p.x, u.y + p.y);
                    v[s0 + k + half] = make_float2(u.x - p.x, u.y - p.y);
                }
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < M; ++k) {
            float2 acc = b[0];
#pragma unroll
            for (int s = 1; s < M; ++s) {
                const int ph = (s * k) % M;
                const float wr = tw[2 * ph], wi = tw[2 * ph + 1];
                acc.x = __builtin_fmaf(b[s].x, wr, acc.x);
                acc.x = __builtin_fmaf(-b[s].y, wi, acc.x);
                acc.y = __builtin_fmaf(b[s].x, wi, acc.y);
                acc.y = __builtin_fmaf(b[s].y, wr, acc.y);
            }
            v[k] = acc;
        }
    }
}

template <bool GENERIC>
__device__ __forceinline__ sy_f32x2 sy_mac(float h, sy_f32x2 x, sy_f32x2 acc)
{
    if (GENERIC) {
        const sy_f32x2 p = x * h;       // (-ffp-contract=off: a product and a sum, as `out += buffer[i] * taps[i]`)
        return acc + p;
    }
    return __builtin_elementwise_fma((sy_f32x2){h, h}, x, acc);
}

template <int M, bool GENERIC>
__global__ void __launch_bounds__(SY_THREADS) pfb_synth_kernel(const PfbSynthArgs a)
{
    static_assert(M >= 2 && M <= SY_FUSED_MAX_CHANS, "2 <= M <= 16");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sy_f32x2 *us = (sy_f32x2 *)smem;                     // [M][RS] branch inputs; later [SY_T][M] outputs
    const int tpf = a.tpf, H = tpf - 1, RS = sy_row(tpf);
    const int t = threadIdx.x, ln = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long t0 = (long long)blockIdx.x * SY_T;
    const int nhalf = (a.numsigs + 1) / 2, ndiff = M - a.numsigs;
    const sy_cfloat_p tw = (sy_cfloat_p)(const float *)a.tw;

    // ---- 1. branch inputs of vectors t0 - H .. t0 + SY_T - 1, column c = vector - (t0 - H)
    for (int c = t; c < SY_T + H; c += SY_THREADS) {
        const long long m = t0 - H + c;
        float2 u[M];
        if (m < 0) {                                     // before the call: the delay lines (first tile only)
            const float2 *sp = a.state_old + (m + H) * M;
#pragma unroll
            for (int f = 0; f < M; ++f) u[f] = sp[f];
        } else if (m >= a.nvec) {                        // past the call: feeds no output that is stored
#pragma unroll
            for (int f = 0; f < M; ++f) u[f] = make_float2(0.f, 0.f);
        } else {
            float2 b[M], v[M];
#pragma unroll
            for (int i = 0; i < M; ++i) b[i] = sy_bin(a, i, nhalf, ndiff, m);
            sy_dft<M>(b, v, tw);
#pragma unroll
            for (int f = 0; f < M; ++f) u[f] = v[M - 1 - f];          // .cc:162: filter M-1-i takes DFT output i
        }
        const int sl = sy_slot(c);
#pragma unroll
        for (int f = 0; f < M; ++f) us[f * RS + sl] = (sy_f32x2){u[f].x, u[f].y};
        // what the next call's delay lines hold: the call's last H vectors, written by the tile that owns them (or,
        // when the call is shorter than H, the older rows moved up)
        if ((c >= H || m < 0) && m < a.nvec && m >= a.nvec - H) {
            float2 *sp = a.state_new + (m - a.nvec + H) * M;
#pragma unroll
            for (int f = 0; f < M; ++f) sp[f] = u[f];
        }
    }
    __syncthreads();

    // ---- 2. FIR along time: out[n][f] = sum_k taps_rev[f][k] u_f[n - H + k], k ascending = oldest sample first
    constexpr int NB = (M + SY_WAVES - 1) / SY_WAVES;
    sy_f32x2 acc[NB][SY_R];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int r = 0; r < SY_R; ++r) acc[b][r] = (sy_f32x2){0.f, 0.f};
    }
    const int tpfp = (tpf + SY_R - 1) / SY_R * SY_R;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int f = w + SY_WAVES * b;
        if (f < M) {
            const sy_f32x2 *xp = us + f * RS + ln * SY_R + ln;        // slot of column 8 ln
            const sy_cfloat_p hp = (sy_cfloat_p)a.taps_rev + (size_t)f * tpf;
            sy_f32x2 win[SY_R];
#pragma unroll
            for (int q = 0; q < SY_R; ++q) win[q] = xp[q];
            for (int k0 = 0; k0 < tpfp; k0 += SY_R) {
                const int nxt = k0 + SY_R + (k0 >> 3) + 1;
#pragma unroll
                for (int qq = 0; qq < SY_R; ++qq) {
                    if (k0 + qq < tpf) {                 // (no zero taps added: GENERIC sums exactly the reference's terms)
                        const float h = hp[k0 + qq];
#pragma unroll
                        for (int r = 0; r < SY_R; ++r) acc[b][r] = sy_mac<GENERIC>(h, win[(qq + r) & (SY_R - 1)], acc[b][r]);
                    }
                    win[qq] = xp[nxt + qq];
                }
            }
        }
    }
    __syncthreads();                                     // every wave is done with the rows

    // ---- 3. [time][branch] through LDS (a pad slot per 8 vectors), then contiguous 16-byte stores
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int f = w + SY_WAVES * b;
        if (f < M) {
#pragma unroll
            for (int r = 0; r < SY_R; ++r) us[(ln * SY_R + r) * M + f + ln] = acc[b][r];
        }
    }
    __syncthreads();
    const long long base = t0 * M, limit = a.nvec * M;
    const bool al16 = ((size_t)a.out & 15) == 0;
    for (int p = t; p < SY_T * M / 2; p += SY_THREADS) {
        const int e = 2 * p;
        const sy_f32x2 x0 = us[e + ((e / M) >> 3)], x1 = us[e + 1 + (((e + 1) / M) >> 3)];
        const long long gi = base + e;
        if (gi + 1 < limit && al16) {
            *reinterpret_cast<float4 *>(a.out + gi) = make_float4(x0.x, x0.y, x1.x, x1.y);
        } else {
            if (gi < limit) a.out[gi] = make_float2(x0.x, x0.y);
            if (gi + 1 < limit) a.out[gi + 1] = make_float2(x1.x, x1.y);
        }
    }
}

// ---- general path -----------------------------------------------------------------------------------------------
// scratch row r (0 <= r < H + nvec), column f: r < H: the delay lines (u_f[r - H]); else u_f[r - H] = V_{r-H}[M-1-f]
__global__ void __launch_bounds__(SY_THREADS) pfb_synth_dft_any(const PfbSynthArgs a)
{
    const int M = a.M, H = a.tpf - 1;
    const long long idx = (long long)blockIdx.x * SY_THREADS + threadIdx.x;
    if (idx >= (H + a.nvec) * M) return;
    const long long r = idx / M;
    const int f = (int)(idx - r * M);
    if (r < H) {
        a.scratch[idx] = a.state_old[idx];
        return;
    }
    const long long m = r - H;
    const int k = M - 1 - f;
    const int nhalf = (a.numsigs + 1) / 2, ndiff = M - a.numsigs;
    float2 acc = sy_bin(a, 0, nhalf, ndiff, m);
    int ph = 0;
    for (int i = 1; i < M; ++i) {
        ph += k;
        if (ph >= M) ph -= M;                            // (i*k) mod M
        const float2 b = sy_bin(a, i, nhalf, ndiff, m);
        const float2 wv = a.tw[ph];
        acc.x = __builtin_fmaf(b.x, wv.x, acc.x);
        acc.x = __builtin_fmaf(-b.y, wv.y, acc.x);
        acc.y = __builtin_fmaf(b.x, wv.y, acc.y);
        acc.y = __builtin_fmaf(b.y, wv.x, acc.y);
    }
    a.scratch[idx] = acc;
}

template <bool GENERIC>
__global__ void __launch_bounds__(SY_THREADS) pfb_synth_fir_any(const PfbSynthArgs a)
{
    const int M = a.M, tpf = a.tpf;
    const long long idx = (long long)blockIdx.x * SY_THREADS + threadIdx.x;
    if (idx >= a.nvec * M) return;
    const int f = (int)(idx % M);
    const float2 *x = a.scratch + idx;                   // row n, column f: the oldest sample of output n
    const float *h = a.taps_t + f;
    sy_f32x2 acc = (sy_f32x2){0.f, 0.f};
    for (int k = 0; k < tpf; ++k) {
        const float2 s = x[(long long)k * M];
        acc = sy_mac<GENERIC>(h[(size_t)k * M], (sy_f32x2){s.x, s.y}, acc);
    }
    a.out[idx] = make_float2(acc.x, acc.y);
}

template <int M>
int launch_fused(const PfbSynthArgs &a, bool generic, hipStream_t st)
{
    const size_t lds = (size_t)M * sy_row(a.tpf) * sizeof(float2);
    const void *k = generic ? (const void *)pfb_synth_kernel<M, true> : (const void *)pfb_synth_kernel<M, false>;
    if (int rc = allow_lds(k, lds)) return rc;
    const unsigned grid = (unsigned)((a.nvec + SY_T - 1) / SY_T);
    if (generic) hipLaunchKernelGGL((pfb_synth_kernel<M, true>), dim3(grid), dim3(SY_THREADS), lds, st, a);
    else hipLaunchKernelGGL((pfb_synth_kernel<M, false>), dim3(grid), dim3(SY_THREADS), lds, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

bool pfb_synth_fused(int M, int tpf)
{
    // the halo no longer than the tile: beyond that a tile recomputes more vectors than it owns
    return M >= 2 && M <= SY_FUSED_MAX_CHANS && tpf >= 1 && tpf - 1 <= SY_T &&
           (size_t)M * sy_row(tpf) * sizeof(float2) <= SY_LDS_MAX;
}

int launch_pfb_synth(const PfbSynthArgs &a, bool generic, hipStream_t st)
{
    if (a.nvec <= 0) return GRHIP_OK;
    if (pfb_synth_fused(a.M, a.tpf)) {
        switch (a.M) {
        case 2: return launch_fused<2>(a, generic, st);
        case 3: return launch_fused<3>(a, generic, st);
        case 4: return launch_fused<4>(a, generic, st);
        case 5: return launch_fused<5>(a, generic, st);
        case 6: return launch_fused<6>(a, generic, st);
        case 7: return launch_fused<7>(a, generic, st);
        case 8: return launch_fused<8>(a, generic, st);
        case 9: return launch_fused<9>(a, generic, st);
        case 10: return launch_fused<10>(a, generic, st);
        case 11: return launch_fused<11>(a, generic, st);
        case 12: return launch_fused<12>(a, generic, st);
        case 13: return launch_fused<13>(a, generic, st);
        case 14: return launch_fused<14>(a, generic, st);
        case 15: return launch_fused<15>(a, generic, st);
        case 16: return launch_fused<16>(a, generic, st);
        default: break;
        }
    }
    if (!a.scratch) return fail(GRHIP_EINVAL, "pfb_synthesis_filterbank: no scratch buffer");
    const long long H = a.tpf - 1;
    const long long n1 = (H + a.nvec) * a.M, n2 = a.nvec * a.M;
    hipLaunchKernelGGL(pfb_synth_dft_any, dim3((unsigned)((n1 + SY_THREADS - 1) / SY_THREADS)), dim3(SY_THREADS), 0, st, a);
    GRHIP_HIP(hipGetLastError());
    if (generic) hipLaunchKernelGGL(pfb_synth_fir_any<true>, dim3((unsigned)((n2 + SY_THREADS - 1) / SY_THREADS)), dim3(SY_THREADS), 0, st, a);
    else hipLaunchKernelGGL(pfb_synth_fir_any<false>, dim3((unsigned)((n2 + SY_THREADS - 1) / SY_THREADS)), dim3(SY_THREADS), 0, st, a);
    GRHIP_HIP(hipGetLastError());
    if (H > 0)          // rows nvec .. nvec + H - 1 are u[nvec - H .. nvec - 1]: the next call's state
        GRHIP_HIP(hipMemcpyAsync(a.state_new, a.scratch + a.nvec * a.M, (size_t)H * a.M * sizeof(float2),
                                 hipMemcpyDeviceToDevice, st));
    return GRHIP_OK;
}

}  // namespace grhip
