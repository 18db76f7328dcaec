// am_demod.hip -- the AM demodulator hier block of blks2impl/am_demod.py:42-58:
// gr_complex_to_mag -> gr_add_const_ff(-1) -> gr_fir_filter_fff(D, taps).
//
// The composed path runs the blocks one after the other on a work row of the handle: amd_v_kernel writes the carried
// delay line and v = (float)(|x| - 1.0f) behind it, the FIR family's generic-order kernel filters the row, and
// amd_tail_kernel keeps the row's last ntaps - 1 values for the next call.
//
// amd_fused_kernel is the three in one pass: 8 bytes read per input sample and 4 / D written, nothing in between.
// One workgroup per (stream, tile of AMD_TILE input samples):
//   (a) v of the tile and of the ntaps - 1 samples in front of it, formed once per sample into LDS; where those reach
//       in front of the call's start, the carried delay line stands in (zeros at a stream's start: the FIR's delay
//       line holds zeros of v, it is not |0| - 1);
//   (b) the decimated outputs with f32 FMAs, taps in ascending order.
//       D == 1, the blocked step: a lane forms AMD_R = 8 adjacent outputs.  It holds the 8 samples under tap k and
//       reads the 8 in front of them once per block of 8 taps: 64 FMAs on 16 registers per 8 LDS words, one LDS read
//       per 8 FMAs (the FM kernel's step reads one per FMA).  A lane's samples start 8 apart; with one word of padding
//       per 8 the lane stride in LDS is 9 words, odd, so the 64 lanes of a wave read 64 different banks.  The taps
//       are wave-uniform: they come through scalar loads, 8 at a time, from a buffer padded to a multiple of 8; the
//       last block uses only the taps there are.
//       D > 1, the plain step of the FM kernel: consecutive lanes on consecutive outputs, one LDS read per FMA, one
//       word of padding per 64.
// The last tile writes the carried delay line into the state's other copy (tiles at the call's start read the old one).
#include "am_demod.h"
#include "spectrum_math.h"

namespace grhip {

namespace {

__device__ __forceinline__ float amd_v(float2 x) { return __fadd_rn(mag_val(x.x, x.y), -1.0f); }

// grid (blocks, S)
__global__ void __launch_bounds__(256)
amd_v_kernel(const float2 *__restrict__ in, int n_in, const float *__restrict__ hist, int H, float *__restrict__ row,
             long long row_stride)
{
    const int s = blockIdx.y;
    const float2 *__restrict__ x = in + (long long)s * n_in;
    float *__restrict__ r = row + (long long)s * row_stride;
    const long long stride = (long long)gridDim.x * 256;
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < (long long)H + n_in; u += stride)
        r[u] = u < H ? hist[(long long)s * H + u] : amd_v(x[u - H]);
}

__global__ void __launch_bounds__(256)
amd_tail_kernel(int n_in, const float *__restrict__ row, long long row_stride, int H, float *__restrict__ hist,
                int *__restrict__ d_produced, int produced)
{
    const int s = blockIdx.y;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < H; k += gridDim.x * 256)
        hist[(long long)s * H + k] = row[(long long)s * row_stride + n_in + k];
    if (blockIdx.x == 0 && threadIdx.x == 0 && s == 0 && d_produced) *d_produced = produced;
}

// LDS word of local sample u: one word of padding per AMD_R (blocked) or per 64 (plain)
template <bool BLOCKED>
__device__ __forceinline__ int amd_slot(int u) { return BLOCKED ? u + (u >> 3) : u + (u >> 6); }

// One block of the blocked step: nk <= AMD_R taps t[0 .. nk) over hi (the samples under t[0]) and lo (the AMD_R in front
// of them); hi becomes lo.  t holds AMD_R readable entries whatever nk is.
__device__ __forceinline__ void amd_block(const float *__restrict__ s_lo, const float *__restrict__ tp, int nk, float (&hi)[AMD_R],
                                          float (&acc)[AMD_R])
{
    float lo[AMD_R], t[AMD_R];
#pragma unroll
    for (int e = 0; e < AMD_R; ++e) { lo[e] = s_lo[e]; t[e] = tp[e]; }
#pragma unroll
    for (int kk = 0; kk < AMD_R; ++kk) {
        if (kk < nk) {
#pragma unroll
            for (int r = 0; r < AMD_R; ++r) acc[r] = __builtin_fmaf(t[kk], r >= kk ? hi[r - kk] : lo[AMD_R + r - kk], acc[r]);
        }
    }
#pragma unroll
    for (int e = 0; e < AMD_R; ++e) hi[e] = lo[e];
}

// grid (tiles, S).  BLOCKED: a.D == 1 (then a.o0 == 0 and a.produced == a.n_in)
template <bool BLOCKED>
__global__ void __launch_bounds__(256)
amd_fused_kernel(AmdFused a)
{
    static_assert(AMD_R == 8 && AMD_TILE % (256 * AMD_R) == 0, "the blocked step's shape");
    __shared__ float s_v[AMD_SLOTS];
    const int tid = threadIdx.x;
    const int s = blockIdx.y;
    const int H = a.ntaps - 1;
    const int F = 8 + ((8 - (H & 7)) & 7);                  // 8 .. 15 zeroed words in front; F + H is a multiple of 8
    const int t0 = blockIdx.x * AMD_TILE;
    const int nt = a.n_in - t0 < AMD_TILE ? a.n_in - t0 : AMD_TILE;
    const float2 *__restrict__ x = a.in + (long long)s * a.n_in;

    // (a): local sample u is the call's item t0 - H + u, at word amd_slot(F + u); u < H + nt <= AMD_MAX_HIST + AMD_TILE
    for (int u = tid; u < F; u += 256) s_v[amd_slot<BLOCKED>(u)] = 0.f;
    for (int u = tid; u < H + nt; u += 256) {
        const int i = t0 - H + u;
        s_v[amd_slot<BLOCKED>(F + u)] = i < 0 ? a.rd.hist[(long long)s * H + H + i] : amd_v(x[i]);
    }
    __syncthreads();

    // (b)
    if (BLOCKED) {
        float *__restrict__ o = a.out + (long long)s * a.produced + t0;
        const float *__restrict__ taps = a.taps;
        for (int pass = 0; pass < AMD_TILE / (256 * AMD_R); ++pass) {
            const int jj0 = pass * 256 * AMD_R + tid * AMD_R;
            if (jj0 >= nt) continue;
            const int B = F + H + jj0;                      // a multiple of 8: the 8 words from sb on are contiguous
            const int sb = B + (B >> 3);
            float hi[AMD_R], acc[AMD_R];
#pragma unroll
            for (int r = 0; r < AMD_R; ++r) { hi[r] = s_v[sb + r]; acc[r] = 0.f; }
            // block kb: taps kb .. kb + 7 over hi = samples B - kb .. B - kb + 7 and lo = the 8 in front of them; the
            // last block stops at the last tap (a padded tap of zero would turn an infinite sample into a NaN)
            const int full = a.ntaps & ~(AMD_R - 1);
            int kb = 0, lb = sb - (AMD_R + 1);
            for (; kb < full; kb += AMD_R, lb -= AMD_R + 1) amd_block(s_v + lb, taps + kb, AMD_R, hi, acc);
            if (kb < a.ntaps) amd_block(s_v + lb, taps + kb, a.ntaps - kb, hi, acc);
            if (jj0 + AMD_R <= nt && (((uintptr_t)(o + jj0)) & 15) == 0) {
                *(float4 *)(o + jj0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                *(float4 *)(o + jj0 + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
            } else {
#pragma unroll
                for (int r = 0; r < AMD_R; ++r)
                    if (jj0 + r < nt) o[jj0 + r] = acc[r];
            }
        }
    } else {
        const long long t1 = (long long)t0 + nt;
        const int jlo = t0 <= a.o0 ? 0 : (int)(((long long)t0 - a.o0 + a.D - 1) / a.D);
        const int jhi = t1 <= a.o0 ? 0 : (int)((t1 - a.o0 + a.D - 1) / a.D);
        float *__restrict__ o = a.out + (long long)s * a.produced;
        for (int j = jlo + tid; j < jhi; j += 256) {
            const int base = F + H + (int)(a.o0 + (long long)j * a.D - t0);
            float acc = 0.f;
            for (int k = 0; k < a.ntaps; ++k) acc = __builtin_fmaf(a.taps[k], s_v[amd_slot<false>(base - k)], acc);
            o[j] = acc;
        }
    }
    if (t0 + nt == a.n_in) {
        for (int k = tid; k < H; k += 256) a.wr.hist[(long long)s * H + k] = s_v[amd_slot<BLOCKED>(F + nt + k)];
        if (tid == 0 && s == 0 && a.d_produced) *a.d_produced = a.produced;
    }
}

inline unsigned amd_blocks(long long n)
{
    long long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}

}  // namespace

int amd_v_launch(const float2 *in, int n_in, int nstreams, const float *hist, int H, float *row, long long row_stride, hipStream_t st)
{
    if (n_in <= 0 || nstreams <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(amd_v_kernel, dim3(amd_blocks((long long)H + n_in), nstreams), dim3(256), 0, st, in, n_in, hist, H, row,
                       row_stride);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int amd_tail_launch(int n_in, int nstreams, const float *row, long long row_stride, int H, float *hist, int *d_produced,
                    int produced, hipStream_t st)
{
    if (n_in <= 0 || nstreams <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(amd_tail_kernel, dim3(amd_blocks(H), nstreams), dim3(256), 0, st, n_in, row, row_stride, H, hist, d_produced,
                       produced);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int amd_fused_launch(const AmdFused &a, hipStream_t st)
{
    if (a.n_in <= 0 || a.nstreams <= 0) return GRHIP_OK;
    const int H = a.ntaps - 1;
    if (a.ntaps < 1 || H > AMD_MAX_HIST || a.D < 1 || a.o0 < 0 || a.o0 >= a.D || (a.D == 1 && a.produced != a.n_in) ||
        a.n_in > 0x7fffffff - AMD_TILE)
        return fail(GRHIP_EINVAL, "am_demod: the fused kernel cannot take this shape");
    const unsigned tiles = (unsigned)(((long long)a.n_in + AMD_TILE - 1) / AMD_TILE);
    if (a.D == 1) hipLaunchKernelGGL(amd_fused_kernel<true>, dim3(tiles, a.nstreams), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(amd_fused_kernel<false>, dim3(tiles, a.nstreams), dim3(256), 0, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
