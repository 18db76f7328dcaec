// modulator_fused.hip -- generic_mod (gr-digital/python/generic_mod_demod.py:114-150), engine 1: bytes in, samples out.
//
// packed_to_unpacked_bb(k, MSB_FIRST) -> map_bb(pre_diff_code) -> diff_encoder_bb(2^k) -> chunks_to_symbols_bc(points)
// -> pfb_arb_resampler_ccf(sps, rrc, 32) as one kernel behind a carry pre-pass.  Nothing in the chain is serial: a
// symbol's bits are a closed form of its index, the encoder is a prefix sum modulo 2^k, and the resampler's schedule
// (ArbSched, csrc/sched_plan.h) is a closed form per output.
//
// mod_fused_kernel: one workgroup = `tile` consecutive outputs of one stream (blockIdx.y), as arb_kernel
// (csrc/arb_resampler.hip).  From the schedule it derives the symbols its outputs read, [count_first - tpf,
// count_last) of the call; those in front of the call's first symbol come from the stream's history (the last tpf
// symbols of the calls before, complex zeros in front of the stream's start: not point 0), the others it makes itself:
// every lane unpacks and maps a run of consecutive symbols from the one or two bytes that hold each, the runs are
// scanned across the workgroup from the tile's carry, and the points go into LDS where arb_kernel has its staged
// input.  The polyphase step is arb_kernel's, statement for statement, so GRHIP_MODE_GENERIC is engine 0 bit for bit.
// Per symbol the kernel reads k/8 bytes and writes 8 * sps; the five blocks in a row move about 38 at sps 2.
//
// The pre-pass (differential only): mod_segment_sum_kernel sums the mapped symbols between the first new symbols of
// consecutive tiles (modulator_plan.h: the segments tile the call's symbols), diff_carry_kernel (csrc/modulator.hip)
// turns the sums into the encoder's state in front of every tile and leaves last_out behind the call.  Afterwards
// mod_state_kernel writes the stream's last tpf symbols, walking back from last_out, and keeps the call's last byte.
#include "arb_resampler.h"
#include "fir_arith.h"
#include "grhip_internal.h"
#include "modulator.h"

namespace grhip {

namespace {

static_assert(MOD_THREADS_FUSED == ARB_THREADS, "the polyphase step is arb_kernel's");

// symbol i of the call in front of the encoder: its k bits from bit address base + i*k, byte 0 being the carried
// byte and byte j + 1 in[j], most significant first (gr_packed_to_unpacked_XX.cc.t:104-111), then map_bb
__device__ __forceinline__ unsigned mod_symbol(const ModLaunch &a, const unsigned char *__restrict__ in, unsigned carry_byte, long long i,
                                               const unsigned char *map)
{
    const unsigned long long b = a.base + (unsigned long long)i * a.k;
    const long long byte = (long long)(b >> 3);
    const unsigned sh = (unsigned)(b & 7u);
    const unsigned b0 = byte == 0 ? carry_byte : (byte - 1 < a.n_bytes ? in[byte - 1] : 0u);
    const unsigned b1 = (sh + a.k > 8u && byte < a.n_bytes) ? in[byte] : 0u;
    const unsigned v = (((b0 << 8) | b1) >> (16u - sh - a.k)) & a.mask;
    return map ? map[v] : v;
}

constexpr int MOD_WAVES = MOD_THREADS_FUSED / 64;

// inclusive scan modulo mask + 1 of one value per lane: inside each wave of 64 by shuffles, across the waves through
// ps[MOD_WAVES] and one barrier
__device__ __forceinline__ unsigned block_scan_mask(unsigned v, unsigned mask, unsigned *ps)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(v, off, 64);
        if (lane >= off) v += up;
    }
    if (lane == 63) ps[w] = v;
    __syncthreads();
    unsigned add = 0;
#pragma unroll
    for (int i = 0; i < MOD_WAVES - 1; ++i)
        if (i < w) add += ps[i];
    return (v + add) & mask;
}

// the sum of one value per lane, in lane 0 of wave 0 (ps as above)
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned *ps)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) ps[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned s = 0;
#pragma unroll
    for (int i = 0; i < MOD_WAVES; ++i) s += ps[i];
    return s;
}

// ---- the carry pre-pass: the sum of the mapped symbols of segment t, modulo 2^k ---------------------------------------------
__global__ void __launch_bounds__(MOD_THREADS_FUSED) mod_segment_sum_kernel(ModLaunch a)
{
    __shared__ unsigned ps[MOD_WAVES];
    const int t = threadIdx.x;
    const long long seg = blockIdx.x;
    const unsigned char *__restrict__ in = a.in + (long long)blockIdx.y * a.n_bytes;
    const unsigned cb = a.carry_byte[blockIdx.y];
    const long long lo = mod_tile_first_symbol(a.sc, (unsigned)a.R, a.tpf, a.tile, seg, a.ntiles, a.nsym);
    const long long hi = mod_tile_first_symbol(a.sc, (unsigned)a.R, a.tpf, a.tile, seg + 1, a.ntiles, a.nsym);
    unsigned s = 0;
    for (long long i = lo + t; i < hi; i += MOD_THREADS_FUSED) s += mod_symbol(a, in, cb, i, a.map);    // far below 2^32
    s = block_sum(s, ps);
    if (t == 0) a.carries[diff_carry_slot(blockIdx.y, a.ntiles, seg)] = s & a.mask;
}

// ---- the fused kernel ------------------------------------------------------------------------------------------------------
template <bool GENERIC>
__global__ void __launch_bounds__(MOD_THREADS_FUSED) mod_fused_kernel(ModLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float2 pts[256];
    __shared__ unsigned ps[MOD_WAVES];
    __shared__ unsigned char smap[256];
    float2 *hs = reinterpret_cast<float2 *>(smem);                                          // [R][S]
    float2 *xs = reinterpret_cast<float2 *>(smem + (size_t)a.R * a.S * sizeof(float2));     // [span_cap]
    const int t = threadIdx.x;
    const long long k0 = (long long)blockIdx.x * a.tile;
    if (k0 >= a.nout) return;                                                               // the whole workgroup
    const int kn = (int)(a.nout - k0 < a.tile ? a.nout - k0 : a.tile);
    const unsigned char *__restrict__ in = a.in + (long long)blockIdx.y * a.n_bytes;
    const float2 *__restrict__ hist = a.hist + (long long)blockIdx.y * a.tpf;
    float2 *out = a.out + (long long)blockIdx.y * a.out_stride + k0;
    const unsigned R = (unsigned)a.R;

    // the tile's first count and what local positions start from, as arb_kernel
    const unsigned long long Tb = a.sc.A0 + (unsigned long long)k0 * a.sc.F;
    const unsigned long long pb = a.sc.j0 + (unsigned long long)k0 * a.sc.D + (Tb >> 23);
    const long long cf = a.sc.c0 + (long long)(pb / R);
    const unsigned rb = (unsigned)(pb % R);
    const unsigned Tm = (unsigned)(Tb & 0x7fffffu);
    const unsigned long long tl_last = Tm + (unsigned long long)(kn - 1) * a.sc.F;
    const unsigned pl_last = rb + (unsigned)(kn - 1) * a.sc.D + (unsigned)(tl_last >> 23);
    const long long clast = cf + pl_last / R;
    int span = (int)(clast - cf) + a.tpf;
    if (span > a.span_cap) span = a.span_cap;           // never past the LDS image (the host sizes tiles so it fits)

    for (int i = t; i < a.R * a.S; i += MOD_THREADS_FUSED) hs[i] = a.taps[i];
    pts[t] = (unsigned)t < a.npoints ? a.points[t] : make_float2(0.f, 0.f);        // an index outside the table: zeros
    smap[t] = a.map ? a.map[t] : (unsigned char)t;

    // xs[u] is item cf + u of [history | the call's symbols]: the first nh of them are history
    long long nh64 = (long long)a.tpf - cf;
    const int nh = nh64 < 0 ? 0 : (nh64 > span ? span : (int)nh64);
    for (int u = t; u < nh; u += MOD_THREADS_FUSED) xs[u] = hist[cf + u];
    __syncthreads();                                                                // pts and smap

    // the others are symbols r0 .. r0 + nn of the call: a run of `per` consecutive ones per lane
    const long long r0 = cf + nh - a.tpf;
    const int nn = span - nh;
    constexpr int MAX_PER = MOD_SPAN_ITEMS / MOD_THREADS_FUSED;                      // span <= span_cap <= MOD_SPAN_ITEMS
    const int per = (nn + MOD_THREADS_FUSED - 1) / MOD_THREADS_FUSED;
    const int v0 = t * per < nn ? t * per : nn, v1 = v0 + per < nn ? v0 + per : nn;
    const unsigned cb = a.carry_byte[blockIdx.y];
    unsigned sym[MAX_PER];
    unsigned s = 0;
#pragma unroll
    for (int q = 0; q < MAX_PER; ++q) {
        const bool live = v0 + q < v1 && r0 + v0 + q < a.nsym;
        sym[q] = live ? mod_symbol(a, in, cb, r0 + v0 + q, smap) : 0u;
        s += sym[q];
    }
    unsigned run = 0;
    if (a.differential) {                                                           // uniform
        s &= a.mask;
        const unsigned incl = block_scan_mask(s, a.mask, ps);
        run = (a.carries[diff_carry_slot(blockIdx.y, a.ntiles, blockIdx.x)] + incl - s) & a.mask;
    }
#pragma unroll
    for (int q = 0; q < MAX_PER; ++q) {
        if (v0 + q < v1) {
            unsigned e = sym[q];
            if (a.differential) e = run = (run + e) & a.mask;                       // gr_diff_encoder_bb.cc:56-57
            xs[nh + v0 + q] = r0 + v0 + q < a.nsym ? pts[e & 255u] : make_float2(0.f, 0.f);
        }
    }
    __syncthreads();

    // arb_kernel's polyphase step
    for (int k = t; k < kn; k += MOD_THREADS_FUSED) {
        const unsigned long long tl = Tm + (unsigned long long)k * a.sc.F;
        const unsigned pl = rb + (unsigned)k * a.sc.D + (unsigned)(tl >> 23);
        const int off = (int)(pl / R), j = (int)(pl - (unsigned)off * R);
        const float acc = (float)(unsigned)(tl & 0x7fffffu) * (1.0f / 8388608.0f);
        const float2 *h = hs + j * a.S;
        const float2 *x = xs + off;
        const int n = a.tpf;
        float2 r;
        if (GENERIC) {
            // gr_fir_ccf_generic (gr_fir_XXX_generic.cc.t:59-78): two accumulators, the tail into acc0, unfused
            float2 ac[2], dc[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) { ac[q] = make_float2(0.f, 0.f); dc[q] = make_float2(0.f, 0.f); }
            const int nn2 = (n / 2) * 2;
            int i = 0;
#pragma unroll 4
            for (; i < nn2; i += 2) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float2 hq = h[i + q];
                    const float2 xq = x[i + q];
                    ac[q] = mac_unfused(ac[q], hq.x, xq);
                    dc[q] = mac_unfused(dc[q], hq.y, xq);
                }
            }
            for (; i < n; ++i) {
                const float2 h0 = h[i];
                const float2 x0 = x[i];
                ac[0] = mac_unfused(ac[0], h0.x, x0);
                dc[0] = mac_unfused(dc[0], h0.y, x0);
            }
            const float2 o0 = add(ac[0], ac[1]), o1 = add(dc[0], dc[1]);
            r = mac_unfused(o0, acc, o1);                                           // o0 + o1*acc (.cc:187)
        } else {
            float2 a0 = make_float2(0.f, 0.f), a1 = make_float2(0.f, 0.f);
            int i = 0;
#pragma unroll 4
            for (; i + 1 < n; i += 2) {
                const float2 h0 = h[i], h1 = h[i + 1];
                a0 = mac_fma(a0, __builtin_fmaf(acc, h0.y, h0.x), x[i]);
                a1 = mac_fma(a1, __builtin_fmaf(acc, h1.y, h1.x), x[i + 1]);
            }
            if (i < n) a0 = mac_fma(a0, __builtin_fmaf(acc, h[i].y, h[i].x), x[i]);
            r = add(a0, a1);
        }
        out[k] = r;
    }
}

// ---- after the call: the stream's last tpf symbols and its last byte -----------------------------------------------------------
// One workgroup per stream.  Lane i makes history item i, symbol nsym - tpf + i of the call: an item of the old history
// where that lies in front of the call, else the point of the encoder's output there, which is last_out (now the
// state behind the call) minus the mapped symbols behind it.
__global__ void __launch_bounds__(128) mod_state_kernel(ModLaunch a)
{
    const int i = threadIdx.x;
    const unsigned char *__restrict__ in = a.in + (long long)blockIdx.x * a.n_bytes;
    float2 *hist = a.hist + (long long)blockIdx.x * a.tpf;
    const unsigned cb = a.carry_byte[blockIdx.x];
    float2 p = make_float2(0.f, 0.f);
    if (i < a.tpf) {
        const long long r = a.nsym - a.tpf + i;
        if (r < 0) {
            p = hist[a.nsym + i];
        } else {
            unsigned e = mod_symbol(a, in, cb, r, a.map);
            if (a.differential) {
                e = a.last_out[blockIdx.x];
                for (long long q = r + 1; q < a.nsym; ++q) e -= mod_symbol(a, in, cb, q, a.map);
                e &= a.mask;
            }
            if (e < a.npoints) p = a.points[e];
        }
    }
    __syncthreads();                                    // every lane has read the old history and the carried byte
    if (i < a.tpf) hist[i] = p;
    if (i == 0 && a.n_bytes > 0) a.carry_byte[blockIdx.x] = in[a.n_bytes - 1];
}

// ---- engine 0's glue ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
mod_stage_bytes_kernel(const unsigned char *__restrict__ in, long long n_bytes, unsigned char *__restrict__ carry_byte,
                       unsigned char *__restrict__ staged)
{
    const unsigned char *__restrict__ x = in + (long long)blockIdx.y * n_bytes;
    unsigned char *__restrict__ y = staged + (long long)blockIdx.y * (n_bytes + 1);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i <= n_bytes; i += stride)
        y[i] = i == 0 ? carry_byte[blockIdx.y] : x[i - 1];
}

__global__ void __launch_bounds__(64) mod_keep_byte_kernel(const unsigned char *__restrict__ in, long long n_bytes, int nstreams,
                                                           unsigned char *__restrict__ carry_byte)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nstreams) carry_byte[s] = in[(long long)s * n_bytes + n_bytes - 1];
}

__global__ void __launch_bounds__(128)
mod_copy_items_kernel(const float2 *__restrict__ src, long long src_stride, float2 *__restrict__ dst, long long dst_stride, int n)
{
    for (int i = threadIdx.x; i < n; i += 128) dst[(long long)blockIdx.x * dst_stride + i] = src[(long long)blockIdx.x * src_stride + i];
}

unsigned grid_for(long long n)
{
    const long long b = (n + 255) / 256, cap = (long long)device_cus() * 32;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <bool GENERIC>
int fused_go(const ModLaunch &a, hipStream_t st)
{
    const size_t lds = (size_t)a.R * a.S * sizeof(float2) + (size_t)a.span_cap * sizeof(float2);
    if (int rc = allow_lds((const void *)mod_fused_kernel<GENERIC>, lds + sizeof(float2) * 256 + sizeof(unsigned) * MOD_THREADS_FUSED + 256))
        return rc;
    hipLaunchKernelGGL((mod_fused_kernel<GENERIC>), dim3((unsigned)a.ntiles, (unsigned)a.n_streams), dim3(MOD_THREADS_FUSED), lds, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

int modulator_fused_launch(bool generic, const ModLaunch &a, hipStream_t st)
{
    if (a.n_bytes <= 0 || a.n_streams <= 0) return GRHIP_OK;
    if (a.ntiles > 0x7fffffffLL || a.n_streams > 65535) return fail(GRHIP_EINVAL, "generic_mod: grid too large");
    if (a.tpf > 128 || a.npoints > 256 || a.span_cap > MOD_SPAN_ITEMS) return fail(GRHIP_EINVAL, "generic_mod: outside the fused kernel's limits");
    if (a.differential && a.ntiles > 0) {
        hipLaunchKernelGGL(mod_segment_sum_kernel, dim3((unsigned)a.ntiles, (unsigned)a.n_streams), dim3(MOD_THREADS_FUSED), 0, st, a);
        GRHIP_HIP(hipGetLastError());
        if (int rc = diff_carry_launch(a.carries, a.ntiles, a.mask + 1u, a.last_out, a.n_streams, st)) return rc;
    }
    if (a.ntiles > 0)
        if (int rc = generic ? fused_go<true>(a, st) : fused_go<false>(a, st)) return rc;
    hipLaunchKernelGGL(mod_state_kernel, dim3((unsigned)a.n_streams), dim3(128), 0, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int mod_stage_bytes_launch(const unsigned char *in, long long n_bytes, int nstreams, unsigned char *carry_byte, unsigned char *staged,
                           hipStream_t st)
{
    if (n_bytes <= 0 || nstreams <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(mod_stage_bytes_kernel, dim3(grid_for(n_bytes + 1), (unsigned)nstreams), dim3(256), 0, st, in, n_bytes, carry_byte, staged);
    GRHIP_HIP(hipGetLastError());
    hipLaunchKernelGGL(mod_keep_byte_kernel, dim3((unsigned)((nstreams + 63) / 64)), dim3(64), 0, st, in, n_bytes, nstreams, carry_byte);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int mod_copy_items_launch(const float2 *src, long long src_stride, float2 *dst, long long dst_stride, int n, int nstreams, hipStream_t st)
{
    if (n <= 0 || nstreams <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(mod_copy_items_kernel, dim3((unsigned)nstreams), dim3(128), 0, st, src, src_stride, dst, dst_stride, n);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
