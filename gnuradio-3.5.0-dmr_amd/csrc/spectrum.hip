// spectrum.hip -- kernels of the spectrum-estimate blocks: gr_complex_to_mag_squared, gr_single_pole_iir_filter_ff,
// gr_nlog10_ff and gr_keep_one_in_n, the stages of blks2.logpwrfft behind its transform (logpwrfft.py:57-63).
//
// Every arithmetic step is written with the round-to-nearest intrinsics, so none can be contracted to an FMA whatever
// the flags: mag^2 is two float products and one add (gr_complex_to_xxx.cc:198), the IIR two double products and one
// double add narrowed to float (gr_single_pole_iir.h:93 with tap_type double, o_type float).
#include <cmath>

#include "spectrum.h"
#include "spectrum_math.h"

namespace grhip {

namespace {

constexpr int THREADS = 256;
constexpr long long MAX_BLOCKS = 8 * 256;       // memory-bound element-wise passes: grid-stride from here on

unsigned blocks_for(long long n)
{
    const long long b = (n + THREADS - 1) / THREADS;
    return (unsigned)(b < 1 ? 1 : b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

__global__ void __launch_bounds__(THREADS)
mag_squared_kernel(const float2 *__restrict__ in, float *__restrict__ out, long long n)
{
    for (long long i = blockIdx.x * (long long)THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * THREADS) {
        const float2 v = in[i];
        out[i] = mag_squared_val(v.x, v.y);
    }
}

__global__ void __launch_bounds__(THREADS)
mag_kernel(const float2 *__restrict__ in, float *__restrict__ out, long long n)
{
    for (long long i = blockIdx.x * (long long)THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * THREADS) {
        const float2 v = in[i];
        out[i] = mag_val(v.x, v.y);
    }
}

__global__ void __launch_bounds__(THREADS)
nlog10_kernel(const float *in, float *out, long long count, float n, float k)
{
    for (long long i = blockIdx.x * (long long)THREADS + threadIdx.x; i < count; i += (long long)gridDim.x * THREADS)
        out[i] = nlog10_val(in[i], n, k);
}

// W: unsigned (items of whole, aligned words) or unsigned char
template <class W>
__global__ void __launch_bounds__(THREADS)
keep_one_kernel(const W *__restrict__ in, W *__restrict__ out, long long words, long long n_in, long long n_out,
                long long first, long long n, long long total)
{
    for (long long i = blockIdx.x * (long long)THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * THREADS) {
        const long long item = i / words, w = i - item * words;
        const long long s = item / n_out, o = item - s * n_out;
        out[i] = in[(s * n_in + first + o * n) * words + w];
    }
}

// One lane per (chunk, stream, element) walks its chunk of the item axis in order, the state in a register; the loads of
// the next four items are issued before the four dependent double chains of the current ones.
//   ENDS: start from 0, write nothing but the value after the chunk (ends[chunk][lane]): the chunk's local answer.
//   else: start from start[chunk][lane] (the state itself when there is one chunk), write every y, and the last chunk
//         stores the state.
//   LOG (not with ENDS): what is written is nlog10_val(y, log_n, log_k) of every y (the last two stages of
//         blks2.logpwrfft in one pass, logpwrfft.py:58-63); the recurrence and the stored state stay linear.
template <bool ENDS, bool LOG = false>
__global__ void __launch_bounds__(THREADS)
iir_walk_kernel(const float *in, float *out, long long n, int lanes, int vlen, long long chunk, int nchunks,
                double alpha, double oma, const float *start, float *ends, float *state, float log_n, float log_k)
{
    const long long id = blockIdx.x * (long long)THREADS + threadIdx.x;
    if (id >= (long long)lanes * nchunks) return;
    const int c = (int)(id / lanes), l = (int)(id - (long long)c * lanes);
    const int s = l / vlen, e = l - s * vlen;
    const long long j0 = c * chunk, j1 = j0 + chunk < n ? j0 + chunk : n;
    const long long base = ((long long)s * n + j0) * vlen + e;
    const float *p = in + base;
    float *q = out + base;
    float y = ENDS ? 0.f : start[id];
    float xa[4], xb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xa[i] = j0 + i < j1 ? p[(long long)i * vlen] : 0.f;
    for (long long j = j0; j < j1; j += 4) {
        p += 4LL * vlen;
#pragma unroll
        for (int i = 0; i < 4; ++i) xb[i] = j + 4 + i < j1 ? p[(long long)i * vlen] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (j + i < j1) {
                y = (float)__dadd_rn(__dmul_rn(alpha, (double)xa[i]), __dmul_rn(oma, (double)y));
                if (!ENDS) q[(long long)i * vlen] = LOG ? nlog10_val(y, log_n, log_k) : y;
            }
        }
        q += 4LL * vlen;
#pragma unroll
        for (int i = 0; i < 4; ++i) xa[i] = xb[i];
    }
    if (ENDS) ends[id] = y;
    else if (c == nchunks - 1) state[l] = y;
}

// The recurrence is affine in its start value: after a chunk of len items, y = local_end + (1 - alpha)^len * y_start.
// One lane per (stream, element) chains the chunks' local ends into every chunk's start value.
__global__ void __launch_bounds__(THREADS)
iir_carry_kernel(const float *__restrict__ ends, float *__restrict__ start, const float *__restrict__ state, int lanes,
                 int nchunks, double p_chunk)
{
    const int l = blockIdx.x * THREADS + threadIdx.x;
    if (l >= lanes) return;
    float y = state[l];
    for (int c = 0; c < nchunks; ++c) {
        start[(long long)c * lanes + l] = y;
        y = (float)__dadd_rn((double)ends[(long long)c * lanes + l], __dmul_rn(p_chunk, (double)y));
    }
}

}  // namespace

int mag_squared_launch(const float2 *in, float *out, long long n, hipStream_t st)
{
    if (n <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(mag_squared_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, st, in, out, n);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int mag_launch(const float2 *in, float *out, long long n, hipStream_t st)
{
    if (n <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(mag_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, st, in, out, n);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int nlog10_launch(const float *in, float *out, long long count, float n, float k, hipStream_t st)
{
    if (count <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(nlog10_kernel, dim3(blocks_for(count)), dim3(THREADS), 0, st, in, out, count, n, k);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int keep_one_launch(const void *in, void *out, size_t item_size, long long n_in, long long n_out, long long first,
                    long long n, int nstreams, hipStream_t st)
{
    if (n_out <= 0) return GRHIP_OK;
    if (first < 0 || n < 1 || first + (n_out - 1) * n >= n_in) return fail(GRHIP_EINVAL, "keep_one_in_n: kept item past the input");
    const bool words = !(item_size & 3) && !((uintptr_t)in & 3) && !((uintptr_t)out & 3);
    const long long w = words ? (long long)(item_size / 4) : (long long)item_size, total = (long long)nstreams * n_out * w;
    if (words)
        hipLaunchKernelGGL(keep_one_kernel<unsigned>, dim3(blocks_for(total)), dim3(THREADS), 0, st, (const unsigned *)in,
                           (unsigned *)out, w, n_in, n_out, first, n, total);
    else
        hipLaunchKernelGGL(keep_one_kernel<unsigned char>, dim3(blocks_for(total)), dim3(THREADS), 0, st,
                           (const unsigned char *)in, (unsigned char *)out, w, n_in, n_out, first, n, total);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

bool iir_chunked(bool fast, const IirLaunch &a)
{
    return fast && (long long)a.nstreams * a.vlen < IIR_FILL_LANES && a.n > IIR_CHUNK;
}

template <bool ENDS>
static int walk(const IirLaunch &a, int lanes, long long chunk, int nchunks, const float *start, float *ends, hipStream_t st)
{
    const long long blocks = ((long long)lanes * nchunks + THREADS - 1) / THREADS;
    if (blocks > 0x7fffffffLL) return fail(GRHIP_EINVAL, "single_pole_iir: too many lanes in one call");
    if (!ENDS && a.log)
        hipLaunchKernelGGL((iir_walk_kernel<false, true>), dim3((unsigned)blocks), dim3(THREADS), 0, st, a.in, a.out, a.n, lanes,
                           a.vlen, chunk, nchunks, a.alpha, 1.0 - a.alpha, start, ends, a.state, a.log_n, a.log_k);
    else
        hipLaunchKernelGGL((iir_walk_kernel<ENDS>), dim3((unsigned)blocks), dim3(THREADS), 0, st, a.in, a.out, a.n, lanes,
                           a.vlen, chunk, nchunks, a.alpha, 1.0 - a.alpha, start, ends, a.state, 0.f, 0.f);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int single_pole_iir_launch(bool fast, const IirLaunch &a, DevBuf &scratch, hipStream_t st)
{
    if (a.n <= 0) return GRHIP_OK;
    const long long lanes_ll = (long long)a.nstreams * a.vlen;
    if (lanes_ll > 0x7fffffffLL) return fail(GRHIP_EINVAL, "single_pole_iir: streams x vlen past 2^31");
    const int lanes = (int)lanes_ll;
    if (!iir_chunked(fast, a))
        return walk<false>(a, lanes, a.n, 1, a.state, nullptr, st);
    const long long nc = (a.n + IIR_CHUNK - 1) / IIR_CHUNK;
    if (nc > 0x7fffffffLL) return fail(GRHIP_EINVAL, "single_pole_iir: too many items in one call");
    const int nchunks = (int)nc;
    const size_t plane = (size_t)lanes * nchunks * sizeof(float);
    int rc = scratch.reserve(2 * plane);
    if (rc) return rc;
    float *ends = scratch.as<float>(), *start = ends + (size_t)lanes * nchunks;
    if ((rc = walk<true>(a, lanes, IIR_CHUNK, nchunks, nullptr, ends, st))) return rc;
    hipLaunchKernelGGL(iir_carry_kernel, dim3((lanes + THREADS - 1) / THREADS), dim3(THREADS), 0, st, ends, start, a.state,
                       lanes, nchunks, std::pow(1.0 - a.alpha, (double)IIR_CHUNK));
    GRHIP_HIP(hipGetLastError());
    return walk<false>(a, lanes, IIR_CHUNK, nchunks, start, nullptr, st);
}

}  // namespace grhip
