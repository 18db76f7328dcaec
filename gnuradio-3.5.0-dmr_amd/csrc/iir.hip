// iir.hip -- gr_iir_filter_ffd (filter/gr_iir_filter_ffd.cc:56-82, filter/gri_iir.h:126-163): float in, float out,
// taps and accumulator in double.  One output is
//     acc = ff[0] x[t];  acc += ff[i] x[t-i], i = 1 .. n-1;  acc += fb[i] y[t-i], i = 1 .. m-1;  out = (float)acc
// with y the accumulators in double, every product and every add rounded once, in that order.
//
// iirffd_walk_kernel   the recurrence in order, one wavefront per stream: the wave loads a window of inputs coalesced into
//                   LDS behind the delay line (the next window's loads in flight), lane 0 walks the window and leaves
//                   the accumulators in LDS behind the output delay line, the wave narrows and stores them coalesced.
//                   Bit for bit the reference; GRHIP_MODE_GENERIC, and every mode where the chunked form does not apply.
//
// The chunked form.  With K = m - 1 the recurrence is linear in the K last accumulators: over a chunk of L items
// state_end = C^L state_start + (the end reached from a zero state), C the companion matrix of fb.
//   iirffd_chunk_kernel<false>   one lane per (stream, chunk): the chunk's walk from zero accumulators (the n - 1 inputs in
//                             front of it are the real ones: the buffer's, or the carried delay line's), leaves the end.
//   iirffd_carry_kernel          one lane per stream chains the chunks: start of the next = C^256 start + end, in double.
//   iirffd_chunk_kernel<true>    the walk again from every chunk's true start, writing the outputs; the last chunk's lane
//                             writes the stream's output delay line.
//   iirffd_xstate_kernel         the stream's input delay line (after the walks, which read the old one).
#include <cmath>
#include <cstring>

#include "iir.h"

namespace grhip {

namespace {

constexpr int IIR_WIN = 1024;

__global__ void __launch_bounds__(64)
iirffd_walk_kernel(const float *__restrict__ in, float *__restrict__ out, long long in_stride, long long out_stride,
                long long n_items, int n, int m,
                const double *__restrict__ taps, float *__restrict__ xstate, double *__restrict__ ystate)
{
    // s_x[IIR_HIST + i] is item i of the window, s_x[IIR_HIST - k] the item k in front of it (k <= 63); s_y alike
    __shared__ float s_x[IIR_HIST + IIR_WIN];
    __shared__ double s_y[IIR_HIST + IIR_WIN];
    __shared__ double s_ff[IIR_MAX_TAPS], s_fb[IIR_MAX_TAPS];
    const int s = blockIdx.x, lane = threadIdx.x;
    const float *__restrict__ x = in + (long long)s * in_stride;
    float *__restrict__ y = out + (long long)s * out_stride;
    float *__restrict__ xs = xstate + (long long)s * IIR_HIST;
    double *__restrict__ ys = ystate + (long long)s * IIR_HIST;
    s_ff[lane] = lane < n ? taps[lane] : 0.0;
    s_fb[lane] = lane < m ? taps[IIR_MAX_TAPS + lane] : 0.0;
    if (lane < IIR_HIST - 1) {
        s_x[IIR_HIST - 1 - lane] = lane < n - 1 ? xs[lane] : 0.f;
        s_y[IIR_HIST - 1 - lane] = lane < m - 1 ? ys[lane] : 0.0;
    }
    float v[IIR_WIN / 64];
#pragma unroll
    for (int q = 0; q < IIR_WIN / 64; ++q) {
        const long long i = lane + 64 * q;
        v[q] = i < n_items ? x[i] : 0.f;
    }
    for (long long base = 0; base < n_items; base += IIR_WIN) {
        const int cnt = (int)(n_items - base < IIR_WIN ? n_items - base : IIR_WIN);
#pragma unroll
        for (int q = 0; q < IIR_WIN / 64; ++q) s_x[IIR_HIST + lane + 64 * q] = v[q];
        __syncthreads();
        // the next window's loads, in flight while this one is walked
#pragma unroll
        for (int q = 0; q < IIR_WIN / 64; ++q) {
            const long long i = base + IIR_WIN + lane + 64 * q;
            v[q] = i < n_items ? x[i] : 0.f;
        }
        if (lane == 0) {
            const double ff0 = s_ff[0], fb1 = s_fb[1];
            double y1 = s_y[IIR_HIST - 1];
            for (int t = 0; t < cnt; ++t) {
                const int p = IIR_HIST + t;
                double acc = __dmul_rn(ff0, (double)s_x[p]);                                        // gri_iir.h:141
                for (int i = 1; i < n; ++i) acc = __dadd_rn(acc, __dmul_rn(s_ff[i], (double)s_x[p - i]));   // :142-143
                if (m > 1) acc = __dadd_rn(acc, __dmul_rn(fb1, y1));                                // :144-145
                for (int i = 2; i < m; ++i) acc = __dadd_rn(acc, __dmul_rn(s_fb[i], s_y[p - i]));
                s_y[p] = acc;
                y1 = acc;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < IIR_WIN / 64; ++q) {
            const int i = lane + 64 * q;
            if (i < cnt) y[base + i] = (float)s_y[IIR_HIST + i];                                    // :162
        }
        if (base + IIR_WIN < n_items) {
            // the window's last 63 items become the delay line in front of the next
            float hx = 0.f;
            double hy = 0.0;
            if (lane < IIR_HIST - 1) { hx = s_x[IIR_WIN + 1 + lane]; hy = s_y[IIR_WIN + 1 + lane]; }
            __syncthreads();
            if (lane < IIR_HIST - 1) { s_x[1 + lane] = hx; s_y[1 + lane] = hy; }
        } else {
            if (lane < n - 1) xs[lane] = s_x[IIR_HIST + cnt - 1 - lane];
            if (lane < m - 1) ys[lane] = s_y[IIR_HIST + cnt - 1 - lane];
        }
    }
}

// One lane per (stream, chunk).  start / ends = [total][IIR_MAX_K] doubles, entry j the accumulator j + 1 items back.
template <bool WRITE>
__global__ void __launch_bounds__(64)
iirffd_chunk_kernel(const float *__restrict__ in, float *__restrict__ out, long long in_stride, long long out_stride,
                 long long n_items, int nch, long long total,
                 int n, int m, const double *__restrict__ taps, const float *__restrict__ xstate,
                 double *__restrict__ ystate, const double *__restrict__ start, double *__restrict__ ends)
{
    const long long q = (long long)blockIdx.x * 64 + threadIdx.x;
    if (q >= total) return;
    const long long s = q / nch;
    const int c = (int)(q - s * nch);
    const int K = m - 1;
    const float *__restrict__ x = in + s * in_stride;
    const float *__restrict__ xs = xstate + s * IIR_HIST;
    const long long i0 = (long long)c * IIR_CHUNK;
    const long long i1 = i0 + IIR_CHUNK < n_items ? i0 + IIR_CHUNK : n_items;
    double fb[IIR_MAX_K], yh[IIR_MAX_K];
#pragma unroll
    for (int j = 0; j < IIR_MAX_K; ++j) {
        fb[j] = j < K ? taps[IIR_MAX_TAPS + 1 + j] : 0.0;
        yh[j] = (WRITE && j < K) ? start[q * IIR_MAX_K + j] : 0.0;
    }
    const double ff0 = taps[0];
    for (long long i = i0; i < i1; ++i) {
        double acc = __dmul_rn(ff0, (double)x[i]);
        for (int j = 1; j < n; ++j) {
            const long long k = i - j;
            const float xv = k >= 0 ? x[k] : xs[-1 - k];
            acc = __dadd_rn(acc, __dmul_rn(taps[j], (double)xv));
        }
#pragma unroll
        for (int j = 0; j < IIR_MAX_K; ++j)
            if (j < K) acc = __dadd_rn(acc, __dmul_rn(fb[j], yh[j]));
        if (WRITE) out[s * out_stride + i] = (float)acc;
#pragma unroll
        for (int j = IIR_MAX_K - 1; j > 0; --j) yh[j] = yh[j - 1];
        yh[0] = acc;
    }
    if (!WRITE) {
#pragma unroll
        for (int j = 0; j < IIR_MAX_K; ++j) ends[q * IIR_MAX_K + j] = yh[j];
    } else if (c == nch - 1) {
#pragma unroll
        for (int j = 0; j < IIR_MAX_K; ++j)
            if (j < K) ystate[s * IIR_HIST + j] = yh[j];
    }
}

// One lane per stream.
__global__ void __launch_bounds__(64)
iirffd_carry_kernel(int nstreams, int nch, int K, IirCarry cm, const double *__restrict__ ystate,
                 const double *__restrict__ ends, double *__restrict__ start)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nstreams) return;
    double st[IIR_MAX_K];
#pragma unroll
    for (int j = 0; j < IIR_MAX_K; ++j) st[j] = j < K ? ystate[(long long)s * IIR_HIST + j] : 0.0;
    for (int c = 0; c < nch; ++c) {
        const long long q = (long long)s * nch + c;
        double nx[IIR_MAX_K];
#pragma unroll
        for (int r = 0; r < IIR_MAX_K; ++r) {
            start[q * IIR_MAX_K + r] = st[r];
            double a = ends[q * IIR_MAX_K + r];
#pragma unroll
            for (int k = 0; k < IIR_MAX_K; ++k) a += cm.full[r * IIR_MAX_K + k] * st[k];
            nx[r] = a;
        }
#pragma unroll
        for (int r = 0; r < IIR_MAX_K; ++r) st[r] = r < K ? nx[r] : 0.0;
    }
}

// One wavefront per stream; n_items >= IIR_HIST here (a chunked call is longer than one chunk).
__global__ void __launch_bounds__(64)
iirffd_xstate_kernel(const float *__restrict__ in, long long in_stride, long long n_items, int n, float *__restrict__ xstate)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (lane < n - 1) xstate[(long long)s * IIR_HIST + lane] = in[(long long)s * in_stride + n_items - 1 - lane];
}

inline int iir_chunks(int n_items) { return (n_items + IIR_CHUNK - 1) / IIR_CHUNK; }

}  // namespace

// largest ||C^j||_inf, j = 1 .. IIR_CHUNK, the chunked form accepts: the zero-input response does not grow
constexpr double IIR_MAX_GROWTH = 64.0;

// whether the chunked form may run these taps, and C^IIR_CHUNK if so
bool iir_plan(const std::vector<double> &f, const std::vector<double> &b, IirCarry *out)
{
    if (f.empty() || b.empty()) return false;
    const int K = (int)b.size() - 1;
    if (K > IIR_MAX_K) return false;
    for (double t : f) if (!std::isfinite(t)) return false;
    for (double t : b) if (!std::isfinite(t)) return false;
    constexpr int W = IIR_MAX_K;
    double C[W * W] = {}, P[W * W] = {}, T[W * W];
    for (int k = 0; k < K; ++k) C[k] = b[(size_t)k + 1];
    for (int r = 1; r < K; ++r) C[r * W + r - 1] = 1.0;
    for (int r = 0; r < W; ++r) P[r * W + r] = r < K ? 1.0 : 0.0;
    for (int j = 1; j <= IIR_CHUNK; ++j) {
        for (int r = 0; r < W; ++r)
            for (int c = 0; c < W; ++c) {
                double a = 0.0;
                for (int k = 0; k < W; ++k) a += C[r * W + k] * P[k * W + c];
                T[r * W + c] = a;
            }
        double norm = 0.0;
        for (int r = 0; r < W; ++r) {
            double row = 0.0;
            for (int c = 0; c < W; ++c) { P[r * W + c] = T[r * W + c]; row += std::fabs(T[r * W + c]); }
            if (!(row <= norm)) norm = row;         // a NaN row lands here too
        }
        if (!(norm <= IIR_MAX_GROWTH)) return false;
    }
    if (out) memcpy(out->full, P, sizeof(P));
    return true;
}

size_t iir_scratch_bytes(const IirLaunch &a)
{
    return (size_t)a.nstreams * iir_chunks(a.n_items) * 2 * IIR_MAX_K * sizeof(double);
}

int iir_walk_launch(const IirLaunch &a, hipStream_t st)
{
    if (a.n_items <= 0 || a.nstreams <= 0) return GRHIP_OK;
    if (a.n < 1 || a.n > IIR_MAX_TAPS || a.m < 1 || a.m > IIR_MAX_TAPS) return fail(GRHIP_EINVAL, "iir: tap counts out of range");
    hipLaunchKernelGGL(iirffd_walk_kernel, dim3(a.nstreams), dim3(64), 0, st, a.in, a.out, a.in_stride, a.out_stride,
                       (long long)a.n_items, a.n, a.m, a.taps, a.xstate, a.ystate);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int iir_chunked_launch(const IirLaunch &a, const IirCarry &c, void *scratch, hipStream_t st)
{
    if (a.n_items <= IIR_CHUNK || a.nstreams <= 0 || a.n < 1 || a.n > IIR_MAX_TAPS || a.m < 1 || a.m - 1 > IIR_MAX_K || !scratch)
        return fail(GRHIP_EINVAL, "iir: the chunked form cannot take this call");
    const int nch = iir_chunks(a.n_items);
    const long long total = (long long)a.nstreams * nch;
    double *ends = (double *)scratch;
    double *start = ends + total * IIR_MAX_K;
    const unsigned blocks = (unsigned)((total + 63) / 64);
    if (a.m > 1) {
        hipLaunchKernelGGL((iirffd_chunk_kernel<false>), dim3(blocks), dim3(64), 0, st, a.in, a.out, a.in_stride, a.out_stride,
                           (long long)a.n_items, nch, total, a.n, a.m, a.taps, (const float *)a.xstate, a.ystate, (const double *)start, ends);
        GRHIP_HIP(hipGetLastError());
        hipLaunchKernelGGL(iirffd_carry_kernel, dim3((a.nstreams + 63) / 64), dim3(64), 0, st, a.nstreams, nch, a.m - 1, c,
                           (const double *)a.ystate, (const double *)ends, start);
        GRHIP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((iirffd_chunk_kernel<true>), dim3(blocks), dim3(64), 0, st, a.in, a.out, a.in_stride, a.out_stride,
                       (long long)a.n_items, nch, total,
                       a.n, a.m, a.taps, (const float *)a.xstate, a.ystate, (const double *)start, ends);
    GRHIP_HIP(hipGetLastError());
    if (a.n > 1) {
        hipLaunchKernelGGL(iirffd_xstate_kernel, dim3(a.nstreams), dim3(64), 0, st, a.in, a.in_stride, (long long)a.n_items, a.n, a.xstate);
        GRHIP_HIP(hipGetLastError());
    }
    return GRHIP_OK;
}

}  // namespace grhip
