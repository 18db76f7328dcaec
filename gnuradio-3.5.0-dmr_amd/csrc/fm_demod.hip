// fm_demod.hip -- the FM demodulator hier block of blks2impl/fm_demod.py:51-72 and nbfm_rx.py:67-88:
// gr_quadrature_demod_cf -> fm_deemph (gr_iir_filter_ffd over two taps a side) -> gr_fir_filter_fff(D, taps).
//
// The composed path runs the three blocks one after the other on work buffers of the handle; this file holds its
// demodulator (quad_demod_one over S streams whose history item is the carried sample) and the two small kernels
// that move the FIR's delay line in and out.
//
// fmd_fused_kernel is the three in one pass: 8 bytes read per input sample and 4 / D written, nothing in between.
// One workgroup per (stream, tile of FMD_TILE input samples):
//   (a) the tile and the W0 + ntaps - 1 samples in front of it (clipped at the call's start), demodulated with
//       quad_demod_one into LDS as floats; a tile that reaches the call's start puts the carried FIR delay line in
//       front of them;
//   (b) every lane walks a contiguous sub-chunk of the de-emphasis recurrence from a zero accumulator, in double.
//       The sub-chunk length is odd, so the 64 lanes of a wave read 64 different banks;
//   (c) y_end = a1^len y_start + e composes: an ordered scan over the wave (shuffles) and over the four waves (LDS)
//       gives every lane its true start;
//   (d) the walk again from there, (float)y written over q in place (the reference narrows in front of the FIR);
//   (e) the decimated outputs from LDS with f32 FMAs, consecutive lanes on consecutive outputs.
// The accumulator at the left edge of a tile that does not reach the call's start is taken as zero: W0 is chosen so
// that |a1|^W0 <= 2^-60, below the rounding of the doubles.  The last tile writes the carried state into the state's
// other copy (the first tile of the same launch reads the old one).
#include "device_math.h"
#include "fm_demod.h"
#include "iir.h"

namespace grhip {

namespace {

__device__ __forceinline__ void fmd_load_tab(float2 *s_tab, const float *__restrict__ tab)
{
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_tab[i] = make_float2(tab[i], tab[i + 1]);
}

// grid (blocks, S)
__global__ void __launch_bounds__(256)
fmd_demod_kernel(const float2 *__restrict__ in, int n_in, float gain, const float *__restrict__ tab,
                 const float2 *__restrict__ last, float *__restrict__ q, long long q_stride)
{
    __shared__ float2 s_tab[256];
    fmd_load_tab(s_tab, tab);
    __syncthreads();
    const int s = blockIdx.y;
    const float2 *__restrict__ x = in + (long long)s * n_in;
    float *__restrict__ o = q + (long long)s * q_stride;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_in; i += stride) {
        const float2 prev = i > 0 ? x[i - 1] : last[s];
        o[i] = quad_demod_one(x[i], prev, gain, s_tab);
    }
}

// grid (blocks, S)
__global__ void __launch_bounds__(256)
fmd_hist_in_kernel(const float *__restrict__ hist, int H, float *__restrict__ row, long long row_stride)
{
    const int s = blockIdx.y;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < H; k += gridDim.x * 256)
        row[(long long)s * row_stride + k] = hist[(long long)s * H + k];
}

__global__ void __launch_bounds__(256)
fmd_tail_kernel(const float2 *__restrict__ in, int n_in, const float *__restrict__ row, long long row_stride, int H,
                float2 *__restrict__ last, float *__restrict__ hist, int *__restrict__ d_produced, int produced)
{
    const int s = blockIdx.y;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < H; k += gridDim.x * 256)
        hist[(long long)s * H + k] = row[(long long)s * row_stride + n_in + k];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        last[s] = in[(long long)s * n_in + n_in - 1];
        if (s == 0 && d_produced) *d_produced = produced;
    }
}

// Sample u of a workgroup's LDS lies at word u + u / 64: one word of padding per 64.  Step (e) reads at a stride of D
// words across the lanes; with the padding the D rows of 64 words that a wave touches start on different banks, so a
// power-of-two D is conflict-free (an odd D is without it, and nearly so with it).
__device__ __forceinline__ int fmd_slot(int u) { return u + (u >> 6); }

// grid (tiles, S)
__global__ void __launch_bounds__(256)
fmd_fused_kernel(FmdFused a)
{
    __shared__ float s_y[FMD_SLOTS];
    __shared__ float2 s_tab[256];
    __shared__ double s_A[4], s_E[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y;
    const int H = a.ntaps - 1;
    const int E = a.W0 + H;
    const int t0 = blockIdx.x * FMD_TILE;
    const int t1 = a.n_in - t0 < FMD_TILE ? a.n_in : t0 + FMD_TILE;
    const int L0 = t0 > E ? t0 - E : 0;
    const int M = t1 - L0;                                  // <= FMD_TILE + W0 + H: fmd_slot(H + M) <= FMD_SLOTS (the launcher checks)
    const bool first = L0 == 0, final = t1 == a.n_in;
    const float2 *__restrict__ x = a.in + (long long)s * a.n_in;

    fmd_load_tab(s_tab, a.atan_tab);
    if (first)
        for (int k = tid; k < H; k += 256) s_y[fmd_slot(k)] = a.rd.hist[(long long)s * H + k];
    __syncthreads();
    // (a)
    for (int i = L0 + tid; i < t1; i += 256) {
        const float2 prev = i > 0 ? x[i - 1] : a.rd.last[s];
        s_y[fmd_slot(H + i - L0)] = quad_demod_one(x[i], prev, a.gain, s_tab);
    }
    __syncthreads();
    if (a.deemph) {
        const int Lc = ((M + 255) / 256) | 1;
        const int j0 = tid * Lc;
        const int j1 = j0 + Lc < M ? j0 + Lc : M;           // empty where j0 >= M
        float qfront = 0.f;
        if (j0 < M) qfront = j0 > 0 ? s_y[fmd_slot(H + j0 - 1)] : first ? a.rd.xs[(long long)s * IIR_HIST] : 0.f;
        // (b)
        double A = 1.0, e = 0.0;
        {
            float qp = qfront;
            for (int j = j0; j < j1; ++j) {
                const float q = s_y[fmd_slot(H + j)];
                double acc = __dmul_rn(a.b0, (double)q);
                acc = __dadd_rn(acc, __dmul_rn(a.b1, (double)qp));
                acc = __dadd_rn(acc, __dmul_rn(a.a1, e));
                e = acc;
                qp = q;
                A *= a.a1;
            }
        }
        // (c): inclusive scan of y -> A y + e, earlier lanes first
#pragma unroll
        for (int d = 1; d < 64; d *= 2) {
            const double Ao = __shfl_up(A, d), eo = __shfl_up(e, d);
            if (lane >= d) { e = A * eo + e; A = A * Ao; }
        }
        if (lane == 63) { s_A[wave] = A; s_E[wave] = e; }
        __syncthreads();
        double y = first ? a.rd.ys[(long long)s * IIR_HIST] : 0.0;
        for (int w = 0; w < wave; ++w) y = s_A[w] * y + s_E[w];
        {
            const double Ap = __shfl_up(A, 1), ep = __shfl_up(e, 1);
            if (lane > 0) y = Ap * y + ep;
        }
        // (d)
        float qp = qfront;
        for (int j = j0; j < j1; ++j) {
            const float q = s_y[fmd_slot(H + j)];
            double acc = __dmul_rn(a.b0, (double)q);
            acc = __dadd_rn(acc, __dmul_rn(a.b1, (double)qp));
            acc = __dadd_rn(acc, __dmul_rn(a.a1, y));
            s_y[fmd_slot(H + j)] = (float)acc;
            y = acc;
            qp = q;
        }
        if (final && j0 < M && j1 == M) {
            a.wr.xs[(long long)s * IIR_HIST] = qp;
            a.wr.ys[(long long)s * IIR_HIST] = y;
        }
        __syncthreads();
    }
    // (e)
    {
        const int jlo = t0 <= a.o0 ? 0 : (t0 - a.o0 + a.D - 1) / a.D;
        const int jhi = t1 <= a.o0 ? 0 : (t1 - a.o0 + a.D - 1) / a.D;
        float *__restrict__ o = a.out + (long long)s * a.produced;
        for (int j = jlo + tid; j < jhi; j += 256) {
            const int base = H + (int)(a.o0 + (long long)j * a.D) - L0;
            float acc = 0.f;
            for (int k = 0; k < a.ntaps; ++k) acc = __builtin_fmaf(a.taps[k], s_y[fmd_slot(base - k)], acc);
            o[j] = acc;
        }
    }
    if (final) {
        for (int k = tid; k < H; k += 256) a.wr.hist[(long long)s * H + k] = s_y[fmd_slot(a.n_in - L0 + k)];
        if (tid == 0) {
            a.wr.last[s] = x[a.n_in - 1];
            if (s == 0 && a.d_produced) *a.d_produced = a.produced;
        }
    }
}

inline unsigned fmd_blocks(long long n)
{
    long long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}

}  // namespace

int fmd_demod_launch(const float2 *in, int n_in, int nstreams, float gain, const float *atan_tab, const float2 *last, float *q,
                     long long q_stride, hipStream_t st)
{
    if (n_in <= 0 || nstreams <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(fmd_demod_kernel, dim3(fmd_blocks(n_in), nstreams), dim3(256), 0, st, in, n_in, gain, atan_tab, last, q,
                       q_stride);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int fmd_hist_in_launch(const float *hist, int H, int nstreams, float *row, long long row_stride, hipStream_t st)
{
    if (H <= 0 || nstreams <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(fmd_hist_in_kernel, dim3(fmd_blocks(H), nstreams), dim3(256), 0, st, hist, H, row, row_stride);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int fmd_tail_launch(const float2 *in, int n_in, int nstreams, const float *row, long long row_stride, int H, float2 *last,
                    float *hist, int *d_produced, int produced, hipStream_t st)
{
    if (n_in <= 0 || nstreams <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(fmd_tail_kernel, dim3(fmd_blocks(H), nstreams), dim3(256), 0, st, in, n_in, row, row_stride, H, last, hist,
                       d_produced, produced);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int fmd_fused_launch(const FmdFused &a, hipStream_t st)
{
    if (a.n_in <= 0 || a.nstreams <= 0) return GRHIP_OK;
    const int H = a.ntaps - 1;
    if (a.ntaps < 1 || H > FMD_MAX_HIST || a.W0 < 0 || a.W0 > FMD_TILE / 8 || a.D < 1 || a.o0 < 0 || a.o0 >= a.D ||
        (a.deemph && a.W0 < 1) || H + FMD_TILE + a.W0 + H + (H + FMD_TILE + a.W0 + H) / 64 + 1 > FMD_SLOTS)
        return fail(GRHIP_EINVAL, "fm_demod: the fused kernel cannot take this shape");
    const unsigned tiles = (unsigned)(((long long)a.n_in + FMD_TILE - 1) / FMD_TILE);
    hipLaunchKernelGGL(fmd_fused_kernel, dim3(tiles, a.nstreams), dim3(256), 0, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
