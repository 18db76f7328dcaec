// cpm.hip -- the continuous-phase transmitter: gr_frequency_modulator_fc (general/gr_frequency_modulator_fc.cc:49-72),
// gr_bytes_to_syms (general/gr_bytes_to_syms.cc:45-71), gr_char_to_float (general/gri_char_to_float.cc:26-40),
// gr_chunks_to_symbols_bf (gengen/gr_chunks_to_symbols_XX.cc.t:51-74) and the fused modulator behind cpmmod_bc
// (gr-digital/lib/digital_cpmmod_bc.cc:44-72) and gmsk_mod (gr-digital/python/gmsk.py:84-120): kernels.
//
// The frequency modulator is phase += sensitivity * in[i] in double, out[i] = (cos, sin) of (float)phase, and after the
// last item of a work call |phase| > 16 pi is brought back by whole turns.
//
// fm_walk_kernel   the recurrence as the reference writes it, every double operation rounded once.  One wavefront per
//                  stream (the form of agc_walk_kernel): a window of samples goes coalesced into LDS with the next
//                  window's loads in flight, every lane walks the recurrence out of LDS, lane l keeps the phase of
//                  sample l of each group of 64 and forms that sample's output, so the stores are coalesced.
//
// The scan (every mode but GENERIC), three launches whose order is the only ordering between workgroups:
//   fm_sums_kernel   per tile of FM_TILE items the sum of sensitivity * x in double
//   fm_carry_kernel  one wavefront per stream: the tile sums become the tiles' start phases from the call's entry
//                    phase; the total, wrapped by the reference's rule, becomes the stream's state
//   fm_tile_kernel   per tile a workgroup scan in double from the tile's start: a lane adds FM_PER consecutive items,
//                    the lanes' totals are scanned over the wave and the waves' over LDS.  phi - 2 pi rint(phi / 2 pi)
//                    in double, then the float polynomial sine and cosine, out through LDS in whole lines.
// A call of at most one tile is fm_tile_kernel<.., true> alone.  Every prefix is a sum of EARLIER items only, so what
// lies in front of a stream's first non-finite product stays finite, and everything from it on is NaN.
//
// The kernels take their frequency samples from a source: FloatSrc reads them; FusedSrc forms them from a tile's symbols
// (one byte per symbol, or per eight) against the interpolator's taps in LDS, in gr_fir_fff_generic's order, so that
// they are the floats the interpolator would have stored.
#include "cpm.h"
#include "cpm_blocks.h"
#include "device_math.h"
#include "grhip_internal.h"
#include "loop_math.h"

namespace grhip {

namespace {

constexpr double FM_INV_TWOPI = 0.15915494309189533577;
constexpr double FM_TWOPI_HI = 6.28318530717958647692, FM_TWOPI_LO = 2.4492935982947064e-16;      // 2 pi in two doubles

// gr_frequency_modulator_fc.cc:66-69
__device__ __forceinline__ double fm_wrap(double phase)
{
    if (fabs(phase) > 16 * CPM_PI) {
        const double ii = trunc(phase / (2 * CPM_PI));
        phase = __dsub_rn(phase, __dmul_rn(__dmul_rn(ii, 2.0), CPM_PI));
    }
    return phase;
}

// ---- the serial walk ----------------------------------------------------------------------------------------------------
constexpr int FM_WIN = 1024;

__global__ void __launch_bounds__(64)
fm_walk_kernel(const float *__restrict__ in, float2 *__restrict__ out, long long n, double sens, double *__restrict__ phase)
{
    __shared__ float s_x[FM_WIN];
    const int s = blockIdx.x, lane = threadIdx.x;
    const float *__restrict__ x = in + (long long)s * n;
    float2 *__restrict__ y = out + (long long)s * n;
    double ph = phase[s];
    float v[FM_WIN / 64];
#pragma unroll
    for (int q = 0; q < FM_WIN / 64; ++q) {
        const long long i = lane + 64 * q;
        v[q] = i < n ? x[i] : 0.f;
    }
    for (long long base = 0; base < n; base += FM_WIN) {
        const int m = (int)(n - base < FM_WIN ? n - base : FM_WIN);
#pragma unroll
        for (int q = 0; q < FM_WIN / 64; ++q) s_x[lane + 64 * q] = v[q];
        __syncthreads();
        // the next window's loads, in flight while this one is walked
#pragma unroll
        for (int q = 0; q < FM_WIN / 64; ++q) {
            const long long i = base + FM_WIN + lane + 64 * q;
            v[q] = i < n ? x[i] : 0.f;
        }
        for (int g0 = 0; g0 < m; g0 += 64) {
            const int cnt = m - g0 < 64 ? m - g0 : 64;
            double kp = ph;
            for (int j = 0; j < cnt; ++j) {
                ph = __dadd_rn(ph, __dmul_rn(sens, (double)s_x[g0 + j]));                 // .cc:58
                kp = lane == j ? ph : kp;
            }
            if (lane < cnt) {
                float oq, oi;
                sincos_rounded(__double2float_rn(kp), oq, oi);                             // :60, gr_sincosf takes a float
                y[base + g0 + lane] = make_float2(oi, oq);                                 // :61
            }
        }
        __syncthreads();
    }
    if (lane == 0) phase[s] = fm_wrap(ph);
}

// ---- the sources of frequency samples ---------------------------------------------------------------------------------------
// LDS index of a tile's item: a lane's FM_PER consecutive items lie 9 words apart from its neighbour's, not 8
__device__ __forceinline__ int fm_pad(int i) { return i + (i >> 3); }
constexpr int FM_TILE_PAD = FM_TILE + FM_TILE / 8;

struct FloatSrc {
    const float *in;
    struct Shared {};
    // s_f[fm_pad(i)] = item o0 + i of stream s for i < m, zero behind; each lane reads back only what it wrote, or
    // after a barrier
    __device__ __forceinline__ void stage(Shared &, float *s_f, int s, long long o0, int m, long long n, bool) const
    {
        const float *__restrict__ x = in + (long long)s * n + o0;
#pragma unroll
        for (int j = 0; j < FM_PER; ++j) {
            const int i = threadIdx.x + j * FM_THREADS;
            s_f[fm_pad(i)] = i < m ? x[i] : 0.f;
        }
    }
};

struct FusedSrc {
    CpmFused a;
    struct Shared {
        float rows[CPM_FUSED_MAX_ROWS];
        float sym[FM_TILE + CPM_FUSED_MAX_NT];
    };
    // symbol j of the call's stream s; j < 0: the history
    __device__ __forceinline__ float symbol(int s, long long j) const
    {
        if (j < 0) return a.hist[(long long)(s + 1) * (a.nt - 1) + j];
        const unsigned char *__restrict__ x = a.in + (long long)s * a.n_in;
        if (a.bits) return ((x[j >> 3] >> (7 - (int)(j & 7))) & 1) ? 1.f : -1.f;          // gr_bytes_to_syms.cc:60-67
        return (float)(signed char)x[j];                                                   // gri_char_to_float.cc:29
    }
    __device__ __forceinline__ void stage(Shared &sh, float *s_f, int s, long long o0, int m, long long n, bool store) const
    {
        const long long i0 = o0 / a.sps;
        const int off = (int)(o0 - i0 * a.sps);
        const int count = (off + m - 1) / a.sps + a.nt;             // symbols i0 - (nt - 1) .. i0 + (off + m - 1) / sps
        for (int q = threadIdx.x; q < count; q += FM_THREADS) sh.sym[q] = symbol(s, i0 - (a.nt - 1) + q);
        for (int q = threadIdx.x; q < a.sps * a.nt; q += FM_THREADS) sh.rows[q] = a.rows[q];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FM_PER; ++j) {
            const int i = threadIdx.x + j * FM_THREADS;
            float f = 0.f;
            if (i < m) {
                const int sym = (off + i) / a.sps, filt = off + i - sym * a.sps;
                f = fir_fff_generic_sum(&sh.rows[filt * a.nt], &sh.sym[sym], a.nt);        // gr_interp_fir_filter_XXX.cc.t:139
                if (store && a.freq) a.freq[(long long)s * n + o0 + i] = f;
            }
            s_f[fm_pad(i)] = f;
        }
    }
};

// ---- the scan -----------------------------------------------------------------------------------------------------------
// grid (tiles, S); sums [S][tiles]
template <class Src>
__global__ void __launch_bounds__(FM_THREADS)
fm_sums_kernel(Src src, long long n, double sens, double *__restrict__ sums)
{
    __shared__ typename Src::Shared sh;
    __shared__ float s_f[FM_TILE_PAD];
    __shared__ double s_w[FM_THREADS / 64];
    const int s = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long o0 = (long long)blockIdx.x * FM_TILE;
    const int m = (int)(n - o0 < FM_TILE ? n - o0 : FM_TILE);
    src.stage(sh, s_f, s, o0, m, n, false);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < FM_PER; ++j) {
        const int i = threadIdx.x + j * FM_THREADS;
        if (i < m) acc += sens * (double)s_f[fm_pad(i)];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d);
    if (lane == 0) s_w[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) sums[(long long)s * gridDim.x + blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// one wavefront per stream: q[t] <- entry phase + the sums in front of tile t; the stream's state <- the wrapped total
__global__ void __launch_bounds__(64)
fm_carry_kernel(double *__restrict__ sums, long long ntiles, double *__restrict__ phase)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    double *__restrict__ q = sums + (long long)s * ntiles;
    double carry = phase[s];
    for (long long base = 0; base < ntiles; base += 64) {
        const long long i = base + lane;
        double inc = i < ntiles ? q[i] : 0.0;
#pragma unroll
        for (int d = 1; d < 64; d *= 2) {
            const double t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        const double before = __shfl_up(inc, 1);
        if (i < ntiles) q[i] = lane ? carry + before : carry;
        carry += __shfl(inc, 63);
    }
    if (lane == 0) phase[s] = fm_wrap(carry);
}

// grid (tiles, S).  SINGLE: the call is this one tile; the start is the stream's state, which the kernel leaves updated.
template <class Src, bool SINGLE>
__global__ void __launch_bounds__(FM_THREADS)
fm_tile_kernel(Src src, float2 *__restrict__ out, long long n, double sens, double *__restrict__ phase, const double *__restrict__ starts)
{
    __shared__ typename Src::Shared sh;
    __shared__ float s_f[FM_TILE_PAD];
    __shared__ float2 s_o[FM_TILE_PAD];
    __shared__ double s_w[FM_THREADS / 64];
    const int s = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long o0 = (long long)blockIdx.x * FM_TILE;
    const int m = (int)(n - o0 < FM_TILE ? n - o0 : FM_TILE);
    const double start = SINGLE ? phase[s] : starts[(long long)s * gridDim.x + blockIdx.x];
    src.stage(sh, s_f, s, o0, m, n, true);
    __syncthreads();
    const int b = threadIdx.x * FM_PER;
    double p[FM_PER], run = 0.0;
#pragma unroll
    for (int j = 0; j < FM_PER; ++j) {
        if (b + j < m) run += sens * (double)s_f[fm_pad(b + j)];
        p[j] = run;
    }
    double inc = run;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const double t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    double before = __shfl_up(inc, 1);
    if (lane == 0) before = 0.0;
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    for (int k = 0; k < w; ++k) before += s_w[k];
#pragma unroll
    for (int j = 0; j < FM_PER; ++j) {
        const double phi = start + (before + p[j]);
        const double k = rint(phi * FM_INV_TWOPI);
        const double r = fma(-k, FM_TWOPI_LO, fma(-k, FM_TWOPI_HI, phi));
        float sn, cs;
        sincos_fast(__double2float_rn(r), sn, cs);
        s_o[fm_pad(b + j)] = make_float2(cs, sn);
    }
    __syncthreads();
    float2 *__restrict__ y = out + (long long)s * n + o0;
#pragma unroll
    for (int j = 0; j < FM_PER; ++j) {
        const int i = threadIdx.x + j * FM_THREADS;
        if (i < m) y[i] = s_o[fm_pad(i)];
    }
    if (SINGLE && threadIdx.x == FM_THREADS - 1) phase[s] = fm_wrap(start + (before + run));
}

template <class Src>
int scan_launch(const Src &src, float2 *out, long long n, int nstreams, double sens, double *phase, double *scratch, hipStream_t st)
{
    if (n <= 0 || nstreams <= 0) return GRHIP_OK;
    if (nstreams > 65535) return fail(GRHIP_EINVAL, "frequency_modulator_fc: grid too large");
    const long long tiles = fm_tiles(n);
    if (tiles > 0x7fffffffLL) return fail(GRHIP_EINVAL, "frequency_modulator_fc: too many items for one call");
    if (tiles == 1) {
        hipLaunchKernelGGL((fm_tile_kernel<Src, true>), dim3(1, (unsigned)nstreams), dim3(FM_THREADS), 0, st, src, out, n, sens, phase,
                           (const double *)nullptr);
        GRHIP_HIP(hipGetLastError());
        return GRHIP_OK;
    }
    if (!scratch) return fail(GRHIP_EINVAL, "frequency_modulator_fc: no scratch for the tile sums");
    const dim3 grid((unsigned)tiles, (unsigned)nstreams);
    hipLaunchKernelGGL((fm_sums_kernel<Src>), grid, dim3(FM_THREADS), 0, st, src, n, sens, scratch);
    GRHIP_HIP(hipGetLastError());
    hipLaunchKernelGGL(fm_carry_kernel, dim3((unsigned)nstreams), dim3(64), 0, st, scratch, tiles, phase);
    GRHIP_HIP(hipGetLastError());
    hipLaunchKernelGGL((fm_tile_kernel<Src, false>), grid, dim3(FM_THREADS), 0, st, src, out, n, sens, phase, (const double *)scratch);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

__global__ void __launch_bounds__(64)
cpm_history_kernel(FusedSrc src, long long nsym, int nstreams)
{
    const int s = blockIdx.x * 64 + threadIdx.x, h = src.a.nt - 1;
    if (s >= nstreams) return;
    // entry k takes symbol nsym - h + k: the history's entry k + nsym or a symbol of the call, never an entry below k
    for (int k = 0; k < h; ++k) src.a.hist[(long long)s * h + k] = src.symbol(s, nsym - h + k);
}

// ---- one lane per output item ---------------------------------------------------------------------------------------------
constexpr int CPM_THREADS = 256;

unsigned blocks_for(long long n)
{
    const long long b = (n + CPM_THREADS - 1) / CPM_THREADS, cap = (long long)device_cus() * 32;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

__global__ void __launch_bounds__(CPM_THREADS)
bytes_to_syms_kernel(const unsigned char *__restrict__ in, long long in_stride, float *__restrict__ out, long long out_stride, long long n_out)
{
    const unsigned char *__restrict__ x = in + (long long)blockIdx.y * in_stride;
    float *__restrict__ y = out + (long long)blockIdx.y * out_stride;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += stride)
        y[o] = (float)(int)((((unsigned)x[o >> 3] >> (7 - (int)(o & 7))) & 0x1u) << 1) - 1.f;        // ((x >> b) & 1) << 1) - 1
}

__global__ void __launch_bounds__(CPM_THREADS)
char_to_float_kernel(const unsigned char *__restrict__ in, long long in_stride, float *__restrict__ out, long long out_stride, long long n)
{
    const unsigned char *__restrict__ x = in + (long long)blockIdx.y * in_stride;
    float *__restrict__ y = out + (long long)blockIdx.y * out_stride;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < n; o += stride) y[o] = (float)(signed char)x[o];
}

__global__ void __launch_bounds__(CPM_THREADS)
chunks_to_symbols_bf_kernel(const unsigned char *__restrict__ in, float *__restrict__ out, long long n_out, const float *__restrict__ table,
                            unsigned table_size, unsigned D)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += stride) {
        const long long c = D == 1 ? o : o / D;
        const unsigned d = (unsigned)(o - c * D);
        const unsigned long long first = (unsigned long long)in[c] * D;
        out[o] = first + D <= table_size ? table[first + d] : 0.f;
    }
}

}  // namespace

int fm_walk_launch(const float *in, float2 *out, long long n, int nstreams, double sensitivity, double *phase, hipStream_t st)
{
    if (n <= 0 || nstreams <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(fm_walk_kernel, dim3((unsigned)nstreams), dim3(64), 0, st, in, out, n, sensitivity, phase);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int fm_scan_launch(const float *in, float2 *out, long long n, int nstreams, double sensitivity, double *phase, double *scratch,
                   hipStream_t st)
{
    return scan_launch(FloatSrc{in}, out, n, nstreams, sensitivity, phase, scratch, st);
}

int cpm_fused_launch(const CpmFused &src, float2 *out, long long n, int nstreams, double sensitivity, double *phase, double *scratch,
                     hipStream_t st)
{
    if (src.sps < 1 || !cpm_fused_fits((unsigned)src.sps, (unsigned)src.nt)) return fail(GRHIP_EINVAL, "cpm: the taps do not fit the fused kernel");
    return scan_launch(FusedSrc{src}, out, n, nstreams, sensitivity, phase, scratch, st);
}

int cpm_history_launch(const CpmFused &src, long long nsym, int nstreams, hipStream_t st)
{
    if (nsym <= 0 || nstreams <= 0 || src.nt <= 1) return GRHIP_OK;
    hipLaunchKernelGGL(cpm_history_kernel, dim3((unsigned)((nstreams + 63) / 64)), dim3(64), 0, st, FusedSrc{src}, nsym, nstreams);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int bytes_to_syms_launch(const unsigned char *in, long long in_stride, float *out, long long out_stride, long long n_bytes, int nstreams,
                         hipStream_t st)
{
    if (n_bytes <= 0 || nstreams <= 0) return GRHIP_OK;
    if (nstreams > 65535) return fail(GRHIP_EINVAL, "bytes_to_syms: grid too large");
    hipLaunchKernelGGL(bytes_to_syms_kernel, dim3(blocks_for(n_bytes * 8), (unsigned)nstreams), dim3(CPM_THREADS), 0, st, in, in_stride, out,
                       out_stride, n_bytes * 8);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int char_to_float_launch(const unsigned char *in, long long in_stride, float *out, long long out_stride, long long n, int nstreams,
                         hipStream_t st)
{
    if (n <= 0 || nstreams <= 0) return GRHIP_OK;
    if (nstreams > 65535) return fail(GRHIP_EINVAL, "char_to_float: grid too large");
    hipLaunchKernelGGL(char_to_float_kernel, dim3(blocks_for(n), (unsigned)nstreams), dim3(CPM_THREADS), 0, st, in, in_stride, out, out_stride, n);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int chunks_to_symbols_bf_launch(const unsigned char *in, float *out, long long n, const float *table, unsigned table_size, unsigned D,
                                hipStream_t st)
{
    if (n <= 0) return GRHIP_OK;
    if (D < 1 || table_size < 1) return fail(GRHIP_EINVAL, "chunks_to_symbols_bf: bad table or D");
    hipLaunchKernelGGL(chunks_to_symbols_bf_kernel, dim3(blocks_for(n * (long long)D)), dim3(CPM_THREADS), 0, st, in, out, n * (long long)D, table,
                       table_size, D);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
