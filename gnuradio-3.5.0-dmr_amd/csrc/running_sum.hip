// running_sum.hip -- kernels of gr_dc_blocker_ff / _cc (filter/gr_dc_blocker_ff.cc:41-53,105-138, _cc.cc likewise),
// gr_moving_average_XX (gengen/gr_moving_average_XX.cc.t:64-93) and gr_integrate_XX (gengen/gr_integrate_XX.cc.t:52-67).
//
// dc_generic_kernel<T, S>: GENERIC, bit-exact.  One wavefront per stream (the form of pager_slicer_fb); the
//   whole state of the S moving_averager stages lives in LDS for the call: per stage its last inputs, in front of a
//   window of RSUM_GEN_WIN samples.  Per window and stage all lanes form x[n] - x[n - D] in parallel (four per lane),
//   then the dependent adds y = (x[n] - x[n - D]) + y are walked in stream order: the addend of step l is read out of
//   lane l's register (v_readlane), so the chain is one add per sample and touches no memory; lane l keeps y, divides
//   it by (float)D -- a division, as the reference -- and stores it as the next stage's input.  The stages run one
//   after the other within a window.
//
// win_fast_kernel<T, IO, DC>: FAST, every output a true window sum.  One workgroup stages E = 256 R samples (tile plus
//   halo; R odd, so the lanes' runs of R consecutive samples start on different banks) and for each stage
//     1. forms the prefix sums P WITHIN blocks of D samples (blocks aligned to the staged array): every lane scans its
//        run, a segmented scan over the lanes (shuffles) and over the four waves (LDS) supplies its carry;
//     2. forms each D-window sum from at most three P: the rest of the window's first block, P[block end] - P[i - 1],
//        plus P[i + D - 1], the part in the next block.
//   No partial sum is longer than one block, so the rounding error is a few ulp of D max|x| whatever the tile or the
//   stream, and the work per sample does not depend on D.  dc_blocker runs 2 or 4 such stages over
//   tile + stages (D - 1) samples (multiplying by 1 / D in between) and subtracts the last from the staged input
//   delayed by the group delay; samples in front of the call come from the handle's history of the last inputs.
//   moving_average is one stage, scaled on the way out; the integer types run it with wrapping sums, which are exact
//   in any order, so their FAST and GENERIC results are equal.
//
// ma_generic_kernel: one lane per reference work call (max_iter outputs): sum = 0, the first length - 1 items in
//   order, then sum += in[i + length - 1]; out = sum * scale; sum -= in[i].
// integrate_generic_kernel: one lane per output, j ascending from 0.  integrate_fast_kernel: 1 .. 64 lanes per output
//   (a power of two), strided partial sums and a butterfly.
#include <cstdint>

#include "grhip_internal.h"
#include "running_sum.h"

namespace grhip {

namespace {

__device__ __forceinline__ float radd(float a, float b) { return a + b; }
__device__ __forceinline__ float2 radd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ int radd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ short radd(short a, short b) { return (short)(unsigned short)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ float rsub(float a, float b) { return a - b; }
__device__ __forceinline__ float2 rsub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ int rsub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ short rsub(short a, short b) { return (short)(unsigned short)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ float rshfl_up(float v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ int rshfl_up(int v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ float2 rshfl_up(float2 v, int d) { return make_float2(__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64)); }
__device__ __forceinline__ float rshfl_xor(float v, int d) { return __shfl_xor(v, d, 64); }
__device__ __forceinline__ int rshfl_xor(int v, int d) { return __shfl_xor(v, d, 64); }
__device__ __forceinline__ float2 rshfl_xor(float2 v, int d) { return make_float2(__shfl_xor(v.x, d, 64), __shfl_xor(v.y, d, 64)); }
__device__ __forceinline__ float rlane(float v, int l)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ float2 rlane(float2 v, int l) { return make_float2(rlane(v.x, l), rlane(v.y, l)); }
__device__ __forceinline__ float rdiv(float a, float d) { return a / d; }
__device__ __forceinline__ float2 rdiv(float2 a, float d) { return make_float2(a.x / d, a.y / d); }
__device__ __forceinline__ float rmul(float a, float m) { return a * m; }
__device__ __forceinline__ float2 rmul(float2 a, float m) { return make_float2(a.x * m, a.y * m); }
template <class T> __device__ __forceinline__ T rzero() { return T(0); }
template <> __device__ __forceinline__ float2 rzero<float2>() { return make_float2(0.f, 0.f); }

// sum * scale of gr_moving_average_XX, in the output type
struct MaScale {
    float2 c;
    int i;
};
__device__ __forceinline__ float ma_scale(float s, const MaScale &k) { return s * k.c.x; }
__device__ __forceinline__ float2 ma_scale(float2 s, const MaScale &k)
{
    return make_float2(s.x * k.c.x - s.y * k.c.y, s.x * k.c.y + s.y * k.c.x);      // std::complex's product, unfused
}
__device__ __forceinline__ int ma_scale(int s, const MaScale &k) { return (int)((unsigned)s * (unsigned)k.i); }
__device__ __forceinline__ short ma_scale(short s, const MaScale &k) { return (short)(unsigned short)((unsigned)(int)s * (unsigned)k.i); }

// ---- dc_blocker, GENERIC ---------------------------------------------------------------------------------------
template <class T, int S>
__global__ void __launch_bounds__(64) dc_generic_kernel(DcLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    T *lds = reinterpret_cast<T *>(rs_lds);
    constexpr int W = RSUM_GEN_WIN, K4 = W / 64;
    const int lane = threadIdx.x, D = a.D;
    const long long s = blockIdx.y;
    const T *in = (const T *)a.in + s * a.n;
    T *out = (T *)a.out + s * a.n;
    T *state = (T *)a.state + s * (long long)dc_state_elems(D, S);
    const float Df = (float)D;
    const int gd = (S == 4 ? 2 : 1) * (D - 1);              // get_group_delay(): delayed_sig(), long form D - 1 more
    // stage k: H(k) last inputs, then the window
    auto H = [&](int k) { return k == 0 ? 2 * D : D; };
    auto off = [&](int k) { return k == 0 ? 0 : (2 * D + W) + (k - 1) * (D + W); };
    auto soff = [&](int k) { return k == 0 ? 0 : (k + 1) * D; };

    T y[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        for (int i = lane; i < H(k); i += 64) lds[off(k) + i] = state[soff(k) + i];
        y[k] = state[(S + 1) * D + k];
    }
    __syncthreads();

    for (long long n0 = 0; n0 < a.n; n0 += W) {
        const int w = (int)(a.n - n0 < W ? a.n - n0 : W);
        T *x0 = lds + 2 * D;
#pragma unroll
        for (int q = 0; q < K4; ++q) {
            const int j = q * 64 + lane;
            x0[j] = j < w ? in[n0 + j] : rzero<T>();
        }
        __syncthreads();
        T u[K4];
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const T *b = lds + off(k) + H(k);
            T d[K4];
#pragma unroll
            for (int q = 0; q < K4; ++q) {
                const int j = q * 64 + lane;
                d[q] = rsub(b[j], b[j - D]);                 // x - d_out_d1
                u[q] = rzero<T>();
            }
            T yy = y[k];
#pragma unroll
            for (int q = 0; q < K4; ++q) {
                const int cnt = w - q * 64;                  // wave-uniform
                if (cnt >= 64) {
#pragma unroll
                    for (int l = 0; l < 64; ++l) {
                        yy = radd(rlane(d[q], l), yy);       // ... + d_out_d2
                        if (lane == l) u[q] = yy;
                    }
                } else {
                    for (int l = 0; l < cnt; ++l) {
                        yy = radd(rlane(d[q], l), yy);
                        if (lane == l) u[q] = yy;
                    }
                }
            }
            y[k] = yy;
#pragma unroll
            for (int q = 0; q < K4; ++q) u[q] = rdiv(u[q], Df);          // y / (float)d_length
            if (k + 1 < S) {
                T *nx = lds + off(k + 1) + H(k + 1);
#pragma unroll
                for (int q = 0; q < K4; ++q) nx[q * 64 + lane] = u[q];
                __syncthreads();
            }
        }
#pragma unroll
        for (int q = 0; q < K4; ++q) {
            const int j = q * 64 + lane;
            if (j < w) out[n0 + j] = rsub(x0[j - gd], u[q]);
        }
        __syncthreads();
        // Slide every stage's inputs down by w, 64 at a time and ascending.  Across chunks: a chunk's reads lie above
        // everything written so far.  Within a chunk source and destination overlap when w < 64; that is safe ONLY
        // because this workgroup is a single wavefront, which executes the load for all 64 lanes before the store
        // (__launch_bounds__(64), wave64: the launcher never starts this kernel with more lanes).
#pragma unroll
        for (int k = 0; k < S; ++k) {
            T *b = lds + off(k);
            for (int i = lane; i < H(k); i += 64) {
                const T v = b[w + i];
                b[i] = v;
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < S; ++k) {
        for (int i = lane; i < H(k); i += 64) state[soff(k) + i] = lds[off(k) + i];
        if (lane == 0) state[(S + 1) * D + k] = y[k];
    }
}

// ---- FAST: block prefix sums and window sums in LDS ----------------------------------------------------------------
struct WinArgs {
    const void *in, *hist;
    void *out;
    long long n, n_in;          // outputs and readable inputs per stream
    int D, stages, halo, back, gd, R;
    float invD;
    MaScale scale;
};

template <class T, class IO> __device__ __forceinline__ T rs_load(const IO *p, long long i) { return p[i]; }
template <> __device__ __forceinline__ int rs_load<int, short>(const short *p, long long i) { return (int)p[i]; }

template <class T>
__device__ __forceinline__ void block_prefix(const T *src, T *P, int R, int D, T *wt, int *wf)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = tid * R, r0 = a % D;
    T run = rzero<T>();
    int flag = 0, r = r0;
    for (int j = 0; j < R; ++j) {
        if (r == 0) { run = rzero<T>(); flag = 1; }
        run = radd(run, src[a + j]);
        if (++r == D) r = 0;
    }
    T agg = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T v2 = rshfl_up(agg, d);
        const int f2 = __shfl_up(flag, d, 64);
        if (lane >= d) {
            if (!flag) agg = radd(v2, agg);
            flag |= f2;
        }
    }
    T ex = rshfl_up(agg, 1);
    int exf = __shfl_up(flag, 1, 64);
    if (lane == 0) { ex = rzero<T>(); exf = 0; }
    if (lane == 63) { wt[wave] = agg; wf[wave] = flag; }
    __syncthreads();
    T c = rzero<T>();
    for (int w = 0; w < wave; ++w) c = wf[w] ? wt[w] : radd(c, wt[w]);
    run = exf ? ex : radd(c, ex);
    r = r0;
    for (int j = 0; j < R; ++j) {
        if (r == 0) run = rzero<T>();
        run = radd(run, src[a + j]);
        P[a + j] = run;
        if (++r == D) r = 0;
    }
}

template <class T, class IO, bool DC>
__global__ void __launch_bounds__(RSUM_THREADS) win_fast_kernel(WinArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    __shared__ T wt[4];
    __shared__ int wf[4];
    const int tid = threadIdx.x, D = a.D, E = RSUM_THREADS * a.R, tile = E - a.halo;
    T *X = reinterpret_cast<T *>(rs_lds), *P = X + E, *V = P + E;      // V: dc_blocker only
    const long long s = blockIdx.y, t0 = (long long)blockIdx.x * tile;
    const IO *in = (const IO *)a.in + s * a.n_in;
    IO *out = (IO *)a.out + s * a.n;
    const IO *hist = a.hist ? (const IO *)a.hist + s * a.halo + a.halo : nullptr;

    for (int m = tid; m < E; m += RSUM_THREADS) {
        const long long g = t0 - a.back + m;
        T v = rzero<T>();
        if (g >= 0) { if (g < a.n_in) v = rs_load<T, IO>(in, g); }
        else if (hist) v = rs_load<T, IO>(hist, g);
        X[m] = v;
    }
    __syncthreads();

    const int live = (int)(a.n - t0 < tile ? a.n - t0 : tile);
    const T *src = X;
    for (int st = 0; st < a.stages; ++st) {
        block_prefix(src, P, a.R, D, wt, wf);
        __syncthreads();
        const bool last = st + 1 == a.stages;
        const int cnt = last ? live : E - (st + 1) * (D - 1);       // the windows that lie inside the staged samples
        const int step = RSUM_THREADS % D;
        int r = tid % D;
        for (int m = tid; m < (last ? cnt : E); m += RSUM_THREADS) {
            T v = rzero<T>();
            if (m < cnt) {
                v = P[m + D - 1];
                if (r != 0) v = radd(rsub(P[m - r + D - 1], P[m - 1]), v);
            }
            if constexpr (DC) {
                v = rmul(v, a.invD);
                if (last) out[t0 + m] = rsub(X[m + a.halo - a.gd], v);
                else V[m] = v;
            } else {
                out[t0 + m] = (IO)ma_scale((IO)v, a.scale);
            }
            r += step;
            if (r >= D) r -= D;
        }
        __syncthreads();
        src = V;
    }
}

template <class T>
__global__ void __launch_bounds__(256) dc_hist_kernel(const T *in, const T *old, T *nw, long long n, int halo)
{
    const long long s = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= halo) return;
    const long long g = n - halo + i;
    nw[s * halo + i] = g < 0 ? old[s * halo + halo + g] : in[s * n + g];
}

// ---- moving_average, GENERIC -----------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(64) ma_generic_kernel(const T *in, T *out, long long n, int length, int max_iter, MaScale k)
{
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x, o0 = c * max_iter;
    if (o0 >= n) return;
    const int cnt = (int)(n - o0 < max_iter ? n - o0 : max_iter);
    const T *p = in + o0;
    T *q = out + o0;
    T sum = rzero<T>();
    for (int i = 0; i < length - 1; ++i) sum = radd(sum, p[i]);
    for (int i = 0; i < cnt; ++i) {
        sum = radd(sum, p[i + length - 1]);
        q[i] = ma_scale(sum, k);
        sum = rsub(sum, p[i]);
    }
}

// ---- integrate ---------------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) integrate_generic_kernel(const T *in, T *out, long long n, int decim)
{
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= n) return;
    const T *p = in + o * decim;
    T acc = rzero<T>();
    for (int j = 0; j < decim; ++j) acc = radd(acc, p[j]);
    out[o] = acc;
}

template <class T, class IO>
__global__ void __launch_bounds__(256) integrate_fast_kernel(const IO *in, IO *out, long long n, int decim, int lg)
{
    const long long gl = (long long)blockIdx.x * 256 + threadIdx.x;
    const int L = 1 << lg;
    const long long o = gl >> lg;
    const int l = (int)(gl & (L - 1));
    T acc = rzero<T>();
    if (o < n) {
        const IO *p = in + o * decim;
        for (int j = l; j < decim; j += L) acc = radd(acc, rs_load<T, IO>(p, j));
    }
    for (int d = L >> 1; d >= 1; d >>= 1) acc = radd(acc, rshfl_xor(acc, d));
    if (o < n && l == 0) out[o] = (IO)acc;
}

int pick_R(int halo, int rmax)
{
    int want = (4 * halo + RSUM_THREADS - 1) / RSUM_THREADS;
    if (want < 9) want = 9;
    want |= 1;
    return want < rmax ? want : rmax;
}

template <class T, class IO, bool DC>
int launch_win(WinArgs a, int nstreams, hipStream_t st)
{
    const int bufs = DC ? 3 : 2;
    int rmax = RSUM_LDS_BYTES / (bufs * (int)sizeof(T) * RSUM_THREADS);
    if (!(rmax & 1)) rmax -= 1;
    a.R = pick_R(a.halo, rmax);
    const int E = RSUM_THREADS * a.R, tile = E - a.halo;
    if (tile < RSUM_MIN_TILE) return fail(GRHIP_EINVAL, "running sum: a halo of %d samples does not fit the LDS layout", a.halo);
    const size_t lds = (size_t)bufs * E * sizeof(T);
    if (int rc = allow_lds((const void *)win_fast_kernel<T, IO, DC>, lds)) return rc;
    const long long tiles = (a.n + tile - 1) / tile;
    if (tiles > 0x7fffffffLL || nstreams > 65535) return fail(GRHIP_EINVAL, "running sum: too many outputs or streams for one call");
    hipLaunchKernelGGL((win_fast_kernel<T, IO, DC>), dim3((unsigned)tiles, (unsigned)nstreams), dim3(RSUM_THREADS), lds, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <class T, int S>
int launch_dc_generic(const DcLaunch &a, hipStream_t st)
{
    const size_t lds = ((size_t)(2 * a.D + RSUM_GEN_WIN) + (size_t)(S - 1) * (a.D + RSUM_GEN_WIN)) * sizeof(T);
    if (int rc = allow_lds((const void *)dc_generic_kernel<T, S>, lds)) return rc;
    hipLaunchKernelGGL((dc_generic_kernel<T, S>), dim3(1, (unsigned)a.nstreams), dim3(64), lds, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <class T>
int launch_dc(bool fast, const DcLaunch &a, hipStream_t st)
{
    if (!fast) return a.stages == 4 ? launch_dc_generic<T, 4>(a, st) : launch_dc_generic<T, 2>(a, st);
    WinArgs w = {};
    w.in = a.in; w.hist = a.hist_old; w.out = a.out;
    w.n = a.n; w.n_in = a.n;
    w.D = a.D; w.stages = a.stages;
    w.halo = a.stages * (a.D - 1); w.back = w.halo;
    w.gd = (a.stages == 4 ? 2 : 1) * (a.D - 1);
    w.invD = 1.0f / (float)a.D;
    if (int rc = launch_win<T, T, true>(w, a.nstreams, st)) return rc;
    if (w.halo > 0) {
        hipLaunchKernelGGL(dc_hist_kernel<T>, dim3((unsigned)((w.halo + 255) / 256), (unsigned)a.nstreams), dim3(256), 0, st,
                           (const T *)a.in, (const T *)a.hist_old, (T *)a.hist_new, a.n, w.halo);
        GRHIP_HIP(hipGetLastError());
    }
    return GRHIP_OK;
}

template <class T, class IO>
int launch_ma_fast(const MaLaunch &a, hipStream_t st)
{
    WinArgs w = {};
    w.in = a.in; w.out = a.out;
    w.n = a.n; w.n_in = a.n + a.length - 1;
    w.D = a.length; w.stages = 1;
    w.halo = a.length - 1;
    w.scale.c = a.scale; w.scale.i = a.iscale;
    return launch_win<T, IO, false>(w, 1, st);
}

template <class T>
int launch_ma_generic(const MaLaunch &a, hipStream_t st)
{
    const long long calls = (a.n + a.max_iter - 1) / a.max_iter, wgs = (calls + 63) / 64;
    if (wgs > 0x7fffffffLL) return fail(GRHIP_EINVAL, "moving_average: too many work calls for one launch");
    MaScale k;
    k.c = a.scale; k.i = a.iscale;
    hipLaunchKernelGGL(ma_generic_kernel<T>, dim3((unsigned)wgs), dim3(64), 0, st, (const T *)a.in, (T *)a.out, a.n, a.length,
                       a.max_iter, k);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <class T, class IO>
int launch_integrate(bool fast, const void *in, void *out, long long n, int decim, hipStream_t st)
{
    if (!fast) {
        const long long wgs = (n + 255) / 256;
        if (wgs > 0x7fffffffLL) return fail(GRHIP_EINVAL, "integrate: too many outputs for one call");
        hipLaunchKernelGGL(integrate_generic_kernel<IO>, dim3((unsigned)wgs), dim3(256), 0, st, (const IO *)in, (IO *)out, n, decim);
    } else {
        int lg = 0;
        while (lg < 6 && (1 << lg) < decim) ++lg;
        const long long wgs = ((n << lg) + 255) / 256;
        if (n > (1LL << 56) || wgs > 0x7fffffffLL) return fail(GRHIP_EINVAL, "integrate: too many outputs for one call");
        hipLaunchKernelGGL((integrate_fast_kernel<T, IO>), dim3((unsigned)wgs), dim3(256), 0, st, (const IO *)in, (IO *)out, n, decim, lg);
    }
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

int dc_blocker_launch(int type, bool fast, const DcLaunch &a, hipStream_t st)
{
    if (a.n <= 0 || a.nstreams <= 0) return GRHIP_OK;
    if (a.D < 1 || a.D > RSUM_DC_MAX_D || (a.stages != 2 && a.stages != 4) || a.nstreams > 65535)
        return fail(GRHIP_EINVAL, "dc_blocker: bad launch");
    if (type == RSUM_F) return launch_dc<float>(fast, a, st);
    if (type == RSUM_C) return launch_dc<float2>(fast, a, st);
    return fail(GRHIP_EINVAL, "dc_blocker: float and complex items only");
}

int moving_average_launch(int type, bool fast, const MaLaunch &a, hipStream_t st)
{
    if (a.n <= 0) return GRHIP_OK;
    if (a.length < 1 || a.length > RSUM_MA_MAX_LEN || a.max_iter < 1) return fail(GRHIP_EINVAL, "moving_average: bad launch");
    switch (type) {
    case RSUM_F: return fast ? launch_ma_fast<float, float>(a, st) : launch_ma_generic<float>(a, st);
    case RSUM_C: return fast ? launch_ma_fast<float2, float2>(a, st) : launch_ma_generic<float2>(a, st);
    case RSUM_S: return fast ? launch_ma_fast<int, short>(a, st) : launch_ma_generic<short>(a, st);
    case RSUM_I: return fast ? launch_ma_fast<int, int>(a, st) : launch_ma_generic<int>(a, st);
    default: return fail(GRHIP_EINVAL, "moving_average: bad item type");
    }
}

int integrate_launch(int type, bool fast, const void *in, void *out, long long n, int decim, hipStream_t st)
{
    if (n <= 0) return GRHIP_OK;
    if (decim < 1) return fail(GRHIP_EINVAL, "integrate: bad launch");
    switch (type) {
    case RSUM_F: return launch_integrate<float, float>(fast, in, out, n, decim, st);
    case RSUM_C: return launch_integrate<float2, float2>(fast, in, out, n, decim, st);
    case RSUM_S: return launch_integrate<int, short>(fast, in, out, n, decim, st);
    case RSUM_I: return launch_integrate<int, int>(fast, in, out, n, decim, st);
    default: return fail(GRHIP_EINVAL, "integrate: bad item type");
    }
}

}  // namespace grhip
