// trellis.hip -- the kernels of trellis_encoder_XX (gr-trellis/src/lib/trellis_encoder_XX.cc.t:50-75) and of
// trellis_metrics_X / trellis_constellation_metrics_cf (calc_metric.cc:29-72, :212-250; digital_constellation.cc:160-201).
//
// Encoder: out[i] = OS[st * I + in[i]], st = NS[st * I + in[i]].  The serial form is one wavefront per stream: its lanes
// move windows of the stream through LDS, coalesced, and one lane walks each window.  The
// parallel form (S <= ENC_MAX_S) cuts the items into chunks of ENC_CHUNK: one wavefront per chunk walks it from every
// start state at once (lane s starts in state s; the inputs are the same for every lane) and leaves the chunk's end-state
// map; one lane per stream chains the maps; one lane per chunk walks its chunk again from its true start state.
// An input outside [0, I) raises *flag, and then no state is written back.
//
// Metrics: statement for statement with the round-to-nearest intrinsics, so nothing contracts.
#include "trellis_metric.h"

namespace grhip {

namespace {

// ---- encoder -----------------------------------------------------------------------------------------------------------
template <class Ti>
__device__ inline bool enc_symbol(Ti x, int I, int &sym)
{
    sym = (int)x;
    return (unsigned)sym < (unsigned)I;
}

// one wavefront per stream: the 64 lanes load a window of ENC_WIN items coalesced into LDS, lane 0 walks the window out
// of LDS into an output window, the 64 lanes store it coalesced
template <class Ti, class To>
__global__ void __launch_bounds__(64)
enc_serial_kernel(const Ti *__restrict__ in, To *__restrict__ out, int n, int I, const int *__restrict__ NS,
                  const int *__restrict__ OS, int *__restrict__ state, unsigned *__restrict__ flag)
{
    __shared__ Ti win_in[ENC_WIN];
    __shared__ To win_out[ENC_WIN];
    __shared__ int bad;
    const int strm = blockIdx.x, lane = threadIdx.x;
    const Ti *x = in + (size_t)strm * n;
    To *y = out + (size_t)strm * n;
    int st = state[strm];
    if (lane == 0) bad = 0;
    for (int w0 = 0; w0 < n; w0 += ENC_WIN) {
        const int len = n - w0 < ENC_WIN ? n - w0 : ENC_WIN;
        for (int i = lane; i < len; i += 64) win_in[i] = x[w0 + i];
        __syncthreads();
        if (lane == 0)
            for (int i = 0; i < len; ++i) {
                int sym;
                if (!enc_symbol(win_in[i], I, sym)) { bad = 1; break; }
                win_out[i] = (To)OS[(size_t)st * I + sym];
                st = NS[(size_t)st * I + sym];
            }
        __syncthreads();
        if (bad) break;                              // uniform: every lane reads the same word
        for (int i = lane; i < len; i += 64) y[w0 + i] = win_out[i];
        __syncthreads();
    }
    if (lane == 0) {
        if (bad) atomicOr(flag, 1u);
        else state[strm] = st;
    }
}

// grid (chunks, streams), 64 lanes: lane s < S walks the chunk from state s
template <class Ti>
__global__ void __launch_bounds__(64)
enc_map_kernel(const Ti *__restrict__ in, int n, int I, int S, const int *__restrict__ NS, unsigned char *__restrict__ maps,
               unsigned *__restrict__ flag)
{
    const int chunk = blockIdx.x, strm = blockIdx.y, chunks = gridDim.x, lane = threadIdx.x;
    const Ti *x = in + (size_t)strm * n + (size_t)chunk * ENC_CHUNK;
    const int len = n - chunk * ENC_CHUNK < ENC_CHUNK ? n - chunk * ENC_CHUNK : ENC_CHUNK;
    __shared__ Ti win[ENC_CHUNK];                                   // the chunk, loaded coalesced once
    for (int i = lane; i < len; i += 64) win[i] = x[i];
    __syncthreads();
    int st = lane < S ? lane : 0;
    bool bad = false;
    for (int i = 0; i < len; ++i) {
        int sym;
        if (!enc_symbol(win[i], I, sym)) { bad = true; break; }    // uniform across the lanes
        st = NS[(size_t)st * I + sym];
    }
    if (bad && lane == 0) atomicOr(flag, 1u);
    if (lane < S) maps[((size_t)strm * chunks + chunk) * S + lane] = (unsigned char)st;
}

__global__ void enc_chain_kernel(int streams, int chunks, int S, const unsigned char *__restrict__ maps, int *__restrict__ starts,
                                 int *__restrict__ state, const unsigned *__restrict__ flag)
{
    const int strm = blockIdx.x * blockDim.x + threadIdx.x;
    if (strm >= streams) return;
    int st = state[strm];
    for (int c = 0; c < chunks; ++c) {
        starts[(size_t)strm * chunks + c] = st;
        st = maps[((size_t)strm * chunks + c) * S + st];
    }
    if (*flag == 0) state[strm] = st;
}

template <class Ti, class To>
__global__ void enc_walk_kernel(const Ti *__restrict__ in, To *__restrict__ out, int n, int streams, int chunks, int I,
                                const int *__restrict__ NS, const int *__restrict__ OS, const int *__restrict__ starts)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)streams * chunks) return;
    const int strm = (int)(g / chunks), chunk = (int)(g - (long long)strm * chunks);
    const Ti *x = in + (size_t)strm * n + (size_t)chunk * ENC_CHUNK;
    To *y = out + (size_t)strm * n + (size_t)chunk * ENC_CHUNK;
    const int len = n - chunk * ENC_CHUNK < ENC_CHUNK ? n - chunk * ENC_CHUNK : ENC_CHUNK;
    int st = starts[g];
    for (int i = 0; i < len; ++i) {
        int sym;
        if (!enc_symbol(x[i], I, sym)) return;                      // the map kernel has raised the flag
        y[i] = (To)OS[(size_t)st * I + sym];
        st = NS[(size_t)st * I + sym];
    }
}

template <class Ti, class To>
int enc_serial(const void *in, void *out, int n, int streams, int I, const int *NS, const int *OS, int *state, unsigned *flag,
               hipStream_t st)
{
    hipLaunchKernelGGL((enc_serial_kernel<Ti, To>), dim3(streams), dim3(64), 0, st, (const Ti *)in, (To *)out, n, I, NS, OS, state,
                       flag);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <class Ti, class To>
int enc_chunked(const void *in, void *out, int n, int streams, int I, int S, const int *NS, const int *OS, int *state,
                unsigned *flag, unsigned char *maps, int *starts, hipStream_t st)
{
    const int chunks = (n + ENC_CHUNK - 1) / ENC_CHUNK;
    hipLaunchKernelGGL((enc_map_kernel<Ti>), dim3(chunks, streams), dim3(64), 0, st, (const Ti *)in, n, I, S, NS, maps, flag);
    GRHIP_HIP(hipGetLastError());
    hipLaunchKernelGGL(enc_chain_kernel, dim3((streams + 63) / 64), dim3(64), 0, st, streams, chunks, S, maps, starts, state, flag);
    GRHIP_HIP(hipGetLastError());
    const long long lanes = (long long)streams * chunks;
    hipLaunchKernelGGL((enc_walk_kernel<Ti, To>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, (const Ti *)in, (To *)out, n,
                       streams, chunks, I, NS, OS, starts);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

// ---- metrics -----------------------------------------------------------------------------------------------------------
// one lane per output float
template <class T>
__global__ void metrics_euclid_kernel(const T *__restrict__ in, float *__restrict__ out, long long total, int O, int D,
                                      const T *__restrict__ table)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const long long step = g / O;
    const int o = (int)(g - step * O);
    out[g] = metric_of(in + step * D, table, o, D);
}

// one lane per step: the first minimum in o order, from FLT_MAX (:48-65)
template <class T>
__global__ void metrics_hard_kernel(const T *__restrict__ in, float *__restrict__ out, long long steps, int O, int D,
                                    const T *__restrict__ table)
{
    const long long step = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (step >= steps) return;
    float minm = FLT_MAX;
    int minmi = 0;
    for (int o = 0; o < O; ++o) {
        const float m = metric_of(in + step * D, table, o, D);
        if (m < minm) { minm = m; minmi = o; }
    }
    for (int o = 0; o < O; ++o) out[step * O + o] = o == minmi ? 0.0f : 1.0f;
}

template <class T>
int metrics_typed(int type, const void *in, float *out, long long steps, int O, int D, const void *table, hipStream_t st)
{
    if (type == TRELLIS_EUCLIDEAN) {
        const long long total = steps * O;
        hipLaunchKernelGGL((metrics_euclid_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T *)in, out,
                           total, O, D, (const T *)table);
    } else {
        hipLaunchKernelGGL((metrics_hard_kernel<T>), dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, st, (const T *)in, out,
                           steps, O, D, (const T *)table);
    }
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

#define GRHIP_ENC_DISPATCH(CALL)                                                                                      \
    if (tin == TR_B && tout == TR_B) return CALL(unsigned char, unsigned char);                                       \
    if (tin == TR_B && tout == TR_S) return CALL(unsigned char, short);                                               \
    if (tin == TR_B && tout == TR_I) return CALL(unsigned char, int);                                                 \
    if (tin == TR_S && tout == TR_S) return CALL(short, short);                                                       \
    if (tin == TR_S && tout == TR_I) return CALL(short, int);                                                         \
    if (tin == TR_I && tout == TR_I) return CALL(int, int);                                                           \
    return fail(GRHIP_EINVAL, "trellis_encoder: no such signature")

int encoder_serial_launch(int tin, int tout, const void *in, void *out, int n, int streams, int I, const int *NS, const int *OS,
                          int *state, unsigned *flag, hipStream_t st)
{
#define GRHIP_ENC_SERIAL(TI, TO) enc_serial<TI, TO>(in, out, n, streams, I, NS, OS, state, flag, st)
    GRHIP_ENC_DISPATCH(GRHIP_ENC_SERIAL);
#undef GRHIP_ENC_SERIAL
}

int encoder_chunked_launch(int tin, int tout, const void *in, void *out, int n, int streams, int I, int S, const int *NS,
                           const int *OS, int *state, unsigned *flag, unsigned char *maps, int *starts, hipStream_t st)
{
#define GRHIP_ENC_CHUNKED(TI, TO) enc_chunked<TI, TO>(in, out, n, streams, I, S, NS, OS, state, flag, maps, starts, st)
    GRHIP_ENC_DISPATCH(GRHIP_ENC_CHUNKED);
#undef GRHIP_ENC_CHUNKED
}

#undef GRHIP_ENC_DISPATCH

int metrics_launch(int t, int type, const void *in, float *out, long long steps, int O, int D, const void *table, hipStream_t st)
{
    if (steps < 1) return GRHIP_OK;
    switch (t) {
    case TR_S: return metrics_typed<short>(type, in, out, steps, O, D, table, st);
    case TR_I: return metrics_typed<int>(type, in, out, steps, O, D, table, st);
    case TR_F: return metrics_typed<float>(type, in, out, steps, O, D, table, st);
    case TR_C: return metrics_typed<tr_cplx>(type, in, out, steps, O, D, table, st);
    }
    return fail(GRHIP_EINVAL, "trellis_metrics: bad item type");
}

}  // namespace grhip
