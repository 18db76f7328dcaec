// constellation.hip -- the blocks of gr-digital/python/generic_mod_demod.py:296-313 behind timing recovery:
// digital_constellation_receiver_cb (gr-digital/lib/digital_constellation_receiver_cb.cc:80-122),
// digital_constellation_decoder_cb (digital_constellation_decoder_cb.cc:63-78), gr_diff_decoder_bb
// (general/gr_diff_decoder_bb.cc:48-61), gr_map_bb (general/gr_map_bb.cc:49-61), and the tail from symbols to bits
// fused into the receiver's store path.  The decisions are csrc/constellation.h's, the same text as on the host.
//
// receiver_walk_kernel<FORM, KIND, OUT> is a sibling of costas_walk_kernel (carrier.hip): one wavefront per stream, a
// window of CARRIER_WIN samples in LDS with the next window's loads in flight, every lane walks the recurrence out of
// LDS (a broadcast), lane l keeps sample l's outputs of each group of 64 and stores them itself.  The constellation's
// points, its sector table and the angles of its points are in LDS as well.
//   RX_FORM_GENERIC    the reference's statements in order, every operation rounded once: nco = expj(phase) with
//                      (float)cos((double)phase) and (float)sin((double)phase), sample = nco * in, the decision,
//                      error = 0 + -(float)atan2((double)im, (double)re) of sample * conj(point), the loop step.
//   RX_FORM_CARTESIAN  the same chain with the float polynomial NCO (sincos_fast), plain complex products, rect's
//                      sector from one fused multiply-add per axis and the device library's atan2f: nothing on the
//                      double pipe but phase_wrap.  For rect and calcdist.
//   RX_FORM_ANGLE      for bpsk, qpsk, dqpsk, 8psk and psk, whose decision and error depend on the derotated sample's
//                      angle alone: the lanes turn their samples into theta = atan2f(im, re) on the way into LDS (as
//                      pll_walk_kernel does), and the chain is t = wrap(theta + phase), sign or sector tests on t,
//                      error = -wrap(t - angle of the decided point), the loop step: no sine, cosine or arctangent
//                      on the serial chain.
// OUT: 0 symbols; 1 symbols, error, phase and frequency (the last two AFTER the update, :113-115); 2 the bits of
// constellation_demod_cb: each lane holds its symbol and the one before it (its neighbour's, lane 0 the previous
// group's last, the first of a call the stream's stored one), takes the difference modulo the arity, looks it up in
// the map in LDS and stores its k bytes, as one store where k is 1, 2 or 4 and the output is aligned to k.
//
// Termination and bounds (every bit pattern of the samples; the host refuses the parameters this rests on,
// control_loop.h and constellation.h): the only loops whose trip count depends on data are phase_wrap's.  The error
// is NaN or bounded: atan2 and atan2f give NaN or a value within [-pi, pi] (float(pi) at most), and wrap() of a
// value within 3 pi + 1e-6 in magnitude is within pi + 1e-6; theta + phase and t - angle are within 3 pi since
// theta, t and the angles are within [-pi, pi] (+ 1e-6) and the stored phase is within [-2 pi, 2 pi] or NaN.  So
// after advance_loop the phase is NaN, which fails both comparisons, or below 2 pi + 1024 + 4 * 7 + 7 in magnitude:
// at most 170 trips, the bound of carrier.hip.  Indices: a symbol index comes from a closed form (at most 7, and
// the kind fixes the arity at 2, 4 or 8), from closest_point (below the arity) or out of the sector table, whose
// entries the host computed with closest_point; a sector index goes through clamp_sector or sector_clamp_f, which
// give 0 for a NaN and at most n - 1; n_real * n_imag and n_sectors are the table's length, n_ang the angle table's
// (the arity, or n_sectors for psk; pick8 masks its index to 0 .. 7 and reads registers).  The tail's map index is a
// difference modulo the arity (at most 255) or a symbol.
#include <cmath>
#include <cstdint>

#include "constellation_blocks.h"
#include "loop_math.h"

namespace grhip {

namespace {

constexpr float HALFPI_UP = 1.57079637f, QPI_F = 0.785398163f, TQPI_F = 2.35619449f;
constexpr float TWOPI_LO = (float)(CL_TWOPI - (double)TWOPI_UP);        // 2 pi = TWOPI_UP + TWOPI_LO to 2^-48
static_assert((double)HALFPI_UP > CL_PI / 2, "atan2f(x, 0) = float(pi/2) is not below it");

// a value within 3 pi (+ 1e-6) in magnitude -> within pi (+ 1e-6), 2 pi taken off in two floats; a NaN stays
__device__ __forceinline__ float wrap(float t)
{
    if (t >= PI_UP) return __fsub_rn(__fsub_rn(t, TWOPI_UP), TWOPI_LO);
    if (t <= -PI_UP) return __fadd_rn(__fadd_rn(t, TWOPI_UP), TWOPI_LO);
    return t;
}

// a float position -> 0 .. n-1; NaN -> 0
__device__ __forceinline__ unsigned sector_clamp_f(float v, unsigned n)
{
    if (!(v > 0.f)) return 0;
    if (v >= (float)n) return n - 1;
    return (unsigned)v;
}

__host__ __device__ inline unsigned round4(unsigned v) { return (v + 3u) & ~3u; }
// the LDS of receiver_walk_kernel: the window, the points, the angles, the sector table, the map
__host__ __device__ inline unsigned lds_pts(const ConstDev &) { return CARRIER_WIN * 8; }
__host__ __device__ inline unsigned lds_ang(const ConstDev &c) { return lds_pts(c) + c.arity * 8; }
__host__ __device__ inline unsigned lds_val(const ConstDev &c) { return lds_ang(c) + c.n_ang * 4; }
__host__ __device__ inline unsigned lds_map(const ConstDev &c) { return lds_val(c) + round4(c.n_sectors); }
__host__ __device__ inline unsigned lds_total(const ConstDev &c) { return lds_map(c) + 256; }

struct RxTail {
    const unsigned char *map;
    unsigned k, differential;
};

// the decision on a derotated sample: a symbol
template <int FORM>
__device__ __forceinline__ unsigned decide_cartesian(int kind, float re, float im, const ConstDev &c, const cfloat *s_pts,
                                                     const unsigned char *s_val, float inv_wr, float inv_wi)
{
    switch (kind) {
    case CONST_BPSK: return decide_bpsk(re, im);
    case CONST_QPSK: return decide_qpsk(re, im);
    case CONST_DQPSK: return decide_dqpsk(re, im);
    case CONST_8PSK: return decide_8psk(re, im);
    case CONST_PSK: return s_val[psk_sector_of(re, im, c.n_sectors)];
    case CONST_RECT:
        if (FORM == RX_FORM_GENERIC) return s_val[rect_axis(re, c.w_real, c.n_real) * c.n_imag + rect_axis(im, c.w_imag, c.n_imag)];
        return s_val[sector_clamp_f(__builtin_fmaf(re, inv_wr, 0.5f * (float)c.n_real), c.n_real) * c.n_imag +
                     sector_clamp_f(__builtin_fmaf(im, inv_wi, 0.5f * (float)c.n_imag), c.n_imag)];
    default: {
        const cfloat s = {re, im};
        return closest_point(s_pts, c.arity, 1, &s);
    }
    }
}

// the decision on the derotated sample's angle t (NaN or within [-pi, pi] + 1e-6): an index into the angle table, which
// is the symbol itself except for psk, where it is the sector, and dqpsk, where it is the quadrant.  re > 0 is |t| < pi/2, im > 0 is 0 < t < pi.
__device__ __forceinline__ unsigned decide_angle(int kind, float t, unsigned n_sectors, float inv_width)
{
    const float at = __builtin_fabsf(t);
    const unsigned a = at < HALFPI_UP, b = t > 0.f && t < PI_UP;
    switch (kind) {
    case CONST_BPSK: return a;
    case CONST_QPSK: return 2 * b + a;
    case CONST_DQPSK: return 2 * b + a;         // the quadrant as qpsk numbers it; dqpsk_of_quadrant() names the symbol
    case CONST_8PSK: return ((at >= QPI_F && at <= TQPI_F) ? 4u : 0u) | (at >= HALFPI_UP ? 1u : 0u) | ((t <= 0.f || t >= PI_UP) ? 2u : 0u);
    default: {
        float pos = __builtin_floorf(__builtin_fmaf(t, inv_width, 0.5f));
        if (pos < 0.f) pos = __fadd_rn(pos, (float)n_sectors);
        return sector_clamp_f(pos, n_sectors);
    }
    }
}

// digital_constellation.cc:493-512 from the quadrant 2 * (im > 0) + (re > 0): 0 -> 2, 1 -> 3, 2 -> 1, 3 -> 0, by shifts
__device__ __forceinline__ unsigned dqpsk_of_quadrant(unsigned q) { return (0x0132u >> (4u * (q & 3u))) & 0xfu; }

// a[idx & 7] by three levels of selects: no indexed register access, no memory
__device__ __forceinline__ float pick8(const float (&a)[8], unsigned idx)
{
    const bool b0 = idx & 1u, b1 = idx & 2u, b2 = idx & 4u;
    const float p0 = b0 ? a[1] : a[0], p1 = b0 ? a[3] : a[2], p2 = b0 ? a[5] : a[4], p3 = b0 ? a[7] : a[6];
    const float q0 = b1 ? p1 : p0, q1 = b1 ? p3 : p2;
    return b2 ? q1 : q0;
}

template <int FORM, int KIND, int OUT>
__global__ void __launch_bounds__(64)
receiver_walk_kernel(const float2 *__restrict__ in, unsigned char *__restrict__ out, float *__restrict__ o_err,
                     float *__restrict__ o_phase, float *__restrict__ o_freq, long long n, ConstState *__restrict__ state,
                     CarrierParams p, ConstDev c, RxTail tl)
{
    extern __shared__ __align__(16) unsigned char lds[];
    constexpr bool ANGLE = FORM == RX_FORM_ANGLE;
    float2 *s_x = (float2 *)lds;                                // the window's samples ...
    float *s_t = (float *)lds;                                  // ... or their angles
    cfloat *s_pts = (cfloat *)(lds + lds_pts(c));
    float *s_ang = (float *)(lds + lds_ang(c));
    unsigned char *s_val = lds + lds_val(c);
    unsigned char *s_map = lds + lds_map(c);
    const int kind = KIND < 0 ? c.kind : KIND;
    const int s = blockIdx.x, lane = threadIdx.x;
    const float2 *__restrict__ x = in + (long long)s * n;
    for (unsigned t = lane; t < c.arity; t += 64) s_pts[t] = c.points[t];
    if (ANGLE)
        for (unsigned t = lane; t < c.n_ang; t += 64) s_ang[t] = c.ang[t];
    if (c.sval)
        for (unsigned t = lane; t < c.n_sectors; t += 64) s_val[t] = c.sval[t];
    if (OUT == 2)
        for (unsigned t = lane; t < 256; t += 64) s_map[t] = tl.map ? tl.map[t] : (unsigned char)t;
    float phase = state[s].phase, freq = state[s].freq;
    unsigned prev = state[s].prev;
    const float inv_wr = kind == CONST_RECT ? 1.0f / c.w_real : 0.f, inv_wi = kind == CONST_RECT ? 1.0f / c.w_imag : 0.f;
    const float inv_width = kind == CONST_PSK ? (float)((double)c.n_sectors / CL_TWOPI) : 0.f;
    float a8[8];                                                // the angles of the first 8 points (angle form, not psk)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const unsigned src = kind == CONST_DQPSK ? dqpsk_of_quadrant(t) : (unsigned)t;     // dqpsk walks by quadrant
        a8[t] = (ANGLE && kind != CONST_PSK && src < c.n_ang) ? c.ang[src] : 0.f;
    }
    float2 v[CARRIER_WIN / 64];
#pragma unroll
    for (int q = 0; q < CARRIER_WIN / 64; ++q) {
        const long long i = lane + 64 * q;
        v[q] = i < n ? x[i] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    for (long long base = 0; base < n; base += CARRIER_WIN) {
        const int m = (int)(n - base < CARRIER_WIN ? n - base : CARRIER_WIN);
#pragma unroll
        for (int q = 0; q < CARRIER_WIN / 64; ++q) {
            if (ANGLE) s_t[lane + 64 * q] = atan2f(v[q].y, v[q].x);
            else s_x[lane + 64 * q] = v[q];
        }
        __syncthreads();
        // the next window's loads, in flight while this one is walked
#pragma unroll
        for (int q = 0; q < CARRIER_WIN / 64; ++q) {
            const long long i = base + CARRIER_WIN + lane + 64 * q;
            v[q] = i < n ? x[i] : make_float2(0.f, 0.f);
        }
        for (int g0 = 0; g0 < m; g0 += 64) {
            const int cnt = m - g0 < 64 ? m - g0 : 64;
            unsigned ki = 0;                                    // this lane's symbol (angle form: its table index)
            float ke = 0.f, kp = phase, kf = freq;              // its error, and the phase and frequency behind it
#pragma unroll 2
            for (int j = 0; j < cnt; ++j) {
                unsigned idx;
                float error;
                if (ANGLE) {
                    const float t = wrap(__fadd_rn(s_t[g0 + j], phase));
                    idx = decide_angle(kind, t, c.n_sectors, inv_width);
                    // the decided point's angle: out of registers for the kinds of at most 8 points, out of LDS for psk
                    error = -wrap(__fsub_rn(t, kind == CONST_PSK ? s_ang[idx] : pick8(a8, idx)));
                } else {
                    const float2 xi = s_x[g0 + j];
                    float sn, cs;                               // gr_expj(d_phase), :104
                    cfloat smp, z;
                    if (FORM == RX_FORM_GENERIC) {
                        sincos_rounded(phase, sn, cs);
                        smp = cmul(cfloat{cs, sn}, cfloat{xi.x, xi.y});                           // :105
                    } else {
                        sincos_fast(phase, sn, cs);
                        smp = cfloat{__fsub_rn(__fmul_rn(cs, xi.x), __fmul_rn(sn, xi.y)), __fadd_rn(__fmul_rn(cs, xi.y), __fmul_rn(sn, xi.x))};
                    }
                    idx = decide_cartesian<FORM>(kind, smp.re, smp.im, c, s_pts, s_val, inv_wr, inv_wi);
                    const cfloat pt = s_pts[idx];
                    // digital_constellation.cc:119-121: `*phase_error = 0; *phase_error += -arg(sample * conj(point))`
                    if (FORM == RX_FORM_GENERIC) {
                        z = cmul(smp, cfloat{pt.re, -pt.im});
                        error = __fadd_rn(0.f, -arg_f(z.im, z.re));
                    } else {
                        z = cfloat{__fadd_rn(__fmul_rn(smp.re, pt.re), __fmul_rn(smp.im, pt.im)), __fsub_rn(__fmul_rn(smp.im, pt.re), __fmul_rn(smp.re, pt.im))};
                        error = -atan2f(z.im, z.re);
                    }
                }
                loop_step(phase, freq, error, p);               // :108, phase_error_tracking
                ki = lane == j ? idx : ki;
                ke = lane == j ? error : ke;
                kp = lane == j ? phase : kp;
                kf = lane == j ? freq : kf;
            }
            unsigned sym = !ANGLE ? ki : (kind == CONST_PSK ? s_val[ki] : (kind == CONST_DQPSK ? dqpsk_of_quadrant(ki) : ki));
            const long long i = (long long)s * n + base + g0 + lane;
            if (OUT == 2) {
                if (lane >= cnt) sym = 0;
                unsigned before = __shfl_up(sym, 1);
                if (lane == 0) before = prev;
                prev = __shfl(sym, cnt - 1);
                // gr_diff_decoder_bb.cc:57: an int difference, converted to unsigned for the %
                // (`& (arity - 1)` is `% arity` for a power of two, without the division)
                const unsigned df = (unsigned)((int)sym - (int)before);
                const unsigned d = !tl.differential ? sym : ((c.arity & (c.arity - 1)) == 0 ? df & (c.arity - 1) : df % c.arity);
                const unsigned mv = s_map[d & 255u];
                if (lane < cnt) {
                    unsigned char *o = out + (size_t)i * tl.k;
                    const bool wide = ((uintptr_t)out % tl.k) == 0;
                    // gr_unpack_k_bits_bb.cc:64-69: bit k-1 first
                    if (tl.k == 1) o[0] = mv & 1u;
                    else if (tl.k == 2 && wide) *(unsigned short *)o = (unsigned short)(((mv >> 1) & 1u) | ((mv & 1u) << 8));
                    else if (tl.k == 4 && wide) *(unsigned *)o = ((mv >> 3) & 1u) | (((mv >> 2) & 1u) << 8) | (((mv >> 1) & 1u) << 16) | ((mv & 1u) << 24);
                    else
                        for (unsigned b = 0; b < tl.k; ++b) o[b] = (mv >> (tl.k - 1 - b)) & 1u;
                }
            } else if (lane < cnt) {
                out[i] = (unsigned char)sym;                    // :110
                if (OUT == 1) {
                    o_err[i] = ke;                              // :113-115
                    o_phase[i] = kp;
                    o_freq[i] = kf;
                }
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        state[s].phase = phase;
        state[s].freq = freq;
        if (OUT == 2) state[s].prev = prev;
    }
}

template <int FORM, int KIND>
int receiver_go(const ConstDev &c, const ReceiverLaunch &a, hipStream_t st)
{
    const RxTail tl = {a.map, a.k, a.differential ? 1u : 0u};
    const unsigned lds = lds_total(c);
#define GRHIP_RX_GO(OUT)                                                                                               \
    do {                                                                                                               \
        if (int rc = allow_lds((const void *)receiver_walk_kernel<FORM, KIND, OUT>, lds)) return rc;                   \
        hipLaunchKernelGGL((receiver_walk_kernel<FORM, KIND, OUT>), dim3(a.nstreams), dim3(64), lds, st, a.in, a.sym, a.err, a.phase, \
                           a.freq, (long long)a.n, a.state, a.p, c, tl);                                               \
    } while (0)
    if (a.tail) GRHIP_RX_GO(2);
    else if (a.err) GRHIP_RX_GO(1);
    else GRHIP_RX_GO(0);
#undef GRHIP_RX_GO
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

// ---- digital_constellation_decoder_cb: one lane per output ----------------------------------------------------------
__global__ void __launch_bounds__(256)
decoder_kernel(const float2 *__restrict__ in, unsigned char *__restrict__ out, long long total, ConstDev c)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const cfloat *smp = (const cfloat *)(in + i * c.dim);   // digital_constellation_decoder_cb.cc:72
        unsigned k;
        switch (c.kind) {
        case CONST_BPSK: k = decide_bpsk(smp->re, smp->im); break;
        case CONST_QPSK: k = decide_qpsk(smp->re, smp->im); break;
        case CONST_DQPSK: k = decide_dqpsk(smp->re, smp->im); break;
        case CONST_8PSK: k = decide_8psk(smp->re, smp->im); break;
        case CONST_PSK: k = c.sval[psk_sector_of(smp->re, smp->im, c.n_sectors)]; break;
        case CONST_RECT: k = c.sval[rect_axis(smp->re, c.w_real, c.n_real) * c.n_imag + rect_axis(smp->im, c.w_imag, c.n_imag)]; break;
        default: k = closest_point(c.points, c.arity, c.dim, smp); break;
        }
        out[i] = (unsigned char)k;
    }
}

// ---- gr_diff_decoder_bb ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
diff_decoder_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, long long n, unsigned modulus,
                    const unsigned *__restrict__ prev, int prev_stride)
{
    const int s = blockIdx.y;
    const unsigned char *__restrict__ x = in + (long long)s * n;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int before = i ? (int)x[i - 1] : (int)(prev[(long long)s * prev_stride] & 255u);
        out[(long long)s * n + i] = (unsigned char)((unsigned)((int)x[i] - before) % modulus);      // gr_diff_decoder_bb.cc:57
    }
}

// after diff_decoder_kernel, in stream order: the stream's last input becomes the next call's in[-1]
__global__ void __launch_bounds__(64)
diff_carry_kernel(const unsigned char *__restrict__ in, long long n, int nstreams, unsigned *__restrict__ prev, int prev_stride)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nstreams) prev[(long long)s * prev_stride] = in[(long long)s * n + n - 1];
}

// ---- gr_map_bb -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
map_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, long long n, const unsigned char *__restrict__ map)
{
    __shared__ unsigned char s_map[256];
    s_map[threadIdx.x] = map[threadIdx.x];
    __syncthreads();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = s_map[in[i]];      // gr_map_bb.cc:58
}

unsigned blocks_for(long long n)
{
    const long long b = (n + 255) / 256, cap = (long long)device_cus() * 32;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

int receiver_launch(int form, const ConstDev &c, const ReceiverLaunch &a, hipStream_t st)
{
    if (a.n <= 0 || a.nstreams <= 0) return GRHIP_OK;
    if (c.dim != 1) return fail(GRHIP_EINVAL, "constellation_receiver_cb: This receiver only works with constellations of dimension 1.");
    if (form == RX_FORM_GENERIC) return receiver_go<RX_FORM_GENERIC, -1>(c, a, st);
    if (form == RX_FORM_CARTESIAN) {
        switch (c.kind) {
        case CONST_RECT: return receiver_go<RX_FORM_CARTESIAN, CONST_RECT>(c, a, st);
        case CONST_CALCDIST: return receiver_go<RX_FORM_CARTESIAN, CONST_CALCDIST>(c, a, st);
        }
        return fail(GRHIP_EINVAL, "receiver: the cartesian form is for rect and calcdist");
    }
    if (form == RX_FORM_ANGLE && c.ang) {
        switch (c.kind) {
        case CONST_BPSK: return receiver_go<RX_FORM_ANGLE, CONST_BPSK>(c, a, st);
        case CONST_QPSK: return receiver_go<RX_FORM_ANGLE, CONST_QPSK>(c, a, st);
        case CONST_DQPSK: return receiver_go<RX_FORM_ANGLE, CONST_DQPSK>(c, a, st);
        case CONST_8PSK: return receiver_go<RX_FORM_ANGLE, CONST_8PSK>(c, a, st);
        case CONST_PSK: return receiver_go<RX_FORM_ANGLE, CONST_PSK>(c, a, st);
        }
    }
    return fail(GRHIP_EINVAL, "receiver: bad form %d for kind %d", form, c.kind);
}

int decoder_launch(const ConstDev &c, const float2 *in, unsigned char *out, int n, int nstreams, hipStream_t st)
{
    if (n <= 0 || nstreams <= 0) return GRHIP_OK;
    const long long total = (long long)n * nstreams;           // the streams lie back to back on both sides
    hipLaunchKernelGGL(decoder_kernel, dim3(blocks_for(total)), dim3(256), 0, st, in, out, total, c);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int diff_decoder_launch(const unsigned char *in, unsigned char *out, int n, int nstreams, unsigned modulus, unsigned *prev,
                        int prev_stride, hipStream_t st)
{
    if (n <= 0 || nstreams <= 0) return GRHIP_OK;
    if (modulus == 0) return fail(GRHIP_EINVAL, "diff_decoder_bb: the modulus must not be 0");
    hipLaunchKernelGGL(diff_decoder_kernel, dim3(blocks_for(n), (unsigned)nstreams), dim3(256), 0, st, in, out, (long long)n, modulus,
                       (const unsigned *)prev, prev_stride);
    GRHIP_HIP(hipGetLastError());
    hipLaunchKernelGGL(diff_carry_kernel, dim3((unsigned)((nstreams + 63) / 64)), dim3(64), 0, st, in, (long long)n, nstreams, prev, prev_stride);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int map_launch(const unsigned char *in, unsigned char *out, long long n, const unsigned char *map, hipStream_t st)
{
    if (n <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(map_kernel, dim3(blocks_for(n)), dim3(256), 0, st, in, out, n, map);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
