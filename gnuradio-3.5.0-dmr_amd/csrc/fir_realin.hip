// fir_realin.hip -- the throughput kernel for REAL input with complex taps: gr_fir_fcc / gr_fir_scc (filterN /
// filterNdec, gr_fir_filter_fcc / _scc) and the inner FIR of gr_freq_xlating_fir_filter_fcf / _fcc / _scf / _scc
// (FIR_TYPE = gr_fir_ + i_code + cc, filter/generate_gr_freq_xlating_fir_filter_XXX.py:30) with the rotator epilogue.
//
// y[n] = sum_k c[k] x[nD + k], x real (float or int16), c complex.  Per tap and output the work is one packed FMA,
// (x, x) * (cr, ci) + acc -- the mirror image of gr_fir_ccf's (xr, xi) * (t, t) -- so the kernel has the shape of
// fir_tiled_kernel with half the bytes per staged sample:
//  * persistent 256-lane workgroups walk tiles of NT = 256 R consecutive outputs (static split);
//  * the tile's input is read from HBM with 16-byte raw buffer loads (the range check supplies the end of the
//    stream).  Items are only 4-byte (float) or 2-byte (int16) aligned -- a scheduler's read pointer lands anywhere --
//    so the loads are aligned to 16 bytes in memory, not to the stream; the one chunk at each end of the stream that
//    reaches outside [x, x + n_in) is read item by item instead, so no byte outside the buffer is touched;
//  * items are widened to float once, at staging, and written to LDS de-interleaved into the D polyphase components
//    (x_p[m] = x[mD + p]) with one pad slot per R samples: the lane stride is R + 1 (odd) 4-byte slots, conflict-free;
//  * each lane keeps R complex accumulators and slides over its samples in blocks of R: one LDS read feeds R FMAs;
//  * the taps are wave-uniform, phase-major, and reach the FMAs as SGPR pairs (scalar loads of 8 complex taps);
//  * epilogue: plain store, or the rotator multiply with the exact-recurrence phase table of XlatingCore::ensure_rot
//    (the reference's unfused complex product, gr_rotator.h:43).  Results leave through vector stores.
#include <cstdint>
#include <vector>

#include "device_math.h"
#include "fir_kernels.h"
#include "grhip_internal.h"

namespace grhip {

namespace {

constexpr int RI_R = 8;                     // outputs per lane
constexpr int RI_T = 256;                   // lanes per workgroup
constexpr int RI_NT = RI_T * RI_R;          // outputs per tile
constexpr int RI_MAX_TAPS = 1024;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef const float __attribute__((address_space(4))) *cfloat_p;      // wave-uniform operands: s_load

// LDS geometry: MM = NT + Tq polyphase samples per component, slot(m) = m + m / R
// (+ R: the MAC loop requests one block beyond the last it uses)
__host__ __device__ constexpr int ri_mm(int Tq) { return RI_NT + Tq + RI_R; }
__host__ __device__ constexpr int ri_phase_stride(int Tq) { return ri_mm(Tq) + ri_mm(Tq) / RI_R + 1; }
inline size_t ri_lds_bytes(int D, int Tq) { return (size_t)D * ri_phase_stride(Tq) * sizeof(float); }

template <typename T, int D, bool ROT>
__global__ void __launch_bounds__(RI_T, 2)
fir_realin_kernel(const T *__restrict__ x, long long n_in, cfloat_p hp, int Tq, float2 *__restrict__ y, long long n_out,
                  const float2 *__restrict__ gtab, long long ntiles)
{
    extern __shared__ __attribute__((aligned(16))) float xs[];
    constexpr int E = 16 / (int)sizeof(T);                  // items per 16-byte chunk
    constexpr int LOGD = D == 1 ? 0 : D == 2 ? 1 : D == 4 ? 2 : 3;
    const int tid = threadIdx.x;
    const int MM = ri_mm(Tq), PS = ri_phase_stride(Tq);
    const int S = MM * D;                                   // items staged per tile

    // buffer resource over [x rounded down to 16 bytes, x + n_in): every 16-byte load is aligned in memory
    const uintptr_t xa = (uintptr_t)x;
    const uintptr_t base = xa & ~(uintptr_t)15;
    const long long lead0 = (long long)((xa - base) / sizeof(T));      // items between base and x
    const long long rec = (long long)(xa - base) + n_in * (long long)sizeof(T);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)rec, 0x00020000);

    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long t0 = tile * RI_NT;
        const long long g0 = t0 * D;                        // first item of the tile (relative to x)
        // chunk c covers items [c0 + cE, c0 + cE + E) where c0 = g0 - lead (aligned in memory)
        const long long a0 = lead0 + g0;                    // item index relative to base
        const long long c0 = a0 - (a0 % E);
        const int nch = (int)((a0 - c0 + S + E - 1) / E);
        for (int c = tid; c < nch; c += RI_T) {
            const long long gb = c0 + (long long)c * E - lead0;            // item index (relative to x) of the chunk's first
            float v[E];
            if (gb >= 0 && gb + E <= n_in) {
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((c0 + (long long)c * E) * sizeof(T)), 0, 0);
                if (sizeof(T) == 4) {
                    typedef float f32x4 __attribute__((ext_vector_type(4)));
                    const f32x4 f = __builtin_bit_cast(f32x4, w);
                    v[0] = f.x; v[1 % E] = f.y; v[2 % E] = f.z; v[3 % E] = f.w;
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) v[e] = (float)(short)(w[e >> 1] >> (16 * (e & 1)));
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const long long gi = gb + e;
                    v[e] = (gi >= 0 && gi < n_in) ? (float)x[gi] : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const long long u = gb + e - g0;            // item within the tile
                if (u >= 0 && u < S) {
                    const int uu = (int)u, m = uu >> LOGD, p = uu & (D - 1);
                    xs[p * PS + m + m / RI_R] = v[e];
                }
            }
        }
        __syncthreads();

        // ---- MAC loop: outputs t0 + tid R + r -----------------------------------------------------------
        f32x2 acc[RI_R];
#pragma unroll
        for (int r = 0; r < RI_R; ++r) acc[r] = f32x2{0.f, 0.f};
        // The lane's samples of component p come in blocks of R (block b = samples tid R + bR .. + R - 1, LDS slot
        // offset (tid + b)(R + 1)); step k multiplies taps kR .. kR + R - 1 against blocks k and k + 1.  What step k + 1
        // needs -- block k + 2 and its taps -- is requested at the top of step k, so the wait for it sits behind
        // R * R packed FMAs.  Three register sets take the block and tap roles in turn: nothing is moved.
        const int nb = Tq / RI_R;
        typedef f32x2 blk_t[RI_R / 2];
        typedef float tapv __attribute__((ext_vector_type(2 * RI_R)));
        for (int p = 0; p < D; ++p) {
            const float *xp = xs + p * PS + tid * (RI_R + 1);
            const cfloat_p hph = hp + (size_t)p * Tq * 2;
            auto load_blk = [&](blk_t &dst, int b) {
                const float *xb = xp + b * (RI_R + 1);
#pragma unroll
                for (int j = 0; j < RI_R / 2; ++j) dst[j] = f32x2{xb[2 * j], xb[2 * j + 1]};
            };
            // One step is ONE asm statement: the scalar load of the next step's taps, the R * R packed FMAs and the
            // wait for that load (tools/gen_realin_step.py).  Left to the compiler, the tap load lands next to its
            // use and every step waits a scalar-cache latency, which also drains the LDS reads just issued (SMEM and
            // LDS share a counter).  The tap table is padded by R taps: the last step's load reads the pad.
            auto step = [&](const blk_t &cur, const blk_t &nxt, blk_t &ld, tapv &tc, int k) {
                load_blk(ld, k + 2);
                const f32x2 t0{tc[0], tc[1]}, t1{tc[2], tc[3]}, t2{tc[4], tc[5]}, t3{tc[6], tc[7]};
                const f32x2 t4{tc[8], tc[9]}, t5{tc[10], tc[11]}, t6{tc[12], tc[13]}, t7{tc[14], tc[15]};
                const cfloat_p src = hph + (size_t)(k + 1) * RI_R * 2;
                tapv tn;
                asm volatile(
#include "realin_step.inc"
                    : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]),
                      "+v"(acc[7]), "=&s"(tn)
                    : "v"(cur[0]), "v"(cur[1]), "v"(cur[2]), "v"(cur[3]), "v"(nxt[0]), "v"(nxt[1]), "v"(nxt[2]),
                      "v"(nxt[3]), "s"(t0), "s"(t1), "s"(t2), "s"(t3), "s"(t4), "s"(t5), "s"(t6), "s"(t7), "s"(src));
                tc = tn;
            };
            blk_t bA, bB, bC;
            tapv tc = *reinterpret_cast<const tapv __attribute__((address_space(4))) *>(hph);
            load_blk(bA, 0);
            load_blk(bB, 1);
            int k = 0;
            for (; k + 3 <= nb; k += 3) {
                step(bA, bB, bC, tc, k);
                step(bB, bC, bA, tc, k + 1);
                step(bC, bA, bB, tc, k + 2);
            }
            if (k < nb) step(bA, bB, bC, tc, k);
            if (k + 1 < nb) step(bB, bC, bA, tc, k + 1);
        }

        // ---- epilogue: vector stores ---------------------------------------------------------------------
#pragma unroll
        for (int r = 0; r < RI_R; ++r) {
            const long long o = t0 + (long long)tid * RI_R + r;
            if (o < n_out) {
                float2 v = make_float2(acc[r].x, acc[r].y);
                if (ROT) v = cmul_ref(v, gtab[o]);          // gr_rotator::rotate: z = in * d_phase
                y[o] = v;
            }
        }
        __syncthreads();                                    // the next tile overwrites the LDS
    }
}

template <typename T, int D, bool ROT>
int launch_realin_inst(const float *hp, int Tq, const void *x, long long n_in, float2 *y, long long n_out, const float2 *gtab,
                       hipStream_t st)
{
    const size_t lds = ri_lds_bytes(D, Tq);
    if (int rc = allow_lds((const void *)fir_realin_kernel<T, D, ROT>, lds)) return rc;
    const long long ntiles = (n_out + RI_NT - 1) / RI_NT;
    const int per_cu = lds * 2 <= 160 * 1024 ? 2 : 1;
    long long grid = (long long)device_cus() * per_cu;
    if (grid > ntiles) grid = ntiles;
    hipLaunchKernelGGL((fir_realin_kernel<T, D, ROT>), dim3((unsigned)grid), dim3(RI_T), lds, st, (const T *)x, n_in,
                       (cfloat_p)hp, Tq, y, n_out, gtab, ntiles);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <typename T, bool ROT>
int launch_realin_d(int decim, const float *hp, int Tq, const void *x, long long n_in, float2 *y, long long n_out,
                    const float2 *gtab, hipStream_t st)
{
    switch (decim) {
    case 1: return launch_realin_inst<T, 1, ROT>(hp, Tq, x, n_in, y, n_out, gtab, st);
    case 2: return launch_realin_inst<T, 2, ROT>(hp, Tq, x, n_in, y, n_out, gtab, st);
    case 4: return launch_realin_inst<T, 4, ROT>(hp, Tq, x, n_in, y, n_out, gtab, st);
    case 8: return launch_realin_inst<T, 8, ROT>(hp, Tq, x, n_in, y, n_out, gtab, st);
    default: return fail(GRHIP_EINVAL, "real-input FIR: decimation %d has no fast kernel", decim);
    }
}

// (short)acc as the reference's x86-64 build converts it (gr_fir_fsf: float engines, then this pass)
__global__ void __launch_bounds__(256) f2s_kernel(const float *__restrict__ a, short *__restrict__ o, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = ref_f2s(a[i]);
}

}  // namespace

bool realin_supported(int decim, int ntaps)
{
    if (!(decim == 1 || decim == 2 || decim == 4 || decim == 8)) return false;
    if (ntaps < 1 || ntaps > RI_MAX_TAPS) return false;
    const int per = (ntaps + decim - 1) / decim;
    const int Tq = ((per + RI_R - 1) / RI_R) * RI_R;
    return ri_lds_bytes(decim, Tq) <= 80 * 1024;        // two workgroups per CU
}

int realin_pack_taps(const float *c, int ntaps, int decim, std::vector<float> &hp)
{
    const int per = (ntaps + decim - 1) / decim;
    int Tq = ((per + RI_R - 1) / RI_R) * RI_R;
    if (Tq == 0) Tq = RI_R;
    hp.assign(((size_t)decim * Tq + RI_R) * 2, 0.f);
    for (int k = 0; k < ntaps; ++k) {
        const int p = k % decim, q = k / decim;
        hp[((size_t)p * Tq + q) * 2] = c[2 * (size_t)k];
        hp[((size_t)p * Tq + q) * 2 + 1] = c[2 * (size_t)k + 1];
    }
    return Tq;
}

int launch_fir_realin(bool in_short, int decim, const float *hp, int Tq, const void *x, long long n_in, float2 *y,
                      long long n_out, const float2 *gtab, hipStream_t st)
{
    if (n_out <= 0) return GRHIP_OK;
    if (((uintptr_t)x) & (in_short ? 1 : 3)) return fail(GRHIP_EINVAL, "real-input FIR: items not naturally aligned");
    if (((uintptr_t)y) & 7) return fail(GRHIP_EINVAL, "real-input FIR: output not 8-byte aligned");
    if ((n_in + 8) * (in_short ? 2 : 4) >= 0x7fffffffll) return fail(GRHIP_EINVAL, "real-input FIR: input over 2 GiB");
    if (in_short)
        return gtab ? launch_realin_d<short, true>(decim, hp, Tq, x, n_in, y, n_out, gtab, st)
                    : launch_realin_d<short, false>(decim, hp, Tq, x, n_in, y, n_out, gtab, st);
    return gtab ? launch_realin_d<float, true>(decim, hp, Tq, x, n_in, y, n_out, gtab, st)
                : launch_realin_d<float, false>(decim, hp, Tq, x, n_in, y, n_out, gtab, st);
}

int launch_f2s(const float *a, short *o, long long n, hipStream_t st)
{
    if (n <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(f2s_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, o, n);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
