// modulator.hip -- the byte and symbol blocks in front of the pulse shaper of gr-digital/python/generic_mod_demod.py:114-150:
// gr_packed_to_unpacked_bb (gengen/gr_packed_to_unpacked_XX.cc.t:84-137), gr_unpacked_to_packed_bb
// (gengen/gr_unpacked_to_packed_XX.cc.t:66-129), gr_diff_encoder_bb (general/gr_diff_encoder_bb.cc:44-62) and
// gr_chunks_to_symbols_bc (gengen/gr_chunks_to_symbols_XX.cc.t:51-74): kernels.
//
// None of them has a serial dependency that needs one lane per stream: the two repackers are a closed form per output
// item, the symbol table a lookup per output item, and the differential encoder a prefix sum modulo its modulus
// (modulator_plan.h says for which moduli), run as tile sums, a carry pass and the tiles again from their carries.
// The arithmetic is integer throughout, so every mode gives the same bytes.
#include "grhip_internal.h"
#include "modulator.h"

namespace grhip {

namespace {

constexpr int MOD_THREADS = 256;

unsigned blocks_for(long long n)
{
    const long long b = (n + MOD_THREADS - 1) / MOD_THREADS, cap = (long long)device_cus() * 32;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- gr_packed_to_unpacked_bb: one lane per output chunk -------------------------------------------------------------------
// Chunk i is the k bits from bit address index + i*k: at most two bytes.  MSB_FIRST counts a byte's bits from the top
// (get_bit_be, .cc.t:77-82), LSB_FIRST from the bottom (get_bit_le, :70-75); both shift the bits in from the right
// (x = (x << 1) | bit, :109 and :119), so the LSB_FIRST chunk is its bits in reverse.
template <bool LSB>
__global__ void __launch_bounds__(MOD_THREADS)
p2u_kernel(const unsigned char *__restrict__ in, long long ninput, unsigned char *__restrict__ out, long long noutput, unsigned k,
           unsigned index)
{
    const unsigned char *__restrict__ x = in + (long long)blockIdx.y * ninput;
    unsigned char *__restrict__ y = out + (long long)blockIdx.y * noutput;
    const unsigned mask = (1u << k) - 1u;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < noutput; i += stride) {
        const unsigned long long b = index + (unsigned long long)i * k;
        const long long byte = (long long)(b >> 3);
        const unsigned sh = (unsigned)(b & 7u);
        const unsigned b0 = byte < ninput ? x[byte] : 0u;
        const unsigned b1 = (sh + k > 8u && byte + 1 < ninput) ? x[byte + 1] : 0u;      // only when the chunk reaches into it
        unsigned v;
        if (LSB) v = __brev(((b0 | (b1 << 8)) >> sh) & mask) >> (32u - k);
        else v = (((b0 << 8) | b1) >> (16u - sh - k)) & mask;
        y[i] = (unsigned char)v;
    }
}

// ---- gr_unpacked_to_packed_bb: one lane per output byte --------------------------------------------------------------------
// Byte i is the 8 bits from bit address index + i*8, where address a is bit k-1 - a%k of chunk a/k (get_bit_be1,
// .cc.t:66-73).  MSB_FIRST shifts them in from the right (:101), LSB_FIRST from the top down (:112): the first bit
// ends as bit 0.
template <bool LSB>
__global__ void __launch_bounds__(MOD_THREADS)
u2p_kernel(const unsigned char *__restrict__ in, long long ninput, unsigned char *__restrict__ out, long long noutput, unsigned k,
           unsigned index)
{
    const unsigned char *__restrict__ x = in + (long long)blockIdx.y * ninput;
    unsigned char *__restrict__ y = out + (long long)blockIdx.y * noutput;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < noutput; i += stride) {
        const unsigned long long a = index + (unsigned long long)i * 8u;
        long long c = (long long)(a / k);
        unsigned r = (unsigned)(a - (unsigned long long)c * k);
        unsigned cur = c < ninput ? x[c] : 0u, v = 0;
#pragma unroll
        for (unsigned j = 0; j < 8; ++j) {
            const unsigned bit = (cur >> (k - 1u - r)) & 1u;
            v = LSB ? (v | (bit << j)) : ((v << 1) | bit);
            if (++r == k && j < 7) {
                r = 0;
                ++c;
                cur = c < ninput ? x[c] : 0u;
            }
        }
        y[i] = (unsigned char)v;
    }
}

// ---- gr_diff_encoder_bb ----------------------------------------------------------------------------------------------------
// inclusive scan modulo m of one value (below m) per lane of the workgroup
__device__ __forceinline__ unsigned block_scan_mod(unsigned v, unsigned m, unsigned *ps)
{
    const int t = threadIdx.x;
    ps[t] = v;
    __syncthreads();
    for (int off = 1; off < DIFF_THREADS; off <<= 1) {
        const unsigned add = t >= off ? ps[t - off] : 0u;
        __syncthreads();
        v = (v + add) % m;
        ps[t] = v;
        __syncthreads();
    }
    return v;
}

// pass 1: the sum of every tile modulo m
__global__ void __launch_bounds__(DIFF_THREADS)
diff_tile_sum_kernel(const unsigned char *__restrict__ in, long long n, long long tiles, unsigned m, unsigned *__restrict__ sums)
{
    __shared__ unsigned ps[DIFF_THREADS];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * DIFF_TILE;
    const unsigned char *__restrict__ x = in + (long long)blockIdx.y * n + base;
    const int cnt = (int)(n - base < DIFF_TILE ? n - base : DIFF_TILE);
    unsigned s = 0;
    for (int u = t; u < cnt; u += DIFF_THREADS) s += x[u];             // at most 8 * 255
    ps[t] = s;
    __syncthreads();
    for (int off = DIFF_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) ps[t] += ps[t + off];                             // at most 2048 * 255
        __syncthreads();
    }
    if (t == 0) sums[diff_carry_slot(blockIdx.y, tiles, blockIdx.x)] = ps[0] % m;
}

// pass 2, one workgroup per stream: the tile sums become the tiles' carries (the encoder's last_out in front of the
// tile), seeded with the stream's last_out, which is left as the value behind the last tile
__global__ void __launch_bounds__(DIFF_THREADS)
diff_carry_kernel(unsigned *__restrict__ sums, long long tiles, unsigned m, unsigned *__restrict__ last_out)
{
    __shared__ unsigned ps[DIFF_THREADS];
    const int t = threadIdx.x;
    unsigned *__restrict__ row = sums + diff_carry_slot(blockIdx.x, tiles, 0);
    const long long per = (tiles + DIFF_THREADS - 1) / DIFF_THREADS;
    const long long lo = t * per < tiles ? t * per : tiles, hi = lo + per < tiles ? lo + per : tiles;
    unsigned s = 0;
    for (long long i = lo; i < hi; ++i) s = (s + row[i]) % m;
    const unsigned seed = last_out[blockIdx.x] % m;
    const unsigned incl = block_scan_mod(s, m, ps);                    // every lane has read the seed behind its barriers
    unsigned run = (seed + incl + m - s) % m;                          // seed + the lanes in front
    for (long long i = lo; i < hi; ++i) {
        const unsigned v = row[i];
        row[i] = run;
        run = (run + v) % m;
    }
    if (t == DIFF_THREADS - 1) last_out[blockIdx.x] = (seed + incl) % m;
}

// pass 3: every tile again, from its carry
__global__ void __launch_bounds__(DIFF_THREADS)
diff_encode_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, long long n, long long tiles, unsigned m,
                   const unsigned *__restrict__ carry)
{
    __shared__ __attribute__((aligned(8))) unsigned char buf[DIFF_TILE];
    __shared__ unsigned ps[DIFF_THREADS];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * DIFF_TILE;
    const unsigned char *__restrict__ x = in + (long long)blockIdx.y * n + base;
    unsigned char *__restrict__ y = out + (long long)blockIdx.y * n + base;
    const int cnt = (int)(n - base < DIFF_TILE ? n - base : DIFF_TILE);
    for (int u = t; u < DIFF_TILE; u += DIFF_THREADS) buf[u] = u < cnt ? x[u] : (unsigned char)0;    // zeros add nothing
    __syncthreads();
    unsigned char *mine = buf + t * DIFF_PER_LANE;
    unsigned s = 0;
#pragma unroll
    for (int j = 0; j < DIFF_PER_LANE; ++j) s += mine[j];
    s %= m;
    const unsigned incl = block_scan_mod(s, m, ps);
    unsigned v = (carry[diff_carry_slot(blockIdx.y, tiles, blockIdx.x)] + incl + m - s) % m;
#pragma unroll
    for (int j = 0; j < DIFF_PER_LANE; ++j) {
        v = (v + mine[j]) % m;                                         // gr_diff_encoder_bb.cc:56-57
        mine[j] = (unsigned char)v;                                    // m <= 256: v is the byte
    }
    __syncthreads();
    for (int u = t; u < cnt; u += DIFF_THREADS) y[u] = buf[u];
}

// moduli 257 .. 510: the reference's loop, one lane per stream
__global__ void __launch_bounds__(64)
diff_serial_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, long long n, int nstreams, unsigned modulus,
                   unsigned *__restrict__ last_out)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstreams) return;
    const unsigned char *__restrict__ x = in + (long long)s * n;
    unsigned char *__restrict__ y = out + (long long)s * n;
    unsigned last = last_out[s];
    for (long long i = 0; i < n; ++i) {
        const unsigned char o = (unsigned char)((x[i] + last) % modulus);      // :56
        y[i] = o;
        last = o;                                                              // :57, read back from the byte
    }
    last_out[s] = last;
}

// ---- gr_chunks_to_symbols_bc: one lane per output item, 8-byte stores ------------------------------------------------------
// out[i*D + d] = table[in[i]*D + d] (.cc.t:65-69); an index whose D entries do not lie inside the table gives zeros,
// where the reference asserts (:66) or reads outside its vector.
template <bool IN_LDS>
__global__ void __launch_bounds__(MOD_THREADS)
c2s_kernel(const unsigned char *__restrict__ in, long long in_stride, float2 *__restrict__ out, long long out_stride, long long n_out,
           const float2 *__restrict__ table, unsigned table_size, unsigned D)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const float2 *tab = table;
    if (IN_LDS) {
        float2 *ts = reinterpret_cast<float2 *>(smem);
        for (unsigned i = threadIdx.x; i < table_size; i += MOD_THREADS) ts[i] = table[i];
        __syncthreads();
        tab = ts;
    }
    const unsigned char *__restrict__ x = in + (long long)blockIdx.y * in_stride;
    float2 *__restrict__ y = out + (long long)blockIdx.y * out_stride;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += stride) {
        const long long c = D == 1 ? o : o / D;
        const unsigned d = (unsigned)(o - c * D);
        const unsigned long long first = (unsigned long long)x[c] * D;
        float2 r = make_float2(0.f, 0.f);
        if (first + D <= table_size) r = tab[first + d];
        y[o] = r;
    }
}

}  // namespace

int packed_to_unpacked_launch(const unsigned char *in, long long ninput, unsigned char *out, long long noutput, int nstreams,
                              unsigned k, bool lsb_first, unsigned index, hipStream_t st)
{
    if (noutput <= 0 || nstreams <= 0) return GRHIP_OK;
    // index 8 skips in[0]: generic_mod's call that carries no bits but keeps the carried byte in front
    if (!pack_k_ok(k) || index > 8u) return fail(GRHIP_EINVAL, "packed_to_unpacked_bb: bad bits_per_chunk or index");
    const dim3 grid(blocks_for(noutput), (unsigned)nstreams);
    if (lsb_first) hipLaunchKernelGGL(p2u_kernel<true>, grid, dim3(MOD_THREADS), 0, st, in, ninput, out, noutput, k, index);
    else hipLaunchKernelGGL(p2u_kernel<false>, grid, dim3(MOD_THREADS), 0, st, in, ninput, out, noutput, k, index);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int unpacked_to_packed_launch(const unsigned char *in, long long ninput, unsigned char *out, long long noutput, int nstreams,
                              unsigned k, bool lsb_first, unsigned index, hipStream_t st)
{
    if (noutput <= 0 || nstreams <= 0) return GRHIP_OK;
    if (!pack_k_ok(k) || index >= k) return fail(GRHIP_EINVAL, "unpacked_to_packed_bb: bad bits_per_chunk or index");
    const dim3 grid(blocks_for(noutput), (unsigned)nstreams);
    if (lsb_first) hipLaunchKernelGGL(u2p_kernel<true>, grid, dim3(MOD_THREADS), 0, st, in, ninput, out, noutput, k, index);
    else hipLaunchKernelGGL(u2p_kernel<false>, grid, dim3(MOD_THREADS), 0, st, in, ninput, out, noutput, k, index);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int diff_carry_launch(unsigned *sums, long long tiles, unsigned m, unsigned *last_out, int nstreams, hipStream_t st)
{
    if (tiles <= 0 || nstreams <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(diff_carry_kernel, dim3((unsigned)nstreams), dim3(DIFF_THREADS), 0, st, sums, tiles, m, last_out);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int diff_encoder_launch(const unsigned char *in, unsigned char *out, long long n, int nstreams, unsigned modulus,
                        unsigned *last_out, unsigned *scratch, hipStream_t st)
{
    if (n <= 0 || nstreams <= 0) return GRHIP_OK;
    if (modulus == 0) return fail(GRHIP_EINVAL, "diff_encoder_bb: the modulus must not be 0");
    const unsigned m = diff_scan_modulus(modulus);
    if (m == 0) {       // 257 .. 510: no scan (modulator_plan.h)
        hipLaunchKernelGGL(diff_serial_kernel, dim3((unsigned)((nstreams + 63) / 64)), dim3(64), 0, st, in, out, n, nstreams, modulus,
                           last_out);
        GRHIP_HIP(hipGetLastError());
        return GRHIP_OK;
    }
    const long long tiles = diff_tiles(n);
    if (tiles > 0x7fffffffLL || nstreams > 65535) return fail(GRHIP_EINVAL, "diff_encoder_bb: grid too large");
    const dim3 grid((unsigned)tiles, (unsigned)nstreams);
    hipLaunchKernelGGL(diff_tile_sum_kernel, grid, dim3(DIFF_THREADS), 0, st, in, n, tiles, m, scratch);
    GRHIP_HIP(hipGetLastError());
    if (int rc = diff_carry_launch(scratch, tiles, m, last_out, nstreams, st)) return rc;
    hipLaunchKernelGGL(diff_encode_kernel, grid, dim3(DIFF_THREADS), 0, st, in, out, n, tiles, m, (const unsigned *)scratch);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int chunks_to_symbols_launch(const unsigned char *in, long long in_stride, float2 *out, long long out_stride, long long n, int nstreams,
                             const float2 *table, unsigned table_size, unsigned D, hipStream_t st)
{
    if (n <= 0 || nstreams <= 0) return GRHIP_OK;
    if (D < 1 || table_size < 1 || table_size > (unsigned)C2S_MAX_ENTRIES) return fail(GRHIP_EINVAL, "chunks_to_symbols_bc: bad table or D");
    if (nstreams > 65535) return fail(GRHIP_EINVAL, "chunks_to_symbols_bc: grid too large");
    const long long n_out = n * (long long)D;
    const dim3 grid(blocks_for(n_out), (unsigned)nstreams);
    if (table_size <= (unsigned)C2S_LDS_ENTRIES)
        hipLaunchKernelGGL(c2s_kernel<true>, grid, dim3(MOD_THREADS), (size_t)table_size * sizeof(float2), st, in, in_stride, out, out_stride,
                           n_out, table, table_size, D);
    else
        hipLaunchKernelGGL(c2s_kernel<false>, grid, dim3(MOD_THREADS), 0, st, in, in_stride, out, out_stride, n_out, table, table_size, D);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
