// lfsr_blocks.hip -- kernels of gr_scrambler_bb (general/gr_scrambler_bb.cc:44-57), gr_descrambler_bb
// (general/gr_descrambler_bb.cc:44-57) and gr_additive_scrambler_bb (general/gr_additive_scrambler_bb.cc:46-65) on
// gri_lfsr (general/gri_lfsr.h:103-147), S streams back to back.
//
// The serial kernel is the reference's statements, one lane per stream.  The parallel kernels rest on the register's
// step being linear over GF(2) once no bit lies above reg_len (csrc/gf2.h):
//   descrambler  no feedback: the register in front of item i is the reg_len + 1 input bits before it (and what is left
//                of the stream's register), so a lane rebuilds it from 32 input bytes and walks LFSR_WALK items;
//   additive     the register does not depend on the data: a lane jumps it to its first item with M^(2^j) and walks;
//   scrambler    reg' = M reg ^ in e_L is affine: lanes walk their chunk from a zero register, a workgroup scans the
//                results with M^(LFSR_CHUNK 2^j), a carry pass runs along the tiles of a stream, and the tiles run
//                again from their true registers (the structure of diff_encoder_bb, csrc/modulator.hip).
#include "packet.h"

namespace grhip {

namespace {

// gri_lfsr.h:120-125 and :127-132
__device__ __forceinline__ unsigned scramble_step(unsigned &reg, unsigned in, unsigned mask, unsigned len)
{
    const unsigned out = reg & 1u;
    reg = lfsr_step_or(reg, lfsr_parity(reg & mask) ^ (in & 1u), len);
    return out;
}
__device__ __forceinline__ unsigned descramble_step(unsigned &reg, unsigned in, unsigned mask, unsigned len)
{
    const unsigned out = lfsr_parity(reg & mask) ^ (in & 1u);
    reg = lfsr_step_or(reg, in & 1u, len);
    return out;
}
// gr_additive_scrambler_bb.cc:55-61: the whole input byte XOR the bit
__device__ __forceinline__ unsigned additive_step(unsigned &reg, unsigned &bits, unsigned in, const LfsrParams &p)
{
    const unsigned out = in ^ (reg & 1u);
    reg = lfsr_next(reg, p.mask, p.len);
    if (p.count > 0u && ++bits == p.count) { reg = p.seed; bits = 0u; }
    return out;
}

__global__ void __launch_bounds__(64)
lfsr_serial_kernel(int kind, const unsigned char *__restrict__ in, unsigned char *__restrict__ out, long long n, long long first,
                   long long cnt, int nstreams, LfsrParams p, LfsrState *__restrict__ state)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nstreams) return;
    const unsigned char *x = in + (long long)s * n + first;
    unsigned char *y = out + (long long)s * n + first;
    LfsrState t = state[s];
    if (kind == LFSR_SCRAMBLE)
        for (long long i = 0; i < cnt; ++i) y[i] = (unsigned char)scramble_step(t.reg, x[i], p.mask, p.len);
    else if (kind == LFSR_DESCRAMBLE)
        for (long long i = 0; i < cnt; ++i) y[i] = (unsigned char)descramble_step(t.reg, x[i], p.mask, p.len);
    else
        for (long long i = 0; i < cnt; ++i) y[i] = (unsigned char)additive_step(t.reg, t.bits, x[i], p);
    state[s] = t;
}

// ---- descrambler ----------------------------------------------------------------------------------------------------
// the register in front of item i of the call: the stream's register shifted down i times, ORed with the input bits of
// the 32 items before i, the last one at bit len
__device__ __forceinline__ unsigned descramble_reg_at(const unsigned char *__restrict__ x, long long i, unsigned reg0, unsigned len)
{
    unsigned reg = i < 32 ? reg0 >> (unsigned)i : 0u;
    const long long j0 = i - 32 > 0 ? i - 32 : 0;
    for (long long j = j0; j < i; ++j) {
        const unsigned back = (unsigned)(i - 1 - j);
        if (back <= len) reg |= (unsigned)(x[j] & 1u) << (len - back);
    }
    return reg;
}

__global__ void __launch_bounds__(LFSR_THREADS)
descramble_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, long long n, long long first, LfsrParams p,
                  const LfsrState *__restrict__ state)
{
    const int s = blockIdx.y;
    const unsigned char *x = in + (long long)s * n;
    unsigned char *y = out + (long long)s * n;
    const long long i0 = first + ((long long)blockIdx.x * LFSR_THREADS + threadIdx.x) * LFSR_WALK;
    if (i0 >= n) return;
    const int cnt = (int)(n - i0 < LFSR_WALK ? n - i0 : LFSR_WALK);
    unsigned reg = descramble_reg_at(x, i0, state[s].reg, p.len);
    for (int j = 0; j < cnt; ++j) y[i0 + j] = (unsigned char)descramble_step(reg, x[i0 + j], p.mask, p.len);
}

__global__ void __launch_bounds__(64)
descramble_state_kernel(const unsigned char *__restrict__ in, long long n, int nstreams, LfsrParams p, LfsrState *__restrict__ state)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nstreams) return;
    state[s].reg = descramble_reg_at(in + (long long)s * n, n, state[s].reg, p.len);
}

// ---- additive scrambler ---------------------------------------------------------------------------------------------
// (register, d_bits) in front of item i of the call, from those at its start
__device__ __forceinline__ LfsrState additive_state_at(long long i, LfsrState t0, const LfsrParams &p, const unsigned *__restrict__ pw)
{
    if (p.count == 0u) return LfsrState{lfsr_advance(t0.reg, (unsigned)i, p.mask, p.len, pw), t0.bits};
    const long long left = (long long)p.count - t0.bits;        // items until the first reset
    if (i < left) return LfsrState{lfsr_advance(t0.reg, (unsigned)i, p.mask, p.len, pw), t0.bits + (unsigned)i};
    const unsigned pos = (unsigned)((i - left) % p.count);
    return LfsrState{lfsr_advance(p.seed, pos, p.mask, p.len, pw), pos};
}

__global__ void __launch_bounds__(LFSR_THREADS)
additive_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, long long n, long long first, LfsrParams p,
                const LfsrState *__restrict__ state, const unsigned *__restrict__ pw)
{
    const int s = blockIdx.y;
    const unsigned char *x = in + (long long)s * n;
    unsigned char *y = out + (long long)s * n;
    const long long i0 = first + ((long long)blockIdx.x * LFSR_THREADS + threadIdx.x) * LFSR_WALK;
    if (i0 >= n) return;
    const int cnt = (int)(n - i0 < LFSR_WALK ? n - i0 : LFSR_WALK);
    LfsrState t = additive_state_at(i0, state[s], p, pw);
    for (int j = 0; j < cnt; ++j) y[i0 + j] = (unsigned char)additive_step(t.reg, t.bits, x[i0 + j], p);
}

__global__ void __launch_bounds__(64)
additive_state_kernel(long long n, int nstreams, LfsrParams p, LfsrState *__restrict__ state, const unsigned *__restrict__ pw)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nstreams) return;
    state[s] = additive_state_at(n, state[s], p, pw);
}

// ---- scrambler ------------------------------------------------------------------------------------------------------
// the linear step: equal to scramble_step for a register without bits above len
__device__ __forceinline__ unsigned scramble_xor(unsigned reg, unsigned in, unsigned mask, unsigned len)
{
    return (reg >> 1) ^ ((lfsr_parity(reg & mask) ^ (in & 1u)) << len);
}

// One tile of one stream.  WRITE false: every lane walks its chunk from a zero register, the scan composes the chunks,
// and the tile's effect on a zero register goes to tile_regs.  WRITE true: lane 0 starts from the tile's true register
// (tile_regs, after the carry pass), so the scan gives every chunk's true end register; the chunks run again from
// the one before them and write.  The tile's bytes pass through LDS both ways, so that global loads and stores are
// of consecutive bytes per wave.  Lanes behind the stream's end hold nothing anybody reads.
template <bool WRITE>
__global__ void __launch_bounds__(LFSR_SCAN_THREADS)
scramble_tile_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, long long n, long long first, long long tiles,
                     LfsrParams p, unsigned *__restrict__ tile_regs, LfsrState *__restrict__ state, const unsigned *__restrict__ mats)
{
    __shared__ __attribute__((aligned(16))) unsigned char buf[LFSR_TILE];
    __shared__ unsigned ps[LFSR_SCAN_THREADS];
    const int s = blockIdx.y, t = threadIdx.x;
    const long long npar = n - first, tile_base = (long long)blockIdx.x * LFSR_TILE;
    const int tile_cnt = (int)(npar - tile_base < LFSR_TILE ? npar - tile_base : LFSR_TILE);     // >= 1: the grid has lfsr_tiles(npar) tiles
    const unsigned char *x = in + (long long)s * n + first + tile_base;
    for (int u = t; u < LFSR_TILE; u += LFSR_SCAN_THREADS) buf[u] = u < tile_cnt ? x[u] : (unsigned char)0;
    __syncthreads();
    const int left = tile_cnt - t * LFSR_CHUNK;
    const int cnt = left < 0 ? 0 : (left < LFSR_CHUNK ? left : LFSR_CHUNK);
    unsigned *mine = reinterpret_cast<unsigned *>(buf + t * LFSR_CHUNK);
    unsigned bits = 0;                                          // bit j: the input bit of the chunk's item j
#pragma unroll
    for (int k = 0; k < LFSR_CHUNK / 4; ++k) bits |= ((((mine[k] & 0x01010101u) * 0x01020408u) >> 24) & 0xfu) << (4 * k);
    const unsigned start0 = WRITE && t == 0 ? tile_regs[(long long)s * tiles + blockIdx.x] : 0u;
    unsigned b = start0;
    for (int j = 0; j < cnt; ++j) b = scramble_xor(b, bits >> j, p.mask, p.len);
    const unsigned *scan = mats + 32 * LFSR_MAT_SCAN;
    for (int j = 0, off = 1; off < LFSR_SCAN_THREADS; ++j, off <<= 1) {
        ps[t] = b;
        __syncthreads();
        if (t >= off) b ^= gf2_matvec(scan + 32 * j, ps[t - off]);      // the chunks before, carried over `off` chunks
        __syncthreads();
    }
    if (!WRITE) {
        if (t == LFSR_SCAN_THREADS - 1) tile_regs[(long long)s * tiles + blockIdx.x] = b;
        return;
    }
    ps[t] = b;
    __syncthreads();
    unsigned reg = t == 0 ? start0 : ps[t - 1];
#pragma unroll
    for (int k = 0; k < LFSR_CHUNK / 4; ++k) {                  // the chunk's outputs over its inputs, four to a word
        unsigned w = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = 4 * k + q;
            w |= (reg & 1u) << (8 * q);
            if (j < cnt) reg = scramble_xor(reg, bits >> j, p.mask, p.len);
        }
        mine[k] = w;
    }
    if (cnt > 0 && t * LFSR_CHUNK + cnt == tile_cnt && tile_base + tile_cnt == npar) state[s].reg = reg;
    __syncthreads();
    unsigned char *y = out + (long long)s * n + first + tile_base;
    for (int u = t; u < tile_cnt; u += LFSR_SCAN_THREADS) y[u] = buf[u];
}

// tile_regs: in, what each tile does to a zero register; out, the register in front of each tile
__global__ void __launch_bounds__(64)
scramble_carry_kernel(long long tiles, int nstreams, unsigned *__restrict__ tile_regs, const LfsrState *__restrict__ state,
                      const unsigned *__restrict__ mats)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nstreams) return;
    unsigned *r = tile_regs + (long long)s * tiles;
    unsigned c = state[s].reg;
    for (long long k = 0; k < tiles; ++k) {
        const unsigned e = r[k];
        r[k] = c;
        c = gf2_matvec(mats + 32 * LFSR_MAT_TILE, c) ^ e;
    }
}

}  // namespace

int lfsr_serial_launch(int kind, const unsigned char *in, unsigned char *out, long long n, long long first, long long cnt, int nstreams,
                       const LfsrParams &p, LfsrState *state, hipStream_t st)
{
    if (cnt <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(lfsr_serial_kernel, dim3((unsigned)((nstreams + 63) / 64)), dim3(64), 0, st, kind, in, out, n, first, cnt, nstreams, p,
                       state);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int lfsr_parallel_launch(int kind, const unsigned char *in, unsigned char *out, long long n, long long first, int nstreams,
                         const LfsrParams &p, LfsrState *state, const unsigned *mats, unsigned *scratch, hipStream_t st)
{
    const long long npar = n - first;
    if (npar <= 0) return GRHIP_OK;
    if (nstreams > 65535) return fail(GRHIP_EINVAL, "scrambler: at most 65535 streams");
    const dim3 per_stream((unsigned)((nstreams + 63) / 64));
    if (kind == LFSR_SCRAMBLE) {
        const long long tiles = lfsr_tiles(npar);
        if (tiles > 0x7fffffffLL) return fail(GRHIP_EINVAL, "scrambler_bb: grid too large");
        const dim3 grid((unsigned)tiles, (unsigned)nstreams);
        if (tiles > 1)      // a lone tile starts from the stream's register, whatever the carry pass finds in its slot
            hipLaunchKernelGGL(scramble_tile_kernel<false>, grid, dim3(LFSR_SCAN_THREADS), 0, st, in, out, n, first, tiles, p, scratch, state, mats);
        hipLaunchKernelGGL(scramble_carry_kernel, per_stream, dim3(64), 0, st, tiles, nstreams, scratch, (const LfsrState *)state, mats);
        hipLaunchKernelGGL(scramble_tile_kernel<true>, grid, dim3(LFSR_SCAN_THREADS), 0, st, in, out, n, first, tiles, p, scratch, state, mats);
    } else {
        const long long chunks = (npar + LFSR_WALK - 1) / LFSR_WALK, blocks = (chunks + LFSR_THREADS - 1) / LFSR_THREADS;
        if (blocks > 0x7fffffffLL) return fail(GRHIP_EINVAL, "scrambler: grid too large");
        const dim3 grid((unsigned)blocks, (unsigned)nstreams);
        if (kind == LFSR_DESCRAMBLE) {
            hipLaunchKernelGGL(descramble_kernel, grid, dim3(LFSR_THREADS), 0, st, in, out, n, first, p, (const LfsrState *)state);
            hipLaunchKernelGGL(descramble_state_kernel, per_stream, dim3(64), 0, st, in, n, nstreams, p, state);
        } else {
            hipLaunchKernelGGL(additive_kernel, grid, dim3(LFSR_THREADS), 0, st, in, out, n, first, p, (const LfsrState *)state,
                               mats + 32 * LFSR_MAT_POW);
            hipLaunchKernelGGL(additive_state_kernel, per_stream, dim3(64), 0, st, n, nstreams, p, state, mats + 32 * LFSR_MAT_POW);
        }
    }
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
