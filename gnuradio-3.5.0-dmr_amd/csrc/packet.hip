// packet.hip -- the packet layer's kernels: digital_update_crc32 (gr-digital/lib/digital_crc32.cc:45-134) over a device
// buffer, make_packet (gr-digital/python/packet_utils.py:104-149) for a batch of payloads and unmake_packet (:175-194,
// crc.py:30-38) for a batch of framed messages.
//
// The CRC is linear over GF(2): the raw CRC (start value 0) of a run of bytes, multiplied by x^(8 * bytes behind it)
// modulo the generator, is what the run contributes to the CRC of the whole, and the start value enters as
// start * x^(8 * len).  So every lane takes bytes of its own and the contributions are XORed (csrc/gf2.h).
#include "packet.h"

namespace grhip {

namespace {

struct Xpow8Arg { unsigned p[32]; };        // x^(8 2^j) mod P by value: wave-uniform kernel arguments

// the 256-entry table of digital_crc32.cc:48-113 into LDS, by 256 lanes or by 64
__device__ __forceinline__ void fill_crc_table(unsigned *T, int tid, int nthreads)
{
    for (int i = tid; i < 256; i += nthreads) T[i] = crc32_byte(0u, (unsigned char)i);
    __syncthreads();
}

// four bytes in memory order (digital_crc32.cc:117, four times)
__device__ __forceinline__ unsigned crc_word(unsigned crc, unsigned w, const unsigned *T)
{
    crc ^= __builtin_bswap32(w);
    crc = (crc << 8) ^ T[crc >> 24];
    crc = (crc << 8) ^ T[crc >> 24];
    crc = (crc << 8) ^ T[crc >> 24];
    crc = (crc << 8) ^ T[crc >> 24];
    return crc;
}
__device__ __forceinline__ unsigned crc_step(unsigned crc, unsigned byte, const unsigned *T)
{
    return (crc << 8) ^ T[(crc >> 24) ^ byte];
}

__device__ __forceinline__ unsigned wave_xor(unsigned v)
{
    for (int off = 32; off > 0; off >>= 1) v ^= (unsigned)__shfl_xor((int)v, off, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_or(unsigned v)
{
    for (int off = 32; off > 0; off >>= 1) v |= (unsigned)__shfl_xor((int)v, off, 64);
    return v;
}

// XOR over the workgroup's 256 lanes, valid in thread 0
__device__ __forceinline__ unsigned block_xor(unsigned v, unsigned *red, int tid)
{
    v = wave_xor(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] ^ red[1] ^ red[2] ^ red[3];
}

// ---- the body: whole passes of 16-byte aligned data -----------------------------------------------------------------
__global__ void __launch_bounds__(CRC_THREADS)
crc_body_kernel(const uint4 *__restrict__ body, long long passes, long long passes_per_wg, Xpow8Arg xp, unsigned *__restrict__ partial)
{
    __shared__ unsigned T[256];
    __shared__ unsigned red[4];
    const int tid = threadIdx.x;
    fill_crc_table(T, tid, CRC_THREADS);
    const long long p0 = (long long)blockIdx.x * passes_per_wg;
    const long long np = passes - p0 < passes_per_wg ? passes - p0 : passes_per_wg;
    const unsigned xpass = xpow8_from(xp.p, (unsigned long long)CRC_PASS_BYTES);
    constexpr int Q = CRC_LANE_BYTES / 16;
    const uint4 *src = body + p0 * (CRC_PASS_BYTES / 16) + tid * Q;
    unsigned acc = 0;
    for (long long p = 0; p < np; ++p, src += CRC_PASS_BYTES / 16) {
        uint4 q[Q];
#pragma unroll
        for (int k = 0; k < Q; ++k) q[k] = src[k];
        unsigned c = 0;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            c = crc_word(c, q[k].x, T);
            c = crc_word(c, q[k].y, T);
            c = crc_word(c, q[k].z, T);
            c = crc_word(c, q[k].w, T);
        }
        acc = (p ? gf2_mulmod(acc, xpass) : 0u) ^ c;            // the lane's earlier runs lie one pass further in front
    }
    // behind the lane's last run, inside this workgroup's bytes: the runs of the lanes after it
    const unsigned v = gf2_mulmod(acc, xpow8_from(xp.p, (unsigned long long)CRC_LANE_BYTES * (unsigned)(CRC_THREADS - 1 - tid)));
    const unsigned r = block_xor(v, red, tid);
    if (tid == 0) partial[blockIdx.x] = r;
}

// ---- the finish: loose bytes, the partial CRCs, the start value -----------------------------------------------------
__global__ void __launch_bounds__(CRC_THREADS)
crc_finish_kernel(const unsigned char *__restrict__ buf, long long len, long long head, long long tail, long long passes,
                  long long passes_per_wg, long long groups, const unsigned *__restrict__ partial, unsigned crc_in, unsigned final_xor,
                  Xpow8Arg xp, unsigned *__restrict__ d_crc)
{
    __shared__ unsigned T[256];
    __shared__ unsigned red[4];
    const int tid = threadIdx.x;
    fill_crc_table(T, tid, CRC_THREADS);
    unsigned v = 0;
    // the bytes behind the last whole pass, CRC_LANE_BYTES per lane and turn
    const long long t0 = len - tail;
    for (long long a = (long long)tid * CRC_LANE_BYTES; a < tail; a += (long long)CRC_THREADS * CRC_LANE_BYTES) {
        const long long e = a + CRC_LANE_BYTES < tail ? a + CRC_LANE_BYTES : tail;
        unsigned c = 0;
        for (long long k = a; k < e; ++k) c = crc_step(c, buf[t0 + k], T);
        v ^= gf2_mulmod(c, xpow8_from(xp.p, (unsigned long long)(tail - e)));
    }
    // the partial CRC of workgroup g: behind it the passes of the workgroups after it and the tail
    for (long long g = tid; g < groups; g += CRC_THREADS) {
        const long long done = (g + 1) * passes_per_wg < passes ? (g + 1) * passes_per_wg : passes;
        v ^= gf2_mulmod(partial[g], xpow8_from(xp.p, (unsigned long long)((passes - done) * CRC_PASS_BYTES + tail)));
    }
    if (tid == CRC_THREADS - 1) {
        unsigned c = 0;                                         // up to 15 bytes in front of the first 16-byte boundary
        for (long long k = 0; k < head; ++k) c = crc_step(c, buf[k], T);
        v ^= gf2_mulmod(c, xpow8_from(xp.p, (unsigned long long)(len - head)));
        v ^= gf2_mulmod(crc_in, xpow8_from(xp.p, (unsigned long long)len));
    }
    const unsigned r = block_xor(v, red, tid);
    if (tid == 0) *d_crc = r ^ final_xor;
}

// ---- one wavefront, one message -------------------------------------------------------------------------------------
// digital_crc32 of `len` bytes that get(k) hands out: lane l takes bytes [l * run, (l + 1) * run)
template <class Get>
__device__ __forceinline__ unsigned wave_crc32(Get &&get, unsigned len, unsigned lane, const unsigned *T, const Xpow8Arg &xp)
{
    const unsigned run = (len + 63u) / 64u;
    const unsigned a = lane * run < len ? lane * run : len, e = a + run < len ? a + run : len;
    unsigned c = 0;
    for (unsigned k = a; k < e; ++k) c = crc_step(c, get(k), T);
    unsigned v = gf2_mulmod(c, xpow8_from(xp.p, len - e));
    if (lane == 0) v ^= gf2_mulmod(0xffffffffu, xpow8_from(xp.p, len));
    return wave_xor(v) ^ 0xffffffffu;
}

constexpr int PKT_WAVES = 4;        // packets per workgroup

__global__ void __launch_bounds__(64 * PKT_WAVES)
packet_make_kernel(int n, const PacketJob *__restrict__ jobs, const unsigned char *__restrict__ payloads, unsigned char *__restrict__ out,
                   PacketFormat f, const unsigned char *__restrict__ mask, Xpow8Arg xp)
{
    __shared__ unsigned T[256];
    fill_crc_table(T, threadIdx.x, 64 * PKT_WAVES);
    const unsigned lane = threadIdx.x & 63u;
    const long long i = (long long)blockIdx.x * PKT_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const PacketJob jb = jobs[i];
    const unsigned char *src = payloads + jb.in_offset;
    unsigned char *dst = out + jb.out_offset;
    const unsigned len = jb.length, o = jb.whitener_offset, L = len + 4u;
    // the records come from device memory: one that plan() would have refused would read past the mask, and is skipped
    if (len > (unsigned)WHITEN_LEN - 4u || (unsigned long long)L + o > (unsigned long long)WHITEN_LEN) return;
    const unsigned crc = wave_crc32([&](unsigned k) -> unsigned { return src[k]; }, len, lane, T, xp);   // crc.py:26-28
    const unsigned hdr = ((o & 0xfu) << 12) | (L & 0x0fffu);                    // make_header, packet_utils.py:98-102
    const unsigned at_access = 2u, at_hdr = at_access + (unsigned)f.access_bytes, at_pay = at_hdr + 4u, at_crc = at_pay + len,
                   at_end = at_crc + 4u;
    unsigned total = at_end + 1u;                                               // one 0x55 (:139-143)
    if (f.byte_modulus) total += (f.byte_modulus - total % f.byte_modulus) % f.byte_modulus;   // _npadding_bytes, :151-172
    for (unsigned j = lane; j < total; j += 64u) {
        unsigned b;
        if (j < at_access) b = j ? 0xF2u : 0xA4u;                               // the preamble, :74-75
        else if (j < at_hdr) b = f.access[j - at_access];
        else if (j < at_pay) b = (hdr >> (((j - at_hdr) & 1u) ? 0 : 8)) & 0xffu;   // '!HH' of (val, val)
        else if (j < at_end) {
            const unsigned k = j - at_pay;
            b = j < at_crc ? src[k] : (crc >> (8u * (3u - (j - at_crc)))) & 0xffu;   // struct.pack(">I", crc)
            if (f.whitening) b ^= mask[o + k];                                  // whiten, :89-92
        } else b = 0x55u;
        dst[j] = (unsigned char)b;
    }
}

// src and dst may be the same buffer: a lane reads the bytes it writes, and nothing else
__global__ void __launch_bounds__(64 * PKT_WAVES)
packet_check_kernel(int n_streams, int max_msgs, const PacketJob *__restrict__ recs, long long rec_stride, const unsigned *__restrict__ counts,
                    int count_stride_words, const unsigned char *pool, long long pool_stride, int dewhitening, unsigned char *payload_out,
                    unsigned char *__restrict__ ok, const unsigned char *__restrict__ mask, Xpow8Arg xp)
{
    __shared__ unsigned T[256];
    fill_crc_table(T, threadIdx.x, 64 * PKT_WAVES);
    const unsigned lane = threadIdx.x & 63u;
    const long long i = (long long)blockIdx.x * PKT_WAVES + (threadIdx.x >> 6);
    if (i >= (long long)n_streams * max_msgs) return;
    const long long s = i / max_msgs, m = i % max_msgs;
    unsigned good = 0;
    const long long have = counts ? (long long)counts[s * count_stride_words] : (long long)max_msgs;
    if (m < have) {
        const PacketJob r = recs[s * rec_stride + m];
        const unsigned len = r.length, o = r.whitener_offset;
        // crc.py:31-32: shorter than a CRC is (False, ''); past the mask's end the reference raises
        if (len >= 4u && (unsigned long long)len + o <= (unsigned long long)WHITEN_LEN) {
            const unsigned char *src = pool + s * pool_stride + r.in_offset;
            unsigned char *dst = payload_out + s * pool_stride + r.in_offset;
            const unsigned body = len - 4u;
            unsigned expected = 0;
            const unsigned run = (len + 63u) / 64u;
            const unsigned a = lane * run < len ? lane * run : len, e = a + run < len ? a + run : len;
            unsigned c = 0, behind = 0;
            for (unsigned k = a; k < e; ++k) {
                unsigned b = src[k];
                if (dewhitening) b ^= mask[o + k];                              // dewhiten, :94-95
                dst[k] = (unsigned char)b;
                if (k < body) { c = crc_step(c, b, T); behind = body - 1u - k; }
                else expected |= b << (8u * (len - 1u - k));                    // struct.unpack(">I", s[-4:])
            }
            unsigned v = gf2_mulmod(c, xpow8_from(xp.p, behind));
            if (lane == 0) v ^= gf2_mulmod(0xffffffffu, xpow8_from(xp.p, body));
            const unsigned actual = wave_xor(v) ^ 0xffffffffu;
            good = actual == wave_or(expected) ? 1u : 0u;
        }
    }
    if (lane == 0) ok[i] = (unsigned char)good;
}

Xpow8Arg xpow8_arg()
{
    static const Xpow8Table t;
    Xpow8Arg a;
    for (int j = 0; j < 32; ++j) a.p[j] = t.p[j];
    return a;
}

}  // namespace

int crc32_launch(const unsigned char *buf, long long len, const CrcSplit &s, unsigned crc_in, unsigned final_xor, unsigned *partial,
                 unsigned *d_crc, hipStream_t st)
{
    if (s.groups > 0x7fffffffLL) return fail(GRHIP_EINVAL, "crc32: grid too large");
    const Xpow8Arg xp = xpow8_arg();
    if (s.groups > 0)
        hipLaunchKernelGGL(crc_body_kernel, dim3((unsigned)s.groups), dim3(CRC_THREADS), 0, st, (const uint4 *)(buf + s.head), s.passes,
                           s.passes_per_wg, xp, partial);
    hipLaunchKernelGGL(crc_finish_kernel, dim3(1), dim3(CRC_THREADS), 0, st, buf, len, s.head, s.tail, s.passes, s.passes_per_wg, s.groups,
                       (const unsigned *)partial, crc_in, final_xor, xp, d_crc);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int packet_make_launch(int n, const PacketJob *jobs, const unsigned char *payloads, unsigned char *out, const PacketFormat &f,
                       const unsigned char *mask, hipStream_t st)
{
    if (n <= 0) return GRHIP_OK;
    hipLaunchKernelGGL(packet_make_kernel, dim3((unsigned)((n + PKT_WAVES - 1) / PKT_WAVES)), dim3(64 * PKT_WAVES), 0, st, n, jobs, payloads,
                       out, f, mask, xpow8_arg());
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

int packet_check_launch(int n_streams, int max_msgs, const PacketJob *recs, long long rec_stride, const unsigned *counts,
                        int count_stride_words, const unsigned char *pool, long long pool_stride, int dewhitening,
                        unsigned char *payload_out, unsigned char *ok, const unsigned char *mask, hipStream_t st)
{
    const long long total = (long long)n_streams * max_msgs;
    if (total <= 0) return GRHIP_OK;
    if ((total + PKT_WAVES - 1) / PKT_WAVES > 0x7fffffffLL) return fail(GRHIP_EINVAL, "packet_check: grid too large");
    hipLaunchKernelGGL(packet_check_kernel, dim3((unsigned)((total + PKT_WAVES - 1) / PKT_WAVES)), dim3(64 * PKT_WAVES), 0, st, n_streams,
                       max_msgs, recs, rec_stride, counts, count_stride_words, pool, pool_stride, dewhitening, payload_out, ok, mask,
                       xpow8_arg());
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace grhip
