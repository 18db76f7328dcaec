// gf2.h -- the arithmetic over GF(2) behind the CRC-32, the whitening table and the scramblers: polynomials modulo the
// CRC's generator, 32 x 32 bit matrices, the one-step matrix of gri_lfsr and the packet layer's closed forms.  Plain
// C++ without HIP, so host/gf2_test.cc can run it under the sanitizers; what a kernel needs too is GF2_HD.  Not part
// of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define GF2_HD __host__ __device__ inline
#else
#define GF2_HD inline
#endif

namespace grhip {

// ---- polynomials modulo P = 0x104C11DB7, bit 31 the coefficient of x^31 (MSB first, no reflection) ------------------
constexpr uint32_t CRC32_POLY = 0x04C11DB7u;        // gr-digital/lib/digital_crc32.cc:44

GF2_HD uint32_t gf2_mulmod(uint32_t a, uint32_t b)              // a * b mod P
{
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) {
        r = (r << 1) ^ ((r >> 31) ? CRC32_POLY : 0u);           // r * x
        r ^= ((b >> (31 - i)) & 1u) ? a : 0u;
    }
    return r;
}

// one byte into a raw CRC (digital_crc32.cc:117 without the table): crc * x^8 + byte * x^32, mod P
GF2_HD uint32_t crc32_byte(uint32_t crc, unsigned char byte)
{
    crc ^= (uint32_t)byte << 24;
    for (int i = 0; i < 8; ++i) crc = (crc << 1) ^ ((crc >> 31) ? CRC32_POLY : 0u);
    return crc;
}

inline uint32_t crc32_update_serial(uint32_t crc, const unsigned char *p, size_t n)     // digital_update_crc32
{
    for (size_t i = 0; i < n; ++i) crc = crc32_byte(crc, p[i]);
    return crc;
}

inline void crc32_table(uint32_t t[256])                        // the table of digital_crc32.cc:48-113
{
    for (int i = 0; i < 256; ++i) t[i] = crc32_byte(0u, (unsigned char)i);
}

// x^(8 * 2^j) mod P, j = 0 .. 31
struct Xpow8Table {
    uint32_t p[32];
    Xpow8Table()
    {
        p[0] = 0x100u;                                          // x^8
        for (int j = 1; j < 32; ++j) p[j] = gf2_mulmod(p[j - 1], p[j - 1]);
    }
};

GF2_HD uint32_t xpow8_from(const uint32_t *table, uint64_t n)   // x^(8 n) mod P, n < 2^32
{
    uint32_t r = 1u;
    for (int j = 0; j < 32 && (n >> j); ++j)
        if ((n >> j) & 1u) r = gf2_mulmod(r, table[j]);
    return r;
}

inline uint32_t xpow8(uint64_t n)
{
    static const Xpow8Table t;
    return xpow8_from(t.p, n);
}

// raw CRC (start value 0) of A followed by B from those of A and of B: A's is shifted past B's lenB bytes
inline uint32_t crc_combine(uint32_t crcA_raw, uint32_t crcB_raw, uint64_t lenB)
{
    return gf2_mulmod(crcA_raw, xpow8(lenB)) ^ crcB_raw;
}

// ---- 32 x 32 bit matrices: c[b] is column b, the image of the vector 1 << b -----------------------------------------
struct Gf2Mat { uint32_t c[32]; };

GF2_HD uint32_t gf2_matvec(const uint32_t *cols, uint32_t v)
{
    uint32_t r = 0;
    for (int b = 0; b < 32; ++b) r ^= cols[b] & (0u - ((v >> b) & 1u));
    return r;
}

inline Gf2Mat gf2_matmul(const Gf2Mat &a, const Gf2Mat &b)      // a * b: b first
{
    Gf2Mat r;
    for (int i = 0; i < 32; ++i) r.c[i] = gf2_matvec(a.c, b.c[i]);
    return r;
}

inline Gf2Mat gf2_identity()
{
    Gf2Mat r;
    for (int i = 0; i < 32; ++i) r.c[i] = 1u << i;
    return r;
}

inline Gf2Mat gf2_matpow(Gf2Mat m, uint64_t n)
{
    Gf2Mat r = gf2_identity();
    for (; n; n >>= 1) {
        if (n & 1u) r = gf2_matmul(m, r);
        m = gf2_matmul(m, m);
    }
    return r;
}

// ---- gri_lfsr (gnuradio-core/src/lib/general/gri_lfsr.h:103-132) ----------------------------------------------------
constexpr uint32_t LFSR_MAX_LEN = 31;                           // :109-110 throws above

GF2_HD uint32_t lfsr_parity(uint32_t x)                         // popCount(x) % 2, :94-99 and :115
{
    return (uint32_t)__builtin_popcount(x) & 1u;
}

// the reference's statement: the new bit is ORed in (:116, :123, :130)
GF2_HD uint32_t lfsr_step_or(uint32_t reg, uint32_t newbit, uint32_t len) { return (reg >> 1) | (newbit << len); }
GF2_HD uint32_t lfsr_next(uint32_t reg, uint32_t mask, uint32_t len) { return lfsr_step_or(reg, lfsr_parity(reg & mask), len); }

// A register with no bit above `len` never gets one, and then bit `len` of reg >> 1 is clear: the OR is an XOR and
// the step is linear.  Bits of the seed above `len` shift out within 31 steps.
GF2_HD bool lfsr_clean(uint32_t reg, uint32_t len) { return len >= 31u || (reg >> (len + 1u)) == 0u; }

// the one-step matrix of next_bit() with the XOR: reg' = (reg >> 1) ^ (parity(reg & mask) << len)
inline Gf2Mat lfsr_matrix(uint32_t mask, uint32_t len)
{
    Gf2Mat m;
    for (int b = 0; b < 32; ++b) m.c[b] = ((1u << b) >> 1) ^ (((mask >> b) & 1u) << len);
    return m;
}

// `k` steps of next_bit() from `reg`: the reference's statement while the register has bits above `len`, then
// pw[j] = M^(2^j), j = 0 .. 30.  k < 2^31.
GF2_HD uint32_t lfsr_advance(uint32_t reg, uint32_t k, uint32_t mask, uint32_t len, const uint32_t *pw)
{
    while (k && !lfsr_clean(reg, len)) { reg = lfsr_next(reg, mask, len); --k; }
    for (int j = 0; j < 31 && (k >> j); ++j)
        if ((k >> j) & 1u) reg = gf2_matvec(pw + 32 * j, reg);
    return reg;
}

// ---- the whitening table (gr-digital/python/packet_utils.py:198-454) ------------------------------------------------
// bytes 0 .. 4093 are next_bit() of gri_lfsr(0x3, 0x3FFF, 14), eight to a byte, least significant bit first; the table's
// last two bytes are 255, 63
constexpr int WHITEN_LEN = 4096;
inline void whitening_table(unsigned char t[WHITEN_LEN])
{
    uint32_t reg = 0x3FFFu;
    for (int i = 0; i < WHITEN_LEN - 2; ++i) {
        unsigned v = 0;
        for (int b = 0; b < 8; ++b) {
            v |= (reg & 1u) << b;
            reg = lfsr_next(reg, 0x3u, 14u);
        }
        t[i] = (unsigned char)v;
    }
    t[WHITEN_LEN - 2] = 255;
    t[WHITEN_LEN - 1] = 63;
}

// ---- make_packet's closed forms (packet_utils.py:104-172) -----------------------------------------------------------
struct PacketJob { uint32_t whitener_offset, length, in_offset, out_offset; };    // grhip_packet_job

inline long long gf2_gcd(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

// _npadding_bytes (:151-172) in Python 2's integer arithmetic; -1: byte_modulus is 0 and the reference divides by it
inline long long packet_byte_modulus(int sps, int bps)
{
    const long long lcm = 16 / gf2_gcd(16, sps) * sps;          // gru.lcm(128 / 8, samples_per_symbol)
    return lcm * bps / sps;
}
inline long long packet_npadding(long long pkt_byte_len, int sps, int bps)
{
    const long long byte_modulus = packet_byte_modulus(sps, bps);
    if (byte_modulus <= 0) return -1;
    const long long r = pkt_byte_len % byte_modulus;
    return r == 0 ? 0 : byte_modulus - r;
}

// bytes of one packet: preamble 2, the access code's bytes, header 4, payload + CRC, one 0x55, the padding
inline long long packet_bytes(int access_bytes, int payload_len, int sps, int bps, bool pad_for_usrp)
{
    const long long unpadded = 2 + access_bytes + 4 + (long long)payload_len + 4 + 1;
    if (!pad_for_usrp) return unpadded;
    const long long pad = packet_npadding(unpadded, sps, bps);
    return pad < 0 ? -1 : unpadded + pad;
}

// why (payload_len, whitener_offset) is refused, or null: L = len + 4 <= 4096, o >= 0, L + o <= 4096
inline const char *packet_refusal(long long payload_len, long long whitener_offset)
{
    if (payload_len < 0) return "negative payload length";
    if (payload_len + 4 > WHITEN_LEN) return "len(payload) + 4 must be in [0, 4096]";
    if (whitener_offset < 0) return "negative whitener_offset";
    if (payload_len + 4 + whitener_offset > WHITEN_LEN) return "payload + CRC + whitener_offset pass the 4096-byte mask";
    return nullptr;
}

// the job records of n packets, payloads and packets back to back; returns null or the refusal (jobs then unspecified)
inline const char *packet_plan(int n, const int *lengths, const int *whitener_offsets, int access_bytes, int sps, int bps,
                               bool pad_for_usrp, PacketJob *jobs, long long *total_in, long long *total_out)
{
    long long in = 0, out = 0;
    for (int i = 0; i < n; ++i) {
        const long long o = whitener_offsets ? whitener_offsets[i] : 0;
        if (const char *bad = packet_refusal(lengths[i], o)) return bad;
        const long long nb = packet_bytes(access_bytes, lengths[i], sps, bps, pad_for_usrp);
        if (nb < 0) return "samples_per_symbol and bits_per_symbol leave a byte modulus of 0";
        if (out + nb > 0xffffffffLL) return "more than 4 GiB of packets in one plan";
        jobs[i] = PacketJob{(uint32_t)o, (uint32_t)lengths[i], (uint32_t)in, (uint32_t)out};
        in += lengths[i];
        out += nb;
    }
    if (total_in) *total_in = in;
    if (total_out) *total_out = out;
    return nullptr;
}

// the access code: '0' / '1', 1 .. 64 characters, packed with leading zeros to whole bytes
// (conv_1_0_string_to_packed_binary_string, :40-69); returns the byte count or -1
inline int pack_access_code(const char *code, unsigned char out[8])
{
    if (!code) return -1;
    size_t n = 0;
    while (code[n]) {
        if (code[n] != '0' && code[n] != '1') return -1;
        if (++n > 64) return -1;
    }
    if (n == 0) return -1;
    const int nbytes = (int)((n + 7) / 8);
    uint64_t v = 0;
    for (size_t i = 0; i < n; ++i) v = (v << 1) | (uint64_t)(code[i] - '0');
    for (int i = 0; i < nbytes; ++i) out[i] = (unsigned char)(v >> (8 * (nbytes - 1 - i)));
    return nbytes;
}

}  // namespace grhip
