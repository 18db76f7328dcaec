// packet.h -- launchers of csrc/packet.hip (CRC-32, make_packet and unmake_packet in batches) and csrc/lfsr_blocks.hip
// (the three scramblers).  Used by csrc/capi_packet.hip and csrc/capi_lfsr.hip.  Not part of the ABI.
#pragma once
#include "gf2.h"
#include "grhip_internal.h"

namespace grhip {

// ---- CRC-32 ---------------------------------------------------------------------------------------------------------
// A lane takes CRC_LANE_BYTES in a row, a workgroup CRC_PASS_BYTES per pass and `passes_per_wg` passes in a row.  What
// is left in front of the first 16-byte boundary and behind the last whole pass goes to the finishing workgroup,
// which also folds the partial CRCs and the start value.
constexpr int CRC_THREADS = 256;
constexpr int CRC_LANE_BYTES = 64;
constexpr int CRC_PASS_BYTES = CRC_THREADS * CRC_LANE_BYTES;

struct CrcSplit {
    long long head, passes, passes_per_wg, groups, tail;        // bytes, passes, passes, workgroups, bytes
};
// passes_per_wg: the handle's knob, or 0 for one that fills the device
inline CrcSplit crc_split(const void *buf, long long len, long long passes_per_wg, int cus)
{
    CrcSplit s{0, 0, 1, 0, len};
    const long long head = (long long)((16 - ((uintptr_t)buf & 15)) & 15);
    if (len < head + CRC_PASS_BYTES) return s;
    s.head = head;
    s.passes = (len - head) / CRC_PASS_BYTES;
    s.tail = len - head - s.passes * CRC_PASS_BYTES;
    const long long want = (long long)cus * 8;
    s.passes_per_wg = passes_per_wg > 0 ? passes_per_wg : (s.passes + want - 1) / want;
    s.groups = (s.passes + s.passes_per_wg - 1) / s.passes_per_wg;
    return s;
}
// *d_crc = update(crc_in, buf, len) ^ final_xor; partial: room for split.groups words
int crc32_launch(const unsigned char *buf, long long len, const CrcSplit &split, unsigned crc_in, unsigned final_xor, unsigned *partial,
                 unsigned *d_crc, hipStream_t st);

// ---- packets --------------------------------------------------------------------------------------------------------
struct PacketFormat {
    unsigned char access[8];
    int access_bytes;
    unsigned byte_modulus;      // of the padding; 0: none
    int whitening;
};
int packet_make_launch(int n, const PacketJob *jobs, const unsigned char *payloads, unsigned char *out, const PacketFormat &f,
                       const unsigned char *mask, hipStream_t st);
int packet_check_launch(int n_streams, int max_msgs, const PacketJob *recs, long long rec_stride, const unsigned *counts,
                        int count_stride_words, const unsigned char *pool, long long pool_stride, int dewhitening,
                        unsigned char *payload_out, unsigned char *ok, const unsigned char *mask, hipStream_t st);

// ---- scramblers -----------------------------------------------------------------------------------------------------
enum LfsrKind { LFSR_SCRAMBLE = 0, LFSR_DESCRAMBLE = 1, LFSR_ADDITIVE = 2 };
struct LfsrState { unsigned reg, bits; };                       // d_shift_register and d_bits of one stream
struct LfsrParams { unsigned mask, seed, len, count; };

constexpr int LFSR_THREADS = 256;
constexpr int LFSR_WALK = 16;                                   // items a lane of the descrambler / additive kernels walks
constexpr int LFSR_SCAN_THREADS = 128;                          // the scrambler's scan: lanes of a tile,
constexpr int LFSR_CHUNK = 32;                                  // items a lane walks (their input bits fill a word)
constexpr int LFSR_TILE = LFSR_SCAN_THREADS * LFSR_CHUNK;
constexpr int LFSR_HEAD = 32;                                   // a seed's bits above reg_len are gone after 31 steps
// the matrices a handle keeps on the device, 32 words each: M^(2^j) j = 0 .. 30, M^(LFSR_CHUNK 2^j) j = 0 .. 7, M^LFSR_TILE
constexpr int LFSR_MAT_POW = 0, LFSR_MAT_SCAN = 31, LFSR_MAT_TILE = 39, LFSR_MATS = 40;
inline long long lfsr_tiles(long long n) { return n <= 0 ? 0 : (n + LFSR_TILE - 1) / LFSR_TILE; }

// items [first, first + cnt) of every stream by the reference's statements, one lane per stream
int lfsr_serial_launch(int kind, const unsigned char *in, unsigned char *out, long long n, long long first, long long cnt, int nstreams,
                       const LfsrParams &p, LfsrState *state, hipStream_t st);
// items [first, n) of every stream in parallel; the scrambler needs clean registers (no bit above reg_len) and
// scratch of nstreams * lfsr_tiles(n - first) words
int lfsr_parallel_launch(int kind, const unsigned char *in, unsigned char *out, long long n, long long first, int nstreams,
                         const LfsrParams &p, LfsrState *state, const unsigned *mats, unsigned *scratch, hipStream_t st);

}  // namespace grhip
