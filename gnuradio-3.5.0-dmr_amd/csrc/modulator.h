// modulator.h -- launchers of the modulator's byte and symbol kernels (csrc/modulator.hip): gr_packed_to_unpacked_bb,
// gr_unpacked_to_packed_bb, gr_diff_encoder_bb and gr_chunks_to_symbols_bc.  Used by csrc/capi_modulator.hip.  Not
// part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "modulator_plan.h"

namespace grhip {

// the table of chunks_to_symbols_bc sits in LDS up to this many entries (32 KB); a longer one is read from memory
constexpr int C2S_LDS_ENTRIES = 4096;
constexpr int C2S_MAX_ENTRIES = 65536;

// S streams back to back on both sides: in [S][ninput], out [S][noutput]; `index` is the bit address of the first
// output's first bit within in[0] (packed_to_unpacked: below 8) or within the chunks' k-bit fields (unpacked_to_packed:
// below k).  The caller has checked that the ninput items cover what the outputs read (modulator_plan.h).
int packed_to_unpacked_launch(const unsigned char *in, long long ninput, unsigned char *out, long long noutput, int nstreams,
                              unsigned k, bool lsb_first, unsigned index, hipStream_t st);
int unpacked_to_packed_launch(const unsigned char *in, long long ninput, unsigned char *out, long long noutput, int nstreams,
                              unsigned k, bool lsb_first, unsigned index, hipStream_t st);

// in and out [S][n]; last_out one unsigned per stream, read and left up to date; `scratch` holds
// nstreams * diff_tiles(n) unsigned (unused by the serial walk of moduli 257 .. 510)
int diff_encoder_launch(const unsigned char *in, unsigned char *out, long long n, int nstreams, unsigned modulus,
                        unsigned *last_out, unsigned *scratch, hipStream_t st);

// pass 2 of the encoder's scan on its own: sums[s * tiles + t] (each below m) become the exclusive running sums modulo m
// seeded with last_out[s], which is left as the total
int diff_carry_launch(unsigned *sums, long long tiles, unsigned m, unsigned *last_out, int nstreams, hipStream_t st);

// n input bytes per stream at in + s * in_stride, n * D items out at out + s * out_stride (the block keeps no state, so
// streams that lie back to back may also run as one)
int chunks_to_symbols_launch(const unsigned char *in, long long in_stride, float2 *out, long long out_stride, long long n, int nstreams,
                             const float2 *table, unsigned table_size, unsigned D, hipStream_t st);

// ---- generic_mod, engine 1 (csrc/modulator_fused.hip) -----------------------------------------------------------------------
constexpr int MOD_THREADS_FUSED = 256;
constexpr int MOD_MAX_TILE = 1024;
constexpr int MOD_SPAN_ITEMS = 2048;        // LDS items reserved at most for a tile's symbols (16 KB); sps >= 2 needs 566

// One call of the fused modulator (modulator_plan.h has the indexing).  Bytes in, samples out; what the call reads of
// earlier ones is carry_byte, last_out and hist, all left up to date for the next call.
struct ModLaunch {
    const unsigned char *in = nullptr;      // [S][n_bytes]
    long long n_bytes = 0, nsym = 0;
    unsigned base = 8, k = 1;               // ModCall
    unsigned char *carry_byte = nullptr;    // [S] the last byte of the call before
    const unsigned char *map = nullptr;     // 256 bytes, or null: no map_bb
    bool differential = false;
    unsigned mask = 0;                      // 2^k - 1
    unsigned *last_out = nullptr;           // [S]
    unsigned *carries = nullptr;            // [S][ntiles] scratch of the carry pre-pass
    const float2 *points = nullptr;
    unsigned npoints = 0;                   // at most 256
    float2 *hist = nullptr;                 // [S][tpf] the last tpf symbols (zeros in front of the stream's start)
    float2 *out = nullptr;
    long long out_stride = 0, nout = 0, ntiles = 0;
    int n_streams = 1;
    const float2 *taps = nullptr;           // [R][S] (h, dh) pairs as arb_kernel reads them
    int R = 1, tpf = 1, S = 1, tile = 1, span_cap = 0;
    ArbSched sc;
};

// generic: gr_fir_ccf_generic's order and the unfused o0 + o1 * acc, bit for bit arb_kernel's GENERIC; else the blended
// tap and FMAs.  Launches the carry pre-pass (differential only), the fused kernel and the state update.
int modulator_fused_launch(bool generic, const ModLaunch &a, hipStream_t st);

// engine 0's glue: staged[s] = carry_byte[s], in[s][0 .. n_bytes); then carry_byte[s] = in[s][n_bytes - 1]
int mod_stage_bytes_launch(const unsigned char *in, long long n_bytes, int nstreams, unsigned char *carry_byte, unsigned char *staged,
                           hipStream_t st);
// engine 0's glue: dst[s][0 .. n) = src[s][0 .. n) with strides (history into the symbol buffer and back)
int mod_copy_items_launch(const float2 *src, long long src_stride, float2 *dst, long long dst_stride, int n, int nstreams, hipStream_t st);

}  // namespace grhip
