// modulator_plan.h -- the data-independent bookkeeping of gr_packed_to_unpacked_bb, gr_unpacked_to_packed_bb,
// gr_diff_encoder_bb and generic_mod as plain host arithmetic: what one general_work needs, produces, consumes and
// carries, how a stream is cut into scan tiles, and for generic_mod the bits carried, the symbols and outputs of a call
// and the symbols of an output tile.  Used by csrc/capi_modulator.hip, whose handles keep only state and locking, by the
// kernels for the few functions marked for the device, and by host/modulator_plan_test.cc, which runs the closed forms
// against the reference's loops on a CPU.  Includes no HIP header.  Not part of the ABI.
#pragma once
#include <algorithm>
#include <cstdint>
#include <limits>

#include "sched_plan.h"

namespace grhip {

// ---- gr_packed_to_unpacked_bb / gr_unpacked_to_packed_bb (gengen/gr_packed_to_unpacked_XX.cc.t:58-137,
// gr_unpacked_to_packed_XX.cc.t:56-129) ----------------------------------------------------------------------------------
//
// The reference walks an unsigned bit address from d_index.  packed_to_unpacked: output chunk i is the k bits from
// address d_index + i*k of the bytes; d_index is below 8.  unpacked_to_packed: output byte i is the 8 bits from
// address d_index + i*8 of the chunks' k low bits laid end to end; d_index is below k.  Either way the address is
// a 32-bit unsigned in the reference and wraps at 2^32, so a call whose last address would pass it is refused here.

constexpr int PACK_BITS = 8;                            // BITS_PER_TYPE of the bb expansion
constexpr uint64_t PACK_MAX_ADDR = 0xffffffffull;       // the reference's index_tmp is an unsigned int

struct PackPlan {
    bool ok = false;            // false: the addresses pass 2^32 (nothing else is set)
    long long needed = 0;       // forecast: input items the call reads
    long long consumed = 0;     // consume_each
    unsigned index_after = 0;   // d_index left for the next call
};

inline bool pack_k_ok(unsigned k) { return k >= 1 && k <= (unsigned)PACK_BITS; }

// packed_to_unpacked: noutput chunks of k bits from bit address `index` (< 8)
inline PackPlan p2u_plan(unsigned index, long long noutput, unsigned k)
{
    PackPlan p;
    if (noutput < 0 || !pack_k_ok(k) || index >= (unsigned)PACK_BITS) return p;
    const uint64_t end = (uint64_t)index + (uint64_t)noutput * k;         // noutput < 2^63 / 8 for every int
    if (end > PACK_MAX_ADDR) return p;
    p.ok = true;
    p.needed = (long long)((end + PACK_BITS - 1) / PACK_BITS);            // .cc.t:62, the ceil of a double quotient
    p.consumed = (long long)(end / PACK_BITS);                            // .cc.t:133
    p.index_after = (unsigned)(end % PACK_BITS);                          // .cc.t:134
    return p;
}

// unpacked_to_packed: noutput bytes from bit address `index` (< k) of chunks of k bits
inline PackPlan u2p_plan(unsigned index, long long noutput, unsigned k)
{
    PackPlan p;
    if (noutput < 0 || !pack_k_ok(k) || index >= k) return p;
    const uint64_t end = (uint64_t)index + (uint64_t)noutput * PACK_BITS;
    if (end > PACK_MAX_ADDR) return p;
    p.ok = true;
    p.needed = (long long)((end + k - 1) / k);                            // .cc.t:59
    p.consumed = (long long)(end / k);                                    // .cc.t:125
    p.index_after = (unsigned)(end % k);                                  // .cc.t:126
    return p;
}

// ---- gr_diff_encoder_bb (general/gr_diff_encoder_bb.cc:44-62) ------------------------------------------------------------
//
// out[i] = (in[i] + last_out) % modulus in unsigned, stored as a byte and read back from it.  Which arithmetic the
// stored bytes follow depends on the modulus alone:
//   modulus <= 256     every result is below 256, the byte store changes nothing: a prefix sum modulo `modulus`
//   modulus  > 510     in + last_out <= 510 is never reduced; the byte store is the only reduction: a prefix sum
//                      modulo 256
//   257 .. 510         the % and the byte store both act: a result in [256, modulus) loses 256 in the store, which no
//                      sum modulo anything sees (m = 300: 255, 255, 50, 0, 252 gives 255, 210, 4, 4, 0 serially, and
//                      812 % 300 % 256 = 212 from the sum), so these moduli walk serially
// diff_scan_modulus: the modulus of the scan, or 0 for the serial walk.
inline unsigned diff_scan_modulus(unsigned modulus)
{
    if (modulus == 0) return 0;
    if (modulus <= 256) return modulus;
    return modulus > 510 ? 256u : 0u;
}

// the scan's tiles: DIFF_TILE consecutive items of one stream; tile t of stream s keeps its sum, and later its
// carry (the encoder's last_out in front of the tile's first item), at s * tiles + t
constexpr int DIFF_THREADS = 256;
constexpr int DIFF_PER_LANE = 8;
constexpr int DIFF_TILE = DIFF_THREADS * DIFF_PER_LANE;

// (constexpr: the kernels call them too)
constexpr long long diff_tiles(long long n) { return n <= 0 ? 0 : (n + DIFF_TILE - 1) / DIFF_TILE; }
constexpr long long diff_carry_slot(long long stream, long long tiles, long long tile) { return stream * tiles + tile; }

// ---- generic_mod (gr-digital/python/generic_mod_demod.py:114-150) -----------------------------------------------------------
//
// The handle takes new bytes only.  Between calls it carries, for all streams alike, the `pending` unread bits of the
// last byte (fewer than k, so they lie in that one byte) and the resampler's place in its schedule, and per stream the
// last byte, the encoder's last_out and the last tpf symbols.  A call's bits are the pending ones and the new bytes';
// with the carried byte in front of the new ones, symbol i of the call starts at bit address base + i*k, base =
// 8 - pending (8: the carried byte is not read).

constexpr unsigned MOD_NFILTS = 32;                     // :132
constexpr int MOD_MIN_SPS = 2;                          // :114
// the resampler keeps both tap banks in LDS: MOD_NFILTS * ((11 * int(sps)) | 1) <= ARB_MAX_TAP_PAIRS (arb_resampler.h)
// ends at 11 * int(sps) <= 127
constexpr int MOD_MAX_INT_SPS = 11;

inline int mod_ntaps(double sps) { return (int)MOD_NFILTS * 11 * (int)sps; }             // :133

struct ModCall {
    long long nsym = 0;             // symbols the call completes
    unsigned base = 8;              // bit address of the first one's first bit, the carried byte being byte 0
    unsigned pending_after = 0;
};

inline ModCall mod_call(unsigned pending, long long n_bytes, unsigned k)
{
    ModCall c;
    const long long bits = (long long)pending + 8 * n_bytes;
    c.nsym = bits / k;
    c.pending_after = (unsigned)(bits % k);
    c.base = 8u - pending;
    return c;
}

// The outputs of a call that brings nsym symbols: those whose count lies below the symbols that have arrived (the rule
// of pfb_arb_resampler's run_captures_device), from state s whose count is relative to the call's first symbol.
inline ArbPlan mod_outputs(const ArbState &s, const ArbRate &r, long long nsym)
{
    return arb_plan(s, r, nsym, std::numeric_limits<long long>::max() / 4);
}

// the state in front of the next call: the count again relative to its first symbol (the overshoot, never negative)
inline ArbState mod_next_state(const ArbPlan &p, long long nsym)
{
    ArbState s = p.end;
    s.count = std::max(0LL, p.end.count - nsym);
    return s;
}

// Engine 1 cuts a call's outputs into tiles of `tile`.  Output k reads the tpf symbols in front of symbol count_k, so
// tile t's span starts at symbol count(t * tile) - tpf of the call; what lies before the call's first symbol is
// history.  The carry pre-pass sums the call's symbols in segments [first(t), first(t + 1)), first(ntiles) = nsym:
// they tile [0, nsym) in order, so an exclusive scan over t, seeded with last_out, is the encoder's state in front
// of every tile's first new symbol.
GRHIP_HOST_DEVICE inline long long mod_tile_count(const ArbSched &sc, unsigned R, long long k0)
{
    const unsigned long long Tb = sc.A0 + (unsigned long long)k0 * sc.F;
    const unsigned long long pb = sc.j0 + (unsigned long long)k0 * sc.D + (Tb >> 23);
    return sc.c0 + (long long)(pb / R);
}

GRHIP_HOST_DEVICE inline long long mod_tile_first_symbol(const ArbSched &sc, unsigned R, int tpf, int tile, long long t,
                                                         long long ntiles, long long nsym)
{
    if (t >= ntiles) return nsym;
    const long long a = mod_tile_count(sc, R, t * tile) - tpf;
    return a < 0 ? 0 : (a > nsym ? nsym : a);
}

}  // namespace grhip
