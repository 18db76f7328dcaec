// modulator_plan_test.cc -- the bookkeeping of csrc/modulator_plan.h against the reference's loops, on the CPU: what a
// call of packed_to_unpacked_bb / unpacked_to_packed_bb needs, consumes and carries against a walk of the reference's
// index arithmetic (gr_packed_to_unpacked_XX.cc.t:62, 108-134; gr_unpacked_to_packed_XX.cc.t:59, 100-126), the counts
// at the int limits that the entries accept and refuse, the scan modulus of diff_encoder_bb against its serial loop,
// and generic_mod's calls: symbols and bits carried, outputs per call against the resampler's schedule over the whole
// stream, and the segments of the carry pre-pass.  k = 1 .. 8, calls of 0, 1 and 7 bytes.  Exits non-zero with the
// first disagreeing case printed.  Links nothing of HIP.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/modulator_plan.h"

using namespace grhip;

namespace {

int fails = 0;
long long checks = 0;

#define EXPECT(cond, ...)                                                                                              \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            if (fails < 20) { printf("%s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); }   \
            ++fails;                                                                                                   \
        }                                                                                                              \
    } while (0)

// the reference's own index arithmetic for one call, walked bit by bit
void walk_p2u(unsigned index, int noutput, unsigned k, long long *needed, long long *consumed, unsigned *after)
{
    unsigned index_tmp = index;
    long long last_byte = -1;
    for (int i = 0; i < noutput; i++)
        for (unsigned j = 0; j < k; j++, index_tmp++) last_byte = index_tmp >> 3;       // get_bit_be / get_bit_le read this byte
    *needed = last_byte + 1;
    *consumed = index_tmp >> 3;                                                         // .cc.t:133
    *after = index_tmp & 7u;                                                            // :134
}

void walk_u2p(unsigned index, int noutput, unsigned k, long long *needed, long long *consumed, unsigned *after)
{
    unsigned index_tmp = index;
    long long last_item = -1;
    for (int i = 0; i < noutput; i++)
        for (unsigned j = 0; j < 8; j++, index_tmp++) last_item = (int)index_tmp / k;   // get_bit_be1 reads this item
    *needed = last_item + 1;
    *consumed = (int)(index_tmp / k);                                                   // .cc.t:125
    *after = index_tmp % k;                                                             // :126
}

void repackers()
{
    const int NOUT[] = {0, 1, 2, 7, 8, 9, 63, 64, 65, 1000};
    for (unsigned k = 1; k <= 8; ++k)
        for (int n : NOUT) {
            for (unsigned index = 0; index < 8; ++index) {
                const PackPlan p = p2u_plan(index, n, k);
                long long needed, consumed;
                unsigned after;
                walk_p2u(index, n, k, &needed, &consumed, &after);
                // forecast (.cc.t:62) is the ceil of (d_index + n*k) / 8: what the walk reads, or one byte more when a
                // call of no outputs starts inside a byte
                const long long forecast = ((long long)index + (long long)n * k + 7) / 8;
                EXPECT(p.ok && p.needed == forecast && p.needed >= needed && p.consumed == consumed && p.index_after == after,
                       "p2u k %u n %d index %u: plan (%lld, %lld, %u), walk (%lld, %lld, %u)", k, n, index, p.needed, p.consumed,
                       p.index_after, needed, consumed, after);
                EXPECT(n == 0 || p.needed == needed, "p2u k %u n %d index %u: forecast %lld, the walk reads %lld", k, n, index, p.needed, needed);
            }
            for (unsigned index = 0; index < k; ++index) {
                const PackPlan p = u2p_plan(index, n, k);
                long long needed, consumed;
                unsigned after;
                walk_u2p(index, n, k, &needed, &consumed, &after);
                const long long forecast = ((long long)index + 8LL * n + k - 1) / k;
                EXPECT(p.ok && p.needed == forecast && p.consumed == consumed && p.index_after == after,
                       "u2p k %u n %d index %u: plan (%lld, %lld, %u), walk (%lld, %u)", k, n, index, p.needed, p.consumed, p.index_after,
                       consumed, after);
                EXPECT(n == 0 || p.needed == needed, "u2p k %u n %d index %u: forecast %lld, the walk reads %lld", k, n, index, p.needed, needed);
            }
        }
    // a stream cut into calls of 1 and 7 outputs carries the same index as one call
    for (unsigned k = 1; k <= 8; ++k)
        for (int per : {1, 7}) {
            unsigned ia = 0, ib = 0;
            long long ca = 0, cb = 0;
            for (int c = 0; c < 50; ++c) {
                const PackPlan a = p2u_plan(ia, per, k), b = u2p_plan(ib, per, k);
                ia = a.index_after; ca += a.consumed;
                ib = b.index_after; cb += b.consumed;
            }
            const PackPlan a = p2u_plan(0, 50 * per, k), b = u2p_plan(0, 50 * per, k);
            EXPECT(ia == a.index_after && ca == a.consumed && ib == b.index_after && cb == b.consumed, "k %u calls of %d", k, per);
        }
    // the int limits: the reference's index is an unsigned int, so the last address may be 2^32 - 1 and no more
    for (unsigned k = 1; k <= 8; ++k) {
        const long long most = (0xffffffffLL - 7) / k;
        EXPECT(p2u_plan(7, most, k).ok && !p2u_plan(7, most + 1, k).ok, "p2u k %u: %lld outputs accepted, one more refused", k, most);
        EXPECT(p2u_plan(0, INT_MAX, k).ok == ((long long)INT_MAX * k <= 0xffffffffLL), "p2u k %u at INT_MAX", k);
        const long long most8 = (0xffffffffLL - (k - 1)) / 8;
        EXPECT(u2p_plan(k - 1, most8, k).ok && !u2p_plan(k - 1, most8 + 1, k).ok, "u2p k %u: %lld outputs accepted", k, most8);
        EXPECT(!u2p_plan(0, INT_MAX, k).ok, "u2p k %u at INT_MAX", k);
        const PackPlan p = p2u_plan(7, most, k);
        EXPECT(p.needed * 8 >= 7 + most * k && p.consumed <= p.needed && p.index_after < 8, "p2u k %u at the limit", k);
    }
    EXPECT(!p2u_plan(0, 1, 0).ok && !p2u_plan(0, 1, 9).ok && !p2u_plan(8, 1, 3).ok && !p2u_plan(0, -1, 3).ok, "p2u refusals");
    EXPECT(!u2p_plan(0, 1, 0).ok && !u2p_plan(0, 1, 9).ok && !u2p_plan(3, 1, 3).ok && !u2p_plan(0, -1, 3).ok, "u2p refusals");
}

// gr_diff_encoder_bb.cc:52-60 against the prefix sum modulo diff_scan_modulus
void encoder()
{
    std::vector<unsigned char> in(5000);
    unsigned seed = 12345;
    for (auto &b : in) { seed = seed * 1664525u + 1013904223u; b = (unsigned char)(seed >> 24); }
    for (size_t i = 0; i < 600; ++i) in[i] = 255;
    for (unsigned modulus : {1u, 2u, 3u, 4u, 7u, 8u, 200u, 255u, 256u, 257u, 300u, 510u, 511u, 512u, 1000u, 0xffffffffu}) {
        const unsigned m = diff_scan_modulus(modulus);
        unsigned last_out = 0;
        unsigned long long sum = 0;
        bool same = true;
        for (unsigned char b : in) {
            const unsigned char out = (unsigned char)((b + last_out) % modulus);
            last_out = out;
            sum += b;
            if (m && out != (unsigned char)(sum % m)) same = false;
        }
        if (modulus <= 256 || modulus > 510) EXPECT(m == (modulus <= 256 ? modulus : 256u) && same, "modulus %u: the scan modulo %u", modulus, m);
        else EXPECT(m == 0, "modulus %u must walk serially", modulus);
    }
    EXPECT(diff_scan_modulus(0) == 0, "modulus 0");
    EXPECT(diff_tiles(0) == 0 && diff_tiles(1) == 1 && diff_tiles(DIFF_TILE) == 1 && diff_tiles(DIFF_TILE + 1) == 2 &&
               diff_tiles(INT_MAX) == ((long long)INT_MAX + DIFF_TILE - 1) / DIFF_TILE,
           "diff_tiles");
    EXPECT(diff_carry_slot(2, 5, 3) == 13, "diff_carry_slot");
}

// generic_mod: a stream in calls against the stream in one piece
void modulator()
{
    const float RATES[] = {2.f, 2.5f, 3.f, 4.f, 8.f, 11.5f};
    const int CALLS[] = {0, 1, 7, 1, 0, 7, 7, 1, 100, 0, 1};
    for (unsigned k = 1; k <= 8; ++k)
        for (float sps : RATES) {
            ArbRate rp;
            EXPECT(arb_rate_params(MOD_NFILTS, sps, &rp) == nullptr, "rate %g", (double)sps);
            const int tpf = 11 * (int)sps + 1;
            EXPECT(mod_ntaps(sps) == 32 * 11 * (int)sps, "ntaps");
            unsigned pending = 0;
            ArbState st;
            long long bytes = 0, symbols = 0, outputs = 0;
            for (int n : CALLS) {
                const ModCall mc = mod_call(pending, n, k);
                EXPECT(mc.base == 8 - pending && mc.base >= 1 && mc.base <= 8 && mc.pending_after < k, "k %u: base %u", k, mc.base);
                EXPECT((long long)pending + 8LL * n == mc.nsym * k + mc.pending_after, "k %u: bits", k);
                // the last bit of the call's last symbol lies inside the carried byte and the n new ones
                EXPECT(mc.nsym == 0 || (mc.base + mc.nsym * k - 1) / 8 <= n, "k %u n %d: the last symbol's byte", k, n);
                ArbPlan p = mod_outputs(st, rp, mc.nsym);
                EXPECT(p.closed && !p.too_many && st.count == 0 && (mc.nsym == 0) == (p.n == 0), "k %u sps %g n %d: plan", k, (double)sps, n);
                if (p.n > 0) {
                    // the tiles' segments of the carry pre-pass tile [0, nsym) in order, and every output of a tile reads
                    // symbols from its tile's first on
                    for (int tile : {1, 3, 1024}) {
                        const long long ntiles = (p.n + tile - 1) / tile;
                        long long prev = 0;
                        EXPECT(mod_tile_first_symbol(p.sc, MOD_NFILTS, tpf, tile, 0, ntiles, mc.nsym) == 0, "the first segment starts at 0");
                        for (long long t = 0; t <= ntiles; ++t) {
                            const long long a = mod_tile_first_symbol(p.sc, MOD_NFILTS, tpf, tile, t, ntiles, mc.nsym);
                            EXPECT(a >= prev && a <= mc.nsym, "k %u sps %g tile %d: segment %lld starts at %lld after %lld", k, (double)sps,
                                   tile, t, a, prev);
                            prev = a;
                            if (t < ntiles) {
                                const long long c = mod_tile_count(p.sc, MOD_NFILTS, t * tile);
                                EXPECT(c < mc.nsym && (c - tpf < 0 ? 0 : c - tpf) == a, "tile %lld: count %lld", t, c);
                            }
                        }
                        EXPECT(prev == mc.nsym, "the last segment ends at nsym");
                        int span = 0;
                        const int tl = arb_closed_tile(MOD_NFILTS, p.D, (unsigned)tpf, 2048, 1024, &span);
                        EXPECT(tl == 1024 && span <= 2048 && span >= tpf, "sps %g: tile %d span %d", (double)sps, tl, span);
                    }
                }
                st = mod_next_state(p, mc.nsym);
                pending = mc.pending_after;
                bytes += n; symbols += mc.nsym; outputs += p.n;
            }
            EXPECT(symbols == bytes * 8 / k && pending == (unsigned)(bytes * 8 % k), "k %u: %lld symbols of %lld bytes", k, symbols, bytes);
            const ArbPlan whole = mod_outputs(ArbState(), rp, symbols);
            const ArbState end = mod_next_state(whole, symbols);
            EXPECT(whole.n == outputs && end.count == st.count && end.j == st.j && memcmp(&end.acc, &st.acc, 4) == 0,
                   "k %u sps %g: %lld outputs in calls, %lld in one piece", k, (double)sps, outputs, whole.n);
        }
    // the int limit: every byte count an int holds gives counts that fit
    for (unsigned k = 1; k <= 8; ++k) {
        const ModCall mc = mod_call(k - 1, INT_MAX, k);
        EXPECT(mc.nsym == ((long long)(k - 1) + 8LL * INT_MAX) / k && mc.pending_after < k, "k %u at INT_MAX bytes", k);
        ArbRate rp;
        arb_rate_params(MOD_NFILTS, 11.5f, &rp);
        const ArbPlan p = mod_outputs(ArbState(), rp, mc.nsym);
        EXPECT(!p.too_many && p.closed && p.n >= (long long)(11.4 * (double)mc.nsym) && p.n <= (long long)(11.6 * (double)mc.nsym) + 1,
               "k %u: %lld outputs of %lld symbols", k, p.n, mc.nsym);
        EXPECT(mod_next_state(p, mc.nsym).count == 0, "k %u: the call ends at its last symbol", k);
    }
}

}  // namespace

int main()
{
    repackers();
    encoder();
    modulator();
    if (fails) {
        printf("modulator_plan_test: %d of %lld checks failed\n", fails, checks);
        return 1;
    }
    printf("modulator_plan_test ok: %lld checks\n", checks);
    return 0;
}
