// logpwr_plan_test -- the fused-versus-composed predicate of blks2.logpwrfft (csrc/logpwr_plan.h) on the CPU, under the
// address and undefined-behaviour sanitizers.  fft16x_kernel's kept-frame addressing is restated here lane by lane:
// for every call the predicate accepts, the largest byte a lane of any group can reach through the group's descriptor
// (its 32-bit offset, the instruction's point offset and the item on top) must stay below 2^32 -- in fact at or below
// the 2^31 the header promises -- and the descriptor's range must hold it; everything beyond the stated limit must be
// sent to the composed path.  For tests/test_logpwrfft_cpu.py; no arguments.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../csrc/logpwr_plan.h"

using namespace grhip;

static long long frame_of(long long ov, long long n_frames, long long n_out, long long first, long long n)
{
    const long long s = ov / n_out, o = ov - s * n_out;
    return s * n_frames + first + o * n;
}

// the largest end (exclusive) of any lane's access relative to its group's descriptor base, over every group of the call;
// also checks each group's range as the kernel forms it
static int walk(int N, int item, long long S, long long n_frames, long long n_out, long long first, long long n,
                unsigned long long *max_end)
{
    const long long vpg = 4096 / N, lpv = N / 16, total = S * n_out, ngroups = (total + vpg - 1) / vpg;
    int fails = 0;
    *max_end = 0;
    for (long long g = 0; g < ngroups; ++g) {
        const long long ov0 = g * vpg, ovl = ov0 + vpg - 1 < total - 1 ? ov0 + vpg - 1 : total - 1;
        const long long f0 = frame_of(ov0, n_frames, n_out, first, n), fl = frame_of(ovl, n_frames, n_out, first, n);
        const unsigned long long range = (unsigned long long)(fl - f0 + 1) * N * item;
        if (range > (unsigned long long)LOGPWR_MAX_RANGE) { printf("range %llu past the limit\n", range); fails++; }
        for (long long vl = 0; vl < vpg; ++vl) {
            const long long ov = ov0 + vl;
            unsigned long long voff = range;                        // a lane past the last vector
            if (ov <= ovl) voff = (unsigned long long)(frame_of(ov, n_frames, n_out, first, n) - f0) * N * item + (unsigned long long)item * (lpv - 1);
            const unsigned long long end = voff + (unsigned long long)item * lpv * 15 + item;
            if (end > *max_end) *max_end = end;
            if (ov <= ovl && end > range) { printf("a valid lane reaches past its descriptor\n"); fails++; }
            if (ov > ovl && voff < range) { printf("an invalid lane is in range\n"); fails++; }
        }
    }
    return fails;
}

int main()
{
    int fails = 0;
    long long cases = 0;
    const int sizes[] = {32, 64, 128, 256, 512, 1024, 2048};
    for (int N : sizes)
        for (int item : {4, 8}) {
            const long long vpg = 4096 / N, frame = (long long)N * item;
            // one stream: the bound is exact, limit = the largest decimation whose group range is <= 2^31 bytes
            const long long limit = (LOGPWR_MAX_RANGE - frame) / ((vpg - 1) * frame);
            const long long decims[] = {1, 2, 3, 81, 326, 1000, limit / 2, limit - 1, limit};
            for (long long n : decims) {
                for (long long n_out : {1ll, vpg - 1, vpg, vpg + 1, 3 * vpg + vpg / 2 + 1}) {
                    if (n_out < 1) continue;
                    for (long long first : {0ll, n - 1}) {
                        const long long n_frames = first + (n_out - 1) * n + 1 + 2;
                        cases++;
                        if (!logpwr_fused_ok(N, item, 1, n_frames, n_out, n)) {
                            printf("N %d item %d decimation %lld n_out %lld: refused below the limit %lld\n", N, item, n, n_out, limit);
                            fails++;
                            continue;
                        }
                        unsigned long long end = 0;
                        fails += walk(N, item, 1, n_frames, n_out, first, n, &end);
                        if (end >= (1ull << 32)) { printf("N %d item %d decimation %lld: offset %llu wraps\n", N, item, n, end); fails++; }
                    }
                }
            }
            // beyond the limit (a full group in one stream): composed
            for (long long n : {limit + 1, limit + 2, 2 * limit, 1ll << 31, 1ll << 45}) {
                cases++;
                if (logpwr_fused_ok(N, item, 1, (vpg + 2) * n, vpg, n)) {
                    printf("N %d item %d decimation %lld: accepted beyond the limit %lld\n", N, item, n, limit);
                    fails++;
                }
            }
            // several streams: a group straddles stream ends; whatever is accepted must stay in reach
            for (long long S : {2ll, 3ll, 200ll})
                for (long long n_out : {1ll, 2ll, vpg / 2 + 1, vpg + 3})
                    for (long long n : {1ll, 3ll, 1000ll})
                        for (long long extra : {0ll, 5ll, 1ll << 14, 1ll << 20, 1ll << 26}) {
                            const long long n_frames = (n_out - 1) * n + 1 + extra;
                            cases++;
                            if (!logpwr_fused_ok(N, item, S, n_frames, n_out, n)) continue;
                            unsigned long long end = 0;
                            fails += walk(N, item, S, n_frames, n_out, 0, n, &end);
                            if (end >= (1ull << 32)) { printf("N %d item %d S %lld: offset %llu wraps\n", N, item, S, end); fails++; }
                        }
            printf("N %4d item %d: one stream fused up to decimation %lld\n", N, item, limit);
        }
    // the sizes with a descriptor per vector take any decimation; other sizes are never fused
    if (!logpwr_fused_ok(4096, 8, 3, 1ll << 30, 5, 1ll << 20) || !logpwr_fused_ok(8192, 4, 1, 1ll << 20, 7, 81)) fails++;
    if (logpwr_fused_ok(16, 8, 1, 10, 5, 2) || logpwr_fused_ok(100, 8, 1, 10, 5, 2) || logpwr_fused_ok(16384, 8, 1, 10, 5, 2)) fails++;
    if (logpwr_fused_ok(4096, 8, 65535, 1 << 20, 1 << 20, 1)) fails++;              // more vectors than one launch counts
    printf("%lld cases, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
