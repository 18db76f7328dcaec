// pfb_clock_sync_test.cc -- csrc/pfb_clock_sync.h (gr_pfb_clock_sync_ccf's tap partition, create_diff_taps, update_gains
// and the loop's scalar step) under the address and undefined-behaviour sanitizers: host arithmetic only, needs
// neither libgrhip.so nor HIP.
//
//   pfb_clock_sync_test                    the checks below; prints "pfb_clock_sync_test ok"
//   pfb_clock_sync_test taps NF T0 T1 ...  the bank, then the derivative bank as hex bit patterns (taps given as hex bit patterns)
//   pfb_clock_sync_test gains BW DF ...    per pair (loop_bw, damping; both as hex bit patterns, damping "-" for the constructor's)
//                                          alpha and beta as hex bit patterns: pcs_gains itself, then the same pair through
//                                          PcsLoop::init, set_damping_factor and set_loop_bandwidth, as a handle's setters go
// (tests/test_pfb_clock_sync_cpu.py holds the printed banks against the reference's.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#include "../csrc/pfb_clock_sync.h"

using namespace grhip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
static float from_bits(unsigned u) { float v; memcpy(&v, &u, 4); return v; }

// one evaluation from a hostile k: the trips stay bounded, the arm inside the bank, the position inside the rule
static void hostile_wrap(float k, int nf, long long pos, long long lo)
{
    const long long pos0 = pos;
    int slips = 0, trips = 0;
    const int fn = pcs_wrap(k, pos, lo, nf, slips, trips);
    CHECK(trips >= 0 && trips <= PCS_WRAP_TRIPS);
    CHECK(fn >= 0 && fn < nf);
    CHECK(pos >= lo && pos <= (pos0 > lo ? pos0 : lo) + PCS_CARRY);
    CHECK(std::isfinite(k) && k >= 0.f && k <= (float)nf);
    CHECK(slips >= 0 && slips <= 3);
}

int main(int argc, char **argv)
{
    if (argc >= 4 && std::string(argv[1]) == "taps") {
        std::vector<float> t, b, d;
        for (int i = 3; i < argc; ++i) t.push_back(from_bits((unsigned)strtoul(argv[i], nullptr, 16)));
        int tpf = 0;
        if (const char *e = pcs_design(t.data(), (long long)t.size(), atoi(argv[2]), b, d, tpf)) { printf("%s\n", e); return 1; }
        for (const std::vector<float> *v : {&b, &d})
            for (float x : *v) printf("%08x\n", bits(x));
        return 0;
    }
    if (argc >= 4 && argc % 2 == 0 && std::string(argv[1]) == "gains") {
        for (int i = 2; i + 1 < argc; i += 2) {
            const float bw = from_bits((unsigned)strtoul(argv[i], nullptr, 16));
            const bool own = std::string(argv[i + 1]) == "-";
            const float df = own ? sqrtf(2.0f) / 2.0f : from_bits((unsigned)strtoul(argv[i + 1], nullptr, 16));
            float a, b;
            pcs_gains(df, bw, a, b);
            PcsLoop loop;
            // the setters' way there: from another bandwidth, the damping first
            if (!loop.init(0.0628f, 1.5f) || (!own && !loop.set_damping_factor(df)) || !loop.set_loop_bandwidth(bw)) { printf("refused\n"); return 1; }
            printf("%08x %08x %08x %08x\n", bits(a), bits(b), bits(loop.alpha), bits(loop.beta));
        }
        return 0;
    }
    const float nanf_ = std::numeric_limits<float>::quiet_NaN(), inff = std::numeric_limits<float>::infinity();
    std::vector<float> b, d;
    int tpf = -1;
    // ---- the designer: 2 taps, a count that is no multiple of the arm count, the limits
    const float two[2] = {1.f, -2.f};
    CHECK(!pcs_design(two, 2, 1, b, d, tpf) && tpf == 2 && b.size() == 2 && d.size() == 2 && b[0] == 1.f && b[1] == -2.f && d[0] == 0.f && d[1] == 0.f);
    CHECK(!pcs_design(two, 2, 256, b, d, tpf) && tpf == 1 && b.size() == 256 && b[1] == -2.f && b[2] == 0.f && b[255] == 0.f);
    std::vector<float> t13(13);
    for (int i = 0; i < 13; ++i) t13[i] = (float)(i * i) - 20.f;
    CHECK(!pcs_design(t13.data(), 13, 5, b, d, tpf) && tpf == 3 && b.size() == 15);
    for (int f = 0; f < 5; ++f)
        for (int j = 0; j < 3; ++j) CHECK(b[f * 3 + j] == (f + 5 * j < 13 ? t13[f + 5 * j] : 0.f));
    CHECK(d[0] == 0.f && d[2 * 3 + 2] == 0.f);                  // the derivative's first and last (index 12 = arm 2, tap 2) are 0
    {   // create_diff_taps: pwr gathers the partial sums -t[i], -t[i], t[i+2] - t[i]
        float pwr = 0;
        for (int i = 0; i < 11; ++i) { float tap = -t13[i]; pwr += fabsf(tap); pwr += fabsf(tap); tap += t13[i + 2]; pwr += fabsf(tap); }
        CHECK(d[1 * 3 + 0] == (t13[2] - t13[0]) * pwr);          // derivative tap 1 = arm 1, tap 0
    }
    std::vector<float> big(PCS_MAX_BANK, 0.25f);
    CHECK(!pcs_design(big.data(), PCS_MAX_BANK, 64, b, d, tpf) && tpf == 64);
    CHECK(!pcs_design(big.data(), PCS_MAX_BANK, 16, b, d, tpf) && tpf == 256);
    CHECK(!pcs_design(big.data(), PCS_MAX_BANK, 256, b, d, tpf) && tpf == 16);
    CHECK(!pcs_design(big.data(), PCS_MAX_BANK - 255, 256, b, d, tpf) && tpf == 16 && b.size() == (size_t)PCS_MAX_BANK);
    // ---- every refusal; a refused design leaves the vectors alone
    const std::vector<float> keep = b;
    big.push_back(0.f);
    CHECK(pcs_design(big.data(), PCS_MAX_BANK + 1, 64, b, d, tpf));         // 65 taps per arm of 64: 4160 in the bank
    CHECK(pcs_design(big.data(), 300, 1, b, d, tpf));                       // 300 taps per arm
    CHECK(pcs_design(big.data(), 1, 1, b, d, tpf) && pcs_design(big.data(), 0, 4, b, d, tpf) && pcs_design(big.data(), -5, 4, b, d, tpf));
    CHECK(pcs_design(big.data(), 64, 0, b, d, tpf) && pcs_design(big.data(), 64, -1, b, d, tpf) && pcs_design(big.data(), 64, 257, b, d, tpf));
    CHECK(pcs_design(nullptr, 64, 4, b, d, tpf));
    big[7] = nanf_;
    CHECK(pcs_design(big.data(), 64, 4, b, d, tpf));
    big[7] = inff;
    CHECK(pcs_design(big.data(), 64, 4, b, d, tpf));
    big[7] = 3e38f;                                                         // finite taps, a derivative that is not
    big[9] = -3e38f;
    CHECK(pcs_design(big.data(), 64, 4, b, d, tpf));
    CHECK(b == keep && tpf == 16);
    CHECK(pcs_check_args(0.99, 0.06f, 0, 1.5f, 1) && pcs_check_args(256.0, 0.06f, 0, 1.5f, 1) && pcs_check_args(nanf_, 0.06f, 0, 1.5f, 1));
    CHECK(pcs_check_args(2, -0.01f, 0, 1.5f, 1) && pcs_check_args(2, nanf_, 0, 1.5f, 1) && pcs_check_args(2, inff, 0, 1.5f, 1));
    CHECK(pcs_check_args(2, 0.06f, nanf_, 1.5f, 1) && pcs_check_args(2, 0.06f, inff, 1.5f, 1) && pcs_check_args(2, 0.06f, 0, nanf_, 1));
    CHECK(pcs_check_args(2, 0.06f, 0, 1.5f, 0) && pcs_check_args(2, 0.06f, 0, 1.5f, -1) && pcs_check_args(2, 0.06f, 0, 1.5f, 9));
    CHECK(!pcs_check_args(1.0, 0.f, -3.5f, 0.f, 8) && !pcs_check_args(255.9, 0.06f, 31.5f, -1.5f, 1));
    // ---- the loop's host side
    PcsLoop loop;
    CHECK(loop.init(0.0628f, 1.5f) && loop.damping == sqrtf(2.0f) / 2.0f && loop.alpha > 0 && loop.beta > 0);
    const PcsLoop was = loop;
    CHECK(!loop.set_loop_bandwidth(-1.f) && !loop.set_loop_bandwidth(nanf_) && !loop.set_loop_bandwidth(inff) && !loop.set_loop_bandwidth(3e38f));
    CHECK(!loop.set_damping_factor(-0.1f) && !loop.set_damping_factor(1.1f) && !loop.set_damping_factor(nanf_));
    CHECK(!loop.set_alpha(-0.1f) && !loop.set_alpha(1.5f) && !loop.set_alpha(nanf_) && !loop.set_beta(-1.f) && !loop.set_beta(2.f) && !loop.set_beta(nanf_));
    CHECK(!loop.set_max_dev(nanf_) && !loop.set_max_dev(inff));
    CHECK(!memcmp(&loop, &was, sizeof(loop)));
    CHECK(loop.set_alpha(0.f) && loop.set_alpha(1.f) && loop.set_beta(1.f) && loop.set_damping_factor(0.f) && loop.set_damping_factor(1.f));
    float ri, rf;
    pcs_rate(2.5, 32, ri, rf);
    CHECK(ri == 16.f && rf == 0.f);
    pcs_rate(2.0, 32, ri, rf);
    CHECK(ri == 0.f && rf == 0.f);
    // ---- the shared step on hostile states.  Such states are never tried on a device.
    const float ks[] = {0.f, -0.f, 31.999f, 32.f, -1e-10f, 1e30f, -1e30f, 3.4e38f, -3.4e38f, inff, -inff, nanf_, 536870912.f, -536870912.f,
                        536870880.f, -536870880.f, 2047.5f, -2047.5f, 2048.f, 2049.f, -2049.f, 65.f * 32.f, -65.f * 32.f, 1e-45f, -1e-45f};
    for (float k : ks)
        for (int nf : {1, 2, 5, 32, 256})
            for (long long pos : {0LL, 1LL, 7LL, 1000000LL, 4000000000000LL})
                for (long long back : {0LL, 1LL, 3LL}) hostile_wrap(k, nf, pos, pos - back > 0 ? pos - back : 0);
    // a whole symbol with errors of 1e30 and max_dev 0: the state stays finite where the clip holds it, k is wrapped again
    for (float md : {0.f, 1.5f})
        for (float e : {1e30f, -1e30f, 3e38f}) {
            PcsParams p = {1.f, 1.f, md, 16.f, 32, 23, 2, 2};
            PcsState s = {5.f, 0.25f, 0.f, 0, 100};
            for (int sym = 0; sym < 50; ++sym) {
                const long long lo = s.pos - p.isps + 1, start = s.pos;
                for (int kk = 0; kk < p.osps; ++kk) {
                    int trips = 0;
                    const int fn = pcs_wrap(s.k, s.pos, lo, p.nfilters, s.slips, trips);
                    CHECK(fn >= 0 && fn < p.nfilters && trips <= PCS_WRAP_TRIPS);
                    CHECK(s.pos >= lo && s.pos <= start + (kk + 1) * PCS_CARRY);
                    s.k = pcs_advance(s.k, p.rate_i, s.rate_f);
                }
                pcs_step(s, p, e, 1.f, 1.f, 0.f);               // error_r = e
                CHECK(fabsf(s.rate_f) <= md || !std::isfinite(s.rate_f));
                s.pos += p.isps;
                CHECK(s.pos > start - p.isps + 1);
            }
            CHECK(s.slips > 0);
        }
    // the clip, literally: inside the limit the value comes back, outside the limit itself
    CHECK(pcs_clip(0.25f, 1.5f) == 0.25f && pcs_clip(7.f, 1.5f) == 1.5f && pcs_clip(-7.f, 1.5f) == -1.5f && pcs_clip(0.3f, 0.f) == 0.f);
    if (fails) return 1;
    printf("pfb_clock_sync_test ok\n");
    return 0;
}
