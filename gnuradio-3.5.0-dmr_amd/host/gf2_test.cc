// gf2_test.cc -- csrc/gf2.h on the host, under the address and undefined-behaviour sanitizers (no device, no library):
//   * xpow8 against repeated multiplication by x^8, the CRC table's first entries, the CRC's known values;
//   * crc_combine against the serial CRC on random splits;
//   * lfsr_advance (the serial steps while bits lie above reg_len, then M^(2^j)) against n serial steps of
//     gri_lfsr.h:113-118 for the parameter sets of tests/golden/ref_packet.npz, and the affine scan step of the scrambler;
//   * the whitening table's ends and the packet plan's offsets and padding against the closed form of
//     packet_utils.py:151-172 for samples_per_symbol 1 .. 8 x bits_per_symbol 1 .. 4, and the refusals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../csrc/gf2.h"

using namespace grhip;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static const unsigned PARAMS[][4] = {                                       // mask, seed, reg_len, count
    {0x8a, 0x7f, 7, 0}, {0x3, 0x3FFF, 14, 0}, {0x1, 0x1, 0, 0}, {0x3, 0x2, 1, 0}, {0x20000029u, 0x12345678u, 30, 0},
    {0x80000057u, 0xdeadbeefu, 31, 0}, {0x8a, 0xABCDEF7Fu, 7, 0}, {0xFFFF008Au, 0x7f, 7, 0}, {0xF000001Du, 0xF00F0055u, 4, 0},
    {0x8a, 0x7f, 7, 1}, {0x8a, 0x7f, 7, 7}, {0x8a, 0x7f, 7, 100}, {0x8a, 0x7f, 7, 4097}, {0x8a, 0xABCDEF7Fu, 7, 100}, {0x19, 0xFFFFFFF1u, 4, 33}};

static void test_crc()
{
    uint32_t t[256];
    crc32_table(t);
    CHECK(t[0] == 0u && t[1] == 0x04C11DB7u && t[2] == 0x09823B6Eu && t[255] == 0xB1F740B4u);      // digital_crc32.cc:49, :112
    uint32_t p = 1;
    for (unsigned n = 0; n < 3000; ++n) {
        CHECK(xpow8(n) == p);
        p = gf2_mulmod(p, 0x100u);
    }
    CHECK(xpow8(1ull << 31) == gf2_mulmod(xpow8(1ull << 30), xpow8(1ull << 30)));
    const char *nine = "123456789";
    CHECK((crc32_update_serial(0xffffffffu, (const unsigned char *)nine, 9) ^ 0xffffffffu) == 0xFC891918u);
    std::vector<unsigned char> z(100, '0'), o(100, '1'), d;
    for (int i = 0; i < 10; ++i) d.insert(d.end(), (const unsigned char *)"0123456789", (const unsigned char *)"0123456789" + 10);
    CHECK((crc32_update_serial(0xffffffffu, z.data(), 100) ^ 0xffffffffu) == 2943744955u);         // qa_crc32.py
    CHECK((crc32_update_serial(0xffffffffu, o.data(), 100) ^ 0xffffffffu) == 2326594156u);
    CHECK((crc32_update_serial(0xffffffffu, d.data(), 100) ^ 0xffffffffu) == 3774345973u);

    std::mt19937 rng(7);
    std::vector<unsigned char> buf(20000);
    for (auto &b : buf) b = (unsigned char)rng();
    for (int k = 0; k < 200; ++k) {
        const size_t len = rng() % (buf.size() + 1), cut = len ? rng() % (len + 1) : 0;
        const uint32_t whole = crc32_update_serial(0u, buf.data(), len);
        const uint32_t a = crc32_update_serial(0u, buf.data(), cut), b = crc32_update_serial(0u, buf.data() + cut, len - cut);
        CHECK(crc_combine(a, b, len - cut) == whole);
        const uint32_t init = (uint32_t)rng();                                                     // the start value's term
        CHECK((gf2_mulmod(init, xpow8(len)) ^ whole) == crc32_update_serial(init, buf.data(), len));
    }
}

static void test_lfsr()
{
    std::mt19937 rng(11);
    for (const auto &q : PARAMS) {
        const uint32_t mask = q[0], seed = q[1], len = q[2];
        std::vector<uint32_t> pw(31 * 32);
        Gf2Mat m = lfsr_matrix(mask, len);
        for (int j = 0; j < 31; ++j) {
            std::memcpy(&pw[(size_t)j * 32], m.c, sizeof(m.c));
            m = gf2_matmul(m, m);
        }
        // n serial steps of the reference's statement against the jump
        uint32_t reg = seed;
        for (unsigned n = 0; n <= 5000; ++n) {
            if (n < 70 || n % 97 == 0 || n == 4096 || n == 5000) CHECK(lfsr_advance(seed, n, mask, len, pw.data()) == reg);
            reg = lfsr_next(reg, mask, len);
        }
        // past the first 31 steps the register is clean and the matrix alone is the step
        uint32_t clean = seed;
        for (int i = 0; i < 32; ++i) clean = lfsr_next(clean, mask, len);
        CHECK(lfsr_clean(clean, len));
        const Gf2Mat m1 = lfsr_matrix(mask, len);
        CHECK(gf2_matvec(m1.c, clean) == lfsr_next(clean, mask, len));
        CHECK(gf2_matvec(gf2_matpow(m1, 1000).c, clean) == lfsr_advance(clean, 1000, mask, len, pw.data()));
        CHECK(gf2_matvec(gf2_matpow(m1, (1u << 31) - 1u).c, clean) == lfsr_advance(clean, (1u << 31) - 1u, mask, len, pw.data()));
        // the scrambler's step is affine on clean registers: the walk from `clean` is M^k clean ^ the walk from 0
        uint32_t a = clean, z = 0;
        for (int k = 1; k <= 300; ++k) {
            const uint32_t in = rng() & 1u;
            a = lfsr_step_or(a, lfsr_parity(a & mask) ^ in, len);
            z = lfsr_step_or(z, lfsr_parity(z & mask) ^ in, len);
            if (k % 16 == 0 || k == 300) CHECK(a == (gf2_matvec(gf2_matpow(m1, (uint64_t)k).c, clean) ^ z));
        }
    }
}

static void test_packets()
{
    std::vector<unsigned char> w(WHITEN_LEN);
    whitening_table(w.data());
    const unsigned char first[16] = {255, 63, 0, 16, 0, 12, 0, 5, 192, 3, 16, 1, 204, 0, 85, 192};   // packet_utils.py:199
    CHECK(std::memcmp(w.data(), first, 16) == 0 && w[4094] == 255 && w[4095] == 63);

    unsigned char code[8];
    CHECK(pack_access_code("1010110011011", code) == 2 && code[0] == 0x15 && code[1] == 0x9B);      // 13 characters, 3 leading zeros
    CHECK(pack_access_code("1", code) == 1 && code[0] == 1);
    std::string c64(64, '1'), c65(65, '1');
    CHECK(pack_access_code(c64.c_str(), code) == 8 && code[0] == 0xff && code[7] == 0xff);
    CHECK(pack_access_code(c65.c_str(), code) == -1 && pack_access_code("", code) == -1 && pack_access_code("012", code) == -1 &&
          pack_access_code(nullptr, code) == -1);

    const int lengths[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4091, 4092};
    const int offs[] = {0, 1, 15, 0, 1, 15, 0, 1, 15, 0, 1, 15, 0, 1, 0};
    const int n = (int)(sizeof(lengths) / sizeof(lengths[0]));
    for (int sps = 1; sps <= 8; ++sps)
        for (int bps = 1; bps <= 4; ++bps)
            for (int pad = 0; pad < 2; ++pad)
                for (int ab = 1; ab <= 8; ab += 7) {
                    std::vector<PacketJob> jobs((size_t)n);
                    long long tin = -1, tout = -1;
                    CHECK(packet_plan(n, lengths, offs, ab, sps, bps, pad != 0, jobs.data(), &tin, &tout) == nullptr);
                    long long in = 0, out = 0;
                    for (int i = 0; i < n; ++i) {
                        CHECK(jobs[i].in_offset == in && jobs[i].out_offset == out && jobs[i].length == (unsigned)lengths[i] &&
                              jobs[i].whitener_offset == (unsigned)offs[i]);
                        long long len = 2 + ab + 4 + lengths[i] + 4 + 1;
                        if (pad) {                                          // _npadding_bytes as it stands, :167-172
                            int a = 16, b = sps;
                            while (b) { const int t = a % b; a = b; b = t; }
                            const long long byte_modulus = (long long)(16 * sps / a) * bps / sps;
                            const long long r = len % byte_modulus;
                            if (r) len += byte_modulus - r;
                            CHECK(len % byte_modulus == 0);
                        }
                        CHECK(packet_bytes(ab, lengths[i], sps, bps, pad != 0) == len);
                        in += lengths[i];
                        out += len;
                    }
                    CHECK(tin == in && tout == out);
                }
    PacketJob j[2];
    const int bad_len[] = {4093}, neg_len[] = {-1}, ok_len[] = {4092}, one[] = {1}, neg[] = {-1}, len100[] = {100}, o3993[] = {3993}, o3992[] = {3992};
    CHECK(packet_plan(1, bad_len, nullptr, 8, 2, 1, true, j, nullptr, nullptr) != nullptr);        // L > 4096
    CHECK(packet_plan(1, neg_len, nullptr, 8, 2, 1, true, j, nullptr, nullptr) != nullptr);
    CHECK(packet_plan(1, ok_len, nullptr, 8, 2, 1, true, j, nullptr, nullptr) == nullptr);          // L = 4096
    CHECK(packet_plan(1, ok_len, one, 8, 2, 1, true, j, nullptr, nullptr) != nullptr);              // L + o > 4096
    CHECK(packet_plan(1, len100, neg, 8, 2, 1, true, j, nullptr, nullptr) != nullptr);              // o < 0
    CHECK(packet_plan(1, len100, o3992, 8, 2, 1, true, j, nullptr, nullptr) == nullptr && j[0].whitener_offset == 3992u);
    CHECK(packet_plan(1, len100, o3993, 8, 2, 1, true, j, nullptr, nullptr) != nullptr);
    CHECK(packet_plan(0, nullptr, nullptr, 8, 2, 1, true, j, nullptr, nullptr) == nullptr);
}

int main()
{
    test_crc();
    test_lfsr();
    test_packets();
    if (failures) { std::printf("gf2_test: %d failure(s)\n", failures); return 1; }
    std::printf("gf2_test ok\n");
    return 0;
}
