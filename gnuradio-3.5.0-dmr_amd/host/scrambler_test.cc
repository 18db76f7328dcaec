// scrambler_test.cc -- the host blocks gr_make_scrambler_bb, gr_make_descrambler_bb and gr_make_additive_scrambler_bb
// (host/grhip_blocks.h) on a device: qa_scrambler.py:33-61 as work() calls cut at odd places, the factory signatures of
// general/gr_scrambler_bb.h:31-32, gr_descrambler_bb.h:31-32 and gr_additive_scrambler_bb.h:31-32, and the refusal of
// a register length above 31.
#include <cstdio>
#include <type_traits>
#include <vector>

#include "grhip_blocks.h"

static_assert(std::is_same<decltype(&gr_make_scrambler_bb), grhip_scrambler_bb_sptr (*)(int, int, int, int)>::value, "");
static_assert(std::is_same<decltype(&gr_make_descrambler_bb), grhip_descrambler_bb_sptr (*)(int, int, int, int)>::value, "");
static_assert(std::is_same<decltype(&gr_make_additive_scrambler_bb), grhip_additive_scrambler_bb_sptr (*)(int, int, int, int, int)>::value, "");
static_assert(std::is_base_of<gr_sync_block, grhip_scrambler_bb_blk>::value && std::is_base_of<gr_sync_block, grhip_additive_scrambler_bb_blk>::value, "");
static_assert(!std::is_copy_constructible<grhip_scrambler_bb_blk>::value, "");

template <class F> static bool throws(F f)
{
    try { f(); } catch (const std::exception &) { return true; }
    return false;
}

// work() over `x`, cut at 7 and 4097 items
template <class B> static std::vector<unsigned char> run(B blk, const std::vector<unsigned char> &x)
{
    std::vector<unsigned char> y(x.size());
    const size_t cuts[] = {0, 7, 4097 < x.size() ? 4097 : x.size(), x.size()};
    for (int c = 0; c < 3; ++c) {
        if (cuts[c + 1] == cuts[c]) continue;
        gr_vector_const_void_star in{x.data() + cuts[c]};
        gr_vector_void_star out{y.data() + cuts[c]};
        if (blk->work((int)(cuts[c + 1] - cuts[c]), in, out) != (int)(cuts[c + 1] - cuts[c])) return {};
    }
    return y;
}

int main()
{
    if (!throws([] { gr_make_scrambler_bb(0x8a, 0x7f, 32); }) || !throws([] { gr_make_descrambler_bb(0x8a, 0x7f, 32); }) ||
        !throws([] { gr_make_additive_scrambler_bb(0x8a, 0x7f, 32, 0); })) {
        std::printf("FAIL: a register length of 32 was accepted\n");
        return 1;
    }
    const std::vector<unsigned char> src(5000, 1);
    for (int mode : {GRHIP_MODE_FAST, GRHIP_MODE_GENERIC}) {
        auto s = gr_make_scrambler_bb(0x8a, 0x7F, 7);                        // CCSDS 7-bit scrambler
        auto d = gr_make_descrambler_bb(0x8a, 0x7F, 7);
        s->set_mode(mode);
        d->set_mode(mode);
        const std::vector<unsigned char> mid = run(s, src), dst = run(d, mid);
        if (dst.size() != src.size() || mid == src) { std::printf("FAIL: scrambler output\n"); return 1; }
        for (size_t i = 8; i < dst.size(); ++i)                              // skip garbage during synchronization
            if (dst[i] != src[i - 8]) { std::printf("FAIL: descrambled item %zu (mode %d)\n", i, mode); return 1; }
        for (int count : {0, 100}) {
            auto a = gr_make_additive_scrambler_bb(0x8a, 0x7f, 7, count), b = gr_make_additive_scrambler_bb(0x8a, 0x7f, 7, count);
            a->set_mode(mode);
            b->set_mode(mode);
            const std::vector<unsigned char> m2 = run(a, src);
            if (m2 == src || run(b, m2) != src) { std::printf("FAIL: additive scrambler, count %d (mode %d)\n", count, mode); return 1; }
        }
    }
    std::printf("scrambler_test ok\n");
    return 0;
}
