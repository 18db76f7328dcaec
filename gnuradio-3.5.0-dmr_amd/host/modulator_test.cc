// modulator_test -- the modulator's blocks of grhip_blocks.h: the reference's factory signatures, io signatures, rates and
// refusals, and small flowgraphs under the stand-in executor (grhip_executor.h).
//   * packed_to_unpacked_bb -> unpacked_to_packed_bb gives the bytes back (qa_packed_to_unpacked.py tests 009-011), in
//     calls of at most 37 items, whose chunks straddle the calls;
//   * packed_to_unpacked_bb -> map_bb -> diff_encoder_bb -> chunks_to_symbols_bc -> pfb_arb_resampler_ccf as a flowgraph,
//     in uneven calls, gives bit for bit (GRHIP_MODE_GENERIC) the samples of generic_mod in one run and in pieces, both
//     engines, with chunks of 2 and of 3 bits, samples_per_symbol 2 and 2.5;
//   * the literal vectors of qa_packed_to_unpacked.py tests 001-004 through general_work directly.
// For tests/test_gpu_host_modulator.py; no arguments.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

namespace {

template <class F> bool throws(F f)
{
    try { f(); } catch (const std::invalid_argument &) { return true; }
    return false;
}

std::vector<unsigned char> seeded_bytes(size_t n)
{
    std::vector<unsigned char> x(n);
    unsigned lcg = 2463534242u;
    for (auto &b : x) { lcg = lcg * 1664525u + 1013904223u; b = (unsigned char)(lcg >> 24); }
    return x;
}

std::vector<unsigned char> run_chain(const std::vector<gr_block_sptr> &chain, const std::vector<unsigned char> &x, size_t at, size_t n, int max_noutput)
{
    grhip_linear_flowgraph fg(max_noutput, true);
    for (const gr_block_sptr &b : chain) fg.connect(b);
    return fg.run(x.data() + at, n);
}

// the factories carry the reference's signatures, with the device behind them
static_assert(std::is_same<decltype(&grhip_make_packed_to_unpacked_bb), grhip_packed_to_unpacked_bb_sptr (*)(unsigned int, gr_endianness_t, int)>::value, "");
static_assert(std::is_same<decltype(&grhip_make_unpacked_to_packed_bb), grhip_unpacked_to_packed_bb_sptr (*)(unsigned int, gr_endianness_t, int)>::value, "");
static_assert(std::is_same<decltype(&grhip_make_diff_encoder_bb), grhip_diff_encoder_bb_sptr (*)(unsigned int, int)>::value, "");
static_assert(std::is_same<decltype(&grhip_make_chunks_to_symbols_bc), grhip_chunks_to_symbols_bc_sptr (*)(const std::vector<gr_complex> &, const int, int)>::value, "");
static_assert(std::is_same<decltype(&grhip_make_generic_mod), grhip_generic_mod_sptr (*)(grhip_constellation_sptr, double, bool, double, bool, int)>::value, "");
static_assert(std::is_base_of<gr_block, grhip_packed_to_unpacked_bb_blk>::value && !std::is_base_of<gr_sync_block, grhip_packed_to_unpacked_bb_blk>::value, "");
static_assert(std::is_base_of<gr_sync_block, grhip_diff_encoder_bb_blk>::value && !std::is_base_of<gr_sync_interpolator, grhip_diff_encoder_bb_blk>::value, "");
static_assert(std::is_base_of<gr_sync_interpolator, grhip_chunks_to_symbols_bc_blk>::value, "");
static_assert(std::is_base_of<gr_block, grhip_generic_mod_blk>::value && !std::is_base_of<gr_sync_block, grhip_generic_mod_blk>::value, "");
static_assert(!std::is_copy_constructible<grhip_generic_mod_blk>::value && !std::is_copy_constructible<grhip_diff_encoder_bb_blk>::value, "");
static_assert(GR_MSB_FIRST == GRHIP_MSB_FIRST && GR_LSB_FIRST == GRHIP_LSB_FIRST, "");

int surface()
{
    int fails = 0;
    grhip_packed_to_unpacked_bb_sptr p = grhip_make_packed_to_unpacked_bb(3, GR_MSB_FIRST);
    grhip_unpacked_to_packed_bb_sptr u = grhip_make_unpacked_to_packed_bb(3, GR_LSB_FIRST);
    if (p->relative_rate() != 8.0 / 3 || u->relative_rate() != 3 / 8.0 || p->history() != 1 || p->name() != "packed_to_unpacked_bb" ||
        p->input_signature()->sizeof_stream_item(0) != 1 || u->output_signature()->sizeof_stream_item(0) != 1) fails++;
    gr_vector_int req(1);
    p->forecast(5, req);                                    // ceil(15 / 8)
    if (req[0] != 2) fails++;
    u->forecast(5, req);                                    // ceil(40 / 3)
    if (req[0] != 14) fails++;
    if (!throws([] { grhip_make_packed_to_unpacked_bb(0, GR_MSB_FIRST); }) || !throws([] { grhip_make_packed_to_unpacked_bb(9, GR_MSB_FIRST); }) ||
        !throws([] { grhip_make_unpacked_to_packed_bb(0, GR_LSB_FIRST); }) || !throws([] { grhip_make_diff_encoder_bb(0); }) ||
        !throws([] { grhip_make_chunks_to_symbols_bc({}, 1); }) || !throws([] { grhip_make_chunks_to_symbols_bc({gr_complex(1, 0)}, 0); })) fails++;
    grhip_chunks_to_symbols_bc_sptr c = grhip_make_chunks_to_symbols_bc({gr_complex(1, 0), gr_complex(0, 1), gr_complex(-1, 0), gr_complex(0, -1)}, 2);
    if (c->D() != 2 || c->interpolation() != 2 || c->output_multiple() != 2 || c->symbol_table().size() != 4 ||
        c->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex)) fails++;
    grhip_constellation_sptr dq = digital_make_constellation_dqpsk();
    grhip_generic_mod_sptr m = grhip_make_generic_mod(dq, 2.5, true, 0.35);
    if (m->bits_per_symbol() != 2 || m->samples_per_symbol() != 2.5 || m->engine() != 1 || m->taps().size() != 32 * 11 * 2 + 1 ||
        m->relative_rate() != 10.0 || m->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex)) fails++;
    if (m->taps() != grhip_firdes_root_raised_cosine_taps(32, 32, 1.0, 0.35, 32 * 11 * 2)) fails++;
    grhip_constellation_sptr c2 = digital_make_constellation_calcdist({gr_complex(1, 0), gr_complex(1, 0), gr_complex(-1, 0), gr_complex(-1, 0)}, {}, 1, 2);
    if (!throws([&] { grhip_make_generic_mod(dq, 1.5); }) || !throws([&] { grhip_make_generic_mod(dq, 12); }) ||
        !throws([&] { grhip_make_generic_mod(c2, 2); }) || !throws([&] { m->set_engine(2); }) || !throws([&] { m->set_mode(11); })) fails++;
    // qa_packed_to_unpacked.py tests 001-004, one general_work each
    struct { unsigned k; gr_endianness_t e; unsigned char src; std::vector<unsigned char> want; } qa[] = {
        {1, GR_MSB_FIRST, 0x80, {1, 0, 0, 0, 0, 0, 0, 0}}, {1, GR_LSB_FIRST, 0x80, {0, 0, 0, 0, 0, 0, 0, 1}},
        {3, GR_LSB_FIRST, 0x11, {4, 2}}, {3, GR_MSB_FIRST, 0x11, {0, 4}}};
    for (auto &q : qa) {
        grhip_packed_to_unpacked_bb_sptr b = grhip_make_packed_to_unpacked_bb(q.k, q.e);
        std::vector<unsigned char> out(q.want.size());
        gr_vector_int nin(1, 1);
        gr_vector_const_void_star in(1, &q.src);
        gr_vector_void_star o(1, out.data());
        if (b->general_work((int)out.size(), nin, in, o) != (int)out.size() || out != q.want || b->consumed() != (int)(out.size() * q.k / 8)) fails++;
    }
    if (fails) printf("surface: %d failure(s)\n", fails);
    return fails;
}

int round_trips()
{
    int fails = 0;
    struct { unsigned k; gr_endianness_t e; size_t n, back; } cases[] = {{3, GR_MSB_FIRST, 202, 201}, {7, GR_MSB_FIRST, 56, 56},
                                                                        {7, GR_LSB_FIRST, 56, 56}, {8, GR_LSB_FIRST, 64, 64}};
    for (auto &c : cases) {
        const std::vector<unsigned char> x = seeded_bytes(c.n);
        const std::vector<unsigned char> y = run_chain({grhip_make_packed_to_unpacked_bb(c.k, c.e), grhip_make_unpacked_to_packed_bb(c.k, c.e)}, x, 0, x.size(), 37);
        if (y.size() != c.back || memcmp(y.data(), x.data(), y.size())) {
            printf("round trip k %u: %zu bytes back, %zu expected\n", c.k, y.size(), c.back);
            fails++;
        }
    }
    return fails;
}

int chain_against_generic_mod()
{
    int fails = 0;
    const std::vector<unsigned char> x = seeded_bytes(700);
    struct { grhip_constellation_sptr c; double sps; bool diff; } cases[] = {{digital_make_constellation_dqpsk(), 2, true},
                                                                            {digital_make_constellation_8psk(), 2.5, true},
                                                                            {digital_make_constellation_qpsk(), 2.5, false}};
    for (auto &cs : cases) {
        const unsigned k = cs.c->bits_per_symbol();
        const std::vector<unsigned int> pre_diff = cs.c->pre_diff_code();
        const std::vector<int> code(pre_diff.begin(), pre_diff.end());
        std::vector<gr_block_sptr> chain = {grhip_make_packed_to_unpacked_bb(k, GR_MSB_FIRST), gr_make_map_bb(code)};
        if (cs.diff) chain.push_back(grhip_make_diff_encoder_bb(1u << k));
        chain.push_back(grhip_make_chunks_to_symbols_bc(cs.c->points()));
        grhip_pfb_arb_resampler_ccf_sptr arb =
            grhip_make_pfb_arb_resampler_ccf((float)cs.sps, grhip_firdes_root_raised_cosine_taps(32, 32, 1.0, 0.35, 32 * 11 * (int)cs.sps));
        arb->set_mode(GRHIP_MODE_GENERIC);
        chain.push_back(arb);
        const std::vector<unsigned char> want = run_chain(chain, x, 0, x.size(), 37);
        const size_t nsym = x.size() * 8 / k;
        if (want.size() / sizeof(gr_complex) < (size_t)(nsym * cs.sps) - 1) { printf("the chain gave %zu samples\n", want.size() / sizeof(gr_complex)); fails++; }
        for (int engine = 0; engine < 2; ++engine) {
            for (int pieces = 0; pieces < 2; ++pieces) {
                grhip_generic_mod_sptr m = grhip_make_generic_mod(cs.c, cs.sps, cs.diff, 0.35, true);
                m->set_engine(engine);
                m->set_mode(GRHIP_MODE_GENERIC);
                std::vector<unsigned char> got;
                const size_t cut[] = {0, 1, 38, 333, x.size()};
                for (int i = 0; i < 4; ++i) {
                    const size_t a = pieces ? cut[i] : 0, b = pieces ? cut[i + 1] : x.size();
                    const std::vector<unsigned char> part = run_chain({m}, x, a, b - a, pieces ? 37 : 1 << 20);
                    got.insert(got.end(), part.begin(), part.end());
                    if (!pieces) break;
                }
                if (got != want) {
                    printf("generic_mod k %u sps %g engine %d %s: %zu samples, the chain %zu\n", k, cs.sps, engine, pieces ? "in pieces" : "in one run",
                           got.size() / sizeof(gr_complex), want.size() / sizeof(gr_complex));
                    fails++;
                }
            }
        }
    }
    return fails;
}

}  // namespace

int main()
{
    try {
        int fails = surface() + round_trips() + chain_against_generic_mod();
        if (fails) {
            printf("modulator_test FAILED: %d\n", fails);
            return 1;
        }
        printf("modulator_test ok\n");
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "modulator_test: " << e.what() << "\n";
        return 1;
    }
}
