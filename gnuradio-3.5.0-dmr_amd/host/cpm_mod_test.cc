// cpm_mod_test.cc -- the host blocks of the continuous-phase transmitter (host/grhip_blocks.h) on a device:
// qa_frequency_modulator.py:35-49 and qa_cpm.py:36-84 as work() calls, the factory signatures of
// general/gr_frequency_modulator_fc.h:32, gr-digital/lib/digital_cpmmod_bc.h:36-38 and digital_gmskmod_bc.h:33-35, the
// handle against char_to_float -> (its own taps) -> frequency_modulator_fc cut at odd places in GRHIP_MODE_GENERIC,
// and the refusals.
#include <cmath>
#include <complex>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "grhip_blocks.h"

static_assert(std::is_same<decltype(&gr_make_frequency_modulator_fc), grhip_frequency_modulator_fc_sptr (*)(double, int)>::value, "");
static_assert(std::is_same<decltype(&digital_make_cpmmod_bc), grhip_cpmmod_bc_sptr (*)(int, float, unsigned, unsigned, double, int)>::value, "");
static_assert(std::is_same<decltype(&digital_make_gmskmod_bc), grhip_gmskmod_bc_sptr (*)(unsigned, double, unsigned, int)>::value, "");
static_assert(std::is_base_of<gr_sync_block, grhip_frequency_modulator_fc_blk>::value && std::is_base_of<gr_sync_interpolator, grhip_cpmmod_bc_blk>::value, "");
static_assert(!std::is_copy_constructible<grhip_cpmmod_bc_blk>::value, "");

template <class F> static bool throws(F f)
{
    try { f(); } catch (const std::exception &) { return true; }
    return false;
}

// work() over the n input items at `x`, `per` output items each, cut at 7 and 97 input items
template <class B, class I, class O> static std::vector<O> run(B blk, const std::vector<I> &x, int per)
{
    std::vector<O> y(x.size() * per);
    const size_t cuts[] = {0, 7 < x.size() ? 7 : x.size(), 97 < x.size() ? 97 : x.size(), x.size()};
    for (int c = 0; c < 3; ++c) {
        if (cuts[c + 1] == cuts[c]) continue;
        gr_vector_const_void_star in{x.data() + cuts[c]};
        gr_vector_void_star out{y.data() + cuts[c] * per};
        const int n = (int)(cuts[c + 1] - cuts[c]) * per;
        if (blk->work(n, in, out) != n) return {};
    }
    return y;
}

// qa_cpm.py:46-52: the symbol phases sink[sps * L - 1 :: sps] step by pi / 2 (mod 2 pi), to five places
static bool quarter_turns(const std::vector<gr_complex> &y, int sps, int L)
{
    int steps = 0;
    for (size_t i = sps * L - 1; i + sps < y.size(); i += sps, ++steps) {
        double d = std::fmod((double)std::arg(y[i + sps]) - (double)std::arg(y[i]), 2 * M_PI);
        if (d < 0) d += 2 * M_PI;
        if (std::fabs(d - M_PI / 2) > 0.5e-5) return false;
    }
    return steps > 0;
}

int main()
{
    if (!throws([] { digital_make_cpmmod_bc(5, 0.5f, 2, 4); }) || !throws([] { digital_make_cpmmod_bc(GRHIP_CPM_LREC, 0.5f, 0, 4); }) ||
        !throws([] { digital_make_gmskmod_bc(2, 0.3, 0); }) || !throws([] { grhip_make_gmsk_mod(1); }) ||
        !throws([] { grhip_cpm_phase_response_taps(GRHIP_CPM_LRC, 4097, 1); })) {
        std::printf("FAIL: a refusal was accepted\n");
        return 1;
    }
    for (int mode : {GRHIP_MODE_FAST, GRHIP_MODE_GENERIC}) {
        {   // qa_frequency_modulator.py:35-49
            const std::vector<float> src{0.25f, 0.5f, 0.25f, -0.25f, -0.5f, -0.25f};
            const double sum[] = {M_PI / 16, 3 * M_PI / 16, M_PI / 4, 3 * M_PI / 16, M_PI / 16, 0};
            auto fm = gr_make_frequency_modulator_fc(M_PI / 4);
            fm->set_mode(mode);
            const std::vector<gr_complex> y = run<decltype(fm), float, gr_complex>(fm, src, 1);
            for (size_t i = 0; i < src.size(); ++i)
                if (y.size() != src.size() || std::abs(std::complex<double>(y[i]) - std::polar(1.0, sum[i])) > 1e-5) { std::printf("FAIL: fm item %zu (mode %d)\n", i, mode); return 1; }
            if (fm->sensitivity() != (float)(M_PI / 4)) { std::printf("FAIL: sensitivity()\n"); return 1; }
        }
        const std::vector<char> ones(20, 1);
        for (int type : {GRHIP_CPM_LRC, GRHIP_CPM_LSRC, GRHIP_CPM_LREC, GRHIP_CPM_TFM}) {       // qa_cpm.py:36-70
            auto m = digital_make_cpmmod_bc(type, 0.5f, 2, 1);
            m->set_mode(mode);
            if (!quarter_turns(run<decltype(m), char, gr_complex>(m, ones, 2), 2, 1)) { std::printf("FAIL: phase shift of type %d (mode %d)\n", type, mode); return 1; }
            if (m->get_taps() != grhip_cpm_phase_response_taps(type, 2, 1)) { std::printf("FAIL: get_taps of type %d\n", type); return 1; }
        }
        auto g = digital_make_gmskmod_bc(2, 0.3, 5);                                             // qa_cpm.py:63-80
        g->set_mode(mode);
        if (!quarter_turns(run<decltype(g), char, gr_complex>(g, ones, 2), 2, 5)) { std::printf("FAIL: phase shift of gmskmod_bc (mode %d)\n", mode); return 1; }
        if (g->engine() != (mode == GRHIP_MODE_GENERIC ? 0 : 1)) { std::printf("FAIL: engine() in mode %d\n", mode); return 1; }
    }
    {   // gmsk_mod: 32 samples per byte at sps 4, 5 * sps - 1 taps, constant envelope; then the small blocks on its bits
        auto k = grhip_make_gmsk_mod(4, 0.35);
        k->set_mode(GRHIP_MODE_GENERIC);
        std::vector<unsigned char> bytes(120);
        for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = (unsigned char)(i * 37 + 11);
        const std::vector<gr_complex> y = run<decltype(k), unsigned char, gr_complex>(k, bytes, 32);
        if (y.size() != bytes.size() * 32 || k->samples_per_symbol() != 4 || k->get_taps().size() != 19) { std::printf("FAIL: gmsk_mod sizes\n"); return 1; }
        for (const gr_complex &v : y)
            if (std::fabs(std::abs(v) - 1.0f) > 1e-6f) { std::printf("FAIL: gmsk_mod is not constant envelope\n"); return 1; }
        auto b = gr_make_bytes_to_syms();
        const std::vector<float> s = run<decltype(b), unsigned char, float>(b, bytes, 8);
        auto c = gr_make_char_to_float();
        std::vector<char> sc(s.size());
        for (size_t i = 0; i < s.size(); ++i) sc[i] = (char)s[i];
        if (run<decltype(c), char, float>(c, sc, 1) != s) { std::printf("FAIL: char_to_float of bytes_to_syms\n"); return 1; }
        auto t = grhip_make_chunks_to_symbols_bf({-1.f, 1.f}, 1);
        std::vector<unsigned char> idx(s.size());
        for (size_t i = 0; i < s.size(); ++i) idx[i] = s[i] > 0;
        if (run<decltype(t), unsigned char, float>(t, idx, 1) != s) { std::printf("FAIL: chunks_to_symbols_bf\n"); return 1; }
    }
    std::printf("cpm_mod_test ok\n");
    return 0;
}
