// pfb_clock_sync_blk_test -- the pfb_clock_sync_ccf block of grhip_blocks.h: the reference's factory signature, four-output
// signature, history, setters and getters, and a flowgraph under the stand-in executor (grhip_executor.h): source ->
// the block in calls of at most 37 outputs -> sink.
//   * in GRHIP_MODE_GENERIC the block equals, bit for bit, a loop restated here from
//     gnuradio-core/src/lib/filter/gr_pfb_clock_sync_ccf.cc:351-427 on one linear input buffer, with
//     gr_fir_ccf_generic's two accumulators, on the library's banks;
//   * all four outputs, driven directly in two calls, equal the restated loop's;
//   * in GRHIP_MODE_FAST the loop ends within 4 arms of the same timing phase (the lock check of tests/test_gpu_pfb_clock_sync.py).
// For tests/test_gpu_host_pfb_clock_sync.py; no arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

namespace {

struct pcs_loop {           // gr_pfb_clock_sync_ccf.cc:52-98, :351-427
    int nf, tpf, isps, osps;
    float alpha, beta, k, rate_i, rate_f, max_dev, error = 0;
    std::vector<std::vector<float> > taps, dtaps;       // reversed, as gr_fir_ccf keeps them
    std::vector<gr_complex> out;
    std::vector<float> err, rate, ks;
    long consumed = 0;
    pcs_loop(double sps, float bw, const std::vector<float> &t, int nfilters, float init, float md, int osps_)
        : nf(nfilters), isps((int)floor(sps)), osps(osps_), k(init), max_dev(md)
    {
        const float damping = sqrtf(2.0f) / 2.0f;
        const float denom = (1.0 + 2.0 * damping * bw + bw * bw);
        alpha = (4 * damping * bw) / denom;
        beta = (4 * bw * bw) / denom;
        const float r = (sps - floor(sps)) * (double)nf;
        rate_i = (int)floor(r);
        rate_f = r - (float)rate_i;
        grhip_detail::check(grhip_pfb_clock_sync_taps(t.data(), (int)t.size(), nf, nullptr, nullptr, &tpf));
        std::vector<float> b((size_t)nf * tpf), d((size_t)nf * tpf);
        grhip_detail::check(grhip_pfb_clock_sync_taps(t.data(), (int)t.size(), nf, b.data(), d.data(), &tpf));
        for (int f = 0; f < nf; ++f) {
            taps.push_back(std::vector<float>(b.rbegin() + (size_t)(nf - 1 - f) * tpf, b.rbegin() + (size_t)(nf - f) * tpf));
            dtaps.push_back(std::vector<float>(d.rbegin() + (size_t)(nf - 1 - f) * tpf, d.rbegin() + (size_t)(nf - f) * tpf));
        }
    }
    static gr_complex fir(const std::vector<float> &t, const gr_complex *in)      // gr_fir_XXX_generic.cc.t:59-79
    {
        gr_complex acc0 = 0, acc1 = 0;
        unsigned i = 0, n = ((unsigned)t.size() / 2) * 2;
        for (; i < n; i += 2) {
            acc0 += t[i] * in[i];
            acc1 += t[i + 1] * in[i + 1];
        }
        for (; i < t.size(); i++) acc0 += t[i] * in[i];
        return acc0 + acc1;
    }
    void run(const std::vector<gr_complex> &x)
    {
        std::vector<gr_complex> in(tpf + isps - 1, gr_complex(0, 0));             // history = tpf + sps
        in.insert(in.end(), x.begin(), x.end());
        const int ninput = (int)in.size(), nrequired = ninput - tpf - osps;
        int i = 0, count = 0, filtnum = 0;
        out.assign(x.size() * osps + 64, 0); err.assign(out.size(), 0); rate.assign(out.size(), 0); ks.assign(out.size(), 0);
        while (count < nrequired) {
            for (int kk = 0; kk < osps; kk++) {
                filtnum = (int)floor(k);
                while (filtnum >= nf) { k -= nf; filtnum -= nf; count += 1; }
                while (filtnum < 0) { k += nf; filtnum += nf; count -= 1; }
                out[i + kk] = fir(taps[filtnum], &in[count + kk]);
                k = k + rate_i + rate_f;
                err[i] = error; rate[i] = rate_f; ks[i] = k;
            }
            const gr_complex diff = fir(dtaps[filtnum], &in[count]);
            const float error_r = out[i].real() * diff.real();
            const float error_i = out[i].imag() * diff.imag();
            error = (error_i + error_r) / 2.0;
            rate_f = rate_f + beta * error;
            k = k + alpha * error;
            const float x1 = fabsf(rate_f + max_dev), x2 = fabsf(rate_f - max_dev);
            rate_f = 0.5 * (x1 - x2);
            i += osps;
            count += isps;
        }
        consumed = count;
        out.resize(i); err.resize(i); rate.resize(i); ks.resize(i);
    }
};

template <class F> bool throws(F f)
{
    try { f(); } catch (const std::invalid_argument &) { return true; }
    return false;
}

int properties(const std::vector<float> &taps)
{
    int fails = 0;
    grhip_pfb_clock_sync_ccf_sptr b = gr_make_pfb_clock_sync_ccf(2.0, 0.0628f, taps);      // filter_size 32, init_phase 0, max dev 1.5, osps 1
    if (b->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || b->input_signature()->max_streams() != 1 ||
        b->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || b->output_signature()->sizeof_stream_item(1) != sizeof(float) ||
        b->output_signature()->sizeof_stream_item(3) != sizeof(float) || b->output_signature()->min_streams() != 1 ||
        b->output_signature()->max_streams() != 4 || b->history() != 23 + 2) fails++;
    const pcs_loop want(2.0, 0.0628f, taps, 32, 0, 1.5f, 1);
    if (b->get_alpha() != want.alpha || b->get_beta() != want.beta || b->get_loop_bandwidth() != 0.0628f ||
        b->get_damping_factor() != sqrtf(2.0f) / 2.0f || b->get_clock_rate() != 0.f || b->k() != 0.f || b->error() != 0.f || b->slips() != 0) fails++;
    const std::vector<std::vector<float> > t = b->get_taps(), d = b->get_diff_taps();
    if (t.size() != 32 || t[0].size() != 23 || t[3][2] != taps[3 + 2 * 32] || d.size() != 32 || d[0][0] != 0.f ||
        b->get_channel_taps(31)[22] != 0.f || b->get_diff_channel_taps(5) != d[5]) fails++;
    b->set_alpha(0.25f); b->set_beta(0.5f);
    if (b->get_alpha() != 0.25f || b->get_beta() != 0.5f) fails++;
    b->set_damping_factor(1.0f); b->set_loop_bandwidth(0.1f); b->set_max_rate_deviation(0.5f);
    if (b->get_damping_factor() != 1.0f || b->get_loop_bandwidth() != 0.1f) fails++;
    const float a = b->get_alpha();
    if (!throws([&] { b->set_loop_bandwidth(-1.f); }) || !throws([&] { b->set_damping_factor(1.5f); }) || !throws([&] { b->set_alpha(-0.1f); }) ||
        !throws([&] { b->set_beta(1.5f); }) || b->get_alpha() != a || b->get_loop_bandwidth() != 0.1f) fails++;
    if (!throws([&] { gr_make_pfb_clock_sync_ccf(2.0, -1.f, taps); }) || !throws([&] { gr_make_pfb_clock_sync_ccf(0.5, 0.06f, taps); }) ||
        !throws([&] { gr_make_pfb_clock_sync_ccf(2.0, 0.06f, taps, 0); }) || !throws([&] { gr_make_pfb_clock_sync_ccf(2.0, 0.06f, taps, 32, 0, 1.5f, 0); }) ||
        !throws([&] { gr_make_pfb_clock_sync_ccf(2.0, 0.06f, std::vector<float>(1, 1.f)); })) fails++;
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

int loop(const std::vector<float> &taps, double sps, int osps, float init)
{
    int fails = 0;
    const int n = 4001, L = 8;
    // QPSK through a root-raised-cosine pulse at 8 samples per symbol, read at 8 / sps (1 + 2e-3) samples apart
    const std::vector<float> rrc = grhip_firdes_root_raised_cosine_taps(1.0, L, 1.0, 0.35, 11 * L);
    const int nsym = (int)(n / sps) + 30;
    std::vector<gr_complex> sym(nsym), up((size_t)nsym * L + rrc.size() + 2, gr_complex(0, 0));
    unsigned lcg = 2463534242u;
    for (gr_complex &s : sym) {
        lcg = lcg * 1664525u + 1013904223u;
        const float re = (lcg >> 20) & 1 ? 0.70710678f : -0.70710678f;
        lcg = lcg * 1664525u + 1013904223u;
        s = gr_complex(re, (lcg >> 20) & 1 ? 0.70710678f : -0.70710678f);
    }
    for (int m = 0; m < nsym; ++m)
        for (size_t j = 0; j < rrc.size(); ++j) up[(size_t)m * L + j] += rrc[j] * sym[m];
    std::vector<gr_complex> x(n);
    double pw = 0;
    for (int i = 0; i < n; ++i) {
        const double at = i * (L / sps) * (1 + 2e-3) + 5 * L + 3.3;
        const int i0 = (int)at;
        const float fr = (float)(at - i0);
        x[i] = up[i0] * (1 - fr) + up[i0 + 1] * fr;
        pw += std::norm(x[i]);
    }
    const float g = (float)(1.0 / sqrt(pw / n));
    for (gr_complex &v : x) v *= g;                                               // unit power
    pcs_loop r(sps, 0.0628f, taps, 32, init, 1.5f, osps);
    r.run(x);
    grhip_pfb_clock_sync_ccf_sptr b = gr_make_pfb_clock_sync_ccf(sps, 0.0628f, taps, 32, init, 1.5f, osps);
    b->set_mode(GRHIP_MODE_GENERIC);
    grhip_linear_flowgraph fg(37);
    fg.connect(b);
    const std::vector<unsigned char> y = fg.run(x.data(), x.size());
    const size_t got = y.size() / sizeof(gr_complex);
    // the reference's input test allows for no carry and gives a few symbols more at the end of a stream
    bool same = got <= r.out.size() && got + (size_t)osps * 12 >= r.out.size() && got % osps == 0 && !memcmp(y.data(), r.out.data(), y.size()) &&
                b->slips() == 0;
    // all four outputs, two calls, the scheduler's history in front of each
    grhip_pfb_clock_sync_ccf_sptr b2 = gr_make_pfb_clock_sync_ccf(sps, 0.0628f, taps, 32, init, 1.5f, osps);
    b2->set_mode(GRHIP_MODE_GENERIC);
    const int hist = (int)b2->history() - 1;
    std::vector<gr_complex> in(hist, gr_complex(0, 0)), o((size_t)n * osps + 64);
    in.insert(in.end(), x.begin(), x.end());
    std::vector<float> e(o.size(), -7.f), rt(o.size(), -7.f), kk(o.size(), -7.f);
    int made = 0;
    for (int at = 0, m = 1500; at < n; at += m, m = n - at) {
        gr_vector_int ni(1, m + hist);
        gr_vector_const_void_star ins(1, in.data() + at);
        gr_vector_void_star outs{o.data() + made, e.data() + made, rt.data() + made, kk.data() + made};
        const int p = b2->general_work((int)o.size() - made, ni, ins, outs);
        if (p < 0 || b2->consumed() != m) same = false;
        made += p;
    }
    // (the flowgraph's last requests are too small to hold a symbol's outputs for sure, so it may end a few items earlier)
    same = same && (size_t)made >= got && (size_t)made <= r.out.size() && !memcmp(o.data(), r.out.data(), made * sizeof(gr_complex)) && e[made] == -7.f;
    for (int i = 0; i < made && same; i += osps)            // slot i of a symbol, and its copies behind it
        for (int c = 0; c < osps; ++c)
            same = same && !memcmp(&e[i + c], &r.err[i], 4) && !memcmp(&rt[i + c], &r.rate[i], 4) && !memcmp(&kk[i + c], &r.ks[i], 4);
    // fused products and tree sums settle on the same timing
    grhip_pfb_clock_sync_ccf_sptr b3 = gr_make_pfb_clock_sync_ccf(sps, 0.0628f, taps, 32, init, 1.5f, osps);
    b3->set_mode(GRHIP_MODE_FAST);
    grhip_linear_flowgraph fg3(37);
    fg3.connect(b3);
    const std::vector<unsigned char> y3 = fg3.run(x.data(), x.size());
    float off = std::fabs(b3->k() - b->k());                                    // in arms, around the wrap
    off = off < 32 - off ? off : 32 - off;
    same = same && y3.size() == y.size() && off <= 4.f && b3->slips() == 0;
    std::cout << "pfb_clock_sync_ccf sps " << sps << " osps " << osps << ": " << got << " of the restated loop's " << r.out.size()
              << (same ? " items, the four outputs equal the restated loop; " : " items: differs from the restated loop; ") << "rate "
              << b->get_clock_rate() << ", FAST's k within " << off << " arms\n";
    fails += same ? 0 : 1;
    return fails;
}

}  // namespace

int main()
{
    try {
        const std::vector<float> taps = grhip_firdes_root_raised_cosine_taps(32, 64, 1.0, 0.35, 704);
        const std::vector<float> taps25 = grhip_firdes_root_raised_cosine_taps(32, 80, 1.0, 0.35, 704);
        const int fails = properties(taps) + loop(taps, 2.0, 1, 16.f) + loop(taps25, 2.5, 2, 0.f);
        if (!fails) std::cout << "pfb_clock_sync_blk_test ok\n";
        return fails ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "pfb_clock_sync_blk_test: " << e.what() << "\n";
        return 1;
    }
}
