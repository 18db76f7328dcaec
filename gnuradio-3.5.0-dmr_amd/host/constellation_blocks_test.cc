// constellation_blocks_test -- the constellation classes and the blocks behind timing recovery of grhip_blocks.h: the
// reference's factory signatures, io signatures, getters, and small flowgraphs under the stand-in executor
// (grhip_executor.h): the source in pieces of uneven size, each run in calls of at most 37 items.
//   * constellation_receiver_cb in GRHIP_MODE_GENERIC equals, bit for bit, a loop restated here from
//     gr-digital/lib/digital_constellation_receiver_cb.cc:80-122 around the library's own host decision_maker_pe, with
//     the float-rounded double sine and cosine; its four outputs, driven directly, are symbol, error, phase, frequency;
//   * in the other modes it gives the same symbols, for a qpsk (angle form) and a 16-point rect (cartesian form) signal;
//   * receiver -> diff_decoder_bb -> map_bb -> unpack_k_bits_bb as a flowgraph gives, in uneven calls, the bytes of
//     constellation_demod_cb in one call, both engines;
//   * constellation_decoder_cb equals decision_maker, also for a two-dimensional constellation.
// For tests/test_gpu_host_constellation.py; no arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

namespace {

const double TWOPI = 2.0f * M_PI;       // gri_control_loop.cc:31
const float LOOP_BW = (float)(2 * M_PI / 100), FMIN = -0.25f, FMAX = 0.25f;

struct receiver_loop {      // digital_constellation_receiver_cb.cc:102-117 around gri_control_loop.cc:49-80
    float alpha, beta, phase = 0, freq = 0;
    grhip_constellation_sptr c;
    receiver_loop(grhip_constellation_sptr cons, float bw) : c(cons)
    {
        const float damping = sqrtf(2.0f) / 2.0f;
        const float denom = (1.0 + 2.0 * damping * bw + bw * bw);
        alpha = (4 * damping * bw) / denom;
        beta = (4 * bw * bw) / denom;
    }
    unsigned step(gr_complex in, float &error)
    {
        const gr_complex nco((float)cos((double)phase), (float)sin((double)phase));
        const gr_complex sample(nco.real() * in.real() - nco.imag() * in.imag(), nco.real() * in.imag() + nco.imag() * in.real());
        const unsigned k = c->decision_maker_pe(&sample, &error);
        freq = freq + beta * error;
        phase = phase + freq + alpha * error;
        while (phase > TWOPI) phase -= TWOPI;
        while (phase < -TWOPI) phase += TWOPI;
        if (freq > FMAX) freq = FMAX;
        else if (freq < FMIN) freq = FMIN;
        return k;
    }
};

template <class F> bool throws(F f)
{
    try { f(); } catch (const std::invalid_argument &) { return true; }
    return false;
}

std::vector<gr_complex> qam16()
{
    std::vector<gr_complex> p;      // qam.py make_differential_constellation(16, False)
    const float g[2] = {1 / 3.f, 1.f};
    for (int i = 0; i < 16; ++i) {
        const int y = i & 1, x = (i >> 1) & 1, quad = i >> 2;
        const gr_complex q[4] = {gr_complex(g[x], g[y]), gr_complex(-g[y], g[x]), gr_complex(-g[x], -g[y]), gr_complex(g[y], -g[x])};
        p.push_back(q[quad]);
    }
    return p;
}

// seeded symbols of the constellation, rotated by 0.15 rad + 0.01 rad/sample, a little deterministic noise
std::vector<gr_complex> signal(grhip_constellation_sptr c, int n)
{
    const std::vector<gr_complex> pts = c->points();
    std::vector<gr_complex> x(n);
    unsigned lcg = 2463534242u;
    for (int i = 0; i < n; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        const gr_complex p = pts[(lcg >> 20) % pts.size()];
        lcg = lcg * 1664525u + 1013904223u;
        const double nr = ((lcg >> 8) & 0xffff) / 65536.0 - 0.5;
        lcg = lcg * 1664525u + 1013904223u;
        const double ni = ((lcg >> 8) & 0xffff) / 65536.0 - 0.5;
        const double rot = -(0.15 + 0.01 * i);
        x[i] = gr_complex((float)(p.real() * cos(rot) - p.imag() * sin(rot) + 0.02 * nr), (float)(p.real() * sin(rot) + p.imag() * cos(rot) + 0.02 * ni));
    }
    return x;
}

template <class Item>
std::vector<unsigned char> in_pieces(const std::vector<gr_block_sptr> &chain, const std::vector<Item> &x, bool drain = true)
{
    const size_t pieces[] = {1000, 37, 1, 2999, 257};
    std::vector<unsigned char> y;
    size_t at = 0;
    for (int k = 0; at < x.size(); ++k) {
        const size_t m = std::min(k < 5 ? pieces[k] : (size_t)1301, x.size() - at);
        grhip_linear_flowgraph fg(37, drain);
        for (const gr_block_sptr &b : chain) fg.connect(b);
        const std::vector<unsigned char> part = fg.run(x.data() + at, m);
        y.insert(y.end(), part.begin(), part.end());
        at += m;
    }
    return y;
}

int properties()
{
    int fails = 0;
    grhip_constellation_sptr q = digital_make_constellation_qpsk(), d = digital_make_constellation_dqpsk(), b = digital_make_constellation_bpsk(),
                             p8 = digital_make_constellation_8psk();
    if (q->arity() != 4 || q->bits_per_symbol() != 2 || q->rotational_symmetry() != 4 || q->dimensionality() != 1 || q->apply_pre_diff_code() ||
        !d->apply_pre_diff_code() || d->pre_diff_code() != std::vector<unsigned int>({0, 1, 3, 2}) || b->arity() != 2 || p8->arity() != 8 ||
        p8->bits_per_symbol() != 3 || q->points().size() != 4) fails++;
    const gr_complex s(0.5f, -0.5f);
    float pe = 1;
    if (q->decision_maker(&s) != 1 || d->decision_maker(&s) != 3 || b->decision_maker(&s) != 1 || q->decision_maker_pe(&s, &pe) != 1 || fabsf(pe) > 1e-6f) fails++;
    grhip_constellation_sptr r = digital_make_constellation_rect(qam16(), {}, 4, 4, 4, 2 / 3.f, 2 / 3.f);
    grhip_constellation_sptr c2 = digital_make_constellation_calcdist({gr_complex(1, 0), gr_complex(1, 0), gr_complex(-1, 0), gr_complex(-1, 0)}, {}, 1, 2);
    if (r->arity() != 16 || r->bits_per_symbol() != 4 || c2->arity() != 2 || c2->dimensionality() != 2) fails++;
    if (!throws([&] { digital_make_constellation_calcdist(std::vector<gr_complex>(257), {}, 1, 1); }) ||
        !throws([&] { digital_make_constellation_calcdist(std::vector<gr_complex>(4), {0, 1, 2}, 1, 1); }) ||
        !throws([&] { digital_make_constellation_psk(std::vector<gr_complex>(4), {}, 0); }) ||
        !throws([&] { digital_make_constellation_receiver_cb(c2, LOOP_BW, FMIN, FMAX); }) || !throws([&] { gr_make_diff_decoder_bb(0); })) fails++;
    grhip_constellation_receiver_cb_sptr rx = digital_make_constellation_receiver_cb(q, LOOP_BW, FMIN, FMAX);
    if (rx->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || rx->output_signature()->sizeof_stream_item(0) != 1 ||
        rx->output_signature()->sizeof_stream_item(1) != sizeof(float) || rx->output_signature()->sizeof_stream_item(3) != sizeof(float) ||
        rx->output_signature()->min_streams() != 1 || rx->output_signature()->max_streams() != 4 || rx->history() != 1) fails++;
    const receiver_loop want(q, LOOP_BW);
    if (rx->get_loop_bandwidth() != LOOP_BW || rx->get_alpha() != want.alpha || rx->get_beta() != want.beta || rx->get_phase() != 0.f) fails++;
    rx->set_frequency(2.f);
    if (rx->get_frequency() != FMIN || rx->form() != 2) fails++;
    rx->set_mode(GRHIP_MODE_GENERIC);
    if (rx->form() != 0 || digital_make_constellation_receiver_cb(r, LOOP_BW, FMIN, FMAX)->form() != 1) fails++;
    if (!throws([&] { rx->set_alpha(2.f); }) || !throws([&] { digital_make_constellation_receiver_cb(q, -1.f, FMIN, FMAX); })) fails++;
    grhip_diff_decoder_bb_sptr dd = gr_make_diff_decoder_bb(4);
    grhip_constellation_decoder_cb_sptr dec = digital_make_constellation_decoder_cb(c2);
    grhip_constellation_demod_cb_sptr dm = grhip_make_constellation_demod_cb(p8, LOOP_BW, FMIN, FMAX);
    if (dd->history() != 2 || dec->relative_rate() != 0.5 || dm->interpolation() != 3 || dm->output_multiple() != 3 || dm->engine() != 1) fails++;
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

int receiver()
{
    int fails = 0;
    const int n = 6037;
    grhip_constellation_sptr cons[2] = {digital_make_constellation_qpsk(), digital_make_constellation_rect(qam16(), {}, 4, 4, 4, 2 / 3.f, 2 / 3.f)};
    for (grhip_constellation_sptr c : cons) {
        const std::vector<gr_complex> x = signal(c, n);
        receiver_loop r(c, LOOP_BW);
        std::vector<unsigned char> want(n);
        std::vector<float> we(n), wp(n), wf(n);
        for (int i = 0; i < n; ++i) { want[i] = (unsigned char)r.step(x[i], we[i]); wp[i] = r.phase; wf[i] = r.freq; }
        grhip_constellation_receiver_cb_sptr b = digital_make_constellation_receiver_cb(c, LOOP_BW, FMIN, FMAX);
        b->set_mode(GRHIP_MODE_GENERIC);
        const std::vector<unsigned char> y = in_pieces({b}, x);
        const float ph = b->get_phase(), fr = b->get_frequency();
        bool same = y == want && !memcmp(&ph, &r.phase, 4) && !memcmp(&fr, &r.freq, 4);
        // the four outputs, one call
        grhip_constellation_receiver_cb_sptr b2 = digital_make_constellation_receiver_cb(c, LOOP_BW, FMIN, FMAX);
        b2->set_mode(GRHIP_MODE_GENERIC);
        std::vector<unsigned char> s(n);
        std::vector<float> e(n), p(n), f(n);
        gr_vector_int ni(1, n);
        gr_vector_const_void_star in(1, x.data());
        gr_vector_void_star out{s.data(), e.data(), p.data(), f.data()};
        same = same && b2->general_work(n, ni, in, out) == n && b2->consumed() == n && s == want && !memcmp(e.data(), we.data(), 4 * n) &&
               !memcmp(p.data(), wp.data(), 4 * n) && !memcmp(f.data(), wf.data(), 4 * n);
        // the fast forms decide the same symbols
        grhip_constellation_receiver_cb_sptr b3 = digital_make_constellation_receiver_cb(c, LOOP_BW, FMIN, FMAX);
        const std::vector<unsigned char> yf = in_pieces({b3}, x);
        same = same && yf == want;
        std::cout << "constellation_receiver_cb, " << c->arity() << " points: " << n
                  << (same ? " items, the four outputs and the state equal; form " : " items: differs from the restated loop; form ") << b3->form() << "\n";
        fails += same ? 0 : 1;
    }
    return fails;
}

int tail()
{
    int fails = 0;
    const int n = 6037;
    grhip_constellation_sptr cons[2] = {digital_make_constellation_dqpsk(), digital_make_constellation_8psk()};
    for (grhip_constellation_sptr c : cons) {
        const std::vector<gr_complex> x = signal(c, n);
        std::vector<gr_block_sptr> chain = {digital_make_constellation_receiver_cb(c, LOOP_BW, FMIN, FMAX), gr_make_diff_decoder_bb(c->arity())};
        if (c->apply_pre_diff_code()) {
            const std::vector<unsigned int> code = c->pre_diff_code();
            std::vector<int> inv(code.size());
            for (size_t i = 0; i < code.size(); ++i) inv[code[i]] = (int)i;     // invert_code of a permutation
            chain.push_back(gr_make_map_bb(inv));
        }
        chain.push_back(grhip_make_unpack_k_bits_bb(c->bits_per_symbol()));
        const std::vector<unsigned char> row = in_pieces(chain, x, false);    // the interpolators take whole output multiples
        bool same = row.size() == (size_t)n * c->bits_per_symbol();
        for (int engine : {1, 0}) {
            grhip_constellation_demod_cb_sptr dm = grhip_make_constellation_demod_cb(c, LOOP_BW, FMIN, FMAX, true, true);
            dm->set_engine(engine);
            std::vector<unsigned char> y(row.size());
            gr_vector_const_void_star in(1, x.data());
            gr_vector_void_star out(1, y.data());
            same = same && dm->work((int)y.size(), in, out) == (int)y.size() && y == row;
            same = same && in_pieces({grhip_make_constellation_demod_cb(c, LOOP_BW, FMIN, FMAX, true, true)}, x, false) == row;
        }
        std::cout << "constellation_demod_cb, " << c->arity() << " points: " << (same ? "both engines equal the four blocks in a row" : "FAIL") << "\n";
        fails += same ? 0 : 1;
    }
    return fails;
}

int decoder()
{
    int fails = 0;
    grhip_constellation_sptr c2 = digital_make_constellation_calcdist(
        {gr_complex(1, 0), gr_complex(1, 0), gr_complex(1, 0), gr_complex(-1, 0), gr_complex(-1, 0), gr_complex(1, 0), gr_complex(-1, 0), gr_complex(-1, 0)}, {}, 1, 2);
    grhip_constellation_sptr cons[3] = {digital_make_constellation_8psk(), digital_make_constellation_rect(qam16(), {}, 4, 4, 4, 2 / 3.f, 2 / 3.f), c2};
    for (grhip_constellation_sptr c : cons) {
        const std::vector<gr_complex> x = signal(digital_make_constellation_8psk(), 4098);
        const unsigned d = c->dimensionality();
        std::vector<unsigned char> want(x.size() / d);
        for (size_t i = 0; i < want.size(); ++i) want[i] = (unsigned char)c->decision_maker(&x[i * d]);
        grhip_linear_flowgraph fg(37);       // one run: a piece of odd length would leave half an item behind
        fg.connect(digital_make_constellation_decoder_cb(c));
        const bool same = fg.run(x.data(), x.size()) == want;
        std::cout << "constellation_decoder_cb, dimensionality " << d << ": " << (same ? "equals decision_maker" : "FAIL") << "\n";
        fails += same ? 0 : 1;
    }
    return fails;
}

}  // namespace

int main()
{
    try {
        const int fails = properties() + receiver() + tail() + decoder();
        if (!fails) std::cout << "constellation_blocks_test ok\n";
        return fails ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "constellation_blocks_test: " << e.what() << "\n";
        return 1;
    }
}
