// spectrum_test -- the spectrum-estimate blocks of grhip_blocks.h (complex_to_mag_squared, single_pole_iir_filter_ff,
// nlog10_ff, keep_one_in_n): that they report the reference's item sizes, history and relative_rate,
// throw what the reference's preconditions throw (std::out_of_range for alpha outside [0, 1]), and, run under the
// stand-in executor (grhip_executor.h), produce bit for bit what ONE call of the C ABI produces on the whole stream
// (GRHIP_MODE_GENERIC: the IIR's state and the keep-one countdown carry across the executor's calls).
// For tests/test_gpu_spectrum.py; no arguments.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

static int properties()
{
    int fails = 0;
    try { gr_make_single_pole_iir_filter_ff(1.5); fails++; } catch (const std::out_of_range &) {}
    try { gr_make_single_pole_iir_filter_ff(-0.5, 4); fails++; } catch (const std::out_of_range &) {}
    grhip_complex_to_mag_squared_sptr m = gr_make_complex_to_mag_squared(8);
    if (m->input_signature()->sizeof_stream_item(0) != 8 * sizeof(gr_complex) ||
        m->output_signature()->sizeof_stream_item(0) != 8 * sizeof(float) || m->history() != 1 || m->relative_rate() != 1.0) fails++;
    grhip_single_pole_iir_filter_ff_sptr f = gr_make_single_pole_iir_filter_ff(0.125);
    if (f->input_signature()->sizeof_stream_item(0) != sizeof(float) || f->history() != 1) fails++;
    try { f->set_taps(1.0001); fails++; } catch (const std::out_of_range &) {}
    {   // qa_single_pole_iir test_002, and set_taps keeps the state
        const float x[6] = {0, 1000, 2000, 3000, 4000, 5000};
        float y[6];
        gr_vector_const_void_star in(1, x);
        gr_vector_void_star out(1, y);
        if (f->work(6, in, out) != 6 || y[1] != 125.f || y[2] != 359.375f || y[3] != 689.453125f) fails++;
        f->set_taps(0.0);                                   // y stays at its last value
        const float last = y[5];
        if (f->work(2, in, out) != 2 || y[0] != last || y[1] != last) fails++;
    }
    grhip_nlog10_ff_sptr l = gr_make_nlog10_ff(10, 4, -3.f);
    if (l->output_signature()->sizeof_stream_item(0) != 4 * sizeof(float) || l->history() != 1) fails++;
    grhip_keep_one_in_n_sptr k = gr_make_keep_one_in_n(24, 5);
    if (k->input_signature()->sizeof_stream_item(0) != 24 || k->relative_rate() != 0.2) fails++;
    k->set_n(0);
    if (k->relative_rate() != 1.0) fails++;
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

template <class T>
static int same(const char *what, const std::vector<unsigned char> &y, const std::vector<T> &one)
{
    if (y.size() != one.size() * sizeof(T) || memcmp(y.data(), one.data(), y.size())) {
        std::cout << what << ": executor output differs from the single call (" << y.size() / sizeof(T) << " vs " << one.size() << " elements)\n";
        return 1;
    }
    std::cout << what << ": " << one.size() << " elements equal\n";
    return 0;
}

static int under_executor()
{
    int fails = 0;
    const int N = 256, F = 600;
    const size_t n = (size_t)N * F;
    unsigned lcg = 2463534242u;
    std::vector<gr_complex> z(n);
    std::vector<float> x(n);
    for (size_t i = 0; i < n; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        x[i] = (float)(lcg >> 8) / 8388608.f - 1.f;
        lcg = lcg * 1664525u + 1013904223u;
        z[i] = gr_complex(x[i], (float)(lcg >> 8) / 8388608.f - 1.f);
    }
    {   // the chain's last three stages as three blocks, small calls, against one call each of the C ABI
        grhip_linear_flowgraph fg(37);
        grhip_complex_to_mag_squared_sptr m = gr_make_complex_to_mag_squared(N);
        grhip_single_pole_iir_filter_ff_sptr f = gr_make_single_pole_iir_filter_ff(0.2, N);
        grhip_nlog10_ff_sptr l = gr_make_nlog10_ff(10, N, -12.5f);
        m->set_mode(GRHIP_MODE_GENERIC); f->set_mode(GRHIP_MODE_GENERIC); l->set_mode(GRHIP_MODE_GENERIC);
        fg.connect(m); fg.connect(f); fg.connect(l);
        std::vector<unsigned char> y = fg.run(z.data(), F);
        grhip_complex_to_mag_squared *hm = nullptr;
        grhip_single_pole_iir_filter_ff *hf = nullptr;
        grhip_nlog10_ff *hl = nullptr;
        grhip_detail::check(grhip_complex_to_mag_squared_create(&hm, N, 0));
        grhip_detail::check(grhip_single_pole_iir_filter_ff_create(&hf, 0.2, N, 0));
        grhip_detail::check(grhip_nlog10_ff_create(&hl, 10, N, -12.5f, 0));
        grhip_detail::check(grhip_single_pole_iir_filter_ff_set_mode(hf, GRHIP_MODE_GENERIC));
        std::vector<float> a(n), b(n), c(n);
        grhip_detail::check(grhip_complex_to_mag_squared_work(hm, F, z.data(), a.data()));
        grhip_detail::check(grhip_single_pole_iir_filter_ff_work(hf, F, a.data(), b.data()));
        grhip_detail::check(grhip_nlog10_ff_work(hl, F, b.data(), c.data()));
        grhip_complex_to_mag_squared_destroy(hm);
        grhip_single_pole_iir_filter_ff_destroy(hf);
        grhip_nlog10_ff_destroy(hl);
        fails += same("mag_squared -> single_pole_iir -> nlog10", y, c);
    }
    {
        grhip_linear_flowgraph fg(50);
        grhip_keep_one_in_n_sptr k = gr_make_keep_one_in_n(N * sizeof(float), 7);
        fg.connect(k);
        std::vector<unsigned char> y = fg.run(x.data(), F);
        std::vector<float> one;
        for (int i = 6; i < F; i += 7) one.insert(one.end(), x.begin() + (size_t)i * N, x.begin() + (size_t)(i + 1) * N);
        fails += same("keep_one_in_n", y, one);
    }
    return fails;
}

int main()
{
    try {
        return (properties() + under_executor()) ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "spectrum_test: " << e.what() << "\n";
        return 1;
    }
}
