// analytic_test -- drives grhip_hilbert_fc, grhip_filter_delay_fc and grhip_goertzel_fc (grhip_blocks.h) under the
// stand-in executor (grhip_executor.h) with its default chunking and compares what the block produced, bit for bit,
// with ONE call of the C ABI on the whole stream (GRHIP_MODE_GENERIC).  For tests/test_gpu_analytic.py.
//
//   analytic_test hilbert <ntaps> <in.bin> <out.bin>
//   analytic_test delay   <taps.bin> <in.bin> <out.bin>
//   analytic_test goertzel <rate> <len> <freq> <in.bin> <out.bin>
//   analytic_test errors
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

static std::vector<float> read_floats(const char *path)
{
    std::vector<float> v;
    FILE *f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    float buf[1 << 14];
    size_t n;
    while ((n = fread(buf, sizeof(float), 1 << 14, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static void write_file(const char *path, const std::vector<unsigned char> &b)
{
    FILE *fo = fopen(path, "wb");
    if (!fo || fwrite(b.data(), 1, b.size(), fo) != b.size()) throw std::runtime_error("cannot write output");
    fclose(fo);
}

static int same(const std::vector<unsigned char> &y, const std::vector<gr_complex> &one)
{
    if (y.size() != one.size() * sizeof(gr_complex) || memcmp(y.data(), one.data(), y.size())) {
        std::cout << "executor output differs from the single call (" << y.size() / sizeof(gr_complex) << " vs "
                  << one.size() << " items)\n";
        return 1;
    }
    std::cout << one.size() << " items equal\n";
    return 0;
}

static int errors()
{
    int fails = 0;
    try { grhip_make_hilbert_fc(1); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_filter_delay_fc(std::vector<float>()); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_goertzel_fc(8000, 0, 100.f); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_goertzel_fc(0, 64, 100.f); fails++; } catch (const std::invalid_argument &) {}
    grhip_hilbert_fc_sptr hb = grhip_make_hilbert_fc(50);
    if (hb->history() != 51 || hb->taps().size() != 51 || hb->relative_rate() != 1.0) fails++;
    if (hb->input_signature()->sizeof_stream_item(0) != sizeof(float) || hb->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex)) fails++;
    grhip_filter_delay_fc_sptr fd = grhip_make_filter_delay_fc(std::vector<float>(8, 0.5f));
    if (fd->history() != 8 || fd->input_signature()->max_streams() != 2 || fd->input_signature()->min_streams() != 1) fails++;
    grhip_goertzel_fc_sptr gz = grhip_make_goertzel_fc(8000, 400, 100.f);
    if (gz->decimation() != 400 || gz->history() != 1 || gz->relative_rate() != 1.0 / 400) fails++;
    std::cout << "errors test: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

int main(int argc, char **argv)
{
    try {
        const std::string what = argc > 1 ? argv[1] : "";
        if (what == "errors" && argc == 2) return errors();
        grhip_linear_flowgraph fg;                          // default chunking
        std::vector<unsigned char> y;
        std::vector<gr_complex> one;
        if (what == "hilbert" && argc == 5) {
            std::vector<float> x = read_floats(argv[3]);
            grhip_hilbert_fc_sptr b = grhip_make_hilbert_fc((unsigned)atoi(argv[2]));
            b->set_mode(GRHIP_MODE_GENERIC);
            fg.connect(b);
            y = fg.run(x.data(), x.size());
            grhip_hilbert_fc *h = nullptr;
            grhip_detail::check(grhip_hilbert_fc_create(&h, (unsigned)atoi(argv[2]), 0));
            grhip_detail::check(grhip_hilbert_fc_set_mode(h, GRHIP_MODE_GENERIC));
            std::vector<float> xh((size_t)grhip_hilbert_fc_history(h) - 1, 0.f);
            xh.insert(xh.end(), x.begin(), x.end());
            one.resize(x.size());
            grhip_detail::check(grhip_hilbert_fc_work(h, (int)x.size(), xh.data(), one.data()));
            grhip_hilbert_fc_destroy(h);
            write_file(argv[4], y);
        } else if (what == "delay" && argc == 5) {
            std::vector<float> taps = read_floats(argv[2]), x = read_floats(argv[3]);
            grhip_filter_delay_fc_sptr b = grhip_make_filter_delay_fc(taps);
            b->set_mode(GRHIP_MODE_GENERIC);
            fg.connect(b);
            y = fg.run(x.data(), x.size());
            grhip_filter_delay_fc *h = nullptr;
            grhip_detail::check(grhip_filter_delay_fc_create(&h, taps.data(), taps.size(), 0));
            grhip_detail::check(grhip_filter_delay_fc_set_mode(h, GRHIP_MODE_GENERIC));
            std::vector<float> xh(taps.size() - 1, 0.f);
            xh.insert(xh.end(), x.begin(), x.end());
            one.resize(x.size());
            grhip_detail::check(grhip_filter_delay_fc_work(h, (int)x.size(), xh.data(), nullptr, one.data()));
            grhip_filter_delay_fc_destroy(h);
            write_file(argv[4], y);
        } else if (what == "goertzel" && argc == 7) {
            const int rate = atoi(argv[2]), len = atoi(argv[3]);
            const float freq = (float)atof(argv[4]);
            std::vector<float> x = read_floats(argv[5]);
            grhip_goertzel_fc_sptr b = grhip_make_goertzel_fc(rate, len, freq);
            b->set_mode(GRHIP_MODE_GENERIC);
            fg.connect(b);
            y = fg.run(x.data(), x.size());
            grhip_goertzel_fc *h = nullptr;
            grhip_detail::check(grhip_goertzel_fc_create(&h, rate, len, freq, 0));
            grhip_detail::check(grhip_goertzel_fc_set_mode(h, GRHIP_MODE_GENERIC));
            one.resize(x.size() / (size_t)len);
            grhip_detail::check(grhip_goertzel_fc_work(h, (int)one.size(), x.data(), one.data()));
            grhip_goertzel_fc_destroy(h);
            write_file(argv[6], y);
        } else {
            std::cerr << "usage: " << argv[0] << " hilbert ntaps in out | delay taps in out | goertzel rate len freq in out | errors\n";
            return 2;
        }
        return same(y, one);
    } catch (const std::exception &e) {
        std::cerr << "analytic_test: " << e.what() << "\n";
        return 1;
    }
}
