// fft_real_test -- drives grhip_fft_filter_fff and grhip_fft_vfc (grhip_blocks.h) under the stand-in executor
// (grhip_executor.h) in scheduler-sized calls and writes what the block produced, for tests/test_gpu_fft_real.py.
//
//   fft_real_test filter <decimation> <max_noutput> <taps.bin> <in.bin> <out.bin>
//   fft_real_test retap  <decimation> <max_noutput> <taps1.bin> <taps2.bin> <in.bin> <out.bin>
//   fft_real_test vfc    <fft_size>   <max_noutput> <window.bin> <in.bin> <out.bin>
//   fft_real_test errors
// filter: whole output multiples only (the reference's scheduler never asks the block for less).  retap: the stream's
// first half through taps1, then set_taps(taps2): the next work() returns 0 and changes the output multiple, the second
// half then goes through what is a fresh filter; prints the two output multiples.  vfc: an empty window file = no window.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

static std::vector<unsigned char> read_file(const char *path)
{
    std::vector<unsigned char> v;
    FILE *f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static std::vector<float> read_floats(const char *path)
{
    std::vector<unsigned char> b = read_file(path);
    std::vector<float> v(b.size() / 4);
    memcpy(v.data(), b.data(), v.size() * 4);
    return v;
}

static void write_file(const char *path, const std::vector<unsigned char> &b)
{
    FILE *fo = fopen(path, "wb");
    if (!fo || fwrite(b.data(), 1, b.size(), fo) != b.size()) throw std::runtime_error("cannot write output");
    fclose(fo);
}

static int errors()
{
    int fails = 0;
    const std::vector<float> taps(30, 0.5f);
    try { grhip_make_fft_filter_fff(0, taps); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_fft_filter_fff(1, std::vector<float>()); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_fft_vfc(8, false, std::vector<float>()); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_fft_vfc(0, true, std::vector<float>()); fails++; } catch (const std::out_of_range &) {}
    grhip_fft_filter_fff_sptr f = grhip_make_fft_filter_fff(3, taps);          // fftsize 64, nsamples 35
    if (f->history() != 1 || f->output_multiple() != 35 || f->decimation() != 3 || f->relative_rate() != 1.0 / 3) fails++;
    if (f->input_signature()->sizeof_stream_item(0) != sizeof(float) || f->output_signature()->sizeof_stream_item(0) != sizeof(float)) fails++;
    grhip_fft_vfc_sptr v = grhip_make_fft_vfc(8, true, std::vector<float>());
    if (v->input_signature()->sizeof_stream_item(0) != 8 * sizeof(float) ||
        v->output_signature()->sizeof_stream_item(0) != 8 * sizeof(gr_complex)) fails++;
    if (v->set_window(std::vector<float>(3, 1.f))) fails++;                    // wrong size: refused (gr_fft_vfc.cc:112-117)
    if (!v->set_window(std::vector<float>(8, 1.f)) || !v->set_window(std::vector<float>())) fails++;
    std::cout << "errors test: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && std::string(argv[1]) == "errors") return errors();
        const std::string what = argc > 1 ? argv[1] : "";
        if (!((what == "filter" && argc == 7) || (what == "retap" && argc == 8) || (what == "vfc" && argc == 7))) {
            std::cerr << "usage: " << argv[0] << " filter D max taps in out | retap D max taps1 taps2 in out | vfc N max window in out | errors\n";
            return 2;
        }
        const int a = atoi(argv[2]), max_noutput = atoi(argv[3]);
        std::vector<unsigned char> y;
        if (what == "vfc") {
            std::vector<unsigned char> xb = read_file(argv[5]);
            grhip_linear_flowgraph fg(max_noutput, false);
            fg.connect(grhip_make_fft_vfc(a, true, read_floats(argv[4])));
            y = fg.run(xb.data(), xb.size() / (sizeof(float) * (size_t)a));
            write_file(argv[6], y);
        } else if (what == "filter") {
            std::vector<unsigned char> xb = read_file(argv[5]);
            grhip_linear_flowgraph fg(max_noutput, false);
            fg.connect(grhip_make_fft_filter_fff(a, read_floats(argv[4])));
            y = fg.run(xb.data(), xb.size() / sizeof(float));
            write_file(argv[6], y);
        } else {
            std::vector<unsigned char> xb = read_file(argv[6]);
            const size_t n = xb.size() / sizeof(float), half = n / 2;
            grhip_fft_filter_fff_sptr f = grhip_make_fft_filter_fff(a, read_floats(argv[4]));
            const int m1 = f->output_multiple();
            grhip_linear_flowgraph fg(max_noutput, false);
            fg.connect(f);
            y = fg.run(xb.data(), half);
            f->set_taps(read_floats(argv[5]));
            // the executor calls the block again after the work() that returns 0 (the new output multiple then holds)
            std::vector<unsigned char> y2 = fg.run(xb.data() + half * sizeof(float), n - half);
            std::cout << "multiples " << m1 << " " << f->output_multiple() << " first " << y.size() / sizeof(float) << "\n";
            y.insert(y.end(), y2.begin(), y2.end());
            write_file(argv[7], y);
        }
        std::cout << y.size() << " bytes\n";
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "fft_real_test: " << e.what() << "\n";
        return 1;
    }
}
