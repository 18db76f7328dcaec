// frac_interp_test -- drives grhip_fractional_interpolator_{ff,cc} (grhip_blocks.h) through the stand-in executor
// (grhip_executor.h) in scheduler-style calls and writes what the block produced, for
// tests/test_gpu_fractional_interp.py.
//
//   frac_interp_test ff|cc <phase_shift> <interp_ratio> generic|fast <in.bin> <out.bin>
//   frac_interp_test errors
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
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

static int errors()
{
    int fails = 0;
    // gr_fractional_interpolator_ff.cc:44-47
    try { grhip_make_fractional_interpolator_ff(0.0f, 0.0f); fails++; }
    catch (const std::out_of_range &) {}
    try { grhip_make_fractional_interpolator_cc(0.0f, -1.0f); fails++; }
    catch (const std::out_of_range &) {}
    try { grhip_make_fractional_interpolator_ff(-0.1f, 1.0f); fails++; }
    catch (const std::out_of_range &) {}
    try { grhip_make_fractional_interpolator_cc(1.1f, 1.0f); fails++; }
    catch (const std::out_of_range &) {}
    try { grhip_make_fractional_interpolator_ff(0.0f, 2097152.0f); fails++; }       // the kernel's limit
    catch (const std::invalid_argument &) {}
    grhip_fractional_interpolator_ff_sptr f = grhip_make_fractional_interpolator_ff(1.0f, 1.25f);   // 1 is allowed
    if (f->history() != 1 || std::fabs(f->relative_rate() - 0.8) > 1e-12) fails++;
    if (f->mu() != 1.0f || f->interp_ratio() != 1.25f) fails++;
    gr_vector_int req(1);
    f->forecast(100, req);
    if (req[0] != 133) fails++;                                            // ceil(100 * 1.25 + 8)
    f->forecast(3, req);
    if (req[0] != 12) fails++;                                             // ceil(3.75 + 8)
    f->set_interp_ratio(0.3f);
    f->forecast(3, req);
    if (req[0] != 9 || f->interp_ratio() != 0.3f) fails++;                // 3 * 0.3f + 8 = 8.900001 in float
    f->set_mu(0.5f);
    if (f->mu() != 0.5f) fails++;
    try { f->set_mu(2.0f); fails++; }
    catch (const std::out_of_range &) {}
    try { f->set_interp_ratio(0.0f); fails++; }
    catch (const std::out_of_range &) {}
    if (f->mu() != 0.5f || f->interp_ratio() != 0.3f) fails++;            // refused values leave the block as it was
    std::cout << "errors test: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && std::string(argv[1]) == "errors") return errors();
        if (argc != 7) {
            std::cerr << "usage: " << argv[0] << " ff|cc phase_shift interp_ratio generic|fast in.bin out.bin\n";
            return 2;
        }
        const bool cplx = std::string(argv[1]) == "cc";
        const float phase = strtof(argv[2], nullptr), ratio = strtof(argv[3], nullptr);
        const int mode = std::string(argv[4]) == "generic" ? GRHIP_MODE_GENERIC : GRHIP_MODE_FAST;
        std::vector<unsigned char> xb = read_file(argv[5]);
        grhip_linear_flowgraph fg(1 << 16);
        size_t item;
        if (cplx) {
            grhip_fractional_interpolator_cc_sptr b = grhip_make_fractional_interpolator_cc(phase, ratio);
            b->set_mode(mode);
            fg.connect(b);
            item = sizeof(gr_complex);
        } else {
            grhip_fractional_interpolator_ff_sptr b = grhip_make_fractional_interpolator_ff(phase, ratio);
            b->set_mode(mode);
            fg.connect(b);
            item = sizeof(float);
        }
        std::vector<unsigned char> y = fg.run(xb.data(), xb.size() / item);
        FILE *fo = fopen(argv[6], "wb");
        if (!fo || fwrite(y.data(), 1, y.size(), fo) != y.size()) throw std::runtime_error("cannot write output");
        fclose(fo);
        std::cout << y.size() / item << " items\n";
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "frac_interp_test: " << e.what() << "\n";
        return 1;
    }
}
