// constellation.h -- the constellation objects of gr-digital/lib/digital_constellation.{h,cc} in the reference's types.
// Host arithmetic only: no HIP, so host/constellation_test.cc runs it under the sanitizers, and the two decision
// entries of the C ABI need no device.  The free functions marked CONST_HD are the decisions themselves; under hipcc
// they are also device functions, so the kernels of constellation.hip decide with the same text.
//
// One struct holds every kind; what a kind computes is spelled where the reference spells it (the line numbers are
// digital_constellation.cc's).  A create function returns false where the reference throws std::runtime_error, and
// where one of the deviations below refuses an argument; `why` then says which.
//
// Deviations (include/grhip.h states them at the entries):
//   * the arity is at most CONST_MAX_ARITY = 256: the receiver's and the decoder's output item is a byte;
//   * n_sectors (psk), real_sectors * imag_sectors (rect) are at least 1 and at most CONST_MAX_SECTORS = 16384;
//   * a sample that is not finite gets a defined sector: the reference converts a NaN or an out-of-range double to
//     int, which is undefined.  Here a NaN position is sector 0 and every index is clamped to the table;
//   * arg(), cos() and sin() of a float are the float-rounded double functions here ((float)atan2((double)im,
//     (double)re) and so on), as the device's GENERIC mode has them: glibc's atan2f, cosf and sinf are within an ulp
//     of these but not reproducible from one library version to the next;
//   * rect's sector widths must be finite and not zero, every point finite;
//   * dimensionality above 1 is taken by calcdist only (the other kinds have none), and decision_maker_pe then reads
//     d_constellation[index + d] as the reference does (:121), which stays inside the table for every index.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define CONST_HD __host__ __device__ inline
#else
#define CONST_HD inline
#endif

namespace grhip {

constexpr unsigned CONST_MAX_ARITY = 256;
constexpr unsigned CONST_MAX_SECTORS = 16384;
constexpr double CONST_TWOPI = 2 * 3.14159265358979323846;     // digital_constellation.cc:38 `#define M_TWOPI (2*M_PI)`
constexpr double CONST_SQRT_TWO = 0.707107;                     // :39

enum ConstellationKind { CONST_BPSK = 0, CONST_QPSK, CONST_DQPSK, CONST_8PSK, CONST_CALCDIST, CONST_PSK, CONST_RECT };

struct cfloat {
    float re, im;
};

// gr_complex * gr_complex as g++ forms it without -ffast-math: four products, a difference and a sum, and the
// recovery of C99 Annex G.5.1 where both come out NaN (libgcc's __mulsc3)
CONST_HD cfloat cmul(cfloat x, cfloat y)
{
    float a = x.re, b = x.im, c = y.re, d = y.im;
    const float ac = a * c, bd = b * d, ad = a * d, bc = b * c;
    cfloat r = {ac - bd, ad + bc};
    if (r.re != r.re && r.im != r.im) {
        bool recalc = false;
        if (std::isinf(a) || std::isinf(b)) {
            a = std::copysign(std::isinf(a) ? 1.f : 0.f, a);
            b = std::copysign(std::isinf(b) ? 1.f : 0.f, b);
            if (c != c) c = std::copysign(0.f, c);
            if (d != d) d = std::copysign(0.f, d);
            recalc = true;
        }
        if (std::isinf(c) || std::isinf(d)) {
            c = std::copysign(std::isinf(c) ? 1.f : 0.f, c);
            d = std::copysign(std::isinf(d) ? 1.f : 0.f, d);
            if (a != a) a = std::copysign(0.f, a);
            if (b != b) b = std::copysign(0.f, b);
            recalc = true;
        }
        if (!recalc && (std::isinf(ac) || std::isinf(bd) || std::isinf(ad) || std::isinf(bc))) {
            if (a != a) a = std::copysign(0.f, a);
            if (b != b) b = std::copysign(0.f, b);
            if (c != c) c = std::copysign(0.f, c);
            if (d != d) d = std::copysign(0.f, d);
            recalc = true;
        }
        if (recalc) {
            r.re = INFINITY * (a * c - b * d);
            r.im = INFINITY * (a * d + b * c);
        }
    }
    return r;
}

CONST_HD float arg_f(float im, float re) { return (float)atan2((double)im, (double)re); }
CONST_HD float cos_f(float x) { return (float)cos((double)x); }
CONST_HD float sin_f(float x) { return (float)sin((double)x); }
// one IEEE float division (hipcc may otherwise pick a faster one on the device)
CONST_HD float div_f(float a, float b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// a double position -> an index in 0 .. n-1; NaN -> 0 (the deviation above).  For every value the reference's
// int(...) and its two clamps (:306-309) define, this is what they give.
CONST_HD unsigned clamp_sector(double v, unsigned n)
{
    if (!(v > 0)) return 0;                     // negative, zero, -0 or NaN; int() truncates (-1, 0) to 0 as well
    if (v >= (double)n) return n - 1;
    return (unsigned)(int)v;
}

// :355-365: a float arg, a float width from a double, floor(phase/width + 0.5) in double
CONST_HD unsigned psk_sector_of(float re, float im, unsigned n_sectors)
{
    const float phase = arg_f(im, re);
    const float width = (float)(CONST_TWOPI / n_sectors);
    double s = floor(div_f(phase, width) + 0.5);
    if (s != s) return 0;
    if (s < 0) s += n_sectors;
    return clamp_sector(s, n_sectors);
}

// :305-309 and :311-315: int(v / width + n / 2.0) and the two clamps
CONST_HD unsigned rect_axis(float v, float width, unsigned n) { return clamp_sector(div_f(v, width) + n / 2.0, n); }

CONST_HD unsigned decide_bpsk(float re, float) { return re > 0; }                             // :394-397
CONST_HD unsigned decide_qpsk(float re, float im) { return 2 * (im > 0) + (re > 0); }         // :434-438
CONST_HD unsigned decide_dqpsk(float re, float im)                                            // :493-512
{
    return re > 0 ? (im > 0 ? 0x0 : 0x3) : (im > 0 ? 0x1 : 0x2);
}
CONST_HD unsigned decide_8psk(float re, float im)                                             // :539-554
{
    unsigned ret = 0;
    if (fabsf(re) <= fabsf(im)) ret = 4;
    if (re <= 0) ret |= 1;
    if (im <= 0) ret |= 2;
    return ret;
}

// get_closest_point (:96-113) over `arity` points of `dim` samples: float norms, the first strict minimum
CONST_HD unsigned closest_point(const cfloat *points, unsigned arity, unsigned dim, const cfloat *sample)
{
    unsigned min_index = 0;
    float min_d = 0;
    for (unsigned j = 0; j < arity; ++j) {
        float dist = 0;                                          // get_distance, :86-94
        for (unsigned i = 0; i < dim; ++i) {
            const cfloat p = points[(size_t)j * dim + i];
            const float dr = sample[i].re - p.re, di = sample[i].im - p.im;
            dist += dr * dr + di * di;
        }
        if (j == 0 || dist < min_d) { min_d = dist; min_index = j; }
    }
    return min_index;
}

struct Constellation {
    int kind = CONST_CALCDIST;
    std::vector<cfloat> points;                 // d_constellation: arity * dimensionality
    std::vector<unsigned> pre_diff;             // d_pre_diff_code
    bool apply_pre_diff = false;
    unsigned rot_sym = 0, dim = 1, arity = 0;
    unsigned n_sectors = 0, n_real = 0, n_imag = 0;
    float w_real = 0.f, w_imag = 0.f;
    std::vector<unsigned> sector_values;
    const char *why = "";

    bool refuse(const char *w) { why = w; return false; }

    // the base constructor (:43-59) and calc_arity (:203-209)
    bool base(const cfloat *pts, size_t npts, const unsigned *code, size_t ncode, unsigned rs, unsigned dimensionality)
    {
        if (dimensionality < 1) return refuse("the dimensionality must be at least 1");
        if (npts && !pts) return refuse("null points");
        if (ncode && !code) return refuse("null pre-diff code");
        if (ncode != 0 && ncode != npts) return refuse("The constellation and pre-diff code must be of the same length.");
        if (npts % dimensionality != 0) return refuse("Constellation vector size must be a multiple of the dimensionality.");
        if (npts / dimensionality < 1) return refuse("a constellation needs at least one point");
        if (npts / dimensionality > CONST_MAX_ARITY) return refuse("at most 256 points: a symbol is a byte");
        points.assign(pts, pts + npts);
        pre_diff.assign(code, code + ncode);
        apply_pre_diff = ncode != 0;
        rot_sym = rs; dim = dimensionality; arity = (unsigned)(npts / dimensionality);
        return true;
    }

    void fixed(int k, std::vector<cfloat> pts, std::vector<unsigned> code, bool apply, unsigned rs)
    {
        kind = k; points = std::move(pts); pre_diff = std::move(code); apply_pre_diff = apply;
        rot_sym = rs; dim = 1; arity = (unsigned)points.size();
    }

    void make_bpsk() { fixed(CONST_BPSK, {{-1, 0}, {1, 0}}, {}, false, 2); }    // :383-391
    void make_qpsk()                                                             // :406-431
    {
        const float s = (float)CONST_SQRT_TWO;
        // the default constructor leaves d_apply_pre_diff_code false (:62) and this one does not set it
        fixed(CONST_QPSK, {{-s, -s}, {s, -s}, {-s, s}, {s, s}}, {0x0, 0x2, 0x3, 0x1}, false, 4);
    }
    void make_dqpsk()                                                            // :468-490
    {
        const float s = (float)CONST_SQRT_TWO;
        fixed(CONST_DQPSK, {{s, s}, {-s, s}, {-s, -s}, {s, -s}}, {0x0, 0x1, 0x3, 0x2}, true, 4);
    }
    void make_8psk()                                                             // :520-536
    {
        const float angle = (float)(3.14159265358979323846 / 8.0);
        static const int mult[8] = {1, 7, 15, 9, 3, 5, 13, 11};
        std::vector<cfloat> p(8);
        // cos(i*angle) on a float product is the float overload
        for (int i = 0; i < 8; ++i) p[i] = cfloat{cos_f(mult[i] * angle), sin_f(mult[i] * angle)};
        fixed(CONST_8PSK, p, {}, false, 8);
    }
    bool make_calcdist(const cfloat *pts, size_t npts, const unsigned *code, size_t ncode, unsigned rs, unsigned dimensionality)
    {
        kind = CONST_CALCDIST;
        return base(pts, npts, code, ncode, rs, dimensionality);
    }
    bool make_psk(const cfloat *pts, size_t npts, const unsigned *code, size_t ncode, unsigned sectors)     // :346-352
    {
        kind = CONST_PSK;
        if (sectors < 1 || sectors > CONST_MAX_SECTORS) return refuse("1 .. 16384 sectors");
        if (!base(pts, npts, code, ncode, (unsigned)npts, 1)) return false;
        n_sectors = sectors;
        find_sector_values();
        return true;
    }
    bool make_rect(const cfloat *pts, size_t npts, const unsigned *code, size_t ncode, unsigned rs, unsigned real_sectors,
                   unsigned imag_sectors, float width_real, float width_imag)                                // :287-297
    {
        kind = CONST_RECT;
        if (real_sectors < 1 || imag_sectors < 1 || (unsigned long long)real_sectors * imag_sectors > CONST_MAX_SECTORS)
            return refuse("1 .. 16384 sectors");
        if (!std::isfinite(width_real) || !std::isfinite(width_imag) || width_real == 0 || width_imag == 0)
            return refuse("the sector widths must be finite and not zero");
        if (!base(pts, npts, code, ncode, rs, 1)) return false;
        for (const cfloat &p : points)
            if (!std::isfinite(p.re) || !std::isfinite(p.im)) return refuse("the points must be finite");
        n_real = real_sectors; n_imag = imag_sectors; w_real = width_real; w_imag = width_imag;
        n_sectors = real_sectors * imag_sectors;
        find_sector_values();
        return true;
    }

    unsigned bits_per_symbol() const    // digital_constellation.h: floor(log(double(size))/dimensionality/log(2.0))
    {
        return (unsigned)std::floor(std::log((double)points.size()) / dim / std::log(2.0));
    }

    unsigned get_closest_point(const cfloat *sample) const { return closest_point(points.data(), arity, dim, sample); }
    unsigned psk_sector(const cfloat *sample) const { return psk_sector_of(sample->re, sample->im, n_sectors); }
    unsigned rect_sector(const cfloat *sample) const                                          // :300-319
    {
        return rect_axis(sample->re, w_real, n_real) * n_imag + rect_axis(sample->im, w_imag, n_imag);
    }

    unsigned calc_sector_value(unsigned sector) const
    {
        cfloat c;
        if (kind == CONST_PSK) {                                 // :368-374
            const float phase = (float)(sector * CONST_TWOPI / n_sectors);
            c = cfloat{cos_f(phase), sin_f(phase)};
        } else {                                                 // :322-333
            const unsigned rs = (unsigned)((float)sector / n_imag);
            const unsigned is = sector - rs * n_imag;
            c = cfloat{(float)((rs + 0.5 - n_real / 2.0) * w_real), (float)((is + 0.5 - n_imag / 2.0) * w_imag)};
        }
        return get_closest_point(&c);
    }

    void find_sector_values()                                    // :262-270
    {
        sector_values.clear();
        for (unsigned i = 0; i < n_sectors; ++i) sector_values.push_back(calc_sector_value(i));
    }

    unsigned decision_maker(const cfloat *sample) const
    {
        const float re = sample->re, im = sample->im;
        switch (kind) {
        case CONST_BPSK: return decide_bpsk(re, im);
        case CONST_QPSK: return decide_qpsk(re, im);
        case CONST_DQPSK: return decide_dqpsk(re, im);
        case CONST_8PSK: return decide_8psk(re, im);
        case CONST_PSK: return sector_values[psk_sector(sample)];                // :254-260
        case CONST_RECT: return sector_values[rect_sector(sample)];
        default: return get_closest_point(sample);                               // :238-242
        }
    }

    unsigned decision_maker_pe(const cfloat *sample, float *phase_error) const   // :115-123
    {
        const unsigned index = decision_maker(sample);
        float pe = 0;
        for (unsigned d = 0; d < dim; ++d) {
            const cfloat p = points[index + d];
            const cfloat z = cmul(sample[d], cfloat{p.re, -p.im});
            pe += -arg_f(z.im, z.re);
        }
        *phase_error = pe;
        return index;
    }
};

// gr-digital/python/utils/mod_codes.py invert_code: the positions of 0, 1, 2 .. in `code` (a stable sort by value)
inline std::vector<int> invert_code(const std::vector<unsigned> &code)
{
    std::vector<int> inv;
    std::vector<char> used(code.size(), 0);
    for (size_t k = 0; k < code.size(); ++k) {
        size_t best = code.size();
        for (size_t i = 0; i < code.size(); ++i)
            if (!used[i] && (best == code.size() || code[i] < code[best])) best = i;
        used[best] = 1;
        inv.push_back((int)best);
    }
    return inv;
}

}  // namespace grhip
