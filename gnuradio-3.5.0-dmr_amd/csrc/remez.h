// remez.h -- gr_remez, the Parks-McClellan exchange (general/gr_remez.cc:98-867), and the designers of
// gnuradio/optfir.py (:45-78, :116-156, :160-310) in host arithmetic (internal; no HIP, no device, no library).
//
// The arithmetic is the reference's statement for statement in double: the same operation order, the same Pi literal,
// the same constants, so that a design comes back bit for bit (tests/test_optfir_cpu.py holds it to the reference's own
// code).  What differs is the memory: every array is a std::vector sized by what is written into it, so nothing is
// read or written outside an array and nothing is leaked on the error paths, and sizes the reference cannot take are
// refused (include/grhip.h states them).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace grhip {

constexpr int REMEZ_BANDPASS = 1, REMEZ_DIFFERENTIATOR = 2, REMEZ_HILBERT = 3;
constexpr int REMEZ_MAX_TAPS = 4096;        // the reference's InitialGuess overflows an int from about 23 000 taps
constexpr int REMEZ_MAX_DENSITY = 1024;
constexpr int REMEZ_MAX_BANDS = 64;
// status: 0, or one of these with *msg set (the values are GRHIP_EINVAL, GRHIP_ERANGE and GRHIP_ERUNTIME)
constexpr int REMEZ_EINVAL = -1, REMEZ_ERANGE = -2, REMEZ_EFAILED = -3;

namespace remez_detail {

constexpr int NEGATIVE = 0, POSITIVE = 1;
constexpr double Pi = 3.14159265358979323846;
constexpr double Pi2 = 2 * Pi;
constexpr int GRIDDENSITY = 16;
constexpr int MAXITERATIONS = 40;

typedef std::vector<double> dvec;

// what band `band` of the dense grid starts at and how many points it gets (gr_remez.cc:107-120)
inline void grid_band(int r, const double bands[], int symmetry, int griddensity, int band, double *lowf, int *k)
{
    const double delf = 0.5 / (griddensity * r);
    const double grid0 = (symmetry == NEGATIVE) && (delf > bands[0]) ? delf : bands[0];
    *lowf = (band == 0 ? grid0 : bands[2 * band]);
    const double highf = bands[2 * band + 1];
    const double kk = (highf - *lowf) / delf + 0.5;     /* .5 for rounding */
    *k = kk > 0.0 ? (int)kk : 0;
}

// gr_remez.cc:98-142.  Grid, D and W hold at least `written` (the points of all bands) and gridsize entries.
inline void CreateDenseGrid(int r, int numtaps, int numband, const double bands[], const double des[], const double weight[],
                            int gridsize, dvec &Grid, dvec &D, dvec &W, int symmetry, int griddensity)
{
    const double delf = 0.5 / (griddensity * r);
    int j = 0;
    for (int band = 0; band < numband; band++) {
        double lowf;
        int k;
        grid_band(r, bands, symmetry, griddensity, band, &lowf, &k);
        const double highf = bands[2 * band + 1];
        for (int i = 0; i < k; i++) {
            D[j] = des[2 * band] + i * (des[2 * band + 1] - des[2 * band]) / (k - 1);
            W[j] = weight[band];
            Grid[j] = lowf;
            lowf += delf;
            j++;
        }
        if (j > 0) Grid[j - 1] = highf;                 // (the reference writes Grid[-1] for an empty first band)
    }
    if ((symmetry == NEGATIVE) && (Grid[gridsize - 1] > (0.5 - delf)) && (numtaps % 2)) Grid[gridsize - 1] = 0.5 - delf;
}

// gr_remez.cc:161-168; the product in 64 bits (it stays below 2^31 under REMEZ_MAX_TAPS and REMEZ_MAX_DENSITY anyway)
inline void InitialGuess(int r, std::vector<int> &Ext, int gridsize)
{
    for (int i = 0; i <= r; i++) Ext[i] = (int)((long long)i * (gridsize - 1) / r);
}

// gr_remez.cc:191-245
inline void CalcParms(int r, const std::vector<int> &Ext, const dvec &Grid, const dvec &D, const dvec &W, dvec &ad, dvec &x, dvec &y)
{
    int i, j, k, ld;
    double sign, xi, delta, denom, numer;

    for (i = 0; i <= r; i++) x[i] = cos(Pi2 * Grid[Ext[i]]);

    ld = (r - 1) / 15 + 1;         /* Skips around to avoid round errors */
    for (i = 0; i <= r; i++) {
        denom = 1.0;
        xi = x[i];
        for (j = 0; j < ld; j++) {
            for (k = j; k <= r; k += ld)
                if (k != i) denom *= 2.0 * (xi - x[k]);
        }
        if (fabs(denom) < 0.00001) denom = 0.00001;
        ad[i] = 1.0 / denom;
    }

    numer = denom = 0;
    sign = 1;
    for (i = 0; i <= r; i++) {
        numer += ad[i] * D[Ext[i]];
        denom += sign * ad[i] / W[Ext[i]];
        sign = -sign;
    }
    delta = numer / denom;
    sign = 1;

    for (i = 0; i <= r; i++) {
        y[i] = D[Ext[i]] - sign * delta / W[Ext[i]];
        sign = -sign;
    }
}

// gr_remez.cc:269-291
inline double ComputeA(double freq, int r, const dvec &ad, const dvec &x, const dvec &y)
{
    double xc, c, denom, numer;
    denom = numer = 0;
    xc = cos(Pi2 * freq);
    for (int i = 0; i <= r; i++) {
        c = xc - x[i];
        if (fabs(c) < 1.0e-7) {
            numer = y[i];
            denom = 1;
            break;
        }
        c = ad[i] / c;
        denom += c;
        numer += c * y[i];
    }
    return numer / denom;
}

// gr_remez.cc:318-331
inline void CalcError(int r, const dvec &ad, const dvec &x, const dvec &y, int gridsize, const dvec &Grid, const dvec &D,
                      const dvec &W, dvec &E)
{
    for (int i = 0; i < gridsize; i++) {
        const double A = ComputeA(Grid[i], r, ad, x, y);
        E[i] = W[i] * (D[i] - A);
    }
}

// gr_remez.cc:357-474; gridsize >= 2
inline int Search(int r, std::vector<int> &Ext, int gridsize, const dvec &E)
{
    int i, j, k, l, extra;
    int up, alt;
    std::vector<int> foundExt((size_t)2 * r);
    k = 0;

    if (((E[0] > 0.0) && (E[0] > E[1])) || ((E[0] < 0.0) && (E[0] < E[1]))) foundExt[k++] = 0;

    for (i = 1; i < gridsize - 1; i++) {
        if (((E[i] >= E[i - 1]) && (E[i] > E[i + 1]) && (E[i] > 0.0)) || ((E[i] <= E[i - 1]) && (E[i] < E[i + 1]) && (E[i] < 0.0))) {
            if (k >= 2 * r) return -3;
            foundExt[k++] = i;
        }
    }

    j = gridsize - 1;
    if (((E[j] > 0.0) && (E[j] > E[j - 1])) || ((E[j] < 0.0) && (E[j] < E[j - 1]))) {
        if (k >= 2 * r) return -3;
        foundExt[k++] = j;
    }

    if (k < r + 1) return -2;

    extra = k - (r + 1);
    while (extra > 0) {
        if (E[foundExt[0]] > 0.0)
            up = 1;                /* first one is a maxima */
        else
            up = 0;                /* first one is a minima */

        l = 0;
        alt = 1;
        for (j = 1; j < k; j++) {
            if (fabs(E[foundExt[j]]) < fabs(E[foundExt[l]])) l = j;               /* new smallest error. */
            if ((up) && (E[foundExt[j]] < 0.0))
                up = 0;             /* switch to a minima */
            else if ((!up) && (E[foundExt[j]] > 0.0))
                up = 1;             /* switch to a maxima */
            else {
                alt = 0;
                break;              /* two non-alternating extrema: delete the smallest so far */
            }
        }

        if ((alt) && (extra == 1)) {
            if (fabs(E[foundExt[k - 1]]) < fabs(E[foundExt[0]]))
                l = k - 1;          /* Delete last extremal */
            else
                l = 0;              /* Delete first extremal */
        }

        for (j = l; j < k - 1; j++) foundExt[j] = foundExt[j + 1];
        k--;
        extra--;
    }

    for (i = 0; i <= r; i++) Ext[i] = foundExt[i];
    return 0;
}

// gr_remez.cc:494-551; A holds N / 2 + 1 entries
inline void FreqSample(int N, const dvec &A, double h[], int symm)
{
    int n, k;
    double x, val, M;

    M = (N - 1.0) / 2.0;
    if (symm == POSITIVE) {
        if (N % 2) {
            for (n = 0; n < N; n++) {
                val = A[0];
                x = Pi2 * (n - M) / N;
                for (k = 1; k <= M; k++) val += 2.0 * A[k] * cos(x * k);
                h[n] = val / N;
            }
        } else {
            for (n = 0; n < N; n++) {
                val = A[0];
                x = Pi2 * (n - M) / N;
                for (k = 1; k <= (N / 2 - 1); k++) val += 2.0 * A[k] * cos(x * k);
                h[n] = val / N;
            }
        }
    } else {
        if (N % 2) {
            for (n = 0; n < N; n++) {
                val = 0;
                x = Pi2 * (n - M) / N;
                for (k = 1; k <= M; k++) val += 2.0 * A[k] * sin(x * k);
                h[n] = val / N;
            }
        } else {
            for (n = 0; n < N; n++) {
                val = A[N / 2] * sin(Pi * (n - M));
                x = Pi2 * (n - M) / N;
                for (k = 1; k <= (N / 2 - 1); k++) val += 2.0 * A[k] * sin(x * k);
                h[n] = val / N;
            }
        }
    }
}

// gr_remez.cc:571-587
inline bool isDone(int r, const std::vector<int> &Ext, const dvec &E)
{
    double min, max, current;
    min = max = fabs(E[Ext[0]]);
    for (int i = 1; i <= r; i++) {
        current = fabs(E[Ext[i]]);
        if (current < min) min = current;
        if (current > max) max = current;
    }
    return (((max - min) / max) < 0.0001);
}

// gr_remez.cc:612-775.  Returns 0, the reference's -1 / -2 / -3, or -4: a dense grid of fewer than two points (the
// reference then reads outside it).  bands are on [0, 0.5].
inline int remez(double h[], int numtaps, int numband, const double bands[], const double des[], const double weight[], int type,
                 int griddensity)
{
    int i, iter, gridsize, r;
    double c;
    const int symmetry = type == REMEZ_BANDPASS ? POSITIVE : NEGATIVE;

    r = numtaps / 2;                  /* number of extrema */
    if ((numtaps % 2) && (symmetry == POSITIVE)) r++;

    gridsize = 0;
    for (i = 0; i < numband; i++) gridsize += (int)(2 * r * griddensity * (bands[2 * i + 1] - bands[2 * i]) + .5);
    if (symmetry == NEGATIVE) gridsize--;
    if (gridsize < 2) return -4;

    // CreateDenseGrid writes the points of every band: where that is more than gridsize (a hilbert transformer that
    // starts above the first grid step gets one more), the arrays hold them all; the loops below still run to gridsize
    long long written = 0;
    for (i = 0; i < numband; i++) {
        double lowf;
        int k;
        remez_detail::grid_band(r, bands, symmetry, griddensity, i, &lowf, &k);
        written += k;
    }
    const size_t room = (size_t)(written > gridsize ? written : gridsize);
    dvec Grid(room, 0.0), D(room, 0.0), W(room, 0.0), E(room, 0.0);
    std::vector<int> Ext((size_t)r + 1);
    dvec taps((size_t)(numtaps / 2 > r ? numtaps / 2 : r) + 1), x((size_t)r + 1), y((size_t)r + 1), ad((size_t)r + 1);

    CreateDenseGrid(r, numtaps, numband, bands, des, weight, gridsize, Grid, D, W, symmetry, griddensity);
    InitialGuess(r, Ext, gridsize);

    if (type == REMEZ_DIFFERENTIATOR) {
        for (i = 0; i < gridsize; i++) {
            if (D[i] > 0.0001) W[i] = W[i] / Grid[i];
        }
    }

    if (symmetry == POSITIVE) {
        if (numtaps % 2 == 0) {
            for (i = 0; i < gridsize; i++) {
                c = cos(Pi * Grid[i]);
                D[i] /= c;
                W[i] *= c;
            }
        }
    } else {
        if (numtaps % 2) {
            for (i = 0; i < gridsize; i++) {
                c = sin(Pi2 * Grid[i]);
                D[i] /= c;
                W[i] *= c;
            }
        } else {
            for (i = 0; i < gridsize; i++) {
                c = sin(Pi * Grid[i]);
                D[i] /= c;
                W[i] *= c;
            }
        }
    }

    for (iter = 0; iter < MAXITERATIONS; iter++) {
        CalcParms(r, Ext, Grid, D, W, ad, x, y);
        CalcError(r, ad, x, y, gridsize, Grid, D, W, E);
        int err = Search(r, Ext, gridsize, E);
        if (err) return err;
        if (isDone(r, Ext, E)) break;
    }

    CalcParms(r, Ext, Grid, D, W, ad, x, y);

    for (i = 0; i <= numtaps / 2; i++) {
        if (symmetry == POSITIVE) {
            if (numtaps % 2)
                c = 1;
            else
                c = cos(Pi * (double)i / numtaps);
        } else {
            if (numtaps % 2)
                c = sin(Pi2 * (double)i / numtaps);
            else
                c = sin(Pi * (double)i / numtaps);
        }
        taps[i] = ComputeA((double)i / numtaps, r, ad, x, y) * c;
    }

    FreqSample(numtaps, taps, h, symmetry);
    return iter < MAXITERATIONS ? 0 : -1;
}

inline bool finite_all(const double *v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace remez_detail

// gr_remez(order, bands, response, weight, filter_type, grid_density) (gr_remez.cc:791-867): taps receives order + 1
// doubles.  nweight == 0: every band weighs 1.  On an error taps is empty and *msg names it (the reference's words
// where it throws).
// the argument checks of gr_remez() (gr_remez.cc:800-851) and the stated limits
inline int remez_check(int order, const double *bands_in, size_t nbands2, const double *response, size_t nresponse,
                       const double *weight_in, size_t nweight, int filter_type, int grid_density, const char **msg)
{
    using namespace remez_detail;
    if (order < 3) { *msg = "gr_remez: number of taps must be >= 3"; return REMEZ_EINVAL; }
    if (order > REMEZ_MAX_TAPS - 1) { *msg = "gr_remez: more than 4096 taps"; return REMEZ_ERANGE; }
    const size_t numbands = nbands2 / 2;
    if (numbands < 1 || nbands2 % 2 == 1) { *msg = "gr_remez: must have an even number of band edges"; return REMEZ_EINVAL; }
    if (numbands > (size_t)REMEZ_MAX_BANDS) { *msg = "gr_remez: more than 64 bands"; return REMEZ_EINVAL; }
    if (!bands_in || !response || (nweight && !weight_in)) { *msg = "gr_remez: null argument"; return REMEZ_EINVAL; }
    if (!finite_all(bands_in, nbands2)) { *msg = "gr_remez: an argument is not finite"; return REMEZ_EINVAL; }
    for (size_t i = 1; i < nbands2; i++)
        if (bands_in[i] < bands_in[i - 1]) { *msg = "gr_remez: band edges must be nondecreasing"; return REMEZ_EINVAL; }
    if (bands_in[0] < 0 || bands_in[nbands2 - 1] > 1) { *msg = "gr_remez: band edges must be in the range [0,1]"; return REMEZ_EINVAL; }
    if (nresponse != nbands2) { *msg = "gr_remez: must have one response magnitude for each band edge"; return REMEZ_EINVAL; }
    if (nweight != 0 && nweight != numbands) { *msg = "gr_remez: need one weight for each band [=length(band)/2]"; return REMEZ_EINVAL; }
    if (!finite_all(response, nresponse) || !finite_all(weight_in, nweight)) { *msg = "gr_remez: an argument is not finite"; return REMEZ_EINVAL; }
    if (filter_type != REMEZ_BANDPASS && filter_type != REMEZ_DIFFERENTIATOR && filter_type != REMEZ_HILBERT) {
        *msg = "gr_remez: unknown ftype";
        return REMEZ_EINVAL;
    }
    if (grid_density < 16) { *msg = "gr_remez: grid_density is too low; must be >= 16"; return REMEZ_EINVAL; }
    if (grid_density > REMEZ_MAX_DENSITY) { *msg = "gr_remez: grid_density above 1024"; return REMEZ_EINVAL; }
    return 0;
}

inline int remez_design(int order, const double *bands_in, size_t nbands2, const double *response, size_t nresponse,
                        const double *weight_in, size_t nweight, int filter_type, int grid_density, std::vector<double> &taps,
                        const char **msg)
{
    using namespace remez_detail;
    const char *dummy;
    if (!msg) msg = &dummy;
    *msg = "";
    taps.clear();
    const int rc = remez_check(order, bands_in, nbands2, response, nresponse, weight_in, nweight, filter_type, grid_density, msg);
    if (rc) return rc;
    const int numtaps = order + 1;
    const size_t numbands = nbands2 / 2;

    // Divide by 2 to fit with the implementation that uses a sample rate of [0, 0.5] instead of [0, 1.0]
    std::vector<double> bands(nbands2), weight(numbands, 1.0);
    for (size_t i = 0; i < nbands2; i++) bands[i] = bands_in[i] / 2;
    for (size_t i = 0; i < nweight; i++) weight[i] = weight_in[i];

    std::vector<double> coeff((size_t)numtaps);
    const int err = remez(coeff.data(), numtaps, (int)numbands, bands.data(), response, weight.data(), filter_type, grid_density);
    if (err == -1) { *msg = "gr_remez: failed to converge"; return REMEZ_EFAILED; }
    if (err == -2) { *msg = "gr_remez: insufficient extremals -- cannot continue"; return REMEZ_EFAILED; }
    if (err == -3) { *msg = "gr_remez: too many extremals -- cannot continue"; return REMEZ_EFAILED; }
    if (err) { *msg = "gr_remez: the bands give a dense grid of fewer than two points"; return REMEZ_EINVAL; }
    taps.swap(coeff);
    return 0;
}

// ---- gnuradio/optfir.py -----------------------------------------------------------------------------------------------
// optfir.py:160-166.  -atten_db / 20 is a true division (Python 2 floors it for two integers; the same for 60)
inline double optfir_stopband_atten_to_dev(double atten_db) { return pow(10.0, -atten_db / 20); }
inline double optfir_passband_ripple_to_dev(double ripple_db)
{
    return (pow(10.0, ripple_db / 20) - 1) / (pow(10.0, ripple_db / 20) + 1);
}

// optfir.py:276-310
inline double optfir_lporder(double freq1, double freq2, double delta_p, double delta_s)
{
    const double df = fabs(freq2 - freq1);
    const double ddp = log10(delta_p);
    const double dds = log10(delta_s);

    const double a1 = 5.309e-3, a2 = 7.114e-2, a3 = -4.761e-1, a4 = -2.66e-3, a5 = -5.941e-1, a6 = -4.278e-1;
    const double b1 = 11.01217, b2 = 0.5124401;

    const double t1 = a1 * ddp * ddp;
    const double t2 = a2 * ddp;
    const double t3 = a4 * ddp * ddp;
    const double t4 = a5 * ddp;

    const double dinf = ((t1 + t2 + a3) * dds) + (t3 + t4 + a6);
    const double ff = b1 + b2 * (ddp - dds);
    return dinf / df - ff * df + 1;
}

// what remezord returns (optfir.py:170-272): the order for gr_remez and its band edges, amplitudes and weights
struct OptfirSpec {
    int order = 0;
    std::vector<double> bands, ampl, weight;
};

// remezord(fcuts, mags, devs, fsamp): mags and devs of nbands entries, fcuts of 2 (nbands - 1).  nbands is 2 or 3 here.
// Returns 0 or REMEZ_EINVAL (an estimate that is not a finite count of taps: the reference raises on int(ceil(nan))).
inline int optfir_remezord(std::vector<double> fcuts, const std::vector<double> &mags, std::vector<double> devs, double fsamp,
                           OptfirSpec &s, const char **msg)
{
    const size_t nbands = mags.size();
    for (size_t i = 0; i < fcuts.size(); i++) fcuts[i] = fcuts[i] / fsamp;
    for (size_t i = 0; i < nbands; i++)
        if (mags[i] != 0) devs[i] = devs[i] / mags[i];     // if not stopband, get relative deviation

    // separate the passband and stopband edges: f1 = fcuts[0::2], f2 = fcuts[1::2]
    size_t n = 0;
    double min_delta = 2;
    for (size_t i = 0; i < fcuts.size() / 2; i++) {
        if (fcuts[2 * i + 1] - fcuts[2 * i] < min_delta) {
            n = i;
            min_delta = fcuts[2 * i + 1] - fcuts[2 * i];
        }
    }
    double l;
    if (nbands == 2) {
        l = optfir_lporder(fcuts[2 * n], fcuts[2 * n + 1], devs[0], devs[1]);
    } else {
        l = 0;
        for (size_t i = 1; i + 1 < nbands; i++) {
            const double l1 = optfir_lporder(fcuts[2 * (i - 1)], fcuts[2 * (i - 1) + 1], devs[i], devs[i - 1]);
            const double l2 = optfir_lporder(fcuts[2 * i], fcuts[2 * i + 1], devs[i], devs[i + 1]);
            // max (l, l1, l2) as Python evaluates it: the first of the largest, a later one only where it is greater
            double m = l;
            if (l1 > m) m = l1;
            if (l2 > m) m = l2;
            l = m;
        }
    }
    const double cl = ceil(l);
    if (!(cl > -1e9 && cl < 1e9)) { *msg = "optfir: the order estimate is not finite"; return REMEZ_EINVAL; }
    s.order = (int)cl - 1;                      // need order, not length for remez

    s.bands.assign(1, 0.0);
    for (size_t i = 0; i < fcuts.size(); i++) s.bands.push_back(fcuts[i] * 2);
    s.bands.push_back(1.0);
    s.ampl.clear();
    for (size_t i = 0; i < nbands; i++) { s.ampl.push_back(mags[i]); s.ampl.push_back(mags[i]); }
    double max_dev = devs[0];
    for (size_t i = 1; i < nbands; i++)
        if (devs[i] > max_dev) max_dev = devs[i];
    s.weight.resize(nbands);
    for (size_t i = 0; i < nbands; i++) s.weight[i] = max_dev / devs[i];
    return 0;
}

constexpr int OPTFIR_LOW_PASS = 0, OPTFIR_HIGH_PASS = 1, OPTFIR_BAND_PASS = 2, OPTFIR_BAND_REJECT = 3;

// The arguments optfir.low_pass / high_pass / band_pass / band_reject hand to gr.remez (optfir.py:45-78, :116-156).
// f holds the designer's band edges in its order: two for low_pass and high_pass, four for the other two.
inline int optfir_spec(int kind, double gain, double fs, const double *f, double passband_ripple_db, double stopband_atten_db,
                       int nextra_taps, OptfirSpec &s, const char **msg)
{
    const char *dummy;
    if (!msg) msg = &dummy;
    *msg = "";
    const int nf = (kind == OPTFIR_LOW_PASS || kind == OPTFIR_HIGH_PASS) ? 2 : 4;
    if (kind < OPTFIR_LOW_PASS || kind > OPTFIR_BAND_REJECT) { *msg = "optfir: unknown designer"; return REMEZ_EINVAL; }
    if (!std::isfinite(gain) || !std::isfinite(fs) || !remez_detail::finite_all(f, (size_t)nf) || !std::isfinite(passband_ripple_db) ||
        !std::isfinite(stopband_atten_db)) {
        *msg = "optfir: an argument is not finite";
        return REMEZ_EINVAL;
    }
    if (fs == 0.0) { *msg = "optfir: the sampling rate is zero"; return REMEZ_EINVAL; }
    if (nextra_taps < -REMEZ_MAX_TAPS || nextra_taps > REMEZ_MAX_TAPS) { *msg = "optfir: nextra_taps out of range"; return REMEZ_EINVAL; }
    const double passband_dev = optfir_passband_ripple_to_dev(passband_ripple_db);
    const double stopband_dev = optfir_stopband_atten_to_dev(stopband_atten_db);
    std::vector<double> fcuts(f, f + nf), mags, devs;
    switch (kind) {
    case OPTFIR_LOW_PASS: mags = {gain, 0}; devs = {passband_dev, stopband_dev}; break;
    case OPTFIR_HIGH_PASS: mags = {0, 1}; devs = {stopband_dev, passband_dev}; break;      // the gain is not used
    case OPTFIR_BAND_PASS: mags = {0, gain, 0}; devs = {stopband_dev, passband_dev, stopband_dev}; break;
    default: mags = {gain, 0, gain}; devs = {passband_dev, stopband_dev, passband_dev}; break;
    }
    int rc = optfir_remezord(fcuts, mags, devs, fs, s, msg);
    if (rc) return rc;
    // For a HPF (and the band reject), we need to use an odd number of taps
    if ((kind == OPTFIR_HIGH_PASS || kind == OPTFIR_BAND_REJECT) && (s.order + nextra_taps) % 2 != 0) s.order += 1;
    s.order += nextra_taps;
    return 0;
}

inline int optfir_design(int kind, double gain, double fs, const double *f, double passband_ripple_db, double stopband_atten_db,
                         int nextra_taps, std::vector<double> &taps, const char **msg)
{
    OptfirSpec s;
    taps.clear();
    int rc = optfir_spec(kind, gain, fs, f, passband_ripple_db, stopband_atten_db, nextra_taps, s, msg);
    if (rc) return rc;
    return remez_design(s.order, s.bands.data(), s.bands.size(), s.ampl.data(), s.ampl.size(), s.weight.data(), s.weight.size(),
                        REMEZ_BANDPASS, remez_detail::GRIDDENSITY, taps, msg);
}

}  // namespace grhip
