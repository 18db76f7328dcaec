// capi_fir.hip -- C ABI for gr_fir_filter_XXX, gr_freq_xlating_fir_filter_XXX,
// gr_quadrature_demod_cf and the fused xlating->demod hier block.
#include <cmath>
#include <complex>

#include "fft_kernels.h"
#include "fir_kernels.h"
#include "grhip_internal.h"
#include "mfma_tables.h"
#include "xlating_core.h"

using namespace grhip;
typedef std::complex<float> cf;

namespace grhip {

static int upload(DevBuf &b, const void *src, size_t bytes)
{
    int rc = b.reserve(bytes ? bytes : 16);
    if (rc) return rc;
    if (bytes) GRHIP_HIP(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return GRHIP_OK;
}

template <class A> static A zeroed() { A a; memset(&a, 0, sizeof(a)); return a; }

// ============================================================================
// FirEngines (fir_engines.h): every engine of the family packed and launched here
// ============================================================================
// taps per phase of the tiled kernel, padded to its R outputs per lane
static int tiled_Tq(int T, int D)
{
    const int R = tiled_R(), per = (T + D - 1) / D;
    return per ? ((per + R - 1) / R) * R : R;
}

// c[k] multiplies x[nD + k]; hp[p*Tq + q] = c[qD + p], zero padded.
static int pack_phase_major(const float *c, int T, int tw, int D, std::vector<float> &hp)
{
    const int R = tiled_R(), Tq = tiled_Tq(T, D);
    hp.assign(((size_t)D * Tq + R) * tw, 0.f);     // + R taps: the kernel prefetches one iteration ahead
    for (int k = 0; k < T; ++k) {
        int p = k % D, q = k / D;
        for (int w = 0; w < tw; ++w) hp[((size_t)p * Tq + q) * tw + w] = c[(size_t)k * tw + w];
    }
    return Tq;
}

FirCaps FirEngines::caps(int ntaps, int decim, int tiled_decim)
{
    FirCaps c;
    c.tiled_real = c.tiled_cplx = tiled_decim > 0 && tiled_supported(tiled_decim, tiled_Tq(ntaps, tiled_decim));
    c.mfma = mfma_supported(decim, ntaps); c.hidec = hidec_supported(decim, ntaps); c.realin = realin_supported(decim, ntaps);
    return c;
}

FirTuning FirEngines::tuning()
{
    FirTuning tn;
#ifdef GRHIP_DIAG       // diagnostic builds only (tools/bench_decim.py, tools/bench_ols_crossover.py)
    if (const char *e = getenv("GRHIP_HIDEC")) tn.hidec = atoi(e);
    if (const char *e = getenv("GRHIP_OLS_MIN")) tn.ols_min = atoi(e);
#endif
    return tn;
}

int FirEngines::build_tiled(const float *c, int tw)
{
    std::vector<float> hp;
    Tq = pack_phase_major(c, ntaps, tw, plan.tiled_decim, hp);
    return upload(d_hp, hp.data(), hp.size() * sizeof(float));
}

// operand tables of the matrix-core engine (mfma_tables.h): real taps, both alignment parities.  The pre-mix form's table
// carries the correction band G of the reference's tap-angle quantisation behind A; plain real taps (gr_fir_ccf): G all zero
int FirEngines::build_mfma(const float *c, float fwT0)
{
    const int KS = mf::ksteps_inst(decim, ntaps);
    mf_kexp = mf::tap_scale_exp(c, ntaps);
    for (int off = 0; off < 2; ++off) {
        std::vector<uint16_t> A;
        mf::build_A(c, ntaps, decim, KS, off, mf_kexp, A);
        mf::build_G(c, ntaps, decim, KS, off, mf_kexp, fwT0, A);
        int rc = upload(d_mf_A[off], A.data(), A.size() * sizeof(uint16_t));
        if (rc) return rc;
    }
    return GRHIP_OK;
}

// the engine convolves: h[k] = c[ntaps-1-k] multiplies x[i-k], as complex taps
int FirEngines::build_ols(const float *c, int tw)
{
    std::vector<float> h((size_t)ntaps * 2);
    for (int k = 0; k < ntaps; ++k) {
        const float *t = c + (size_t)(ntaps - 1 - k) * tw;
        h[2 * k] = t[0];
        h[2 * k + 1] = tw == 2 ? t[1] : 0.f;
    }
    return ols_build(h.data(), ntaps, decim, d_ols_tw, d_ols_H, &ols_L, &ols_fold);
}

int FirEngines::build_hidec(const float *c, int tw)
{
    std::vector<float> hp;
    hidec_pad_taps(c, ntaps, tw, decim, hp);
    return upload(d_hidec_taps, hp.data(), hp.size() * sizeof(float));
}

int FirEngines::build_realin(const float *c)
{
    std::vector<float> hp;
    ri_Tq = realin_pack_taps(c, ntaps, decim, hp);
    return upload(d_ri_hp, hp.data(), hp.size() * sizeof(float));
}

int FirEngines::build_plain(FirKind kind, int decimation, const float *rev, int n)
{
    ntaps = n; decim = decimation;
    const int tw = fir_kind_ctaps(kind) ? 2 : 1;
    plan = fir_plan_plain(kind, decim, ntaps, caps(ntaps, decim, fir_tiled_decim(kind, decim)), tuning());
    int rc = GRHIP_OK;
    if (plan.use_realin) rc = build_realin(rev);
    if (!rc && plan.use_tiled) rc = build_tiled(rev, tw);
    if (!rc && plan.use_mfma) rc = build_mfma(rev);
    if (!rc && plan.use_ols) rc = build_ols(rev, tw);
    if (!rc && plan.use_hidec) rc = build_hidec(rev, tw);
    return rc;
}

int FirEngines::launch_mfma(FirMfmaArgs a, const FirIo &io, bool premix, int epi, hipStream_t st)
{
    a.x = (const float2 *)io.x; a.x_stride = io.x_stride; a.n_in = io.n_in; a.n_lo = io.n_lo; a.n_out = io.n_out;
    a.n_streams = io.n_streams;
    a.off = io.parity();
    a.A = d_mf_A[a.off].p; a.kexp = mf_kexp;
    const bool demod = epi == EPI_DEMOD;
    if (demod) a.d_out = (float *)io.out; else a.y_out = (float2 *)io.out;
    a.y_stride = io.out_stride; a.d_stride = io.out_stride;
    a.vec_store = (((uintptr_t)io.out) & (demod ? 7 : 15)) == 0 && !(io.out_stride & 1);
    a.sched = mf_sched.get();
    return launch_fir_mfma(decim, ntaps, premix, epi, a, st);
}

int FirEngines::launch_tiled(FirTiledArgs a, const FirIo &io, bool ctaps, bool premix, int epi, hipStream_t st)
{
    a.x = (const float2 *)io.x; a.x_stride = io.x_stride; a.n_in = io.n_in; a.n_lo = io.n_lo; a.n_out = io.n_out;
    a.hp = d_hp.as<float>(); a.Tq = Tq;
    const bool demod = epi == EPI_DEMOD;
    if (demod) a.d_out = (float *)io.out; else a.y_out = (float2 *)io.out;
    a.y_stride = io.out_stride; a.d_stride = io.out_stride;
    a.vec_store = (((uintptr_t)io.out) & 15) == 0 && ((io.out_stride * (demod ? 4 : 8)) & 15) == 0;
    a.sched = sched.get();
    return launch_fir_tiled(plan.tiled_decim, ctaps, premix, epi, a, io.n_streams, st);
}

int FirEngines::launch_hidec(bool ctaps, const FirIo &io, const float2 *gtab, const float2 *etab, const float2 *vtab, hipStream_t st)
{
    return launch_fir_hidec(ctaps, d_hidec_taps.as<float>(), ntaps, decim, (const float2 *)io.x, (io.n_out - 1) * decim + ntaps,
                            (float2 *)io.out, io.n_out, gtab, st, etab, vtab);
}

// y[n] = sum_k taps[k] x[nD + ntaps-1-k]: the ntaps-1 history items in front of io.x are the engine's "previous call"
// samples, the rest is the stream (the scheduler guarantees (n-1)*D + ntaps items: nothing past the last needed sample is read)
int FirEngines::launch_ols(bool real_data, const FirIo &io, hipStream_t st)
{
    const long long nin = (io.n_out - 1) * decim + 1;
    if (real_data) {
        const float *xf = (const float *)io.x;
        return launch_fftfilt4096_real(xf + (ntaps - 1), nin, xf, ntaps, d_ols_tw.as<float2>(), d_ols_H.as<float2>(),
                                       (float *)io.out, io.n_out, decim, ols_L, ols_fold, st);
    }
    const float2 *x = (const float2 *)io.x;
    return launch_fftfilt4096(x + (ntaps - 1), nin, x, ntaps, d_ols_tw.as<float2>(), d_ols_H.as<float2>(), (float2 *)io.out,
                              io.n_out, decim, ols_L, ols_fold, st);
}

int FirEngines::launch_realin(bool in_short, const FirIo &io, const float2 *gtab, hipStream_t st)
{
    return launch_fir_realin(in_short, decim, d_ri_hp.as<float>(), ri_Tq, io.x, io.n_in, (float2 *)io.out, io.n_out, gtab, st);
}

int FirEngines::run_plain(FirKind ekind, int mode, const float *taps_rev, const void *d_in, void *d_out, long long n, int dec,
                          hipStream_t st)
{
    if (n <= 0) return GRHIP_OK;
    FirCall c;
    c.mode = mode; c.same_decim = dec == decim; c.n = n;
    c.in_aligned = !(((uintptr_t)d_in) & (ekind == FIR_SCC ? 1 : 3));
    c.out_aligned = !(((uintptr_t)d_out) & 7);
    FirIo io{d_in, (n - 1) * dec + ntaps, n, d_out};
    switch (fir_route(plan, c).engine) {
    case ENG_REALIN: return launch_realin(ekind == FIR_SCC, io, nullptr, st);
    case ENG_MFMA: return launch_mfma(zeroed<FirMfmaArgs>(), io, false, EPI_NONE, st);
    case ENG_TILED: {
        FirTiledArgs a = zeroed<FirTiledArgs>();
        if (ekind != FIR_FFF) return launch_tiled(a, io, ekind == FIR_CCC, false, EPI_NONE, st);
        // gr_fir_fff: output pairs (y[2j], y[2j+1]); an odd last output goes through the generic kernel
        a.fpair = dec;
        io.n_out = n / 2;
        int rc = launch_tiled(a, io, false, false, EPI_NONE, st);
        if (rc || !(n & 1)) return rc;
        return launch_fir_generic(ekind, taps_rev, ntaps, (const float *)d_in + (n - 1) * dec, (float *)d_out + (n - 1), 1, dec,
                                  nullptr, st);
    }
    case ENG_HIDEC: return launch_hidec(ekind == FIR_CCC, io, nullptr, nullptr, nullptr, st);
    case ENG_OLS: return launch_ols(ekind == FIR_FFF, io, st);
    default: return launch_fir_generic(ekind, taps_rev, ntaps, d_in, d_out, n, dec, nullptr, st);
    }
}

// ============================================================================
// XlatingCore
// ============================================================================
// v[i] = e^{j angle(i)}, the angle in double
template <class Angle>
static std::vector<cf> phasors(int n, Angle &&angle)
{
    std::vector<cf> v(n);
    for (int i = 0; i < n; ++i) {
        const double ang = angle(i);
        v[i] = cf((float)cos(ang), (float)sin(ang));
    }
    return v;
}

static int upload(DevBuf &b, const std::vector<cf> &v) { return upload(b, v.data(), v.size() * sizeof(cf)); }

int XlatingCore::build(int device)
{
    // build_composite_fir (filter/gr_freq_xlating_fir_filter_XXX.cc.t:72-83)
    ntaps = (int)proto.size();
    ctaps.resize(ntaps);
    float fwT0 = 2 * M_PI * center_freq / sampling_freq;
    bool real_proto = true;
    for (unsigned i = 0; i < (unsigned)ntaps; i++) {
        cf e = std::exp(cf(0, i * fwT0));
        // complex product in libgcc order (ac - bd, ad + bc)
        float a = proto[i].real(), b = proto[i].imag(), c = e.real(), d = e.imag();
        if (b != 0.0f) real_proto = false;
        if (real_tap_type) { ctaps[i] = cf(a * c, a * d); continue; }       // float * complex
        float ac = a * c, bd = b * d, ad = a * d, bc = b * c;
        ctaps[i] = cf(ac - bd, ad + bc);
    }
    // d_r.set_phase_incr(exp(gr_complex(0, fwT0 * decimation()))) ; incr / abs(incr)
    cf inc = std::exp(cf(0, fwT0 * decim));
    float mag = hypotf(inc.real(), inc.imag());
    incr = cf(inc.real() / mag, inc.imag() / mag);
    omega = (double)fwT0;
    (void)device;

    // generic kernel wants d_taps order; after reverse(reverse()) that is ctaps itself
    int rc = upload(d_taps_generic, ctaps);
    if (rc) return rc;
    eng.ntaps = ntaps; eng.decim = decim;
    eng.plan = fir_plan_xlating(in_kind, real_proto, for_demod, decim, ntaps, FirEngines::caps(ntaps, decim, decim),
                                FirEngines::tuning());
    const FirPlan &p = eng.plan;
    // the engines' taps, c[k] multiplying x[nD + k]: the composite taps, or the real prototype under the pre-mix forms
    const float *cc = (const float *)ctaps.data();
    std::vector<float> pr(ntaps);
    for (int i = 0; i < ntaps; ++i) pr[i] = proto[i].real();
    if (p.use_realin) rc = eng.build_realin(cc);
    if (!rc && p.use_tiled) rc = p.premix ? eng.build_tiled(pr.data(), 1) : eng.build_tiled(cc, 2);
    if (!rc && p.premix) {
        // phasor tables of the pre-mix form, computed in double (see fir_tiled.hip): W[v+1] = e^{jw(v-D)}, S[i] = e^{jw 512 i},
        // V[j] = e^{-jw j D} with V[NT] = e^{+jwD}
        const int NT = tiled_NT();
        std::vector<cf> V = phasors(NT + 1, [&](int j) { return -omega * (double)j * (double)decim; });
        V[NT] = cf((float)cos(omega * decim), (float)sin(omega * decim));
        rc = upload(d_stab, phasors(tiled_stab_len(), [&](int i) { return omega * (double)tiled_load_span() * (double)i; }));
        if (!rc) rc = upload(d_wtab, phasors(tiled_wtab_len(), [&](int i) { return omega * (double)(i - 1 - decim); }));
        if (!rc) rc = upload(d_vtab, V);
    }
    if (!rc && p.use_mfma) {
        // pre-mix form on the matrix cores: x'[u] = x[u] e^{jw(u - off)}, real prototype taps
        rc = eng.build_mfma(pr.data(), fwT0);
        // 256 staging lanes (fir_mfma_kernel) or 512 (fir_mfma_rs_kernel): e^{jw(2t - off)}
        for (int off = 0; off < 2 && !rc; ++off)
            rc = upload(d_mf_wlane[off], phasors(2 * mf::THREADS, [&](int t) { return omega * (double)(2 * t - off); }));
        mf_wstep[0] = (float)cos(omega); mf_wstep[1] = (float)sin(omega);
        if (!rc) rc = upload(d_mf_stab, phasors(mf::rounds(decim, mf::ksteps_inst(decim, ntaps)),
                                                [&](int i) { return omega * (double)mf::ROUND * (double)i; }));
        if (!rc) rc = upload(d_mf_vtab, phasors(mf::NTC + 2, [&](int j) { return -omega * (double)j * (double)decim; }));
    }
    if (!rc && p.use_ols) rc = eng.build_ols(cc, 2);
    if (!rc && p.use_hidec) {
        rc = p.hidec_premix ? eng.build_hidec(pr.data(), 1) : eng.build_hidec(cc, 2);
        std::vector<float> et, vt;
        if (p.hidec_premix) hidec_premix_tables(omega, decim, et, vt);
        if (!rc && p.hidec_premix) rc = upload(d_hidec_etab, et.data(), et.size() * sizeof(float));
        if (!rc && p.hidec_premix) rc = upload(d_hidec_vtab, vt.data(), vt.size() * sizeof(float));
    }
    if (rc) return rc;
    reset();
    return GRHIP_OK;
}

void XlatingCore::reset()
{
    pos = 0;
    if (tab_start != 0) { tab_start = 0; tab_len = 0; }
    if (tab_len == 0) { gen_phase = cf(1.f, 0.f); gen_counter = 0; }
    if (built_incr != incr) {   // a table generated for another increment is useless
        tab_start = 0; tab_len = 0; gen_phase = cf(1.f, 0.f); gen_counter = 0;
        built_incr = incr;
    }
}

// make sure d_rot covers outputs [pos, pos+n); *gtab = device pointer of phase(pos)
int XlatingCore::ensure_rot(long long n, const float2 **gtab, hipStream_t st)
{
    const long long CAP = 1ll << 25;
    // The table is extended in place behind what earlier launches read; only when its front is
    // rewritten (restart, re-anchor) may a launch still in flight on `st` be reading those entries.
    bool rewrites_front = false;
    if (pos < tab_start) { tab_start = 0; tab_len = 0; gen_phase = cf(1.f, 0.f); gen_counter = 0; rewrites_front = true; }
    long long tab_end = tab_start + tab_len;
    if (pos + n > tab_end) {
        if (pos == tab_end && tab_len > 0 && (pos + n - tab_start) > CAP) {
            tab_start = pos; tab_len = 0;   // re-anchor, generator state is already at pos
            rewrites_front = true;
        }
        if (tab_len == 0) rewrites_front = true;
        if (rewrites_front && d_rot.p) GRHIP_HIP(hipStreamSynchronize(st));
        long long need = pos + n - (tab_start + tab_len);
        std::vector<cf> fresh((size_t)need);
        // gr_rotator::rotate (filter/gr_rotator.h:40-50), exact float recurrence
        float pr = gen_phase.real(), pi = gen_phase.imag();
        const float ir = incr.real(), ii = incr.imag();
        unsigned cnt = gen_counter;
        // (runs of steps up to the next multiple of 512 without the counter test inside: the recurrence is a serial chain
        // of one multiply and one add per step, and this loop is what a streaming stand-alone xlating block waits for)
        for (long long i = 0; i < need;) {
            long long run = 512 - (long long)(cnt % 512);
            if (run > need - i) run = need - i;
            cf *dstp = fresh.data() + (size_t)i;
            for (long long r = 0; r < run; ++r) {
                dstp[r] = cf(pr, pi);
                const float ac = pr * ir, bd = pi * ii, ad = pr * ii, bc = pi * ir;
                pr = ac - bd; pi = ad + bc;
            }
            i += run;
            cnt += (unsigned)run;
            if ((cnt % 512) == 0) {
                float a = hypotf(pr, pi);
                pr = pr / a; pi = pi / a;
            }
        }
        gen_phase = cf(pr, pi); gen_counter = cnt;
        size_t new_items = (size_t)(tab_len + need);
        if (new_items * sizeof(cf) > d_rot.cap) {
            DevBuf nb;
            int rc = nb.reserve(new_items * sizeof(cf) * 2);
            if (rc) return rc;
            if (tab_len) GRHIP_HIP(hipMemcpy(nb.p, d_rot.p, (size_t)tab_len * sizeof(cf), hipMemcpyDeviceToDevice));
            d_rot.swap(nb);         // nb frees the old table on leaving this scope
        }
        GRHIP_HIP(hipMemcpy(d_rot.as<cf>() + tab_len, fresh.data(), (size_t)need * sizeof(cf),
                            hipMemcpyHostToDevice));
        tab_len += need;
    }
    *gtab = reinterpret_cast<const float2 *>(d_rot.as<cf>() + (pos - tab_start));
    return GRHIP_OK;
}

// rotator phase of output pos-1 (for converting the demodulator carry between the
// frames of the two epilogues at a mode switch): phase(pos) * conj(incr)
int XlatingCore::phase_before_pos(std::complex<float> *g)
{
    const float2 *gtab = nullptr;
    int rc = ensure_rot(1, &gtab, nullptr);
    if (rc) return rc;
    cf ph;
    GRHIP_HIP(hipMemcpy(&ph, gtab, sizeof(ph), hipMemcpyDeviceToHost));
    *g = ph * std::conj(incr);
    return GRHIP_OK;
}

template <class Fir>
int XlatingCore::demod_second(const FirIo &io, float gain, const float2 *y_prev, float2 *y_last, const float *atan_tab,
                              hipStream_t st, Fir &&fir)
{
    const long long ys = io.n_out + 1;
    int rc = scratch_y.reserve((size_t)ys * io.n_streams * sizeof(float2));
    if (rc) return rc;
    float2 *sy = scratch_y.as<float2>();
    if (y_prev) GRHIP_HIP(hipMemcpy2DAsync(sy, ys * sizeof(float2), y_prev, sizeof(float2), sizeof(float2), io.n_streams,
                                           hipMemcpyDeviceToDevice, st));
    else GRHIP_HIP(hipMemset2DAsync(sy, ys * sizeof(float2), 0, sizeof(float2), io.n_streams, st));
    FirIo o = io;
    o.out = sy + 1; o.out_stride = ys;
    if ((rc = fir(o))) return rc;
    for (int s = 0; s < io.n_streams; ++s) {
        rc = launch_quad_demod(sy + s * ys, (float *)io.out + s * io.out_stride, io.n_out, gain, atan_tab, st);
        if (rc) return rc;
    }
    if (y_last) GRHIP_HIP(hipMemcpy2DAsync(y_last, sizeof(float2), sy + io.n_out, ys * sizeof(float2), sizeof(float2),
                                           io.n_streams, hipMemcpyDeviceToDevice, st));
    return GRHIP_OK;
}

// run the FIR + rotator (+ demod) for n_out outputs on device pointers.
// d_in item 0 = input[0] of output 0; n_in readable items.
int XlatingCore::run(int mode, const float2 *d_in, long long n_in, long long n_out, float2 *d_y,
                     float *d_demod, float gain, const float2 *y_prev, float2 *y_last,
                     const float *atan_tab, hipStream_t st, int n_streams, long long x_stride,
                     long long n_lo, long long out_stride)
{
    if (n_out <= 0) return GRHIP_OK;
    const bool demod = d_demod != nullptr, sh = in_kind == 2;
    FirCall c;
    c.mode = mode; c.demod = demod; c.batched = !(n_streams == 1 && n_lo == 0);
    c.in_aligned = !(((uintptr_t)d_in) & (sh ? 1 : 3)); c.out_aligned = !(((uintptr_t)d_y) & 7);
    c.odd_stride_multi = n_streams != 1 && (x_stride & 1);
    FirRoute r = fir_route(eng.plan, c);
    const float2 *gtab = nullptr;
    int rc = GRHIP_OK;
    if (r.need_rot && (rc = ensure_rot(n_out, &gtab, st))) return rc;
    if (r.engine == ENG_GENERIC_DEMOD) {
        rc = launch_fir_generic_demod(d_taps_generic.as<float>(), ntaps, d_in, d_demod, n_out, decim, gtab, gain, atan_tab,
                                      y_prev, y_last, st, n_streams, x_stride, out_stride, n_lo);
        if (rc == GRHIP_OK) pos += n_out;
        if (rc != 1) return rc;
        c.generic_fused = false;            // no such kernel for this shape: the two kernels, one stream
        r = fir_route(eng.plan, c);
    }
    if (r.engine == ENG_EINVAL)
        return fail(GRHIP_EINVAL, eng.plan.real_in ? "real-input xlating: one stream, no demodulator"
                                                   : "generic-order path: this shape runs one stream with explicit history");
    const FirPlan &p = eng.plan;
    const int epi = r.epilogue == EPILOGUE_DEMOD_FUSED ? EPI_DEMOD : EPI_ROTATE;
    // the route's FIR: o.out receives y times the rotator's phases, or the fused demodulator's output
    auto fir = [&](const FirIo &o) -> int {
        switch (r.engine) {
        case ENG_REALIN: return eng.launch_realin(sh, o, gtab, st);
        case ENG_MFMA: {
            FirMfmaArgs a = zeroed<FirMfmaArgs>();
            a.wlane = d_mf_wlane[o.parity()].as<float2>(); a.wstep = make_float2(mf_wstep[0], mf_wstep[1]);
            a.stab = d_mf_stab.as<float>(); a.vtab = d_mf_vtab.as<float2>(); a.gtab = gtab;
            a.gain = gain; a.y_prev = y_prev; a.y_last = y_last; a.atan_tab = atan_tab;
            a.ctaps = d_taps_generic.as<float2>(); a.T = ntaps;
            a.max_wg_per_cu = mf_wg_cap; a.max_cus = mf_cu_cap;
            a.omega = omega; a.tapq = mode == GRHIP_MODE_FAST_REFTAPS;
            return eng.launch_mfma(a, o, true, epi, st);
        }
        case ENG_TILED: {
            FirTiledArgs a = zeroed<FirTiledArgs>();
            a.wtab = d_wtab.as<float2>(); a.stab = d_stab.as<float2>(); a.vtab = d_vtab.as<float2>(); a.gtab = gtab;
            a.gain = gain; a.atan_tab = atan_tab;
            if (r.epilogue != EPILOGUE_DEMOD_SECOND) { a.y_prev = y_prev; a.y_last = y_last; }
            // (demodulator as a second kernel: complex prototype taps, the tiled kernel writes y)
            return eng.launch_tiled(a, o, !p.premix, p.premix, epi, st);
        }
        case ENG_HIDEC:
            if (epi == EPI_DEMOD)
                return launch_fir_hidec_demod(eng.d_hidec_taps.as<float>(), ntaps, decim, d_in,
                                              c.batched ? n_in : (n_out - 1) * decim + ntaps, d_demod, n_out, gain, y_prev, y_last,
                                              atan_tab, d_hidec_etab.as<float2>(), d_hidec_vtab.as<float2>(), st, n_streams,
                                              x_stride, out_stride, n_lo, mf_wg_cap, mf_cu_cap);
            return eng.launch_hidec(!p.hidec_premix, o, gtab,            // rotator multiply inside
                                    p.hidec_premix ? d_hidec_etab.as<float2>() : nullptr,
                                    p.hidec_premix ? d_hidec_vtab.as<float2>() : nullptr, st);
        case ENG_OLS: {
            // overlap-save FIR, then the rotator table multiply
            int rc = eng.launch_ols(false, o, st);
            return rc ? rc : launch_rotate((float2 *)o.out, gtab, n_out, st);
        }
        default:    // generic order (bit-exact) FIR + rotate
            return launch_fir_generic(in_kind == 0 ? FIR_CCC : sh ? FIR_SCC : FIR_FCC, d_taps_generic.as<float>(), ntaps, d_in,
                                      o.out, n_out, decim, gtab, st);
        }
    };
    const FirIo io{d_in, n_in, n_out, demod ? (void *)d_demod : (void *)d_y, n_streams, x_stride, n_lo, out_stride};
    rc = r.epilogue == EPILOGUE_DEMOD_SECOND ? demod_second(io, gain, y_prev, y_last, atan_tab, st, fir) : fir(io);
    if (rc) return rc;
    pos += n_out;
    return GRHIP_OK;
}

}  // namespace grhip

// ============================================================================
// gr_fir_filter_XXX
// ============================================================================
// the body of every set_mode entry.  Not ModeBlock's (stream_block.h): these handles read the mode in work outside
// setter_mutex, which guards only their latched taps, so the setter takes no lock either
template <class H>
static int set_mode_of(H *h, int mode)
{
    if (!h || !mode_valid(mode)) return fail(GRHIP_EINVAL, "bad mode");
    h->mode = mode;
    return GRHIP_OK;
}

// the taps in d_taps order on the device (rev[k] = taps[ntaps-1-k]: correlation order, rev[k] multiplies x[nD + k])
static int upload_reversed(DevBuf &d_taps_rev, const std::vector<float> &taps, int ntaps, int tw, std::vector<float> &rev)
{
    rev.resize(taps.size());
    for (int k = 0; k < ntaps; ++k)
        for (int w = 0; w < tw; ++w) rev[(size_t)k * tw + w] = taps[(size_t)(ntaps - 1 - k) * tw + w];
    return upload(d_taps_rev, rev.data(), rev.size() * sizeof(float));
}

struct grhip_fir_filter : HandleBase {
    FirKind kind;
    int decim = 1;
    int mode = GRHIP_MODE_FAST;
    std::vector<float> taps;        // current forward taps (floats; x2 for ccc)
    std::vector<float> new_taps;    // latched by set_taps
    bool updated = false;
    int ntaps = 0;
    DevBuf d_taps_rev;
    FirEngines eng;                 // FAST mode (fir_plan.h)
    DevBuf d_scratch;               // fsf: the float outputs before the conversion

    int tw() const { return fir_kind_ctaps(kind) ? 2 : 1; }
    size_t in_item() const { return kind == FIR_SCC ? 2 : (kind == FIR_FFF || kind == FIR_FSF || kind == FIR_FCC) ? 4 : 8; }
    size_t out_item() const { return kind == FIR_FFF ? 4 : kind == FIR_FSF ? 2 : 8; }

    int install(const std::vector<float> &t)
    {
        taps = t;
        ntaps = (int)(taps.size() / tw());
        std::vector<float> rev;
        int rc = upload_reversed(d_taps_rev, taps, ntaps, tw(), rev);
        return rc ? rc : eng.build_plain(kind, decim, rev.data(), ntaps);
    }

    int run(const void *d_in, void *d_out, long long n, int dec, hipStream_t st)
    {
        if (n <= 0) return GRHIP_OK;
        if (kind != FIR_FSF) return eng.run_plain(kind, mode, d_taps_rev.as<float>(), d_in, d_out, n, dec, st);
        // fsf: the generic kernel converts itself; FAST runs the fff engines and converts in a pass of its own
        if (!mode_fast(mode)) return launch_fir_generic(kind, d_taps_rev.as<float>(), ntaps, d_in, d_out, n, dec, nullptr, st);
        int rc = d_scratch.reserve((size_t)n * sizeof(float));
        if (!rc) rc = eng.run_plain(FIR_FFF, mode, d_taps_rev.as<float>(), d_in, d_scratch.p, n, dec, st);
        if (!rc) rc = launch_f2s(d_scratch.as<float>(), (short *)d_out, n, st);
        return rc;
    }

    // host buffers: n outputs at decimation dec from (n - 1) * dec + ntaps items; returns n or the error
    long long host_run(const void *in, void *out, long long n, int dec)
    {
        size_t n_in = (size_t)((n - 1) * dec + ntaps);
        if (n_in == 0) n_in = 1;
        return host_call(in, n_in * in_item(), n_in * in_item() + 16, (size_t)n * out_item(), out, out_item(),
                         [&](void *d_in, void *d_out, hipStream_t st) {
                             int rc = run(d_in, d_out, n, dec, st);
                             return rc ? (long long)rc : n;
                         });
    }
};

extern "C" {

int grhip_fir_filter_create(grhip_fir_filter **h, const char *kind, int decimation, const float *taps,
                            size_t ntaps, int device)
{
    if (!h || !kind) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    FirKind k;
    if (!fir_kind_parse(kind, &k)) return fail(GRHIP_EINVAL, "unknown FIR kind '%s'", kind);
    if (decimation < 1) return fail(GRHIP_EINVAL, "decimation must be >= 1");
    if (ntaps && !taps) return fail(GRHIP_EINVAL, "taps is NULL");
    return make_handle(h, [&](grhip_fir_filter *f) {
        f->kind = k; f->decim = decimation; f->mode = default_mode();
        int rc = f->init_device(device);
        if (!rc) rc = f->install(std::vector<float>(taps, taps + ntaps * f->tw()));
        return rc;
    });
}

void grhip_fir_filter_destroy(grhip_fir_filter *h)
{
    destroy_handle(h);
}

int grhip_fir_filter_set_taps(grhip_fir_filter *h, const float *taps, size_t ntaps)
{
    if (!h || (ntaps && !taps)) return fail(GRHIP_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    h->new_taps.assign(taps, taps + ntaps * h->tw());   // d_new_taps (.cc.t:59-64)
    h->updated = true;
    return GRHIP_OK;
}

int grhip_fir_filter_set_mode(grhip_fir_filter *h, int mode) { return set_mode_of(h, mode); }

int grhip_fir_filter_history(const grhip_fir_filter *h)
{
    // set_history(d_fir->ntaps()) (.cc.t:51,77); gr_block history is at least 1
    return h ? (h->ntaps > 0 ? h->ntaps : 1) : GRHIP_EINVAL;
}

int grhip_fir_filter_decimation(const grhip_fir_filter *h) { return h ? h->decim : GRHIP_EINVAL; }

// `st`: the stream this work call will use.  install() rewrites the tap buffers: an earlier *_work_device
// launch may still be reading them, so the streams are drained first.
static int fir_apply_update(grhip_fir_filter *h, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    if (!h->updated) return 0;
    int rc = h->drain(st);
    if (!rc) rc = h->install(h->new_taps);
    if (rc) return rc;
    h->updated = false;
    return 1;
}

int grhip_fir_filter_work_device(grhip_fir_filter *h, int noutput_items, const void *d_in, void *d_out,
                                 void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    int rc = h->bind();
    if (rc) return rc;
    rc = fir_apply_update(h, h->pick(stream));
    if (rc < 0) return rc;
    if (rc == 1) return 0;   // history requirements may have changed (.cc.t:74-79)
    rc = h->run(d_in, d_out, noutput_items, h->decim, h->pick(stream));
    return rc ? rc : noutput_items;
}

int grhip_fir_filter_work(grhip_fir_filter *h, int noutput_items, const void *in, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    int rc = h->bind();
    if (rc) return rc;
    rc = fir_apply_update(h, h->own_stream);
    if (rc < 0) return rc;
    if (rc == 1) return 0;
    if (noutput_items == 0) return 0;
    return (int)h->host_run(in, out, noutput_items, h->decim);
}

int grhip_fir_filterNdec(grhip_fir_filter *h, void *output, const void *input, unsigned long n,
                         unsigned decimate)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (decimate < 1) return fail(GRHIP_EINVAL, "decimate must be >= 1");
    int rc = h->bind();
    if (rc) return rc;
    if (n == 0) return GRHIP_OK;
    const long long r = h->host_run(input, output, (long long)n, (int)decimate);
    return r < 0 ? (int)r : GRHIP_OK;
}

}  // extern "C"

// ============================================================================
// gri_fir_filter_with_buffer_{ccf,ccc,fff}  (second half)
//   filter/gri_fir_filter_with_buffer_XXX.h.t:44-126, .cc.t:30-121
// The reference object owns its delay line (2 * ntaps items, zeroed by set_taps) and is called with NEW
// samples only: filterNdec(out, in, n, dec) consumes n * dec items.  Here the delay line is the last
// ntaps - 1 items, kept in HBM; a call lays [delay line | new items] out once and runs an engine of the FIR
// family over it: out[o] = sum_k rev[k] * both[(dec - 1) + dec * o + k].  GENERIC mode uses the
// reference's own accumulation order (one accumulator, term after term): bit-exact.
// ============================================================================
struct grhip_fir_filter_with_buffer : HandleBase {
    FirKind kind = FIR_CCF;
    int mode = GRHIP_MODE_FAST;
    std::vector<float> rev;             // reversed taps (x2 floats for ccc)
    int ntaps = 0;
    DevBuf d_taps_rev;
    FirEngines eng;                     // FAST mode: engines of the FIR family at the decimation last used
    int eng_dec = 0;                    // (0: none built yet)
    DevBuf d_hist, d_both;
    size_t item() const { return kind == FIR_FFF ? 4 : 8; }
    int tw() const { return kind == FIR_CCC ? 2 : 1; }
    // new taps, delay line zeroed (memset(d_buffer, 0), .cc.t:55-57); nothing of the handle is in flight
    int install(const float *taps, size_t n)
    {
        ntaps = (int)n;
        eng_dec = 0;
        int rc = upload_reversed(d_taps_rev, std::vector<float>(taps, taps + n * tw()), ntaps, tw(), rev);
        const size_t bytes = (size_t)(ntaps > 1 ? ntaps - 1 : 1) * item();
        if (!rc) rc = d_hist.reserve(bytes);
        return rc ? rc : zero_device(d_hist.p, bytes);
    }
    // `st`: the stream of the coming call.  A rebuild rewrites the operands an earlier launch may still be reading
    int ensure_engines(int dec, hipStream_t st)
    {
        if (eng_dec == dec) return GRHIP_OK;
        int rc = eng_dec ? drain(st) : GRHIP_OK;
        eng_dec = 0;
        if (!rc) rc = eng.build_plain(kind, dec, rev.data(), ntaps);
        if (!rc) eng_dec = dec;
        return rc;
    }
};

extern "C" {

int grhip_fir_filter_with_buffer_create(grhip_fir_filter_with_buffer **h, const char *kind, const float *taps,
                                        size_t ntaps, int device)
{
    if (!h || !kind) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    FirKind k;
    if (!fir_kind_parse(kind, &k) || !(k == FIR_CCF || k == FIR_FFF || k == FIR_CCC))
        return fail(GRHIP_EINVAL, "unknown FIR kind '%s'", kind);
    if (ntaps && !taps) return fail(GRHIP_EINVAL, "taps is NULL");
    return make_handle(h, [&](grhip_fir_filter_with_buffer *f) {
        f->kind = k; f->mode = default_mode();
        int rc = f->init_device(device);
        if (rc) return rc;
        return f->install(taps, ntaps);
    });
}

void grhip_fir_filter_with_buffer_destroy(grhip_fir_filter_with_buffer *h)
{
    destroy_handle(h);
}

// set_taps (.cc.t:44-59): new taps, delay line zeroed, takes effect at once (this is a kernel-level object,
// not a block: there is no "returns 0 once")
int grhip_fir_filter_with_buffer_set_taps(grhip_fir_filter_with_buffer *h, const float *taps, size_t ntaps)
{
    if (!h || (ntaps && !taps)) return fail(GRHIP_EINVAL, "null argument");
    int rc = h->bind();
    if (rc) return rc;
    GRHIP_HIP(hipDeviceSynchronize());      // no launch may still be reading the taps or the delay line
    return h->install(taps, ntaps);
}

int grhip_fir_filter_with_buffer_set_mode(grhip_fir_filter_with_buffer *h, int mode) { return set_mode_of(h, mode); }

int grhip_fir_filter_with_buffer_ntaps(const grhip_fir_filter_with_buffer *h) { return h ? h->ntaps : GRHIP_EINVAL; }

int grhip_fir_filter_with_buffer_filterNdec_device(grhip_fir_filter_with_buffer *h, void *d_output, const void *d_input,
                                                   unsigned long n, unsigned long decimate, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (decimate < 1) return fail(GRHIP_EINVAL, "decimate must be >= 1");
    if (n == 0) return GRHIP_OK;
    if (!d_output || !d_input) return fail(GRHIP_EINVAL, "null buffer");
    int rc = h->bind();
    if (rc) return rc;
    hipStream_t st = h->pick(stream);
    const size_t it = h->item(), T = (size_t)h->ntaps, nin = (size_t)n * decimate;
    if (T == 0) {                                   // no taps: every output is the empty sum
        GRHIP_HIP(hipMemsetAsync(d_output, 0, (size_t)n * it, st));
        return GRHIP_OK;
    }
    const size_t H = T - 1;
    if ((rc = h->d_both.reserve((H + nin) * it + 64))) return rc;
    unsigned char *both = h->d_both.as<unsigned char>();
    if (H) GRHIP_HIP(hipMemcpyAsync(both, h->d_hist.p, H * it, hipMemcpyDeviceToDevice, st));
    GRHIP_HIP(hipMemcpyAsync(both + H * it, d_input, nin * it, hipMemcpyDeviceToDevice, st));
    const void *first = both + (decimate - 1) * it;         // window of output 0 ends at new item decimate - 1
    if (!mode_fast(h->mode))        // (GENERIC needs no engines: the reference's order, one accumulator)
        rc = launch_fir_generic(h->kind, h->d_taps_rev.as<float>(), (int)T, first, d_output, (long long)n, (int)decimate,
                                nullptr, st, true);
    else if (!(rc = h->ensure_engines((int)decimate, st)))
        rc = h->eng.run_plain(h->kind, h->mode, h->d_taps_rev.as<float>(), first, d_output, (long long)n, (int)decimate, st);
    if (rc) return rc;
    if (H) GRHIP_HIP(hipMemcpyAsync(h->d_hist.p, both + nin * it, H * it, hipMemcpyDeviceToDevice, st));   // the last ntaps - 1 items
    return GRHIP_OK;
}

int grhip_fir_filter_with_buffer_filterNdec(grhip_fir_filter_with_buffer *h, void *output, const void *input, unsigned long n,
                                            unsigned long decimate)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (decimate < 1) return fail(GRHIP_EINVAL, "decimate must be >= 1");
    if (n == 0) return GRHIP_OK;
    if (!output || !input) return fail(GRHIP_EINVAL, "null buffer");
    int rc = h->bind();
    if (rc) return rc;
    const size_t it = h->item(), nin = (size_t)n * decimate;
    const long long r = h->host_call(input, nin * it, nin * it + 16, (size_t)n * it, output, it,
                                     [&](void *d_in, void *d_out, hipStream_t st) {
                                         rc = grhip_fir_filter_with_buffer_filterNdec_device(h, d_out, d_in, n, decimate, st);
                                         return rc ? (long long)rc : (long long)n;
                                     });
    return r < 0 ? (int)r : GRHIP_OK;
}

}  // extern "C"

// ============================================================================
// gr_quadrature_demod_cf, fused xlating -> demod hier block
// ============================================================================
struct grhip_quadrature_demod_cf : HandleBase {
    float gain = 1.f;
    const DeviceTables *tabs = nullptr;
};

struct grhip_xlating_demod : HandleBase {
    XlatingCore core;
    int mode = GRHIP_MODE_FAST;
    float gain = 1.f;
    const DeviceTables *tabs = nullptr;
    DevBuf ystate;   // float2[4]: [0],[1] ping-pong carry of the demodulator's previous
                     // sample, [2] constant zero (the history item of a fresh block)
    int cur = 0;
    bool fresh = true;
    bool carry_direct = false;   // frame of the carried sample (fir_kernels.h, EPI_DEMOD)
};

static int xlating_args_ok(int decimation, const float *taps, size_t ntaps, double sampling_freq)
{
    if (decimation < 1) return fail(GRHIP_EINVAL, "decimation must be >= 1");
    if (ntaps && !taps) return fail(GRHIP_EINVAL, "taps is NULL");
    if (sampling_freq == 0.0) return fail(GRHIP_EINVAL, "sampling_freq is 0");
    return GRHIP_OK;
}

extern "C" {

// ---- quadrature_demod_cf -----------------------------------------------------
int grhip_quadrature_demod_cf_create(grhip_quadrature_demod_cf **h, float gain, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    return make_handle(h, [&](grhip_quadrature_demod_cf *q) {
        q->gain = gain;
        int rc = q->init_device(device);
        if (!rc) rc = get_device_tables(device, &q->tabs);
        return rc;
    });
}

void grhip_quadrature_demod_cf_destroy(grhip_quadrature_demod_cf *h)
{
    destroy_handle(h);
}

int grhip_quadrature_demod_cf_work_device(grhip_quadrature_demod_cf *h, int noutput_items, const void *d_in,
                                          void *d_out, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    int rc = h->bind();
    if (rc) return rc;
    rc = launch_quad_demod((const float2 *)d_in, (float *)d_out, noutput_items, h->gain, h->tabs->atan_tab,
                           h->pick(stream));
    return rc ? rc : noutput_items;
}

int grhip_quadrature_demod_cf_work(grhip_quadrature_demod_cf *h, int noutput_items, const void *in, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    if (noutput_items == 0) return 0;
    int rc = h->bind();
    if (rc) return rc;
    size_t n = (size_t)noutput_items;
    return (int)h->host_call(in, (n + 1) * 8, (n + 1) * 8, n * 4, out, 4, [&](void *d_in, void *d_out, hipStream_t st) {
        rc = launch_quad_demod((const float2 *)d_in, (float *)d_out, (long long)n, h->gain, h->tabs->atan_tab, st);
        return rc ? rc : noutput_items;
    });
}

// ---- fused xlating -> demod ----------------------------------------------------
int grhip_xlating_demod_create(grhip_xlating_demod **h, int decimation, const float *taps, size_t ntaps,
                               double center_freq, double sampling_freq, float gain, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    int rc = xlating_args_ok(decimation, taps, ntaps, sampling_freq);
    if (rc) return rc;
    return make_handle(h, [&](grhip_xlating_demod *x) {
        x->mode = default_mode();
        x->gain = gain;
        int rc = x->init_device(device);
        if (!rc) rc = get_device_tables(device, &x->tabs);
        if (rc) return rc;
        x->core.decim = decimation;
        x->core.for_demod = true;
        x->core.proto.assign((const cf *)taps, (const cf *)taps + ntaps);
        x->core.center_freq = center_freq; x->core.sampling_freq = sampling_freq;
        if ((rc = x->core.build(device))) return rc;
        if ((rc = x->ystate.reserve(4 * sizeof(float2)))) return rc;
        return zero_device(x->ystate.p, 4 * sizeof(float2));
    });
}

void grhip_xlating_demod_destroy(grhip_xlating_demod *h)
{
    destroy_handle(h);
}

int grhip_xlating_demod_set_mode(grhip_xlating_demod *h, int mode) { return set_mode_of(h, mode); }

int grhip_xlating_demod_reset(grhip_xlating_demod *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    int rc = h->bind();
    if (rc) return rc;
    h->core.reset();     // host-side only: no device work, no synchronisation
    h->fresh = true;
    return GRHIP_OK;
}

int grhip_xlating_demod_history(const grhip_xlating_demod *h)
{
    return h ? (h->core.ntaps > 0 ? h->core.ntaps : 1) : GRHIP_EINVAL;
}

int grhip_xlating_demod_work_device(grhip_xlating_demod *h, int noutput_items, const void *d_in, void *d_out,
                                    void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    if (noutput_items == 0) return 0;
    int rc = h->bind();
    if (rc) return rc;
    long long n = noutput_items;
    long long n_in = (n - 1) * h->core.decim + h->core.ntaps;
    float2 *ys = h->ystate.as<float2>();
    const bool direct = h->core.demod_is_direct(h->mode, true);
    if (!h->fresh && direct != h->carry_direct) {
        // mode switch in mid-stream: move the one-sample carry into the other epilogue's frame
        cf g, y;
        if ((rc = h->core.phase_before_pos(&g))) return rc;
        GRHIP_HIP(hipStreamSynchronize(h->pick(stream)));
        GRHIP_HIP(hipMemcpy(&y, ys + h->cur, sizeof(y), hipMemcpyDeviceToHost));
        y = direct ? y * std::conj(g) : y * g;
        GRHIP_HIP(hipMemcpy(ys + h->cur, &y, sizeof(y), hipMemcpyHostToDevice));
    }
    h->carry_direct = direct;
    rc = h->core.run(h->mode, (const float2 *)d_in, n_in, n, nullptr, (float *)d_out, h->gain,
                     h->fresh ? ys + 2 : ys + h->cur, ys + (h->cur ^ 1), h->tabs->atan_tab, h->pick(stream));
    if (rc) return rc;
    h->cur ^= 1;
    h->fresh = false;
    return noutput_items;
}

int grhip_xlating_demod_run_captures_device(grhip_xlating_demod *h, int n_streams, size_t n_samples,
                                            const void *d_in, size_t in_stride_items, void *d_out,
                                            size_t out_stride_items, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (n_streams < 1) return fail(GRHIP_EINVAL, "n_streams must be >= 1");
    int rc = h->bind();
    if (rc) return rc;
    const long long n_out = (long long)(n_samples / (size_t)h->core.decim);
    if (n_out <= 0) return GRHIP_OK;
    // (GRHIP_MODE_GENERIC: the fused generic-order kernel takes batches at decimation 1 / 2 / 4; run() says so otherwise)
    if (mode_fast(h->mode) && !fir_has_batched_engine(h->core.eng.plan, h->mode))
        return fail(GRHIP_EINVAL, "run_captures needs a batched engine (FAST mode, supported decimation)");
    if (h->core.tab_start != 0 && !h->core.demod_is_direct(h->mode, true, true))
        return fail(GRHIP_EINVAL, "handle has streamed past its cached rotator table; use a fresh handle");
    const long long hist = h->core.ntaps > 0 ? h->core.ntaps - 1 : 0;
    const long long keep = h->core.pos;
    h->core.pos = 0;                                  // every capture starts at rotator phase 1
    rc = h->core.run(h->mode, (const float2 *)d_in - hist, hist + (long long)n_samples, n_out, nullptr,
                     (float *)d_out, h->gain, nullptr, nullptr, h->tabs->atan_tab, h->pick(stream), n_streams,
                     (long long)in_stride_items, hist, (long long)out_stride_items);
    h->core.pos = keep;
    return rc;
}

int grhip_xlating_demod_work(grhip_xlating_demod *h, int noutput_items, const void *in, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    if (noutput_items == 0) return 0;
    int rc = h->bind();
    if (rc) return rc;
    long long n = noutput_items;
    size_t n_in = (size_t)((n - 1) * h->core.decim + h->core.ntaps);
    if (n_in == 0) n_in = 1;
    return (int)h->host_call(in, n_in * 8, n_in * 8 + 16, (size_t)n * 4, out, 4, [&](void *d_in, void *d_out, hipStream_t st) {
        rc = grhip_xlating_demod_work_device(h, noutput_items, d_in, d_out, st);
        return rc < 0 ? rc : noutput_items;
    });
}

}  // extern "C"

// ============================================================================
// gr_freq_xlating_fir_filter_{ccc,ccf,fcf,fcc,scf,scc}, one handle for the family
//   filter/generate_gr_freq_xlating_fir_filter_XXX.py:30 (signatures, FIR_TYPE = gr_fir_ + i_code + cc),
//   filter/gr_freq_xlating_fir_filter_XXX.cc.t:38-123
// The grhip_freq_xlating_fir_filter_ccc_* entries are the family handle of kind "ccc".
// ============================================================================
struct grhip_freq_xlating_fir_filter : HandleBase {
    XlatingCore core;
    int mode = GRHIP_MODE_FAST;
    bool ctaps_in = true;           // ?cc: interleaved complex taps; ?cf: float taps
    size_t in_item = 8;
    // latched by the setters (.cc.t:86-98)
    std::vector<cf> new_proto; double new_center_freq = 0; bool updated = false;

    void set_proto(std::vector<cf> &dst, const float *taps, size_t ntaps) const
    {
        if (ctaps_in) dst.assign((const cf *)taps, (const cf *)taps + ntaps);
        else {
            dst.resize(ntaps);
            for (size_t i = 0; i < ntaps; ++i) dst[i] = cf(taps[i], 0.f);
        }
    }
};

struct grhip_freq_xlating_fir_filter_ccc : grhip_freq_xlating_fir_filter {};

// H: the family handle, or its _ccc type
template <class H>
static int xlating_create(H **h, const char *kind, int decimation, const float *taps, size_t ntaps, double center_freq,
                          double sampling_freq, int device)
{
    if (!h || !kind) return fail(GRHIP_EINVAL, "null argument");
    *h = nullptr;
    int in_kind;
    bool ctaps_in;
    if (!strcmp(kind, "ccc")) { in_kind = 0; ctaps_in = true; }
    else if (!strcmp(kind, "ccf")) { in_kind = 0; ctaps_in = false; }
    else if (!strcmp(kind, "fcf")) { in_kind = 1; ctaps_in = false; }
    else if (!strcmp(kind, "fcc")) { in_kind = 1; ctaps_in = true; }
    else if (!strcmp(kind, "scf")) { in_kind = 2; ctaps_in = false; }
    else if (!strcmp(kind, "scc")) { in_kind = 2; ctaps_in = true; }
    else return fail(GRHIP_EINVAL, "unknown freq_xlating kind '%s'", kind);
    int rc = xlating_args_ok(decimation, taps, ntaps, sampling_freq);
    if (rc) return rc;
    return make_handle(h, [&](H *x) {
        x->mode = default_mode();
        x->ctaps_in = ctaps_in;
        x->in_item = in_kind == 0 ? 8 : in_kind == 1 ? 4 : 2;
        int rc = x->init_device(device);
        if (rc) return rc;
        x->core.decim = decimation;
        x->core.in_kind = in_kind;
        x->core.real_tap_type = !ctaps_in;
        x->set_proto(x->core.proto, taps, ntaps);
        x->core.center_freq = center_freq; x->core.sampling_freq = sampling_freq;
        return x->core.build(device);
    });
}

extern "C" {

int grhip_freq_xlating_fir_filter_create(grhip_freq_xlating_fir_filter **h, const char *kind, int decimation,
                                         const float *taps, size_t ntaps, double center_freq, double sampling_freq,
                                         int device)
{
    return xlating_create(h, kind, decimation, taps, ntaps, center_freq, sampling_freq, device);
}

void grhip_freq_xlating_fir_filter_destroy(grhip_freq_xlating_fir_filter *h) { destroy_handle(h); }

int grhip_freq_xlating_fir_filter_set_center_freq(grhip_freq_xlating_fir_filter *h, double center_freq)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    if (!h->updated) h->new_proto = h->core.proto;
    h->new_center_freq = center_freq;
    h->updated = true;
    return GRHIP_OK;
}

int grhip_freq_xlating_fir_filter_set_taps(grhip_freq_xlating_fir_filter *h, const float *taps, size_t ntaps)
{
    if (!h || (ntaps && !taps)) return fail(GRHIP_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    if (!h->updated) h->new_center_freq = h->core.center_freq;
    h->set_proto(h->new_proto, taps, ntaps);
    h->updated = true;
    return GRHIP_OK;
}

int grhip_freq_xlating_fir_filter_set_mode(grhip_freq_xlating_fir_filter *h, int mode) { return set_mode_of(h, mode); }

int grhip_freq_xlating_fir_filter_history(const grhip_freq_xlating_fir_filter *h)
{
    return h ? (h->core.ntaps > 0 ? h->core.ntaps : 1) : GRHIP_EINVAL;
}

int grhip_freq_xlating_fir_filter_decimation(const grhip_freq_xlating_fir_filter *h) { return h ? h->core.decim : GRHIP_EINVAL; }

int grhip_freq_xlating_fir_filter_reset(grhip_freq_xlating_fir_filter *h)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    h->core.reset();
    return GRHIP_OK;
}

// work(): set_history; build_composite_fir(); d_updated = false; return 0 (.cc.t:109-114).
// NB the reference keeps the rotator's d_phase/d_counter and only replaces
// d_phase_incr; XlatingCore::rebuild_keep_phase does the same.
static int xlf_apply_update(grhip_freq_xlating_fir_filter *h, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    if (!h->updated) return 0;
    int rc = h->drain(st);       // see fir_apply_update
    if (rc) return rc;
    h->core.proto = h->new_proto;
    h->core.center_freq = h->new_center_freq;
    rc = h->core.rebuild_keep_phase(h->device);
    if (rc) return rc;
    h->updated = false;
    return 1;
}

int grhip_freq_xlating_fir_filter_work_device(grhip_freq_xlating_fir_filter *h, int noutput_items, const void *d_in,
                                              void *d_out, void *stream)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    int rc = h->bind();
    if (rc) return rc;
    rc = xlf_apply_update(h, h->pick(stream));
    if (rc < 0) return rc;
    if (rc == 1) return 0;
    long long n = noutput_items;
    long long n_in = n > 0 ? (n - 1) * h->core.decim + h->core.ntaps : 0;
    rc = h->core.run(h->mode, (const float2 *)d_in, n_in, n, (float2 *)d_out, nullptr, 0.f, nullptr, nullptr, nullptr,
                     h->pick(stream));
    return rc ? rc : noutput_items;
}

int grhip_freq_xlating_fir_filter_work(grhip_freq_xlating_fir_filter *h, int noutput_items, const void *in, void *out)
{
    if (!h) return fail(GRHIP_EINVAL, "null handle");
    if (noutput_items < 0) return fail(GRHIP_EINVAL, "negative noutput_items");
    int rc = h->bind();
    if (rc) return rc;
    rc = xlf_apply_update(h, h->own_stream);
    if (rc < 0) return rc;
    if (rc == 1) return 0;
    if (noutput_items == 0) return 0;
    long long n = noutput_items;
    size_t n_in = (size_t)((n - 1) * h->core.decim + h->core.ntaps);
    if (n_in == 0) n_in = 1;
    const size_t it = h->in_item;
    return (int)h->host_call(in, n_in * it, n_in * it + 16, (size_t)n * 8, out, 8, [&](void *d_in, void *d_out, hipStream_t st) {
        rc = h->core.run(h->mode, (const float2 *)d_in, (long long)n_in, n, (float2 *)d_out, nullptr, 0.f, nullptr, nullptr,
                         nullptr, st);
        return rc ? rc : noutput_items;
    });
}

// ---- gr_freq_xlating_fir_filter_ccc: forwards to the family entries ----
int grhip_freq_xlating_fir_filter_ccc_create(grhip_freq_xlating_fir_filter_ccc **h, int decimation, const float *taps,
                                             size_t ntaps, double center_freq, double sampling_freq, int device)
{
    return xlating_create(h, "ccc", decimation, taps, ntaps, center_freq, sampling_freq, device);
}

void grhip_freq_xlating_fir_filter_ccc_destroy(grhip_freq_xlating_fir_filter_ccc *h) { destroy_handle(h); }

int grhip_freq_xlating_fir_filter_ccc_set_center_freq(grhip_freq_xlating_fir_filter_ccc *h, double center_freq)
{
    return grhip_freq_xlating_fir_filter_set_center_freq(h, center_freq);
}

int grhip_freq_xlating_fir_filter_ccc_set_taps(grhip_freq_xlating_fir_filter_ccc *h, const float *taps, size_t ntaps)
{
    return grhip_freq_xlating_fir_filter_set_taps(h, taps, ntaps);
}

int grhip_freq_xlating_fir_filter_ccc_set_mode(grhip_freq_xlating_fir_filter_ccc *h, int mode)
{
    return grhip_freq_xlating_fir_filter_set_mode(h, mode);
}

int grhip_freq_xlating_fir_filter_ccc_history(const grhip_freq_xlating_fir_filter_ccc *h)
{
    return grhip_freq_xlating_fir_filter_history(h);
}

int grhip_freq_xlating_fir_filter_ccc_reset(grhip_freq_xlating_fir_filter_ccc *h) { return grhip_freq_xlating_fir_filter_reset(h); }

int grhip_freq_xlating_fir_filter_ccc_work(grhip_freq_xlating_fir_filter_ccc *h, int noutput_items, const void *in, void *out)
{
    return grhip_freq_xlating_fir_filter_work(h, noutput_items, in, out);
}

int grhip_freq_xlating_fir_filter_ccc_work_device(grhip_freq_xlating_fir_filter_ccc *h, int noutput_items, const void *d_in,
                                                  void *d_out, void *stream)
{
    return grhip_freq_xlating_fir_filter_work_device(h, noutput_items, d_in, d_out, stream);
}

}  // extern "C"
