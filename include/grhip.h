/*
 * grhip.h -- C ABI of libgrhip.so: the MI355X (gfx950) implementation of the
 * GNU Radio 3.5.0 DMR demodulation hot path.
 *
 * Plain C types only; no exceptions cross this boundary.  Every entry point
 * returns an int status (GRHIP_OK or a negative GRHIP_E*), except the *_work
 * calls which return the number of items produced (>= 0) like
 * gr_block::general_work (gnuradio-core/src/lib/runtime/gr_block.h:107-127)
 * or a negative GRHIP_E*.
 *
 * Each block type mirrors one reference block.  The citation on every group
 * names the reference interface it replaces (paths relative to the reference
 * tree).  Semantics common to all blocks:
 *
 *  - *_work(h, noutput_items, in, out): HOST pointers, same contract as
 *    gr_sync_block / gr_sync_decimator ::work: `in` points at the oldest
 *    history item, i.e. in[0 .. history-2] are items the block saw before
 *    (runtime/gr_block.h:76-84, runtime/gr_sync_block.cc:46-50), and
 *    noutput_items*decimation + history - 1 items are readable
 *    (runtime/gr_sync_decimator.cc:46-50).  The call copies to the device,
 *    runs the kernels on the handle's stream, copies back and returns when
 *    the output is in `out`.
 *  - *_work_device(..., stream): same contract with DEVICE pointers; enqueues
 *    on `stream` (a hipStream_t passed as void*; NULL = the handle's own
 *    stream) and returns without synchronising.
 *  - device pointers need the natural alignment of their item (1, 2, 4 or 8
 *    bytes; a gr_buffer's read and write pointers advance by whole items) and
 *    nothing more, and a stream stride is any item count.  Wider alignment, or
 *    a stride that keeps every stream on a 16-byte boundary, only selects a
 *    faster path; the results are the same.  A pointer that is not aligned to
 *    its item is the caller's error: some entries return GRHIP_EINVAL for it,
 *    at the others the behaviour is undefined.  Exceptions are stated at the entry
 *    (tests/test_gpu_device_offsets.py lists them and runs every other entry
 *    at every item offset).
 *  - setters latch a new value that takes effect at the next work call, which
 *    then returns 0 items once, exactly as the reference does
 *    (filter/gr_fir_filter_XXX.cc.t:74-79,
 *     filter/gr_freq_xlating_fir_filter_XXX.cc.t:109-114).
 *  - one handle is driven by one thread at a time (thread-per-block scheduler,
 *    runtime/gr_scheduler_tpb.cc:70-77); setters may be called from another
 *    thread.
 *  - complex items are interleaved float (re, im) == gr_complex
 *    (runtime/gr_complex.h:26).
 */
#ifndef INCLUDED_GRHIP_H
#define INCLUDED_GRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define GRHIP_API __attribute__((visibility("default")))
#else
#define GRHIP_API
#endif

/* ---- status codes -------------------------------------------------------
 * The C++ block wrappers rethrow them as the exception type the reference
 * throws for the same precondition. */
#define GRHIP_OK 0
#define GRHIP_EINVAL (-1)   /* std::invalid_argument */
#define GRHIP_ERANGE (-2)   /* std::out_of_range     */
#define GRHIP_ERUNTIME (-3) /* std::runtime_error (HIP call failed) */
#define GRHIP_ENOMEM (-4)   /* std::bad_alloc        */
#define GRHIP_ENODEV (-5)   /* no usable gfx950 device / HIP runtime */
/* NOT an error: a work call's way to say WORK_DONE (runtime/gr_block.h:63-66, where it is -1).  The
 * reference's -1 would collide with GRHIP_EINVAL, so the ABI reports it as the largest int, which no
 * call can produce as an item count (grhip_head never copies more than INT_MAX - 1 items per call).
 * Every negative return is an error. */
#define GRHIP_WORK_DONE 0x7fffffff

GRHIP_API const char *grhip_strerror(int status);
/* thread-local detail of the last failing call on this thread ("" if none) */
GRHIP_API const char *grhip_last_error(void);
GRHIP_API int grhip_device_count(int *count);
/* blocks until everything enqueued on the handle-independent default work has
 * finished on `device` (hipDeviceSynchronize) */
GRHIP_API int grhip_device_synchronize(int device);
GRHIP_API const char *grhip_version(void);

/* numeric mode of the FIR-type blocks (process-wide default, may be
 * overridden per handle):
 *   GRHIP_MODE_FAST    fastest engine for the shape, own summation order (within
 *                      1e-5 relative of the reference): tiled vector-FMA kernels, the
 *                      overlap-save engine, and -- long real-tap filters at decimation
 *                      2 / 4 -- the matrix-core engine (split-binary16 MFMA, f32
 *                      accumulation; csrc/fir_mfma.hip)
 *   GRHIP_MODE_FAST_VALU  as FAST but never the matrix cores: f32 FMAs on the vector
 *                      pipes only (the north-star's "no MFMA" form; ~2x slower at 256 taps)
 *   GRHIP_MODE_FAST_REFTAPS  as FAST, and freq_xlating's matrix-core engine also reproduces the
 *                      reference's TAP-ANGLE QUANTISATION -- its composite taps are
 *                      proto[i] * exp(j * (float)(i * fwT0)), the product rounded to binary32
 *                      (filter/gr_freq_xlating_fir_filter_XXX.cc.t:79): up to 7.6e-6 rad per tap at 256
 *                      taps, which FAST's exact angles do not carry -- to first order, by a second band
 *                      matrix on the middle k-steps.  cfg2, per element of the demodulator output: 1.16e-5
 *                      against the reference's generic build and 8.9e-6 against its SSE build (the two are
 *                      9.9e-6 apart; FAST: 1.80e-5), at 0.92 of FAST's rate.  Shapes the matrix-core
 *                      engine does not take run as in FAST.
 *   GRHIP_MODE_GENERIC summation order and unfused arithmetic of
 *                      gr_fir_XXX_generic (filter/gr_fir_XXX_generic.cc.t:30-79):
 *                      bit-exact against the generic reference path
 * Error bound of the matrix-core engine (FAST, FAST_REFTAPS): every staged tile of ~2000 outputs is scaled by ONE
 * power of two taken from its largest finite sample, so |error| <= 2^-21 * sum|taps| * (largest |sample| of the
 * tile): absolute within a tile, not relative to the local signal (a quiet stretch beside a burst keeps the
 * infinity-norm tolerance, not a per-element one); a non-finite sample spoils the outputs whose window holds it and
 * at most the rest of their 16-output block. */
#define GRHIP_MODE_FAST 0
#define GRHIP_MODE_GENERIC 1
#define GRHIP_MODE_FAST_VALU 2
#define GRHIP_MODE_FAST_REFTAPS 3
GRHIP_API int grhip_set_default_mode(int mode);
GRHIP_API int grhip_get_default_mode(void);

/* ======================================================================
 * gr_fir_filter_{ccf,fff,ccc,fcc,scc,fsf}
 *   replaces gr_make_fir_filter_XXX(int decimation, const std::vector<TAP>&)
 *   filter/gr_fir_filter_XXX.h.t:36-66, filter/gr_fir_filter_XXX.cc.t:37-88
 *   (signatures: filter/generate_utils.py:25)
 * kind: "ccf" | "fff" | "ccc" | "fcc" | "scc" | "fsf".  taps in forward order (complex taps
 * interleaved, ntaps counts taps not floats).  history = ntaps.
 *   kind  item in  item out  taps
 *   fcc   float    complex   complex      real input: float / int16 items read as they are (no widened copy)
 *   scc   int16    complex   complex
 *   fsf   float    int16     float        output (short)acc as the reference's x86-64 build converts it:
 *                                         truncation to int32, low 16 bits; NaN and |acc| >= 2^31 give 0
 * GRHIP_MODE_GENERIC: gr_fir_XXX_generic's order (filter/gr_fir_XXX_generic.cc.t as generate_gr_fir_XXX.py:31-66
 * expands it: fcc / scc N_UNROLL 2 with complex * float products, scc's (float) cast; fsf N_UNROLL 4), bit-exact.
 * FAST: fcc / scc at decimation 1 / 2 / 4 / 8 with up to 1024 taps run the real-input kernel (fir_realin.hip, 1e-5);
 * other shapes run the generic-order kernel.  fsf runs fff's FAST engines, then the conversion (within 1 LSB).
 * ====================================================================== */
typedef struct grhip_fir_filter grhip_fir_filter;
GRHIP_API int grhip_fir_filter_create(grhip_fir_filter **h, const char *kind, int decimation,
                                      const float *taps, size_t ntaps, int device);
GRHIP_API void grhip_fir_filter_destroy(grhip_fir_filter *h);
GRHIP_API int grhip_fir_filter_set_taps(grhip_fir_filter *h, const float *taps, size_t ntaps);
GRHIP_API int grhip_fir_filter_set_mode(grhip_fir_filter *h, int mode);
GRHIP_API int grhip_fir_filter_history(const grhip_fir_filter *h);
GRHIP_API int grhip_fir_filter_decimation(const grhip_fir_filter *h);
GRHIP_API int grhip_fir_filter_work(grhip_fir_filter *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_fir_filter_work_device(grhip_fir_filter *h, int noutput_items, const void *d_in,
                                           void *d_out, void *stream);
/* kernel-level seam: gr_fir_XXX::filterN / filterNdec
 * (filter/gr_fir_XXX.h.t:87-100): output[i] = filter(&input[i*decimate]);
 * ignores latched updates, never returns 0-because-updated. */
GRHIP_API int grhip_fir_filterNdec(grhip_fir_filter *h, void *output, const void *input,
                                   unsigned long n, unsigned decimate);

/* ======================================================================
 * gri_fir_filter_with_buffer_{ccf,ccc,fff}  (the FIR kernel object that owns its delay line)
 *   replaces gri_fir_filter_with_buffer_XXX(const std::vector<TAP> &taps)
 *   filter/gri_fir_filter_with_buffer_XXX.h.t:44-126, .cc.t:30-121
 * kind "ccf" | "ccc" | "fff"; taps in forward order.  filterNdec(output, input, n, decimate) takes NEW items
 * only (n * decimate of them) -- output[i] = filter(&input[i * decimate], decimate), .cc.t:110-121; filterN is
 * decimate = 1 and filter(x) is n = 1 -- and continues from the delay line the previous calls left
 * (zeros after create / set_taps, .cc.t:44-59).  GRHIP_MODE_GENERIC accumulates in the reference's order
 * (one accumulator, term after term, .cc.t:75-79): bit-exact.  A kernel-level object: set_taps acts at once.
 * ====================================================================== */
typedef struct grhip_fir_filter_with_buffer grhip_fir_filter_with_buffer;
GRHIP_API int grhip_fir_filter_with_buffer_create(grhip_fir_filter_with_buffer **h, const char *kind, const float *taps,
                                                  size_t ntaps, int device);
GRHIP_API void grhip_fir_filter_with_buffer_destroy(grhip_fir_filter_with_buffer *h);
GRHIP_API int grhip_fir_filter_with_buffer_set_taps(grhip_fir_filter_with_buffer *h, const float *taps, size_t ntaps);
GRHIP_API int grhip_fir_filter_with_buffer_set_mode(grhip_fir_filter_with_buffer *h, int mode);
GRHIP_API int grhip_fir_filter_with_buffer_ntaps(const grhip_fir_filter_with_buffer *h);
GRHIP_API int grhip_fir_filter_with_buffer_filterNdec(grhip_fir_filter_with_buffer *h, void *output, const void *input,
                                                      unsigned long n, unsigned long decimate);
GRHIP_API int grhip_fir_filter_with_buffer_filterNdec_device(grhip_fir_filter_with_buffer *h, void *d_output,
                                                             const void *d_input, unsigned long n,
                                                             unsigned long decimate, void *stream);

/* ======================================================================
 * gr_freq_xlating_fir_filter_ccc
 *   replaces gr_make_freq_xlating_fir_filter_ccc(int decimation,
 *       const std::vector<gr_complex>& taps, double center_freq, double sampling_freq)
 *   filter/gr_freq_xlating_fir_filter_XXX.h.t:64-99, .cc.t:38-123
 * history = ntaps.  Carries the gr_rotator state (filter/gr_rotator.h:29-52)
 * across calls.
 * ====================================================================== */
typedef struct grhip_freq_xlating_fir_filter_ccc grhip_freq_xlating_fir_filter_ccc;
GRHIP_API int grhip_freq_xlating_fir_filter_ccc_create(grhip_freq_xlating_fir_filter_ccc **h,
                                                       int decimation, const float *taps,
                                                       size_t ntaps, double center_freq,
                                                       double sampling_freq, int device);
GRHIP_API void grhip_freq_xlating_fir_filter_ccc_destroy(grhip_freq_xlating_fir_filter_ccc *h);
GRHIP_API int grhip_freq_xlating_fir_filter_ccc_set_center_freq(grhip_freq_xlating_fir_filter_ccc *h,
                                                               double center_freq);
GRHIP_API int grhip_freq_xlating_fir_filter_ccc_set_taps(grhip_freq_xlating_fir_filter_ccc *h,
                                                        const float *taps, size_t ntaps);
GRHIP_API int grhip_freq_xlating_fir_filter_ccc_set_mode(grhip_freq_xlating_fir_filter_ccc *h, int mode);
GRHIP_API int grhip_freq_xlating_fir_filter_ccc_history(const grhip_freq_xlating_fir_filter_ccc *h);
GRHIP_API int grhip_freq_xlating_fir_filter_ccc_work(grhip_freq_xlating_fir_filter_ccc *h,
                                                     int noutput_items, const void *in, void *out);
GRHIP_API int grhip_freq_xlating_fir_filter_ccc_work_device(grhip_freq_xlating_fir_filter_ccc *h,
                                                            int noutput_items, const void *d_in,
                                                            void *d_out, void *stream);
/* restart the stream (rotator phase 1, counter 0) without rebuilding taps:
 * what constructing a fresh block for the next capture does. */
GRHIP_API int grhip_freq_xlating_fir_filter_ccc_reset(grhip_freq_xlating_fir_filter_ccc *h);

/* ======================================================================
 * gr_freq_xlating_fir_filter_{ccf,fcf,fcc,scf,scc} (and ccc): one handle for the family
 *   replaces gr_make_freq_xlating_fir_filter_XXX(int decimation, const std::vector<TAP>& taps,
 *       double center_freq, double sampling_freq)
 *   filter/generate_gr_freq_xlating_fir_filter_XXX.py:30, filter/gr_freq_xlating_fir_filter_XXX.cc.t:38-123
 * kind: "ccf" | "fcf" | "fcc" | "scf" | "scc" | "ccc" (items in: c complex, f float, s int16; out: complex).
 * taps: float for ?cf, interleaved complex for ?cc (ntaps counts taps).  The contract of _ccc: history = ntaps,
 * set_center_freq / set_taps latch and the next work returns 0 once, set_center_freq keeps the rotator phase and
 * counter (.cc.t:82).  Composite taps with the reference's arithmetic (.cc.t:72-83): for ?cf, proto[i] * exp(...) is
 * float * complex = (a*c, a*d).  Inner FIR (FIR_TYPE = gr_fir_ + i_code + cc): gr_fir_ccc for ccf / ccc, gr_fir_fcc
 * for fcf / fcc, gr_fir_scc for scf / scc.  "ccc" gives the _ccc entries' results bit for bit.
 * GRHIP_MODE_GENERIC: bit-exact.  FAST: ccf / ccc run the complex-input engines of _ccc; the real-input kinds run
 * the real-input kernel (fir_realin.hip) at decimation 1 / 2 / 4 / 8 with up to 1024 taps, otherwise the
 * generic-order kernel, both with the rotator table multiply in the epilogue.
 * ====================================================================== */
typedef struct grhip_freq_xlating_fir_filter grhip_freq_xlating_fir_filter;
GRHIP_API int grhip_freq_xlating_fir_filter_create(grhip_freq_xlating_fir_filter **h, const char *kind, int decimation,
                                                   const float *taps, size_t ntaps, double center_freq,
                                                   double sampling_freq, int device);
GRHIP_API void grhip_freq_xlating_fir_filter_destroy(grhip_freq_xlating_fir_filter *h);
GRHIP_API int grhip_freq_xlating_fir_filter_set_center_freq(grhip_freq_xlating_fir_filter *h, double center_freq);
GRHIP_API int grhip_freq_xlating_fir_filter_set_taps(grhip_freq_xlating_fir_filter *h, const float *taps, size_t ntaps);
GRHIP_API int grhip_freq_xlating_fir_filter_set_mode(grhip_freq_xlating_fir_filter *h, int mode);
GRHIP_API int grhip_freq_xlating_fir_filter_history(const grhip_freq_xlating_fir_filter *h);
GRHIP_API int grhip_freq_xlating_fir_filter_decimation(const grhip_freq_xlating_fir_filter *h);
GRHIP_API int grhip_freq_xlating_fir_filter_reset(grhip_freq_xlating_fir_filter *h);
GRHIP_API int grhip_freq_xlating_fir_filter_work(grhip_freq_xlating_fir_filter *h, int noutput_items, const void *in,
                                                 void *out);
GRHIP_API int grhip_freq_xlating_fir_filter_work_device(grhip_freq_xlating_fir_filter *h, int noutput_items,
                                                        const void *d_in, void *d_out, void *stream);

/* ======================================================================
 * gr_quadrature_demod_cf
 *   replaces gr_make_quadrature_demod_cf(float gain)
 *   general/gr_quadrature_demod_cf.h, general/gr_quadrature_demod_cf.cc:31-62
 *   (+ gr_fast_atan2f, general/gr_fast_atan2f.cc:125-198).  history = 2.
 * ====================================================================== */
typedef struct grhip_quadrature_demod_cf grhip_quadrature_demod_cf;
GRHIP_API int grhip_quadrature_demod_cf_create(grhip_quadrature_demod_cf **h, float gain, int device);
GRHIP_API void grhip_quadrature_demod_cf_destroy(grhip_quadrature_demod_cf *h);
GRHIP_API int grhip_quadrature_demod_cf_work(grhip_quadrature_demod_cf *h, int noutput_items,
                                             const void *in, void *out);
GRHIP_API int grhip_quadrature_demod_cf_work_device(grhip_quadrature_demod_cf *h, int noutput_items,
                                                    const void *d_in, void *d_out, void *stream);

/* ======================================================================
 * Fused hier block: freq_xlating_fir_filter_ccc -> quadrature_demod_cf
 * (what tb.connect(xlating, demod) builds; one kernel, the xlating output
 * never goes to HBM).  Same arguments as the two blocks.  `in` has the
 * xlating history (ntaps-1) in front; out is float.  Carries the rotator and
 * the demodulator's previous sample across calls.
 * ====================================================================== */
typedef struct grhip_xlating_demod grhip_xlating_demod;
GRHIP_API int grhip_xlating_demod_create(grhip_xlating_demod **h, int decimation, const float *taps,
                                         size_t ntaps, double center_freq, double sampling_freq,
                                         float gain, int device);
GRHIP_API void grhip_xlating_demod_destroy(grhip_xlating_demod *h);
GRHIP_API int grhip_xlating_demod_set_mode(grhip_xlating_demod *h, int mode);
GRHIP_API int grhip_xlating_demod_reset(grhip_xlating_demod *h);
GRHIP_API int grhip_xlating_demod_history(const grhip_xlating_demod *h);
GRHIP_API int grhip_xlating_demod_work(grhip_xlating_demod *h, int noutput_items, const void *in,
                                       void *out);
GRHIP_API int grhip_xlating_demod_work_device(grhip_xlating_demod *h, int noutput_items,
                                              const void *d_in, void *d_out, void *stream);
/* n_streams independent captures in ONE launch, every one of them processed
 * like a fresh block instance (rotator phase 1, demodulator history 0): what
 * n_streams flowgraphs with identical parameters compute.  Capture s starts at
 * d_in + s*in_stride_items complex items and has NO history in front (the
 * ntaps-1 zeros a fresh flowgraph preloads are supplied by the kernel);
 * n_samples items each; output s at d_out + s*out_stride_items floats,
 * n_samples/decimation items.  Does not touch the handle's streaming state.
 * FAST modes: every shape a batched engine takes.  GRHIP_MODE_GENERIC (bit-exact against the reference's generic
 * build): decimation 1 / 2 / 4 with at least 8 taps and a tile that fits local memory,
 * decimation * (1024 + ntaps / decimation + 3) * 8 + ntaps * 8 + 64 <= 150 KiB (about 9000 taps at decimation 1, 7500
 * at 4), and with more than one capture an even in_stride_items (an exception to the common rule on strides: every
 * capture must sit at the same offset from a 16-byte boundary; d_in itself needs only a complex item's alignment);
 * other shapes, an odd in_stride_items among them, return GRHIP_EINVAL and write nothing (run them a capture at a
 * time through work_device). */
GRHIP_API int grhip_xlating_demod_run_captures_device(grhip_xlating_demod *h, int n_streams,
                                                      size_t n_samples, const void *d_in,
                                                      size_t in_stride_items, void *d_out,
                                                      size_t out_stride_items, void *stream);

/* ======================================================================
 * digital_clock_recovery_mm_ff
 *   replaces digital_make_clock_recovery_mm_ff(float omega, float gain_omega,
 *       float mu, float gain_mu, float omega_relative_limit)
 *   gr-digital/include/digital_clock_recovery_mm_ff.h:44-92,
 *   gr-digital/lib/digital_clock_recovery_mm_ff.cc:37-139
 * general_work contract: consumes *consumed items (consume_each), returns
 * items produced; uses at most ninput_items - 8 inputs (.cc:113).
 * GRHIP_ERANGE if omega < 1 or a gain is negative (.cc:58-61).
 * Deviation: a loop whose timing error drives its sample position below 0
 * (a step back before the first item of the call's buffer) ends there: the
 * reference goes on and reads before its buffer.  The symbols up to that
 * point are the reference's, *consumed is the negative position, and the
 * handle stays ended: later general_work calls produce and consume nothing.
 * The device form reports the negative position in d_counts[1] and leaves
 * stopping to the caller.
 * ====================================================================== */
typedef struct grhip_clock_recovery_mm_ff grhip_clock_recovery_mm_ff;
GRHIP_API int grhip_clock_recovery_mm_ff_create(grhip_clock_recovery_mm_ff **h, float omega,
                                                float gain_omega, float mu, float gain_mu,
                                                float omega_relative_limit, int device);
GRHIP_API void grhip_clock_recovery_mm_ff_destroy(grhip_clock_recovery_mm_ff *h);
GRHIP_API int grhip_clock_recovery_mm_ff_forecast(const grhip_clock_recovery_mm_ff *h, int noutput_items);
GRHIP_API int grhip_clock_recovery_mm_ff_general_work(grhip_clock_recovery_mm_ff *h, int noutput_items,
                                                      int ninput_items, const float *in, float *out,
                                                      int *consumed);
/* device form: produced/consumed are written to d_counts[0], d_counts[1]
 * (device int[2]) so a following kernel can read them without a host sync */
GRHIP_API int grhip_clock_recovery_mm_ff_general_work_device(grhip_clock_recovery_mm_ff *h,
                                                             int noutput_items, int ninput_items,
                                                             const float *d_in, float *d_out,
                                                             int *d_counts, void *stream);
GRHIP_API float grhip_clock_recovery_mm_ff_mu(grhip_clock_recovery_mm_ff *h);
GRHIP_API float grhip_clock_recovery_mm_ff_omega(grhip_clock_recovery_mm_ff *h);
GRHIP_API float grhip_clock_recovery_mm_ff_gain_mu(grhip_clock_recovery_mm_ff *h);
GRHIP_API float grhip_clock_recovery_mm_ff_gain_omega(grhip_clock_recovery_mm_ff *h);
GRHIP_API int grhip_clock_recovery_mm_ff_set_gain_mu(grhip_clock_recovery_mm_ff *h, float v);
GRHIP_API int grhip_clock_recovery_mm_ff_set_gain_omega(grhip_clock_recovery_mm_ff *h, float v);
GRHIP_API int grhip_clock_recovery_mm_ff_set_mu(grhip_clock_recovery_mm_ff *h, float v);
GRHIP_API int grhip_clock_recovery_mm_ff_set_omega(grhip_clock_recovery_mm_ff *h, float v);

/* ======================================================================
 * digital_binary_slicer_fb
 *   replaces digital_make_binary_slicer_fb()
 *   gr-digital/lib/digital_binary_slicer_fb.cc:31-59
 * ====================================================================== */
typedef struct grhip_binary_slicer_fb grhip_binary_slicer_fb;
GRHIP_API int grhip_binary_slicer_fb_create(grhip_binary_slicer_fb **h, int device);
GRHIP_API void grhip_binary_slicer_fb_destroy(grhip_binary_slicer_fb *h);
GRHIP_API int grhip_binary_slicer_fb_work(grhip_binary_slicer_fb *h, int noutput_items,
                                          const float *in, unsigned char *out);
GRHIP_API int grhip_binary_slicer_fb_work_device(grhip_binary_slicer_fb *h, int noutput_items,
                                                 const float *d_in, unsigned char *d_out, void *stream);

/* ======================================================================
 * pager_slicer_fb  (the 4-level symbol decisions a 4FSK chain needs)
 *   replaces pager_make_slicer_fb(float alpha)
 *   gr-pager/lib/pager_slicer_fb.h:30-58, pager_slicer_fb.cc:34-84
 * One-pole DC tracker (d_avg = d_avg*beta + x*alpha, floats) followed by the
 * decisions {0,1,2,3} at -2, 0, +2 of the DC-free sample.  The tracker is a
 * serial float recurrence: bit-exact, one wavefront per stream.
 * ====================================================================== */
typedef struct grhip_pager_slicer_fb grhip_pager_slicer_fb;
GRHIP_API int grhip_pager_slicer_fb_create(grhip_pager_slicer_fb **h, float alpha, int device);
GRHIP_API void grhip_pager_slicer_fb_destroy(grhip_pager_slicer_fb *h);
GRHIP_API int grhip_pager_slicer_fb_work(grhip_pager_slicer_fb *h, int noutput_items,
                                         const float *in, unsigned char *out);
GRHIP_API int grhip_pager_slicer_fb_work_device(grhip_pager_slicer_fb *h, int noutput_items,
                                                const float *d_in, unsigned char *d_out, void *stream);
/* pager_slicer_fb::dc_offset() (.h:56); synchronises with the handle's last launch */
GRHIP_API int grhip_pager_slicer_fb_dc_offset(grhip_pager_slicer_fb *h, float *dc_offset);

/* ======================================================================
 * gr_unpack_k_bits_bb  (dibits -> bits ahead of the correlator)
 *   replaces gr_make_unpack_k_bits_bb(unsigned k)
 *   general/gr_unpack_k_bits_bb.cc:32-74  (gr_sync_interpolator, k outputs per input,
 *   most significant of the k bits first); GRHIP_ERANGE if k == 0 (.cc:45-46),
 *   GRHIP_EINVAL if k > 32 (the reference shifts an unsigned int by up to k-1).
 *   noutput_items must be a multiple of k (the scheduler guarantees it, .cc:72).
 * ====================================================================== */
typedef struct grhip_unpack_k_bits_bb grhip_unpack_k_bits_bb;
GRHIP_API int grhip_unpack_k_bits_bb_create(grhip_unpack_k_bits_bb **h, unsigned k, int device);
GRHIP_API void grhip_unpack_k_bits_bb_destroy(grhip_unpack_k_bits_bb *h);
GRHIP_API int grhip_unpack_k_bits_bb_work(grhip_unpack_k_bits_bb *h, int noutput_items,
                                          const unsigned char *in, unsigned char *out);
GRHIP_API int grhip_unpack_k_bits_bb_work_device(grhip_unpack_k_bits_bb *h, int noutput_items,
                                                 const unsigned char *d_in, unsigned char *d_out, void *stream);

/* ======================================================================
 * gr_stream_to_vector, gr_vector_to_streams, gr_head  (the remaining harness adapters)
 *   gr_make_stream_to_vector(size_t item_size, size_t nitems_per_block)
 *       general/gr_stream_to_vector.cc:31-60: gr_sync_decimator, work = one memcpy: grouping items into
 *       vectors moves no data;
 *   gr_make_head(size_t sizeof_stream_item, unsigned long long nitems)
 *       general/gr_head.cc:31-62: copies until nitems have passed, then work() returns WORK_DONE --
 *       GRHIP_WORK_DONE here (the reference's -1 is an error code of this ABI);
 *   gr_make_vector_to_streams(size_t item_size, size_t nstreams)
 *       general/gr_vector_to_streams.cc:31-70: item j of every input vector goes to stream j -- the data
 *       movement of gr_stream_to_streams: create it with grhip_stream_adapter_create(split = 1, ...).
 * work(): host pointers (a host memcpy, as the reference); work_device(): device pointers, the copy is
 * queued on `stream` (0 = the handle's own).  noutput_items counts OUTPUT items (vectors for
 * stream_to_vector).
 * ====================================================================== */
typedef struct grhip_copy_adapter grhip_copy_adapter;
GRHIP_API int grhip_stream_to_vector_create(grhip_copy_adapter **h, size_t item_size, size_t nitems_per_block,
                                            int device);
GRHIP_API int grhip_head_create(grhip_copy_adapter **h, size_t sizeof_stream_item, unsigned long long nitems,
                                int device);
GRHIP_API int grhip_head_reset(grhip_copy_adapter *h);
GRHIP_API void grhip_copy_adapter_destroy(grhip_copy_adapter *h);
GRHIP_API int grhip_copy_adapter_work(grhip_copy_adapter *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_copy_adapter_work_device(grhip_copy_adapter *h, int noutput_items, const void *d_in, void *d_out,
                                             void *stream);

/* ======================================================================
 * digital_clock_recovery_mm_cc  (the complex sibling of the M&M timing loop)
 *   replaces digital_make_clock_recovery_mm_cc(float omega, float gain_omega, float mu,
 *                                              float gain_mu, float omega_relative_limit)
 *   gr-digital/include/digital_clock_recovery_mm_cc.h:44-110,
 *   gr-digital/lib/digital_clock_recovery_mm_cc.cc:37-215 (FUDGE = 16, history 3)
 * gr_block: general_work(noutput_items, ninput_items, in, out, err, &consumed) returns the items
 * produced and stores what consume_each() would get; `err` is the optional second output (the
 * clipped timing error, .cc:137-168) and may be NULL -- as in the reference its presence selects
 * the clip limit (4.0 with, 1.0 without).  GRHIP_ERANGE for omega <= 0 or negative gains (.cc:62-65).
 * Getters store into *v and return a status.
 * ====================================================================== */
typedef struct grhip_clock_recovery_mm_cc grhip_clock_recovery_mm_cc;
GRHIP_API int grhip_clock_recovery_mm_cc_create(grhip_clock_recovery_mm_cc **h, float omega, float gain_omega,
                                                float mu, float gain_mu, float omega_relative_limit, int device);
GRHIP_API void grhip_clock_recovery_mm_cc_destroy(grhip_clock_recovery_mm_cc *h);
GRHIP_API int grhip_clock_recovery_mm_cc_forecast(grhip_clock_recovery_mm_cc *h, int noutput_items);
GRHIP_API int grhip_clock_recovery_mm_cc_history(const grhip_clock_recovery_mm_cc *h);
GRHIP_API int grhip_clock_recovery_mm_cc_general_work(grhip_clock_recovery_mm_cc *h, int noutput_items,
                                                      int ninput_items, const void *in, void *out, float *err,
                                                      int *consumed);
GRHIP_API int grhip_clock_recovery_mm_cc_general_work_device(grhip_clock_recovery_mm_cc *h, int noutput_items,
                                                             int ninput_items, const void *d_in, void *d_out,
                                                             float *d_err, int *consumed, void *stream);
GRHIP_API int grhip_clock_recovery_mm_cc_mu(grhip_clock_recovery_mm_cc *h, float *v);
GRHIP_API int grhip_clock_recovery_mm_cc_omega(grhip_clock_recovery_mm_cc *h, float *v);
GRHIP_API int grhip_clock_recovery_mm_cc_gain_mu(grhip_clock_recovery_mm_cc *h, float *v);
GRHIP_API int grhip_clock_recovery_mm_cc_gain_omega(grhip_clock_recovery_mm_cc *h, float *v);
GRHIP_API int grhip_clock_recovery_mm_cc_set_mu(grhip_clock_recovery_mm_cc *h, float v);
GRHIP_API int grhip_clock_recovery_mm_cc_set_omega(grhip_clock_recovery_mm_cc *h, float v);
GRHIP_API int grhip_clock_recovery_mm_cc_set_gain_mu(grhip_clock_recovery_mm_cc *h, float v);
GRHIP_API int grhip_clock_recovery_mm_cc_set_gain_omega(grhip_clock_recovery_mm_cc *h, float v);

/* ======================================================================
 * gr_pfb_decimator_ccf  (polyphase decimator, one output channel)
 *   replaces gr_make_pfb_decimator_ccf(unsigned decim, const std::vector<float> &taps,
 *                                      unsigned channel)
 *   filter/gr_pfb_decimator_ccf.h:100-140, filter/gr_pfb_decimator_ccf.cc:43-68 (constructor),
 *   77-111 (set_taps: filter j gets taps[j + t*decim], history = taps per filter), 130-180 (work:
 *   `decim` input streams, stream s feeds filter decim-1-s, the filter outputs go through a
 *   decim-point backward FFT of which bin `channel` is the output item).
 * gr_sync_block: work() returns 0 once after set_taps (.cc:138-141).  ins[s] / the device
 * streams carry history()-1 old items in front; on the device stream s starts at
 * d_in + s * stream_stride_items complex items.
 * ====================================================================== */
typedef struct grhip_pfb_decimator_ccf grhip_pfb_decimator_ccf;
GRHIP_API int grhip_pfb_decimator_ccf_create(grhip_pfb_decimator_ccf **h, unsigned decim, const float *taps,
                                             size_t ntaps, unsigned channel, int device);
GRHIP_API void grhip_pfb_decimator_ccf_destroy(grhip_pfb_decimator_ccf *h);
GRHIP_API int grhip_pfb_decimator_ccf_set_taps(grhip_pfb_decimator_ccf *h, const float *taps, size_t ntaps);
GRHIP_API int grhip_pfb_decimator_ccf_history(const grhip_pfb_decimator_ccf *h);
GRHIP_API int grhip_pfb_decimator_ccf_work(grhip_pfb_decimator_ccf *h, int noutput_items, const void *const *ins,
                                           void *out);
GRHIP_API int grhip_pfb_decimator_ccf_work_device(grhip_pfb_decimator_ccf *h, int noutput_items, const void *d_in,
                                                  size_t stream_stride_items, void *d_out, void *stream);

/* ======================================================================
 * gr_pfb_arb_resampler_ccf / gr_pfb_arb_resampler_fff  (arbitrary-rate polyphase resampler)
 *   replaces gr_make_pfb_arb_resampler_ccf(float rate, const std::vector<float> &taps,
 *                                          unsigned int filter_size = 32)   (and _fff: float items)
 *   filter/gr_pfb_arb_resampler_ccf.h:166-170 (set_rate: D = floor(R/rate), f = R/rate - D in float),
 *   filter/gr_pfb_arb_resampler_ccf.cc:42-83 (constructor), 93-124 (create_taps: R = filter_size filters,
 *   tpf = ceil(ntaps/R), filter i gets taps[i + t*R], zero padded; history tpf + 1), 126-139 (create_diff_taps:
 *   a second bank from taps[i+1] - taps[i], the last difference repeated), 158-209 (general_work:
 *   out = filters[j].filter(&in[count]) + diff_filters[j].filter(&in[count]) * acc, then acc += f,
 *   j += D + floor(acc), acc = fmod(acc, 1), count += j / R when j passes R; outputs while count < ninput - tpf;
 *   state j, acc and the overshoot d_start_index carried between calls; consumes min(count, ninput)).
 * gr_block: history() = tpf + 1, forecast(n) = n + tpf (gr_block's default, runtime/gr_block.cc:51-56).  The first
 * general_work after create returns 0 and consumes nothing (d_updated, .cc:166-169); set_rate does not do that.
 * Refused with GRHIP_EINVAL (undefined in the reference; std::invalid_argument in host/grhip_blocks.h):
 *   - fewer than 2 taps (create_diff_taps underflows size()-1 for none, repeats an unset difference for one)
 *   - filter_size == 0 (.cc:100 divides by it)
 *   - rate <= 0 or not finite (set_relative_rate throws for negative rates, 0 gives floor(inf))
 * Limits of the kernel (GRHIP_EINVAL beyond them): filter_size * (tpf | 1) <= 4096 (both banks in LDS, rows of an
 * odd stride); filter_size / rate < 2^20.
 * Modes: GRHIP_MODE_GENERIC is bit-exact against the reference's generic build (gr_fir_XXX_generic.cc.t:59-78 for
 * both filters, the blend as a multiply and an add).  GRHIP_MODE_FAST, _FAST_VALU and _FAST_REFTAPS all mean the
 * same FMA kernel with one blended tap h + acc*dh (there is no matrix-core engine for this block); the schedule is
 * exact in every mode.  The default mode is grhip_get_default_mode() at create.
 * Positions: the reference carries `count` through a float (.cc:196), exact below 2^24 items per call; this
 * library keeps every position in exact integers (64-bit in run_captures_device), so calls of more than 2^24 items
 * are where the two can part.
 * The schedule: while the fractional rate f and the carried acc are multiples of 2^-23 it is a closed form the
 * kernel evaluates per output, and the device entries never wait.  That holds for every call at rate <= filter_size
 * from fresh state, and after set_rate between such rates.  Otherwise the float sums round: rate > filter_size, or
 * a call at rate > filter_size left acc off the grid, after which a later rate <= filter_size keeps it off.  Then
 * the host walks the reference's float32 arithmetic and uploads one entry per output.  Before that upload the
 * device entries wait for this handle's previous walked launch to finish (that launch only, not the device).
 * ====================================================================== */
typedef struct grhip_pfb_arb_resampler_ccf grhip_pfb_arb_resampler_ccf;
GRHIP_API int grhip_pfb_arb_resampler_ccf_create(grhip_pfb_arb_resampler_ccf **h, float rate, const float *taps,
                                                 size_t ntaps, unsigned filter_size, int device);
GRHIP_API void grhip_pfb_arb_resampler_ccf_destroy(grhip_pfb_arb_resampler_ccf *h);
/* .h:166-170; takes effect at the next general_work, acc and j carried */
GRHIP_API int grhip_pfb_arb_resampler_ccf_set_rate(grhip_pfb_arb_resampler_ccf *h, float rate);
GRHIP_API int grhip_pfb_arb_resampler_ccf_set_mode(grhip_pfb_arb_resampler_ccf *h, int mode);
GRHIP_API int grhip_pfb_arb_resampler_ccf_history(const grhip_pfb_arb_resampler_ccf *h);
GRHIP_API int grhip_pfb_arb_resampler_ccf_taps_per_filter(const grhip_pfb_arb_resampler_ccf *h);
GRHIP_API int grhip_pfb_arb_resampler_ccf_forecast(const grhip_pfb_arb_resampler_ccf *h, int noutput_items);
/* general_work (.cc:158-209) on HOST buffers: in[0 .. ninput_items) with the history in front, out room for
 * noutput_items; returns the items produced, *consumed the items to consume (consume_each, .cc:207) */
GRHIP_API int grhip_pfb_arb_resampler_ccf_general_work(grhip_pfb_arb_resampler_ccf *h, int noutput_items,
                                                       int ninput_items, const void *in, void *out, int *consumed);
/* the same on DEVICE buffers, enqueued on `stream`; produced and *consumed are known on return (the schedule
 * does not depend on the data), the outputs once the stream has run */
GRHIP_API int grhip_pfb_arb_resampler_ccf_general_work_device(grhip_pfb_arb_resampler_ccf *h, int noutput_items,
                                                              int ninput_items, const void *d_in, void *d_out,
                                                              int *consumed, void *stream);
/* n_streams captures in one launch, each from fresh state with the tpf history zeros a fresh flowgraph supplies
 * (NOT in d_in): capture s at d_in + s*in_stride_items (n_samples items), its outputs at d_out + s*out_stride_items.
 * *n_out receives the outputs per capture, the same for all: those with count_k < n_samples, exactly what the
 * block produces from the whole stream however it is split into calls.  d_out == NULL only sets *n_out.  The
 * handle's own state (j, acc, the first-call 0) is left alone. */
GRHIP_API int grhip_pfb_arb_resampler_ccf_run_captures_device(grhip_pfb_arb_resampler_ccf *h, int n_streams,
                                                              size_t n_samples, const void *d_in,
                                                              size_t in_stride_items, void *d_out,
                                                              size_t out_stride_items, size_t *n_out, void *stream);

typedef struct grhip_pfb_arb_resampler_fff grhip_pfb_arb_resampler_fff;
GRHIP_API int grhip_pfb_arb_resampler_fff_create(grhip_pfb_arb_resampler_fff **h, float rate, const float *taps,
                                                 size_t ntaps, unsigned filter_size, int device);
GRHIP_API void grhip_pfb_arb_resampler_fff_destroy(grhip_pfb_arb_resampler_fff *h);
GRHIP_API int grhip_pfb_arb_resampler_fff_set_rate(grhip_pfb_arb_resampler_fff *h, float rate);
GRHIP_API int grhip_pfb_arb_resampler_fff_set_mode(grhip_pfb_arb_resampler_fff *h, int mode);
GRHIP_API int grhip_pfb_arb_resampler_fff_history(const grhip_pfb_arb_resampler_fff *h);
GRHIP_API int grhip_pfb_arb_resampler_fff_taps_per_filter(const grhip_pfb_arb_resampler_fff *h);
GRHIP_API int grhip_pfb_arb_resampler_fff_forecast(const grhip_pfb_arb_resampler_fff *h, int noutput_items);
GRHIP_API int grhip_pfb_arb_resampler_fff_general_work(grhip_pfb_arb_resampler_fff *h, int noutput_items,
                                                       int ninput_items, const void *in, void *out, int *consumed);
GRHIP_API int grhip_pfb_arb_resampler_fff_general_work_device(grhip_pfb_arb_resampler_fff *h, int noutput_items,
                                                              int ninput_items, const void *d_in, void *d_out,
                                                              int *consumed, void *stream);
GRHIP_API int grhip_pfb_arb_resampler_fff_run_captures_device(grhip_pfb_arb_resampler_fff *h, int n_streams,
                                                              size_t n_samples, const void *d_in,
                                                              size_t in_stride_items, void *d_out,
                                                              size_t out_stride_items, size_t *n_out, void *stream);

/* ======================================================================
 * gr_fractional_interpolator_ff / gr_fractional_interpolator_cc  (MMSE fractional resampler)
 *   replaces gr_make_fractional_interpolator_ff(float phase_shift, float interp_ratio)   (and _cc: complex items)
 *   filter/gr_fractional_interpolator_ff.cc:38-50 (constructor), 57-65 (forecast), 67-93 (general_work:
 *   out[oo++] = interp->interpolate(&in[ii], mu); s = mu + mu_inc (a float sum); f = floor(s); mu = s - f;
 *   ii += f; consume_each(ii)), filter/gr_fractional_interpolator_ff.h:51-54 (mu, interp_ratio, set_mu,
 *   set_interp_ratio), filter/gri_mmse_fir_interpolator.cc:61-71 (imu = rint(mu * 128), filters[imu]: 8 taps
 *   through gr_fir_fff / gr_fir_ccf).  One output per interp_ratio input items.
 * gr_block: history() = 1 (the block never calls set_history), forecast(n) = (int) ceil(n * mu_inc + 8) evaluated
 * in float as the reference writes it.
 * GRHIP_ERANGE (std::out_of_range in the reference, .cc:44-47): interp_ratio <= 0, phase_shift < 0 or > 1 -- at
 * create, and for set_interp_ratio / set_mu as well, where the reference accepts the value and trips the
 * interpolator's assert on imu later -- and values that are not finite.  GRHIP_EINVAL: interp_ratio >= 2^20, the
 * limit of the kernel (positions inside a tile are 32-bit; on the host every position is a 64-bit integer).
 * Input shortfall: the reference trusts forecast and always produces noutput_items.  Here a call produces the
 * outputs k < noutput_items with ii_k + 8 <= ninput_items and consumes ii after the last one produced, at most
 * ninput_items; what a short call could not consume is carried and skipped at the start of the next.  With
 * forecast honoured that is the reference's result, and nothing but mu is carried.  So from fresh state the outputs
 * of a stream of N items are exactly those with ii_k + 8 <= N, however the stream is cut into calls; there are no
 * history zeros in front.
 * Modes: GRHIP_MODE_GENERIC is bit-exact against the reference's generic build (gr_fir_XXX_generic.cc.t:59-78).
 * GRHIP_MODE_FAST, _FAST_VALU and _FAST_REFTAPS all mean one FMA kernel (there is no matrix-core engine for 8
 * taps); the schedule is exact in every mode.  The default mode is grhip_get_default_mode() at create.
 * The schedule: the float sum mu + mu_inc is the one operation of the walk that rounds.  It is exact while mu and
 * mu_inc are multiples of a power of two g with 1 + mu_inc <= 2^24 * g (ratios such as 0.5, 0.75, 1.25, 2.5 or 10,
 * and 1.3f, 160/147.f or 4.8f, whose last bits happen to be zero, from a phase on the same grid); the walk is then a closed form the kernel evaluates per output, and the device
 * entries never wait.  mu == 1.0f at the start of a call (phase_shift = 1 or set_mu(1)) is such a case too: its
 * first output uses filter 128 at offset 0.  Otherwise (1.0001f, 147/160.f, 0.01f, a phase of 0.1f) the host walks
 * the reference's arithmetic and uploads one entry per output; before that upload the device entries wait for this
 * handle's previous walked launch to finish (that launch only, not the device).
 * ====================================================================== */
typedef struct grhip_fractional_interpolator_ff grhip_fractional_interpolator_ff;
GRHIP_API int grhip_fractional_interpolator_ff_create(grhip_fractional_interpolator_ff **h, float phase_shift,
                                                      float interp_ratio, int device);
GRHIP_API void grhip_fractional_interpolator_ff_destroy(grhip_fractional_interpolator_ff *h);
/* .h:51-54; the setters take effect at the next general_work */
GRHIP_API int grhip_fractional_interpolator_ff_set_mu(grhip_fractional_interpolator_ff *h, float mu);
GRHIP_API int grhip_fractional_interpolator_ff_set_interp_ratio(grhip_fractional_interpolator_ff *h,
                                                                float interp_ratio);
GRHIP_API float grhip_fractional_interpolator_ff_mu(grhip_fractional_interpolator_ff *h);
GRHIP_API float grhip_fractional_interpolator_ff_interp_ratio(grhip_fractional_interpolator_ff *h);
GRHIP_API int grhip_fractional_interpolator_ff_set_mode(grhip_fractional_interpolator_ff *h, int mode);
GRHIP_API int grhip_fractional_interpolator_ff_history(const grhip_fractional_interpolator_ff *h);
GRHIP_API int grhip_fractional_interpolator_ff_forecast(grhip_fractional_interpolator_ff *h, int noutput_items);
/* general_work (.cc:67-93) on HOST buffers: in[0 .. ninput_items), out room for noutput_items; returns the items
 * produced, *consumed the items to consume (consume_each, .cc:90) */
GRHIP_API int grhip_fractional_interpolator_ff_general_work(grhip_fractional_interpolator_ff *h, int noutput_items,
                                                            int ninput_items, const void *in, void *out,
                                                            int *consumed);
/* the same on DEVICE buffers, enqueued on `stream`; produced and *consumed are known on return (the schedule
 * does not depend on the data), the outputs once the stream has run */
GRHIP_API int grhip_fractional_interpolator_ff_general_work_device(grhip_fractional_interpolator_ff *h,
                                                                   int noutput_items, int ninput_items,
                                                                   const void *d_in, void *d_out, int *consumed,
                                                                   void *stream);
/* n_streams captures in one launch, each from fresh state (mu = the phase_shift given at create, the current
 * interp_ratio): capture s at d_in + s*in_stride_items (n_samples items), its outputs at d_out + s*out_stride_items.
 * *n_out receives the outputs per capture, the same for all: those with ii_k + 8 <= n_samples, exactly what the
 * block produces from the whole stream however it is split into calls.  d_out == NULL only sets *n_out.  The
 * handle's own mu is left alone. */
GRHIP_API int grhip_fractional_interpolator_ff_run_captures_device(grhip_fractional_interpolator_ff *h, int n_streams,
                                                                   size_t n_samples, const void *d_in,
                                                                   size_t in_stride_items, void *d_out,
                                                                   size_t out_stride_items, size_t *n_out,
                                                                   void *stream);

typedef struct grhip_fractional_interpolator_cc grhip_fractional_interpolator_cc;
GRHIP_API int grhip_fractional_interpolator_cc_create(grhip_fractional_interpolator_cc **h, float phase_shift,
                                                      float interp_ratio, int device);
GRHIP_API void grhip_fractional_interpolator_cc_destroy(grhip_fractional_interpolator_cc *h);
GRHIP_API int grhip_fractional_interpolator_cc_set_mu(grhip_fractional_interpolator_cc *h, float mu);
GRHIP_API int grhip_fractional_interpolator_cc_set_interp_ratio(grhip_fractional_interpolator_cc *h,
                                                                float interp_ratio);
GRHIP_API float grhip_fractional_interpolator_cc_mu(grhip_fractional_interpolator_cc *h);
GRHIP_API float grhip_fractional_interpolator_cc_interp_ratio(grhip_fractional_interpolator_cc *h);
GRHIP_API int grhip_fractional_interpolator_cc_set_mode(grhip_fractional_interpolator_cc *h, int mode);
GRHIP_API int grhip_fractional_interpolator_cc_history(const grhip_fractional_interpolator_cc *h);
GRHIP_API int grhip_fractional_interpolator_cc_forecast(grhip_fractional_interpolator_cc *h, int noutput_items);
GRHIP_API int grhip_fractional_interpolator_cc_general_work(grhip_fractional_interpolator_cc *h, int noutput_items,
                                                            int ninput_items, const void *in, void *out,
                                                            int *consumed);
GRHIP_API int grhip_fractional_interpolator_cc_general_work_device(grhip_fractional_interpolator_cc *h,
                                                                   int noutput_items, int ninput_items,
                                                                   const void *d_in, void *d_out, int *consumed,
                                                                   void *stream);
GRHIP_API int grhip_fractional_interpolator_cc_run_captures_device(grhip_fractional_interpolator_cc *h, int n_streams,
                                                                   size_t n_samples, const void *d_in,
                                                                   size_t in_stride_items, void *d_out,
                                                                   size_t out_stride_items, size_t *n_out,
                                                                   void *stream);

/* ======================================================================
 * gr_interp_fir_filter_{ccf,fff,ccc}  (interpolating FIR: I outputs per input item)
 *   replaces gr_make_interp_fir_filter_XXX(unsigned interpolation, const std::vector<TAP> &taps)
 *   filter/gr_interp_fir_filter_XXX.cc.t:72-109 (set_taps: zeros in FRONT of the taps up to a multiple of I;
 *   install_taps: nt = len/I, filter n gets taps[n + k*I], reversed by gr_fir_XXX::set_taps; set_history(nt)),
 *   112-145 (work: out[i*I + nf] = firs[nf]->filter(&in[i])); runtime/gr_sync_interpolator.h:48-53
 *   (output_multiple = I, forecast n/I + nt - 1, consumes n/I).
 * kind: "ccf" | "fff" | "ccc" as grhip_fir_filter_create (complex taps interleaved, ntaps counts taps).
 * history() = nt, so the input of work carries nt - 1 history items in front: in[0 .. n/I + nt - 1).
 * The constructor installs the taps; set_taps latches new ones, and the next work call installs them and returns 0
 * (nt, and with it history(), changes then).  That call waits for the handle's earlier launches (the bank is
 * rewritten); no other call waits for the device beyond the host-buffer entries' own copies.
 * Refused: interpolation == 0 -> GRHIP_ERANGE (std::out_of_range, as the reference); ntaps == 0 -> GRHIP_EINVAL
 * (filters of 0 taps are outside the reference's defined behaviour); noutput_items not a multiple of I ->
 * GRHIP_EINVAL (output_multiple); interpolation > 2^20 and shapes beyond the kernel's limits below -> GRHIP_EINVAL.
 * Modes: GRHIP_MODE_GENERIC is bit-exact against the reference's generic build (gr_fir_XXX_generic.cc.t:59-78:
 * 2 accumulators for ccf/ccc, 4 for fff, the tail into acc0, no contraction).  GRHIP_MODE_FAST, _FAST_VALU and
 * _FAST_REFTAPS all mean the same FMA kernel (there is no matrix-core engine for these blocks), within 1e-5 of the
 * output peak.  The default mode is grhip_get_default_mode() at create.
 * Kernel limits (both blocks; g = gcd(I, D)): a workgroup stages 64 periods of input in LDS, so
 * 63*D/g + nt + (a few items) must fit 160 KiB (about 20000 complex or 40000 float items).
 * ====================================================================== */
typedef struct grhip_interp_fir_filter grhip_interp_fir_filter;
GRHIP_API int grhip_interp_fir_filter_create(grhip_interp_fir_filter **h, const char *kind, unsigned interpolation,
                                             const float *taps, size_t ntaps, int device);
GRHIP_API void grhip_interp_fir_filter_destroy(grhip_interp_fir_filter *h);
GRHIP_API int grhip_interp_fir_filter_set_taps(grhip_interp_fir_filter *h, const float *taps, size_t ntaps);
GRHIP_API int grhip_interp_fir_filter_set_mode(grhip_interp_fir_filter *h, int mode);
GRHIP_API int grhip_interp_fir_filter_history(const grhip_interp_fir_filter *h);
GRHIP_API int grhip_interp_fir_filter_interpolation(const grhip_interp_fir_filter *h);
/* work on HOST buffers: in holds noutput_items/I + history() - 1 items; returns noutput_items (0 when it installs
 * latched taps) */
GRHIP_API int grhip_interp_fir_filter_work(grhip_interp_fir_filter *h, int noutput_items, const void *in, void *out);
/* the same on DEVICE buffers, enqueued on `stream` (NULL: the handle's own stream) */
GRHIP_API int grhip_interp_fir_filter_work_device(grhip_interp_fir_filter *h, int noutput_items, const void *d_in,
                                                  void *d_out, void *stream);
/* n_streams fresh captures in one launch: capture s at d_in + s*in_stride_items (n_samples items, the nt - 1 history
 * zeros implied, NOT in d_in), its I*n_samples outputs at d_out + s*out_stride_items.  *n_out receives I*n_samples;
 * d_out == NULL only sets it.  Uses the installed taps (a latched set_taps waits for the next work call); positions
 * are 64-bit, n_samples <= 2^40. */
GRHIP_API int grhip_interp_fir_filter_run_captures_device(grhip_interp_fir_filter *h, int n_streams, size_t n_samples,
                                                          const void *d_in, size_t in_stride_items, void *d_out,
                                                          size_t out_stride_items, size_t *n_out, void *stream);

/* ======================================================================
 * gr_rational_resampler_base_{ccf,fff,ccc}  (interpolate by I, decimate by D)
 *   replaces gr_make_rational_resampler_base_XXX(unsigned interpolation, unsigned decimation,
 *                                                 const std::vector<TAP> &taps)
 *   filter/gr_rational_resampler_base_XXX.cc.t:49-72 (constructor; relative_rate I/D), 83-120 (set_taps /
 *   install_taps: the bank of gr_interp_fir_filter_XXX), 135-141 (forecast), 144-172 (general_work: from ctr = d_ctr,
 *   out[i++] = firs[ctr]->filter(in); ctr += D; while (ctr >= I) { ctr -= I; in++; }; consume_each(in - in0)).
 * Closed form: output o of a call that starts at ctr = c0 uses filter (c0 + o*D) % I at in + (c0 + o*D) / I; a call of
 * n outputs consumes (c0 + n*D) / I items and leaves ctr = (c0 + n*D) % I.
 * history() returns the block's own nt.  The reference's class declares its own d_history / history() /
 * set_history() (.h.t:51,72-73), which hide gr_block's non-virtual ones: the SCHEDULER-VISIBLE history is 1, there
 * are no zeros in front of the stream, and the first output reads in[0 .. nt-1] of the raw stream.  nt appears only in
 * forecast(n) = max(1, (int)((double)(n+1)*D/I) + nt - 1).
 * The constructor installs the taps; set_taps latches, and the next general_work installs them and returns 0,
 * consuming nothing (waiting for the handle's earlier launches, as the interpolator).
 * Refused: interpolation or decimation == 0 -> GRHIP_ERANGE; ntaps == 0 -> GRHIP_EINVAL (outside the reference's
 * defined behaviour); ninput_items below what the call reads, (c0 + (n-1)*D)/I + nt, or below what it consumes,
 * (c0 + n*D)/I -> GRHIP_EINVAL (the reference would read or consume past its input); I or D > 2^20 and the kernel
 * limits of gr_interp_fir_filter -> GRHIP_EINVAL.  Modes as gr_interp_fir_filter.
 * ====================================================================== */
typedef struct grhip_rational_resampler_base grhip_rational_resampler_base;
GRHIP_API int grhip_rational_resampler_base_create(grhip_rational_resampler_base **h, const char *kind,
                                                   unsigned interpolation, unsigned decimation, const float *taps,
                                                   size_t ntaps, int device);
GRHIP_API void grhip_rational_resampler_base_destroy(grhip_rational_resampler_base *h);
GRHIP_API int grhip_rational_resampler_base_set_taps(grhip_rational_resampler_base *h, const float *taps, size_t ntaps);
GRHIP_API int grhip_rational_resampler_base_set_mode(grhip_rational_resampler_base *h, int mode);
GRHIP_API int grhip_rational_resampler_base_history(const grhip_rational_resampler_base *h);
GRHIP_API int grhip_rational_resampler_base_interpolation(const grhip_rational_resampler_base *h);
GRHIP_API int grhip_rational_resampler_base_decimation(const grhip_rational_resampler_base *h);
GRHIP_API int grhip_rational_resampler_base_forecast(const grhip_rational_resampler_base *h, int noutput_items);
/* general_work on HOST buffers: in[0 .. ninput_items), no history in front; returns the items produced (all
 * noutput_items, or 0 when it installs latched taps), *consumed the items to consume */
GRHIP_API int grhip_rational_resampler_base_general_work(grhip_rational_resampler_base *h, int noutput_items,
                                                         int ninput_items, const void *in, void *out, int *consumed);
/* the same on DEVICE buffers, enqueued on `stream`; produced and *consumed are known on return (the schedule does not
 * depend on the data) without a device sync, the outputs once the stream has run */
GRHIP_API int grhip_rational_resampler_base_general_work_device(grhip_rational_resampler_base *h, int noutput_items,
                                                                int ninput_items, const void *d_in, void *d_out,
                                                                int *consumed, void *stream);
/* n_streams fresh captures (ctr = 0, no zeros in front) in one launch: capture s at d_in + s*in_stride_items
 * (n_samples items), its outputs at d_out + s*out_stride_items.  *n_out receives the outputs per capture: every o
 * whose window fits, (o*D)/I + nt <= n_samples.  A real scheduler may stop a few outputs earlier, because forecast asks
 * for one output more than it produces.  d_out == NULL only sets *n_out.  The handle's ctr is left alone; the installed
 * taps are used.  Positions are 64-bit, n_samples <= 2^40. */
GRHIP_API int grhip_rational_resampler_base_run_captures_device(grhip_rational_resampler_base *h, int n_streams,
                                                                size_t n_samples, const void *d_in,
                                                                size_t in_stride_items, void *d_out,
                                                                size_t out_stride_items, size_t *n_out, void *stream);

/* ======================================================================
 * gr_pfb_interpolator_ccf  (polyphase interpolator: R outputs per input item)
 *   replaces gr_make_pfb_interpolator_ccf(unsigned interp, const std::vector<float> &taps)
 *   filter/gr_pfb_interpolator_ccf.cc:40-60 (constructor: a gr_sync_interpolator by interp), 69-104 (set_taps:
 *   tpf = ceil(ntaps/interp), zeros at the END of the taps -- gr_interp_fir_filter pads in front --, filter j gets
 *   padded[j + k*interp] through gr_fir_ccf; set_history(tpf)), 122-148 (work: out[n*interp + j] =
 *   filters[j]->filter(&in[n])).
 * The schedule, the kernel, the tap-update convention, the modes and the kernel limits are gr_interp_fir_filter's
 * (GRHIP_MODE_GENERIC: bit-exact against gr_fir_ccf_generic per branch); only the bank differs.
 * Refused: interp == 0 -> GRHIP_ERANGE; ntaps == 0, noutput_items not a multiple of interp -> GRHIP_EINVAL.
 * ====================================================================== */
typedef struct grhip_pfb_interpolator_ccf grhip_pfb_interpolator_ccf;
GRHIP_API int grhip_pfb_interpolator_ccf_create(grhip_pfb_interpolator_ccf **h, unsigned interp, const float *taps,
                                                size_t ntaps, int device);
GRHIP_API void grhip_pfb_interpolator_ccf_destroy(grhip_pfb_interpolator_ccf *h);
GRHIP_API int grhip_pfb_interpolator_ccf_set_taps(grhip_pfb_interpolator_ccf *h, const float *taps, size_t ntaps);
GRHIP_API int grhip_pfb_interpolator_ccf_set_mode(grhip_pfb_interpolator_ccf *h, int mode);
GRHIP_API int grhip_pfb_interpolator_ccf_history(const grhip_pfb_interpolator_ccf *h);         /* tpf (.cc:101) */
GRHIP_API int grhip_pfb_interpolator_ccf_interpolation(const grhip_pfb_interpolator_ccf *h);
/* work on HOST buffers (.cc:122-148): in holds noutput_items/interp + history() - 1 items; returns noutput_items (0
 * when it installs latched taps) */
GRHIP_API int grhip_pfb_interpolator_ccf_work(grhip_pfb_interpolator_ccf *h, int noutput_items, const void *in,
                                              void *out);
/* the same on DEVICE buffers, enqueued on `stream` (NULL: the handle's own stream) */
GRHIP_API int grhip_pfb_interpolator_ccf_work_device(grhip_pfb_interpolator_ccf *h, int noutput_items, const void *d_in,
                                                     void *d_out, void *stream);

/* ======================================================================
 * gr_pfb_synthesis_filterbank_ccf  (polyphase synthesis: 1..numchans streams in, one stream at numchans times the rate)
 *   replaces gr_make_pfb_synthesis_filterbank_ccf(unsigned numchans, const std::vector<float> &taps)
 *   filter/gr_pfb_synthesis_filterbank_ccf.cc:41-62 (constructor: a gr_sync_interpolator by numchans = M, 1..M inputs;
 *   gri_fft_complex(M, true): a FORWARD unnormalised DFT), 71-106 (set_taps: tpf = ceil(ntaps/M), zeros at the END,
 *   branch f gets h_f[q] = padded[f + q*M]; set_history(tpf + 1)), 122-169 (work);
 *   gri_fir_filter_with_buffer_XXX.cc.t:41-78 (the branches: delay lines that start at zero and live across calls).
 * Output vector n of a call (numsigs connected streams, ndiff = M - numsigs, nhalf = ceil(numsigs/2)):
 *   bin i < nhalf is ins[i][n + i], bins nhalf <= i < nhalf + ndiff are zero, bin i >= nhalf + ndiff is
 *   ins[i - ndiff][n + i] (.cc:139-156; the offset + i is the reference's `(in+i)[n]`);
 *   V = forward DFT of the bins; branch f is fed V[M-1-f] and writes out[n*M + f] = sum_q h_f[q] u_f[n-q] (.cc:161-163).
 * Tap updates as gr_interp_fir_filter: create installs the taps; set_taps latches new ones; the next work call installs
 * them, clears the delay lines (waiting for the launches that still read them) and returns 0; history() and taps_per_filter() report the installed taps.
 * Modes: GRHIP_MODE_GENERIC sums every branch in the reference's order (one accumulator, oldest sample first, a product
 * and a sum per term) over the library's float32 DFT; the FAST modes are one FMA kernel.  The DFT is not the reference's
 * FFTW bit for bit; with a single connected stream, or M = 1, 2, 4, it is exact and GENERIC equals the reference.
 * Refused with GRHIP_EINVAL: numchans == 0 or > 256 (the kernels' limit); ntaps == 0; more than 65536 taps per filter;
 * numsigs outside 1..M; noutput_items not a multiple of M; and numsigs >= 2 with M - 1 > tpf: bin M-1 reads item
 * n + M - 1 of its stream while the scheduler only provides items up to n + tpf, so the reference reads past its input
 * there (undefined).  numsigs == 1 fills only bin 0 and is always in range.
 * ====================================================================== */
typedef struct grhip_pfb_synthesis_filterbank_ccf grhip_pfb_synthesis_filterbank_ccf;
GRHIP_API int grhip_pfb_synthesis_filterbank_ccf_create(grhip_pfb_synthesis_filterbank_ccf **h, unsigned numchans,
                                                        const float *taps, size_t ntaps, int device);
GRHIP_API void grhip_pfb_synthesis_filterbank_ccf_destroy(grhip_pfb_synthesis_filterbank_ccf *h);
GRHIP_API int grhip_pfb_synthesis_filterbank_ccf_set_taps(grhip_pfb_synthesis_filterbank_ccf *h, const float *taps,
                                                          size_t ntaps);
GRHIP_API int grhip_pfb_synthesis_filterbank_ccf_set_mode(grhip_pfb_synthesis_filterbank_ccf *h, int mode);
GRHIP_API int grhip_pfb_synthesis_filterbank_ccf_history(const grhip_pfb_synthesis_filterbank_ccf *h);   /* tpf + 1 (.cc:103) */
GRHIP_API int grhip_pfb_synthesis_filterbank_ccf_taps_per_filter(const grhip_pfb_synthesis_filterbank_ccf *h);
GRHIP_API int grhip_pfb_synthesis_filterbank_ccf_numchans(const grhip_pfb_synthesis_filterbank_ccf *h);
/* work on HOST buffers (.cc:122-169): ins[0 .. numsigs) each hold noutput_items/M + tpf items (history() - 1 old ones
 * in front); out receives noutput_items items.  Returns noutput_items (0 when it installs latched taps). */
GRHIP_API int grhip_pfb_synthesis_filterbank_ccf_work(grhip_pfb_synthesis_filterbank_ccf *h, int noutput_items,
                                                      const void *const *ins, int numsigs, void *out);
/* the same on DEVICE buffers: stream s at d_in + s*stream_stride_items (complex items), as the channeliser's device
 * entry; d_out 16-byte aligned for full-width stores.  Enqueued on `stream` (NULL: the handle's own stream).  On the
 * fused kernel's shapes (numchans 2..16, at most 513 taps per filter) the call never waits for the device.  The other
 * shapes keep a scratch buffer of (noutput_items/numchans + tpf - 1) * numchans complex items in device memory; a call
 * larger than every earlier one grows it, and that reallocation waits for the device.  Calls that continue a stream
 * must be enqueued in order (the delay lines are carried in device memory). */
GRHIP_API int grhip_pfb_synthesis_filterbank_ccf_work_device(grhip_pfb_synthesis_filterbank_ccf *h, int noutput_items,
                                                             const void *d_in, size_t stream_stride_items, int numsigs,
                                                             void *d_out, void *stream);

/* ======================================================================
 * gr_framer_sink_1  (the consumer of the correlator's flag bit)
 *   replaces gr_make_framer_sink_1(gr_msg_queue_sptr target_queue)
 *   general/gr_framer_sink_1.h:62-98, general/gr_framer_sink_1.cc:34-66 (states), 90-190 (work):
 *   items carry the data bit in bit 0 and "first bit after the access code" in bit 1; the flagged
 *   item starts a 32-bit header (two equal 16-bit words: 4 bits whitener offset, 12 bits payload
 *   length), followed by 8 * length payload bits, most significant bit of each byte first.  Flags
 *   inside a header or payload are ignored; a header whose halves differ returns to the search.
 * The reference inserts gr_message(type 0, arg1 = whitener offset, arg2 = 0, length) into its queue
 * from inside work(); here work()/work_device() collect the messages on the device and the caller
 * moves them into its queue with message_count() + pop():
 *   message_count  waits for the queued work on `stream`, brings every complete message to the host
 *                  and returns how many are waiting to be popped;
 *   pop            next message in order: returns the payload length (0..4095), stores arg1 in
 *                  *whitener_offset and the payload in `payload` (capacity >= 4096 always fits).
 * work() returns noutput_items (a sink consumes everything, .cc:189).  State (partial header,
 * partial payload) carries across calls exactly as in the reference.
 * ====================================================================== */
typedef struct grhip_framer_sink_1 grhip_framer_sink_1;
GRHIP_API int grhip_framer_sink_1_create(grhip_framer_sink_1 **h, int device);
GRHIP_API void grhip_framer_sink_1_destroy(grhip_framer_sink_1 *h);
/* tuning: items per segment of the segment-parallel walk of long calls (0 = chosen per call, about sqrt(160 n);
 * results do not depend on it -- the tests use 64 to force the walk's divergence branch) */
GRHIP_API int grhip_framer_sink_1_set_segment_items(grhip_framer_sink_1 *h, long long items);
GRHIP_API int grhip_framer_sink_1_work(grhip_framer_sink_1 *h, int noutput_items, const unsigned char *in);
GRHIP_API int grhip_framer_sink_1_work_device(grhip_framer_sink_1 *h, int noutput_items, const unsigned char *d_in,
                                              void *stream);
GRHIP_API int grhip_framer_sink_1_message_count(grhip_framer_sink_1 *h, void *stream);
GRHIP_API int grhip_framer_sink_1_pop(grhip_framer_sink_1 *h, int *whitener_offset, unsigned char *payload,
                                      int capacity);
/* several messages at once (after message_count): offsets, lengths and the payloads back to back;
 * stops before a message whose payload would not fit; returns how many were popped */
GRHIP_API int grhip_framer_sink_1_drain(grhip_framer_sink_1 *h, int max_msgs, int *whitener_offsets, int *lengths,
                                        unsigned char *payload, size_t payload_capacity);

/* Multi-capture entry of gr_framer_sink_1 (same reference, general/gr_framer_sink_1.cc:90-190): n_streams
 * independent item streams framed by one call, one wavefront per stream, every stream from the search
 * state (a capture is framed whole, as the chain processes it; a packet cut off by the end of the
 * capture is dropped, as the reference drops it when the flowgraph ends).  Stream s is at
 * d_in + s * stream_stride_items and holds min(n_items_max, d_nitems[s * nitems_stride]) items (d_nitems,
 * a device array, may be NULL: n_items_max each) -- e.g. the d_bits / d_nbits of grhip_dmr_chain.
 *   run_device  enqueues on `stream`, no synchronisation;
 *   fetch       waits for it, brings every stream's messages to the host, returns their total number;
 *   count/get   messages of one stream, in order: get returns the payload length (0..4095), stores arg1. */
typedef struct grhip_framer_sink_1_batch grhip_framer_sink_1_batch;
GRHIP_API int grhip_framer_sink_1_batch_create(grhip_framer_sink_1_batch **h, int n_streams, size_t max_items_per_stream,
                                               int device);
GRHIP_API void grhip_framer_sink_1_batch_destroy(grhip_framer_sink_1_batch *h);
GRHIP_API int grhip_framer_sink_1_batch_run_device(grhip_framer_sink_1_batch *h, const unsigned char *d_in,
                                                   size_t stream_stride_items, const int *d_nitems, int nitems_stride,
                                                   size_t n_items_max, void *stream);
GRHIP_API int grhip_framer_sink_1_batch_fetch(grhip_framer_sink_1_batch *h, void *stream);
GRHIP_API int grhip_framer_sink_1_batch_count(grhip_framer_sink_1_batch *h, int stream_index);
GRHIP_API int grhip_framer_sink_1_batch_get(grhip_framer_sink_1_batch *h, int stream_index, int msg_index,
                                            int *whitener_offset, unsigned char *payload, int capacity);

/* ======================================================================
 * gr_stream_to_streams / gr_streams_to_stream  (the adapters either side of the
 * channeliser)
 *   replace gr_make_stream_to_streams(size_t item_size, size_t nstreams) and
 *           gr_make_streams_to_stream(size_t item_size, size_t nstreams)
 *   general/gr_stream_to_streams.cc:32-66 (gr_sync_decimator by nstreams),
 *   general/gr_streams_to_stream.cc:32-69 (gr_sync_interpolator by nstreams)
 * `split` selects the direction at creation.  work(): `streams` is the array of nstreams
 * host pointers the scheduler hands over; work_device(): stream j lives at
 * d_streams + j * stream_stride_items items (the convention of the PFB's inputs).
 * n_items_per_stream = noutput_items for stream_to_streams, noutput_items / nstreams for
 * streams_to_stream (which must divide, .cc:56).
 * ====================================================================== */
typedef struct grhip_stream_adapter grhip_stream_adapter;
GRHIP_API int grhip_stream_adapter_create(grhip_stream_adapter **h, int split, size_t item_size, size_t nstreams,
                                          int device);
GRHIP_API void grhip_stream_adapter_destroy(grhip_stream_adapter *h);
GRHIP_API int grhip_stream_adapter_work(grhip_stream_adapter *h, int n_items_per_stream, void *single,
                                        void *const *streams);
GRHIP_API int grhip_stream_adapter_work_device(grhip_stream_adapter *h, int n_items_per_stream, void *d_single,
                                               void *d_streams, size_t stream_stride_items, void *stream);

/* ======================================================================
 * digital_correlate_access_code_bb
 *   replaces digital_make_correlate_access_code_bb(const std::string&
 *       access_code, int threshold)
 *   gr-digital/include/digital_correlate_access_code_bb.h,
 *   gr-digital/lib/digital_correlate_access_code_bb.cc:37-133
 * access_code: string of '0'/'1' characters (only the LSB of each byte is
 * used, .cc:80); GRHIP_ERANGE if longer than 64 (.cc:54-57).
 * ====================================================================== */
typedef struct grhip_correlate_access_code_bb grhip_correlate_access_code_bb;
GRHIP_API int grhip_correlate_access_code_bb_create(grhip_correlate_access_code_bb **h,
                                                    const char *access_code, size_t len,
                                                    int threshold, int device);
GRHIP_API void grhip_correlate_access_code_bb_destroy(grhip_correlate_access_code_bb *h);
GRHIP_API int grhip_correlate_access_code_bb_set_access_code(grhip_correlate_access_code_bb *h,
                                                             const char *access_code, size_t len);
GRHIP_API int grhip_correlate_access_code_bb_work(grhip_correlate_access_code_bb *h, int noutput_items,
                                                  const unsigned char *in, unsigned char *out);
GRHIP_API int grhip_correlate_access_code_bb_work_device(grhip_correlate_access_code_bb *h,
                                                         int noutput_items, const unsigned char *d_in,
                                                         unsigned char *d_out, void *stream);

/* ======================================================================
 * gr_fft_vcc
 *   replaces gr_make_fft_vcc(int fft_size, bool forward,
 *       const std::vector<float>& window, bool shift)
 *   general/gr_fft_vcc.h:41-59, general/gr_fft_vcc.cc:34-64,
 *   general/gr_fft_vcc_fftw.cc:39-103 (FFTW3f c2c, unnormalised)
 * items are vectors of fft_size complex.  window: NULL/0 or fft_size floats.
 * GRHIP_ERANGE if fft_size <= 0 (general/gri_fft.cc:104-105).  Every other size the
 * reference hands to FFTW is taken (general/gri_fft.cc:97-123): powers of two up to 8192
 * by the radix-16 register kernels, larger ones (up to 2^26) in four-step form, sizes that
 * are not a power of two by a direct DFT (<= 128) or Bluestein's chirp convolution (up to
 * 2^25); beyond that GRHIP_EINVAL (a handle's work buffers are sized for 2^26 points).
 * Parity against a float64 DFT (1e-6 log2 N of the spectrum's peak) is pinned by the test
 * suite for powers of two up to 2^26 and for Bluestein up to a convolution length of
 * L = 2^23 (fft_size 3 000 001; L is the power of two >= 2 fft_size - 1).  Larger Bluestein
 * sizes (fft_size above 2^22 that is not a power of two, L = 2^24 ... 2^26) are accepted and
 * run the same code, but their parity is unpinned: the set-up alone needs up to 1 GB of host
 * doubles and many seconds, too much for a per-commit test.
 * ====================================================================== */
typedef struct grhip_fft_vcc grhip_fft_vcc;
GRHIP_API int grhip_fft_vcc_create(grhip_fft_vcc **h, int fft_size, int forward, const float *window,
                                   size_t window_len, int shift, int device);
GRHIP_API void grhip_fft_vcc_destroy(grhip_fft_vcc *h);
/* returns 1 if accepted, 0 if the length is wrong (gr_fft_vcc::set_window) */
GRHIP_API int grhip_fft_vcc_set_window(grhip_fft_vcc *h, const float *window, size_t window_len);
GRHIP_API int grhip_fft_vcc_work(grhip_fft_vcc *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_fft_vcc_work_device(grhip_fft_vcc *h, int noutput_items, const void *d_in,
                                        void *d_out, void *stream);

/* ======================================================================
 * gr_fft_filter_ccc  
 *   replaces gr_make_fft_filter_ccc(int decimation, const std::vector<gr_complex>& taps)
 *   filter/gr_fft_filter_ccc.cc:46-128, filter/gri_fft_filter_ccc_generic.cc:63-170
 * Overlap-add fast convolution with the reference's sizes (fftsize = 2*2^ceil(log2 ntaps),
 * nsamples = fftsize - ntaps + 1 = the block's output multiple), taps pre-scaled by
 * 1/fftsize, tail carried between blocks and calls.  gr_sync_decimator, history 1.
 * noutput_items must be a multiple of nsamples (the reference asserts it, .cc:121).
 * set_taps takes effect at the next work call, which returns 0 (.cc:113-118) and clears
 * the tail (generic.cc:69-71).  Any tap count up to 2^25 (fftsize <= 2^26; beyond 4096 taps the
 * transforms run in four-step form).
 * ====================================================================== */
typedef struct grhip_fft_filter_ccc grhip_fft_filter_ccc;
GRHIP_API int grhip_fft_filter_ccc_create(grhip_fft_filter_ccc **h, int decimation, const float *taps,
                                          size_t ntaps, int device);
GRHIP_API void grhip_fft_filter_ccc_destroy(grhip_fft_filter_ccc *h);
GRHIP_API int grhip_fft_filter_ccc_set_taps(grhip_fft_filter_ccc *h, const float *taps, size_t ntaps);
GRHIP_API int grhip_fft_filter_ccc_nsamples(const grhip_fft_filter_ccc *h);   /* output multiple */
GRHIP_API int grhip_fft_filter_ccc_decimation(const grhip_fft_filter_ccc *h);
GRHIP_API int grhip_fft_filter_ccc_work(grhip_fft_filter_ccc *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_fft_filter_ccc_work_device(grhip_fft_filter_ccc *h, int noutput_items, const void *d_in,
                                               void *d_out, void *stream);

/* ======================================================================
 * gr_fft_filter_fff  
 *   replaces gr_make_fft_filter_fff(int decimation, const std::vector<float>& taps)
 *   filter/gr_fft_filter_fff.cc:44-97, filter/gri_fft_filter_fff_generic.cc:34-158
 * The real-signal sibling of gr_fft_filter_ccc: float items in and out, float taps; the same
 * sizes (fftsize = 2*2^ceil(log2 ntaps), nsamples = fftsize - ntaps + 1 = the output multiple),
 * taps pre-scaled by 1/fftsize, tail carried between blocks and calls.  gr_sync_decimator,
 * history 1.  noutput_items must be a multiple of nsamples (the reference asserts it, .cc:90;
 * GRHIP_EINVAL here).  set_taps takes effect at the next work call, which returns 0 (.cc:83-88)
 * and clears the carried state (generic.cc:56-58).  Any tap count up to 2^25.  No bit-exact
 * mode: the reference's transforms are FFTW, unpinned.
 * Two consecutive blocks share one complex transform (one in the real plane, the next in the
 * imaginary plane; the transformed taps of a real filter are Hermitian, so the planes come out
 * apart with no untangling step).  Caveat: a non-finite sample (Inf, NaN) in one engine block
 * therefore reaches the outputs of the block it is paired with, the EARLIER one included; the
 * reference confines such a sample to its own block and the next.  For finite input the leakage
 * between paired blocks is rounding error of the transform, bounded by the parity tolerance
 * 2e-6 * log2(2 * nsamples) of the call's peak.
 * ====================================================================== */
typedef struct grhip_fft_filter_fff grhip_fft_filter_fff;
GRHIP_API int grhip_fft_filter_fff_create(grhip_fft_filter_fff **h, int decimation, const float *taps,
                                          size_t ntaps, int device);
GRHIP_API void grhip_fft_filter_fff_destroy(grhip_fft_filter_fff *h);
GRHIP_API int grhip_fft_filter_fff_set_taps(grhip_fft_filter_fff *h, const float *taps, size_t ntaps);
GRHIP_API int grhip_fft_filter_fff_nsamples(const grhip_fft_filter_fff *h);   /* output multiple */
GRHIP_API int grhip_fft_filter_fff_decimation(const grhip_fft_filter_fff *h);
GRHIP_API int grhip_fft_filter_fff_work(grhip_fft_filter_fff *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_fft_filter_fff_work_device(grhip_fft_filter_fff *h, int noutput_items, const void *d_in,
                                               void *d_out, void *stream);

/* ======================================================================
 * gr_fft_vfc
 *   replaces gr_make_fft_vfc(int fft_size, bool forward, const std::vector<float>& window)
 *   general/gr_fft_vfc.cc:42-118
 * items are vectors of fft_size floats in, fft_size complex out (the full spectrum).  Forward
 * only: forward == 0 is GRHIP_EINVAL (.cc:54-57).  No shift.  window: NULL/0 or fft_size floats.
 * GRHIP_ERANGE if fft_size <= 0 (general/gri_fft.cc:104-105); the same sizes as gr_fft_vcc.
 * The result equals gr_fft_vcc (shift off) on the widened input value for value: powers of two
 * up to 8192 read the floats directly in the register kernels (12 B of memory traffic per
 * sample), the other sizes widen into the output buffer first and transform it in place.
 * ====================================================================== */
typedef struct grhip_fft_vfc grhip_fft_vfc;
GRHIP_API int grhip_fft_vfc_create(grhip_fft_vfc **h, int fft_size, int forward, const float *window,
                                   size_t window_len, int device);
GRHIP_API void grhip_fft_vfc_destroy(grhip_fft_vfc *h);
/* returns 1 if accepted, 0 if the length is wrong (gr_fft_vfc::set_window); the old window stays */
GRHIP_API int grhip_fft_vfc_set_window(grhip_fft_vfc *h, const float *window, size_t window_len);
GRHIP_API int grhip_fft_vfc_work(grhip_fft_vfc *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_fft_vfc_work_device(grhip_fft_vfc *h, int noutput_items, const void *d_in,
                                        void *d_out, void *stream);

/* ======================================================================
 * gr_firdes::hilbert  -- host only, no device needed
 *   replaces gr_firdes::hilbert(unsigned ntaps, win_type windowtype, double beta)
 *   general/gr_firdes.cc:538-565 with gr_firdes::window, :720-780
 * out receives ntaps floats.  window_type is gr_firdes::win_type (0 Hamming, 1 Hann, 2 Blackman,
 * 3 rectangular, 4 Kaiser, 5 Blackman-harris).  Reproduced literally: window()'s WIN_RECTANGULAR
 * case has no break and runs on into WIN_HAMMING, so type 3 gives the taps of type 0; the taps
 * are formed in float (1/(float)i, the alternating recurrence gain = taps[h+i] - gain, a float
 * division by 2*fabs(gain)).  GRHIP_ERANGE for an even ntaps or a window type out of range (the
 * reference throws std::out_of_range).
 * ====================================================================== */
GRHIP_API int grhip_firdes_hilbert(unsigned ntaps, int window_type, double beta, float *out);

/* gr_firdes::low_pass  -- host only, no device needed
 *   replaces gr_firdes::low_pass(double gain, double sampling_freq, double cutoff_freq,
 *       double transition_width, win_type window, double beta)
 *   general/gr_firdes.cc:104-148 with compute_ntaps, :680-695, and gr_firdes::window as above
 * *ntaps receives the tap count, (int)(width_factor[window] / (transition / fs) + 0.5) made odd, and
 * out, of `cap` floats, the taps; with cap too small (out may then be null) only *ntaps is written
 * and the call returns GRHIP_ERANGE, so a first call with cap = 0 asks for the size.  The arithmetic
 * is the reference's: the ideal response and the window product in double, narrowed to float per
 * tap, the sum for the gain in double over those floats, the scaling a double product narrowed again.
 * GRHIP_EINVAL where the reference throws (fs <= 0, cutoff <= 0 or > fs / 2, transition <= 0), and,
 * a deviation, for an argument that is not finite, a window type outside 0 .. 4 (the reference
 * reads past its width_factor table for type 5) and a tap count above 2^24. */
GRHIP_API int grhip_firdes_low_pass(double gain, double fs, double cutoff, double transition, int window_type, double beta,
                                    float *out, size_t cap, size_t *ntaps);

/* gr_firdes::root_raised_cosine  -- host only, no device needed
 *   replaces gr_firdes::root_raised_cosine(double gain, double sampling_freq, double symbol_rate,
 *       double alpha, int ntaps)
 *   general/gr_firdes.cc:601-650
 * The reference's statements one for one: ntaps |= 1, both branches of |x3| >= 1e-6, the tap of -1
 * for alpha == 1 on the singular branch (it stays out of the scale), every tap narrowed to float
 * before it is added to the double scale, then taps[i] * gain / scale.  The taps are the reference's
 * bit for bit (tests/test_fll_band_edge_cpu.py).  *ntaps receives ntaps | 1 and out, of `cap` floats,
 * the taps; the size query is grhip_firdes_low_pass's (cap too small: only *ntaps, GRHIP_ERANGE).
 * Deviations: GRHIP_EINVAL for an argument that is not finite, ntaps < 1 (the reference then throws
 * from std::vector or writes nothing) and ntaps from 2^24 on.  A symbol_rate of 0 gives taps that are
 * not finite, as in the reference. */
GRHIP_API int grhip_firdes_root_raised_cosine(double gain, double fs, double symbol_rate, double alpha, int ntaps, float *out,
                                              size_t cap, size_t *ntaps_out);

/* gr_remez  -- host only, no device needed
 *   replaces gr_remez(int order, const std::vector<double> &bands, const std::vector<double> &ampl,
 *       const std::vector<double> &error_weight, const std::string filter_type, int grid_density)
 *   general/gr_remez.cc:98-867 (CreateDenseGrid, InitialGuess, CalcParms, ComputeA, CalcError, Search,
 *   FreqSample, isDone, remez and the argument checks of gr_remez())
 * The Parks-McClellan exchange in double, restated statement for statement: the same operation
 * order, the same Pi literal, GRIDDENSITY 16, MAXITERATIONS 40.  The taps of a design are the
 * reference's bit for bit (tests/test_optfir_cpu.py).  bands holds nbands2 edges on [0, 1] (1 is
 * Nyquist), ampl one response per edge (nbands2 of them), weight one per band or none (nweight ==
 * 0: all 1).  filter_type: 1 bandpass, 2 differentiator, 3 hilbert.  grid_density: 16 is the
 * reference's default.  *ntaps receives order + 1 and out, of `cap` doubles, the taps; with cap too
 * small (out may then be null) only *ntaps is written and the call returns GRHIP_ERANGE, as
 * grhip_firdes_low_pass.  The arguments are checked before the size is answered.
 * GRHIP_EINVAL where the reference throws on an argument: order < 3 (fewer than 4 taps), an odd
 * number of band edges or none, decreasing edges, edges outside [0, 1], nweight neither 0 nor
 * nbands2 / 2, grid_density < 16, an unknown filter_type.
 * GRHIP_ERUNTIME where the exchange fails; grhip_last_error() is the reference's message:
 * "gr_remez: failed to converge", "gr_remez: insufficient extremals -- cannot continue" or
 * "gr_remez: too many extremals -- cannot continue".
 * Stated deviations: an argument that is not finite, more than 64 bands, a grid_density above 1024
 * and bands so narrow that the dense grid has fewer than two points are GRHIP_EINVAL; more than 4096
 * taps are GRHIP_ERANGE (the reference computes i * (gridsize - 1) / r in int, which overflows from
 * about 23 000 taps, and then reads outside its grid).  Every array is sized by what is written into
 * it and no path reads or writes outside one: the reference writes one point past its grid for a
 * hilbert transformer or differentiator whose first edge lies above the first grid step, and
 * Grid[-1] for an empty first band; here those designs run on arrays that hold the point, with the
 * arithmetic otherwise unchanged.  Nothing is leaked on the error paths (the reference leaks its
 * work arrays there). */
GRHIP_API int grhip_remez(int order, const double *bands, size_t nbands2, const double *ampl, const double *weight,
                          size_t nweight, int filter_type, int grid_density, double *out, size_t cap, size_t *ntaps);

/* optfir.low_pass / high_pass / band_pass / band_reject  -- host only, no device needed
 *   replaces gnuradio/optfir.py:45-78, :116-156 with remezord, lporder, stopband_atten_to_dev and
 *   passband_ripple_to_dev, :160-310
 * Every argument a double, the taps in double as gr.remez returns them, the size query as above.
 * Kept literally: the order int(ceil(l)) - 1 + nextra_taps (the reference's default for nextra_taps
 * is 2); one more where high_pass or band_reject would get an even number of taps; high_pass
 * ignoring its gain (desired_ampls = (0, 1)); the relative deviations devs[i] / mags[i]; the weights
 * max_dev / devs[i]; max(l, l1, l2) over the two transitions of a three-band design.  The band edges
 * are in the reference's order: (freq1, freq2), band_pass (sb1, pb1, pb2, sb2), band_reject (pb1,
 * sb1, sb2, pb2).
 * Stated deviations: -atten_db / 20 is a true division (Python 2 floors it for two integers; the
 * two agree for every caller in the reference, 60 and 0.1); arguments that are not finite, fs == 0
 * and an order estimate that is not finite are GRHIP_EINVAL; the limits of grhip_remez hold.
 * complex_band_pass and bporder (unused in the reference) are not built.
 * grhip_optfir_spec returns what the designer `kind` (0 low_pass, 1 high_pass, 2 band_pass, 3
 * band_reject; freqs: its 2 or 4 band edges) hands to gr.remez: the order, 2 * *nbands band edges
 * and amplitudes (room for 6 each) and *nbands weights (room for 3). */
GRHIP_API int grhip_optfir_low_pass(double gain, double fs, double freq1, double freq2, double passband_ripple_db,
                                    double stopband_atten_db, int nextra_taps, double *out, size_t cap, size_t *ntaps);
GRHIP_API int grhip_optfir_high_pass(double gain, double fs, double freq1, double freq2, double passband_ripple_db,
                                     double stopband_atten_db, int nextra_taps, double *out, size_t cap, size_t *ntaps);
GRHIP_API int grhip_optfir_band_pass(double gain, double fs, double freq_sb1, double freq_pb1, double freq_pb2, double freq_sb2,
                                     double passband_ripple_db, double stopband_atten_db, int nextra_taps, double *out,
                                     size_t cap, size_t *ntaps);
GRHIP_API int grhip_optfir_band_reject(double gain, double fs, double freq_pb1, double freq_sb1, double freq_sb2, double freq_pb2,
                                       double passband_ripple_db, double stopband_atten_db, int nextra_taps, double *out,
                                       size_t cap, size_t *ntaps);
GRHIP_API int grhip_optfir_spec(int kind, double gain, double fs, const double *freqs, size_t nfreqs, double passband_ripple_db,
                                double stopband_atten_db, int nextra_taps, int *order, double *bands, double *ampl,
                                double *weight, size_t *nbands);

/* ======================================================================
 * gr_hilbert_fc
 *   replaces gr_make_hilbert_fc(unsigned int ntaps)
 *   filter/gr_hilbert_fc.cc:39-67, taps from general/gr_firdes.cc:538-565
 * float in, complex out: out[i] = (in[i + d_ntaps/2], fir_fff(&in[i])) with d_ntaps = ntaps | 1
 * and the taps of grhip_firdes_hilbert(d_ntaps, 3, 6.76).  gr_sync_block, history = d_ntaps: work
 * reads noutput_items + d_ntaps - 1 items.
 * Stated deviation: ntaps <= 1 is GRHIP_EINVAL.  The reference accepts it, divides 0 by 0 in
 * gr_firdes::hilbert and filters with one NaN tap.
 * GRHIP_MODE_GENERIC sums every tap, zeros included, in gr_fir_fff_generic's order: bit-exact.
 * FAST uses the structure of the taps (see gr_filter_delay_fc below).  work takes host pointers,
 * work_device device pointers (items 4-byte aligned, at any offset) and a stream.
 * taps() copies the d_ntaps forward taps into out (capacity floats) and returns their number.
 * ====================================================================== */
typedef struct grhip_hilbert_fc grhip_hilbert_fc;
GRHIP_API int grhip_hilbert_fc_create(grhip_hilbert_fc **h, unsigned ntaps, int device);
GRHIP_API void grhip_hilbert_fc_destroy(grhip_hilbert_fc *h);
GRHIP_API int grhip_hilbert_fc_set_mode(grhip_hilbert_fc *h, int mode);
GRHIP_API int grhip_hilbert_fc_history(const grhip_hilbert_fc *h);
GRHIP_API int grhip_hilbert_fc_ntaps(const grhip_hilbert_fc *h);
GRHIP_API int grhip_hilbert_fc_taps(const grhip_hilbert_fc *h, float *out, size_t capacity);
GRHIP_API int grhip_hilbert_fc_is_sparse(const grhip_hilbert_fc *h);
GRHIP_API int grhip_hilbert_fc_work(grhip_hilbert_fc *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_hilbert_fc_work_device(grhip_hilbert_fc *h, int noutput_items, const void *d_in, void *d_out,
                                           void *stream);

/* ======================================================================
 * gr_filter_delay_fc
 *   replaces gr_make_filter_delay_fc(const std::vector<float> &taps)
 *   filter/gr_filter_delay_fc.cc:38-80
 * One or two float inputs, complex out: out[j] = (in0[j + d_delay], fir_fff(&in1[j])) with
 * d_delay = ntaps / 2 and history = ntaps on every input; in1 == NULL is the one-input form
 * (in1 = in0).  Any tap count from 1 to 16384, even counts included.  The reference block has no
 * set_taps; neither has this one.
 * GRHIP_MODE_GENERIC: bit-exact (gr_fir_fff_generic's order over all taps).  FAST: when the taps
 * are of odd length >= 3, exactly zero at every even distance from the centre and exactly
 * antisymmetric (is_sparse() == 1; checked on the given floats, no tolerance) and there is one
 * input, a kernel that multiplies t[h+i] by (x[c-i] - x[c+i]) over odd i only; otherwise, and
 * with two inputs, a kernel that uses every tap.  Above 2048 taps FAST runs the GENERIC kernel.
 * Stated deviation of that first kernel: the zero taps are never multiplied.  A sample that is
 * not finite therefore reaches the imaginary part of the outputs it lies an odd distance <= h
 * from the centre of, and no other; the reference (and GENERIC) also form 0 * inf = NaN at the
 * even distances.  The real part carries the sample itself in every mode.
 * ====================================================================== */
typedef struct grhip_filter_delay_fc grhip_filter_delay_fc;
GRHIP_API int grhip_filter_delay_fc_create(grhip_filter_delay_fc **h, const float *taps, size_t ntaps, int device);
GRHIP_API void grhip_filter_delay_fc_destroy(grhip_filter_delay_fc *h);
GRHIP_API int grhip_filter_delay_fc_set_mode(grhip_filter_delay_fc *h, int mode);
GRHIP_API int grhip_filter_delay_fc_history(const grhip_filter_delay_fc *h);
GRHIP_API int grhip_filter_delay_fc_ntaps(const grhip_filter_delay_fc *h);
GRHIP_API int grhip_filter_delay_fc_taps(const grhip_filter_delay_fc *h, float *out, size_t capacity);
GRHIP_API int grhip_filter_delay_fc_is_sparse(const grhip_filter_delay_fc *h);
GRHIP_API int grhip_filter_delay_fc_work(grhip_filter_delay_fc *h, int noutput_items, const void *in0,
                                         const void *in1, void *out);
GRHIP_API int grhip_filter_delay_fc_work_device(grhip_filter_delay_fc *h, int noutput_items, const void *d_in0,
                                                const void *d_in1, void *d_out, void *stream);

/* ======================================================================
 * gr_goertzel_fc
 *   replaces gr_make_goertzel_fc(int rate, int len, float freq)
 *   filter/gr_goertzel_fc.cc:38-78, filter/gri_goertzel.cc:36-75
 * gr_sync_decimator by len: one DFT bin per block of len floats, no state across blocks.
 * w = (float)(2 pi freq / rate), wr = 2 cosf(w), wi = sinf(w) on the host; per sample
 * y = (x + wr*d1) - d2 in float; out = ((float)((0.5*wr*d1 - d2)/len) formed in double,
 * (wi*d1)/(float)len in float).  set_freq / set_rate hold from the next call on (the reference
 * has no latch here).  GRHIP_EINVAL for len < 1 (or above 2^24) and for rate == 0.
 * GRHIP_MODE_GENERIC is that recurrence, one lane per block: bit-exact, and as inaccurate as the
 * reference at low bin frequencies (its float state loses 3e-4 at rate 8000, len 2000, freq 5).
 * FAST evaluates the recurrence's closed form, sum_n x[n] (cos((len-n)w'), wi U_(len-1-n)) / len
 * with cos w' = wr/2, from a table built in double: a better-conditioned sum than the
 * reference's, so it is compared with the float64 recurrence, not with the float one.
 * ====================================================================== */
typedef struct grhip_goertzel_fc grhip_goertzel_fc;
GRHIP_API int grhip_goertzel_fc_create(grhip_goertzel_fc **h, int rate, int len, float freq, int device);
GRHIP_API void grhip_goertzel_fc_destroy(grhip_goertzel_fc *h);
GRHIP_API int grhip_goertzel_fc_set_freq(grhip_goertzel_fc *h, float freq);
GRHIP_API int grhip_goertzel_fc_set_rate(grhip_goertzel_fc *h, int rate);
GRHIP_API int grhip_goertzel_fc_set_mode(grhip_goertzel_fc *h, int mode);
GRHIP_API int grhip_goertzel_fc_decimation(const grhip_goertzel_fc *h);   /* len */
GRHIP_API int grhip_goertzel_fc_work(grhip_goertzel_fc *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_goertzel_fc_work_device(grhip_goertzel_fc *h, int noutput_items, const void *d_in, void *d_out,
                                            void *stream);

/* ======================================================================
 * gr_dc_blocker_ff / gr_dc_blocker_cc
 *   replaces gr_make_dc_blocker_ff(int D = 32, bool long_form = true), _cc likewise
 *   filter/gr_dc_blocker_ff.cc:31-53 (moving_averager_f::filter), 57-80, 96-103 (get_group_delay),
 *   105-138 (work); filter/gr_dc_blocker_cc.cc the same lines
 * gr_sync_block, history 1.  2 (short form) or 4 (long form) moving averagers in a row, each
 * y = (x - x[n-D]) + y_prev kept as a float recurrence and returned as y / (float)D; the output is
 * the input delayed by get_group_delay() = D - 1 (short) or 2D - 2 (long) minus the last average.
 * All state is in the handle and carries across calls.  D = 1 is legal; GRHIP_EINVAL for D < 1 (the
 * reference's deque(D - 1) throws) and for D > 1345, the most the FAST kernel's LDS layout carries
 * in its tightest form (complex, long form).
 * GRHIP_MODE_GENERIC is that recurrence, one wavefront per stream: bit-exact, including the rounding
 * errors the recurrence never forgets (the output drifts from the float64 value of the same filter
 * by about 1e-4 of a DC level of 1 over 2 M samples, 1e-3 at DC 10).  FAST forms every stage as a true
 * D-window sum of the stage before it: no state older than the filter's span, an error of a few ulp
 * of the input level whatever the stream length; it is compared with the float64 filter.
 * The two modes keep different states; set_mode and set_streams restart the filter from zero.
 * set_streams(S): work and work_device then take S streams of noutput_items each, back to back in
 * `in` and `out`, each with its own state (S = 1 after create).
 * ====================================================================== */
typedef struct grhip_dc_blocker_ff grhip_dc_blocker_ff;
GRHIP_API int grhip_dc_blocker_ff_create(grhip_dc_blocker_ff **h, int D, int long_form, int device);
GRHIP_API void grhip_dc_blocker_ff_destroy(grhip_dc_blocker_ff *h);
GRHIP_API int grhip_dc_blocker_ff_set_mode(grhip_dc_blocker_ff *h, int mode);
GRHIP_API int grhip_dc_blocker_ff_set_streams(grhip_dc_blocker_ff *h, int nstreams);
GRHIP_API int grhip_dc_blocker_ff_group_delay(const grhip_dc_blocker_ff *h);
GRHIP_API int grhip_dc_blocker_ff_work(grhip_dc_blocker_ff *h, int noutput_items, const void *in,
                                            void *out);
GRHIP_API int grhip_dc_blocker_ff_work_device(grhip_dc_blocker_ff *h, int noutput_items,
                                                   const void *d_in, void *d_out, void *stream);
typedef struct grhip_dc_blocker_cc grhip_dc_blocker_cc;
GRHIP_API int grhip_dc_blocker_cc_create(grhip_dc_blocker_cc **h, int D, int long_form, int device);
GRHIP_API void grhip_dc_blocker_cc_destroy(grhip_dc_blocker_cc *h);
GRHIP_API int grhip_dc_blocker_cc_set_mode(grhip_dc_blocker_cc *h, int mode);
GRHIP_API int grhip_dc_blocker_cc_set_streams(grhip_dc_blocker_cc *h, int nstreams);
GRHIP_API int grhip_dc_blocker_cc_group_delay(const grhip_dc_blocker_cc *h);
GRHIP_API int grhip_dc_blocker_cc_work(grhip_dc_blocker_cc *h, int noutput_items, const void *in,
                                            void *out);
GRHIP_API int grhip_dc_blocker_cc_work_device(grhip_dc_blocker_cc *h, int noutput_items,
                                                   const void *d_in, void *d_out, void *stream);

/* ======================================================================
 * gr_moving_average_ff / _cc / _ss / _ii
 *   replaces gr_make_moving_average_XX(int length, O scale, int max_iter = 4096)
 *   gengen/gr_moving_average_XX.cc.t:38-50 (set_history(length)), 56-62 (set_length_and_scale),
 *   64-93 (work)
 * gr_sync_block, history = length.  Every work call starts sum at 0, adds the first length - 1
 * items in order and then, per output, sum += in[i+length-1]; out = sum * scale; sum -= in[i]; it
 * returns min(noutput_items, max_iter).  _ss sums in a short and _ii in an int (wrapping), and
 * multiplies by scale in the output type; _cc's scale is complex.  set_length_and_scale latches:
 * the next work (or work_device) call applies it, computes nothing and returns 0 (.cc.t:69-75).
 * work is ONE reference work call: `in` holds min(noutput_items, max_iter) + length - 1 items.
 * work_device stands for the SUCCESSIVE reference work calls that produce noutput_items outputs:
 * calls of exactly max_iter outputs, the last one shorter; d_in holds noutput_items + length - 1
 * items and it returns noutput_items.  The reference scheduler's own chunking depends on buffer
 * fill and is not deterministic, so this chunking is the one DEFINED HERE; GRHIP_MODE_GENERIC is
 * bit-exact to the reference's arithmetic run with it.  FAST forms every window sum on its own
 * (no dependence on the chunking, error a few ulp of length max|x|); the integer types are exact
 * in both modes.  GRHIP_EINVAL for length < 1, length > 8449 (LDS layout) and max_iter < 1.
 * ====================================================================== */
typedef struct grhip_moving_average_ff grhip_moving_average_ff;
GRHIP_API void grhip_moving_average_ff_destroy(grhip_moving_average_ff *h);
GRHIP_API int grhip_moving_average_ff_set_mode(grhip_moving_average_ff *h, int mode);
GRHIP_API int grhip_moving_average_ff_history(const grhip_moving_average_ff *h);
GRHIP_API int grhip_moving_average_ff_max_iter(const grhip_moving_average_ff *h);
GRHIP_API int grhip_moving_average_ff_work(grhip_moving_average_ff *h, int noutput_items,
                                                const void *in, void *out);
GRHIP_API int grhip_moving_average_ff_work_device(grhip_moving_average_ff *h, int noutput_items,
                                                       const void *d_in, void *d_out, void *stream);
typedef struct grhip_moving_average_cc grhip_moving_average_cc;
GRHIP_API void grhip_moving_average_cc_destroy(grhip_moving_average_cc *h);
GRHIP_API int grhip_moving_average_cc_set_mode(grhip_moving_average_cc *h, int mode);
GRHIP_API int grhip_moving_average_cc_history(const grhip_moving_average_cc *h);
GRHIP_API int grhip_moving_average_cc_max_iter(const grhip_moving_average_cc *h);
GRHIP_API int grhip_moving_average_cc_work(grhip_moving_average_cc *h, int noutput_items,
                                                const void *in, void *out);
GRHIP_API int grhip_moving_average_cc_work_device(grhip_moving_average_cc *h, int noutput_items,
                                                       const void *d_in, void *d_out, void *stream);
typedef struct grhip_moving_average_ss grhip_moving_average_ss;
GRHIP_API void grhip_moving_average_ss_destroy(grhip_moving_average_ss *h);
GRHIP_API int grhip_moving_average_ss_set_mode(grhip_moving_average_ss *h, int mode);
GRHIP_API int grhip_moving_average_ss_history(const grhip_moving_average_ss *h);
GRHIP_API int grhip_moving_average_ss_max_iter(const grhip_moving_average_ss *h);
GRHIP_API int grhip_moving_average_ss_work(grhip_moving_average_ss *h, int noutput_items,
                                                const void *in, void *out);
GRHIP_API int grhip_moving_average_ss_work_device(grhip_moving_average_ss *h, int noutput_items,
                                                       const void *d_in, void *d_out, void *stream);
typedef struct grhip_moving_average_ii grhip_moving_average_ii;
GRHIP_API void grhip_moving_average_ii_destroy(grhip_moving_average_ii *h);
GRHIP_API int grhip_moving_average_ii_set_mode(grhip_moving_average_ii *h, int mode);
GRHIP_API int grhip_moving_average_ii_history(const grhip_moving_average_ii *h);
GRHIP_API int grhip_moving_average_ii_max_iter(const grhip_moving_average_ii *h);
GRHIP_API int grhip_moving_average_ii_work(grhip_moving_average_ii *h, int noutput_items,
                                                const void *in, void *out);
GRHIP_API int grhip_moving_average_ii_work_device(grhip_moving_average_ii *h, int noutput_items,
                                                       const void *d_in, void *d_out, void *stream);
GRHIP_API int grhip_moving_average_ff_create(grhip_moving_average_ff **h, int length, float scale, int max_iter,
                                             int device);
GRHIP_API int grhip_moving_average_cc_create(grhip_moving_average_cc **h, int length, float scale_re, float scale_im,
                                             int max_iter, int device);
GRHIP_API int grhip_moving_average_ss_create(grhip_moving_average_ss **h, int length, short scale, int max_iter,
                                             int device);
GRHIP_API int grhip_moving_average_ii_create(grhip_moving_average_ii **h, int length, int scale, int max_iter,
                                             int device);
GRHIP_API int grhip_moving_average_ff_set_length_and_scale(grhip_moving_average_ff *h, int length, float scale);
GRHIP_API int grhip_moving_average_cc_set_length_and_scale(grhip_moving_average_cc *h, int length, float scale_re,
                                                           float scale_im);
GRHIP_API int grhip_moving_average_ss_set_length_and_scale(grhip_moving_average_ss *h, int length, short scale);
GRHIP_API int grhip_moving_average_ii_set_length_and_scale(grhip_moving_average_ii *h, int length, int scale);

/* ======================================================================
 * gr_integrate_ff / _cc / _ss / _ii
 *   replaces gr_make_integrate_XX(int decim)
 *   gengen/gr_integrate_XX.cc.t:38-46, 52-67
 * gr_sync_decimator by decim, no state (d_count is unused): out[i] = 0, then += in[i*decim + j] for
 * j ascending.  GRHIP_MODE_GENERIC keeps that order (bit-exact); FAST sums each output with up to
 * 64 lanes; the integer types wrap and are exact in both.  GRHIP_EINVAL for decim < 1.
 * ====================================================================== */
typedef struct grhip_integrate_ff grhip_integrate_ff;
GRHIP_API int grhip_integrate_ff_create(grhip_integrate_ff **h, int decim, int device);
GRHIP_API void grhip_integrate_ff_destroy(grhip_integrate_ff *h);
GRHIP_API int grhip_integrate_ff_set_mode(grhip_integrate_ff *h, int mode);
GRHIP_API int grhip_integrate_ff_decimation(const grhip_integrate_ff *h);
GRHIP_API int grhip_integrate_ff_work(grhip_integrate_ff *h, int noutput_items, const void *in,
                                           void *out);
GRHIP_API int grhip_integrate_ff_work_device(grhip_integrate_ff *h, int noutput_items,
                                                  const void *d_in, void *d_out, void *stream);
typedef struct grhip_integrate_cc grhip_integrate_cc;
GRHIP_API int grhip_integrate_cc_create(grhip_integrate_cc **h, int decim, int device);
GRHIP_API void grhip_integrate_cc_destroy(grhip_integrate_cc *h);
GRHIP_API int grhip_integrate_cc_set_mode(grhip_integrate_cc *h, int mode);
GRHIP_API int grhip_integrate_cc_decimation(const grhip_integrate_cc *h);
GRHIP_API int grhip_integrate_cc_work(grhip_integrate_cc *h, int noutput_items, const void *in,
                                           void *out);
GRHIP_API int grhip_integrate_cc_work_device(grhip_integrate_cc *h, int noutput_items,
                                                  const void *d_in, void *d_out, void *stream);
typedef struct grhip_integrate_ss grhip_integrate_ss;
GRHIP_API int grhip_integrate_ss_create(grhip_integrate_ss **h, int decim, int device);
GRHIP_API void grhip_integrate_ss_destroy(grhip_integrate_ss *h);
GRHIP_API int grhip_integrate_ss_set_mode(grhip_integrate_ss *h, int mode);
GRHIP_API int grhip_integrate_ss_decimation(const grhip_integrate_ss *h);
GRHIP_API int grhip_integrate_ss_work(grhip_integrate_ss *h, int noutput_items, const void *in,
                                           void *out);
GRHIP_API int grhip_integrate_ss_work_device(grhip_integrate_ss *h, int noutput_items,
                                                  const void *d_in, void *d_out, void *stream);
typedef struct grhip_integrate_ii grhip_integrate_ii;
GRHIP_API int grhip_integrate_ii_create(grhip_integrate_ii **h, int decim, int device);
GRHIP_API void grhip_integrate_ii_destroy(grhip_integrate_ii *h);
GRHIP_API int grhip_integrate_ii_set_mode(grhip_integrate_ii *h, int mode);
GRHIP_API int grhip_integrate_ii_decimation(const grhip_integrate_ii *h);
GRHIP_API int grhip_integrate_ii_work(grhip_integrate_ii *h, int noutput_items, const void *in,
                                           void *out);
GRHIP_API int grhip_integrate_ii_work_device(grhip_integrate_ii *h, int noutput_items,
                                                  const void *d_in, void *d_out, void *stream);

/* ======================================================================
 * The spectrum-estimate blocks: the stages of blks2.logpwrfft behind its transform
 * (python/gnuradio/blks2impl/logpwrfft.py:47-63), each a block of its own.
 * All of them take S streams back to back in `in` and `out` ([S][items], S = 1 after create;
 * set_streams(S) restarts a block from the reference's initial state).  set_mode keeps the state.
 *
 * gr_complex_to_mag_squared
 *   replaces gr_make_complex_to_mag_squared(unsigned int vlen = 1)
 *   general/gr_complex_to_xxx.cc:180-203
 * Items of vlen gr_complex in, vlen floats out: re * re + im * im as two rounded float products and
 * one rounded add, never contracted.  Bit-exact in both modes (the modes do not differ).
 * ====================================================================== */
typedef struct grhip_complex_to_mag_squared grhip_complex_to_mag_squared;
GRHIP_API int grhip_complex_to_mag_squared_create(grhip_complex_to_mag_squared **h, int vlen, int device);
GRHIP_API void grhip_complex_to_mag_squared_destroy(grhip_complex_to_mag_squared *h);
GRHIP_API int grhip_complex_to_mag_squared_set_mode(grhip_complex_to_mag_squared *h, int mode);
GRHIP_API int grhip_complex_to_mag_squared_set_streams(grhip_complex_to_mag_squared *h, int nstreams);
GRHIP_API int grhip_complex_to_mag_squared_work(grhip_complex_to_mag_squared *h, int noutput_items, const void *in,
                                                void *out);
GRHIP_API int grhip_complex_to_mag_squared_work_device(grhip_complex_to_mag_squared *h, int noutput_items,
                                                       const void *d_in, void *d_out, void *stream);

/* ======================================================================
 * gr_complex_to_mag
 *   replaces gr_make_complex_to_mag(unsigned int vlen = 1)
 *   general/gr_complex_to_xxx.cc:143-171 (the std::abs loop)
 * Items of vlen gr_complex in, vlen floats out, S streams back to back as above.  One form in every
 * mode: (float)sqrt((double)re * re + (double)im * im) -- two rounded double products, one rounded
 * add, a correctly rounded double square root, one narrowing, never contracted.  As hypotf, an
 * infinite part gives +inf whatever the other part is.  std::abs(gr_complex) is glibc's hypotf; this
 * form equals the hypotf of glibc 2.35 on the recorded set of tests/golden/ref_complex_to_mag.npz
 * (normals over 60 decades, zeros, denormals, axis-aligned values, squares that overflow a float,
 * infinities and NaNs) bit for bit, and on x86-64 it did on 20 000 000 random pairs.
 * ====================================================================== */
typedef struct grhip_complex_to_mag grhip_complex_to_mag;
GRHIP_API int grhip_complex_to_mag_create(grhip_complex_to_mag **h, int vlen, int device);
GRHIP_API void grhip_complex_to_mag_destroy(grhip_complex_to_mag *h);
GRHIP_API int grhip_complex_to_mag_set_mode(grhip_complex_to_mag *h, int mode);
GRHIP_API int grhip_complex_to_mag_set_streams(grhip_complex_to_mag *h, int nstreams);
GRHIP_API int grhip_complex_to_mag_work(grhip_complex_to_mag *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_complex_to_mag_work_device(grhip_complex_to_mag *h, int noutput_items, const void *d_in, void *d_out,
                                               void *stream);

/* ======================================================================
 * gr_single_pole_iir_filter_ff
 *   replaces gr_make_single_pole_iir_filter_ff(double alpha, unsigned int vlen = 1)
 *   filter/gr_single_pole_iir.h:60-97 (set_taps, filter), filter/gr_single_pole_iir_filter_ff.cc:53-81
 * Items of vlen floats, one filter per element.  The taps are double and the state is a float:
 * y = (float)(alpha * (double)x + (1.0 - alpha) * (double)y_prev), two double products and one
 * double add, never contracted.  The state starts at 0, carries across calls, and set_taps keeps
 * it.  GRHIP_ERANGE for alpha outside [0, 1] (create and set_taps; std::out_of_range there).
 * GRHIP_MODE_GENERIC: one lane per (stream, element) walks the items in order; bit-exact for any
 * vlen.  With vlen == 1 that is one lane per stream: correct and slow.
 * GRHIP_MODE_FAST: the same kernel when streams x vlen is at least 65536 lanes (the device is full
 * then); otherwise the item axis is cut into chunks of grhip_single_pole_iir_filter_ff_chunk() items:
 * every chunk's answer from a zero start, the chunks chained through the recurrence's affine form
 * (y_end = local_end + (1 - alpha)^len y_start), and a second walk from each chunk's true start.
 * Within 1e-5 of the output's peak of the float64 recurrence.
 * ====================================================================== */
typedef struct grhip_single_pole_iir_filter_ff grhip_single_pole_iir_filter_ff;
GRHIP_API int grhip_single_pole_iir_filter_ff_create(grhip_single_pole_iir_filter_ff **h, double alpha, int vlen,
                                                     int device);
GRHIP_API void grhip_single_pole_iir_filter_ff_destroy(grhip_single_pole_iir_filter_ff *h);
GRHIP_API int grhip_single_pole_iir_filter_ff_set_taps(grhip_single_pole_iir_filter_ff *h, double alpha);
GRHIP_API int grhip_single_pole_iir_filter_ff_set_mode(grhip_single_pole_iir_filter_ff *h, int mode);
GRHIP_API int grhip_single_pole_iir_filter_ff_set_streams(grhip_single_pole_iir_filter_ff *h, int nstreams);
GRHIP_API int grhip_single_pole_iir_filter_ff_chunk(void);
GRHIP_API int grhip_single_pole_iir_filter_ff_work(grhip_single_pole_iir_filter_ff *h, int noutput_items,
                                                   const void *in, void *out);
GRHIP_API int grhip_single_pole_iir_filter_ff_work_device(grhip_single_pole_iir_filter_ff *h, int noutput_items,
                                                          const void *d_in, void *d_out, void *stream);

/* ======================================================================
 * gr_nlog10_ff
 *   replaces gr_make_nlog10_ff(float n, unsigned vlen = 1, float k = 0)
 *   general/gr_nlog10_ff.cc:49-64
 * out = n * log10(max(in, 1e-18f)) + k in float.  The device's log10f is not glibc's, so neither
 * mode is bit-exact: both stay within 4 float ulps (at the output's magnitude) of the value computed
 * in float64 from the same float input.  Zero and negative inputs give what the clamp gives,
 * n * -18 + k; a NaN stays NaN (std::max returns its first argument then).
 * ====================================================================== */
typedef struct grhip_nlog10_ff grhip_nlog10_ff;
GRHIP_API int grhip_nlog10_ff_create(grhip_nlog10_ff **h, float n, int vlen, float k, int device);
GRHIP_API void grhip_nlog10_ff_destroy(grhip_nlog10_ff *h);
GRHIP_API int grhip_nlog10_ff_set_mode(grhip_nlog10_ff *h, int mode);
GRHIP_API int grhip_nlog10_ff_set_streams(grhip_nlog10_ff *h, int nstreams);
GRHIP_API int grhip_nlog10_ff_work(grhip_nlog10_ff *h, int noutput_items, const void *in, void *out);
GRHIP_API int grhip_nlog10_ff_work_device(grhip_nlog10_ff *h, int noutput_items, const void *d_in, void *d_out,
                                          void *stream);

/* ======================================================================
 * gr_keep_one_in_n
 *   replaces gr_make_keep_one_in_n(size_t item_size, int n)
 *   general/gr_keep_one_in_n.cc:52-65 (set_n), 67-105 (general_work)
 * A countdown starts at n, drops by one per input item, and the item at which it reaches 0 is
 * copied out and reloads it.  set_n clamps n to >= 1 and reloads the countdown; the countdown
 * carries across calls.  work / work_device take n_in input items (per stream) and return the items
 * produced; `out` needs room for grhip_keep_one_in_n_produced(h, n_in) items, which tells the count
 * without changing the state.  The streams share the countdown.  Tags are out of scope.
 * ====================================================================== */
typedef struct grhip_keep_one_in_n grhip_keep_one_in_n;
GRHIP_API int grhip_keep_one_in_n_create(grhip_keep_one_in_n **h, size_t item_size, int n, int device);
GRHIP_API void grhip_keep_one_in_n_destroy(grhip_keep_one_in_n *h);
GRHIP_API int grhip_keep_one_in_n_set_n(grhip_keep_one_in_n *h, int n);
GRHIP_API int grhip_keep_one_in_n_set_streams(grhip_keep_one_in_n *h, int nstreams);
GRHIP_API int grhip_keep_one_in_n_produced(grhip_keep_one_in_n *h, int n_in);
GRHIP_API int grhip_keep_one_in_n_work(grhip_keep_one_in_n *h, int n_in, const void *in, void *out);
GRHIP_API int grhip_keep_one_in_n_work_device(grhip_keep_one_in_n *h, int n_in, const void *d_in, void *d_out,
                                              void *stream);

/* ======================================================================
 * blks2.logpwrfft_c / blks2.logpwrfft_f
 *   replaces logpwrfft_c(sample_rate, fft_size, ref_scale, frame_rate, avg_alpha, average, win=None)
 *   gnuradio-core/src/python/gnuradio/blks2impl/logpwrfft.py:26-154,
 *   blks2impl/stream_to_vector_decimator.py:24-93, gnuradio/window.py:166-176,
 *   general/gr_keep_one_in_n.cc:52-105
 * The hier block stream_to_vector -> keep_one_in_n(decim) -> fft_vcc | fft_vfc (forward, windowed)
 * -> complex_to_mag_squared -> single_pole_iir_filter_ff -> nlog10_ff(10, fft_size, k) in one
 * transform kernel (plus one in-place averaging pass when averaging is on).  Results are bit for bit
 * those of this library's own blocks run in that order, in every mode (set_mode selects the IIR's
 * GENERIC / FAST form as for single_pole_iir_filter_ff).
 *   decim = max(1, (int)round(sample_rate / fft_size / frame_rate)), round half away from zero;
 *   k = -20 log10(fft_size) - 10 log10(window_power / fft_size) - 20 log10(ref_scale / 2), in double,
 *       narrowed to float; window_power = the sum of squares of the window's doubles, in order.
 * `window` holds the DOUBLES the reference's win(fft_size) returns; NULL / 0 is the default,
 * grhip_window_blackmanharris.  The transform gets them narrowed to float.  A window whose length
 * is neither 0 nor fft_size is refused by gr_fft_vcc::set_window and the refusal ignored, as in the
 * reference: the transform runs unwindowed while k comes from the given values.
 * All arithmetic is true division; Python 2's integer division of all-integer arguments is not
 * reproduced.
 * Averaging off means IIR taps of exactly 1.0: the kernel stores dB directly and leaves the power of
 * every stream's last kept frame in the filter's state.  The reference computes
 * (float)(1.0 x + 0.0 y_prev), which is x for every finite y_prev; after a non-finite state the two
 * differ.  Non-finite input is out of scope.
 * work / work_device: the input is nstreams x n_frames whole frames of fft_size samples (gr_complex
 * for _c, float for _f), streams back to back; the output is nstreams x produced frames of fft_size
 * floats; the return value is the frames produced per stream (grhip_logpwrfft_X_produced tells it
 * without changing anything).  A call that keeps nothing returns 0 and advances the countdown.
 * set_streams restarts state and countdown (the streams share the countdown); set_decimation,
 * set_vec_rate and set_sample_rate reload the countdown; set_average and set_avg_alpha keep the
 * filter's state.
 * GRHIP_ERANGE: fft_size <= 0, avg_alpha outside [0, 1].  GRHIP_EINVAL: ref_scale <= 0, a window of
 * power zero, fft_size == 1 with the default window (the reference's ValueError /
 * ZeroDivisionError), a decimation that is not finite.  All refused before any device work.
 * ====================================================================== */
typedef struct grhip_logpwrfft_c grhip_logpwrfft_c;
GRHIP_API int grhip_logpwrfft_c_create(grhip_logpwrfft_c **h, double sample_rate, int fft_size, double ref_scale,
                                       double frame_rate, double avg_alpha, int average, const double *window,
                                       size_t window_len, int device);
GRHIP_API void grhip_logpwrfft_c_destroy(grhip_logpwrfft_c *h);
GRHIP_API int grhip_logpwrfft_c_set_mode(grhip_logpwrfft_c *h, int mode);
GRHIP_API int grhip_logpwrfft_c_set_streams(grhip_logpwrfft_c *h, int nstreams);
/* logpwrfft.py:70-108; set_decimation is stream_to_vector_decimator.py:66-72 */
GRHIP_API int grhip_logpwrfft_c_set_decimation(grhip_logpwrfft_c *h, double decim);
GRHIP_API int grhip_logpwrfft_c_set_vec_rate(grhip_logpwrfft_c *h, double vec_rate);
GRHIP_API int grhip_logpwrfft_c_set_sample_rate(grhip_logpwrfft_c *h, double sample_rate);
GRHIP_API int grhip_logpwrfft_c_set_average(grhip_logpwrfft_c *h, int average);
GRHIP_API int grhip_logpwrfft_c_set_avg_alpha(grhip_logpwrfft_c *h, double avg_alpha);
/* logpwrfft.py:110-138, stream_to_vector_decimator.py:77-93 (NaN for a null handle) */
GRHIP_API double grhip_logpwrfft_c_sample_rate(grhip_logpwrfft_c *h);
GRHIP_API int grhip_logpwrfft_c_decimation(grhip_logpwrfft_c *h);
GRHIP_API double grhip_logpwrfft_c_frame_rate(grhip_logpwrfft_c *h);
GRHIP_API int grhip_logpwrfft_c_average(grhip_logpwrfft_c *h);
GRHIP_API double grhip_logpwrfft_c_avg_alpha(grhip_logpwrfft_c *h);
GRHIP_API int grhip_logpwrfft_c_produced(grhip_logpwrfft_c *h, int n_frames);
/* the averaging filter's state, nstreams x fft_size floats of linear power, after the work queued so far */
GRHIP_API int grhip_logpwrfft_c_state(grhip_logpwrfft_c *h, float *out);
GRHIP_API int grhip_logpwrfft_c_work(grhip_logpwrfft_c *h, int n_frames, const void *in, void *out);
GRHIP_API int grhip_logpwrfft_c_work_device(grhip_logpwrfft_c *h, int n_frames, const void *d_in, void *d_out,
                                            void *stream);

typedef struct grhip_logpwrfft_f grhip_logpwrfft_f;
GRHIP_API int grhip_logpwrfft_f_create(grhip_logpwrfft_f **h, double sample_rate, int fft_size, double ref_scale,
                                       double frame_rate, double avg_alpha, int average, const double *window,
                                       size_t window_len, int device);
GRHIP_API void grhip_logpwrfft_f_destroy(grhip_logpwrfft_f *h);
GRHIP_API int grhip_logpwrfft_f_set_mode(grhip_logpwrfft_f *h, int mode);
GRHIP_API int grhip_logpwrfft_f_set_streams(grhip_logpwrfft_f *h, int nstreams);
/* logpwrfft.py:70-108; set_decimation is stream_to_vector_decimator.py:66-72 */
GRHIP_API int grhip_logpwrfft_f_set_decimation(grhip_logpwrfft_f *h, double decim);
GRHIP_API int grhip_logpwrfft_f_set_vec_rate(grhip_logpwrfft_f *h, double vec_rate);
GRHIP_API int grhip_logpwrfft_f_set_sample_rate(grhip_logpwrfft_f *h, double sample_rate);
GRHIP_API int grhip_logpwrfft_f_set_average(grhip_logpwrfft_f *h, int average);
GRHIP_API int grhip_logpwrfft_f_set_avg_alpha(grhip_logpwrfft_f *h, double avg_alpha);
/* logpwrfft.py:110-138, stream_to_vector_decimator.py:77-93 (NaN for a null handle) */
GRHIP_API double grhip_logpwrfft_f_sample_rate(grhip_logpwrfft_f *h);
GRHIP_API int grhip_logpwrfft_f_decimation(grhip_logpwrfft_f *h);
GRHIP_API double grhip_logpwrfft_f_frame_rate(grhip_logpwrfft_f *h);
GRHIP_API int grhip_logpwrfft_f_average(grhip_logpwrfft_f *h);
GRHIP_API double grhip_logpwrfft_f_avg_alpha(grhip_logpwrfft_f *h);
GRHIP_API int grhip_logpwrfft_f_produced(grhip_logpwrfft_f *h, int n_frames);
/* the averaging filter's state, nstreams x fft_size floats of linear power, after the work queued so far */
GRHIP_API int grhip_logpwrfft_f_state(grhip_logpwrfft_f *h, float *out);
GRHIP_API int grhip_logpwrfft_f_work(grhip_logpwrfft_f *h, int n_frames, const void *in, void *out);
GRHIP_API int grhip_logpwrfft_f_work_device(grhip_logpwrfft_f *h, int n_frames, const void *d_in, void *d_out,
                                            void *stream);

/* window.blackmanharris(fft_size) (gnuradio/window.py:166-176): out[i] = sum over c of
 * (-1)**c * coeff[c] * cos(2.0 * c * pi * (i + 0.5) / (fft_size - 1)), accumulated from 0 in
 * coefficient order, coeff = (0.35875, 0.48829, 0.14128, 0.01168).  Host arithmetic only, no device
 * needed.  GRHIP_EINVAL for fft_size == 1 (division by zero there) and negative sizes. */
GRHIP_API int grhip_window_blackmanharris(int fft_size, double *out);

/* ======================================================================
 * The power squelch blocks.  A handle takes S streams back to back in `in` ([S][n_in], S = 1 after
 * create); stream s writes its items from out + s * n_in items and produced[s] tells how many: n_in
 * without gating, fewer with it, and what lies behind them in `out` is not touched.  `out` may not
 * overlap `in`.  work / work_device return GRHIP_OK; n_in == 0 is a successful no-op; work_device
 * (device buffers, d_produced S ints on the device) does not synchronise.  Finite inputs only.
 * Per stream the block remembers the detector's output, the machine's state, the ramp position and
 * the envelope, on the device and across calls.  set_streams resizes that and restarts every stream
 * from the reference's initial state; every other setter keeps it and holds from the next work call.
 * unmuted(h, s) is 1 or 0; state(h, s, ...) reads one stream's state (0 muted, 1 attack, 2 unmuted,
 * 3 decay: the reference's enum order); both wait for the handle's queued work.
 * GRHIP_ERANGE for alpha outside [0, 1]; GRHIP_EINVAL for ramp < 0 (or past 2^24), S < 1, n_in < 0.
 *
 * gr_pwr_squelch_cc
 *   replaces gr_make_pwr_squelch_cc(double db, double alpha = 0.0001, int ramp = 0, bool gate = false)
 *   general/gr_pwr_squelch_cc.h:58 (set_threshold: pow(10.0, db / 10)), :57 (threshold: 10 log10),
 *   general/gr_pwr_squelch_cc.cc:52-55 (update_state), gr_pwr_squelch_cc.h:52 (mute: y < threshold),
 *   general/gr_squelch_base_cc.cc:42-93 (general_work: the machine, the envelope, gating)
 * Detector: re * re + im * im in float (two rounded products, one rounded add), widened to double,
 * y = alpha * p + (1.0 - alpha) * y with two double products and one double add.  The machine runs
 * per sample after the detector and the output uses the state after it: MUTED and not mute ->
 * ATTACK (ramp 0: UNMUTED); UNMUTED and mute -> DECAY (ramp 0: MUTED); ATTACK: ++ramped, envelope
 * 0.5 - cos(M_PI * ramped / ramp) / 2.0, UNMUTED with envelope 1.0 once ramped >= ramp; DECAY:
 * --ramped, the same formula, MUTED at 0.  Not MUTED: in * gr_complex(envelope, 0.0), the envelope
 * narrowed to float and the whole complex product formed in float; MUTED: a zero, or with gating
 * nothing.  The envelope values come from a table made by the host's cos in double.
 * GRHIP_MODE_GENERIC: one lane per stream walks the detector in order.  Every other mode: the FAST
 * form, chunks of grhip_pwr_squelch_chunk() samples chained through the recurrence's affine form;
 * its y differs from the serial one by parts in 1e14, so the outputs are the same wherever the
 * detector stays that far from the threshold, and the machine, the envelope and
 * the products are the same code in both modes.
 * Deviations: set_ramp(0) while a stream is in ATTACK or DECAY is refused with GRHIP_ERANGE (the
 * reference divides by zero there and emits NaN); a stream that became UNMUTED without a ramp
 * (ramped == 0) and is given one later decays over the whole ramp (the reference counts down from
 * 0 and never ends that decay).
 * ====================================================================== */
typedef struct grhip_pwr_squelch_cc grhip_pwr_squelch_cc;
GRHIP_API int grhip_pwr_squelch_cc_create(grhip_pwr_squelch_cc **h, double db, double alpha, int ramp, int gate, int device);
GRHIP_API void grhip_pwr_squelch_cc_destroy(grhip_pwr_squelch_cc *h);
GRHIP_API int grhip_pwr_squelch_cc_set_mode(grhip_pwr_squelch_cc *h, int mode);
GRHIP_API int grhip_pwr_squelch_cc_set_streams(grhip_pwr_squelch_cc *h, int nstreams);
GRHIP_API double grhip_pwr_squelch_cc_threshold(grhip_pwr_squelch_cc *h);
GRHIP_API int grhip_pwr_squelch_cc_set_threshold(grhip_pwr_squelch_cc *h, double db);
GRHIP_API int grhip_pwr_squelch_cc_set_alpha(grhip_pwr_squelch_cc *h, double alpha);
GRHIP_API int grhip_pwr_squelch_cc_ramp(grhip_pwr_squelch_cc *h);
GRHIP_API int grhip_pwr_squelch_cc_set_ramp(grhip_pwr_squelch_cc *h, int ramp);
GRHIP_API int grhip_pwr_squelch_cc_gate(grhip_pwr_squelch_cc *h);
GRHIP_API int grhip_pwr_squelch_cc_set_gate(grhip_pwr_squelch_cc *h, int gate);
GRHIP_API int grhip_pwr_squelch_cc_unmuted(grhip_pwr_squelch_cc *h, int s);
GRHIP_API int grhip_pwr_squelch_cc_state(grhip_pwr_squelch_cc *h, int s, int *state, int *ramped, double *envelope, double *y);
GRHIP_API int grhip_pwr_squelch_cc_work(grhip_pwr_squelch_cc *h, int n_in, const void *in, void *out, int *produced);
GRHIP_API int grhip_pwr_squelch_cc_work_device(grhip_pwr_squelch_cc *h, int n_in, const void *d_in, void *d_out, int *d_produced,
                                     void *stream);

/* gr_pwr_squelch_ff
 *   replaces gr_make_pwr_squelch_ff(double db, double alpha = 0.0001, int ramp = 0, bool gate = false)
 *   general/gr_pwr_squelch_ff.{h,cc} (detector: x * x in float), general/gr_squelch_base_ff.cc:42-93
 * As pwr_squelch_cc on floats; the output is (float)((double)in * envelope), the product in double. */
typedef struct grhip_pwr_squelch_ff grhip_pwr_squelch_ff;
GRHIP_API int grhip_pwr_squelch_ff_create(grhip_pwr_squelch_ff **h, double db, double alpha, int ramp, int gate, int device);
GRHIP_API void grhip_pwr_squelch_ff_destroy(grhip_pwr_squelch_ff *h);
GRHIP_API int grhip_pwr_squelch_ff_set_mode(grhip_pwr_squelch_ff *h, int mode);
GRHIP_API int grhip_pwr_squelch_ff_set_streams(grhip_pwr_squelch_ff *h, int nstreams);
GRHIP_API double grhip_pwr_squelch_ff_threshold(grhip_pwr_squelch_ff *h);
GRHIP_API int grhip_pwr_squelch_ff_set_threshold(grhip_pwr_squelch_ff *h, double db);
GRHIP_API int grhip_pwr_squelch_ff_set_alpha(grhip_pwr_squelch_ff *h, double alpha);
GRHIP_API int grhip_pwr_squelch_ff_ramp(grhip_pwr_squelch_ff *h);
GRHIP_API int grhip_pwr_squelch_ff_set_ramp(grhip_pwr_squelch_ff *h, int ramp);
GRHIP_API int grhip_pwr_squelch_ff_gate(grhip_pwr_squelch_ff *h);
GRHIP_API int grhip_pwr_squelch_ff_set_gate(grhip_pwr_squelch_ff *h, int gate);
GRHIP_API int grhip_pwr_squelch_ff_unmuted(grhip_pwr_squelch_ff *h, int s);
GRHIP_API int grhip_pwr_squelch_ff_state(grhip_pwr_squelch_ff *h, int s, int *state, int *ramped, double *envelope, double *y);
GRHIP_API int grhip_pwr_squelch_ff_work(grhip_pwr_squelch_ff *h, int n_in, const void *in, void *out, int *produced);
GRHIP_API int grhip_pwr_squelch_ff_work_device(grhip_pwr_squelch_ff *h, int n_in, const void *d_in, void *d_out, int *d_produced,
                                     void *stream);

/* gr_simple_squelch_cc
 *   replaces gr_make_simple_squelch_cc(double threshold_db, double alpha = 0.0001)
 *   general/gr_simple_squelch_cc.cc:53-71 (work), :74-93 (set_threshold, threshold, set_alpha)
 * The same detector; out = (y >= threshold) ? in : 0, no ramp, no gating, produced[s] == n_in;
 * unmuted() is y_last >= threshold after the call. */
typedef struct grhip_simple_squelch_cc grhip_simple_squelch_cc;
GRHIP_API int grhip_simple_squelch_cc_create(grhip_simple_squelch_cc **h, double threshold_db, double alpha, int device);
GRHIP_API void grhip_simple_squelch_cc_destroy(grhip_simple_squelch_cc *h);
GRHIP_API int grhip_simple_squelch_cc_set_mode(grhip_simple_squelch_cc *h, int mode);
GRHIP_API int grhip_simple_squelch_cc_set_streams(grhip_simple_squelch_cc *h, int nstreams);
GRHIP_API double grhip_simple_squelch_cc_threshold(grhip_simple_squelch_cc *h);
GRHIP_API int grhip_simple_squelch_cc_set_threshold(grhip_simple_squelch_cc *h, double db);
GRHIP_API int grhip_simple_squelch_cc_set_alpha(grhip_simple_squelch_cc *h, double alpha);
GRHIP_API int grhip_simple_squelch_cc_unmuted(grhip_simple_squelch_cc *h, int s);
GRHIP_API int grhip_simple_squelch_cc_state(grhip_simple_squelch_cc *h, int s, int *state, int *ramped, double *envelope, double *y);
GRHIP_API int grhip_simple_squelch_cc_work(grhip_simple_squelch_cc *h, int n_in, const void *in, void *out, int *produced);
GRHIP_API int grhip_simple_squelch_cc_work_device(grhip_simple_squelch_cc *h, int n_in, const void *d_in, void *d_out, int *d_produced,
                                     void *stream);
/* samples per chunk of the FAST detector */
GRHIP_API int grhip_pwr_squelch_chunk(void);

/* ======================================================================
 * gr_ctcss_squelch_ff
 *   replaces gr_make_ctcss_squelch_ff(int rate, float freq, float level = 0.01, int len = 0,
 *       int ramp = 0, bool gate = false)
 *   general/gr_ctcss_squelch_ff.cc:53-85 (constructor: len == 0 is (int)(rate / 10.0); the guards are
 *   the adjacent tones of the 38 standard ones, found by an exact float compare, or freq * 0.98 /
 *   freq * 1.02, formed in double and stored to float, for a non-standard tone and on the outer side
 *   of the first and the last; d_mute starts true), :97-112 (update_state),
 *   filter/gri_goertzel.cc:36-75 (the filters), general/gr_squelch_base_ff.cc:42-93 (the machine)
 * Streams, buffers, produced[], the overlap rule, work / work_device, unmuted and the machine are
 * those of the power squelch blocks above.  The detector: three Goertzel filters (left guard,
 * tone, right guard) take every sample, y = (x + wr * d1) - d2 in float and unfused; after every
 * len samples their outputs ((0.5 * wr * d1 - d2) / len in double, (wi * d1) / len in float) give
 * |l|, |c|, |r| as (float)sqrt((double)re * re + (double)im * im), the filters are cleared and
 * d_mute = c < level || c < l || c < r (a NaN level never mutes); the sample that completes a block
 * already sees its decision and the decision holds until the next block ends.  Blocks run across
 * calls: a stream keeps the raw samples of its unfinished block (at most len - 1) and its last
 * decision on the device, and a block is evaluated whole, from a zero start, in the call that
 * completes it, so in each mode a stream's outputs depend on the concatenated input alone and never
 * on where the calls cut it.  After set_mode a block in progress is evaluated in the mode in force
 * when it completes.
 * GRHIP_MODE_GENERIC: the float recurrences in the reference's order, bit for bit.  Every other
 * mode: the closed form sum_n x[n] tab[n] against three tables built in double (goertzel_fc's FAST
 * form); its magnitudes differ from the recurrence's by what the float recurrence itself loses
 * (DESIGN.md 4.18), so the flags are the same wherever no comparison is that close to a tie.
 * state(): the machine's state, ramp position and envelope, d_mute, and the length of the
 * unfinished block.  tones(): the three frequencies.  last_magnitudes(): |l|, |c|, |r| of the
 * blocks of stream s that the last work call completed (3 floats each, cap_blocks of room);
 * returns their number; for tests.  set_streams restarts every stream (muted, d_mute true, nothing
 * carried); set_level, set_ramp, set_gate and set_mode keep everything and hold from the next call.
 * GRHIP_EINVAL: rate <= 0, a non-finite freq, len < 0, ramp < 0 (or past 2^24), S < 1, n_in < 0;
 * GRHIP_ERANGE: the effective len outside 1 .. 2^20, set_ramp(0) while a stream is in a ramp.
 * Deviations: finite samples only (hypotf special-cases the others); len is capped at 2^20; the
 * reference accepts len < 1 and then never decides; set_ramp(0) inside a ramp as above.
 * ====================================================================== */
typedef struct grhip_ctcss_squelch_ff grhip_ctcss_squelch_ff;
GRHIP_API int grhip_ctcss_squelch_ff_create(grhip_ctcss_squelch_ff **h, int rate, float freq, float level, int len, int ramp,
                                            int gate, int device);
GRHIP_API void grhip_ctcss_squelch_ff_destroy(grhip_ctcss_squelch_ff *h);
GRHIP_API int grhip_ctcss_squelch_ff_set_mode(grhip_ctcss_squelch_ff *h, int mode);
GRHIP_API int grhip_ctcss_squelch_ff_set_streams(grhip_ctcss_squelch_ff *h, int nstreams);
GRHIP_API float grhip_ctcss_squelch_ff_level(grhip_ctcss_squelch_ff *h);
GRHIP_API int grhip_ctcss_squelch_ff_set_level(grhip_ctcss_squelch_ff *h, float level);
GRHIP_API int grhip_ctcss_squelch_ff_len(grhip_ctcss_squelch_ff *h);
GRHIP_API int grhip_ctcss_squelch_ff_ramp(grhip_ctcss_squelch_ff *h);
GRHIP_API int grhip_ctcss_squelch_ff_set_ramp(grhip_ctcss_squelch_ff *h, int ramp);
GRHIP_API int grhip_ctcss_squelch_ff_gate(grhip_ctcss_squelch_ff *h);
GRHIP_API int grhip_ctcss_squelch_ff_set_gate(grhip_ctcss_squelch_ff *h, int gate);
GRHIP_API int grhip_ctcss_squelch_ff_squelch_range(float *range);
GRHIP_API int grhip_ctcss_squelch_ff_unmuted(grhip_ctcss_squelch_ff *h, int s);
GRHIP_API int grhip_ctcss_squelch_ff_state(grhip_ctcss_squelch_ff *h, int s, int *state, int *ramped, double *envelope, int *mute,
                                           int *pending);
GRHIP_API int grhip_ctcss_squelch_ff_tones(grhip_ctcss_squelch_ff *h, float *f_l, float *f_c, float *f_r);
GRHIP_API int grhip_ctcss_squelch_ff_last_magnitudes(grhip_ctcss_squelch_ff *h, int s, float *out, int cap_blocks);
GRHIP_API int grhip_ctcss_squelch_ff_work(grhip_ctcss_squelch_ff *h, int n_in, const void *in, void *out, int *produced);
GRHIP_API int grhip_ctcss_squelch_ff_work_device(grhip_ctcss_squelch_ff *h, int n_in, const void *d_in, void *d_out,
                                                 int *d_produced, void *stream);

/* ======================================================================
 * The gain loops.  A handle takes S streams back to back in `in` ([S][n_in], S = 1 after create);
 * stream s reads from in + s * n_in items and writes as many items from out + s * n_in (sync blocks,
 * history 1).  `out` may not overlap `in`.  work / work_device return GRHIP_OK; n_in == 0 is a
 * successful no-op; work_device (device buffers) does not synchronise.  Per stream the block
 * remembers its gain, one float on the device, across calls.  set_streams resizes that and sets
 * every stream's gain to the constructor's; set_gain sets every stream's gain (the reference's block
 * has one); gain(h, s, &g) reads one stream's and waits for the handle's queued work.  The other
 * setters act at once, as the reference's do: they hold from the next work call.  All state and
 * all parameters are float.  Nothing is refused at construction, the reference checks nothing; NaN
 * and infinities go through the arithmetic as they do there.
 * GRHIP_EINVAL: S < 1, n_in < 0, a null pointer, overlapping buffers.
 *
 * gr_agc_cc
 *   replaces gr_make_agc_cc(float rate = 1e-4, float reference = 1.0, float gain = 1.0,
 *       float max_gain = 0.0)
 *   general/gri_agc_cc.h:53-61 (scale), :43-51 (accessors), general/gr_agc_cc.cc:47-56 (work)
 * out = in * g (two rounded float products), then g += rate * (reference - sqrtf(re * re + im * im))
 * on the OUTPUT's parts, every product, the add and the square root rounded once, then
 * if (max_gain > 0 && g > max_gain) g = max_gain.
 * GRHIP_MODE_GENERIC: that recurrence in order, one wavefront per stream, bit for bit.  Every other
 * mode, for calls of more than grhip_agc_chunk() items: with g >= 0 a step is
 * g' = min(a g + b, M), a = 1 - rate |x|, b = rate reference, and such maps compose; the call is cut
 * into chunks of grhip_agc_chunk() items from its first item, every chunk's composed map is formed in
 * double and chained, and the reference's float steps then run again from every chunk's start gain
 * (rounded to float).  A chunk holding a sample with rate |x| > 1, an infinity or a NaN, and a chunk
 * entered with a negative gain, is walked sample by sample in the float arithmetic instead, so such
 * input costs time and never correctness.  The gain then deviates from the float64 recurrence by no
 * more than the serial float recurrence itself does; within that the result
 * depends on where the calls cut the input.  The serial walk runs whatever the mode for calls of at
 * most one chunk and where rate < 0, reference < 0 or rate, reference or max_gain is not finite.
 * ====================================================================== */
typedef struct grhip_agc_cc grhip_agc_cc;
GRHIP_API int grhip_agc_cc_create(grhip_agc_cc **h, float rate, float reference, float gain, float max_gain, int device);
GRHIP_API void grhip_agc_cc_destroy(grhip_agc_cc *h);
GRHIP_API int grhip_agc_cc_set_mode(grhip_agc_cc *h, int mode);
GRHIP_API int grhip_agc_cc_set_streams(grhip_agc_cc *h, int nstreams);
GRHIP_API float grhip_agc_cc_rate(grhip_agc_cc *h);
GRHIP_API float grhip_agc_cc_reference(grhip_agc_cc *h);
GRHIP_API float grhip_agc_cc_max_gain(grhip_agc_cc *h);
GRHIP_API int grhip_agc_cc_gain(grhip_agc_cc *h, int s, float *gain);
GRHIP_API int grhip_agc_cc_set_rate(grhip_agc_cc *h, float rate);
GRHIP_API int grhip_agc_cc_set_reference(grhip_agc_cc *h, float reference);
GRHIP_API int grhip_agc_cc_set_max_gain(grhip_agc_cc *h, float max_gain);
GRHIP_API int grhip_agc_cc_set_gain(grhip_agc_cc *h, float gain);
GRHIP_API int grhip_agc_cc_work(grhip_agc_cc *h, int n_in, const void *in, void *out);
GRHIP_API int grhip_agc_cc_work_device(grhip_agc_cc *h, int n_in, const void *d_in, void *d_out, void *stream);

/* gr_agc_ff
 *   replaces gr_make_agc_ff(float rate = 1e-4, float reference = 1.0, float gain = 1.0,
 *       float max_gain = 0.0)
 *   general/gri_agc_ff.h:51-57 (scale), general/gr_agc_ff.cc:45-54 (work)
 * As agc_cc on floats: g += (reference - fabsf(out)) * rate, the same clamp, the same two modes. */
typedef struct grhip_agc_ff grhip_agc_ff;
GRHIP_API int grhip_agc_ff_create(grhip_agc_ff **h, float rate, float reference, float gain, float max_gain, int device);
GRHIP_API void grhip_agc_ff_destroy(grhip_agc_ff *h);
GRHIP_API int grhip_agc_ff_set_mode(grhip_agc_ff *h, int mode);
GRHIP_API int grhip_agc_ff_set_streams(grhip_agc_ff *h, int nstreams);
GRHIP_API float grhip_agc_ff_rate(grhip_agc_ff *h);
GRHIP_API float grhip_agc_ff_reference(grhip_agc_ff *h);
GRHIP_API float grhip_agc_ff_max_gain(grhip_agc_ff *h);
GRHIP_API int grhip_agc_ff_gain(grhip_agc_ff *h, int s, float *gain);
GRHIP_API int grhip_agc_ff_set_rate(grhip_agc_ff *h, float rate);
GRHIP_API int grhip_agc_ff_set_reference(grhip_agc_ff *h, float reference);
GRHIP_API int grhip_agc_ff_set_max_gain(grhip_agc_ff *h, float max_gain);
GRHIP_API int grhip_agc_ff_set_gain(grhip_agc_ff *h, float gain);
GRHIP_API int grhip_agc_ff_work(grhip_agc_ff *h, int n_in, const void *in, void *out);
GRHIP_API int grhip_agc_ff_work_device(grhip_agc_ff *h, int n_in, const void *d_in, void *d_out, void *stream);

/* gr_agc2_cc
 *   replaces gr_make_agc2_cc(float attack_rate = 1e-1, float decay_rate = 1e-2,
 *       float reference = 1.0, float gain = 1.0, float max_gain = 0.0)
 *   general/gri_agc2_cc.h:54-76 (scale), general/gr_agc2_cc.cc:47-56 (work)
 * out = in * g; tmp = -reference + sqrtf(re * re + im * im) on the output; rate = (tmp > g) ?
 * attack_rate : decay_rate; g -= tmp * rate; if (g < 0) g = 10e-5; then the clamp of agc_cc.  The
 * rate switches on a comparison with the gain, so there is no composed form: every mode runs the
 * serial walk, one wavefront per stream, bit for bit the reference. */
typedef struct grhip_agc2_cc grhip_agc2_cc;
GRHIP_API int grhip_agc2_cc_create(grhip_agc2_cc **h, float attack_rate, float decay_rate, float reference, float gain,
                                   float max_gain, int device);
GRHIP_API void grhip_agc2_cc_destroy(grhip_agc2_cc *h);
GRHIP_API int grhip_agc2_cc_set_mode(grhip_agc2_cc *h, int mode);
GRHIP_API int grhip_agc2_cc_set_streams(grhip_agc2_cc *h, int nstreams);
GRHIP_API float grhip_agc2_cc_attack_rate(grhip_agc2_cc *h);
GRHIP_API float grhip_agc2_cc_decay_rate(grhip_agc2_cc *h);
GRHIP_API float grhip_agc2_cc_reference(grhip_agc2_cc *h);
GRHIP_API float grhip_agc2_cc_max_gain(grhip_agc2_cc *h);
GRHIP_API int grhip_agc2_cc_gain(grhip_agc2_cc *h, int s, float *gain);
GRHIP_API int grhip_agc2_cc_set_attack_rate(grhip_agc2_cc *h, float rate);
GRHIP_API int grhip_agc2_cc_set_decay_rate(grhip_agc2_cc *h, float rate);
GRHIP_API int grhip_agc2_cc_set_reference(grhip_agc2_cc *h, float reference);
GRHIP_API int grhip_agc2_cc_set_max_gain(grhip_agc2_cc *h, float max_gain);
GRHIP_API int grhip_agc2_cc_set_gain(grhip_agc2_cc *h, float gain);
GRHIP_API int grhip_agc2_cc_work(grhip_agc2_cc *h, int n_in, const void *in, void *out);
GRHIP_API int grhip_agc2_cc_work_device(grhip_agc2_cc *h, int n_in, const void *d_in, void *d_out, void *stream);

/* gr_agc2_ff
 *   replaces gr_make_agc2_ff(float attack_rate = 1e-1, float decay_rate = 1e-2,
 *       float reference = 1.0, float gain = 1.0, float max_gain = 0.0)
 *   general/gri_agc2_ff.h:55-75 (scale), general/gr_agc2_ff.cc:48-57 (work)
 * As agc2_cc on floats with tmp = fabsf(out) - reference and the rate test fabsf(tmp) > g (the
 * reference's two agc2 blocks differ in this test, and so do these). */
typedef struct grhip_agc2_ff grhip_agc2_ff;
GRHIP_API int grhip_agc2_ff_create(grhip_agc2_ff **h, float attack_rate, float decay_rate, float reference, float gain,
                                   float max_gain, int device);
GRHIP_API void grhip_agc2_ff_destroy(grhip_agc2_ff *h);
GRHIP_API int grhip_agc2_ff_set_mode(grhip_agc2_ff *h, int mode);
GRHIP_API int grhip_agc2_ff_set_streams(grhip_agc2_ff *h, int nstreams);
GRHIP_API float grhip_agc2_ff_attack_rate(grhip_agc2_ff *h);
GRHIP_API float grhip_agc2_ff_decay_rate(grhip_agc2_ff *h);
GRHIP_API float grhip_agc2_ff_reference(grhip_agc2_ff *h);
GRHIP_API float grhip_agc2_ff_max_gain(grhip_agc2_ff *h);
GRHIP_API int grhip_agc2_ff_gain(grhip_agc2_ff *h, int s, float *gain);
GRHIP_API int grhip_agc2_ff_set_attack_rate(grhip_agc2_ff *h, float rate);
GRHIP_API int grhip_agc2_ff_set_decay_rate(grhip_agc2_ff *h, float rate);
GRHIP_API int grhip_agc2_ff_set_reference(grhip_agc2_ff *h, float reference);
GRHIP_API int grhip_agc2_ff_set_max_gain(grhip_agc2_ff *h, float max_gain);
GRHIP_API int grhip_agc2_ff_set_gain(grhip_agc2_ff *h, float gain);
GRHIP_API int grhip_agc2_ff_work(grhip_agc2_ff *h, int n_in, const void *in, void *out);
GRHIP_API int grhip_agc2_ff_work_device(grhip_agc2_ff *h, int n_in, const void *d_in, void *d_out, void *stream);
/* items per chunk of the chunked form of agc_cc / agc_ff */
GRHIP_API int grhip_agc_chunk(void);

/* ======================================================================
 * The carrier loops: the four blocks built on gri_control_loop (general/gri_control_loop.{h,cc}).  A
 * handle takes S streams back to back as the gain loops do ([S][n_in], S = 1 after create; stream s
 * at s * n_in items of every buffer; buffers may not overlap; work / work_device return GRHIP_OK,
 * n_in == 0 is a successful no-op, work_device does not synchronise).  Per stream the device holds
 * d_phase and d_freq (and carrier tracking's d_locksig), all float, zero after create and after
 * set_streams, carried across calls.  Per sample every block forms an error from the sample and the
 * phase, then
 *     freq += beta * error;  phase = phase + freq + alpha * error          (advance_loop, :56-61)
 *     while (phase > 2 pi) phase -= 2 pi;  while (phase < -2 pi) phase += 2 pi  (phase_wrap, :64-71:
 *         the comparison against the double (2.0f*M_PI), the subtraction in double, narrowed)
 *     if (freq > max_freq) freq = max_freq; else if (freq < min_freq) freq = min_freq  (:73-80)
 * with every float operation rounded once.  One wavefront per stream walks this in order.
 * The setters are gri_control_loop's and act at once on every stream (they hold from the next work
 * call); where the reference throws std::out_of_range they return GRHIP_EINVAL and change nothing:
 *   set_loop_bandwidth   :86-95    bw < 0 is refused; damping stays, the gains are recomputed
 *   set_damping_factor   :97-106   outside [0, 1] is refused; the gains are recomputed
 *   set_alpha, set_beta  :108-124  outside [0, 1] is refused
 *   set_frequency        :126-135  freq > max_freq stores MIN_freq, freq < min_freq stores MAX_freq
 *   set_phase            :137-145  stored after the reference's wrap loops
 * The gains are :49-54: float denom = 1.0 + 2.0 * damping * bw + bw * bw (a double expression around
 * the float product bw * bw), alpha = (4 * damping * bw) / denom and beta = (4 * bw * bw) / denom in
 * float; damping starts as sqrtf(2.0f) / 2.0f (:38).  get_loop_bandwidth, get_damping_factor,
 * get_alpha and get_beta return the value (:153-175); get_frequency and get_phase (:177-187) read
 * one stream's and wait for the handle's queued work.
 * Deviations, all so that the walk ends for every argument (the reference's phase_wrap does not end
 * once phase - 2 pi rounds back to phase):
 *   * create refuses max_freq / min_freq that are not finite or above 1024 rad/sample in magnitude;
 *   * a bandwidth or damping factor whose gains come out not finite (bw = NaN, bw above 9e18) is
 *     refused, and so is a NaN alpha or beta, which passes the reference's comparisons;
 *   * set_phase refuses values that are not finite or above 2^20 in magnitude;
 *   * samples must be finite.  A NaN goes through the arithmetic; where the reference then reads
 *     outside its arctangent table, the device clamps the index.  The kernels terminate and stay in
 *     bounds for every bit pattern (csrc/carrier.hip states why).
 * GRHIP_EINVAL: the above, S < 1, n_in < 0, a null pointer, overlapping buffers.
 * set_mode: the three PLLs run one engine in every mode; costas_loop_cc see below.
 *
 * gr_pll_freqdet_cf
 *   replaces gr_make_pll_freqdet_cf(float loop_bw, float max_freq, float min_freq)
 *   general/gr_pll_freqdet_cf.cc:69-90 (work), :50-67 (mod_2pi, phase_detector)
 * Complex in, float out: out = d_freq BEFORE the sample's update (:81); error =
 * mod_2pi(gr_fast_atan2f(im, re) - phase), mod_2pi comparing against the double M_PI and adding
 * -+(2.0f*M_PI) in double.  Output and state are the reference's bit for bit in every mode.
 * ====================================================================== */
typedef struct grhip_pll_freqdet_cf grhip_pll_freqdet_cf;
GRHIP_API int grhip_pll_freqdet_cf_create(grhip_pll_freqdet_cf **h, float loop_bw, float max_freq, float min_freq, int device);
GRHIP_API void grhip_pll_freqdet_cf_destroy(grhip_pll_freqdet_cf *h);
GRHIP_API int grhip_pll_freqdet_cf_set_mode(grhip_pll_freqdet_cf *h, int mode);
GRHIP_API int grhip_pll_freqdet_cf_set_streams(grhip_pll_freqdet_cf *h, int nstreams);
GRHIP_API int grhip_pll_freqdet_cf_set_loop_bandwidth(grhip_pll_freqdet_cf *h, float bw);
GRHIP_API int grhip_pll_freqdet_cf_set_damping_factor(grhip_pll_freqdet_cf *h, float df);
GRHIP_API int grhip_pll_freqdet_cf_set_alpha(grhip_pll_freqdet_cf *h, float alpha);
GRHIP_API int grhip_pll_freqdet_cf_set_beta(grhip_pll_freqdet_cf *h, float beta);
GRHIP_API int grhip_pll_freqdet_cf_set_frequency(grhip_pll_freqdet_cf *h, float freq);
GRHIP_API int grhip_pll_freqdet_cf_set_phase(grhip_pll_freqdet_cf *h, float phase);
GRHIP_API float grhip_pll_freqdet_cf_get_loop_bandwidth(grhip_pll_freqdet_cf *h);
GRHIP_API float grhip_pll_freqdet_cf_get_damping_factor(grhip_pll_freqdet_cf *h);
GRHIP_API float grhip_pll_freqdet_cf_get_alpha(grhip_pll_freqdet_cf *h);
GRHIP_API float grhip_pll_freqdet_cf_get_beta(grhip_pll_freqdet_cf *h);
GRHIP_API int grhip_pll_freqdet_cf_get_frequency(grhip_pll_freqdet_cf *h, int s, float *freq);
GRHIP_API int grhip_pll_freqdet_cf_get_phase(grhip_pll_freqdet_cf *h, int s, float *phase);
GRHIP_API int grhip_pll_freqdet_cf_work(grhip_pll_freqdet_cf *h, int n_in, const void *in, void *out);
GRHIP_API int grhip_pll_freqdet_cf_work_device(grhip_pll_freqdet_cf *h, int n_in, const void *d_in, void *d_out, void *stream);

/* gr_pll_refout_cc
 *   replaces gr_make_pll_refout_cc(float loop_bw, float max_freq, float min_freq)
 *   general/gr_pll_refout_cc.cc:70-93 (work)
 * Complex in, complex out: out = (cos, sin) of the phase BEFORE the update (:83-84), the same error
 * and loop.  The state is the reference's bit for bit.  Sine and cosine are (float)sin((double)phase)
 * and (float)cos((double)phase) where the reference calls sincosf: within one float ulp of it. */
typedef struct grhip_pll_refout_cc grhip_pll_refout_cc;
GRHIP_API int grhip_pll_refout_cc_create(grhip_pll_refout_cc **h, float loop_bw, float max_freq, float min_freq, int device);
GRHIP_API void grhip_pll_refout_cc_destroy(grhip_pll_refout_cc *h);
GRHIP_API int grhip_pll_refout_cc_set_mode(grhip_pll_refout_cc *h, int mode);
GRHIP_API int grhip_pll_refout_cc_set_streams(grhip_pll_refout_cc *h, int nstreams);
GRHIP_API int grhip_pll_refout_cc_set_loop_bandwidth(grhip_pll_refout_cc *h, float bw);
GRHIP_API int grhip_pll_refout_cc_set_damping_factor(grhip_pll_refout_cc *h, float df);
GRHIP_API int grhip_pll_refout_cc_set_alpha(grhip_pll_refout_cc *h, float alpha);
GRHIP_API int grhip_pll_refout_cc_set_beta(grhip_pll_refout_cc *h, float beta);
GRHIP_API int grhip_pll_refout_cc_set_frequency(grhip_pll_refout_cc *h, float freq);
GRHIP_API int grhip_pll_refout_cc_set_phase(grhip_pll_refout_cc *h, float phase);
GRHIP_API float grhip_pll_refout_cc_get_loop_bandwidth(grhip_pll_refout_cc *h);
GRHIP_API float grhip_pll_refout_cc_get_damping_factor(grhip_pll_refout_cc *h);
GRHIP_API float grhip_pll_refout_cc_get_alpha(grhip_pll_refout_cc *h);
GRHIP_API float grhip_pll_refout_cc_get_beta(grhip_pll_refout_cc *h);
GRHIP_API int grhip_pll_refout_cc_get_frequency(grhip_pll_refout_cc *h, int s, float *freq);
GRHIP_API int grhip_pll_refout_cc_get_phase(grhip_pll_refout_cc *h, int s, float *phase);
GRHIP_API int grhip_pll_refout_cc_work(grhip_pll_refout_cc *h, int n_in, const void *in, void *out);
GRHIP_API int grhip_pll_refout_cc_work_device(grhip_pll_refout_cc *h, int n_in, const void *d_in, void *d_out, void *stream);

/* gr_pll_carriertracking_cc
 *   replaces gr_make_pll_carriertracking_cc(float loop_bw, float max_freq, float min_freq)
 *   general/gr_pll_carriertracking_cc.cc:92-120 (work), :74-90 (lock_detector, squelch_enable,
 *   set_lock_threshold)
 * Complex in, complex out: out = in * (cos, -sin) of the phase before the update (:104-105), the same
 * error and loop (state bit for bit), then locksig = locksig * (1.0 - alpha) + alpha * (re * cos +
 * im * sin) in the reference's float/double mix (:113-114).  With the squelch enabled, output n is
 * zero unless fabsf(locksig) > threshold AFTER sample n's update (:116-117).  Sine and cosine as in
 * pll_refout_cc, so outputs and lock signal follow the reference to a few ulps, not
 * bit for bit.  locksig(h, s, &v) and lock_detector(h, s, &locked) read one stream's; squelch_enable
 * and set_lock_threshold (both start as 0) act on every stream. */
typedef struct grhip_pll_carriertracking_cc grhip_pll_carriertracking_cc;
GRHIP_API int grhip_pll_carriertracking_cc_create(grhip_pll_carriertracking_cc **h, float loop_bw, float max_freq, float min_freq, int device);
GRHIP_API void grhip_pll_carriertracking_cc_destroy(grhip_pll_carriertracking_cc *h);
GRHIP_API int grhip_pll_carriertracking_cc_set_mode(grhip_pll_carriertracking_cc *h, int mode);
GRHIP_API int grhip_pll_carriertracking_cc_set_streams(grhip_pll_carriertracking_cc *h, int nstreams);
GRHIP_API int grhip_pll_carriertracking_cc_set_loop_bandwidth(grhip_pll_carriertracking_cc *h, float bw);
GRHIP_API int grhip_pll_carriertracking_cc_set_damping_factor(grhip_pll_carriertracking_cc *h, float df);
GRHIP_API int grhip_pll_carriertracking_cc_set_alpha(grhip_pll_carriertracking_cc *h, float alpha);
GRHIP_API int grhip_pll_carriertracking_cc_set_beta(grhip_pll_carriertracking_cc *h, float beta);
GRHIP_API int grhip_pll_carriertracking_cc_set_frequency(grhip_pll_carriertracking_cc *h, float freq);
GRHIP_API int grhip_pll_carriertracking_cc_set_phase(grhip_pll_carriertracking_cc *h, float phase);
GRHIP_API float grhip_pll_carriertracking_cc_get_loop_bandwidth(grhip_pll_carriertracking_cc *h);
GRHIP_API float grhip_pll_carriertracking_cc_get_damping_factor(grhip_pll_carriertracking_cc *h);
GRHIP_API float grhip_pll_carriertracking_cc_get_alpha(grhip_pll_carriertracking_cc *h);
GRHIP_API float grhip_pll_carriertracking_cc_get_beta(grhip_pll_carriertracking_cc *h);
GRHIP_API int grhip_pll_carriertracking_cc_get_frequency(grhip_pll_carriertracking_cc *h, int s, float *freq);
GRHIP_API int grhip_pll_carriertracking_cc_get_phase(grhip_pll_carriertracking_cc *h, int s, float *phase);
GRHIP_API int grhip_pll_carriertracking_cc_work(grhip_pll_carriertracking_cc *h, int n_in, const void *in, void *out);
GRHIP_API int grhip_pll_carriertracking_cc_work_device(grhip_pll_carriertracking_cc *h, int n_in, const void *d_in, void *d_out, void *stream);
GRHIP_API int grhip_pll_carriertracking_cc_locksig(grhip_pll_carriertracking_cc *h, int s, float *locksig);
GRHIP_API int grhip_pll_carriertracking_cc_lock_detector(grhip_pll_carriertracking_cc *h, int s, int *locked);
GRHIP_API int grhip_pll_carriertracking_cc_squelch_enable(grhip_pll_carriertracking_cc *h, int enable);
GRHIP_API int grhip_pll_carriertracking_cc_set_lock_threshold(grhip_pll_carriertracking_cc *h, float threshold);

/* digital_costas_loop_cc
 *   replaces digital_make_costas_loop_cc(float loop_bw, int order)
 *   gr-digital/lib/digital_costas_loop_cc.cc:110-153 (work), :69-108 (the detectors), :41-67
 * Complex in, complex out and, optionally, float out.  Per sample: nco = gr_expj(-phase); out = in *
 * nco (four products, a difference and a sum); error = the detector of `order` on out (order 2:
 * re * im in float; orders 4 and 8 in double, narrowed once, K = (float)(sqrt(2.0) - 1));
 * error = gr_branchless_clip(error, 1.0); then the loop above with max_freq = 1.0 and min_freq =
 * -1.0 (:46).  freq_out, where given, is d_freq AFTER the update (:137); out is the same with and
 * without it.  An order other than 2, 4 or 8 is refused with GRHIP_EINVAL (the reference throws
 * std::invalid_argument).
 * The NCO sits inside the loop, so the result depends on the sine and cosine to the bit, and the
 * reference's sincosf is not reproduced.  GRHIP_MODE_GENERIC: sine and cosine are
 * (float)sin((double)-phase) and (float)cos((double)-phase), everything else as the reference writes
 * it.  Every other mode: a float polynomial NCO (absolute error below 2e-7) off the double pipe.  In
 * both the phase stays as close to the float64 recurrence as the reference's own does, and outputs
 * are within 1e-5 of the input's peak of that recurrence's.
 * work: freq_out NULL or n_in floats per stream. */
typedef struct grhip_costas_loop_cc grhip_costas_loop_cc;
GRHIP_API int grhip_costas_loop_cc_create(grhip_costas_loop_cc **h, float loop_bw, int order, int device);
GRHIP_API void grhip_costas_loop_cc_destroy(grhip_costas_loop_cc *h);
GRHIP_API int grhip_costas_loop_cc_set_mode(grhip_costas_loop_cc *h, int mode);
GRHIP_API int grhip_costas_loop_cc_set_streams(grhip_costas_loop_cc *h, int nstreams);
GRHIP_API int grhip_costas_loop_cc_set_loop_bandwidth(grhip_costas_loop_cc *h, float bw);
GRHIP_API int grhip_costas_loop_cc_set_damping_factor(grhip_costas_loop_cc *h, float df);
GRHIP_API int grhip_costas_loop_cc_set_alpha(grhip_costas_loop_cc *h, float alpha);
GRHIP_API int grhip_costas_loop_cc_set_beta(grhip_costas_loop_cc *h, float beta);
GRHIP_API int grhip_costas_loop_cc_set_frequency(grhip_costas_loop_cc *h, float freq);
GRHIP_API int grhip_costas_loop_cc_set_phase(grhip_costas_loop_cc *h, float phase);
GRHIP_API float grhip_costas_loop_cc_get_loop_bandwidth(grhip_costas_loop_cc *h);
GRHIP_API float grhip_costas_loop_cc_get_damping_factor(grhip_costas_loop_cc *h);
GRHIP_API float grhip_costas_loop_cc_get_alpha(grhip_costas_loop_cc *h);
GRHIP_API float grhip_costas_loop_cc_get_beta(grhip_costas_loop_cc *h);
GRHIP_API int grhip_costas_loop_cc_get_frequency(grhip_costas_loop_cc *h, int s, float *freq);
GRHIP_API int grhip_costas_loop_cc_get_phase(grhip_costas_loop_cc *h, int s, float *phase);
GRHIP_API int grhip_costas_loop_cc_work(grhip_costas_loop_cc *h, int n_in, const void *in, void *out, void *freq_out);
GRHIP_API int grhip_costas_loop_cc_work_device(grhip_costas_loop_cc *h, int n_in, const void *d_in, void *d_out, void *d_freq_out,
                                               void *stream);

/* digital_fll_band_edge_cc
 *   replaces digital_make_fll_band_edge_cc(float samps_per_sym, float rolloff, int filter_size,
 *       float bandwidth)
 *   gr-digital/lib/digital_fll_band_edge_cc.cc:208-259 (work), :148-188 (design_filter), :53-120
 * Complex in; complex out and, optionally, three float outputs.  The loop above with max_freq =
 * (float)(2 pi * (2.0 / sps)) and min_freq = -max_freq (:58).
 *
 * What is computed.  The reference's work (history = filter_size + 1) writes out[i + fs - 1] = in[i] *
 * gr_expj(d_phase), fs - 1 items beyond noutput_items, filters out[i .. i + fs - 1] and returns
 * noutput_items; in the runtime's double-mapped ring the items written ahead are the first items of
 * the next call, so what a reader sees is a linear stream.  That stream is the contract here, with
 * fs = filter_size:
 *     xz   = fs zeros, then the input
 *     d[j] = xz[j] * expj(phase before step j)          (ac - bd, ad + bc)
 *     step j filters d[j-fs+1 .. j], tap k on d[j-fs+1+k], zeros before the start:
 *         error = norm(sum lower[k] d) - norm(sum upper[k] d);  advance_loop, phase_wrap, frequency_limit
 *     out[n] = d[n - (fs - 1)]: the input delayed by 2 fs - 1 items, the first 2 fs - 1 outputs zero
 *     frq[n], phs[n], err[n] = d_freq, d_phase, error after step n
 * The handle works on new items only (as am_demod_cf and fm_demod_cf do): per stream the device holds
 * the last fs inputs, the last fs - 1 derotated samples, phase and frequency, zero after create and
 * after set_streams.  THE RESULT DEPENDS ON THE CONCATENATED INPUT ALONE, never on where calls cut it.
 * The reference agrees with this as long as its reader keeps up; when its downstream ring is full it
 * overwrites unread items instead, which nothing here does.
 *
 * The filters.  grhip_fll_band_edge_taps(sps, rolloff, filter_size, lower, upper) is design_filter
 * (host only, no device needed) and writes filter_size (re, im) float pairs to each of lower and upper,
 * stored reversed as the reference stores them: float k = -M + i*2.0/sps with M = rint(size / sps), the
 * two sincs (a double sine narrowed to float), the float running sum `power`, N = (size - 1.0)/2.0
 * truncated, gr_expj of the double argument -+2 pi (1 + rolloff) k narrowed to float (sincosf on the
 * host, as a Linux build of the reference calls it).  Bit for bit the reference's taps.
 * GRHIP_EINVAL where the reference throws std::out_of_range (sps <= 0, rolloff outside [0, 1],
 * filter_size <= 0) and, stated deviations: filter_size above 1024; taps that are not finite (the
 * baseband taps sum to 0, so tap / power is not a number); an sps whose 2 pi 2 / sps exceeds the
 * family's 1024 rad/sample (or is not finite).
 *
 * The setters of the loop are the family's (above).  set_samples_per_symbol, set_rolloff and
 * set_filter_size (:92-120) redesign the filters and wait for the device; a refused value changes
 * nothing.  set_samples_per_symbol leaves max_freq / min_freq as they are, as the reference does.
 * set_filter_size zeroes the two per-stream histories, phase and frequency stay: a stated deviation
 * (the reference leaves its ring as it is and returns 0 items once); the other two keep the histories.
 *
 * phase_wrap, a stated deviation: the error is a difference of two filter powers and unbounded, unlike
 * every other loop of the family, and the reference's subtract loop does not end for a large phase.
 * The kernel runs that loop for at most 256 trips each way and beyond that takes the exact double
 * remainder fmod(phase, 2 pi), narrowed to float.  Only input of a scale where (alpha + beta) |error|
 * passes about 570 reaches it.  The kernel ends and stays in bounds for every bit pattern
 * (csrc/fll_band_edge.hip states why).
 *
 * GRHIP_MODE_GENERIC: sine and cosine are (float)sin((double)phase) and (float)cos((double)phase);
 * every product and sum is rounded once, as g++ forms complex<float> arithmetic without contraction,
 * and the two filter sums run in the reference's order k = 0 .. fs - 1.  Bit for bit the restatement
 * in tests/fll_ref.py; not the reference's sincosf to the bit.  Every other mode: the
 * float polynomial NCO of costas_loop_cc, fused multiply-adds and tree-order sums.
 * work / work_device: frq, phs and err are n_in floats per stream each, all given or all NULL
 * (GRHIP_EINVAL otherwise); out is the same either way.  No buffer may overlap another. */
typedef struct grhip_fll_band_edge_cc grhip_fll_band_edge_cc;
GRHIP_API int grhip_fll_band_edge_taps(float sps, float rolloff, int filter_size, void *lower, void *upper);
GRHIP_API int grhip_fll_band_edge_cc_create(grhip_fll_band_edge_cc **h, float samps_per_sym, float rolloff, int filter_size,
                                            float bandwidth, int device);
GRHIP_API void grhip_fll_band_edge_cc_destroy(grhip_fll_band_edge_cc *h);
GRHIP_API int grhip_fll_band_edge_cc_set_mode(grhip_fll_band_edge_cc *h, int mode);
GRHIP_API int grhip_fll_band_edge_cc_set_streams(grhip_fll_band_edge_cc *h, int nstreams);
GRHIP_API int grhip_fll_band_edge_cc_set_loop_bandwidth(grhip_fll_band_edge_cc *h, float bw);
GRHIP_API int grhip_fll_band_edge_cc_set_damping_factor(grhip_fll_band_edge_cc *h, float df);
GRHIP_API int grhip_fll_band_edge_cc_set_alpha(grhip_fll_band_edge_cc *h, float alpha);
GRHIP_API int grhip_fll_band_edge_cc_set_beta(grhip_fll_band_edge_cc *h, float beta);
GRHIP_API int grhip_fll_band_edge_cc_set_frequency(grhip_fll_band_edge_cc *h, float freq);
GRHIP_API int grhip_fll_band_edge_cc_set_phase(grhip_fll_band_edge_cc *h, float phase);
GRHIP_API float grhip_fll_band_edge_cc_get_loop_bandwidth(grhip_fll_band_edge_cc *h);
GRHIP_API float grhip_fll_band_edge_cc_get_damping_factor(grhip_fll_band_edge_cc *h);
GRHIP_API float grhip_fll_band_edge_cc_get_alpha(grhip_fll_band_edge_cc *h);
GRHIP_API float grhip_fll_band_edge_cc_get_beta(grhip_fll_band_edge_cc *h);
GRHIP_API int grhip_fll_band_edge_cc_get_frequency(grhip_fll_band_edge_cc *h, int s, float *freq);
GRHIP_API int grhip_fll_band_edge_cc_get_phase(grhip_fll_band_edge_cc *h, int s, float *phase);
GRHIP_API int grhip_fll_band_edge_cc_set_samples_per_symbol(grhip_fll_band_edge_cc *h, float sps);
GRHIP_API int grhip_fll_band_edge_cc_set_rolloff(grhip_fll_band_edge_cc *h, float rolloff);
GRHIP_API int grhip_fll_band_edge_cc_set_filter_size(grhip_fll_band_edge_cc *h, int filter_size);
GRHIP_API float grhip_fll_band_edge_cc_get_samples_per_symbol(grhip_fll_band_edge_cc *h);
GRHIP_API float grhip_fll_band_edge_cc_get_rolloff(grhip_fll_band_edge_cc *h);
GRHIP_API int grhip_fll_band_edge_cc_get_filter_size(grhip_fll_band_edge_cc *h);
GRHIP_API int grhip_fll_band_edge_cc_work(grhip_fll_band_edge_cc *h, int n_in, const void *in, void *out, void *frq, void *phs,
                                          void *err);
GRHIP_API int grhip_fll_band_edge_cc_work_device(grhip_fll_band_edge_cc *h, int n_in, const void *d_in, void *d_out, void *d_frq,
                                                 void *d_phs, void *d_err, void *stream);

/* gr_pfb_clock_sync_ccf
 *   replaces gr_make_pfb_clock_sync_ccf(double sps, float loop_bw, const std::vector<float> &taps,
 *       unsigned int filter_size, float init_phase, float max_rate_deviation, int osps)
 *   gnuradio-core/src/lib/filter/gr_pfb_clock_sync_ccf.cc:351-427 (general_work), :208-274 (set_taps,
 *   create_diff_taps), :200-205 (update_gains); filter/gr_fir_XXX_generic.cc.t:59-79; general/gr_math.h:63-69
 * Complex in; complex out and, optionally, three float outputs.  Polyphase timing recovery: the
 * prototype taps are split into nfilters = filter_size arms of tpf = ceil(ntaps / nfilters) taps (arm f's
 * tap j is taps[f + j nfilters], zeros beyond the prototype), a second bank is built from the
 * differentiated prototype, and per symbol the loop takes osps outputs of arm floor(k) and one output of
 * the derivative arm, forms error = (out.im diff.im + out.re diff.re) / 2 and steps rate_f += beta error,
 * k += alpha error.  A wrap of k over [0, nfilters) is a step of one item in the input: a carry.
 *
 * The stream.  With isps = (int)floor(sps), xz is tpf + isps - 1 zeros followed by the input: the
 * reference's set_history(tpf + sps) as a reader of a linear stream sees it.  pos is an absolute index
 * into xz and starts at 0.  An evaluation at pos reads xz[pos .. pos + tpf - 1]; tap j of arm f
 * multiplies xz[pos + tpf - 1 - j] (gr_fir_ccf stores its taps reversed).
 *
 * One symbol, literally :379-423.  lo = max(pos - isps + 1, 0).  For kk = 0 .. osps - 1:
 *     filtnum = (int)floor(k); the two wrap loops, each trip k -+= nfilters (float), pos +-= 1;
 *     out[i + kk] = arm filtnum at pos + kk;   k = (k + rate_i) + rate_f
 * then diff = derivative arm filtnum (the last one) at pos, error from out[i] (the first of the osps
 * outputs), the step, rate_f = gr_branchless_clip(rate_f, max_dev), pos += isps.  Every float operation
 * is rounded once and nothing is contracted; `/ 2.0` and `0.5 *` are done in double and narrowed;
 * update_gains keeps its mix: float denom = 1.0 + 2.0 damping bw + (float)(bw bw) from a double
 * expression, alpha = (4 damping bw) / denom and beta = (4 bw bw) / denom in float.
 *
 * Cuts.  The handle takes NEW ITEMS ONLY, S streams back to back, as fll_band_edge_cc does.  Per stream
 * the device keeps k, rate_f, error, pos, the slips and the last need + isps items of xz, where
 * need = osps PCS_CARRY + osps + tpf and PCS_CARRY = 8.  A symbol starts once pos + need items of xz
 * have arrived: then every item it may read is there, whatever it turns out to carry, and no symbol is
 * rolled back.  THE OUTPUT DEPENDS ON THE CONCATENATED INPUT ALONE, never on where the calls cut it.  The
 * reference's `ninput - tpf - osps` and `noutput_items - osps` tests are other forms of the same
 * rule and are not reproduced (its input test allows for no carry, so at the end of a stream it gives a few
 * symbols more from the same items; a later call gives them here); its "return 0 once after
 * set_taps" (d_updated) is not reproduced either.
 *
 * Three stated deviations keep the walk finite and the history bounded; each event is counted per
 * stream in slips(s), which is 0 on every signal of a sane scale:
 *   backward: after its wraps an evaluation may not stand before lo, one item behind the position at
 *       which the symbol before took its derivative arm; it is put at lo.  So a symbol moves that
 *       position on by at least one item and produced <= osps (n_in + isps).  (The reference there
 *       reads in front of its window, and a net negative consume_each fails an assertion in gr_buffer.)
 *   forward: at most PCS_CARRY forward carries move pos per evaluation; k is still wrapped fully.
 *   the wrap loops run for at most 64 trips together and only for |k| < 2^29; beyond that k becomes
 *       the exact double remainder fmod(k, nfilters) (made non-negative) and the carries it stands for
 *       are cut as above.  A k that is not finite becomes 0, with a slip counted.
 * The kernel ends and stays in bounds for every bit pattern of the input (csrc/pfb_clock_sync.hip
 * states why).
 *
 * Refused with GRHIP_EINVAL where the reference throws (loop_bw < 0; set_damping_factor, set_alpha,
 * set_beta outside [0, 1]) and, stated deviations: ntaps < 2 (create_diff_taps indexes with size() - 2,
 * unsigned); filter_size < 1 or above 256; more than 256 taps per arm or 4096 taps in a padded bank;
 * sps < 1 or >= 256; osps < 1 or above 8; any argument, tap or derivative tap that is not finite;
 * gains that are not finite.  A refused setter changes nothing.  The setters act on the next symbol.
 * set_taps after construction is not offered; pfb_clock_sync_fff (an older loop in this reference, with
 * the arms assigned in reverse) is not built.
 *
 * grhip_pfb_clock_sync_taps(taps, ntaps, nfilters, bank, diff_bank, &tpf) needs no device: *tpf always,
 * and nfilters * tpf floats to each of bank and diff_bank that is not NULL, arm by arm, as get_taps()
 * and get_diff_taps() return them.  create_diff_taps is reproduced literally: its pwr gathers fabsf of
 * the partial sums inside the j loop, and the derivative taps are multiplied by it.
 *
 * Outputs.  out holds out_cap complex items per stream, stream s at out + s * out_cap; err, rate and k
 * (all three given or all NULL) hold out_cap floats per stream each.  produced[s] (S ints) tells the
 * items written; for work_device it is on the device and the entry does not synchronise (the squelch
 * blocks' convention).  grhip_pfb_clock_sync_ccf_max_produced(h, n_in) = osps (n_in + isps) tells an
 * out_cap that always suffices; a smaller one is GRHIP_EINVAL, and so is one above 2^31 - 1.  Slot i
 * of a symbol holds what the reference writes there: d_error and d_rate_f from before the step, d_k
 * after the last phase advance;
 * the osps - 1 slots behind it get the same values (the reference leaves them unwritten: a stated
 * deviation).  n_in may be 0.  No buffer may overlap another.
 *
 * GRHIP_MODE_GENERIC: the arm sums run in gr_fir_ccf_generic's order (two complex accumulators over the
 * even and the odd taps, the tail of an odd count into the first, acc0 + acc1), each product and sum
 * rounded once: bit for bit the restatement in tests/pfb_clock_sync_ref.py and through it the
 * reference (tests/golden/ref_pfb_clock_sync.npz).  Every other mode: the same scalar loop arithmetic,
 * the dot products in fused multiply-adds and tree order.
 * get_clock_rate, k, error, slips and position read stream s's state (they wait for the device). */
typedef struct grhip_pfb_clock_sync_ccf grhip_pfb_clock_sync_ccf;
GRHIP_API int grhip_pfb_clock_sync_taps(const float *taps, int ntaps, int nfilters, float *bank, float *diff_bank, int *tpf);
GRHIP_API int grhip_pfb_clock_sync_ccf_create(grhip_pfb_clock_sync_ccf **h, double sps, float loop_bw, const float *taps, int ntaps,
                                              int filter_size, float init_phase, float max_rate_deviation, int osps, int device);
GRHIP_API void grhip_pfb_clock_sync_ccf_destroy(grhip_pfb_clock_sync_ccf *h);
GRHIP_API int grhip_pfb_clock_sync_ccf_set_mode(grhip_pfb_clock_sync_ccf *h, int mode);
GRHIP_API int grhip_pfb_clock_sync_ccf_set_streams(grhip_pfb_clock_sync_ccf *h, int nstreams);
GRHIP_API int grhip_pfb_clock_sync_ccf_set_loop_bandwidth(grhip_pfb_clock_sync_ccf *h, float bw);
GRHIP_API int grhip_pfb_clock_sync_ccf_set_damping_factor(grhip_pfb_clock_sync_ccf *h, float df);
GRHIP_API int grhip_pfb_clock_sync_ccf_set_alpha(grhip_pfb_clock_sync_ccf *h, float alpha);
GRHIP_API int grhip_pfb_clock_sync_ccf_set_beta(grhip_pfb_clock_sync_ccf *h, float beta);
GRHIP_API int grhip_pfb_clock_sync_ccf_set_max_rate_deviation(grhip_pfb_clock_sync_ccf *h, float max_rate_deviation);
GRHIP_API float grhip_pfb_clock_sync_ccf_get_loop_bandwidth(grhip_pfb_clock_sync_ccf *h);
GRHIP_API float grhip_pfb_clock_sync_ccf_get_damping_factor(grhip_pfb_clock_sync_ccf *h);
GRHIP_API float grhip_pfb_clock_sync_ccf_get_alpha(grhip_pfb_clock_sync_ccf *h);
GRHIP_API float grhip_pfb_clock_sync_ccf_get_beta(grhip_pfb_clock_sync_ccf *h);
GRHIP_API float grhip_pfb_clock_sync_ccf_get_max_rate_deviation(grhip_pfb_clock_sync_ccf *h);
GRHIP_API int grhip_pfb_clock_sync_ccf_get_clock_rate(grhip_pfb_clock_sync_ccf *h, int s, float *rate);
GRHIP_API int grhip_pfb_clock_sync_ccf_k(grhip_pfb_clock_sync_ccf *h, int s, float *k);
GRHIP_API int grhip_pfb_clock_sync_ccf_error(grhip_pfb_clock_sync_ccf *h, int s, float *error);
GRHIP_API int grhip_pfb_clock_sync_ccf_slips(grhip_pfb_clock_sync_ccf *h, int s, int *slips);
GRHIP_API int grhip_pfb_clock_sync_ccf_position(grhip_pfb_clock_sync_ccf *h, int s, long long *pos);
GRHIP_API int grhip_pfb_clock_sync_ccf_get_taps(grhip_pfb_clock_sync_ccf *h, float *bank, size_t cap, int *nfilters, int *tpf);
GRHIP_API int grhip_pfb_clock_sync_ccf_get_diff_taps(grhip_pfb_clock_sync_ccf *h, float *bank, size_t cap, int *nfilters, int *tpf);
GRHIP_API int grhip_pfb_clock_sync_ccf_max_produced(grhip_pfb_clock_sync_ccf *h, int n_in);
GRHIP_API int grhip_pfb_clock_sync_ccf_work(grhip_pfb_clock_sync_ccf *h, int n_in, const void *in, long long out_cap, void *out, void *err,
                                            void *rate, void *k, int *produced);
GRHIP_API int grhip_pfb_clock_sync_ccf_work_device(grhip_pfb_clock_sync_ccf *h, int n_in, const void *d_in, long long out_cap, void *d_out,
                                                   void *d_err, void *d_rate, void *d_k, int *d_produced, void *stream);

/* ======================================================================
 * digital_constellation and its kinds (host objects; no device is needed)
 *   replaces digital_make_constellation_bpsk / _qpsk / _dqpsk / _8psk (), digital_make_constellation_calcdist
 *       (constellation, pre_diff_code, rotational_symmetry, dimensionality), digital_make_constellation_psk
 *       (constellation, pre_diff_code, n_sectors), digital_make_constellation_rect (constellation, pre_diff_code,
 *       rotational_symmetry, real_sectors, imag_sectors, width_real_sectors, width_imag_sectors)
 *   gr-digital/lib/digital_constellation.cc, gr-digital/include/digital_constellation.h
 * Points travel as npoints (re, im) float pairs; a pre_diff_code of length 0 means none
 * (apply_pre_diff_code() is then 0; constellation_qpsk has a code and does not apply it, as in the
 * reference).  bpsk, qpsk, dqpsk and 8psk decide by the reference's closed forms; calcdist by
 * get_closest_point (float norms, the first strict minimum); psk and rect through a sector table
 * (get_sector, calc_sector_value).  decision_maker takes `dimensionality` samples and gives the
 * symbol; decision_maker_pe also gives 0 + sum_d -arg(sample[d] * conj(points[index + d])), the
 * complex product as g++ forms it without -ffast-math (C99 Annex G recovery included).  Both run on
 * the host.  bits_per_symbol is floor(log(npoints) / dimensionality / log(2.0)).
 * Refused with GRHIP_EINVAL (the reference throws std::runtime_error): a pre_diff_code whose length is
 * neither 0 nor npoints; npoints that is no multiple of the dimensionality.
 * Deviations: at most 256 symbols (a symbol is a byte at the blocks' outputs) and at least one; at most
 * 16384 sectors and at least one; rect's widths finite and not zero, its points finite; a sample
 * that is not finite gets a defined sector (a NaN position is sector 0, every index is clamped to the
 * table; the reference converts such a double to int, which is undefined); arg, cos and sin of a float
 * are the float-rounded double functions, within an ulp of glibc's atan2f / cosf / sinf but the same
 * on host, device and in the tests.  Dimensionality above 1 exists for calcdist only; the receiver
 * refuses it, the decoder takes it.
 * points / pre_diff_code / sector_values copy at most `capacity` entries and return how many there are. */
typedef struct grhip_constellation grhip_constellation;
GRHIP_API int grhip_constellation_create_bpsk(grhip_constellation **h);
GRHIP_API int grhip_constellation_create_qpsk(grhip_constellation **h);
GRHIP_API int grhip_constellation_create_dqpsk(grhip_constellation **h);
GRHIP_API int grhip_constellation_create_8psk(grhip_constellation **h);
GRHIP_API int grhip_constellation_create_calcdist(grhip_constellation **h, const float *points_re_im, size_t npoints, const unsigned *pre_diff_code,
                                                  size_t ncode, unsigned rotational_symmetry, unsigned dimensionality);
GRHIP_API int grhip_constellation_create_psk(grhip_constellation **h, const float *points_re_im, size_t npoints, const unsigned *pre_diff_code,
                                             size_t ncode, unsigned n_sectors);
GRHIP_API int grhip_constellation_create_rect(grhip_constellation **h, const float *points_re_im, size_t npoints, const unsigned *pre_diff_code,
                                              size_t ncode, unsigned rotational_symmetry, unsigned real_sectors, unsigned imag_sectors,
                                              float width_real_sectors, float width_imag_sectors);
GRHIP_API void grhip_constellation_destroy(grhip_constellation *h);
GRHIP_API int grhip_constellation_arity(const grhip_constellation *h);
GRHIP_API int grhip_constellation_dimensionality(const grhip_constellation *h);
GRHIP_API int grhip_constellation_rotational_symmetry(const grhip_constellation *h);
GRHIP_API int grhip_constellation_bits_per_symbol(const grhip_constellation *h);
GRHIP_API int grhip_constellation_apply_pre_diff_code(const grhip_constellation *h);
GRHIP_API int grhip_constellation_n_sectors(const grhip_constellation *h);
GRHIP_API int grhip_constellation_points(const grhip_constellation *h, float *points_re_im, size_t capacity);
GRHIP_API int grhip_constellation_pre_diff_code(const grhip_constellation *h, unsigned *code, size_t capacity);
GRHIP_API int grhip_constellation_sector_values(const grhip_constellation *h, unsigned *values, size_t capacity);
GRHIP_API int grhip_constellation_decision_maker(const grhip_constellation *h, const float *sample_re_im, unsigned *index);
GRHIP_API int grhip_constellation_decision_maker_pe(const grhip_constellation *h, const float *sample_re_im, unsigned *index, float *phase_error);

/* digital_constellation_decoder_cb, gr_diff_decoder_bb, gr_map_bb
 *   replace digital_make_constellation_decoder_cb (constellation), gr_make_diff_decoder_bb (modulus),
 *       gr_make_map_bb (map)
 *   gr-digital/lib/digital_constellation_decoder_cb.cc:63-78, general/gr_diff_decoder_bb.cc:48-61,
 *   general/gr_map_bb.cc:36-60
 * Handles take S streams back to back as the carrier loops do; `out` may not overlap `in` (map_bb may
 * run in place); n == 0 is a successful no-op; work_device does not synchronise.  A block copies its
 * constellation, which may be destroyed before the block.
 * constellation_decoder_cb: n outputs from n * dimensionality complex items per stream, byte for byte
 * the host's decision_maker in every mode.
 * diff_decoder_bb: out[i] = (unsigned)((int)in[i] - (int)in[i-1]) % modulus, so a negative difference
 * wraps at 2^32 before the % (what the reference computes for a modulus that is no power of two); the
 * byte in front of a call's first is the stream's last of the call before, 0 after create and
 * set_streams.  modulus 0 is refused (the reference divides by it).
 * map_bb: a 256-entry table, the identity behind the nmap entries given; at most 256 are taken, each
 * narrowed to a byte. */
typedef struct grhip_constellation_decoder_cb grhip_constellation_decoder_cb;
GRHIP_API int grhip_constellation_decoder_cb_create(grhip_constellation_decoder_cb **h, const grhip_constellation *constellation, int device);
GRHIP_API void grhip_constellation_decoder_cb_destroy(grhip_constellation_decoder_cb *h);
GRHIP_API int grhip_constellation_decoder_cb_set_mode(grhip_constellation_decoder_cb *h, int mode);
GRHIP_API int grhip_constellation_decoder_cb_set_streams(grhip_constellation_decoder_cb *h, int nstreams);
GRHIP_API int grhip_constellation_decoder_cb_work(grhip_constellation_decoder_cb *h, int n, const void *in, void *out);
GRHIP_API int grhip_constellation_decoder_cb_work_device(grhip_constellation_decoder_cb *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_diff_decoder_bb grhip_diff_decoder_bb;
GRHIP_API int grhip_diff_decoder_bb_create(grhip_diff_decoder_bb **h, unsigned modulus, int device);
GRHIP_API void grhip_diff_decoder_bb_destroy(grhip_diff_decoder_bb *h);
GRHIP_API int grhip_diff_decoder_bb_set_mode(grhip_diff_decoder_bb *h, int mode);
GRHIP_API int grhip_diff_decoder_bb_set_streams(grhip_diff_decoder_bb *h, int nstreams);
GRHIP_API int grhip_diff_decoder_bb_work(grhip_diff_decoder_bb *h, int n, const void *in, void *out);
GRHIP_API int grhip_diff_decoder_bb_work_device(grhip_diff_decoder_bb *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_map_bb grhip_map_bb;
GRHIP_API int grhip_map_bb_create(grhip_map_bb **h, const int *map, size_t nmap, int device);
GRHIP_API void grhip_map_bb_destroy(grhip_map_bb *h);
GRHIP_API int grhip_map_bb_set_mode(grhip_map_bb *h, int mode);
GRHIP_API int grhip_map_bb_set_streams(grhip_map_bb *h, int nstreams);
GRHIP_API int grhip_map_bb_work(grhip_map_bb *h, int n, const void *in, void *out);
GRHIP_API int grhip_map_bb_work_device(grhip_map_bb *h, int n, const void *d_in, void *d_out, void *stream);

/* digital_constellation_receiver_cb
 *   replaces digital_make_constellation_receiver_cb (constellation, loop_bw, fmin, fmax)
 *   gr-digital/lib/digital_constellation_receiver_cb.cc:80-122
 * Complex in; a symbol byte out and, all three or none, the phase error, the loop's phase and its
 * frequency as floats, the last two AFTER the update (:113-115).  Per sample: nco = gr_expj(+phase);
 * sample = nco * in; (symbol, error) = decision_maker_pe(sample); then gri_control_loop's advance_loop,
 * phase_wrap, frequency_limit with max_freq = fmax, min_freq = fmin.  The loop's setters, getters and
 * refusals are those of the carrier loops above.  A constellation of dimensionality above 1 is refused
 * (the reference throws std::runtime_error), as is a call with one or two of the three float outputs.
 * The decision sits inside the loop, so the result depends on sine, cosine and arctangent to the bit, and
 * glibc's are not reproduced.  GRHIP_MODE_GENERIC: the reference's statements in order
 * with the float-rounded double functions.  Every other mode, by the constellation's kind (form()
 * says which: 0 GENERIC, 1 cartesian, 2 angle): bpsk, qpsk, dqpsk, 8psk and psk run on the sample's angle
 * (theta = atan2f(im, re) off the serial chain; t = wrap(theta + phase); the decision from t; error =
 * -wrap(t - angle of the decided point)); rect and calcdist keep the chain with a float polynomial
 * NCO, rect's sector from one multiply-add per axis and atan2f.  In every mode the phase stays as close
 * to the float64 recurrence as the reference's own does, and the symbols are the reference's wherever no
 * derotated sample lies within 1e-3 of its magnitude of a decision border. */
typedef struct grhip_constellation_receiver_cb grhip_constellation_receiver_cb;
GRHIP_API int grhip_constellation_receiver_cb_create(grhip_constellation_receiver_cb **h, const grhip_constellation *constellation, float loop_bw,
                                                     float fmin, float fmax, int device);
GRHIP_API void grhip_constellation_receiver_cb_destroy(grhip_constellation_receiver_cb *h);
GRHIP_API int grhip_constellation_receiver_cb_set_mode(grhip_constellation_receiver_cb *h, int mode);
GRHIP_API int grhip_constellation_receiver_cb_set_streams(grhip_constellation_receiver_cb *h, int nstreams);
GRHIP_API int grhip_constellation_receiver_cb_form(grhip_constellation_receiver_cb *h);
GRHIP_API int grhip_constellation_receiver_cb_set_loop_bandwidth(grhip_constellation_receiver_cb *h, float bw);
GRHIP_API int grhip_constellation_receiver_cb_set_damping_factor(grhip_constellation_receiver_cb *h, float df);
GRHIP_API int grhip_constellation_receiver_cb_set_alpha(grhip_constellation_receiver_cb *h, float alpha);
GRHIP_API int grhip_constellation_receiver_cb_set_beta(grhip_constellation_receiver_cb *h, float beta);
GRHIP_API int grhip_constellation_receiver_cb_set_frequency(grhip_constellation_receiver_cb *h, float freq);
GRHIP_API int grhip_constellation_receiver_cb_set_phase(grhip_constellation_receiver_cb *h, float phase);
GRHIP_API float grhip_constellation_receiver_cb_get_loop_bandwidth(grhip_constellation_receiver_cb *h);
GRHIP_API float grhip_constellation_receiver_cb_get_damping_factor(grhip_constellation_receiver_cb *h);
GRHIP_API float grhip_constellation_receiver_cb_get_alpha(grhip_constellation_receiver_cb *h);
GRHIP_API float grhip_constellation_receiver_cb_get_beta(grhip_constellation_receiver_cb *h);
GRHIP_API int grhip_constellation_receiver_cb_get_frequency(grhip_constellation_receiver_cb *h, int s, float *freq);
GRHIP_API int grhip_constellation_receiver_cb_get_phase(grhip_constellation_receiver_cb *h, int s, float *phase);
GRHIP_API int grhip_constellation_receiver_cb_work(grhip_constellation_receiver_cb *h, int n_in, const void *in, void *symbols, void *error,
                                                   void *phase, void *freq);
GRHIP_API int grhip_constellation_receiver_cb_work_device(grhip_constellation_receiver_cb *h, int n_in, const void *d_in, void *d_symbols,
                                                          void *d_error, void *d_phase, void *d_freq, void *stream);

/* constellation_demod_cb: generic_demod behind timing recovery as one handle
 *   gr-digital/python/generic_mod_demod.py:296-313
 * constellation_receiver_cb -> diff_decoder_bb(arity) if differential -> map_bb(invert_code(pre_diff_code))
 * if gray_coded and the constellation applies a pre-diff code -> unpack_k_bits_bb(bits_per_symbol).
 * n complex items in, n * bits_per_symbol bytes out per stream (one bit each, most significant first).
 * engine 1 (the default) stores the bits from the receiver's walk; engine 0 runs the library's own
 * blocks in a row inside the handle; both give the same bytes and keep the same state, so the engine
 * may change between calls.  A constellation of fewer than 2 points has no bits and is refused. */
typedef struct grhip_constellation_demod_cb grhip_constellation_demod_cb;
GRHIP_API int grhip_constellation_demod_cb_create(grhip_constellation_demod_cb **h, const grhip_constellation *constellation, float loop_bw,
                                                  float fmin, float fmax, int differential, int gray_coded, int device);
GRHIP_API void grhip_constellation_demod_cb_destroy(grhip_constellation_demod_cb *h);
GRHIP_API int grhip_constellation_demod_cb_set_mode(grhip_constellation_demod_cb *h, int mode);
GRHIP_API int grhip_constellation_demod_cb_set_streams(grhip_constellation_demod_cb *h, int nstreams);
GRHIP_API int grhip_constellation_demod_cb_form(grhip_constellation_demod_cb *h);
GRHIP_API int grhip_constellation_demod_cb_set_loop_bandwidth(grhip_constellation_demod_cb *h, float bw);
GRHIP_API int grhip_constellation_demod_cb_set_damping_factor(grhip_constellation_demod_cb *h, float df);
GRHIP_API int grhip_constellation_demod_cb_set_alpha(grhip_constellation_demod_cb *h, float alpha);
GRHIP_API int grhip_constellation_demod_cb_set_beta(grhip_constellation_demod_cb *h, float beta);
GRHIP_API int grhip_constellation_demod_cb_set_frequency(grhip_constellation_demod_cb *h, float freq);
GRHIP_API int grhip_constellation_demod_cb_set_phase(grhip_constellation_demod_cb *h, float phase);
GRHIP_API float grhip_constellation_demod_cb_get_loop_bandwidth(grhip_constellation_demod_cb *h);
GRHIP_API float grhip_constellation_demod_cb_get_damping_factor(grhip_constellation_demod_cb *h);
GRHIP_API float grhip_constellation_demod_cb_get_alpha(grhip_constellation_demod_cb *h);
GRHIP_API float grhip_constellation_demod_cb_get_beta(grhip_constellation_demod_cb *h);
GRHIP_API int grhip_constellation_demod_cb_get_frequency(grhip_constellation_demod_cb *h, int s, float *freq);
GRHIP_API int grhip_constellation_demod_cb_get_phase(grhip_constellation_demod_cb *h, int s, float *phase);
GRHIP_API int grhip_constellation_demod_cb_set_engine(grhip_constellation_demod_cb *h, int engine);
GRHIP_API int grhip_constellation_demod_cb_engine(grhip_constellation_demod_cb *h);
GRHIP_API int grhip_constellation_demod_cb_bits_per_symbol(grhip_constellation_demod_cb *h);
GRHIP_API int grhip_constellation_demod_cb_work(grhip_constellation_demod_cb *h, int n_in, const void *in, void *bits);
GRHIP_API int grhip_constellation_demod_cb_work_device(grhip_constellation_demod_cb *h, int n_in, const void *d_in, void *d_bits, void *stream);

/* ======================================================================
 * The blocks in front of the pulse shaper of generic_mod (gr-digital/python/generic_mod_demod.py:114-150):
 * gr_packed_to_unpacked_bb, gr_unpacked_to_packed_bb, gr_diff_encoder_bb, gr_chunks_to_symbols_bc
 *   replace gr_make_packed_to_unpacked_bb (bits_per_chunk, endianness), gr_make_unpacked_to_packed_bb (same),
 *       gr_make_diff_encoder_bb (modulus), gr_make_chunks_to_symbols_bc (symbol_table, D)
 *   gengen/gr_packed_to_unpacked_XX.cc.t:58-137, gengen/gr_unpacked_to_packed_XX.cc.t:56-129,
 *   general/gr_diff_encoder_bb.cc:44-62, gengen/gr_chunks_to_symbols_XX.cc.t:51-74
 * Handles take S streams back to back as diff_decoder_bb and map_bb do (S = 1 after create); set_mode is
 * accepted and every mode gives the same bytes (the arithmetic is integer, the symbols are copied); an
 * output that overlaps its input is refused; n == 0 (noutput_items == 0) is a successful no-op; the device
 * entries do not synchronise.
 *
 * packed_to_unpacked_bb: output chunk i is the bits_per_chunk bits from bit address d_index + i * k of
 * the input bytes, the first bit the chunk's most significant.  GRHIP_MSB_FIRST counts a byte's bits from
 * the top, GRHIP_LSB_FIRST from the bottom; the reference shifts left for both (x = (x << 1) | bit,
 * .cc.t:109 and :119), so an LSB_FIRST chunk is the byte's bits in reverse order.  A gr_block:
 * forecast(n) = ceil((d_index + n * k) / 8) (.cc.t:62); general_work reads in [S][ninput_items], writes
 * out [S][noutput_items], returns noutput_items and sets *consumed = d_index >> 3, keeping d_index & 7:
 * one value for all streams, as in the reference, 0 after create and set_streams.  The counts do not
 * depend on the data, so the device entry has them on return.  Refused: bits_per_chunk outside 1 .. 8
 * and an endianness that is neither (the reference asserts); ninput_items below forecast (the reference
 * only asserts, .cc.t:129); a call whose last bit address passes 2^32, where the reference's unsigned
 * index wraps (noutput_items * k < 2^32 - 8).
 * unpacked_to_packed_bb: the inverse.  Output byte i is the 8 bits from bit address d_index + i * 8 of
 * the chunks' bits_per_chunk low bits laid end to end, most significant first (get_bit_be1, .cc.t:66-73);
 * MSB_FIRST shifts them in from the right, LSB_FIRST builds the byte from the top down (:112), so the
 * first bit ends as bit 0.  forecast(n) = ceil((d_index + 8 n) / k) (.cc.t:59), *consumed =
 * d_index / k, d_index % k is kept (it counts bits within an input chunk).  Refusals as above, the
 * address limit being noutput_items * 8 < 2^32 - 8.
 * diff_encoder_bb: out[i] = (in[i] + last_out) % modulus in unsigned, stored as a byte, last_out = the
 * byte (.cc:55-58); last_out is kept per stream, 0 after create and set_streams.  Moduli up to 256 are a
 * prefix sum modulo the modulus whether or not the inputs lie below it, moduli above 510 (where
 * in + last_out <= 510 is never reduced and the byte store alone wraps) one modulo 256: both run as a
 * scan -- per-tile sums, a carry pass seeded with last_out, the tile again from its carry -- and give
 * the serial loop's bytes.  For 257 .. 510 the byte store between two steps breaks associativity, and
 * those moduli walk serially, one lane per stream.  Modulus 0 is refused (the reference divides by it).
 * chunks_to_symbols_bc: n input bytes per stream give n * D complex items, table[in * D .. in * D + D)
 * (.cc.t:65-69).  Deviation: an index whose D entries do not lie inside the table gives zeros; the
 * reference asserts (:66) or, built without assertions, reads outside its vector.  Refused: an empty
 * table, more than 65536 entries, D < 1, n * D above INT_MAX (the reference's noutput_items).
 * ====================================================================== */
#define GRHIP_MSB_FIRST 0 /* GR_MSB_FIRST, gengen/gr_endianness.h:25 */
#define GRHIP_LSB_FIRST 1 /* GR_LSB_FIRST */
typedef struct grhip_packed_to_unpacked_bb grhip_packed_to_unpacked_bb;
GRHIP_API int grhip_packed_to_unpacked_bb_create(grhip_packed_to_unpacked_bb **h, unsigned bits_per_chunk, int endianness, int device);
GRHIP_API void grhip_packed_to_unpacked_bb_destroy(grhip_packed_to_unpacked_bb *h);
GRHIP_API int grhip_packed_to_unpacked_bb_set_mode(grhip_packed_to_unpacked_bb *h, int mode);
GRHIP_API int grhip_packed_to_unpacked_bb_set_streams(grhip_packed_to_unpacked_bb *h, int nstreams);
GRHIP_API int grhip_packed_to_unpacked_bb_forecast(grhip_packed_to_unpacked_bb *h, int noutput_items);
GRHIP_API int grhip_packed_to_unpacked_bb_general_work(grhip_packed_to_unpacked_bb *h, int noutput_items, int ninput_items,
                                                       const void *in, void *out, int *consumed);
GRHIP_API int grhip_packed_to_unpacked_bb_general_work_device(grhip_packed_to_unpacked_bb *h, int noutput_items, int ninput_items,
                                                              const void *d_in, void *d_out, int *consumed, void *stream);
typedef struct grhip_unpacked_to_packed_bb grhip_unpacked_to_packed_bb;
GRHIP_API int grhip_unpacked_to_packed_bb_create(grhip_unpacked_to_packed_bb **h, unsigned bits_per_chunk, int endianness, int device);
GRHIP_API void grhip_unpacked_to_packed_bb_destroy(grhip_unpacked_to_packed_bb *h);
GRHIP_API int grhip_unpacked_to_packed_bb_set_mode(grhip_unpacked_to_packed_bb *h, int mode);
GRHIP_API int grhip_unpacked_to_packed_bb_set_streams(grhip_unpacked_to_packed_bb *h, int nstreams);
GRHIP_API int grhip_unpacked_to_packed_bb_forecast(grhip_unpacked_to_packed_bb *h, int noutput_items);
GRHIP_API int grhip_unpacked_to_packed_bb_general_work(grhip_unpacked_to_packed_bb *h, int noutput_items, int ninput_items,
                                                       const void *in, void *out, int *consumed);
GRHIP_API int grhip_unpacked_to_packed_bb_general_work_device(grhip_unpacked_to_packed_bb *h, int noutput_items, int ninput_items,
                                                              const void *d_in, void *d_out, int *consumed, void *stream);
typedef struct grhip_diff_encoder_bb grhip_diff_encoder_bb;
GRHIP_API int grhip_diff_encoder_bb_create(grhip_diff_encoder_bb **h, unsigned modulus, int device);
GRHIP_API void grhip_diff_encoder_bb_destroy(grhip_diff_encoder_bb *h);
GRHIP_API int grhip_diff_encoder_bb_set_mode(grhip_diff_encoder_bb *h, int mode);
GRHIP_API int grhip_diff_encoder_bb_set_streams(grhip_diff_encoder_bb *h, int nstreams);
GRHIP_API int grhip_diff_encoder_bb_work(grhip_diff_encoder_bb *h, int n, const void *in, void *out);
GRHIP_API int grhip_diff_encoder_bb_work_device(grhip_diff_encoder_bb *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_chunks_to_symbols_bc grhip_chunks_to_symbols_bc;
GRHIP_API int grhip_chunks_to_symbols_bc_create(grhip_chunks_to_symbols_bc **h, const float *symbol_table_re_im, size_t nsymbols, int D,
                                                int device);
GRHIP_API void grhip_chunks_to_symbols_bc_destroy(grhip_chunks_to_symbols_bc *h);
GRHIP_API int grhip_chunks_to_symbols_bc_set_mode(grhip_chunks_to_symbols_bc *h, int mode);
GRHIP_API int grhip_chunks_to_symbols_bc_set_streams(grhip_chunks_to_symbols_bc *h, int nstreams);
GRHIP_API int grhip_chunks_to_symbols_bc_D(grhip_chunks_to_symbols_bc *h);
GRHIP_API int grhip_chunks_to_symbols_bc_work(grhip_chunks_to_symbols_bc *h, int n, const void *in, void *out);
GRHIP_API int grhip_chunks_to_symbols_bc_work_device(grhip_chunks_to_symbols_bc *h, int n, const void *d_in, void *d_out, void *stream);

/* generic_mod: the digital modulator as one handle
 *   replaces digital.generic_mod (constellation, samples_per_symbol, differential, excess_bw, gray_coded)
 *   gr-digital/python/generic_mod_demod.py:76-157
 * packed_to_unpacked_bb(bits_per_symbol, MSB_FIRST) -> map_bb(pre_diff_code) if gray_coded ->
 * diff_encoder_bb(2^bits_per_symbol) if differential -> chunks_to_symbols_bc(points) ->
 * pfb_arb_resampler_ccf(samples_per_symbol, root_raised_cosine(32, 32, 1.0, excess_bw,
 * 32 * 11 * int(samples_per_symbol)), 32)   (:114-150).  firdes makes the tap count odd: ntaps() is one more,
 * and a filter has 11 * int(samples_per_symbol) + 1 taps.  samples_per_symbol and excess_bw are doubles, as the
 * Python floats of the reference are: the taps are designed from the double excess_bw, the resampler's rate is
 * samples_per_symbol narrowed to float (gr_make_pfb_arb_resampler_ccf takes a float).
 * The modulator does not ask apply_pre_diff_code() (:123-124): an empty code is the identity, and
 * constellation_qpsk's code IS applied here although constellation_demod_cb / generic_demod skip it.  The
 * asymmetry is the reference's.
 * Refused: samples_per_symbol below 2 (the reference raises, :114-115) or not finite; int(samples_per_symbol)
 * above 11, the handle's limit (with 32 arms the resampler's tap banks leave LDS at 12); a constellation of
 * dimensionality above 1, of fewer than 2 points or of more than 8 bits per symbol; an excess_bw that leaves no
 * finite taps.
 * The handle takes NEW BYTES ONLY, S streams back to back ([S][n_bytes]).  Between calls it keeps, per stream, the
 * unread bits of the last byte, the encoder's last_out and the last taps-per-filter symbols, and for all
 * streams the bit index and the resampler's (j, acc).  So the output depends on the concatenated input alone,
 * never on where the calls cut it: a chunk that straddles two calls (3 or 6 bits per symbol) comes with the
 * call that completes it, and output m comes with the call that brings symbol count_m (the rule of
 * pfb_arb_resampler_ccf_run_captures_device, "count_k < n_samples"; the scheduler's history zeros in front of
 * the stream are complex zeros, not point 0).  The reference's first general_work that returns 0 (d_updated)
 * is a scheduler artefact without effect on the stream and is not reproduced.
 * *produced, the items per stream, is known on return (the schedule does not depend on the data) and is the
 * same for every stream; max_produced(n_bytes) is that number for the NEXT call of n_bytes, from the handle's
 * current state.  An out_capacity (items per stream) below it is refused before anything is written or
 * carried.  work: out is [S][*produced] back to back.  work_device: stream s at d_out + s * out_stride_items;
 * it does not synchronise.  n_bytes == 0 is a successful no-op.  The output may not overlap the input.
 * engine 0 runs the library's own five blocks in a row inside the handle and is the yardstick.  engine 1 (the
 * default) is one fused kernel behind a carry pre-pass (csrc/modulator_fused.hip): k/8 bytes in and
 * 8 * samples_per_symbol bytes out per symbol.  Both keep the same state, so the engine may change between
 * calls.  GRHIP_MODE_GENERIC: gr_fir_ccf_generic's order and the unfused o0 + o1 * acc, engine 1 equal to
 * engine 0 and to the reference bit for bit.  Every other mode: the blended tap h + acc * dh and FMAs, as
 * pfb_arb_resampler_ccf. */
typedef struct grhip_generic_mod grhip_generic_mod;
GRHIP_API int grhip_generic_mod_create(grhip_generic_mod **h, const grhip_constellation *constellation, double samples_per_symbol,
                                       int differential, double excess_bw, int gray_coded, int device);
GRHIP_API void grhip_generic_mod_destroy(grhip_generic_mod *h);
GRHIP_API int grhip_generic_mod_set_mode(grhip_generic_mod *h, int mode);
GRHIP_API int grhip_generic_mod_set_streams(grhip_generic_mod *h, int nstreams);
GRHIP_API int grhip_generic_mod_set_engine(grhip_generic_mod *h, int engine);
GRHIP_API int grhip_generic_mod_engine(grhip_generic_mod *h);
GRHIP_API int grhip_generic_mod_bits_per_symbol(grhip_generic_mod *h);
GRHIP_API double grhip_generic_mod_samples_per_symbol(grhip_generic_mod *h);
GRHIP_API int grhip_generic_mod_ntaps(grhip_generic_mod *h);
GRHIP_API int grhip_generic_mod_taps(grhip_generic_mod *h, float *taps, size_t capacity);
GRHIP_API long long grhip_generic_mod_max_produced(grhip_generic_mod *h, int n_bytes);
GRHIP_API int grhip_generic_mod_work(grhip_generic_mod *h, int n_bytes, const void *in, void *out, long long out_capacity,
                                     long long *produced);
GRHIP_API int grhip_generic_mod_work_device(grhip_generic_mod *h, int n_bytes, const void *d_in, void *d_out, long long out_stride_items,
                                            long long out_capacity, long long *produced, void *stream);

/* ======================================================================
 * The packet layer: CRC-32, make_packet / unmake_packet in batches, the whitening table
 *   replace digital_crc32 / digital_update_crc32          gr-digital/lib/digital_crc32.cc:45-134
 *           packet_utils.make_packet, unmake_packet        gr-digital/python/packet_utils.py:89-194
 *           crc.gen_and_append_crc32, crc.check_crc32      gr-digital/python/crc.py:26-38
 *           packet_utils.random_mask_tuple                 gr-digital/python/packet_utils.py:198-454
 * as gr-digital/python/pkt.py:78-100 (transmit) and :143-167 (receive) use them.  The Reed-Solomon code of
 * digital_crc32.cc:142-883 is not built.
 *
 * CRC-32: polynomial 0x04C11DB7, most significant bit first, no reflection; compute is
 * update(0xFFFFFFFF, buf, len) ^ 0xFFFFFFFF (.cc:133), update the bare loop of .cc:115-120.  len is 0 ..
 * 2^31 - 1; a buffer may start at any byte.  The device entries queue on `stream`, wait for it and store the
 * CRC in the host word *crc; the host-buffer entries stage the bytes to the device (there is no CPU path).
 * Every lane takes bytes of its own from a raw CRC of 0 and multiplies the result by x^(8 * bytes behind it)
 * modulo the generator; the start value enters as crc * x^(8 len).  set_segment_bytes is a tuning and test
 * knob: the bytes one workgroup takes in a row, rounded up to 16 KiB passes (0: chosen per call); results do
 * not depend on it.
 *
 * grhip_whitening_table writes the 4096 bytes of random_mask_tuple.  They are generated, not stored: bytes
 * 0 .. 4093 are next_bit() of gri_lfsr(0x3, 0x3FFF, 14), eight to a byte, least significant bit first, and the
 * last two are 255, 63.
 *
 * packet_maker: make_packet for n payloads in one call.  create takes the access code as '0' / '1'
 * characters, 1 .. 64 of them (more is refused, a deviation: correlate_access_code_bb takes 64; anything else
 * in the string is refused as :121-122 raises), samples_per_symbol (int() of it is used, :146),
 * bits_per_symbol, pad_for_usrp and whitening.  packet_bytes(payload_len) is the length of one packet;
 * plan fills n 16-byte job records, payloads and packets back to back, and the two totals (either may be
 * NULL; whitener_offsets NULL: 0 each); work_device, one wavefront per packet, writes the preamble A4 F2, the
 * packed access code (leading zeros up to a whole byte), the header '!HH' of
 * ((o & 0xf) << 12) | (L & 0x0fff) twice, the payload and its CRC-32 big-endian XORed with the mask from
 * offset o, one 0x55, and with pad_for_usrp _npadding_bytes more (:151-172, Python 2's integer
 * arithmetic).  As in the reference L = len + 4 <= 4096, L = 4096 puts 0 into the header, and the mask is read
 * from the full o.  Refused: o < 0 (:124 only means to), L + o > 4096 (numpy raises), a byte modulus of 0.
 * work_device takes the records from device memory, as plan wrote them or with out_offset moved; a record
 * whose length or whitener_offset breaks these limits is skipped on the device: nothing is written for it.
 * work is the same for host buffers; out_capacity below the total is refused before anything runs.
 *
 * packet_check: unmake_packet for messages that lie on the device.  Message m of stream s is
 * d_recs[s * rec_stride + m] (grhip_packet_rec, the layout framer_sink_1_batch keeps), its bytes at
 * d_pool + s * pool_stride + offset; stream s has d_counts[s * count_stride_words] messages (d_counts NULL:
 * max_msgs each).  One wavefront per message dewhitens (if dewhitening) into d_payload_out at the same
 * stride and offset -- d_payload_out may be d_pool -- and compares the CRC of all but the last 4 bytes with
 * those 4, big-endian: d_ok[s * max_msgs + m] is 1 or 0; the payload is the first length - 4 bytes.  0 too
 * for length < 4 (crc.py:31-32, (False, '')), for length + whitener_offset > 4096 (deviation: the
 * reference's watcher thread dies on numpy's exception) and for m at or above the stream's count; nothing is
 * written for those.  No synchronisation.
 *
 * grhip_framer_sink_1_batch_device_view: where the batch framer keeps its records, counts and pool on the
 * device, in the terms of packet_check's arguments.  Addresses and strides are fixed at create; what they hold
 * is the last run_device's, once its stream has come that far, until the next run.  Read-only.  The
 * single-stream framer has no such view: its buffers move when they grow.
 * ====================================================================== */
typedef struct grhip_packet_job { unsigned whitener_offset, length, in_offset, out_offset; } grhip_packet_job;
typedef struct grhip_packet_rec { unsigned whitener_offset, length, offset, reserved; } grhip_packet_rec;
GRHIP_API int grhip_whitening_table(unsigned char *table, size_t capacity);
typedef struct grhip_crc32 grhip_crc32;
GRHIP_API int grhip_crc32_create(grhip_crc32 **h, int device);
GRHIP_API void grhip_crc32_destroy(grhip_crc32 *h);
GRHIP_API int grhip_crc32_set_segment_bytes(grhip_crc32 *h, long long bytes);
GRHIP_API int grhip_crc32_compute_device(grhip_crc32 *h, const void *d_buf, long long len, unsigned *crc, void *stream);
GRHIP_API int grhip_crc32_update_device(grhip_crc32 *h, unsigned crc_in, const void *d_buf, long long len, unsigned *crc, void *stream);
GRHIP_API int grhip_crc32_compute(grhip_crc32 *h, const void *buf, long long len, unsigned *crc);
GRHIP_API int grhip_crc32_update(grhip_crc32 *h, unsigned crc_in, const void *buf, long long len, unsigned *crc);
typedef struct grhip_packet_maker grhip_packet_maker;
GRHIP_API int grhip_packet_maker_create(grhip_packet_maker **h, const char *access_code, double samples_per_symbol, int bits_per_symbol,
                                        int pad_for_usrp, int whitening, int device);
GRHIP_API void grhip_packet_maker_destroy(grhip_packet_maker *h);
GRHIP_API long long grhip_packet_maker_packet_bytes(grhip_packet_maker *h, int payload_len);
GRHIP_API int grhip_packet_maker_plan(grhip_packet_maker *h, int n, const int *lengths, const int *whitener_offsets,
                                      grhip_packet_job *jobs_out, long long *total_in, long long *total_out);
GRHIP_API int grhip_packet_maker_work_device(grhip_packet_maker *h, int n, const grhip_packet_job *d_jobs, const void *d_payloads,
                                             void *d_out, void *stream);
GRHIP_API int grhip_packet_maker_work(grhip_packet_maker *h, int n, const int *lengths, const int *whitener_offsets, const void *payloads,
                                      void *out, long long out_capacity, long long *total);
typedef struct grhip_packet_check grhip_packet_check;
GRHIP_API int grhip_packet_check_create(grhip_packet_check **h, int device);
GRHIP_API void grhip_packet_check_destroy(grhip_packet_check *h);
GRHIP_API int grhip_packet_check_work_device(grhip_packet_check *h, int n_streams, int max_msgs, const grhip_packet_rec *d_recs,
                                             long long rec_stride, const unsigned *d_counts, int count_stride_words, const void *d_pool,
                                             long long pool_stride, int dewhitening, void *d_payload_out, unsigned char *d_ok,
                                             void *stream);
GRHIP_API int grhip_framer_sink_1_batch_device_view(grhip_framer_sink_1_batch *h, const grhip_packet_rec **d_recs, long long *rec_stride,
                                                    const unsigned **d_counts, int *count_stride_words, const unsigned char **d_pool,
                                                    long long *pool_stride);

/* ======================================================================
 * gr_scrambler_bb, gr_descrambler_bb, gr_additive_scrambler_bb
 *   replace gr_make_scrambler_bb (mask, seed, len), gr_make_descrambler_bb (mask, seed, len),
 *       gr_make_additive_scrambler_bb (mask, seed, len, count = 0)
 *   general/gr_scrambler_bb.cc:44-57, general/gr_descrambler_bb.cc:44-57,
 *   general/gr_additive_scrambler_bb.cc:46-65, general/gri_lfsr.h:103-147
 * Bytes in, bytes out, S streams back to back ([S][n], S = 1 after create; `out` may not overlap `in`; n == 0
 * is a successful no-op; work_device does not synchronise).  Per stream the handle keeps gri_lfsr's 32-bit
 * register on the device, additive_scrambler_bb d_bits as well, across calls: the output depends on the
 * concatenated input alone.  set_streams restarts every stream from the seed.
 *   scrambler_bb    out = register bit 0; the register shifts right and takes parity(reg & mask) ^ (in & 1)
 *                   at bit len (gri_lfsr.h:120-125);
 *   descrambler_bb  out = parity(reg & mask) ^ (in & 1); the register takes in & 1 at bit len (:127-132);
 *   additive        out = in ^ register bit 0 -- the whole input byte is XORed with the 0/1 bit, .cc:55 --
 *                   and after every `count` items (count > 0) the register is the seed again (.cc:56-61).
 * len above 31 is refused (gri_lfsr.h:109-110 throws); mask and seed are taken as 32-bit patterns.
 * GRHIP_MODE_GENERIC is one lane per stream running the reference's statements.  Every other mode is the
 * parallel form and gives the same bytes: the step is linear over GF(2) once the register has no bit above
 * len, where the reference's OR of the new bit is an XOR.  The descrambler's register is the len + 1 input
 * bits before an item; the additive register does not depend on the data and is jumped to a lane's first item
 * with the powers M^(2^j) of the one-step matrix; the scrambler's step reg' = M reg ^ in e_len is affine and
 * is scanned (chunks from a zero register, a scan over a tile's chunks, a carry pass along a stream's tiles,
 * the tiles again from their true registers).  Bits of the seed above len shift out within 31 steps; until
 * then the reference's statement runs: the scrambler walks the first 32 items of a stream's life serially,
 * the additive jump steps serially while such bits remain, the descrambler's register needs no such care.
 * ====================================================================== */
typedef struct grhip_scrambler_bb grhip_scrambler_bb;
GRHIP_API int grhip_scrambler_bb_create(grhip_scrambler_bb **h, int mask, int seed, int len, int device);
GRHIP_API void grhip_scrambler_bb_destroy(grhip_scrambler_bb *h);
GRHIP_API int grhip_scrambler_bb_set_mode(grhip_scrambler_bb *h, int mode);
GRHIP_API int grhip_scrambler_bb_set_streams(grhip_scrambler_bb *h, int nstreams);
GRHIP_API int grhip_scrambler_bb_work(grhip_scrambler_bb *h, int n, const void *in, void *out);
GRHIP_API int grhip_scrambler_bb_work_device(grhip_scrambler_bb *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_descrambler_bb grhip_descrambler_bb;
GRHIP_API int grhip_descrambler_bb_create(grhip_descrambler_bb **h, int mask, int seed, int len, int device);
GRHIP_API void grhip_descrambler_bb_destroy(grhip_descrambler_bb *h);
GRHIP_API int grhip_descrambler_bb_set_mode(grhip_descrambler_bb *h, int mode);
GRHIP_API int grhip_descrambler_bb_set_streams(grhip_descrambler_bb *h, int nstreams);
GRHIP_API int grhip_descrambler_bb_work(grhip_descrambler_bb *h, int n, const void *in, void *out);
GRHIP_API int grhip_descrambler_bb_work_device(grhip_descrambler_bb *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_additive_scrambler_bb grhip_additive_scrambler_bb;
GRHIP_API int grhip_additive_scrambler_bb_create(grhip_additive_scrambler_bb **h, int mask, int seed, int len, int count, int device);
GRHIP_API void grhip_additive_scrambler_bb_destroy(grhip_additive_scrambler_bb *h);
GRHIP_API int grhip_additive_scrambler_bb_set_mode(grhip_additive_scrambler_bb *h, int mode);
GRHIP_API int grhip_additive_scrambler_bb_set_streams(grhip_additive_scrambler_bb *h, int nstreams);
GRHIP_API int grhip_additive_scrambler_bb_work(grhip_additive_scrambler_bb *h, int n, const void *in, void *out);
GRHIP_API int grhip_additive_scrambler_bb_work_device(grhip_additive_scrambler_bb *h, int n, const void *d_in, void *d_out, void *stream);

/* ======================================================================
 * gr_frequency_modulator_fc
 *   replaces gr_make_frequency_modulator_fc (double sensitivity)
 *   general/gr_frequency_modulator_fc.cc:49-72 (work), .h:42-52 (d_sensitivity, d_phase, set_sensitivity)
 * Float in, complex out, S streams back to back ([S][n], S = 1 after create; `out` may not overlap `in`; n == 0
 * is a successful no-op; work_device does not synchronise).  Per item phase += sensitivity * in[i] in double
 * and out[i] = (cos, sin) of (float)phase (.cc:58-61).  After the LAST item of a work call only, |phase| > 16 pi
 * becomes phase - trunc(phase / 2 pi) * 2 pi (.cc:66-69).  The float cast sees the unwrapped phase inside a
 * call, so THE OUTPUT DEPENDS ON WHERE THE CALLS ARE CUT, exactly as the reference's does on its scheduler's
 * calls: a stream run as one call, and the same stream cut in two, differ by float roundings of the phase
 * wherever it has passed 16 pi.  The phase is one double per stream on the device; set_streams zeroes it.
 * set_sensitivity takes a float and widens it, as .h:51 does, and holds from the next work call; sensitivity()
 * returns the float of .h:52.  phase() / set_phase() read one stream's d_phase and set every stream's.
 *   GRHIP_MODE_GENERIC  one wavefront per stream walks the recurrence in the reference's order, every double
 *       operation rounded once; out = ((float)cos((double)p), (float)sin((double)p)) of p = (float)phase.  The
 *       phase state equals the reference's bit for bit, across cuts; the outputs are within one float ulp per
 *       component of glibc's sincosf, which is not the rounded double sine (as for pll_refout_cc).
 *   every other mode  a scan in three launches: sums of sensitivity * x in double per tile of
 *       grhip_frequency_modulator_fc_tile() items, the tiles' start phases from the call's entry phase, then a
 *       workgroup scan per tile; phi - 2 pi rint(phi / 2 pi) in double before the float cast and a float
 *       polynomial sine / cosine.  Calls of at most one tile are one launch.  Every output lies within
 *       1e-5 + 2^-50 * Phi of exp(j phi) evaluated in double, Phi = sum |sensitivity * x| over the call plus
 *       |entry phase| -- inside long calls that is closer than the reference, whose float cast loses
 *       2^-24 |phase|.  The wrap rule is applied to the call's total, so the state follows GENERIC within
 *       n * 2^-53 * Phi.
 * From a stream's first non-finite product on, every output of that stream is NaN in both modes and its state
 * is non-finite; other streams are untouched.
 * ====================================================================== */
typedef struct grhip_frequency_modulator_fc grhip_frequency_modulator_fc;
GRHIP_API int grhip_frequency_modulator_fc_create(grhip_frequency_modulator_fc **h, double sensitivity, int device);
GRHIP_API void grhip_frequency_modulator_fc_destroy(grhip_frequency_modulator_fc *h);
GRHIP_API int grhip_frequency_modulator_fc_set_mode(grhip_frequency_modulator_fc *h, int mode);
GRHIP_API int grhip_frequency_modulator_fc_set_streams(grhip_frequency_modulator_fc *h, int nstreams);
GRHIP_API int grhip_frequency_modulator_fc_work(grhip_frequency_modulator_fc *h, int n, const void *in, void *out);
GRHIP_API int grhip_frequency_modulator_fc_work_device(grhip_frequency_modulator_fc *h, int n, const void *d_in, void *d_out, void *stream);
GRHIP_API int grhip_frequency_modulator_fc_set_sensitivity(grhip_frequency_modulator_fc *h, float sensitivity);
GRHIP_API float grhip_frequency_modulator_fc_sensitivity(grhip_frequency_modulator_fc *h);
GRHIP_API int grhip_frequency_modulator_fc_phase(grhip_frequency_modulator_fc *h, int stream, double *phase);
GRHIP_API int grhip_frequency_modulator_fc_set_phase(grhip_frequency_modulator_fc *h, double phase);
GRHIP_API int grhip_frequency_modulator_fc_tile(void);

/* ======================================================================
 * gr_bytes_to_syms, gr_char_to_float, gr_chunks_to_symbols_bf
 *   replace gr_make_bytes_to_syms (), gr_make_char_to_float (),
 *       gr_make_chunks_to_symbols_bf (const std::vector<float> &symbol_table, const int D = 1)
 *   general/gr_bytes_to_syms.cc:45-71, general/gr_char_to_float.cc:42-53 with general/gri_char_to_float.cc:26-40,
 *   gengen/gr_chunks_to_symbols_XX.cc.t:51-74
 * Bytes in, floats out, S streams back to back, one lane per output item, the reference's values bit for bit
 * in every mode; nothing is kept between calls.
 *   bytes_to_syms         n bytes in, 8 n floats out: bit 7 first, 0 -> -1, 1 -> +1
 *   char_to_float         out = (float)(signed char)in
 *   chunks_to_symbols_bf  n bytes in, n * D floats out, symbol_table[in * D + d]; an index whose D entries do
 *                         not lie inside the table gives zeros (the reference asserts), as chunks_to_symbols_bc;
 *                         at most 65536 entries, D >= 1
 * ====================================================================== */
typedef struct grhip_bytes_to_syms grhip_bytes_to_syms;
GRHIP_API int grhip_bytes_to_syms_create(grhip_bytes_to_syms **h, int device);
GRHIP_API void grhip_bytes_to_syms_destroy(grhip_bytes_to_syms *h);
GRHIP_API int grhip_bytes_to_syms_set_mode(grhip_bytes_to_syms *h, int mode);
GRHIP_API int grhip_bytes_to_syms_set_streams(grhip_bytes_to_syms *h, int nstreams);
GRHIP_API int grhip_bytes_to_syms_work(grhip_bytes_to_syms *h, int n, const void *in, void *out);
GRHIP_API int grhip_bytes_to_syms_work_device(grhip_bytes_to_syms *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_char_to_float grhip_char_to_float;
GRHIP_API int grhip_char_to_float_create(grhip_char_to_float **h, int device);
GRHIP_API void grhip_char_to_float_destroy(grhip_char_to_float *h);
GRHIP_API int grhip_char_to_float_set_mode(grhip_char_to_float *h, int mode);
GRHIP_API int grhip_char_to_float_set_streams(grhip_char_to_float *h, int nstreams);
GRHIP_API int grhip_char_to_float_work(grhip_char_to_float *h, int n, const void *in, void *out);
GRHIP_API int grhip_char_to_float_work_device(grhip_char_to_float *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_chunks_to_symbols_bf grhip_chunks_to_symbols_bf;
GRHIP_API int grhip_chunks_to_symbols_bf_create(grhip_chunks_to_symbols_bf **h, const float *symbol_table, size_t nsymbols, int D, int device);
GRHIP_API void grhip_chunks_to_symbols_bf_destroy(grhip_chunks_to_symbols_bf *h);
GRHIP_API int grhip_chunks_to_symbols_bf_set_mode(grhip_chunks_to_symbols_bf *h, int mode);
GRHIP_API int grhip_chunks_to_symbols_bf_set_streams(grhip_chunks_to_symbols_bf *h, int nstreams);
GRHIP_API int grhip_chunks_to_symbols_bf_work(grhip_chunks_to_symbols_bf *h, int n, const void *in, void *out);
GRHIP_API int grhip_chunks_to_symbols_bf_work_device(grhip_chunks_to_symbols_bf *h, int n, const void *d_in, void *d_out, void *stream);
GRHIP_API int grhip_chunks_to_symbols_bf_D(grhip_chunks_to_symbols_bf *h);

/* ======================================================================
 * gr_cpm::phase_response, gr_firdes::gaussian, the taps of gmsk_mod: host arithmetic, no device
 *   replace gr_cpm::phase_response (type, samples_per_sym, L, beta = 0.3)   general/gr_cpm.cc:43-218
 *       gr_firdes::gaussian (gain, spb, bt, ntaps)                          general/gr_firdes.cc:571-594
 *       numpy.convolve(gaussian(1, sps, bt, 4 sps), (1,) * sps)             gr-digital/python/gmsk.py:99-107
 * Each returns the tap count and, when `taps` is not null, writes that many floats (`capacity` is the room at
 * `taps`; too little is GRHIP_EINVAL).  The statements and types are the reference's; boost::math::erf is
 * std::erf.  type: GRHIP_CPM_LRC .. GRHIP_CPM_GAUSSIAN; any other value gives LREC with L = 1, as
 * gr_cpm.cc:214 does.
 * Refused with GRHIP_EINVAL: samples_per_sym * L == 0; more than 4096 taps (samples_per_sym * L, ntaps,
 * 5 * samples_per_symbol - 1); ntaps < 1; samples_per_symbol < 2 for the gmsk taps (gmsk.py:87-88 raises); a
 * non-finite beta, gain, spb or bt.
 * ====================================================================== */
#define GRHIP_CPM_LRC 0
#define GRHIP_CPM_LSRC 1
#define GRHIP_CPM_LREC 2
#define GRHIP_CPM_TFM 3
#define GRHIP_CPM_GAUSSIAN 4
GRHIP_API int grhip_cpm_phase_response(int type, unsigned samples_per_sym, unsigned L, double beta, float *taps, size_t capacity);
GRHIP_API int grhip_firdes_gaussian(double gain, double spb, double bt, int ntaps, float *taps, size_t capacity);
GRHIP_API int grhip_gmsk_mod_taps(int samples_per_symbol, double bt, float *taps, size_t capacity);

/* ======================================================================
 * digital_cpmmod_bc, digital_gmskmod_bc, gmsk_mod
 *   replace digital_make_cpmmod_bc (type, h, samples_per_sym, L, beta = 0.3)     gr-digital/lib/digital_cpmmod_bc.cc:30-72
 *       digital_make_gmskmod_bc (samples_per_sym = 2, bt = 0.3, L = 4)           gr-digital/lib/digital_gmskmod_bc.cc:31-45
 *       gmsk_mod (samples_per_symbol = 2, bt = 0.35)                             gr-digital/python/gmsk.py:55-120
 * One handle each for the hier block, on NEW items only, S streams back to back:
 *   cpmmod_bc   char_to_float -> interp_fir_filter_fff(samples_per_sym, phase_response(type, ...)) ->
 *               frequency_modulator_fc(pi * h): n signed-char symbols in, n * samples_per_sym items out
 *   gmskmod_bc  cpmmod_bc(GAUSSIAN, 0.5, samples_per_sym, L, bt)
 *   gmsk_mod    bytes_to_syms -> interp_fir_filter_fff(sps, gmsk_mod_taps(sps, bt)) ->
 *               frequency_modulator_fc((pi / 2) / sps): n bytes in, 8 * n * sps items out
 * Per stream the interpolator's last nt - 1 symbols (nt taps per filter; zeros at the start, as the scheduler's
 * history) and the modulator's phase stay on the device; set_streams restarts every stream.  A work call of the
 * handle is a work call of every inner block, so the modulator's end-of-call wrap (above) falls where the
 * handle's calls end and THE OUTPUT DEPENDS ON THE CUTS as the inner modulator's does.  freq_out / d_freq_out
 * is optional (null: not wanted): the interpolator's output, [S][outputs] floats, the second output of
 * digital_cpmmod_bc's signature.
 * The phase integrates the frequency samples, so both engines form them in gr_fir_fff_generic's order in every
 * mode: they are the reference's floats bit for bit.
 *   engine 0  the library's blocks in a row; the only engine in GRHIP_MODE_GENERIC, where the handle equals the
 *             composition of char_to_float / bytes_to_syms, interp_fir_filter_fff and frequency_modulator_fc bit
 *             for bit, whatever the cuts.
 *   engine 1  the default in every other mode when the taps fit: at most 16 taps per filter and at most 1024
 *             taps after padding to a multiple of samples_per_sym (cpmmod_bc: L <= 16, samples_per_sym * L <=
 *             1024; gmsk_mod: sps <= 204).  One fused kernel behind a carry pre-pass: per tile of
 *             grhip_cpmmod_bc_tile() outputs the symbols go to LDS, each output's frequency sample is nt products
 *             against taps in LDS, and the tile is scanned in double as frequency_modulator_fc does; 1 / sps + 8
 *             bytes move per output.  Within frequency_modulator_fc's bound of the double evaluation.
 *   set_engine(1) where the taps do not fit is GRHIP_EINVAL; engine() reports the engine the next call runs.
 * Refused: a type outside GRHIP_CPM_LRC .. GRHIP_CPM_GAUSSIAN (digital_cpmmod_bc.cc:64-65 throws); what the
 * designers refuse; gmsk_mod's samples_per_symbol < 2; outputs per stream that do not fit an int.
 * Not built: cpm_mod of gr-digital/python/cpm.py (on pfb_arb_resampler_fff), cpfsk_bc, vco_f, gmsk_demod.
 * ====================================================================== */
typedef struct grhip_cpmmod_bc grhip_cpmmod_bc;
GRHIP_API int grhip_cpmmod_bc_create(grhip_cpmmod_bc **h, int type, float h_index, unsigned samples_per_sym, unsigned L, double beta, int device);
GRHIP_API void grhip_cpmmod_bc_destroy(grhip_cpmmod_bc *h);
GRHIP_API int grhip_cpmmod_bc_set_mode(grhip_cpmmod_bc *h, int mode);
GRHIP_API int grhip_cpmmod_bc_set_streams(grhip_cpmmod_bc *h, int nstreams);
GRHIP_API int grhip_cpmmod_bc_set_engine(grhip_cpmmod_bc *h, int engine);
GRHIP_API int grhip_cpmmod_bc_engine(grhip_cpmmod_bc *h);
GRHIP_API int grhip_cpmmod_bc_samples_per_symbol(grhip_cpmmod_bc *h);
GRHIP_API int grhip_cpmmod_bc_filter_taps(grhip_cpmmod_bc *h, float *taps, size_t capacity);
GRHIP_API int grhip_cpmmod_bc_phase(grhip_cpmmod_bc *h, int stream, double *phase);
GRHIP_API int grhip_cpmmod_bc_work(grhip_cpmmod_bc *h, int n, const void *in, void *out, void *freq_out);
GRHIP_API int grhip_cpmmod_bc_work_device(grhip_cpmmod_bc *h, int n, const void *d_in, void *d_out, void *d_freq_out, void *stream);
GRHIP_API int grhip_cpmmod_bc_tile(void);
typedef struct grhip_gmskmod_bc grhip_gmskmod_bc;
GRHIP_API int grhip_gmskmod_bc_create(grhip_gmskmod_bc **h, unsigned samples_per_sym, double bt, unsigned L, int device);
GRHIP_API void grhip_gmskmod_bc_destroy(grhip_gmskmod_bc *h);
GRHIP_API int grhip_gmskmod_bc_set_mode(grhip_gmskmod_bc *h, int mode);
GRHIP_API int grhip_gmskmod_bc_set_streams(grhip_gmskmod_bc *h, int nstreams);
GRHIP_API int grhip_gmskmod_bc_set_engine(grhip_gmskmod_bc *h, int engine);
GRHIP_API int grhip_gmskmod_bc_engine(grhip_gmskmod_bc *h);
GRHIP_API int grhip_gmskmod_bc_samples_per_symbol(grhip_gmskmod_bc *h);
GRHIP_API int grhip_gmskmod_bc_filter_taps(grhip_gmskmod_bc *h, float *taps, size_t capacity);
GRHIP_API int grhip_gmskmod_bc_phase(grhip_gmskmod_bc *h, int stream, double *phase);
GRHIP_API int grhip_gmskmod_bc_work(grhip_gmskmod_bc *h, int n, const void *in, void *out, void *freq_out);
GRHIP_API int grhip_gmskmod_bc_work_device(grhip_gmskmod_bc *h, int n, const void *d_in, void *d_out, void *d_freq_out, void *stream);
typedef struct grhip_gmsk_mod grhip_gmsk_mod;
GRHIP_API int grhip_gmsk_mod_create(grhip_gmsk_mod **h, int samples_per_symbol, double bt, int device);
GRHIP_API void grhip_gmsk_mod_destroy(grhip_gmsk_mod *h);
GRHIP_API int grhip_gmsk_mod_set_mode(grhip_gmsk_mod *h, int mode);
GRHIP_API int grhip_gmsk_mod_set_streams(grhip_gmsk_mod *h, int nstreams);
GRHIP_API int grhip_gmsk_mod_set_engine(grhip_gmsk_mod *h, int engine);
GRHIP_API int grhip_gmsk_mod_engine(grhip_gmsk_mod *h);
GRHIP_API int grhip_gmsk_mod_samples_per_symbol(grhip_gmsk_mod *h);
GRHIP_API int grhip_gmsk_mod_filter_taps(grhip_gmsk_mod *h, float *taps, size_t capacity);
GRHIP_API int grhip_gmsk_mod_phase(grhip_gmsk_mod *h, int stream, double *phase);
GRHIP_API int grhip_gmsk_mod_work(grhip_gmsk_mod *h, int n, const void *in, void *out, void *freq_out);
GRHIP_API int grhip_gmsk_mod_work_device(grhip_gmsk_mod *h, int n, const void *d_in, void *d_out, void *d_freq_out, void *stream);

/* ======================================================================
 * gr_iir_filter_ffd
 *   replaces gr_make_iir_filter_ffd(const std::vector<double> &fftaps,
 *       const std::vector<double> &fbtaps)
 *   filter/gr_iir_filter_ffd.cc:56-82 (work), filter/gri_iir.h:90-163 (set_taps, filter)
 * Float in, float out, n feed-forward and m feedback taps in double (the counts may differ).  The
 * handle takes S streams back to back as the gain loops do ([S][n_in], S = 1 after create; `out` may
 * not overlap `in`; work / work_device return GRHIP_OK, n_in == 0 is a successful no-op, work_device
 * does not synchronise).  One output is
 *     acc = ff[0] x[t];  acc += ff[i] x[t-i], i = 1 .. n-1;  acc += fb[i] y[t-i], i = 1 .. m-1;
 *     out[t] = (float)acc,   y[t] = acc
 * in double, every product and every add rounded once, nothing contracted, in that order.  fb[0] is
 * never read and the feedback is ADDED (the reference's convention: a pole at +p has fb[1] = +p; the
 * taps of fm_deemph carry a negative a1 for that reason, and stay as they are).  Per stream the
 * device holds the last n - 1 inputs as float and the last m - 1 accumulators as DOUBLE (the
 * reference's d_prev_output is of tap_type); both start at zero and carry across calls.  n == 0
 * writes zeros and touches no state.  set_taps is latched: it takes effect at the start of the next
 * work call and zeroes both delay lines (gri_iir::set_taps); set_streams zeroes them too.
 * Deviations: n > 0 with m == 0 is GRHIP_EINVAL (the reference writes past an empty vector there);
 * more than 64 taps on either side is GRHIP_EINVAL.  Taps that are not finite are accepted and run
 * serially.  GRHIP_EINVAL also: S < 1, n_in < 0, a null pointer, overlapping buffers.
 * GRHIP_MODE_GENERIC: the recurrence in order, one wavefront per stream, bit for bit the reference.
 * Every other mode, for calls of more than grhip_iir_filter_ffd_chunk() = 256 items, where
 * K = m - 1 <= 8, every tap is finite and max over j = 1 .. 256 of ||C^j||_inf <= 64 (C the K x K
 * companion matrix of fb: the zero-input response does not grow): the call is cut into chunks of 256
 * items from its first item; every chunk is walked from zero accumulators (its inputs in front are
 * the real ones), the chunks are chained in double, start of the next = C^256 start + end, and every
 * chunk is walked again from its true start in the arithmetic above.  Both forms work in double and
 * differ by the rounding of that chain alone: every output is within ulp_float(|y|) + 2^-40 peak of
 * GENERIC's, peak the largest |y| of the call and its carried state (the chain's error is at most
 * 256 * 64 * 2^-53 of it); within that the result depends on where the calls cut the input.  Samples
 * that are not finite spread through the chain as NaN.  Anything else -- K > 8, unstable or
 * non-finite taps, a call of at most one chunk -- runs the serial walk whatever the mode: such
 * input costs time, never correctness.  chunked(h) is 1 if the next call of more than one chunk
 * would take the chunked form (a latched set_taps counted), else 0.
 * ====================================================================== */
typedef struct grhip_iir_filter_ffd grhip_iir_filter_ffd;
GRHIP_API int grhip_iir_filter_ffd_create(grhip_iir_filter_ffd **h, const double *fftaps, size_t n, const double *fbtaps,
                                          size_t m, int device);
GRHIP_API void grhip_iir_filter_ffd_destroy(grhip_iir_filter_ffd *h);
GRHIP_API int grhip_iir_filter_ffd_set_taps(grhip_iir_filter_ffd *h, const double *fftaps, size_t n, const double *fbtaps,
                                            size_t m);
GRHIP_API int grhip_iir_filter_ffd_set_mode(grhip_iir_filter_ffd *h, int mode);
GRHIP_API int grhip_iir_filter_ffd_set_streams(grhip_iir_filter_ffd *h, int nstreams);
GRHIP_API int grhip_iir_filter_ffd_chunked(grhip_iir_filter_ffd *h);
GRHIP_API int grhip_iir_filter_ffd_work(grhip_iir_filter_ffd *h, int n_in, const void *in, void *out);
GRHIP_API int grhip_iir_filter_ffd_work_device(grhip_iir_filter_ffd *h, int n_in, const void *d_in, void *d_out, void *stream);
/* items per chunk of the chunked form of iir_filter_ffd */
GRHIP_API int grhip_iir_filter_ffd_chunk(void);

/* The taps of blks2.fm_deemph(fs, tau) (blks2impl/fm_emph.py:55-63) in double, host arithmetic only:
 * w_pp = tan((1 / tau) / (fs * 2)), a = [1, (w_pp - 1) / (w_pp + 1)], b0 = b1 = w_pp / (1 + w_pp).
 * fm_deemph is gr.iir_filter_ffd(b, a): b and a (two doubles each) are the fftaps and fbtaps of
 * grhip_iir_filter_ffd_create as they stand.  GRHIP_EINVAL: a null pointer, fs or tau zero or not
 * finite (the reference divides by them). */
GRHIP_API int grhip_fm_deemph_taps(double fs, double tau, double *b, double *a);

/* ======================================================================
 * blks2.fm_demod_cf / blks2.nbfm_rx  (hier block)
 *   blks2impl/fm_demod.py:51-72, nbfm_rx.py:67-88, fm_emph.py:44-72:
 *   gr_quadrature_demod_cf(k) -> fm_deemph, one gr_iir_filter_ffd(fftaps, fbtaps)
 *       -> gr_fir_filter_fff(audio_decim, audio_taps)
 * n == m == 0 means no de-emphasis (tau = None in the reference); taps on one side only are
 * GRHIP_EINVAL, as are more than 64 of them, audio_decim outside 1 .. 65536 and ntaps outside
 * 1 .. 65536.  The handle is the hier block as the scheduler runs it, NEW ITEMS ONLY: complex in as
 * [S][n_in] (S = 1 after create), float out, every inner block from a zero history -- the
 * demodulator's x[-1] = 0, the IIR's delay lines zero, the FIR's ntaps - 1 delay line zero -- so
 * output j is the FIR over the de-emphasised samples j D - (ntaps - 1) .. j D of the whole stream.
 * Per stream the device keeps the last complex sample, the IIR's state and the last ntaps - 1
 * de-emphasised floats across calls; the handle keeps the stream position modulo D (one for all
 * streams).  produced(h, n_in) is the number of j with j D inside the next call of n_in items;
 * stream s writes that many floats from out + s * produced.  work's *produced and work_device's
 * *d_produced (a device int; either may be null) receive it.  n_in == 0 is a successful no-op;
 * work_device does not synchronise; `out` may not overlap `in`.  set_streams restarts every stream.
 * GRHIP_MODE_GENERIC: the three blocks one after the other inside the handle -- the demodulator of
 * grhip_quadrature_demod_cf, the serial walk of grhip_iir_filter_ffd, the generic-order FIR of
 * grhip_fir_filter (fff) -- bit for bit the reference's chain; the outputs depend on the
 * concatenated input alone, never on where the calls cut it.
 * Every other mode: one fused kernel (engine(h) == 1) where n <= 2 and m <= 2, |a1| < 1 (a1 =
 * fbtaps[1]), W0 = ceil(60 ln 2 / -ln |a1|) <= tile() / 8 and ntaps <= 1025 (any audio_decim): one
 * workgroup per stream and tile of tile() = 8192 input samples demodulates the tile and the
 * W0 + ntaps - 1 samples in front of it into LDS (the demodulator is grhip_quadrature_demod_cf's,
 * which has one form), runs the de-emphasis over it in double as an affine scan over the lanes'
 * sub-chunks, narrows to float and forms the decimated outputs with f32 FMAs: 8 + 4 / D bytes of
 * memory traffic per input sample.  A tile that does not reach the call's start begins from a zero
 * accumulator W0 samples early: the truncation is at most 2^-60 of the peak.  Every other shape
 * (engine(h) == 0) runs the three blocks in a row, the IIR in its chunked form where
 * grhip_iir_filter_ffd would chunk it.  Either way every output is within 1e-5 of the output's peak
 * of the float64 chain over the same demodulator output (the FIR family's FAST contract); within
 * that the result depends on where the calls cut the input.  (For 75 us, W0 is 97 at 32 kHz and
 * 998 at 320 kHz.)
 * ====================================================================== */
typedef struct grhip_fm_demod_cf grhip_fm_demod_cf;
GRHIP_API int grhip_fm_demod_cf_create(grhip_fm_demod_cf **h, float k, const double *fftaps, size_t n, const double *fbtaps,
                                       size_t m, int audio_decim, const float *audio_taps, size_t ntaps, int device);
GRHIP_API void grhip_fm_demod_cf_destroy(grhip_fm_demod_cf *h);
GRHIP_API int grhip_fm_demod_cf_set_mode(grhip_fm_demod_cf *h, int mode);
GRHIP_API int grhip_fm_demod_cf_set_streams(grhip_fm_demod_cf *h, int nstreams);
GRHIP_API int grhip_fm_demod_cf_produced(grhip_fm_demod_cf *h, int n_in);
GRHIP_API int grhip_fm_demod_cf_engine(grhip_fm_demod_cf *h);
GRHIP_API int grhip_fm_demod_cf_tile(void);
GRHIP_API int grhip_fm_demod_cf_work(grhip_fm_demod_cf *h, int n_in, const void *in, void *out, int *produced);
GRHIP_API int grhip_fm_demod_cf_work_device(grhip_fm_demod_cf *h, int n_in, const void *d_in, void *d_out, int *d_produced,
                                            void *stream);

/* ======================================================================
 * blks2.am_demod_cf / blks2.demod_10k0a3e_cf  (hier block)
 *   blks2impl/am_demod.py:42-58, :60-76:
 *   gr_complex_to_mag -> gr_add_const_ff(-1.0) -> gr_fir_filter_fff(audio_decim, audio_taps)
 * (the reference designs audio_taps with optfir.low_pass(0.5, channel_rate, audio_pass, audio_stop,
 * 0.1, 60): grhip_optfir_low_pass, narrowed to float per tap.)  GRHIP_EINVAL: null taps, audio_decim
 * outside 1 .. 65536, ntaps outside 1 .. 65536.  The handle is the hier block as the scheduler runs
 * it, NEW ITEMS ONLY: complex in as [S][n_in] (S = 1 after create), float out,
 *     out[j] = sum_k taps[k] v[j D - k],  v[i] = (float)(|x[i]| - 1.0f) for i >= 0, a rounded float
 * add on grhip_complex_to_mag's magnitude, and v[i] = 0 for i < 0: the FIR's delay line starts as
 * zeros of ITS input, it is not |0| - 1 = -1.  Per stream the device keeps the last ntaps - 1 values
 * of v across calls; the handle keeps the stream position modulo D (one for all streams).
 * produced(h, n_in), *produced, *d_produced, n_in == 0, the output layout (stream s from out + s *
 * produced), overlap and set_streams are grhip_fm_demod_cf's.
 * GRHIP_MODE_GENERIC: the three steps one after the other inside the handle, the FIR the generic-
 * order one of grhip_fir_filter (fff): bit for bit the reference's chain; the outputs depend on the
 * concatenated input alone, never on where the calls cut it.
 * Every other mode: one fused kernel (engine(h) == 1) for ntaps <= max_taps() = 1025 and any
 * audio_decim: one workgroup per stream and tile of tile() = 4096 input samples forms v of the tile
 * and of the ntaps - 1 samples in front of it once per sample into LDS (the carried delay line where
 * those lie in front of the call) and the decimated outputs with f32 FMAs, taps ascending: 8 + 4 / D
 * bytes of memory traffic per input sample.  With audio_decim == 1 a lane forms outputs_per_lane()
 * = 8 adjacent outputs from a register window, one LDS word read per 8 FMAs; other decimations take
 * the plain step of the FM kernel (one read per FMA).  Longer filters (engine(h) == 0) run the three
 * steps in a row.  v is the same in every mode; every output is within 1e-5 of the output's peak of
 * the float64 FIR over the same float v (the FIR family's FAST contract).
 * ====================================================================== */
typedef struct grhip_am_demod_cf grhip_am_demod_cf;
GRHIP_API int grhip_am_demod_cf_create(grhip_am_demod_cf **h, int audio_decim, const float *audio_taps, size_t ntaps,
                                       int device);
GRHIP_API void grhip_am_demod_cf_destroy(grhip_am_demod_cf *h);
GRHIP_API int grhip_am_demod_cf_set_mode(grhip_am_demod_cf *h, int mode);
GRHIP_API int grhip_am_demod_cf_set_streams(grhip_am_demod_cf *h, int nstreams);
GRHIP_API int grhip_am_demod_cf_produced(grhip_am_demod_cf *h, int n_in);
GRHIP_API int grhip_am_demod_cf_engine(grhip_am_demod_cf *h);
GRHIP_API int grhip_am_demod_cf_tile(void);
GRHIP_API int grhip_am_demod_cf_outputs_per_lane(void);
GRHIP_API int grhip_am_demod_cf_max_taps(void);
GRHIP_API int grhip_am_demod_cf_work(grhip_am_demod_cf *h, int n_in, const void *in, void *out, int *produced);
GRHIP_API int grhip_am_demod_cf_work_device(grhip_am_demod_cf *h, int n_in, const void *d_in, void *d_out, int *d_produced,
                                            void *stream);

/* ======================================================================
 * gr_pfb_channelizer_ccf
 *   replaces gr_make_pfb_channelizer_ccf(unsigned numchans,
 *       const std::vector<float>& taps, float oversample_rate)
 *   filter/gr_pfb_channelizer_ccf.h:115-178, filter/gr_pfb_channelizer_ccf.cc:36-200
 * numchans input streams, one output stream of numchans-complex vectors.
 * history = taps_per_filter + 1 on every input.  GRHIP_EINVAL if
 * numchans/oversample_rate is not an integer (.cc:57-60).
 * general_work: ins[j] points at stream j including history; returns
 * noutput_items, *consumed = items to consume on every input.
 * ====================================================================== */
typedef struct grhip_pfb_channelizer_ccf grhip_pfb_channelizer_ccf;
GRHIP_API int grhip_pfb_channelizer_ccf_create(grhip_pfb_channelizer_ccf **h, unsigned numchans,
                                               const float *taps, size_t ntaps, float oversample_rate,
                                               int device);
GRHIP_API void grhip_pfb_channelizer_ccf_destroy(grhip_pfb_channelizer_ccf *h);
GRHIP_API int grhip_pfb_channelizer_ccf_set_taps(grhip_pfb_channelizer_ccf *h, const float *taps,
                                                 size_t ntaps);
GRHIP_API int grhip_pfb_channelizer_ccf_history(const grhip_pfb_channelizer_ccf *h);
GRHIP_API int grhip_pfb_channelizer_ccf_output_multiple(const grhip_pfb_channelizer_ccf *h);
GRHIP_API int grhip_pfb_channelizer_ccf_general_work(grhip_pfb_channelizer_ccf *h, int noutput_items,
                                                     const void *const *ins, void *out, int *consumed);
/* device form: the numchans streams live in ONE device buffer, stream j at
 * d_in + j*stream_stride_items complex items */
GRHIP_API int grhip_pfb_channelizer_ccf_general_work_device(grhip_pfb_channelizer_ccf *h,
                                                            int noutput_items, const void *d_in,
                                                            size_t stream_stride_items, void *d_out,
                                                            void *stream);

/* The hier block blks2.pfb_channelizer_ccf (gnuradio-core/src/python/gnuradio/blks2impl/pfb_channelizer.py:25-75:
 * gr_stream_to_streams -> gr_pfb_channelizer_ccf -> gr_vector_to_streams) as ONE call on the handle above: ONE
 * interleaved input stream (general/gr_stream_to_streams.cc:57-63: stream j's item m is d_in[m * numchans + j]), numchans
 * output streams (general/gr_vector_to_streams.cc:57-63: channel k's stream at d_out + k * out_stride_items, item t is
 * bin k of output vector t).  d_in carries taps_per_filter * numchans history items in front (the channeliser's history
 * of taps_per_filter + 1 on each of its inputs), zeros at the start of a flowgraph.  noutput_items and the return value are
 * the inner block's (output vectors = items per output stream); results equal the three blocks run one after the other
 * bit for bit.  Oversample rate 1 with 2 / 4 / 8 / 16 channels takes one fused kernel (16 B of memory traffic per
 * sample instead of 48); every other shape runs the three kernels on work buffers of the handle. */
GRHIP_API int grhip_pfb_channelizer_ccf_hier_work_device(grhip_pfb_channelizer_ccf *h, int noutput_items,
                                                         const void *d_in, void *d_out, size_t out_stride_items,
                                                         void *stream);

/* ======================================================================
 * Full DMR chain as one device-resident pipeline (hier block):
 *   freq_xlating_fir_filter_ccc -> quadrature_demod_cf ->
 *   clock_recovery_mm_ff -> binary_slicer_fb -> correlate_access_code_bb
 * for n_streams independent captures with identical parameters (SURVEY 8(e):
 * streams are independent units; this is the multi-stream batch that fills
 * the device for the serial M&M stage).  Each stream starts from fresh block
 * state on every run() (a capture is processed whole).
 * Decimation 1 / 2 / 4 with any taps; every other decimation up to 256 with a
 * real prototype (imaginary parts zero) of up to 1024 taps -- create fails with
 * GRHIP_EINVAL for a shape no batched engine takes.
 * ====================================================================== */
typedef struct grhip_dmr_chain grhip_dmr_chain;
typedef struct grhip_dmr_chain_params {
    int decimation;
    const float *taps; /* complex prototype taps, interleaved */
    size_t ntaps;
    double center_freq, sampling_freq;
    float demod_gain;
    float omega, gain_omega, mu, gain_mu, omega_relative_limit;
    const char *access_code;
    size_t access_code_len;
    int threshold;
} grhip_dmr_chain_params;
GRHIP_API int grhip_dmr_chain_create(grhip_dmr_chain **h, const grhip_dmr_chain_params *p,
                                     int n_streams, size_t max_samples_per_stream, int device);
GRHIP_API void grhip_dmr_chain_destroy(grhip_dmr_chain *h);
/* GRHIP_MODE_GENERIC runs the xlating FIR in gr_fir_ccc_generic order (one
 * stream at a time): the whole chain is then bit-exact against the reference's
 * generic path, symbols and bit decisions included. */
GRHIP_API int grhip_dmr_chain_set_mode(grhip_dmr_chain *h, int mode);
/* Scheduling of the clock recovery (digital_clock_recovery_mm_ff.cc:116-134, a serial recurrence per capture): one
 * wavefront per capture (1), eight captures per wavefront (8: the shape for batches of more than a thousand
 * captures, where the loop then leaves the FIR its full grid), or thirty-two (32: two lanes per capture, the samples
 * through a FIFO in registers; the loop on a sixteenth of the CUs -- measured slower per symbol, DESIGN 4.3, an option);
 * 0 = chosen by n_streams (the default: 1 or 8).  Results are identical (every form is bit-exact on its input). */
GRHIP_API int grhip_dmr_chain_set_captures_per_wave(grhip_dmr_chain *h, int captures);
/* Upper bound on the symbols the clock recovery produces per capture: the noutput_items of its general_work
 * (digital_clock_recovery_mm_ff.cc:113, `oo < noutput_items`); 0 = no bound but the output rows (the default).
 * A capture stops at exactly that many symbols, whichever form of the loop runs. */
GRHIP_API int grhip_dmr_chain_set_max_symbols(grhip_dmr_chain *h, size_t max_symbols);
/* 4FSK tail: with enable != 0 the symbols go through pager_slicer_fb(alpha)
 * (gr-pager/lib/pager_slicer_fb.cc:47-84) -> gr_unpack_k_bits_bb(2) (general/gr_unpack_k_bits_bb.cc:64-69) ->
 * the access-code correlator instead of the binary slicer: both bits of every symbol, most significant first.
 * d_bits then receives TWO items per symbol (bits_stride >= 2 * n_samples / decimation) and d_nbits their
 * number per stream.  The access code is matched against that dibit stream (gr-digital/python/pkt.py:143-147
 * feeds the correlator unpacked bits in the same way). */
GRHIP_API int grhip_dmr_chain_set_four_level(grhip_dmr_chain *h, int enable, float pager_alpha);
/* d_in: n_streams captures of n_samples complex each, stream s at
 * d_in + s*stream_stride_items (NO history in front: the chain supplies the
 * zeros a fresh flowgraph would).  d_bits: n_streams * bits_stride bytes;
 * d_nbits: n_streams ints (symbols produced per stream). */
GRHIP_API int grhip_dmr_chain_run_device(grhip_dmr_chain *h, const void *d_in, size_t n_samples,
                                         size_t stream_stride_items, unsigned char *d_bits,
                                         size_t bits_stride, int *d_nbits, void *stream);
/* intermediate products of the last run (device pointers owned by the handle):
 * which: 0 demod floats, 1 M&M soft symbols, 2 pager_slicer symbols (bytes, 4FSK tail only);
 * *stride receives the per-stream stride in items */
GRHIP_API int grhip_dmr_chain_intermediate(grhip_dmr_chain *h, int which, void **d_ptr, size_t *stride);

/* ======================================================================
 * fsm -- gr-trellis' finite-state machine
 *   replaces fsm (gr-trellis/src/lib/fsm.cc:34-452, base.cc:29-81)
 * Host arithmetic, no device.  The constructors, in the reference's order:
 *   create            fsm(I, S, O, NS, OS), :60-70
 *   create_text/_file fsm(const char *name), :82-117: "I S O", S * I next states, S * I outputs; the rest is comment
 *   create_generator  fsm(k, n, G), the (n, k) binary convolutional code, :125-224
 *   create_isi        fsm(mod_size, ch_length), :234-253
 *   create_cpm        fsm(P, M, L), :267-292
 *   create_joint      fsm(FSM1, FSM2), :307-329
 *   create_radix      fsm(FSM, n), :338-364
 * The tables: NS, OS (I * S ints, [state][input]); PS(state), PI(state), the (state, input) pairs that lead to
 * `state` in ascending (state, input) order (generate_PS_PI, :377-395 -- the decoder's tie-breaking depends on that
 * order); TMl, TMi (S * S ints, generate_TM / find_es, :401-452).  A table getter copies into `out` (cap ints) and
 * returns the count; with out == NULL it only returns the count.
 * Deviations:
 *   - the reference validates nothing and indexes out of range; here I, S, O < 1, table lengths other than I * S,
 *     an NS entry outside [0, S) and an OS entry outside [0, O) are GRHIP_EINVAL;
 *   - a text that ends early (or holds something that is no number) is GRHIP_EINVAL; the reference leaves the
 *     entries unset;
 *   - a disconnected FSM is accepted, as in the reference, which prints a message (:420-424) and goes on;
 *     grhip_fsm_connected() returns 0 for it instead of printing;
 *   - sizes are capped where an int product of the reference would overflow or a table would not be practical:
 *     S <= 2048, I <= 2^21, O <= 2^24, I * S <= 2^22; k <= 21, n <= 24 and a generator matrix without an all-zero
 *     row (the reference shifts by -1 there), ch_length, L and the radix at most 64.
 * Not built: write_trellis_svg, write_fsm_txt.
 * ====================================================================== */
typedef struct grhip_fsm grhip_fsm;
GRHIP_API int grhip_fsm_create(grhip_fsm **h, int I, int S, int O, const int *NS, int n_NS, const int *OS, int n_OS);
GRHIP_API int grhip_fsm_create_text(grhip_fsm **h, const char *text);
GRHIP_API int grhip_fsm_create_file(grhip_fsm **h, const char *path);
GRHIP_API int grhip_fsm_create_generator(grhip_fsm **h, int k, int n, const int *G, int n_G);
GRHIP_API int grhip_fsm_create_isi(grhip_fsm **h, int mod_size, int ch_length);
GRHIP_API int grhip_fsm_create_cpm(grhip_fsm **h, int P, int M, int L);
GRHIP_API int grhip_fsm_create_joint(grhip_fsm **h, const grhip_fsm *fsm1, const grhip_fsm *fsm2);
GRHIP_API int grhip_fsm_create_radix(grhip_fsm **h, const grhip_fsm *fsm, int n);
GRHIP_API void grhip_fsm_destroy(grhip_fsm *h);
GRHIP_API int grhip_fsm_I(const grhip_fsm *h);
GRHIP_API int grhip_fsm_S(const grhip_fsm *h);
GRHIP_API int grhip_fsm_O(const grhip_fsm *h);
GRHIP_API int grhip_fsm_connected(const grhip_fsm *h);
GRHIP_API int grhip_fsm_NS(const grhip_fsm *h, int *out, int cap);
GRHIP_API int grhip_fsm_OS(const grhip_fsm *h, int *out, int cap);
GRHIP_API int grhip_fsm_PS(const grhip_fsm *h, int state, int *out, int cap);
GRHIP_API int grhip_fsm_PI(const grhip_fsm *h, int state, int *out, int cap);
GRHIP_API int grhip_fsm_TMl(const grhip_fsm *h, int *out, int cap);
GRHIP_API int grhip_fsm_TMi(const grhip_fsm *h, int *out, int cap);

/* ======================================================================
 * trellis_encoder_bb / bs / bi / ss / si / ii
 *   replace trellis_make_encoder_XX (FSM, ST)
 *   gr-trellis/src/lib/trellis_encoder_XX.cc.t:50-75: out[i] = OS[ST * I + in[i]], ST = NS[ST * I + in[i]]
 * S streams back to back ([S][n], S = 1 after create; `out` may not overlap `in`; n == 0 is a successful no-op).
 * The handle copies the FSM and keeps one state per stream on the device across calls; ST(stream) reads it,
 * set_ST sets every stream's, set_streams restarts every stream from the constructor's (or the last set) ST.
 * Deviations:
 *   - with several streams the reference starts every stream of a call from the same d_ST and keeps the last
 *     stream's end state; here every stream carries its own.  For one stream the two agree, across any cuts;
 *   - an input symbol >= I or < 0 makes the reference read outside its tables; here the call fails with
 *     GRHIP_EINVAL, the outputs of that call are unspecified and every state is as before the call.  The check is
 *     a flag word written by the kernels and read after the call, so work_device waits for its stream;
 *   - ST outside [0, S) is GRHIP_EINVAL.
 * GRHIP_MODE_GENERIC: one wavefront per stream moves windows of 1024 items through LDS, coalesced, and one lane walks
 * each window.  Every other mode, for S <= 64 and calls above 256
 * items: the items are cut into chunks of 256; one wavefront per chunk runs the chunk from every start state at
 * once (lane s starts in state s) and leaves an S-byte end-state map; the maps are chained along the stream; every
 * chunk is walked again from its true start state, one lane per chunk.  The outputs are the same bytes.
 * ====================================================================== */
typedef struct grhip_trellis_encoder_bb grhip_trellis_encoder_bb;
GRHIP_API int grhip_trellis_encoder_bb_create(grhip_trellis_encoder_bb **h, const grhip_fsm *fsm, int ST, int device);
GRHIP_API void grhip_trellis_encoder_bb_destroy(grhip_trellis_encoder_bb *h);
GRHIP_API int grhip_trellis_encoder_bb_set_mode(grhip_trellis_encoder_bb *h, int mode);
GRHIP_API int grhip_trellis_encoder_bb_set_streams(grhip_trellis_encoder_bb *h, int nstreams);
GRHIP_API int grhip_trellis_encoder_bb_ST(grhip_trellis_encoder_bb *h, int stream, int *ST);
GRHIP_API int grhip_trellis_encoder_bb_set_ST(grhip_trellis_encoder_bb *h, int ST);
GRHIP_API int grhip_trellis_encoder_bb_work(grhip_trellis_encoder_bb *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_encoder_bb_work_device(grhip_trellis_encoder_bb *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_encoder_bs grhip_trellis_encoder_bs;
GRHIP_API int grhip_trellis_encoder_bs_create(grhip_trellis_encoder_bs **h, const grhip_fsm *fsm, int ST, int device);
GRHIP_API void grhip_trellis_encoder_bs_destroy(grhip_trellis_encoder_bs *h);
GRHIP_API int grhip_trellis_encoder_bs_set_mode(grhip_trellis_encoder_bs *h, int mode);
GRHIP_API int grhip_trellis_encoder_bs_set_streams(grhip_trellis_encoder_bs *h, int nstreams);
GRHIP_API int grhip_trellis_encoder_bs_ST(grhip_trellis_encoder_bs *h, int stream, int *ST);
GRHIP_API int grhip_trellis_encoder_bs_set_ST(grhip_trellis_encoder_bs *h, int ST);
GRHIP_API int grhip_trellis_encoder_bs_work(grhip_trellis_encoder_bs *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_encoder_bs_work_device(grhip_trellis_encoder_bs *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_encoder_bi grhip_trellis_encoder_bi;
GRHIP_API int grhip_trellis_encoder_bi_create(grhip_trellis_encoder_bi **h, const grhip_fsm *fsm, int ST, int device);
GRHIP_API void grhip_trellis_encoder_bi_destroy(grhip_trellis_encoder_bi *h);
GRHIP_API int grhip_trellis_encoder_bi_set_mode(grhip_trellis_encoder_bi *h, int mode);
GRHIP_API int grhip_trellis_encoder_bi_set_streams(grhip_trellis_encoder_bi *h, int nstreams);
GRHIP_API int grhip_trellis_encoder_bi_ST(grhip_trellis_encoder_bi *h, int stream, int *ST);
GRHIP_API int grhip_trellis_encoder_bi_set_ST(grhip_trellis_encoder_bi *h, int ST);
GRHIP_API int grhip_trellis_encoder_bi_work(grhip_trellis_encoder_bi *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_encoder_bi_work_device(grhip_trellis_encoder_bi *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_encoder_ss grhip_trellis_encoder_ss;
GRHIP_API int grhip_trellis_encoder_ss_create(grhip_trellis_encoder_ss **h, const grhip_fsm *fsm, int ST, int device);
GRHIP_API void grhip_trellis_encoder_ss_destroy(grhip_trellis_encoder_ss *h);
GRHIP_API int grhip_trellis_encoder_ss_set_mode(grhip_trellis_encoder_ss *h, int mode);
GRHIP_API int grhip_trellis_encoder_ss_set_streams(grhip_trellis_encoder_ss *h, int nstreams);
GRHIP_API int grhip_trellis_encoder_ss_ST(grhip_trellis_encoder_ss *h, int stream, int *ST);
GRHIP_API int grhip_trellis_encoder_ss_set_ST(grhip_trellis_encoder_ss *h, int ST);
GRHIP_API int grhip_trellis_encoder_ss_work(grhip_trellis_encoder_ss *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_encoder_ss_work_device(grhip_trellis_encoder_ss *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_encoder_si grhip_trellis_encoder_si;
GRHIP_API int grhip_trellis_encoder_si_create(grhip_trellis_encoder_si **h, const grhip_fsm *fsm, int ST, int device);
GRHIP_API void grhip_trellis_encoder_si_destroy(grhip_trellis_encoder_si *h);
GRHIP_API int grhip_trellis_encoder_si_set_mode(grhip_trellis_encoder_si *h, int mode);
GRHIP_API int grhip_trellis_encoder_si_set_streams(grhip_trellis_encoder_si *h, int nstreams);
GRHIP_API int grhip_trellis_encoder_si_ST(grhip_trellis_encoder_si *h, int stream, int *ST);
GRHIP_API int grhip_trellis_encoder_si_set_ST(grhip_trellis_encoder_si *h, int ST);
GRHIP_API int grhip_trellis_encoder_si_work(grhip_trellis_encoder_si *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_encoder_si_work_device(grhip_trellis_encoder_si *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_encoder_ii grhip_trellis_encoder_ii;
GRHIP_API int grhip_trellis_encoder_ii_create(grhip_trellis_encoder_ii **h, const grhip_fsm *fsm, int ST, int device);
GRHIP_API void grhip_trellis_encoder_ii_destroy(grhip_trellis_encoder_ii *h);
GRHIP_API int grhip_trellis_encoder_ii_set_mode(grhip_trellis_encoder_ii *h, int mode);
GRHIP_API int grhip_trellis_encoder_ii_set_streams(grhip_trellis_encoder_ii *h, int nstreams);
GRHIP_API int grhip_trellis_encoder_ii_ST(grhip_trellis_encoder_ii *h, int stream, int *ST);
GRHIP_API int grhip_trellis_encoder_ii_set_ST(grhip_trellis_encoder_ii *h, int ST);
GRHIP_API int grhip_trellis_encoder_ii_work(grhip_trellis_encoder_ii *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_encoder_ii_work_device(grhip_trellis_encoder_ii *h, int n, const void *d_in, void *d_out, void *stream);

/* ======================================================================
 * trellis_metrics_s / i / f / c, trellis_constellation_metrics_cf
 *   replace trellis_make_metrics_X (O, D, TABLE, TYPE), trellis_make_constellation_metrics_cf (constellation, TYPE)
 *   gr-trellis/src/lib/trellis_metrics_X.cc.t, calc_metric.cc:29-72 (s, i, f) and :212-250 (c),
 *   trellis_constellation_metrics_cf.cc, gr-digital/lib/digital_constellation.cc:86-94, :160-201
 * `n` counts trellis steps per stream: a step takes D items (short, int, float, complex) and gives O floats;
 * S streams back to back ([S][n * D] in, [S][n * O] out).  TABLE holds O * D items, [o][d]; set_TABLE replaces it
 * (its length must stay O * D).  The constellation form takes O = arity, D = dimensionality and the points of a
 * grhip_constellation, and get_distance's sum is the complex form's.
 * TYPE: GRHIP_TRELLIS_EUCLIDEAN  metric[o] = sum over d of s * s, s = in[d] - TABLE[o * D + d];
 *       GRHIP_TRELLIS_HARD_SYMBOL  0 for the first minimum of those sums in o order, from FLT_MAX, 1 elsewhere.
 * GRHIP_TRELLIS_HARD_BIT and every other value are refused at creation (GRHIP_EINVAL): the reference throws in work.
 * The arithmetic is the reference's, statement for statement and bit for bit in every mode: s is formed in the item's
 * type and metric[o] += s * s in float.  For short the difference is truncated to short and the product is an int;
 * for int difference and product wrap in two's complement (the reference's signed overflow beyond |s| > 46340 is
 * undefined); for complex the term is re * re + im * im, then the add.
 * ====================================================================== */
#define GRHIP_TRELLIS_EUCLIDEAN 200     /* gr-digital/include/digital_metric_type.h:26-28 */
#define GRHIP_TRELLIS_HARD_SYMBOL 201
#define GRHIP_TRELLIS_HARD_BIT 202
typedef struct grhip_trellis_metrics_s grhip_trellis_metrics_s;
GRHIP_API int grhip_trellis_metrics_s_create(grhip_trellis_metrics_s **h, int O, int D, const void *TABLE, int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_metrics_s_destroy(grhip_trellis_metrics_s *h);
GRHIP_API int grhip_trellis_metrics_s_set_mode(grhip_trellis_metrics_s *h, int mode);
GRHIP_API int grhip_trellis_metrics_s_set_streams(grhip_trellis_metrics_s *h, int nstreams);
GRHIP_API int grhip_trellis_metrics_s_set_TABLE(grhip_trellis_metrics_s *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_metrics_s_O(grhip_trellis_metrics_s *h);
GRHIP_API int grhip_trellis_metrics_s_D(grhip_trellis_metrics_s *h);
GRHIP_API int grhip_trellis_metrics_s_TYPE(grhip_trellis_metrics_s *h);
GRHIP_API int grhip_trellis_metrics_s_work(grhip_trellis_metrics_s *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_metrics_s_work_device(grhip_trellis_metrics_s *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_metrics_i grhip_trellis_metrics_i;
GRHIP_API int grhip_trellis_metrics_i_create(grhip_trellis_metrics_i **h, int O, int D, const void *TABLE, int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_metrics_i_destroy(grhip_trellis_metrics_i *h);
GRHIP_API int grhip_trellis_metrics_i_set_mode(grhip_trellis_metrics_i *h, int mode);
GRHIP_API int grhip_trellis_metrics_i_set_streams(grhip_trellis_metrics_i *h, int nstreams);
GRHIP_API int grhip_trellis_metrics_i_set_TABLE(grhip_trellis_metrics_i *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_metrics_i_O(grhip_trellis_metrics_i *h);
GRHIP_API int grhip_trellis_metrics_i_D(grhip_trellis_metrics_i *h);
GRHIP_API int grhip_trellis_metrics_i_TYPE(grhip_trellis_metrics_i *h);
GRHIP_API int grhip_trellis_metrics_i_work(grhip_trellis_metrics_i *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_metrics_i_work_device(grhip_trellis_metrics_i *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_metrics_f grhip_trellis_metrics_f;
GRHIP_API int grhip_trellis_metrics_f_create(grhip_trellis_metrics_f **h, int O, int D, const void *TABLE, int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_metrics_f_destroy(grhip_trellis_metrics_f *h);
GRHIP_API int grhip_trellis_metrics_f_set_mode(grhip_trellis_metrics_f *h, int mode);
GRHIP_API int grhip_trellis_metrics_f_set_streams(grhip_trellis_metrics_f *h, int nstreams);
GRHIP_API int grhip_trellis_metrics_f_set_TABLE(grhip_trellis_metrics_f *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_metrics_f_O(grhip_trellis_metrics_f *h);
GRHIP_API int grhip_trellis_metrics_f_D(grhip_trellis_metrics_f *h);
GRHIP_API int grhip_trellis_metrics_f_TYPE(grhip_trellis_metrics_f *h);
GRHIP_API int grhip_trellis_metrics_f_work(grhip_trellis_metrics_f *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_metrics_f_work_device(grhip_trellis_metrics_f *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_metrics_c grhip_trellis_metrics_c;
GRHIP_API int grhip_trellis_metrics_c_create(grhip_trellis_metrics_c **h, int O, int D, const void *TABLE, int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_metrics_c_destroy(grhip_trellis_metrics_c *h);
GRHIP_API int grhip_trellis_metrics_c_set_mode(grhip_trellis_metrics_c *h, int mode);
GRHIP_API int grhip_trellis_metrics_c_set_streams(grhip_trellis_metrics_c *h, int nstreams);
GRHIP_API int grhip_trellis_metrics_c_set_TABLE(grhip_trellis_metrics_c *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_metrics_c_O(grhip_trellis_metrics_c *h);
GRHIP_API int grhip_trellis_metrics_c_D(grhip_trellis_metrics_c *h);
GRHIP_API int grhip_trellis_metrics_c_TYPE(grhip_trellis_metrics_c *h);
GRHIP_API int grhip_trellis_metrics_c_work(grhip_trellis_metrics_c *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_metrics_c_work_device(grhip_trellis_metrics_c *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_constellation_metrics_cf grhip_trellis_constellation_metrics_cf;
GRHIP_API int grhip_trellis_constellation_metrics_cf_create(grhip_trellis_constellation_metrics_cf **h, const grhip_constellation *constellation,
                                                            int TYPE, int device);
GRHIP_API void grhip_trellis_constellation_metrics_cf_destroy(grhip_trellis_constellation_metrics_cf *h);
GRHIP_API int grhip_trellis_constellation_metrics_cf_set_mode(grhip_trellis_constellation_metrics_cf *h, int mode);
GRHIP_API int grhip_trellis_constellation_metrics_cf_set_streams(grhip_trellis_constellation_metrics_cf *h, int nstreams);
GRHIP_API int grhip_trellis_constellation_metrics_cf_O(grhip_trellis_constellation_metrics_cf *h);
GRHIP_API int grhip_trellis_constellation_metrics_cf_D(grhip_trellis_constellation_metrics_cf *h);
GRHIP_API int grhip_trellis_constellation_metrics_cf_TYPE(grhip_trellis_constellation_metrics_cf *h);
GRHIP_API int grhip_trellis_constellation_metrics_cf_work(grhip_trellis_constellation_metrics_cf *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_constellation_metrics_cf_work_device(grhip_trellis_constellation_metrics_cf *h, int n, const void *d_in,
                                                                 void *d_out, void *stream);

/* ======================================================================
 * trellis_viterbi_b / s / i
 *   replace trellis_make_viterbi_X (FSM, K, S0, SK)
 *   gr-trellis/src/lib/trellis_viterbi_X.cc.t:163-183, core_algorithms.cc:45-109 (viterbi_algorithm)
 * `n` counts output items per stream: [S][n * O] floats in, [S][n] bytes, shorts or ints out.  Every K steps are a
 * block that starts in S0 (negative: any state) and ends in SK (negative: the best state) and is decoded on its own.
 * The handle keeps nothing between calls, so n must be a multiple of K (set_output_multiple(K) in the reference):
 * any other n is GRHIP_EINVAL.  Refused at creation: K < 1, S0 >= S, SK >= S, S > 1024, and sizes whose byte counts do
 * not fit an int (in a call as well).
 * For every block the outputs equal viterbi_algorithm's in every mode: the predecessors of a state are tried in
 * PS[j] order under a strict <, so the first wins a tie; minm starts from INF = 1.0e9f and minmi from 0, so minmi = 0
 * where nothing is below INF; the step's norm is subtracted in float; for SK < 0 the first minimum below INF in state
 * order ends the path, state 0 where there is none.  NaN and infinite metrics go through the same statements: a NaN
 * never wins a comparison and never becomes the norm.
 * One deviation: where the traceback stands in a state without a predecessor the reference indexes an empty vector;
 * the handle writes input symbol 0 for that step, stays in that state and counts the event in dead_ends(), which
 * adds up over the handle's life in 64 bits and waits for the handle's stream.
 * The lanes of a wavefront are the states.  For S <= 64 a wavefront decodes blocks_per_wavefront() = 64 / S blocks
 * side by side; for larger S one workgroup of S lanes decodes one block.  Workgroups are persistent and loop over
 * the call's blocks; resident_blocks() is how many blocks the grid holds at once: 8 workgroups per CU for S <= 64; for the
 * large form what 7 waves per SIMD and two workgroups' LDS allow, one workgroup per CU from 449 states on.  Decisions are bit-packed,
 * ceil(log2 Pmax) bits per state and step (Pmax: the longest predecessor list).  trace_window() is the number of
 * steps whose trace fits in LDS (INT_MAX where a decision takes no bit); a larger K flushes the trace to a workspace
 * owned by the handle, sized by the resident blocks, not by the call, and reported by workspace_bytes().  The
 * workspace is capped at 1 GiB: fewer blocks are then resident, and a K whose single block needs more is GRHIP_EINVAL.
 * GRHIP_MODE_GENERIC reads metrics and predecessor table from device memory; every other mode stages the metrics in
 * an LDS window and keeps short predecessor lists in registers.  The bytes are the same.
 * Not built: splitting one block across wavefronts (a (min,+) matrix scan would not be bit-exact), sliding-window
 * decoding, trellis_siso_f / siso_combined_f, the sccc / pccc encoders and decoders,
 * trellis_permutation and the interleaver.
 * ====================================================================== */
typedef struct grhip_trellis_viterbi_b grhip_trellis_viterbi_b;
GRHIP_API int grhip_trellis_viterbi_b_create(grhip_trellis_viterbi_b **h, const grhip_fsm *fsm, int K, int S0, int SK, int device);
GRHIP_API void grhip_trellis_viterbi_b_destroy(grhip_trellis_viterbi_b *h);
GRHIP_API int grhip_trellis_viterbi_b_set_mode(grhip_trellis_viterbi_b *h, int mode);
GRHIP_API int grhip_trellis_viterbi_b_set_streams(grhip_trellis_viterbi_b *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_b_K(grhip_trellis_viterbi_b *h);
GRHIP_API int grhip_trellis_viterbi_b_S0(grhip_trellis_viterbi_b *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_b_SK(grhip_trellis_viterbi_b *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_b_trace_window(grhip_trellis_viterbi_b *h);
GRHIP_API int grhip_trellis_viterbi_b_resident_blocks(grhip_trellis_viterbi_b *h);
GRHIP_API int grhip_trellis_viterbi_b_blocks_per_wavefront(grhip_trellis_viterbi_b *h);
GRHIP_API int grhip_trellis_viterbi_b_workspace_bytes(grhip_trellis_viterbi_b *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_b_dead_ends(grhip_trellis_viterbi_b *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_b_work(grhip_trellis_viterbi_b *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_b_work_device(grhip_trellis_viterbi_b *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_s grhip_trellis_viterbi_s;
GRHIP_API int grhip_trellis_viterbi_s_create(grhip_trellis_viterbi_s **h, const grhip_fsm *fsm, int K, int S0, int SK, int device);
GRHIP_API void grhip_trellis_viterbi_s_destroy(grhip_trellis_viterbi_s *h);
GRHIP_API int grhip_trellis_viterbi_s_set_mode(grhip_trellis_viterbi_s *h, int mode);
GRHIP_API int grhip_trellis_viterbi_s_set_streams(grhip_trellis_viterbi_s *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_s_K(grhip_trellis_viterbi_s *h);
GRHIP_API int grhip_trellis_viterbi_s_S0(grhip_trellis_viterbi_s *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_s_SK(grhip_trellis_viterbi_s *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_s_trace_window(grhip_trellis_viterbi_s *h);
GRHIP_API int grhip_trellis_viterbi_s_resident_blocks(grhip_trellis_viterbi_s *h);
GRHIP_API int grhip_trellis_viterbi_s_blocks_per_wavefront(grhip_trellis_viterbi_s *h);
GRHIP_API int grhip_trellis_viterbi_s_workspace_bytes(grhip_trellis_viterbi_s *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_s_dead_ends(grhip_trellis_viterbi_s *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_s_work(grhip_trellis_viterbi_s *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_s_work_device(grhip_trellis_viterbi_s *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_i grhip_trellis_viterbi_i;
GRHIP_API int grhip_trellis_viterbi_i_create(grhip_trellis_viterbi_i **h, const grhip_fsm *fsm, int K, int S0, int SK, int device);
GRHIP_API void grhip_trellis_viterbi_i_destroy(grhip_trellis_viterbi_i *h);
GRHIP_API int grhip_trellis_viterbi_i_set_mode(grhip_trellis_viterbi_i *h, int mode);
GRHIP_API int grhip_trellis_viterbi_i_set_streams(grhip_trellis_viterbi_i *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_i_K(grhip_trellis_viterbi_i *h);
GRHIP_API int grhip_trellis_viterbi_i_S0(grhip_trellis_viterbi_i *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_i_SK(grhip_trellis_viterbi_i *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_i_trace_window(grhip_trellis_viterbi_i *h);
GRHIP_API int grhip_trellis_viterbi_i_resident_blocks(grhip_trellis_viterbi_i *h);
GRHIP_API int grhip_trellis_viterbi_i_blocks_per_wavefront(grhip_trellis_viterbi_i *h);
GRHIP_API int grhip_trellis_viterbi_i_workspace_bytes(grhip_trellis_viterbi_i *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_i_dead_ends(grhip_trellis_viterbi_i *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_i_work(grhip_trellis_viterbi_i *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_i_work_device(grhip_trellis_viterbi_i *h, int n, const void *d_in, void *d_out, void *stream);

/* ======================================================================
 * trellis_viterbi_combined_{s,i,f,c}{b,s,i}
 *   replace trellis_make_viterbi_combined_XX (FSM, K, S0, SK, D, TABLE, TYPE)
 *   gr-trellis/src/lib/trellis_viterbi_combined_XX.cc.t, core_algorithms.cc:147-217 (viterbi_algorithm_combined)
 * The metrics of trellis_metrics_X computed per step inside the decoder of trellis_viterbi_X: [S][n * D] items (short,
 * int, float, complex) in, [S][n] bytes, shorts or ints out, n a multiple of K.  TABLE holds O * D items; set_TABLE
 * replaces it (same length).  Everything the two sections above state holds here: the metric arithmetic, the metric
 * types (GRHIP_TRELLIS_HARD_BIT and unknown types are GRHIP_EINVAL at creation), the decoder's contract, its one
 * deviation and its refusals; D outside 1 .. 65536 is GRHIP_EINVAL as well.  The outputs are the reference's in every
 * mode and engine.
 * Engine 0 runs the library's metrics kernel into a scratch buffer owned by the handle and then the decoder.  Engine 1,
 * the default, forms the step's O metrics inside the decoder's LDS window from the D raw inputs, so that a step moves
 * D * sizeof(item) bytes instead of 4 * O.  GRHIP_MODE_GENERIC, and an O too large for the metric window, run engine 0
 * whatever was set; engine() returns the engine the next call takes.
 * ====================================================================== */
typedef struct grhip_trellis_viterbi_combined_sb grhip_trellis_viterbi_combined_sb;
GRHIP_API int grhip_trellis_viterbi_combined_sb_create(grhip_trellis_viterbi_combined_sb **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_sb_destroy(grhip_trellis_viterbi_combined_sb *h);
GRHIP_API int grhip_trellis_viterbi_combined_sb_set_mode(grhip_trellis_viterbi_combined_sb *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_sb_set_streams(grhip_trellis_viterbi_combined_sb *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_sb_set_TABLE(grhip_trellis_viterbi_combined_sb *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_sb_set_engine(grhip_trellis_viterbi_combined_sb *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_sb_engine(grhip_trellis_viterbi_combined_sb *h);
GRHIP_API int grhip_trellis_viterbi_combined_sb_D(grhip_trellis_viterbi_combined_sb *h);
GRHIP_API int grhip_trellis_viterbi_combined_sb_TYPE(grhip_trellis_viterbi_combined_sb *h);
GRHIP_API int grhip_trellis_viterbi_combined_sb_K(grhip_trellis_viterbi_combined_sb *h);
GRHIP_API int grhip_trellis_viterbi_combined_sb_S0(grhip_trellis_viterbi_combined_sb *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_sb_SK(grhip_trellis_viterbi_combined_sb *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_sb_resident_blocks(grhip_trellis_viterbi_combined_sb *h);
GRHIP_API int grhip_trellis_viterbi_combined_sb_blocks_per_wavefront(grhip_trellis_viterbi_combined_sb *h);
GRHIP_API int grhip_trellis_viterbi_combined_sb_workspace_bytes(grhip_trellis_viterbi_combined_sb *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_sb_trace_window(grhip_trellis_viterbi_combined_sb *h);
GRHIP_API int grhip_trellis_viterbi_combined_sb_dead_ends(grhip_trellis_viterbi_combined_sb *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_sb_work(grhip_trellis_viterbi_combined_sb *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_sb_work_device(grhip_trellis_viterbi_combined_sb *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_ss grhip_trellis_viterbi_combined_ss;
GRHIP_API int grhip_trellis_viterbi_combined_ss_create(grhip_trellis_viterbi_combined_ss **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_ss_destroy(grhip_trellis_viterbi_combined_ss *h);
GRHIP_API int grhip_trellis_viterbi_combined_ss_set_mode(grhip_trellis_viterbi_combined_ss *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_ss_set_streams(grhip_trellis_viterbi_combined_ss *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_ss_set_TABLE(grhip_trellis_viterbi_combined_ss *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_ss_set_engine(grhip_trellis_viterbi_combined_ss *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_ss_engine(grhip_trellis_viterbi_combined_ss *h);
GRHIP_API int grhip_trellis_viterbi_combined_ss_D(grhip_trellis_viterbi_combined_ss *h);
GRHIP_API int grhip_trellis_viterbi_combined_ss_TYPE(grhip_trellis_viterbi_combined_ss *h);
GRHIP_API int grhip_trellis_viterbi_combined_ss_K(grhip_trellis_viterbi_combined_ss *h);
GRHIP_API int grhip_trellis_viterbi_combined_ss_S0(grhip_trellis_viterbi_combined_ss *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_ss_SK(grhip_trellis_viterbi_combined_ss *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_ss_resident_blocks(grhip_trellis_viterbi_combined_ss *h);
GRHIP_API int grhip_trellis_viterbi_combined_ss_blocks_per_wavefront(grhip_trellis_viterbi_combined_ss *h);
GRHIP_API int grhip_trellis_viterbi_combined_ss_workspace_bytes(grhip_trellis_viterbi_combined_ss *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_ss_trace_window(grhip_trellis_viterbi_combined_ss *h);
GRHIP_API int grhip_trellis_viterbi_combined_ss_dead_ends(grhip_trellis_viterbi_combined_ss *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_ss_work(grhip_trellis_viterbi_combined_ss *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_ss_work_device(grhip_trellis_viterbi_combined_ss *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_si grhip_trellis_viterbi_combined_si;
GRHIP_API int grhip_trellis_viterbi_combined_si_create(grhip_trellis_viterbi_combined_si **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_si_destroy(grhip_trellis_viterbi_combined_si *h);
GRHIP_API int grhip_trellis_viterbi_combined_si_set_mode(grhip_trellis_viterbi_combined_si *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_si_set_streams(grhip_trellis_viterbi_combined_si *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_si_set_TABLE(grhip_trellis_viterbi_combined_si *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_si_set_engine(grhip_trellis_viterbi_combined_si *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_si_engine(grhip_trellis_viterbi_combined_si *h);
GRHIP_API int grhip_trellis_viterbi_combined_si_D(grhip_trellis_viterbi_combined_si *h);
GRHIP_API int grhip_trellis_viterbi_combined_si_TYPE(grhip_trellis_viterbi_combined_si *h);
GRHIP_API int grhip_trellis_viterbi_combined_si_K(grhip_trellis_viterbi_combined_si *h);
GRHIP_API int grhip_trellis_viterbi_combined_si_S0(grhip_trellis_viterbi_combined_si *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_si_SK(grhip_trellis_viterbi_combined_si *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_si_resident_blocks(grhip_trellis_viterbi_combined_si *h);
GRHIP_API int grhip_trellis_viterbi_combined_si_blocks_per_wavefront(grhip_trellis_viterbi_combined_si *h);
GRHIP_API int grhip_trellis_viterbi_combined_si_workspace_bytes(grhip_trellis_viterbi_combined_si *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_si_trace_window(grhip_trellis_viterbi_combined_si *h);
GRHIP_API int grhip_trellis_viterbi_combined_si_dead_ends(grhip_trellis_viterbi_combined_si *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_si_work(grhip_trellis_viterbi_combined_si *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_si_work_device(grhip_trellis_viterbi_combined_si *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_ib grhip_trellis_viterbi_combined_ib;
GRHIP_API int grhip_trellis_viterbi_combined_ib_create(grhip_trellis_viterbi_combined_ib **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_ib_destroy(grhip_trellis_viterbi_combined_ib *h);
GRHIP_API int grhip_trellis_viterbi_combined_ib_set_mode(grhip_trellis_viterbi_combined_ib *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_ib_set_streams(grhip_trellis_viterbi_combined_ib *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_ib_set_TABLE(grhip_trellis_viterbi_combined_ib *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_ib_set_engine(grhip_trellis_viterbi_combined_ib *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_ib_engine(grhip_trellis_viterbi_combined_ib *h);
GRHIP_API int grhip_trellis_viterbi_combined_ib_D(grhip_trellis_viterbi_combined_ib *h);
GRHIP_API int grhip_trellis_viterbi_combined_ib_TYPE(grhip_trellis_viterbi_combined_ib *h);
GRHIP_API int grhip_trellis_viterbi_combined_ib_K(grhip_trellis_viterbi_combined_ib *h);
GRHIP_API int grhip_trellis_viterbi_combined_ib_S0(grhip_trellis_viterbi_combined_ib *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_ib_SK(grhip_trellis_viterbi_combined_ib *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_ib_resident_blocks(grhip_trellis_viterbi_combined_ib *h);
GRHIP_API int grhip_trellis_viterbi_combined_ib_blocks_per_wavefront(grhip_trellis_viterbi_combined_ib *h);
GRHIP_API int grhip_trellis_viterbi_combined_ib_workspace_bytes(grhip_trellis_viterbi_combined_ib *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_ib_trace_window(grhip_trellis_viterbi_combined_ib *h);
GRHIP_API int grhip_trellis_viterbi_combined_ib_dead_ends(grhip_trellis_viterbi_combined_ib *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_ib_work(grhip_trellis_viterbi_combined_ib *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_ib_work_device(grhip_trellis_viterbi_combined_ib *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_is grhip_trellis_viterbi_combined_is;
GRHIP_API int grhip_trellis_viterbi_combined_is_create(grhip_trellis_viterbi_combined_is **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_is_destroy(grhip_trellis_viterbi_combined_is *h);
GRHIP_API int grhip_trellis_viterbi_combined_is_set_mode(grhip_trellis_viterbi_combined_is *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_is_set_streams(grhip_trellis_viterbi_combined_is *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_is_set_TABLE(grhip_trellis_viterbi_combined_is *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_is_set_engine(grhip_trellis_viterbi_combined_is *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_is_engine(grhip_trellis_viterbi_combined_is *h);
GRHIP_API int grhip_trellis_viterbi_combined_is_D(grhip_trellis_viterbi_combined_is *h);
GRHIP_API int grhip_trellis_viterbi_combined_is_TYPE(grhip_trellis_viterbi_combined_is *h);
GRHIP_API int grhip_trellis_viterbi_combined_is_K(grhip_trellis_viterbi_combined_is *h);
GRHIP_API int grhip_trellis_viterbi_combined_is_S0(grhip_trellis_viterbi_combined_is *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_is_SK(grhip_trellis_viterbi_combined_is *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_is_resident_blocks(grhip_trellis_viterbi_combined_is *h);
GRHIP_API int grhip_trellis_viterbi_combined_is_blocks_per_wavefront(grhip_trellis_viterbi_combined_is *h);
GRHIP_API int grhip_trellis_viterbi_combined_is_workspace_bytes(grhip_trellis_viterbi_combined_is *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_is_trace_window(grhip_trellis_viterbi_combined_is *h);
GRHIP_API int grhip_trellis_viterbi_combined_is_dead_ends(grhip_trellis_viterbi_combined_is *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_is_work(grhip_trellis_viterbi_combined_is *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_is_work_device(grhip_trellis_viterbi_combined_is *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_ii grhip_trellis_viterbi_combined_ii;
GRHIP_API int grhip_trellis_viterbi_combined_ii_create(grhip_trellis_viterbi_combined_ii **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_ii_destroy(grhip_trellis_viterbi_combined_ii *h);
GRHIP_API int grhip_trellis_viterbi_combined_ii_set_mode(grhip_trellis_viterbi_combined_ii *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_ii_set_streams(grhip_trellis_viterbi_combined_ii *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_ii_set_TABLE(grhip_trellis_viterbi_combined_ii *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_ii_set_engine(grhip_trellis_viterbi_combined_ii *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_ii_engine(grhip_trellis_viterbi_combined_ii *h);
GRHIP_API int grhip_trellis_viterbi_combined_ii_D(grhip_trellis_viterbi_combined_ii *h);
GRHIP_API int grhip_trellis_viterbi_combined_ii_TYPE(grhip_trellis_viterbi_combined_ii *h);
GRHIP_API int grhip_trellis_viterbi_combined_ii_K(grhip_trellis_viterbi_combined_ii *h);
GRHIP_API int grhip_trellis_viterbi_combined_ii_S0(grhip_trellis_viterbi_combined_ii *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_ii_SK(grhip_trellis_viterbi_combined_ii *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_ii_resident_blocks(grhip_trellis_viterbi_combined_ii *h);
GRHIP_API int grhip_trellis_viterbi_combined_ii_blocks_per_wavefront(grhip_trellis_viterbi_combined_ii *h);
GRHIP_API int grhip_trellis_viterbi_combined_ii_workspace_bytes(grhip_trellis_viterbi_combined_ii *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_ii_trace_window(grhip_trellis_viterbi_combined_ii *h);
GRHIP_API int grhip_trellis_viterbi_combined_ii_dead_ends(grhip_trellis_viterbi_combined_ii *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_ii_work(grhip_trellis_viterbi_combined_ii *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_ii_work_device(grhip_trellis_viterbi_combined_ii *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_fb grhip_trellis_viterbi_combined_fb;
GRHIP_API int grhip_trellis_viterbi_combined_fb_create(grhip_trellis_viterbi_combined_fb **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_fb_destroy(grhip_trellis_viterbi_combined_fb *h);
GRHIP_API int grhip_trellis_viterbi_combined_fb_set_mode(grhip_trellis_viterbi_combined_fb *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_fb_set_streams(grhip_trellis_viterbi_combined_fb *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_fb_set_TABLE(grhip_trellis_viterbi_combined_fb *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_fb_set_engine(grhip_trellis_viterbi_combined_fb *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_fb_engine(grhip_trellis_viterbi_combined_fb *h);
GRHIP_API int grhip_trellis_viterbi_combined_fb_D(grhip_trellis_viterbi_combined_fb *h);
GRHIP_API int grhip_trellis_viterbi_combined_fb_TYPE(grhip_trellis_viterbi_combined_fb *h);
GRHIP_API int grhip_trellis_viterbi_combined_fb_K(grhip_trellis_viterbi_combined_fb *h);
GRHIP_API int grhip_trellis_viterbi_combined_fb_S0(grhip_trellis_viterbi_combined_fb *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_fb_SK(grhip_trellis_viterbi_combined_fb *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_fb_resident_blocks(grhip_trellis_viterbi_combined_fb *h);
GRHIP_API int grhip_trellis_viterbi_combined_fb_blocks_per_wavefront(grhip_trellis_viterbi_combined_fb *h);
GRHIP_API int grhip_trellis_viterbi_combined_fb_workspace_bytes(grhip_trellis_viterbi_combined_fb *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_fb_trace_window(grhip_trellis_viterbi_combined_fb *h);
GRHIP_API int grhip_trellis_viterbi_combined_fb_dead_ends(grhip_trellis_viterbi_combined_fb *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_fb_work(grhip_trellis_viterbi_combined_fb *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_fb_work_device(grhip_trellis_viterbi_combined_fb *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_fs grhip_trellis_viterbi_combined_fs;
GRHIP_API int grhip_trellis_viterbi_combined_fs_create(grhip_trellis_viterbi_combined_fs **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_fs_destroy(grhip_trellis_viterbi_combined_fs *h);
GRHIP_API int grhip_trellis_viterbi_combined_fs_set_mode(grhip_trellis_viterbi_combined_fs *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_fs_set_streams(grhip_trellis_viterbi_combined_fs *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_fs_set_TABLE(grhip_trellis_viterbi_combined_fs *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_fs_set_engine(grhip_trellis_viterbi_combined_fs *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_fs_engine(grhip_trellis_viterbi_combined_fs *h);
GRHIP_API int grhip_trellis_viterbi_combined_fs_D(grhip_trellis_viterbi_combined_fs *h);
GRHIP_API int grhip_trellis_viterbi_combined_fs_TYPE(grhip_trellis_viterbi_combined_fs *h);
GRHIP_API int grhip_trellis_viterbi_combined_fs_K(grhip_trellis_viterbi_combined_fs *h);
GRHIP_API int grhip_trellis_viterbi_combined_fs_S0(grhip_trellis_viterbi_combined_fs *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_fs_SK(grhip_trellis_viterbi_combined_fs *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_fs_resident_blocks(grhip_trellis_viterbi_combined_fs *h);
GRHIP_API int grhip_trellis_viterbi_combined_fs_blocks_per_wavefront(grhip_trellis_viterbi_combined_fs *h);
GRHIP_API int grhip_trellis_viterbi_combined_fs_workspace_bytes(grhip_trellis_viterbi_combined_fs *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_fs_trace_window(grhip_trellis_viterbi_combined_fs *h);
GRHIP_API int grhip_trellis_viterbi_combined_fs_dead_ends(grhip_trellis_viterbi_combined_fs *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_fs_work(grhip_trellis_viterbi_combined_fs *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_fs_work_device(grhip_trellis_viterbi_combined_fs *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_fi grhip_trellis_viterbi_combined_fi;
GRHIP_API int grhip_trellis_viterbi_combined_fi_create(grhip_trellis_viterbi_combined_fi **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_fi_destroy(grhip_trellis_viterbi_combined_fi *h);
GRHIP_API int grhip_trellis_viterbi_combined_fi_set_mode(grhip_trellis_viterbi_combined_fi *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_fi_set_streams(grhip_trellis_viterbi_combined_fi *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_fi_set_TABLE(grhip_trellis_viterbi_combined_fi *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_fi_set_engine(grhip_trellis_viterbi_combined_fi *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_fi_engine(grhip_trellis_viterbi_combined_fi *h);
GRHIP_API int grhip_trellis_viterbi_combined_fi_D(grhip_trellis_viterbi_combined_fi *h);
GRHIP_API int grhip_trellis_viterbi_combined_fi_TYPE(grhip_trellis_viterbi_combined_fi *h);
GRHIP_API int grhip_trellis_viterbi_combined_fi_K(grhip_trellis_viterbi_combined_fi *h);
GRHIP_API int grhip_trellis_viterbi_combined_fi_S0(grhip_trellis_viterbi_combined_fi *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_fi_SK(grhip_trellis_viterbi_combined_fi *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_fi_resident_blocks(grhip_trellis_viterbi_combined_fi *h);
GRHIP_API int grhip_trellis_viterbi_combined_fi_blocks_per_wavefront(grhip_trellis_viterbi_combined_fi *h);
GRHIP_API int grhip_trellis_viterbi_combined_fi_workspace_bytes(grhip_trellis_viterbi_combined_fi *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_fi_trace_window(grhip_trellis_viterbi_combined_fi *h);
GRHIP_API int grhip_trellis_viterbi_combined_fi_dead_ends(grhip_trellis_viterbi_combined_fi *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_fi_work(grhip_trellis_viterbi_combined_fi *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_fi_work_device(grhip_trellis_viterbi_combined_fi *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_cb grhip_trellis_viterbi_combined_cb;
GRHIP_API int grhip_trellis_viterbi_combined_cb_create(grhip_trellis_viterbi_combined_cb **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_cb_destroy(grhip_trellis_viterbi_combined_cb *h);
GRHIP_API int grhip_trellis_viterbi_combined_cb_set_mode(grhip_trellis_viterbi_combined_cb *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_cb_set_streams(grhip_trellis_viterbi_combined_cb *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_cb_set_TABLE(grhip_trellis_viterbi_combined_cb *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_cb_set_engine(grhip_trellis_viterbi_combined_cb *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_cb_engine(grhip_trellis_viterbi_combined_cb *h);
GRHIP_API int grhip_trellis_viterbi_combined_cb_D(grhip_trellis_viterbi_combined_cb *h);
GRHIP_API int grhip_trellis_viterbi_combined_cb_TYPE(grhip_trellis_viterbi_combined_cb *h);
GRHIP_API int grhip_trellis_viterbi_combined_cb_K(grhip_trellis_viterbi_combined_cb *h);
GRHIP_API int grhip_trellis_viterbi_combined_cb_S0(grhip_trellis_viterbi_combined_cb *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_cb_SK(grhip_trellis_viterbi_combined_cb *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_cb_resident_blocks(grhip_trellis_viterbi_combined_cb *h);
GRHIP_API int grhip_trellis_viterbi_combined_cb_blocks_per_wavefront(grhip_trellis_viterbi_combined_cb *h);
GRHIP_API int grhip_trellis_viterbi_combined_cb_workspace_bytes(grhip_trellis_viterbi_combined_cb *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_cb_trace_window(grhip_trellis_viterbi_combined_cb *h);
GRHIP_API int grhip_trellis_viterbi_combined_cb_dead_ends(grhip_trellis_viterbi_combined_cb *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_cb_work(grhip_trellis_viterbi_combined_cb *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_cb_work_device(grhip_trellis_viterbi_combined_cb *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_cs grhip_trellis_viterbi_combined_cs;
GRHIP_API int grhip_trellis_viterbi_combined_cs_create(grhip_trellis_viterbi_combined_cs **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_cs_destroy(grhip_trellis_viterbi_combined_cs *h);
GRHIP_API int grhip_trellis_viterbi_combined_cs_set_mode(grhip_trellis_viterbi_combined_cs *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_cs_set_streams(grhip_trellis_viterbi_combined_cs *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_cs_set_TABLE(grhip_trellis_viterbi_combined_cs *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_cs_set_engine(grhip_trellis_viterbi_combined_cs *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_cs_engine(grhip_trellis_viterbi_combined_cs *h);
GRHIP_API int grhip_trellis_viterbi_combined_cs_D(grhip_trellis_viterbi_combined_cs *h);
GRHIP_API int grhip_trellis_viterbi_combined_cs_TYPE(grhip_trellis_viterbi_combined_cs *h);
GRHIP_API int grhip_trellis_viterbi_combined_cs_K(grhip_trellis_viterbi_combined_cs *h);
GRHIP_API int grhip_trellis_viterbi_combined_cs_S0(grhip_trellis_viterbi_combined_cs *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_cs_SK(grhip_trellis_viterbi_combined_cs *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_cs_resident_blocks(grhip_trellis_viterbi_combined_cs *h);
GRHIP_API int grhip_trellis_viterbi_combined_cs_blocks_per_wavefront(grhip_trellis_viterbi_combined_cs *h);
GRHIP_API int grhip_trellis_viterbi_combined_cs_workspace_bytes(grhip_trellis_viterbi_combined_cs *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_cs_trace_window(grhip_trellis_viterbi_combined_cs *h);
GRHIP_API int grhip_trellis_viterbi_combined_cs_dead_ends(grhip_trellis_viterbi_combined_cs *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_cs_work(grhip_trellis_viterbi_combined_cs *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_cs_work_device(grhip_trellis_viterbi_combined_cs *h, int n, const void *d_in, void *d_out, void *stream);
typedef struct grhip_trellis_viterbi_combined_ci grhip_trellis_viterbi_combined_ci;
GRHIP_API int grhip_trellis_viterbi_combined_ci_create(grhip_trellis_viterbi_combined_ci **h, const grhip_fsm *fsm, int K, int S0, int SK, int D, const void *TABLE,
    int n_TABLE, int TYPE, int device);
GRHIP_API void grhip_trellis_viterbi_combined_ci_destroy(grhip_trellis_viterbi_combined_ci *h);
GRHIP_API int grhip_trellis_viterbi_combined_ci_set_mode(grhip_trellis_viterbi_combined_ci *h, int mode);
GRHIP_API int grhip_trellis_viterbi_combined_ci_set_streams(grhip_trellis_viterbi_combined_ci *h, int nstreams);
GRHIP_API int grhip_trellis_viterbi_combined_ci_set_TABLE(grhip_trellis_viterbi_combined_ci *h, const void *TABLE, int n_TABLE);
GRHIP_API int grhip_trellis_viterbi_combined_ci_set_engine(grhip_trellis_viterbi_combined_ci *h, int engine);
GRHIP_API int grhip_trellis_viterbi_combined_ci_engine(grhip_trellis_viterbi_combined_ci *h);
GRHIP_API int grhip_trellis_viterbi_combined_ci_D(grhip_trellis_viterbi_combined_ci *h);
GRHIP_API int grhip_trellis_viterbi_combined_ci_TYPE(grhip_trellis_viterbi_combined_ci *h);
GRHIP_API int grhip_trellis_viterbi_combined_ci_K(grhip_trellis_viterbi_combined_ci *h);
GRHIP_API int grhip_trellis_viterbi_combined_ci_S0(grhip_trellis_viterbi_combined_ci *h, int *S0);
GRHIP_API int grhip_trellis_viterbi_combined_ci_SK(grhip_trellis_viterbi_combined_ci *h, int *SK);
GRHIP_API int grhip_trellis_viterbi_combined_ci_resident_blocks(grhip_trellis_viterbi_combined_ci *h);
GRHIP_API int grhip_trellis_viterbi_combined_ci_blocks_per_wavefront(grhip_trellis_viterbi_combined_ci *h);
GRHIP_API int grhip_trellis_viterbi_combined_ci_workspace_bytes(grhip_trellis_viterbi_combined_ci *h, unsigned long long *bytes);
GRHIP_API int grhip_trellis_viterbi_combined_ci_trace_window(grhip_trellis_viterbi_combined_ci *h);
GRHIP_API int grhip_trellis_viterbi_combined_ci_dead_ends(grhip_trellis_viterbi_combined_ci *h, long long *count);
GRHIP_API int grhip_trellis_viterbi_combined_ci_work(grhip_trellis_viterbi_combined_ci *h, int n, const void *in, void *out);
GRHIP_API int grhip_trellis_viterbi_combined_ci_work_device(grhip_trellis_viterbi_combined_ci *h, int n, const void *d_in, void *d_out, void *stream);

/* ---- small device-memory helpers for hosts without a HIP binding -------- */
GRHIP_API int grhip_malloc(void **d_ptr, size_t bytes, int device);
GRHIP_API int grhip_free(void *d_ptr);
GRHIP_API int grhip_memcpy_h2d(void *d_dst, const void *src, size_t bytes);
GRHIP_API int grhip_memcpy_d2h(void *dst, const void *d_src, size_t bytes);
GRHIP_API int grhip_stream_synchronize(void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INCLUDED_GRHIP_H */
