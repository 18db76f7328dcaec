// trellis_metric.h -- calc_metric's arithmetic (gr-trellis/src/lib/calc_metric.cc:29-72, :212-250) as device functions,
// shared by the metrics kernels (trellis.hip) and the combined decoder (trellis_viterbi.hip): statement for statement with
// the round-to-nearest intrinsics, so nothing contracts.  Not part of the ABI.
#pragma once
#include <cfloat>

#include "trellis.h"

namespace grhip {

struct tr_cplx { float re, im; };

// metric += s * s with T s = in - table, in T's arithmetic (calc_metric.cc:41-44)
__device__ inline float metric_term(float acc, float x, float t)
{
    const float s = __fsub_rn(x, t);
    return __fadd_rn(acc, __fmul_rn(s, s));
}
__device__ inline float metric_term(float acc, short x, short t)
{
    const short s = (short)((int)x - (int)t);                       // truncated to short; the product is an int
    return __fadd_rn(acc, (float)((int)s * (int)s));
}
__device__ inline float metric_term(float acc, int x, int t)
{
    const unsigned s = (unsigned)x - (unsigned)t;                   // the two's-complement wrap of both statements
    return __fadd_rn(acc, (float)(int)(s * s));
}
__device__ inline float metric_term(float acc, tr_cplx x, tr_cplx t)   // :223-224
{
    const float re = __fsub_rn(x.re, t.re), im = __fsub_rn(x.im, t.im);
    return __fadd_rn(acc, __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)));
}

template <class T>
__device__ inline float metric_of(const T *x, const T *table, int o, int D)
{
    float m = 0.0f;
    for (int d = 0; d < D; ++d) m = metric_term(m, x[d], table[(size_t)o * D + d]);
    return m;
}

// metric[o] of one step as `type` defines it: the sum, or 0 for the first minimum of the sums in o order from FLT_MAX and
// 1 elsewhere (:48-65)
template <class T>
__device__ inline float metric_entry(const T *x, const T *table, int o, int O, int D, int type)
{
    if (type == TRELLIS_EUCLIDEAN) return metric_of(x, table, o, D);
    float minm = FLT_MAX;
    int minmi = 0;
    for (int q = 0; q < O; ++q) {
        const float m = metric_of(x, table, q, D);
        if (m < minm) { minm = m; minmi = q; }
    }
    return o == minmi ? 0.0f : 1.0f;
}

// the same for an item type known at run time (TR_S, TR_I, TR_F, TR_C)
__device__ inline float metric_entry_any(int t, const void *x, const void *table, int o, int O, int D, int type)
{
    switch (t) {
    case TR_S: return metric_entry((const short *)x, (const short *)table, o, O, D, type);
    case TR_I: return metric_entry((const int *)x, (const int *)table, o, O, D, type);
    case TR_C: return metric_entry((const tr_cplx *)x, (const tr_cplx *)table, o, O, D, type);
    default: return metric_entry((const float *)x, (const float *)table, o, O, D, type);
    }
}

}  // namespace grhip
