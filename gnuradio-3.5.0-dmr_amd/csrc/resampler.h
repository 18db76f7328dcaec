// resampler.h -- launcher of the rational-resampler kernel (csrc/resampler.hip), used by csrc/capi_resampler.hip
// for gr_rational_resampler_base_XXX and gr_interp_fir_filter_XXX.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace grhip {

enum RsKind { RS_CCF = 0, RS_FFF = 1, RS_CCC = 2 };

constexpr int RS_THREADS = 256;
constexpr size_t RS_LDS_SOFT = 48 * 1024;      // tiles are sized to this when they can be (several workgroups per CU)
constexpr size_t RS_LDS_MAX = 160 * 1024;      // and never beyond the CU's LDS

// One launch of the closed form.  Output o (0 <= o < nout) of a call that starts at ctr = c0 uses filter
// (c0 + o*D) % I at logical input (c0 + o*D) / I.  The logical input is `lead` zeros, then n_phys items at `in`.
// With g = gcd(I, D), P = I/g and Dp = D/g, output o = m*P + r (period m, residue r) uses filter f_r = (c0 + r*D) % I
// at s_r + m*Dp, s_r = (c0 + r*D) / I: the filter depends on r alone.
struct RsLaunch {
    const void *in = nullptr;
    long long in_stride = 0, lead = 0, n_phys = 0;
    void *out = nullptr;
    long long out_stride = 0, nout = 0;
    int n_streams = 1;
    const void *bank = nullptr;     // [I + 1][RS] taps (float, or float2 for ccc): row f = WP zeros, the reversed taps
                                    // of filter f, WP zeros; row I is all zeros
    unsigned long long I = 1, D = 1, c0 = 0;
    int P = 1, Dp = 1, nt = 1, WP = 0, RS = 1;
};

// the tiling of one launch (rs_config)
struct RsConfig {
    int RG = 1;                 // residues per wave task (kernel template)
    int RB = 1;                 // residues per workgroup
    int TM = 64;                // periods per workgroup (64 per wave task)
    int span_cap = 0;           // input items a workgroup reads, at most
    int L = 0;                  // LDS row of one input phase (items); the input image is Dp rows
    size_t lds = 0;             // dynamic LDS bytes
};

// residues per wave task of the FAST kernel for P residues (the GENERIC kernel takes one)
int rs_group(int P, bool generic);

// Tiling of a kind/shape, or GRHIP_EINVAL when no tile fits the LDS.  nperiods (> 0) lets small launches use smaller
// tiles; pass 0 for the worst case (the check at create).
int rs_config(RsKind kind, bool generic, unsigned long long I, unsigned long long D, int nt, long long nperiods,
              RsConfig *cfg);

// Raise the kernels' dynamic-LDS limit on the CURRENT device (the attribute is per device).
int rs_prepare_device(RsKind kind);

int rs_launch(RsKind kind, bool generic, const RsLaunch &a, hipStream_t st);

// install_taps (gr_rational_resampler_base_XXX.cc.t:102-120) as RsLaunch::bank: `padded` holds a multiple of I taps of
// w floats each; filter f gets padded[f + k*I], reversed as gr_fir_XXX::set_taps stores them.  Row f = WP zeros, the
// reversed taps, WP zeros; row I zeros.  Leaves the taps per filter and the pad in *nt and *WP.
inline std::vector<float> rs_bank(const std::vector<float> &padded, int w, unsigned long long I, unsigned long long D,
                                  unsigned long long P, int *nt, int *WP)
{
    const size_t n = padded.size() / w;
    *nt = (int)(n / I);
    *WP = (int)(((unsigned long long)(rs_group((int)std::min<unsigned long long>(P, 64), false) - 1) * D + I - 1) / I);
    const size_t RS = (size_t)*nt + 2 * (size_t)*WP;
    std::vector<float> bank((I + 1) * RS * w, 0.f);
    for (unsigned long long f = 0; f < I; ++f)
        for (int k = 0; k < *nt; ++k) {
            const size_t src = f + (size_t)(*nt - 1 - k) * I;
            for (int c = 0; c < w; ++c) bank[(f * RS + *WP + k) * w + c] = padded[src * w + c];
        }
    return bank;
}

}  // namespace grhip
