// The bins and kernels of vpz_pcm_cqt (include/vorbispizza_pcm_cqt.h states the definition): host code only, no device, so that
// tests/test_cqt_cpu.py can hold vpz_cqt_bins and vpz_cqt_kernel to a float64 restatement.  Every value is evaluated in double, in the
// order the header writes it, and rounded once to float32.
#pragma once
#include <math.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "../../include/vorbispizza_pcm_cqt.h"

namespace vpz {

struct CqtBins {
    std::vector<double> f;   // f_k
    std::vector<int32_t> n;  // N_k: never longer than the bin before it
};

// f_k and N_k; false: a field outside the limits of the definition
inline bool cqt_bins(const vpz_cqt_spec &s, CqtBins *out)
{
    if (!(s.sample_rate > 0.0) || !(s.f_min > 0.0) || !(s.filter_scale > 0.0) || !(s.gamma >= 0.0)) return false;  // (a NaN fails every one)
    if (!isfinite(s.sample_rate) || !isfinite(s.f_min) || !isfinite(s.filter_scale) || !isfinite(s.gamma)) return false;
    if (s.n_bins < 1 || s.n_bins > VPZ_CQT_MAX_BINS || s.bins_per_octave < 1 || s.bins_per_octave > VPZ_CQT_MAX_BINS_PER_OCTAVE) return false;
    if (s.hop < 1 || s.hop > VPZ_CQT_MAX_HOP) return false;
    if (s.window != VPZ_CQT_HANN && s.window != VPZ_CQT_HAMMING) return false;
    if (s.scale != VPZ_CQT_SCALE_NONE && s.scale != VPZ_CQT_SCALE_SQRT_LENGTH) return false;
    if (s.pad != VPZ_CQT_PAD_REFLECT && s.pad != VPZ_CQT_PAD_ZERO) return false;
    if (s.output != VPZ_CQT_COMPLEX && s.output != VPZ_CQT_MAGNITUDE && s.output != VPZ_CQT_POWER) return false;
    if (s.layout != VPZ_CQT_BINS_FIRST && s.layout != VPZ_CQT_FRAMES_FIRST) return false;
    for (int32_t r : s.reserved)
        if (r != 0) return false;
    const double B = (double)s.bins_per_octave;
    const double alpha = exp2(1.0 / B) - 1.0, Q = s.filter_scale / alpha;
    CqtBins b;
    b.f.resize((size_t)s.n_bins);
    b.n.resize((size_t)s.n_bins);
    for (int k = 0; k < s.n_bins; ++k) {
        const double f = s.f_min * exp2((double)k / B);
        const double len = ceil(Q * s.sample_rate / (f + s.gamma / alpha));
        if (!(f <= s.sample_rate / 2.0) || !(len >= 2.0) || !(len <= (double)VPZ_CQT_MAX_LENGTH)) return false;
        b.f[(size_t)k] = f;
        b.n[(size_t)k] = (int32_t)len;
    }
    if (out) *out = std::move(b);
    return true;
}

// hr[j * stride], hi[j * stride], j = 0 .. n-1, of a bin at f with n taps
inline void cqt_kernel_fill(const vpz_cqt_spec &s, double f, int n, float *hr, float *hi, size_t stride)
{
    const double two_pi = 6.283185307179586476925286766559;
    const double a0 = s.window == VPZ_CQT_HAMMING ? 0.54 : 0.5, a1 = s.window == VPZ_CQT_HAMMING ? 0.46 : 0.5;
    std::vector<double> g((size_t)n);
    double G = 0.0;
    for (int j = 0; j < n; ++j) {
        g[(size_t)j] = a0 - a1 * cos(two_pi * (double)j / (double)n);
        G += g[(size_t)j];
    }
    const double sk = s.scale == VPZ_CQT_SCALE_SQRT_LENGTH ? sqrt((double)n) / G : 1.0 / G;
    const int half = n / 2;
    for (int j = 0; j < n; ++j) {
        const double phi = two_pi * f * (double)(j - half) / s.sample_rate, sg = sk * g[(size_t)j];
        hr[(size_t)j * stride] = (float)(sg * cos(phi));
        hi[(size_t)j * stride] = (float)(-(sg * sin(phi)));
    }
}

}  // namespace vpz
