// The tables of vpz_pcm_logmel (include/vorbispizza_pcm_logmel.h states the definition): host code only, no device, so that
// tests/test_logmel_cpu.py can hold vpz_logmel_dft_table and vpz_mel_filterbank to a float64 restatement.  Every value is evaluated in
// double and rounded once to float32.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "../../include/vorbispizza_pcm_logmel.h"

namespace vpz {

inline bool logmel_nfft_ok(int64_t n_fft) { return n_fft >= VPZ_LOGMEL_MIN_NFFT && n_fft <= VPZ_LOGMEL_MAX_NFFT && n_fft % 2 == 0; }

// every field but n_fft inside the limits of the definition (`floor` only where the output mode reads it): what vpz_pcm_logmel and
// vpz_pcm_melspec (melspec_tables.hpp), which differ in the transform sizes they take, ask alike
inline bool mel_spec_rest_ok(const vpz_logmel_spec &s)
{
    if (s.n_fft < 1 || s.hop < 1 || s.hop > s.n_fft || s.n_mels < 1 || s.n_mels > VPZ_LOGMEL_MAX_MELS) return false;
    if (!(s.sample_rate > 0.0) || !isfinite(s.sample_rate) || !(s.f_min >= 0.0) || !(s.f_min < s.f_max) || !(s.f_max <= s.sample_rate / 2.0))
        return false;
    if (s.mel_scale != VPZ_MEL_HTK && s.mel_scale != VPZ_MEL_SLANEY) return false;
    if (s.mel_norm != VPZ_MEL_NORM_NONE && s.mel_norm != VPZ_MEL_NORM_SLANEY) return false;
    if (s.output != VPZ_MEL_POWER && s.output != VPZ_MEL_LOG10) return false;
    if (s.layout != VPZ_MEL_BANDS_FIRST && s.layout != VPZ_MEL_FRAMES_FIRST) return false;
    if (s.output == VPZ_MEL_LOG10 && (!((float)s.floor > 0.0f) || !isfinite((float)s.floor))) return false;
    for (int i = 0; i < 9; ++i)
        if (s.reserved[i] != 0) return false;
    return true;
}

inline bool logmel_spec_ok(const vpz_logmel_spec &s) { return logmel_nfft_ok(s.n_fft) && mel_spec_rest_ok(s); }

// table[m][0 .. nb) = w[m] cos, table[m][nb .. 2 nb) = w[m] sin, nb = n_fft / 2 + 1; `ld` floats between two rows (>= 2 * nb), the sin
// columns start at column `sin_at` (>= nb): the exported table is dense (ld = 2 nb, sin_at = nb), the device copy pads both halves
inline void logmel_dft_fill(int n_fft, float *table, size_t ld, size_t sin_at)
{
    const double two_pi = 6.283185307179586476925286766559;
    const int nb = n_fft / 2 + 1;
    for (int m = 0; m < n_fft; ++m) {
        const double w = 0.5 - 0.5 * cos(two_pi * (double)m / (double)n_fft);
        float *row = table + (size_t)m * ld;
        for (int k = 0; k < nb; ++k) {
            const int64_t j = ((int64_t)m * k) % n_fft;
            const double a = two_pi * (double)j / (double)n_fft;
            // (on the axes the values are exact, not the 1e-16 that cos and sin give at a rounded multiple of pi / 2: the sin columns of
            // k = 0 and k = n_fft / 2 are zeros)
            const double c = 4 * j == n_fft || 4 * j == 3 * (int64_t)n_fft ? 0.0 : cos(a), s = j == 0 || 2 * j == n_fft ? 0.0 : sin(a);
            row[k] = (float)(w * c);
            row[sin_at + (size_t)k] = (float)(w * s);
        }
    }
}

inline double mel_of_hz(double f, int scale)
{
    if (scale == VPZ_MEL_HTK) return 2595.0 * log10(1.0 + f / 700.0);
    if (f < 1000.0) return f / (200.0 / 3.0);
    return 15.0 + log(f / 1000.0) / (log(6.4) / 27.0);
}

inline double hz_of_mel(double mel, int scale)
{
    if (scale == VPZ_MEL_HTK) return 700.0 * (pow(10.0, mel / 2595.0) - 1.0);
    if (mel < 15.0) return mel * (200.0 / 3.0);
    return 1000.0 * exp((log(6.4) / 27.0) * (mel - 15.0));
}

struct MelFilterbank {
    std::vector<int32_t> first, count;  // [n_mels]
    std::vector<float> weights;         // band after band, each band's live bins
    int32_t most = 0;                   // the largest live-bin count of a band
};

// (the caller has checked the spec)
inline void mel_build(const vpz_logmel_spec &s, MelFilterbank &fb)
{
    const int nb = s.n_fft / 2 + 1, n = s.n_mels;
    std::vector<double> pts((size_t)n + 2);
    const double m_lo = mel_of_hz(s.f_min, s.mel_scale), m_hi = mel_of_hz(s.f_max, s.mel_scale);
    for (int i = 0; i < n + 2; ++i) pts[(size_t)i] = hz_of_mel(m_lo + (m_hi - m_lo) * (double)i / (double)(n + 1), s.mel_scale);
    fb.first.assign((size_t)n, 0);
    fb.count.assign((size_t)n, 0);
    fb.weights.clear();
    fb.most = 0;
    for (int b = 0; b < n; ++b) {
        const double f0 = pts[(size_t)b], f1 = pts[(size_t)b + 1], f2 = pts[(size_t)b + 2];
        const double scale = s.mel_norm == VPZ_MEL_NORM_SLANEY ? 2.0 / (f2 - f0) : 1.0;
        int first = -1, last = -1;
        for (int k = 0; k < nb; ++k) {
            const double fk = (double)k * s.sample_rate / (double)s.n_fft;
            const double up = (fk - f0) / (f1 - f0), down = (f2 - fk) / (f2 - f1);
            const double w = up < down ? up : down;
            if (w > 0.0) {
                if (first < 0) first = k;
                last = k;
            }
        }
        if (first < 0) continue;
        fb.first[(size_t)b] = first;
        fb.count[(size_t)b] = last - first + 1;
        if (last - first + 1 > fb.most) fb.most = last - first + 1;
        for (int k = first; k <= last; ++k) {
            const double fk = (double)k * s.sample_rate / (double)s.n_fft;
            const double up = (fk - f0) / (f1 - f0), down = (f2 - fk) / (f2 - f1);
            const double w = up < down ? up : down;
            fb.weights.push_back((float)((w > 0.0 ? w : 0.0) * scale));
        }
    }
}

// what vpz_mel_filterbank and vpz_melspec_filterbank return for a spec each has checked against its own limits
inline int mel_filterbank_out(const vpz_logmel_spec &spec, int32_t *first_bin, int32_t *n_bins, float *weights, int64_t capacity, int64_t *total)
{
    MelFilterbank fb;
    try {
        mel_build(spec, fb);
    } catch (const std::bad_alloc &) {
        return VPZ_E_NOMEM;
    }
    if (total) *total = (int64_t)fb.weights.size();
    if (first_bin) memcpy(first_bin, fb.first.data(), sizeof(int32_t) * fb.first.size());
    if (n_bins) memcpy(n_bins, fb.count.data(), sizeof(int32_t) * fb.count.size());
    if (!weights) return VPZ_OK;
    if ((uint64_t)capacity < fb.weights.size()) return VPZ_E_CAPACITY;
    if (!fb.weights.empty()) memcpy(weights, fb.weights.data(), sizeof(float) * fb.weights.size());
    return VPZ_OK;
}

}  // namespace vpz
