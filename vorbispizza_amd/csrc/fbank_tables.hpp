// The tables of vpz_pcm_fbank (include/vorbispizza_pcm_fbank.h states the definition): host code only, no device, so that
// tests/test_fbank_cpu.py can hold vpz_fbank_table and vpz_fbank_filterbank to a float64 restatement.  Every value is evaluated in
// double and rounded once to float32.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/vorbispizza_pcm_fbank.h"

namespace vpz {

// the upper edge of the mel bank: high_freq itself, or an offset from the Nyquist frequency
inline double fbank_high(const vpz_fbank_spec &s) { return s.high_freq > 0.0 ? s.high_freq : s.sample_rate / 2.0 + s.high_freq; }

// every field inside the limits of the definition (`floor` only where the output mode reads it)
inline bool fbank_spec_ok(const vpz_fbank_spec &s)
{
    if (s.n_fft < VPZ_FBANK_MIN_NFFT || s.n_fft > VPZ_FBANK_MAX_NFFT || s.n_fft % 2 != 0) return false;
    if (s.win < 2 || s.win > s.n_fft || s.hop < 1 || s.hop > s.win || s.n_mels < 1 || s.n_mels > VPZ_FBANK_MAX_MELS) return false;
    if (!(s.sample_rate > 0.0) || !isfinite(s.sample_rate) || !isfinite(s.high_freq)) return false;
    if (!(s.low_freq >= 0.0) || !(s.low_freq < fbank_high(s)) || !(fbank_high(s) <= s.sample_rate / 2.0)) return false;
    if (!(s.preemphasis >= 0.0) || !(s.preemphasis <= 1.0)) return false;
    if (!isfinite((float)s.scale) || (float)s.scale == 0.0f || !isfinite((float)s.pad_value)) return false;
    if (s.window != VPZ_FBANK_HANNING && s.window != VPZ_FBANK_HAMMING && s.window != VPZ_FBANK_POVEY) return false;
    if (s.remove_dc != 0 && s.remove_dc != 1) return false;
    if (s.output != VPZ_FBANK_POWER && s.output != VPZ_FBANK_LOG) return false;
    if (s.layout != VPZ_FBANK_BANDS_FIRST && s.layout != VPZ_FBANK_FRAMES_FIRST) return false;
    if (s.output == VPZ_FBANK_LOG && (!((float)s.floor > 0.0f) || !isfinite((float)s.floor))) return false;
    for (int i = 0; i < 10; ++i)
        if (s.reserved[i] != 0) return false;
    return true;
}

inline double fbank_window(int window, int m, int win)
{
    const double two_pi = 6.283185307179586476925286766559;
    const double c = cos(two_pi * (double)m / (double)(win - 1));
    if (window == VPZ_FBANK_HAMMING) return 0.54 - 0.46 * c;
    const double hann = 0.5 - 0.5 * c;
    return window == VPZ_FBANK_POVEY ? pow(hann, 0.85) : hann;
}

// Steps 1, 3, 4 and 5 of the definition as one matrix: with y = x - mu,
//     re[k] = sum_m z[m] w[m] cos(m k),  z[0] = (1 - c) y[0],  z[m] = y[m] - c y[m-1]
// collects y[m] in  w[m] cos(m k) - c w[m+1] cos((m+1) k)  (the second term absent for m = win - 1), and y[0] once more in -c w[0];
// times `scale`.  table[m][0 .. nb) the cos part, table[m][sin_at .. sin_at + nb) the sin part, nb = n_fft / 2, `ld` floats between two
// rows: the exported table is dense (ld = 2 nb, sin_at = nb), the device copy pads both halves (the caller has zeroed the padding)
inline void fbank_table_fill(const vpz_fbank_spec &s, float *table, size_t ld, size_t sin_at)
{
    const double two_pi = 6.283185307179586476925286766559;
    const int n_fft = s.n_fft, nb = n_fft / 2, win = s.win;
    const double c = s.preemphasis;
    // (on the axes the values are exact, not the 1e-16 that cos and sin give at a rounded multiple of pi / 2)
    auto cs = [&](int m, int k, double *co, double *si) {
        const int64_t j = ((int64_t)m * k) % n_fft;
        const double a = two_pi * (double)j / (double)n_fft;
        *co = 4 * j == n_fft || 4 * j == 3 * (int64_t)n_fft ? 0.0 : cos(a);
        *si = j == 0 || 2 * j == n_fft ? 0.0 : sin(a);
    };
    for (int m = 0; m < win; ++m) {
        const double w0 = fbank_window(s.window, m, win), w1 = m + 1 < win ? fbank_window(s.window, m + 1, win) : 0.0;
        float *row = table + (size_t)m * ld;
        for (int k = 0; k < nb; ++k) {
            double c0, s0, c1 = 0.0, s1 = 0.0;
            cs(m, k, &c0, &s0);
            if (m + 1 < win) cs(m + 1, k, &c1, &s1);
            double vc = w0 * c0 - c * w1 * c1, vs = w0 * s0 - c * w1 * s1;
            if (m == 0) vc -= c * w0;  // (z[0] = y[0] - c y[0]: frame sample 0 stands in for the one before it)
            row[k] = (float)(s.scale * vc);
            row[sin_at + (size_t)k] = (float)(s.scale * vs);
        }
    }
}

inline double fbank_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }

struct FbankBank {
    std::vector<int32_t> first, count;  // [n_mels]
    std::vector<float> weights;         // band after band, each band's live bins
};

// (the caller has checked the spec)
inline void fbank_bank_build(const vpz_fbank_spec &s, FbankBank &fb)
{
    const int nb = s.n_fft / 2, n = s.n_mels;
    const double m_lo = fbank_mel(s.low_freq), m_hi = fbank_mel(fbank_high(s)), d = (m_hi - m_lo) / (double)(n + 1);
    std::vector<double> mk((size_t)nb);
    for (int k = 0; k < nb; ++k) mk[(size_t)k] = fbank_mel((double)k * s.sample_rate / (double)s.n_fft);
    fb.first.assign((size_t)n, 0);
    fb.count.assign((size_t)n, 0);
    fb.weights.clear();
    for (int b = 0; b < n; ++b) {
        const double left = m_lo + (double)b * d, right = left + 2.0 * d;
        auto weight = [&](int k) {
            const double up = (mk[(size_t)k] - left) / d, down = (right - mk[(size_t)k]) / d;
            return up < down ? up : down;
        };
        int first = -1, last = -1;
        for (int k = 0; k < nb; ++k)
            if (weight(k) > 0.0) {
                if (first < 0) first = k;
                last = k;
            }
        if (first < 0) continue;
        fb.first[(size_t)b] = first;
        fb.count[(size_t)b] = last - first + 1;
        for (int k = first; k <= last; ++k) {
            const double w = weight(k);
            fb.weights.push_back((float)(w > 0.0 ? w : 0.0));
        }
    }
}

}  // namespace vpz
