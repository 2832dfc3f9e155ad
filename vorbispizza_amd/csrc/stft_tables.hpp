// The table of vpz_pcm_stft (include/vorbispizza_pcm_stft.h states the definition): host code only, no device, so that
// tests/test_stft_cpu.py can hold vpz_stft_table to a float64 restatement.  Every value is evaluated in double and rounded once to
// float32.  The twiddles are melspec_tables.hpp's, value for value.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/vorbispizza_pcm_stft.h"

namespace vpz {

inline bool stft_nfft_ok(int64_t n_fft) { return n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096 || n_fft == 8192; }

inline bool stft_table_ok(int64_t n_fft, int64_t win_length, int64_t window)
{
    return stft_nfft_ok(n_fft) && win_length >= 2 && win_length <= n_fft && (window == VPZ_STFT_HANN || window == VPZ_STFT_HAMMING);
}

// every field inside the limits of the definition
inline bool stft_spec_ok(const vpz_stft_spec &s)
{
    if (!stft_table_ok(s.n_fft, s.win_length, s.window) || s.hop < 1 || s.hop > s.n_fft) return false;
    if (s.output != VPZ_STFT_COMPLEX && s.output != VPZ_STFT_MAGNITUDE && s.output != VPZ_STFT_POWER) return false;
    if (s.layout != VPZ_STFT_BINS_FIRST && s.layout != VPZ_STFT_FRAMES_FIRST) return false;
    for (int32_t r : s.reserved)
        if (r != 0) return false;
    return true;
}

// table[0 .. n) = w[m]: g over win_length, centred in n; table[n + 2k], table[n + 2k + 1] = cos, -sin of 2 pi k / n, k = 0 .. n-1: 3 n floats
inline void stft_table_fill(int n, int win_length, int window, float *table)
{
    const double two_pi = 6.283185307179586476925286766559;
    const int left = (n - win_length) / 2;
    const double a0 = window == VPZ_STFT_HAMMING ? 0.54 : 0.5, a1 = window == VPZ_STFT_HAMMING ? 0.46 : 0.5;
    for (int m = 0; m < n; ++m) {
        const int j = m - left;
        table[m] = j < 0 || j >= win_length ? 0.0f : (float)(a0 - a1 * cos(two_pi * (double)j / (double)win_length));
    }
    for (int k = 0; k < n; ++k) {
        const double a = two_pi * (double)k / (double)n;
        // (on the axes the values are exact, not the 1e-16 that cos and sin give at a rounded multiple of pi / 2; no -0.0 either)
        const double c = 4 * k == n || 4 * k == 3 * n ? 0.0 : cos(a), s = k == 0 || 2 * k == n ? 0.0 : -sin(a);
        table[n + 2 * k] = (float)c;
        table[n + 2 * k + 1] = (float)s;
    }
}

}  // namespace vpz
