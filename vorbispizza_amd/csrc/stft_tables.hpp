// The table of vpz_pcm_stft (include/vorbispizza_pcm_stft.h states the definition): host code only, no device, so that
// tests/test_stft_cpu.py can hold vpz_stft_table to a float64 restatement.  Every value is evaluated in double and rounded once to
// float32.  The twiddles are melspec_tables.hpp's twiddle_fill.
#pragma once
#include <math.h>
#include <stdint.h>

#include "melspec_tables.hpp"
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

// table[0 .. n) = w[m]: g over win_length, centred in n; table[n ..) = the twiddles: 3 n floats
inline void stft_table_fill(int n, int win_length, int window, float *table)
{
    const double two_pi = 6.283185307179586476925286766559;
    const int left = (n - win_length) / 2;
    const double a0 = window == VPZ_STFT_HAMMING ? 0.54 : 0.5, a1 = window == VPZ_STFT_HAMMING ? 0.46 : 0.5;
    for (int m = 0; m < n; ++m) {
        const int j = m - left;
        table[m] = j < 0 || j >= win_length ? 0.0f : (float)(a0 - a1 * cos(two_pi * (double)j / (double)win_length));
    }
    twiddle_fill(n, table + n);
}

}  // namespace vpz
