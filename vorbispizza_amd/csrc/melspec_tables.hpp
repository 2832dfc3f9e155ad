// The tables of vpz_pcm_melspec (include/vorbispizza_pcm_melspec.h states the definition): host code only, no device, so that
// tests/test_melspec_cpu.py can hold vpz_melspec_twiddles and vpz_melspec_filterbank to a float64 restatement.  Every value is evaluated
// in double and rounded once to float32.  The filterbank and every limit but n_fft's are logmel_tables.hpp's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "logmel_tables.hpp"
#include "../../include/vorbispizza_pcm_melspec.h"

namespace vpz {

inline bool melspec_nfft_ok(int64_t n_fft) { return n_fft == 2048 || n_fft == 4096 || n_fft == 8192; }

inline bool melspec_spec_ok(const vpz_logmel_spec &s) { return melspec_nfft_ok(s.n_fft) && mel_spec_rest_ok(s); }

// out[2k], out[2k + 1] = cos, -sin of 2 pi k / n, k = 0 .. n-1: the twiddles of the real FFT, vpz_pcm_stft's (stft_tables.hpp) as well
inline void twiddle_fill(int n, float *out)
{
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < n; ++k) {
        const double a = two_pi * (double)k / (double)n;
        // (on the axes the values are exact, not the 1e-16 that cos and sin give at a rounded multiple of pi / 2; no -0.0 either)
        const double c = 4 * k == n || 4 * k == 3 * n ? 0.0 : cos(a), s = k == 0 || 2 * k == n ? 0.0 : -sin(a);
        out[2 * k] = (float)c;
        out[2 * k + 1] = (float)s;
    }
}

// table[0 .. n) = w[m]; table[n ..) = the twiddles: 3 n floats
inline void melspec_twiddle_fill(int n, float *table)
{
    const double two_pi = 6.283185307179586476925286766559;
    for (int m = 0; m < n; ++m) table[m] = (float)(0.5 - 0.5 * cos(two_pi * (double)m / (double)n));
    twiddle_fill(n, table + n);
}

}  // namespace vpz
