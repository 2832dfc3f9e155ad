// The cepstral matrix of vpz_pcm_mfcc (include/vorbispizza_pcm_mfcc.h states the definition): host code only, no device, so that
// tests/test_mfcc_cpu.py can hold vpz_mfcc_table to a float64 restatement.  Every value is evaluated in double and rounded once to float32.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fbank_tables.hpp"
#include "../../include/vorbispizza_pcm_mfcc.h"

namespace vpz {

// every field inside the limits of the definition
inline bool mfcc_spec_ok(const vpz_mfcc_spec &s)
{
    if (!fbank_spec_ok(s.fbank) || s.fbank.output != VPZ_FBANK_LOG) return false;
    if (s.n_ceps < 1 || s.n_ceps > s.fbank.n_mels) return false;
    if (!(s.lifter >= 0.0) || !isfinite(s.lifter) || !(s.energy_floor >= 0.0) || !isfinite(s.energy_floor)) return false;
    for (int32_t flag : {s.use_energy, s.htk_compat, s.subtract_mean})
        if (flag != 0 && flag != 1) return false;
    for (int i = 0; i < 12; ++i)
        if (s.reserved[i] != 0) return false;
    return true;
}

// C[i][b] of the definition's item 2: the lifter times Kaldi's DCT, times sqrt(2) for HTK's C0
inline float mfcc_weight(const vpz_mfcc_spec &s, int i, int b)
{
    const double pi = 3.141592653589793238462643383279, N = (double)s.fbank.n_mels;
    const double dct = i == 0 ? sqrt(1.0 / N) : sqrt(2.0 / N) * cos(pi * (double)i * ((double)b + 0.5) / N);
    const double lift = s.lifter > 0.0 ? 1.0 + 0.5 * s.lifter * sin(pi * (double)i / s.lifter) : 1.0;
    return (float)(lift * dct * (s.htk_compat && !s.use_energy && i == 0 ? sqrt(2.0) : 1.0));
}

// the coefficient a frame's j-th stored value holds (item 4)
inline int mfcc_stored(const vpz_mfcc_spec &s, int j) { return !s.htk_compat ? j : j == s.n_ceps - 1 ? 0 : j + 1; }

}  // namespace vpz
