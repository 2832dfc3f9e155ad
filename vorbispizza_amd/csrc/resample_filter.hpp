// The coefficient table of vpz_pcm_resample (include/vorbispizza_pcm_resample.h states the filter): host code only, no device, so that
// tests/test_resample_cpu.py can hold vpz_resample_filter -- or this header compiled into a program of its own -- to a float64
// restatement.  Everything that decides WHICH taps exist is integer arithmetic; a coefficient is evaluated in double and rounded once.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace vpz {

constexpr int64_t kResampleMaxUp = 1024, kResampleMaxDownPerUp = 32;

inline int64_t resample_gcd(int64_t a, int64_t b)
{
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// a ratio in lowest terms inside the limits
inline bool resample_ratio_ok(int64_t up, int64_t down)
{
    return up >= 1 && down >= 1 && up <= kResampleMaxUp && down <= kResampleMaxDownPerUp * up && resample_gcd(up, down) == 1;
}

// |s * u| < 6 for u = n / up, s = 0.99 * min(up, down) / down, in integers
inline bool resample_tap_live(int64_t n, int64_t up, int64_t down)
{
    const int64_t a = n < 0 ? -n : n, lo = up < down ? up : down;
    return a * 99 * lo < 600 * up * down;
}

// h(n / up)
inline double resample_h(int64_t n, int64_t up, int64_t down)
{
    const double pi = 3.14159265358979323846;
    const double s = 0.99 * (double)(up < down ? up : down) / (double)down;
    const double x = s * (double)n / (double)up;
    const double w = cos(pi * x / 12.0);
    const double a = pi * x;
    return s * (n == 0 ? 1.0 : sin(a) / a) * w * w;
}

struct ResampleFilter {
    int32_t up = 0, down = 0, taps = 0;
    std::vector<int32_t> first;  // [up]: the first live tap of a phase, relative to floor(j * down / up)
    std::vector<float> coeff;    // [up][taps], zeros behind a phase's live taps
};

// false: a refused ratio
inline bool resample_build(int64_t up, int64_t down, ResampleFilter &f)
{
    if (!resample_ratio_ok(up, down)) return false;
    f.up = (int32_t)up;
    f.down = (int32_t)down;
    f.first.assign((size_t)up, 0);
    if (up == down) {  // (1:1 in lowest terms: the copy)
        f.taps = 1;
        f.coeff.assign(1, 1.0f);
        return true;
    }
    const int64_t lo = up < down ? up : down;
    const int64_t reach = (600 * down + 99 * lo - 1) / (99 * lo) + 1;  // no tap lies further than this from floor(j * down / up)
    std::vector<int32_t> count((size_t)up, 0);
    f.taps = 0;
    for (int64_t p = 0; p < up; ++p) {
        const int64_t r = (p * down) % up;  // j * down = q * up + r for every j of phase p
        int64_t d = -reach;
        while (!resample_tap_live(d * up - r, up, down)) ++d;  // (d = 0 is live: r < up and the support is wider than one sample)
        f.first[(size_t)p] = (int32_t)d;
        while (resample_tap_live(d * up - r, up, down)) ++d;
        count[(size_t)p] = (int32_t)(d - f.first[(size_t)p]);
        if (count[(size_t)p] > f.taps) f.taps = count[(size_t)p];
    }
    f.coeff.assign((size_t)up * (size_t)f.taps, 0.0f);
    for (int64_t p = 0; p < up; ++p) {
        const int64_t r = (p * down) % up;
        for (int32_t k = 0; k < count[(size_t)p]; ++k)
            f.coeff[(size_t)p * (size_t)f.taps + (size_t)k] = (float)resample_h((f.first[(size_t)p] + k) * up - r, up, down);
    }
    return true;
}

}  // namespace vpz
