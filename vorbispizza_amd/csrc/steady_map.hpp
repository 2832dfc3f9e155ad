// The index maps of steady_stereo_kernel (steady_stereo.hip): where the values a lane holds after the 2048-point
// transform's last twiddle belong, so that a steady frame -- a 2048 block after a 2048 block, long windows on both sides -- is
// overlap-added in the lanes, with no h in LDS.
//
// imdct2048_wave_x2_spectrum (imdct_core.hpp) leaves in lane l, register q, with j = l + 64 q:
//   A = Re W[j] = h[2j]          B = -Im W[j] = h[1023 - 2j]          (h[m] = y[512 + m], m in [0, 1024))
// h[0:512) is what this frame adds to the PCM, h[512:1024) what the NEXT frame overlaps with (its "tail", tail[i] = h[512 + i]):
//   q < 4  : A is the current value h[k], k = 2j;         B the tail value tail[511 - 2j]
//   q >= 4 : B is the current value h[k], k = 1023 - 2j;  A the tail value tail[2j - 512]
// A current value h[k] makes two samples of the frame's 1024: 511 - k (negated, mirrored half) and 512 + k, and both are
// overlapped with tail_prev[511 - k] -- which is the tail index of the SAME lane and register.  The two samples' window values are
// slope[511 - k] and slope[512 + k], each the other's partner (slope[s] and slope[1023 - s]).
// Lane (l, q) and lane (63 - l, 7 - q) hold neighbouring samples: each keeps one, sends the other, and stores a pair.
#pragma once

namespace vpz {
namespace steady {

constexpr int kLanes = 64, kRegs = 8;
constexpr int point(int lane, int q) { return lane + 64 * q; }
// the tail value a (lane, register) leaves for the next frame, as an index into the natural-order tail (state_h's order)
constexpr int tail_index(int lane, int q) { return q < 4 ? 511 - 2 * point(lane, q) : 2 * point(lane, q) - 512; }
// the current value h[k] a (lane, register) holds
constexpr int cur_index(int lane, int q) { return q < 4 ? 2 * point(lane, q) : 1023 - 2 * point(lane, q); }
// the two samples of a current value h[k]
constexpr int sample_lo(int k) { return 511 - k; }   // -h[k] x slope[511 - k] + tail_prev[511 - k] x slope[512 + k]
constexpr int sample_hi(int k) { return 512 + k; }   //  h[k] x slope[512 + k] + tail_prev[511 - k] x slope[511 - k]
// the sample a (lane, register) keeps (the even one of its pair) and the one it sends to (63 - lane, 7 - q)
constexpr int kept_sample(int lane, int q) { return q < 4 ? sample_hi(cur_index(lane, q)) : sample_lo(cur_index(lane, q)); }
constexpr int sent_sample(int lane, int q) { return q < 4 ? sample_lo(cur_index(lane, q)) : sample_hi(cur_index(lane, q)); }
// where the pair (kept, received) is stored: 8 bytes per lane, a register's wave-store one contiguous 512-byte span
constexpr int store_index(int lane, int q) { return q < 4 ? 512 + 2 * point(lane, q) : 2 * point(lane, q) - 512; }

constexpr bool sweep()
{
    bool tail_seen[512] = {}, sample_seen[1024] = {};
    for (int q = 0; q < kRegs; ++q)
        for (int l = 0; l < kLanes; ++l) {
            const int t = tail_index(l, q), k = cur_index(l, q);
            if (t < 0 || t >= 512 || tail_seen[t]) return false;  // the tails: a permutation of 0 .. 511
            tail_seen[t] = true;
            if (k < 0 || k >= 512) return false;
            if (t != 511 - k) return false;  // the tail both samples need is the one this (lane, register) made a frame earlier
            const int a = sample_lo(k), b = sample_hi(k);
            if (a < 0 || a >= 512 || b < 512 || b >= 1024 || sample_seen[a] || sample_seen[b]) return false;
            sample_seen[a] = sample_seen[b] = true;  // the samples: a permutation of 0 .. 1023
            // the swap partner: its sent sample is the one after this one's kept sample, and the pair is stored where it lies
            const int pl = 63 - l, pq = 7 - q;
            if (kept_sample(l, q) & 1) return false;
            if (sent_sample(pl, pq) != kept_sample(l, q) + 1) return false;
            if (store_index(l, q) != kept_sample(l, q)) return false;
            // what the transform leaves: A = h[2j], B = h[1023 - 2j]; one of them is the current value, the other the tail value
            const int j = point(l, q), ia = 2 * j, ib = 1023 - 2 * j;
            if (q < 4 ? (ia != k || ib != 512 + t) : (ib != k || ia != 512 + t)) return false;
        }
    for (int i = 0; i < 512; ++i)
        if (!tail_seen[i]) return false;
    for (int i = 0; i < 1024; ++i)
        if (!sample_seen[i]) return false;
    return true;
}
static_assert(sweep(), "steady_stereo_kernel's index maps: tails a permutation of 0..511, samples of 0..1023, swap partners (63 - l, 7 - q)");

}  // namespace steady
}  // namespace vpz
