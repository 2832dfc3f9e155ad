// vpz_pcm_true_peak (include/vorbispizza_pcm_r128.h, which states the definition): the true peak -- the largest magnitude of the F-times
// oversampled signal -- and the sample peak of windows of an interleaved float32 device PCM array; vpz_true_peak_filter,
// vpz_loudness_range and vpz_loudness_maxima, host only.
//
// The mapping.  An interleaved window is ONE run of floats: element e = i * C + c, and output position i of channel c reads the elements
// e, e - C, .. e - 11 C.  So a TILE is kTpTile consecutive ELEMENTS of a row's (L + 11) * C output elements, whatever the channel count:
// no channel groups and no edges between them; a tile may begin in the middle of a sample.  A workgroup of kTpBlock lanes stages its
// tile into LDS with a halo of 11 * C elements in front, consecutive lanes on consecutive addresses, and everything outside [0, L * C)
// as zero -- what lies around a window in the source array is another member.  Lane t then takes the elements t, t + kTpBlock, .. of
// the tile: its twelve values lie at lds[halo + e - k * C], consecutive lanes on consecutive banks at every k, and it computes the
// F - 1 phases from that one set, each a chain of one multiply and eleven fused multiply-adds, k ascending.  The 36 (F = 4) or 12 (F = 2)
// coefficients are a kernel argument by value: scalar registers.  The identity phase is the element itself, which is also the sample
// peak; at F = 1 nothing else is computed.  The workgroup reduces its maxima through DPP shuffles and eight floats of LDS and leaves one
// pair (true, sample) per tile in the context's scratch; true_peak_finish, one wave per descriptor, takes the maximum of a row's pairs
// and writes the row once.  A maximum of non-negative floats has no order, fmaxf passes a NaN over: a row's bits do not depend on the
// launch around it.  No atomics, no private scratch memory.  LDS: kTpTile + 11 * C + 8 floats, 27.6 KB at 255 channels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "../../include/vorbispizza_pcm_r128.h"

namespace vpz {

namespace {

constexpr int kTpBlock = 256;     // lanes of a workgroup
constexpr int kTpTile = 4096;     // output elements (position * channels + channel) of a tile
constexpr int kTpTaps = 12;       // per phase (VPZ_TRUE_PEAK_TAPS)
constexpr int kTpMaxGridY = 4096; // descriptors side by side in the grid's y; a workgroup takes every kTpMaxGridY-th beyond that
static_assert(kTpTaps == VPZ_TRUE_PEAK_TAPS && kTpTile % kTpBlock == 0 && kTpBlock % 64 == 0, "the mapping's premises");

// a descriptor's tiles, uploaded behind the descriptors in records of their size (upload_rows): its pairs are base .. base + tiles - 1
struct RowTiles {
    int64_t base, tiles, elems;  // elems = (L + 11) * C where L > 0, else 0
};
static_assert(sizeof(RowTiles) == sizeof(vpz_pack_row), "RowTiles rides in upload_rows' records");

template <int F>
struct TpCoeffs {  // a kernel argument, by value: c[p - 1][k] = (float)h[p + k F]
    float c[F > 1 ? F - 1 : 1][kTpTaps];
};

__device__ __forceinline__ float wave_max(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

template <int F>
__global__ __launch_bounds__(kTpBlock) void true_peak_tiles(const float *__restrict__ src, const vpz_pack_row *__restrict__ rows,
                                                            const RowTiles *__restrict__ tiles, int n_rows, int C, TpCoeffs<F> h,
                                                            float2 *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [halo + kTpTile], then the waves' maxima
    const int lane = threadIdx.x;
    const int halo = (kTpTaps - 1) * C;
    float *wave_part = lds + halo + kTpTile;
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const RowTiles u = tiles[r];
        if ((int64_t)blockIdx.x >= u.tiles) continue;  // (the same for every lane of the workgroup)
        const vpz_pack_row d = rows[r];
        const int64_t live = d.samples * C;                   // elements of the window
        const int64_t e0 = (int64_t)blockIdx.x * kTpTile;    // the tile's first output element
        const int count = (int)min((int64_t)kTpTile, u.elems - e0);
        const float *in = src + d.src;
        __syncthreads();  // (the tile before has been consumed)
        for (int s = lane; s < halo + count; s += kTpBlock) {
            const int64_t e = e0 - halo + s;
            lds[s] = e >= 0 && e < live ? in[e] : 0.0f;
        }
        __syncthreads();
        float tp = 0.0f, sp = 0.0f;
        for (int t = lane; t < count; t += kTpBlock) {
            const float *p = lds + halo + t;
            float x[kTpTaps];
#pragma unroll
            for (int k = 0; k < kTpTaps; ++k) x[k] = p[-k * C];
            sp = fmaxf(sp, fabsf(x[0]));
            if (F > 1) {
#pragma unroll
                for (int ph = 0; ph < F - 1; ++ph) {
                    float a = h.c[ph][0] * x[0];
#pragma unroll
                    for (int k = 1; k < kTpTaps; ++k) a = __builtin_fmaf(h.c[ph][k], x[k], a);
                    tp = fmaxf(tp, fabsf(a));
                }
            }
        }
        tp = wave_max(fmaxf(tp, sp));
        sp = wave_max(sp);
        if ((lane & 63) == 0) {
            wave_part[2 * (lane >> 6)] = tp;
            wave_part[2 * (lane >> 6) + 1] = sp;
        }
        __syncthreads();
        if (lane == 0) {
            for (int w = 1; w < kTpBlock / 64; ++w) {
                tp = fmaxf(tp, wave_part[2 * w]);
                sp = fmaxf(sp, wave_part[2 * w + 1]);
            }
            part[u.base + blockIdx.x] = make_float2(tp, sp);
        }
    }
}

// one wave per descriptor: the maximum of its tiles' pairs; a row without tiles (an empty window) gets zeros
__global__ __launch_bounds__(64) void true_peak_finish(const vpz_pack_row *__restrict__ rows, const RowTiles *__restrict__ tiles, int n_rows,
                                                       const float2 *__restrict__ part, float *__restrict__ true_peak,
                                                       float *__restrict__ sample_peak)
{
    for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const RowTiles u = tiles[r];
        float tp = 0.0f, sp = 0.0f;
        for (int64_t t = threadIdx.x; t < u.tiles; t += 64) {
            const float2 v = part[u.base + t];
            tp = fmaxf(tp, v.x);
            sp = fmaxf(sp, v.y);
        }
        tp = wave_max(tp);
        sp = wave_max(sp);
        if (threadIdx.x == 0) {
            const int64_t row = rows[r].row;
            true_peak[row] = tp;
            if (sample_peak) sample_peak[row] = sp;
        }
    }
}

int32_t factor_of(int32_t fs) { return fs < 96000 ? 4 : fs < 192000 ? 2 : 1; }

// the interpolator of a factor, as the header states it
void interpolator_of(int32_t F, double h[VPZ_TRUE_PEAK_MAX_COEFFS])
{
    const double pi = 3.14159265358979323846;
    const int N = kTpTaps * F + 1;
    for (int j = 0; j < VPZ_TRUE_PEAK_MAX_COEFFS; ++j) h[j] = 0.0;
    for (int j = 0; j < N; ++j) {
        const int m = j - (kTpTaps / 2) * F;
        if (m % F == 0) {
            h[j] = m == 0 ? 1.0 : 0.0;  // (by definition: sin(pi k) is not 0 in double)
            continue;
        }
        const double t = (double)m / F;
        h[j] = sin(pi * t) / (pi * t) * 0.5 * (1.0 - cos(2.0 * pi * j / (N - 1)));
    }
}

template <int F>
TpCoeffs<F> coeffs_of()
{
    double h[VPZ_TRUE_PEAK_MAX_COEFFS];
    interpolator_of(F, h);
    TpCoeffs<F> c;
    memset(&c, 0, sizeof c);
    for (int p = 1; p < F; ++p)
        for (int k = 0; k < kTpTaps; ++k) c.c[p - 1][k] = (float)h[p + k * F];
    return c;
}

template <int F>
void launch_tiles(Context *ctx, dim3 grid, size_t lds_bytes, const float *src, const vpz_pack_row *d_rows, const RowTiles *d_tiles, int n_rows, int C,
                  float2 *part)
{
    true_peak_tiles<F><<<grid, kTpBlock, lds_bytes, ctx->stream>>>(src, d_rows, d_tiles, n_rows, C, coeffs_of<F>(), part);
}

// p = total / (blocks' samples); l = -0.691 + 10 log10 p: the level of a block of `len` steps from step k on, the sum taken i ascending
double block_power(const double *sums, int64_t k, int len, int32_t step_len)
{
    double total = 0.0;
    for (int i = 0; i < len; ++i) total += sums[k + i];
    return total / ((double)len * (double)step_len);
}
double level_of(double p) { return -0.691 + 10.0 * log10(p); }

}  // namespace

}  // namespace vpz

extern "C" int vpz_true_peak_filter(int32_t sample_rate, int32_t *factor, double h[49])
{
    if (!factor || !h || sample_rate < VPZ_LOUDNESS_MIN_RATE || sample_rate > VPZ_LOUDNESS_MAX_RATE) return VPZ_E_INVALID_ARG;
    *factor = vpz::factor_of(sample_rate);
    vpz::interpolator_of(*factor, h);
    return VPZ_OK;
}

extern "C" int vpz_loudness_range(const double *sums, int64_t n_steps, int32_t step_len, double *range, double *low, double *high,
                                  int64_t *blocks_kept)
{
    if (!range || n_steps < 0 || step_len < 1 || (!sums && n_steps > 0)) return VPZ_E_INVALID_ARG;
    *range = 0.0;
    if (low) *low = -HUGE_VAL;
    if (high) *high = -HUGE_VAL;
    if (blocks_kept) *blocks_kept = 0;
    const int64_t blocks = n_steps - 29;
    if (blocks < 1) return VPZ_OK;
    std::vector<double> p, kept;
    try {
        p.resize((size_t)blocks);
        kept.reserve((size_t)blocks);
    } catch (const std::bad_alloc &) {
        return VPZ_E_NOMEM;
    }
    // the absolute gate (a NaN level fails the comparison)
    double total = 0.0;
    int64_t passed = 0;
    for (int64_t k = 0; k < blocks; ++k) {
        p[(size_t)k] = vpz::block_power(sums, k, 30, step_len);
        if (vpz::level_of(p[(size_t)k]) > -70.0) {
            total += p[(size_t)k];
            ++passed;
        }
    }
    if (passed == 0) return VPZ_OK;
    const double relative = vpz::level_of(total / (double)passed) - 20.0;
    // the relative gate, among those
    for (int64_t k = 0; k < blocks; ++k) {
        const double l = vpz::level_of(p[(size_t)k]);
        if (l > -70.0 && l > relative) kept.push_back(l);
    }
    if (kept.empty()) return VPZ_OK;
    std::sort(kept.begin(), kept.end());
    const double m1 = (double)(kept.size() - 1);
    const double lo = kept[(size_t)floor(0.10 * m1 + 0.5)], hi = kept[(size_t)floor(0.95 * m1 + 0.5)];
    *range = hi - lo;
    if (low) *low = lo;
    if (high) *high = hi;
    if (blocks_kept) *blocks_kept = (int64_t)kept.size();
    return VPZ_OK;
}

extern "C" int vpz_loudness_maxima(const double *sums, int64_t n_steps, int32_t step_len, double *momentary_max, double *short_term_max)
{
    if ((!momentary_max && !short_term_max) || n_steps < 0 || step_len < 1 || (!sums && n_steps > 0)) return VPZ_E_INVALID_ARG;
    const int lens[2] = {4, 30};
    double *const outs[2] = {momentary_max, short_term_max};
    for (int which = 0; which < 2; ++which) {
        if (!outs[which]) continue;
        double most = -HUGE_VAL;
        for (int64_t k = 0; k + lens[which] <= n_steps; ++k) {
            const double l = vpz::level_of(vpz::block_power(sums, k, lens[which], step_len));
            if (l > most) most = l;  // (a NaN level fails the comparison)
        }
        *outs[which] = most;
    }
    return VPZ_OK;
}

extern "C" int vpz_pcm_true_peak(vpz_context *c, const void *src_dev, int64_t src_elems, int32_t channels, int32_t sample_rate, int32_t n_rows,
                                 const vpz_pack_row *rows, float *true_peak_dev, float *sample_peak_dev, int64_t dst_rows)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (channels < 1 || channels > VPZ_MAX_CHANNELS) return refuse("vpz_pcm_true_peak: channels outside 1..VPZ_MAX_CHANNELS");
    if (sample_rate < VPZ_LOUDNESS_MIN_RATE || sample_rate > VPZ_LOUDNESS_MAX_RATE) return refuse("vpz_pcm_true_peak: a sample rate outside the limits");
    // (a window has no cap on its length: `frames` caps nothing)
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_true_peak", src_dev, src_elems, sizeof(float), channels, 1, 1, INT64_MAX, n_rows, rows,
                                                       true_peak_dev, dst_rows, (unsigned __int128)1, sizeof(float)});
    // (the sample peaks: the same shape; the descriptors have been looked at)
    if (rc == VPZ_OK && sample_peak_dev)
        rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_true_peak (sample peak)", src_dev, src_elems, sizeof(float), channels, 1, 1, INT64_MAX, 0, rows,
                                                       sample_peak_dev, dst_rows, (unsigned __int128)1, sizeof(float)});
    if (rc != VPZ_OK || n_rows == 0) return rc;
    if (n_rows > 0x3fffff00) return refuse("vpz_pcm_true_peak: too many descriptors for one launch");

    // what goes up in upload_rows' records: the descriptors, then their tiles
    std::vector<vpz_pack_row> up;
    try {
        up.resize(2 * (size_t)n_rows);
    } catch (const std::bad_alloc &) {
        return vpz::set_error(ctx, VPZ_E_NOMEM, "vpz_pcm_true_peak: out of host memory");
    }
    memcpy(up.data(), rows, sizeof(vpz_pack_row) * (size_t)n_rows);
    int64_t total = 0, most_tiles = 0;
    for (int32_t r = 0; r < n_rows; ++r) {
        // (samples * channels <= src_elems: 11 more samples cannot overflow)
        const int64_t elems = rows[r].samples > 0 ? (rows[r].samples + vpz::kTpTaps - 1) * channels : 0;
        const vpz::RowTiles u{total, (elems + vpz::kTpTile - 1) / vpz::kTpTile, elems};
        memcpy(&up[(size_t)n_rows + r], &u, sizeof u);
        total += u.tiles;
        most_tiles = std::max(most_tiles, u.tiles);
    }
    if (most_tiles > 0x7fffffff) return refuse("vpz_pcm_true_peak: a row too long for one launch");
    rc = ctx->tp_scratch.grow(ctx, (size_t)total * sizeof(float2) + 64, "vpz_pcm_true_peak: hipMalloc(scratch)");
    if (rc != VPZ_OK) return rc;
    float2 *part = static_cast<float2 *>(ctx->tp_scratch.p);

    const vpz_pack_row *d_up = nullptr;
    rc = vpz::upload_rows(ctx, (int32_t)up.size(), up.data(), &d_up);
    if (rc != VPZ_OK) return rc;
    const vpz::RowTiles *d_tiles = reinterpret_cast<const vpz::RowTiles *>(d_up + n_rows);

    const float *src = static_cast<const float *>(src_dev);
    const unsigned grid_y = (unsigned)std::min<int64_t>(n_rows, vpz::kTpMaxGridY);
    const size_t lds_bytes = ((size_t)(vpz::kTpTaps - 1) * channels + vpz::kTpTile + 2 * (vpz::kTpBlock / 64)) * sizeof(float);
    if (most_tiles > 0) {
        const dim3 grid((unsigned)most_tiles, grid_y);
        const int32_t F = vpz::factor_of(sample_rate);
        if (F == 4) vpz::launch_tiles<4>(ctx, grid, lds_bytes, src, d_up, d_tiles, n_rows, channels, part);
        else if (F == 2) vpz::launch_tiles<2>(ctx, grid, lds_bytes, src, d_up, d_tiles, n_rows, channels, part);
        else vpz::launch_tiles<1>(ctx, grid, lds_bytes, src, d_up, d_tiles, n_rows, channels, part);
    }
    vpz::true_peak_finish<<<grid_y, 64, 0, ctx->stream>>>(d_up, d_tiles, n_rows, part, true_peak_dev, sample_peak_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "pcm_true_peak kernel launch", e);
    return VPZ_OK;
}
