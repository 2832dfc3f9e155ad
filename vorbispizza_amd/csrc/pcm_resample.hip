// vpz_pcm_resample and vpz_resample_filter (include/vorbispizza_pcm_resample.h, which states the filter): windows of a device PCM array
// at one sample rate, optionally mixed down to mono, as a dense, zero-padded batch in device memory.
//
// The mapping:
//   a TILE is kRsBlock consecutive output samples [j0, j0 + kRsBlock) of one destination row, all its output channels; one workgroup per
//   tile and descriptor, one lane per output sample, so consecutive lanes are consecutive phases p = j mod up;
//   the tile's SOURCE SPAN -- source samples floor(j0 * down / up) + first_min up to the last tap of the tile's last output -- is staged
//   in LDS, de-interleaved (channel cc at stage[cc * span_cap ..]) or already mixed to mono, with coalesced loads; a sample outside the
//   window's [0, L) is staged as ZERO and never read: what lies around a window in the source array is the roll and the next member;
//   as many channels are staged side by side as kRsLds holds (`per_pass`, all of them at the usual ratios, one at the steepest), the
//   others in further passes over the same tile; the LDS is dynamic, sized by the launch for its ratio (8 KiB for stereo at 160 / 441);
//   a lane accumulates its output's taps in float32 -- coefficients [tap][phase], so a wave reads a tap's coefficients in one line --,
//   and the results of a pass leave through LDS so that the interleaved layouts store consecutive elements from consecutive lanes too.
//   Tiles behind a window's J outputs store the row's zeros; a tile computes nothing it does not store.
// All element indices are 64-bit.  No scratch memory.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "device_table.hpp"
#include "resample_filter.hpp"
#include "synth_common.hpp"
#include "../../include/vorbispizza_pcm_resample.h"

namespace vpz {

namespace {

constexpr int kRsBlock = 256;       // outputs of a tile, lanes of a workgroup
constexpr int kRsLds = 8704;        // floats a pass stages at the most: one channel's span at the steepest ratio, rounded up
constexpr int kRsMaxTaps = 388;     // the support is |d - r / up| < 6 / s <= 6 * 32 / 0.99 = 193.94: an open interval shorter than 388
// a tile's span is at most (kRsBlock - 1) * down / up + 2 + taps samples (vpz_pcm_resample, below), and down <= 32 * up: one channel always fits
static_assert((kRsBlock - 1) * (int)kResampleMaxDownPerUp + 2 + kRsMaxTaps <= kRsLds, "the steepest ratio's span must fit the LDS stage");
constexpr int kRsMaxPass = 8;       // channels staged side by side at most (the results' LDS is sized for it)
constexpr int kRsMaxGridY = 4096;   // descriptors side by side in the grid's y; a workgroup takes every kRsMaxGridY-th beyond that

struct ResampleArgs {
    const float *src;
    const vpz_pack_row *rows;
    void *dst;
    const float *coeff;    // [taps][up]
    const int32_t *first;  // [up]
    int64_t frames;
    int32_t n_rows, channels, out_channels, downmix, up, down, taps, first_min;
    int32_t span_cap, per_pass;  // floats between two staged channels; channels of a pass
};

__device__ __forceinline__ void put(float *p, float v) { *p = v; }
__device__ __forceinline__ void put(int16_t *p, float v) { *p = (int16_t)to_s16(v); }

template <typename T, bool kPlanar>
__global__ __launch_bounds__(kRsBlock) void pcm_resample_kernel(const ResampleArgs a)
{
    // dynamic LDS, sized by the launch for its ratio: `per_pass` channels' spans, then `per_pass` channels' results of the tile
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *stage = lds, *outs = lds + (size_t)a.per_pass * a.span_cap;
    const int t = threadIdx.x;
    const int C = a.channels, Co = a.out_channels, up = a.up, down = a.down, taps = a.taps;
    const int64_t j0 = (int64_t)blockIdx.x * kRsBlock, j = j0 + t, frames = a.frames;
    const int nj = (int)(frames - j0 < kRsBlock ? frames - j0 : kRsBlock);  // the tile's elements of a run (the grid covers `frames`)
    T *dst = static_cast<T *>(a.dst);
    const float inv_c = 1.0f / (float)C;
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_pack_row d = a.rows[r];
        const int64_t L = d.samples, J = (L * up + down - 1) / down;
        const bool work = j0 < J;  // (the same for the whole workgroup)
        int64_t m_lo = 0;
        int span = 0, rel = 0, p = 0;
        if (work) {
            const int64_t jl = (J < j0 + kRsBlock ? J : j0 + kRsBlock) - 1;  // the tile's last output
            m_lo = j0 * down / up + a.first_min;
            span = (int)(jl * down / up + a.first_min + 1 + taps - m_lo);  // (a phase's first tap is first_min or first_min + 1) <= span_cap
            if (j < J) {
                p = (int)(j % up);
                rel = (int)(j * down / up + a.first[p] - m_lo);
            }
        }
        const float *in = a.src + d.src;
        for (int c0 = 0; c0 < Co; c0 += a.per_pass) {
            const int cn = Co - c0 < a.per_pass ? Co - c0 : a.per_pass;
            if (work && a.downmix) {
                for (int i = t; i < span; i += kRsBlock) {
                    const int64_t m = m_lo + i;
                    float v = 0.0f;
                    if (m >= 0 && m < L) {
                        const float *f = in + m * C;
                        v = f[0];
                        for (int c = 1; c < C; ++c) v += f[c];
                        v *= inv_c;
                    }
                    stage[i] = v;
                }
            } else if (work) {
                const int n = span * cn;
                for (int i = t; i < n; i += kRsBlock) {
                    const int mi = i / cn, cc = i - mi * cn;
                    const int64_t m = m_lo + mi;
                    stage[cc * a.span_cap + mi] = m >= 0 && m < L ? in[m * C + c0 + cc] : 0.0f;
                }
            }
            __syncthreads();
            for (int cc = 0; cc < cn; ++cc) {
                float acc = 0.0f;
                if (work && j < J) {
                    const float *s = stage + cc * a.span_cap + rel;
                    const float *h = a.coeff + p;
                    acc = s[0];  // (up == down, 1:1 in lowest terms: the copy, a sample's bits as they are)
                    if (up != down) {
                        acc *= h[0];
                        for (int k = 1; k < taps; ++k) acc = __builtin_fmaf(h[(int64_t)k * up], s[k], acc);
                    }
                }
                outs[cc * kRsBlock + t] = acc;
            }
            __syncthreads();
            if (kPlanar) {
                if (t < nj)
                    for (int cc = 0; cc < cn; ++cc) put(dst + (d.row * Co + c0 + cc) * frames + j, outs[cc * kRsBlock + t]);
            } else {
                const int n = nj * cn;
                for (int i = t; i < n; i += kRsBlock) {
                    const int tt = i / cn, cc = i - tt * cn;
                    put(dst + (d.row * frames + j0 + tt) * Co + c0 + cc, outs[cc * kRsBlock + tt]);
                }
            }
            // (the next pass writes `stage` at once and `outs` behind its first barrier: every lane has read both by then)
        }
    }
}

// the context's device copy of a ratio's table, built on first use: the coefficients by tap, the phases' first taps behind them
int ratio_table(Context *ctx, int up, int down, const Context::ResampleTable **out)
{
    return table_for(ctx, ctx->resample_tables, std::make_pair(up, down), "vpz_pcm_resample: out of host memory", out, [&](Context::ResampleTable &tb) {
        ResampleFilter f;
        if (!resample_build(up, down, f)) return set_error(ctx, VPZ_E_INVALID_ARG, "vpz_pcm_resample: a refused ratio");
        std::vector<float> by_tap(f.coeff.size());
        for (int p = 0; p < up; ++p)
            for (int k = 0; k < f.taps; ++k) by_tap[(size_t)k * (size_t)up + (size_t)p] = f.coeff[(size_t)p * (size_t)f.taps + (size_t)k];
        tb.taps = f.taps;
        tb.first_min = *std::min_element(f.first.begin(), f.first.end());
        return upload(ctx, "vpz_pcm_resample: coefficient table upload", tb,
                      {{by_tap.data(), by_tap.size() * sizeof(float), reinterpret_cast<void **>(&tb.d_coeff)},
                       {f.first.data(), f.first.size() * sizeof(int32_t), reinterpret_cast<void **>(&tb.d_first)}});
    });
}

}  // namespace

}  // namespace vpz

extern "C" int vpz_resample_filter(int32_t up, int32_t down, int32_t *taps, int32_t *first_tap, float *coeffs, int64_t capacity)
{
    if (!taps || capacity < 0 || !vpz::resample_ratio_ok(up, down)) return VPZ_E_INVALID_ARG;
    vpz::ResampleFilter f;
    try {
        if (!vpz::resample_build(up, down, f)) return VPZ_E_INVALID_ARG;
    } catch (const std::bad_alloc &) {
        return VPZ_E_NOMEM;
    }
    *taps = f.taps;
    if (first_tap) memcpy(first_tap, f.first.data(), sizeof(int32_t) * f.first.size());
    if (!coeffs) return VPZ_OK;
    if ((uint64_t)capacity < f.coeff.size()) return VPZ_E_CAPACITY;
    memcpy(coeffs, f.coeff.data(), sizeof(float) * f.coeff.size());
    return VPZ_OK;
}

extern "C" int vpz_pcm_resample(vpz_context *c, const void *src_dev, int64_t src_elems, int32_t channels, int32_t up, int32_t down,
                                int32_t downmix, int32_t n_rows, const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows,
                                int32_t out_channels, int64_t frames, int32_t dst_layout)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (channels < 1 || channels > VPZ_MAX_CHANNELS) return refuse("vpz_pcm_resample: channels outside 1..VPZ_MAX_CHANNELS");
    if (downmix != 0 && downmix != 1) return refuse("vpz_pcm_resample: downmix is 0 or 1");
    if (out_channels != (downmix ? 1 : channels)) return refuse("vpz_pcm_resample: out_channels is `channels`, or 1 with downmix");
    if (!vpz::resample_ratio_ok(up, down)) return refuse("vpz_pcm_resample: a refused ratio (lowest terms, up <= 1024, down <= 32 * up)");
    bool s16, planar;
    if (!vpz::layout_of(dst_layout, &s16, &planar)) return refuse("vpz_pcm_resample: bad layout");
    // (a sample index times `up` or `down` must fit 63 bits like the sizes in bytes: every index the kernel forms fits an int64_t)
    if (frames > 0 && (unsigned __int128)(uint64_t)frames * (uint64_t)std::max(up, down) > (uint64_t)INT64_MAX / 4)
        return refuse("vpz_pcm_resample: sizes overflow");
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_resample", src_dev, src_elems, sizeof(float), channels, up, down, frames, n_rows, rows, dst_dev,
                                                       dst_rows, (unsigned __int128)(uint64_t)frames * (uint64_t)out_channels,
                                                       s16 ? sizeof(int16_t) : sizeof(float)});
    if (rc != VPZ_OK || n_rows == 0) return rc;
    const int64_t blocks = (frames + vpz::kRsBlock - 1) / vpz::kRsBlock;
    if (blocks > 0x7fffffff) return refuse("vpz_pcm_resample: a row too long for one launch");

    const vpz::Context::ResampleTable *tb = nullptr;
    rc = vpz::ratio_table(ctx, up, down, &tb);
    if (rc != VPZ_OK) return rc;
    vpz::ResampleArgs a;
    rc = vpz::upload_rows(ctx, n_rows, rows, &a.rows);
    if (rc != VPZ_OK) return rc;
    a.src = static_cast<const float *>(src_dev);
    a.dst = dst_dev;
    a.coeff = tb->d_coeff;
    a.first = tb->d_first;
    a.frames = frames;
    a.n_rows = n_rows;
    a.channels = channels;
    a.out_channels = out_channels;
    a.downmix = downmix;
    a.up = up;
    a.down = down;
    a.taps = tb->taps;
    a.first_min = tb->first_min;
    // a tile's span: its last output starts at most (kRsBlock - 1) * down / up + 1 samples behind its first, a phase's first tap is
    // first_min or one more, and `taps` samples follow
    a.span_cap = (int32_t)((int64_t)(vpz::kRsBlock - 1) * down / up + 2 + tb->taps);
    // (<= kRsLds inside the ratio's limits: the static_assert above)
    // tests/test_pcm_resample_limits_gpu.py runs every value per_pass takes (1, 2, 3, 4, 5, 8), last passes narrower than the others, 255
    // channels and the ratios at which span_cap comes within 2 % of kRsLds; tests/test_resample_cpu.py restates this plan and holds the
    // tests' case list to it, so a change of a constant above fails there first
    a.per_pass = std::max(1, std::min(std::min<int32_t>(out_channels, vpz::kRsMaxPass), vpz::kRsLds / a.span_cap));
    const dim3 grid((unsigned)blocks, (unsigned)std::min<int64_t>(n_rows, vpz::kRsMaxGridY));
    const size_t lds = sizeof(float) * (size_t)a.per_pass * ((size_t)a.span_cap + vpz::kRsBlock);  // (at most 42 KiB: kRsLds + kRsMaxPass tiles)
    if (s16 && planar) vpz::pcm_resample_kernel<int16_t, true><<<grid, vpz::kRsBlock, lds, ctx->stream>>>(a);
    else if (s16) vpz::pcm_resample_kernel<int16_t, false><<<grid, vpz::kRsBlock, lds, ctx->stream>>>(a);
    else if (planar) vpz::pcm_resample_kernel<float, true><<<grid, vpz::kRsBlock, lds, ctx->stream>>>(a);
    else vpz::pcm_resample_kernel<float, false><<<grid, vpz::kRsBlock, lds, ctx->stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "pcm_resample kernel launch", e);
    return VPZ_OK;
}
