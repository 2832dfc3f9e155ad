// vpz_pcm_logmel, vpz_logmel_dft_table and vpz_mel_filterbank (include/vorbispizza_pcm_logmel.h, which states the definition): windows
// of a mono device PCM array as (log-)mel feature frames, one launch, no spectrogram in device memory.
//
// The mapping:
//   a TILE is Tt consecutive frames [t0, t0 + Tt) of one destination row (Tt = 64, 32 or 16: the largest whose LDS fits -- 32 rather
//   than 64 when the launch is too small to fill the chip at 64 --, chosen by the launch); one workgroup of four waves per tile and
//   descriptor;
//   the tile's SOURCE SPAN -- extended samples t0 * hop - n_fft/2 up to the last sample of the tile's last frame -- is staged in LDS,
//   the zero extension [L, F) and the reflection at both ends resolved in the staging index, so a frame is a plain slice of the span;
//   the DFT of the tile is a matrix product on the exact float32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, so a result
//   does not depend on how frames are grouped into tiles): frames are the A operand, read out of the span as A[t][m] = span[t * hop + m],
//   the table is the B operand.  A wave owns 32 bins at a time -- the cos columns AND the sin columns of those bins, for every frame of
//   the tile: four (two at Tt <= 32) independent accumulators -- and reads its B values straight from the table (L2): no other wave of
//   the workgroup reads the same columns, so a trip through LDS would be a copy without reuse; the loads of the next four k-steps are
//   issued before the MFMAs of the current four;
//   the A read is a strided LDS access (lane = frame): the span is stored SKEWED, sample i at i + floor(i / hop) when hop is even, so
//   that consecutive frames lie hop + 1 -- an odd number of -- words apart and the 32 frames of a tile fall on 32 different banks (an
//   odd hop needs no skew);
//   P = re^2 + im^2 goes from the accumulators into an LDS tile [Tt][n_fft/2 + 1, made odd]; then one lane per (frame, band) sums its
//   band's live bins in ascending k, takes the log and stores, consecutive lanes along the layout's inner dimension.
//   The table's columns are padded with zeros to a multiple of 32 per half: the inner loop has no branch.  A tile whose span lies
//   wholly in a row's zeros stores the silence value without computing (every product would be with zero).
// All element indices are 64-bit.  No scratch memory.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "device_table.hpp"
#include "logmel_tables.hpp"
#include "../../include/vorbispizza_pcm_logmel.h"

namespace vpz {

namespace {

constexpr int kLmBlock = 256;      // lanes of a workgroup: four waves
constexpr int kLmCols = 32;        // bins a wave owns at a time (the MFMA's N)
constexpr int kLmLdsFloats = 40960;  // 160 KiB: what a workgroup may use
constexpr int kLmMaxGridY = 2048;  // descriptors side by side in the grid's y; a workgroup takes every kLmMaxGridY-th beyond that
constexpr int kLmAhead = 4;        // k-steps (of two samples) whose table values are loaded ahead

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct LogmelArgs {
    const float *src;
    const vpz_pack_row *rows;
    float *dst;
    const float *table;   // [n_fft][2 * cols]
    const int32_t *meta;  // [n_mels][3]
    const float *w;
    int64_t frames, T;
    int32_t n_rows, n_fft, hop, nb, cols, n_mels, log, frames_first;
    int32_t Tt, skew, pstride, span_cap;  // frames of a tile; 1: the span is skewed; floats between two rows of the power tile; floats of the span
    float floor, silence;
};

// RT: 32-frame row tiles of a workgroup's tile (2 at Tt = 64, 1 at Tt <= 32)
template <int RT>
__global__ __launch_bounds__(kLmBlock) void pcm_logmel_kernel(const LogmelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *span = lds, *pw = lds + a.span_cap;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, h = lane >> 5;
    const int n_fft = a.n_fft, hop = a.hop, nb = a.nb, n_mels = a.n_mels, Tt = a.Tt, skew = a.skew, pstride = a.pstride;
    const int64_t F = a.frames, T = a.T;
    const int64_t t0 = (int64_t)blockIdx.x * Tt;
    const int nt = (int)(T - t0 < Tt ? T - t0 : Tt);          // the tile's frames (the grid covers T)
    const int64_t lo = t0 * hop - n_fft / 2;                  // the span's first extended sample
    const int count = (nt - 1) * hop + n_fft;                 // its samples
    const int64_t hi = lo + count - 1;
    const int items = nt * n_mels;
    const size_t ld = 2 * (size_t)a.cols;
    int base[RT];
    for (int rt = 0; rt < RT; ++rt) {
        const int row = rt * 32 + col;
        base[rt] = (row < nt ? row : nt - 1) * (hop + skew);  // (a row behind the tile's frames repeats the last one: its results are not stored)
    }
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_pack_row d = a.rows[r];
        const int64_t L = d.samples;
        // every sample of the span is one of the row's zeros (behind F - 1 the span reflects: its last sample reaches back furthest)
        const bool silent = L == 0 || (lo >= L && (hi <= F - 1 || 2 * (F - 1) - hi >= L));  // (the same for the whole workgroup)
        if (!silent) {
            const float *in = a.src + d.src;
            for (int i = t; i < count; i += kLmBlock) {
                const int64_t e = lo + i;
                const int64_t x = e < 0 ? -e : e > F - 1 ? 2 * (F - 1) - e : e;
                span[i + (skew ? i / hop : 0)] = x < L ? in[x] : 0.0f;
            }
            __syncthreads();
            for (int k0 = wave * kLmCols; k0 < nb; k0 += (kLmBlock / 64) * kLmCols) {
                f32x16 re[RT], im[RT];
                for (int rt = 0; rt < RT; ++rt)
                    for (int i = 0; i < 16; ++i) re[rt][i] = im[rt][i] = 0.0f;
                // this lane's sample of a k-step: m = 2 * step + h, as its place g = m + skew * floor(m / hop) in a frame
                int g = h + (skew && h >= hop ? 1 : 0), rem = h >= hop ? h - hop : h;
                auto step_a = [&]() {  // (an even hop is at least 2: one wrap per step at the most; an odd hop has no skew)
                    rem += 2;
                    const int c = rem >= hop ? 1 : 0;
                    rem -= c ? hop : 0;
                    g += 2 + (skew ? c : 0);
                };
                const float *tp = a.table + (size_t)h * ld + k0 + col;  // table row m = h, this lane's cos column
                const int pairs = n_fft / 2, blocks = pairs / kLmAhead;
                float cre[kLmAhead], cim[kLmAhead], nre[kLmAhead], nim[kLmAhead];
                if (blocks > 0) {
#pragma unroll
                    for (int u = 0; u < kLmAhead; ++u) {
                        const float *p = tp + (size_t)(2 * u) * ld;
                        cre[u] = p[0];
                        cim[u] = p[a.cols];
                    }
                }
                for (int blk = 0; blk < blocks; ++blk) {
                    const int nxt = blk + 1 < blocks ? blk + 1 : blk;  // (the last block loads itself again: no branch)
#pragma unroll
                    for (int u = 0; u < kLmAhead; ++u) {
                        const float *p = tp + (size_t)(2 * (nxt * kLmAhead + u)) * ld;
                        nre[u] = p[0];
                        nim[u] = p[a.cols];
                    }
#pragma unroll
                    for (int u = 0; u < kLmAhead; ++u) {
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            const float av = span[base[rt] + g];
                            re[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, cre[u], re[rt], 0, 0, 0);
                            im[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, cim[u], im[rt], 0, 0, 0);
                        }
                        step_a();
                    }
#pragma unroll
                    for (int u = 0; u < kLmAhead; ++u) {
                        cre[u] = nre[u];
                        cim[u] = nim[u];
                    }
                }
                for (int pr = blocks * kLmAhead; pr < pairs; ++pr) {
                    const float *p = tp + (size_t)(2 * pr) * ld;
                    const float br = p[0], bi = p[a.cols];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const float av = span[base[rt] + g];
                        re[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, br, re[rt], 0, 0, 0);
                        im[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bi, im[rt], 0, 0, 0);
                    }
                    step_a();
                }
                // the accumulators' map: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
                const int k = k0 + col;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int row = rt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        if (k < nb && row < Tt) pw[row * pstride + k] = re[rt][i] * re[rt][i] + im[rt][i] * im[rt][i];
                    }
            }
            __syncthreads();
        }
        // (the next descriptor's staging writes the span, which no lane reads any more, and its barrier stands before the power tile is
        // written again)
        for (int it = t; it < items; it += kLmBlock) {
            int tl, b;
            if (a.frames_first) {
                tl = it / n_mels;
                b = it - tl * n_mels;
            } else {
                b = it / nt;
                tl = it - b * nt;
            }
            float v = a.silence;
            if (!silent) {
                const int first = a.meta[3 * b], cnt = a.meta[3 * b + 1];
                const float *p = pw + tl * pstride + first, *ww = a.w + a.meta[3 * b + 2];
                float acc = 0.0f;
                for (int i = 0; i < cnt; ++i) acc = __builtin_fmaf(ww[i], p[i], acc);
                v = !a.log ? acc : acc <= a.floor ? a.silence : log10f(acc);
            }
            const int64_t at = a.frames_first ? (d.row * T + t0 + tl) * n_mels + b : (d.row * n_mels + b) * T + t0 + tl;
            a.dst[at] = v;
        }
    }
}

int dft_for(Context *ctx, int n_fft, const Context::LogmelDft **out)
{
    return table_for(ctx, ctx->logmel_dft, n_fft, "vpz_pcm_logmel: out of host memory", out, [&](Context::LogmelDft &tb) {
        tb.cols = (n_fft / 2 + 1 + kLmCols - 1) / kLmCols * kLmCols;
        std::vector<float> host((size_t)n_fft * 2 * (size_t)tb.cols, 0.0f);
        logmel_dft_fill(n_fft, host.data(), 2 * (size_t)tb.cols, (size_t)tb.cols);
        return upload(ctx, "vpz_pcm_logmel: DFT table upload", tb, {{host.data(), host.size() * sizeof(float), reinterpret_cast<void **>(&tb.d_table)}});
    });
}

int bank_for(Context *ctx, const vpz_logmel_spec &s, const Context::LogmelBank **out)
{
    const std::array<double, 7> key = {s.sample_rate, (double)s.n_fft, (double)s.n_mels, s.f_min, s.f_max, (double)s.mel_scale, (double)s.mel_norm};
    return table_for(ctx, ctx->logmel_banks, key, "vpz_pcm_logmel: out of host memory", out, [&](Context::LogmelBank &bk) {
        MelFilterbank fb;
        mel_build(s, fb);
        return upload_bank(ctx, "vpz_pcm_logmel: filterbank upload", fb, bk);
    });
}

// floats of a tile's LDS at `Tt` frames: the skewed span, then the power tile
void lds_plan(const vpz_logmel_spec &s, int Tt, int *span_cap, int *pstride)
{
    const int count = (Tt - 1) * s.hop + s.n_fft, skew = s.hop % 2 == 0 ? 1 : 0;
    *span_cap = count + (skew ? count / s.hop : 0) + 1;
    *pstride = (s.n_fft / 2 + 1) | 1;
}

}  // namespace

}  // namespace vpz

extern "C" int vpz_logmel_dft_table(int32_t n_fft, float *table, int64_t capacity)
{
    if (!vpz::logmel_nfft_ok(n_fft) || capacity < 0) return VPZ_E_INVALID_ARG;
    if (!table) return VPZ_OK;
    const int64_t nb = n_fft / 2 + 1;
    if (capacity < (int64_t)n_fft * 2 * nb) return VPZ_E_CAPACITY;
    vpz::logmel_dft_fill(n_fft, table, (size_t)(2 * nb), (size_t)nb);
    return VPZ_OK;
}

extern "C" int vpz_mel_filterbank(const vpz_logmel_spec *spec, int32_t *first_bin, int32_t *n_bins, float *weights, int64_t capacity,
                                  int64_t *total)
{
    if (!spec || capacity < 0 || !vpz::logmel_spec_ok(*spec)) return VPZ_E_INVALID_ARG;
    return vpz::mel_filterbank_out(*spec, first_bin, n_bins, weights, capacity, total);
}

extern "C" int vpz_pcm_logmel(vpz_context *c, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_logmel_spec *spec,
                              int32_t n_rows, const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!spec) return refuse("vpz_pcm_logmel: null pointer");
    if (!vpz::logmel_spec_ok(*spec)) return refuse("vpz_pcm_logmel: a spec outside the limits");
    const vpz_logmel_spec &s = *spec;
    if (frames < s.n_fft / 2 + 1) return refuse("vpz_pcm_logmel: frames < n_fft / 2 + 1 (the reflection needs it)");
    if (frames > INT64_MAX / 8) return refuse("vpz_pcm_logmel: sizes overflow");
    const int64_t T = 1 + frames / s.hop;
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_logmel", src_dev, src_elems, sizeof(float), 1, 1, 1, frames, n_rows, rows, dst_dev, dst_rows,
                                                       (unsigned __int128)(uint64_t)T * (uint64_t)s.n_mels, sizeof(float)});
    if (rc != VPZ_OK || n_rows == 0) return rc;

    const vpz::Context::LogmelDft *tb = nullptr;
    const vpz::Context::LogmelBank *bk = nullptr;
    rc = vpz::dft_for(ctx, s.n_fft, &tb);
    if (rc == VPZ_OK) rc = vpz::bank_for(ctx, s, &bk);
    if (rc != VPZ_OK) return rc;

    vpz::LogmelArgs a;
    // the tile: 64 frames where the row has more than 32 and the LDS holds them -- every tile reads the whole table from L2 (643 KB at
    // n_fft 400), so the larger tile halves that traffic --, else 32, else 16 (n_fft 1024 at a hop near it: the span alone is 128 KiB at 32)
    // -- a launch too small to give every CU two workgroups at 64 takes 32 (a result does not depend on the tile: the same bits)
    // tests/test_logmel_cpu.py restates lds_plan and this choice (tile_plan); tests/test_pcm_logmel_limits_gpu.py runs every tile next to
    // the LDS budget (n_fft 1024: 64 frames up to hop 111, 32 up to 757) and the leftover k-steps of an n_fft that is no multiple of 8
    a.Tt = 0;
    const bool few = ((T + 63) / 64) * (int64_t)n_rows < 2 * (int64_t)ctx->num_cu;
    for (int Tt : {64, 32, 16}) {
        vpz::lds_plan(s, Tt, &a.span_cap, &a.pstride);
        if ((Tt == 64 && (T <= 32 || few)) || a.span_cap + Tt * a.pstride > vpz::kLmLdsFloats) continue;
        a.Tt = Tt;
        break;
    }
    if (a.Tt == 0) return vpz::set_error(ctx, VPZ_E_UNSUPPORTED, "vpz_pcm_logmel: no tile fits the LDS");  // (16 frames fit at every spec inside the limits)
    const int64_t blocks = (T + a.Tt - 1) / a.Tt;
    if (blocks > 0x7fffffff) return refuse("vpz_pcm_logmel: a row too long for one launch");

    rc = vpz::upload_rows(ctx, n_rows, rows, &a.rows);
    if (rc != VPZ_OK) return rc;

    a.src = static_cast<const float *>(src_dev);
    a.dst = static_cast<float *>(dst_dev);
    a.table = tb->d_table;
    a.meta = bk->d_meta;
    a.w = bk->d_w;
    a.frames = frames;
    a.T = T;
    a.n_rows = n_rows;
    a.n_fft = s.n_fft;
    a.hop = s.hop;
    a.nb = s.n_fft / 2 + 1;
    a.cols = tb->cols;
    a.n_mels = s.n_mels;
    a.log = s.output == VPZ_MEL_LOG10;
    a.frames_first = s.layout == VPZ_MEL_FRAMES_FIRST;
    a.skew = s.hop % 2 == 0 ? 1 : 0;
    a.floor = a.log ? (float)s.floor : 0.0f;
    a.silence = a.log ? (float)log10((double)a.floor) : 0.0f;
    const dim3 grid((unsigned)blocks, (unsigned)std::min<int64_t>(n_rows, vpz::kLmMaxGridY));
    const size_t lds = sizeof(float) * ((size_t)a.span_cap + (size_t)a.Tt * (size_t)a.pstride);
    // (the attribute is the kernel's, not the launch's: always the whole budget, so that two contexts never lower it under each other)
    const int max_lds = (int)(sizeof(float) * vpz::kLmLdsFloats);
    if (a.Tt == 64) {
        VPZ_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&vpz::pcm_logmel_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        vpz::pcm_logmel_kernel<2><<<grid, vpz::kLmBlock, lds, ctx->stream>>>(a);
    } else {
        VPZ_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&vpz::pcm_logmel_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        vpz::pcm_logmel_kernel<1><<<grid, vpz::kLmBlock, lds, ctx->stream>>>(a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "pcm_logmel kernel launch", e);
    return VPZ_OK;
}
