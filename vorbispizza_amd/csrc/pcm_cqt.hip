// vpz_pcm_cqt, vpz_cqt_bins and vpz_cqt_kernel (include/vorbispizza_pcm_cqt.h, which states the definition): windows of a float32 device
// PCM array as constant-Q spectrograms -- complex, magnitude or power --, one launch.
//
// The mapping:
//   the bins are cut into COLUMN BLOCKS of kCqCols = 32 (the MFMA's N).  A block's kernels are centre-aligned in its longest one, N_b
//   (its first bin's): kernel k starts at row floor(N_b / 2) - floor(N_k / 2) of the block's table [len_b][2][32] (len_b = N_b made even:
//   the MFMA takes two rows a step; the Re columns, then the Im columns), zeros before and behind it.  Frame t's A operand for the block
//   is then one plain slice of the row, x[t * hop - floor(N_b / 2) + m], m = 0 .. len_b-1, and only the block's own length is run: the
//   dead range of the shorter blocks is skipped (sum of len_b = 13 408 at the default spec, against 3 * 11 339 dense);
//   a TILE is Tt consecutive frames [t0, t0 + Tt) of one destination row (Tt = 64, 32 or 16, chosen by the launch from the spec and T
//   alone: tile_plan below); one workgroup per (tile, descriptor, column block): grid (tiles, rows, blocks);
//   a workgroup has one wave per (32 frames, component): wave w computes component w & 1 (Re or Im) of frames 32 (w >> 1) ..: four waves
//   at Tt = 64, two at 32 and 16.  All run the same k-range at the same time, each ONE accumulator chain on the exact float32 MFMA
//   (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain from +0), which issues back to back;
//   k is staged in CHUNKS of kCqChunk samples: for chunk [c0, c0 + cl) the span x[t0 * hop - floor(N_b / 2) + c0 ..] of (nt - 1) * hop +
//   cl samples goes to LDS, the zero extension [L, F) and the padding mode resolved in the staging index, SKEWED as pcm_logmel.hip skews
//   it (sample i at i + floor(i / hop) when hop is even, so that the 32 frames of a wave fall on 32 banks); the accumulators live across
//   the chunks.  No spec needs a whole span in LDS;
//   a wave reads its B values straight from the table (L2 / MALL), the loads of the next kCqAhead k-steps issued before the MFMAs of the
//   current ones;
//   the accumulators go to an LDS stage [2][Tt][33]; then one lane per (frame, bin) forms the output and stores, consecutive lanes along
//   the layout's inner dimension.
//   A tile whose whole span (of the block) lies in a row's zeros stores zeros without computing.
// All element indices are 64-bit.  No scratch memory.  Built with -ffp-contract=off: every fused step is written as one.
#include <algorithm>
#include <array>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "device_table.hpp"
#include "cqt_tables.hpp"
#include "../../include/vorbispizza_pcm_cqt.h"

namespace vpz {

namespace {

constexpr int kCqCols = 32;          // bins of a column block (the MFMA's N)
constexpr int kCqChunk = 2048;       // samples of k staged at a time (even)
constexpr int kCqLdsFloats = 40960;  // 160 KiB: what a workgroup may use
constexpr int kCqMaxGridY = 2048;    // descriptors side by side in the grid's y; a workgroup takes every kCqMaxGridY-th beyond that
constexpr int kCqMaxTile = 64;       // the tile sizes: kCqMaxTile, 32 and kCqMinTile frames
constexpr int kCqMinTile = 16;
constexpr int kCqStageStride = 33;   // floats between two frames of the stage (odd: the accumulators' rows fall on different banks)
constexpr int kCqAhead = 16;         // k-steps (of two samples) whose table values are loaded ahead: 16 MFMAs are 1024 cycles, an L2 round trip

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct CqBlock {
    int64_t at;    // floats from the table's start to the block's [len][2][32]
    int32_t len;   // rows: the block's longest kernel, made even
    int32_t half;  // floor(longest / 2): the block's rows start that many samples before a frame's centre
};

struct CqtArgs {
    const float *src;
    const vpz_pack_row *rows;
    float *dst;
    const float *table;
    const CqBlock *blocks;
    int64_t frames, T;
    int32_t n_rows, n_bins, hop, output, frames_first, pad_zero, reach;  // reach: floor(N_0 / 2), how far the reflection goes
    int32_t Tt, skew, span_cap;  // frames of a tile; 1: the span is skewed; floats of the span
};

__global__ __launch_bounds__(256) void pcm_cqt_kernel(const CqtArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *const span = lds, *const stage = lds + a.span_cap;
    const int t = threadIdx.x, lanes = blockDim.x, lane = t & 63, wave = t >> 6, col = lane & 31, h = lane >> 5;
    const int comp = wave & 1, fh = wave >> 1;
    const int hop = a.hop, Tt = a.Tt, skew = a.skew, output = a.output, n_bins = a.n_bins;
    const int64_t F = a.frames, T = a.T;
    const CqBlock blk = a.blocks[blockIdx.z];
    const int k0 = (int)blockIdx.z * kCqCols;
    const int nbk = n_bins - k0 < kCqCols ? n_bins - k0 : kCqCols;  // the block's bins
    const int64_t t0 = (int64_t)blockIdx.x * Tt;
    const int nt = (int)(T - t0 < Tt ? T - t0 : Tt);  // the tile's frames (the grid covers T)
    const int64_t lo = t0 * hop - blk.half;            // the first extended sample the block reads
    const int64_t hi = lo + (int64_t)(nt - 1) * hop + blk.len - 1;
    const int frame = fh * 32 + col;
    const int base = (frame < nt ? frame : nt - 1) * (hop + skew);  // (a frame behind the tile's repeats the last one: its results are not stored)
    const float *const tab = a.table + blk.at + comp * kCqCols + col;  // row m of this lane's column: tab[m * 64]
    constexpr size_t ld = 2 * kCqCols;
    const int items = nt * nbk;
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_pack_row d = a.rows[r];
        const int64_t L = d.samples;
        // every sample the block reads is one of the row's zeros (behind F - 1 a reflected span's last sample reaches back furthest)
        const bool silent = L == 0 || (lo >= L && (a.pad_zero || hi <= F - 1 || 2 * (F - 1) - hi >= L));  // (the same for the whole workgroup)
        if (!silent) {
            const float *in = a.src + d.src;
            f32x16 acc;
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
            for (int c0 = 0; c0 < blk.len; c0 += kCqChunk) {
                const int cl = blk.len - c0 < kCqChunk ? blk.len - c0 : kCqChunk;  // (even, as len and the chunk are)
                const int count = (nt - 1) * hop + cl;
                for (int i = t; i < count; i += lanes) {
                    const int64_t e = lo + c0 + i;
                    // (beyond the reflection x is zero: -1 stands for it)
                    const int64_t x = a.pad_zero ? e : e < 0 ? -e : e <= F - 1 ? e : e - (F - 1) <= a.reach ? 2 * (F - 1) - e : -1;
                    span[i + (skew ? i / hop : 0)] = x >= 0 && x < L ? in[x] : 0.0f;
                }
                __syncthreads();
                // this lane's sample of a k-step: m = 2 * step + h, as its place g = m + skew * floor(m / hop) in a frame
                int g = h + (skew && h >= hop ? 1 : 0), rem = h >= hop ? h - hop : h;
                auto step_a = [&]() {  // (an even hop is at least 2: one wrap per step at the most; an odd hop has no skew)
                    rem += 2;
                    const int c = rem >= hop ? 1 : 0;
                    rem -= c ? hop : 0;
                    g += 2 + (skew ? c : 0);
                };
                const float *tp = tab + (size_t)(c0 + h) * ld;
                const int pairs = cl / 2, groups = pairs / kCqAhead;
                float cur[kCqAhead], nxt[kCqAhead];
                if (groups > 0) {
#pragma unroll
                    for (int u = 0; u < kCqAhead; ++u) cur[u] = tp[(size_t)(2 * u) * ld];
                }
                for (int gr = 0; gr < groups; ++gr) {
                    const int ng = gr + 1 < groups ? gr + 1 : gr;  // (the last group loads itself again: no branch)
#pragma unroll
                    for (int u = 0; u < kCqAhead; ++u) nxt[u] = tp[(size_t)(2 * (ng * kCqAhead + u)) * ld];
#pragma unroll
                    for (int u = 0; u < kCqAhead; ++u) {
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(span[base + g], cur[u], acc, 0, 0, 0);
                        step_a();
                    }
#pragma unroll
                    for (int u = 0; u < kCqAhead; ++u) cur[u] = nxt[u];
                }
                for (int pr = groups * kCqAhead; pr < pairs; ++pr) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(span[base + g], tp[(size_t)(2 * pr) * ld], acc, 0, 0, 0);
                    step_a();
                }
                __syncthreads();  // (the next chunk's staging writes the span)
            }
            // the accumulators' map: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = fh * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (row < nt) stage[(comp * Tt + row) * kCqStageStride + col] = acc[i];
            }
            __syncthreads();
        }
        for (int it = t; it < items; it += lanes) {
            int tl, kk;
            if (a.frames_first) {
                tl = it / nbk;
                kk = it - tl * nbk;
            } else {
                kk = it / nt;
                tl = it - kk * nt;
            }
            const float re = silent ? 0.0f : stage[tl * kCqStageStride + kk], im = silent ? 0.0f : stage[(Tt + tl) * kCqStageStride + kk];
            const int64_t at = a.frames_first ? (d.row * T + t0 + tl) * n_bins + k0 + kk : (d.row * n_bins + k0 + kk) * T + t0 + tl;
            if (output == VPZ_CQT_COMPLEX) {
                reinterpret_cast<float2 *>(a.dst)[at] = make_float2(re, im);
            } else {
                const float P = __builtin_fmaf(re, re, im * im);
                a.dst[at] = output == VPZ_CQT_POWER ? P : __builtin_sqrtf(P);  // (the correctly rounded root: the build's default for sqrtf)
            }
        }
        __syncthreads();  // (the stage is read before the next descriptor's accumulators are written)
    }
}

// the table of a spec: per column block [len][2][32], and the blocks' records behind it
int cqt_table_for(Context *ctx, const vpz_cqt_spec &s, const CqtBins &bins, const Context::CqtTable **out)
{
    const std::array<double, 8> key = {s.sample_rate, s.f_min, s.filter_scale, s.gamma, (double)s.n_bins, (double)s.bins_per_octave, (double)s.window, (double)s.scale};
    return table_for(ctx, ctx->cqt_tables, key, "vpz_pcm_cqt: out of host memory", out, [&](Context::CqtTable &tb) {
        const int n_blocks = (s.n_bins + kCqCols - 1) / kCqCols;
        std::vector<CqBlock> blocks((size_t)n_blocks);
        int64_t total = 0;
        for (int b = 0; b < n_blocks; ++b) {
            const int longest = bins.n[(size_t)b * kCqCols];
            blocks[(size_t)b] = CqBlock{total, (longest + 1) & ~1, longest / 2};
            total += (int64_t)blocks[(size_t)b].len * 2 * kCqCols;
        }
        std::vector<float> host((size_t)total, 0.0f);
        for (int k = 0; k < s.n_bins; ++k) {
            const CqBlock &b = blocks[(size_t)(k / kCqCols)];
            const int n = bins.n[(size_t)k];
            float *hr = host.data() + b.at + (size_t)(b.half - n / 2) * 2 * kCqCols + k % kCqCols;
            cqt_kernel_fill(s, bins.f[(size_t)k], n, hr, hr + kCqCols, 2 * kCqCols);
        }
        tb.n_blocks = n_blocks;
        tb.n0 = bins.n[0];
        return upload(ctx, "vpz_pcm_cqt: table upload", tb, {{host.data(), host.size() * sizeof(float), reinterpret_cast<void **>(&tb.d_table)},
                                                             {blocks.data(), blocks.size() * sizeof(CqBlock), &tb.d_blocks}});
    });
}

// floats of a tile's span at `Tt` frames: the longest chunk of every frame, skewed where the hop is even
int span_floats(int hop, int Tt)
{
    const int count = (Tt - 1) * hop + kCqChunk;
    return count + (hop % 2 == 0 ? count / hop : 0) + 1;
}

// floats of a tile's LDS: the span, then the stage of both components
int lds_floats(int hop, int Tt) { return span_floats(hop, Tt) + 2 * Tt * kCqStageStride; }

// THE TILE PLAN, from hop and T alone (a result does not depend on the tile: the same bits): kCqMaxTile frames where the row has more than
// 32 and the LDS holds them, else 32 where the LDS holds them, else kCqMinTile (which fits at every hop inside the limits); a workgroup
// has 64 lanes per (32 frames, component).  tests/cqt_truth.py restates it (tile_plan)
int tile_plan(int hop, int64_t T)
{
    for (int Tt : {kCqMaxTile, 32, kCqMinTile}) {
        if ((Tt == kCqMaxTile && T <= 32) || lds_floats(hop, Tt) > kCqLdsFloats) continue;
        return Tt;
    }
    return 0;
}

}  // namespace

}  // namespace vpz

extern "C" int vpz_cqt_bins(const vpz_cqt_spec *spec, double *freqs, int32_t *lengths, int32_t capacity)
{
    vpz::CqtBins bins;
    if (!spec || capacity < 0 || !vpz::cqt_bins(*spec, &bins)) return VPZ_E_INVALID_ARG;
    if ((freqs || lengths) && capacity < spec->n_bins) return VPZ_E_CAPACITY;
    if (freqs) memcpy(freqs, bins.f.data(), bins.f.size() * sizeof(double));
    if (lengths) memcpy(lengths, bins.n.data(), bins.n.size() * sizeof(int32_t));
    return VPZ_OK;
}

extern "C" int vpz_cqt_kernel(const vpz_cqt_spec *spec, int32_t k, float *table, int64_t capacity, int32_t *length)
{
    vpz::CqtBins bins;
    if (!spec || capacity < 0 || !vpz::cqt_bins(*spec, &bins) || k < 0 || k >= spec->n_bins) return VPZ_E_INVALID_ARG;
    const int n = bins.n[(size_t)k];
    if (length) *length = n;
    if (!table) return VPZ_OK;
    if (capacity < 2 * (int64_t)n) return VPZ_E_CAPACITY;
    vpz::cqt_kernel_fill(*spec, bins.f[(size_t)k], n, table, table + n, 1);
    return VPZ_OK;
}

extern "C" int vpz_pcm_cqt(vpz_context *c, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_cqt_spec *spec, int32_t n_rows,
                           const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!spec) return refuse("vpz_pcm_cqt: null pointer");
    vpz::CqtBins bins;
    try {
        if (!vpz::cqt_bins(*spec, &bins)) return refuse("vpz_pcm_cqt: a spec outside the limits");
    } catch (const std::bad_alloc &) {
        return vpz::set_error(ctx, VPZ_E_NOMEM, "vpz_pcm_cqt: out of host memory");
    }
    const vpz_cqt_spec &s = *spec;
    if (frames < 1) return refuse("vpz_pcm_cqt: frames < 1");
    if (s.pad == VPZ_CQT_PAD_REFLECT && frames < bins.n[0] / 2 + 1) return refuse("vpz_pcm_cqt: frames < floor(N_0 / 2) + 1 (the reflection needs it)");
    if (frames > INT64_MAX / 8) return refuse("vpz_pcm_cqt: sizes overflow");
    const int64_t T = 1 + frames / s.hop;
    const bool complex_out = s.output == VPZ_CQT_COMPLEX;
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_cqt", src_dev, src_elems, sizeof(float), 1, 1, 1, frames, n_rows, rows, dst_dev, dst_rows,
                                                       (unsigned __int128)(uint64_t)T * (uint64_t)s.n_bins * (complex_out ? 2u : 1u), sizeof(float)});
    if (rc != VPZ_OK) return rc;
    if (complex_out && reinterpret_cast<uintptr_t>(dst_dev) % (2 * sizeof(float)) != 0)
        return refuse("vpz_pcm_cqt: dst_dev is not aligned to a pair of float32");

    vpz::CqtArgs a;
    a.Tt = vpz::tile_plan(s.hop, T);
    if (a.Tt == 0) return vpz::set_error(ctx, VPZ_E_UNSUPPORTED, "vpz_pcm_cqt: no tile fits the LDS");  // (the smallest fits at every hop inside the limits)
    const int64_t tiles = (T + a.Tt - 1) / a.Tt;
    if (tiles > 0x7fffffff) return refuse("vpz_pcm_cqt: a row too long for one launch");
    if (n_rows == 0) return VPZ_OK;

    const vpz::Context::CqtTable *tb = nullptr;
    rc = vpz::cqt_table_for(ctx, s, bins, &tb);
    if (rc != VPZ_OK) return rc;
    rc = vpz::upload_rows(ctx, n_rows, rows, &a.rows);
    if (rc != VPZ_OK) return rc;

    a.src = static_cast<const float *>(src_dev);
    a.dst = static_cast<float *>(dst_dev);
    a.table = tb->d_table;
    a.blocks = static_cast<const vpz::CqBlock *>(tb->d_blocks);
    a.frames = frames;
    a.T = T;
    a.n_rows = n_rows;
    a.n_bins = s.n_bins;
    a.hop = s.hop;
    a.output = s.output;
    a.frames_first = s.layout == VPZ_CQT_FRAMES_FIRST;
    a.pad_zero = s.pad == VPZ_CQT_PAD_ZERO;
    a.reach = tb->n0 / 2;
    a.skew = s.hop % 2 == 0 ? 1 : 0;
    a.span_cap = vpz::span_floats(s.hop, a.Tt);
    const dim3 grid((unsigned)tiles, (unsigned)std::min<int64_t>(n_rows, vpz::kCqMaxGridY), (unsigned)tb->n_blocks);
    const unsigned lanes = a.Tt > 32 ? 256 : 128;
    const size_t lds = sizeof(float) * (size_t)vpz::lds_floats(s.hop, a.Tt);
    // (the attribute is the kernel's, not the launch's: always the whole budget, so that two contexts never lower it under each other)
    VPZ_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&vpz::pcm_cqt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(sizeof(float) * vpz::kCqLdsFloats)));
    vpz::pcm_cqt_kernel<<<grid, lanes, lds, ctx->stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "pcm_cqt kernel launch", e);
    return VPZ_OK;
}
