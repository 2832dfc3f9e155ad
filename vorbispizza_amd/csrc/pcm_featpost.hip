// vpz_feat_post and its host helpers (include/vorbispizza_pcm_featpost.h, which states the definition): delta features and mean /
// variance normalisation over a row or a sliding window, on a padded batch of float32 feature frames in device memory.
//
// Three kernels, one workgroup per (row, tile of 64 frames = one chunk, 32 columns), over one VALUE function, fp_val: element (t, block i,
// column) of "the tensor that is normalised or stored" -- the source itself (i = 0), or its i-th delta, the fused multiply-add chain over
// the scales -- read from source frames that the workgroup has staged in LDS with the chain's halo, so that a source element is loaded
// from memory once per workgroup that needs it and a tap costs an LDS read.
//   featpost_chunk_kernel   fp_val of the chunk into LDS side by side, then one thread per column adds S1 and S2 in float64, frames
//                           ascending, into the call's scratch memory [descriptor][chunk][column] (a double2 each).  Launched only when
//                           norm != NONE and a descriptor has a real frame.
//   featpost_apply_kernel   every delta block of the launch from ONE staged tile: pad_value, or fp_val, or (VPZ_NORM_ROW) fp_val normalised
//                           by the sum of its row's chunk sums, which one thread per column adds once for the workgroup.
//   featpost_slide_kernel   VPZ_NORM_SLIDING, one delta block a workgroup.  The windows of a tile's frames start inside two neighbouring
//                           chunks and end inside two, so the workgroup puts fp_val of the frames those partial chunks can cover, and of
//                           its own tile, into LDS once, and every output adds its left partial chunk from LDS, whole chunks from the
//                           scratch memory and its right partial chunk from LDS (from the scratch memory when the window ends with the
//                           row: the same sum).
// In the chunk and the sliding kernel the delta block is the grid's z, in the apply kernel a loop: either way the scales are read at
// wave-uniform indices of the kernel's arguments (scalar loads, no private array).  Frames first: consecutive lanes are consecutive columns
// of one frame; columns first: consecutive lanes are consecutive frames of one column -- both ways a wave's loads and stores are runs of
// consecutive 4-byte words.  DESIGN.md section 6 says what was measured.
// The calls:
//   deltas alone                 apply (blocks 0 .. order)
//   normalisation alone          chunk, apply or slide
//   VPZ_POST_DELTAS_FIRST        chunk, and apply or slide, over the delta view, blocks 0 .. order: the deltas are computed in both, bit
//                                for bit the same chain, in place of a tensor between the stages
//   VPZ_POST_NORM_FIRST          chunk, apply or slide into block 0 of the destination, apply of blocks 1 .. order with block 0 as its source
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "../../include/vorbispizza_pcm_featpost.h"

static_assert(sizeof(vpz_feat_row) == sizeof(vpz_pack_row), "upload_rows carries vpz_feat_row as vpz_pack_row");
static_assert(sizeof(vpz_feat_post_spec) == 96, "vpz_feat_post_spec is part of the C ABI");

namespace vpz {

namespace {

constexpr int kFpBlock = 256;
constexpr int kFpMaxGridY = 4096;  // descriptors side by side in the grid's y; a workgroup takes every kFpMaxGridY-th beyond that
constexpr int kFpChunk = VPZ_FEAT_CHUNK;
constexpr int kFpMaxScales = 12 * VPZ_FEAT_MAX_DELTA_WINDOW + 3;  // orders 1, 2, 3 side by side: (2 w + 1) + (4 w + 1) + (6 w + 1)

struct FpArgs {
    const vpz_feat_row *rows;
    const float *src;  // what fp_val reads: the call's source, or its destination (block 0) in the third launch of NORM_FIRST
    float *dst;
    double2 *chunks;  // [descriptor][nck][ncols_norm]: (S1, S2)
    int64_t T, src_row_elems, dst_row_elems, nck;
    double var_floor;
    float pad;
    int32_t n_rows, D, D_out, src_cols;  // src_cols: the columns of a frame of `src` in memory (D, or D_out when src is the destination)
    int32_t src_is_dst, ff, w;
    int32_t block0;      // the launch's first delta block (the chunk and the sliding kernel: the grid's z = 0)
    int32_t nblocks;     // the apply kernel: the launch's delta blocks, one workgroup for all of them
    int32_t delta_view;  // fp_val takes deltas (else the launch has block 0 alone)
    int32_t norm, norm_vars, center, W, minw, ncols_norm;
    float sc[kFpMaxScales];
};

__host__ __device__ inline int scales_offset(int i, int w) { return w * i * (i - 1) + (i - 1); }  // sum over m < i of 2 m w + 1

// item 2 of the definition, for host and device alike
__host__ __device__ inline void cmn_window(int norm, int center, int64_t W, int64_t minw, int64_t t, int64_t n, int64_t *pa, int64_t *pb)
{
    int64_t a, b;
    if (norm == VPZ_NORM_ROW) {
        a = 0;
        b = n;
    } else {
        if (center) {
            a = t - W / 2;
            b = a + W;
        } else {
            a = t - W;
            b = t + 1;
        }
        if (a < 0) {
            b -= a;
            a = 0;
        }
        if (!center) b = t + 1 > minw ? t + 1 : minw;
        if (b > n) {
            a -= b - n;
            b = n;
            if (a < 0) a = 0;
        }
    }
    *pa = a;
    *pb = b;
}

__device__ __forceinline__ float fp_ld(const FpArgs &a, const float *rb, int64_t t, int d)
{
    return rb[a.ff ? t * a.src_cols + d : (int64_t)d * a.T + t];
}

// item 3's last step: x normalised by the sums of its window of c frames
__device__ __forceinline__ float fp_normalised(const FpArgs &a, float x, double s1, double s2, int64_t c)
{
    const double m = s1 / (double)c, xd = (double)x - m;
    if (!a.norm_vars) return (float)xd;
    if (c == 1) return (float)(xd * 0.0);
    double v = fma(-m, m, s2 / (double)c);
    if (!(v >= a.var_floor)) v = a.var_floor;
    return (float)(xd / sqrt(v));
}

// The kernels cut a row into tiles of 64 frames (one chunk) by kSlCols columns, one workgroup each.  A frame in LDS has one float of
// padding (lanes a frame apart hit different banks).  A delta's taps reach kFpHalo frames to either side at the most
constexpr int kSlCols = 32, kSlStride = kSlCols + 1;
constexpr int kFpHalo = VPZ_FEAT_MAX_DELTA_ORDER * VPZ_FEAT_MAX_DELTA_WINDOW;
constexpr int kTileStage = kFpChunk + 2 * kFpHalo;  // a tile of source frames and its halo
// the sliding kernel's values: frames [lbase, lbase + 128) (the chunks the tile's windows start in), [rbase, rbase + 128) (those they
// end in) and the tile's own 64; a region of source frames and its halo beside them
constexpr int kSlRegion = 2 * kFpChunk, kSlRows = 2 * kSlRegion + kFpChunk, kRegionStage = kSlRegion + 2 * kFpHalo;

struct FpTile {
    int64_t t0;
    int c0, nc;
};
__device__ __forceinline__ FpTile fp_tile(const FpArgs &a)
{
    const int ctiles = (a.D + kSlCols - 1) / kSlCols;
    FpTile t;
    t.t0 = (int64_t)(blockIdx.x / ctiles) * kFpChunk;
    t.c0 = (int)(blockIdx.x % ctiles) * kSlCols;
    t.nc = a.D - t.c0 < kSlCols ? a.D - t.c0 : kSlCols;
    return t;
}

// element e of `count` frames by nc columns as (frame, column): consecutive lanes are consecutive words of the tensor's layout
__device__ __forceinline__ void fp_split(const FpArgs &a, int e, int count, int nc, int *fr, int *c)
{
    if (a.ff) {
        *fr = e / nc;
        *c = e - *fr * nc;
    } else {
        *c = e / count;
        *fr = e - *c * count;
    }
}

// source frames [f0, f1), columns [c0, c0 + nc), into stage[(f - f0) * kSlStride + c]: every element is loaded once, by one lane
__device__ __forceinline__ void fp_stage(const FpArgs &a, const float *rb, int64_t f0, int64_t f1, int c0, int nc, float *stage)
{
    const int count = (int)(f1 - f0);
    for (int e = threadIdx.x; e < count * nc; e += kFpBlock) {
        int fr, c;
        fp_split(a, e, count, nc, &fr, &c);
        stage[fr * kSlStride + c] = fp_ld(a, rb, f0 + fr, c0 + c);
    }
}

// element (t, block i, column c0 + c) of the tensor behind the source, from source frames staged from s0 on (the taps' clamped frames
// among them): block 0 is the source, block i its i-th delta -- the fused chain over the scales; i is uniform in a workgroup
__device__ __forceinline__ float fp_val(const FpArgs &a, const float *stage, int64_t s0, int64_t n, int64_t t, int i, int c)
{
    if (i == 0) return stage[(t - s0) * kSlStride + c];
    const int H = i * a.w, off = scales_offset(i, a.w);
    float acc = 0.0f;
    for (int j = -H; j <= H; ++j) {
        const float s = a.sc[off + j + H];
        if (s != 0.0f) {
            int64_t u = t + j;
            u = u < 0 ? 0 : (u > n - 1 ? n - 1 : u);
            acc = fmaf(s, stage[(u - s0) * kSlStride + c], acc);
        }
    }
    return acc;
}

// fp_val of frames [f0, f1) into vals[(f - base) * kSlStride + c].  Block 0: the source goes straight into `vals`.  A delta block: the
// frames and their halo go through `stage` first, so the chain reads LDS.  Every thread of the workgroup calls it (a delta block has
// two barriers inside; f0, f1 and vi are uniform); the caller's barrier stands before `vals` is read
__device__ __forceinline__ void fp_values(const FpArgs &a, const float *rb, int64_t n, int64_t f0, int64_t f1, int64_t base, int vi, int c0, int nc,
                                          float *vals, float *stage)
{
    if (vi == 0) {
        if (f1 > f0) fp_stage(a, rb, f0, f1, c0, nc, vals + (f0 - base) * kSlStride);
        return;
    }
    const int H = vi * a.w;
    const int64_t s0 = f0 - H > 0 ? f0 - H : 0, s1 = f1 + H < n ? f1 + H : n;
    if (f1 > f0) fp_stage(a, rb, s0, s1, c0, nc, stage);
    __syncthreads();
    const int count = (int)(f1 - f0);
    for (int e = threadIdx.x; e < count * nc; e += kFpBlock) {
        const int fr = e / nc, c = e - fr * nc;
        vals[(f0 + fr - base) * kSlStride + c] = fp_val(a, stage, s0, n, f0 + fr, vi, c);
    }
    __syncthreads();  // (`stage` is free again)
}

// One workgroup per (row, chunk, 32 columns): the chunk's values into LDS side by side, then one thread per column adds its 64 in
// float64, frames ascending
__global__ __launch_bounds__(kFpBlock) void featpost_chunk_kernel(const FpArgs a)
{
    __shared__ float vals[kFpChunk * kSlStride];
    __shared__ float stage[kTileStage * kSlStride];
    const int i = a.block0 + (int)blockIdx.z, vi = a.delta_view ? i : 0;
    const FpTile tile = fp_tile(a);
    const int64_t k = tile.t0 / kFpChunk;
    for (int64_t r = blockIdx.y; r < a.n_rows; r += gridDim.y) {  // (every thread of the workgroup takes the same rounds: the barriers are uniform)
        const vpz_feat_row row = a.rows[r];
        const int64_t n = row.real_frames;
        const int cnt = tile.t0 < n ? (int)(n - tile.t0 < kFpChunk ? n - tile.t0 : kFpChunk) : 0;
        const float *rb = cnt > 0 ? a.src + row.src_row * a.src_row_elems : nullptr;
        fp_values(a, rb, n, tile.t0, tile.t0 + cnt, tile.t0, vi, tile.c0, tile.nc, vals, stage);
        __syncthreads();
        if (cnt > 0 && (int)threadIdx.x < tile.nc) {
            double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
            for (int fr = 0; fr < cnt; ++fr) {
                const double x = (double)vals[fr * kSlStride + threadIdx.x];
                s1 += x;
                s2 = fma(x, x, s2);
            }
            a.chunks[(r * a.nck + k) * a.ncols_norm + (i * a.D + tile.c0 + (int)threadIdx.x)] = make_double2(s1, s2);
        }
        __syncthreads();  // (the next round fills the LDS again)
    }
}

// One workgroup per (row, tile of 64 frames, 32 columns), for every delta block of the launch: the tile's source frames and the halo of
// the launch's longest chain go into LDS once -- each source element is read from memory once --, and every destination element of the
// tile is pad_value, or fp_val from LDS, or (VPZ_NORM_ROW) that normalised by the sum of its row's chunk sums, which one thread per column
// adds once for the workgroup, chunks ascending
__global__ __launch_bounds__(kFpBlock) void featpost_apply_kernel(const FpArgs a)
{
    __shared__ float stage[kTileStage * kSlStride];
    __shared__ double2 sums[kSlCols];
    const FpTile tile = fp_tile(a);
    const int H = a.delta_view ? (a.block0 + a.nblocks - 1) * a.w : 0;
    for (int64_t r = blockIdx.y; r < a.n_rows; r += gridDim.y) {  // (every thread of the workgroup takes the same rounds: the barriers are uniform)
        const vpz_feat_row row = a.rows[r];
        const int64_t n = row.real_frames;
        float *ob = a.dst + row.row * a.dst_row_elems;
        const int cnt = tile.t0 < n ? (int)(n - tile.t0 < kFpChunk ? n - tile.t0 : kFpChunk) : 0;
        int64_t s0 = 0;
        if (cnt > 0) {
            const float *rb = a.src_is_dst ? ob : a.src + row.src_row * a.src_row_elems;
            const int64_t s1 = tile.t0 + cnt + H < n ? tile.t0 + cnt + H : n;
            s0 = tile.t0 - H > 0 ? tile.t0 - H : 0;
            fp_stage(a, rb, s0, s1, tile.c0, tile.nc, stage);
        }
        __syncthreads();
        for (int ib = 0; ib < a.nblocks; ++ib) {
            const int i = a.block0 + ib, vi = a.delta_view ? i : 0;
            if (a.norm != VPZ_NORM_NONE) {  // VPZ_NORM_ROW (the sliding window has a kernel of its own): no partial chunk but the row's last
                if (cnt > 0 && (int)threadIdx.x < tile.nc) {
                    const double2 *ck = a.chunks + r * a.nck * a.ncols_norm + (i * a.D + tile.c0 + (int)threadIdx.x);
                    double s1 = 0.0, s2 = 0.0;
                    for (int64_t u = 0; u < n; u += kFpChunk) {
                        const double2 s = ck[(u / kFpChunk) * a.ncols_norm];
                        s1 += s.x;
                        s2 += s.y;
                    }
                    sums[threadIdx.x] = make_double2(s1, s2);
                }
                __syncthreads();
            }
            for (int e = threadIdx.x; e < kFpChunk * tile.nc; e += kFpBlock) {
                int tt, c;
                fp_split(a, e, kFpChunk, tile.nc, &tt, &c);
                const int64_t t = tile.t0 + tt;
                if (t >= a.T) continue;
                const int col = i * a.D + tile.c0 + c;
                float out = a.pad;
                if (t < n) {
                    out = fp_val(a, stage, s0, n, t, vi, c);
                    if (a.norm != VPZ_NORM_NONE) out = fp_normalised(a, out, sums[c].x, sums[c].y, n);
                }
                ob[a.ff ? t * a.D_out + col : (int64_t)col * a.T + t] = out;
            }
            if (a.norm != VPZ_NORM_NONE) __syncthreads();  // (the next block's sums)
        }
        __syncthreads();  // (the next round fills the LDS again)
    }
}

// VPZ_NORM_SLIDING: one workgroup per (row, tile of 64 frames, 32 columns) and delta block
__global__ __launch_bounds__(kFpBlock) void featpost_slide_kernel(const FpArgs a)
{
    extern __shared__ float lds[];  // the values; behind them, in a launch over the delta view, the staged source (slide_lds_bytes)
    float *stage = lds + kSlRows * kSlStride;
    const int i = a.block0 + (int)blockIdx.z, vi = a.delta_view ? i : 0;
    const FpTile tile = fp_tile(a);
    const int64_t t0 = tile.t0;
    const int c0 = tile.c0, nc = tile.nc;
    for (int64_t r = blockIdx.y; r < a.n_rows; r += gridDim.y) {  // (every thread of the workgroup takes the same rounds: the barriers are uniform)
        const vpz_feat_row row = a.rows[r];
        const int64_t n = row.real_frames;
        float *ob = a.dst + row.row * a.dst_row_elems;
        const float *rb = nullptr;
        int64_t lbase = 0, rbase = 0, l0 = 0, l1 = 0, r1 = 0, o1 = t0;
        if (t0 < n) {
            rb = a.src + row.src_row * a.src_row_elems;
            // both ends of the window move by 0 or 1 from a frame to the next: the windows of the tile's frames start between its first
            // frame's start a0 and its last frame's a1 <= a0 + 63, and end between b0 and b1 <= b0 + 63.  The left partial chunks lie in
            // [a0, the chunk boundary at or behind a1), the right ones in [the boundary at or before b0, b1): only those are staged
            const int64_t tl = t0 + kFpChunk - 1 < n - 1 ? t0 + kFpChunk - 1 : n - 1;
            int64_t a0, b0, a1, b1;
            cmn_window(a.norm, a.center, a.W, a.minw, t0, n, &a0, &b0);
            cmn_window(a.norm, a.center, a.W, a.minw, tl, n, &a1, &b1);
            lbase = a0 / kFpChunk * kFpChunk;
            rbase = b0 / kFpChunk * kFpChunk;
            l0 = a0;
            l1 = (a1 + kFpChunk - 1) / kFpChunk * kFpChunk;
            if (l1 > b1) l1 = b1;
            r1 = b1;
            o1 = tl + 1;
        }
        fp_values(a, rb, n, l0, l1, lbase, vi, c0, nc, lds, stage);
        fp_values(a, rb, n, rbase, r1, rbase, vi, c0, nc, lds + kSlRegion * kSlStride, stage);
        fp_values(a, rb, n, t0, o1, t0, vi, c0, nc, lds + 2 * kSlRegion * kSlStride, stage);
        __syncthreads();
        for (int e = threadIdx.x; e < kFpChunk * nc; e += kFpBlock) {
            int tt, c;
            fp_split(a, e, kFpChunk, nc, &tt, &c);
            const int64_t t = t0 + tt;
            if (t >= a.T) continue;
            const int col = i * a.D + c0 + c;
            float out = a.pad;
            if (t < n) {
                int64_t wa, wb;
                cmn_window(a.norm, a.center, a.W, a.minw, t, n, &wa, &wb);
                const double2 *ck = a.chunks + r * a.nck * a.ncols_norm + col;
                const float *left = lds + c, *right = lds + kSlRegion * kSlStride + c;
                double s1 = 0.0, s2 = 0.0;
                int64_t u = (wa + kFpChunk - 1) / kFpChunk * kFpChunk;
                if (u > wb) u = wb;
                if (u > wa) {  // the left partial chunk, or the whole window when it crosses no boundary
                    double l1s = 0.0, l2s = 0.0;
#pragma unroll 8
                    for (int64_t f = wa; f < u; ++f) {  // (unrolled: the LDS loads of eight frames go out together, the adds stay in order)
                        const double x = (double)left[(f - lbase) * kSlStride];
                        l1s += x;
                        l2s = fma(x, x, l2s);
                    }
                    s1 += l1s;
                    s2 += l2s;
                }
                for (; u + kFpChunk <= wb; u += kFpChunk) {
                    const double2 s = ck[(u / kFpChunk) * a.ncols_norm];
                    s1 += s.x;
                    s2 += s.y;
                }
                if (u < wb) {  // the right partial chunk; where the window ends with the row, the row's last chunk sum is that sum
                    double r1s = 0.0, r2s = 0.0;
                    if (wb == n) {
                        const double2 s = ck[(u / kFpChunk) * a.ncols_norm];
                        r1s = s.x;
                        r2s = s.y;
                    } else {
#pragma unroll 8
                        for (int64_t f = u; f < wb; ++f) {
                            const double x = (double)right[(f - rbase) * kSlStride];
                            r1s += x;
                            r2s = fma(x, x, r2s);
                        }
                    }
                    s1 += r1s;
                    s2 += r2s;
                }
                out = fp_normalised(a, lds[(2 * kSlRegion + tt) * kSlStride + c], s1, s2, wb - wa);
            }
            ob[a.ff ? t * a.D_out + col : (int64_t)col * a.T + t] = out;
        }
        __syncthreads();  // (the next round fills the LDS again)
    }
}

// the sliding kernel's dynamic LDS: three workgroups a CU without the delta view, two with it
size_t slide_lds_bytes(bool view) { return sizeof(float) * kSlStride * (size_t)(kSlRows + (view ? kRegionStage : 0)); }

bool spec_ok(const vpz_feat_post_spec &s)
{
    if (s.norm != VPZ_NORM_NONE && s.norm != VPZ_NORM_ROW && s.norm != VPZ_NORM_SLIDING) return false;
    if ((s.norm_vars != 0 && s.norm_vars != 1) || (s.center != 0 && s.center != 1)) return false;
    if (s.cmn_window < 1 || s.cmn_window > VPZ_FEAT_MAX_CMN_WINDOW || s.min_window < 1 || s.min_window > s.cmn_window) return false;
    if (s.delta_order < 0 || s.delta_order > VPZ_FEAT_MAX_DELTA_ORDER) return false;
    if (s.delta_window < 1 || s.delta_window > VPZ_FEAT_MAX_DELTA_WINDOW) return false;
    if (s.order != VPZ_POST_NORM_FIRST && s.order != VPZ_POST_DELTAS_FIRST) return false;
    if (s.layout != VPZ_FEAT_COLUMNS_FIRST && s.layout != VPZ_FEAT_FRAMES_FIRST) return false;
    if (!std::isfinite(s.var_floor) || !(s.var_floor > 0.0) || !std::isfinite(s.pad_value)) return false;
    for (int32_t word : s.reserved)
        if (word != 0) return false;
    return s.norm != VPZ_NORM_NONE || s.delta_order != 0;
}

// s_i of item 1: the integers N_i over Z^i, one division in double each
void delta_scales(int w, int i, float *out)
{
    std::vector<int64_t> prev{1}, cur;
    int64_t Z = 0, Zi = 1;
    for (int j = -w; j <= w; ++j) Z += (int64_t)j * j;
    for (int m = 1; m <= i; ++m) {
        cur.assign((size_t)(2 * m * w + 1), 0);
        const int hp = (m - 1) * w;
        for (int k = -m * w; k <= m * w; ++k)
            for (int j = -w; j <= w; ++j)
                if (k - j >= -hp && k - j <= hp) cur[(size_t)(k + m * w)] += (int64_t)j * prev[(size_t)(k - j + hp)];
        prev.swap(cur);
        Zi *= Z;
    }
    for (size_t k = 0; k < prev.size(); ++k) out[k] = (float)((double)prev[k] / (double)Zi);
}

// the normalised columns of a call and its scratch elements (float64); false: the size overflows
bool scratch_need(const vpz_feat_post_spec &s, int64_t n_rows, int64_t T, int32_t D, int64_t *elems)
{
    if (s.norm == VPZ_NORM_NONE) {
        *elems = 0;
        return true;
    }
    const int64_t cols = s.order == VPZ_POST_DELTAS_FIRST ? (int64_t)D * (s.delta_order + 1) : D;
    const unsigned __int128 need = (unsigned __int128)(uint64_t)n_rows * (uint64_t)((T + kFpChunk - 1) / kFpChunk) * (uint64_t)cols * 2u;
    if (need > (uint64_t)INT64_MAX / sizeof(double)) return false;
    *elems = (int64_t)need;
    return true;
}

bool ranges_overlap(const void *p, uint64_t pn, const void *q, uint64_t qn)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return pn != 0 && qn != 0 && a < b + qn && b < a + pn;
}

}  // namespace

}  // namespace vpz

extern "C" int vpz_feat_delta_scales(const vpz_feat_post_spec *spec, int32_t i, float *scales, int64_t capacity)
{
    if (!spec || capacity < 0 || !vpz::spec_ok(*spec) || i < 0 || i > spec->delta_order) return VPZ_E_INVALID_ARG;
    if (!scales) return VPZ_OK;
    if (capacity < 2 * (int64_t)i * spec->delta_window + 1) return VPZ_E_CAPACITY;
    vpz::delta_scales(spec->delta_window, i, scales);
    return VPZ_OK;
}

extern "C" int vpz_feat_cmn_window(const vpz_feat_post_spec *spec, int64_t t, int64_t n, int64_t *a, int64_t *b)
{
    if (!spec || !a || !b || !vpz::spec_ok(*spec) || spec->norm == VPZ_NORM_NONE || n < 1 || t < 0 || t >= n) return VPZ_E_INVALID_ARG;
    vpz::cmn_window(spec->norm, spec->center, spec->cmn_window, spec->min_window, t, n, a, b);
    return VPZ_OK;
}

extern "C" int vpz_feat_post_scratch(const vpz_feat_post_spec *spec, int32_t n_rows, int64_t T, int32_t D, int64_t *elems)
{
    if (!spec || !elems || !vpz::spec_ok(*spec) || n_rows < 0 || T < 1 || D < 1 || D > VPZ_FEAT_MAX_COLUMNS) return VPZ_E_INVALID_ARG;
    return vpz::scratch_need(*spec, n_rows, T, D, elems) ? VPZ_OK : VPZ_E_INVALID_ARG;
}

extern "C" int vpz_feat_post(vpz_context *c, const void *src_dev, int64_t src_rows, int64_t T, int32_t D, const vpz_feat_post_spec *spec,
                             int32_t n_rows, const vpz_feat_row *rows, void *dst_dev, int64_t dst_rows, void *scratch_dev, int64_t scratch_elems)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!spec || !rows) return refuse("vpz_feat_post: null pointer");
    if (!vpz::spec_ok(*spec)) return refuse("vpz_feat_post: a spec outside the limits");
    if (D < 1 || D > VPZ_FEAT_MAX_COLUMNS || T < 1) return refuse("vpz_feat_post: D outside 1 .. 256 or T < 1");
    if (src_rows < 0 || dst_rows < 0 || n_rows < 0 || scratch_elems < 0) return refuse("vpz_feat_post: a negative count");
    const vpz_feat_post_spec &s = *spec;
    const int32_t D_out = D * (s.delta_order + 1);
    // (sizes in bytes must fit 63 bits, so that every element index a kernel forms fits an int64_t)
    const unsigned __int128 src_elems = (unsigned __int128)(uint64_t)src_rows * (uint64_t)T * (uint64_t)D;
    const unsigned __int128 row_elems = (unsigned __int128)(uint64_t)T * (uint64_t)D_out;
    if (src_elems > (uint64_t)INT64_MAX / sizeof(float) || row_elems > (uint64_t)INT64_MAX / sizeof(float)) return refuse("vpz_feat_post: sizes overflow");
    int64_t need = 0;
    if (!vpz::scratch_need(s, n_rows, T, D, &need)) return refuse("vpz_feat_post: sizes overflow");

    // the descriptors as a row launch's: window [src_row * T * D, + n * D) of the source's elements, in rows of T * D elements
    std::vector<vpz_pack_row> as_pack;
    try {
        as_pack.reserve((size_t)n_rows);
    } catch (const std::bad_alloc &) {
        return vpz::set_error(ctx, VPZ_E_NOMEM, "vpz_feat_post: out of host memory");
    }
    bool any_real = false;  // (descriptors without real frames -- pad rows -- need neither chunk sums nor scratch memory)
    for (int32_t r = 0; r < n_rows; ++r) {
        const vpz_feat_row &d = rows[r];
        any_real = any_real || d.real_frames > 0;
        if (d.real_frames < 0 || d.real_frames > T) return refuse("vpz_feat_post: a descriptor's real frames exceed T");
        // (a row without real frames reads nothing: it may name a row of a source that has none)
        if (d.src_row < 0 || (d.real_frames > 0 && d.src_row >= src_rows)) return refuse("vpz_feat_post: a descriptor's source row is out of range");
        as_pack.push_back(vpz_pack_row{d.real_frames > 0 ? d.src_row * T * D : 0, d.real_frames * D, d.row});
    }
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_feat_post", src_dev, (int64_t)src_elems, sizeof(float), 1, 1, 1, T * D, n_rows,
                                                       n_rows ? as_pack.data() : reinterpret_cast<const vpz_pack_row *>(rows),
                                                       dst_dev, dst_rows, row_elems, sizeof(float)});
    if (rc != VPZ_OK) return rc;
    const uint64_t src_bytes = (uint64_t)src_elems * sizeof(float), dst_bytes = (uint64_t)(row_elems * (uint64_t)dst_rows) * sizeof(float);
    if (vpz::ranges_overlap(src_dev, src_bytes, dst_dev, dst_bytes)) return refuse("vpz_feat_post: source and destination overlap");
    if (!any_real) need = 0;
    if (need > 0) {
        if (!scratch_dev) return refuse("vpz_feat_post: null pointer");
        if (scratch_elems < need) return vpz::set_error(ctx, VPZ_E_CAPACITY, "vpz_feat_post: the scratch memory is too small");
        const uint64_t bytes = (uint64_t)need * sizeof(double);
        if (reinterpret_cast<uintptr_t>(scratch_dev) % sizeof(double2)) return refuse("vpz_feat_post: the scratch memory is not aligned to 16 bytes");
        if (!vpz::device_range(ctx, scratch_dev, bytes))
            return refuse("vpz_feat_post: the scratch memory is not device memory of the context's device, or leaves its allocation");
        if (vpz::ranges_overlap(scratch_dev, bytes, src_dev, src_bytes) || vpz::ranges_overlap(scratch_dev, bytes, dst_dev, dst_bytes))
            return refuse("vpz_feat_post: the scratch memory overlaps the source or the destination");
    }
    if (n_rows == 0) return VPZ_OK;
    const int64_t nck = (T + vpz::kFpChunk - 1) / vpz::kFpChunk;
    const int64_t tile_blocks = nck * ((D + vpz::kSlCols - 1) / vpz::kSlCols);
    if (tile_blocks > 0x7fffffff) return refuse("vpz_feat_post: a row too long for one launch");

    vpz::FpArgs a;
    memset(&a, 0, sizeof a);
    const vpz_pack_row *d_rows = nullptr;
    rc = vpz::upload_rows(ctx, n_rows, reinterpret_cast<const vpz_pack_row *>(rows), &d_rows);
    if (rc != VPZ_OK) return rc;
    a.rows = reinterpret_cast<const vpz_feat_row *>(d_rows);
    a.src = static_cast<const float *>(src_dev);
    a.dst = static_cast<float *>(dst_dev);
    a.chunks = static_cast<double2 *>(scratch_dev);
    a.T = T;
    a.src_row_elems = T * D;
    a.dst_row_elems = T * D_out;
    a.nck = nck;
    a.var_floor = s.var_floor;
    a.pad = (float)s.pad_value;
    a.n_rows = n_rows;
    a.D = D;
    a.D_out = D_out;
    a.src_cols = D;
    a.ff = s.layout == VPZ_FEAT_FRAMES_FIRST;
    a.w = s.delta_window;
    a.norm = s.norm;
    a.norm_vars = s.norm_vars;
    a.center = s.center;
    a.W = s.cmn_window;
    a.minw = s.min_window;
    for (int i = 1; i <= s.delta_order; ++i) vpz::delta_scales(s.delta_window, i, a.sc + vpz::scales_offset(i, s.delta_window));

    const unsigned gy = (unsigned)std::min<int32_t>(n_rows, vpz::kFpMaxGridY);
    const bool deltas = s.delta_order > 0, norm = s.norm != VPZ_NORM_NONE;
    // the blocks that the normalisation covers: all of them behind the deltas, block 0 in front of them or alone
    const bool view = deltas && (!norm || s.order == VPZ_POST_DELTAS_FIRST);
    const unsigned nz = view ? (unsigned)s.delta_order + 1 : 1;
    a.delta_view = view;
    a.ncols_norm = view ? D_out : D;
    a.nblocks = (int32_t)nz;
    if (norm && any_real) {
        vpz::featpost_chunk_kernel<<<dim3((unsigned)tile_blocks, gy, nz), vpz::kFpBlock, 0, ctx->stream>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "featpost_chunk kernel launch", e);
    }
    if (s.norm == VPZ_NORM_SLIDING)
        vpz::featpost_slide_kernel<<<dim3((unsigned)tile_blocks, gy, nz), vpz::kFpBlock, vpz::slide_lds_bytes(view), ctx->stream>>>(a);
    else
        vpz::featpost_apply_kernel<<<dim3((unsigned)tile_blocks, gy, 1), vpz::kFpBlock, 0, ctx->stream>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "featpost_apply / featpost_slide kernel launch", e);
    if (deltas && !view) {  // VPZ_POST_NORM_FIRST: the deltas of block 0, which the launch before wrote into the destination
        a.src = a.dst;
        a.src_is_dst = 1;
        a.src_cols = D_out;
        a.norm = VPZ_NORM_NONE;
        a.delta_view = 1;
        a.block0 = 1;
        a.nblocks = s.delta_order;
        vpz::featpost_apply_kernel<<<dim3((unsigned)tile_blocks, gy, 1), vpz::kFpBlock, 0, ctx->stream>>>(a);
        e = hipGetLastError();
        if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "featpost_apply kernel launch", e);
    }
    return VPZ_OK;
}
