// vpz_pcm_stft and vpz_stft_table (include/vorbispizza_pcm_stft.h, which states the definition; the network is
// include/vorbispizza_pcm_melspec.h's): windows of a float32 device PCM array as short-time Fourier spectrograms -- complex, magnitude
// or power -- with transforms of 512 to 8192 samples, one launch.  The complex arithmetic and the span staging are real_fft.hpp's; the
// passes are the network of pcm_melspec.hip, and tests/test_rfft_one_network_gpu.py holds the two kernels to each other bit for bit.
//
// The mapping:
//   a TILE is Tt consecutive frames [t0, t0 + Tt) of one destination row (Tt = 32, 16, 8, 4, 2 or 1: the largest whose LDS fits, chosen
//   by the launch from the spec alone); one workgroup of four waves per tile and descriptor;
//   the tile's SOURCE SPAN -- extended samples t0 * hop - n_fft/2 up to the last sample of the tile's last frame -- is staged in LDS
//   once, the zero extension [L, F) and the reflection at both ends resolved in the staging index, so a frame is a plain slice of it;
//   a frame's transform takes kLanes = min(H/4, 256) lanes, a lane one radix-4 butterfly of a pass at a time (H = n_fft/2): at n_fft
//   2048 and above the workgroup takes the tile's frames ONE AFTER THE OTHER, as pcm_melspec.hip does; at 1024 and 512 H/4 is 128 and 64
//   lanes, and the workgroup carries G = 2 or 4 frames of the tile SIDE BY SIDE -- lane t works on frame t / kLanes of the round as lane
//   t % kLanes, by the same lane-to-butterfly rule; every frame has its own pair of complex LDS arrays, and the barriers between the
//   passes are the workgroup's.  A frame's bits depend on its n_fft samples only;
//   a lane's window values and twiddles are the same for every frame and are read from the table (3 * n_fft floats) once, into registers;
//   the split pass turns Z[k], Z[H-k] into X[k], X[H-k] in registers.  VPZ_STFT_FRAMES_FIRST: a frame's spectrum is one contiguous run of
//   the destination and is stored from the registers, consecutive lanes consecutive bins.  VPZ_STFT_BINS_FIRST: the spectra of the
//   tile's frames are staged in LDS ([Tt][n_freq] values), and after the tile's last frame one lane per (bin, frame) stores, consecutive
//   lanes running along t.
//   LDS floats: G * 2 n_fft (the complex arrays) + (Tt - 1) hop + n_fft, rounded up to even (the span) + bins-first: Tt * n_freq values
//   of one float or two (the stage).
//   A tile whose span lies wholly in a row's zeros stores zeros without transforming.
// All element indices are 64-bit.  No scratch memory.  Built with -ffp-contract=off: every fused step is written as one.
#include <algorithm>
#include <array>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "device_table.hpp"
#include "stft_tables.hpp"
#include "real_fft.hpp"
#include "../../include/vorbispizza_pcm_stft.h"

namespace vpz {

namespace {

constexpr int kStBlock = 256;        // lanes of a workgroup: four waves
constexpr int kStLdsFloats = 40960;  // 160 KiB: what a workgroup may use (pcm_melspec.hip's kMsLdsFloats)
constexpr int kStMaxGridY = 2048;    // descriptors side by side in the grid's y; a workgroup takes every kStMaxGridY-th beyond that
constexpr int kStMaxTile = 32;       // the tile sizes: kStMaxTile, halved down to the frames a workgroup carries side by side

struct StftArgs {
    const float *src;
    const vpz_pack_row *rows;
    float *dst;
    const float *table;  // [3 * n_fft]: the window, then t[k] = (cos, -sin)
    int64_t frames, T;
    int32_t n_rows, hop, output, frames_first;
    int32_t Tt, span_cap;  // frames of a tile; floats of the span (even)
};

// one bin of one frame on its way out: `at` is the value's index in the destination row or in the stage
__device__ __forceinline__ void emit(float *to, int64_t at, float2 X, int output)
{
    if (output == VPZ_STFT_COMPLEX) {
        reinterpret_cast<float2 *>(to)[at] = X;
    } else {
        const float P = __builtin_fmaf(X.x, X.x, X.y * X.y);
        to[at] = output == VPZ_STFT_POWER ? P : __builtin_sqrtf(P);  // (the correctly rounded root: the build's default for sqrtf)
    }
}

template <int N>
__global__ __launch_bounds__(kStBlock) void pcm_stft_kernel(const StftArgs a)
{
    constexpr int H = N / 2, Q = H / 4, NF = H + 1;
    constexpr int kLanes = Q < kStBlock ? Q : kStBlock;  // lanes of one frame's transform
    constexpr int G = kStBlock / kLanes;                 // frames side by side
    constexpr int kPasses = H >= 4096 ? 6 : H >= 1024 ? 5 : 4;
    constexpr bool kRadix2 = H == 512 || H == 2048;
    constexpr int kPer = Q / kLanes, kWin = H / kLanes, kSplit = H / 2 / kLanes + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int t = threadIdx.x, g = t / kLanes, tl = t % kLanes;
    float2 *const buf0 = reinterpret_cast<float2 *>(lds) + g * N, *const buf1 = buf0 + H;  // frame g of a round: its own pair
    float *const span = lds + G * 2 * N, *const stage = span + a.span_cap;
    const int hop = a.hop, Tt = a.Tt, output = a.output;
    const int64_t F = a.frames, T = a.T;
    const int64_t t0 = (int64_t)blockIdx.x * Tt;
    const int nt = (int)(T - t0 < Tt ? T - t0 : Tt);  // the tile's frames (the grid covers T)
    const int64_t lo = t0 * hop - H;                  // the span's first extended sample
    const int count = (nt - 1) * hop + N;             // its samples
    const float2 *const win = reinterpret_cast<const float2 *>(a.table);
    const float2 *const tw = reinterpret_cast<const float2 *>(a.table + N);
    // what a lane reads from the table does not depend on the frame: its window values, the twiddles of its butterflies in every pass
    // and of its bins in the split pass are loaded once, so that no pass waits for L2
    float2 wv[kWin], t1[kPasses][kPer], t2[kPasses][kPer], t3[kPasses][kPer], ts[kSplit];
#pragma unroll
    for (int u = 0; u < kWin; ++u) wv[u] = win[tl + u * kLanes];
#pragma unroll
    for (int ps = 0; ps < kPasses; ++ps)
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int k1 = 2 * (((tl + u * kLanes) >> (2 * ps)) << (2 * ps));  // 2 p s: p = i >> ls, s = 1 << ls, ls = 2 ps
            t1[ps][u] = tw[k1];
            t2[ps][u] = tw[2 * k1];
            t3[ps][u] = tw[3 * k1];
        }
#pragma unroll
    for (int u = 0; u < kSplit; ++u) ts[u] = tw[min(tl + u * kLanes, H / 2)];
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_pack_row d = a.rows[r];
        const int64_t L = d.samples;
        const bool silent = span_silent(lo, count, F, L);
        if (!silent) {
            span_stage<kStBlock>(span, a.src + d.src, lo, count, F, L, t);
            __syncthreads();
            for (int f0 = 0; f0 < nt; f0 += G) {
                const int f = f0 + g;
                const bool on = f < nt;  // (a round's last frames may lie behind the tile: their lanes keep the barriers)
                if (on) {
                    const float *x = span + f * hop;
#pragma unroll
                    for (int u = 0; u < kWin; ++u) {
                        const int j = tl + u * kLanes;
                        buf0[j] = make_float2(x[2 * j] * wv[u].x, x[2 * j + 1] * wv[u].y);
                    }
                }
                __syncthreads();
                float2 *in = buf0, *out = buf1;
                // the radix-4 passes: length n = H >> ls, stride s = 1 << ls
#pragma unroll
                for (int ps = 0; ps < kPasses; ++ps) {
                    const int ls = 2 * ps, s = 1 << ls;
                    if (on) {
#pragma unroll
                        for (int u = 0; u < kPer; ++u) {
                            const int i = tl + u * kLanes;
                            const int p = i >> ls, q = i & (s - 1);
                            const float2 va = in[i], vb = in[i + Q], vc = in[i + 2 * Q], vd = in[i + 3 * Q];
                            const float2 apc = cadd(va, vc), amc = csub(va, vc), bpd = cadd(vb, vd), bmd = csub(vb, vd);
                            const int o = q + (p << (ls + 2));
                            out[o] = cadd(apc, bpd);
                            out[o + s] = cmul(t1[ps][u], make_float2(amc.x + bmd.y, amc.y - bmd.x));      // (a - c) - i (b - d)
                            out[o + 2 * s] = cmul(t2[ps][u], csub(apc, bpd));
                            out[o + 3 * s] = cmul(t3[ps][u], make_float2(amc.x - bmd.y, amc.y + bmd.x));  // (a - c) + i (b - d)
                        }
                    }
                    __syncthreads();
                    float2 *const sw = in;
                    in = out;
                    out = sw;
                }
                if (kRadix2) {  // the radix-2 pass: n = 2, s = H / 2
                    if (on) {
#pragma unroll
                        for (int i = tl; i < H / 2; i += kLanes) {
                            const float2 va = in[i], vb = in[i + H / 2];
                            out[i] = cadd(va, vb);
                            out[i + H / 2] = csub(va, vb);
                        }
                    }
                    __syncthreads();
                    float2 *const sw = in;
                    in = out;
                    out = sw;
                }
                // the split pass: Z is `in`; X[k] and X[H - k] leave from the registers -- into the frame's run of the destination, or
                // into its row of the stage
                if (on) {
                    float *const to = a.frames_first ? a.dst : stage;
                    const int64_t base = a.frames_first ? (d.row * T + t0 + f) * NF : (int64_t)f * NF;
#pragma unroll
                    for (int u = 0; u < kSplit; ++u) {
                        const int k = tl + u * kLanes;
                        if (k <= H / 2) {
                            const float2 zk = in[k], zm = in[(H - k) & (H - 1)];
                            const float2 E = make_float2((zk.x + zm.x) * 0.5f, (zk.y - zm.y) * 0.5f);
                            const float2 O = make_float2((zk.y + zm.y) * 0.5f, (zm.x - zk.x) * 0.5f);  // -i (Z[k] - conj Z[H-k]) / 2
                            const float2 tO = cmul(ts[u], O);
                            const float2 X1 = cadd(E, tO), X2 = csub(E, tO);
                            emit(to, base + k, X1, output);
                            if (k < H / 2) emit(to, base + H - k, make_float2(X2.x, -X2.y), output);  // conj(E - t O); (bin H/2 is its own mirror)
                        }
                    }
                }
                __syncthreads();  // (the next round's windowing writes buf0, which may be Z)
            }
        }
        // (the next descriptor's staging writes the span, which no lane reads any more, and its barrier stands before the stage is written
        // again)
        if (!a.frames_first) {
            const int items = nt * NF;
            for (int it = t; it < items; it += kStBlock) {
                const int k = it / nt, fl = it - k * nt;
                const int64_t at = (d.row * NF + k) * T + t0 + fl;
                if (output == VPZ_STFT_COMPLEX)
                    reinterpret_cast<float2 *>(a.dst)[at] = silent ? make_float2(0.0f, 0.0f) : reinterpret_cast<const float2 *>(stage)[fl * NF + k];
                else
                    a.dst[at] = silent ? 0.0f : stage[fl * NF + k];
            }
            __syncthreads();  // (the stage is read before the next descriptor's frames write it)
        } else if (silent) {
            const int64_t base = (d.row * T + t0) * NF, items = (int64_t)nt * NF * (output == VPZ_STFT_COMPLEX ? 2 : 1);
            for (int64_t it = t; it < items; it += kStBlock) a.dst[(output == VPZ_STFT_COMPLEX ? 2 * base : base) + it] = 0.0f;
        }
    }
}

// the context's table cache, keyed by what the table is made of
int stft_table_for(Context *ctx, const vpz_stft_spec &s, const Context::LogmelDft **out)
{
    const std::array<int, 3> key = {s.n_fft, s.win_length, s.window};
    return table_for(ctx, ctx->stft_tables, key, "vpz_pcm_stft: out of host memory", out, [&](Context::LogmelDft &tb) {
        tb.cols = 0;
        std::vector<float> host(3 * (size_t)s.n_fft);
        stft_table_fill(s.n_fft, s.win_length, s.window, host.data());
        return upload(ctx, "vpz_pcm_stft: table upload", tb, {{host.data(), host.size() * sizeof(float), reinterpret_cast<void **>(&tb.d_table)}});
    });
}

// frames a workgroup carries side by side: 256 lanes over the n_fft / 8 a frame's transform takes
int side_by_side(int n_fft) { return std::max(1, kStBlock / (n_fft / 8)); }

// floats of a tile's span, rounded up to even: the stage behind it holds pairs
int span_floats(int n_fft, int hop, int Tt) { return ((Tt - 1) * hop + n_fft + 1) & ~1; }

// floats of a tile's LDS at `Tt` frames: the complex arrays, the span, and bins-first the stage
int lds_floats(const vpz_stft_spec &s, int Tt)
{
    const int stage = s.layout == VPZ_STFT_BINS_FIRST ? Tt * (s.n_fft / 2 + 1) * (s.output == VPZ_STFT_COMPLEX ? 2 : 1) : 0;
    return side_by_side(s.n_fft) * 2 * s.n_fft + span_floats(s.n_fft, s.hop, Tt) + stage;
}

}  // namespace

}  // namespace vpz

extern "C" int vpz_stft_table(int32_t n_fft, int32_t win_length, int32_t window, float *table, int64_t capacity)
{
    if (!vpz::stft_table_ok(n_fft, win_length, window) || capacity < 0) return VPZ_E_INVALID_ARG;
    if (!table) return VPZ_OK;
    if (capacity < 3 * (int64_t)n_fft) return VPZ_E_CAPACITY;
    vpz::stft_table_fill(n_fft, win_length, window, table);
    return VPZ_OK;
}

extern "C" int vpz_pcm_stft(vpz_context *c, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_stft_spec *spec, int32_t n_rows,
                            const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!spec) return refuse("vpz_pcm_stft: null pointer");
    if (!vpz::stft_spec_ok(*spec)) return refuse("vpz_pcm_stft: a spec outside the limits");
    const vpz_stft_spec &s = *spec;
    if (frames < s.n_fft / 2 + 1) return refuse("vpz_pcm_stft: frames < n_fft / 2 + 1 (the reflection needs it)");
    if (frames > INT64_MAX / 8) return refuse("vpz_pcm_stft: sizes overflow");
    const int64_t T = 1 + frames / s.hop;
    const bool complex_out = s.output == VPZ_STFT_COMPLEX;
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_stft", src_dev, src_elems, sizeof(float), 1, 1, 1, frames, n_rows, rows, dst_dev, dst_rows,
                                                       (unsigned __int128)(uint64_t)T * (uint64_t)(s.n_fft / 2 + 1) * (complex_out ? 2u : 1u), sizeof(float)});
    if (rc != VPZ_OK) return rc;
    if (complex_out && reinterpret_cast<uintptr_t>(dst_dev) % (2 * sizeof(float)) != 0)
        return refuse("vpz_pcm_stft: dst_dev is not aligned to a pair of float32");

    // the tile: the largest of 32, 16, .. down to the frames a workgroup carries side by side whose LDS fits -- the span is staged once for
    // the tile's overlapping frames, and a bins-first store runs along a tile's frames -- from the spec alone (a result does not depend on
    // the tile: the same bits).  tests/stft_truth.py restates lds_floats and this choice (tile_plan)
    vpz::StftArgs a;
    a.Tt = 0;
    for (int Tt = vpz::kStMaxTile; Tt >= vpz::side_by_side(s.n_fft); Tt /= 2) {
        if (vpz::lds_floats(s, Tt) > vpz::kStLdsFloats) continue;
        a.Tt = Tt;
        break;
    }
    if (a.Tt == 0) return vpz::set_error(ctx, VPZ_E_UNSUPPORTED, "vpz_pcm_stft: no tile fits the LDS");  // (the smallest fits at every spec inside the limits)
    const int64_t blocks = (T + a.Tt - 1) / a.Tt;
    if (blocks > 0x7fffffff) return refuse("vpz_pcm_stft: a row too long for one launch");
    if (n_rows == 0) return VPZ_OK;

    const vpz::Context::LogmelDft *tb = nullptr;
    rc = vpz::stft_table_for(ctx, s, &tb);
    if (rc != VPZ_OK) return rc;
    rc = vpz::upload_rows(ctx, n_rows, rows, &a.rows);
    if (rc != VPZ_OK) return rc;

    a.src = static_cast<const float *>(src_dev);
    a.dst = static_cast<float *>(dst_dev);
    a.table = tb->d_table;
    a.frames = frames;
    a.T = T;
    a.n_rows = n_rows;
    a.hop = s.hop;
    a.output = s.output;
    a.frames_first = s.layout == VPZ_STFT_FRAMES_FIRST;
    a.span_cap = vpz::span_floats(s.n_fft, s.hop, a.Tt);
    const dim3 grid((unsigned)blocks, (unsigned)std::min<int64_t>(n_rows, vpz::kStMaxGridY));
    const size_t lds = sizeof(float) * (size_t)vpz::lds_floats(s, a.Tt);
    void (*kernel)(vpz::StftArgs) = nullptr;
    switch (s.n_fft) {
    case 512: kernel = &vpz::pcm_stft_kernel<512>; break;
    case 1024: kernel = &vpz::pcm_stft_kernel<1024>; break;
    case 2048: kernel = &vpz::pcm_stft_kernel<2048>; break;
    case 4096: kernel = &vpz::pcm_stft_kernel<4096>; break;
    default: kernel = &vpz::pcm_stft_kernel<8192>; break;
    }
    return vpz::launch_in_lds(ctx, kernel, "pcm_stft kernel launch", a, grid, vpz::kStBlock, lds, sizeof(float) * vpz::kStLdsFloats);
}
