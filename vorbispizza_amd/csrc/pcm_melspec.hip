// vpz_pcm_melspec, vpz_melspec_twiddles and vpz_melspec_filterbank (include/vorbispizza_pcm_melspec.h, which states the definition and
// the network): windows of a mono device PCM array as (log-)mel frames with transforms of 2048, 4096 and 8192 samples, one launch, no
// spectrogram in device memory.
//
// The mapping:
//   a TILE is Tt consecutive frames [t0, t0 + Tt) of one destination row (Tt = 16, 8 or 2: the largest whose LDS fits, chosen by the
//   launch from n_fft and hop alone); one workgroup of four waves per tile and descriptor;
//   the tile's SOURCE SPAN -- extended samples t0 * hop - n_fft/2 up to the last sample of the tile's last frame -- is staged in LDS
//   once, the zero extension [L, F) and the reflection at both ends resolved in the staging index, so a frame is a plain slice of it;
//   the workgroup takes the tile's frames ONE AFTER THE OTHER, each with a transform of its own (a frame's bits depend on its n_fft
//   samples only): windowing packs the frame's even and odd samples into H = n_fft/2 complex values in LDS; every pass of the Stockham
//   network reads one LDS array and writes the other, a lane one radix-4 butterfly at a time -- its four inputs H/4 apart, so a wave
//   reads consecutive float2 --, a barrier between passes; a lane's window values and twiddles are the same for every frame and are read
//   from the table (3 * n_fft floats) once, into registers; the split pass turns Z[k], Z[H-k] into P[k], P[H-k] in the array the last
//   pass left free; then one lane per band sums its band's live bins in ascending k -- the loads of 16 steps issued together -- into the
//   MEL TILE [Tt][n_mels] in LDS;
//   after the tile's last frame one lane per (frame, band) takes the log and stores, consecutive lanes along the layout's inner
//   dimension.
//   LDS floats: 2 n_fft (the two complex arrays) + (Tt - 1) hop + n_fft (the span) + Tt * 256 (the mel tile, sized for the most bands).
//   A tile whose span lies wholly in a row's zeros stores the silence value without computing.
// The complex arithmetic and the span staging are real_fft.hpp's, shared with pcm_stft.hip, whose passes are this network once more.
// All element indices are 64-bit.  No scratch memory.  Built with -ffp-contract=off: every fused step is written as one.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "device_table.hpp"
#include "melspec_tables.hpp"
#include "real_fft.hpp"
#include "../../include/vorbispizza_pcm_melspec.h"

namespace vpz {

namespace {

constexpr int kMsBlock = 256;        // lanes of a workgroup: four waves
constexpr int kMsLdsFloats = 40960;  // 160 KiB: what a workgroup may use
constexpr int kMsMaxGridY = 2048;    // descriptors side by side in the grid's y; a workgroup takes every kMsMaxGridY-th beyond that
constexpr int kMsMelRoom = 256;      // bands the mel tile has room for per frame (VPZ_MELSPEC_MAX_MELS)
constexpr int kMsAhead = 16;         // steps of a band sum whose loads are issued together
constexpr int kMsTileA = 16;         // the tile sizes, largest first
constexpr int kMsTileB = 8;
constexpr int kMsTileC = 2;

struct MelspecArgs {
    const float *src;
    const vpz_pack_row *rows;
    float *dst;
    const float *table;   // [3 * n_fft]: the window, then t[k] = (cos, -sin)
    const int32_t *meta;  // [n_mels][3]
    const float *w;
    int64_t frames, T;
    int32_t n_rows, hop, n_mels, log, frames_first;
    int32_t Tt, span_cap;  // frames of a tile; floats of the span
    float floor, silence;
};

template <int N>
__global__ __launch_bounds__(kMsBlock) void pcm_melspec_kernel(const MelspecArgs a)
{
    constexpr int H = N / 2, Q = H / 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float2 *const buf0 = reinterpret_cast<float2 *>(lds), *const buf1 = buf0 + H;
    float *const span = lds + 2 * N, *const mel = span + a.span_cap;
    const int t = threadIdx.x;
    const int hop = a.hop, n_mels = a.n_mels, Tt = a.Tt;
    const int64_t F = a.frames, T = a.T;
    const int64_t t0 = (int64_t)blockIdx.x * Tt;
    const int nt = (int)(T - t0 < Tt ? T - t0 : Tt);  // the tile's frames (the grid covers T)
    const int64_t lo = t0 * hop - H;                  // the span's first extended sample
    const int count = (nt - 1) * hop + N;             // its samples
    const int items = nt * n_mels;
    const float2 *const win = reinterpret_cast<const float2 *>(a.table);
    const float2 *const tw = reinterpret_cast<const float2 *>(a.table + N);
    // what a lane reads from the table does not depend on the frame: its window values, the twiddles of its butterflies in every pass
    // and of its bins in the split pass are loaded once, so that no pass waits for L2
    constexpr int kPasses = H == 4096 ? 6 : 5, kPer = Q / kMsBlock, kWin = H / kMsBlock, kSplit = H / 2 / kMsBlock + 1;
    float2 wv[kWin], t1[kPasses][kPer], t2[kPasses][kPer], t3[kPasses][kPer], ts[kSplit];
#pragma unroll
    for (int u = 0; u < kWin; ++u) wv[u] = win[t + u * kMsBlock];
#pragma unroll
    for (int ps = 0; ps < kPasses; ++ps)
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int k1 = 2 * (((t + u * kMsBlock) >> (2 * ps)) << (2 * ps));  // 2 p s: p = i >> ls, s = 1 << ls, ls = 2 ps
            t1[ps][u] = tw[k1];
            t2[ps][u] = tw[2 * k1];
            t3[ps][u] = tw[3 * k1];
        }
#pragma unroll
    for (int u = 0; u < kSplit; ++u) ts[u] = tw[min(t + u * kMsBlock, H / 2)];
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_pack_row d = a.rows[r];
        const int64_t L = d.samples;
        const bool silent = span_silent(lo, count, F, L);
        if (!silent) {
            span_stage<kMsBlock>(span, a.src + d.src, lo, count, F, L, t);
            __syncthreads();
            for (int f = 0; f < nt; ++f) {
                const float *x = span + f * hop;
#pragma unroll
                for (int u = 0; u < kWin; ++u) {
                    const int j = t + u * kMsBlock;
                    buf0[j] = make_float2(x[2 * j] * wv[u].x, x[2 * j + 1] * wv[u].y);
                }
                __syncthreads();
                float2 *in = buf0, *out = buf1;
                // the radix-4 passes: length n = H >> ls, stride s = 1 << ls
#pragma unroll
                for (int ps = 0; ps < kPasses; ++ps) {
                    const int ls = 2 * ps, s = 1 << ls;
#pragma unroll
                    for (int u = 0; u < kPer; ++u) {
                        const int i = t + u * kMsBlock;
                        const int p = i >> ls, q = i & (s - 1);
                        const float2 va = in[i], vb = in[i + Q], vc = in[i + 2 * Q], vd = in[i + 3 * Q];
                        const float2 apc = cadd(va, vc), amc = csub(va, vc), bpd = cadd(vb, vd), bmd = csub(vb, vd);
                        const int o = q + (p << (ls + 2));
                        out[o] = cadd(apc, bpd);
                        out[o + s] = cmul(t1[ps][u], make_float2(amc.x + bmd.y, amc.y - bmd.x));      // (a - c) - i (b - d)
                        out[o + 2 * s] = cmul(t2[ps][u], csub(apc, bpd));
                        out[o + 3 * s] = cmul(t3[ps][u], make_float2(amc.x - bmd.y, amc.y + bmd.x));  // (a - c) + i (b - d)
                    }
                    __syncthreads();
                    float2 *const sw = in;
                    in = out;
                    out = sw;
                }
                if (H == 2048) {  // the radix-2 pass: n = 2, s = H / 2
#pragma unroll
                    for (int i = t; i < H / 2; i += kMsBlock) {
                        const float2 va = in[i], vb = in[i + H / 2];
                        out[i] = cadd(va, vb);
                        out[i + H / 2] = csub(va, vb);
                    }
                    __syncthreads();
                    float2 *const sw = in;
                    in = out;
                    out = sw;
                }
                // the split pass: Z is `in`; P[0 .. H] goes where the last pass read
                float *const P = reinterpret_cast<float *>(out);
#pragma unroll
                for (int u = 0; u < kSplit; ++u) {
                    const int k = t + u * kMsBlock;
                    if (k <= H / 2) {
                        const float2 zk = in[k], zm = in[(H - k) & (H - 1)];
                        const float2 E = make_float2((zk.x + zm.x) * 0.5f, (zk.y - zm.y) * 0.5f);
                        const float2 O = make_float2((zk.y + zm.y) * 0.5f, (zm.x - zk.x) * 0.5f);  // -i (Z[k] - conj Z[H-k]) / 2
                        const float2 tO = cmul(ts[u], O);
                        const float2 X1 = cadd(E, tO), X2 = csub(E, tO);
                        P[k] = __builtin_fmaf(X1.x, X1.x, X1.y * X1.y);
                        P[H - k] = __builtin_fmaf(X2.x, X2.x, X2.y * X2.y);  // (k = H/2 writes the same value twice)
                    }
                }
                __syncthreads();
                for (int b = t; b < n_mels; b += kMsBlock) {
                    const int first = a.meta[3 * b], cnt = a.meta[3 * b + 1];
                    const float *p = P + first, *ww = a.w + a.meta[3 * b + 2];
                    float acc = 0.0f;
                    // one chain, k ascending; the loads of kMsAhead steps are issued before the first of them is used (a step beyond the
                    // band reads the band's last bin again and is not added)
                    for (int i0 = 0; i0 < cnt; i0 += kMsAhead) {
                        float wq[kMsAhead], pq[kMsAhead];
#pragma unroll
                        for (int u = 0; u < kMsAhead; ++u) {
                            const int i = min(i0 + u, cnt - 1);
                            wq[u] = ww[i];
                            pq[u] = p[i];
                        }
#pragma unroll
                        for (int u = 0; u < kMsAhead; ++u) acc = i0 + u < cnt ? __builtin_fmaf(wq[u], pq[u], acc) : acc;
                    }
                    mel[f * n_mels + b] = acc;
                }
                __syncthreads();  // (the next frame's windowing writes buf0, which may be P)
            }
        }
        // (the next descriptor's staging writes the span, which no lane reads any more, and its barrier stands before the mel tile is
        // written again)
        for (int it = t; it < items; it += kMsBlock) {
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
                const float acc = mel[tl * n_mels + b];
                v = !a.log ? acc : acc <= a.floor ? a.silence : log10f(acc);
            }
            const int64_t at = a.frames_first ? (d.row * T + t0 + tl) * n_mels + b : (d.row * n_mels + b) * T + t0 + tl;
            a.dst[at] = v;
        }
        __syncthreads();  // (the mel tile is read before the next descriptor's frames write it)
    }
}

// (the context's one table cache: an n_fft of this stage is no n_fft of vpz_pcm_logmel, so the two share the maps without meeting)
int twiddles_for(Context *ctx, int n_fft, const Context::LogmelDft **out)
{
    return table_for(ctx, ctx->logmel_dft, n_fft, "vpz_pcm_melspec: out of host memory", out, [&](Context::LogmelDft &tb) {
        tb.cols = 0;
        std::vector<float> host(3 * (size_t)n_fft);
        melspec_twiddle_fill(n_fft, host.data());
        return upload(ctx, "vpz_pcm_melspec: twiddle table upload", tb, {{host.data(), host.size() * sizeof(float), reinterpret_cast<void **>(&tb.d_table)}});
    });
}

int melspec_bank_for(Context *ctx, const vpz_logmel_spec &s, const Context::LogmelBank **out)
{
    const std::array<double, 7> key = {s.sample_rate, (double)s.n_fft, (double)s.n_mels, s.f_min, s.f_max, (double)s.mel_scale, (double)s.mel_norm};
    return table_for(ctx, ctx->logmel_banks, key, "vpz_pcm_melspec: out of host memory", out, [&](Context::LogmelBank &bk) {
        MelFilterbank fb;
        mel_build(s, fb);
        return upload_bank(ctx, "vpz_pcm_melspec: filterbank upload", fb, bk);
    });
}

// floats of a tile's LDS at `Tt` frames: the two complex arrays, the span, the mel tile
int lds_floats(int n_fft, int hop, int Tt) { return 2 * n_fft + (Tt - 1) * hop + n_fft + Tt * kMsMelRoom; }

}  // namespace

}  // namespace vpz

extern "C" int vpz_melspec_twiddles(int32_t n_fft, float *table, int64_t capacity)
{
    if (!vpz::melspec_nfft_ok(n_fft) || capacity < 0) return VPZ_E_INVALID_ARG;
    if (!table) return VPZ_OK;
    if (capacity < 3 * (int64_t)n_fft) return VPZ_E_CAPACITY;
    vpz::melspec_twiddle_fill(n_fft, table);
    return VPZ_OK;
}

extern "C" int vpz_melspec_filterbank(const vpz_logmel_spec *spec, int32_t *first_bin, int32_t *n_bins, float *weights, int64_t capacity,
                                      int64_t *total)
{
    if (!spec || capacity < 0 || !vpz::melspec_spec_ok(*spec)) return VPZ_E_INVALID_ARG;
    return vpz::mel_filterbank_out(*spec, first_bin, n_bins, weights, capacity, total);
}

extern "C" int vpz_pcm_melspec(vpz_context *c, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_logmel_spec *spec,
                               int32_t n_rows, const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!spec) return refuse("vpz_pcm_melspec: null pointer");
    if (!vpz::melspec_spec_ok(*spec)) return refuse("vpz_pcm_melspec: a spec outside the limits");
    const vpz_logmel_spec &s = *spec;
    if (frames < s.n_fft / 2 + 1) return refuse("vpz_pcm_melspec: frames < n_fft / 2 + 1 (the reflection needs it)");
    if (frames > INT64_MAX / 8) return refuse("vpz_pcm_melspec: sizes overflow");
    const int64_t T = 1 + frames / s.hop;
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_melspec", src_dev, src_elems, sizeof(float), 1, 1, 1, frames, n_rows, rows, dst_dev, dst_rows,
                                                       (unsigned __int128)(uint64_t)T * (uint64_t)s.n_mels, sizeof(float)});
    if (rc != VPZ_OK || n_rows == 0) return rc;

    const vpz::Context::LogmelDft *tb = nullptr;
    const vpz::Context::LogmelBank *bk = nullptr;
    rc = vpz::twiddles_for(ctx, s.n_fft, &tb);
    if (rc == VPZ_OK) rc = vpz::melspec_bank_for(ctx, s, &bk);
    if (rc != VPZ_OK) return rc;

    vpz::MelspecArgs a;
    // the tile: the largest of 16, 8 and 2 frames whose LDS fits -- the span is staged once for the tile's overlapping frames, and a
    // bands-first store runs along a tile's frames -- from n_fft and hop alone (a result does not depend on the tile: the same bits).
    // 16 frames fit at every hop of n_fft 2048, up to hop 1638 at 4096 and 819 at 8192; 8 up to 3803 and 2048; 2 always.
    // tests/test_melspec_cpu.py restates lds_floats and this choice (tile_plan)
    a.Tt = 0;
    for (int Tt : {vpz::kMsTileA, vpz::kMsTileB, vpz::kMsTileC}) {
        if (vpz::lds_floats(s.n_fft, s.hop, Tt) > vpz::kMsLdsFloats) continue;
        a.Tt = Tt;
        break;
    }
    if (a.Tt == 0) return vpz::set_error(ctx, VPZ_E_UNSUPPORTED, "vpz_pcm_melspec: no tile fits the LDS");  // (2 frames fit at every spec inside the limits)
    const int64_t blocks = (T + a.Tt - 1) / a.Tt;
    if (blocks > 0x7fffffff) return refuse("vpz_pcm_melspec: a row too long for one launch");

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
    a.hop = s.hop;
    a.n_mels = s.n_mels;
    a.log = s.output == VPZ_MEL_LOG10;
    a.frames_first = s.layout == VPZ_MEL_FRAMES_FIRST;
    a.span_cap = (a.Tt - 1) * s.hop + s.n_fft;
    a.floor = a.log ? (float)s.floor : 0.0f;
    a.silence = a.log ? (float)log10((double)a.floor) : 0.0f;
    const dim3 grid((unsigned)blocks, (unsigned)std::min<int64_t>(n_rows, vpz::kMsMaxGridY));
    const size_t lds = sizeof(float) * (size_t)vpz::lds_floats(s.n_fft, s.hop, a.Tt);
    void (*const kernel)(vpz::MelspecArgs) = s.n_fft == 2048   ? &vpz::pcm_melspec_kernel<2048>
                                             : s.n_fft == 4096 ? &vpz::pcm_melspec_kernel<4096>
                                                               : &vpz::pcm_melspec_kernel<8192>;
    return vpz::launch_in_lds(ctx, kernel, "pcm_melspec kernel launch", a, grid, vpz::kMsBlock, lds, sizeof(float) * vpz::kMsLdsFloats);
}
