// vpz_pcm_fbank, vpz_fbank_table and vpz_fbank_filterbank (include/vorbispizza_pcm_fbank.h, which states the definition): windows of a
// mono device PCM array as Kaldi filterbank feature frames, one launch, neither framed copy nor spectrogram in device memory.
//
// The mapping is that of pcm_logmel.hip where the two definitions agree:
//   a TILE is Tt consecutive frames [t0, t0 + Tt) of one destination row (Tt = 64, 32 or 16, chosen by the launch); one workgroup of
//   four waves per tile and descriptor;
//   a row has T_L real frames, its own number: of a tile's frames the first nr = min(Tt, T_L - t0) are computed, the others hold
//   pad_value; a tile with nr <= 0 stores without staging or computing;
//   the SOURCE SPAN of the real frames -- samples t0 * hop up to the last sample of frame t0 + nr - 1, every one a real sample: no
//   reflection, no zero extension -- is staged in LDS once, stored SKEWED for an even hop (sample i at i + floor(i / hop)), so that the
//   32 frames a wave reads at once lie hop + 1 words apart and fall on 32 different banks;
//   THE MEAN of every frame comes from the staged span before the product: four lanes per frame sum every fourth sample in ascending
//   order, two shuffles add the partial sums as (s0 + s1) + (s2 + s3), one division by win -- the order the header states, the same at
//   every tile size -- and the value goes through LDS to the lanes that read the frame;
//   the folded operator of the frame is a matrix product on the exact float32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain):
//   the frames are the A operand, A[t][m] = span[t * hop + m] - mu[t], subtracted on the read; the table B[m][k] is the B operand, read
//   straight from L2 four k-steps ahead.  The k loop runs over win, not n_fft: floor(win / 2) steps of two samples; an odd win adds one step
//   whose second sample is 0 against a zero last table row.  A wave owns 32 bins' cos and sin columns at a time;
//   P = re^2 + im^2 goes into an LDS tile [Tt][n_fft/2, made odd] (no Nyquist column); then one lane per (frame, band) sums its band's
//   live bins in ascending k, takes the natural log and stores, consecutive lanes along the layout's inner dimension.
// All element indices are 64-bit.  No scratch memory.
//
// vpz_pcm_mfcc and vpz_mfcc_table (include/vorbispizza_pcm_mfcc.h, which states that definition) are the same tile core with three things
// more (fb_tile_core<RT, CEP = true>, launched as pcm_mfcc_kernel):
//   THE ENERGY of every frame comes from the staged span behind the mean: the same four lanes square-sum fl(x - mu) over every fourth
//   sample with one fmaf each, the same two shuffles add, and S goes to LDS beside the mean;
//   the band-sum stage writes the log-mel values into an LDS tile [Tt][n_mels, made odd] of its own instead of storing;
//   behind a barrier one lane per (frame, coefficient) runs the fmaf chain over the bands against the cepstral matrix (read from L2,
//   stored [band][coefficient] so that the lanes of a frame read side by side), puts the energy in c[0]'s place and stores, consecutive
//   lanes along the layout's inner dimension, htk_compat applied on the store index.
// subtract_mean is a second launch on the same stream, pcm_cmn_kernel: one wave per (row, stored coefficient) over the row's real frames.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "device_table.hpp"
#include "fbank_tables.hpp"
#include "mfcc_tables.hpp"
#include "../../include/vorbispizza_pcm_fbank.h"
#include "../../include/vorbispizza_pcm_mfcc.h"

namespace vpz {

namespace {

constexpr int kFbBlock = 256;        // lanes of a workgroup: four waves
constexpr int kFbCols = 32;          // bins a wave owns at a time (the MFMA's N)
constexpr int kFbLdsFloats = 40960;  // 160 KiB: what a workgroup may use
constexpr int kFbMaxGridY = 2048;    // descriptors side by side in the grid's y; a workgroup takes every kFbMaxGridY-th beyond that
constexpr int kFbAhead = 4;          // k-steps (of two samples) whose table values are loaded ahead
constexpr int kFbMeans = 64;         // floats of the tile's means in LDS (one per frame of the largest tile)

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct FbankArgs {
    const float *src;
    const vpz_pack_row *rows;
    float *dst;
    const float *table;   // [2 * ceil(win / 2)][2 * cols]
    const int32_t *meta;  // [n_mels][3]
    const float *w;
    int64_t T;
    int32_t n_rows, win, hop, nb, cols, n_mels, log, frames_first, remove_dc;
    int32_t Tt, skew, pstride, span_cap;  // frames of a tile; 1: the span is skewed; floats between two rows of the power tile; floats of the span
    float floor, log_floor, pad;
};

// what the cepstral stage of vpz_pcm_mfcc adds to a launch (CEP): a.n_mels stays the mel stage's, a.log is 1
struct CepArgs {
    const float *ct;  // the cepstral matrix, [n_mels][n_ceps]: ct[b * n_ceps + i] = C[i][b]
    int32_t n_ceps, use_energy, htk, estride;  // ...; floats between two rows of the log-mel tile
    float sc2, log_eps, log_efloor;  // fl(scale)^2; logf(2^-23); logf(energy_floor), -Inf without one
};

struct MfccArgs {
    FbankArgs f;
    CepArgs c;
};

// The tile core of both launches.  RT: 32-frame row tiles of a workgroup's tile (2 at Tt = 64, 1 at Tt <= 32); CEP: the cepstral stage
// behind the band sums (`c` is read only then).  LDS: the span, the means, [CEP: the energies,] the power tile [, CEP: the log-mel tile]
template <int RT, bool CEP>
__device__ __forceinline__ void fb_tile_core(const FbankArgs a, const CepArgs c)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *span = lds, *mean = lds + a.span_cap, *en = mean + kFbMeans, *pw = CEP ? en + kFbMeans : en, *et = pw + a.Tt * a.pstride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, h = lane >> 5;
    const int win = a.win, hop = a.hop, nb = a.nb, n_mels = a.n_mels, Tt = a.Tt, skew = a.skew, pstride = a.pstride;
    const int64_t T = a.T;
    const int64_t t0 = (int64_t)blockIdx.x * Tt;
    const int nt = (int)(T - t0 < Tt ? T - t0 : Tt);  // the tile's frames (the grid covers T)
    const int items = nt * n_mels;
    const int pairs = win / 2;                        // whole k-steps of two samples (an odd win has half a step more)
    const size_t ld = 2 * (size_t)a.cols;
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_pack_row d = a.rows[r];
        const int64_t L = d.samples;
        const int64_t TL = L < win ? 0 : 1 + (L - win) / hop;  // the row's real frames
        const int nr = (int)(TL - t0 < 0 ? 0 : TL - t0 < nt ? TL - t0 : nt);  // ... of this tile (the same for the whole workgroup)
        if (nr > 0) {
            // the last staged sample is t0 * hop + (nr - 1) * hop + win - 1 <= (TL - 1) * hop + win - 1 <= L - 1
            const float *in = a.src + d.src + t0 * hop;
            const int count = (nr - 1) * hop + win;
            for (int i = t; i < count; i += kFbBlock) span[i + (skew ? i / hop : 0)] = in[i];
            __syncthreads();
            if (a.remove_dc) {
                // four lanes per frame, 64 frames: lane q of a frame sums x[q], x[q + 4], ... (a frame behind the real ones repeats the last)
                const int f = t >> 2, q = t & 3, fr = f < nr ? f : nr - 1;
                const float *fp = span + fr * (hop + skew);
                float s = 0.0f;
                int g = q, rem = q;
                if (skew) {
                    g += q / hop;
                    rem = q % hop;
                }
                for (int m = q; m < win; m += 4) {
                    s += fp[g];
                    g += 4;
                    if (skew) {
                        rem += 4;
                        while (rem >= hop) {
                            rem -= hop;
                            ++g;
                        }
                    }
                }
                s += __shfl_xor(s, 1);  // s0 + s1 | s2 + s3
                s += __shfl_xor(s, 2);  // (s0 + s1) + (s2 + s3), the same bits in all four
                if (q == 0) mean[f] = s / (float)win;
                __syncthreads();
            }
            if constexpr (CEP) {
                if (c.use_energy) {
                    // the same four lanes per frame once more, over fl(x - mu): the A operand's own values
                    const int f = t >> 2, q = t & 3, fr = f < nr ? f : nr - 1;
                    const float *fp = span + fr * (hop + skew);
                    const float m0 = a.remove_dc ? mean[fr] : 0.0f;
                    float s = 0.0f;
                    int g = q, rem = q;
                    if (skew) {
                        g += q / hop;
                        rem = q % hop;
                    }
                    for (int m = q; m < win; m += 4) {
                        const float av = fp[g] - m0;
                        s = __builtin_fmaf(av, av, s);
                        g += 4;
                        if (skew) {
                            rem += 4;
                            while (rem >= hop) {
                                rem -= hop;
                                ++g;
                            }
                        }
                    }
                    s += __shfl_xor(s, 1);
                    s += __shfl_xor(s, 2);
                    if (q == 0) en[f] = c.sc2 * s;
                    // (no barrier of its own: the one behind the MFMA phase stands before the energies are read)
                }
            }
            int base[RT];
            float mu[RT];
            for (int rt = 0; rt < RT; ++rt) {
                const int row = rt * 32 + col, fr = row < nr ? row : nr - 1;  // (a row behind the real frames repeats the last one: its results are not stored)
                base[rt] = fr * (hop + skew);
                mu[rt] = a.remove_dc ? mean[fr] : 0.0f;
            }
            for (int k0 = wave * kFbCols; k0 < nb; k0 += (kFbBlock / 64) * kFbCols) {
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
                const int blocks = pairs / kFbAhead;
                float cre[kFbAhead], cim[kFbAhead], nre[kFbAhead], nim[kFbAhead];
                if (blocks > 0) {
#pragma unroll
                    for (int u = 0; u < kFbAhead; ++u) {
                        const float *p = tp + (size_t)(2 * u) * ld;
                        cre[u] = p[0];
                        cim[u] = p[a.cols];
                    }
                }
                for (int blk = 0; blk < blocks; ++blk) {
                    const int nxt = blk + 1 < blocks ? blk + 1 : blk;  // (the last block loads itself again: no branch)
#pragma unroll
                    for (int u = 0; u < kFbAhead; ++u) {
                        const float *p = tp + (size_t)(2 * (nxt * kFbAhead + u)) * ld;
                        nre[u] = p[0];
                        nim[u] = p[a.cols];
                    }
#pragma unroll
                    for (int u = 0; u < kFbAhead; ++u) {
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            const float av = span[base[rt] + g] - mu[rt];
                            re[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, cre[u], re[rt], 0, 0, 0);
                            im[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, cim[u], im[rt], 0, 0, 0);
                        }
                        step_a();
                    }
#pragma unroll
                    for (int u = 0; u < kFbAhead; ++u) {
                        cre[u] = nre[u];
                        cim[u] = nim[u];
                    }
                }
                for (int pr = blocks * kFbAhead; pr < pairs; ++pr) {
                    const float *p = tp + (size_t)(2 * pr) * ld;
                    const float br = p[0], bi = p[a.cols];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const float av = span[base[rt] + g] - mu[rt];
                        re[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, br, re[rt], 0, 0, 0);
                        im[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bi, im[rt], 0, 0, 0);
                    }
                    step_a();
                }
                if (win & 1) {  // the last sample alone: the step's second sample is no sample of the frame (0, against the table's zero row)
                    const float *p = tp + (size_t)(2 * pairs) * ld;
                    const float br = p[0], bi = p[a.cols];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const float av = h ? 0.0f : span[base[rt] + g] - mu[rt];
                        re[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, br, re[rt], 0, 0, 0);
                        im[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bi, im[rt], 0, 0, 0);
                    }
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
            if constexpr (CEP) {
                // the log-mel values of the real frames, into their tile: consecutive lanes along the bands
                for (int it = t; it < nr * n_mels; it += kFbBlock) {
                    const int tl = it / n_mels, b = it - tl * n_mels;
                    const int first = a.meta[3 * b], cnt = a.meta[3 * b + 1];
                    const float *p = pw + tl * pstride + first, *ww = a.w + a.meta[3 * b + 2];
                    float acc = 0.0f;
                    for (int i = 0; i < cnt; ++i) acc = __builtin_fmaf(ww[i], p[i], acc);
                    et[tl * c.estride + b] = acc <= a.floor ? a.log_floor : logf(acc);
                }
                __syncthreads();
            }
        }
        // (the next descriptor's staging writes the span, which no lane reads any more; its first barrier stands before the means and the
        // power tile are written again.  CEP: the energies and the log-mel tile have room of their own -- nothing overlays the span --, and
        // that same first barrier stands before the energies are written again, three more before the log-mel tile is: the cepstral
        // stage of this descriptor needs no barrier behind it)
        if constexpr (CEP) {
            const int n_ceps = c.n_ceps;
            for (int it = t; it < nt * n_ceps; it += kFbBlock) {
                int tl, i;
                if (a.frames_first) {
                    tl = it / n_ceps;
                    i = it - tl * n_ceps;
                } else {
                    i = it / nt;
                    tl = it - i * nt;
                }
                float v = a.pad;
                if (tl < nr) {
                    if (c.use_energy && i == 0) {
                        const float S = en[tl];
                        v = S <= 0x1p-23f ? c.log_eps : logf(S);
                        v = v < c.log_efloor ? c.log_efloor : v;
                    } else {
                        const float *e = et + tl * c.estride, *cp = c.ct + i;
                        v = 0.0f;
                        for (int b = 0; b < n_mels; ++b) v = __builtin_fmaf(cp[(size_t)b * n_ceps], e[b], v);
                    }
                }
                const int j = !c.htk ? i : i == 0 ? n_ceps - 1 : i - 1;  // where the frame stores c[i]
                const int64_t at = a.frames_first ? (d.row * T + t0 + tl) * n_ceps + j : (d.row * n_ceps + j) * T + t0 + tl;
                a.dst[at] = v;
            }
            continue;  // (the filterbank's own store, below, is the other launch's)
        }
        for (int it = t; it < items; it += kFbBlock) {
            int tl, b;
            if (a.frames_first) {
                tl = it / n_mels;
                b = it - tl * n_mels;
            } else {
                b = it / nt;
                tl = it - b * nt;
            }
            float v = a.pad;
            if (tl < nr) {
                const int first = a.meta[3 * b], cnt = a.meta[3 * b + 1];
                const float *p = pw + tl * pstride + first, *ww = a.w + a.meta[3 * b + 2];
                float acc = 0.0f;
                for (int i = 0; i < cnt; ++i) acc = __builtin_fmaf(ww[i], p[i], acc);
                v = !a.log ? acc : acc <= a.floor ? a.log_floor : logf(acc);
            }
            const int64_t at = a.frames_first ? (d.row * T + t0 + tl) * n_mels + b : (d.row * n_mels + b) * T + t0 + tl;
            a.dst[at] = v;
        }
    }
}

template <int RT>
__global__ __launch_bounds__(kFbBlock) void pcm_fbank_kernel(const FbankArgs a)
{
    fb_tile_core<RT, false>(a, CepArgs{});
}

template <int RT>
__global__ __launch_bounds__(kFbBlock) void pcm_mfcc_kernel(const MfccArgs a)
{
    fb_tile_core<RT, true>(a.f, a.c);
}

struct CmnArgs {
    const vpz_pack_row *rows;
    float *dst;
    int64_t T;
    int32_t n_rows, win, hop, n_ceps, frames_first;
};

// Cepstral mean subtraction behind pcm_mfcc_kernel: one wave per (row, stored coefficient).  Lane q sums the real frames t = q (mod 64)
// in float64, t ascending; six xor shuffles (1, 2, 4, 8, 16, 32) combine the 64 partial sums into the same bits in every lane; the mean
// is rounded once to float32 and subtracted from the real frames.  Pad frames are neither read nor written
__global__ __launch_bounds__(kFbBlock) void pcm_cmn_kernel(const CmnArgs a)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * (kFbBlock / 64) + (threadIdx.x >> 6);
    if (j >= a.n_ceps) return;  // (no barrier in this kernel)
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_pack_row d = a.rows[r];
        const int64_t L = d.samples;
        const int64_t TL = L < a.win ? 0 : 1 + (L - a.win) / a.hop;
        float *p = a.dst + (a.frames_first ? d.row * a.T * a.n_ceps + j : (d.row * a.n_ceps + j) * a.T);
        const int64_t stride = a.frames_first ? a.n_ceps : 1;
        double s = 0.0;
        for (int64_t tt = lane; tt < TL; tt += 64) s += (double)p[tt * stride];
        for (int dd = 1; dd < 64; dd <<= 1) s += __shfl_xor(s, dd);
        const float m = (float)(s / (double)TL);
        for (int64_t tt = lane; tt < TL; tt += 64) p[tt * stride] = p[tt * stride] - m;
    }
}

int folded_for(Context *ctx, const vpz_fbank_spec &s, const Context::LogmelDft **out)
{
    const std::array<double, 5> key = {(double)s.win, (double)s.n_fft, (double)s.window, s.preemphasis, s.scale};
    return table_for(ctx, ctx->fbank_tables, key, "vpz_pcm_fbank: out of host memory", out, [&](Context::LogmelDft &tb) {
        tb.cols = (s.n_fft / 2 + kFbCols - 1) / kFbCols * kFbCols;
        const size_t rows = 2 * (size_t)((s.win + 1) / 2);  // (an odd win: one more row, of zeros)
        std::vector<float> host(rows * 2 * (size_t)tb.cols, 0.0f);
        fbank_table_fill(s, host.data(), 2 * (size_t)tb.cols, (size_t)tb.cols);
        return upload(ctx, "vpz_pcm_fbank: table upload", tb, {{host.data(), host.size() * sizeof(float), reinterpret_cast<void **>(&tb.d_table)}});
    });
}

int bank_for(Context *ctx, const vpz_fbank_spec &s, const Context::LogmelBank **out)
{
    const std::array<double, 5> key = {s.sample_rate, (double)s.n_fft, (double)s.n_mels, s.low_freq, s.high_freq};
    return table_for(ctx, ctx->fbank_banks, key, "vpz_pcm_fbank: out of host memory", out, [&](Context::LogmelBank &bk) {
        FbankBank fb;
        fbank_bank_build(s, fb);
        return upload_bank(ctx, "vpz_pcm_fbank: mel bank upload", fb, bk);
    });
}

// floats of a tile's LDS at `Tt` frames: the skewed span, then (behind the means) the power tile
void lds_plan(const vpz_fbank_spec &s, int Tt, int *span_cap, int *pstride)
{
    const int count = (Tt - 1) * s.hop + s.win, skew = s.hop % 2 == 0 ? 1 : 0;
    *span_cap = count + (skew ? count / s.hop : 0) + 1;
    *pstride = (s.n_fft / 2) | 1;
}

// the cepstral matrix of a spec on the device, transposed: [n_mels][n_ceps], coefficient i in column i (the kernel permutes on the store)
int cepstra_for(Context *ctx, const vpz_mfcc_spec &s, const float **out)
{
    const std::array<double, 5> key = {(double)s.fbank.n_mels, (double)s.n_ceps, s.lifter, (double)s.htk_compat, (double)s.use_energy};
    const DeviceTable *rec = nullptr;
    const int rc = table_for(ctx, ctx->mfcc_tables, key, "vpz_pcm_mfcc: out of host memory", &rec, [&](DeviceTable &ct) {
        const int N = s.fbank.n_mels, n_ceps = s.n_ceps;
        std::vector<float> host((size_t)N * (size_t)n_ceps);
        for (int b = 0; b < N; ++b)
            for (int i = 0; i < n_ceps; ++i) host[(size_t)b * n_ceps + i] = mfcc_weight(s, i, b);
        void *at = nullptr;
        return upload(ctx, "vpz_pcm_mfcc: cepstral matrix upload", ct, {{host.data(), host.size() * sizeof(float), &at}});
    });
    if (rc == VPZ_OK) *out = static_cast<const float *>(rec->mem);
    return rc;
}

// floats of an MFCC tile's LDS at `Tt` frames: lds_plan's span and power tile, a second kFbMeans area for the energies behind the means,
// and behind the power tile the log-mel tile, `estride` floats between two of its rows -- room of its own, nothing overlays the span.
// tests/test_mfcc_cpu.py restates it and holds that 16 frames fit at every spec inside the limits
int mfcc_lds_plan(const vpz_fbank_spec &s, int Tt, int *span_cap, int *pstride, int *estride)
{
    lds_plan(s, Tt, span_cap, pstride);
    *estride = s.n_mels | 1;
    return *span_cap + 2 * kFbMeans + Tt * *pstride + Tt * *estride;
}

// The launch both entry points share, planned (`q.name` is the entry point's, in front of every refusal; the spec has passed its check):
// the frames and the row launch checked, the tables fetched, the tile chosen, the descriptors on their way, `a` filled.  `floats(Tt, a)`
// is the tile's LDS at Tt frames and sets a's span_cap and pstride; `columns` are what a frame stores.  VPZ_OK with *grid's x = 0: a
// launch of no rows, nothing to do
template <class Floats>
int plan_launch(Context *ctx, const vpz_fbank_spec &s, int64_t frames, RowLaunch q, int columns, Floats floats, FbankArgs &a, dim3 *grid, size_t *lds)
{
    char text[96];
    auto refuse = [&](int status, const char *what) {
        snprintf(text, sizeof text, "%s: %s", q.name, what);
        return set_error(ctx, status, text);
    };
    *grid = dim3(0, 0, 0);
    if (frames < s.win) return refuse(VPZ_E_INVALID_ARG, "frames < win (a row holds no frame)");
    if (frames > INT64_MAX / 8) return refuse(VPZ_E_INVALID_ARG, "sizes overflow");
    const int64_t T = 1 + (frames - s.win) / s.hop;
    q.frames = frames;
    q.row_elems = (unsigned __int128)(uint64_t)T * (uint64_t)columns;
    int rc = check_row_launch(ctx, q);
    if (rc != VPZ_OK || q.n_rows == 0) return rc;

    const Context::LogmelDft *tb = nullptr;
    const Context::LogmelBank *bk = nullptr;
    rc = folded_for(ctx, s, &tb);
    if (rc == VPZ_OK) rc = bank_for(ctx, s, &bk);
    if (rc != VPZ_OK) return rc;

    // the tile: 64 frames where the row has more than 32, the launch gives every CU two workgroups at that size and the LDS holds them
    // (every tile reads the whole table from L2, so the larger tile halves that traffic); else 32 where the row has more than 16 and the
    // LDS holds them; else 16 (a result does not depend on the tile: the same bits).  tests/test_fbank_cpu.py restates lds_plan and this
    // choice (tile_plan), tests/mfcc_truth.py the same over mfcc_lds_plan, and hold them at every spec inside the limits
    a.Tt = 0;
    int room = 0;
    const bool few = ((T + 63) / 64) * (int64_t)q.n_rows < 2 * (int64_t)ctx->num_cu;
    for (int Tt : {64, 32, 16}) {
        room = floats(Tt, a);
        if ((Tt == 64 && (T <= 32 || few)) || (Tt == 32 && T <= 16) || room > kFbLdsFloats) continue;
        a.Tt = Tt;
        break;
    }
    if (a.Tt == 0) return refuse(VPZ_E_UNSUPPORTED, "no tile fits the LDS");  // (16 frames fit at every spec inside the limits)
    const int64_t blocks = (T + a.Tt - 1) / a.Tt;
    if (blocks > 0x7fffffff) return refuse(VPZ_E_INVALID_ARG, "a row too long for one launch");

    rc = upload_rows(ctx, q.n_rows, q.rows, &a.rows);
    if (rc != VPZ_OK) return rc;

    a.src = static_cast<const float *>(q.src);
    a.dst = static_cast<float *>(q.dst);
    a.table = tb->d_table;
    a.meta = bk->d_meta;
    a.w = bk->d_w;
    a.T = T;
    a.n_rows = q.n_rows;
    a.win = s.win;
    a.hop = s.hop;
    a.nb = s.n_fft / 2;
    a.cols = tb->cols;
    a.n_mels = s.n_mels;
    a.log = s.output == VPZ_FBANK_LOG;  // (vpz_pcm_mfcc's spec has no other output)
    a.frames_first = s.layout == VPZ_FBANK_FRAMES_FIRST;
    a.remove_dc = s.remove_dc;
    a.skew = s.hop % 2 == 0 ? 1 : 0;
    a.floor = a.log ? (float)s.floor : 0.0f;
    a.log_floor = a.log ? (float)log((double)a.floor) : 0.0f;
    a.pad = (float)s.pad_value;
    *grid = dim3((unsigned)blocks, (unsigned)std::min<int64_t>(q.n_rows, kFbMaxGridY));
    *lds = sizeof(float) * (size_t)room;
    return VPZ_OK;
}

// the tile core at the plan's tile; the attribute is the kernel's, not the launch's: always the whole budget, so that two contexts never
// lower it under each other
template <class Args>
int launch_tiles(Context *ctx, void (*two)(const Args), void (*one)(const Args), const Args &args, int Tt, dim3 grid, size_t lds, const char *what)
{
    void (*kernel)(const Args) = Tt == 64 ? two : one;
    VPZ_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(float) * kFbLdsFloats)));
    kernel<<<grid, kFbBlock, lds, ctx->stream>>>(args);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(ctx, VPZ_E_HIP, what, e);
    return VPZ_OK;
}

}  // namespace

}  // namespace vpz

extern "C" int vpz_fbank_table(const vpz_fbank_spec *spec, float *table, int64_t capacity)
{
    if (!spec || capacity < 0 || !vpz::fbank_spec_ok(*spec)) return VPZ_E_INVALID_ARG;
    if (!table) return VPZ_OK;
    const int64_t nb = spec->n_fft / 2;
    if (capacity < (int64_t)spec->win * 2 * nb) return VPZ_E_CAPACITY;
    vpz::fbank_table_fill(*spec, table, (size_t)(2 * nb), (size_t)nb);
    return VPZ_OK;
}

extern "C" int vpz_fbank_filterbank(const vpz_fbank_spec *spec, int32_t *first_bin, int32_t *n_bins, float *weights, int64_t capacity,
                                    int64_t *total)
{
    if (!spec || capacity < 0 || !vpz::fbank_spec_ok(*spec)) return VPZ_E_INVALID_ARG;
    vpz::FbankBank fb;
    try {
        vpz::fbank_bank_build(*spec, fb);
    } catch (const std::bad_alloc &) {
        return VPZ_E_NOMEM;
    }
    if (total) *total = (int64_t)fb.weights.size();
    if (first_bin) memcpy(first_bin, fb.first.data(), sizeof(int32_t) * fb.first.size());
    if (n_bins) memcpy(n_bins, fb.count.data(), sizeof(int32_t) * fb.count.size());
    if (!weights) return VPZ_OK;
    if ((uint64_t)capacity < fb.weights.size()) return VPZ_E_CAPACITY;
    if (!fb.weights.empty()) memcpy(weights, fb.weights.data(), sizeof(float) * fb.weights.size());
    return VPZ_OK;
}

extern "C" int vpz_pcm_fbank(vpz_context *c, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_fbank_spec *spec, int32_t n_rows,
                             const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!spec) return refuse("vpz_pcm_fbank: null pointer");
    if (!vpz::fbank_spec_ok(*spec)) return refuse("vpz_pcm_fbank: a spec outside the limits");
    vpz::FbankArgs a;
    dim3 grid;
    size_t lds = 0;
    const auto floats = [&](int Tt, vpz::FbankArgs &f) {
        vpz::lds_plan(*spec, Tt, &f.span_cap, &f.pstride);
        return f.span_cap + vpz::kFbMeans + Tt * f.pstride;
    };
    const int rc = vpz::plan_launch(ctx, *spec, frames, vpz::RowLaunch{"vpz_pcm_fbank", src_dev, src_elems, sizeof(float), 1, 1, 1, 0, n_rows, rows, dst_dev, dst_rows, 0, sizeof(float)},
                                    spec->n_mels, floats, a, &grid, &lds);
    if (rc != VPZ_OK || grid.x == 0) return rc;
    return vpz::launch_tiles(ctx, &vpz::pcm_fbank_kernel<2>, &vpz::pcm_fbank_kernel<1>, a, a.Tt, grid, lds, "pcm_fbank kernel launch");
}

extern "C" int vpz_mfcc_table(const vpz_mfcc_spec *spec, float *table, int64_t capacity)
{
    if (!spec || capacity < 0 || !vpz::mfcc_spec_ok(*spec)) return VPZ_E_INVALID_ARG;
    if (!table) return VPZ_OK;
    const int N = spec->fbank.n_mels;
    if (capacity < (int64_t)spec->n_ceps * N) return VPZ_E_CAPACITY;
    for (int j = 0; j < spec->n_ceps; ++j)
        for (int b = 0; b < N; ++b) table[(size_t)j * N + b] = vpz::mfcc_weight(*spec, vpz::mfcc_stored(*spec, j), b);
    return VPZ_OK;
}

extern "C" int vpz_pcm_mfcc(vpz_context *c, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_mfcc_spec *spec, int32_t n_rows,
                            const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!spec) return refuse("vpz_pcm_mfcc: null pointer");
    if (!vpz::mfcc_spec_ok(*spec)) return refuse("vpz_pcm_mfcc: a spec outside the limits");
    const vpz_fbank_spec &s = spec->fbank;
    vpz::MfccArgs m;
    vpz::FbankArgs &a = m.f;
    dim3 grid;
    size_t lds = 0;
    const auto floats = [&](int Tt, vpz::FbankArgs &f) { return vpz::mfcc_lds_plan(s, Tt, &f.span_cap, &f.pstride, &m.c.estride); };
    int rc = vpz::plan_launch(ctx, s, frames, vpz::RowLaunch{"vpz_pcm_mfcc", src_dev, src_elems, sizeof(float), 1, 1, 1, 0, n_rows, rows, dst_dev, dst_rows, 0, sizeof(float)},
                              spec->n_ceps, floats, a, &grid, &lds);
    if (rc != VPZ_OK || grid.x == 0) return rc;

    // the cepstral stage's own
    rc = vpz::cepstra_for(ctx, *spec, &m.c.ct);
    if (rc != VPZ_OK) return rc;
    m.c.n_ceps = spec->n_ceps;
    m.c.use_energy = spec->use_energy;
    m.c.htk = spec->htk_compat;
    m.c.sc2 = (float)s.scale * (float)s.scale;
    m.c.log_eps = (float)log((double)0x1p-23f);
    m.c.log_efloor = (float)spec->energy_floor > 0.0f ? (float)log((double)(float)spec->energy_floor) : -INFINITY;
    rc = vpz::launch_tiles(ctx, &vpz::pcm_mfcc_kernel<2>, &vpz::pcm_mfcc_kernel<1>, m, a.Tt, grid, lds, "pcm_mfcc kernel launch");
    if (rc != VPZ_OK || !spec->subtract_mean) return rc;

    // the mean over a row's real frames: behind the cepstra on the same stream, over the same descriptors
    const vpz::CmnArgs q{a.rows, a.dst, a.T, n_rows, s.win, s.hop, spec->n_ceps, a.frames_first};
    const int per = vpz::kFbBlock / 64;
    vpz::pcm_cmn_kernel<<<dim3((unsigned)((spec->n_ceps + per - 1) / per), grid.y), vpz::kFbBlock, 0, ctx->stream>>>(q);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "pcm_cmn kernel launch", e);
    return VPZ_OK;
}
