// vpz_pcm_normalize (include/vorbispizza_pcm_normalize.h, which states the definition): windows of a planar float32 device array as a
// dense, zero-padded batch whose rows are normalised on the way -- zero mean and unit variance, a peak or RMS level, a given gain.
//
// Three launches, no atomics, no workgroup that waits for another:
//   normalize_chunk_kernel   one WAVE per chunk of VPZ_NORM_CHUNK samples of one channel of one descriptor: a lane reads four quads of
//                            four consecutive samples (one 16-byte load each where the quad's address allows it, element by element
//                            where not: the same values in the same order), adds them and their squares in float64, the lanes fold by
//                            halves; lane 0 leaves { S1, S2, P } of the chunk in the scratch memory;
//   normalize_final_kernel   one wave per descriptor: the chunk sums in the stated order (64 at a time into the lanes, then added one by
//                            one), m and g in float64, rounded once; { m, g } into the scratch memory, the result record where asked for;
//   normalize_planar_kernel  the values of a planar destination, vpz_pcm_pack's mapping: one lane per 16-byte tile of the destination
//                            ADDRESS, read in 16-byte loads where the source is aligned too;
//   normalize_inter_kernel   the values of a frames-major destination: a workgroup reads a tile of frames of every channel along the
//                            channels, turns it in LDS and stores the tile's [frame][channel] elements in address order, 16 bytes a lane.
// A chunk is counted from the window's first sample, never from an address: a row's bits do not depend on where it lies.
// All element indices are 64-bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "synth_common.hpp"
#include "../../include/vorbispizza_pcm_normalize.h"

namespace vpz {

namespace {

constexpr int kNzBlock = 256;       // lanes of a workgroup: tiles of the planar kernel, four chunks of the chunk kernel
constexpr int kNzWaves = kNzBlock / 64;
constexpr int kNzMaxGridY = 4096;   // descriptors side by side in the grid's y; a workgroup takes every kNzMaxGridY-th beyond that
constexpr int kNzMaxFinal = 1 << 16;  // workgroups of the final kernel at the most; each takes every kNzMaxFinal-th descriptor beyond
constexpr int kNzTile = 4096;       // floats of the frames-major kernel's LDS tile: 16 KiB
static_assert(VPZ_NORM_CHUNK == 16 * 64, "a lane adds four quads of a chunk");
static_assert(4 * VPZ_MAX_CHANNELS <= kNzTile, "four frames of every channel must fit the tile");

struct NormArgs {
    const float *src;
    const vpz_norm_row *rows;
    void *dst;
    double *chunks;        // [n_rows][channels][nck] of { S1, S2, P }
    double *mg;            // [n_rows] of { m, g }, the float32 values widened
    vpz_norm_result *result;
    double target, eps, ceiling;
    int64_t frames, nck;   // nck: chunks of a channel of `frames` samples
    int32_t n_rows, channels, mode, stats;  // stats: m and g come from `mg` (else m = 0, g = the descriptor's gain)
    int32_t tile_frames;   // frames of the frames-major kernel's tile, a multiple of 4
};

struct alignas(16) Quad {
    float v[4];
};

__global__ __launch_bounds__(kNzBlock) void normalize_chunk_kernel(const NormArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * kNzWaves + (threadIdx.x >> 6);  // the chunk among the descriptor's channels * nck
    if (k >= a.channels * a.nck) return;
    const int64_t c = k / a.nck, q = k - c * a.nck;
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_norm_row d = a.rows[r];
        const int64_t first = q * VPZ_NORM_CHUNK;
        if (first >= d.samples) continue;
        const int64_t n = min((int64_t)VPZ_NORM_CHUNK, d.samples - first);  // the chunk's samples
        const float *in = a.src + d.src + c * a.frames + first;
        const bool aligned = reinterpret_cast<uintptr_t>(in) % 16 == 0;
        double s1 = 0.0, s2 = 0.0;
        float p = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int e0 = t * 256 + 4 * lane;
            Quad x;
            if (aligned && e0 + 4 <= n) {
                x = *reinterpret_cast<const Quad *>(in + e0);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) x.v[i] = e0 + i < n ? in[e0 + i] : 0.0f;  // (+0.0 changes neither sum nor peak)
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double v = (double)x.v[i];
                s1 += v;
                s2 += v * v;
                p = fmaxf(p, fabsf(x.v[i]));
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {  // lane l with lane l + off: the sum is the same from either side
            s1 += __shfl_xor(s1, off);
            s2 += __shfl_xor(s2, off);
            p = fmaxf(p, __shfl_xor(p, off));
        }
        if (lane == 0) {
            double *out = a.chunks + ((int64_t)r * a.channels * a.nck + k) * 3;
            out[0] = s1;
            out[1] = s2;
            out[2] = (double)p;
        }
    }
}

__global__ __launch_bounds__(64) void normalize_final_kernel(const NormArgs a)
{
    const int lane = threadIdx.x;
    for (int r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const vpz_norm_row d = a.rows[r];
        const int64_t nq = (d.samples + VPZ_NORM_CHUNK - 1) / VPZ_NORM_CHUNK;  // the chunks of a channel that hold samples
        double S1 = 0.0, S2 = 0.0, P = 0.0;
        for (int c = 0; c < a.channels; ++c) {
            const double *in = a.chunks + ((int64_t)r * a.channels + c) * a.nck * 3;
            for (int64_t q0 = 0; q0 < nq; q0 += 64) {
                const int cnt = (int)min((int64_t)64, nq - q0);
                double v1 = 0.0, v2 = 0.0, vp = 0.0;
                if (lane < cnt) {
                    v1 = in[(q0 + lane) * 3];
                    v2 = in[(q0 + lane) * 3 + 1];
                    vp = in[(q0 + lane) * 3 + 2];
                }
                for (int i = 0; i < cnt; ++i) {  // every lane adds the same values in the same order
                    S1 += __shfl(v1, i);
                    S2 += __shfl(v2, i);
                    P = fmax(P, __shfl(vp, i));
                }
            }
        }
        const double N = (double)((int64_t)a.channels * d.samples);
        double m = 0.0, g = 1.0;
        if (N > 0.0 && P > 0.0) {
            if (a.mode == VPZ_NORM_MEANVAR) {
                m = S1 / N;
                const double e2 = S2 / N, mm = m * m;
                double v = e2 - mm;
                v = v > 0.0 ? v : 0.0;
                g = 1.0 / sqrt(v + a.eps);
            } else if (a.mode == VPZ_NORM_PEAK) {
                g = a.target / P;
            } else if (a.mode == VPZ_NORM_RMS) {
                g = a.target / sqrt(S2 / N);
            } else {
                g = d.gain;
            }
            if (a.ceiling > 0.0 && g * P > a.ceiling) g = a.ceiling / P;
        }
        const float mf = (float)m, gf = (float)g;
        if (lane == 0) {
            if (a.stats) {
                a.mg[2 * (int64_t)r] = (double)mf;
                a.mg[2 * (int64_t)r + 1] = (double)gf;
            }
            if (a.result) {
                vpz_norm_result o;
                o.sum = S1;
                o.sum_sq = S2;
                o.peak = P;
                o.mean = (double)mf;
                o.gain = (double)gf;
                a.result[r] = o;
            }
        }
    }
}

// m and g of descriptor r as the value kernels use them
__device__ __forceinline__ void offset_and_gain(const NormArgs &a, int r, const vpz_norm_row &d, float *m, float *g)
{
    if (a.stats) {
        *m = (float)a.mg[2 * (int64_t)r];
        *g = (float)a.mg[2 * (int64_t)r + 1];
    } else {
        *m = 0.0f;
        *g = (float)d.gain;
    }
}

// item 3 of the definition: two float32 operations (this unit is built with -ffp-contract=off)
__device__ __forceinline__ float value(float x, float m, float g)
{
    const float t = x - m;
    return t * g;
}

__device__ __forceinline__ float as_elem(float v, float *) { return v; }
__device__ __forceinline__ int16_t as_elem(float v, int16_t *) { return (int16_t)to_s16(v); }

struct alignas(16) Wide {  // the 16 bytes of a destination tile
    uint32_t w[4];
};

// the run's element a tile starts at (negative: the run starts inside the tile): vpz_pcm_pack's rule
__device__ __forceinline__ int64_t tile_begin(int64_t tile, int shift, int vec) { return tile * vec - shift; }

template <typename T>
__global__ __launch_bounds__(kNzBlock) void normalize_planar_kernel(const NormArgs a, int64_t tiles_per_run)
{
    constexpr int kVec = 16 / (int)sizeof(T);
    const int64_t lane = (int64_t)blockIdx.x * kNzBlock + threadIdx.x;
    const int64_t run = lane / tiles_per_run;  // the channel
    const int64_t tile = lane - run * tiles_per_run;
    const int64_t len = a.frames;
    if (run >= a.channels) return;
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_norm_row d = a.rows[r];
        T *out = static_cast<T *>(a.dst) + (d.row * a.channels + run) * len;
        const int shift = (int)((reinterpret_cast<uintptr_t>(out) / sizeof(T)) % kVec);
        const int64_t lo = tile_begin(tile, shift, kVec);
        if (lo >= len) continue;
        float m, g;
        offset_and_gain(a, r, d, &m, &g);
        const float *in = a.src + d.src + run * a.frames;
        const bool whole = lo >= 0 && lo + kVec <= len;
        float x[kVec];
        bool real[kVec];
        if (whole && lo + kVec <= d.samples && reinterpret_cast<uintptr_t>(in + lo) % 16 == 0) {
#pragma unroll
            for (int j = 0; j < kVec / 4; ++j) {
                const Quad w = *reinterpret_cast<const Quad *>(in + lo + 4 * j);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    x[4 * j + i] = w.v[i];
                    real[4 * j + i] = true;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                const int64_t e = lo + i;
                real[i] = e >= 0 && e < d.samples;
                x[i] = real[i] ? in[e] : 0.0f;
            }
        }
        T v[kVec];
#pragma unroll
        for (int i = 0; i < kVec; ++i) v[i] = real[i] ? as_elem(value(x[i], m, g), (T *)nullptr) : (T)0;
        if (whole) {
            Wide w;
            __builtin_memcpy(&w, v, 16);
            *reinterpret_cast<Wide *>(out + lo) = w;
        } else {
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                const int64_t e = lo + i;
                if (e >= 0 && e < len) out[e] = v[i];
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kNzBlock) void normalize_inter_kernel(const NormArgs a)
{
    constexpr int kVec = 16 / (int)sizeof(T);
    __shared__ float stage[kNzTile];  // [frame of the tile][channel]
    const int C = a.channels, F = a.tile_frames, quads = F / 4;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    if (f0 >= a.frames) return;
    const int64_t len = min((int64_t)F, a.frames - f0) * C;  // the tile's elements in the destination, one stretch
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const vpz_norm_row d = a.rows[r];
        float m, g;
        offset_and_gain(a, r, d, &m, &g);
        for (int idx = threadIdx.x; idx < C * quads; idx += kNzBlock) {  // consecutive lanes: consecutive quads of one channel
            const int c = idx / quads, qd = idx - c * quads;
            const int64_t f = f0 + 4 * qd;
            const float *in = a.src + d.src + (int64_t)c * a.frames + f;
            Quad x;
            if (f + 4 <= d.samples && reinterpret_cast<uintptr_t>(in) % 16 == 0) {
                x = *reinterpret_cast<const Quad *>(in);
#pragma unroll
                for (int i = 0; i < 4; ++i) x.v[i] = value(x.v[i], m, g);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) x.v[i] = f + i < d.samples ? value(in[i], m, g) : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) stage[(4 * qd + i) * C + c] = x.v[i];
        }
        __syncthreads();
        T *out = static_cast<T *>(a.dst) + (d.row * a.frames + f0) * C;
        const int shift = (int)((reinterpret_cast<uintptr_t>(out) / sizeof(T)) % kVec);
        const int64_t tiles = len / kVec + 2;
        for (int64_t t = threadIdx.x; t < tiles; t += kNzBlock) {
            const int64_t lo = tile_begin(t, shift, kVec);
            if (lo >= len) break;
            T v[kVec];
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                const int64_t e = lo + i;
                v[i] = e >= 0 && e < len ? as_elem(stage[e], (T *)nullptr) : (T)0;
            }
            if (lo >= 0 && lo + kVec <= len) {
                Wide w;
                __builtin_memcpy(&w, v, 16);
                *reinterpret_cast<Wide *>(out + lo) = w;
            } else {
#pragma unroll
                for (int i = 0; i < kVec; ++i) {
                    const int64_t e = lo + i;
                    if (e >= 0 && e < len) out[e] = v[i];
                }
            }
        }
        __syncthreads();  // the next descriptor's values overwrite the tile
    }
}

bool spec_ok(const vpz_norm_spec &s)
{
    if (s.mode != VPZ_NORM_MEANVAR && s.mode != VPZ_NORM_PEAK && s.mode != VPZ_NORM_RMS && s.mode != VPZ_NORM_GAIN) return false;
    if (s.channels < 1 || s.channels > VPZ_MAX_CHANNELS) return false;
    if ((s.mode == VPZ_NORM_PEAK || s.mode == VPZ_NORM_RMS) && !(std::isfinite(s.target) && s.target > 0.0)) return false;
    if (!std::isfinite(s.eps) || s.eps < 0.0 || !std::isfinite(s.ceiling) || s.ceiling < 0.0) return false;
    if (s.mode == VPZ_NORM_MEANVAR && s.ceiling != 0.0) return false;
    for (int32_t word : s.reserved)
        if (word != 0) return false;
    return true;
}

// the scratch elements (float64) of a call; false: the size overflows
bool scratch_need(int64_t n_rows, int32_t channels, int64_t frames, int64_t *doubles)
{
    const uint64_t nck = (uint64_t)((frames - 1) / VPZ_NORM_CHUNK + 1);
    const unsigned __int128 per_row = (unsigned __int128)nck * (uint64_t)channels * 3u + 2u;
    const unsigned __int128 need = per_row * (uint64_t)n_rows;
    if (per_row > (uint64_t)INT64_MAX / sizeof(double) || need > (uint64_t)INT64_MAX / sizeof(double)) return false;
    *doubles = (int64_t)need;
    return true;
}

bool ranges_overlap(const void *p, uint64_t pn, const void *q, uint64_t qn)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return pn != 0 && qn != 0 && a < b + qn && b < a + pn;
}

}  // namespace

}  // namespace vpz

extern "C" int vpz_pcm_normalize_scratch(int32_t n_rows, int32_t channels, int64_t frames, int64_t *doubles)
{
    if (!doubles || n_rows < 0 || channels < 1 || channels > VPZ_MAX_CHANNELS || frames < 1) return VPZ_E_INVALID_ARG;
    return vpz::scratch_need(n_rows, channels, frames, doubles) ? VPZ_OK : VPZ_E_INVALID_ARG;
}

extern "C" int vpz_pcm_normalize(vpz_context *c, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_norm_spec *spec,
                                 int32_t n_rows, const vpz_norm_row *rows, void *dst_dev, int64_t dst_rows, int32_t dst_layout,
                                 void *scratch_dev, int64_t scratch_doubles, vpz_norm_result *result_dev)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!spec || !rows) return refuse("vpz_pcm_normalize: null pointer");
    if (!vpz::spec_ok(*spec)) return refuse("vpz_pcm_normalize: a spec outside the limits");
    const vpz_norm_spec &s = *spec;
    const int32_t channels = s.channels;
    bool s16, planar;
    if (!vpz::layout_of(dst_layout, &s16, &planar)) return refuse("vpz_pcm_normalize: bad layout");
    planar = planar || channels == 1;  // (one channel: planar and frames-major are the same array)
    if (frames < 1 || n_rows < 0 || dst_rows < 0 || src_elems < 0 || scratch_doubles < 0) return refuse("vpz_pcm_normalize: frames < 1 or a negative count");
    if ((unsigned __int128)(uint64_t)frames * (uint64_t)channels > (uint64_t)INT64_MAX / sizeof(float)) return refuse("vpz_pcm_normalize: sizes overflow");
    if (((int64_t)n_rows * 4 + 2) / 3 > 0x7fffffff) return refuse("vpz_pcm_normalize: too many descriptors for one launch");

    // the descriptors as a row launch's, one channel of src_elems elements: its check covers samples, rows and both arrays
    std::vector<vpz_pack_row> as_pack, upload;
    try {
        as_pack.reserve((size_t)n_rows);
        upload.resize(((size_t)n_rows * sizeof(vpz_norm_row) + sizeof(vpz_pack_row) - 1) / sizeof(vpz_pack_row));
    } catch (const std::bad_alloc &) {
        return vpz::set_error(ctx, VPZ_E_NOMEM, "vpz_pcm_normalize: out of host memory");
    }
    bool any_real = false;  // (descriptors without samples -- zero rows -- need neither statistics nor scratch memory)
    const int64_t reach = (int64_t)(channels - 1) * frames;  // from a window's first sample to its last channel's
    for (int32_t r = 0; r < n_rows; ++r) {
        const vpz_norm_row &d = rows[r];
        any_real = any_real || d.samples > 0;
        if (d.samples < 0 || d.samples > frames) return refuse("vpz_pcm_normalize: a descriptor's samples exceed frames");
        if (d.src < 0 || d.src > src_elems || (d.samples > 0 && (reach > src_elems - d.src || d.samples > src_elems - d.src - reach)))
            return refuse("vpz_pcm_normalize: a descriptor's source range leaves the source array");
        if (s.mode == VPZ_NORM_GAIN && !(std::isfinite(d.gain) && d.gain > 0.0)) return refuse("vpz_pcm_normalize: a descriptor's gain is not finite or not > 0");
        as_pack.push_back(vpz_pack_row{d.src, d.samples, d.row});
    }
    const unsigned __int128 row_elems = (unsigned __int128)(uint64_t)frames * (uint64_t)channels;
    const uint64_t elem = s16 ? sizeof(int16_t) : sizeof(float);
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_normalize", src_dev, src_elems, sizeof(float), 1, 1, 1, frames, n_rows,
                                                       n_rows ? as_pack.data() : reinterpret_cast<const vpz_pack_row *>(rows), dst_dev, dst_rows,
                                                       row_elems, elem});
    if (rc != VPZ_OK) return rc;
    const uint64_t src_bytes = (uint64_t)src_elems * sizeof(float), dst_bytes = (uint64_t)(row_elems * (uint64_t)dst_rows) * elem;
    if (vpz::ranges_overlap(src_dev, src_bytes, dst_dev, dst_bytes)) return refuse("vpz_pcm_normalize: source and destination overlap");
    const uint64_t result_bytes = (uint64_t)n_rows * sizeof(vpz_norm_result);
    if (result_dev && n_rows > 0) {
        if (reinterpret_cast<uintptr_t>(result_dev) % sizeof(double) || !vpz::device_range(ctx, result_dev, result_bytes))
            return refuse("vpz_pcm_normalize: the result array is not device memory of the context's device, or leaves its allocation");
        if (vpz::ranges_overlap(result_dev, result_bytes, src_dev, src_bytes) || vpz::ranges_overlap(result_dev, result_bytes, dst_dev, dst_bytes))
            return refuse("vpz_pcm_normalize: the result array overlaps the source or the destination");
    }
    // statistics: every mode but a plain gain, and whenever the caller wants them; none where no descriptor has a sample
    const bool wanted = s.mode != VPZ_NORM_GAIN || s.ceiling > 0.0 || result_dev != nullptr;
    const bool stats = wanted && any_real;
    if (stats) {
        int64_t need = 0;
        if (!vpz::scratch_need(n_rows, channels, frames, &need)) return refuse("vpz_pcm_normalize: sizes overflow");
        if (!scratch_dev) return refuse("vpz_pcm_normalize: null pointer (the scratch memory)");
        if (scratch_doubles < need) return refuse("vpz_pcm_normalize: the scratch memory is too small");
        const uint64_t bytes = (uint64_t)need * sizeof(double);
        if (reinterpret_cast<uintptr_t>(scratch_dev) % sizeof(double)) return refuse("vpz_pcm_normalize: the scratch memory is not aligned to 8 bytes");
        if (!vpz::device_range(ctx, scratch_dev, bytes))
            return refuse("vpz_pcm_normalize: the scratch memory is not device memory of the context's device, or leaves its allocation");
        if (vpz::ranges_overlap(scratch_dev, bytes, src_dev, src_bytes) || vpz::ranges_overlap(scratch_dev, bytes, dst_dev, dst_bytes) ||
            (result_dev && vpz::ranges_overlap(scratch_dev, bytes, result_dev, result_bytes)))
            return refuse("vpz_pcm_normalize: the scratch memory overlaps the source, the destination or the result array");
    }
    if (n_rows == 0) return VPZ_OK;

    vpz::NormArgs a;
    memset(&a, 0, sizeof a);
    a.nck = (frames - 1) / VPZ_NORM_CHUNK + 1;
    a.tile_frames = std::max(4, (vpz::kNzTile / channels) & ~3);
    const int64_t vec = 16 / (int64_t)elem;
    const int64_t tiles_per_run = frames / vec + 2;  // a run that starts anywhere in a 16-byte unit touches at most that many tiles
    const int64_t value_blocks = planar ? (tiles_per_run * channels + vpz::kNzBlock - 1) / vpz::kNzBlock : (frames + a.tile_frames - 1) / a.tile_frames;
    const int64_t chunk_blocks = (a.nck * channels + vpz::kNzWaves - 1) / vpz::kNzWaves;
    if (value_blocks > 0x7fffffff || chunk_blocks > 0x7fffffff) return refuse("vpz_pcm_normalize: a row too long for one launch");

    // the 32-byte descriptors travel in the row launches' buffer, as so many of its 24-byte ones
    memcpy(upload.data(), rows, (size_t)n_rows * sizeof(vpz_norm_row));
    const vpz_pack_row *d_rows = nullptr;
    rc = vpz::upload_rows(ctx, (int32_t)upload.size(), upload.data(), &d_rows);
    if (rc != VPZ_OK) return rc;
    a.rows = reinterpret_cast<const vpz_norm_row *>(d_rows);
    a.src = static_cast<const float *>(src_dev);
    a.dst = dst_dev;
    a.chunks = stats ? static_cast<double *>(scratch_dev) : nullptr;
    a.mg = stats ? a.chunks + (int64_t)n_rows * channels * a.nck * 3 : nullptr;
    a.result = result_dev;
    a.target = s.target;
    a.eps = s.eps;
    a.ceiling = s.ceiling;
    a.frames = frames;
    a.n_rows = n_rows;
    a.channels = channels;
    a.mode = s.mode;
    a.stats = stats;

    const unsigned gy = (unsigned)std::min<int32_t>(n_rows, vpz::kNzMaxGridY);
    hipError_t e;
    if (stats) {
        vpz::normalize_chunk_kernel<<<dim3((unsigned)chunk_blocks, gy), vpz::kNzBlock, 0, ctx->stream>>>(a);
        e = hipGetLastError();
        if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "normalize_chunk kernel launch", e);
    }
    if (stats || result_dev) {  // (without samples anywhere it reads no chunk and fills the result array with { 0, 0, 0, 0, 1 })
        vpz::normalize_final_kernel<<<(unsigned)std::min<int32_t>(n_rows, vpz::kNzMaxFinal), 64, 0, ctx->stream>>>(a);
        e = hipGetLastError();
        if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "normalize_final kernel launch", e);
    }
    const dim3 grid((unsigned)value_blocks, gy);
    if (planar && s16)
        vpz::normalize_planar_kernel<int16_t><<<grid, vpz::kNzBlock, 0, ctx->stream>>>(a, tiles_per_run);
    else if (planar)
        vpz::normalize_planar_kernel<float><<<grid, vpz::kNzBlock, 0, ctx->stream>>>(a, tiles_per_run);
    else if (s16)
        vpz::normalize_inter_kernel<int16_t><<<grid, vpz::kNzBlock, 0, ctx->stream>>>(a);
    else
        vpz::normalize_inter_kernel<float><<<grid, vpz::kNzBlock, 0, ctx->stream>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "normalize value kernel launch", e);
    return VPZ_OK;
}
