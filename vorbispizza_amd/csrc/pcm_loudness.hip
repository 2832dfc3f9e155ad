// vpz_pcm_loudness (include/vorbispizza_pcm_loudness.h, which states the definition): windows of an interleaved float32 device PCM array
// as K-weighted 100 ms step sums and a sample peak per row; vpz_loudness_filter, vpz_loudness_weights and vpz_loudness_gate, host only.
//
// The K-weighting filter is a recurrence (its high-pass pole has radius 0.995 at 48 kHz), and it is linear, so it is cut into parallel
// pieces without changing its answer.  A UNIT is one step -- S samples -- of one channel of one row; the samples
// behind a row's last whole step are one more, shorter unit, which only the peak needs.
//   (a) loudness_pass<false>: every unit filters its samples from ZERO state and keeps its final state z -- four doubles, the two stages
//       in transposed direct form II -- and the largest |x| it saw;
//   (b) loudness_carry: one lane per (row, channel) walks the steps in order, s[j + 1] = P s[j] + z[j], with P the 4x4 transition of S
//       samples of silence, built on the host in long double per rate: the exact sequential carry, no truncation (|P| is 1e-9, far
//       above the bound), and leaves s[j] where z[j] was;
//   (c) loudness_pass<true>: every whole step filters again from its entering state and sums y^2, i ascending;
//   (d) loudness_finish: sums[row][j] = sum_c w[c] * e[c][j], c ascending, +0.0 behind the row's steps, and the row's peak.
// Every sum has one order and no atomics; a unit reads its own samples only: a row's result does not depend on the launch around it.
//
// The mapping of (a) and (c).  A workgroup of 256 lanes takes G = 256 / channels consecutive steps of a row, lane = step * channels +
// channel, and goes through them in chunks of kChunk samples: the chunk of a step is kChunk * channels contiguous floats of the source,
// staged into LDS with consecutive lanes on consecutive addresses (no lane walks global memory at a stride of S), at a row pitch of
// `stride` floats, stride = kChunk * channels rounded up to channels modulo 32.  Lane (s, c) then reads lds[s * stride + t * channels + c]:
// that is lane + t * channels modulo 32, so the 32 lanes of a ds_read_b32 group lie on 32 different banks at every t.  De-interleaving
// is that read.  34 KiB of LDS at most: four workgroups to a CU.  No scratch memory: a lane's state is eight doubles.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "vpz_internal.hpp"
#include "../../include/vorbispizza_pcm_loudness.h"

namespace vpz {

namespace {

constexpr int kLoudBlock = 256;     // lanes (units) of a workgroup of the two passes
constexpr int kChunk = 32;          // samples of a unit staged at a time
constexpr int kLoudMaxGridY = 4096; // descriptors side by side in the grid's y; a workgroup takes every kLoudMaxGridY-th beyond that

// a descriptor's units, uploaded behind the descriptors in records of their size (upload_rows): the units of channel c are
// base + c * units + j, j = 0 .. units-1, the first `steps` of them whole steps
struct RowUnits {
    int64_t base, units, steps;
};
static_assert(sizeof(RowUnits) == sizeof(vpz_pack_row), "RowUnits rides in upload_rows' records");

struct LoudFilter {  // a kernel argument, by value
    double c[10];  // b0 b1 b2 a1 a2, twice
    double P[16];  // row-major: the state after S samples of silence is P times the state before
};

// the two stages in transposed direct form II, one sample: the one statement of the recurrence on the device
__device__ __forceinline__ double k_filter(const LoudFilter &f, double x, double &s1, double &s2, double &s3, double &s4)
{
    const double y1 = f.c[0] * x + s1;
    s1 = f.c[1] * x - f.c[3] * y1 + s2;
    s2 = f.c[2] * x - f.c[4] * y1;
    const double y2 = f.c[5] * y1 + s3;
    s3 = f.c[6] * y1 - f.c[8] * y2 + s4;
    s4 = f.c[7] * y1 - f.c[9] * y2;
    return y2;
}

// (a): kSum false, over every unit, from zero state: `state` gets the final state, `unit_peak` the largest |x|.
// (c): kSum true, over the whole steps, from the state (b) left in `state`: `energy` gets the sum of y^2.
template <bool kSum>
__global__ __launch_bounds__(kLoudBlock) void loudness_pass(const float *__restrict__ src, const vpz_pack_row *__restrict__ rows,
                                                            const RowUnits *__restrict__ units, int n_rows, int C, int S, int G, int stride,
                                                            LoudFilter f, double *__restrict__ state, double *__restrict__ energy,
                                                            float *__restrict__ unit_peak)
{
    extern __shared__ float lds[];
    const int lane = threadIdx.x;
    const int s = lane / C, c = lane - s * C;
    const int run = kChunk * C;  // floats of a step's chunk
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const vpz_pack_row d = rows[r];
        const RowUnits u = units[r];
        const int64_t count = kSum ? u.steps : u.units;
        const int64_t j0 = (int64_t)blockIdx.x * G;
        if (j0 >= count) continue;  // (the same for every lane of the workgroup)
        const int64_t j = j0 + s;
        const bool live = s < G && j < count;
        const int len = live ? (int)min((int64_t)S, d.samples - j * S) : 0;
        const int tile = (int)min((int64_t)G, count - j0);  // steps this workgroup stages
        const int64_t unit = u.base + (int64_t)c * u.units + j;
        double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, acc = 0.0;
        float pk = 0.0f;
        if (kSum && live) {
            s1 = state[unit * 4 + 0];
            s2 = state[unit * 4 + 1];
            s3 = state[unit * 4 + 2];
            s4 = state[unit * 4 + 3];
        }
        const float *in = src + d.src + j0 * S * C;
        for (int t0 = 0; t0 < S; t0 += kChunk) {
            __syncthreads();  // (the chunk before has been consumed)
            for (int e = lane; e < tile * run; e += kLoudBlock) {
                const int ss = e / run, k = e - ss * run;
                // the samples step j0 + ss has from t0 on, in this chunk
                const int64_t have = min(min(d.samples - (j0 + ss) * S, (int64_t)S) - t0, (int64_t)kChunk);
                if (k < have * C) lds[ss * stride + k] = in[((int64_t)ss * S + t0) * C + k];
            }
            __syncthreads();
            const int tn = min(kChunk, len - t0);
            const float *p = lds + s * stride + c;
            for (int t = 0; t < tn; ++t) {
                const float x = p[t * C];
                const double y = k_filter(f, (double)x, s1, s2, s3, s4);
                if (kSum) acc = y * y + acc;
                else pk = fmaxf(pk, fabsf(x));
            }
        }
        if (!live) continue;
        if (kSum) {
            energy[unit] = acc;
        } else {
            state[unit * 4 + 0] = s1;
            state[unit * 4 + 1] = s2;
            state[unit * 4 + 2] = s3;
            state[unit * 4 + 3] = s4;
            unit_peak[unit] = pk;
        }
    }
}

// (b): one lane per (descriptor, channel)
__global__ __launch_bounds__(64) void loudness_carry(const RowUnits *__restrict__ units, int n_rows, int C, LoudFilter f,
                                                     double *__restrict__ state, const float *__restrict__ unit_peak,
                                                     float *__restrict__ chan_peak)
{
    const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (int64_t)n_rows * C) return;
    const int r = (int)(idx / C), c = (int)(idx - (int64_t)r * C);
    const RowUnits u = units[r];
    const int64_t first = u.base + (int64_t)c * u.units;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    float pk = 0.0f;
    for (int64_t j = 0; j < u.units; ++j) {
        pk = fmaxf(pk, unit_peak[first + j]);
        if (j >= u.steps) continue;
        double *z = state + (first + j) * 4;
        const double z1 = z[0], z2 = z[1], z3 = z[2], z4 = z[3];
        z[0] = s1;
        z[1] = s2;
        z[2] = s3;
        z[3] = s4;
        const double n1 = f.P[0] * s1 + f.P[1] * s2 + f.P[2] * s3 + f.P[3] * s4 + z1;
        const double n2 = f.P[4] * s1 + f.P[5] * s2 + f.P[6] * s3 + f.P[7] * s4 + z2;
        const double n3 = f.P[8] * s1 + f.P[9] * s2 + f.P[10] * s3 + f.P[11] * s4 + z3;
        const double n4 = f.P[12] * s1 + f.P[13] * s2 + f.P[14] * s3 + f.P[15] * s4 + z4;
        s1 = n1;
        s2 = n2;
        s3 = n3;
        s4 = n4;
    }
    chan_peak[idx] = pk;
}

// (d): one lane per element of a named row of `sums`; lane 0 of a row takes its peak along
__global__ __launch_bounds__(kLoudBlock) void loudness_finish(const vpz_pack_row *__restrict__ rows, const RowUnits *__restrict__ units,
                                                              const double *__restrict__ weights, int n_rows, int C,
                                                              const double *__restrict__ energy, const float *__restrict__ chan_peak,
                                                              double *__restrict__ sums, float *__restrict__ peak, int64_t max_steps)
{
    const int64_t j = (int64_t)blockIdx.x * kLoudBlock + threadIdx.x;
    if (j >= max_steps) return;
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const int64_t row = rows[r].row;
        const RowUnits u = units[r];
        double v = 0.0;
        if (j < u.steps)
            for (int c = 0; c < C; ++c) v = weights[c] * energy[u.base + (int64_t)c * u.units + j] + v;
        sums[row * max_steps + j] = v;
        if (j == 0) {
            float pk = 0.0f;
            for (int c = 0; c < C; ++c) pk = fmaxf(pk, chan_peak[(int64_t)r * C + c]);
            peak[row] = pk;
        }
    }
}

// the coefficients of a rate, as the header states them
void filter_of(int32_t fs, double c[10])
{
    const double pi = 3.14159265358979323846;
    {
        const double K = tan(pi * 1681.974450955533 / fs), Q = 0.7071752369554196;
        const double Vh = pow(10.0, 3.999843853973347 / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double K = tan(pi * 38.13547087602444 / fs), Q = 0.5003270373238773;
        const double a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0;
        c[6] = -2.0;
        c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
}

int32_t step_of(int32_t fs) { return (fs + 5) / 10; }

// P: column k is what S samples of silence make of the k-th unit state -- the recurrence of k_filter with x = 0, in long double
void transition_of(const double c[10], int32_t S, double P[16])
{
    for (int k = 0; k < 4; ++k) {
        long double s[4] = {0, 0, 0, 0};
        s[k] = 1;
        for (int32_t i = 0; i < S; ++i) {
            const long double y1 = s[0];
            s[0] = -(long double)c[3] * y1 + s[1];
            s[1] = -(long double)c[4] * y1;
            const long double y2 = (long double)c[5] * y1 + s[2];
            s[2] = (long double)c[6] * y1 - (long double)c[8] * y2 + s[3];
            s[3] = (long double)c[7] * y1 - (long double)c[9] * y2;
        }
        for (int i = 0; i < 4; ++i) P[i * 4 + k] = (double)s[i];
    }
}

int rate_for(Context *ctx, int32_t fs, const Context::LoudnessRate **out)
{
    auto it = ctx->loudness_rates.find(fs);
    if (it == ctx->loudness_rates.end()) {
        Context::LoudnessRate lr;
        filter_of(fs, lr.coeffs);
        transition_of(lr.coeffs, step_of(fs), lr.P);
        try {
            it = ctx->loudness_rates.emplace(fs, lr).first;
        } catch (const std::bad_alloc &) {
            return set_error(ctx, VPZ_E_NOMEM, "vpz_pcm_loudness: out of host memory");
        }
    }
    *out = &it->second;
    return VPZ_OK;
}

}  // namespace

}  // namespace vpz

extern "C" int vpz_loudness_filter(int32_t sample_rate, double coeffs[10])
{
    if (!coeffs || sample_rate < VPZ_LOUDNESS_MIN_RATE || sample_rate > VPZ_LOUDNESS_MAX_RATE) return VPZ_E_INVALID_ARG;
    vpz::filter_of(sample_rate, coeffs);
    return VPZ_OK;
}

extern "C" int vpz_loudness_weights(int32_t channels, double *w)
{
    if (!w || channels < 1 || channels > VPZ_MAX_CHANNELS) return VPZ_E_INVALID_ARG;
    static const double table[8][8] = {
        {1, 0, 0, 0, 0, 0, 0, 0},          {1, 1, 0, 0, 0, 0, 0, 0},          {1, 1, 1, 0, 0, 0, 0, 0},          {1, 1, 1.41, 1.41, 0, 0, 0, 0},
        {1, 1, 1, 1.41, 1.41, 0, 0, 0},    {1, 1, 1, 1.41, 1.41, 0, 0, 0},    {1, 1, 1, 1.41, 1.41, 1, 0, 0},    {1, 1, 1, 1.41, 1.41, 1, 1, 0},
    };
    for (int32_t c = 0; c < channels; ++c) w[c] = channels > 8 ? 1.0 : table[channels - 1][c];
    return VPZ_OK;
}

extern "C" int vpz_loudness_gate(const double *sums, int64_t n_steps, int32_t step_len, double *lufs, int64_t *blocks_kept)
{
    if (!lufs || n_steps < 0 || step_len < 1 || (!sums && n_steps > 0)) return VPZ_E_INVALID_ARG;
    *lufs = -HUGE_VAL;
    if (blocks_kept) *blocks_kept = 0;
    const int64_t blocks = n_steps - 3;
    const double per = 4.0 * (double)step_len;
    auto power = [&](int64_t k) { return (sums[k] + sums[k + 1] + sums[k + 2] + sums[k + 3]) / per; };
    auto level = [](double p) { return -0.691 + 10.0 * log10(p); };
    // the absolute gate
    double total = 0.0;
    int64_t passed = 0;
    for (int64_t k = 0; k < blocks; ++k) {
        const double p = power(k);
        if (level(p) > -70.0) {
            total += p;
            ++passed;
        }
    }
    if (passed == 0) return VPZ_OK;
    const double relative = level(total / (double)passed) - 10.0;
    // the relative gate, among those
    total = 0.0;
    int64_t kept = 0;
    for (int64_t k = 0; k < blocks; ++k) {
        const double p = power(k), l = level(p);
        if (l > -70.0 && l > relative) {
            total += p;
            ++kept;
        }
    }
    if (kept == 0) return VPZ_OK;
    *lufs = level(total / (double)kept);
    if (blocks_kept) *blocks_kept = kept;
    return VPZ_OK;
}

extern "C" int vpz_pcm_loudness(vpz_context *c, const void *src_dev, int64_t src_elems, int32_t channels, int32_t sample_rate,
                                const double *weights, int32_t n_rows, const vpz_pack_row *rows, double *sums_dev, float *peak_dev,
                                int64_t dst_rows, int64_t max_steps)
{
    if (!c) return VPZ_E_INVALID_ARG;
    vpz::Context *ctx = &c->impl;
    auto refuse = [&](const char *what) { return vpz::set_error(ctx, VPZ_E_INVALID_ARG, what); };
    if (!weights || !peak_dev) return refuse("vpz_pcm_loudness: null pointer");
    if (channels < 1 || channels > VPZ_MAX_CHANNELS) return refuse("vpz_pcm_loudness: channels outside 1..VPZ_MAX_CHANNELS");
    if (sample_rate < VPZ_LOUDNESS_MIN_RATE || sample_rate > VPZ_LOUDNESS_MAX_RATE) return refuse("vpz_pcm_loudness: a sample rate outside the limits");
    const int32_t S = vpz::step_of(sample_rate);
    if (max_steps < 1) return refuse("vpz_pcm_loudness: max_steps < 1");
    if (max_steps > INT64_MAX / S - 2) return refuse("vpz_pcm_loudness: sizes overflow");
    for (int32_t k = 0; k < channels; ++k)
        if (!std::isfinite(weights[k]) || weights[k] < 0.0) return refuse("vpz_pcm_loudness: a weight is negative or not finite");
    // L / S <= max_steps  <=>  L <= (max_steps + 1) * S - 1: the row launch's `frames`
    const int64_t most = (max_steps + 1) * S - 1;
    int rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_loudness", src_dev, src_elems, sizeof(float), channels, 1, 1, most, n_rows, rows, sums_dev,
                                                       dst_rows, (unsigned __int128)(uint64_t)max_steps, sizeof(double)});
    // (the peaks: one float32 a row; the descriptors have been looked at)
    if (rc == VPZ_OK)
        rc = vpz::check_row_launch(ctx, vpz::RowLaunch{"vpz_pcm_loudness (peak)", src_dev, src_elems, sizeof(float), channels, 1, 1, most, 0, rows, peak_dev,
                                                       dst_rows, (unsigned __int128)1, sizeof(float)});
    if (rc != VPZ_OK || n_rows == 0) return rc;
    if (n_rows > 0x3fffff00) return refuse("vpz_pcm_loudness: too many descriptors for one launch");

    const vpz::Context::LoudnessRate *lr = nullptr;
    rc = vpz::rate_for(ctx, sample_rate, &lr);
    if (rc != VPZ_OK) return rc;

    // what goes up in upload_rows' records: the descriptors, their units, the weights
    const size_t w_records = ((size_t)channels * sizeof(double) + sizeof(vpz_pack_row) - 1) / sizeof(vpz_pack_row);
    std::vector<vpz_pack_row> up;
    int64_t total = 0, most_units = 0;  // units of all descriptors; of one channel of the longest
    try {
        up.resize(2 * (size_t)n_rows + w_records);
    } catch (const std::bad_alloc &) {
        return vpz::set_error(ctx, VPZ_E_NOMEM, "vpz_pcm_loudness: out of host memory");
    }
    memcpy(up.data(), rows, sizeof(vpz_pack_row) * (size_t)n_rows);
    for (int32_t r = 0; r < n_rows; ++r) {
        const vpz::RowUnits u{total, (rows[r].samples + S - 1) / S, rows[r].samples / S};
        memcpy(&up[(size_t)n_rows + r], &u, sizeof u);
        total += u.units * channels;
        most_units = std::max(most_units, u.units);
    }
    memcpy(&up[2 * (size_t)n_rows], weights, sizeof(double) * (size_t)channels);

    // scratch: state [total][4] and energy [total] doubles, then unit_peak [total] and chan_peak [n_rows][channels] floats
    const size_t need = (size_t)total * (5 * sizeof(double) + sizeof(float)) + (size_t)n_rows * channels * sizeof(float) + 64;
    rc = ctx->loud_scratch.grow(ctx, need, "vpz_pcm_loudness: hipMalloc(scratch)");
    if (rc != VPZ_OK) return rc;
    double *state = static_cast<double *>(ctx->loud_scratch.p), *energy = state + 4 * total;
    float *unit_peak = reinterpret_cast<float *>(energy + total), *chan_peak = unit_peak + total;

    const int G = vpz::kLoudBlock / channels;
    int stride = vpz::kChunk * channels;
    stride += ((channels - stride) % 32 + 32) % 32;  // the least one >= kChunk * channels that is `channels` modulo 32
    const size_t lds_bytes = (size_t)G * stride * sizeof(float);
    const int64_t tiles = (most_units + G - 1) / G, finish_blocks = (max_steps + vpz::kLoudBlock - 1) / vpz::kLoudBlock;
    if (tiles > 0x7fffffff || finish_blocks > 0x7fffffff) return refuse("vpz_pcm_loudness: a row too long for one launch");

    const vpz_pack_row *d_up = nullptr;
    rc = vpz::upload_rows(ctx, (int32_t)up.size(), up.data(), &d_up);
    if (rc != VPZ_OK) return rc;
    const vpz::RowUnits *d_units = reinterpret_cast<const vpz::RowUnits *>(d_up + n_rows);
    const double *d_weights = reinterpret_cast<const double *>(d_up + 2 * (size_t)n_rows);

    vpz::LoudFilter f;
    memcpy(f.c, lr->coeffs, sizeof f.c);
    memcpy(f.P, lr->P, sizeof f.P);
    const float *src = static_cast<const float *>(src_dev);
    const unsigned grid_y = (unsigned)std::min<int64_t>(n_rows, vpz::kLoudMaxGridY);
    if (tiles > 0) {
        vpz::loudness_pass<false><<<dim3((unsigned)tiles, grid_y), vpz::kLoudBlock, lds_bytes, ctx->stream>>>(src, d_up, d_units, n_rows, channels, S, G, stride,
                                                                                                           f, state, energy, unit_peak);
        vpz::loudness_carry<<<(unsigned)(((int64_t)n_rows * channels + 63) / 64), 64, 0, ctx->stream>>>(d_units, n_rows, channels, f, state, unit_peak, chan_peak);
        vpz::loudness_pass<true><<<dim3((unsigned)tiles, grid_y), vpz::kLoudBlock, lds_bytes, ctx->stream>>>(src, d_up, d_units, n_rows, channels, S, G, stride,
                                                                                                          f, state, energy, unit_peak);
    } else {
        // (no descriptor has a sample: the peaks are zero, and (d) reads chan_peak)
        VPZ_HIP_TRY(ctx, hipMemsetAsync(chan_peak, 0, (size_t)n_rows * channels * sizeof(float), ctx->stream));
    }
    vpz::loudness_finish<<<dim3((unsigned)finish_blocks, grid_y), vpz::kLoudBlock, 0, ctx->stream>>>(d_up, d_units, d_weights, n_rows, channels, energy, chan_peak,
                                                                                                    sums_dev, peak_dev, max_steps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpz::set_error(ctx, VPZ_E_HIP, "pcm_loudness kernel launch", e);
    return VPZ_OK;
}
