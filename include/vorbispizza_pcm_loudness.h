/*
 * vorbispizza_pcm_loudness.h -- windows of a device PCM array measured for programme loudness (ITU-R BS.1770-4 / EBU R 128) on the
 * device, libvorbispizza_synth.so.
 *
 * A loudness scanner (ReplayGain, EBU R 128 normalisation) wants a handful of numbers per stream, not its samples.  After a synth call
 * into device memory the PCM is there already: vpz_pcm_loudness filters every window with the K-weighting filter, sums the squares of
 * every 100 ms step and takes the sample peak, so that a few hundred bytes per second of audio cross the host link.  The gate of the
 * integrated value -- a few operations per step -- runs on the host: vpz_loudness_gate.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).
 * Filter.  Per channel two biquads in cascade, y = b0 x + b1 x[-1] + b2 x[-2] - a1 y[-1] - a2 y[-2], coefficients in double for a whole
 * sample rate fs, VPZ_LOUDNESS_MIN_RATE <= fs <= VPZ_LOUDNESS_MAX_RATE.  With K = tan(pi f0 / fs) and a0 = 1 + K/Q + K^2 both stages
 * have a1 = 2 (K^2 - 1) / a0, a2 = (1 - K/Q + K^2) / a0.
 *     Stage 1 (shelf): f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20),
 *         Vb = Vh^0.4996667741545416;  b0 = (Vh + Vb K/Q + K^2) / a0, b1 = 2 (K^2 - Vh) / a0, b2 = (Vh - Vb K/Q + K^2) / a0.
 *     Stage 2 (high-pass): f0 = 38.13547087602444, Q = 0.5003270373238773;  b = 1, -2, 1 (not normalised).
 * At 48 000 Hz these are BS.1770's published coefficients to 3.3e-16 relative.  The filter starts from zero state at a window's first
 * sample: a window is measured as a clip of its own.  All filter arithmetic is float64.
 * Steps.  S = (fs + 5) / 10 in integers is the 100 ms step (1 103 at 11 025 Hz).  A window of L samples has n = L / S whole steps; the
 * samples behind the last whole step are filtered but not summed.
 *     sum[j] = sum_c w[c] * sum_{i in step j} y_c[i]^2,   j = 0 .. n-1,   divided by nothing.
 * Peak.  The largest |x| over all L samples of all channels, whatever their weight: the sample peak, exact, 0 for an empty window.
 * Samples that are not finite.  A +-Inf or NaN sample makes sum[j] not finite (Inf or NaN) from the step it lies in to the window's
 * last, also where its channel's weight is 0 (0 x NaN is NaN); the steps before it, and every other row, are the same bits as without
 * it.  The peak is +Inf for an infinite sample; a NaN is passed over, and the peak is the largest |x| of the window's other samples.
 * Gate (vpz_loudness_gate).  Block k is steps k .. k+3, k = 0 .. n-4 (400 ms, 75 % overlap): p_k = (the sum of its four) / (4 S),
 * l_k = -0.691 + 10 log10 p_k.  The blocks with l_k > -70 pass the absolute gate; of those, the ones with l_k above
 * -0.691 + 10 log10(mean p of those) - 10 are kept; the integrated loudness is -0.691 + 10 log10(mean p of the kept), in LUFS.
 *
 * Out of scope: the true peak (oversampled); loudness range and the short-term and momentary values; int16 sources; the vpzr_* reader
 * (vorbispizza_reader.h).  A gain applied on delivery is vpz_pcm_normalize's (vorbispizza_pcm_normalize.h), and
 * vpzm_decode_ranges_normalized (vorbispizza_multi_normalize.h) measures and applies it in one call.
 *
 * A header of its own: vorbispizza_synth.h, the older vorbispizza_pcm_*.h, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_LOUDNESS_H
#define VORBISPIZZA_PCM_LOUDNESS_H

#include <stdint.h>

#include "vorbispizza_pcm_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_LOUDNESS_MIN_RATE 8000
#define VPZ_LOUDNESS_MAX_RATE 384000

/* coeffs = b0 b1 b2 a1 a2 of stage 1, then of stage 2; needs no device.
 * VPZ_E_INVALID_ARG: coeffs null, a rate outside the limits. */
int vpz_loudness_filter(int32_t sample_rate, double coeffs[10]);

/* The channel weights of BS.1770-4 Table 4 in Vorbis channel order, w[0 .. channels): 1 in general, 1.41 for the side or rear pair of a
 * surround layout (at +-90 / +-110 degrees), 0 for the LFE --
 *     1: {1}   2: {1, 1}   3: {1, 1, 1}   4: {1, 1, 1.41, 1.41}   5: {1, 1, 1, 1.41, 1.41}   6: {1, 1, 1, 1.41, 1.41, 0}
 *     7: {1, 1, 1, 1.41, 1.41, 1, 0}   8: {1, 1, 1, 1.41, 1.41, 1, 1, 0}   above 8: all 1.
 * Needs no device.  VPZ_E_INVALID_ARG: w null, channels outside 1..VPZ_MAX_CHANNELS. */
int vpz_loudness_weights(int32_t channels, double *w);

/* Source: `src_elems` float32 elements of device memory, interleaved [sample][channel] -- what a synth call with VPZ_OUT_INTERLEAVED
 * writes.  Descriptors are vpz_pcm_pack's: `src` the element offset of the window's first sample (channel 0), `samples` = L, `row` the
 * destination row.  Row r of sums_dev[dst_rows][max_steps] (float64) gets sum[0 .. n) and then +0.0 up to max_steps; peak_dev[r]
 * (float32, dst_rows elements) gets the peak.  Every element of a named row is written exactly once, rows that no descriptor names are
 * not touched.  A row's sums and peak are the same bits whatever else is in the launch and wherever the row sits: every sum is taken in
 * one stated order, without atomics.
 * `rows` and `weights` (channels doubles, host memory) are free again when the call returns; the kernels run asynchronously on the
 * context's stream (vpz_context_synchronize completes them).  Scratch memory and the constants of a rate are kept by the context and
 * grown on demand (VPZ_E_NOMEM).
 * VPZ_E_INVALID_ARG, with nothing launched: a null pointer; channels outside 1..VPZ_MAX_CHANNELS; a rate outside the limits;
 * max_steps < 1; n_rows < 0; dst_rows < 0; a descriptor whose source range [src, src + samples * channels) leaves [0, src_elems), whose
 * whole steps L / S exceed max_steps or whose row is out of range or named twice; a weight that is negative or not finite; a pointer not
 * aligned to its element; src_dev, sums_dev or peak_dev not device memory of the context's device, or not inside one allocation over
 * its whole extent. */
int vpz_pcm_loudness(vpz_context *ctx, const void *src_dev, int64_t src_elems, int32_t channels, int32_t sample_rate,
                     const double *weights, int32_t n_rows, const vpz_pack_row *rows, double *sums_dev, float *peak_dev, int64_t dst_rows,
                     int64_t max_steps);

/* The gated integrated loudness of `n_steps` step sums of steps of `step_len` (= S) samples, as the definition states it; needs no
 * device.  *blocks_kept (when not null) is the number of blocks behind the result.  With fewer than four steps, or nothing kept, *lufs
 * is -HUGE_VAL and *blocks_kept 0, and the status is VPZ_OK.
 * VPZ_E_INVALID_ARG: lufs null; sums null with n_steps > 0; n_steps < 0; step_len < 1. */
int vpz_loudness_gate(const double *sums, int64_t n_steps, int32_t step_len, double *lufs, int64_t *blocks_kept);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_LOUDNESS_H */
