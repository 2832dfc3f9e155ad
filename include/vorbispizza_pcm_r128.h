/*
 * vorbispizza_pcm_r128.h -- what an EBU R 128 scanner needs beside the integrated loudness: the true peak of windows of a device PCM
 * array, on the device, and the loudness range and the maximum momentary and short-term loudness of their step sums, on the host
 * (libvorbispizza_synth.so).
 *
 * vorbispizza_pcm_loudness.h gives the gated integrated loudness and the sample peak and lists the true peak, the loudness range and the
 * short-term and momentary values as out of scope: this header supplies what that one leaves out.  The range and the maxima are a few
 * operations per 100 ms step on the step sums vpz_pcm_loudness already delivers: host code, like vpz_loudness_gate.  The true peak reads
 * every sample: vpz_pcm_true_peak.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).
 * Oversampling factor F of a whole rate fs, VPZ_LOUDNESS_MIN_RATE <= fs <= VPZ_LOUDNESS_MAX_RATE:  F = 4 for fs < 96 000,  F = 2 for
 * 96 000 <= fs < 192 000,  F = 1 from 192 000 up (BS.1770-4 Annex 2 asks for at least 192 kHz after oversampling).
 * Interpolator.  A Hann-windowed sinc of 12 taps per phase, N = 12 F + 1 coefficients.  For j = 0 .. N-1, in double, with m = j - 6 F:
 *     h[j] = sinc(m / F) * 0.5 (1 - cos(2 pi j / (N - 1))),   sinc(t) = sin(pi t) / (pi t),  sinc(0) = 1.
 * By definition h[j] is exactly 0 where j is a multiple of F and j != 6 F, and h[6 F] = 1.  h[j] = h[N-1-j].  A device coefficient is the
 * float32 nearest to h[j].
 * Output.  x[m] = 0 outside the window [0, L): a window is a clip of its own, as in vpz_pcm_loudness.  Per channel, for i = 0 .. L + 10:
 *     y[i F]     = x[i - 6]                              (the sample itself)
 *     y[i F + p] = sum_{k=0..11} h[p + k F] x[i - k],    p = 1 .. F-1,
 * accumulated in float32 in ONE order: a = h[p] x[i] rounded, then a = fma(h[p + k F], x[i - k], a) for k = 1 .. 11 ascending -- twelve
 * roundings, no pairing of symmetric taps.
 * True peak of a row.  The largest |y| over all channels and all outputs, the 11 positions behind the last sample included: with causal
 * indexing every inter-sample peak of the last six samples lies in that tail.  So the true peak is >= the sample peak (as float32 bits),
 * equals it where F = 1, and is 0 for an empty window.  With F = 2 the one computed phase has exactly the coefficients of F = 4's
 * middle phase.
 * Non-finite samples.  A y that is NaN is passed over (fmaxf); an infinite sample gives +Inf through the identity phase; every other row
 * has the same bits as it would without that row.
 * Range (vpz_loudness_range, EBU Tech 3342).  With S the step of vorbispizza_pcm_loudness.h, short-term block k is steps k .. k+29 (3 s,
 * a hop of one step), k = 0 .. n-30:  p_k = (the sum of its thirty, i ascending) / (30 S),  l_k = -0.691 + 10 log10 p_k.  The absolute
 * gate keeps the blocks with l_k > -70; the relative gate keeps, among those, the ones with
 * l_k > -0.691 + 10 log10(mean p of those, summed in order) - 20.  With the kept l sorted ascending as v[0 .. m):
 *     low = v[floor(0.10 (m-1) + 0.5)],   high = v[floor(0.95 (m-1) + 0.5)],   range = high - low   in LU.
 * A block whose level is NaN fails both comparisons and is not kept.
 * Maxima (vpz_loudness_maxima).  The largest l over the gate's 400 ms blocks (steps k .. k+3, p = the sum of the four / (4 S)): the
 * maximum momentary loudness; the largest l over the 3 s blocks above: the maximum short-term loudness.  A NaN level is passed over.
 *
 * Out of scope (a gain applied on delivery is vpz_pcm_normalize's, vorbispizza_pcm_normalize.h): int16 sources; per-channel peaks; an oversampling other than the factor rule above; the
 * vpzr_* reader (vorbispizza_reader.h).
 *
 * A header of its own: vorbispizza_synth.h, the older vorbispizza_pcm_*.h, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_R128_H
#define VORBISPIZZA_PCM_R128_H

#include <stdint.h>

#include "vorbispizza_pcm_loudness.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_TRUE_PEAK_TAPS 12       /* per phase */
#define VPZ_TRUE_PEAK_MAX_COEFFS 49 /* 12 * 4 + 1 */

/* *factor = F of the rate, h[0 .. 12 F] the interpolator in double, the rest of h[49] zero; needs no device.
 * VPZ_E_INVALID_ARG: factor or h null, a rate outside the limits. */
int vpz_true_peak_filter(int32_t sample_rate, int32_t *factor, double h[49]);

/* Source and descriptors as in vpz_pcm_loudness: `src_elems` float32 elements of device memory, interleaved [sample][channel]; `src`
 * the element offset of the window's first sample (channel 0), `samples` = L, `row` the destination row.  true_peak_dev[row] (float32,
 * dst_rows elements) gets the row's true peak and, where sample_peak_dev is not null, sample_peak_dev[row] (the same shape) its sample
 * peak, the bits vpz_pcm_loudness gives.  Every element of a named row is written exactly once, rows that no descriptor names are not
 * touched.  A row's result is the same bits whatever else is in the launch and wherever the row sits: every output has the one order
 * stated above, a maximum has none, and there are no atomics.
 * `rows` is free again when the call returns; the kernels run asynchronously on the context's stream (vpz_context_synchronize completes
 * them).  Scratch memory is kept by the context and grown on demand (VPZ_E_NOMEM).
 * VPZ_E_INVALID_ARG, with nothing launched: what vpz_pcm_loudness refuses for the same arguments -- a null pointer (sample_peak_dev
 * excepted); channels outside 1..VPZ_MAX_CHANNELS; a rate outside the limits; n_rows < 0; dst_rows < 0; a descriptor whose source range
 * [src, src + samples * channels) leaves [0, src_elems) or whose row is out of range or named twice; a pointer not aligned to its
 * element; src_dev, true_peak_dev or sample_peak_dev not device memory of the context's device, or not inside one allocation over its
 * whole extent. */
int vpz_pcm_true_peak(vpz_context *ctx, const void *src_dev, int64_t src_elems, int32_t channels, int32_t sample_rate, int32_t n_rows,
                      const vpz_pack_row *rows, float *true_peak_dev, float *sample_peak_dev, int64_t dst_rows);

/* The loudness range of `n_steps` step sums of steps of `step_len` (= S) samples, as the definition states it; needs no device.  *low
 * and *high (when not null) are the two percentile levels in LUFS, *blocks_kept (when not null) the 3 s blocks behind them.  With fewer
 * than 30 steps, or nothing kept: *range 0, *low = *high = -HUGE_VAL, *blocks_kept 0, and the status is VPZ_OK.
 * VPZ_E_INVALID_ARG: range null; sums null with n_steps > 0; n_steps < 0; step_len < 1.  VPZ_E_NOMEM. */
int vpz_loudness_range(const double *sums, int64_t n_steps, int32_t step_len, double *range, double *low, double *high, int64_t *blocks_kept);

/* The largest momentary (400 ms) and short-term (3 s) level of the step sums, in LUFS; needs no device.  Either pointer may be null, not
 * both.  -HUGE_VAL where there is no block or no finite level (digital silence reads -HUGE_VAL).
 * VPZ_E_INVALID_ARG: both outputs null; sums null with n_steps > 0; n_steps < 0; step_len < 1. */
int vpz_loudness_maxima(const double *sums, int64_t n_steps, int32_t step_len, double *momentary_max, double *short_term_max);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_R128_H */
