/*
 * vorbispizza_pcm_resample.h -- windows of a device PCM array delivered at ONE sample rate, optionally mixed down to mono, as a dense,
 * zero-padded batch in device memory, libvorbispizza_synth.so.
 *
 * vpz_pcm_pack (vorbispizza_pcm_pack.h) delivers every window at its stream's own rate and channel count.  A model wants one rate:
 * vpz_pcm_resample is the same delivery -- trim, layout, zero fill, one launch -- with a polyphase windowed-sinc filter in between.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).  Source rate fs and target rate ft are reduced by their gcd
 * to down = fs / g and up = ft / g.  A window of L samples per channel, x[0..L), is resampled as a clip of its own: x is zero outside
 * [0, L) -- the samples that lie in front of the window and behind it in the source array are NOT filter context --, so the result is
 * what a loader gets that resamples the decoded clip, and it is NOT the slice of the resampled whole stream.  The output has
 * J = ceil(L * up / down) samples:
 *
 *     y[j] = sum over m of  x[m] * h(m - j * down / up)       (the argument is exact as the rational (m * up - j * down) / up)
 *     h(u) = s * sinc(pi * s * u) * cos^2(pi * s * u / 12)      for |s * u| < 6,  0 otherwise;   sinc(0) = 1
 *     s    = 0.99 * min(up, down) / down
 *
 * the filter of torchaudio.functional.resample at its defaults (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99).  With
 * n = m * up - j * down the support is decided in integers: a tap is live when |n| * 99 * min(up, down) < 600 * up * down.
 * up == down: no filter, the samples are copied (the formula at 1:1 is not the identity, s being 0.99).
 * Downmix: y_mono = (1 / C) * sum over c of y_c (the kernel mixes before it filters).  float32 rows are not clipped: a resampled signal
 * may overshoot +-1.  The int16 layouts are the float32 value through the library's one conversion, (int)(x * 32768f) clamped.
 * Limits: up and down in lowest terms, 1 <= up <= 1024, 1 <= down <= 32 * up; any other ratio is refused.
 *
 * A header of its own: vorbispizza_synth.h, vorbispizza_pcm_pack.h, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_RESAMPLE_H
#define VORBISPIZZA_PCM_RESAMPLE_H

#include <stdint.h>

#include "vorbispizza_pcm_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_RESAMPLE_MAX_UP 1024         /* up <= 1024 */
#define VPZ_RESAMPLE_MAX_DOWN_PER_UP 32  /* down <= 32 * up */

/* The filter of a ratio as the kernel uses it, computed on the host in double and rounded once to float32; needs no device.
 * Output j has phase p = j mod up and starts at source sample floor(j * down / up) + first_tap[p]; its taps are coeffs[p * taps + k],
 * k = 0 .. taps - 1, for consecutive source samples (a phase with fewer live taps ends in zeros).  *taps is the largest number of live
 * taps of a phase (1 at up == down: first_tap[0] = 0, coeffs[0] = 1).  first_tap (when not null) has room for `up` entries; coeffs
 * (when not null) for `capacity` floats.  coeffs == null: *taps (and first_tap) only, to size the table.
 * VPZ_E_INVALID_ARG: taps null, a refused ratio, capacity < 0.  VPZ_E_CAPACITY: coeffs given and capacity < up * taps (*taps is set). */
int vpz_resample_filter(int32_t up, int32_t down, int32_t *taps, int32_t *first_tap, float *coeffs, int64_t capacity);

/* Source: `src_elems` float32 elements of device memory, interleaved [sample][channel] -- what a synth call with VPZ_OUT_INTERLEAVED
 * writes (always float32: an int16 batch converts once, at the end).  A descriptor is a vpz_pack_row: `src` the element offset of the
 * window's first sample (channel 0), `samples` = L, `row` the destination row.  One ratio per launch.  dst_layout names the element
 * type and order as for vpz_pcm_pack: dst[dst_rows][out_channels][frames] (planar) or dst[dst_rows][frames][out_channels], float32 or
 * int16.  Row `row` receives J = ceil(L * up / down) samples per output channel, then zeros; every element of a named row is written
 * exactly once, rows that no descriptor names are not touched.  `rows` is host memory and is free again when the call returns; the
 * kernel runs asynchronously on the context's stream.  The coefficient table of a ratio is built on first use and kept by the context.
 * VPZ_E_INVALID_ARG, with nothing launched: what vpz_pcm_pack refuses (with J in the place of `samples`: J <= frames); a refused ratio;
 * downmix other than 0 or 1; out_channels other than `channels` (downmix 0) or 1 (downmix 1). */
int vpz_pcm_resample(vpz_context *ctx, const void *src_dev, int64_t src_elems, int32_t channels, int32_t up, int32_t down, int32_t downmix,
                     int32_t n_rows, const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows, int32_t out_channels, int64_t frames,
                     int32_t dst_layout);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_RESAMPLE_H */
