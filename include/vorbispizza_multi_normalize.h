/*
 * vorbispizza_multi_normalize.h -- the dispatcher of vorbispizza_multi.h: the resampled device batch of vorbispizza_multi_resample.h
 * delivered NORMALISED -- every row at zero mean and unit variance, at a peak, an RMS level or a programme loudness, or through one gain,
 * with an optional ceiling on the delivered peak (libvorbispizza_host.so).
 *
 * vpzm_decode_ranges_resampled gives a waveform model its clips; the model's feature extractor (wav2vec 2.0, HuBERT, WavLM) then takes
 * a masked mean, a masked variance and a masked scale over the batch, and a music loader that wants every clip at one loudness decodes
 * every window twice: vpzm_measure_loudness, then the delivery.  vpzm_decode_ranges_normalized is the resampled call -- the same
 * partition, sub-batches, routes, fall-backs and statuses -- with one more stage: the resample launches write planar float32 rows into
 * the lane's temporary, and one vpz_pcm_normalize launch set per sub-batch (vorbispizza_pcm_normalize.h, which states the statistics,
 * their order, the values and the error bound) delivers them into the group's piece in the caller's layout.
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_NORMALIZE_H
#define VORBISPIZZA_MULTI_NORMALIZE_H

#include <stdint.h>

#include "vorbispizza_multi_loudness.h"
#include "vorbispizza_multi_resample.h"
#include "vorbispizza_pcm_normalize.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZM_NORM_MEANVAR 1  /* the stage's four, with its values */
#define VPZM_NORM_PEAK 2
#define VPZM_NORM_RMS 3
#define VPZM_NORM_GAIN 4     /* `target` is ONE linear gain for every entry: with a ceiling a level rule of its own, and at target 1, ceiling 0 the resampled call, bit for bit */
#define VPZM_NORM_LOUDNESS 5 /* `target` in LUFS: every entry's window measured as vpzm_measure_loudness measures it, then delivered through g = 10^((target - L) / 20) */

/* sizeof(vpzm_norm_spec) == 64: 3 doubles, 1 + 9 int32 */
typedef struct vpzm_norm_spec {
    double target;        /* PEAK, RMS, GAIN: linear, finite and > 0; LOUDNESS: LUFS, finite; MEANVAR: not read */
    double eps;           /* MEANVAR: added to the variance (1e-7: Wav2Vec2FeatureExtractor's); finite and >= 0 in every mode */
    double ceiling;       /* 0: none; > 0 (not with MEANVAR): the delivered row's peak g * P stays at or below it */
    int32_t mode;         /* VPZM_NORM_* */
    int32_t reserved[9];  /* zero: room to grow */
} vpzm_norm_spec;

/* sizeof(vpzm_norm_out) == 32.  An entry that delivered nothing: { 1, 0, 0, -HUGE_VAL } */
typedef struct vpzm_norm_out {
    double gain;     /* g: the row was made with (float)gain.  The float32 value itself, widened -- but in the loudness mode, where the ceiling
                      * did not bind, the 10^((target - L) / 20) it is the rounding of */
    double mean;     /* m, the float32 value the row was made with (0 but for MEANVAR) */
    double peak;     /* P, max |x| over the resampled row's real samples, before the gain */
    double loudness; /* LOUDNESS: the window's integrated loudness in LUFS, vpzm_measure_loudness's `integrated` bit for bit; -HUGE_VAL otherwise */
} vpzm_norm_out;

/* vpzm_decode_ranges_resampled with its rows normalised.  Every argument up to `stats` is that call's and means what it means there;
 * results[k].samples, the per-entry statuses (VPZM_E_CHANNELS, VPZM_E_RATE, VPZM_E_CAPACITY and the rest) and the zero rows of entries
 * that deliver nothing are that call's too.  Statistics are joint over an entry's channels * J delivered samples (after the resample and
 * the downmix), the padding stays +0.0 / 0.
 * VPZM_NORM_LOUDNESS: entry k's window is measured at the stream's own rate, before the resample, exactly as vpzm_measure_loudness
 * measures it (one vpz_pcm_loudness launch per rate among a sub-batch's members, the small copy down, vpz_loudness_gate on the issuing
 * thread); g = pow(10, (target - L) / 20) in double, 1 where L is -HUGE_VAL (a window shorter than 400 ms, or gated away); the sub-batch
 * is then delivered in VPZ_NORM_GAIN mode with the spec's ceiling, which applies to the peak of the resampled row -- what is delivered.
 * A stream whose rate vpz_pcm_loudness refuses (outside 8000 .. 384000 Hz) ends as VPZM_E_RATE.
 * `out`: null, or n records; out[k] is entry k's.  A failed delivery launch (the step is named vpz_pcm_normalize in vpzm_last_error)
 * costs the sub-batch's members VPZM_E_SYNTH and leaves them zero rows, as in the resampled call.
 * VPZM_E_ARG: what vpzm_decode_ranges_resampled refuses; a null spec; an unknown mode; a target its mode reads that is not finite or (a
 * linear one) not > 0; eps or ceiling not finite or < 0; a ceiling with MEANVAR; a non-zero reserved word. */
int vpzm_decode_ranges_normalized(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size,
                                  const vpzm_range *ranges, int32_t sample_rate, int32_t channels, int32_t downmix, int64_t frames,
                                  int32_t out_layout, void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats,
                                  const vpzm_norm_spec *spec, vpzm_norm_out *out);

#ifdef __cplusplus
}
#endif
#endif
