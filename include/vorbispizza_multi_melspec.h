/*
 * vorbispizza_multi_melspec.h -- the dispatcher of vorbispizza_multi.h: the window batch of vorbispizza_multi_resample.h delivered as
 * (log-)mel spectrogram frames with transforms of 2048, 4096 and 8192 samples, computed on the device (libvorbispizza_host.so).
 *
 * vpzm_decode_ranges_logmel (vorbispizza_multi_logmel.h) stops at n_fft = 1024, a speech limit.  The mel front ends of music models
 * -- 22.05, 44.1 and 48 kHz, n_fft 2048 or 4096, a hop of 512 or 1024, 128 bands -- take vpzm_decode_ranges_melspec: the same call --
 * the same partition, sub-batches, routes and fall-backs -- with vpz_pcm_melspec (vorbispizza_pcm_melspec.h, which states the
 * definition) as its feature stage: one launch per sub-batch, one real FFT per frame, no spectrogram in device memory.
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_MELSPEC_H
#define VORBISPIZZA_MULTI_MELSPEC_H

#include <stdint.h>

#include "vorbispizza_multi_resample.h"
#include "vorbispizza_pcm_melspec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vpzm_decode_ranges_resampled(sample_rate = spec->sample_rate, channels 1, downmix 1, float32) followed by vpz_pcm_melspec(spec) with
 * every row's delivered samples J as its L.  `frames` is the padded length F in OUTPUT samples (at spec->sample_rate, a whole number
 * of Hz); every row has T = 1 + frames / hop feature frames.  group_dst[g] is group g's piece, float32 device memory on that group's
 * device, [hi - lo][n_mels][T] (VPZ_MEL_BANDS_FIRST) or [hi - lo][T][n_mels], entry k in row k - lo (vpzm_batch_partition).  The
 * resampled rows never reach the caller: they live in a device temporary of the dispatcher's.
 * results[k] is what vpzm_decode_ranges_resampled reports: `samples` the OUTPUT samples J of the window.  Per-entry statuses are those
 * of the resampled call with downmix 1: VPZM_E_RATE for a refused ratio, VPZM_E_CAPACITY when ceil(window * up / down) > frames, and
 * the older ones.  The row of an entry that delivered nothing -- whatever its status -- is the SILENCE ROW of the spec: 0, or
 * log10f(floor).
 * VPZM_E_ARG: spec null or outside the limits of vorbispizza_pcm_melspec.h; a sample_rate that is no whole number of Hz; frames <
 * n_fft / 2 + 1; what vpzm_decode_ranges_resampled refuses. */
int vpzm_decode_ranges_melspec(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                               const vpz_logmel_spec *spec, int64_t frames, void *const *group_dst, vpzm_stream_result *results,
                               vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
