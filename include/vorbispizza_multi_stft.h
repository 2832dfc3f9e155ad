/*
 * vorbispizza_multi_stft.h -- the dispatcher of vorbispizza_multi.h: the window batch of vorbispizza_multi_resample.h delivered as
 * per-channel short-time Fourier spectrograms -- complex, magnitude or power -- with transforms of 512 to 8192 samples, computed on the
 * device (libvorbispizza_host.so).
 *
 * The other feature calls of the family (vpzm_decode_ranges_logmel, _melspec, _fbank, _mfcc) reduce the spectrum to mel bands and are
 * mono.  vpzm_decode_ranges_stft keeps the spectrum and keeps the channels: the same call -- the same partition, sub-batches, routes and
 * fall-backs -- with vpz_pcm_stft (vorbispizza_pcm_stft.h, which states the definition) as its feature stage: one launch per sub-batch
 * with one descriptor per (member, channel).
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_STFT_H
#define VORBISPIZZA_MULTI_STFT_H

#include <stdint.h>

#include "vorbispizza_multi_resample.h"
#include "vorbispizza_pcm_stft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vpzm_decode_ranges_resampled(sample_rate, channels, downmix, planar float32) followed by vpz_pcm_stft(spec) with every channel of
 * every row as a row of its own and the row's delivered samples J as its L.  `channels` and `downmix` are the resampled call's: C =
 * channels rows per entry, or, with downmix 1 (and channels 1), the one mixed-down row.  `frames` is the padded length F in OUTPUT
 * samples (at sample_rate); every row has T = 1 + frames / hop spectrum frames of n_freq = n_fft / 2 + 1 bins.  group_dst[g] is group
 * g's piece, float32 device memory on that group's device, [hi - lo][C][n_freq][T] (VPZ_STFT_BINS_FIRST; a last dimension of 2 for
 * VPZ_STFT_COMPLEX) or [hi - lo][C][T][n_freq], entry k's channel c in row (k - lo) * C + c (vpzm_batch_partition).  The resampled rows
 * never reach the caller: they live in a device temporary of the dispatcher's, [members][C][frames].
 * results[k] is what vpzm_decode_ranges_resampled reports: `samples` the OUTPUT samples J of the window.  Per-entry statuses are those
 * of the resampled call: VPZM_E_CHANNELS without downmix for a stream of another channel count, VPZM_E_RATE for a refused ratio,
 * VPZM_E_CAPACITY when ceil(window * up / down) > frames, and the older ones.  The rows of an entry that delivered nothing -- whatever
 * its status -- are zeros in all its channels.
 * VPZM_E_ARG: spec null or outside the limits of vorbispizza_pcm_stft.h; frames < n_fft / 2 + 1; what vpzm_decode_ranges_resampled
 * refuses. */
int vpzm_decode_ranges_stft(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                            int32_t sample_rate, int32_t channels, int32_t downmix, const vpz_stft_spec *spec, int64_t frames,
                            void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
