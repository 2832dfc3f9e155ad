/*
 * vorbispizza_multi_cqt.h -- the dispatcher of vorbispizza_multi.h: the window batch of vorbispizza_multi_resample.h delivered as
 * per-channel constant-Q spectrograms -- complex, magnitude or power --, computed on the device (libvorbispizza_host.so).
 *
 * vpzm_decode_ranges_cqt is vpzm_decode_ranges_stft (vorbispizza_multi_stft.h) with vpz_pcm_cqt (vorbispizza_pcm_cqt.h, which states the
 * definition) as its feature stage: the same call -- the same partition, sub-batches, routes and fall-backs --, one launch per sub-batch
 * with one descriptor per (member, channel).
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_CQT_H
#define VORBISPIZZA_MULTI_CQT_H

#include <stdint.h>

#include "vorbispizza_multi_resample.h"
#include "vorbispizza_pcm_cqt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vpzm_decode_ranges_resampled(sample_rate, channels, downmix, planar float32) followed by vpz_pcm_cqt(spec) with every channel of
 * every row as a row of its own and the row's delivered samples J as its L.  `channels` and `downmix` are the resampled call's: C =
 * channels rows per entry, or, with downmix 1 (and channels 1), the one mixed-down row.  `frames` is the padded length F in OUTPUT
 * samples (at sample_rate, which a caller sets to the spec's); every row has T = 1 + frames / hop frames of n_bins bins.  group_dst[g]
 * is group g's piece, float32 device memory on that group's device, [hi - lo][C][n_bins][T] (VPZ_CQT_BINS_FIRST; a last dimension of 2
 * for VPZ_CQT_COMPLEX) or [hi - lo][C][T][n_bins], entry k's channel c in row (k - lo) * C + c (vpzm_batch_partition).  The resampled
 * rows never reach the caller: they live in a device temporary of the dispatcher's, [members][C][frames].
 * results[k] is what vpzm_decode_ranges_resampled reports: `samples` the OUTPUT samples J of the window.  Per-entry statuses are those
 * of the resampled call: VPZM_E_CHANNELS without downmix for a stream of another channel count, VPZM_E_RATE for a refused ratio,
 * VPZM_E_CAPACITY when ceil(window * up / down) > frames, and the older ones.  The rows of an entry that delivered nothing -- whatever
 * its status -- are zeros in all its channels.
 * VPZM_E_ARG: spec null or outside the limits of vorbispizza_pcm_cqt.h; frames < 1; VPZ_CQT_PAD_REFLECT and frames < floor(N_0 / 2) + 1;
 * what vpzm_decode_ranges_resampled refuses. */
int vpzm_decode_ranges_cqt(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                           int32_t sample_rate, int32_t channels, int32_t downmix, const vpz_cqt_spec *spec, int64_t frames,
                           void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
