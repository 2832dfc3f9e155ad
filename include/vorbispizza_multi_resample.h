/*
 * vorbispizza_multi_resample.h -- the dispatcher of vorbispizza_multi.h: the padded device batch of vorbispizza_multi_batch.h delivered
 * at ONE sample rate, optionally mixed down to mono (libvorbispizza_host.so).
 *
 * vpzm_decode_ranges_batch gives every row at its stream's own rate, and one channel count per batch.  A loader that feeds a model
 * follows it with a resample per distinct rate and a downmix.  vpzm_decode_ranges_resampled is the same call -- the same partition,
 * sub-batches, routes and fall-backs -- whose last stage is vpz_pcm_resample (vorbispizza_pcm_resample.h, which states the filter)
 * instead of vpz_pcm_pack.
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_RESAMPLE_H
#define VORBISPIZZA_MULTI_RESAMPLE_H

#include <stdint.h>

#include "vorbispizza_multi_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZM_E_RATE (-16)  /* per-entry status: the ratio of the stream's rate to the batch's is one vpz_pcm_resample refuses */

/* vpzm_decode_ranges_batch at `sample_rate`.  `ranges` stay in SOURCE samples, at each stream's own rate.  Entry k's window -- the L
 * samples vpzm_decode_ranges delivers for it -- is resampled as a clip of its own (zero outside [0, L): neither the decoder's roll nor
 * what follows the window is filter context, so a row is NOT the slice of the resampled whole stream) by up / down =
 * sample_rate / the stream's rate in lowest terms, and row k holds its J = ceil(L * up / down) samples, then zeros.
 * downmix 0: rows have `channels` channels and a stream needs as many.  downmix 1: `channels` must be 1, every stream is accepted and
 * its channels are averaged.  Row shapes, element types and group_dst are those of vpzm_decode_ranges_batch.
 * results[k] is what vpzm_decode_ranges_batch reports, with `samples` the OUTPUT samples in the row (ceil(delivered * up / down) for
 * whatever the window delivered, a damaged stream's included); `sample_rate` and `channels` stay the stream's own.  Per-entry statuses:
 * VPZM_E_CHANNELS as above; VPZM_E_RATE for a refused ratio (up > 1024 or down > 32 * up); VPZM_E_CAPACITY when
 * ceil(window * up / down) > frames.  A call with `sample_rate` equal to every stream's rate and downmix 0 delivers what
 * vpzm_decode_ranges_batch delivers, bit for bit, in all four layouts.
 * VPZM_E_ARG: what vpzm_decode_ranges_batch refuses; sample_rate < 1; downmix other than 0 or 1; downmix 1 with channels != 1. */
int vpzm_decode_ranges_resampled(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size,
                                 const vpzm_range *ranges, int32_t sample_rate, int32_t channels, int32_t downmix, int64_t frames,
                                 int32_t out_layout, void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
