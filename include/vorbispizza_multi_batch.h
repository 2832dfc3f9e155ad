/*
 * vorbispizza_multi_batch.h -- the dispatcher of vorbispizza_multi.h: the windows of vorbispizza_multi_ranges.h delivered as a
 * padded batch in DEVICE memory (libvorbispizza_host.so).
 *
 * vpzm_decode_ranges brings every window down to the host.  A dataset loader feeds a model that runs on the GPU the decoder ran
 * on: it would pad the windows on the CPU, stack them and upload them again.  vpzm_decode_ranges_batch is the same call -- the
 * same partition, sub-batches, routes and fall-backs -- whose last stage is vpz_pcm_pack (vorbispizza_pcm_pack.h) instead of the
 * download: entry k's window becomes row k of a dense tensor [n][channels][frames] (or [n][frames][channels]) on the device,
 * zeros behind its samples, and no PCM crosses the host link.
 *
 * A header of its own: vorbispizza_multi.h, its structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_BATCH_H
#define VORBISPIZZA_MULTI_BATCH_H

#include <stdint.h>

#include "vorbispizza_multi_ranges.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZM_E_CHANNELS (-15)  /* per-entry status: the stream does not have the batch's channel count */

/* group g of the dispatcher decodes entries [lo, hi) of an n-entry call: lo = n*g/D, hi = n*(g+1)/D, D = vpzm_device_count(m).
 * The rule of every call of the dispatcher (vpzm_decode_library, vpzm_decode_ranges, vpzm_decode_ranges_batch).
 * VPZM_E_ARG: a null pointer, n < 0, a group outside 0..D-1. */
int vpzm_batch_partition(vpzm_dispatcher *m, int32_t n, int32_t group, int32_t *lo, int32_t *hi);

/* vpzm_decode_ranges with a device destination.  group_dst[g] is device memory on group g's device and holds the rows of the
 * group's entries [lo_g, hi_g) (vpzm_batch_partition): entry k is row k - lo_g there, channels * frames elements -- float32 for
 * VPZ_OUT_PLANAR / VPZ_OUT_INTERLEAVED, int16 for the two _S16 layouts; planar rows are [channels][frames], interleaved ones
 * [frames][channels].  Groups that share a device may be handed consecutive pieces of one array: a one-GPU caller gets one tensor.
 * Entry k's row holds the samples vpzm_decode_ranges delivers for it, bit for bit, and zeros behind them; results[k] is what
 * vpzm_decode_ranges reports, with two statuses that speak of the batch: a window of more than `frames` samples is
 * VPZM_E_CAPACITY, a stream whose channel count is not `channels` VPZM_E_CHANNELS.  The row of an entry that delivers no samples
 * -- a failed entry, an empty window, a damaged stream that gave nothing after the roll -- is all zeros.  When the call returns
 * the lanes' streams have drained, every row of every group's piece is defined and nothing outside the pieces has been written.
 * VPZM_E_ARG: what vpzm_decode_ranges refuses; group_dst null, or null for a group with hi > lo; channels < 1 (or above
 * VPZ_MAX_CHANNELS); frames < 1; a layout other than the four. */
int vpzm_decode_ranges_batch(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size,
                             const vpzm_range *ranges, int32_t channels, int64_t frames, int32_t out_layout,
                             void *const *group_dst, vpzm_stream_result *results, vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
