/*
 * vorbispizza_multi_ranges.h -- the dispatcher of vorbispizza_multi.h: a WINDOW of samples out of every stream in one batched
 * call (libvorbispizza_host.so).
 *
 * vpzm_decode_library decodes every stream from its first packet to its last.  A caller that wants a second out of each of a
 * thousand songs -- a dataset loader, a preview generator, a loudness scanner -- would decode the thousand songs and slice on
 * the host.  vpzm_decode_ranges decodes, per entry, only the packets its window needs (vpzh_window, vorbispizza_front.h: the
 * pre-roll packet before the window's first sample through the packet of its last), through the same pipeline: the same
 * partition, sub-batches, routes (vpzm_options.gpu_entropy, vpzm_set_mixed_setups) and fall-backs.  An IMDCT frame depends on
 * its own packet only and overlap-add on the one block before it, so a window decoded from its pre-roll packet is the same
 * bits as the same samples of the whole decode.
 *
 * A header of its own: vorbispizza_multi.h, its structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_RANGES_H
#define VORBISPIZZA_MULTI_RANGES_H

#include <stdint.h>

#include "vorbispizza_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZM_E_RANGE (-14)   /* per-stream status: start < 0 or beyond the stream's total samples (vpzh_total_samples) */

typedef struct vpzm_range {
    int64_t start, count;    /* samples per channel; count < 0: to the end of the stream */
} vpzm_range;

/* Entry k is the window ranges[k] of the first logical stream of container k (the same container may appear many times).
 * Its samples -- min(count, total - start) of them, vpzh_window's `samples` -- land at pcm_out + pcm_offset[k], interleaved,
 * float32 or int16 as in vpzm_decode_library, and nothing else of the caller's array is written; pcm_capacity[k] smaller
 * than that is VPZM_E_CAPACITY, a window outside the stream VPZM_E_RANGE: statuses of the entry, which costs only itself.
 * results[k].samples: samples delivered; .packets: the packets decoded for the window, the pre-roll packet included (0 for an
 * empty window, which is VPZM_OK); .skipped_packets: the skipped ones among those.
 * No packet of the window skipped: the samples are bit for bit samples [start, start + samples) of what vpzm_decode_library
 * writes for the container, on both routes, for both PCM types, whatever the partition, the sub-batch cut and the options.
 * The decoder's stream is set to the counted position of the window's first packet before it, so a window that reaches the
 * last packet gets the whole decode's end-of-stream trim.
 * A packet of the window skipped (a damaged stream): the entry gets what the decoder produced from the window's packets
 * after dropping the samples before `start` -- possibly fewer than asked, never more; both routes give the same bytes.
 * Everything else -- arguments, stats, the one call at a time -- is vpzm_decode_library's. */
int vpzm_decode_ranges(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                       int32_t out_layout, void *pcm_out, const int64_t *pcm_offset, const int64_t *pcm_capacity,
                       vpzm_stream_result *results, vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
