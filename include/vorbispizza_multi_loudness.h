/*
 * vorbispizza_multi_loudness.h -- the dispatcher of vorbispizza_multi.h: windows of streams, or whole streams, measured for programme
 * loudness (ITU-R BS.1770-4 / EBU R 128) on the device (libvorbispizza_host.so).
 *
 * vorbispizza_multi_ranges.h names a loudness scanner among the callers of a ranges call.  What a scanner wants of a stream is a
 * handful of numbers, and a ranges call brings all of its PCM down the host link for them.  vpzm_measure_loudness is the batch call of
 * vorbispizza_multi_batch.h -- the same partition, sub-batches, routes and fall-backs -- with vpz_pcm_loudness
 * (vorbispizza_pcm_loudness.h, which states the definition) as its delivery: the PCM stays in the lane's device array, one launch per
 * sample rate among a sub-batch's members measures it there, the step sums and peaks come down in one small copy, and
 * vpz_loudness_gate runs per member on the issuing thread.
 *
 * Out of scope: the true peak, loudness range and short-term values, the vpzr_* reader.  A gain applied on delivery is
 * vpzm_decode_ranges_normalized's (vorbispizza_multi_normalize.h): its loudness mode measures as this call does and delivers in one call.
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_LOUDNESS_H
#define VORBISPIZZA_MULTI_LOUDNESS_H

#include <stdint.h>

#include "vorbispizza_multi_ranges.h"
#include "vorbispizza_pcm_loudness.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vpzm_loudness {
    double integrated;    /* LUFS, gated (vpz_loudness_gate); -HUGE_VAL with fewer than four steps or nothing kept */
    double peak;          /* the sample peak: the largest |x| over all channels, a float32 value */
    int64_t steps;        /* whole 100 ms steps measured: samples / ((sample_rate + 5) / 10) */
    int64_t blocks_kept;  /* 400 ms blocks behind `integrated` */
} vpzm_loudness;

/* Entry k's window ranges[k] (ranges == null: every stream whole, the range {0, -1}) is decoded as vpzm_decode_ranges_batch decodes it,
 * at the stream's own rate and channel count -- there is no caller tensor and no cap on a window's length --, and measured as a clip of
 * its own with the channel weights vpz_loudness_weights(channels): out[k] is vpz_pcm_loudness of the window's interleaved float32
 * samples followed by vpz_loudness_gate, bit for bit, on every route.  out and results have n entries.
 * results[k] is what the batch call reports, `samples` the samples measured.  Per-entry statuses are the batch call's, and VPZM_E_RATE
 * for a stream whose rate is outside VPZ_LOUDNESS_MIN_RATE .. VPZ_LOUDNESS_MAX_RATE; a failed launch gives its sub-batch's members
 * VPZM_E_SYNTH.  An entry that delivered nothing -- whatever its status -- has out[k] = {-HUGE_VAL, 0, 0, 0}.
 * VPZM_E_ARG: out null with n > 0; what vpzm_decode_ranges refuses. */
int vpzm_measure_loudness(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                          vpzm_loudness *out, vpzm_stream_result *results, vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
