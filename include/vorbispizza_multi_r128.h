/*
 * vorbispizza_multi_r128.h -- the dispatcher of vorbispizza_multi.h: windows of streams, or whole streams, measured for everything an
 * EBU R 128 scanner reports, on the device (libvorbispizza_host.so).
 *
 * vorbispizza_multi_loudness.h gives the gated integrated loudness and the sample peak of every entry and lists the true peak, the
 * loudness range and the short-term values as out of scope: this header supplies what that one leaves out.  vpzm_measure_r128 is
 * vpzm_measure_loudness -- the same arguments, statuses, partition, sub-batches, routes and fall-backs -- with one more launch in its
 * delivery: per sample rate among a sub-batch's members one vpz_pcm_loudness and one vpz_pcm_true_peak launch
 * (vorbispizza_pcm_r128.h, which states the definitions); the step sums, sample peaks and true peaks come down in the one small copy, and
 * vpz_loudness_gate, vpz_loudness_range and vpz_loudness_maxima run per member on the issuing thread.  No PCM crosses the host link.
 *
 * Out of scope: int16 sources, per-channel peaks, the vpzr_* reader.  A gain applied on delivery is vpzm_decode_ranges_normalized's
 * (vorbispizza_multi_normalize.h), whose loudness mode measures the integrated loudness and applies the gain in one call.
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_R128_H
#define VORBISPIZZA_MULTI_R128_H

#include <stdint.h>

#include "vorbispizza_multi_loudness.h"
#include "vorbispizza_pcm_r128.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vpzm_r128 {
    double integrated;      /* LUFS, gated (vpz_loudness_gate): vpzm_measure_loudness's bits */
    double range;           /* LU (vpz_loudness_range); 0 with fewer than 30 steps or nothing kept */
    double range_low;       /* LUFS: the 10th percentile behind `range`; -HUGE_VAL with it */
    double range_high;      /* LUFS: the 95th */
    double momentary_max;   /* LUFS: the loudest 400 ms block (vpz_loudness_maxima); -HUGE_VAL without a finite level */
    double short_term_max;  /* LUFS: the loudest 3 s block */
    double true_peak;       /* the largest |y| of the oversampled signal over all channels (vpz_pcm_true_peak), a float32 value */
    double sample_peak;     /* the largest |x| over all channels, a float32 value: vpzm_loudness's `peak` */
    int64_t steps;          /* whole 100 ms steps measured */
    int64_t blocks_kept;    /* 400 ms blocks behind `integrated` */
    int64_t range_blocks;   /* 3 s blocks behind `range` */
} vpzm_r128;

/* Every argument is vpzm_measure_loudness's, and so is what results[k] and the call report -- VPZM_E_RATE for a stream whose rate is
 * outside VPZ_LOUDNESS_MIN_RATE .. VPZ_LOUDNESS_MAX_RATE, VPZM_E_SYNTH for the members of a sub-batch whose launch failed.  out[k] is
 * vpz_pcm_loudness and vpz_pcm_true_peak of the window's interleaved float32 samples followed by the gate, the range and the maxima, bit
 * for bit, on every route; `integrated`, `sample_peak`, `steps` and `blocks_kept` are vpzm_measure_loudness's bits for the same entry.
 * An entry that delivered nothing -- whatever its status -- has
 * out[k] = {-HUGE_VAL, 0, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL, 0, 0, 0, 0, 0}.
 * VPZM_E_ARG: out null with n > 0; what vpzm_decode_ranges refuses. */
int vpzm_measure_r128(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                      vpzm_r128 *out, vpzm_stream_result *results, vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
