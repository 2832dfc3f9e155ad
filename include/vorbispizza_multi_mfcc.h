/*
 * vorbispizza_multi_mfcc.h -- the dispatcher of vorbispizza_multi.h: the window batch of vorbispizza_multi_resample.h delivered as
 * Kaldi MFCC feature frames, computed on the device (libvorbispizza_host.so).
 *
 * vpzm_decode_ranges_fbank (vorbispizza_multi_fbank.h) covers the Kaldi filterbank.  A loader for an MFCC recipe -- speaker-ID, keyword
 * spotting, alignment, GMM / TDNN systems -- follows it with a second mono resampled call for the energy (a second decode), unfold, mean
 * and square-sum on that PCM, a matmul with the DCT, a lifter multiply, a column overwrite, a mean over frames and a subtraction.
 * vpzm_decode_ranges_mfcc is the fbank call -- the same partition, sub-batches, routes and fall-backs -- with vpz_pcm_mfcc
 * (vorbispizza_pcm_mfcc.h, which states the definition) as the feature stage: one launch per sub-batch, two with subtract_mean.
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_MFCC_H
#define VORBISPIZZA_MULTI_MFCC_H

#include <stdint.h>

#include "vorbispizza_multi_resample.h"
#include "vorbispizza_pcm_mfcc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vpzm_decode_ranges_resampled(sample_rate = spec->fbank.sample_rate, channels 1, downmix 1, float32) followed by vpz_pcm_mfcc(spec)
 * with every row's delivered samples J as its L.  `frames` is the padded length F in OUTPUT samples (at spec->fbank.sample_rate, a whole
 * number of Hz); every row has T = 1 + (frames - win) / hop feature frames.  group_dst[g] is group g's piece, float32 device memory on
 * that group's device, [hi - lo][T][n_ceps] (VPZ_FBANK_FRAMES_FIRST) or [hi - lo][n_ceps][T], entry k in row k - lo
 * (vpzm_batch_partition).  The resampled rows never reach the caller: they live in a device temporary of the dispatcher's.
 * results[k] is what vpzm_decode_ranges_resampled reports: `samples` the OUTPUT samples J of the window, from which the caller has the
 * row's real frames T_L (0 if J < win, else 1 + (J - win) / hop); the frames behind them hold pad_value.  Per-entry statuses are those
 * of the resampled call with downmix 1.  The row of an entry that delivered nothing -- whatever its status -- holds pad_value in every
 * element.
 * VPZM_E_ARG: spec null or outside the limits of vorbispizza_pcm_mfcc.h; a sample_rate that is no whole number of Hz; frames < win;
 * what vpzm_decode_ranges_resampled refuses. */
int vpzm_decode_ranges_mfcc(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                            const vpz_mfcc_spec *spec, int64_t frames, void *const *group_dst, vpzm_stream_result *results,
                            vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
