/*
 * vorbispizza_multi_fbank.h -- the dispatcher of vorbispizza_multi.h: the window batch of vorbispizza_multi_resample.h delivered as
 * Kaldi filterbank feature frames, computed on the device (libvorbispizza_host.so).
 *
 * vpzm_decode_ranges_logmel (vorbispizza_multi_logmel.h) covers the Whisper-style front end.  A loader for a Kaldi-style recipe --
 * WeNet, icefall / k2, ESPnet, most Conformer and Zipformer models -- follows the mono resampled call with unfold, mean, pre-emphasis,
 * window, pad, rfft, power, matmul and log, and the framed copy of the batch and the complex spectrogram go through device memory on the
 * way.  vpzm_decode_ranges_fbank is the same call -- the same partition, sub-batches, routes and fall-backs -- with one more stage,
 * vpz_pcm_fbank (vorbispizza_pcm_fbank.h, which states the definition): one launch per sub-batch.
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_FBANK_H
#define VORBISPIZZA_MULTI_FBANK_H

#include <stdint.h>

#include "vorbispizza_multi_resample.h"
#include "vorbispizza_pcm_fbank.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vpzm_decode_ranges_resampled(sample_rate = spec->sample_rate, channels 1, downmix 1, float32) followed by vpz_pcm_fbank(spec) with
 * every row's delivered samples J as its L.  `frames` is the padded length F in OUTPUT samples (at spec->sample_rate, a whole number
 * of Hz); every row has T = 1 + (frames - win) / hop feature frames.  group_dst[g] is group g's piece, float32 device memory on that
 * group's device, [hi - lo][T][n_mels] (VPZ_FBANK_FRAMES_FIRST) or [hi - lo][n_mels][T], entry k in row k - lo (vpzm_batch_partition).
 * The resampled rows never reach the caller: they live in a device temporary of the dispatcher's.
 * results[k] is what vpzm_decode_ranges_resampled reports: `samples` the OUTPUT samples J of the window, from which the caller has the
 * row's real frames T_L (0 if J < win, else 1 + (J - win) / hop); the frames behind them hold pad_value.  Per-entry statuses are those
 * of the resampled call with downmix 1: VPZM_E_RATE for a refused ratio, VPZM_E_CAPACITY when ceil(window * up / down) > frames, and
 * the older ones.  The row of an entry that delivered nothing -- whatever its status -- holds pad_value in every element.
 * VPZM_E_ARG: spec null or outside the limits of vorbispizza_pcm_fbank.h; a sample_rate that is no whole number of Hz; frames < win;
 * what vpzm_decode_ranges_resampled refuses. */
int vpzm_decode_ranges_fbank(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                             const vpz_fbank_spec *spec, int64_t frames, void *const *group_dst, vpzm_stream_result *results,
                             vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
