/*
 * vorbispizza_multi_featpost.h -- the dispatcher of vorbispizza_multi.h: the Kaldi filterbank and MFCC window batches of
 * vorbispizza_multi_fbank.h and vorbispizza_multi_mfcc.h with Kaldi's feature post-processing -- delta features, mean / variance
 * normalisation over the row or a sliding window -- behind them, on the device (libvorbispizza_host.so).
 *
 * A loader that follows vpzm_decode_ranges_mfcc with add-deltas and apply-cmvn-sliding in a framework masks the pad frames by hand, runs
 * one padded convolution per delta order (which does not match Kaldi at the edges from the second order on) and a cumsum / unfold chain
 * per row for the window's edge rules, because every row has its own real length.  These calls are the existing ones -- the same
 * partition, sub-batches, routes and fall-backs -- with vpz_feat_post (vorbispizza_pcm_featpost.h, which states the definition) behind
 * the feature launch: per sub-batch the feature launch writes a device temporary of the dispatcher's, [members][T][D], and
 * vpz_feat_post's one to three launches on the same stream deliver it into the group's piece with every row's real frames.
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_FEATPOST_H
#define VORBISPIZZA_MULTI_FEATPOST_H

#include <stdint.h>

#include "vorbispizza_multi_fbank.h"
#include "vorbispizza_multi_mfcc.h"
#include "vorbispizza_pcm_featpost.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vpzm_decode_ranges_fbank(spec) followed by vpz_feat_post(post) over its tensor, with real_frames of entry k = T_L(J), J the window's
 * delivered output samples (results[k].samples; T_L = 0 if J < win, else 1 + (J - win) / hop) -- bit for bit, without that tensor ever
 * reaching the caller.  D = spec->n_mels; group_dst[g] is float32 device memory [hi - lo][T][D_out] (VPZ_FBANK_FRAMES_FIRST) or
 * [hi - lo][D_out][T], D_out = D * (post->delta_order + 1), entry k in row k - lo (vpzm_batch_partition).  post->layout is the
 * feature spec's layout (the VPZ_FEAT_* values are the VPZ_FBANK_* ones); frames behind a row's real ones hold post->pad_value, and so
 * does the whole row of an entry that delivered nothing -- whatever its status -- from a launch that reads nothing.  results, per-entry
 * statuses, stats and the VPZM_FAIL_DELIVERY switch are those of vpzm_decode_ranges_fbank.
 * post == NULL: vpzm_decode_ranges_fbank itself, bit for bit.
 * VPZM_E_ARG: what vpzm_decode_ranges_fbank refuses; a post spec outside the limits of vorbispizza_pcm_featpost.h or in the other
 * layout. */
int vpzm_decode_ranges_fbank_post(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                                  const vpz_fbank_spec *spec, const vpz_feat_post_spec *post, int64_t frames, void *const *group_dst,
                                  vpzm_stream_result *results, vpzm_stats *stats);

/* The same over vpzm_decode_ranges_mfcc(spec): D = spec->n_ceps, the layout is spec->fbank.layout.  The MFCC spec's own subtract_mean
 * may be combined with a post spec: it runs first, as vorbispizza_pcm_mfcc.h defines it, inside the feature stage. */
int vpzm_decode_ranges_mfcc_post(vpzm_dispatcher *m, int32_t n, const uint8_t *const *data, const uint64_t *size, const vpzm_range *ranges,
                                 const vpz_mfcc_spec *spec, const vpz_feat_post_spec *post, int64_t frames, void *const *group_dst,
                                 vpzm_stream_result *results, vpzm_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
