/*
 * vorbispizza_pcm_pack.h -- windows of a device PCM array delivered as a dense, zero-padded batch in device memory,
 * libvorbispizza_synth.so.
 *
 * A batched synth call into device memory leaves every stream's PCM in an area of its own, interleaved, with more samples
 * than a caller's window in front and behind.  A host whose consumer runs on the same device -- a loader that feeds a model
 * -- wants one dense tensor [batch][channels][frames] and no trip over the host link: vpz_pcm_pack trims every window out of
 * its area, lays it out in the batch's format and fills the rest of its row with zeros, in one kernel launch.
 *
 * A header of its own: vorbispizza_synth.h, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_PACK_H
#define VORBISPIZZA_PCM_PACK_H

#include <stdint.h>

#include "vorbispizza_synth.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vpz_pack_row {
    int64_t src;      /* element offset of the window's first sample (channel 0) in the source array */
    int64_t samples;  /* samples per channel to copy, 0 <= samples <= frames; the rest of the row becomes zero */
    int64_t row;      /* destination row, 0 <= row < dst_rows */
} vpz_pack_row;

/* Source: `src_elems` elements of device memory, interleaved [sample][channel] -- what a synth call with VPZ_OUT_INTERLEAVED
 * (float32) or VPZ_OUT_INTERLEAVED_S16 (int16) writes.  dst_layout names the element type and the destination's order: float32
 * for VPZ_OUT_INTERLEAVED and VPZ_OUT_PLANAR, int16 for the two _S16 layouts (the values are moved as bits, never converted);
 * the planar layouts give dst[dst_rows][channels][frames], the interleaved ones dst[dst_rows][frames][channels], dense.
 * Every element of every row named by a descriptor is written exactly once -- `samples` samples per channel from the source,
 * then zeros (+0.0f / 0) --, rows that no descriptor names are not touched.  `rows` is host memory and is free again when the
 * call returns; the kernel runs asynchronously on the context's stream (vpz_context_synchronize completes it).
 * VPZ_E_INVALID_ARG, with nothing launched: a null pointer; channels outside 1..VPZ_MAX_CHANNELS; frames < 1; n_rows < 0;
 * dst_rows < 0; a layout other than the four; a descriptor whose source range [src, src + samples * channels) leaves
 * [0, src_elems), whose samples exceed frames or whose row is out of range or named twice; dst_dev not aligned to its element;
 * src_dev or dst_dev not device memory of the context's device, or [dst_dev, dst_dev + dst_rows * channels * frames elements)
 * (for the source: src_elems elements) not inside one allocation. */
int vpz_pcm_pack(vpz_context *ctx, const void *src_dev, int64_t src_elems, int32_t channels,
                 int32_t n_rows, const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows, int64_t frames, int32_t dst_layout);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_PACK_H */
