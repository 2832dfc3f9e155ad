/*
 * vorbispizza_entropy_group.h -- vpz_entropy_decode (vorbispizza_entropy.h) for streams of DIFFERENT setup headers in one
 * call, libvorbispizza_synth.so.
 *
 * vpz_entropy_decode knows one setup image, so a library of many setups is decoded in many small calls, and a small call
 * costs what a large one costs: the latency of one packet's bit chain.  A group holds up to 256 validated images of one
 * class -- the same channel count and block sizes -- and decodes a batch whose streams each name their setup: one payload,
 * one launch, one set of outputs in the layout vpz_decoder_synth takes.  The decoder that consumes the result is created
 * from the union of the setups' floors and mappings, every setup's mappings starting at a base of its own
 * (stream_mapping_base); the records carry the index in that union.
 *
 * A header of its own: vorbispizza_entropy.h, VPZ_ENTROPY_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, POD structs, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_ENTROPY_GROUP_H
#define VORBISPIZZA_ENTROPY_GROUP_H

#include <stdint.h>

#include "vorbispizza_entropy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_ENTROPY_GROUP_MAX_SETUPS 256

typedef struct vpz_entropy_group vpz_entropy_group;  /* validated images of one class on one context's device */

/* Validates images[s] (sizes[s] bytes), s < n_setups, each as vpz_entropy_setup_create validates its image, and uploads them.
 * VPZ_E_INVALID_ARG with the reason in the context's error text, nothing allocated: an image that fails a check, n_setups
 * outside 1 .. VPZ_ENTROPY_GROUP_MAX_SETUPS, images that differ in channels, block_size0 or block_size1.  The group owns its
 * images and all per-call scratch; it belongs to `ctx`, serves one call at a time and is destroyed before its context. */
int  vpz_entropy_group_create(vpz_context *ctx, const void *const *images, const uint64_t *sizes, int32_t n_setups,
                              vpz_entropy_group **out);
void vpz_entropy_group_destroy(vpz_entropy_group *g);

/* vpz_entropy_decode over streams of the group's setups.  Its contract, with these differences:
 *   packet k belongs to stream packets[k].stream, which must lie in [0, n_streams);
 *   stream_setup[n_streams]: the setup of each stream, < n_setups (host memory, always);
 *   stream_mapping_base[n_streams]: packets[k].mapping - stream_mapping_base[stream] is the mapping index in the stream's own
 *     setup; for a decoded packet it must lie in [0, that setup's mapping_count);
 *   VPZ_RESIDUE_I16 only when every setup of the group allows it.
 * Every stream's posts, post counts and residue are what the CPU front end writes for it from its own setup.  A bad batch
 * is VPZ_E_INVALID_ARG with nothing written. */
int vpz_entropy_group_decode(vpz_entropy_group *g, int32_t n_streams, const uint8_t *stream_setup,
                             const uint8_t *stream_mapping_base, int64_t n_packets, const vpz_packet *packets,
                             const vpz_entropy_span *spans, const uint8_t *payload, int64_t payload_bytes, int32_t residue_format,
                             void *residue, int64_t residue_values, int16_t *posts, uint8_t *post_counts, int64_t n_records,
                             int32_t mem_space);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_ENTROPY_GROUP_H */
