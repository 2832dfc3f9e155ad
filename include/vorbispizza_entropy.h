/*
 * vorbispizza_entropy.h -- the per-packet entropy decode of Vorbis audio packets on the GPU, libvorbispizza_synth.so.
 *
 * The CPU front end (vorbispizza_front.h) pages the container and reads the setup header; for a setup it can decode on the
 * device (vpzh_gpu_decode_supported) it exports the decode tables as one flat, position-independent image
 * (vpzh_get_entropy_setup) and plans a range of packets (vpzh_plan_range): the vpz_packet records vpz_decoder_synth takes,
 * byte for byte what vpzh_decode_range_ex writes, plus each packet's bytes in one payload area.  vpz_entropy_decode then
 * writes what the CPU's decode_packet writes -- Floor1 posts, post counts, the residue -- from that payload, bit for bit.
 *
 * A header of its own: VPZ_ABI_VERSION of vorbispizza_synth.h and its bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, POD structs, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_ENTROPY_H
#define VORBISPIZZA_ENTROPY_H

#include <stdint.h>

#include "vorbispizza_synth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_ENTROPY_VERSION 1               /* vpz_entropy_version() */

/* ---- the setup image --------------------------------------------------------------------------------------------------
 * One contiguous block of little-endian words: a header, then arrays of the records below, then the tables they point to.
 * Every "offset" is a byte offset from the start of the image (4-byte aligned for 32-bit tables), every "count" a number
 * of elements; there are no pointers.  Padding bytes are zero, so that streams whose setup headers are equal produce
 * byte-identical images. */
#define VPZ_ENTROPY_IMAGE_MAGIC   0x45505A56u  /* "VZPE" */
#define VPZ_ENTROPY_IMAGE_VERSION 1
#define VPZ_ENTROPY_MAX_FLOOR1_PARTITIONS 32   /* 5-bit count */
#define VPZ_ENTROPY_MAX_FLOOR1_CLASSES    16   /* 4-bit class numbers */
#define VPZ_ENTROPY_MAX_SUBMAPS           16

typedef struct vpz_entropy_image_header {
    uint32_t magic;              /* VPZ_ENTROPY_IMAGE_MAGIC */
    uint32_t version;            /* VPZ_ENTROPY_IMAGE_VERSION */
    uint32_t total_bytes;        /* size of the whole image */
    int32_t channels, block_size0, block_size1;
    int32_t mode_field_bits;     /* ilog(mode_count - 1) */
    int32_t residue_integral;    /* 1: vpzh_residue_is_integral -- the int16 residue form is exact */
    int32_t book_count, floor_count, residue_count, mapping_count, mode_count;
    uint32_t books, floors, residues, mappings, modes;  /* offsets of the record arrays */
    uint32_t reserved[2];         /* zero */
} vpz_entropy_image_header;

/* A codebook (Codebook.cs / Huffman.cs).  decode: the first prefix_bits bits of the stream index the prefix table, whose
 * word is value << 6 | length (length 0: the code is longer than the table); then the overflow list in its order,
 * a code matching when (next max_bits bits & mask) == bits.  A miss is -1. */
typedef struct vpz_entropy_book {
    int32_t dimensions, entries, max_bits, prefix_bits;
    uint32_t prefix;             /* offset of prefix_count uint32 words */
    int32_t prefix_count;        /* 1 << prefix_bits, or 0 for a book without codes */
    uint32_t overflow;           /* offset of overflow_count vpz_entropy_code records */
    int32_t overflow_count;
    uint32_t lookup_f32;         /* offset of lookup_count float values: entry e, dimension d at e * dimensions + d */
    int32_t lookup_count;        /* entries * dimensions, or 0 for a book without value mapping */
    uint32_t lookup_i16;         /* offset of lookup_i16_count int16 values: the same, where every value is a 16-bit integer */
    int32_t lookup_i16_count;    /* lookup_count, or 0 */
} vpz_entropy_book;

typedef struct vpz_entropy_code {
    uint32_t value, length, bits, mask;
} vpz_entropy_code;

/* Floor type 1 (Floor1.cs:39-219), the part its Unpack reads. */
typedef struct vpz_entropy_floor1 {
    int32_t partition_count, y_bits;
    uint8_t partition_class[VPZ_ENTROPY_MAX_FLOOR1_PARTITIONS];
    uint8_t class_dimensions[VPZ_ENTROPY_MAX_FLOOR1_CLASSES];
    uint8_t class_subclasses[VPZ_ENTROPY_MAX_FLOOR1_CLASSES];
    uint8_t class_masterbooks[VPZ_ENTROPY_MAX_FLOOR1_CLASSES];
    int16_t subclass_books[VPZ_ENTROPY_MAX_FLOOR1_CLASSES * 8];  /* [class * 8 + subclass], -1: no book */
} vpz_entropy_floor1;

/* Residue types 0, 1, 2 (Residue0.cs). */
typedef struct vpz_entropy_residue {
    int32_t type, begin, end, partition_size, classifications, class_book, max_stages, class_dim;
    uint32_t stage_book;         /* offset of classifications * 8 int16: value book of (class, stage), -1: none */
    uint32_t decode_map;         /* offset of decode_map_count uint8: class of partition k of class word w at w * class_dim + k */
    int32_t decode_map_count;
    uint32_t word_stage_mask;    /* offset of word_stage_mask_count uint32: bit k of [w * 8 + stage] -- partition k of word w has
                                    a book at that stage (0 entries when class_dim > 32) */
    int32_t word_stage_mask_count;
    int32_t reserved;
} vpz_entropy_residue;

typedef struct vpz_entropy_mapping {  /* Mapping.cs:19-95 */
    int32_t submaps, coupling_steps;
    uint8_t submap_floor[VPZ_ENTROPY_MAX_SUBMAPS];
    uint8_t submap_residue[VPZ_ENTROPY_MAX_SUBMAPS];
    uint8_t mux[VPZ_MAX_CHANNELS + 1];
    uint8_t coupling_magnitude[VPZ_MAX_COUPLING];
    uint8_t coupling_angle[VPZ_MAX_COUPLING];
} vpz_entropy_mapping;

typedef struct vpz_entropy_mode {
    int32_t block_flag, mapping;
} vpz_entropy_mode;

/* Where packet k's bytes lie in the payload area: payload[offset .. offset + size).  The area holds at least 8 more bytes
 * after every packet (the device reads whole words). */
typedef struct vpz_entropy_span {
    int64_t offset;
    int64_t size;
} vpz_entropy_span;

typedef struct vpz_entropy_setup vpz_entropy_setup;  /* the validated image on one context's device */

int vpz_entropy_version(void);

/* Validates `image` (magic, version, size, every offset and count in range, every book / floor / residue / mapping index
 * in range, the residues' value books tiling their partitions) and uploads it once.  VPZ_E_INVALID_ARG for an image that
 * fails any check, nothing allocated.  The setup belongs to `ctx` and is destroyed before it. */
int  vpz_entropy_setup_create(vpz_context *ctx, const void *image, uint64_t size, vpz_entropy_setup **out);
void vpz_entropy_setup_destroy(vpz_entropy_setup *setup);

/* Entropy-decodes n_packets planned packets (vpzh_plan_range) of streams of this setup.
 *   packets[n_packets], spans[n_packets]: host memory, always.  Packets with VPZ_PKT_NOT_DECODED are not decoded.
 *   payload[payload_bytes]: the packets' bytes (mem_space; for VPZ_MEM_DEVICE 4-byte aligned); every span must satisfy
 *     0 <= offset, 0 <= size < 2^28 and offset + size + 8 <= payload_bytes.
 *   residue_format: VPZ_RESIDUE_F32 (float) or VPZ_RESIDUE_I16 (int16_t; only for a setup whose image says residue_integral).
 *   residue[residue_values]: each decoded packet writes channels * blocksize/2 values at its residue_offset -- the values
 *     vpzh_decode_range_ex (vpzh_decode_range_i16) writes there; nothing else of the buffer is written.
 *   posts[n_records * 64], post_counts[n_records]: records r = k * channels + c of every packet, as the CPU writes them
 *     (zeros for packets not decoded); n_records >= n_packets * channels.
 * Bounds are checked as vpz_decoder_synth checks them: a decoded packet's residue beyond residue_values, a span outside the
 * payload, too few records, a mapping index out of range, a bad format or mem_space are VPZ_E_INVALID_ARG with nothing
 * written.  VPZ_MEM_DEVICE: asynchronous on the context stream (a vpz_decoder_synth on the same context may consume the
 * outputs without a synchronise).  VPZ_MEM_HOST: uploads, decodes, downloads and synchronises. */
int vpz_entropy_decode(vpz_entropy_setup *setup, int64_t n_packets, const vpz_packet *packets, const vpz_entropy_span *spans,
                       const uint8_t *payload, int64_t payload_bytes, int32_t residue_format, void *residue,
                       int64_t residue_values, int16_t *posts, uint8_t *post_counts, int64_t n_records, int32_t mem_space);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_ENTROPY_H */
