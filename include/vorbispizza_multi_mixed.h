/*
 * vorbispizza_multi_mixed.h -- the dispatcher of vorbispizza_multi.h: streams of DIFFERENT setup headers in one device-decoded
 * sub-batch, and the counts of the last call (libvorbispizza_host.so).
 *
 * vpzm_decode_library cuts its sub-batches per setup header.  A library of many setups -- several encoder versions, quality
 * settings, sample rates -- is cut into many small ones, and each pays a launch's latency, its own upload, synth call and
 * downloads.  With mixed_setups on (and vpzm_options.gpu_entropy: only device-decoded sub-batches mix) the streams of a MERGE
 * CLASS -- setups the device can decode that agree in channel count, block sizes and in whether their residue is integral --
 * are pooled in job order and cut by the same limits; a sub-batch of several setups is one payload upload, one
 * vpz_entropy_group_decode (vorbispizza_entropy_group.h) and one vpz_decoder_synth on a decoder created from the union of
 * the setups' floors and mappings (at most 256 mappings and 64 floors, what a decoder takes: a class with more is cut into
 * several such unions).  The PCM and the results are the same bit for bit.  Off (the default), every cut, call and byte is
 * what vorbispizza_multi.h describes.
 *
 * A header of its own: vorbispizza_multi.h, its structs and their bindings do not change with it.
 */
#ifndef VORBISPIZZA_MULTI_MIXED_H
#define VORBISPIZZA_MULTI_MIXED_H

#include <stdint.h>

#include "vorbispizza_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: sub-batches may hold streams of different setups.  Default 0.  The call takes the dispatcher's turn like a
 * vpzm_decode_library call and holds from the next one on.  VPZM_E_ARG for a null dispatcher. */
int vpzm_set_mixed_setups(vpzm_dispatcher *m, int32_t on);

typedef struct vpzm_call_counts {
    int64_t sub_batches;                 /* of the last vpzm_decode_library call, all groups */
    int64_t device_decoded_sub_batches;  /* ... those that were entropy-decoded on the device */
    int64_t mixed_sub_batches;           /* sub-batches whose members have two or more different setups */
    int64_t max_setups_per_sub_batch;
    int64_t decoders_created;            /* vpz_decoder_create calls of that call */
    int64_t reserved[3];
} vpzm_call_counts;

/* The counts of the last vpzm_decode_library call (zeros before the first, and for a call that returned an error), written
 * whatever the options are.
 * VPZM_E_ARG for a null argument. */
int vpzm_last_call_counts(vpzm_dispatcher *m, vpzm_call_counts *out);

#ifdef __cplusplus
}
#endif
#endif
