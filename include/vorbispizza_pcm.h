/*
 * vorbispizza_pcm.h -- bringing pieces of a device PCM array to the host without a synchronise per piece,
 * libvorbispizza_synth.so.
 *
 * A batched synth call into device memory leaves every stream's PCM in an area of its own.  vpz_memcpy_d2h waits for every
 * copy; a host that wants many small pieces -- a window out of every area -- queues them with vpz_pcm_download and waits once.
 *
 * A header of its own: vorbispizza_synth.h, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_H
#define VORBISPIZZA_PCM_H

#include <stdint.h>

#include "vorbispizza_synth.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Queues the copy of `bytes` bytes of device memory to host memory (page-locked or not) on the context's stream and returns:
 * vpz_context_synchronize completes it (vpz_memcpy_d2h is the same copy with the synchronise inside). */
int vpz_pcm_download(vpz_context *ctx, void *host_dst, const void *dev_src, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_H */
