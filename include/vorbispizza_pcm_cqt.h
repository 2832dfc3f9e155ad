/*
 * vorbispizza_pcm_cqt.h -- windows of a float32 device PCM array delivered as constant-Q (or variable-Q) spectrograms, one row per
 * descriptor: geometrically spaced bins, one analysis window per bin, libvorbispizza_synth.so.
 *
 * The other feature stages of the family take one window length for all bins (vpz_pcm_stft and the mel stages above it).  Where the
 * frequency axis must be pitch -- transcription, chord and key models, pitch trackers, chroma -- every bin has its own window, as long
 * as its frequency is low: 11 339 samples at 32.70 Hz and 22.05 kHz.  vpz_pcm_cqt computes that transform directly, as a framed matrix
 * product whose dead ranges are skipped.  The stage has no notion of channels: a channel of a planar array is a row like any other.
 *
 * Out of scope: chroma (the caller folds octaves: cqt.view(n, C, -1, 12, T).sum(2) at 12 bins per octave); the recursive
 * octave-downsampling transform of librosa, and bit parity with any library; the inverse transform; dB scaling and per-bin loudness
 * weighting; trainable kernels.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).
 * Signal.  A descriptor is a vpz_pack_row over a float32 device array: `src` the element offset of the window's first sample, `samples`
 * = L consecutive elements, `row` the destination row.  The call has one padded length F (`frames`): x[0..L) are the source samples,
 * x[L..F) are zeros; source elements at or behind src + L are not read.
 * Extension.  VPZ_CQT_PAD_REFLECT: x[-i] = x[i] and x[F-1+i] = x[F-1-i] for 1 <= i <= floor(N_0 / 2), the centring of the other stages;
 * it requires F >= floor(N_0 / 2) + 1.  Beyond the reflection x is zero (one sample can lie there: x[F + floor(N_0 / 2)], which the last
 * frame of a bin as long as an odd N_0 reads when hop divides F).  VPZ_CQT_PAD_ZERO: x is zero outside [0, F); F >= 1 is all it asks: the mode for clips shorter
 * than the lowest bin's window.
 * Bins.  With B = bins_per_octave, all in double:
 *     f_k = f_min * 2^(k / B), k = 0 .. n_bins-1;   alpha = 2^(1/B) - 1;   Q = filter_scale / alpha;
 *     N_k = ceil(Q * sample_rate / (f_k + gamma / alpha)).
 * 2^x is the C library's exp2 of the double x.  gamma = 0 is the constant-Q transform, gamma > 0 the variable-Q one.  N_0 is the longest
 * length.
 * Frames.  Every row has T = 1 + floor(F / hop) frames; frame t is centred on sample t * hop: bin k of frame t reads
 * x[t*hop - floor(N_k / 2) + j], j = 0 .. N_k-1.
 * Kernel of a bin.  g_k[j] = 0.5 - 0.5 cos(2 pi j / N_k) (VPZ_CQT_HANN) or 0.54 - 0.46 cos(2 pi j / N_k) (VPZ_CQT_HAMMING), the periodic
 * windows over N_k; G_k = sum_j g_k[j], summed in ascending j.  s_k = 1 / G_k (VPZ_CQT_SCALE_NONE: a unit cosine at f_k reads 0.5) or
 * s_k = sqrt(N_k) / G_k (VPZ_CQT_SCALE_SQRT_LENGTH: white noise reads flat across the bins).  With phi = 2 pi f_k (j - floor(N_k / 2)) /
 * sample_rate:
 *     hr_k[j] = (s_k g_k[j]) cos(phi),     hi_k[j] = -((s_k g_k[j]) sin(phi)):
 * the phase is referred to the frame's centre sample.  Every coefficient is evaluated in double and rounded once to float32.
 * Sums.  Re X[t][k] = sum_j x hr_k[j] and Im X[t][k] = sum_j x hi_k[j], each ONE float32 chain over j ascending, from +0, every step one
 * fused multiply-add: acc = fma(x, h, acc).  This is what the float32 matrix instruction computes, bit for bit.  A step whose coefficient
 * is zero leaves a FINITE chain unchanged, so a kernel may be padded with zeros and the dead range of a column skipped without changing
 * a bit.  This holds for finite input only: an infinity or a NaN among the samples that a zero coefficient meets yields NaN where the
 * definition has none, and the results of a row that holds one are not specified beyond being that row's own.
 * A value's bits depend on (the row's samples, t, k) alone: not on the tile, the chunk, the row's place in the launch or the place of the
 * window in the source array.
 * Output.  VPZ_CQT_COMPLEX: the pair (Re X, Im X) as two float32.  VPZ_CQT_POWER: P = fma(re, re, im * im).  VPZ_CQT_MAGNITUDE: the
 * correctly rounded float32 square root of that P.
 * Destination.  float32 dst[dst_rows][n_bins][T] (VPZ_CQT_BINS_FIRST) or dst[dst_rows][T][n_bins] (VPZ_CQT_FRAMES_FIRST); VPZ_CQT_COMPLEX
 * adds a last dimension of 2.  Every element of a named row is written exactly once, rows that no descriptor names are not touched.  A
 * samples = 0 descriptor reads nothing and yields zeros.
 * Limits.  sample_rate > 0; f_min > 0; f_(n_bins-1) <= sample_rate / 2; n_bins 1 .. 512; bins_per_octave 1 .. 96; filter_scale > 0;
 * gamma >= 0; N_k >= 2 for every k and N_0 <= 65 536; hop 1 .. 2048; L <= F; reserved words zero.  (f_min 32.70 Hz: N_0 = 11 339 at
 * 22.05 kHz and B = 12, 22 678 at 44.1 kHz, 34 683 at 22.05 kHz and B = 36, 46 021 at 44.1 kHz and B = 24; 69 365 at 44.1 kHz and B = 36
 * is refused: that caller resamples.)
 * THE BOUND.  With u = 2^-24 and S_k = sum_j |x[j]| |h_k[j]| over the frame (h the exact coefficient), Re and Im lie within
 *     d = (N_k + 2) u S_k
 * of the exact value.  Derivation.  The stored coefficient is h' = h (1 + e), |e| <= u: rounded once.  A chain of n fused multiply-adds
 * from zero is a recursive inner product whose products are not rounded: the term of step j passes through the roundings of steps j .. n,
 * at most n of them, each a factor (1 + e_i) with |e_i| <= u, so |computed - sum_j x h'| <= gamma_n sum_j |x| |h'| with gamma_n =
 * n u / (1 - n u), the standard bound; Jeannerod and Rump (Improved error bounds for inner products in floating-point arithmetic, SIAM
 * J. Matrix Anal. Appl. 34, 2013) show that n u itself holds in its place, without the terms of higher order and for every n.  Then
 *     |computed - exact| <= n u sum |x| |h'| + sum |x| |h' - h| <= n u (1 + u) S_k + u S_k = (n + 1 + n u) u S_k <= (n + 2) u S_k
 * with n = N_k, as N_k u <= 2^-8 inside the limits (N_k <= 65 536): that is what covers the second order.  Zero coefficients that pad a
 * kernel add no term and no rounding.
 *   Power.  |P - exact| <= e_P = 2 |re| d + 2 |im| d + 2 d^2 + 3u P: (re + a)^2 + (im + b)^2 with |a|, |b| <= d, then one rounded
 *   product, one fused multiply-add and the second order.
 *   Magnitude.  |M - |X|| <= e = sqrt(2) d + 3u |X|.  The reverse triangle inequality bounds the distance of the moduli by the modulus
 *   of the distance, at most sqrt(2) d over both components.  The two roundings under the root (relative 2u in P) are halved by it, the
 *   root adds one rounding of its own: 2u; the third u covers the second order.
 * The bound is loose -- it takes every rounding at its worst and with one sign -- and catches gross errors only; the sharp statement is
 * the chain above, which a float32 restatement reproduces bit for bit (tests/cqt_truth.py).
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.  Conventions are those of
 * vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_CQT_H
#define VORBISPIZZA_PCM_CQT_H

#include <stdint.h>

#include "vorbispizza_pcm_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_CQT_MAX_BINS 512
#define VPZ_CQT_MAX_BINS_PER_OCTAVE 96
#define VPZ_CQT_MAX_LENGTH 65536
#define VPZ_CQT_MAX_HOP 2048

#define VPZ_CQT_HANN 0
#define VPZ_CQT_HAMMING 1

#define VPZ_CQT_SCALE_NONE 0
#define VPZ_CQT_SCALE_SQRT_LENGTH 1

#define VPZ_CQT_PAD_REFLECT 0
#define VPZ_CQT_PAD_ZERO 1

#define VPZ_CQT_COMPLEX 0
#define VPZ_CQT_MAGNITUDE 1
#define VPZ_CQT_POWER 2

#define VPZ_CQT_BINS_FIRST 0
#define VPZ_CQT_FRAMES_FIRST 1

typedef struct vpz_cqt_spec {
    double sample_rate;      /* > 0 */
    double f_min;            /* > 0: f_0 */
    double filter_scale;     /* > 0 */
    double gamma;            /* >= 0; 0: constant Q */
    int32_t n_bins;          /* 1 .. 512 */
    int32_t bins_per_octave; /* 1 .. 96 */
    int32_t hop;             /* 1 .. 2048 */
    int32_t window;          /* VPZ_CQT_HANN / VPZ_CQT_HAMMING (periodic, over N_k) */
    int32_t scale;           /* VPZ_CQT_SCALE_NONE / VPZ_CQT_SCALE_SQRT_LENGTH */
    int32_t pad;             /* VPZ_CQT_PAD_REFLECT / VPZ_CQT_PAD_ZERO */
    int32_t output;          /* VPZ_CQT_COMPLEX / VPZ_CQT_MAGNITUDE / VPZ_CQT_POWER */
    int32_t layout;          /* VPZ_CQT_BINS_FIRST / VPZ_CQT_FRAMES_FIRST */
    int32_t reserved[8];     /* zero */
} vpz_cqt_spec;              /* 96 bytes */

/* f_k and N_k of a spec; needs no device.  `freqs` and `lengths` have room for `capacity` values each and receive n_bins; either may be
 * null and is then not written (both null: the call says whether the spec lies inside the limits, and the arrays' size is the spec's
 * n_bins).  VPZ_E_INVALID_ARG: a null spec, a spec outside the limits (every field, reserved words included), capacity < 0.
 * VPZ_E_CAPACITY: an array given and capacity < n_bins. */
int vpz_cqt_bins(const vpz_cqt_spec *spec, double *freqs, int32_t *lengths, int32_t capacity);

/* Bin k's coefficients as the kernel multiplies them, computed on the host in double and rounded once to float32; needs no device.
 * 2 * N_k floats: table[j] = hr_k[j], table[N_k + j] = hi_k[j].  *length, where given, receives N_k.  table == null: nothing is written
 * (the size is 2 * N_k floats).  VPZ_E_INVALID_ARG: a null spec, a spec outside the limits, k outside 0 .. n_bins-1, capacity < 0.
 * VPZ_E_CAPACITY: table given and capacity < 2 * N_k.  (How the device holds the kernels is the launch's business.) */
int vpz_cqt_kernel(const vpz_cqt_spec *spec, int32_t k, float *table, int64_t capacity, int32_t *length);

/* Source: `src_elems` float32 elements of device memory.  `frames` is F.  dst_dev has dst_rows * n_bins * T float32 elements (twice as
 * many for VPZ_CQT_COMPLEX), T = 1 + frames / hop.  `rows` is host memory and is free again when the call returns; the kernel runs
 * asynchronously on the context's stream (vpz_context_synchronize completes it).  The table of a spec is built on first use and kept by
 * the context, under the fields that shape it: all but hop, output, layout and pad.
 * VPZ_E_INVALID_ARG, with nothing launched: a null pointer; a spec outside the limits (reserved words not zero included); frames < 1;
 * VPZ_CQT_PAD_REFLECT and frames < floor(N_0 / 2) + 1; n_rows < 0; dst_rows < 0; a row count and T that do not fit one launch; a
 * descriptor whose samples exceed frames, whose source span [src, src + samples) leaves [0, src_elems) or whose row is out of range or
 * named twice; a pointer not aligned to float32 (dst_dev of a VPZ_CQT_COMPLEX call: to a pair of them, which the kernel stores as one);
 * src_dev or dst_dev not device memory of the context's device, or not inside one allocation over its whole extent. */
int vpz_pcm_cqt(vpz_context *ctx, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_cqt_spec *spec, int32_t n_rows,
                const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_CQT_H */
