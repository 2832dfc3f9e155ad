/*
 * vorbispizza_pcm_stft.h -- windows of a float32 device PCM array delivered as short-time Fourier spectrograms, one row per descriptor,
 * with transforms of 512, 1024, 2048, 4096 and 8192 samples, libvorbispizza_synth.so.
 *
 * The feature stages of the family (vpz_pcm_logmel, vpz_pcm_melspec, vpz_pcm_fbank, vpz_pcm_mfcc) reduce a short-time spectrum to a few
 * dozen mel bands inside the kernel and are mono.  vpz_pcm_stft is the building block under them: it keeps the spectrum -- complex, as
 * magnitudes or as power -- and stores it, for the models that take it as it is (source separation and enhancement: the complex STFT of
 * every channel; vocoders: linear magnitudes; a filterbank of the caller's own: power).  The stage has no notion of channels: a channel
 * of a planar array (what vpz_pcm_resample writes with downmix 0 and a planar float32 layout) is a row like any other.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).  Signal and Frames are vorbispizza_pcm_melspec.h's, word for word.
 * Signal.  A descriptor is a vpz_pack_row over a float32 device array: `src` the element offset of the window's first sample, `samples`
 * = L consecutive elements, `row` the destination row.  The call has one padded length F (`frames`): x[0..L) are the source samples,
 * x[L..F) are zeros; source elements at or behind src + L are not read.  x is extended by reflection at both ends without repeating the
 * edge sample: x[-i] = x[i] and x[F-1+i] = x[F-1-i] for 1 <= i <= n_fft/2.
 * Frames.  Every row has T = 1 + floor(F / hop) frames; frame t covers x[t*hop - n_fft/2 + m], m = 0 .. n_fft-1 -- torch.stft(row,
 * n_fft, hop, win_length, window, center=True, pad_mode="reflect", normalized=False, onesided=True) of a row of the padded batch.
 * Window.  With left = floor((n_fft - win_length) / 2):  w[m] = g[m - left] for left <= m < left + win_length, 0 elsewhere;
 *     g[j] = 0.5 - 0.5 cos(2 pi j / win_length) (VPZ_STFT_HANN),   g[j] = 0.54 - 0.46 cos(2 pi j / win_length) (VPZ_STFT_HAMMING),
 * the periodic windows, evaluated in double and rounded once to float32: torch.stft's centring of torch.hann_window(win_length) /
 * torch.hamming_window(win_length).
 * Spectrum.  With N = n_fft, H = N/2 and y[m] = fl(x[m] * w[m]) (one float32 product),
 *     X[k] = sum_m y[m] e^(-2 pi i m k / N),   k = 0 .. H,
 * computed by THE NETWORK of vorbispizza_pcm_melspec.h in float32 -- packing z[j] = y[2j] + i y[2j+1]; the radix-4 Stockham passes of
 * the H-point transform, decimation in frequency, the first with length n = H and stride s = 1; the radix-2 pass without twiddles where
 * log2 H is odd; the split pass X[k] = E + t[k] O, X[H-k] = conj(E - t[k] O) -- stated there for H = 1024 .. 4096 and taken here for
 * H = 256 .. 4096 as it stands:
 *     n_fft   512    1024       2048   4096       8192
 *     passes  4 r4   4 r4 + r2  5 r4   5 r4 + r2  6 r4
 * with the same twiddles t[k] = e^(-2 pi i k / N) = (cos, -sin), evaluated in double and rounded once to float32, exact on the axes, the
 * complex product written the same way ((fma(v.re, c, -(v.im * s')), fma(v.re, s', v.im * c)) for t = (c, s')), every complex sum two
 * float32 sums, the halving exact, and no two steps fused.  A frame's values depend on that frame's N samples only, bit for bit: no two
 * frames share a transform, and neither the tile a frame falls into nor its place in it changes a bit.
 * Output.  VPZ_STFT_COMPLEX: the pair (Re X[k], Im X[k]) as two float32 -- torch.view_as_real(torch.stft(..., return_complex=True)).
 * (Im X itself: vorbispizza_pcm_melspec.h's `im` is -Im X, which its power does not see.)  VPZ_STFT_POWER: P = fma(re, re, im * im).
 * VPZ_STFT_MAGNITUDE: the correctly rounded float32 square root of that P.
 * Destination.  With n_freq = N/2 + 1: float32 dst[dst_rows][n_freq][T] (VPZ_STFT_BINS_FIRST, torch's order) or dst[dst_rows][T][n_freq]
 * (VPZ_STFT_FRAMES_FIRST); VPZ_STFT_COMPLEX adds a last dimension of 2.  Every element of a named row is written exactly once, rows
 * that no descriptor names are not touched.  A samples = 0 descriptor reads nothing and yields zeros.
 * THE BOUND.  With u = 2^-24 and S = sum_m |x[m]| w[m] over the frame, Re and Im lie within d = K(n_fft) u S of the exact value:
 *     K(n_fft) = sqrt(2) * (5 r4 + r2 + 2) + 7:    38.1, 39.5, 45.2, 46.6, 52.3  at n_fft = 512 .. 8192.
 * It is vorbispizza_pcm_melspec.h's derivation, which nothing ties to a size: every input reaches an output along one path, and
 * |Z[k] - exact| <= ((1 + e)^passes - 1) sum |z|, e a pass's relative perturbation of a path in the complex modulus -- a complex sum
 * u, a product 2u, a once-rounded twiddle u: a radix-4 pass 2u + 3u, the radix-2 pass u, the windowing 2u (w rounded, the product
 * rounded).  The split pass combines Z[k] and Z[H-k] with coefficients whose moduli add up to at most sqrt(2), and adds
 * u |E| + 4u |O| + u |X| <= 6u S of its own; the last 1 covers every term of second order (K^2 u < 2^-11).
 *   Power.  |P - exact| <= e_P = 2 |re| d + 2 |im| d + 2 d^2 + 3u P: (re + a)^2 + (im + b)^2 with |a|, |b| <= d, then one rounded
 *   product, one fused multiply-add and the second order.
 *   Magnitude.  |M - |X|| <= e = sqrt(2) d + 3u |X|.  The reverse triangle inequality bounds the distance of the moduli by the modulus
 *   of the distance, at most sqrt(2) d over both components.  The two roundings under the root (relative 2u in P) are halved by it, the
 *   root adds one rounding of its own: 2u; the third u covers the second order.
 * Limits.  n_fft 512, 1024, 2048, 4096 or 8192; 1 <= hop <= n_fft; 2 <= win_length <= n_fft; F >= n_fft/2 + 1; L <= F; reserved words
 * zero.
 *
 * A header of its own: the older headers, their structs and their bindings do not change with it.  Conventions are those of
 * vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_STFT_H
#define VORBISPIZZA_PCM_STFT_H

#include <stdint.h>

#include "vorbispizza_pcm_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_STFT_MIN_NFFT 512
#define VPZ_STFT_MAX_NFFT 8192

#define VPZ_STFT_HANN 0
#define VPZ_STFT_HAMMING 1

#define VPZ_STFT_COMPLEX 0
#define VPZ_STFT_MAGNITUDE 1
#define VPZ_STFT_POWER 2

#define VPZ_STFT_BINS_FIRST 0
#define VPZ_STFT_FRAMES_FIRST 1

typedef struct vpz_stft_spec {
    int32_t n_fft;        /* 512, 1024, 2048, 4096, 8192 */
    int32_t hop;          /* 1 .. n_fft */
    int32_t win_length;   /* 2 .. n_fft */
    int32_t window;       /* VPZ_STFT_HANN / VPZ_STFT_HAMMING (periodic, over win_length) */
    int32_t output;       /* VPZ_STFT_COMPLEX / VPZ_STFT_MAGNITUDE / VPZ_STFT_POWER */
    int32_t layout;       /* VPZ_STFT_BINS_FIRST / VPZ_STFT_FRAMES_FIRST */
    int32_t reserved[10]; /* zero */
} vpz_stft_spec;          /* 64 bytes */

/* The table as the kernel reads it, computed on the host in double and rounded once to float32; needs no device.  3 * n_fft floats:
 * table[m] = w[m], m = 0 .. n_fft-1, then table[n_fft + 2k] = cos(2 pi k / n_fft), table[n_fft + 2k + 1] = -sin(2 pi k / n_fft),
 * k = 0 .. n_fft-1 (t[k] of the definition).  table == null: nothing is written (the size is 3 * n_fft floats).
 * VPZ_E_INVALID_ARG: n_fft, win_length or window outside the limits, capacity < 0.  VPZ_E_CAPACITY: table given and capacity <
 * 3 * n_fft. */
int vpz_stft_table(int32_t n_fft, int32_t win_length, int32_t window, float *table, int64_t capacity);

/* Source: `src_elems` float32 elements of device memory.  `frames` is F.  dst_dev has dst_rows * n_freq * T float32 elements (twice as
 * many for VPZ_STFT_COMPLEX), T = 1 + frames / hop.  `rows` is host memory and is free again when the call returns; the kernel runs
 * asynchronously on the context's stream (vpz_context_synchronize completes it).  The table of an (n_fft, win_length, window) is built
 * on first use and kept by the context.
 * VPZ_E_INVALID_ARG, with nothing launched: a null pointer; a spec outside the limits (reserved words not zero included); frames <
 * n_fft/2 + 1; n_rows < 0; dst_rows < 0; a row count and T that do not fit one launch; a descriptor whose samples exceed frames, whose
 * source span [src, src + samples) leaves [0, src_elems) or whose row is out of range or named twice; a pointer not aligned to float32 (dst_dev of a VPZ_STFT_COMPLEX call: to a pair of them, which the kernel stores as one);
 * src_dev or dst_dev not device memory of the context's device, or not inside one allocation over its whole extent. */
int vpz_pcm_stft(vpz_context *ctx, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_stft_spec *spec, int32_t n_rows,
                 const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_STFT_H */
