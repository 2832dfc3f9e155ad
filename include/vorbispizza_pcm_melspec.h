/*
 * vorbispizza_pcm_melspec.h -- windows of a mono device PCM array delivered as (log-)mel spectrogram frames with transforms of 2048,
 * 4096 and 8192 samples, libvorbispizza_synth.so.
 *
 * vpz_pcm_logmel (vorbispizza_pcm_logmel.h) stops at n_fft = 1024: it takes the DFT as a matrix product, n_fft * (n_fft + 2) multiply-adds
 * a frame.  The mel front ends of music models (22.05, 44.1, 48 kHz) use n_fft = 2048 or 4096, a hop of 512 or 1024 and 128 bands:
 * vpz_pcm_melspec is the stage for those -- framing, Hann window, a real FFT in LDS, power, mel filterbank, log -- in one launch, with no
 * spectrogram in device memory.  The spec is vpz_logmel_spec, the same 96 bytes.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).  It is vorbispizza_pcm_logmel.h's, item for item, but for the
 * Spectrum and the Limits:
 * Signal.  A descriptor is a vpz_pack_row over a MONO float32 device array: `src` the element offset of the window's first sample,
 * `samples` = L, `row` the destination row.  The call has one padded length F (`frames`): x[0..L) are the source samples, x[L..F) are
 * zeros; source elements at or behind src + L are not read.  x is extended by reflection at both ends without repeating the edge
 * sample: x[-i] = x[i] and x[F-1+i] = x[F-1-i] for 1 <= i <= n_fft/2 -- torch.stft(row, center=True, pad_mode="reflect") of a row
 * of the padded batch.
 * Frames.  Every row has T = 1 + floor(F / hop) frames; frame t covers x[t*hop - n_fft/2 + m], m = 0 .. n_fft-1.
 * Window.  w[m] = 0.5 - 0.5 cos(2 pi m / n_fft) (the periodic Hann window), evaluated in double and rounded once to float32.
 * Spectrum.  With N = n_fft, H = N/2 and y[m] = fl(x[m] * w[m]) (one float32 product),
 *     X[k] = sum_m y[m] e^(-2 pi i m k / N),  re = Re X[k],  im = -Im X[k],  k = 0 .. H,    P = re^2 + im^2,
 * computed by THE NETWORK below in float32; a frame's values depend on that frame's N samples only, bit for bit -- no two frames share
 * a transform.  The value is not the ascending fused chain of vorbispizza_pcm_logmel.h; it is held to THE BOUND below.
 *   1. Packing.  z[j] = y[2j] + i y[2j+1], j = 0 .. H-1: the even and odd samples of ONE frame as one complex sequence.
 *   2. A complex FFT of H points, decimation in frequency, self-sorting (Stockham: every pass reads one array and writes the other, the
 *      result is in natural order).  A pass has a length n and a stride s with n * s = H; the first has n = H, s = 1.  While n >= 4 the
 *      pass is of radix 4: for p = 0 .. n/4-1, q = 0 .. s-1, with a, b, c, d = in[q + s (p + j n/4)], j = 0 .. 3,
 *          out[q + s (4p)]     =          (a + c) + (b + d)
 *          out[q + s (4p + 1)] = t[2ps]  * ((a - c) - i (b - d))
 *          out[q + s (4p + 2)] = t[4ps]  * ((a + c) - (b + d))
 *          out[q + s (4p + 3)] = t[6ps]  * ((a - c) + i (b - d))
 *      and then n /= 4, s *= 4.  A last pass with n = 2 (H = 2048 only) is of radix 2 without twiddles: out[q] = a + b, out[q + s] = a - b,
 *      a, b = in[q], in[q + s].  H = 1024: five radix-4 passes; 2048: five and the radix-2 pass; 4096: six.  No two steps are fused.
 *   3. The split pass.  For k = 0 .. H/2, with Z[H] = Z[0]:  E = (Z[k] + conj Z[H-k]) / 2,  O = -i (Z[k] - conj Z[H-k]) / 2,
 *          X[k] = E + t[k] O,    X[H-k] = conj(E - t[k] O).
 * t[k] = e^(-2 pi i k / N), k = 0 .. N-1: (cos, -sin) evaluated in double and rounded once to float32, exact on the axes.  Every complex
 * sum is two float32 sums.  A complex product t * v, t = (c, s'), is written  (fma(v.re, c, -(v.im * s')), fma(v.re, s', v.im * c)):
 * one rounded product and one fused multiply-add per component.  The halving is exact.
 * THE BOUND.  With u = 2^-24 and S = sum_m |x[m]| w[m] over the frame, re and im lie within d = K(n_fft) u S of the exact value:
 *     K(n_fft) = sqrt(2) * (5 r4 + r2 + 2) + 7,    (r4, r2) = (5, 0), (5, 1), (6, 0) at n_fft = 2048, 4096, 8192:   45.2, 46.6, 52.3.
 * Every input reaches an output along one path, and |Z[k] - exact| <= ((1 + e)^passes - 1) sum |z| <= ... S, e a pass's relative
 * perturbation of a path in the complex modulus: a complex sum u, a product 2u, a once-rounded twiddle u -- a radix-4 pass 2u + 3u, the
 * radix-2 pass u, the windowing 2u (w rounded, the product rounded).  The split pass combines Z[k] and Z[H-k] with coefficients whose
 * moduli add up to at most sqrt(2), and adds u |E| + 4u |O| + u |X| <= 6u S of its own; the last 1 covers every term of second order
 * (K^2 u < 2^-11).  The matrix kernel's constant is n_fft + 2.
 * Mel filterbank, Output, Destination: as in vorbispizza_pcm_logmel.h.  W[b][k] = max(0, min(up, down)) over n_mels + 2 points evenly
 * spaced on the mel scale (VPZ_MEL_HTK / VPZ_MEL_SLANEY, VPZ_MEL_NORM_NONE / VPZ_MEL_NORM_SLANEY), evaluated in double and rounded once;
 * M[t][b] = sum_k W[b][k] P[t][k] over the band's live bins, k ascending, every step one fused multiply-add; a band with no bin under
 * it is all zeros.  VPZ_MEL_POWER: M.  VPZ_MEL_LOG10: log10(max(M, floor)).  float32 dst[dst_rows][n_mels][T] (VPZ_MEL_BANDS_FIRST) or
 * dst[dst_rows][T][n_mels] (VPZ_MEL_FRAMES_FIRST); every element of a named row is written exactly once, rows that no descriptor names
 * are not touched.  A samples = 0 descriptor reads nothing and yields the SILENCE ROW: 0, or log10f(floor) (evaluated on the host,
 * (float)log10((double)(float)floor)).
 * Limits.  n_fft 2048, 4096 or 8192; 1 <= hop <= n_fft; 1 <= n_mels <= 256; 0 <= f_min < f_max <= sample_rate / 2; F >= n_fft/2 + 1;
 * L <= F.
 *
 * A header of its own: vorbispizza_pcm_logmel.h, its limits, vpz_pcm_logmel, vpz_mel_filterbank and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_MELSPEC_H
#define VORBISPIZZA_PCM_MELSPEC_H

#include <stdint.h>

#include "vorbispizza_pcm_logmel.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_MELSPEC_MIN_NFFT 2048
#define VPZ_MELSPEC_MAX_NFFT 8192
#define VPZ_MELSPEC_MAX_MELS 256

/* The table as the kernel reads it, computed on the host in double and rounded once to float32; needs no device.  3 * n_fft floats:
 * table[m] = w[m], m = 0 .. n_fft-1, then table[n_fft + 2k] = cos(2 pi k / n_fft), table[n_fft + 2k + 1] = -sin(2 pi k / n_fft),
 * k = 0 .. n_fft-1 (t[k] of the definition).  table == null: nothing is written (the size is 3 * n_fft floats).
 * VPZ_E_INVALID_ARG: n_fft not 2048, 4096 or 8192, capacity < 0.  VPZ_E_CAPACITY: table given and capacity < 3 * n_fft. */
int vpz_melspec_twiddles(int32_t n_fft, float *table, int64_t capacity);

/* vpz_mel_filterbank (vorbispizza_pcm_logmel.h) under this header's limits: the same outputs, the same sizing calls, the same statuses;
 * n_fft is 2048, 4096 or 8192.  (vpz_mel_filterbank itself keeps refusing an n_fft above 1024.) */
int vpz_melspec_filterbank(const vpz_logmel_spec *spec, int32_t *first_bin, int32_t *n_bins, float *weights, int64_t capacity, int64_t *total);

/* Source: `src_elems` float32 elements of device memory, mono -- what vpz_pcm_resample writes with downmix 1 and a planar float32
 * layout.  `frames` is F.  dst_dev has dst_rows * n_mels * T float32 elements, T = 1 + frames / hop.  `rows` is host memory and is free
 * again when the call returns; the kernel runs asynchronously on the context's stream (vpz_context_synchronize completes it).  The
 * table of an n_fft and the filterbank of a spec are built on first use and kept by the context.
 * VPZ_E_INVALID_ARG, with nothing launched: a null pointer; a spec outside the limits (reserved words not zero included); frames <
 * n_fft/2 + 1; n_rows < 0; dst_rows < 0; a descriptor whose samples exceed frames, whose source span [src, src + samples) leaves
 * [0, src_elems) or whose row is out of range or named twice; a pointer not aligned to float32; src_dev or dst_dev not device memory of
 * the context's device, or not inside one allocation over its whole extent. */
int vpz_pcm_melspec(vpz_context *ctx, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_logmel_spec *spec, int32_t n_rows,
                    const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_MELSPEC_H */
