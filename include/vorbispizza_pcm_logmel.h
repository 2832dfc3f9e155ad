/*
 * vorbispizza_pcm_logmel.h -- windows of a mono device PCM array delivered as (log-)mel feature frames in device memory,
 * libvorbispizza_synth.so.
 *
 * vpz_pcm_resample (vorbispizza_pcm_resample.h) delivers every window at one rate, mixed down to mono.  A speech or audio model takes
 * log-mel frames of that: vpz_pcm_logmel is the stage behind it -- framing, Hann window, DFT, power, mel filterbank, log -- in one
 * launch, with no spectrogram in device memory.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).
 * Signal.  A descriptor is a vpz_pack_row over a MONO float32 device array: `src` the element offset of the window's first sample,
 * `samples` = L, `row` the destination row.  The call has one padded length F (`frames`): x[0..L) are the source samples, x[L..F) are
 * zeros; source elements at or behind src + L are not read.  x is extended by reflection at both ends without repeating the edge
 * sample: x[-i] = x[i] and x[F-1+i] = x[F-1-i] for 1 <= i <= n_fft/2 -- torch.stft(row, center=True, pad_mode="reflect") of a row
 * of the padded batch.
 * Frames.  Every row has T = 1 + floor(F / hop) frames; frame t covers x[t*hop - n_fft/2 + m], m = 0 .. n_fft-1.
 * Spectrum.  w[m] = 0.5 - 0.5 cos(2 pi m / n_fft) (the periodic Hann window);
 *     re[t][k] = sum_m x w[m] cos(2 pi m k / n_fft),  im[t][k] = sum_m x w[m] sin(2 pi m k / n_fft),  k = 0 .. n_fft/2,
 *     P = re^2 + im^2.
 * The angle is reduced as the integer (m*k mod n_fft) before the double-precision cos and sin; a coefficient w cos / w sin is rounded
 * once to float32.  A sum runs over m ascending, every step one fused multiply-add in float32.
 * Mel filterbank (torchaudio.functional.melscale_fbanks / librosa.filters.mel).  n_mels + 2 points evenly spaced on the mel scale
 * between f_min and f_max, mapped back to Hz as f_pts; bin frequencies f_k = k * sample_rate / n_fft;
 *     W[b][k] = max(0, min((f_k - f_pts[b]) / (f_pts[b+1] - f_pts[b]), (f_pts[b+2] - f_k) / (f_pts[b+2] - f_pts[b+1]))).
 *     VPZ_MEL_HTK:    mel = 2595 log10(1 + f/700).
 *     VPZ_MEL_SLANEY: mel = f / (200/3) below 1000 Hz, 15 + ln(f/1000) / (ln(6.4)/27) at and above it.
 *     VPZ_MEL_NORM_NONE: the weights as they are.  VPZ_MEL_NORM_SLANEY: multiplied by 2 / (f_pts[b+2] - f_pts[b]).
 * W is evaluated in double and rounded once to float32.  M[t][b] = sum_k W[b][k] P[t][k] over the band's live bins (W > 0), k
 * ascending.  A band with no bin under it is all zeros: allowed, not an error.
 * Output.  VPZ_MEL_POWER: M.  VPZ_MEL_LOG10: log10(max(M, floor)), floor > 0 (as float32) supplied by the caller.
 * Destination.  float32, dst[dst_rows][n_mels][T] (VPZ_MEL_BANDS_FIRST) or dst[dst_rows][T][n_mels] (VPZ_MEL_FRAMES_FIRST).  Every
 * element of a named row is written exactly once; rows that no descriptor names are not touched.  A samples = 0 descriptor reads
 * nothing and yields the SILENCE ROW: 0, or log10f(floor) (evaluated on the host, (float)log10((double)(float)floor)).
 * Limits.  n_fft even, 32 <= n_fft <= 1024; 1 <= hop <= n_fft; 1 <= n_mels <= 256; 0 <= f_min < f_max <= sample_rate / 2;
 * F >= n_fft/2 + 1; L <= F.
 *
 * A header of its own: vorbispizza_synth.h, the older vorbispizza_pcm_*.h, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_LOGMEL_H
#define VORBISPIZZA_PCM_LOGMEL_H

#include <stdint.h>

#include "vorbispizza_pcm_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_LOGMEL_MIN_NFFT 32
#define VPZ_LOGMEL_MAX_NFFT 1024
#define VPZ_LOGMEL_MAX_MELS 256

#define VPZ_MEL_HTK 0
#define VPZ_MEL_SLANEY 1
#define VPZ_MEL_NORM_NONE 0
#define VPZ_MEL_NORM_SLANEY 1
#define VPZ_MEL_POWER 0
#define VPZ_MEL_LOG10 1
#define VPZ_MEL_BANDS_FIRST 0
#define VPZ_MEL_FRAMES_FIRST 1

typedef struct vpz_logmel_spec {
    double sample_rate;  /* Hz, of the mono array */
    double f_min, f_max; /* 0 <= f_min < f_max <= sample_rate / 2 */
    double floor;        /* VPZ_MEL_LOG10: > 0 as float32; VPZ_MEL_POWER: not looked at */
    int32_t n_fft;       /* even, 32 .. 1024 */
    int32_t hop;         /* 1 .. n_fft */
    int32_t n_mels;      /* 1 .. 256 */
    int32_t mel_scale;   /* VPZ_MEL_HTK / VPZ_MEL_SLANEY */
    int32_t mel_norm;    /* VPZ_MEL_NORM_NONE / VPZ_MEL_NORM_SLANEY */
    int32_t output;      /* VPZ_MEL_POWER / VPZ_MEL_LOG10 */
    int32_t layout;      /* VPZ_MEL_BANDS_FIRST / VPZ_MEL_FRAMES_FIRST */
    int32_t reserved[9]; /* zero: room to grow */
} vpz_logmel_spec;

/* The DFT table as the kernel uses it, the window folded in, computed on the host in double and rounded once to float32; needs no
 * device.  With nb = n_fft/2 + 1 the table is [n_fft][2 * nb]: table[m * 2 * nb + k] = w[m] cos(2 pi (m*k mod n_fft) / n_fft) and
 * table[m * 2 * nb + nb + k] = w[m] sin(...), k = 0 .. nb-1.  table == null: nothing is written (the size is n_fft * 2 * nb floats).
 * VPZ_E_INVALID_ARG: n_fft outside the limits, capacity < 0.  VPZ_E_CAPACITY: table given and capacity < n_fft * 2 * nb. */
int vpz_logmel_dft_table(int32_t n_fft, float *table, int64_t capacity);

/* The mel filterbank of a spec (sample_rate, n_fft, n_mels, f_min, f_max, mel_scale, mel_norm; the other fields are not looked at but
 * must be inside their limits), computed in double and rounded once; needs no device.  Band b's live bins are first_bin[b] ..
 * first_bin[b] + n_bins[b] - 1 (n_bins[b] = 0, first_bin[b] = 0: no bin under it), their weights weights[o_b ..], o_b the sum of
 * n_bins in front of b.  first_bin and n_bins (when not null) have room for n_mels entries, weights (when not null) for `capacity`
 * floats; *total (when not null) is the sum of all n_bins -- a call with null outputs sizes the arrays.
 * VPZ_E_INVALID_ARG: spec null or outside the limits, capacity < 0.  VPZ_E_CAPACITY: weights given and capacity < *total. */
int vpz_mel_filterbank(const vpz_logmel_spec *spec, int32_t *first_bin, int32_t *n_bins, float *weights, int64_t capacity, int64_t *total);

/* Source: `src_elems` float32 elements of device memory, mono -- what vpz_pcm_resample writes with downmix 1 and a planar float32
 * layout.  `frames` is F.  dst_dev has dst_rows * n_mels * T float32 elements, T = 1 + frames / hop.  `rows` is host memory and is free
 * again when the call returns; the kernel runs asynchronously on the context's stream (vpz_context_synchronize completes it).  The DFT
 * table of an n_fft and the filterbank of a spec are built on first use and kept by the context.
 * VPZ_E_INVALID_ARG, with nothing launched: a null pointer; a spec outside the limits (reserved words not zero included); frames <
 * n_fft/2 + 1; n_rows < 0; dst_rows < 0; a descriptor whose samples exceed frames, whose source span [src, src + samples) leaves
 * [0, src_elems) or whose row is out of range or named twice; a pointer not aligned to float32; src_dev or dst_dev not device memory of
 * the context's device, or not inside one allocation over its whole extent. */
int vpz_pcm_logmel(vpz_context *ctx, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_logmel_spec *spec, int32_t n_rows,
                   const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_LOGMEL_H */
