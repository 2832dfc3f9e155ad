/*
 * vorbispizza_pcm_fbank.h -- windows of a mono device PCM array delivered as Kaldi filterbank feature frames in device memory,
 * libvorbispizza_synth.so.
 *
 * vpz_pcm_logmel (vorbispizza_pcm_logmel.h) is the Whisper-style front end.  The other one speech models use is the Kaldi filterbank --
 * torchaudio.compliance.kaldi.fbank, kaldi-native-fbank, the input of WeNet, icefall / k2 and ESPnet recipes --, which no vpz_logmel_spec
 * expresses: frames are not centred, every frame has its mean removed and is pre-emphasised on its own, the window is shorter than the
 * transform, the mel triangles are linear in mel and the log is natural.  vpz_pcm_fbank is that front end in one launch, with neither
 * the framed copy of the batch nor a spectrogram in device memory.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).
 * Signal.  A descriptor is a vpz_pack_row over a MONO float32 device array: `src` the element offset of the window's first sample,
 * `samples` = L, `row` the destination row.  The call has one padded length F (`frames`).  Source elements at or behind src + L are
 * never read.
 * Frames (Kaldi's snip_edges).  The tensor has T = 1 + (F - win) / hop frames per row (integer division; F >= win).  A row has
 * T_L = 0 real frames if L < win, else T_L = 1 + (L - win) / hop.  Frame t < T_L covers x[t*hop + m], m = 0 .. win-1: every one of its
 * samples is a real sample -- nothing is reflected, nothing is extended by zeros.  Frames t >= T_L hold `pad_value` (as float32) in every
 * band; a samples = 0 descriptor yields a row of pad_value and reads nothing.
 * Per frame, in this order:
 *   1. y[m] = scale * x[m]                      (32768 for recipes that expect 16-bit amplitudes)
 *   2. remove_dc: y[m] -= mean(y), the mean over the frame's win samples
 *   3. pre-emphasis, c in [0, 1]: z[0] = y[0] - c y[0], z[m] = y[m] - c y[m-1]
 *   4. the window w over win points, symmetric (denominator win - 1):
 *        VPZ_FBANK_HANNING  0.5 - 0.5 cos(2 pi m / (win-1))
 *        VPZ_FBANK_HAMMING  0.54 - 0.46 cos(2 pi m / (win-1))
 *        VPZ_FBANK_POVEY    the Hanning window to the power 0.85
 *   5. zero-padded to n_fft:  re[k] = sum_m z[m] w[m] cos(2 pi m k / n_fft),  im[k] = sum_m z[m] w[m] sin(2 pi m k / n_fft),
 *      k = 0 .. n_fft/2 - 1;  P[k] = re^2 + im^2.  The Nyquist bin has weight 0 in every band and is not computed.
 * Mel bank (Kaldi's MelBanks; the numbers of torchaudio's get_mel_banks without VTLN).  mel(f) = 1127 ln(1 + f/700); nyquist =
 * sample_rate / 2; high = high_freq > 0 ? high_freq : nyquist + high_freq; 0 <= low_freq < high <= nyquist;
 * d = (mel(high) - mel(low_freq)) / (n_mels + 1); band b has left = mel(low_freq) + b d, centre = left + d, right = left + 2 d;
 *     W[b][k] = max(0, min((mel(f_k) - left) / d, (right - mel(f_k)) / d)),   f_k = k * sample_rate / n_fft.
 * W is evaluated in double and rounded once to float32.  M[b] = sum_k W[b][k] P[k] over the band's live bins (W > 0; they are
 * consecutive), k ascending.  A band with no bin under it is all zeros: allowed, not an error.
 * Output.  VPZ_FBANK_POWER: M.  VPZ_FBANK_LOG: ln(max(M, floor)), floor > 0 as float32 (Kaldi's is FLT_EPSILON).
 * Destination.  float32, dst[dst_rows][T][n_mels] (VPZ_FBANK_FRAMES_FIRST, Kaldi's own order) or dst[dst_rows][n_mels][T]
 * (VPZ_FBANK_BANDS_FIRST).  Every element of a named row is written exactly once; rows that no descriptor names are not touched.
 * Float32 evaluation.  Steps 1, 3, 4 and 5 are linear and local in the frame: they are folded, in double, into one table B[m][k] -- the
 * angle reduced as the integer (m*k mod n_fft) before cos and sin --, rounded once to float32, and
 *     re[k] = sum_m (x[m] - mu) B[m][k],   m ascending, every step one fused multiply-add in float32 (im likewise).
 * The mean is NOT folded: a frame whose DC dwarfs its signal would cancel in the accumulators.  mu is one float32 value per frame,
 * subtracted from the sample (one float32 rounding) before the multiply-add:
 *     mu = ((s_0 + s_1) + (s_2 + s_3)) / win,   s_q = x[q] + x[q+4] + x[q+8] + ..., m ascending,
 * every addition and the division rounded to float32.  With remove_dc = 0, mu = 0 and nothing is subtracted.  A frame's bits depend on
 * its own win samples and the spec alone.  A sample that is not finite (+-Inf, NaN) makes exactly the frames that cover it not finite
 * (Inf or NaN), in every band that has a bin; every other frame, and every other row, is the same bits as without it.
 * Limits.  n_fft even, 32 <= n_fft <= 1024 (no power of two needed); 2 <= win <= n_fft (odd lengths allowed); 1 <= hop <= win;
 * 1 <= n_mels <= 256; L <= F; preemphasis in [0, 1]; scale finite and not 0 as float32; pad_value finite as float32; reserved words zero.
 * NOT PART OF IT: dither, VTLN, use_energy / raw_energy, subtract_mean across frames, htk_compat, and magnitude instead of power.
 *
 * A header of its own: vorbispizza_synth.h, the older vorbispizza_pcm_*.h, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_FBANK_H
#define VORBISPIZZA_PCM_FBANK_H

#include <stdint.h>

#include "vorbispizza_pcm_pack.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_FBANK_MIN_NFFT 32
#define VPZ_FBANK_MAX_NFFT 1024
#define VPZ_FBANK_MAX_MELS 256

#define VPZ_FBANK_HANNING 0
#define VPZ_FBANK_HAMMING 1
#define VPZ_FBANK_POVEY 2
#define VPZ_FBANK_POWER 0
#define VPZ_FBANK_LOG 1
#define VPZ_FBANK_BANDS_FIRST 0
#define VPZ_FBANK_FRAMES_FIRST 1

/* sizeof(vpz_fbank_spec) == 128: 7 doubles, 8 + 10 int32 */
typedef struct vpz_fbank_spec {
    double sample_rate;   /* Hz, of the mono array */
    double low_freq;      /* 0 <= low_freq < high */
    double high_freq;     /* > 0: high itself; <= 0: an offset from sample_rate / 2 */
    double preemphasis;   /* 0 .. 1 */
    double scale;         /* finite, not 0 (as float32) */
    double floor;         /* VPZ_FBANK_LOG: > 0 as float32; VPZ_FBANK_POWER: not looked at */
    double pad_value;     /* what the frames behind a row's real ones hold; finite as float32 */
    int32_t win;          /* 2 .. n_fft */
    int32_t hop;          /* 1 .. win */
    int32_t n_fft;        /* even, 32 .. 1024 */
    int32_t n_mels;       /* 1 .. 256 */
    int32_t window;       /* VPZ_FBANK_HANNING / VPZ_FBANK_HAMMING / VPZ_FBANK_POVEY */
    int32_t remove_dc;    /* 0 / 1 */
    int32_t output;       /* VPZ_FBANK_POWER / VPZ_FBANK_LOG */
    int32_t layout;       /* VPZ_FBANK_BANDS_FIRST / VPZ_FBANK_FRAMES_FIRST */
    int32_t reserved[10]; /* zero: room to grow */
} vpz_fbank_spec;

/* The folded table B of a spec (win, n_fft, window, preemphasis, scale; the other fields must be inside their limits), computed on the
 * host in double and rounded once to float32; needs no device.  With nb = n_fft / 2 the table is [win][2 * nb]: table[m * 2 * nb + k]
 * the coefficient of x[m] - mu in re[k], table[m * 2 * nb + nb + k] in im[k], k = 0 .. nb-1.  table == null: nothing is written (the size
 * is win * 2 * nb floats).
 * VPZ_E_INVALID_ARG: spec null or outside the limits, capacity < 0.  VPZ_E_CAPACITY: table given and capacity < win * 2 * nb. */
int vpz_fbank_table(const vpz_fbank_spec *spec, float *table, int64_t capacity);

/* The mel bank of a spec (sample_rate, n_fft, n_mels, low_freq, high_freq; the other fields must be inside their limits), computed in
 * double and rounded once; needs no device.  Band b's live bins are first_bin[b] .. first_bin[b] + n_bins[b] - 1 (n_bins[b] = 0,
 * first_bin[b] = 0: no bin under it), their weights weights[o_b ..], o_b the sum of n_bins in front of b.  first_bin and n_bins (when not
 * null) have room for n_mels entries, weights (when not null) for `capacity` floats; *total (when not null) is the sum of all n_bins -- a
 * call with null outputs sizes the arrays.
 * VPZ_E_INVALID_ARG: spec null or outside the limits, capacity < 0.  VPZ_E_CAPACITY: weights given and capacity < *total. */
int vpz_fbank_filterbank(const vpz_fbank_spec *spec, int32_t *first_bin, int32_t *n_bins, float *weights, int64_t capacity, int64_t *total);

/* Source: `src_elems` float32 elements of device memory, mono -- what vpz_pcm_resample writes with downmix 1 and a planar float32
 * layout.  `frames` is F.  dst_dev has dst_rows * T * n_mels float32 elements, T = 1 + (frames - win) / hop.  `rows` is host memory and
 * is free again when the call returns; the kernel runs asynchronously on the context's stream (vpz_context_synchronize completes it).
 * The folded table and the mel bank of a spec are built on first use and kept by the context.
 * VPZ_E_INVALID_ARG, with nothing launched: a null pointer; a spec outside the limits (reserved words not zero included); frames < win;
 * n_rows < 0; dst_rows < 0; a descriptor whose samples exceed frames, whose source span [src, src + samples) leaves [0, src_elems) or
 * whose row is out of range or named twice; a pointer not aligned to float32; src_dev or dst_dev not device memory of the context's
 * device, or not inside one allocation over its whole extent. */
int vpz_pcm_fbank(vpz_context *ctx, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_fbank_spec *spec, int32_t n_rows,
                  const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_FBANK_H */
