/*
 * vorbispizza_pcm_normalize.h -- windows of a planar float32 device array delivered as a dense, zero-padded batch whose rows are
 * normalised on the way: zero mean and unit variance, a peak level, an RMS level or a given gain, libvorbispizza_synth.so.
 *
 * Self-supervised speech models (wav2vec 2.0, HuBERT, WavLM) take waveforms whose every clip has zero mean and unit variance over its
 * REAL samples, the padding left at zero; music and codec loaders bring every clip to a peak, an RMS level or a loudness and keep it
 * from clipping; an int16 batch is only safe with a level rule in front of the conversion.  In a framework this is a mask, a masked
 * mean, a masked variance and a masked scale, which read the batch three times.  vpz_pcm_normalize is that stage on the device: it
 * reads every window twice (its statistics, then its values) and writes it once, in the caller's layout.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).
 * Source.  float32, planar: a descriptor's `src` is the element offset of its window's first sample in channel 0, channel c lies
 * c * frames elements further on (the shape of a [rows][channels][frames] tensor with src = row * channels * frames, but any offset
 * serves).  J = samples real samples per channel, 0 <= J <= frames; N = channels * J.
 * Destination.  dst[dst_rows][channels][frames] (VPZ_OUT_PLANAR, VPZ_OUT_PLANAR_S16) or dst[dst_rows][frames][channels]
 * (VPZ_OUT_INTERLEAVED, VPZ_OUT_INTERLEAVED_S16), float32 or int16.  Every element of a row named by a descriptor is written exactly
 * once -- J values per channel, then +0.0f / 0 --, rows that no descriptor names are not touched; a descriptor with J = 0 reads nothing.
 * A value's bits depend on its window's samples, the spec and (VPZ_NORM_GAIN) its gain alone: not on where the window lies in the
 * source, on its row, on n_rows, on `frames` or on the grid.
 *   1. Statistics, ONE set per descriptor, joint over its N samples (a stereo clip keeps its balance).  x are the float32 samples.
 *      P = max |x|.  S1 = sum of x, S2 = sum of x * x in float64 (a float32 square is exact there), IN THIS ORDER: a channel's J samples
 *      are cut into chunks q = samples 1024 q .. min(1024 q + 1023, J - 1) (VPZ_NORM_CHUNK; counted from the window's first sample, not
 *      from an address).  Inside a chunk, lane l of 64 adds, from an accumulator of 0, samples 256 t + 4 l + i of the chunk for
 *      t = 0 .. 3 and, inside t, i = 0 .. 3, ascending (samples past the chunk's end are left out); the 64 lane sums are folded by
 *      halves: l with l + 32, then with l + 16, 8, 4, 2, 1.  The chunk sums are added from an accumulator of 0, ascending by chunk inside
 *      a channel, the channels ascending.  S1 and S2 take the same path.  No atomics, and no workgroup waits for another one: the chunk
 *      sums are a launch of their own.
 *   2. Offset m and gain g, in float64 and rounded ONCE to float32 (division and square root correctly rounded: they are in this
 *      build, and tests/test_pcm_normalize_gpu.py holds the downloaded `mean` and `gain` to a numpy restatement bit for bit).
 *        VPZ_NORM_MEANVAR  m = S1 / N, v = max(0, S2 / N - m * m) (quotient, product and difference rounded one by one),
 *                          g = 1 / sqrt(v + eps): the population variance; with eps = 1e-7 it is
 *                          Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm over the real samples.  `ceiling` must be 0.
 *        VPZ_NORM_PEAK     m = 0, g = target / P; target linear, > 0.
 *        VPZ_NORM_RMS      m = 0, g = target / sqrt(S2 / N).
 *        VPZ_NORM_GAIN     m = 0, g = the descriptor's `gain`, finite and > 0 (no other mode reads the field).
 *      N = 0 or P = 0 (which is S2 = 0): m = 0, g = 1, whatever the mode.  With ceiling > 0 (PEAK, RMS, GAIN): where g * P > ceiling
 *      (in float64, before g is rounded), g = ceiling / P.  VPZ_NORM_GAIN with ceiling == 0 and no result array needs no statistics
 *      and launches none.
 *   3. Values.  y = fl32(fl32(x - m) * g): two float32 operations, never fused; with m = 0 the first is exact.  float32 rows are not
 *      clipped; int16 rows go through the library's one conversion, (int)(y * 32768f) clamped to the int16 range.
 *   4. Result (optional).  result_dev[r] = { S1, S2, P, m, g } of descriptor r as doubles; m and g are the float32 values the rows
 *      were made with, widened.  In device memory: it is complete when the stream has passed the call.
 * ERROR BOUND, derived, against a numpy.longdouble two-pass restatement (the mean first, then sum (x - mean)^2;
 * tests/normalize_truth.py).  u = 2^-53, w = 2^-24, K = channels * ceil(J / 1024), d = 22 + K (the additions a sample's term passes:
 * 15 in its lane, 6 in the fold, K across the chunks, and one for the first-order remainder), mu, var, g* the truth's mean, variance
 * and gain.
 *      |S1 - sum x| <= d u N P and |S2 - sum x^2| <= d u S2, so |m64 - mu| <= (d + 1) u P.
 *      One-pass variance: S2 / N and m64^2 agree in their leading digits when the mean dominates, and what is left carries their
 *      absolute errors: |v - var| <= (3 d + 5) u P^2 =: dv.  rho = dv / (var + eps); the bound is claimed for rho <= 1 / 2 (the tests
 *      assert that of their cases), where 1 / sqrt(1 - rho) <= 1 + rho.
 *      e_g, the relative error of g: rho + 3 u + w (MEANVAR); (d + 4) u + w (RMS); 2 u + w (PEAK, GAIN; the 2 u also cover a ceiling
 *      taken on one side of g * P = ceiling and not on the other, where the two gains agree to that much).
 *      dm = |m - mu| <= (d + 1) u P + w |mu| (MEANVAR; 0 otherwise): the float32 offset is the definition's, as it is the framework's,
 *      and a row whose mean dwarfs its deviation pays w |mu| g* in every value.
 *      |y - y*| <= g* ((|x - mu| + dm) ((1 + w)^2 (1 + e_g) - 1) + dm) + 2^-150 (the last term: a product in the subnormal range).
 * An int16 value is within 1 of the conversion of the truth where |y - y*| * 32768 < 1 (the truncation moves a value by less than 1).
 * NOT PART OF IT: per-channel statistics; a limiter or compressor; true-peak ceilings; gains from ReplayGain tags.
 *
 * A header of its own: the older headers, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 * Error against the longdouble restatement, largest error / derived bound over the tests' cases on an MI355X: 0.976 (the bound's leading term
 * is the two float32 roundings of a value; mean and gain equalled the float64 numpy restatement bit for bit in every case).
 */
#ifndef VORBISPIZZA_PCM_NORMALIZE_H
#define VORBISPIZZA_PCM_NORMALIZE_H

#include <stdint.h>

#include "vorbispizza_synth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_NORM_MEANVAR 1
#define VPZ_NORM_PEAK 2
#define VPZ_NORM_RMS 3
#define VPZ_NORM_GAIN 4
#define VPZ_NORM_CHUNK 1024 /* samples of a chunk sum */

/* sizeof(vpz_norm_row) == 32 */
typedef struct vpz_norm_row {
    int64_t src;     /* element offset of the window's first sample (channel 0) in the source array */
    int64_t samples; /* J, samples per channel, 0 <= J <= frames; the rest of the row becomes zero */
    int64_t row;     /* destination row, 0 <= row < dst_rows */
    double gain;     /* VPZ_NORM_GAIN: the linear gain, finite and > 0; not read otherwise */
} vpz_norm_row;

/* sizeof(vpz_norm_spec) == 64: 3 doubles, 2 + 8 int32 */
typedef struct vpz_norm_spec {
    double target;        /* PEAK, RMS: the linear level, finite and > 0; not read otherwise */
    double eps;           /* MEANVAR: added to the variance, finite and >= 0; checked in every mode */
    double ceiling;       /* 0: none; > 0 (PEAK, RMS, GAIN): g * P stays at or below it; 0 with MEANVAR */
    int32_t mode;         /* VPZ_NORM_* */
    int32_t channels;     /* 1 .. VPZ_MAX_CHANNELS */
    int32_t reserved[8];  /* zero: room to grow */
} vpz_norm_spec;

/* sizeof(vpz_norm_result) == 40 */
typedef struct vpz_norm_result {
    double sum;    /* S1 */
    double sum_sq; /* S2 */
    double peak;   /* P */
    double mean;   /* m, the float32 value, widened */
    double gain;   /* g, the float32 value, widened */
} vpz_norm_result;

/* The scratch memory of a call, in float64 elements: n_rows * (3 * channels * ceil(frames / 1024) + 2) -- the chunks' S1, S2 and P and
 * every descriptor's m and g, nothing else.  Needs no device.  VPZ_E_INVALID_ARG: a null pointer, n_rows < 0, channels outside
 * 1..VPZ_MAX_CHANNELS, frames < 1, a size that overflows. */
int vpz_pcm_normalize_scratch(int32_t n_rows, int32_t channels, int64_t frames, int64_t *doubles);

/* The stage.  src_dev holds src_elems float32, dst_dev dst_rows * channels * frames elements of dst_layout's type, scratch_dev
 * scratch_doubles float64 (it may be null where no descriptor has a real sample, and for VPZ_NORM_GAIN with ceiling == 0 and no result
 * array: such a call needs and looks at none), result_dev n_rows vpz_norm_result or null; `rows` is host memory and free again when the
 * call returns.  Asynchronous on the context's stream, in three launches: the chunk sums, one wave per descriptor that adds them and
 * works out m and g (so that no workgroup of the third repeats that), the values; one launch where no statistics are needed.  The
 * scratch memory belongs to the call until the stream has passed it.
 * VPZ_E_INVALID_ARG, with nothing launched: what vpz_pcm_pack refuses (a null pointer; frames < 1; negative counts; a layout other than
 * the four; samples above frames; a row out of range or named twice; misaligned pointers; src_dev or dst_dev not device memory of the
 * context's device or leaving its allocation), and in the place of its ranges a descriptor whose source range
 * [src, src + (channels - 1) * frames + samples) leaves [0, src_elems) (with samples == 0: src outside [0, src_elems]); an unknown mode;
 * channels outside 1..VPZ_MAX_CHANNELS; a target or gain that its mode reads and that is not finite or not > 0; eps or ceiling not
 * finite or < 0; ceiling != 0 with MEANVAR; a non-zero reserved word; scratch memory that is needed and null, smaller than
 * vpz_pcm_normalize_scratch's, not aligned to 8 bytes, not device memory of the context's device or overlapping source or destination;
 * a result array that is not such memory; source and destination overlapping. */
int vpz_pcm_normalize(vpz_context *ctx, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_norm_spec *spec,
                      int32_t n_rows, const vpz_norm_row *rows, void *dst_dev, int64_t dst_rows, int32_t dst_layout,
                      void *scratch_dev, int64_t scratch_doubles, vpz_norm_result *result_dev);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_NORMALIZE_H */
