/*
 * vorbispizza_pcm_featpost.h -- Kaldi feature post-processing of a padded batch of feature frames in device memory: delta features and
 * cepstral mean / variance normalisation over a row or a sliding window, libvorbispizza_synth.so.
 *
 * vpz_pcm_fbank and vpz_pcm_mfcc deliver padded [rows][T][D] tensors whose rows have their own real lengths.  What a Kaldi-style loader
 * does before the model sees a frame is the rest of vorbispizza_pcm_mfcc.h's "NOT PART OF IT": apply-cmvn per utterance (with or without
 * variance), add-deltas, apply-cmvn-sliding.  In a framework these need a mask for the pad frames, one padded convolution per delta order
 * (which clamps the first-order deltas at the edges, where Kaldi clamps the INPUT) and a cumsum / unfold chain per row for the window's edge
 * rules.  vpz_feat_post is that stage on the device, over any float32 [rows][T][D] tensor -- log-mel frames are served too.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).
 * Tensors.  Source: float32, src[src_rows][T][D] (layout == VPZ_FEAT_FRAMES_FIRST) or src[src_rows][D][T] (VPZ_FEAT_COLUMNS_FIRST).
 * Destination: float32, D_out = D * (delta_order + 1) columns, the same layout.  The two must not overlap.
 * Row descriptors.  A vpz_feat_row names a source row, its n = real_frames real frames (0 <= n <= T) and a destination row; destination
 * rows are distinct.  Frames t >= n of a named destination row hold `pad_value` (rounded to float32) in every column; every element of a
 * named row is written exactly once, rows that no descriptor names are not touched; a row with n = 0 reads nothing (its src_row is not
 * looked at beyond its sign, and the source may have no rows).  A value's bits depend
 * on its row's real frames and the spec alone: not on where the row sits, on n_rows, on the grid or on T.
 *   1. Deltas (Kaldi DeltaFeatures; w = delta_window).  s_0 = [1]; s_i[k] = (sum over j = -w .. w of j * s_(i-1)[k - j])
 *      / (sum over j of j * j) for k = -i w .. i w (s_(i-1) is zero outside its own support).  Evaluated as s_i[k] = N_i[k] / Z^i with the
 *      integers N_0 = [1], N_i[k] = sum over j of j * N_(i-1)[k - j] and Z = sum over j of j * j: one division in double, rounded once
 *      to float32.  (Order 1, window 2: [-2, -1, 0, 1, 2] / 10; order 2, window 2:
 *      [4, 4, 1, -4, -10, -4, 1, 4, 4] / 100.)  Output column i * D + d of frame t < n is
 *          sum over j = -i w .. i w of s_i[j] * x[clamp(t + j, 0, n - 1)][d],
 *      j ascending from an accumulator of 0, every step one float32 fused multiply-add; terms whose scale is exactly 0 are skipped.  Block 0
 *      is the input, copied.  The clamp is to the row's REAL frames, not to T.  This is not torchaudio's compute_deltas applied twice, which
 *      clamps the first-order deltas: Kaldi convolves the scales and clamps the input once.
 *   2. The window of frame t (Kaldi SlidingWindowCmn; W = cmn_window), in integers.  With `center`: a = t - W / 2 (the quotient truncated),
 *      b = a + W.  Without: a = t - W, b = t + 1 -- the steady window has W + 1 frames, which is Kaldi's and torchaudio's behaviour and is
 *      kept.  If a < 0: b -= a, a = 0.  Without `center`: b = max(t + 1, min_window).  If b > n: a -= b - n, b = n, a = max(a, 0).
 *      c = b - a >= 1 (with `center`, c = min(n, W)).  VPZ_NORM_ROW: a = 0, b = n for every t.
 *   3. Normalisation, per column, x the column's float32 values.  S1 = sum of x, S2 = sum of x * x over [a, b), in float64 (a float32
 *      square is exact there), IN THIS ORDER: the row's real frames are cut into chunks k = frames 64 k .. min(64 k + 63, n - 1); a chunk
 *      sum runs over its frames ascending from 0.  With e = min(b, 64 * ceil(a / 64)), a window's sum is, from an accumulator of 0 and
 *      leaving out what is empty: plus L, the sum of [a, e) ascending from 0 (the left partial chunk, or the whole window when it crosses
 *      no chunk boundary); plus the sums of the whole chunks in [e, b), k ascending; plus R, the sum ascending from 0 of the frames that
 *      are left in front of b (the right partial chunk).  S1 and S2 take the same path.  m = S1 / c.
 *      Without norm_vars: out = fl32((double)x - m).  With norm_vars: c == 1 gives out = fl32(((double)x - m) * 0.0) -- zero, and not
 *      finite where x is not --; otherwise v = fma(-m, m, S2 / c) (one rounding), v = var_floor where not v >= var_floor, and
 *      out = fl32(((double)x - m) / sqrt(v)), division and square root correctly rounded.
 *   4. Composition.  With both stages on, the result is bit for bit that of two single-stage calls in `order`, the tensor between them
 *      float32: VPZ_POST_NORM_FIRST normalises the D input columns and takes deltas of the result; VPZ_POST_DELTAS_FIRST (add-deltas |
 *      apply-cmvn-sliding) takes deltas and normalises all D_out columns.
 *   5. A value that is not finite makes exactly those outputs not finite whose window or non-zero delta taps cover it; every other row keeps
 *      the bits it has without it.
 * Limits.  1 <= D <= VPZ_FEAT_MAX_COLUMNS; T >= 1; 0 <= delta_order <= 3; 1 <= delta_window <= 8; 1 <= min_window <= cmn_window <= 2^20;
 * var_floor finite and > 0 (Kaldi's sliding code: 1e-10); pad_value finite; norm_vars, center 0 or 1; norm, order and layout one of their
 * constants; reserved words zero.  Every field is checked whatever `norm` is; a spec that does nothing (VPZ_NORM_NONE and delta_order 0)
 * is refused.
 * NOT PART OF IT: global CMVN from dataset statistics (one broadcast multiply-add, which a framework already fuses into the next op);
 * online or speaker-level CMVN (statistics carried across utterances: the caller's state, not a batch's); frame splicing / LFR stacking
 * (a strided view of the tensor); VAD frame selection (it changes a row's real frames: select first, then call).
 *
 * A header of its own: the older headers, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 * Error against a longdouble restatement (tests/featpost_truth.py), largest error / derived bound over the tests' cases on an MI355X:
 * 0.996 for the normalised values (the bound's leading term is their own rounding to float32), 0.35 for the deltas.
 */
#ifndef VORBISPIZZA_PCM_FEATPOST_H
#define VORBISPIZZA_PCM_FEATPOST_H

#include <stdint.h>

#include "vorbispizza_synth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VPZ_NORM_NONE 0
#define VPZ_NORM_ROW 1
#define VPZ_NORM_SLIDING 2
#define VPZ_POST_NORM_FIRST 0
#define VPZ_POST_DELTAS_FIRST 1
#define VPZ_FEAT_COLUMNS_FIRST 0 /* [rows][D][T]; the values of VPZ_FBANK_BANDS_FIRST / _FRAMES_FIRST */
#define VPZ_FEAT_FRAMES_FIRST 1  /* [rows][T][D] */
#define VPZ_FEAT_MAX_COLUMNS 256
#define VPZ_FEAT_MAX_DELTA_ORDER 3
#define VPZ_FEAT_MAX_DELTA_WINDOW 8
#define VPZ_FEAT_MAX_CMN_WINDOW (1 << 20)
#define VPZ_FEAT_CHUNK 64 /* frames of a chunk sum */

/* sizeof(vpz_feat_row) == sizeof(vpz_pack_row) == 24 */
typedef struct vpz_feat_row {
    int64_t src_row;     /* 0 <= src_row < src_rows; with real_frames = 0 any src_row >= 0 (nothing is read) */
    int64_t real_frames; /* n, 0 <= n <= T; the rest of the destination row becomes pad_value */
    int64_t row;         /* destination row, 0 <= row < dst_rows */
} vpz_feat_row;

/* sizeof(vpz_feat_post_spec) == 96: 2 doubles, 9 + 11 int32 */
typedef struct vpz_feat_post_spec {
    double var_floor;     /* > 0 */
    double pad_value;     /* what frames t >= n hold */
    int32_t norm;         /* VPZ_NORM_* */
    int32_t norm_vars;    /* 0 / 1 */
    int32_t center;       /* 0 / 1 (VPZ_NORM_SLIDING) */
    int32_t cmn_window;   /* W */
    int32_t min_window;   /* 1 .. W (VPZ_NORM_SLIDING without center) */
    int32_t delta_order;  /* 0 .. 3 */
    int32_t delta_window; /* 1 .. 8 */
    int32_t order;        /* VPZ_POST_* (both stages on) */
    int32_t layout;       /* VPZ_FEAT_*: of source and destination alike */
    int32_t reserved[11]; /* zero: room to grow */
} vpz_feat_post_spec;

/* The host helpers need no device.  VPZ_E_INVALID_ARG: a null pointer, a spec outside the limits, an argument outside what is said. */

/* s_i of item 1, i = 0 .. delta_order, as 2 i w + 1 floats (index j + i w); scales == null: nothing is written.
 * VPZ_E_CAPACITY: scales given and capacity < 2 i w + 1. */
int vpz_feat_delta_scales(const vpz_feat_post_spec *spec, int32_t i, float *scales, int64_t capacity);

/* [a, b) of item 2 for frame t of a row of n real frames, 0 <= t < n (VPZ_NORM_NONE is refused). */
int vpz_feat_cmn_window(const vpz_feat_post_spec *spec, int64_t t, int64_t n, int64_t *a, int64_t *b);

/* The scratch memory of a call, in float64 elements: 0 for VPZ_NORM_NONE, else 2 * n_rows * ceil(T / 64) * (the normalised columns: D,
 * or D_out with VPZ_POST_DELTAS_FIRST) -- the chunk sums S1 and S2, nothing else.  VPZ_E_INVALID_ARG also where the size overflows. */
int vpz_feat_post_scratch(const vpz_feat_post_spec *spec, int32_t n_rows, int64_t T, int32_t D, int64_t *elems);

/* The stage.  src_dev holds src_rows * T * D float32, dst_dev dst_rows * T * D_out, scratch_dev scratch_elems float64 (it may be null
 * where vpz_feat_post_scratch gives 0, or where no descriptor has a real frame: such a call needs and looks at none); `rows` is host memory and free again when the call returns.  Asynchronous on the context's stream:
 * one launch for deltas alone, two for a normalisation alone (chunk sums, then the values; one where no descriptor has a real frame) and
 * for VPZ_POST_DELTAS_FIRST (both take the deltas on their way), three for VPZ_POST_NORM_FIRST (the normalised columns are block 0 of the destination; the third launch reads them
 * there).  The scratch memory belongs to the call until the stream has passed it.
 * VPZ_E_INVALID_ARG, with nothing launched: a null pointer; a spec, T or D outside the limits; a negative count; a descriptor whose
 * src_row, real_frames or row is out of range or whose row is named twice; sizes that overflow; src_dev or dst_dev not aligned to 4 bytes, scratch_dev to 16;
 * src_dev, dst_dev or scratch_dev not device memory of the context's device, or leaving its allocation; source and destination, or the
 * scratch memory and either, overlapping.  VPZ_E_CAPACITY, with nothing launched: scratch_elems below vpz_feat_post_scratch's. */
int vpz_feat_post(vpz_context *ctx, const void *src_dev, int64_t src_rows, int64_t T, int32_t D, const vpz_feat_post_spec *spec,
                  int32_t n_rows, const vpz_feat_row *rows, void *dst_dev, int64_t dst_rows, void *scratch_dev, int64_t scratch_elems);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_FEATPOST_H */
