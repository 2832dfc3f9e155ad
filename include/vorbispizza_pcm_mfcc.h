/*
 * vorbispizza_pcm_mfcc.h -- windows of a mono device PCM array delivered as Kaldi MFCC feature frames in device memory,
 * libvorbispizza_synth.so.
 *
 * vpz_pcm_fbank (vorbispizza_pcm_fbank.h) is the Kaldi filterbank.  The second front end of that family is compute-mfcc-feats /
 * torchaudio.compliance.kaldi.mfcc: cepstra of the log-mel values, C0 replaced by the frame's log energy, cepstral mean subtraction --
 * the input of speaker-ID, keyword-spotting, alignment and GMM / TDNN recipes.  A loader that builds them from vpz_pcm_fbank needs the PCM
 * a second time for the energy and follows with unfold, mean, square-sum, a matmul with the DCT, a lifter multiply, a column overwrite, a
 * mean over frames and a subtraction.  vpz_pcm_mfcc is that front end on the device: the cepstra and the energy come from what the fbank
 * kernel already holds in LDS, and the mean over frames is one more small launch.
 *
 * THE DEFINITION (its one statement; DESIGN.md section 6 refers to it).
 * Descriptors, the padded length F, T = 1 + (F - win) / hop, a row's real frames T_L, the rule that frames t >= T_L hold `pad_value` in
 * every coefficient and the rule that every element of a named row is written exactly once are those of vorbispizza_pcm_fbank.h, with
 * `fbank` as the spec of the mel stage.  Per real frame, with N = fbank.n_mels:
 *   1. Log-mel values.  E[b] = ln(max(M[b], floor)), b = 0 .. N-1: vpz_pcm_fbank's value of the frame (output VPZ_FBANK_LOG), bit for
 *      bit -- the same mean, table, fused multiply-add chain, band sum and logf.
 *   2. Cepstra.  c[i] = sum_b C[i][b] E[b], i = 0 .. n_ceps-1, b ascending from an accumulator of 0, every step one float32 fused
 *      multiply-add.  C[i][b] = l[i] * D[i][b] * (htk_compat && !use_energy && i == 0 ? sqrt(2) : 1) with Kaldi's ComputeDctMatrix
 *          D[0][b] = sqrt(1 / N),   D[i][b] = sqrt(2 / N) cos(pi i (b + 0.5) / N)
 *      and the lifter l[i] = 1 + (Q / 2) sin(pi i / Q) for Q = `lifter` > 0, else 1.  C is evaluated in double and rounded once to float32.
 *   3. Energy (use_energy; Kaldi's raw energy: after scale and DC removal, before pre-emphasis and the window).  With
 *      a[m] = fl(x[m] - mu), the very value the product's A operand uses (mu = 0 without remove_dc),
 *          S = fl(fl(scale) * fl(scale)) * ((s_0 + s_1) + (s_2 + s_3)),   s_q = fma(a[m], a[m], s_q) over m = q, q + 4, ..., ascending
 *      -- the mean's own four-lane pattern, every step rounded to float32 --, e = ln(max(S, 2^-23)); with energy_floor > 0 (as float32),
 *      e = max(e, logf(energy_floor)); c[0] = e.  The mean is not folded, for the reason vorbispizza_pcm_fbank.h gives: a DC of 500 times
 *      the signal does not cost the energy its digits.
 *   4. htk_compat.  The frame is stored as c[1], ..., c[n_ceps-1], c[0].
 *   5. subtract_mean (cepstral mean subtraction), per row and stored coefficient j, after 1 to 4, over the row's T_L real frames only.
 *      The 64 partial sums p_q = sum over t = q (mod 64), t ascending, are taken in float64 and combined as p_q += p_(q xor d) for
 *      d = 1, 2, 4, 8, 16, 32; the sum is divided by T_L in float64 and rounded once to float32; out = fl32(v - mean).  Pad frames keep
 *      pad_value; a row with T_L = 0 reads nothing.  A value's bits depend on its row's samples and the spec alone, wherever the row sits.
 *   6. A sample that is not finite behaves as in vorbispizza_pcm_fbank.h for a frame: exactly the frames that cover it are not finite,
 *      in every coefficient.  With subtract_mean it makes the whole row's real frames not finite, and every other row the same bits as
 *      without it.
 * Destination.  float32, dst[dst_rows][T][n_ceps] (fbank.layout == VPZ_FBANK_FRAMES_FIRST, Kaldi's own order) or dst[dst_rows][n_ceps][T].
 * Limits.  fbank inside the limits of vorbispizza_pcm_fbank.h with output == VPZ_FBANK_LOG; 1 <= n_ceps <= fbank.n_mels; lifter and
 * energy_floor finite and >= 0; use_energy, htk_compat and subtract_mean 0 or 1; reserved words zero.
 * NOT PART OF IT: dither and VTLN; energy after the window (raw_energy = false); an energy column on the filterbank output; deltas;
 * variance normalisation; a sliding-window CMN.
 *
 * A header of its own: vorbispizza_pcm_fbank.h, the older headers, VPZ_ABI_VERSION and their bindings do not change with it.
 * Conventions are those of vorbispizza_synth.h: cdecl, int status (VPZ_OK / VPZ_E_*), caller-owned buffers.
 */
#ifndef VORBISPIZZA_PCM_MFCC_H
#define VORBISPIZZA_PCM_MFCC_H

#include <stdint.h>

#include "vorbispizza_pcm_fbank.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sizeof(vpz_mfcc_spec) == 208: a vpz_fbank_spec (128), 2 doubles, 4 + 12 int32 */
typedef struct vpz_mfcc_spec {
    vpz_fbank_spec fbank;   /* the mel stage: every field under vorbispizza_pcm_fbank.h's limits, output == VPZ_FBANK_LOG; `layout` and
                               `pad_value` are the cepstral tensor's */
    double lifter;          /* Q >= 0; 0: none (Kaldi: 22) */
    double energy_floor;    /* >= 0; 0: none */
    int32_t n_ceps;         /* 1 .. fbank.n_mels */
    int32_t use_energy;     /* 0 / 1 */
    int32_t htk_compat;     /* 0 / 1 */
    int32_t subtract_mean;  /* 0 / 1 */
    int32_t reserved[12];   /* zero: room to grow */
} vpz_mfcc_spec;

/* The matrix C of a spec (fbank.n_mels, n_ceps, lifter, htk_compat, use_energy; the other fields must be inside their limits), computed
 * on the host in double and rounded once to float32; needs no device.  The table is [n_ceps][n_mels] in the STORED order of item 4:
 * table[j * n_mels + b] is the weight of E[b] in the frame's j-th stored value (with htk_compat, row n_ceps - 1 is C[0]).  With
 * use_energy the row of c[0] is still written, though the kernel puts the energy in its place.  table == null: nothing is written (the
 * size is n_ceps * n_mels floats).
 * VPZ_E_INVALID_ARG: spec null or outside the limits, capacity < 0.  VPZ_E_CAPACITY: table given and capacity < n_ceps * n_mels. */
int vpz_mfcc_table(const vpz_mfcc_spec *spec, float *table, int64_t capacity);

/* The contract of vpz_pcm_fbank (source, `frames`, descriptors, asynchronous on the context's stream, tables built on first use and kept
 * by the context) with dst_dev of dst_rows * T * n_ceps float32 elements.  With subtract_mean a second launch follows the first on the
 * same stream.
 * VPZ_E_INVALID_ARG, with nothing launched: what vpz_pcm_fbank refuses; fbank.output != VPZ_FBANK_LOG; n_ceps outside 1 .. n_mels; a
 * negative or non-finite lifter or energy_floor; a flag other than 0 / 1; reserved words not zero. */
int vpz_pcm_mfcc(vpz_context *ctx, const void *src_dev, int64_t src_elems, int64_t frames, const vpz_mfcc_spec *spec, int32_t n_rows,
                 const vpz_pack_row *rows, void *dst_dev, int64_t dst_rows);

#ifdef __cplusplus
}
#endif
#endif /* VORBISPIZZA_PCM_MFCC_H */
