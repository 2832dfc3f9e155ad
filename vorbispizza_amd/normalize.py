"""Window batches normalised on the device (include/vorbispizza_multi_normalize.h): decode_ranges_normalized is
Dispatcher.decode_ranges_batch(..., sample_rate=...) with vpz_pcm_normalize (include/vorbispizza_pcm_normalize.h) as its last stage.  A
function of this module, not a method: the dispatcher's public methods are a closed set."""
import ctypes as C

import numpy as np

MODES = {"meanvar": 1, "peak": 2, "rms": 3, "gain": 4, "loudness": 5}  # VPZM_NORM_*
DEFAULT_TARGETS = {"meanvar": 0.0, "peak": 1.0, "rms": 0.1, "loudness": -23.0, "gain": 1.0}  # what target=None means
EXPORTED_SYMBOLS = ["vpzm_decode_ranges_normalized"]
NORM_OUT_DTYPE = np.dtype([("gain", "<f8"), ("mean", "<f8"), ("peak", "<f8"), ("loudness", "<f8")])  # vpzm_norm_out


class MultiNormSpec(C.Structure):
    """vpzm_norm_spec"""
    _fields_ = [("target", C.c_double), ("eps", C.c_double), ("ceiling", C.c_double), ("mode", C.c_int32), ("reserved", C.c_int32 * 9)]


class MultiNormOut(C.Structure):
    """vpzm_norm_out"""
    _fields_ = [("gain", C.c_double), ("mean", C.c_double), ("peak", C.c_double), ("loudness", C.c_double)]


assert C.sizeof(MultiNormSpec) == 64 and C.sizeof(MultiNormOut) == NORM_OUT_DTYPE.itemsize == 32


def decode_ranges_normalized(dispatcher, datas, ranges, channels, frames, sample_rate, mono=False, mode="meanvar", target=None, eps=1e-7,
                             ceiling=0.0, planar=True, s16=False, out=None):
    """vpzm_decode_ranges_normalized: dispatcher.decode_ranges_batch(datas, ranges, channels, frames, planar, s16, out, sample_rate, mono)
    with every row normalised on the device over its REAL samples, all its channels together; the padding stays zero.
    mode "meanvar": zero mean and unit variance, 1 / sqrt(var + eps) -- Wav2Vec2FeatureExtractor's zero_mean_unit_var_norm;
    "peak" / "rms": the row's peak / RMS level becomes `target` (linear; None: 1.0 / 0.1); "loudness": its programme loudness, measured as
    measure_loudness measures the window, becomes `target` LUFS (None: -23.0); "gain": `target` is one linear gain for every row (None: 1.0).
    ceiling > 0 (not with "meanvar"): a row's delivered peak stays at or below it.  float32 rows are not clipped; s16 rows go through the
    library's one conversion.  Returns (parts, whole_or_None, results, stats) as decode_ranges_batch does, `results` a dict of the
    record array's fields -- "status", "samples" (the OUTPUT samples in the row) and the rest -- plus "gain", "mean", "peak" (float64
    arrays: the float32 gain and offset a row was made with and its peak before the gain) and "loudness" (LUFS; -inf but in the loudness
    mode); an entry that delivered nothing has gain 1, mean 0, peak 0, loudness -inf."""
    if mode not in MODES:
        raise ValueError("decode_ranges_normalized: mode is one of %s" % ", ".join(repr(m) for m in MODES))
    if channels < 1 or frames < 1 or sample_rate is None or int(sample_rate) < 1:
        raise ValueError("decode_ranges_normalized: channels, frames and sample_rate must be at least 1")
    if mono and channels != 1:
        raise ValueError("decode_ranges_normalized: mono needs channels == 1")
    spec = MultiNormSpec()
    spec.mode = MODES[mode]
    spec.target = float(DEFAULT_TARGETS[mode] if target is None else target)
    spec.eps, spec.ceiling = float(eps), float(ceiling)
    records = np.zeros(len(datas), dtype=NORM_OUT_DTYPE)
    parts, whole, results, stats = dispatcher._decode_ranges_normalized(datas, ranges, int(sample_rate), int(channels), bool(mono), int(frames),
                                                                       bool(planar), bool(s16), out, spec, records)
    merged = {name: results[name] for name in results.dtype.names}
    merged.update({name: records[name].copy() for name in NORM_OUT_DTYPE.names})
    return parts, whole, merged, stats
