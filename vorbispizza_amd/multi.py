"""ctypes view of include/vorbispizza_multi.h, include/vorbispizza_multi_mixed.h, include/vorbispizza_multi_ranges.h, include/vorbispizza_multi_batch.h and
include/vorbispizza_multi_resample.h -- the in-process multi-device dispatcher of
libvorbispizza_host.so (one host process, one context group per MI355X, streams partitioned contiguously, no collective).  What a
C# host P/Invokes; tests and bench.py use it from here."""
import ctypes as C

import numpy as np

from . import capi, front

OK, E_ARG, E_DEVICE, E_NOMEM = 0, -1, -2, -3
E_OPEN, E_CAPACITY, E_SYNTH, E_SETUP = -10, -11, -12, -13
E_RANGE = -14  # (vorbispizza_multi_ranges.h)
E_CHANNELS = -15  # (vorbispizza_multi_batch.h)
E_RATE = -16  # (vorbispizza_multi_resample.h)


class Options(C.Structure):
    _fields_ = [("host_threads", C.c_int32), ("streams_per_call", C.c_int32), ("contexts_per_device", C.c_int32),
                ("clip_samples", C.c_int32), ("slots_per_device", C.c_int32), ("float_residue", C.c_int32),
                ("gpu_entropy", C.c_int32), ("reserved", C.c_int32)]


class StreamResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("device_slot", C.c_int32), ("channels", C.c_int32), ("sample_rate", C.c_int32),
                ("samples", C.c_int64), ("packets", C.c_int64), ("skipped_packets", C.c_int64)]


class Stats(C.Structure):
    _fields_ = [("wall_s", C.c_double), ("device_wall_s", C.c_double * 16), ("device_decode_s", C.c_double * 16),
                ("device_synth_s", C.c_double * 16), ("device_streams", C.c_int64 * 16), ("device_samples", C.c_int64 * 16),
                ("threads_per_device", C.c_int32), ("pinned_mib", C.c_int32),
                # (written only by a dispatcher created with gpu_entropy: a caller with the shorter struct is never written past)
                ("device_gpu_entropy_streams", C.c_int64 * 16), ("device_payload_bytes", C.c_int64 * 16)]


class CallCounts(C.Structure):  # vpzm_call_counts (vorbispizza_multi_mixed.h)
    _fields_ = [("sub_batches", C.c_int64), ("device_decoded_sub_batches", C.c_int64), ("mixed_sub_batches", C.c_int64),
                ("max_setups_per_sub_batch", C.c_int64), ("decoders_created", C.c_int64), ("reserved", C.c_int64 * 3)]


RESULT_DTYPE = np.dtype([("status", "<i4"), ("device_slot", "<i4"), ("channels", "<i4"), ("sample_rate", "<i4"),
                         ("samples", "<i8"), ("packets", "<i8"), ("skipped_packets", "<i8")])
assert RESULT_DTYPE.itemsize == C.sizeof(StreamResult)

EXPORTED_SYMBOLS = ["vpzm_create", "vpzm_destroy", "vpzm_last_error", "vpzm_device_count", "vpzm_decode_library"]
MIXED_EXPORTED_SYMBOLS = ["vpzm_set_mixed_setups", "vpzm_last_call_counts"]  # (vorbispizza_multi_mixed.h)
RANGES_EXPORTED_SYMBOLS = ["vpzm_decode_ranges"]  # (vorbispizza_multi_ranges.h)
BATCH_EXPORTED_SYMBOLS = ["vpzm_batch_partition", "vpzm_decode_ranges_batch"]  # (vorbispizza_multi_batch.h)
RESAMPLE_EXPORTED_SYMBOLS = ["vpzm_decode_ranges_resampled"]  # (vorbispizza_multi_resample.h)
LOGMEL_EXPORTED_SYMBOLS = ["vpzm_decode_ranges_logmel"]  # (vorbispizza_multi_logmel.h)
MELSPEC_EXPORTED_SYMBOLS = ["vpzm_decode_ranges_melspec"]  # (vorbispizza_multi_melspec.h)
STFT_EXPORTED_SYMBOLS = ["vpzm_decode_ranges_stft"]  # (vorbispizza_multi_stft.h)
CQT_EXPORTED_SYMBOLS = ["vpzm_decode_ranges_cqt"]  # (vorbispizza_multi_cqt.h)
FBANK_EXPORTED_SYMBOLS = ["vpzm_decode_ranges_fbank"]  # (vorbispizza_multi_fbank.h)
MFCC_EXPORTED_SYMBOLS = ["vpzm_decode_ranges_mfcc"]  # (vorbispizza_multi_mfcc.h)
FEATPOST_EXPORTED_SYMBOLS = ["vpzm_decode_ranges_fbank_post", "vpzm_decode_ranges_mfcc_post"]  # (vorbispizza_multi_featpost.h)
LOUDNESS_EXPORTED_SYMBOLS = ["vpzm_measure_loudness"]  # (vorbispizza_multi_loudness.h)
LOUDNESS_DTYPE = np.dtype([("integrated", "<f8"), ("peak", "<f8"), ("steps", "<i8"), ("blocks_kept", "<i8")])  # vpzm_loudness
R128_EXPORTED_SYMBOLS = ["vpzm_measure_r128"]  # (vorbispizza_multi_r128.h)
R128_DTYPE = np.dtype([("integrated", "<f8"), ("range", "<f8"), ("range_low", "<f8"), ("range_high", "<f8"), ("momentary_max", "<f8"),
                       ("short_term_max", "<f8"), ("true_peak", "<f8"), ("sample_peak", "<f8"), ("steps", "<i8"), ("blocks_kept", "<i8"),
                       ("range_blocks", "<i8")])  # vpzm_r128
RANGE_DTYPE = np.dtype([("start", "<i8"), ("count", "<i8")])  # vpzm_range
_bound = False


def lib():
    global _bound
    L = front.lib()
    if not _bound:
        vp = C.c_void_p
        L.vpzm_create.argtypes = [vp, C.c_int32, C.POINTER(Options), C.POINTER(vp)]
        L.vpzm_create.restype = C.c_int
        L.vpzm_destroy.argtypes = [vp]
        L.vpzm_destroy.restype = None
        L.vpzm_last_error.argtypes = [vp]
        L.vpzm_last_error.restype = C.c_char_p
        L.vpzm_device_count.argtypes = [vp]
        L.vpzm_device_count.restype = C.c_int
        L.vpzm_decode_library.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp, C.POINTER(Stats)]
        L.vpzm_decode_library.restype = C.c_int
        if hasattr(L, "vpzm_set_mixed_setups"):  # (an older build taken through VPZ_LIB_DIR for an A/B run has neither: using one raises)
            L.vpzm_set_mixed_setups.argtypes = [vp, C.c_int32]
            L.vpzm_set_mixed_setups.restype = C.c_int
            L.vpzm_last_call_counts.argtypes = [vp, C.POINTER(CallCounts)]
            L.vpzm_last_call_counts.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges"):
            L.vpzm_decode_ranges.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp, vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_batch"):
            L.vpzm_batch_partition.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
            L.vpzm_batch_partition.restype = C.c_int
            L.vpzm_decode_ranges_batch.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int64, C.c_int32, vp, vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges_batch.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_resampled"):
            L.vpzm_decode_ranges_resampled.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, vp, vp,
                                                       C.POINTER(Stats)]
            L.vpzm_decode_ranges_resampled.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_logmel"):
            L.vpzm_decode_ranges_logmel.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(capi.LogMelSpec), C.c_int64, vp, vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges_logmel.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_melspec"):
            L.vpzm_decode_ranges_melspec.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(capi.LogMelSpec), C.c_int64, vp, vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges_melspec.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_stft"):
            L.vpzm_decode_ranges_stft.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(capi.StftSpec), C.c_int64,
                                                  vp, vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges_stft.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_cqt"):
            L.vpzm_decode_ranges_cqt.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(capi.CqtSpec), C.c_int64,
                                                 vp, vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges_cqt.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_fbank"):
            L.vpzm_decode_ranges_fbank.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(capi.FbankSpec), C.c_int64, vp, vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges_fbank.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_mfcc"):
            L.vpzm_decode_ranges_mfcc.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(capi.MfccSpec), C.c_int64, vp, vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges_mfcc.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_fbank_post"):
            L.vpzm_decode_ranges_fbank_post.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(capi.FbankSpec), C.POINTER(capi.FeatPostSpec), C.c_int64, vp,
                                                        vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges_fbank_post.restype = C.c_int
            L.vpzm_decode_ranges_mfcc_post.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(capi.MfccSpec), C.POINTER(capi.FeatPostSpec), C.c_int64, vp,
                                                       vp, C.POINTER(Stats)]
            L.vpzm_decode_ranges_mfcc_post.restype = C.c_int
        if hasattr(L, "vpzm_measure_loudness"):
            L.vpzm_measure_loudness.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(Stats)]
            L.vpzm_measure_loudness.restype = C.c_int
        if hasattr(L, "vpzm_measure_r128"):
            L.vpzm_measure_r128.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(Stats)]
            L.vpzm_measure_r128.restype = C.c_int
        if hasattr(L, "vpzm_decode_ranges_normalized"):  # (vorbispizza_multi_normalize.h; vorbispizza_amd/normalize.py is its Python surface)
            L.vpzm_decode_ranges_normalized.argtypes = L.vpzm_decode_ranges_resampled.argtypes + [vp, vp]
            L.vpzm_decode_ranges_normalized.restype = C.c_int
        _bound = True
    return L


class MultiError(RuntimeError):
    pass


class Dispatcher:
    """vpzm_dispatcher: one context group per entry of `device_ids` (an id may repeat: several groups on one GPU).
    gpu_entropy: streams whose setup the device can decode (vpzh_gpu_decode_supported) are entropy-decoded there, the others on
    the host threads in the same call; the PCM is the same bit for bit.  mixed_setups (with gpu_entropy): device-decoded
    sub-batches may hold streams of different setups that agree in channels, block sizes and residue type
    (vpzm_set_mixed_setups); set_mixed_setups changes it between calls."""

    def __init__(self, device_ids, host_threads=0, streams_per_call=0, contexts_per_device=0, clip_samples=False,
                 slots_per_device=0, float_residue=False, gpu_entropy=False, mixed_setups=False):
        ids = (C.c_int32 * len(device_ids))(*[int(d) for d in device_ids])
        opt = Options(host_threads, streams_per_call, contexts_per_device, 1 if clip_samples else 0, slots_per_device,
                      1 if float_residue else 0, 1 if gpu_entropy else 0)
        self._h = C.c_void_p()
        rc = lib().vpzm_create(ids, len(device_ids), C.byref(opt), C.byref(self._h))
        if rc != OK:
            self._h = None
            raise MultiError("vpzm_create failed (status %d)" % rc)
        self.n_devices = len(device_ids)
        self.device_ids = [int(d) for d in device_ids]
        if mixed_setups:
            self.set_mixed_setups(True)

    def set_mixed_setups(self, on):
        """vpzm_set_mixed_setups: from the next call on (see the class)"""
        rc = lib().vpzm_set_mixed_setups(self._h, 1 if on else 0)
        if rc != OK:
            raise MultiError("vpzm_set_mixed_setups failed (status %d)" % rc)

    def call_counts(self):
        """vpzm_last_call_counts: the CallCounts of the last decode_library call"""
        counts = CallCounts()
        rc = lib().vpzm_last_call_counts(self._h, C.byref(counts))
        if rc != OK:
            raise MultiError("vpzm_last_call_counts failed (status %d)" % rc)
        return counts

    def close(self):
        """vpzm_destroy, once: contexts, decoders and page-locked memory go"""
        if getattr(self, "_h", None):
            lib().vpzm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        """vpzm_last_error: the first failure text of the last call ('' when it had none)"""
        return lib().vpzm_last_error(self._h).decode()

    # ---- what the decode methods share
    @staticmethod
    def _inputs(datas, ranges=None):
        """-> (n, the containers' pointers, their sizes, the ranges as a contiguous [n, 2] int64 array or None)"""
        n = len(datas)
        ptrs = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
        sizes = (C.c_uint64 * n)(*[d.size for d in datas])
        rng = None if ranges is None else np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(n, 2))
        return n, ptrs, sizes, rng

    @staticmethod
    def _outputs(n):
        """-> (fresh results, fresh stats)"""
        return np.zeros(n, dtype=RESULT_DTYPE), Stats()

    def _group_tensors(self, method, n, shape, dtype, out):
        """The per-group output tensors of a batch call of n entries: shape(rows) is a group's, for its entries [lo, hi) of
        batch_partition.  Without `out` they are allocated -- when all groups share a device, as consecutive pieces of one tensor --, a
        caller's are checked (anything wrong raises ValueError under the method's name).  -> (out, whole_or_None, the library's pointer array)"""
        import torch
        ids = self.device_ids  # (a group's HIP device id is its torch device index)
        cuts = [self.batch_partition(n, g) for g in range(self.n_devices)]
        whole = None
        if out is None:
            if len(set(ids)) == 1:
                whole = torch.empty(shape(n), dtype=dtype, device="cuda:%d" % ids[0])
                out = [whole[lo:hi] for lo, hi in cuts]
            else:
                out = [torch.empty(shape(hi - lo), dtype=dtype, device="cuda:%d" % d) for (lo, hi), d in zip(cuts, ids)]
        if len(out) != self.n_devices:
            raise ValueError("%s: out needs one tensor per group (%d), got %d" % (method, self.n_devices, len(out)))
        for g, (t, (lo, hi), d) in enumerate(zip(out, cuts, ids)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != d:
                raise ValueError("%s: out[%d] is not a tensor on the group's device cuda:%d" % (method, g, d))
            if tuple(t.shape) != shape(hi - lo) or t.dtype != dtype or not t.is_contiguous():
                raise ValueError("%s: out[%d] must be a contiguous %s tensor of shape %s" % (method, g, dtype, shape(hi - lo)))
        return out, whole, (C.c_void_p * self.n_devices)(*[t.data_ptr() if t.numel() else None for t in out])

    def _drain_torch(self):
        """the library writes on its own streams into memory torch may have just recycled: whatever torch has queued there is done first"""
        import torch
        for d in sorted(set(self.device_ids)):
            torch.cuda.current_stream(d).synchronize()

    def _batch_call(self, name, fn, datas, ranges, shape, dtype, out, args, method=None):
        """What the window-batch methods share behind their own argument checks: the inputs, the groups' tensors of shape(rows) and
        `dtype` (checked under `method`: the library call's `name` unless given), torch's streams drained, and the call
        fn(handle, n, containers, sizes, ranges, *args(the groups' pointers), results, stats).  -> (out, whole_or_None, results, stats)"""
        n, ptrs, sizes, rng = self._inputs(datas, ranges)
        out, whole, dst = self._group_tensors(method or name, n, shape, dtype, out)
        self._drain_torch()
        results, stats = self._outputs(n)
        rc = fn(self._h, n, ptrs, sizes, rng.ctypes.data, *args(dst), results.ctypes.data, C.byref(stats))
        if rc != OK:
            raise MultiError("vpzm_%s failed (status %d): %s" % (name, rc, self.last_error()))
        return out, whole, results, stats

    def _measure_call(self, name, fn, datas, ranges, dtype):
        """a measuring call: no tensor, a record of `dtype` per entry.  -> (results, records, stats)"""
        n, ptrs, sizes, rng = self._inputs(datas, ranges)
        self._drain_torch()
        results, stats = self._outputs(n)
        out = np.zeros(n, dtype=dtype)
        rc = fn(self._h, n, ptrs, sizes, None if rng is None else rng.ctypes.data, out.ctypes.data if n else None, results.ctypes.data, C.byref(stats))
        if rc != OK:
            raise MultiError("vpzm_%s failed (status %d): %s" % (name, rc, self.last_error()))
        return results, out, stats

    def decode_library(self, datas, pcm_out, pcm_offset, pcm_capacity, s16=False):
        """datas: list of numpy uint8 arrays (containers); pcm_out: numpy float32 / int16 array (or a torch pinned tensor's
        .numpy()); pcm_offset / pcm_capacity: per stream, elements / samples per channel.  Returns (results, stats):
        a numpy record array (RESULT_DTYPE) and the Stats struct."""
        n, ptrs, sizes, _ = self._inputs(datas)
        offs = np.ascontiguousarray(pcm_offset, dtype=np.int64)
        caps = np.ascontiguousarray(pcm_capacity, dtype=np.int64)
        assert pcm_out.dtype == (np.int16 if s16 else np.float32) and pcm_out.flags["C_CONTIGUOUS"]
        results, stats = self._outputs(n)
        rc = lib().vpzm_decode_library(self._h, n, ptrs, sizes, capi.OUT_INTERLEAVED_S16 if s16 else capi.OUT_INTERLEAVED,
                                       pcm_out.ctypes.data, offs.ctypes.data, caps.ctypes.data, results.ctypes.data,
                                       C.byref(stats))
        if rc != OK:
            raise MultiError("vpzm_decode_library failed (status %d): %s" % (rc, self.last_error()))
        return results, stats

    def decode_ranges(self, datas, ranges, pcm_out, pcm_offset, pcm_capacity, s16=False):
        """vpzm_decode_ranges: decode_library for a window of every stream.  ranges: per entry (start, count) in samples per
        channel, count < 0 for "to the end"; entry k's samples land at pcm_out[pcm_offset[k]:], and its results' `samples` says
        how many, `packets` how many packets were decoded for them.  Returns (results, stats) like decode_library."""
        n, ptrs, sizes, rng = self._inputs(datas, ranges)
        offs = np.ascontiguousarray(pcm_offset, dtype=np.int64)
        caps = np.ascontiguousarray(pcm_capacity, dtype=np.int64)
        assert pcm_out.dtype == (np.int16 if s16 else np.float32) and pcm_out.flags["C_CONTIGUOUS"]
        results, stats = self._outputs(n)
        rc = lib().vpzm_decode_ranges(self._h, n, ptrs, sizes, rng.ctypes.data, capi.OUT_INTERLEAVED_S16 if s16 else capi.OUT_INTERLEAVED,
                                      pcm_out.ctypes.data, offs.ctypes.data, caps.ctypes.data, results.ctypes.data, C.byref(stats))
        if rc != OK:
            raise MultiError("vpzm_decode_ranges failed (status %d): %s" % (rc, self.last_error()))
        return results, stats

    def batch_partition(self, n, group):
        """vpzm_batch_partition: the entries [lo, hi) of an n-entry call that group `group` decodes"""
        lo, hi = C.c_int32(), C.c_int32()
        rc = lib().vpzm_batch_partition(self._h, n, group, C.byref(lo), C.byref(hi))
        if rc != OK:
            raise MultiError("vpzm_batch_partition failed (status %d)" % rc)
        return lo.value, hi.value

    def decode_ranges_batch(self, datas, ranges, channels, frames, planar=True, s16=False, out=None, sample_rate=None, mono=False):
        """vpzm_decode_ranges_batch: decode_ranges delivered as a zero-padded batch in device memory.  Entry k's window becomes row k:
        [channels, frames] (planar) or [frames, channels], float32 or int16 (s16), its samples first, zeros behind them.
        out: a list of torch tensors, one per group, on that group's device, contiguous, of shape [hi - lo, channels, frames] (or
        [hi - lo, frames, channels]) for the group's entries [lo, hi) (batch_partition) -- anything else raises before the library is
        called.  Without `out` the method allocates: when all groups share a device, one tensor whose consecutive pieces the groups get.
        sample_rate / mono (vpzm_decode_ranges_resampled; the defaults are the call above, the same library function as ever): every
        window is delivered at `sample_rate` -- the ranges stay in source samples, a row holds ceil(samples * up / down) output samples and
        results["samples"] counts those --, and with mono=True the rows have one channel (channels must be 1), the mean of the stream's.
        mono needs a `sample_rate`: the library's resampled call has one rate.
        Returns (parts, whole_or_None, results, stats)."""
        import torch
        if channels < 1 or frames < 1:
            raise ValueError("decode_ranges_batch: channels and frames must be at least 1")
        if mono and (sample_rate is None or channels != 1):
            raise ValueError("decode_ranges_batch: mono needs a sample_rate (a resampled call has one rate) and channels == 1")
        shape = (lambda rows: (rows, channels, frames)) if planar else (lambda rows: (rows, frames, channels))
        dtype = torch.int16 if s16 else torch.float32
        layout = {(True, False): capi.OUT_PLANAR, (False, False): capi.OUT_INTERLEAVED, (True, True): capi.OUT_PLANAR_S16,
                  (False, True): capi.OUT_INTERLEAVED_S16}[(bool(planar), bool(s16))]
        if sample_rate is None:
            return self._batch_call("decode_ranges_batch", lib().vpzm_decode_ranges_batch, datas, ranges, shape, dtype, out,
                                    lambda dst: (channels, frames, layout, dst))
        return self._batch_call("decode_ranges_resampled", lib().vpzm_decode_ranges_resampled, datas, ranges, shape, dtype, out,
                                lambda dst: (int(sample_rate), channels, int(bool(mono)), frames, layout, dst), method="decode_ranges_batch")

    def _decode_ranges_normalized(self, datas, ranges, sample_rate, channels, mono, frames, planar, s16, out, spec, records):
        """vpzm_decode_ranges_normalized behind vorbispizza_amd.normalize.decode_ranges_normalized, which checks the arguments and makes
        `spec` (a ctypes vpzm_norm_spec) and `records` (a contiguous array of n vpzm_norm_out): decode_ranges_batch's resampled call with
        the two behind its arguments.  -> (parts, whole_or_None, results, stats)"""
        import torch
        shape = (lambda rows: (rows, channels, frames)) if planar else (lambda rows: (rows, frames, channels))
        layout = {(True, False): capi.OUT_PLANAR, (False, False): capi.OUT_INTERLEAVED, (True, True): capi.OUT_PLANAR_S16,
                  (False, True): capi.OUT_INTERLEAVED_S16}[(bool(planar), bool(s16))]
        fn = lib().vpzm_decode_ranges_normalized
        return self._batch_call("decode_ranges_normalized", lambda *head: fn(*head, C.byref(spec), records.ctypes.data if records.size else None),
                                datas, ranges, shape, torch.int16 if s16 else torch.float32, out,
                                lambda dst: (int(sample_rate), channels, int(bool(mono)), frames, layout, dst))

    def decode_ranges_logmel(self, datas, ranges, frames, sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=None,
                             mel_scale="slaney", mel_norm="slaney", log=True, floor=1e-10, bands_first=True, out=None):
        """vpzm_decode_ranges_logmel: decode_ranges_batch(..., sample_rate=sample_rate, mono=True) with one more stage on the device --
        entry k's window, resampled and mixed down, padded with zeros to `frames` OUTPUT samples, becomes row k of (log-)mel frames:
        [n_mels, T] (bands_first) or [T, n_mels], float32, T = 1 + frames // hop (include/vorbispizza_pcm_logmel.h states the
        definition; f_max None: sample_rate / 2; log False: the mel power).  results["samples"] counts the window's output samples.
        out: as for decode_ranges_batch, one contiguous float32 tensor per group of shape [hi - lo, n_mels, T] (or [hi - lo, T, n_mels])
        on the group's device -- anything else raises before the library is called.  Returns (parts, whole_or_None, results, stats)."""
        import torch
        spec = capi.LogMelSpec.make(sample_rate=sample_rate, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=f_min, f_max=f_max, mel_scale=mel_scale,
                                    mel_norm=mel_norm, log=log, floor=floor, bands_first=bands_first)
        if frames < 1 or hop < 1 or n_mels < 1:
            raise ValueError("decode_ranges_logmel: frames, hop and n_mels must be at least 1")
        T = spec.n_frames(frames)
        shape = (lambda rows: (rows, n_mels, T)) if bands_first else (lambda rows: (rows, T, n_mels))
        return self._batch_call("decode_ranges_logmel", lib().vpzm_decode_ranges_logmel, datas, ranges, shape, torch.float32, out,
                                lambda dst: (C.byref(spec), int(frames), dst))

    def decode_ranges_melspec(self, datas, ranges, frames, sample_rate=22050, n_fft=2048, hop=512, n_mels=128, f_min=0.0, f_max=None,
                              mel_scale="slaney", mel_norm="slaney", log=True, floor=1e-10, bands_first=True, out=None):
        """vpzm_decode_ranges_melspec: decode_ranges_logmel's call, shapes and results with the transforms of music front ends -- n_fft
        2048, 4096 or 8192, one real FFT per frame on the device (include/vorbispizza_pcm_melspec.h states the definition and the error
        bound; the defaults are librosa's mel spectrogram at 22 050 Hz).  Returns (parts, whole_or_None, results, stats)."""
        import torch
        spec = capi.LogMelSpec.make(sample_rate=sample_rate, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=f_min, f_max=f_max, mel_scale=mel_scale,
                                    mel_norm=mel_norm, log=log, floor=floor, bands_first=bands_first)
        if frames < 1 or hop < 1 or n_mels < 1:
            raise ValueError("decode_ranges_melspec: frames, hop and n_mels must be at least 1")
        T = spec.n_frames(frames)
        shape = (lambda rows: (rows, n_mels, T)) if bands_first else (lambda rows: (rows, T, n_mels))
        return self._batch_call("decode_ranges_melspec", lib().vpzm_decode_ranges_melspec, datas, ranges, shape, torch.float32, out,
                                lambda dst: (C.byref(spec), int(frames), dst))

    def decode_ranges_stft(self, datas, ranges, frames, sample_rate=44100, channels=2, mono=False, n_fft=4096, hop=1024, win_length=None,
                           window="hann", output="complex", bins_first=True, out=None):
        """vpzm_decode_ranges_stft: decode_ranges_batch(..., sample_rate=sample_rate, planar float32) with one more stage on the device
        -- every channel of entry k's window, resampled, padded with zeros to `frames` OUTPUT samples, becomes a short-time Fourier
        spectrogram: torch.stft(row, n_fft, hop, win_length, window, center=True, pad_mode="reflect", return_complex=True) with a
        periodic 'hann' or 'hamming' window (include/vorbispizza_pcm_stft.h states the definition and the error bound; n_fft 512 to
        8192; the defaults are a separation model's at 44.1 kHz).  output 'complex' gives complex64 tensors, 'magnitude' and 'power'
        float32: [n, C, n_fft / 2 + 1, T] (bins_first, torch's order) or [n, C, T, n_fft / 2 + 1], T = 1 + frames // hop.  The channel
        dimension is always there: C = channels, or 1 with mono=True (the mean of the stream's channels, whatever `channels` says).
        out: as in decode_ranges_batch, tensors of that shape and element type.  Returns (parts, whole_or_None, results, stats)."""
        import torch
        spec = capi.StftSpec.make(n_fft=n_fft, hop=hop, win_length=win_length, window=window, output=output, bins_first=bins_first)
        C_out = 1 if mono else int(channels)
        if frames < 1 or hop < 1 or n_fft < 2 or C_out < 1:
            raise ValueError("decode_ranges_stft: frames, hop and channels must be at least 1")
        T, n_freq = spec.n_frames(frames), spec.n_freq
        shape = (lambda rows: (rows, C_out, n_freq, T)) if bins_first else (lambda rows: (rows, C_out, T, n_freq))
        return self._batch_call("decode_ranges_stft", lib().vpzm_decode_ranges_stft, datas, ranges, shape,
                                torch.complex64 if output == "complex" else torch.float32, out,
                                lambda dst: (int(sample_rate), C_out, int(bool(mono)), C.byref(spec), int(frames), dst))

    def decode_ranges_cqt(self, datas, ranges, frames, sample_rate=22050, channels=1, mono=True, f_min=32.70319566257483, n_bins=84,
                          bins_per_octave=12, hop=512, filter_scale=1.0, gamma=0.0, window="hann", scale="sqrt_length", pad="reflect",
                          output="magnitude", bins_first=True, out=None):
        """vpzm_decode_ranges_cqt: decode_ranges_stft with the constant-Q transform as its stage -- every channel of entry k's window,
        resampled to `sample_rate`, padded with zeros to `frames` OUTPUT samples, becomes a constant-Q spectrogram: n_bins bins at
        f_min * 2^(k / bins_per_octave), each with its own periodic 'hann' or 'hamming' window of N_k = ceil(Q sample_rate / (f_k +
        gamma / alpha)) samples centred on sample t * hop (include/vorbispizza_pcm_cqt.h states the definition and the error bound;
        the defaults are 84 bins from C1 at 22.05 kHz).  scale 'sqrt_length' reads white noise flat across the bins, 'none' a unit cosine
        as 0.5; pad 'reflect' centres as the other stages do, 'zero' takes clips shorter than the lowest bin's window.  output 'complex'
        gives complex64 tensors, 'magnitude' and 'power' float32: [n, C, n_bins, T] (bins_first) or [n, C, T, n_bins], T = 1 + frames //
        hop.  The channel dimension is always there: C = channels, or 1 with mono=True (the mean of the stream's channels, whatever
        `channels` says).  out: as in decode_ranges_batch, tensors of that shape and element type.  Returns (parts, whole_or_None,
        results, stats)."""
        import torch
        spec = capi.CqtSpec.make(sample_rate=sample_rate, f_min=f_min, n_bins=n_bins, bins_per_octave=bins_per_octave, hop=hop,
                                 filter_scale=filter_scale, gamma=gamma, window=window, scale=scale, pad=pad, output=output, bins_first=bins_first)
        C_out = 1 if mono else int(channels)
        if frames < 1 or hop < 1 or n_bins < 1 or C_out < 1:
            raise ValueError("decode_ranges_cqt: frames, hop, n_bins and channels must be at least 1")
        T, nb = spec.n_frames(frames), int(n_bins)
        shape = (lambda rows: (rows, C_out, nb, T)) if bins_first else (lambda rows: (rows, C_out, T, nb))
        return self._batch_call("decode_ranges_cqt", lib().vpzm_decode_ranges_cqt, datas, ranges, shape,
                                torch.complex64 if output == "complex" else torch.float32, out,
                                lambda dst: (int(sample_rate), C_out, int(bool(mono)), C.byref(spec), int(frames), dst))

    def decode_ranges_fbank(self, datas, ranges, frames, sample_rate=16000, win=400, hop=160, n_fft=512, n_mels=80, low_freq=20.0, high_freq=0.0,
                            preemphasis=0.97, window="povey", remove_dc=True, scale=32768.0, log=True, floor=capi.FLT_EPSILON, pad_value=0.0,
                            frames_first=True, out=None):
        """vpzm_decode_ranges_fbank: decode_ranges_batch(..., sample_rate=sample_rate, mono=True) with one more stage on the device --
        entry k's window, resampled and mixed down, becomes row k of Kaldi filterbank frames: [T, n_mels] (frames_first) or [n_mels, T],
        float32, T = 1 + (frames - win) // hop (include/vorbispizza_pcm_fbank.h states the definition; the defaults are Kaldi's fbank at
        16 kHz with 80 bands; log False: the mel power).  results["samples"] counts the window's output samples J: the row's first
        FbankSpec.n_frames(J) frames are real, the others hold pad_value.
        out: as for decode_ranges_batch, one contiguous float32 tensor per group of shape [hi - lo, T, n_mels] (or [hi - lo, n_mels, T])
        on the group's device -- anything else raises before the library is called.  Returns (parts, whole_or_None, results, stats)."""
        import torch
        spec = capi.FbankSpec.make(sample_rate=sample_rate, win=win, hop=hop, n_fft=n_fft, n_mels=n_mels, low_freq=low_freq, high_freq=high_freq,
                                   preemphasis=preemphasis, window=window, remove_dc=remove_dc, scale=scale, log=log, floor=floor,
                                   pad_value=pad_value, frames_first=frames_first)
        if win < 1 or frames < win or hop < 1 or n_mels < 1:
            raise ValueError("decode_ranges_fbank: hop and n_mels must be at least 1, and frames at least win")
        T = spec.n_frames(frames)
        shape = (lambda rows: (rows, T, n_mels)) if frames_first else (lambda rows: (rows, n_mels, T))
        return self._batch_call("decode_ranges_fbank", lib().vpzm_decode_ranges_fbank, datas, ranges, shape, torch.float32, out,
                                lambda dst: (C.byref(spec), int(frames), dst))

    def decode_ranges_mfcc(self, datas, ranges, frames, sample_rate=16000, win=400, hop=160, n_fft=512, n_mels=23, low_freq=20.0, high_freq=0.0,
                           preemphasis=0.97, window="povey", remove_dc=True, scale=32768.0, floor=capi.FLT_EPSILON, pad_value=0.0,
                           frames_first=True, n_ceps=13, lifter=22.0, use_energy=True, energy_floor=0.0, htk_compat=False,
                           subtract_mean=False, out=None):
        """vpzm_decode_ranges_mfcc: decode_ranges_fbank with the cepstral stage behind the log-mel values -- entry k's window, resampled
        and mixed down, becomes row k of Kaldi MFCC frames: [T, n_ceps] (frames_first) or [n_ceps, T], float32,
        T = 1 + (frames - win) // hop (include/vorbispizza_pcm_mfcc.h states the definition; the defaults are Kaldi's mfcc at 16 kHz:
        13 cepstra of 23 bands, lifter 22, C0 replaced by the log energy).  results["samples"] counts the window's output samples J: the
        row's first MfccSpec.n_frames(J) frames are real, the others hold pad_value.
        out: as for decode_ranges_batch, one contiguous float32 tensor per group of shape [hi - lo, T, n_ceps] (or [hi - lo, n_ceps, T])
        on the group's device -- anything else raises before the library is called.  Returns (parts, whole_or_None, results, stats)."""
        import torch
        spec = capi.MfccSpec.make(sample_rate=sample_rate, win=win, hop=hop, n_fft=n_fft, n_mels=n_mels, low_freq=low_freq, high_freq=high_freq,
                                  preemphasis=preemphasis, window=window, remove_dc=remove_dc, scale=scale, floor=floor, pad_value=pad_value,
                                  frames_first=frames_first, n_ceps=n_ceps, lifter=lifter, use_energy=use_energy, energy_floor=energy_floor,
                                  htk_compat=htk_compat, subtract_mean=subtract_mean)
        if win < 1 or frames < win or hop < 1 or n_ceps < 1:
            raise ValueError("decode_ranges_mfcc: hop and n_ceps must be at least 1, and frames at least win")
        T = spec.n_frames(frames)
        shape = (lambda rows: (rows, T, n_ceps)) if frames_first else (lambda rows: (rows, n_ceps, T))
        return self._batch_call("decode_ranges_mfcc", lib().vpzm_decode_ranges_mfcc, datas, ranges, shape, torch.float32, out,
                                lambda dst: (C.byref(spec), int(frames), dst))

    def _decode_ranges_posted(self, name, fn, datas, ranges, frames, spec, mel, D, post, out):
        """the posted fbank / MFCC call: spec the feature spec, mel its FbankSpec, D its columns"""
        import torch
        if not isinstance(post, capi.FeatPostSpec):
            raise TypeError("%s: post is a capi.FeatPostSpec or None" % name)
        if mel.win < 1 or frames < mel.win or mel.hop < 1 or D < 1:
            raise ValueError("%s: hop and the feature columns must be at least 1, and frames at least win" % name)
        if post.layout != mel.layout:
            raise ValueError("%s: the post spec's layout (frames_first) is the feature spec's" % name)
        if post.delta_order < 0 or post.delta_order > capi.FEAT_MAX_DELTA_ORDER:
            raise ValueError("%s: delta_order is 0 .. %d" % (name, capi.FEAT_MAX_DELTA_ORDER))
        T, D_out = mel.n_frames(frames), post.out_columns(D)
        shape = (lambda rows: (rows, T, D_out)) if mel.layout == capi.FBANK_FRAMES_FIRST else (lambda rows: (rows, D_out, T))
        return self._batch_call(name, fn, datas, ranges, shape, torch.float32, out, lambda dst: (C.byref(spec), C.byref(post), int(frames), dst))

    def decode_ranges_fbank_post(self, datas, ranges, frames, post=None, out=None, **fbank):
        """vpzm_decode_ranges_fbank_post: decode_ranges_fbank(datas, ranges, frames, **fbank) with Kaldi's feature post-processing behind
        it on the device -- post: a capi.FeatPostSpec (deltas, mean / variance normalisation over the row or a sliding window;
        include/vorbispizza_pcm_featpost.h states the definition) in the feature spec's layout.  Row k is [T, D_out] (frames_first) or
        [D_out, T], D_out = n_mels * (delta_order + 1); its first FbankSpec.n_frames(results["samples"][k]) frames are real, the others
        hold the POST spec's pad_value.  The result is, bit for bit, capi.feat_post over decode_ranges_fbank's tensor.  post None:
        decode_ranges_fbank itself.  out: one contiguous float32 tensor per group, [hi - lo, T, D_out] (or [hi - lo, D_out, T]) on the
        group's device -- anything else raises before the library is called.  Returns (parts, whole_or_None, results, stats)."""
        if post is None:
            return self.decode_ranges_fbank(datas, ranges, frames, out=out, **fbank)
        spec = capi.FbankSpec.make(**fbank)
        return self._decode_ranges_posted("decode_ranges_fbank_post", lib().vpzm_decode_ranges_fbank_post, datas, ranges, frames, spec, spec,
                                          spec.n_mels, post, out)

    def decode_ranges_mfcc_post(self, datas, ranges, frames, post=None, out=None, **mfcc):
        """vpzm_decode_ranges_mfcc_post: decode_ranges_mfcc(datas, ranges, frames, **mfcc) with the same post-processing behind it;
        D_out = n_ceps * (delta_order + 1).  The MFCC spec's own subtract_mean may be combined with `post`: it runs first.  post None:
        decode_ranges_mfcc itself."""
        if post is None:
            return self.decode_ranges_mfcc(datas, ranges, frames, out=out, **mfcc)
        spec = capi.MfccSpec.make(**mfcc)
        return self._decode_ranges_posted("decode_ranges_mfcc_post", lib().vpzm_decode_ranges_mfcc_post, datas, ranges, frames, spec, spec.fbank,
                                          spec.n_ceps, post, out)

    def measure_loudness(self, datas, ranges=None):
        """vpzm_measure_loudness: every entry's window (ranges None: the whole stream) measured for programme loudness on the device
        (ITU-R BS.1770-4; include/vorbispizza_pcm_loudness.h states the definition), at the stream's own rate and channel count -- no
        PCM comes down.  Returns (results, integrated, peak, steps, blocks_kept, stats): numpy arrays with an entry per stream --
        float64 LUFS (-inf with fewer than four steps or nothing kept), float64 sample peak, int64 whole 100 ms steps, int64 blocks
        behind the value; results["samples"] counts the samples measured.  An entry that delivered nothing has (-inf, 0, 0, 0)."""
        results, out, stats = self._measure_call("measure_loudness", lib().vpzm_measure_loudness, datas, ranges, LOUDNESS_DTYPE)
        return (results, out["integrated"].copy(), out["peak"].copy(), out["steps"].copy(), out["blocks_kept"].copy(), stats)

    def measure_r128(self, datas, ranges=None):
        """vpzm_measure_r128: every entry's window (ranges None: the whole stream) measured for what an EBU R 128 scanner reports, on the
        device (include/vorbispizza_pcm_r128.h and vorbispizza_pcm_loudness.h state the definitions), at the stream's own rate and
        channel count -- no PCM comes down.  Returns (results, records, stats): records is a numpy array of R128_DTYPE with an entry per
        stream -- integrated LUFS, loudness range in LU with its two percentile levels, maximum momentary and short-term loudness, true
        peak and sample peak (float32 values), whole 100 ms steps, and the blocks behind the integrated value and the range;
        results["samples"] counts the samples measured.  integrated, sample_peak, steps and blocks_kept are measure_loudness's bits.  An
        entry that delivered nothing has (-inf, 0, -inf, -inf, -inf, -inf, 0, 0, 0, 0, 0)."""
        return self._measure_call("measure_r128", lib().vpzm_measure_r128, datas, ranges, R128_DTYPE)
