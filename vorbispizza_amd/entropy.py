"""ctypes binding of include/vorbispizza_entropy.h -- the entropy decode of Vorbis audio packets on the GPU --, of
include/vorbispizza_entropy_group.h -- the same for streams of different setups in one call -- and decode_to_pcm, the whole path of one file on the device: plan (CPU, vpzh_plan_range) -> vpz_entropy_decode ->
vpz_decoder_synth, no residue crossing the host link."""
import ctypes as C

import numpy as np

from . import capi

VERSION = 1
IMAGE_MAGIC, IMAGE_VERSION = 0x45505A56, 1

_vp = C.c_void_p
_SIGNATURES = [
    ("vpz_entropy_version", C.c_int, []),
    ("vpz_entropy_setup_create", C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(_vp)]),
    ("vpz_entropy_setup_destroy", None, [_vp]),
    ("vpz_entropy_decode", C.c_int, [_vp, C.c_int64, _vp, _vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int64, _vp, _vp, C.c_int64,
                                     C.c_int32]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]
_GROUP_SIGNATURES = [
    ("vpz_entropy_group_create", C.c_int, [_vp, _vp, _vp, C.c_int32, C.POINTER(_vp)]),
    ("vpz_entropy_group_destroy", None, [_vp]),
    ("vpz_entropy_group_decode", C.c_int, [_vp, C.c_int32, _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int64, _vp,
                                           _vp, C.c_int64, C.c_int32]),
]
GROUP_EXPORTED_SYMBOLS = [s[0] for s in _GROUP_SIGNATURES]
GROUP_MAX_SETUPS = 256
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = capi.lib()
        for name, restype, argtypes in _SIGNATURES + _GROUP_SIGNATURES:
            if name in GROUP_EXPORTED_SYMBOLS and not hasattr(L, name):
                continue  # (an older build taken through VPZ_LIB_DIR for an A/B run has no group: using one raises)
            fn = getattr(L, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = L
    return _lib


class EntropySetup:
    """vpz_entropy_setup: a validated setup image (OggVorbisFile.entropy_setup()) on the context's device."""

    def __init__(self, ctx, image):
        self.ctx = ctx
        self._image = np.frombuffer(bytes(image), dtype=np.uint8)
        self.channels, self.block_size0, self.block_size1 = (int(v) for v in self._image[12:24].view(np.int32))
        self._h = _vp()
        rc = lib().vpz_entropy_setup_create(ctx._h, self._image.ctypes.data, self._image.size, C.byref(self._h))
        if rc != capi.OK:
            self._h = None
            raise capi.SynthError(rc, ctx.last_error())
        import weakref
        ctx._children.append(weakref.ref(self))

    def close(self):
        if self._h and self.ctx._h:
            lib().vpz_entropy_setup_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_raw(self, packets, spans, payload, residue, posts, post_counts, mem_space, residue_format=None,
                   payload_bytes=None, residue_values=None, n_records=None):
        """Thin call of vpz_entropy_decode.  packets / spans: numpy (host memory, always); payload, residue, posts,
        post_counts: numpy arrays (MEM_HOST) or torch cuda tensors (MEM_DEVICE).  residue_format defaults to the residue's
        element type (int16: RESIDUE_I16).  Returns the status (0 = OK) without raising."""
        packets = np.ascontiguousarray(packets, dtype=capi.PACKET_DTYPE)
        spans = np.ascontiguousarray(spans, dtype=np.int64).reshape(-1, 2)
        if residue_format is None:
            residue_format = capi.RESIDUE_I16 if str(getattr(residue, "dtype", "")) in ("int16", "torch.int16") else capi.RESIDUE_F32
        if mem_space == capi.MEM_DEVICE:
            capi._sync_producer(payload, residue, posts, post_counts)
        return lib().vpz_entropy_decode(
            self._h, len(packets), capi._ptr(packets), capi._ptr(spans), capi._ptr(payload),
            capi._numel(payload) if payload_bytes is None else payload_bytes, int(residue_format), capi._ptr(residue),
            capi._numel(residue) if residue_values is None else residue_values, capi._ptr(posts), capi._ptr(post_counts),
            capi._numel(post_counts) if n_records is None else n_records, int(mem_space))

    def decode(self, packets, spans, payload, residue, posts, post_counts, mem_space=capi.MEM_HOST, residue_format=None):
        """decode_raw that raises SynthError on a failed status."""
        rc = self.decode_raw(packets, spans, payload, residue, posts, post_counts, mem_space, residue_format)
        if rc != capi.OK:
            raise capi.SynthError(rc, self.ctx.last_error())


class EntropyGroup:
    """vpz_entropy_group: validated setup images of one class (channels, block sizes) on the context's device, for
    batches whose streams each name their setup."""

    def __init__(self, ctx, images):
        self.ctx = ctx
        self._images = [np.frombuffer(bytes(im), dtype=np.uint8) for im in images]
        n = len(self._images)
        ptrs = (C.c_void_p * max(1, n))(*[im.ctypes.data for im in self._images])
        sizes = (C.c_uint64 * max(1, n))(*[im.size for im in self._images])
        self._h = _vp()
        rc = lib().vpz_entropy_group_create(ctx._h, ptrs, sizes, n, C.byref(self._h))
        if rc != capi.OK:
            self._h = None
            raise capi.SynthError(rc, ctx.last_error())
        self.n_setups = n
        self.channels, self.block_size0, self.block_size1 = (int(v) for v in self._images[0][12:24].view(np.int32))
        import weakref
        ctx._children.append(weakref.ref(self))

    def close(self):
        if self._h and self.ctx._h:
            lib().vpz_entropy_group_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_raw(self, stream_setup, stream_mapping_base, packets, spans, payload, residue, posts, post_counts, mem_space,
                   residue_format=None, payload_bytes=None, residue_values=None, n_records=None):
        """Thin call of vpz_entropy_group_decode: EntropySetup.decode_raw's arguments after stream_setup / stream_mapping_base
        (one uint8 entry per stream; packets[k]["stream"] indexes them).  Returns the status without raising."""
        stream_setup = np.ascontiguousarray(stream_setup, dtype=np.uint8)
        stream_mapping_base = np.ascontiguousarray(stream_mapping_base, dtype=np.uint8)
        assert stream_setup.size == stream_mapping_base.size
        packets = np.ascontiguousarray(packets, dtype=capi.PACKET_DTYPE)
        spans = np.ascontiguousarray(spans, dtype=np.int64).reshape(-1, 2)
        if residue_format is None:
            residue_format = capi.RESIDUE_I16 if str(getattr(residue, "dtype", "")) in ("int16", "torch.int16") else capi.RESIDUE_F32
        if mem_space == capi.MEM_DEVICE:
            capi._sync_producer(payload, residue, posts, post_counts)
        return lib().vpz_entropy_group_decode(
            self._h, stream_setup.size, capi._ptr(stream_setup), capi._ptr(stream_mapping_base), len(packets), capi._ptr(packets),
            capi._ptr(spans), capi._ptr(payload), capi._numel(payload) if payload_bytes is None else payload_bytes,
            int(residue_format), capi._ptr(residue), capi._numel(residue) if residue_values is None else residue_values,
            capi._ptr(posts), capi._ptr(post_counts), capi._numel(post_counts) if n_records is None else n_records, int(mem_space))

    def decode(self, stream_setup, stream_mapping_base, packets, spans, payload, residue, posts, post_counts,
               mem_space=capi.MEM_HOST, residue_format=None):
        """decode_raw that raises SynthError on a failed status."""
        rc = self.decode_raw(stream_setup, stream_mapping_base, packets, spans, payload, residue, posts, post_counts, mem_space,
                             residue_format)
        if rc != capi.OK:
            raise capi.SynthError(rc, self.ctx.last_error())


def decode_to_pcm(ctx, data, out_layout=capi.OUT_PLANAR, clip_samples=False, residue_i16=False):
    """Decodes one .ogg file (bytes or path) on the device: the CPU plans its packets, vpz_entropy_decode entropy-decodes
    them on the context stream and vpz_decoder_synth (VPZ_MEM_DEVICE) synthesises the PCM from the device-resident result.
    Returns a torch tensor on the context's GPU: [channels, samples] (planar layouts) or [samples, channels] (interleaved),
    float32 or int16 for the _S16 layouts.  residue_i16: the residue as int16 (a stream whose residue is integral).
    A stream the device cannot decode (Floor0, non-tiling residues) raises FrontError: there is no CPU fallback here."""
    import torch

    from .front import FrontError, OggVorbisFile
    f = OggVorbisFile(data)
    try:
        if not f.gpu_decode_supported:
            raise FrontError(f.last_error())
        image = f.entropy_setup()
        packets, spans, payload, residue_values = f.plan_packets()
        channels, size0, size1 = f.channels, f.block_size0, f.block_size1
        floors, mappings = f.floors, f.mappings
    finally:
        f.close()
    dev = torch.device("cuda", ctx.device)
    setup = EntropySetup(ctx, image)
    dec = capi.Decoder(ctx, channels, size0, size1, floors, mappings, n_streams=1, clip_samples=clip_samples)
    try:
        n = len(packets)
        d_payload = torch.from_numpy(payload).to(dev)
        residue = torch.zeros(max(1, residue_values), dtype=torch.int16 if residue_i16 else torch.float32, device=dev)
        posts = torch.zeros((n * channels, 64), dtype=torch.int16, device=dev)
        counts = torch.zeros(n * channels, dtype=torch.uint8, device=dev)
        setup.decode(packets, spans, d_payload, residue, posts, counts, mem_space=capi.MEM_DEVICE)
        per = np.where(packets["flags"] & capi.PKT_BLOCK_FLAG, size1, size0).sum() if n else 0
        capacity = int(per) + 1
        s16 = out_layout in (capi.OUT_INTERLEAVED_S16, capi.OUT_PLANAR_S16)
        pcm = torch.zeros(channels * capacity, dtype=torch.int16 if s16 else torch.float32, device=dev)
        # (same context stream as the decode above: synth consumes its outputs without a synchronise)
        written = dec.synth_raw(packets, residue, posts, counts, pcm, None, capacity, out_layout, capacity, capi.MEM_DEVICE,
                                on_mismatch="ignore")  # (a packet the window check skips is skipped, as on the CPU path)
        ctx.synchronize()
        w = int(written[0])
        if out_layout in (capi.OUT_PLANAR, capi.OUT_PLANAR_S16):
            return pcm.view(channels, capacity)[:, :w].clone()
        return pcm[: w * channels].view(w, channels).clone()
    finally:
        dec.close()
        setup.close()
