"""ctypes binding of include/vorbispizza_synth.h -- the same entry points a C# host P/Invokes.

There is no CPU fallback: if the shared library is missing the import raises, and every compute
call raises SynthError when no MI355X is usable.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (VPZ_LIB_DIR: another build of the two libraries, for A/B runs of two builds on one GPU box -- tools/ab_builds.sh)
LIB_PATH = os.path.join(os.environ.get("VPZ_LIB_DIR") or os.path.join(_HERE, "lib"), "libvorbispizza_synth.so")

OK = 0
E_INVALID_ARG, E_UNSUPPORTED, E_HIP, E_NOMEM, E_WINDOW_MISMATCH, E_NO_DEVICE, E_CAPACITY = -1, -2, -3, -4, -5, -6, -7
MEM_HOST, MEM_DEVICE = 0, 1
RESIDUE_F32, RESIDUE_I16 = 0, 1  # vpz_decoder_set_residue_format (ABI v5)
IMDCT_FAST, IMDCT_EXACT = 0, 1
OUT_INTERLEAVED, OUT_PLANAR, OUT_INTERLEAVED_S16, OUT_PLANAR_S16 = 0, 1, 2, 3
PKT_BLOCK_FLAG, PKT_PREV_FLAG, PKT_NEXT_FLAG, PKT_EOS = 0x01, 0x02, 0x04, 0x08
PKT_NOT_DECODED, PKT_INTERLEAVED, PKT_NO_FLOOR, PKT_RESYNC = 0x10, 0x20, 0x40, 0x80
MAX_FLOOR1_POSTS, POSTS_STRIDE, MAX_CHANNELS, MAX_COUPLING = 65, 64, 255, 256


class Floor1Config(C.Structure):
    _fields_ = [("x_count", C.c_int32), ("multiplier", C.c_int32), ("x_list", C.c_int32 * MAX_FLOOR1_POSTS)]


class Floor0Config(C.Structure):
    _fields_ = [("order", C.c_int32), ("rate", C.c_int32), ("bark_map_size", C.c_int32), ("amp_bits", C.c_int32),
                ("amp_ofs", C.c_int32)]


class MappingConfig(C.Structure):
    _fields_ = [("coupling_steps", C.c_int32),
                ("coupling_magnitude", C.c_uint8 * MAX_COUPLING),
                ("coupling_angle", C.c_uint8 * MAX_COUPLING),
                ("channel_floor", C.c_uint8 * (MAX_CHANNELS + 1)),
                ("residue_begin", C.c_int32 * 2), ("residue_end", C.c_int32 * 2)]


class StreamConfig(C.Structure):
    _fields_ = [("channels", C.c_int32), ("block_size0", C.c_int32), ("block_size1", C.c_int32),
                ("floor_count", C.c_int32), ("floors", C.POINTER(Floor1Config)),
                ("mapping_count", C.c_int32), ("mappings", C.POINTER(MappingConfig)),
                ("clip_samples", C.c_int32),
                ("floor_types", C.POINTER(C.c_uint8)), ("floors0", C.POINTER(Floor0Config))]


class Packet(C.Structure):
    _fields_ = [("stream", C.c_int32), ("flags", C.c_uint8), ("mapping", C.c_uint8),
                ("reserved", C.c_uint16), ("granule", C.c_int64), ("residue_offset", C.c_int64)]


PACKET_DTYPE = np.dtype([("stream", "<i4"), ("flags", "u1"), ("mapping", "u1"), ("reserved", "<u2"),
                         ("granule", "<i8"), ("residue_offset", "<i8")])
assert PACKET_DTYPE.itemsize == C.sizeof(Packet) == 24

# every symbol include/vorbispizza_synth.h declares: (name, restype, argtypes)
_vp = C.c_void_p
_SIGNATURES = [
    ("vpz_abi_version", C.c_int, []),
    ("vpz_error_string", C.c_char_p, [C.c_int]),
    ("vpz_device_count", C.c_int, []),
    ("vpz_context_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("vpz_context_destroy", None, [_vp]),
    ("vpz_context_synchronize", C.c_int, [_vp]),
    ("vpz_context_last_error", C.c_char_p, [_vp]),
    ("vpz_context_stream", _vp, [_vp]),
    ("vpz_context_timer_start", C.c_int, [_vp]),
    ("vpz_context_timer_stop", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("vpz_device_alloc", C.c_int, [_vp, C.c_uint64, C.POINTER(_vp)]),
    ("vpz_device_free", C.c_int, [_vp, _vp]),
    ("vpz_host_alloc", C.c_int, [_vp, C.c_uint64, C.POINTER(_vp)]),
    ("vpz_host_free", C.c_int, [_vp, _vp]),
    ("vpz_memcpy_h2d", C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    ("vpz_memcpy_d2h", C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    ("vpz_imdct_batch", C.c_int, [_vp, C.c_int, C.c_int64, _vp, _vp, C.c_int, C.c_int]),
    ("vpz_decoder_create", C.c_int, [_vp, C.POINTER(StreamConfig), C.c_int32, C.POINTER(_vp)]),
    ("vpz_decoder_destroy", None, [_vp]),
    ("vpz_decoder_reset", C.c_int, [_vp, C.c_int32]),
    ("vpz_decoder_synth", C.c_int, [_vp, C.c_int64, _vp, _vp, C.c_int64, _vp, _vp, C.c_int64, C.c_int, _vp, _vp,
                                    C.c_int64, C.c_int, C.c_int64, _vp]),
    ("vpz_decoder_last_packet_status", C.c_int, [_vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    ("vpz_decoder_set_floor0_data", C.c_int, [_vp, _vp, _vp, C.c_int32]),
    ("vpz_decoder_last_packet_samples", C.c_int, [_vp, _vp, C.c_int64]),
    ("vpz_decoder_has_clipped", C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int32)]),
    ("vpz_decoder_position", C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int64)]),
    ("vpz_decoder_set_position", C.c_int, [_vp, C.c_int32, C.c_int64]),
    ("vpz_decoder_set_residue_format", C.c_int, [_vp, C.c_int32]),
    ("vpz_decoder_set_stream_capacities", C.c_int, [_vp, C.POINTER(C.c_int64), C.c_int32]),
    ("vpz_decoder_set_host_threads", C.c_int, [_vp, C.c_int32]),
]
# include/vorbispizza_synth_debug.h (test-only entry points, not part of the surface a C# host binds)
_DEBUG_SIGNATURES = [
    ("vpz_debug_floor1_indices", C.c_int, [_vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
]
# include/vorbispizza_pcm.h (a header of its own: the product header and its ABI version do not change with it)
_PCM_SIGNATURES = [
    ("vpz_pcm_download", C.c_int, [_vp, _vp, _vp, C.c_uint64]),
]
# include/vorbispizza_pcm_pack.h (a header of its own, like vorbispizza_pcm.h)
_PCM_PACK_SIGNATURES = [
    ("vpz_pcm_pack", C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp, C.c_int64, C.c_int64, C.c_int32]),
]
PACK_ROW_DTYPE = np.dtype([("src", "<i8"), ("samples", "<i8"), ("row", "<i8")])  # vpz_pack_row
# include/vorbispizza_pcm_resample.h (a header of its own again)
_PCM_RESAMPLE_SIGNATURES = [
    ("vpz_resample_filter", C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int64]),
    ("vpz_pcm_resample", C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_int64, C.c_int32,
                                   C.c_int64, C.c_int32]),
]
RESAMPLE_MAX_UP, RESAMPLE_MAX_DOWN_PER_UP = 1024, 32


class LogMelSpec(C.Structure):
    """vpz_logmel_spec (include/vorbispizza_pcm_logmel.h).  LogMelSpec.make(...) takes the names a Python caller uses."""
    _fields_ = [("sample_rate", C.c_double), ("f_min", C.c_double), ("f_max", C.c_double), ("floor", C.c_double),
                ("n_fft", C.c_int32), ("hop", C.c_int32), ("n_mels", C.c_int32), ("mel_scale", C.c_int32), ("mel_norm", C.c_int32),
                ("output", C.c_int32), ("layout", C.c_int32), ("reserved", C.c_int32 * 9)]

    @classmethod
    def make(cls, sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=None, mel_scale="slaney", mel_norm="slaney", log=True,
             floor=1e-10, bands_first=True):
        scales, norms = {"htk": MEL_HTK, "slaney": MEL_SLANEY}, {None: MEL_NORM_NONE, "none": MEL_NORM_NONE, "slaney": MEL_NORM_SLANEY}
        if mel_scale not in scales or mel_norm not in norms:
            raise ValueError("LogMelSpec: mel_scale is 'htk' or 'slaney', mel_norm None or 'slaney'")
        s = cls()
        s.sample_rate, s.f_min, s.f_max, s.floor = float(sample_rate), float(f_min), float(sample_rate / 2.0 if f_max is None else f_max), float(floor)
        s.n_fft, s.hop, s.n_mels = int(n_fft), int(hop), int(n_mels)
        s.mel_scale, s.mel_norm = scales[mel_scale], norms[mel_norm]
        s.output, s.layout = (MEL_LOG10 if log else MEL_POWER), (MEL_BANDS_FIRST if bands_first else MEL_FRAMES_FIRST)
        return s

    def n_frames(self, frames):
        """T of a row of `frames` samples."""
        return 1 + int(frames) // self.hop


MEL_HTK, MEL_SLANEY = 0, 1
MEL_NORM_NONE, MEL_NORM_SLANEY = 0, 1
MEL_POWER, MEL_LOG10 = 0, 1
MEL_BANDS_FIRST, MEL_FRAMES_FIRST = 0, 1
LOGMEL_MIN_NFFT, LOGMEL_MAX_NFFT, LOGMEL_MAX_MELS = 32, 1024, 256
# include/vorbispizza_pcm_logmel.h (a header of its own again)
_PCM_LOGMEL_SIGNATURES = [
    ("vpz_logmel_dft_table", C.c_int, [C.c_int32, _vp, C.c_int64]),
    ("vpz_mel_filterbank", C.c_int, [C.POINTER(LogMelSpec), _vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    ("vpz_pcm_logmel", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(LogMelSpec), C.c_int32, _vp, _vp, C.c_int64]),
]
PCM_LOGMEL_EXPORTED_SYMBOLS = [s[0] for s in _PCM_LOGMEL_SIGNATURES]
MELSPEC_MIN_NFFT, MELSPEC_MAX_NFFT, MELSPEC_MAX_MELS = 2048, 8192, 256
# include/vorbispizza_pcm_melspec.h (a header of its own again; the spec is LogMelSpec)
_PCM_MELSPEC_SIGNATURES = [
    ("vpz_melspec_twiddles", C.c_int, [C.c_int32, _vp, C.c_int64]),
    ("vpz_melspec_filterbank", C.c_int, [C.POINTER(LogMelSpec), _vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    ("vpz_pcm_melspec", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(LogMelSpec), C.c_int32, _vp, _vp, C.c_int64]),
]
PCM_MELSPEC_EXPORTED_SYMBOLS = [s[0] for s in _PCM_MELSPEC_SIGNATURES]


class StftSpec(C.Structure):
    """vpz_stft_spec (include/vorbispizza_pcm_stft.h).  StftSpec.make(...) takes the names a Python caller uses."""
    _fields_ = [("n_fft", C.c_int32), ("hop", C.c_int32), ("win_length", C.c_int32), ("window", C.c_int32), ("output", C.c_int32),
                ("layout", C.c_int32), ("reserved", C.c_int32 * 10)]

    @classmethod
    def make(cls, n_fft=4096, hop=1024, win_length=None, window="hann", output="complex", bins_first=True):
        windows = {"hann": STFT_HANN, "hamming": STFT_HAMMING}
        outputs = {"complex": STFT_COMPLEX, "magnitude": STFT_MAGNITUDE, "power": STFT_POWER}
        if window not in windows or output not in outputs:
            raise ValueError("StftSpec: window is 'hann' or 'hamming', output 'complex', 'magnitude' or 'power'")
        s = cls()
        s.n_fft, s.hop, s.win_length = int(n_fft), int(hop), int(n_fft if win_length is None else win_length)
        s.window, s.output, s.layout = windows[window], outputs[output], (STFT_BINS_FIRST if bins_first else STFT_FRAMES_FIRST)
        return s

    def n_frames(self, frames):
        """T of a row of `frames` samples."""
        return 1 + int(frames) // self.hop

    @property
    def n_freq(self):
        return self.n_fft // 2 + 1

    def row_shape(self, frames):
        """a row of the destination as float32: (n_freq, T) or (T, n_freq), with a last 2 for the complex output"""
        inner = (self.n_freq, self.n_frames(frames)) if self.layout == STFT_BINS_FIRST else (self.n_frames(frames), self.n_freq)
        return inner + ((2,) if self.output == STFT_COMPLEX else ())


STFT_HANN, STFT_HAMMING = 0, 1
STFT_COMPLEX, STFT_MAGNITUDE, STFT_POWER = 0, 1, 2
STFT_BINS_FIRST, STFT_FRAMES_FIRST = 0, 1
STFT_MIN_NFFT, STFT_MAX_NFFT = 512, 8192
# include/vorbispizza_pcm_stft.h (a header of its own again)
_PCM_STFT_SIGNATURES = [
    ("vpz_stft_table", C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int64]),
    ("vpz_pcm_stft", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(StftSpec), C.c_int32, _vp, _vp, C.c_int64]),
]
PCM_STFT_EXPORTED_SYMBOLS = [s[0] for s in _PCM_STFT_SIGNATURES]


class CqtSpec(C.Structure):
    """vpz_cqt_spec (include/vorbispizza_pcm_cqt.h).  CqtSpec.make(...) takes the names a Python caller uses; its defaults are the music
    spec: 84 bins from C1 (32.70 Hz), 12 to the octave, at 22 050 Hz with a hop of 512."""
    _fields_ = [("sample_rate", C.c_double), ("f_min", C.c_double), ("filter_scale", C.c_double), ("gamma", C.c_double),
                ("n_bins", C.c_int32), ("bins_per_octave", C.c_int32), ("hop", C.c_int32), ("window", C.c_int32), ("scale", C.c_int32),
                ("pad", C.c_int32), ("output", C.c_int32), ("layout", C.c_int32), ("reserved", C.c_int32 * 8)]

    @classmethod
    def make(cls, sample_rate=22050, f_min=32.70319566257483, n_bins=84, bins_per_octave=12, hop=512, filter_scale=1.0, gamma=0.0,
             window="hann", scale="sqrt_length", pad="reflect", output="magnitude", bins_first=True):
        windows = {"hann": CQT_HANN, "hamming": CQT_HAMMING}
        scales = {"none": CQT_SCALE_NONE, "sqrt_length": CQT_SCALE_SQRT_LENGTH}
        pads = {"reflect": CQT_PAD_REFLECT, "zero": CQT_PAD_ZERO}
        outputs = {"complex": CQT_COMPLEX, "magnitude": CQT_MAGNITUDE, "power": CQT_POWER}
        if window not in windows or scale not in scales or pad not in pads or output not in outputs:
            raise ValueError("CqtSpec: window is 'hann' or 'hamming', scale 'none' or 'sqrt_length', pad 'reflect' or 'zero', output "
                             "'complex', 'magnitude' or 'power'")
        s = cls()
        s.sample_rate, s.f_min, s.filter_scale, s.gamma = float(sample_rate), float(f_min), float(filter_scale), float(gamma)
        s.n_bins, s.bins_per_octave, s.hop = int(n_bins), int(bins_per_octave), int(hop)
        s.window, s.scale, s.pad, s.output = windows[window], scales[scale], pads[pad], outputs[output]
        s.layout = CQT_BINS_FIRST if bins_first else CQT_FRAMES_FIRST
        return s

    def n_frames(self, frames):
        """T of a row of `frames` samples."""
        return 1 + int(frames) // self.hop

    def row_shape(self, frames):
        """a row of the destination as float32: (n_bins, T) or (T, n_bins), with a last 2 for the complex output"""
        inner = (self.n_bins, self.n_frames(frames)) if self.layout == CQT_BINS_FIRST else (self.n_frames(frames), self.n_bins)
        return inner + ((2,) if self.output == CQT_COMPLEX else ())


CQT_HANN, CQT_HAMMING = 0, 1
CQT_SCALE_NONE, CQT_SCALE_SQRT_LENGTH = 0, 1
CQT_PAD_REFLECT, CQT_PAD_ZERO = 0, 1
CQT_COMPLEX, CQT_MAGNITUDE, CQT_POWER = 0, 1, 2
CQT_BINS_FIRST, CQT_FRAMES_FIRST = 0, 1
CQT_MAX_BINS, CQT_MAX_BINS_PER_OCTAVE, CQT_MAX_LENGTH, CQT_MAX_HOP = 512, 96, 65536, 2048
# include/vorbispizza_pcm_cqt.h (a header of its own again)
_PCM_CQT_SIGNATURES = [
    ("vpz_cqt_bins", C.c_int, [C.POINTER(CqtSpec), _vp, _vp, C.c_int32]),
    ("vpz_cqt_kernel", C.c_int, [C.POINTER(CqtSpec), C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int32)]),
    ("vpz_pcm_cqt", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(CqtSpec), C.c_int32, _vp, _vp, C.c_int64]),
]
PCM_CQT_EXPORTED_SYMBOLS = [s[0] for s in _PCM_CQT_SIGNATURES]


FLT_EPSILON = 2.0 ** -23  # (Kaldi's floor under the log)


class FbankSpec(C.Structure):
    """vpz_fbank_spec (include/vorbispizza_pcm_fbank.h).  FbankSpec.make(...) takes the names a Python caller uses; its defaults are
    Kaldi's fbank at 16 kHz with 80 bands."""
    _fields_ = [("sample_rate", C.c_double), ("low_freq", C.c_double), ("high_freq", C.c_double), ("preemphasis", C.c_double),
                ("scale", C.c_double), ("floor", C.c_double), ("pad_value", C.c_double),
                ("win", C.c_int32), ("hop", C.c_int32), ("n_fft", C.c_int32), ("n_mels", C.c_int32), ("window", C.c_int32),
                ("remove_dc", C.c_int32), ("output", C.c_int32), ("layout", C.c_int32), ("reserved", C.c_int32 * 10)]

    @classmethod
    def make(cls, sample_rate=16000, win=400, hop=160, n_fft=512, n_mels=80, low_freq=20.0, high_freq=0.0, preemphasis=0.97, window="povey",
             remove_dc=True, scale=32768.0, log=True, floor=FLT_EPSILON, pad_value=0.0, frames_first=True):
        windows = {"hanning": FBANK_HANNING, "hamming": FBANK_HAMMING, "povey": FBANK_POVEY}
        if window not in windows:
            raise ValueError("FbankSpec: window is 'hanning', 'hamming' or 'povey'")
        s = cls()
        s.sample_rate, s.low_freq, s.high_freq, s.preemphasis = float(sample_rate), float(low_freq), float(high_freq), float(preemphasis)
        s.scale, s.floor, s.pad_value = float(scale), float(floor), float(pad_value)
        s.win, s.hop, s.n_fft, s.n_mels = int(win), int(hop), int(n_fft), int(n_mels)
        s.window, s.remove_dc = windows[window], int(bool(remove_dc))
        s.output, s.layout = (FBANK_LOG if log else FBANK_POWER), (FBANK_FRAMES_FIRST if frames_first else FBANK_BANDS_FIRST)
        return s

    def n_frames(self, frames):
        """T of a row of `frames` samples (frames >= win); also T_L of a row's `frames` real samples, 0 below win."""
        return 0 if int(frames) < self.win else 1 + (int(frames) - self.win) // self.hop


FBANK_HANNING, FBANK_HAMMING, FBANK_POVEY = 0, 1, 2
FBANK_POWER, FBANK_LOG = 0, 1
FBANK_BANDS_FIRST, FBANK_FRAMES_FIRST = 0, 1
FBANK_MIN_NFFT, FBANK_MAX_NFFT, FBANK_MAX_MELS = 32, 1024, 256
# include/vorbispizza_pcm_fbank.h (a header of its own again)
_PCM_FBANK_SIGNATURES = [
    ("vpz_fbank_table", C.c_int, [C.POINTER(FbankSpec), _vp, C.c_int64]),
    ("vpz_fbank_filterbank", C.c_int, [C.POINTER(FbankSpec), _vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    ("vpz_pcm_fbank", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(FbankSpec), C.c_int32, _vp, _vp, C.c_int64]),
]
PCM_FBANK_EXPORTED_SYMBOLS = [s[0] for s in _PCM_FBANK_SIGNATURES]


class MfccSpec(C.Structure):
    """vpz_mfcc_spec (include/vorbispizza_pcm_mfcc.h).  MfccSpec.make(...) takes FbankSpec.make's names (but `log`: the mel stage's output
    is the log) and the cepstral stage's; its defaults are Kaldi's mfcc at 16 kHz: 13 cepstra of 23 bands, lifter 22, C0 replaced by the
    log energy."""
    _fields_ = [("fbank", FbankSpec), ("lifter", C.c_double), ("energy_floor", C.c_double), ("n_ceps", C.c_int32), ("use_energy", C.c_int32),
                ("htk_compat", C.c_int32), ("subtract_mean", C.c_int32), ("reserved", C.c_int32 * 12)]

    @classmethod
    def make(cls, sample_rate=16000, win=400, hop=160, n_fft=512, n_mels=23, low_freq=20.0, high_freq=0.0, preemphasis=0.97, window="povey",
             remove_dc=True, scale=32768.0, floor=FLT_EPSILON, pad_value=0.0, frames_first=True, n_ceps=13, lifter=22.0, use_energy=True,
             energy_floor=0.0, htk_compat=False, subtract_mean=False):
        s = cls()
        s.fbank = FbankSpec.make(sample_rate=sample_rate, win=win, hop=hop, n_fft=n_fft, n_mels=n_mels, low_freq=low_freq, high_freq=high_freq,
                                 preemphasis=preemphasis, window=window, remove_dc=remove_dc, scale=scale, log=True, floor=floor,
                                 pad_value=pad_value, frames_first=frames_first)
        s.lifter, s.energy_floor, s.n_ceps = float(lifter), float(energy_floor), int(n_ceps)
        s.use_energy, s.htk_compat, s.subtract_mean = int(bool(use_energy)), int(bool(htk_compat)), int(bool(subtract_mean))
        return s

    def n_frames(self, frames):
        """FbankSpec.n_frames of the mel stage: T of a padded length, T_L of a row's real samples."""
        return self.fbank.n_frames(frames)


# include/vorbispizza_pcm_mfcc.h (a header of its own again)
_PCM_MFCC_SIGNATURES = [
    ("vpz_mfcc_table", C.c_int, [C.POINTER(MfccSpec), _vp, C.c_int64]),
    ("vpz_pcm_mfcc", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(MfccSpec), C.c_int32, _vp, _vp, C.c_int64]),
]
PCM_MFCC_EXPORTED_SYMBOLS = [s[0] for s in _PCM_MFCC_SIGNATURES]


NORM_NONE, NORM_ROW, NORM_SLIDING = 0, 1, 2
POST_NORM_FIRST, POST_DELTAS_FIRST = 0, 1
FEAT_COLUMNS_FIRST, FEAT_FRAMES_FIRST = 0, 1
FEAT_MAX_COLUMNS, FEAT_MAX_DELTA_ORDER, FEAT_MAX_DELTA_WINDOW, FEAT_MAX_CMN_WINDOW, FEAT_CHUNK = 256, 3, 8, 1 << 20, 64


class FeatPostSpec(C.Structure):
    """vpz_feat_post_spec (include/vorbispizza_pcm_featpost.h).  FeatPostSpec.make(...) takes the names a Python caller uses; the window's
    defaults are Kaldi's apply-cmvn-sliding (600, 100), the deltas' add-deltas' window 2."""
    _fields_ = [("var_floor", C.c_double), ("pad_value", C.c_double), ("norm", C.c_int32), ("norm_vars", C.c_int32), ("center", C.c_int32),
                ("cmn_window", C.c_int32), ("min_window", C.c_int32), ("delta_order", C.c_int32), ("delta_window", C.c_int32),
                ("order", C.c_int32), ("layout", C.c_int32), ("reserved", C.c_int32 * 11)]

    @classmethod
    def make(cls, norm="none", norm_vars=False, center=False, cmn_window=600, min_window=100, var_floor=1e-10, delta_order=0, delta_window=2,
             deltas_first=False, pad_value=0.0, frames_first=True):
        norms = {None: NORM_NONE, "none": NORM_NONE, "row": NORM_ROW, "sliding": NORM_SLIDING}
        if norm not in norms:
            raise ValueError("FeatPostSpec: norm is None, 'row' or 'sliding'")
        s = cls()
        s.var_floor, s.pad_value = float(var_floor), float(pad_value)
        s.norm, s.norm_vars, s.center = norms[norm], int(bool(norm_vars)), int(bool(center))
        s.cmn_window, s.min_window, s.delta_order, s.delta_window = int(cmn_window), int(min_window), int(delta_order), int(delta_window)
        s.order = POST_DELTAS_FIRST if deltas_first else POST_NORM_FIRST
        s.layout = FEAT_FRAMES_FIRST if frames_first else FEAT_COLUMNS_FIRST
        return s

    def out_columns(self, D):
        """D_out of D source columns."""
        return int(D) * (self.delta_order + 1)


# include/vorbispizza_pcm_featpost.h (a header of its own again)
_PCM_FEATPOST_SIGNATURES = [
    ("vpz_feat_delta_scales", C.c_int, [C.POINTER(FeatPostSpec), C.c_int32, _vp, C.c_int64]),
    ("vpz_feat_cmn_window", C.c_int, [C.POINTER(FeatPostSpec), C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("vpz_feat_post_scratch", C.c_int, [C.POINTER(FeatPostSpec), C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    ("vpz_feat_post", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int32, C.POINTER(FeatPostSpec), C.c_int32, _vp, _vp, C.c_int64, _vp,
                                C.c_int64]),
]
PCM_FEATPOST_EXPORTED_SYMBOLS = [s[0] for s in _PCM_FEATPOST_SIGNATURES]


NORM_MEANVAR, NORM_PEAK, NORM_RMS, NORM_GAIN = 1, 2, 3, 4
NORM_CHUNK = 1024
NORM_MODES = {"meanvar": NORM_MEANVAR, "peak": NORM_PEAK, "rms": NORM_RMS, "gain": NORM_GAIN}
NORM_DEFAULT_TARGETS = {"meanvar": 0.0, "peak": 1.0, "rms": 0.1, "gain": 1.0, "loudness": -23.0}


class NormSpec(C.Structure):
    """vpz_norm_spec (include/vorbispizza_pcm_normalize.h).  NormSpec.make(...) takes the names a Python caller uses; eps is
    Wav2Vec2FeatureExtractor's 1e-7, target=None the mode's usual level (1.0 for a peak, 0.1 for an RMS level; a gain's is per row)."""
    _fields_ = [("target", C.c_double), ("eps", C.c_double), ("ceiling", C.c_double), ("mode", C.c_int32), ("channels", C.c_int32),
                ("reserved", C.c_int32 * 8)]

    @classmethod
    def make(cls, mode="meanvar", channels=1, target=None, eps=1e-7, ceiling=0.0):
        if mode not in NORM_MODES:
            raise ValueError("NormSpec: mode is 'meanvar', 'peak', 'rms' or 'gain'")
        s = cls()
        s.mode, s.channels = NORM_MODES[mode], int(channels)
        s.target = float(NORM_DEFAULT_TARGETS[mode] if target is None else target)
        s.eps, s.ceiling = float(eps), float(ceiling)
        return s


class NormRow(C.Structure):
    """vpz_norm_row"""
    _fields_ = [("src", C.c_int64), ("samples", C.c_int64), ("row", C.c_int64), ("gain", C.c_double)]


NORM_RESULT_FIELDS = ("sum", "sum_sq", "peak", "mean", "gain")  # vpz_norm_result: five doubles
# include/vorbispizza_pcm_normalize.h (a header of its own again)
_PCM_NORMALIZE_SIGNATURES = [
    ("vpz_pcm_normalize_scratch", C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    ("vpz_pcm_normalize", C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(NormSpec), C.c_int32, _vp, _vp, C.c_int64, C.c_int32, _vp,
                                    C.c_int64, _vp]),
]
PCM_NORMALIZE_EXPORTED_SYMBOLS = [s[0] for s in _PCM_NORMALIZE_SIGNATURES]
LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE = 8000, 384000
# include/vorbispizza_pcm_loudness.h (a header of its own again)
_PCM_LOUDNESS_SIGNATURES = [
    ("vpz_loudness_filter", C.c_int, [C.c_int32, _vp]),
    ("vpz_loudness_weights", C.c_int, [C.c_int32, _vp]),
    ("vpz_pcm_loudness", C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, C.c_int64, C.c_int64]),
    ("vpz_loudness_gate", C.c_int, [_vp, C.c_int64, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
]
PCM_LOUDNESS_EXPORTED_SYMBOLS = [s[0] for s in _PCM_LOUDNESS_SIGNATURES]
TRUE_PEAK_TAPS, TRUE_PEAK_MAX_COEFFS = 12, 49
# include/vorbispizza_pcm_r128.h (a header of its own again)
_PCM_R128_SIGNATURES = [
    ("vpz_true_peak_filter", C.c_int, [C.c_int32, _vp, _vp]),
    ("vpz_pcm_true_peak", C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int64]),
    ("vpz_loudness_range", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, _vp, _vp, _vp]),
    ("vpz_loudness_maxima", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, _vp]),
]
PCM_R128_EXPORTED_SYMBOLS = [s[0] for s in _PCM_R128_SIGNATURES]
EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]
PCM_EXPORTED_SYMBOLS = [s[0] for s in _PCM_SIGNATURES]
PCM_PACK_EXPORTED_SYMBOLS = [s[0] for s in _PCM_PACK_SIGNATURES]
PCM_RESAMPLE_EXPORTED_SYMBOLS = [s[0] for s in _PCM_RESAMPLE_SIGNATURES]
DEBUG_SYMBOLS = [s[0] for s in _DEBUG_SIGNATURES]

_lib = None


class SynthError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        name = lib().vpz_error_string(status).decode()
        super().__init__("vorbispizza_synth: %s (%d)%s" % (name, status, (": " + detail) if detail else ""))


def lib():
    """Load libvorbispizza_synth.so (built in-tree by vorbispizza_amd._build.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libvorbispizza_synth.so is not built: run `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64,
        # and a second copy initialised later finds no device.  Importing torch first makes the
        # loader bind this library's NEEDED libamdhip64.so.7 to the copy torch already loaded.
        if not os.environ.get("VPZ_NO_TORCH"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        later = (_PCM_SIGNATURES + _PCM_PACK_SIGNATURES + _PCM_RESAMPLE_SIGNATURES + _PCM_LOGMEL_SIGNATURES + _PCM_FBANK_SIGNATURES
                 + _PCM_LOUDNESS_SIGNATURES + _PCM_R128_SIGNATURES + _PCM_MFCC_SIGNATURES + _PCM_FEATPOST_SIGNATURES + _PCM_MELSPEC_SIGNATURES
                 + _PCM_STFT_SIGNATURES + _PCM_CQT_SIGNATURES + _PCM_NORMALIZE_SIGNATURES)
        for name, restype, argtypes in _SIGNATURES + _DEBUG_SIGNATURES + later:
            if (name, restype, argtypes) in later and not hasattr(L, name):
                continue  # (an older build taken through VPZ_LIB_DIR for an A/B run has none: using one raises)
            fn = getattr(L, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = L
    return _lib


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _sync_producer(*tensors):
    """The C ABI orders work only on the context's own HIP stream.  Tensors produced on torch's
    current stream must be complete before the library reads them, so wait for that stream here."""
    for t in tensors:
        if t is not None and _is_torch(t) and t.is_cuda:
            import torch
            torch.cuda.current_stream(t.device).synchronize()
            return


def _numel(x):
    if x is None:
        return 0
    return int(x.numel()) if _is_torch(x) else int(np.asarray(x).size)


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ctypes.data)


class Context:
    """vpz_context: one GPU, one HIP stream, the per-block-size tables."""

    def __init__(self, device=0):
        self._h = _vp()
        rc = lib().vpz_context_create(device, C.byref(self._h))
        if rc != OK:
            self._h = None
            raise SynthError(rc, "vpz_context_create(device=%d)" % device)
        self.device = device
        self._children = []  # weak references to decoders: they must be destroyed before the context

    def _check(self, rc):
        if rc != OK:
            raise SynthError(rc, lib().vpz_context_last_error(self._h).decode())

    def close(self):
        if self._h:
            for ref in self._children:
                child = ref()
                if child is not None:
                    child.close()
            self._children = []
            lib().vpz_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        """Text of the last failure on this context (what the C# host would put into its exception)."""
        return lib().vpz_context_last_error(self._h).decode()

    def synchronize(self):
        self._check(lib().vpz_context_synchronize(self._h))

    @property
    def stream(self):
        return lib().vpz_context_stream(self._h)

    def timer_start(self):
        self._check(lib().vpz_context_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        self._check(lib().vpz_context_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def imdct_batch(self, spectra, n, mode=IMDCT_FAST, out=None):
        """`Mdct.Reverse` (Mdct.cs:15-19) per row.  numpy in -> numpy out (host memory, synchronous);
        torch cuda tensor in -> torch cuda tensor out (device memory, asynchronous on the context stream)."""
        half = max(n // 2, 1)
        if _is_torch(spectra):
            import torch
            assert spectra.is_cuda and spectra.dtype == torch.float32 and spectra.is_contiguous()
            count = spectra.numel() // half
            if out is None:
                out = torch.empty((count, n), dtype=torch.float32, device=spectra.device)
            _sync_producer(spectra)
            self._check(lib().vpz_imdct_batch(self._h, n, count, _ptr(spectra), _ptr(out), MEM_DEVICE, mode))
            return out
        spectra = np.ascontiguousarray(spectra, dtype=np.float32).reshape(-1, half)
        count = spectra.shape[0]
        if out is None:
            out = np.empty((count, n), dtype=np.float32)
        self._check(lib().vpz_imdct_batch(self._h, n, count, _ptr(spectra), _ptr(out), MEM_HOST, mode))
        return out


def pcm_pack(ctx, src, rows, dst, layout):
    """vpz_pcm_pack (vorbispizza_pcm_pack.h): windows of the device array `src` (a torch tensor, interleaved [sample][channel], float32 or
    int16) into rows of `dst`, a contiguous torch tensor [rows, channels, frames] (OUT_PLANAR / OUT_PLANAR_S16) or [rows, frames, channels]
    (the interleaved layouts); rows: [(src, samples, row)].  Asynchronous on the context's stream; returns the status (OK or
    E_INVALID_ARG and the like: a refusal is an answer here, not an exception)."""
    planar = layout in (OUT_PLANAR, OUT_PLANAR_S16)
    dst_rows, channels, frames = (dst.shape[0], dst.shape[1], dst.shape[2]) if planar else (dst.shape[0], dst.shape[2], dst.shape[1])
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    _sync_producer(src, dst)
    return lib().vpz_pcm_pack(ctx._h, _ptr(src), _numel(src), channels, desc.shape[0], desc.ctypes.data, _ptr(dst), dst_rows, frames, layout)


def pcm_resample(ctx, src, rows, dst, layout, up, down, downmix=False):
    """vpz_pcm_resample (vorbispizza_pcm_resample.h): windows of the device array `src` (a float32 torch tensor, interleaved
    [sample][channel] with `src.shape[-1]` channels) resampled by up / down, mixed down to mono with `downmix`, into rows of `dst` -- a
    contiguous torch tensor [rows, out_channels, frames] (planar layouts) or [rows, frames, out_channels], float32 or int16; rows:
    [(src, samples, row)].  Asynchronous on the context's stream; returns the status (a refusal is an answer, not an exception)."""
    planar = layout in (OUT_PLANAR, OUT_PLANAR_S16)
    dst_rows, out_channels, frames = (dst.shape[0], dst.shape[1], dst.shape[2]) if planar else (dst.shape[0], dst.shape[2], dst.shape[1])
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    _sync_producer(src, dst)
    return lib().vpz_pcm_resample(ctx._h, _ptr(src), _numel(src), int(src.shape[-1]), up, down, int(bool(downmix)), desc.shape[0], desc.ctypes.data,
                                  _ptr(dst), dst_rows, out_channels, frames, layout)


def resample_filter(up, down):
    """vpz_resample_filter: (taps, first_tap[up] int32, coeffs[up, taps] float32) of a ratio in lowest terms; needs no device.  A refused
    ratio raises ValueError."""
    taps = C.c_int32(0)
    first = np.zeros(max(int(up), 1), dtype=np.int32)
    rc = lib().vpz_resample_filter(up, down, C.byref(taps), first.ctypes.data, None, 0)
    if rc != OK:
        raise ValueError("vpz_resample_filter refuses the ratio %d / %d (status %d)" % (up, down, rc))
    coeffs = np.zeros((int(up), taps.value), dtype=np.float32)
    rc = lib().vpz_resample_filter(up, down, C.byref(taps), first.ctypes.data, coeffs.ctypes.data, coeffs.size)
    if rc != OK:
        raise ValueError("vpz_resample_filter failed (status %d)" % rc)
    return taps.value, first, coeffs


def _pcm_feature(fn, ctx, src, rows, dst, spec, frames):
    """a feature launch (vpz_pcm_logmel and its kin have one argument list): rows [(src, samples, row)] of `src` into rows of `dst`"""
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    _sync_producer(src, dst)
    return fn(ctx._h, _ptr(src), _numel(src), int(frames), C.byref(spec), desc.shape[0], desc.ctypes.data, _ptr(dst), int(dst.shape[0]))


def _table_of(fn, name, head, shape, what):
    """a float32 table of the library's: fn(*head, None, 0) says whether it exists (no: ValueError, "<name> refuses <what>"), then
    fn(*head, table, size) fills one of shape() -- worked out behind the refusal"""
    rc = fn(*head, None, 0)
    if rc != OK:
        raise ValueError("%s refuses %s (status %d)" % (name, what, rc))
    table = np.zeros(shape(), dtype=np.float32)
    rc = fn(*head, table.ctypes.data, table.size)
    if rc != OK:
        raise ValueError("%s failed (status %d)" % (name, rc))
    return table


def pcm_logmel(ctx, src, rows, dst, spec, frames):
    """vpz_pcm_logmel (vorbispizza_pcm_logmel.h): windows of the MONO float32 device array `src` (a torch tensor) as (log-)mel frames of
    rows padded to `frames` samples, into rows of `dst` -- a contiguous float32 torch tensor [rows, n_mels, T] (MEL_BANDS_FIRST) or
    [rows, T, n_mels], T = 1 + frames // hop; rows: [(src, samples, row)]; spec: a LogMelSpec.  Asynchronous on the context's stream;
    returns the status (a refusal is an answer, not an exception)."""
    return _pcm_feature(lib().vpz_pcm_logmel, ctx, src, rows, dst, spec, frames)


def logmel_dft_table(n_fft):
    """vpz_logmel_dft_table: float32 [n_fft, 2, n_fft // 2 + 1] -- [m, 0, k] = w[m] cos, [m, 1, k] = w[m] sin; needs no device.  A refused
    n_fft raises ValueError."""
    return _table_of(lib().vpz_logmel_dft_table, "vpz_logmel_dft_table", (n_fft,), lambda: (int(n_fft), 2, int(n_fft) // 2 + 1), "n_fft %r" % (n_fft,))


def mel_filterbank(spec):
    """vpz_mel_filterbank: (first_bin[n_mels] int32, n_bins[n_mels] int32, weights float32 -- band after band, each band's live bins) of a
    LogMelSpec; needs no device.  A refused spec raises ValueError."""
    return _mel_filterbank_of(lib().vpz_mel_filterbank, "vpz_mel_filterbank", spec)


def _mel_filterbank_of(fn, name, spec):
    total = C.c_int64(0)
    rc = fn(C.byref(spec), None, None, None, 0, C.byref(total))
    if rc != OK:
        raise ValueError("%s refuses the spec (status %d)" % (name, rc))
    first, count = np.zeros(spec.n_mels, dtype=np.int32), np.zeros(spec.n_mels, dtype=np.int32)
    weights = np.zeros(total.value, dtype=np.float32)
    rc = fn(C.byref(spec), first.ctypes.data, count.ctypes.data, weights.ctypes.data if total.value else None, weights.size, C.byref(total))
    if rc != OK:
        raise ValueError("%s failed (status %d)" % (name, rc))
    return first, count, weights


def pcm_melspec(ctx, src, rows, dst, spec, frames):
    """vpz_pcm_melspec (vorbispizza_pcm_melspec.h): pcm_logmel's arguments and shapes, for a LogMelSpec with n_fft 2048, 4096 or 8192 (a
    real FFT per frame, held to the header's bound).  Asynchronous on the context's stream; returns the status (a refusal is an answer,
    not an exception)."""
    return _pcm_feature(lib().vpz_pcm_melspec, ctx, src, rows, dst, spec, frames)


def melspec_twiddles(n_fft):
    """vpz_melspec_twiddles: (w float32 [n_fft], t float32 [n_fft, 2]) -- the periodic Hann window and t[k] = (cos, -sin)(2 pi k / n_fft),
    two views of the one table of 3 * n_fft floats the kernel reads; needs no device.  A refused n_fft raises ValueError."""
    table = _table_of(lib().vpz_melspec_twiddles, "vpz_melspec_twiddles", (n_fft,), lambda: 3 * int(n_fft), "n_fft %r" % (n_fft,))
    return table[:int(n_fft)], table[int(n_fft):].reshape(int(n_fft), 2)


def melspec_filterbank(spec):
    """vpz_melspec_filterbank: mel_filterbank's outputs for a LogMelSpec with n_fft 2048, 4096 or 8192; needs no device.  A refused spec
    raises ValueError."""
    return _mel_filterbank_of(lib().vpz_melspec_filterbank, "vpz_melspec_filterbank", spec)


def pcm_stft(ctx, src, rows, dst, spec, frames):
    """vpz_pcm_stft (vorbispizza_pcm_stft.h): windows of the float32 device array `src` (a torch tensor; a channel of a planar array is
    a row) as short-time Fourier spectrograms of rows padded to `frames` samples, into rows of `dst` -- a contiguous torch tensor whose
    first dimension counts the rows: float32 [rows, n_freq, T] (bins first) or [rows, T, n_freq], with a last dimension of 2 for the
    complex output (or the complex64 tensor torch.view_as_complex gives of it).  rows: [(src element offset, samples, destination row)].
    Asynchronous on the context's stream; returns the status (a refusal is an answer, not an exception)."""
    return _pcm_feature(lib().vpz_pcm_stft, ctx, src, rows, dst, spec, frames)


def stft_table(n_fft, win_length=None, window="hann"):
    """vpz_stft_table: (w float32 [n_fft], t float32 [n_fft, 2]) -- the window of win_length centred in n_fft and t[k] = (cos, -sin)(2 pi k
    / n_fft), two views of the one table of 3 * n_fft floats the kernel reads; needs no device.  window: 'hann' / 'hamming' or the
    VPZ_STFT_* value.  Refused arguments raise ValueError."""
    wl = int(n_fft if win_length is None else win_length)
    wd = {"hann": STFT_HANN, "hamming": STFT_HAMMING}.get(window, window)
    table = _table_of(lib().vpz_stft_table, "vpz_stft_table", (int(n_fft), wl, int(wd)), lambda: 3 * int(n_fft),
                      "n_fft %r, win_length %r, window %r" % (n_fft, win_length, window))
    return table[:int(n_fft)], table[int(n_fft):].reshape(int(n_fft), 2)


def pcm_cqt(ctx, src, rows, dst, spec, frames):
    """vpz_pcm_cqt (vorbispizza_pcm_cqt.h): windows of the float32 device array `src` (a torch tensor; a channel of a planar array is a
    row) as constant-Q spectrograms of rows padded to `frames` samples, into rows of `dst` -- a contiguous torch tensor whose first
    dimension counts the rows: float32 [rows, n_bins, T] (bins first) or [rows, T, n_bins], with a last dimension of 2 for the complex
    output.  rows: [(src element offset, samples, destination row)]; spec: a CqtSpec.  Asynchronous on the context's stream; returns the
    status (a refusal is an answer, not an exception)."""
    return _pcm_feature(lib().vpz_pcm_cqt, ctx, src, rows, dst, spec, frames)


def cqt_bins(spec):
    """vpz_cqt_bins: (f_k float64 [n_bins], N_k int32 [n_bins]) of a CqtSpec; needs no device.  A spec outside the limits raises
    ValueError."""
    n = max(0, int(spec.n_bins))
    freqs, lengths = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int32)
    rc = lib().vpz_cqt_bins(C.byref(spec), freqs.ctypes.data, lengths.ctypes.data, n)
    if rc != OK:
        raise ValueError("vpz_cqt_bins refuses the spec (status %d)" % rc)
    return freqs, lengths


def cqt_kernel(spec, k):
    """vpz_cqt_kernel: (hr_k, hi_k), float32 [N_k] each -- bin k's coefficients as the kernel multiplies them; needs no device.  A spec
    outside the limits or a k outside the bins raises ValueError."""
    n = C.c_int32(0)
    rc = lib().vpz_cqt_kernel(C.byref(spec), int(k), None, 0, C.byref(n))
    if rc != OK:
        raise ValueError("vpz_cqt_kernel refuses the spec or bin %r (status %d)" % (k, rc))
    table = np.zeros(2 * n.value, dtype=np.float32)
    rc = lib().vpz_cqt_kernel(C.byref(spec), int(k), table.ctypes.data, table.size, None)
    if rc != OK:
        raise ValueError("vpz_cqt_kernel failed (status %d)" % rc)
    return table[:n.value], table[n.value:]


def pcm_fbank(ctx, src, rows, dst, spec, frames):
    """vpz_pcm_fbank (vorbispizza_pcm_fbank.h): windows of the MONO float32 device array `src` (a torch tensor) as Kaldi filterbank
    frames of rows padded to `frames` samples, into rows of `dst` -- a contiguous float32 torch tensor [rows, T, n_mels]
    (FBANK_FRAMES_FIRST) or [rows, n_mels, T], T = 1 + (frames - win) // hop; rows: [(src, samples, row)]; spec: an FbankSpec.
    Asynchronous on the context's stream; returns the status (a refusal is an answer, not an exception)."""
    return _pcm_feature(lib().vpz_pcm_fbank, ctx, src, rows, dst, spec, frames)


def fbank_table(spec):
    """vpz_fbank_table: float32 [win, 2, n_fft // 2] -- [m, 0, k] the coefficient of x[m] - mu in re[k], [m, 1, k] in im[k]; needs no
    device.  A refused spec raises ValueError."""
    return _table_of(lib().vpz_fbank_table, "vpz_fbank_table", (C.byref(spec),), lambda: (int(spec.win), 2, int(spec.n_fft) // 2), "the spec")


def fbank_filterbank(spec):
    """vpz_fbank_filterbank: (first_bin[n_mels] int32, n_bins[n_mels] int32, weights float32 -- band after band, each band's live bins)
    of an FbankSpec; needs no device.  A refused spec raises ValueError."""
    return _mel_filterbank_of(lib().vpz_fbank_filterbank, "vpz_fbank_filterbank", spec)


def pcm_mfcc(ctx, src, rows, dst, spec, frames):
    """vpz_pcm_mfcc (vorbispizza_pcm_mfcc.h): windows of the MONO float32 device array `src` (a torch tensor) as Kaldi MFCC frames of
    rows padded to `frames` samples, into rows of `dst` -- a contiguous float32 torch tensor [rows, T, n_ceps] (FBANK_FRAMES_FIRST) or
    [rows, n_ceps, T], T = 1 + (frames - win) // hop; rows: [(src, samples, row)]; spec: an MfccSpec.
    Asynchronous on the context's stream; returns the status (a refusal is an answer, not an exception)."""
    return _pcm_feature(lib().vpz_pcm_mfcc, ctx, src, rows, dst, spec, frames)


def mfcc_table(spec):
    """vpz_mfcc_table: float32 [n_ceps, n_mels], row j the weights of the log-mel values in a frame's j-th STORED value; needs no device.
    A refused spec raises ValueError."""
    return _table_of(lib().vpz_mfcc_table, "vpz_mfcc_table", (C.byref(spec),), lambda: (int(spec.n_ceps), int(spec.fbank.n_mels)), "the spec")


def feat_delta_scales(spec, i):
    """vpz_feat_delta_scales: float32 [2 i w + 1], the scales s_i of a FeatPostSpec's deltas (index j + i w); needs no device.  A refused
    spec or order raises ValueError."""
    rc = lib().vpz_feat_delta_scales(C.byref(spec), i, None, 0)
    if rc != OK:
        raise ValueError("vpz_feat_delta_scales refuses the spec or the order %r (status %d)" % (i, rc))
    scales = np.zeros(2 * int(i) * int(spec.delta_window) + 1, dtype=np.float32)
    rc = lib().vpz_feat_delta_scales(C.byref(spec), i, scales.ctypes.data, scales.size)
    if rc != OK:
        raise ValueError("vpz_feat_delta_scales failed (status %d)" % rc)
    return scales


def feat_cmn_window(spec, t, n):
    """vpz_feat_cmn_window: (a, b), the frames [a, b) that frame t of a row of n real frames is normalised over; needs no device.  A refused
    spec, t or n raises ValueError."""
    a, b = C.c_int64(0), C.c_int64(0)
    rc = lib().vpz_feat_cmn_window(C.byref(spec), t, n, C.byref(a), C.byref(b))
    if rc != OK:
        raise ValueError("vpz_feat_cmn_window refuses the spec, t = %r or n = %r (status %d)" % (t, n, rc))
    return a.value, b.value


def feat_post_scratch(spec, n_rows, T, D):
    """vpz_feat_post_scratch: the float64 elements of scratch memory a call needs; needs no device.  A refusal raises ValueError."""
    elems = C.c_int64(0)
    rc = lib().vpz_feat_post_scratch(C.byref(spec), n_rows, T, D, C.byref(elems))
    if rc != OK:
        raise ValueError("vpz_feat_post_scratch refuses the spec or the sizes (status %d)" % rc)
    return elems.value


def feat_post(ctx, src, rows, dst, spec, scratch=None):
    """vpz_feat_post (vorbispizza_pcm_featpost.h): deltas and mean / variance normalisation of rows of the float32 device tensor `src` --
    contiguous, [src_rows, T, D] (FEAT_FRAMES_FIRST) or [src_rows, D, T]: MFCC, filterbank or log-mel frames alike -- into rows of `dst`,
    [dst_rows, T, D_out] or [dst_rows, D_out, T]; rows: [(src_row, real_frames, row)]; spec: a FeatPostSpec.  scratch: a float64 device
    tensor of feat_post_scratch(...) elements, which the caller keeps until the context's stream has passed the call; None: one is made
    here and the call waits for the stream before it returns.  Otherwise asynchronous on the context's stream; returns the status (a
    refusal is an answer, not an exception)."""
    ff = spec.layout == FEAT_FRAMES_FIRST
    if src.dim() != 3 or dst.dim() != 3:
        raise ValueError("feat_post: src and dst have three dimensions")
    T, D = (int(src.shape[1]), int(src.shape[2])) if ff else (int(src.shape[2]), int(src.shape[1]))
    D_out = D * (max(int(spec.delta_order), 0) + 1)
    want = (T, D_out) if ff else (D_out, T)
    if tuple(dst.shape[1:]) != want:
        raise ValueError("feat_post: dst is [rows, %d, %d], not %r" % (want + (tuple(dst.shape),)))
    for x in (src, dst):
        if str(x.dtype) != "torch.float32" or not x.is_contiguous():
            raise ValueError("feat_post: src and dst are contiguous float32 tensors")
    desc =np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    own = None
    if scratch is None:
        need = C.c_int64(0)
        if lib().vpz_feat_post_scratch(C.byref(spec), desc.shape[0], T, D, C.byref(need)) == OK and need.value:
            import torch
            own = scratch = torch.empty(need.value, dtype=torch.float64, device=src.device)
    _sync_producer(src, dst)
    rc = lib().vpz_feat_post(ctx._h, _ptr(src), int(src.shape[0]), T, D, C.byref(spec), desc.shape[0], desc.ctypes.data, _ptr(dst),
                             int(dst.shape[0]), _ptr(scratch), _numel(scratch))
    if own is not None:
        ctx.synchronize()
    return rc


def pcm_normalize_scratch(n_rows, channels, frames):
    """vpz_pcm_normalize_scratch: the float64 elements of scratch memory a call needs; needs no device.  A refusal raises ValueError."""
    doubles = C.c_int64(0)
    rc = lib().vpz_pcm_normalize_scratch(n_rows, channels, frames, C.byref(doubles))
    if rc != OK:
        raise ValueError("vpz_pcm_normalize_scratch refuses the sizes (status %d)" % rc)
    return doubles.value


def pcm_normalize(ctx, src, rows, dst, spec, frames, gains=None, results=False):
    """vpz_pcm_normalize (vorbispizza_pcm_normalize.h): windows of the PLANAR float32 device array `src` (a torch tensor; a window's
    channel c lies c * frames elements behind its channel 0) normalised into rows of `dst` -- a contiguous torch tensor
    [rows, channels, frames] or [rows, frames, channels], float32 or int16: the layout is read off dst's dtype and shape against
    spec.channels and `frames` (planar where both fit).  rows: [(src, samples, row)]; gains: one linear gain per row (NORM_GAIN;
    None: 1.0); spec: a NormSpec.  The scratch memory is made here, so the call waits for the context's stream before it returns.
    Returns the status (a refusal is an answer, not an exception); with `results`, (status, float64 array [n_rows, 5] of
    NORM_RESULT_FIELDS), the array None after a refusal."""
    import torch
    channels, frames = int(spec.channels), int(frames)
    if dst.dim() != 3 or not dst.is_contiguous():
        raise ValueError("pcm_normalize: dst is a contiguous tensor of three dimensions")
    planar = tuple(dst.shape[1:]) == (channels, frames)
    if not planar and tuple(dst.shape[1:]) != (frames, channels):
        raise ValueError("pcm_normalize: dst is [rows, %d, %d] or [rows, %d, %d], not %r" % (channels, frames, frames, channels, tuple(dst.shape)))
    s16 = dst.dtype == torch.int16
    if not s16 and dst.dtype != torch.float32:
        raise ValueError("pcm_normalize: dst is float32 or int16")
    layout = (OUT_PLANAR_S16 if s16 else OUT_PLANAR) if planar else (OUT_INTERLEAVED_S16 if s16 else OUT_INTERLEAVED)
    desc3 = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    n = desc3.shape[0]
    desc = np.zeros(n, dtype=[("src", "<i8"), ("samples", "<i8"), ("row", "<i8"), ("gain", "<f8")])
    desc["src"], desc["samples"], desc["row"] = desc3[:, 0], desc3[:, 1], desc3[:, 2]
    desc["gain"] = 1.0 if gains is None else np.asarray(gains, dtype=np.float64).reshape(n)
    scratch = None
    need = C.c_int64(0)
    if lib().vpz_pcm_normalize_scratch(n, channels, frames, C.byref(need)) == OK and need.value:
        scratch = torch.empty(need.value, dtype=torch.float64, device=src.device)
    res = torch.zeros((n, len(NORM_RESULT_FIELDS)), dtype=torch.float64, device=src.device) if results else None
    _sync_producer(src, dst)
    rc = lib().vpz_pcm_normalize(ctx._h, _ptr(src), _numel(src), frames, C.byref(spec), n, desc.ctypes.data, _ptr(dst), int(dst.shape[0]),
                                 layout, _ptr(scratch), _numel(scratch), _ptr(res))
    ctx.synchronize()
    if not results:
        return rc
    return rc, (res.cpu().numpy() if rc == OK else None)


def loudness_filter(sample_rate):
    """vpz_loudness_filter: the K-weighting filter of a whole sample rate as float64 [2, 5] -- b0 b1 b2 a1 a2 of the shelf, then of the
    high-pass (include/vorbispizza_pcm_loudness.h states them); needs no device.  A refused rate raises ValueError."""
    coeffs = np.zeros((2, 5), dtype=np.float64)
    rc = lib().vpz_loudness_filter(int(sample_rate), coeffs.ctypes.data)
    if rc != OK:
        raise ValueError("vpz_loudness_filter refuses the rate (status %d)" % rc)
    return coeffs


def loudness_step(sample_rate):
    """the 100 ms step of the header in samples: S = (fs + 5) / 10 in integers"""
    return (int(sample_rate) + 5) // 10


def loudness_weights(channels):
    """vpz_loudness_weights: BS.1770-4's channel weights in Vorbis channel order, float64 [channels]; needs no device."""
    w = np.zeros(max(int(channels), 0), dtype=np.float64)
    rc = lib().vpz_loudness_weights(int(channels), w.ctypes.data if w.size else None)
    if rc != OK:
        raise ValueError("vpz_loudness_weights refuses the channel count (status %d)" % rc)
    return w


def loudness_gate(sums, step_len):
    """vpz_loudness_gate: (integrated LUFS, blocks kept) of the step sums of steps of `step_len` samples -- (-inf, 0) with fewer than
    four steps or nothing kept; needs no device."""
    sums = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1)
    lufs, kept = C.c_double(0.0), C.c_int64(0)
    rc = lib().vpz_loudness_gate(sums.ctypes.data if sums.size else None, sums.size, int(step_len), C.byref(lufs), C.byref(kept))
    if rc != OK:
        raise ValueError("vpz_loudness_gate refuses its arguments (status %d)" % rc)
    return lufs.value, kept.value


def pcm_loudness(ctx, src, channels, sample_rate, rows, weights=None, max_steps=None, out=None):
    """vpz_pcm_loudness (vorbispizza_pcm_loudness.h): windows of the interleaved float32 device array `src` (a torch tensor) as
    K-weighted step sums and sample peaks.  rows: [(src, samples, row)]; weights: per channel, loudness_weights(channels) by default;
    max_steps: the row length of the sums, by default the rows' largest count of whole steps (at least 1).
    -> (sums, peak): float64 [dst_rows, max_steps] and float32 [dst_rows] device tensors, dst_rows one more than the largest row named;
    out: a caller's (sums, peak) instead, whose unnamed rows stay as they are.  Asynchronous on the context's stream
    (ctx.synchronize()).  A refusal raises SynthError with nothing launched."""
    import torch
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    w = np.ascontiguousarray(loudness_weights(channels) if weights is None else weights, dtype=np.float64)
    if w.shape != (int(channels),):
        raise ValueError("pcm_loudness: one weight per channel")
    if max_steps is None:
        max_steps = max([1] + [int(s) // loudness_step(sample_rate) for s in desc[:, 1]])
    if out is None:
        dst_rows = int(desc[:, 2].max()) + 1 if desc.shape[0] else 0
        out = (torch.zeros((dst_rows, int(max_steps)), dtype=torch.float64, device=src.device),
               torch.zeros((dst_rows,), dtype=torch.float32, device=src.device))
    sums, peak = out
    _sync_producer(src, sums, peak)
    rc = lib().vpz_pcm_loudness(ctx._h, _ptr(src), _numel(src), int(channels), int(sample_rate), w.ctypes.data, desc.shape[0], desc.ctypes.data,
                                _ptr(sums), _ptr(peak), int(peak.shape[0]), int(max_steps))
    if rc != OK:
        raise SynthError(rc, ctx.last_error() if hasattr(ctx, "last_error") else "vpz_pcm_loudness")
    return sums, peak


def true_peak_filter(sample_rate):
    """vpz_true_peak_filter: (F, h) -- the oversampling factor of a whole sample rate and its interpolator as float64 [12 F + 1]
    (include/vorbispizza_pcm_r128.h states both); needs no device.  A refused rate raises ValueError."""
    h = np.zeros(TRUE_PEAK_MAX_COEFFS, dtype=np.float64)
    factor = C.c_int32(0)
    rc = lib().vpz_true_peak_filter(int(sample_rate), C.addressof(factor), h.ctypes.data)
    if rc != OK:
        raise ValueError("vpz_true_peak_filter refuses the rate (status %d)" % rc)
    assert not h[TRUE_PEAK_TAPS * factor.value + 1:].any()
    return factor.value, h[: TRUE_PEAK_TAPS * factor.value + 1].copy()


def loudness_range(sums, step_len):
    """vpz_loudness_range: (range in LU, low LUFS, high LUFS, 3 s blocks kept) of the step sums of steps of `step_len` samples --
    (0, -inf, -inf, 0) with fewer than thirty steps or nothing kept; needs no device."""
    sums = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1)
    rng, low, high, kept = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
    rc = lib().vpz_loudness_range(sums.ctypes.data if sums.size else None, sums.size, int(step_len), C.addressof(rng), C.addressof(low), C.addressof(high),
                                  C.addressof(kept))
    if rc != OK:
        raise ValueError("vpz_loudness_range refuses its arguments (status %d)" % rc)
    return rng.value, low.value, high.value, kept.value


def loudness_maxima(sums, step_len):
    """vpz_loudness_maxima: (maximum momentary, maximum short-term loudness) in LUFS of the step sums -- -inf where there is no block or
    no finite level; needs no device."""
    sums = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1)
    momentary, short_term = C.c_double(0.0), C.c_double(0.0)
    rc = lib().vpz_loudness_maxima(sums.ctypes.data if sums.size else None, sums.size, int(step_len), C.addressof(momentary), C.addressof(short_term))
    if rc != OK:
        raise ValueError("vpz_loudness_maxima refuses its arguments (status %d)" % rc)
    return momentary.value, short_term.value


def pcm_true_peak(ctx, src, channels, sample_rate, rows, out=None):
    """vpz_pcm_true_peak (vorbispizza_pcm_r128.h): the true peak and the sample peak of windows of the interleaved float32 device array
    `src` (a torch tensor).  rows: [(src, samples, row)].
    -> (true_peak, sample_peak): float32 [dst_rows] device tensors, dst_rows one more than the largest row named; out: a caller's
    (true_peak, sample_peak) instead -- sample_peak may be None --, whose unnamed rows stay as they are.  Asynchronous on the context's
    stream (ctx.synchronize()).  A refusal raises SynthError with nothing launched."""
    import torch
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    if out is None:
        dst_rows = int(desc[:, 2].max()) + 1 if desc.shape[0] else 0
        out = (torch.zeros((dst_rows,), dtype=torch.float32, device=src.device), torch.zeros((dst_rows,), dtype=torch.float32, device=src.device))
    true_peak, sample_peak = out
    _sync_producer(*[t for t in (src, true_peak, sample_peak) if t is not None])
    rc = lib().vpz_pcm_true_peak(ctx._h, _ptr(src), _numel(src), int(channels), int(sample_rate), desc.shape[0], desc.ctypes.data, _ptr(true_peak),
                                 None if sample_peak is None else _ptr(sample_peak), int(true_peak.shape[0]))
    if rc != OK:
        raise SynthError(rc, ctx.last_error() if hasattr(ctx, "last_error") else "vpz_pcm_true_peak")
    return true_peak, sample_peak


def make_packets(count):
    return np.zeros(count, dtype=PACKET_DTYPE)


class Decoder:
    """vpz_decoder: synthesis state of `n_streams` streams that share one setup header."""

    def __init__(self, ctx, channels, block_size0, block_size1, floors=(), mappings=(), n_streams=1,
                 clip_samples=False):
        """floors: [(x_list, multiplier)] for a type-1 floor or {"order":, "rate":, "bark_map_size":, "amp_bits":,
        "amp_ofs":} for a type-0 floor; mappings: [{"coupling": [(mag, ang)], "channel_floor": [..],
        "residue_begin": (short, long), "residue_end": (short, long)}] -- the last two optional (ABI v4: the residue's
        support in bins per channel; 0 / absent = the whole block)"""
        self.ctx = ctx
        self.channels, self.size0, self.size1, self.n_streams = channels, block_size0, block_size1, n_streams
        fl = (Floor1Config * max(1, len(floors)))()
        ftypes = (C.c_uint8 * max(1, len(floors)))()
        fl0 = (Floor0Config * max(1, len(floors)))()
        for i, f in enumerate(floors):
            if isinstance(f, dict):
                ftypes[i] = 0
                fl0[i] = Floor0Config(f["order"], f["rate"], f["bark_map_size"], f["amp_bits"], f["amp_ofs"])
                continue
            ftypes[i] = 1
            xl, mult = f
            if len(xl) > MAX_FLOOR1_POSTS:
                raise SynthError(E_INVALID_ARG, "floor1 X list too long")
            fl[i].x_count = len(xl)
            fl[i].multiplier = mult
            for j, x in enumerate(xl):
                fl[i].x_list[j] = int(x)
        mp = (MappingConfig * max(1, len(mappings)))()
        for i, m in enumerate(mappings):
            cp = m.get("coupling", [])
            mp[i].coupling_steps = len(cp)
            for j, (mag, ang) in enumerate(cp):
                mp[i].coupling_magnitude[j] = mag
                mp[i].coupling_angle[j] = ang
            for c, f in enumerate(m.get("channel_floor", [0] * channels)):
                mp[i].channel_floor[c] = f
            for b in range(2):
                mp[i].residue_begin[b] = int(m.get("residue_begin", (0, 0))[b])
                mp[i].residue_end[b] = int(m.get("residue_end", (0, 0))[b])
        cfg = StreamConfig(channels, block_size0, block_size1, len(floors), fl, len(mappings), mp,
                           1 if clip_samples else 0, ftypes, fl0)
        self._h = _vp()
        rc = lib().vpz_decoder_create(ctx._h, C.byref(cfg), n_streams, C.byref(self._h))
        if rc != OK:
            self._h = None
            raise SynthError(rc, lib().vpz_context_last_error(ctx._h).decode())
        import weakref
        ctx._children.append(weakref.ref(self))

    def close(self):
        if self._h and self.ctx._h:
            lib().vpz_decoder_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=-1):
        self.ctx._check(lib().vpz_decoder_reset(self._h, stream))

    def synth_raw(self, packets, residue, posts, post_counts, pcm_out, stream_out_offset, capacity,
                  out_layout, channel_stride, mem_space, residue_floats=None, n_records=None, on_mismatch="raise"):
        """Thin call of vpz_decoder_synth; returns samples_written (int64 array, per stream).
        residue_floats / n_records default to the extents of the arrays handed in.  A packet skipped by the window check
        (StreamDecoder.cs:777-778) is a per-packet status in the ABI; on_mismatch="raise" turns it into
        SynthError(E_WINDOW_MISMATCH) AFTER the call has done all its work -- what a host does for the stream concerned --,
        "ignore" leaves it to last_packet_status()."""
        written = np.zeros(self.n_streams, dtype=np.int64)
        packets = np.ascontiguousarray(packets, dtype=PACKET_DTYPE)
        # ABI v5: the element type of `residue` is the array's (numpy or torch int16: VPZ_RESIDUE_I16, anything else float32)
        want = RESIDUE_I16 if str(getattr(residue, "dtype", "")) in ("int16", "torch.int16") else RESIDUE_F32
        if getattr(self, "residue_format", RESIDUE_F32) != want:
            self.set_residue_format(want)
        offs = None if stream_out_offset is None else np.ascontiguousarray(stream_out_offset, dtype=np.int64)
        if mem_space == MEM_DEVICE:
            _sync_producer(residue, posts, post_counts, pcm_out)
        if residue_floats is None:
            residue_floats = _numel(residue)
        if n_records is None:
            n_records = 0 if post_counts is None else _numel(post_counts)
        rc = lib().vpz_decoder_synth(self._h, len(packets), _ptr(packets), _ptr(residue), residue_floats, _ptr(posts),
                                     _ptr(post_counts), n_records, mem_space, _ptr(pcm_out), _ptr(offs), capacity,
                                     out_layout, channel_stride, _ptr(written))
        self.ctx._check(rc)
        self.last_written = written
        if on_mismatch == "raise" and self.last_mismatches() > 0:
            raise SynthError(E_WINDOW_MISMATCH, "a packet's previous tail is longer than its window slope "
                             "(StreamDecoder.cs:777-778 throws); the packet was skipped, everything else was synthesised")
        return written

    def last_mismatches(self):
        n = C.c_int64()
        self.ctx._check(lib().vpz_decoder_last_packet_status(self._h, None, 0, C.byref(n)))
        return n.value

    def last_packet_status(self, n_packets):
        out = np.zeros(n_packets, dtype=np.int32)
        self.ctx._check(lib().vpz_decoder_last_packet_status(self._h, _ptr(out), n_packets, None))
        return out

    def synth(self, packets, residue, posts=None, post_counts=None, out_layout=OUT_PLANAR, capacity=None,
              on_mismatch="raise"):
        """Host-memory convenience: returns a list (per stream) of PCM arrays, [channels, samples]
        for OUT_PLANAR or [samples, channels] for OUT_INTERLEAVED (int16 arrays for the _S16 layouts)."""
        packets = np.ascontiguousarray(packets, dtype=PACKET_DTYPE)
        # (int16 values -- ABI v5 -- go over as they are: synth_raw tells the decoder)
        residue = np.ascontiguousarray(residue, dtype=np.int16 if getattr(residue, "dtype", None) == np.int16 else np.float32)
        if posts is not None:
            posts = np.ascontiguousarray(posts, dtype=np.int16)
            post_counts = np.ascontiguousarray(post_counts, dtype=np.uint8)
        if capacity is None:
            per = np.zeros(self.n_streams, dtype=np.int64)
            for s, f in zip(packets["stream"], packets["flags"]):
                per[s] += (self.size1 if f & PKT_BLOCK_FLAG else self.size0)
            capacity = int(per.max()) + 1
        C_ = self.channels
        s16 = out_layout in (OUT_INTERLEAVED_S16, OUT_PLANAR_S16)
        out = np.zeros(self.n_streams * C_ * capacity, dtype=np.int16 if s16 else np.float32)
        offs = np.arange(self.n_streams, dtype=np.int64) * (C_ * capacity)
        written = self.synth_raw(packets, residue, posts, post_counts, out, offs, capacity, out_layout,
                                 capacity, MEM_HOST, on_mismatch=on_mismatch)
        res = []
        for s in range(self.n_streams):
            blk = out[offs[s]: offs[s] + C_ * capacity]
            if out_layout in (OUT_PLANAR, OUT_PLANAR_S16):
                res.append(blk.reshape(C_, capacity)[:, :written[s]].copy())
            else:
                res.append(blk[: written[s] * C_].reshape(written[s], C_).copy())
        return res

    def debug_floor1_indices(self, posts, post_counts, record_floor, record_long):
        """Test-only (vorbispizza_synth_debug.h): the integers of the Floor1 device path for a batch of channel
        records.  Returns (curve [records, size1/2] uint8, final_y [records, 64] int16, step_flags [records, 64]
        uint8, active_count [records] uint8)."""
        posts = np.ascontiguousarray(posts, dtype=np.int16).reshape(-1, 64)
        n = posts.shape[0]
        post_counts = np.ascontiguousarray(post_counts, dtype=np.uint8)
        record_floor = np.ascontiguousarray(record_floor, dtype=np.uint8)
        record_long = np.ascontiguousarray(record_long, dtype=np.uint8)
        assert len(post_counts) == len(record_floor) == len(record_long) == n
        curve = np.full((n, self.size1 // 2), 0xEE, dtype=np.uint8)
        final_y = np.zeros((n, 64), dtype=np.int16)
        flags = np.zeros((n, 64), dtype=np.uint8)
        active = np.zeros(n, dtype=np.uint8)
        self.ctx._check(lib().vpz_debug_floor1_indices(self._h, n, _ptr(posts), _ptr(post_counts), _ptr(record_floor),
                                                       _ptr(record_long), _ptr(curve), _ptr(final_y), _ptr(flags),
                                                       _ptr(active)))
        return curve, final_y, flags, active

    def set_floor0_data(self, amp, coeff):
        """amp [records], coeff [records, stride] (numpy, host memory) for the next synth call."""
        f0 = (np.ascontiguousarray(amp, dtype=np.float32), np.ascontiguousarray(coeff, dtype=np.float32))
        self.ctx._check(lib().vpz_decoder_set_floor0_data(self._h, _ptr(f0[0]), _ptr(f0[1]), f0[1].shape[1]))
        self._f0 = f0  # (a refused call leaves the decoder pointing at the arrays it had: those stay alive)

    def last_packet_samples(self, n_packets):
        out = np.zeros(n_packets, dtype=np.int32)
        self.ctx._check(lib().vpz_decoder_last_packet_samples(self._h, _ptr(out), n_packets))
        return out

    def has_clipped(self, stream=0):
        v = C.c_int32()
        self.ctx._check(lib().vpz_decoder_has_clipped(self._h, stream, C.byref(v)))
        return bool(v.value)

    def position(self, stream=0):
        v = C.c_int64()
        self.ctx._check(lib().vpz_decoder_position(self._h, stream, C.byref(v)))
        return v.value

    def set_residue_format(self, fmt):
        """RESIDUE_F32 (default) or RESIDUE_I16: the element type of `residue` in the synth calls that follow (ABI v5)"""
        self.ctx._check(lib().vpz_decoder_set_residue_format(self._h, int(fmt)))
        self.residue_format = int(fmt)

    def set_host_threads(self, n):
        """Host threads this decoder's synth calls may use for their integer half (0: the process's CPUs, 1: none but the caller's)."""
        self.ctx._check(lib().vpz_decoder_set_host_threads(self._h, int(n)))

    def set_stream_capacities(self, capacities):
        """per-stream output bounds for the synth calls that follow (each tightens the call's stream_out_capacity); None removes them"""
        if capacities is None:
            self.ctx._check(lib().vpz_decoder_set_stream_capacities(self._h, None, 0))
            return
        caps = np.ascontiguousarray(capacities, dtype=np.int64)
        self.ctx._check(lib().vpz_decoder_set_stream_capacities(self._h, caps.ctypes.data_as(C.POINTER(C.c_int64)), int(caps.size)))

    def set_position(self, position, stream=0):
        self.ctx._check(lib().vpz_decoder_set_position(self._h, stream, int(position)))
