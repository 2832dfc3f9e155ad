"""The Python surface of the window-batch family: every public method of multi.Dispatcher and the capi functions that share a body
(the pcm_* feature wrappers, the filterbank and table getters) keep their parameter names, order and defaults, and a docstring.  The
signatures are literals, written down from the commit before the shared bodies were introduced -- never taken from the code under
test.  Needs no device and no built library: importing the modules loads nothing."""
import inspect

DISPATCHER = {
    "batch_partition": "(self, n, group)",
    "call_counts": "(self)",
    "close": "(self)",
    "decode_library": "(self, datas, pcm_out, pcm_offset, pcm_capacity, s16=False)",
    "decode_ranges": "(self, datas, ranges, pcm_out, pcm_offset, pcm_capacity, s16=False)",
    "decode_ranges_batch": "(self, datas, ranges, channels, frames, planar=True, s16=False, out=None, sample_rate=None, mono=False)",
    "decode_ranges_cqt": "(self, datas, ranges, frames, sample_rate=22050, channels=1, mono=True, f_min=32.70319566257483, n_bins=84, "
                         "bins_per_octave=12, hop=512, filter_scale=1.0, gamma=0.0, window='hann', scale='sqrt_length', pad='reflect', "
                         "output='magnitude', bins_first=True, out=None)",
    "decode_ranges_fbank": "(self, datas, ranges, frames, sample_rate=16000, win=400, hop=160, n_fft=512, n_mels=80, low_freq=20.0, "
                           "high_freq=0.0, preemphasis=0.97, window='povey', remove_dc=True, scale=32768.0, log=True, "
                           "floor=1.1920928955078125e-07, pad_value=0.0, frames_first=True, out=None)",
    "decode_ranges_fbank_post": "(self, datas, ranges, frames, post=None, out=None, **fbank)",
    "decode_ranges_logmel": "(self, datas, ranges, frames, sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=None, "
                            "mel_scale='slaney', mel_norm='slaney', log=True, floor=1e-10, bands_first=True, out=None)",
    "decode_ranges_melspec": "(self, datas, ranges, frames, sample_rate=22050, n_fft=2048, hop=512, n_mels=128, f_min=0.0, f_max=None, "
                             "mel_scale='slaney', mel_norm='slaney', log=True, floor=1e-10, bands_first=True, out=None)",
    "decode_ranges_mfcc": "(self, datas, ranges, frames, sample_rate=16000, win=400, hop=160, n_fft=512, n_mels=23, low_freq=20.0, "
                          "high_freq=0.0, preemphasis=0.97, window='povey', remove_dc=True, scale=32768.0, floor=1.1920928955078125e-07, "
                          "pad_value=0.0, frames_first=True, n_ceps=13, lifter=22.0, use_energy=True, energy_floor=0.0, htk_compat=False, "
                          "subtract_mean=False, out=None)",
    "decode_ranges_mfcc_post": "(self, datas, ranges, frames, post=None, out=None, **mfcc)",
    "decode_ranges_stft": "(self, datas, ranges, frames, sample_rate=44100, channels=2, mono=False, n_fft=4096, hop=1024, win_length=None, "
                          "window='hann', output='complex', bins_first=True, out=None)",
    "last_error": "(self)",
    "measure_loudness": "(self, datas, ranges=None)",
    "measure_r128": "(self, datas, ranges=None)",
    "set_mixed_setups": "(self, on)",
}

CAPI = {
    "pcm_logmel": "(ctx, src, rows, dst, spec, frames)",
    "pcm_melspec": "(ctx, src, rows, dst, spec, frames)",
    "pcm_stft": "(ctx, src, rows, dst, spec, frames)",
    "pcm_cqt": "(ctx, src, rows, dst, spec, frames)",
    "pcm_fbank": "(ctx, src, rows, dst, spec, frames)",
    "pcm_mfcc": "(ctx, src, rows, dst, spec, frames)",
    "mel_filterbank": "(spec)",
    "melspec_filterbank": "(spec)",
    "fbank_filterbank": "(spec)",
    "logmel_dft_table": "(n_fft)",
    "melspec_twiddles": "(n_fft)",
    "stft_table": "(n_fft, win_length=None, window='hann')",
    "fbank_table": "(spec)",
    "mfcc_table": "(spec)",
}


def test_the_dispatcher_has_these_public_methods_and_no_others():
    from vorbispizza_amd import multi
    public = sorted(name for name, member in vars(multi.Dispatcher).items() if not name.startswith("_") and callable(member))
    assert public == sorted(DISPATCHER)


def test_every_dispatcher_method_keeps_its_signature_and_a_docstring():
    from vorbispizza_amd import multi
    for name, want in DISPATCHER.items():
        method = getattr(multi.Dispatcher, name)
        assert str(inspect.signature(method)) == want, name
        assert (method.__doc__ or "").strip(), name


def test_every_shared_capi_function_keeps_its_signature_and_a_docstring():
    from vorbispizza_amd import capi
    for name, want in CAPI.items():
        fn = getattr(capi, name)
        assert str(inspect.signature(fn)) == want, name
        assert (fn.__doc__ or "").strip(), name
