"""The dispatcher's harness, shared by the tests/test_multi_*_gpu.py family: Stream and streams() (the containers and their whole decodes, ONE
table per process), the ranges call and its expected array, the library run, the padded-batch call with its device truth and
check_failed_delivery, the resampled call, and each feature kind's call wrapper, variants and refused entries under names that say the
kind.  Nothing here carries a pytest mark."""
import os

import numpy as np
import pytest

import fbank_truth as ft
import mfcc_truth as mt
from resample_truth import ratio_of

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

FIELDS = ("status", "device_slot", "channels", "sample_rate", "samples", "packets", "skipped_packets")
SENTINEL = 7


def golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


class Stream:
    """a container, what the front end says about it and its whole decode (computed once per PCM type, never changed)"""

    def __init__(self, raw, synthetic):
        from vorbispizza_amd.front import FrontError, OggVorbisFile
        self.raw = raw
        self.data = np.frombuffer(raw, dtype=np.uint8)
        self.f = OggVorbisFile(raw)
        self.channels, self.total, self.packets = self.f.channels, int(self.f.total_samples), int(self.f.audio_packets)
        self.bounds = [p for p in range(self.total + 1) if self.f.seek(p)[1] == 0]
        assert self.bounds[0] == 0 and len(self.bounds) >= 3
        if synthetic:  # (nothing trimmed at the end: the counted length is the total)
            with pytest.raises(FrontError):
                self.f.seek(self.total + 1)
        self.whole = {}

    def truth(self, ctx, s16):
        if s16 not in self.whole:
            self.whole[s16] = single_stream_pcm(ctx, self.raw, s16=s16)
        return self.whole[s16]

    def windows(self):
        b, total = self.bounds, self.total
        out = [(0, 1), (0, b[1]), (total, 10), (0, total), (b[2], total + 1000)]
        for i in range(1, len(b)):
            out += [(b[i] - 1, 2), (b[i] + 1, 5), (b[i], -1)]
            if i + 1 < len(b):
                out.append((b[i], b[i + 1] - b[i]))
        # three packets' samples where the packets' lengths change (a short / long transition): the last sample of one, the next one
        # whole, the first sample of the one after
        spans = [b[i + 1] - b[i] for i in range(len(b) - 1)]
        out += [(b[i] - 1, spans[i] + 2) for i in range(1, len(spans)) if spans[i - 1] != spans[i]]
        return out


_streams = {}


def streams():
    import synthetic_streams as ss
    if not _streams:
        for name, packets in (("stereo_coupled_res2", 12), ("stereo_coupled_res2", 30), ("mono_floor1_res1", 12), ("six_channels_51", 12),
                              ("stereo_floor0", 12)):
            st, rng = getattr(ss, name)()
            _streams["%s_%d" % (name, packets)] = Stream(bytes(st.build(rng, packets)[0]), True)
        _streams["1test.ogg"] = Stream(golden("1test.ogg"), False)
        assert _streams["1test.ogg"].packets == 25 and _streams["1test.ogg"].total == 17318
        assert not _streams["stereo_floor0_12"].f.gpu_decode_supported and _streams["stereo_coupled_res2_30"].f.gpu_decode_supported
        # a change of packet length inside every stream of two block sizes
        for name, s in _streams.items():
            spans = {s.bounds[i + 1] - s.bounds[i] for i in range(len(s.bounds) - 1)}
            assert len(spans) > 1 or name == "stereo_floor0_12", name
    return _streams


def all_entries():
    """[(stream, start, count)], every window of every stream, the streams interleaved so that sub-batches mix them"""
    per = [[(s, a, n) for a, n in s.windows()] for s in streams().values()]
    out = []
    for i in range(max(len(p) for p in per)):
        out += [p[i] for p in per if i < len(p)]
    return out


def place(entries, dense, s16, seed=5):
    """the caller's array: areas of exactly the samples asked for -- back to back in entry order (dense), or shuffled with gaps"""
    sizes = [s.f.window(a, n)["samples"] * s.channels for s, a, n in entries]
    caps = np.array([s.f.window(a, n)["samples"] for s, a, n in entries], dtype=np.int64)
    offs = np.zeros(len(entries), dtype=np.int64)
    rng = np.random.default_rng(seed)
    order = np.arange(len(entries)) if dense else rng.permutation(len(entries))
    at = 0
    for k in order:
        at += 0 if dense else int(rng.integers(1, 9))
        offs[k] = at
        at += sizes[k]
    pcm = np.full(at + (0 if dense else 3), SENTINEL, dtype=np.int16 if s16 else np.float32)
    return pcm, offs, caps


def call(entries, s16=False, dense=True, device_ids=(0,), dispatcher=None, **opt):
    from vorbispizza_amd import multi
    pcm, offs, caps = place(entries, dense, s16)
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        results, stats = d.decode_ranges([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], pcm, offs, caps, s16=s16)
    finally:
        if dispatcher is None:
            d.close()
    return pcm, offs, results, stats


def expected(ctx, entries, s16, dense):
    """the array a correct call leaves: the sentinel, and every window's slice of the whole decode in its area"""
    pcm, offs, _ = place(entries, dense, s16)
    for k, (s, a, n) in enumerate(entries):
        w = s.f.window(a, n)
        ref = s.truth(ctx, s16)
        assert ref.shape[0] == s.total  # (a clean stream: the whole decode delivers the total)
        pcm[offs[k]: offs[k] + w["samples"] * s.channels] = ref[a: a + w["samples"]].reshape(-1)
    return pcm


def same_bits(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


OPTIONS = {"host": dict(gpu_entropy=False), "device": dict(gpu_entropy=True), "mixed": dict(gpu_entropy=True, mixed_setups=True)}


def single_stream_pcm(ctx, raw, s16=False):
    """interleaved PCM of one container through the plain ABI: front end + one decoder + one synth call"""
    from vorbispizza_amd import Decoder, capi
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(raw)
    pk, res, posts, counts = f.decode_packets()
    dec = Decoder(ctx, f.channels, f.block_size0, f.block_size1, floors=f.floors, mappings=f.mappings)
    if f.floor0_data is not None:
        dec.set_floor0_data(*f.floor0_data)
    out = dec.synth(pk, res, posts, counts, out_layout=capi.OUT_INTERLEAVED_S16 if s16 else capi.OUT_INTERLEAVED,
                    on_mismatch="ignore")[0]
    dec.close()
    return out


def library(kinds, n):
    raws = [open(os.path.join(GOLDEN, k), "rb").read() for k in kinds]
    return [raws[i % len(raws)] for i in range(n)]


def run_dispatcher(device_ids, raws, s16=False, capacity_slack=2048, **opt):
    from vorbispizza_amd import multi
    from vorbispizza_amd.front import OggVorbisFile
    infos = {}
    for r in set(raws):
        f = OggVorbisFile(r)
        infos[r] = (f.channels, int(f.total_samples))
    caps = np.array([infos[r][1] + capacity_slack for r in raws], dtype=np.int64)
    sizes = np.array([c * infos[r][0] for c, r in zip(caps, raws)], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    pcm = np.full(int(sizes.sum()), 7, dtype=np.int16) if s16 else np.full(int(sizes.sum()), np.float32(7.0), dtype=np.float32)
    datas = [np.frombuffer(r, dtype=np.uint8) for r in raws]
    d = multi.Dispatcher(device_ids, **opt)
    try:
        results, stats = d.decode_library(datas, pcm, offs, caps, s16=s16)
    finally:
        d.close()
    return pcm, offs, results, stats, infos


def entries_of(channels):
    """[(stream, start, count)]: every window of every stream of `channels` channels, the streams interleaved so that sub-batches mix them"""
    per = [[(s, a, n) for a, n in s.windows()] for s in streams().values() if s.channels == channels]
    assert per
    out = []
    for i in range(max(len(p) for p in per)):
        out += [p[i] for p in per if i < len(p)]
    return out


def most_samples(entries):
    return max(s.f.window(a, n)["samples"] for s, a, n in entries)


def truth_rows(ctx, entries, frames, s16, delivered=None):
    """numpy [n, channels, frames]: every entry's slice of its stream's whole decode, zeros behind it (delivered[k] samples; None: the
    window rule's; an entry of None is a zero row)"""
    C = next(s.channels for s, _, _ in entries if s is not None)
    rows = np.zeros((len(entries), C, frames), dtype=np.int16 if s16 else np.float32)
    for k, (s, a, n) in enumerate(entries):
        if s is None:
            continue
        m = s.f.window(a, n)["samples"] if delivered is None else int(delivered[k])
        rows[k, :, :m] = s.truth(ctx, s16)[a: a + m].T
    return rows


_truth = {}


def truth_on_device(ctx, channels, s16):
    """the planar truth of entries_of(channels) at frames = its largest window, on the device as integers (computed once, never changed)"""
    import torch
    if (channels, s16) not in _truth:
        entries = entries_of(channels)
        rows = truth_rows(ctx, entries, most_samples(entries), s16)
        _truth[(channels, s16)] = torch.from_numpy(rows.view(np.int16 if s16 else np.int32)).to("cuda:0")
    return _truth[(channels, s16)]


def as_bits(t):
    import torch
    return t.view(torch.int16 if t.dtype == torch.int16 else torch.int32)


def same_on_device(got, planar_truth, planar):
    import torch
    return torch.equal(as_bits(got), planar_truth if planar else planar_truth.permute(0, 2, 1))


def batch_call(entries, channels, frames, planar=True, s16=False, device_ids=(0,), dispatcher=None, out=None, **opt):
    """-> (the batch as one tensor, results, stats); groups on one device share one tensor"""
    import torch
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        parts, whole, results, stats = d.decode_ranges_batch([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], channels, frames,
                                                             planar=planar, s16=s16, out=out)
    finally:
        if dispatcher is None:
            d.close()
    assert len(parts) == d.n_devices and all(p.is_cuda for p in parts)
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == ((len(entries), channels, frames) if planar else (len(entries), frames, channels))
    assert whole.dtype == (torch.int16 if s16 else torch.float32)
    return whole, results, stats


def sentinel_out(d, n, shape, dtype, value):
    """one tensor per group of `d` for an n-entry call, filled with `value`: shape(rows) is a group's"""
    import torch
    cuts = [d.batch_partition(n, g) for g in range(d.n_devices)]
    return [torch.full(shape(hi - lo), value, dtype=dtype, device="cuda:%d" % i) for (lo, hi), i in zip(cuts, d.device_ids)]


def check_failed_delivery(monkeypatch, d, run, empty_row, step=None):
    """VPZM_FAIL_DELIVERY (host/vorbis_multi.cpp): a sub-batch's delivery launch counts as failed without being made.  run() -> (tensor,
    results) of one call on dispatcher `d` into sentinel-filled tensors.  Every entry that a delivery launch serves -- OK in the plain
    call, with packets -- comes back E_SYNTH with no samples; an entry with a status of its own keeps it, and so does the empty window (OK,
    no packets: it is in no sub-batch, GroupRun::zero_rows alone defines its row); every row is `empty_row`; the next call without the
    switch is the plain call bit for bit.  step: the launch the switch fails -- the dispatcher's error text names it."""
    import torch
    from vorbispizza_amd import multi
    monkeypatch.delenv("VPZM_FAIL_DELIVERY", raising=False)
    plain, plain_results = run()
    monkeypatch.setenv("VPZM_FAIL_DELIVERY", "1")
    got, results = run()
    monkeypatch.delenv("VPZM_FAIL_DELIVERY")
    delivered = (plain_results["status"] == 0) & (plain_results["packets"] > 0)
    assert delivered.sum() >= 3 and (plain_results["status"] != 0).sum() >= 4 and ((plain_results["status"] == 0) & ~delivered).sum() == 1, \
        ("the entries are not the mix this check is for", plain_results["status"], plain_results["packets"])
    assert (results["status"][delivered] == multi.E_SYNTH).all(), results["status"]
    assert np.array_equal(results["status"][~delivered], plain_results["status"][~delivered]), \
        ("an entry outside the failed launch lost its own status", results["status"], plain_results["status"])
    assert (results["samples"] == 0).all(), ("samples reported behind a failed delivery", results["samples"])
    assert (as_bits(got) == empty_row).all(), "a row behind a failed delivery is not the empty row"
    assert not (as_bits(plain) == empty_row).all(), "the plain call delivered nothing: the comparison would be empty"
    assert d.last_error() != "", "the dispatcher kept no error text for the failed launch"
    if step is not None:
        assert step + ":" in d.last_error(), d.last_error()
    again, again_results = run()
    assert torch.equal(as_bits(again), as_bits(plain)), "the call after the failed one is not the plain call bit for bit"
    for field in FIELDS:
        if field != "device_slot":
            assert np.array_equal(again_results[field], plain_results[field]), field


RATE = 16000


def out_len(m, up, down):
    return -(-m * up // down)


def ratio(s, rate):
    return ratio_of(int(s.f.sample_rate), rate)


_rerated = {}


def rerated(rate, packets=12):
    """stereo_coupled_res2 at 12 packets with another rate in its identification header: the same setup header, so it shares sub-batches
    with its 44 100 Hz twin, at another ratio"""
    import synthetic_streams as ss
    if (rate, packets) not in _rerated:
        st, rng = ss.stereo_coupled_res2()
        st.rate = rate
        _rerated[(rate, packets)] = Stream(bytes(st.build(rng, packets)[0]), True)
        assert _rerated[(rate, packets)].f.sample_rate == rate and _rerated[(rate, packets)].channels == 2
    return _rerated[(rate, packets)]


def resampled_call(entries, rate, channels, frames, planar=True, s16=False, mono=False, device_ids=(0,), dispatcher=None, out=None, **opt):
    """-> (the batch as one tensor, results, stats)"""
    import torch
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        parts, whole, results, stats = d.decode_ranges_batch([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], channels, frames,
                                                             planar=planar, s16=s16, sample_rate=rate, mono=mono, out=out)
    finally:
        if dispatcher is None:
            d.close()
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == ((len(entries), channels, frames) if planar else (len(entries), frames, channels))
    assert whole.dtype == (torch.int16 if s16 else torch.float32)
    return whole, results, stats


def most_outputs(entries, rate):
    return max(out_len(s.f.window(a, n)["samples"], *ratio(s, rate)) for s, a, n in entries)


# Kaldi's own defaults, and a second spec so that every window, both output modes, both layouts, remove_dc off, another scale and a
# pad_value pass through the dispatcher
FBANK_VARIANTS = [ft.spec_of(sample_rate=RATE),
            ft.spec_of(sample_rate=RATE, win=96, hop=17, n_fft=128, n_mels=13, low_freq=100.0, high_freq=-1000.0, preemphasis=0.5, window="hamming",
                       remove_dc=False, scale=1.0, log=False, pad_value=-3.5, frames_first=False)]


def fbank_shape_of(n, frames, spec):
    T = ft.n_frames(frames, spec["win"], spec["hop"])
    return (n, T, spec["n_mels"]) if spec["frames_first"] else (n, spec["n_mels"], T)


def fbank_call(entries, frames, spec, device_ids=(0,), dispatcher=None, out=None, **opt):
    """-> (the features as one tensor, results, stats)"""
    import torch
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        parts, whole, results, stats = d.decode_ranges_fbank([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames, out=out, **spec)
    finally:
        if dispatcher is None:
            d.close()
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == fbank_shape_of(len(entries), frames, spec) and whole.dtype == torch.float32
    return whole, results, stats


def bits(t):
    import torch
    return t.view(torch.int32)


def mixed_entries():
    """every window of every stream -- 1, 2 and 6 channels; 44 100, 48 000, 8 000 and 16 000 Hz -- and the stereo setup at two more rates"""
    entries = all_entries()
    for rate in (48000, 22050):
        s = rerated(rate)
        for i, (a, n) in enumerate(s.windows()[:12]):
            entries.insert(5 + 17 * i + (rate == 48000), (s, a, n))
    assert {s.channels for s, _, _ in entries} == {1, 2, 6} and len({ratio(s, RATE) for s, _, _ in entries}) >= 5
    return entries


def refused_entries():
    """-> (entries, J): entry 2 has one output sample more than a row holds; entry 3 is no Ogg; entry 4 is 200 output samples, fewer than
    the Kaldi window; entry 5 has a ratio the resampler refuses; entry 6 is an empty window"""
    s, mono, odd = streams()["stereo_coupled_res2_30"], streams()["mono_floor1_res1_12"], rerated(44101)
    garbage = Stream.__new__(Stream)
    garbage.data = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    up, down = ratio(s, RATE)
    a, n = s.bounds[3] + 7, 7 * down
    J = out_len(n, up, down)
    assert J >= 400 and out_len(n + 1, up, down) == J + 1
    return [(s, a, n), (s, -1, n), (s, a, n + 1), (garbage, a, n), (mono, 5, 100), (odd, 3, 500), (s, s.total, 10), (s, a + 1, n)], J


WHISPER = dict(sample_rate=RATE, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=None, mel_scale="slaney", mel_norm="slaney", floor=1e-10)
# (log, bands_first) and a second spec, so that both output modes, both layouts and both scales pass through the dispatcher
LOGMEL_VARIANTS = [dict(WHISPER, log=True, bands_first=True),
            dict(sample_rate=RATE, n_fft=96, hop=17, n_mels=13, f_min=100.0, f_max=7000.0, mel_scale="htk", mel_norm=None, floor=1e-6, log=False, bands_first=False)]


def logmel_shape_of(n, frames, spec):
    T = 1 + frames // spec["hop"]
    return (n, spec["n_mels"], T) if spec["bands_first"] else (n, T, spec["n_mels"])


def logmel_call(entries, frames, spec, device_ids=(0,), dispatcher=None, out=None, **opt):
    """-> (the features as one tensor, results, stats)"""
    import torch
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        parts, whole, results, stats = d.decode_ranges_logmel([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames, out=out, **spec)
    finally:
        if dispatcher is None:
            d.close()
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == logmel_shape_of(len(entries), frames, spec) and whole.dtype == torch.float32
    return whole, results, stats


def logmel_by_hand(ctx, entries, frames, spec, **opt):
    """capi.pcm_logmel over the mono resampled batch of the same entries, results["samples"] as L: what the call must equal"""
    import torch
    from vorbispizza_amd import capi
    batch, results, _ = resampled_call(entries, spec["sample_rate"], 1, frames, True, False, True, **opt)
    dst = torch.full(logmel_shape_of(len(entries), frames, spec), 7.0, dtype=torch.float32, device="cuda:0")
    rows = [(k * frames, int(results["samples"][k]), k) for k in range(len(entries))]
    assert capi.pcm_logmel(ctx, batch.reshape(-1), rows, dst, capi.LogMelSpec.make(**spec), frames) == capi.OK, ctx.last_error()
    ctx.synchronize()
    return dst, results


OWN = 44100  # the rate of the stereo and six-channel fixture streams
LIBROSA = dict(sample_rate=22050, n_fft=2048, hop=512, n_mels=128, f_min=0.0, f_max=None, mel_scale="slaney", mel_norm="slaney", floor=1e-10)
# (log, bands_first), a second transform size and the other scale, so that both output modes and both layouts pass through the dispatcher
MELSPEC_VARIANTS = [dict(LIBROSA, log=True, bands_first=True),
            dict(sample_rate=OWN, n_fft=4096, hop=441, n_mels=40, f_min=30.0, f_max=16000.0, mel_scale="htk", mel_norm=None, floor=1e-6, log=False, bands_first=False)]


def melspec_shape_of(n, frames, spec):
    T = 1 + frames // spec["hop"]
    return (n, spec["n_mels"], T) if spec["bands_first"] else (n, T, spec["n_mels"])


def melspec_call(entries, frames, spec, device_ids=(0,), dispatcher=None, out=None, **opt):
    """-> (the features as one tensor, results, stats)"""
    import torch
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        parts, whole, results, stats = d.decode_ranges_melspec([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames, out=out, **spec)
    finally:
        if dispatcher is None:
            d.close()
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == melspec_shape_of(len(entries), frames, spec) and whole.dtype == torch.float32
    return whole, results, stats


def melspec_by_hand(ctx, entries, frames, spec, **opt):
    """capi.pcm_melspec over the mono resampled batch of the same entries, results["samples"] as L: what the call must equal"""
    import torch
    from vorbispizza_amd import capi
    batch, results, _ = resampled_call(entries, spec["sample_rate"], 1, frames, True, False, True, **opt)
    dst = torch.full(melspec_shape_of(len(entries), frames, spec), 7.0, dtype=torch.float32, device="cuda:0")
    rows = [(k * frames, int(results["samples"][k]), k) for k in range(len(entries))]
    assert capi.pcm_melspec(ctx, batch.reshape(-1), rows, dst, capi.LogMelSpec.make(**spec), frames) == capi.OK, ctx.last_error()
    ctx.synchronize()
    return dst, results


def channels_of(spec):
    return 1 if spec["mono"] else spec["channels"]


def bits_of_any(t):
    import torch
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32)


# the CQT call's end-to-end truth test (tests/test_multi_cqt_gpu.py) and the CPU case that holds its bound to the reference arithmetic
# (tests/test_cqt_cpu.py): N_0 = 3372, so the reflection reaches 1686 samples
CQT_END_TO_END = dict(sample_rate=22050, f_min=110.0, n_bins=48, bins_per_octave=12, hop=256, filter_scale=1.0, gamma=0.0, window="hann",
                      scale="sqrt_length", pad="reflect")


def end_to_end_entries():
    """a 9000-sample window of a recorded stream (golden/3test.ogg, stereo) and a 5000-sample one of the synthetic stereo stream: the
    STFT call's end-to-end entries"""
    fixture, synthetic = Stream(golden("3test.ogg"), False), streams()["stereo_coupled_res2_30"]
    return [(fixture, fixture.bounds[len(fixture.bounds) // 2] + 11, 9000), (synthetic, synthetic.bounds[3] + 7, 5000)]


def refused_entries_by_channel(spec):
    from vorbispizza_amd import multi
    rate = spec["sample_rate"]
    s, mono, odd = streams()["stereo_coupled_res2_30"], streams()["mono_floor1_res1_12"], rerated(44101)
    garbage = Stream.__new__(Stream)
    garbage.data = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    up, down = ratio(s, rate)
    a, n = s.bounds[3] + 7, 2100 * down
    J = out_len(n, up, down)
    assert J >= 2049 and out_len(n + 1, up, down) == J + 1  # (a row of J samples holds a transform of 4096)
    m_up, m_down = ratio(mono, rate)
    J_mono = out_len(100, m_up, m_down)
    # entry 2: one output sample more than a row holds (too few frames); entry 3: no Ogg; entry 4: a mono stream -- refused in a stereo
    # batch, mixed down to itself in a mono one; entry 5: a ratio the resampler refuses; entry 6: an empty window
    entries = [(s, a, n), (s, -1, n), (s, a, n + 1), (garbage, a, n), (mono, 5, 100), (odd, 3, 500), (s, s.total, 10), (s, a + 1, n), (s, a + 2, n)]
    status = [0, multi.E_RANGE, multi.E_CAPACITY, multi.E_OPEN, 0 if spec["mono"] else multi.E_CHANNELS, multi.E_RATE, 0, 0, 0]
    samples = [J, 0, 0, 0, J_mono if spec["mono"] else 0, 0, 0, J, J]
    return entries, J, status, samples


# Kaldi's own defaults, and a second spec so that the mean over frames, HTK's order without the energy, the other layout, remove_dc off,
# another window and a pad_value pass through the dispatcher
MFCC_VARIANTS = [mt.spec_of(sample_rate=RATE),
            mt.spec_of(sample_rate=RATE, win=96, hop=17, n_fft=128, n_mels=13, n_ceps=9, low_freq=100.0, high_freq=-1000.0, preemphasis=0.5,
                       window="hamming", remove_dc=False, pad_value=-3.5, frames_first=False, lifter=0.0, use_energy=False, htk_compat=True,
                       subtract_mean=True)]


def mfcc_shape_of(n, frames, spec):
    T = ft.n_frames(frames, spec["win"], spec["hop"])
    return (n, T, spec["n_ceps"]) if spec["frames_first"] else (n, spec["n_ceps"], T)


def mfcc_call(entries, frames, spec, device_ids=(0,), dispatcher=None, out=None, **opt):
    """-> (the features as one tensor, results, stats)"""
    import torch
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        parts, whole, results, stats = d.decode_ranges_mfcc([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames, out=out, **spec)
    finally:
        if dispatcher is None:
            d.close()
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == mfcc_shape_of(len(entries), frames, spec) and whole.dtype == torch.float32
    return whole, results, stats


def measure_call(entries, device_ids=(0,), dispatcher=None, ranges=True, **opt):
    """-> (records [n] as a LOUDNESS_DTYPE array, results, stats)"""
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        results, integrated, peak, steps, kept, stats = d.measure_loudness([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries] if ranges else None)
    finally:
        if dispatcher is None:
            d.close()
    rec = np.zeros(len(entries), dtype=multi.LOUDNESS_DTYPE)
    rec["integrated"], rec["peak"], rec["steps"], rec["blocks_kept"] = integrated, peak, steps, kept
    assert integrated.dtype == peak.dtype == np.float64 and steps.dtype == kept.dtype == np.int64
    return rec, results, stats


_entries = []


def loudness_entries():
    """the fbank tests' entries -- every window of every stream, three more rates of the stereo setup among them -- and windows of the
    stereo setup at 8 000 Hz with thirty packets, whole and in parts"""
    if not _entries:
        entries = mixed_entries()
        s = rerated(8000, 30)
        assert s.total >= 6 * 800
        for i, (a, n) in enumerate([(0, -1), (0, s.total), (s.bounds[2], 5 * 800 + 3), (s.bounds[1] + 1, 4 * 800), (s.bounds[3], 4 * 800 - 1)]):
            entries.insert(3 + 11 * i, (s, a, n))
        _entries.extend(entries)
    return list(_entries)


def loudness_refused_entries():
    """entry 1 lies outside its stream; entry 2 is no Ogg; entries 3 and 4 have rates just outside the limits; entry 5 is an empty window;
    entry 6 is shorter than a step"""
    s, mono = rerated(8000, 30), streams()["mono_floor1_res1_12"]
    garbage = Stream.__new__(Stream)
    garbage.data = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    a, n = s.bounds[2] + 7, 5 * 800 + 1
    return [(s, a, n), (s, -1, n), (garbage, a, n), (rerated(7999), 0, -1), (rerated(384001), 3, 500), (s, s.total, 10), (mono, 5, 100), (s, a + 1, n)]
