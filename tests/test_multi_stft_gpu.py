"""vpzm_decode_ranges_stft (include/vorbispizza_multi_stft.h, host/vorbis_multi.cpp): window batches as per-channel STFT spectrograms.

Streams and windows are those of tests/test_multi_logmel_gpu.py.  The call is the resampled call with one more stage, so what is checked of
it is EQUALITY, bit for bit: its tensor is capi.pcm_stft applied to what decode_ranges_batch(..., sample_rate=R, channels, mono) delivers --
channel c of entry k as row k * C + c, results["samples"] as every row's L -- on every route, partition, cut and failure path, stereo
without downmix and mono with it.  The kernel is held to the float64 truth in tests/test_pcm_stft_gpu.py; one test here holds the whole
chain to it end to end (its docstring states the bound)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stft_truth as st  # noqa: E402
from f32_model import U  # noqa: E402
from logmel_truth import frames_of  # noqa: E402
from multi_support import (bits_of_any as bits, channels_of, FIELDS, golden, logmel_by_hand, logmel_call, LOGMEL_VARIANTS,  # noqa: E402
    mixed_entries, most_outputs, OPTIONS, out_len, RATE, ratio, refused_entries_by_channel as refused_entries, rerated,
    resampled_call, Stream, streams)
from resample_truth import bound, resample_truth  # noqa: E402
from stft_truth import stft_refused_specs  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

OWN = 44100  # the rate of the stereo and six-channel fixture streams
# a separation model's front end on both channels, in torch's order; a vocoder's linear magnitudes of the mixed-down signal at another
# rate, with the other window, a shorter win_length and the other layout
VARIANTS = [dict(sample_rate=OWN, channels=2, mono=False, n_fft=4096, hop=1024, win_length=None, window="hann", output="complex", bins_first=True),
            dict(sample_rate=22050, channels=1, mono=True, n_fft=1024, hop=256, win_length=800, window="hamming", output="magnitude", bins_first=False)]
IDS = ["stereo_44100_4096_complex_bins_first", "mono_22050_1024_magnitude_frames_first"]


def shape_of(n, frames, spec):
    T, NF = 1 + frames // spec["hop"], spec["n_fft"] // 2 + 1
    return (n, channels_of(spec)) + ((NF, T) if spec["bins_first"] else (T, NF))


def dtype_of(spec):
    import torch
    return torch.complex64 if spec["output"] == "complex" else torch.float32


def stft_call(entries, frames, spec, device_ids=(0,), dispatcher=None, out=None, **opt):
    """-> (the spectrograms as one tensor, results, stats)"""
    import torch
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        parts, whole, results, stats = d.decode_ranges_stft([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames, out=out, **spec)
    finally:
        if dispatcher is None:
            d.close()
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == shape_of(len(entries), frames, spec) and whole.dtype == dtype_of(spec)
    return whole, results, stats


def make_spec(spec):
    from vorbispizza_amd import capi
    return capi.StftSpec.make(**{k: spec[k] for k in ("n_fft", "hop", "win_length", "window", "output", "bins_first")})


def by_hand(ctx, entries, frames, spec, **opt):
    """capi.pcm_stft over the planar resampled batch of the same entries, every channel a row, results["samples"] as L: what the call
    must equal"""
    import torch
    from vorbispizza_amd import capi
    Cn = channels_of(spec)
    batch, results, _ = resampled_call(entries, spec["sample_rate"], Cn, frames, True, False, spec["mono"], **opt)
    shape = shape_of(len(entries), frames, spec)
    dst = torch.full((len(entries) * Cn,) + shape[2:] + ((2,) if spec["output"] == "complex" else ()), 7.0, dtype=torch.float32, device="cuda:0")
    rows = [((k * Cn + c) * frames, int(results["samples"][k]), k * Cn + c) for k in range(len(entries)) for c in range(Cn)]
    assert capi.pcm_stft(ctx, batch.reshape(-1), rows, dst, make_spec(spec), frames) == capi.OK, ctx.last_error()
    ctx.synchronize()
    if spec["output"] == "complex":
        dst = torch.view_as_complex(dst)
    return dst.view(shape), results


def frames_for(entries, spec, more=5):
    return max(most_outputs(entries, spec["sample_rate"]), spec["n_fft"] // 2 + 1) + more


@pytest.mark.parametrize("variant", [0, 1], ids=IDS)
@pytest.mark.parametrize("route", ["host", "device"])
def test_the_call_is_pcm_stft_of_the_resampled_batch(ctx, route, variant):
    import torch
    from vorbispizza_amd import multi
    spec = VARIANTS[variant]
    entries = mixed_entries()  # (1, 2 and 6 channels; 44 100, 48 000, 22 050, 8 000 and 16 000 Hz: entries at other rates than the call's)
    assert len({int(s.f.sample_rate) for s, _, _ in entries} - {spec["sample_rate"]}) >= 3
    frames = frames_for(entries, spec)
    want, want_results = by_hand(ctx, entries, frames, spec, **OPTIONS[route])
    got, results, _ = stft_call(entries, frames, spec, **OPTIONS[route])
    assert torch.equal(bits(got), bits(want))
    for field in FIELDS:
        assert np.array_equal(results[field], want_results[field]), field
    assert (results["status"] == 0).sum() >= 10 and (results["samples"] > 0).any() and (results["samples"] == 0).any()
    assert torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all()
    other = np.array([s.channels != 2 for s, _, _ in entries])
    if spec["mono"]:
        assert (results["status"] != multi.E_CHANNELS).all()
    else:  # a stream of another channel count costs its entry, and its rows are zeros in both channels
        assert other.any() and (results["status"][other] == multi.E_CHANNELS).all() and (results["status"][~other] != multi.E_CHANNELS).all()
        assert not bits(got[torch.from_numpy(other).to(got.device)]).any()
        live = torch.from_numpy((results["samples"] > 1000)).to(got.device)
        assert live.any() and (got[live].abs().amax(dim=(2, 3)) > 0).all()  # both channels of every entry that delivered a window of some length


def test_the_partition_the_cut_and_the_failure_paths_change_no_bit(ctx, monkeypatch):
    import torch
    for spec in VARIANTS:
        entries = mixed_entries()[::2]
        frames = frames_for(entries, spec, 1)
        one, one_results = by_hand(ctx, entries, frames, spec, gpu_entropy=False)
        for groups in (1, 2, 3):
            for gpu_entropy in ((False, True) if groups < 3 else (True,)):
                got, results, _ = stft_call(entries, frames, spec, device_ids=[0] * groups, streams_per_call=5, gpu_entropy=gpu_entropy, host_threads=2 * groups)
                assert torch.equal(bits(got), bits(one)), (groups, gpu_entropy)
                for field in FIELDS:
                    if field != "device_slot":
                        assert np.array_equal(results[field], one_results[field]), field
        monkeypatch.setenv("VPZM_FAIL_BATCH_CALLS", "1")
        got, results, stats = stft_call(entries, frames, spec, gpu_entropy=True, streams_per_call=64)
        monkeypatch.delenv("VPZM_FAIL_BATCH_CALLS")
        assert torch.equal(bits(got), bits(one))
        for field in FIELDS:
            assert np.array_equal(results[field], one_results[field]), field


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_refused_entry_costs_only_itself_and_leaves_zero_rows_in_all_its_channels(ctx, gpu_entropy):
    import torch
    for spec in VARIANTS:
        entries, J, status, samples = refused_entries(spec)
        want, _ = by_hand(ctx, entries, J, spec, gpu_entropy=gpu_entropy, streams_per_call=2)
        got, results, _ = stft_call(entries, J, spec, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
        assert list(results["status"]) == status and list(results["samples"]) == samples
        assert results["channels"][4] == 1 and results["sample_rate"][5] == 44101
        assert torch.equal(bits(got), bits(want))
        img = bits(got).cpu().numpy().reshape(len(entries), channels_of(spec), -1)
        dead = [k for k in range(len(entries)) if samples[k] == 0]
        live = [k for k in range(len(entries)) if samples[k] > 0]
        assert not img[dead].any() and img[live].any(axis=2).all()  # every channel of a dead entry is zeros, every channel of a live one is not


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_failed_stft_launch_costs_its_members_e_synth_and_leaves_zero_rows(ctx, monkeypatch, gpu_entropy):
    """the entries of the test above under VPZM_FAIL_DELIVERY (check_failed_delivery of multi_support.py): the resample launches into
    the lane's temporary are made, the STFT launch is not"""
    from multi_support import check_failed_delivery, sentinel_out
    from vorbispizza_amd import multi
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        for spec in VARIANTS:
            entries, J, _, _ = refused_entries(spec)
            check_failed_delivery(monkeypatch, d, lambda: stft_call(entries, J, spec, dispatcher=d, out=sentinel_out(
                d, len(entries), lambda rows: shape_of(rows, J, spec), dtype_of(spec), 77.0))[:2], 0, step="vpz_pcm_stft")
    finally:
        d.close()


def test_a_wrong_out_tensor_raises_and_a_wrong_spec_is_refused(ctx):
    import torch
    from vorbispizza_amd import capi, multi
    s = streams()["stereo_coupled_res2_12"]
    entries = [(s, a, n) for a, n in s.windows()[:6]]
    spec = VARIANTS[0]
    frames = frames_for(entries, spec, 0)
    T, NF = 1 + frames // 1024, 2049
    d = multi.Dispatcher([0, 0], host_threads=2)
    try:
        z = lambda *shape, **kw: torch.zeros(shape, **dict(dict(dtype=torch.complex64, device="cuda:0"), **kw))  # noqa: E731
        good = [z(3, 2, NF, T) for _ in range(2)]
        got, _, _ = stft_call(entries, frames, spec, dispatcher=d, out=good)
        assert torch.equal(bits(got), bits(stft_call(entries, frames, spec, dispatcher=d)[0]))
        for bad in ([good[0]], [good[0], z(3, 2, T, NF)], [good[0], z(3, 2, NF, T + 1)], [good[0], z(4, 2, NF, T)], [good[0], z(3, 1, NF, T)], [good[0], z(3, NF, T)],
                    [good[0], z(3, 2, NF, T, dtype=torch.float32)], [good[0], z(3, 2, NF, T, 2, dtype=torch.float32)], [good[0], z(3, 2, NF, T, device="cpu")],
                    [good[0], z(3, 2, NF, 2 * T)[:, :, :, ::2]], [good[0], None]):
            marker = [t.clone() for t in bad if isinstance(t, torch.Tensor)]
            with pytest.raises(ValueError):
                d.decode_ranges_stft([e[0].data for e in entries], [(a, n) for _, a, n in entries], frames, out=bad, **spec)
            assert all(torch.equal(a, b) for a, b in zip(marker, [t for t in bad if isinstance(t, torch.Tensor)]))  # (nothing was written)
        with pytest.raises(ValueError):
            d.decode_ranges_stft([e[0].data for e in entries], [(a, n) for _, a, n in entries], frames, **dict(spec, window="povey"))
        # the library's own refusals: VPZM_E_ARG
        n_e = len(entries)
        ptrs = (C.c_void_p * n_e)(*[e[0].data.ctypes.data for e in entries])
        sizes = (C.c_uint64 * n_e)(*[e[0].data.size for e in entries])
        rng = np.array([(x, c) for _, x, c in entries], dtype=np.int64)
        res = np.zeros(n_e, dtype=multi.RESULT_DTYPE)
        whole = z(n_e, 2, NF, T)
        dst = (C.c_void_p * 2)(whole[:3].data_ptr(), whole[3:].data_ptr())
        ok = make_spec(spec)
        args = lambda **kw: [kw.get(k, v) for k, v in (("m", d._h), ("n", n_e), ("data", ptrs), ("size", sizes), ("ranges", rng.ctypes.data),  # noqa: E731
                                                       ("rate", OWN), ("channels", 2), ("downmix", 0), ("spec", C.byref(ok)), ("frames", frames), ("dst", dst),
                                                       ("results", res.ctypes.data), ("stats", None))]
        L = multi.lib()
        assert L.vpzm_decode_ranges_stft(*args()) == multi.OK
        assert torch.equal(bits(whole), bits(got))
        changes = [dict(spec=None), dict(frames=0), dict(frames=2048), dict(dst=None), dict(m=None), dict(results=None), dict(ranges=None), dict(n=-1),
                   dict(rate=0), dict(channels=0), dict(channels=256), dict(downmix=2), dict(downmix=-1), dict(downmix=1)]  # (downmix 1 needs channels 1)
        changes += [dict(spec=C.byref(sp)) for _, sp in stft_refused_specs(capi)]
        for change in changes:
            assert L.vpzm_decode_ranges_stft(*args(**change)) == multi.E_ARG, change
        assert L.vpzm_decode_ranges_stft(*args(frames=2049)) == multi.OK  # (n_fft / 2 + 1: the entries that need more are refused one by one)
    finally:
        d.close()


def test_the_calls_in_turn_on_one_dispatcher(ctx):
    """the lane's temporary -- mono rows for the older feature calls, planar channels for this one -- and the context's table caches serve
    call after call: the log-mel call and the plain batch still deliver their old bits beside the new one"""
    import torch
    from multi_support import MELSPEC_VARIANTS, melspec_by_hand, melspec_call
    entries = mixed_entries()[::3]
    frames = max(frames_for(entries, spec, 0) for spec in VARIANTS)
    wants = [by_hand(ctx, entries, frames, spec)[0] for spec in VARIANTS]
    old_want = logmel_by_hand(ctx, entries, frames, LOGMEL_VARIANTS[0])[0]
    mel_want = melspec_by_hand(ctx, entries, frames, MELSPEC_VARIANTS[0])[0]
    stereo = resampled_call(entries, RATE, 2, frames, True, False, False)[0]
    from vorbispizza_amd import multi
    d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
    try:
        for _ in range(2):
            for spec, want in zip(VARIANTS, wants):
                assert torch.equal(bits(stft_call(entries, frames, spec, dispatcher=d)[0]), bits(want))
                assert torch.equal(bits(logmel_call(entries, frames, LOGMEL_VARIANTS[0], dispatcher=d)[0]), bits(old_want))
                assert torch.equal(bits(melspec_call(entries, frames, MELSPEC_VARIANTS[0], dispatcher=d)[0]), bits(mel_want))
                assert torch.equal(bits(resampled_call(entries, RATE, 2, frames, True, False, False, dispatcher=d)[0]), bits(stereo))
    finally:
        d.close()


def test_a_fixture_window_against_the_float64_truth_end_to_end(ctx):
    """One window of a recorded stream (golden/3test.ogg, stereo) and one of the synthetic stereo stream, through decode, resample to
    22 050 Hz and the complex STFT of both channels, against the float64 restatements of both definitions over the host's stream-by-stream
    whole decode of the same window.

    THE BOUND.  The resampled row the kernel reads differs from its float64 truth y by at most r[j] = bound(B, up, down, 1)
    (tests/test_resample_cpu.py, the resample's documented bound).  The spectrum is linear in the row, so Re and Im move by at most
    R = sum_m r w; on top come the kernel's own roundings on the row it read, whose magnitudes are at most |y| + r.  So every component
    lies within d = K(n_fft) u sum_m (|y| + r) w + R of the truth."""
    import torch
    rate, n_fft, hop = 22050, 1024, 256
    spec = dict(sample_rate=rate, channels=2, mono=False, n_fft=n_fft, hop=hop, win_length=None, window="hann", output="complex", bins_first=True)
    w = st.window64(n_fft)
    fixture, synthetic = Stream(golden("3test.ogg"), False), streams()["stereo_coupled_res2_30"]
    entries = [(fixture, fixture.bounds[len(fixture.bounds) // 2] + 11, 9000), (synthetic, synthetic.bounds[3] + 7, 5000)]
    frames = most_outputs(entries, rate) + 3 * n_fft  # (the last frames lie wholly in the padding: exactly 0)
    got, results, _ = stft_call(entries, frames, spec, gpu_entropy=False)
    img = got.cpu().numpy().transpose(0, 1, 3, 2)  # [row][channel][T][n_freq]
    worst = 0.0
    for k, (s, a, n) in enumerate(entries):
        up, down = ratio(s, rate)
        m = s.f.window(a, n)["samples"]
        J = out_len(m, up, down)
        assert results["status"][k] == 0 and results["samples"][k] == J and m == n and s.channels == 2
        y, B = resample_truth(s.truth(ctx, False)[a: a + m], up, down, False)
        r = bound(B, up, down, 1)
        for c in range(2):
            X, D = frames_of(y[:, c], J, frames, n_fft, hop), frames_of(r[:, c], J, frames, n_fft, hop)
            Z = st.spectrum64(X, w)
            d = (st.K(n_fft) * U * ((np.abs(X) + D) @ w) + D @ w)[:, None]
            err = np.maximum(np.abs(img[k, c].real.astype(np.float64) - Z.real), np.abs(img[k, c].imag.astype(np.float64) - Z.imag))
            assert (err <= d).all(), (k, c, float((err / np.maximum(d, 1e-300)).max()))
            dead = np.broadcast_to(d == 0, err.shape)
            assert (img[k, c][dead] == 0).all() and dead.any() and (np.abs(Z) > 1e-3).any()
            live = np.broadcast_to(d > 0, err.shape)
            worst = max(worst, float((err[live] / np.broadcast_to(d, err.shape)[live]).max()))
        assert not np.array_equal(img[k, 0], img[k, 1])  # (two channels, not one twice)
    print("end to end: largest error / bound %.4f" % worst)
