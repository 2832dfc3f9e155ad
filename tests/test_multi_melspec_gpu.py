"""vpzm_decode_ranges_melspec (include/vorbispizza_multi_melspec.h, host/vorbis_multi.cpp): window batches as (log-)mel spectrogram frames
with transforms of 2048 to 8192.

Streams and windows are those of tests/test_multi_logmel_gpu.py.  The call is the mono resampled call with one more stage, so what is
checked of it is EQUALITY, bit for bit: its tensor is capi.pcm_melspec applied to what decode_ranges_batch(..., sample_rate=R, mono=True)
delivers, with results["samples"] as every row's L -- on every route, partition, cut and failure path, at the stereo streams' own rate
(44 100 Hz) and at 22 050 Hz.  The kernel is held to the float64 truth in tests/test_pcm_melspec_gpu.py; one test here holds the whole
chain to it end to end (its docstring states the bound)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import melspec_truth as mt  # noqa: E402
from f32_model import U  # noqa: E402
from logmel_truth import frames_of, mel_weights64, silence_value  # noqa: E402
from multi_support import (bits, FIELDS, golden, logmel_by_hand, logmel_call, LOGMEL_VARIANTS, mixed_entries, most_outputs,  # noqa: E402
    OPTIONS, out_len, RATE, ratio, rerated, resampled_call, Stream, streams)
from resample_truth import bound, resample_truth  # noqa: E402
from multi_support import (LIBROSA, MELSPEC_VARIANTS as VARIANTS, melspec_by_hand as by_hand, melspec_call, melspec_shape_of  # noqa: E402
    as shape_of)
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def frames_for(entries, spec, more=5):
    return max(most_outputs(entries, spec["sample_rate"]), spec["n_fft"] // 2 + 1) + more


@pytest.mark.parametrize("variant", [0, 1], ids=["librosa_22050_log_bands_first", "own_rate_4096_power_frames_first"])
@pytest.mark.parametrize("route", ["host", "device"])
def test_the_call_is_pcm_melspec_of_the_mono_resampled_batch(ctx, route, variant):
    import torch
    spec = VARIANTS[variant]
    entries = mixed_entries()  # (1, 2 and 6 channels; 44 100, 48 000, 22 050, 8 000 and 16 000 Hz: entries at other rates than the call's)
    assert len({int(s.f.sample_rate) for s, _, _ in entries} - {spec["sample_rate"]}) >= 3
    frames = frames_for(entries, spec)
    want, want_results = by_hand(ctx, entries, frames, spec, **OPTIONS[route])
    got, results, _ = melspec_call(entries, frames, spec, **OPTIONS[route])
    assert torch.equal(bits(got), bits(want))
    for field in FIELDS:
        assert np.array_equal(results[field], want_results[field]), field
    assert (results["status"] == 0).sum() > len(entries) // 2 and (results["samples"] > 0).any() and (results["samples"] == 0).any()
    assert torch.isfinite(got).all()


def test_the_partition_the_cut_and_the_failure_paths_change_no_bit(ctx, monkeypatch):
    import torch
    spec = VARIANTS[0]
    entries = mixed_entries()
    frames = frames_for(entries, spec, 1)
    one, one_results = by_hand(ctx, entries, frames, spec, gpu_entropy=False)
    for groups in (1, 2, 4):
        for gpu_entropy in ((False, True) if groups < 4 else (True,)):
            got, results, _ = melspec_call(entries, frames, spec, device_ids=[0] * groups, streams_per_call=5, gpu_entropy=gpu_entropy, host_threads=2 * groups)
            assert torch.equal(bits(got), bits(one)), (groups, gpu_entropy)
            for field in FIELDS:
                if field != "device_slot":
                    assert np.array_equal(results[field], one_results[field]), field
    for switch, value in (("VPZM_MAX_CALL_VALUES", "40000"), ("VPZM_FAIL_BATCH_CALLS", "1")):
        monkeypatch.setenv(switch, value)
        got, results, stats = melspec_call(entries, frames, spec, gpu_entropy=True, streams_per_call=64)
        monkeypatch.delenv(switch)
        assert torch.equal(bits(got), bits(one)), switch
        for field in FIELDS:
            assert np.array_equal(results[field], one_results[field]), (switch, field)


def refused_entries(rate):
    s, mono, odd = streams()["stereo_coupled_res2_30"], streams()["mono_floor1_res1_12"], rerated(44101)
    garbage = Stream.__new__(Stream)
    garbage.data = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    up, down = ratio(s, rate)
    a, n = s.bounds[3] + 7, 2100 * down
    J = out_len(n, up, down)
    assert J >= 2049 and out_len(n + 1, up, down) == J + 1  # (a row of J samples holds a transform of 4096)
    m_up, m_down = ratio(mono, rate)
    # entry 2: one output sample more than a row holds; entry 3: no Ogg; entry 5: a ratio the resampler refuses; entry 6: an empty window
    entries = [(s, a, n), (s, -1, n), (s, a, n + 1), (garbage, a, n), (mono, 5, 100), (odd, 3, 500), (s, s.total, 10), (s, a + 1, n)]
    return entries, J, out_len(100, m_up, m_down)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_refused_entry_costs_only_itself_and_leaves_the_silence_row(ctx, gpu_entropy):
    import torch
    from vorbispizza_amd import multi
    for spec in VARIANTS:
        entries, J, J_mono = refused_entries(spec["sample_rate"])
        want, _ = by_hand(ctx, entries, J, spec, gpu_entropy=gpu_entropy, streams_per_call=2)
        got, results, _ = melspec_call(entries, J, spec, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
        assert list(results["status"]) == [0, multi.E_RANGE, multi.E_CAPACITY, multi.E_OPEN, 0, multi.E_RATE, 0, 0]
        assert list(results["samples"]) == [J, 0, 0, 0, J_mono, 0, 0, J]
        assert results["channels"][4] == 1 and results["sample_rate"][5] == 44101
        assert torch.equal(bits(got), bits(want))
        silence = silence_value(spec["floor"]).view(np.uint32) if spec["log"] else np.uint32(0)
        img = got.cpu().numpy()
        assert (img[[1, 2, 3, 5, 6]].view(np.uint32) == silence).all()
        assert (img[[0, 4, 7]].view(np.uint32) != silence).any(axis=(1, 2)).all()


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_failed_melspec_launch_costs_its_members_e_synth_and_leaves_silence_rows(ctx, monkeypatch, gpu_entropy):
    """the entries of test_a_refused_entry_costs_only_itself_and_leaves_the_silence_row under VPZM_FAIL_DELIVERY (check_failed_delivery
    of test_multi_batch_gpu.py): the resample launches into the lane's temporary are made, the mel-spectrogram launch is not"""
    import torch
    from multi_support import check_failed_delivery, sentinel_out
    from vorbispizza_amd import multi
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        for spec in VARIANTS:
            entries, J, _ = refused_entries(spec["sample_rate"])
            silence = int(silence_value(spec["floor"]).view(np.int32)) if spec["log"] else 0
            check_failed_delivery(monkeypatch, d, lambda: melspec_call(entries, J, spec, dispatcher=d, out=sentinel_out(
                d, len(entries), lambda rows: shape_of(rows, J, spec), torch.float32, 77.0))[:2], silence, step="vpz_pcm_melspec")
    finally:
        d.close()


def test_a_wrong_out_tensor_raises_and_a_wrong_spec_is_refused(ctx):
    import torch
    from melspec_truth import melspec_refused_specs
    from vorbispizza_amd import capi, multi
    s = streams()["stereo_coupled_res2_12"]
    entries = [(s, a, n) for a, n in s.windows()[:6]]
    spec = VARIANTS[0]
    frames = frames_for(entries, spec, 0)
    T = 1 + frames // 512
    d = multi.Dispatcher([0, 0], host_threads=2)
    try:
        good = [torch.zeros((3, 128, T), dtype=torch.float32, device="cuda:0") for _ in range(2)]
        got, _, _ = melspec_call(entries, frames, spec, dispatcher=d, out=good)
        assert torch.equal(bits(got), bits(melspec_call(entries, frames, spec, dispatcher=d)[0]))
        for bad in ([good[0]], [good[0], torch.zeros((3, T, 128), dtype=torch.float32, device="cuda:0")], [good[0], torch.zeros((3, 128, T + 1), device="cuda:0")],
                    [good[0], torch.zeros((4, 128, T), device="cuda:0")], [good[0], torch.zeros((3, 128, T), dtype=torch.float64, device="cuda:0")],
                    [good[0], torch.zeros((3, 128, T))], [good[0], torch.zeros((3, 128, 2 * T), device="cuda:0")[:, :, ::2]], [good[0], None]):
            marker = [t.clone() for t in bad if isinstance(t, torch.Tensor)]
            with pytest.raises(ValueError):
                d.decode_ranges_melspec([e[0].data for e in entries], [(a, n) for _, a, n in entries], frames, out=bad, **spec)
            assert all(torch.equal(a, b) for a, b in zip(marker, [t for t in bad if isinstance(t, torch.Tensor)]))  # (nothing was written)
        # the library's own refusals: VPZM_E_ARG
        n_e = len(entries)
        ptrs = (C.c_void_p * n_e)(*[e[0].data.ctypes.data for e in entries])
        sizes = (C.c_uint64 * n_e)(*[e[0].data.size for e in entries])
        rng = np.array([(x, c) for _, x, c in entries], dtype=np.int64)
        res = np.zeros(n_e, dtype=multi.RESULT_DTYPE)
        whole = torch.zeros((n_e, 128, T), dtype=torch.float32, device="cuda:0")
        dst = (C.c_void_p * 2)(whole[:3].data_ptr(), whole[3:].data_ptr())
        ok = capi.LogMelSpec.make(**spec)
        args = lambda **kw: [kw.get(k, v) for k, v in (("m", d._h), ("n", n_e), ("data", ptrs), ("size", sizes), ("ranges", rng.ctypes.data),  # noqa: E731
                                                       ("spec", C.byref(ok)), ("frames", frames), ("dst", dst), ("results", res.ctypes.data), ("stats", None))]
        L = multi.lib()
        assert L.vpzm_decode_ranges_melspec(*args()) == multi.OK
        changes = [dict(spec=None), dict(frames=0), dict(frames=1024), dict(dst=None), dict(m=None), dict(results=None), dict(ranges=None), dict(n=-1)]
        changes += [dict(spec=C.byref(sp)) for _, sp in melspec_refused_specs(capi)]
        changes.append(dict(spec=C.byref(capi.LogMelSpec.make(**LOGMEL_VARIANTS[0]))))  # (the log-mel call's spec: n_fft 400)
        changes.append(dict(spec=C.byref(capi.LogMelSpec.make(**dict(spec, sample_rate=22050.5)))))  # (no whole number of Hz)
        for change in changes:
            assert L.vpzm_decode_ranges_melspec(*args(**change)) == multi.E_ARG, change
        # ... and the log-mel call keeps refusing this one's spec
        assert L.vpzm_decode_ranges_logmel(*args()) == multi.E_ARG
    finally:
        d.close()


def test_the_calls_in_turn_on_one_dispatcher(ctx):
    """the lane's temporary and the context's one table cache serve call after call, between calls of the older kinds: the log-mel call and
    the plain batch still deliver their old bits beside the new one"""
    import torch
    entries = mixed_entries()[::3]
    frames = frames_for(entries, VARIANTS[0], 0)
    wants = [by_hand(ctx, entries, frames, spec)[0] for spec in VARIANTS]
    old_want = logmel_by_hand(ctx, entries, frames, LOGMEL_VARIANTS[0])[0]
    mono = resampled_call(entries, RATE, 1, frames, True, False, True)[0]
    from vorbispizza_amd import multi
    d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
    try:
        for _ in range(2):
            for spec, want in zip(VARIANTS, wants):
                assert torch.equal(bits(melspec_call(entries, frames, spec, dispatcher=d)[0]), bits(want))
                assert torch.equal(bits(logmel_call(entries, frames, LOGMEL_VARIANTS[0], dispatcher=d)[0]), bits(old_want))
                assert torch.equal(bits(resampled_call(entries, RATE, 1, frames, True, False, True, dispatcher=d)[0]), bits(mono))
    finally:
        d.close()


def test_a_fixture_window_against_the_float64_truth_end_to_end(ctx):
    """One window of a recorded stream (golden/3test.ogg, stereo: mixed down) and one of the synthetic stereo stream, through decode,
    downmix, resample to 22 050 Hz and the mel spectrogram, against the float64 restatements of both definitions over the stream-by-stream
    whole decode.

    THE BOUND.  The resampled row the kernel reads differs from its float64 truth y by at most r[j] = bound(B, up, down, channels)
    (tests/test_resample_cpu.py, the resample's documented bound).  The spectrum is linear in the row, so re and im move by at most
    R = sum_m r w; on top come the kernel's own roundings on the row it read, whose magnitudes are at most |y| + r.  So
    d = K(n_fft) u sum_m (|y| + r) w + R, and then as in tests/melspec_truth.py:
        e_P = e0 + 3 u (P + e0),  e0 = 2 |re| d + 2 |im| d + 2 d^2
        e_M = sum_k W e_P + (B + 2) u (M + sum_k W e_P)
    The power output lies within e_M of the truth."""
    rate, n_fft, hop = 22050, 2048, 512
    spec = dict(LIBROSA, log=False, bands_first=True)
    W = mel_weights64(rate, n_fft, 128, 0.0, rate / 2.0, "slaney", "slaney")
    w = mt.hann64(n_fft)
    B_most = int((W > 0).sum(axis=1).max())
    fixture, synthetic = Stream(golden("3test.ogg"), False), streams()["stereo_coupled_res2_30"]
    entries = [(fixture, fixture.bounds[len(fixture.bounds) // 2] + 11, 9000), (synthetic, synthetic.bounds[3] + 7, 5000)]
    frames = most_outputs(entries, rate) + 3 * n_fft  # (the last frames lie wholly in the padding: exactly 0)
    got, results, _ = melspec_call(entries, frames, spec, gpu_entropy=True)
    img = got.cpu().numpy().transpose(0, 2, 1)  # [row][T][n_mels]
    worst = 0.0
    for k, (s, a, n) in enumerate(entries):
        up, down = ratio(s, rate)
        m = s.f.window(a, n)["samples"]
        J = out_len(m, up, down)
        assert results["status"][k] == 0 and results["samples"][k] == J and m == n
        y, B = resample_truth(s.truth(ctx, False)[a: a + m], up, down, True)
        y, r = y[:, 0], bound(B, up, down, s.channels)[:, 0]
        X, D = frames_of(y, J, frames, n_fft, hop), frames_of(r, J, frames, n_fft, hop)
        re_, im_ = mt.spectrum64(X, n_fft)
        d = (mt.K(n_fft) * U * ((np.abs(X) + D) @ w) + D @ w)[:, None]
        P = re_ * re_ + im_ * im_
        e0 = 2 * np.abs(re_) * d + 2 * np.abs(im_) * d + 2 * d * d
        e_P = e0 + 3 * U * (P + e0)
        M = P @ W.T
        e_M = e_P @ W.T + (B_most + 2) * U * (M + e_P @ W.T)
        err = np.abs(img[k].astype(np.float64) - M)
        assert (err <= e_M).all(), (k, float((err[e_M > 0] / e_M[e_M > 0]).max()))
        assert (img[k][e_M == 0].view(np.uint32) == 0).all() and (e_M == 0).any() and (M > 1e-6).any()
        worst = max(worst, float((err[e_M > 0] / e_M[e_M > 0]).max()))
    print("end to end: largest error / bound %.4f" % worst)
