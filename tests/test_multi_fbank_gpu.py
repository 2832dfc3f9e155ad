"""vpzm_decode_ranges_fbank (include/vorbispizza_multi_fbank.h, host/vorbis_multi.cpp): window batches as Kaldi filterbank features.

Streams and windows are those of tests/test_multi_resample_gpu.py (the small synthetic streams of tests/synthetic_streams.py: 1, 2 and 6
channels, several source rates).  The call is the mono resampled call with one more stage, so what is checked of it is EQUALITY, bit for
bit: its tensor is capi.pcm_fbank applied to what decode_ranges_batch(..., sample_rate=R, mono=True) delivers, with results["samples"] as
every row's L -- on every route, partition, cut and failure path -- and those rows lie inside the bound of tests/fbank_truth.py's float64
restatement applied to the same delivered samples.  The kernel alone is held to the truth in tests/test_pcm_fbank_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fbank_truth as ft  # noqa: E402
from multi_support import (all_entries, FIELDS, most_outputs, OPTIONS, out_len, RATE, ratio, rerated, resampled_call, Stream,  # noqa: E402
    streams)
from multi_support import (FBANK_VARIANTS as VARIANTS, bits, fbank_call, mixed_entries, refused_entries, fbank_shape_of as  # noqa: E402
    shape_of)
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def pad_bits(spec):
    return int(np.float32(spec["pad_value"]).view(np.int32))


def by_hand(ctx, entries, frames, spec, truth=False, **opt):
    """capi.pcm_fbank over the mono resampled batch of the same entries, results["samples"] as L: what the call must equal.  With `truth`
    the rows are held to the float64 restatement of the delivered samples as well; -> (tensor, results[, largest error / bound])"""
    import torch
    from vorbispizza_amd import capi
    batch, results, _ = resampled_call(entries, spec["sample_rate"], 1, frames, True, False, True, **opt)
    dst = torch.full(shape_of(len(entries), frames, spec), 7.0, dtype=torch.float32, device="cuda:0")
    rows = [(k * frames, int(results["samples"][k]), k) for k in range(len(entries))]
    assert capi.pcm_fbank(ctx, batch.reshape(-1), rows, dst, capi.FbankSpec.make(**spec), frames) == capi.OK, ctx.last_error()
    ctx.synchronize()
    if not truth:
        return dst, results
    mono, img = batch.cpu().numpy()[:, 0, :], dst.cpu().numpy()
    img = img if spec["frames_first"] else img.transpose(0, 2, 1)
    W, B = ft.mel_weights64(spec), ft.operator64(spec)
    worst = max(ft.check_row(img[k], mono[k, : int(results["samples"][k])], spec, W, B) for k in range(len(entries)))
    return dst, results, worst


@pytest.mark.parametrize("variant", [0, 1], ids=["kaldi_log_frames_first", "hamming_power_bands_first"])
@pytest.mark.parametrize("route", list(OPTIONS))
def test_the_call_is_pcm_fbank_of_the_mono_resampled_batch(ctx, route, variant):
    import torch
    spec = VARIANTS[variant]
    entries = mixed_entries()
    frames = max(most_outputs(entries, RATE), spec["win"]) + 5
    want, want_results, worst = by_hand(ctx, entries, frames, spec, truth=True, **OPTIONS[route])
    print("largest error / bound against the truth of the delivered rows: %.4f" % worst)
    assert worst < 1.0
    got, results, _ = fbank_call(entries, frames, spec, **OPTIONS[route])
    assert torch.equal(bits(got), bits(want))
    for field in FIELDS:
        assert np.array_equal(results[field], want_results[field]), field
    J = results["samples"]
    assert (results["status"] == 0).all() and (J >= spec["win"]).any() and (J == 0).any()
    assert torch.isfinite(got).all()
    img = got.cpu().numpy()
    img = img if spec["frames_first"] else img.transpose(0, 2, 1)
    for k in range(len(entries)):  # the real frames follow from J; everything behind them is pad_value
        TL = ft.n_frames(int(J[k]), spec["win"], spec["hop"])
        assert (img[k, TL:].view(np.int32) == pad_bits(spec)).all() and (TL == 0 or (img[k, :TL].view(np.int32) != pad_bits(spec)).any())


def test_the_partition_the_cut_and_the_failure_paths_change_no_bit(ctx, monkeypatch):
    import torch
    spec = VARIANTS[0]
    entries = mixed_entries()
    frames = max(most_outputs(entries, RATE), spec["win"]) + 1
    one, one_results = by_hand(ctx, entries, frames, spec, gpu_entropy=False)
    for groups in (1, 2):
        for gpu_entropy in (False, True):
            got, results, _ = fbank_call(entries, frames, spec, device_ids=[0] * groups, streams_per_call=5, gpu_entropy=gpu_entropy, host_threads=2 * groups)
            assert torch.equal(bits(got), bits(one)), (groups, gpu_entropy)
            for field in FIELDS:
                if field != "device_slot":
                    assert np.array_equal(results[field], one_results[field]), field
    for switch, value in (("VPZM_MAX_CALL_VALUES", "40000"), ("VPZM_FAIL_BATCH_CALLS", "1"), ("VPZM_FAIL_GPU_ENTROPY", "1")):
        monkeypatch.setenv(switch, value)
        got, results, stats = fbank_call(entries, frames, spec, gpu_entropy=True, streams_per_call=64)
        monkeypatch.delenv(switch)
        assert torch.equal(bits(got), bits(one)), switch
        assert (sum(stats.device_gpu_entropy_streams[g] for g in range(16)) == 0) == (switch == "VPZM_FAIL_GPU_ENTROPY")
        for field in FIELDS:
            assert np.array_equal(results[field], one_results[field]), (switch, field)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_refused_entry_costs_only_itself_and_leaves_the_pad_row(ctx, gpu_entropy):
    import torch
    from vorbispizza_amd import multi
    entries, J = refused_entries()
    for spec in VARIANTS:
        want, _ = by_hand(ctx, entries, J, spec, gpu_entropy=gpu_entropy, streams_per_call=2)
        got, results, _ = fbank_call(entries, J, spec, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
        assert list(results["status"]) == [0, multi.E_RANGE, multi.E_CAPACITY, multi.E_OPEN, 0, multi.E_RATE, 0, 0]
        assert list(results["samples"]) == [J, 0, 0, 0, 200, 0, 0, J]
        assert results["channels"][4] == 1 and results["sample_rate"][5] == 44101
        assert torch.equal(bits(got), bits(want))
        img = got.cpu().numpy().view(np.int32)
        assert (img[[1, 2, 3, 5, 6]] == pad_bits(spec)).all()
        assert (img[[0, 7]] != pad_bits(spec)).any(axis=(1, 2)).all()
        # 200 samples: shorter than the Kaldi window -- all pad, status OK, samples = J --, two frames and more of the 96-sample one
        assert (img[4] == pad_bits(spec)).all() == (spec["win"] > 200)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_failed_fbank_launch_costs_its_members_e_synth_and_leaves_pad_rows(ctx, monkeypatch, gpu_entropy):
    """the entries of test_a_refused_entry_costs_only_itself_and_leaves_the_pad_row under VPZM_FAIL_DELIVERY (check_failed_delivery of
    test_multi_batch_gpu.py): the resample launches into the lane's temporary are made, the fbank launch is not"""
    import torch
    from multi_support import check_failed_delivery, sentinel_out
    from vorbispizza_amd import multi
    entries, J = refused_entries()
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        for spec in VARIANTS:
            check_failed_delivery(monkeypatch, d, lambda: fbank_call(entries, J, spec, dispatcher=d, out=sentinel_out(
                d, len(entries), lambda rows: shape_of(rows, J, spec), torch.float32, 77.0))[:2], pad_bits(spec), step="vpz_pcm_fbank")
    finally:
        d.close()


def test_a_wrong_out_tensor_raises_and_a_wrong_spec_is_refused(ctx):
    import torch
    from fbank_truth import refused_specs
    from vorbispizza_amd import capi, multi
    s = streams()["stereo_coupled_res2_12"]
    entries = [(s, a, n) for a, n in s.windows()[:6]]
    frames = max(most_outputs(entries, RATE), 400)
    spec = VARIANTS[0]
    T = 1 + (frames - 400) // 160
    d = multi.Dispatcher([0, 0], host_threads=2)
    try:
        good = [torch.zeros((3, T, 80), dtype=torch.float32, device="cuda:0") for _ in range(2)]
        got, _, _ = fbank_call(entries, frames, spec, dispatcher=d, out=good)
        assert torch.equal(bits(got), bits(fbank_call(entries, frames, spec, dispatcher=d)[0]))
        for bad in ([good[0]], [good[0], torch.zeros((3, 80, T), dtype=torch.float32, device="cuda:0")], [good[0], torch.zeros((3, T + 1, 80), device="cuda:0")],
                    [good[0], torch.zeros((4, T, 80), device="cuda:0")], [good[0], torch.zeros((3, T, 80), dtype=torch.float64, device="cuda:0")],
                    [good[0], torch.zeros((3, T, 80))], [good[0], torch.zeros((3, T, 160), device="cuda:0")[:, :, ::2]], [good[0], None]):
            marker = [t.clone() for t in bad if isinstance(t, torch.Tensor)]
            with pytest.raises(ValueError):
                d.decode_ranges_fbank([e[0].data for e in entries], [(a, n) for _, a, n in entries], frames, out=bad, **spec)
            assert all(torch.equal(a, b) for a, b in zip(marker, [t for t in bad if isinstance(t, torch.Tensor)]))  # (nothing was written)
        with pytest.raises(ValueError):  # (frames < win: no frame in a row)
            d.decode_ranges_fbank([e[0].data for e in entries], [(a, n) for _, a, n in entries], 399, **spec)
        # the library's own refusals: VPZM_E_ARG
        n_e = len(entries)
        ptrs = (C.c_void_p * n_e)(*[e[0].data.ctypes.data for e in entries])
        sizes = (C.c_uint64 * n_e)(*[e[0].data.size for e in entries])
        rng = np.array([(x, c) for _, x, c in entries], dtype=np.int64)
        res = np.zeros(n_e, dtype=multi.RESULT_DTYPE)
        whole = torch.zeros((n_e, T, 80), dtype=torch.float32, device="cuda:0")
        dst = (C.c_void_p * 2)(whole[:3].data_ptr(), whole[3:].data_ptr())
        ok = capi.FbankSpec.make(**spec)
        args = lambda **kw: [kw.get(k, v) for k, v in (("m", d._h), ("n", n_e), ("data", ptrs), ("size", sizes), ("ranges", rng.ctypes.data),  # noqa: E731
                                                       ("spec", C.byref(ok)), ("frames", frames), ("dst", dst), ("results", res.ctypes.data), ("stats", None))]
        L = multi.lib()
        assert L.vpzm_decode_ranges_fbank(*args()) == multi.OK
        changes = [dict(spec=None), dict(frames=0), dict(frames=399), dict(dst=None), dict(m=None), dict(results=None), dict(ranges=None), dict(n=-1)]
        changes += [dict(spec=C.byref(sp)) for _, sp in refused_specs(capi)]
        changes.append(dict(spec=C.byref(capi.FbankSpec.make(**dict(spec, sample_rate=16000.5)))))  # (no whole number of Hz)
        for change in changes:
            assert L.vpzm_decode_ranges_fbank(*args(**change)) == multi.E_ARG, change
    finally:
        d.close()


def test_the_calls_in_turn_on_one_dispatcher(ctx):
    """the lane's temporary and the context's tables serve call after call, between calls of the older kinds -- log-mel among them"""
    import torch
    from vorbispizza_amd import multi
    entries = mixed_entries()[::3]
    frames = max(most_outputs(entries, RATE), 400)
    wants = [by_hand(ctx, entries, frames, spec)[0] for spec in VARIANTS]
    mono = resampled_call(entries, RATE, 1, frames, True, False, True)[0]
    d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
    try:
        logmel = None
        for _ in range(2):
            for spec, want in zip(VARIANTS, wants):
                assert torch.equal(bits(fbank_call(entries, frames, spec, dispatcher=d)[0]), bits(want))
                assert torch.equal(bits(resampled_call(entries, RATE, 1, frames, True, False, True, dispatcher=d)[0]), bits(mono))
                mel = torch.cat(list(d.decode_ranges_logmel([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames, sample_rate=RATE)[0]))
                assert logmel is None or torch.equal(bits(mel), bits(logmel))
                logmel = mel
            # a shorter padded length: other rows in the same temporary
            short = [e for e in entries if out_len(e[0].f.window(e[1], e[2])["samples"], *ratio(e[0], RATE)) <= 500]
            assert len(short) > 10
            assert torch.equal(bits(fbank_call(short, 500, VARIANTS[0], dispatcher=d)[0]), bits(by_hand(ctx, short, 500, VARIANTS[0])[0]))
    finally:
        d.close()
