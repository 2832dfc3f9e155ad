"""vpzm_decode_ranges_fbank_post / vpzm_decode_ranges_mfcc_post (include/vorbispizza_multi_featpost.h, host/vorbis_multi.cpp): the
filterbank and MFCC window batches with Kaldi's feature post-processing behind them.

Streams and windows are those of tests/test_multi_fbank_gpu.py and tests/test_multi_mfcc_gpu.py (the synthetic streams and the golden
.ogg fixture among them).  The calls are the existing ones with one more stage, so what is checked of them is EQUALITY, bit for bit: the
tensor is capi.feat_post applied to the tensor the call returns without `post`, with every row's real frames taken from
results["samples"] -- on every route, partition, cut and failure path --, results and statuses are those of the call without `post`, and
without a post spec the new entry points are the old ones.  The kernel alone is held to the truth in tests/test_pcm_featpost_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fbank_truth as ft  # noqa: E402
import featpost_truth as pt  # noqa: E402
import multi_support as ms  # noqa: E402
from multi_support import bits, FIELDS, mixed_entries, most_outputs, OPTIONS, RATE, refused_entries, streams  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

# (kind, the feature spec, the post spec): add-deltas | apply-cmvn-sliding over Kaldi's MFCC defaults; apply-cmvn with variance, then
# deltas, over the HTK-order, columns-first MFCC spec with its own subtract_mean; deltas alone over 80 filterbank bands; a short
# uncentred window with variance over the columns-first mel power
CASES = [
    ("mfcc", ms.MFCC_VARIANTS[0], pt.spec_of(norm="sliding", cmn_window=30, min_window=10, center=True, delta_order=2, deltas_first=True, pad_value=-1.5)),
    ("mfcc", ms.MFCC_VARIANTS[1], pt.spec_of(norm="row", norm_vars=True, delta_order=1, delta_window=3, frames_first=False, pad_value=9.0)),
    ("fbank", ms.FBANK_VARIANTS[0], pt.spec_of(delta_order=3, delta_window=1)),
    ("fbank", ms.FBANK_VARIANTS[1], pt.spec_of(norm="sliding", cmn_window=20, min_window=5, norm_vars=True, frames_first=False, pad_value=2.0 ** -130)),
]
IDS = ["mfcc_deltas_sliding", "mfcc_cmvn_deltas_columns_first", "fbank_deltas", "fbank_sliding_vars_columns_first"]


def columns(kind, spec):
    return spec["n_ceps"] if kind == "mfcc" else spec["n_mels"]


def shape_of(n, frames, kind, spec, post):
    T, D_out = ft.n_frames(frames, spec["win"], spec["hop"]), columns(kind, spec) * (post["delta_order"] + 1)
    return (n, T, D_out) if spec["frames_first"] else (n, D_out, T)


def pad_bits(post):
    return int(np.float32(post["pad_value"]).view(np.int32))


def plain_call(kind, *a, **kw):
    return (ms.mfcc_call if kind == "mfcc" else ms.fbank_call)(*a, **kw)


def post_call(kind, entries, frames, spec, post, device_ids=(0,), dispatcher=None, out=None, **opt):
    """-> (the posted features as one tensor, results, stats)"""
    import torch
    from vorbispizza_amd import capi, multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        fn = d.decode_ranges_mfcc_post if kind == "mfcc" else d.decode_ranges_fbank_post
        parts, whole, results, stats = fn([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames,
                                          post=capi.FeatPostSpec.make(**post), out=out, **spec)
    finally:
        if dispatcher is None:
            d.close()
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == shape_of(len(entries), frames, kind, spec, post) and whole.dtype == torch.float32
    return whole, results, stats


def by_hand(ctx, kind, entries, frames, spec, post, **opt):
    """capi.feat_post over the tensor of the call without `post`, results["samples"] giving every row's real frames: what the posted call
    must equal.  -> (tensor, results of the call without post)"""
    import torch
    from vorbispizza_amd import capi
    plain, results, _ = plain_call(kind, entries, frames, spec, **opt)
    dst = torch.full(shape_of(len(entries), frames, kind, spec, post), 7.0, dtype=torch.float32, device="cuda:0")
    rows = [(k, ft.n_frames(int(results["samples"][k]), spec["win"], spec["hop"]), k) for k in range(len(entries))]
    assert capi.feat_post(ctx, plain.contiguous(), rows, dst, capi.FeatPostSpec.make(**post)) == capi.OK, ctx.last_error()
    ctx.synchronize()
    return dst, results


def same_results(a, b, but=()):
    for field in FIELDS:
        if field not in but:
            assert np.array_equal(a[field], b[field]), field


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("route", list(OPTIONS))
def test_the_posted_call_is_feat_post_of_the_call_without_post(ctx, route, case):
    import torch
    kind, spec, post = CASES[case]
    entries = mixed_entries()
    frames = max(most_outputs(entries, RATE), spec["win"]) + 5
    want, want_results = by_hand(ctx, kind, entries, frames, spec, post, **OPTIONS[route])
    got, results, _ = post_call(kind, entries, frames, spec, post, **OPTIONS[route])
    assert torch.equal(bits(got), bits(want))
    same_results(results, want_results)
    J = results["samples"]
    assert (results["status"] == 0).all() and (J >= spec["win"]).any() and (J == 0).any() and ((J > 0) & (J < frames)).any()
    assert torch.isfinite(got).all()
    img = got.cpu().numpy()
    img = img if spec["frames_first"] else img.transpose(0, 2, 1)
    for k in range(len(entries)):  # the real frames follow from J; everything behind them is the post spec's pad_value
        TL = ft.n_frames(int(J[k]), spec["win"], spec["hop"])
        assert (img[k, TL:].view(np.int32) == pad_bits(post)).all() and (TL < 2 or (img[k, :TL].view(np.int32) != pad_bits(post)).any())


def test_the_partition_the_cut_and_the_failure_paths_change_no_bit(ctx, monkeypatch):
    """two groups through vpzm_batch_partition, small sub-batches on both routes, and the switches that cut a call's values, fail the
    batch calls (the member-by-member path) and fail the device's entropy decode (the host route after all)"""
    import torch
    entries = mixed_entries()
    for kind, spec, post in CASES[:2]:
        frames = max(most_outputs(entries, RATE), spec["win"]) + 1
        one, one_results = by_hand(ctx, kind, entries, frames, spec, post, gpu_entropy=False)
        for groups in (1, 2):
            for gpu_entropy in (False, True):
                got, results, _ = post_call(kind, entries, frames, spec, post, device_ids=[0] * groups, streams_per_call=5, gpu_entropy=gpu_entropy,
                                            host_threads=2 * groups)
                assert torch.equal(bits(got), bits(one)), (groups, gpu_entropy)
                same_results(results, one_results, but=("device_slot",))
        for switch, value in (("VPZM_MAX_CALL_VALUES", "40000"), ("VPZM_FAIL_BATCH_CALLS", "1"), ("VPZM_FAIL_GPU_ENTROPY", "1")):
            monkeypatch.setenv(switch, value)
            got, results, stats = post_call(kind, entries, frames, spec, post, gpu_entropy=True, streams_per_call=64)
            monkeypatch.delenv(switch)
            assert torch.equal(bits(got), bits(one)), (kind, switch)
            same_results(results, one_results)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_refused_entry_costs_only_itself_and_leaves_the_pad_row(ctx, gpu_entropy):
    """entries out of range, over capacity, no Ogg, at a ratio the resampler refuses, and an empty window: their rows are the post spec's
    pad_value from a launch that reads nothing; 200 samples are fewer than the Kaldi window -- no real frame, status OK"""
    import torch
    from vorbispizza_amd import multi
    entries, J = refused_entries()
    for kind, spec, post in CASES:
        want, want_results = by_hand(ctx, kind, entries, J, spec, post, gpu_entropy=gpu_entropy, streams_per_call=2)
        got, results, _ = post_call(kind, entries, J, spec, post, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
        assert list(results["status"]) == [0, multi.E_RANGE, multi.E_CAPACITY, multi.E_OPEN, 0, multi.E_RATE, 0, 0]
        assert list(results["samples"]) == [J, 0, 0, 0, 200, 0, 0, J]
        same_results(results, want_results, but=("device_slot",))
        assert torch.equal(bits(got), bits(want))
        img = got.cpu().numpy().view(np.int32)
        assert (img[[1, 2, 3, 5, 6]] == pad_bits(post)).all()
        assert (img[[0, 7]] != pad_bits(post)).any(axis=(1, 2)).all()
        assert (img[4] == pad_bits(post)).all() == (spec["win"] > 200)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_failed_delivery_costs_its_members_e_synth_and_leaves_pad_rows(ctx, monkeypatch, gpu_entropy):
    """the entries of the test above under VPZM_FAIL_DELIVERY (check_failed_delivery of multi_support.py): the resample launches
    into the lane's temporary are made, the feature launch and the post launches behind it are not"""
    import torch
    from multi_support import check_failed_delivery, sentinel_out
    from vorbispizza_amd import multi
    entries, J = refused_entries()
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        for kind, spec, post in CASES[:3]:
            check_failed_delivery(monkeypatch, d, lambda: post_call(kind, entries, J, spec, post, dispatcher=d, out=sentinel_out(
                d, len(entries), lambda rows: shape_of(rows, J, kind, spec, post), torch.float32, 77.0))[:2], pad_bits(post), step="vpz_pcm_" + kind)
    finally:
        d.close()


def test_without_a_post_spec_the_new_entry_points_are_the_old_ones(ctx):
    import torch
    from vorbispizza_amd import capi, multi
    entries = mixed_entries()[::2]
    n_e = len(entries)
    d = multi.Dispatcher([0], host_threads=4, streams_per_call=8, gpu_entropy=True)
    try:
        for kind, spec, _ in CASES:
            frames = max(most_outputs(entries, RATE), spec["win"]) + 3
            old, old_results, _ = plain_call(kind, entries, frames, spec, dispatcher=d)
            fn = d.decode_ranges_mfcc_post if kind == "mfcc" else d.decode_ranges_fbank_post
            parts, whole, results, _ = fn([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames, post=None, **spec)
            assert torch.equal(bits(whole), bits(old))
            same_results(results, old_results, but=("device_slot",))
            # and the C entry point with a null post spec
            ptrs = (C.c_void_p * n_e)(*[e[0].data.ctypes.data for e in entries])
            sizes = (C.c_uint64 * n_e)(*[e[0].data.size for e in entries])
            rng = np.array([(x, c) for _, x, c in entries], dtype=np.int64)
            res = np.zeros(n_e, dtype=multi.RESULT_DTYPE)
            raw = torch.full(tuple(old.shape), 5.0, dtype=torch.float32, device="cuda:0")
            dst = (C.c_void_p * 1)(raw.data_ptr())
            made = (capi.MfccSpec if kind == "mfcc" else capi.FbankSpec).make(**spec)
            call = multi.lib().vpzm_decode_ranges_mfcc_post if kind == "mfcc" else multi.lib().vpzm_decode_ranges_fbank_post
            torch.cuda.synchronize()
            assert call(d._h, n_e, ptrs, sizes, rng.ctypes.data, C.byref(made), None, frames, dst, res.ctypes.data, None) == multi.OK
            assert torch.equal(bits(raw), bits(old))
            same_results(res, old_results, but=("device_slot",))
    finally:
        d.close()


def test_a_wrong_out_tensor_raises_and_a_wrong_post_spec_is_refused(ctx):
    import torch
    from featpost_truth import refused_specs
    from vorbispizza_amd import capi, multi
    s = streams()["stereo_coupled_res2_12"]
    entries = [(s, a, n) for a, n in s.windows()[:6]]
    frames = max(most_outputs(entries, RATE), 400)
    kind, spec, post = CASES[0]
    T = 1 + (frames - 400) // 160
    datas, ranges = [e[0].data for e in entries], [(a, n) for _, a, n in entries]
    d = multi.Dispatcher([0, 0], host_threads=2)
    try:
        good = [torch.zeros((3, T, 39), dtype=torch.float32, device="cuda:0") for _ in range(2)]
        got, _, _ = post_call(kind, entries, frames, spec, post, dispatcher=d, out=good)
        assert torch.equal(bits(got), bits(post_call(kind, entries, frames, spec, post, dispatcher=d)[0]))
        made = capi.FeatPostSpec.make(**post)
        for bad in ([good[0]], [good[0], torch.zeros((3, 39, T), dtype=torch.float32, device="cuda:0")], [good[0], torch.zeros((3, T, 13), device="cuda:0")],
                    [good[0], torch.zeros((4, T, 39), device="cuda:0")], [good[0], torch.zeros((3, T, 39), dtype=torch.float64, device="cuda:0")],
                    [good[0], torch.zeros((3, T, 39))], [good[0], torch.zeros((3, T, 78), device="cuda:0")[:, :, ::2]], [good[0], None]):
            marker = [t.clone() for t in bad if isinstance(t, torch.Tensor)]
            with pytest.raises(ValueError):
                d.decode_ranges_mfcc_post(datas, ranges, frames, post=made, out=bad, **spec)
            assert all(torch.equal(a, b) for a, b in zip(marker, [t for t in bad if isinstance(t, torch.Tensor)]))  # (nothing was written)
        with pytest.raises(ValueError):  # (the other layout than the feature spec's)
            d.decode_ranges_mfcc_post(datas, ranges, frames, post=capi.FeatPostSpec.make(**dict(post, frames_first=False)), **spec)
        with pytest.raises(ValueError):  # (frames < win: no frame in a row)
            d.decode_ranges_mfcc_post(datas, ranges, 399, post=made, **spec)
        with pytest.raises(TypeError):
            d.decode_ranges_mfcc_post(datas, ranges, frames, post=post, **spec)
        # the library's own refusals: VPZM_E_ARG
        n_e = len(entries)
        ptrs = (C.c_void_p * n_e)(*[e.ctypes.data for e in datas])
        sizes = (C.c_uint64 * n_e)(*[e.size for e in datas])
        rng = np.array(ranges, dtype=np.int64)
        res = np.zeros(n_e, dtype=multi.RESULT_DTYPE)
        whole = torch.zeros((n_e, T, 39), dtype=torch.float32, device="cuda:0")
        dst = (C.c_void_p * 2)(whole[:3].data_ptr(), whole[3:].data_ptr())
        ok = capi.MfccSpec.make(**spec)
        args = lambda **kw: [kw.get(k, v) for k, v in (("m", d._h), ("n", n_e), ("data", ptrs), ("size", sizes), ("ranges", rng.ctypes.data),  # noqa: E731
                                                       ("spec", C.byref(ok)), ("post", C.byref(made)), ("frames", frames), ("dst", dst),
                                                       ("results", res.ctypes.data), ("stats", None))]
        L = multi.lib()
        torch.cuda.synchronize()
        assert L.vpzm_decode_ranges_mfcc_post(*args()) == multi.OK
        assert torch.equal(bits(whole), bits(got))
        changes = [dict(spec=None), dict(frames=399), dict(dst=None), dict(m=None), dict(results=None), dict(ranges=None), dict(n=-1)]
        refused = refused_specs(capi)
        changes += [dict(post=C.byref(sp)) for _, sp in refused]
        changes.append(dict(post=C.byref(capi.FeatPostSpec.make(**dict(post, frames_first=False)))))
        before = whole.clone()
        for change in changes:
            assert L.vpzm_decode_ranges_mfcc_post(*args(**change)) == multi.E_ARG, change
        fbank_ok = capi.FbankSpec.make(**CASES[2][1])
        assert L.vpzm_decode_ranges_fbank_post(*args(spec=C.byref(fbank_ok), post=C.byref(refused[0][1]))) == multi.E_ARG
        torch.cuda.synchronize()
        assert torch.equal(bits(whole), bits(before))
    finally:
        d.close()


def test_the_calls_in_turn_on_one_dispatcher(ctx):
    """the lane's two temporaries and its scratch memory serve call after call, between calls of the kinds without a post spec"""
    import torch
    from vorbispizza_amd import multi
    entries = mixed_entries()[::3]
    frames = max(most_outputs(entries, RATE), 400)
    wants = [by_hand(ctx, kind, entries, frames, spec, post)[0] for kind, spec, post in CASES]
    d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
    try:
        plain = None
        for _ in range(2):
            for (kind, spec, post), want in zip(CASES, wants):
                assert torch.equal(bits(post_call(kind, entries, frames, spec, post, dispatcher=d)[0]), bits(want))
                now = plain_call("mfcc", entries, frames, ms.MFCC_VARIANTS[0], dispatcher=d)[0]
                assert plain is None or torch.equal(bits(now), bits(plain))
                plain = now
    finally:
        d.close()
