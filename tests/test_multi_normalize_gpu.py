"""vpzm_decode_ranges_normalized (include/vorbispizza_multi_normalize.h, host/vorbis_multi.cpp) through vorbispizza_amd.normalize: the
resampled device batch delivered normalised.  The streams and windows are those of the resampled call's tests; what a row must be is
vpz_pcm_normalize (held to its own truth in tests/test_pcm_normalize_gpu.py) applied to the planar float32 batch of the resampled call,
and the loudness mode's measurement is vpzm_measure_loudness's: everything is compared as raw bits."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_support import (all_entries, as_bits, check_failed_delivery, entries_of, FIELDS, measure_call, most_outputs, OPTIONS, RATE,  # noqa: E402
    rerated, resampled_call, sentinel_out, Stream, streams)
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

LAYOUTS = ((True, False), (False, False), (True, True), (False, True))  # (planar, int16)
# every mode, with and without a ceiling; the targets are loud enough for both branches of the ceiling to occur among the windows
LEVELS = (dict(mode="meanvar"), dict(mode="peak", target=0.5), dict(mode="peak", target=0.9, ceiling=0.5), dict(mode="rms", target=0.1),
          dict(mode="rms", target=0.2, ceiling=0.3), dict(mode="gain", target=1.7), dict(mode="gain", target=3.0, ceiling=0.25),
          dict(mode="loudness", target=-23.0), dict(mode="loudness", target=-14.0, ceiling=0.2))


def normalized_call(entries, rate, channels, frames, planar=True, s16=False, mono=False, device_ids=(0,), dispatcher=None, out=None, level=None,
                    **opt):
    """-> (the batch as one tensor, the results dict, stats)"""
    import torch
    from vorbispizza_amd import multi, normalize
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        parts, whole, results, stats = normalize.decode_ranges_normalized(d, [s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], channels,
                                                                         frames, rate, mono=mono, planar=planar, s16=s16, out=out, **(level or {}))
    finally:
        if dispatcher is None:
            d.close()
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == ((len(entries), channels, frames) if planar else (len(entries), frames, channels))
    assert whole.dtype == (torch.int16 if s16 else torch.float32)
    return whole, results, stats


def loud_entries():
    """stereo windows of which some are long enough to have a loudness (the 8 000 Hz stream's 0.6 s) and most are not"""
    s = rerated(8000, 30)
    assert s.total >= 6 * 800
    long_ones = [(s, 0, -1), (s, s.bounds[2], 5 * 800 + 3), (s, s.bounds[1] + 1, 4 * 800), (s, s.bounds[3], 4 * 800 - 1)]
    entries = entries_of(2)[::4] + [(s, s.total, 10)]  # (and an empty window)
    for i, e in enumerate(long_ones):
        entries.insert(2 + 5 * i, e)
    return entries


def stage_on(ctx, batch, samples, channels, frames, planar, s16, level, gains=None):
    """capi.pcm_normalize over the planar float32 resampled batch [n, C, frames]: -> (tensor in the layout, results [n, 5])"""
    import torch
    from vorbispizza_amd import capi
    n = batch.shape[0]
    dst = torch.full((n, channels, frames) if planar else (n, frames, channels), 99, dtype=torch.int16 if s16 else torch.float32, device="cuda:0")
    spec = capi.NormSpec.make(level["mode"], channels=channels, target=level.get("target"), eps=level.get("eps", 1e-7), ceiling=level.get("ceiling", 0.0))
    if gains is None:
        gains = [level.get("target", 1.0)] * n
    rc, res = capi.pcm_normalize(ctx, batch.contiguous(), [(k * channels * frames, int(samples[k]), k) for k in range(n)], dst, spec, frames, gains=gains,
                                 results=True)
    assert rc == capi.OK, ctx.last_error()
    return dst, res


@pytest.mark.parametrize("route", ["host", "device"])
def test_unit_gain_is_the_resampled_call_bit_for_bit(ctx, route):  # noqa: F811
    import torch
    entries = entries_of(2)
    frames = most_outputs(entries, RATE) + 3
    assert len({s.f.sample_rate for s, _, _ in entries}) >= 2  # mixed rates in one call
    for planar, s16 in LAYOUTS:
        want, want_results, _ = resampled_call(entries, RATE, 2, frames, planar, s16, **OPTIONS[route])
        got, results, _ = normalized_call(entries, RATE, 2, frames, planar, s16, level=dict(mode="gain", target=1.0), **OPTIONS[route])
        assert torch.equal(as_bits(got), as_bits(want)), (planar, s16)
        for field in FIELDS:
            assert np.array_equal(results[field], want_results[field]), field
        assert (results["gain"] == 1.0).all() and (results["mean"] == 0.0).all() and (results["loudness"] == -np.inf).all()
    # mono from stereo, six channels and mono, every stream in one call; the peak is the resampled row's
    entries = all_entries()
    frames = most_outputs(entries, RATE)
    want, want_results, _ = resampled_call(entries, RATE, 1, frames, True, False, True, **OPTIONS[route])
    got, results, _ = normalized_call(entries, RATE, 1, frames, True, False, True, level=dict(mode="gain", target=1.0), **OPTIONS[route])
    assert torch.equal(as_bits(got), as_bits(want)) and np.array_equal(results["samples"], want_results["samples"])
    assert np.array_equal(results["peak"], want.abs().amax(dim=(1, 2)).cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("route", ["host", "device"])
def test_every_mode_is_the_stage_on_the_resampled_batch(ctx, route):  # noqa: F811
    import torch
    entries = loud_entries()
    frames = most_outputs(entries, RATE) + 5
    batch, plain, _ = resampled_call(entries, RATE, 2, frames, True, False, **OPTIONS[route])
    measured = measure_call(entries, **OPTIONS[route])[0]
    assert np.isfinite(measured["integrated"]).sum() >= 2 and np.isinf(measured["integrated"]).sum() >= 5
    clipped = {}
    for i, level in enumerate(LEVELS):
        planar, s16 = LAYOUTS[i % 4]
        got, results, _ = normalized_call(entries, RATE, 2, frames, planar, s16, level=level, **OPTIONS[route])
        for field in FIELDS:
            assert np.array_equal(results[field], plain[field]), (level, field)
        if level["mode"] == "loudness":
            # the measurement is measure_loudness's bit for bit; the gain is its definition's; a window shorter than 400 ms gets gain 1
            L = results["loudness"]
            assert np.array_equal(L.view(np.uint64), measured["integrated"].view(np.uint64)), level
            free = np.array([10.0 ** ((level["target"] - v) / 20.0) if np.isfinite(v) else 1.0 for v in L])
            if "ceiling" not in level:
                assert (np.abs(results["gain"] / free - 1.0) <= 1e-12).all(), (results["gain"], free)
                assert (results["gain"][np.isinf(L)] == 1.0).all()
            assert (results["gain"] <= free * (1 + 1e-12)).all()  # (a ceiling only lowers it)
            # the rows are the stage's in GAIN mode with the REPORTED gains
            want, res = stage_on(ctx, batch, plain["samples"], 2, frames, planar, s16, dict(mode="gain"), gains=results["gain"])
            clipped[i] = results["gain"] < free * (1 - 1e-6)
        else:
            assert (results["loudness"] == -np.inf).all()
            want, res = stage_on(ctx, batch, plain["samples"], 2, frames, planar, s16, level)
            assert np.array_equal(results["gain"].view(np.uint64), res[:, 4].view(np.uint64)), level
            if "ceiling" in level:
                clipped[i] = results["gain"] * results["peak"] >= level["ceiling"] * (1 - 1e-6)
        assert torch.equal(as_bits(got), as_bits(want)), level
        assert np.array_equal(results["mean"].view(np.uint64), res[:, 3].view(np.uint64)), level
        assert np.array_equal(results["peak"].view(np.uint64), res[:, 2].view(np.uint64)), level
        assert np.array_equal(results["gain"].astype(np.float32), res[:, 4].astype(np.float32)), level  # the row's float32 gain
        silent = plain["samples"] == 0
        assert silent.any() and (results["gain"][silent] == 1.0).all() and (results["peak"][silent] == 0.0).all()
    live = plain["samples"] > 0
    print({LEVELS[i]["mode"]: "%d of %d rows at the ceiling" % (int(hit[live].sum()), int(live.sum())) for i, hit in clipped.items()})
    assert any(hit[live].any() for hit in clipped.values()) and any((~hit[live]).any() for hit in clipped.values())


def test_the_partition_the_route_and_the_cut_change_no_byte(ctx):  # noqa: F811
    import torch
    entries = loud_entries()
    frames = most_outputs(entries, RATE)
    for level in (dict(mode="meanvar"), dict(mode="loudness", target=-20.0, ceiling=0.5)):
        one, one_results, _ = normalized_call(entries, RATE, 2, frames, False, False, level=level, gpu_entropy=False)
        assert one.abs().max() > 0
        for groups in (1, 2, 4):
            for streams_per_call in (3, 64):
                for gpu_entropy in (False, True):
                    got, results, _ = normalized_call(entries, RATE, 2, frames, False, False, level=level, device_ids=[0] * groups,
                                                      streams_per_call=streams_per_call, gpu_entropy=gpu_entropy, host_threads=2 * groups)
                    assert torch.equal(as_bits(got), as_bits(one)), (level, groups, streams_per_call, gpu_entropy)
                    for field in list(FIELDS) + ["gain", "mean", "peak", "loudness"]:
                        if field != "device_slot":
                            assert np.array_equal(results[field], one_results[field]), (level, field)


def bad_entries():
    """the resampled call's mix: entries 1 and 3 outside their stream, 4 one output sample too long, 5 no Ogg, 6 mono in a stereo batch,
    7 an empty window, 8 a refused ratio; entry 10 (4 000 Hz: a ratio the resampler takes, a rate the loudness measurement refuses)"""
    from multi_support import out_len, ratio
    s, mono, odd, slow = streams()["stereo_coupled_res2_30"], streams()["mono_floor1_res1_12"], rerated(44101), rerated(4000)
    garbage = Stream.__new__(Stream)
    garbage.data = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    up, down = ratio(s, RATE)
    a, n = s.bounds[3] + 7, 7 * down
    J = out_len(n, up, down)
    assert math.gcd(44101, RATE) == 1 and out_len(n + 1, up, down) == J + 1 and out_len(40, *ratio(slow, RATE)) <= J
    return [(s, a, n), (s, -1, n), (s, a, n - 2), (s, s.total + 1, n), (s, a, n + 1), (garbage, a, n), (mono, 5, 100), (s, s.total, 10), (odd, 3, 500),
            (s, a + 1, n), (slow, 3, 40)], J


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_bad_entry_costs_only_itself_and_has_the_empty_record(ctx, gpu_entropy):  # noqa: F811
    from vorbispizza_amd import multi
    entries, J = bad_entries()
    own = [0, multi.E_RANGE, 0, multi.E_RANGE, multi.E_CAPACITY, multi.E_OPEN, multi.E_CHANNELS, 0, multi.E_RATE, 0]
    for level, last in ((dict(mode="meanvar"), 0), (dict(mode="loudness"), multi.E_RATE), (dict(mode="peak", target=0.5, ceiling=0.4), 0)):
        for planar, s16 in ((True, False), (False, True)):
            got, results, _ = normalized_call(entries, RATE, 2, J, planar, s16, level=level, device_ids=(0, 0), host_threads=3, streams_per_call=2,
                                              gpu_entropy=gpu_entropy)
            assert list(results["status"]) == own + [last], (level, results["status"])
            plain = resampled_call(entries, RATE, 2, J, planar, s16, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)[1]
            ok = results["status"] == 0
            assert np.array_equal(results["samples"][ok], plain["samples"][ok]) and (results["samples"][~ok] == 0).all()
            img = got.cpu().numpy() if planar else got.cpu().numpy().transpose(0, 2, 1)
            nothing = ~ok | (results["samples"] == 0)
            assert nothing.sum() >= 7 and not img[nothing].any() and img[~nothing].any()
            for field, value in (("gain", 1.0), ("mean", 0.0), ("peak", 0.0), ("loudness", -np.inf)):
                assert (results[field][nothing] == value).all(), (level, field, results[field])
            assert (results["peak"][~nothing] > 0).all()


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_failed_normalize_launch_costs_its_members_e_synth_and_leaves_zero_rows(ctx, monkeypatch, gpu_entropy):  # noqa: F811
    import torch
    from vorbispizza_amd import multi
    entries, J = bad_entries()
    entries = entries[:10]
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        for (planar, s16), level in (((True, False), dict(mode="meanvar")), ((False, True), dict(mode="loudness", ceiling=0.5))):
            dtype, shape = (torch.int16 if s16 else torch.float32), (lambda rows: (rows, 2, J) if planar else (rows, J, 2))
            records = []

            def run():
                got, results, _ = normalized_call(entries, RATE, 2, J, planar, s16, dispatcher=d, level=level,
                                                  out=sentinel_out(d, len(entries), shape, dtype, 77))
                records.append(results)
                return got, results

            check_failed_delivery(monkeypatch, d, run, 0, step="vpz_pcm_normalize")
            failed = records[1]  # (plain, failed, plain again)
            assert (failed["gain"] == 1.0).all() and (failed["peak"] == 0.0).all() and (failed["loudness"] == -np.inf).all()
            assert np.array_equal(records[0]["gain"], records[2]["gain"]) and (records[0]["peak"] > 0).any()
    finally:
        d.close()


def test_what_the_call_refuses(ctx):  # noqa: F811
    import torch
    from vorbispizza_amd import multi, normalize
    entries = entries_of(2)[:6]
    n, frames = len(entries), most_outputs(entries[:6], RATE)
    d = multi.Dispatcher([0], host_threads=2)
    try:
        ptrs = (C.c_void_p * n)(*[e[0].data.ctypes.data for e in entries])
        sizes = (C.c_uint64 * n)(*[e[0].data.size for e in entries])
        rng = np.array([(x, c) for _, x, c in entries], dtype=np.int64)
        res = np.zeros(n, dtype=multi.RESULT_DTYPE)
        out = np.zeros(n, dtype=normalize.NORM_OUT_DTYPE)
        got = torch.zeros((n, 2, frames), dtype=torch.float32, device="cuda:0")
        dst = (C.c_void_p * 1)(got.data_ptr())
        nan, inf = float("nan"), float("inf")

        def spec_of(mode=1, target=1.0, eps=1e-7, ceiling=0.0, word=0):
            s = normalize.MultiNormSpec()
            s.mode, s.target, s.eps, s.ceiling = mode, target, eps, ceiling
            s.reserved[8] = word
            return s

        def call(spec=spec_of(), **kw):
            args = [kw.get(k, v) for k, v in (("m", d._h), ("n", n), ("data", ptrs), ("size", sizes), ("ranges", rng.ctypes.data), ("rate", RATE),
                                              ("channels", 2), ("downmix", 0), ("frames", frames), ("layout", 1), ("dst", dst),
                                              ("results", res.ctypes.data), ("stats", None))]
            return multi.lib().vpzm_decode_ranges_normalized(*args, None if spec is None else C.byref(spec), kw.get("out", out.ctypes.data))

        assert call() == multi.OK and (res["status"] == 0).all() and call(out=None) == multi.OK
        for change in (dict(rate=0), dict(downmix=2), dict(downmix=1), dict(channels=0), dict(frames=0), dict(layout=4), dict(layout=-1), dict(dst=None),
                       dict(m=None), dict(results=None), dict(ranges=None), dict(n=-1)):
            assert call(**change) == multi.E_ARG, change
        for spec in (None, spec_of(mode=0), spec_of(mode=6), spec_of(mode=2, target=0.0), spec_of(mode=3, target=-1.0), spec_of(mode=4, target=nan),
                     spec_of(mode=4, target=0.0), spec_of(mode=5, target=inf), spec_of(mode=5, target=nan), spec_of(eps=-1e-9), spec_of(eps=nan),
                     spec_of(mode=2, ceiling=-1.0), spec_of(mode=3, ceiling=inf), spec_of(ceiling=0.5), spec_of(word=1)):
            assert call(spec) == multi.E_ARG, None if spec is None else (spec.mode, spec.target, spec.eps, spec.ceiling)
        assert call(spec_of(mode=5, target=-60.0)) == multi.OK and call(spec_of(mode=1, target=nan)) == multi.OK  # (targets their modes take)
        with pytest.raises(ValueError):
            normalize.decode_ranges_normalized(d, [], [], 2, 8, RATE, mode="lufs")
        with pytest.raises(ValueError):
            normalize.decode_ranges_normalized(d, [], [], 2, 8, RATE, mono=True)
    finally:
        d.close()
