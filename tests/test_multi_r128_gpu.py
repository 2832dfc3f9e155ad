"""vpzm_measure_r128 (include/vorbispizza_multi_r128.h, host/vorbis_multi.cpp): windows of streams measured for everything an EBU R 128
scanner reports, on the device.

Entries and option sets are those of tests/test_multi_loudness_gpu.py.  The call is vpzm_measure_loudness with one more launch in its
delivery, so what is checked of it is EQUALITY, bit for bit: a record's integrated, sample_peak, steps and blocks_kept are
measure_loudness's; its true_peak is capi.pcm_true_peak of the interleaved float32 row decode_ranges_batch delivers for the same range;
its range and maxima are capi.loudness_range and capi.loudness_maxima of capi.pcm_loudness's sums of that row -- on every route,
partition, cut and failure path.  The kernel alone is held to its truth in tests/test_pcm_true_peak_gpu.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loudness_truth as lt  # noqa: E402
from multi_support import (batch_call, FIELDS, loudness_entries, loudness_refused_entries as refused_entries, measure_call as  # noqa: E402
    loudness_call, most_samples, OPTIONS, rerated, streams)
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

EMPTY = (-np.inf, 0.0, -np.inf, -np.inf, -np.inf, -np.inf, 0.0, 0.0, 0, 0, 0)


def r128_call(entries, device_ids=(0,), dispatcher=None, ranges=True, **opt):
    """-> (records [n] as an R128_DTYPE array, results, stats)"""
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        results, rec, stats = d.measure_r128([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries] if ranges else None)
    finally:
        if dispatcher is None:
            d.close()
    assert rec.dtype == multi.R128_DTYPE and rec.shape == (len(entries),)
    return rec, results, stats


def by_hand(ctx, entries, **opt):
    """capi.pcm_loudness, capi.pcm_true_peak and the three host functions over the interleaved float32 batch of the same ranges, one batch
    call per channel count and one launch of each per rate: what the call must equal.  -> (records, results)"""
    from vorbispizza_amd import capi, multi
    rec = np.zeros(len(entries), dtype=multi.R128_DTYPE)
    rec[:] = EMPTY
    results = np.zeros(len(entries), dtype=multi.RESULT_DTYPE)
    for channels in sorted({s.channels for s, _, _ in entries}):
        at = [k for k, (s, _, _) in enumerate(entries) if s.channels == channels]
        sub = [entries[k] for k in at]
        frames = max(most_samples(sub), 1)
        batch, res, _ = batch_call(sub, channels, frames, planar=False, **opt)
        results[at] = res
        flat = batch.reshape(-1)
        for rate in sorted({int(r) for r in res["sample_rate"]}):
            rows = [(i * frames * channels, int(res["samples"][i]), i) for i in range(len(sub)) if res["sample_rate"][i] == rate and res["samples"][i] > 0]
            if not rows:
                continue
            S = lt.step_of(rate)
            sums, peak = capi.pcm_loudness(ctx, flat, channels, rate, rows, max_steps=frames // S + 3)
            tp, sp = capi.pcm_true_peak(ctx, flat, channels, rate, rows)
            ctx.synchronize()
            sums, peak, tp, sp = sums.cpu().numpy(), peak.cpu().numpy(), tp.cpu().numpy(), sp.cpu().numpy()
            for _, L, i in rows:
                assert sp[i] == peak[i]
                own = sums[i, : L // S]
                lufs, kept = capi.loudness_gate(own, S)
                lra, low, high, blocks = capi.loudness_range(own, S)
                mom, short = capi.loudness_maxima(own, S)
                rec[at[i]] = (lufs, lra, low, high, mom, short, float(tp[i]), float(peak[i]), L // S, kept, blocks)
    return rec, results


def same_records(a, b):
    return a.tobytes() == b.tobytes()


def the_loudness_part(rec):
    from vorbispizza_amd import multi
    out = np.zeros(len(rec), dtype=multi.LOUDNESS_DTYPE)
    out["integrated"], out["peak"], out["steps"], out["blocks_kept"] = rec["integrated"], rec["sample_peak"], rec["steps"], rec["blocks_kept"]
    return out


def long_entries():
    """the loudness tests' entries and a stream long enough for a 3 s block: the stereo setup at 8 000 Hz with 60 packets"""
    entries = loudness_entries()
    s = rerated(8000, 60)
    assert s.total >= 32 * 800
    entries.insert(5, (s, 0, -1))
    entries.insert(40, (s, s.bounds[2] + 3, 31 * 800 + 5))
    return entries


@pytest.mark.parametrize("route", list(OPTIONS))
def test_every_record_is_the_kernels_and_the_host_functions_of_the_batch_row(ctx, route):
    entries = long_entries()
    want, want_results = by_hand(ctx, entries, **OPTIONS[route])
    got, results, _ = r128_call(entries, **OPTIONS[route])
    assert same_records(got, want)
    for field in FIELDS:
        assert np.array_equal(results[field], want_results[field]), field
    assert (results["status"] == 0).all()
    # the loudness part is measure_loudness's, bit for bit
    loud, loud_results, _ = loudness_call(entries, **OPTIONS[route])
    assert same_records(the_loudness_part(got), loud)
    for field in FIELDS:
        assert np.array_equal(results[field], loud_results[field]), field
    # what follows from the definitions
    assert (got["true_peak"].astype(np.float32).view(np.uint32) >= got["sample_peak"].astype(np.float32).view(np.uint32)).all()
    assert (got["true_peak"] == got["true_peak"].astype(np.float32)).all() and (got["true_peak"] > got["sample_peak"]).sum() > len(entries) // 2
    assert (got["range_blocks"] > 0).sum() >= 2 and ((got["range_blocks"] == 0) == np.isneginf(got["range_low"])).all()
    assert (got["range_blocks"][got["steps"] < 30] == 0).all() and (got["range"] >= 0).all() and (got["range_high"] >= got["range_low"]).all()
    assert np.isneginf(got["momentary_max"][got["steps"] < 4]).all() and np.isfinite(got["momentary_max"][got["steps"] >= 4]).all()
    assert (got["momentary_max"] >= got["short_term_max"]).all() and (got["steps"] >= 4).sum() >= 4
    assert (np.isneginf(got["short_term_max"][got["steps"] < 30])).all() and np.isfinite(got["short_term_max"][got["steps"] >= 30]).all()
    empty = results["samples"] == 0
    assert same_records(got[empty], np.array([EMPTY] * int(empty.sum()), dtype=got.dtype))


def test_the_partition_the_cut_and_the_failure_paths_change_no_bit(ctx, monkeypatch):
    entries = long_entries()
    one, one_results = by_hand(ctx, entries, gpu_entropy=False)
    for groups, gpu_entropy in ((2, False), (2, True), (4, True)):
        got, results, _ = r128_call(entries, device_ids=[0] * groups, streams_per_call=5, gpu_entropy=gpu_entropy, host_threads=2 * groups)
        assert same_records(got, one), (groups, gpu_entropy)
        for field in FIELDS:
            if field != "device_slot":
                assert np.array_equal(results[field], one_results[field]), field
    got, _, _ = r128_call(entries, streams_per_call=7, **OPTIONS["mixed"])
    assert OPTIONS["mixed"]["mixed_setups"] and same_records(got, one)
    for switch, value in (("VPZM_MAX_CALL_VALUES", "40000"), ("VPZM_FAIL_BATCH_CALLS", "1"), ("VPZM_FAIL_GPU_ENTROPY", "1")):
        monkeypatch.setenv(switch, value)
        got, results, stats = r128_call(entries, gpu_entropy=True, streams_per_call=64)
        monkeypatch.delenv(switch)
        assert same_records(got, one), switch
        assert (sum(stats.device_gpu_entropy_streams[g] for g in range(16)) == 0) == (switch == "VPZM_FAIL_GPU_ENTROPY")
        for field in FIELDS:
            if field != "device_slot":
                assert np.array_equal(results[field], one_results[field]), (switch, field)


def test_no_ranges_are_whole_streams(ctx):
    names = ["stereo_coupled_res2_30", "mono_floor1_res1_12", "six_channels_51_12", "1test.ogg"]
    whole = [(streams()[name], 0, -1) for name in names] + [(rerated(8000, 60), 0, -1), (rerated(48000), 0, -1)]
    for gpu_entropy in (False, True):
        with_ranges, res_a, _ = r128_call(whole, gpu_entropy=gpu_entropy)
        without, res_b, _ = r128_call(whole, ranges=False, gpu_entropy=gpu_entropy)
        assert same_records(with_ranges, without)
        for field in FIELDS:
            assert np.array_equal(res_a[field], res_b[field]), field
        assert list(res_b["samples"]) == [s.total for s, _, _ in whole] and (res_b["status"] == 0).all()
        assert np.isfinite(without["integrated"][4]) and without["range_blocks"][4] > 0 and np.isfinite(without["short_term_max"][4])
        # streams of two rates and two channel counts (and more) in the one call
        assert len({int(r) for r in res_b["sample_rate"]}) >= 2 and len({int(c) for c in res_b["channels"]}) >= 2


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_refused_entry_costs_only_itself_and_gets_the_empty_record(ctx, gpu_entropy):
    from vorbispizza_amd import multi
    entries = refused_entries()
    n = entries[0][2]
    good = [e if k in (0, 5, 6, 7) else entries[5] for k, e in enumerate(entries)]
    want, _ = by_hand(ctx, good, gpu_entropy=gpu_entropy, streams_per_call=2)
    got, results, _ = r128_call(entries, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    assert list(results["status"]) == [0, multi.E_RANGE, multi.E_OPEN, multi.E_RATE, multi.E_RATE, 0, 0, 0]
    assert list(results["samples"]) == [n, 0, 0, 0, 0, 0, 100, n]
    assert same_records(got, want)
    assert same_records(got[[1, 2, 3, 4, 5]], np.array([EMPTY] * 5, dtype=got.dtype))
    assert list(got["steps"][[0, 6, 7]]) == [5, 0, 5] and np.isfinite(got["integrated"][[0, 7]]).all() and np.isfinite(got["momentary_max"][[0, 7]]).all()
    # 100 samples: peaks, no step
    assert got["integrated"][6] == -np.inf and got["true_peak"][6] >= got["sample_peak"][6] > 0 and got["momentary_max"][6] == -np.inf


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_failed_launch_costs_its_members_e_synth_and_leaves_empty_records(ctx, monkeypatch, gpu_entropy):
    from vorbispizza_amd import multi
    entries = refused_entries()
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        monkeypatch.delenv("VPZM_FAIL_DELIVERY", raising=False)
        plain, plain_results, _ = r128_call(entries, dispatcher=d)
        monkeypatch.setenv("VPZM_FAIL_DELIVERY", "1")
        got, results, _ = r128_call(entries, dispatcher=d)
        monkeypatch.delenv("VPZM_FAIL_DELIVERY")
        delivered = (plain_results["status"] == 0) & (plain_results["packets"] > 0)
        assert delivered.sum() == 3
        assert (results["status"][delivered] == multi.E_SYNTH).all(), results["status"]
        assert np.array_equal(results["status"][~delivered], plain_results["status"][~delivered])
        assert (results["samples"] == 0).all()
        assert same_records(got, np.array([EMPTY] * len(entries), dtype=got.dtype)) and not same_records(plain, got)
        again, again_results, _ = r128_call(entries, dispatcher=d)
        assert same_records(again, plain)
        for field in FIELDS:
            if field != "device_slot":
                assert np.array_equal(again_results[field], plain_results[field]), field
    finally:
        d.close()


def test_the_librarys_own_refusals(ctx):
    import ctypes as C
    from vorbispizza_amd import multi
    s = streams()["stereo_coupled_res2_12"]
    n = 3
    ptrs = (C.c_void_p * n)(*[s.data.ctypes.data] * n)
    sizes = (C.c_uint64 * n)(*[s.data.size] * n)
    out = np.zeros(n, dtype=multi.R128_DTYPE)
    res = np.zeros(n, dtype=multi.RESULT_DTYPE)
    d = multi.Dispatcher([0], host_threads=2)
    try:
        L = multi.lib()
        args = lambda **kw: [kw.get(k, v) for k, v in (("m", d._h), ("n", n), ("data", ptrs), ("size", sizes), ("ranges", None),  # noqa: E731
                                                       ("out", out.ctypes.data), ("results", res.ctypes.data), ("stats", None))]
        assert L.vpzm_measure_r128(*args()) == multi.OK and (res["status"] == 0).all() and (out["true_peak"] >= out["sample_peak"]).all() and (out["sample_peak"] > 0).all()
        for change in (dict(m=None), dict(out=None), dict(results=None), dict(n=-1), dict(data=None), dict(size=None)):
            assert L.vpzm_measure_r128(*args(**change)) == multi.E_ARG, change
        assert L.vpzm_measure_r128(*args(n=0, out=None, data=None, size=None)) == multi.OK  # (no entries: nothing to write)
    finally:
        d.close()


def test_the_calls_in_turn_on_one_dispatcher(ctx):
    """measure_loudness, measure_r128 and decode_ranges_batch in turn: the lane's temporary and the contexts' scratch serve all three,
    and none disturbs another's results"""
    import torch
    from vorbispizza_amd import multi
    entries = long_entries()[::2]
    stereo = [e for e in entries if e[0].channels == 2]
    want, _ = by_hand(ctx, entries)
    want_loud = the_loudness_part(want)
    first = None
    d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
    try:
        for turn in range(2):
            assert same_records(loudness_call(entries, dispatcher=d)[0], want_loud)
            assert same_records(r128_call(entries, dispatcher=d)[0], want)
            batch = batch_call(stereo, 2, most_samples(stereo), dispatcher=d)[0]
            assert same_records(r128_call(entries[:7], dispatcher=d)[0], want[:7])  # (fewer rows in the same temporary)
            if first is None:
                first = batch.clone()
            else:
                assert torch.equal(batch.view(torch.int32), first.view(torch.int32))
    finally:
        d.close()
