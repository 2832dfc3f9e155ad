"""vpzm_measure_loudness (include/vorbispizza_multi_loudness.h, host/vorbis_multi.cpp): windows of streams measured for programme
loudness on the device.

Streams and windows are those of tests/test_multi_fbank_gpu.py (the small synthetic streams of tests/synthetic_streams.py: 1, 2 and 6
channels, several rates, the stereo setup at more rates), and the stereo setup at 8 000 Hz with thirty packets, so that some windows have
the four steps a gated value needs.  The call is a batch call whose delivery measures, so what is checked of it is EQUALITY, bit for bit:
every record is capi.pcm_loudness followed by capi.loudness_gate of the interleaved float32 row decode_ranges_batch delivers for the same
range -- on every route, partition, cut and failure path.  The kernel alone is held to its truth in tests/test_pcm_loudness_gpu.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loudness_truth as lt  # noqa: E402
from multi_support import (batch_call, FIELDS, loudness_entries, loudness_refused_entries as refused_entries, measure_call,  # noqa: E402
    mixed_entries, most_samples, OPTIONS, rerated, Stream, streams)
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

EMPTY = (-np.inf, 0.0, 0, 0)


def by_hand(ctx, entries, **opt):
    """capi.pcm_loudness and capi.loudness_gate over the interleaved float32 batch of the same ranges, one batch call per channel count
    and one launch per rate, results["samples"] as every row's L: what the call must equal.  -> (records, results)"""
    from vorbispizza_amd import capi, multi
    rec = np.zeros(len(entries), dtype=multi.LOUDNESS_DTYPE)
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
            ctx.synchronize()
            sums, peak = sums.cpu().numpy(), peak.cpu().numpy()
            for _, L, i in rows:
                lufs, kept = capi.loudness_gate(sums[i, : L // S], S)
                rec[at[i]] = (lufs, float(peak[i]), L // S, kept)
    return rec, results


def same_records(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("route", list(OPTIONS))
def test_every_record_is_pcm_loudness_and_the_gate_of_the_batch_row(ctx, route):
    entries = loudness_entries()
    want, want_results = by_hand(ctx, entries, **OPTIONS[route])
    got, results, _ = measure_call(entries, **OPTIONS[route])
    assert same_records(got, want)
    for field in FIELDS:
        assert np.array_equal(results[field], want_results[field]), field
    assert (results["status"] == 0).all()
    assert {s.channels for s, _, _ in entries} == {1, 2, 6} and len({int(r) for r in results["sample_rate"]}) >= 5
    # samples measured, whole steps, and what follows from them
    S = np.array([lt.step_of(r) for r in results["sample_rate"]])
    assert np.array_equal(got["steps"], results["samples"] // S)
    assert np.isfinite(got["integrated"]).sum() >= 4 and (got["steps"] >= 4).sum() >= 4
    assert (np.isneginf(got["integrated"]) == (got["blocks_kept"] == 0)).all() and (got["integrated"][got["steps"] < 4] == -np.inf).all()
    assert (got["peak"][results["samples"] == 0] == 0).all() and (got["peak"] > 0).sum() > len(entries) // 2
    assert (got["peak"] == got["peak"].astype(np.float32)).all()
    assert same_records(got[results["samples"] == 0], np.array([EMPTY] * int((results["samples"] == 0).sum()), dtype=got.dtype))


def test_the_partition_the_cut_and_the_failure_paths_change_no_bit(ctx, monkeypatch):
    entries = loudness_entries()
    one, one_results = by_hand(ctx, entries, gpu_entropy=False)
    for groups in (1, 2, 4):
        for gpu_entropy in (False, True):
            got, results, _ = measure_call(entries, device_ids=[0] * groups, streams_per_call=5, gpu_entropy=gpu_entropy, host_threads=2 * groups)
            assert same_records(got, one), (groups, gpu_entropy)
            for field in FIELDS:
                if field != "device_slot":
                    assert np.array_equal(results[field], one_results[field]), field
    for switch, value in (("VPZM_MAX_CALL_VALUES", "40000"), ("VPZM_FAIL_BATCH_CALLS", "1"), ("VPZM_FAIL_GPU_ENTROPY", "1")):
        monkeypatch.setenv(switch, value)
        got, results, stats = measure_call(entries, gpu_entropy=True, streams_per_call=64)
        monkeypatch.delenv(switch)
        assert same_records(got, one), switch
        assert (sum(stats.device_gpu_entropy_streams[g] for g in range(16)) == 0) == (switch == "VPZM_FAIL_GPU_ENTROPY")
        for field in FIELDS:
            if field != "device_slot":
                assert np.array_equal(results[field], one_results[field]), (switch, field)


def test_no_ranges_are_whole_streams(ctx):
    names = ["stereo_coupled_res2_30", "mono_floor1_res1_12", "six_channels_51_12", "stereo_floor0_12", "1test.ogg"]
    whole = [(streams()[name], 0, -1) for name in names] + [(rerated(8000, 30), 0, -1), (rerated(48000), 0, -1)]
    for gpu_entropy in (False, True):
        with_ranges, res_a, _ = measure_call(whole, gpu_entropy=gpu_entropy)
        without, res_b, _ = measure_call(whole, ranges=False, gpu_entropy=gpu_entropy)
        assert same_records(with_ranges, without)
        for field in FIELDS:
            assert np.array_equal(res_a[field], res_b[field]), field
        assert list(res_b["samples"]) == [s.total for s, _, _ in whole] and (res_b["status"] == 0).all()
        assert np.isfinite(without["integrated"][5])


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_refused_entry_costs_only_itself_and_gets_the_empty_record(ctx, gpu_entropy):
    from vorbispizza_amd import multi
    entries = refused_entries()
    n = entries[0][2]
    # (the batch call has no rate to refuse: an empty window stands in for every refused entry, its record is the empty one too)
    good = [e if k in (0, 5, 6, 7) else entries[5] for k, e in enumerate(entries)]
    want, _ = by_hand(ctx, good, gpu_entropy=gpu_entropy, streams_per_call=2)
    got, results, _ = measure_call(entries, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    assert list(results["status"]) == [0, multi.E_RANGE, multi.E_OPEN, multi.E_RATE, multi.E_RATE, 0, 0, 0]
    assert list(results["samples"]) == [n, 0, 0, 0, 0, 0, 100, n]
    assert list(results["sample_rate"][[3, 4]]) == [7999, 384001] and results["channels"][6] == 1
    assert same_records(got, want)
    empty = np.array([EMPTY] * 5, dtype=got.dtype)
    assert same_records(got[[1, 2, 3, 4, 5]], empty)
    assert list(got["steps"][[0, 6, 7]]) == [5, 0, 5] and np.isfinite(got["integrated"][[0, 7]]).all()
    assert got["integrated"][6] == -np.inf and got["peak"][6] > 0 and got["blocks_kept"][6] == 0  # 100 samples: a peak, no step


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_failed_launch_costs_its_members_e_synth_and_leaves_empty_records(ctx, monkeypatch, gpu_entropy):
    """VPZM_FAIL_DELIVERY: every entry a delivery launch serves -- OK in the plain call, with packets -- comes back VPZM_E_SYNTH with no
    samples; an entry with a status of its own keeps it, and so does the empty window; every record is the empty one; the next call
    without the switch is the plain call bit for bit"""
    from vorbispizza_amd import multi
    entries = refused_entries()
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        monkeypatch.delenv("VPZM_FAIL_DELIVERY", raising=False)
        plain, plain_results, _ = measure_call(entries, dispatcher=d)
        monkeypatch.setenv("VPZM_FAIL_DELIVERY", "1")
        got, results, _ = measure_call(entries, dispatcher=d)
        monkeypatch.delenv("VPZM_FAIL_DELIVERY")
        delivered = (plain_results["status"] == 0) & (plain_results["packets"] > 0)
        assert delivered.sum() == 3 and (plain_results["status"] != 0).sum() == 4 and ((plain_results["status"] == 0) & ~delivered).sum() == 1
        assert (results["status"][delivered] == multi.E_SYNTH).all(), results["status"]
        assert np.array_equal(results["status"][~delivered], plain_results["status"][~delivered])
        assert (results["samples"] == 0).all()
        assert same_records(got, np.array([EMPTY] * len(entries), dtype=got.dtype)) and not same_records(plain, got)
        assert "vpz_pcm_loudness" in d.last_error()
        again, again_results, _ = measure_call(entries, dispatcher=d)
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
    out = np.zeros(n, dtype=multi.LOUDNESS_DTYPE)
    res = np.zeros(n, dtype=multi.RESULT_DTYPE)
    d = multi.Dispatcher([0], host_threads=2)
    try:
        L = multi.lib()
        args = lambda **kw: [kw.get(k, v) for k, v in (("m", d._h), ("n", n), ("data", ptrs), ("size", sizes), ("ranges", None),  # noqa: E731
                                                       ("out", out.ctypes.data), ("results", res.ctypes.data), ("stats", None))]
        assert L.vpzm_measure_loudness(*args()) == multi.OK and (res["status"] == 0).all() and (out["peak"] > 0).all()
        for change in (dict(m=None), dict(out=None), dict(results=None), dict(n=-1), dict(data=None), dict(size=None)):
            assert L.vpzm_measure_loudness(*args(**change)) == multi.E_ARG, change
        assert L.vpzm_measure_loudness(*args(n=0, out=None, data=None, size=None)) == multi.OK  # (no entries: nothing to write)
    finally:
        d.close()


def test_the_calls_in_turn_on_one_dispatcher(ctx):
    """the lane's temporary and the context's scratch serve call after call, between calls of the other five kinds of the ranges family,
    whose results the loudness call does not disturb"""
    import torch
    from multi_support import FBANK_VARIANTS as VARIANTS, bits, fbank_call
    from multi_support import call as ranges_call
    from multi_support import same_bits
    from multi_support import RATE, most_outputs, resampled_call
    from vorbispizza_amd import multi
    entries = loudness_entries()[::3]
    stereo = [e for e in entries if e[0].channels == 2]
    frames = max(most_outputs(entries, RATE), 400)
    want, _ = by_hand(ctx, entries)
    short = [e for e in entries if e[0].f.window(e[1], e[2])["samples"] <= 2000]
    want_short, _ = by_hand(ctx, short)
    assert len(short) > 10 and len(stereo) > 10
    first = {}
    d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
    try:
        for turn in range(2):
            assert same_records(measure_call(entries, dispatcher=d)[0], want)
            others = {
                "ranges": ranges_call(stereo, dispatcher=d)[0],
                "batch": batch_call(stereo, 2, most_samples(stereo), dispatcher=d)[0],
                "resampled": resampled_call(entries, RATE, 1, frames, True, False, True, dispatcher=d)[0],
                "logmel": torch.cat(list(d.decode_ranges_logmel([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames, sample_rate=RATE)[0])),
                "fbank": fbank_call(entries, frames, VARIANTS[0], dispatcher=d)[0],
            }
            assert same_records(measure_call(short, dispatcher=d)[0], want_short)  # (fewer, shorter rows in the same temporary)
            for name, value in others.items():
                if turn == 0:
                    first[name] = value
                elif isinstance(value, np.ndarray):
                    assert same_bits(value, first[name]), name
                else:
                    assert torch.equal(bits(value), bits(first[name])), name
        # ... and a dispatcher that never measured gives the other calls the same results
        fresh = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
        try:
            assert same_bits(ranges_call(stereo, dispatcher=fresh)[0], first["ranges"])
            assert torch.equal(bits(fbank_call(entries, frames, VARIANTS[0], dispatcher=fresh)[0]), bits(first["fbank"]))
            assert torch.equal(bits(batch_call(stereo, 2, most_samples(stereo), dispatcher=fresh)[0]), bits(first["batch"]))
        finally:
            fresh.close()
    finally:
        d.close()
