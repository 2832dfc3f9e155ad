"""vpzm_decode_ranges_resampled (include/vorbispizza_multi_resample.h, host/vorbis_multi.cpp): the padded device batch at one sample rate.

Streams and windows are those of tests/test_multi_ranges_gpu.py (stereo at 44 100 Hz, six channels at 48 000, mono at 8 000 and 44 100,
floor-0 stereo at 16 000, which a 16 000 Hz batch copies), the writer's five- and ten-channel streams (more channels than the kernel stages
side by side) and copies of the stereo stream re-rated so that the ratio lies at a limit: (1, 32), (128, 125), (1024, 1023).  The truth of a row is tests/test_resample_cpu.py's float64 restatement applied to
the slice of the stream-by-stream whole decode, held to the derived bound (T + C + 3) * 2^-24 * B[j]; it is never the call under test.
What is compared between two calls of the dispatcher -- layouts, routes, partitions, cuts, failure paths -- is compared as raw bits, and
the int16 layouts are the project's conversion of the float32 output of the same call's float32 twin, bit for bit."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_support import (all_entries, as_bits, batch_call, entries_of, FIELDS, golden, most_outputs, OPTIONS, out_len,  # noqa: E402
    RATE, ratio, rerated, resampled_call, Stream, streams)
from resample_truth import bound, launch_plan, ratio_of, ratio_ok, resample_truth, to_s16  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu


_many = {}


def many_channels(name):
    """the writer's five_channels / ten_channels stream (48 000 Hz) at ten packets"""
    import synthetic_streams as ss
    if name not in _many:
        st, rng = getattr(ss, name)()
        _many[name] = Stream(bytes(st.build(rng, 10)[0]), True)
        assert _many[name].f.sample_rate == 48000 and _many[name].channels == {"five_channels": 5, "ten_channels": 10}[name]
    return _many[name]


_rows = {}


def truth_row(ctx, s, a, m, rate, mono):
    """(y [J, Co], B [J, Co]) of m samples from a of s's whole float32 decode, computed once"""
    key = (id(s), a, m, rate, mono)
    if key not in _rows:
        up, down = ratio(s, rate)
        _rows[key] = resample_truth(s.truth(ctx, False)[a: a + m], up, down, mono)
    return _rows[key]


def check_against_truth(ctx, got_planar, results, entries, rate, mono, delivered=None):
    """a float32 planar batch [n, Co, frames] (numpy) against the restatement, row by row; -> the largest error / bound"""
    worst = 0.0
    for k, (s, a, n) in enumerate(entries):
        m = s.f.window(a, n)["samples"] if delivered is None else int(delivered[k])
        up, down = ratio(s, rate)
        J = out_len(m, up, down)
        assert results["status"][k] == 0 and results["samples"][k] == J, (k, a, n, results["status"][k], results["samples"][k], J)
        assert results["sample_rate"][k] == s.f.sample_rate and results["channels"][k] == s.channels
        assert not got_planar[k, :, J:].view(np.uint32).any(), ("not zero bits behind the samples", k)
        if J == 0:
            continue
        y, B = truth_row(ctx, s, a, m, rate, mono)
        err = np.abs(got_planar[k, :, :J].T.astype(np.float64) - y)
        tol = bound(B, up, down, s.channels if mono else 1)
        assert (err <= tol).all(), (k, a, n, up, down, float(err.max()), int(np.argmax(err - tol)))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    return worst


def four_layouts(entries, rate, channels, frames, mono=False, **opt):
    """the four layouts of one call's inputs; the float32 ones agree bit for bit, the int16 ones are their conversion.  -> (planar float32
    numpy, its results)"""
    import torch
    planar, results, _ = resampled_call(entries, rate, channels, frames, True, False, mono, **opt)
    inter, r2, _ = resampled_call(entries, rate, channels, frames, False, False, mono, **opt)
    assert torch.equal(as_bits(inter), as_bits(planar).permute(0, 2, 1))
    want16 = torch.from_numpy(to_s16(planar.cpu().numpy())).to("cuda:0")
    p16, r3, _ = resampled_call(entries, rate, channels, frames, True, True, mono, **opt)
    i16, r4, _ = resampled_call(entries, rate, channels, frames, False, True, mono, **opt)
    assert torch.equal(p16, want16), "planar int16 is not the conversion of the float32 output"
    assert torch.equal(i16, want16.permute(0, 2, 1)), "interleaved int16 is not the conversion of the float32 output"
    for other in (r2, r3, r4):
        for field in FIELDS:
            assert np.array_equal(results[field], other[field]), field
    return planar.cpu().numpy(), results


@pytest.mark.parametrize("channels", [2, 1, 6])
@pytest.mark.parametrize("route", list(OPTIONS))
def test_every_row_is_the_resampled_slice_of_the_whole_decode(ctx, route, channels):
    entries = entries_of(channels)
    frames = most_outputs(entries, RATE) + 3
    assert len({ratio(s, RATE) for s, _, _ in entries}) >= (2 if channels < 6 else 1)
    got, results = four_layouts(entries, RATE, channels, frames, **OPTIONS[route])
    worst = check_against_truth(ctx, got, results, entries, RATE, False)
    print("%s, %d channels: largest error / bound %.3f" % (route, channels, worst))
    if channels == 2:  # stereo_floor0 is at 16 000 Hz already: its rows are the decode's bits
        for k, (s, a, n) in enumerate(entries):
            if s.f.sample_rate == RATE:
                m = s.f.window(a, n)["samples"]
                assert got[k, :, :m].T.tobytes() == s.truth(ctx, False)[a: a + m].tobytes()


def test_one_mono_call_over_all_streams_with_several_ratios_in_a_sub_batch(ctx, monkeypatch, capfd):
    entries = all_entries()
    for rate in (48000, 22050):  # the stereo setup at two more rates, beside its 44 100 Hz windows
        s = rerated(rate)
        for i, (a, n) in enumerate(s.windows()[:12]):  # (spread out, so that they share sub-batches with the 44 100 Hz windows)
            entries.insert(5 + 17 * i + (rate == 48000), (s, a, n))
    frames = most_outputs(entries, RATE)
    assert {s.channels for s, _, _ in entries} == {1, 2, 6} and len({ratio(s, RATE) for s, _, _ in entries}) >= 5
    monkeypatch.setenv("VPZM_PROFILE", "1")
    for route in ("host", "mixed"):
        capfd.readouterr()
        got, results, _ = resampled_call(entries, RATE, 1, frames, True, False, True, streams_per_call=64, **OPTIONS[route])
        launches = [int(x) for x in re.findall(r"resampled in (\d+) launches", capfd.readouterr().err)]
        assert launches and max(launches) >= 3 and min(launches) >= 1, launches  # (44 100, 48 000 and 22 050 Hz members of one setup)
        worst = check_against_truth(ctx, got.cpu().numpy(), results, entries, RATE, True)
        print("%s, mono over all streams: largest error / bound %.3f, launches per sub-batch %r" % (route, worst, launches))


@pytest.mark.parametrize("channels,rate", [(2, 44100), (6, 48000)])
def test_the_streams_own_rate_is_the_batch_call_bit_for_bit(ctx, channels, rate):
    import torch
    entries = [e for e in entries_of(channels) if e[0].f.sample_rate == rate]
    assert len(entries) > 40
    frames = most_outputs(entries, rate)
    for planar, s16 in ((True, False), (False, False), (True, True), (False, True)):
        for route in ("host", "device"):
            want, want_results, _ = batch_call(entries, channels, frames, planar, s16, **OPTIONS[route])
            got, results, _ = resampled_call(entries, rate, channels, frames, planar, s16, **OPTIONS[route])
            assert torch.equal(as_bits(got), as_bits(want)), (planar, s16, route)
            for field in FIELDS:
                assert np.array_equal(results[field], want_results[field]), field


def test_the_partition_the_cut_and_the_failure_paths_change_no_byte(ctx, monkeypatch):
    import torch
    entries = entries_of(2)
    frames = most_outputs(entries, RATE)
    one, one_results, _ = resampled_call(entries, RATE, 2, frames, False, True, gpu_entropy=False)
    check_against_truth(ctx, resampled_call(entries, RATE, 2, frames, True, False, gpu_entropy=False)[0].cpu().numpy(), one_results, entries, RATE, False)
    for groups in (1, 2, 4):
        for streams_per_call in (3, 64):
            for gpu_entropy in (False, True):
                got, results, _ = resampled_call(entries, RATE, 2, frames, False, True, device_ids=[0] * groups, streams_per_call=streams_per_call,
                                                 gpu_entropy=gpu_entropy, host_threads=2 * groups)
                assert torch.equal(got, one), (groups, streams_per_call, gpu_entropy)
                for field in FIELDS:
                    if field != "device_slot":
                        assert np.array_equal(results[field], one_results[field]), field
    for switch in ("VPZM_FAIL_BATCH_CALLS", "VPZM_FAIL_GPU_ENTROPY"):
        monkeypatch.setenv(switch, "1")
        got, results, stats = resampled_call(entries, RATE, 2, frames, False, True, gpu_entropy=True)
        monkeypatch.delenv(switch)
        assert torch.equal(got, one), switch
        assert (sum(stats.device_gpu_entropy_streams[g] for g in range(16)) == 0) == (switch == "VPZM_FAIL_GPU_ENTROPY")
        for field in FIELDS:
            assert np.array_equal(results[field], one_results[field]), (switch, field)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_bad_entry_costs_only_itself_and_leaves_a_zero_row(ctx, gpu_entropy):
    from vorbispizza_amd import multi
    s, mono, odd = streams()["stereo_coupled_res2_30"], streams()["mono_floor1_res1_12"], rerated(44101)
    garbage = Stream.__new__(Stream)
    garbage.data = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    up, down = ratio(s, RATE)
    assert math.gcd(44101, RATE) == 1  # (up would be 16 000: refused)
    a, n = s.bounds[3] + 7, 7 * down  # (a whole number of periods: one source sample more is one output sample more)
    J = out_len(n, up, down)
    assert out_len(n - 2, up, down) == J and out_len(n + 1, up, down) == J + 1
    # entry 4: one output sample more than a row holds (frames = its J - 1); entry 2 fills the row to its last element
    entries = [(s, a, n), (s, -1, n), (s, a, n - 2), (s, s.total + 1, n), (s, a, n + 1), (garbage, a, n), (mono, 5, 100), (s, s.total, 10), (odd, 3, 500),
               (s, a + 1, n)]
    for planar, s16 in ((True, False), (False, True)):
        got, results, _ = resampled_call(entries, RATE, 2, J, planar, s16, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
        assert list(results["status"]) == [0, multi.E_RANGE, 0, multi.E_RANGE, multi.E_CAPACITY, multi.E_OPEN, multi.E_CHANNELS, 0, multi.E_RATE, 0]
        assert list(results["samples"]) == [J, 0, J, 0, 0, 0, 0, 0, 0, J]
        assert results["channels"][6] == 1 and results["sample_rate"][8] == 44101
        img = got.cpu().numpy() if planar else got.cpu().numpy().transpose(0, 2, 1)
        assert not img[[1, 3, 4, 5, 6, 7, 8]].any()
        for k in (0, 2, 9):
            st, ak, nk = entries[k]
            y, B = truth_row(ctx, st, ak, nk, RATE, False)
            if s16:  # (a sanity check within one step: four_layouts holds the int16 layouts to the float32 output bit for bit)
                assert (np.abs(img[k].T.astype(np.float64) - np.clip(np.trunc(y * 32768.0), -32768, 32767)) <= 1).all(), k
            else:
                assert (np.abs(img[k].T - y) <= bound(B, up, down)).all(), k
    # a mono batch takes every channel count; a downmix into two channels is refused outright
    got, results, _ = resampled_call(entries, RATE, 1, J, True, False, True, gpu_entropy=gpu_entropy)
    assert list(results["status"]) == [0, multi.E_RANGE, 0, multi.E_RANGE, multi.E_CAPACITY, multi.E_OPEN, 0, 0, multi.E_RATE, 0]
    assert results["samples"][6] == 200  # (8 000 Hz -> 16 000)
    with pytest.raises(ValueError):
        resampled_call(entries, RATE, 2, J, True, False, True)
    import ctypes as C
    d = multi.Dispatcher([0], host_threads=2)
    n_e = len(entries)
    ptrs = (C.c_void_p * n_e)(*[e[0].data.ctypes.data for e in entries])
    sizes = (C.c_uint64 * n_e)(*[e[0].data.size for e in entries])
    rng = np.array([(x, c) for _, x, c in entries], dtype=np.int64)
    res = np.zeros(n_e, dtype=multi.RESULT_DTYPE)
    dst = (C.c_void_p * 1)(got.data_ptr())
    args = lambda **kw: [kw.get(k, v) for k, v in (("m", d._h), ("n", n_e), ("data", ptrs), ("size", sizes), ("ranges", rng.ctypes.data), ("rate", RATE),  # noqa: E731
                                                   ("channels", 1), ("downmix", 1), ("frames", J), ("layout", 1), ("dst", dst), ("results", res.ctypes.data),
                                                   ("stats", None))]
    L = multi.lib()
    assert L.vpzm_decode_ranges_resampled(*args()) == multi.OK
    for change in (dict(rate=0), dict(rate=-1), dict(downmix=2), dict(downmix=-1), dict(channels=2), dict(channels=0), dict(frames=0), dict(layout=4),
                   dict(dst=None), dict(m=None), dict(results=None), dict(ranges=None), dict(n=-1)):
        assert L.vpzm_decode_ranges_resampled(*args(**change)) == multi.E_ARG, change
    d.close()


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_failed_resample_launches_cost_their_members_e_synth_and_leave_zero_rows(ctx, monkeypatch, gpu_entropy):
    """the entries of test_a_bad_entry_costs_only_itself_and_leaves_a_zero_row under VPZM_FAIL_DELIVERY (check_failed_delivery of
    test_multi_batch_gpu.py)"""
    import torch
    from multi_support import check_failed_delivery, sentinel_out
    from vorbispizza_amd import multi
    s, mono, odd = streams()["stereo_coupled_res2_30"], streams()["mono_floor1_res1_12"], rerated(44101)
    garbage = Stream.__new__(Stream)
    garbage.data = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    up, down = ratio(s, RATE)
    a, n = s.bounds[3] + 7, 7 * down
    J = out_len(n, up, down)
    entries = [(s, a, n), (s, -1, n), (s, a, n - 2), (s, s.total + 1, n), (s, a, n + 1), (garbage, a, n), (mono, 5, 100), (s, s.total, 10), (odd, 3, 500),
               (s, a + 1, n)]
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        for planar, s16 in ((True, False), (False, True)):
            dtype, shape = (torch.int16 if s16 else torch.float32), (lambda rows: (rows, 2, J) if planar else (rows, J, 2))
            check_failed_delivery(monkeypatch, d, lambda: resampled_call(entries, RATE, 2, J, planar, s16, dispatcher=d,
                                                                         out=sentinel_out(d, len(entries), shape, dtype, 77))[:2], 0,
                                  step="vpz_pcm_resample")
    finally:
        d.close()


def test_damaged_audio_is_the_same_on_both_routes(ctx):
    """a damaged stream has no truth but the host-destination call: the row is the restatement of the samples decode_ranges delivers"""
    import torch
    from synth_support import damage_audio
    from multi_support import call
    damaged = [Stream(damage_audio(raw, seed, hits), False) for raw, (seed, hits) in
               ((golden("3test.ogg"), (1, 8)), (golden("2test.ogg"), (2, 16)), (streams()["stereo_coupled_res2_30"].raw, (3, 6)))]
    entries = []
    for s in damaged:
        b = s.bounds
        if s.channels == 2:
            entries += [(s, 0, -1), (s, b[len(b) // 2] + 3, 4000), (s, b[2] - 1, b[5] - b[2] + 2), (s, max(0, s.total - 3000), -1), (s, b[1], 1)]
    assert len(entries) >= 10
    frames = most_outputs(entries, RATE)
    pcm, offs, ref, _ = call(entries, dense=True, gpu_entropy=False, streams_per_call=4)
    assert (ref["status"] == 0).all()  # (they all opened: the damage is in the audio pages)
    host, results, _ = resampled_call(entries, RATE, 2, frames, True, False, gpu_entropy=False, streams_per_call=4)
    device, results_d, _ = resampled_call(entries, RATE, 2, frames, True, False, gpu_entropy=True, streams_per_call=4)
    assert torch.equal(as_bits(host), as_bits(device))
    img = host.cpu().numpy()
    for k, (s, a, n) in enumerate(entries):
        m = int(ref["samples"][k])
        up, down = ratio(s, RATE)
        J = out_len(m, up, down)
        for field in FIELDS:
            want = J if field == "samples" else ref[field][k]
            assert results[field][k] == want == results_d[field][k], (k, field)
        y, B = resample_truth(pcm[offs[k]: offs[k] + m * 2].reshape(m, 2), up, down)
        assert (np.abs(img[k, :, :J].T - y) <= bound(B, up, down)).all() and not img[k, :, J:].any(), k


def test_the_four_calls_in_turn_on_one_dispatcher(ctx):
    import torch
    from multi_support import most_samples, same_on_device, truth_on_device
    from multi_support import call, expected, same_bits
    from vorbispizza_amd import multi
    entries = entries_of(2)[::3]
    frames = most_samples(entries)
    want_batch = truth_on_device(ctx, 2, False)[::3, :, :frames]
    want_ranges = expected(ctx, entries, False, False)
    s = streams()["stereo_coupled_res2_12"]
    caps = np.array([s.total + 16], dtype=np.int64)
    alone = resampled_call(entries, RATE, 2, frames, True, True, gpu_entropy=True, streams_per_call=4, device_ids=(0, 0))[0]

    def library(d):
        pcm = np.full((s.total + 16) * 2, 7, dtype=np.float32)
        results, _ = d.decode_library([s.data], pcm, np.zeros(1, dtype=np.int64), caps)
        assert results["status"][0] == 0 and same_bits(pcm[: s.total * 2], s.truth(ctx, False).reshape(-1))

    def ranges(d):
        assert same_bits(call(entries, dense=False, dispatcher=d)[0], want_ranges)

    def batch(d):
        got, results, _ = batch_call(entries, 2, frames, True, False, dispatcher=d)
        assert (results["status"] == 0).all() and same_on_device(got, want_batch, True)

    def resampled(d):
        got, results, _ = resampled_call(entries, RATE, 2, frames, True, True, dispatcher=d)
        assert (results["status"] == 0).all() and torch.equal(got, alone)

    for order in ((library, ranges, batch, resampled), (resampled, batch, ranges, library)):
        d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
        try:
            for step in order + order:
                step(d)
        finally:
            d.close()


@pytest.mark.parametrize("mono", [False, True], ids=["unmixed", "mono"])
@pytest.mark.parametrize("route", ["host", "device"])
def test_five_and_ten_channels_take_several_passes_of_the_kernel(ctx, route, mono):
    """48 000 -> 16 000 Hz is (1, 3): five channels in one pass, ten in two (8 + 2) -- more channels than the kernel stages side by side"""
    five, ten = many_channels("five_channels"), many_channels("ten_channels")
    assert launch_plan(1, 3, 5, False)["passes"] == [5] and launch_plan(1, 3, 10, False)["passes"] == [8, 2]
    if mono:  # one call over both streams, their windows in turn
        sets = [(1, [e for pair in zip(*[[(s, a, n) for a, n in s.windows()] for s in (five, ten)]) for e in pair])]
    else:
        sets = [(s.channels, [(s, a, n) for a, n in s.windows()]) for s in (five, ten)]
    for channels, entries in sets:
        assert len(entries) > 20
        frames = most_outputs(entries, RATE) + 3
        got, results = four_layouts(entries, RATE, channels, frames, mono, **OPTIONS[route])
        worst = check_against_truth(ctx, got, results, entries, RATE, mono)
        print("%s, %s channels%s: largest error / bound %.3f" % (route, "5 and 10" if mono else channels, " mixed down" if mono else "", worst))


# (source rate, target rate) -> the ratio: the steepest one, a neighbour with many phases, and up = 1024 exactly (no source rate gives it
# against 16 000 Hz)
LIMIT_RATES = {(512000, RATE): (1, 32), (15625, RATE): (128, 125), (1023, 1024): (1024, 1023)}


@pytest.mark.parametrize("fs,ft", list(LIMIT_RATES))
@pytest.mark.parametrize("route", ["host", "device"])
def test_rates_at_the_limits_of_the_ratio_are_accepted(ctx, route, fs, ft):
    s = rerated(fs, 10)
    assert ratio(s, ft) == LIMIT_RATES[(fs, ft)] and ratio_ok(*ratio(s, ft))
    entries = [(s, a, n) for a, n in s.windows()]
    frames = most_outputs(entries, ft) + 3
    got, results = four_layouts(entries, ft, 2, frames, **OPTIONS[route])
    worst = check_against_truth(ctx, got, results, entries, ft, False)
    mono, results = resampled_call(entries, ft, 1, frames, True, False, True, **OPTIONS[route])[:2]
    worst_mono = check_against_truth(ctx, mono.cpu().numpy(), results, entries, ft, True)
    print("%s, %d -> %d Hz, ratio %r: largest error / bound %.3f, mixed down %.3f" % (route, fs, ft, ratio(s, ft), worst, worst_mono))


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_the_nearest_ratios_beyond_the_limits_are_refused_with_a_zero_row(ctx, gpu_entropy):
    """down = 32 * up + 1 and up = 1025, each beside an accepted neighbour in the same call"""
    from vorbispizza_amd import multi
    for ft, fs_good, fs_bad, refused in ((RATE, 512000, 528000, (1, 33)), (1025, 15625, 1023, (1025, 1023))):
        good, bad = rerated(fs_good, 10), rerated(fs_bad, 10)
        assert ratio_ok(*ratio(good, ft)) and ratio(bad, ft) == refused and not ratio_ok(*refused)
        entries = [e for a, b in zip(good.windows()[:8], bad.windows()[:8]) for e in ((good, *a), (bad, *b))]
        ok = np.arange(0, len(entries), 2)
        frames = most_outputs(entries[::2], ft) + 1
        for planar, s16 in ((True, False), (False, True)):
            got, results, _ = resampled_call(entries, ft, 2, frames, planar, s16, gpu_entropy=gpu_entropy, streams_per_call=4)
            assert (results["status"][ok] == 0).all() and (results["status"][ok + 1] == multi.E_RATE).all(), results["status"]
            assert (results["samples"][ok + 1] == 0).all() and (results["sample_rate"][ok + 1] == fs_bad).all()
            img = got.cpu().numpy() if planar else got.cpu().numpy().transpose(0, 2, 1)
            assert not img[ok + 1].any()
            if not s16:
                check_against_truth(ctx, img[ok], results[ok], entries[::2], ft, False)
            else:
                assert img[ok].any()
