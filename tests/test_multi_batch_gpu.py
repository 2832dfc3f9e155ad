"""vpzm_decode_ranges_batch (include/vorbispizza_multi_batch.h, host/vorbis_multi.cpp): the windows of vpzm_decode_ranges as a zero-padded
batch in device memory.  The truth is the slice of the stream-by-stream whole decode (Stream.truth of tests/test_multi_ranges_gpu.py)
laid out as the batch's row with zeros behind it, compared as raw bits on the device -- never the call under test, and decode_ranges
only for a damaged stream, which has no other truth.  Streams and windows are those of test_multi_ranges_gpu.py, one call per channel
count: the stereo set holds stereo_floor0 (never device-decodable), so with gpu_entropy the host route's device-memory call with
type-0 floors runs beside device-decoded neighbours."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_support import FIELDS, OPTIONS, Stream, golden, streams  # noqa: E402
from multi_support import (as_bits, batch_call, check_failed_delivery, entries_of, most_samples, same_on_device,  # noqa: E402
    sentinel_out, truth_on_device, truth_rows)
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

LAYOUTS = {"planar": (True, False), "interleaved": (False, False), "planar_s16": (True, True), "interleaved_s16": (False, True)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("channels", [2, 1, 6])
@pytest.mark.parametrize("route", list(OPTIONS))
def test_every_row_is_the_slice_of_the_whole_decode_then_zeros(ctx, route, channels, layout):
    planar, s16 = LAYOUTS[layout]
    entries = entries_of(channels)
    frames = most_samples(entries)
    want = truth_on_device(ctx, channels, s16)
    decodable = sum(1 for s, a, n in entries if s.f.gpu_decode_supported and s.f.window(a, n)["n_packets"])
    live = sum(1 for s, a, n in entries if s.f.window(a, n)["n_packets"])
    for streams_per_call in (16, 3):
        got, results, stats = batch_call(entries, channels, frames, planar, s16, streams_per_call=streams_per_call, **OPTIONS[route])
        assert (results["status"] == 0).all(), results["status"]
        for k, (s, a, n) in enumerate(entries):
            w = s.f.window(a, n)
            assert results["samples"][k] == w["samples"] == (s.total - a if n < 0 else min(n, s.total - a)), (k, a, n)
            assert results["packets"][k] == w["n_packets"] and results["skipped_packets"][k] == 0 and results["channels"][k] == channels
        assert same_on_device(got, want, planar), (route, channels, layout, streams_per_call)
        # both routes ran where they should: the device-decodable streams on the device, the others (stereo: stereo_floor0) on the host
        on_device = sum(stats.device_gpu_entropy_streams[g] for g in range(16))
        assert on_device == (decodable if route != "host" else 0)
        if channels == 2:
            assert 0 < decodable < live
    assert any((a, n) == (0, 1) for _, a, n in entries) and any((a, n) == (0, s.total) for s, a, n in entries)  # (a one-sample row beside a whole stream's)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_bad_entry_costs_only_itself_and_leaves_a_zero_row(ctx, gpu_entropy):
    """a window larger than `frames`, another channel count, a window outside the stream, a container of garbage, an empty window"""
    import torch
    from vorbispizza_amd import multi
    s, mono = streams()["stereo_coupled_res2_30"], streams()["mono_floor1_res1_12"]
    garbage = Stream.__new__(Stream)
    garbage.data = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    a, n = s.bounds[3] + 7, 3000
    entries = [(s, a, n), (s, -1, n), (s, a, n - 1), (s, s.total + 1, n), (s, a, n + 1), (garbage, a, n), (mono, 5, 100), (s, s.total, 10), (s, a + 1, n)]
    frames = n  # (entry 4's window is one sample more than a row holds)
    for planar, s16 in ((True, False), (False, True)):
        got, results, _ = batch_call(entries, 2, frames, planar, s16, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
        assert list(results["status"]) == [0, multi.E_RANGE, 0, multi.E_RANGE, multi.E_CAPACITY, multi.E_OPEN, multi.E_CHANNELS, 0, 0]
        assert list(results["samples"]) == [n, 0, n - 1, 0, 0, 0, 0, 0, n]
        assert results["channels"][6] == 1 and results["packets"][7] == 0
        clean = [e if k in (0, 2, 8) else (None, 0, 0) for k, e in enumerate(entries)]
        want = torch.from_numpy(truth_rows(ctx, clean, frames, s16).view(np.int16 if s16 else np.int32)).to("cuda:0")
        assert same_on_device(got, want, planar), (planar, s16)
        assert not as_bits(got)[[1, 3, 4, 5, 6, 7]].any()


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_failed_pack_costs_its_members_e_synth_and_leaves_zero_rows(ctx, monkeypatch, gpu_entropy):
    """the entries of test_a_bad_entry_costs_only_itself_and_leaves_a_zero_row under VPZM_FAIL_DELIVERY (check_failed_delivery)"""
    import torch
    from vorbispizza_amd import multi
    s, mono = streams()["stereo_coupled_res2_30"], streams()["mono_floor1_res1_12"]
    garbage = Stream.__new__(Stream)
    garbage.data = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    a, n = s.bounds[3] + 7, 3000
    entries = [(s, a, n), (s, -1, n), (s, a, n - 1), (s, s.total + 1, n), (s, a, n + 1), (garbage, a, n), (mono, 5, 100), (s, s.total, 10), (s, a + 1, n)]
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        for planar, s16 in ((True, False), (False, True)):
            dtype, shape = (torch.int16 if s16 else torch.float32), (lambda rows: (rows, 2, n) if planar else (rows, n, 2))
            check_failed_delivery(monkeypatch, d, lambda: batch_call(entries, 2, n, planar, s16, dispatcher=d,
                                                                     out=sentinel_out(d, len(entries), shape, dtype, 77))[:2], 0, step="vpz_pcm_pack")
    finally:
        d.close()


def test_the_groups_share_one_tensor_and_change_no_byte(ctx):
    import torch
    from vorbispizza_amd import multi
    entries = entries_of(2)[:61]
    frames = most_samples(entries)
    want = truth_on_device(ctx, 2, True)[:61, :, :frames]
    assert most_samples(entries_of(2)) == frames  # (the whole-stream windows come first: the truth's rows need no cut)
    one = None
    for ids in ((0,), (0, 0), (0, 0, 0, 0)):
        for gpu_entropy in (False, True):
            d = multi.Dispatcher(list(ids), host_threads=2 * len(ids), streams_per_call=5, gpu_entropy=gpu_entropy)
            cuts = [d.batch_partition(len(entries), g) for g in range(len(ids))]
            assert cuts == [(len(entries) * g // len(ids), len(entries) * (g + 1) // len(ids)) for g in range(len(ids))]
            # the caller's tensor, cut by batch_partition, with guard rows on either side
            held = torch.full((len(entries) + 2, 2, frames), 0x5A5A, dtype=torch.int16, device="cuda:0")
            out = [held[1 + lo: 1 + hi] for lo, hi in cuts]
            got, results, _ = batch_call(entries, 2, frames, True, True, device_ids=ids, dispatcher=d, out=out)
            d.close()
            assert (results["status"] == 0).all()
            assert all(cuts[results["device_slot"][k]][0] <= k < cuts[results["device_slot"][k]][1] for k in range(len(entries)))
            assert torch.equal(held[1:-1], want) and (held[0] == 0x5A5A).all() and (held[-1] == 0x5A5A).all(), (ids, gpu_entropy)
            one = held[1:-1].clone() if one is None else one
            assert torch.equal(held[1:-1], one)


def test_fewer_entries_than_groups(ctx):
    import torch
    from vorbispizza_amd import multi
    s = streams()["stereo_coupled_res2_12"]
    entries = [(s, 3, 700), (s, s.bounds[2], 900)]
    d = multi.Dispatcher([0, 0, 0, 0], host_threads=4, gpu_entropy=True)
    assert [d.batch_partition(2, g) for g in range(4)] == [(0, 0), (0, 1), (1, 1), (1, 2)] and d.batch_partition(0, 3) == (0, 0)
    got, results, _ = batch_call(entries, 2, 1000, False, False, device_ids=(0, 0, 0, 0), dispatcher=d)
    assert list(results["status"]) == [0, 0] and list(results["device_slot"]) == [1, 3] and list(results["samples"]) == [700, 900]
    want = torch.from_numpy(truth_rows(ctx, entries, 1000, False).view(np.int32)).to("cuda:0")
    assert same_on_device(got, want, False)
    none = d.decode_ranges_batch([], [], 2, 1000)
    assert len(none[2]) == 0 and none[1].shape[0] == 0
    d.close()


@pytest.mark.parametrize("switch,value", [("VPZM_FAIL_GPU_ENTROPY", "1"), ("VPZM_FAIL_BATCH_CALLS", "1"), ("VPZM_MAX_CALL_VALUES", "40000")])
def test_the_switches_change_no_byte(ctx, monkeypatch, switch, value):
    entries = entries_of(2)
    frames = most_samples(entries)
    for planar, s16 in ((True, False), (False, True)):
        monkeypatch.delenv(switch, raising=False)
        plain = batch_call(entries, 2, frames, planar, s16, gpu_entropy=True)
        monkeypatch.setenv(switch, value)
        other = batch_call(entries, 2, frames, planar, s16, gpu_entropy=True)
        want = truth_on_device(ctx, 2, s16)
        assert same_on_device(plain[0], want, planar) and same_on_device(other[0], want, planar), (switch, planar, s16)
        for field in FIELDS:
            assert np.array_equal(plain[1][field], other[1][field]), (switch, field)
        devs = [sum(r[2].device_gpu_entropy_streams[g] for g in range(16)) for r in (plain, other)]
        assert devs[0] > 0 and (devs[1] == 0) == (switch == "VPZM_FAIL_GPU_ENTROPY")


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_damaged_stream_delivers_what_decode_ranges_delivers_then_zeros(ctx, gpu_entropy):
    """a damaged stream has no truth but the host-destination call: the row is its samples, then zeros"""
    import torch
    from synth_support import damage_audio
    from multi_support import call
    damaged = [Stream(damage_audio(raw, seed, hits), False) for raw, (seed, hits) in
               ((golden("3test.ogg"), (1, 8)), (golden("2test.ogg"), (2, 16)), (streams()["stereo_coupled_res2_30"].raw, (3, 6)),
                (streams()["six_channels_51_12"].raw, (4, 4)))]
    assert {s.channels for s in damaged} >= {2, 6}
    for channels in sorted({s.channels for s in damaged}):  # (a batch has one channel count: a call per count)
        entries = []
        for s in damaged:
            b = s.bounds
            if s.channels == channels:
                entries += [(s, 0, -1), (s, b[len(b) // 2] + 3, 4000), (s, b[2] - 1, b[5] - b[2] + 2), (s, max(0, s.total - 3000), -1), (s, b[1], 1)]
        frames = most_samples(entries)
        pcm, offs, ref_results, _ = call(entries, dense=True, gpu_entropy=False, streams_per_call=4)
        assert (ref_results["status"] == 0).all()  # (they all opened: the damage is in the audio pages)
        want = np.zeros((len(entries), frames, channels), dtype=np.float32)
        for k in range(len(entries)):
            m = int(ref_results["samples"][k])
            want[k, :m] = pcm[offs[k]: offs[k] + m * channels].reshape(m, channels)
        got, results, _ = batch_call(entries, channels, frames, False, False, gpu_entropy=gpu_entropy, streams_per_call=4)
        for field in FIELDS:
            assert np.array_equal(results[field], ref_results[field]), field
        assert torch.equal(as_bits(got), torch.from_numpy(want.view(np.int32)).to("cuda:0")), channels


def test_library_ranges_and_batch_on_one_dispatcher(ctx):
    """the three calls on one dispatcher, in that order and reversed, give what each gives alone"""
    from multi_support import SENTINEL, call, expected, same_bits
    from vorbispizza_amd import multi
    raws = [golden("3test.ogg"), golden("1test.ogg"), streams()["stereo_floor0_12"].raw, streams()["stereo_coupled_res2_30"].raw] * 2
    ss = {r: Stream(r, False) for r in set(raws)}
    caps = np.array([ss[r].total + 16 for r in raws], dtype=np.int64)
    sizes = np.array([c * ss[r].channels for c, r in zip(caps, raws)], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    datas = [ss[r].data for r in raws]
    entries = entries_of(2)[::3]
    frames = most_samples(entries)
    want_batch = truth_on_device(ctx, 2, False)[::3, :, :frames]
    want_ranges = expected(ctx, entries, False, False)

    def library(d):
        pcm = np.full(int(sizes.sum()), SENTINEL, dtype=np.float32)
        results, _ = d.decode_library(datas, pcm, offs, caps)
        for k, r in enumerate(raws):
            ref = ss[r].truth(ctx, False)
            assert results["status"][k] == 0 and results["samples"][k] == ref.shape[0]
            assert same_bits(pcm[offs[k]: offs[k] + ref.size], ref.reshape(-1))

    def ranges(d):
        assert same_bits(call(entries, dense=False, dispatcher=d)[0], want_ranges)

    def batch(d):
        got, results, _ = batch_call(entries, 2, frames, True, False, dispatcher=d)
        assert (results["status"] == 0).all() and same_on_device(got, want_batch, True)

    for order in ((library, ranges, batch), (batch, ranges, library)):
        d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
        try:
            for step in order + order:
                step(d)
        finally:
            d.close()


def test_python_argument_errors_are_raised_before_the_call(ctx, monkeypatch):
    import torch
    from vorbispizza_amd import multi
    s = streams()["stereo_coupled_res2_12"]
    entries = [(s, 0, 100), (s, 50, 100), (s, 70, 10)]
    d = multi.Dispatcher([0, 0], host_threads=2)

    def never(*a):
        raise AssertionError("the library was called")

    monkeypatch.setattr(multi.lib(), "vpzm_decode_ranges_batch", never)
    good = lambda: [torch.zeros((1, 2, 128), device="cuda:0"), torch.zeros((2, 2, 128), device="cuda:0")]  # noqa: E731
    bad = {"a CPU tensor": [good()[0], torch.zeros((2, 2, 128))],
           "a wrong shape": [good()[0], torch.zeros((2, 128, 2), device="cuda:0")],
           "rows of another group": [good()[1], good()[0]],
           "a wrong dtype": [good()[0], torch.zeros((2, 2, 128), dtype=torch.int16, device="cuda:0")],
           "not contiguous": [good()[0], torch.zeros((2, 128, 2), device="cuda:0").permute(0, 2, 1)],
           "one tensor too few": [good()[0]],
           "no tensor at all": [good()[0], np.zeros((2, 2, 128), dtype=np.float32)]}
    for what, out in bad.items():
        with pytest.raises(ValueError):
            d.decode_ranges_batch([e[0].data for e in entries], [(a, n) for _, a, n in entries], 2, 128, out=out)
            pytest.fail(what)
    with pytest.raises(AssertionError, match="the library was called"):  # (... and a good list gets through to it)
        d.decode_ranges_batch([e[0].data for e in entries], [(a, n) for _, a, n in entries], 2, 128, out=good())
    monkeypatch.undo()
    # the C call's own refusals
    parts, _, results, _ = d.decode_ranges_batch([e[0].data for e in entries], [(a, n) for _, a, n in entries], 2, 128, out=good())
    assert list(results["samples"]) == [100, 100, 10]
    import ctypes as C
    L, n = multi.lib(), len(entries)
    ptrs = (C.c_void_p * n)(*[e[0].data.ctypes.data for e in entries])
    sizes = (C.c_uint64 * n)(*[e[0].data.size for e in entries])
    rng = np.array([(a, c) for _, a, c in entries], dtype=np.int64)
    res = np.zeros(n, dtype=multi.RESULT_DTYPE)
    dst = (C.c_void_p * 2)(parts[0].data_ptr(), parts[1].data_ptr())
    holed = (C.c_void_p * 2)(parts[0].data_ptr(), None)
    args = lambda **kw: [kw.get(k, v) for k, v in (("m", d._h), ("n", n), ("data", ptrs), ("size", sizes), ("ranges", rng.ctypes.data), ("channels", 2),  # noqa: E731
                                                   ("frames", 128), ("layout", 1), ("dst", dst), ("results", res.ctypes.data), ("stats", None))]
    assert L.vpzm_decode_ranges_batch(*args()) == multi.OK
    for change in (dict(dst=None), dict(dst=holed), dict(channels=0), dict(frames=0), dict(layout=4), dict(layout=-1), dict(m=None), dict(results=None),
                   dict(ranges=None), dict(n=-1)):
        assert L.vpzm_decode_ranges_batch(*args(**change)) == multi.E_ARG, change
    lo, hi = C.c_int32(), C.c_int32()
    for group in (-1, 2):
        assert L.vpzm_batch_partition(d._h, 3, group, C.byref(lo), C.byref(hi)) == multi.E_ARG
    assert L.vpzm_batch_partition(d._h, -1, 0, C.byref(lo), C.byref(hi)) == multi.E_ARG
    assert L.vpzm_batch_partition(d._h, 3, 0, None, C.byref(hi)) == multi.E_ARG
    d.close()
