"""vpzm_decode_ranges (include/vorbispizza_multi_ranges.h, host/vorbis_multi.cpp): a window of samples out of every stream in one
batched call.  The truth is the slice of the stream-by-stream whole decode (single_stream_pcm of tests/multi_support.py), compared as
raw bits: a window decoded from its pre-roll packet is the same samples, on both routes, for both PCM types, whatever the caller's
layout, the partition, the sub-batch cut and the failure path.

Streams: the writer's stereo_coupled_res2 at 12 and 30 packets, mono_floor1_res1 at 12 (blocks 64 / 512: the three-pass route),
six_channels_51 at 12, stereo_floor0 at 12 (never device-decodable: it rides the host route beside device-decoded neighbours) and
1test.ogg (25 packets, 538 samples of end-of-stream trim).  All of them open, their whole decode skips no packet, and the synthetic
ones' total_samples is their counted length (`streams` asserts it).  Windows per stream, from its packet boundaries b_i (the
positions where seek rolls 0): (0, 1), (0, b_1), (b_i - 1, 2), (b_i, b_i+1 - b_i), (b_i + 1, 5), three packets across a change of
packet length, (b_i, to the end), a count past the end, (total, 10), (0, total) -- every one of them is compared."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multi_support import FIELDS, OPTIONS, SENTINEL, Stream, all_entries, call, expected, golden, place, same_bits, streams  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "gaps"])
@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
@pytest.mark.parametrize("route", list(OPTIONS))
def test_every_window_is_the_slice_of_the_whole_decode(ctx, route, s16, dense):
    entries = all_entries()
    pcm, offs, results, stats = call(entries, s16=s16, dense=dense, **OPTIONS[route])
    assert (results["status"] == 0).all(), results["status"]
    for k, (s, a, n) in enumerate(entries):
        w = s.f.window(a, n)
        assert results["samples"][k] == w["samples"] == (s.total - a if n < 0 else min(n, s.total - a)), (k, a, n)
        assert results["packets"][k] == w["n_packets"] and results["skipped_packets"][k] == 0 and results["channels"][k] == s.channels
        whole = a == 0 and w["samples"] == s.total
        assert (w["n_packets"] == s.packets) == whole and w["n_packets"] <= s.packets, (k, a, n, w)
        got = pcm[offs[k]: offs[k] + w["samples"] * s.channels]
        assert same_bits(got, s.truth(ctx, s16)[a: a + w["samples"]].reshape(-1)), (k, a, n, w)
    assert same_bits(pcm, expected(ctx, entries, s16, dense))  # (and the sentinel everywhere else)
    on_device = sum(stats.device_gpu_entropy_streams[g] for g in range(16))
    decodable = sum(1 for s, a, n in entries if s.f.gpu_decode_supported and s.f.window(a, n)["n_packets"])
    assert on_device == (decodable if route != "host" else 0) and decodable > len(entries) // 2


@pytest.mark.parametrize("groups,streams_per_call", [(1, 3), (1, 64), (2, 3), (2, 64), (4, 3), (4, 64)])
def test_the_partition_and_the_cut_change_no_byte(ctx, groups, streams_per_call):
    entries = all_entries()
    want = expected(ctx, entries, True, False)
    for gpu_entropy in (False, True):
        pcm, _, results, _ = call(entries, s16=True, dense=False, device_ids=[0] * groups, streams_per_call=streams_per_call,
                                  gpu_entropy=gpu_entropy, host_threads=2 * groups)
        assert (results["status"] == 0).all() and same_bits(pcm, want), (groups, streams_per_call, gpu_entropy)
        lo = [len(entries) * g // groups for g in range(groups + 1)]
        assert all(lo[results["device_slot"][k]] <= k < lo[results["device_slot"][k] + 1] for k in range(len(entries)))


def member_calls(err):
    """the synth calls made for single members, from the VPZM_PROFILE line of every sub-batch"""
    import re
    counts = [int(n) for n in re.findall(r"(\d+) member calls", err)]
    assert counts, err[-400:]
    return sum(counts), len(counts)


@pytest.mark.parametrize("switch,value", [("VPZM_FAIL_GPU_ENTROPY", "1"), ("VPZM_FAIL_BATCH_CALLS", "1"), ("VPZM_MAX_CALL_VALUES", "40000")])
def test_the_switches_change_no_byte(ctx, monkeypatch, capfd, switch, value):
    """... and each of them took the path it is for: the device's streams, the member calls and the sub-batches say so"""
    entries = all_entries()
    monkeypatch.setenv("VPZM_PROFILE", "1")
    for s16, dense in ((False, True), (True, False)):
        monkeypatch.delenv(switch, raising=False)
        capfd.readouterr()
        plain = call(entries, s16=s16, dense=dense, gpu_entropy=True)
        plain_calls, plain_subs = member_calls(capfd.readouterr().err)
        assert same_bits(plain[0], expected(ctx, entries, s16, dense))
        monkeypatch.setenv(switch, value)
        other = call(entries, s16=s16, dense=dense, gpu_entropy=True)
        other_calls, other_subs = member_calls(capfd.readouterr().err)
        assert same_bits(plain[0], other[0]), (switch, s16)
        for field in FIELDS:
            assert np.array_equal(plain[2][field], other[2][field]), (switch, field)
        devs = [sum(r[3].device_gpu_entropy_streams[g] for g in range(16)) for r in (plain, other)]
        assert devs[0] > 0 and (devs[1] == 0) == (switch == "VPZM_FAIL_GPU_ENTROPY")
        live = sum(1 for s, a, n in entries if s.f.window(a, n)["n_packets"])
        assert plain_calls == 0 and other_calls == (live if switch == "VPZM_FAIL_BATCH_CALLS" else 0), (switch, other_calls, live)
        assert (other_subs > plain_subs) == (switch == "VPZM_MAX_CALL_VALUES"), (switch, plain_subs, other_subs)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_window_over_a_skipped_last_packet(ctx, gpu_entropy):
    """issue6test.ogg's trailing packet fails the window check: the whole decode ends 63 samples short of the total, and so does a window
    over the last 5 000 samples"""
    from multi_support import single_stream_pcm
    s = Stream(golden("issue6test.ogg"), False)
    ref = single_stream_pcm(ctx, s.raw)
    assert ref.shape[0] == s.total - 63
    entries = [(s, s.total - 5000, 5000), (s, s.total - 5000, -1)]
    pcm, offs, results, _ = call(entries, gpu_entropy=gpu_entropy, dense=False)
    want, _, _ = place(entries, False, False)
    for k in range(2):
        assert results["status"][k] == 0 and results["samples"][k] == 5000 - 63 and results["skipped_packets"][k] == 1
        assert results["packets"][k] == s.f.window(s.total - 5000, 5000)["n_packets"] < s.packets
        want[offs[k]: offs[k] + (5000 - 63) * s.channels] = ref[s.total - 5000:].reshape(-1)
    assert same_bits(pcm, want)


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_bad_entry_costs_only_itself(ctx, gpu_entropy):
    from vorbispizza_amd import multi
    s = streams()["stereo_coupled_res2_30"]
    garbage = np.frombuffer(b"not an ogg file at all" * 10, dtype=np.uint8)
    a, n = s.bounds[3] + 7, 3000
    entries = [(s, a, n)] * 7
    ranges = [(a, n), (-1, n), (a, n), (s.total + 1, n), (a, n), (a, n), (a, n)]
    datas = [s.data] * 5 + [garbage, s.data]
    caps = np.array([n, n, n, n, n - 1, n, n], dtype=np.int64)  # entry 4: an area one sample too small
    pcm, offs, _ = place(entries, False, False)
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    results, _ = d.decode_ranges(datas, ranges, pcm, offs, caps)
    d.close()
    assert list(results["status"]) == [0, multi.E_RANGE, 0, multi.E_RANGE, multi.E_CAPACITY, multi.E_OPEN, 0]
    want, _, _ = place(entries, False, False)
    for k in (0, 2, 6):
        assert results["samples"][k] == n
        want[offs[k]: offs[k] + n * s.channels] = s.truth(ctx, False)[a: a + n].reshape(-1)
    assert (results["samples"][[1, 3, 4, 5]] == 0).all() and same_bits(pcm, want)


def test_damaged_audio_is_the_same_on_both_routes(ctx):
    from synth_support import damage_audio
    from multi_support import single_stream_pcm
    clean = [golden("3test.ogg"), golden("2test.ogg"), streams()["stereo_coupled_res2_30"].raw, streams()["six_channels_51_12"].raw]
    damaged = [Stream(damage_audio(raw, seed, hits), False) for raw, (seed, hits) in zip(clean, ((1, 8), (2, 16), (3, 6), (4, 4)))]
    entries = []
    for s in damaged:
        b = s.bounds
        entries += [(s, 0, -1), (s, b[len(b) // 2] + 3, 4000), (s, b[2] - 1, b[5] - b[2] + 2), (s, max(0, s.total - 3000), -1), (s, b[1], 1)]
    runs = [call(entries, dense=False, gpu_entropy=g, streams_per_call=4) for g in (False, True)]
    assert sum(runs[1][3].device_gpu_entropy_streams[g] for g in range(16)) > 0
    for field in FIELDS:
        assert np.array_equal(runs[0][2][field], runs[1][2][field]), field
    assert same_bits(runs[0][0], runs[1][0])
    pcm, offs, results, _ = runs[0]
    assert (results["status"] == 0).all()  # (they all opened: the damage is in the audio pages)
    whole = [k for k, (s, a, n) in enumerate(entries) if (a, n) == (0, -1)]
    clean_pcm = [golden("3test.ogg"), golden("2test.ogg")]
    for k, raw in zip(whole, clean_pcm):  # ... and it reached the samples: the fixtures' whole windows are not the clean decode
        ref = single_stream_pcm(ctx, raw).reshape(-1)
        m = min(ref.size, int(results["samples"][k]) * entries[k][0].channels)
        assert not np.array_equal(pcm[offs[k]: offs[k] + m], ref[:m])
    covered = np.zeros(pcm.size, dtype=bool)
    for k, (s, a, n) in enumerate(entries):
        assert 0 <= results["samples"][k] <= s.f.window(a, n)["samples"]  # (fewer than asked, never more)
        covered[offs[k]: offs[k] + results["samples"][k] * s.channels] = True
    assert (pcm[~covered] == SENTINEL).all()


def test_library_ranges_library_on_one_dispatcher(ctx):
    from vorbispizza_amd import multi
    raws = [golden("3test.ogg"), golden("1test.ogg"), streams()["stereo_floor0_12"].raw, streams()["stereo_coupled_res2_30"].raw] * 3
    ss = {r: Stream(r, False) for r in set(raws)}
    caps = np.array([ss[r].total + 16 for r in raws], dtype=np.int64)
    sizes = np.array([c * ss[r].channels for c, r in zip(caps, raws)], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    datas = [ss[r].data for r in raws]
    entries = all_entries()
    d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
    try:
        lib = []
        for _ in range(2):
            pcm = np.full(int(sizes.sum()), SENTINEL, dtype=np.float32)
            lib.append((pcm, d.decode_library(datas, pcm, offs, caps)[0]))
            ranged = [call(entries, dense=False, dispatcher=d) for _ in range(2)]
            assert same_bits(ranged[0][0], expected(ctx, entries, False, False)) and same_bits(ranged[0][0], ranged[1][0])
            assert ranged[0][3].pinned_mib == ranged[1][3].pinned_mib  # (a repeated ranges call allocates nothing)
    finally:
        d.close()
    assert same_bits(lib[0][0], lib[1][0])
    for field in FIELDS:
        assert np.array_equal(lib[0][1][field], lib[1][1][field]), field
    for k, r in enumerate(raws):
        ref = ss[r].truth(ctx, False)
        assert lib[0][1]["samples"][k] == ref.shape[0] and same_bits(lib[0][0][offs[k]: offs[k] + ref.size], ref.reshape(-1))
