"""vpzm_options.gpu_entropy (include/vorbispizza_multi.h, host/vorbis_multi.cpp): the dispatcher plans eligible streams on its
host threads and entropy-decodes them on their device.  Every test runs the same job through two dispatchers, the option off and
on: the PCM array -- guard values between the streams' areas included -- and every field of the results are the same byte for
byte, whatever the partition, the sub-batch cut, the PCM type, the residue type, the damage and the failure path."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ("1test.ogg", "2test.ogg", "3test.ogg", "issue6test.ogg")
FIELDS = ("status", "device_slot", "channels", "sample_rate", "samples", "packets", "skipped_packets")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def fixtures():
    return [open(os.path.join(GOLDEN, n), "rb").read() for n in FIXTURES]


def library_24():
    raws = fixtures()
    return [raws[i % 4] for i in range(24)]  # each fixture six times, the setups interleaved


def synthetic(name, packets=24):
    import synthetic_streams as ss
    stream, rng = ss.ALL[name]()
    ogg, _ = stream.build(rng, packets)
    return bytes(ogg)


def supported(raw):
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(raw)
    try:
        return f.gpu_decode_supported
    finally:
        f.close()


def run(raws, gpu_entropy, device_ids=(0,), **opt):
    from multi_support import run_dispatcher
    opt.setdefault("host_threads", 4)
    return run_dispatcher(list(device_ids), raws, gpu_entropy=gpu_entropy, **opt)


def on_device_streams(stats):
    return sum(stats.device_gpu_entropy_streams[g] for g in range(16))


def payload_bytes(stats):
    return sum(stats.device_payload_bytes[g] for g in range(16))


def assert_same(off, on, fields=FIELDS):
    for field in fields:
        assert np.array_equal(off[2][field], on[2][field]), (field, off[2][field], on[2][field])
    assert off[0].dtype == on[0].dtype and off[0].tobytes() == on[0].tobytes()  # (the gaps between the areas still hold their guard value)


_off = {}


def off_24(s16):
    """the 24-stream job with the option off: computed once, compared against by every test that decodes that job"""
    if s16 not in _off:
        _off[s16] = run(library_24(), False, s16=s16)
        assert (_off[s16][2]["status"] == 0).all() and on_device_streams(_off[s16][3]) == 0 and payload_bytes(_off[s16][3]) == 0
    return _off[s16]


@pytest.mark.parametrize("s16", [False, True])
def test_bit_equality_and_accounting(s16):
    off = off_24(s16)
    on = run(library_24(), True, s16=s16)
    assert_same(off, on)
    assert on_device_streams(on[3]) == 24
    assert payload_bytes(on[3]) > 0
    # (the packet bytes of a container are less than the container, and most of it)
    total = sum(len(r) for r in library_24())
    assert total // 2 < payload_bytes(on[3]) < total + 24 * 8
    assert int(on[2]["skipped_packets"].sum()) == 6  # (issue6test.ogg's trailing packet fails the window check, in both)


def test_mixed_eligibility_in_one_call():
    import synthetic_streams as ss
    raws = fixtures() + [synthetic(name) for name in ss.ALL] + fixtures()[:2] + [synthetic("stereo_floor0", 9)]
    want = sum(1 for r in raws if supported(r))
    assert 0 < want < len(raws)  # (both kinds occur: the Floor0 stream stays on the host)
    off = run(raws, False, streams_per_call=3)
    on = run(raws, True, streams_per_call=3)
    assert (off[2]["status"] == 0).all()
    assert_same(off, on)
    assert on_device_streams(on[3]) == want and on_device_streams(off[3]) == 0


@pytest.mark.parametrize("groups", [1, 2, 4])
def test_partitions(groups):
    on = run(library_24(), True, device_ids=[0] * groups, host_threads=2 * groups)
    base = off_24(False)
    if groups == 1:
        assert_same(base, on)
    else:  # (device_slot is the partition's)
        assert_same(base, on, fields=[f for f in FIELDS if f != "device_slot"])
        assert sorted(set(on[2]["device_slot"])) == list(range(groups))
    assert on_device_streams(on[3]) == 24


@pytest.mark.parametrize("streams_per_call", [1, 5, 0])
def test_sub_batch_cuts(streams_per_call):
    on = run(library_24(), True, streams_per_call=streams_per_call)
    assert_same(off_24(False), on)
    assert on_device_streams(on[3]) == 24


def test_a_call_cut_by_the_values_it_holds(monkeypatch):
    from vorbispizza_amd.front import OggVorbisFile
    values = max(OggVorbisFile(r).info.residue_floats for r in fixtures())
    # (two and a half of the largest stream: its six copies ride in three calls, the small fixtures in one or two)
    monkeypatch.setenv("VPZM_MAX_CALL_VALUES", str(values * 5 // 2))
    on = run(library_24(), True, streams_per_call=0)
    monkeypatch.delenv("VPZM_MAX_CALL_VALUES")
    assert_same(off_24(False), on)
    assert on_device_streams(on[3]) == 24


def test_float_residue_on_the_device():
    on = run(library_24(), True, float_residue=True)
    assert_same(off_24(False), on)
    assert on_device_streams(on[3]) == 24


def test_damaged_audio():
    from synth_support import damage_audio
    from vorbispizza_amd.front import OggVorbisFile
    clean = fixtures()
    mono = synthetic("mono_floor1_res1")  # (three modes in a two-bit field: damage can name the unused one)
    damaged = [damage_audio(mono, seed, hits) for seed, hits in ((6, 16), (7, 16), (24, 4), (32, 4))]
    damaged += [damage_audio(clean[i % 4], 40 + i, (1, 4, 16, 64)[i % 4]) for i in range(8)]
    assert len(damaged) == 12
    # the host path itself gives up packets of some of these streams (what skipped_packets counts before any window check)
    failures = []
    for r in damaged:
        f = OggVorbisFile(r)
        f.decode_packets()
        failures.append(f.decode_failures()[0])
        f.close()
    assert sum(1 for n in failures if n > 0) >= 1, failures
    raws = []
    for i, r in enumerate(damaged):
        raws += [clean[i % 4], r] if i % 3 else [mono, r]
    off = run(raws, False, streams_per_call=5)
    on = run(raws, True, streams_per_call=5)
    assert_same(off, on)
    assert (off[2]["skipped_packets"] > 0).any()
    for k, r in enumerate(raws):
        if r in damaged:
            assert off[2]["skipped_packets"][k] >= failures[damaged.index(r)], k
    # (every undamaged neighbour went to the device, and damaged streams with them)
    assert on_device_streams(on[3]) > sum(1 for r in raws if r not in damaged)


def test_member_by_member_after_a_failed_call(monkeypatch):
    monkeypatch.setenv("VPZM_FAIL_BATCH_CALLS", "1")
    on = run(library_24(), True)
    monkeypatch.delenv("VPZM_FAIL_BATCH_CALLS")
    assert_same(off_24(False), on)
    assert on_device_streams(on[3]) == 24


def test_a_sub_batch_the_device_refuses_takes_the_host_path(monkeypatch):
    monkeypatch.setenv("VPZM_FAIL_GPU_ENTROPY", "1")
    on = run(library_24(), True)
    monkeypatch.delenv("VPZM_FAIL_GPU_ENTROPY")
    assert_same(off_24(False), on)
    assert on_device_streams(on[3]) == 0 and payload_bytes(on[3]) == 0


@pytest.mark.parametrize("s16", [False, True])
def test_caller_areas_packed_with_no_slack(s16):
    """capacities that are the streams' lengths and offsets packed: the one layout in which a wrong offset or length of a
    device-decoded member's download overwrites a neighbour's samples instead of a guard gap"""
    raws = fixtures() * 2
    off = run(raws, False, s16=s16, streams_per_call=3, capacity_slack=0)
    on = run(raws, True, s16=s16, streams_per_call=3, capacity_slack=0)
    assert (off[2]["status"] == 0).all()
    assert_same(off, on)
    assert on_device_streams(on[3]) == 8 and on_device_streams(off[3]) == 0


def test_an_area_one_sample_too_small_costs_only_its_stream():
    from vorbispizza_amd import multi
    from vorbispizza_amd.front import OggVorbisFile
    raws = library_24()[:8]
    info = [(OggVorbisFile(r).channels, int(OggVorbisFile(r).total_samples)) for r in raws]
    caps = np.array([n for _, n in info], dtype=np.int64)
    caps[5] -= 1
    guard = 64
    sizes = np.array([c * n + guard for c, n in info], dtype=np.int64)  # (the areas at their exact size, guard values between them)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    outs = []
    for gpu_entropy in (False, True):
        pcm = np.full(int(sizes.sum()), np.float32(7.0), dtype=np.float32)
        d = multi.Dispatcher([0], host_threads=3, streams_per_call=4, gpu_entropy=gpu_entropy)
        try:
            res, stats = d.decode_library([np.frombuffer(r, dtype=np.uint8) for r in raws], pcm, offs, caps)
        finally:
            d.close()
        outs.append((pcm, res, stats))
    (pcm0, res0, _), (pcm1, res1, stats1) = outs
    assert res1["status"][5] == multi.E_CAPACITY and (np.delete(res1["status"], 5) == 0).all()
    for field in FIELDS:
        assert np.array_equal(res0[field], res1[field]), field
    assert pcm0.tobytes() == pcm1.tobytes()
    for k, (c, n) in enumerate(info):
        end = offs[k] + c * int(res1["samples"][k])
        assert (pcm1[end: offs[k] + sizes[k]].view(np.uint32) == np.float32(7.0).view(np.uint32)).all(), k  # nothing beyond what was produced
    assert (pcm1[offs[5]: offs[5] + sizes[5]] == np.float32(7.0)).all()
    assert on_device_streams(stats1) == 7


def test_two_host_threads_share_a_dispatcher():
    from vorbispizza_amd import multi
    from vorbispizza_amd.front import OggVorbisFile
    off = off_24(False)
    raws = library_24()
    infos = {r: (OggVorbisFile(r).channels, int(OggVorbisFile(r).total_samples)) for r in set(raws)}
    caps = np.array([infos[r][1] + 2048 for r in raws], dtype=np.int64)  # (run_dispatcher's layout: the arrays compare whole)
    sizes = np.array([c * infos[r][0] for c, r in zip(caps, raws)], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    d = multi.Dispatcher([0], host_threads=4, gpu_entropy=True)
    jobs = [dict(pcm=np.full(int(sizes.sum()), np.float32(7.0), dtype=np.float32)) for _ in range(2)]

    def call(j):
        try:
            j["res"], j["stats"] = d.decode_library([np.frombuffer(r, dtype=np.uint8) for r in raws], j["pcm"], offs, caps)
        except Exception as e:  # noqa: BLE001 (handed to the asserting thread)
            j["err"] = e

    threads = [threading.Thread(target=call, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    d.close()
    for j in jobs:
        assert "err" not in j, j.get("err")
        for field in FIELDS:
            assert np.array_equal(off[2][field], j["res"][field]), field
        assert j["pcm"].tobytes() == off[0].tobytes()
        assert on_device_streams(j["stats"]) == 24


def test_page_locked_memory_does_not_grow():
    """a device-decoded sub-batch's slot holds packet records, spans and packet bytes: no residue, posts or counts on the host"""
    raws = library_24() * 4
    off = run(raws, False)
    on = run(raws, True)
    assert_same(off, on)
    assert 0 <= on[3].pinned_mib <= off[3].pinned_mib and off[3].pinned_mib > 0
