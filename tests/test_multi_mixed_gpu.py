"""vpzm_set_mixed_setups (include/vorbispizza_multi_mixed.h, host/vorbis_multi.cpp): with gpu_entropy, streams of different setup
headers that agree in channels, block sizes and residue type ride in one device-decoded sub-batch -- one upload, one
vpz_entropy_group_decode, one synth call on a decoder of the merged setup.  Every test runs one library with the option off and
on: the PCM array, guard values between the areas included, and every field of the results are the same byte for byte, whatever
the failure path, the bound of a merged setup, the partition and the damage; vpzm_last_call_counts says what was cut.

Library L: six stereo 256/2048 setups of the writer (synthetic_streams.stereo_coupled_res2, seeds 2 .. 52, 12 packets; every seed
opens and is decodable on the device -- `library` asserts it, none had to be replaced), four copies each in round-robin order; the
four fixtures; the Floor0 stream (host path); the mono stream.  30 streams: one wave at streams_per_call = 8."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("1test.ogg", "2test.ogg", "3test.ogg", "issue6test.ogg")
FIELDS = ("status", "device_slot", "channels", "sample_rate", "samples", "packets", "skipped_packets")
SEEDS = (2, 12, 22, 32, 42, 52)


_RAW = {}


def writer(name, seed=None, packets=12):
    import synthetic_streams as ss
    if (name, seed, packets) not in _RAW:
        st, rng = getattr(ss, name)() if seed is None else getattr(ss, name)(seed)
        _RAW[(name, seed, packets)] = bytes(st.build(rng, packets)[0])
    return _RAW[(name, seed, packets)]


def supported(raw):
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(raw)
    try:
        return f.gpu_decode_supported
    finally:
        f.close()


def library():
    stereo = [writer("stereo_coupled_res2", seed) for seed in SEEDS]
    assert all(supported(r) for r in stereo) and len(set(stereo)) == 6
    raws = [stereo[i % 6] for i in range(24)]
    raws += [open(os.path.join(GOLDEN, n), "rb").read() for n in FIXTURES]
    raws += [writer("stereo_floor0"), writer("mono_floor1_res1")]
    assert len(raws) == 30 and not supported(raws[28])
    return raws


def run(raws, s16=False, mixed=False, device_ids=(0,), dispatcher=None, **opt):
    """tests/test_multi_gpu.py: run_dispatcher's layout (areas with 2048 samples of slack, guard values all over) and the call's counts"""
    from vorbispizza_amd import multi
    from vorbispizza_amd.front import OggVorbisFile
    infos = {}
    for r in set(raws):
        f = OggVorbisFile(r)
        infos[r] = (f.channels, int(f.total_samples))
        f.close()
    caps = np.array([infos[r][1] + 2048 for r in raws], dtype=np.int64)
    sizes = np.array([c * infos[r][0] for c, r in zip(caps, raws)], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    pcm = np.full(int(sizes.sum()), 7, dtype=np.int16) if s16 else np.full(int(sizes.sum()), np.float32(7.0), dtype=np.float32)
    datas = [np.frombuffer(r, dtype=np.uint8) for r in raws]
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 8)
    opt.setdefault("gpu_entropy", True)
    d = dispatcher or multi.Dispatcher(list(device_ids), mixed_setups=mixed, **opt)
    try:
        results, stats = d.decode_library(datas, pcm, offs, caps, s16=s16)
        counts = d.call_counts()
    finally:
        if dispatcher is None:
            d.close()
    return pcm, results, stats, counts


def assert_same(a, b, fields=FIELDS):
    for field in fields:
        assert np.array_equal(a[1][field], b[1][field]), (field, a[1][field], b[1][field])
    assert a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes()  # (the gaps between the areas still hold their guard value)


def on_device_streams(stats):
    return sum(stats.device_gpu_entropy_streams[g] for g in range(16))


_off = {}


def off(s16=False):
    """L with the option off: computed once, compared against by every test"""
    if s16 not in _off:
        _off[s16] = run(library(), s16=s16)
        got = _off[s16]
        assert (got[1]["status"] == 0).all() and on_device_streams(got[2]) == 29
        assert got[3].mixed_sub_batches == 0 and got[3].max_setups_per_sub_batch == 1
        assert got[3].sub_batches == got[3].device_decoded_sub_batches + 1  # (the Floor0 stream's)
    return _off[s16]


@pytest.mark.parametrize("s16", [False, True])
def test_off_against_on(s16):
    on = run(library(), s16=s16, mixed=True)
    assert_same(off(s16), on)
    assert on_device_streams(on[2]) == 29
    # the three sub-batches of eight writer streams each hold all six setups
    assert on[3].mixed_sub_batches >= 3 and on[3].max_setups_per_sub_batch == 6
    assert on[3].sub_batches < off(s16)[3].sub_batches and on[3].decoders_created < off(s16)[3].decoders_created
    assert on[3].sub_batches == on[3].device_decoded_sub_batches + 1


@pytest.mark.parametrize("switch", ["VPZM_FAIL_GPU_ENTROPY", "VPZM_FAIL_BATCH_CALLS"])
def test_the_failure_paths_of_a_mixed_sub_batch(monkeypatch, switch):
    """the device refuses every sub-batch: each member through its own stream handle, the shift, the merged decoder; every batch
    call fails: member by member on the merged decoder"""
    monkeypatch.setenv(switch, "1")
    on = run(library(), mixed=True)
    monkeypatch.delenv(switch)
    assert_same(off(), on)
    assert on[3].mixed_sub_batches >= 3 and on[3].max_setups_per_sub_batch == 6
    assert on_device_streams(on[2]) == (0 if switch == "VPZM_FAIL_GPU_ENTROPY" else 29)
    assert on[3].device_decoded_sub_batches == (0 if switch == "VPZM_FAIL_GPU_ENTROPY" else on[3].sub_batches - 1)


def test_a_bound_on_the_merged_mappings(monkeypatch):
    """every writer setup has two mappings: four mappings are two setups to a merged setup"""
    monkeypatch.setenv("VPZM_MAX_MERGED_MAPPINGS", "4")
    on = run(library(), mixed=True)
    monkeypatch.delenv("VPZM_MAX_MERGED_MAPPINGS")
    assert_same(off(), on)
    assert on[3].max_setups_per_sub_batch == 2 and on[3].mixed_sub_batches >= 3


def test_one_dispatcher_on_off_on():
    from vorbispizza_amd import multi
    d = multi.Dispatcher([0], host_threads=4, streams_per_call=8, gpu_entropy=True, mixed_setups=True)
    try:
        first = run(library(), dispatcher=d)
        d.set_mixed_setups(False)
        second = run(library(), dispatcher=d)
        d.set_mixed_setups(True)
        third = run(library(), dispatcher=d)
    finally:
        d.close()
    for got in (first, second, third):
        assert_same(off(), got)
    assert [g[3].max_setups_per_sub_batch for g in (first, second, third)] == [6, 1, 6]
    assert second[3].mixed_sub_batches == 0 and first[3].mixed_sub_batches == third[3].mixed_sub_batches >= 3
    assert second[3].sub_batches == off()[3].sub_batches and first[3].sub_batches == third[3].sub_batches
    # (the lanes keep their decoders and groups: the third run creates none it had)
    assert third[3].decoders_created <= first[3].decoders_created


@pytest.mark.parametrize("groups", [2, 4])
def test_partitions(groups):
    on = run(library(), mixed=True, device_ids=[0] * groups, host_threads=2 * groups)
    assert_same(off(), on, fields=[f for f in FIELDS if f != "device_slot"])
    assert sorted(set(on[1]["device_slot"])) == list(range(groups))
    assert on_device_streams(on[2]) == 29 and on[3].mixed_sub_batches >= groups


def test_more_setups_than_a_decoder_has_floors():
    """34 writer setups of two floors each, all distinct: 68 floors, and vpz_decoder_create takes 64.  The class's merged setup is full
    at 32 setups and the last two start another: one sub-batch of 32 setups, one of two, every stream decoded as with the option off."""
    from vorbispizza_amd.front import OggVorbisFile
    # (seed 1070, k = 10, is left out: its random books happen to hold 16-bit integers only, which is another merge class)
    raws = [writer("stereo_coupled_res2", 1000 + 7 * k, 4) for k in range(35) if k != 10]
    floors = set()
    for r in raws:
        f = OggVorbisFile(r)
        assert f.gpu_decode_supported and len(f.floors) == 2 and not f.residue_is_integral
        floors |= {(tuple(x), m) for x, m in f.floors}
        f.close()
    assert len(floors) == 68
    base = run(raws, streams_per_call=40)
    on = run(raws, mixed=True, streams_per_call=40)
    assert (base[1]["status"] == 0).all() and (base[1]["samples"] > 0).all() and base[3].sub_batches == 34
    assert_same(base, on)
    assert on[3].sub_batches == 2 and on[3].mixed_sub_batches == 2 and on[3].max_setups_per_sub_batch == 32
    assert on[3].device_decoded_sub_batches == 2 and on_device_streams(on[2]) == 34


def test_a_refused_call_leaves_no_counts():
    """vpzm_last_call_counts is of the LAST call, also when that call was refused for its arguments"""
    import ctypes as C

    from vorbispizza_amd import multi
    d = multi.Dispatcher([0], host_threads=2, streams_per_call=8, gpu_entropy=True, mixed_setups=True)
    try:
        run(library()[:8], dispatcher=d)
        assert d.call_counts().sub_batches > 0
        assert multi.lib().vpzm_decode_library(d._h, -1, None, None, 0, None, None, None, None, None) == multi.E_ARG
        counts = d.call_counts()
        assert bytes(counts) == bytes(C.sizeof(multi.CallCounts))
    finally:
        d.close()


def test_damaged_members_inside_mixed_sub_batches():
    """tests/test_multi_entropy_gpu.py's damage (damage_audio).  Eight writer streams of 24 packets from six setups, three of them
    damaged, are one mixed sub-batch; the two stereo fixtures and a damaged copy of each are another (issue6test.ogg's trailing
    packet fails the window check, so skipped_packets is not all zero)."""
    from synth_support import damage_audio

    clean = [writer("stereo_coupled_res2", seed, 24) for seed in SEEDS]
    fixtures = [open(os.path.join(GOLDEN, n), "rb").read() for n in FIXTURES[2:]]
    raws = [clean[0], damage_audio(clean[1], 41, 16), clean[2], damage_audio(clean[3], 42, 4), clean[4], clean[5],
            damage_audio(clean[0], 43, 64), clean[1],
            fixtures[0], damage_audio(fixtures[1], 44, 16), damage_audio(fixtures[0], 46, 64), fixtures[1]]
    assert all(supported(r) for r in raws)
    base = run(raws)
    on = run(raws, mixed=True)
    assert_same(base, on)
    assert (on[1]["status"] == 0).sum() >= 9 and (on[1]["skipped_packets"] > 0).any()  # (the undamaged ones at least)
    assert on[3].sub_batches == 2 and on[3].mixed_sub_batches == 2 and on[3].max_setups_per_sub_batch == 6
    assert base[3].sub_batches == 8 and base[3].mixed_sub_batches == 0
    assert on_device_streams(on[2]) == on_device_streams(base[2]) >= 9
