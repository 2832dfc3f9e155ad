"""vpz_entropy_group_decode (vorbispizza_entropy_group.h, csrc/entropy.hip: entropy_group_kernel) against the CPU front end: streams
of DIFFERENT setup headers in one call, each stream's posts, post counts and residue byte for byte what vpzh_decode_range_ex /
vpzh_decode_range_i16 write for it from its own setup.

The streams are the writer's (tests/synthetic_streams.py through their seeds, 12 packets each; tests/edge_streams.py for the tiled
ones, which carry not-decoded packets).  Every seed used here was checked on the CPU: its stream opens and gpu_decode_supported
is true (stereo 2 / 12 / 22 / 32, three channels 3 / 13 / 23, mono 1 / 11 / 21; none had to be replaced) -- and `setups` asserts it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from gpu_context import ctx  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
STEREO, THREE, MONO = (2, 12, 22, 32), (3, 13, 23), (1, 11, 21)


def both_spaces():
    from vorbispizza_amd import capi
    return (capi.MEM_HOST, capi.MEM_DEVICE)


# ------------------------------------------------------------------------------------------------ setups and batches
class Setup:
    """One opened stream: its image, its plan and the CPU's decode of it (both computed once, never changed)."""

    def __init__(self, raw, count=None):
        from vorbispizza_amd import capi
        from vorbispizza_amd.front import OggVorbisFile
        self.f = f = OggVorbisFile(raw)
        assert f.gpu_decode_supported, f.last_error()
        self.image = f.entropy_setup()
        self.channels, self.integral = f.channels, f.residue_is_integral
        self.mapping_count = len(f.mappings)
        self.count = f.audio_packets if count is None else count
        self.packets, self.spans, self.payload, self.used = f.plan_packets(0, self.count)
        halves = np.where(self.packets["flags"] & capi.PKT_BLOCK_FLAG, f.block_size1, f.block_size0) // 2
        self.lens = self.channels * halves.astype(np.int64)
        self.decoded = (self.packets["flags"] & capi.PKT_NOT_DECODED) == 0
        self.own = np.zeros(self.used, dtype=bool)  # the residue values its decoded packets write
        for k in np.flatnonzero(self.decoded):
            o = int(self.packets["residue_offset"][k])
            self.own[o:o + int(self.lens[k])] = True
        self._refs = {}

    def ref(self, i16):
        """(residue[used], posts, counts) of the first `count` packets on the CPU"""
        if i16 not in self._refs:
            pk, res, posts, counts = self.f.decode_packets(int16=i16)
            assert pk[:self.count].tobytes() == self.packets.tobytes()
            self._refs[i16] = (res[:self.used], posts[:self.count * self.channels], counts[:self.count * self.channels])
        return self._refs[i16]


_SETUPS = {}


def setups(kind, seeds):
    """the writer's streams of one class, one per seed, 12 packets each"""
    import synthetic_streams as ss
    out = []
    for seed in seeds:
        if (kind, seed) not in _SETUPS:
            st, rng = getattr(ss, kind)(seed)
            _SETUPS[(kind, seed)] = Setup(bytes(st.build(rng, 12)[0]))
        out.append(_SETUPS[(kind, seed)])
    assert len({s.image for s in out}) == len(out)  # different seeds: different setups
    return out


def tiles(kind, seeds):
    import edge_streams as es
    out = []
    for seed in seeds:
        if (kind, seed) not in _SETUPS:
            _SETUPS[(kind, seed)] = Setup(getattr(es, kind)(seed))
        out.append(_SETUPS[(kind, seed)])
    assert len({s.image for s in out}) == len(out)
    return out


class Batch:
    """Streams order[0], order[1] ... (indices into `sets`) back to back in one batch: stream s has the records of its setup's plan
    with stream = s, the residue at a base of its own (`pad` values left free behind every stream) and mapping + bases[setup]."""

    def __init__(self, sets, order, bases=None, pad=0, n_packets=None):
        self.sets, self.order, self.pad = sets, list(order), pad
        self.bases = [0] * len(sets) if bases is None else list(bases)
        self.channels = sets[0].channels
        pk, sp, pay = [], [], []
        self.res_base, self.pk_base = [], []
        res_base = pay_base = pk_base = 0
        for s, i in enumerate(self.order):
            t = sets[i]
            p = t.packets.copy()
            p["stream"] = s
            p["residue_offset"] += res_base
            p["mapping"] += self.bases[i]
            spans = t.spans.copy()
            spans[:, 0] += pay_base
            pk.append(p)
            sp.append(spans)
            pay.append(t.payload)
            self.res_base.append(res_base)
            self.pk_base.append(pk_base)
            res_base += t.used + pad
            pay_base += t.payload.size
            pk_base += t.count
        self.packets, self.spans, self.payload = np.concatenate(pk), np.concatenate(sp), np.concatenate(pay)
        self.n_values = res_base
        self.stream_setup = np.array(self.order, dtype=np.uint8)
        self.stream_base = np.array([self.bases[i] for i in self.order], dtype=np.uint8)
        if n_packets is not None:  # the batch's first n_packets packets (a last stream cut short)
            self.packets, self.spans = self.packets[:n_packets], self.spans[:n_packets]

    def check(self, got, i16, what):
        """every stream of the batch against the CPU's decode of its setup; returns the mask of the residue values written"""
        res, posts, counts = got
        C_ = self.channels
        n = len(self.packets)
        written = np.zeros(res.size, dtype=bool)
        for s, i in enumerate(self.order):
            t = self.sets[i]
            rres, rposts, rcounts = t.ref(i16)
            k0 = self.pk_base[s]
            m = min(t.count, n - k0)
            if m <= 0:
                break
            assert counts[k0 * C_:(k0 + m) * C_].tobytes() == rcounts[:m * C_].tobytes(), (what, s)
            assert posts[k0 * C_:(k0 + m) * C_].tobytes() == rposts[:m * C_].tobytes(), (what, s)
            b = self.res_base[s]
            own = t.own
            if m < t.count:
                own = np.zeros(t.used, dtype=bool)
                for k in np.flatnonzero(t.decoded[:m]):
                    o = int(t.packets["residue_offset"][k])
                    own[o:o + int(t.lens[k])] = True
            assert res[b:b + t.used][own].tobytes() == rres[own].tobytes(), (what, s)
            written[b:b + t.used] = own
        return written


def group_decode(ctx, group, batch, i16, mem_space, sentinel=None, extra_records=0, tail=0):
    """the batch through vpz_entropy_group_decode; residue zeroed (or filled with `sentinel`), posts / counts filled with 0x5A5A / 0xEE"""
    import torch

    from vorbispizza_amd import capi
    n, C_ = len(batch.packets), batch.channels
    dt = np.int16 if i16 else np.float32
    residue = np.full(max(1, batch.n_values + tail), 0 if sentinel is None else sentinel, dtype=dt)
    posts = np.full((n * C_ + extra_records, 64), 0x5A5A, dtype=np.int16)
    counts = np.full(n * C_ + extra_records, 0xEE, dtype=np.uint8)
    if mem_space == capi.MEM_HOST:
        group.decode(batch.stream_setup, batch.stream_base, batch.packets, batch.spans, batch.payload, residue, posts, counts,
                     mem_space=mem_space)
        return residue, posts, counts
    dev = torch.device("cuda", ctx.device)
    d = [torch.from_numpy(a).to(dev) for a in (batch.payload, residue, posts, counts)]
    group.decode(batch.stream_setup, batch.stream_base, batch.packets, batch.spans, d[0], d[1], d[2], d[3], mem_space=mem_space)
    ctx.synchronize()
    return tuple(x.cpu().numpy() for x in d[1:])


def new_group(ctx, sets):
    from vorbispizza_amd.entropy import EntropyGroup
    return EntropyGroup(ctx, [s.image for s in sets])


# ------------------------------------------------------------------------------------------------ the tests
def test_four_stereo_setups_two_copies_each_in_one_call(ctx):
    """streams 0,1,2,3,0,1,2,3 of 12 packets: 64 consecutive packets span five streams, so the lane list reorders them (four runs
    of 24 lanes, each padded to 64)"""
    sets = setups("stereo_coupled_res2", STEREO)
    batch = Batch(sets, [0, 1, 2, 3, 0, 1, 2, 3])
    assert len(batch.packets) == 96
    group = new_group(ctx, sets)
    for ms in both_spaces():
        batch.check(group_decode(ctx, group, batch, False, ms), False, ms)
    group.close()


def test_three_three_channel_setups_in_one_group(ctx):
    """two submaps: the decode buffer; the class-word cache sized by the largest setup"""
    sets = setups("three_channels_two_submaps", THREE)
    batch = Batch(sets, [2, 0, 1, 1, 2, 0, 0])
    group = new_group(ctx, sets)
    for ms in both_spaces():
        batch.check(group_decode(ctx, group, batch, False, ms), False, ms)
    group.close()


def test_three_mono_setups_with_mapping_bases(ctx):
    """the records carry mapping + base (0, 2, 4: every setup has two mappings); one base wrong is refused with nothing written"""
    from vorbispizza_amd import capi
    sets = setups("mono_floor1_res1", MONO)
    assert all(s.mapping_count == 2 for s in sets)
    batch = Batch(sets, [0, 1, 2, 2, 1, 0], bases=[0, 2, 4])
    assert set(batch.packets["mapping"]) == {0, 1, 2, 3, 4, 5}
    group = new_group(ctx, sets)
    for ms in both_spaces():
        batch.check(group_decode(ctx, group, batch, False, ms), False, ms)
    # setup 2 at base 2: its records' 4 and 5 become mappings 2 and 3 of a setup that has two
    bad = batch.stream_base.copy()
    bad[batch.stream_setup == 2] = 2
    n = len(batch.packets)
    residue = np.full(batch.n_values, 7.0, dtype=np.float32)
    posts = np.full((n, 64), 3, dtype=np.int16)
    counts = np.full(n, 9, dtype=np.uint8)
    rc = group.decode_raw(batch.stream_setup, bad, batch.packets, batch.spans, batch.payload, residue, posts, counts, capi.MEM_HOST)
    assert rc == capi.E_INVALID_ARG and (residue == 7.0).all() and (posts == 3).all() and (counts == 9).all()
    group.close()


def test_int16_over_the_two_fixtures(ctx):
    """the first 40 packets of 3test.ogg and issue6test.ogg in one group, VPZ_RESIDUE_I16, against vpzh_decode_range_i16"""
    sets = [Setup(open(os.path.join(GOLDEN, name), "rb").read(), 40) for name in ("3test.ogg", "issue6test.ogg")]
    assert all(s.integral for s in sets) and sets[0].image != sets[1].image
    batch = Batch(sets, [0, 1, 1, 0])
    group = new_group(ctx, sets)
    for ms in both_spaces():
        for i16 in (True, False):
            batch.check(group_decode(ctx, group, batch, i16, ms), i16, (ms, i16))
    group.close()


def test_a_group_of_one_setup_writes_what_vpz_entropy_decode_writes(ctx):
    from synth_support import device_decode

    from vorbispizza_amd.entropy import EntropySetup
    sets = tiles("tile_three_channels", (0,))
    batch = Batch(sets, [0] * 7)
    group = new_group(ctx, sets)
    setup = EntropySetup(ctx, sets[0].image)
    for ms in both_spaces():
        for i16 in (False, True):
            got = group_decode(ctx, group, batch, i16, ms)
            one = device_decode(ctx, setup, batch.packets, batch.spans, batch.payload, batch.n_values, batch.channels, i16, ms)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, one)), (ms, i16)
            batch.check(got, i16, (ms, i16))
    setup.close()
    group.close()


@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("i16", [False, True])
def test_the_call_writes_its_packets_and_nothing_else(ctx, space, i16):
    """Sentinels everywhere first.  After the call: the gaps between the streams' residues (7 values each), the residue regions of
    not-decoded packets (every stream has some) and everything behind the batch still hold them; a not-decoded packet's
    records have count 0 and zero posts; no record beyond n_packets * channels is touched."""
    from vorbispizza_amd import capi
    sets = tiles("tile_three_channels", (0, 1, 2))
    batch = Batch(sets, [0, 1, 2, 1, 0, 2, 2], pad=7)
    n, C_ = len(batch.packets), batch.channels
    idle = np.repeat((batch.packets["flags"] & capi.PKT_NOT_DECODED) != 0, C_)
    for s in range(len(batch.order)):
        assert idle[batch.pk_base[s] * C_:(batch.pk_base[s] + sets[batch.order[s]].count) * C_].any()
    extra_records, tail = 5, 11
    sentinel = 0x1234 if i16 else 12345.0
    group = new_group(ctx, sets)
    residue, posts, counts = group_decode(ctx, group, batch, i16, capi.MEM_HOST if space == "host" else capi.MEM_DEVICE,
                                          sentinel=sentinel, extra_records=extra_records, tail=tail)
    group.close()
    written = batch.check((residue, posts, counts), i16, (space, i16))
    assert (~written).sum() >= tail + 7 * len(batch.order) and (residue[~written] == residue.dtype.type(sentinel)).all()
    assert (posts[n * C_:] == 0x5A5A).all() and (counts[n * C_:] == 0xEE).all()
    assert (counts[:n * C_][idle] == 0).all() and not posts[:n * C_][idle].any()


# lane lists just below and just above 65 536: two mono 64/64 setups of 17 packets, streams alternating, so that each setup's run is
# about half the packets and the first run is padded to a multiple of 64
@pytest.mark.parametrize("n_packets", [65440, 65536, 65600])
def test_both_sides_of_the_launch_switch(ctx, n_packets):
    from vorbispizza_amd import capi
    sets = tiles("tile_mono", (0, 1))
    per = sets[0].count
    assert per == sets[1].count == 17
    copies = -(-n_packets // per)
    batch = Batch(sets, [s % 2 for s in range(copies)], n_packets=n_packets)
    # the lane list's length, as the host builds it: run 0 padded to whole waves, then run 1
    owner = np.repeat(batch.stream_setup, per)[:n_packets]
    n0, n1 = int((owner == 0).sum()), int((owner == 1).sum())
    lanes = -(-n0 // 64) * 64 + n1
    assert (lanes < 65536) == (n_packets == 65440) and lanes - n_packets < 64
    group = new_group(ctx, sets)
    for i16, ms in ((False, capi.MEM_DEVICE), (True, capi.MEM_DEVICE), (False, capi.MEM_HOST)):
        if n_packets != 65536 and ms == capi.MEM_HOST:
            continue
        batch.check(group_decode(ctx, group, batch, i16, ms), i16, (n_packets, i16, ms))
    group.close()


def test_refusals(ctx):
    from vorbispizza_amd import capi, entropy
    stereo, mono = setups("stereo_coupled_res2", STEREO[:2]), setups("mono_floor1_res1", MONO[:1])

    def create(images):
        bufs = [np.frombuffer(im, dtype=np.uint8) for im in images]
        n = len(bufs)
        ptrs = (C.c_void_p * max(1, n))(*[b.ctypes.data for b in bufs])
        sizes = (C.c_uint64 * max(1, n))(*[b.size for b in bufs])
        h = C.c_void_p()
        rc = entropy.lib().vpz_entropy_group_create(ctx._h, ptrs, sizes, n, C.byref(h))
        assert rc != capi.OK and not h.value
        return rc

    assert create([stereo[0].image, mono[0].image]) == capi.E_INVALID_ARG     # two classes
    assert "differ" in ctx.last_error()
    assert create([]) == capi.E_INVALID_ARG
    assert create([stereo[0].image] * 257) == capi.E_INVALID_ARG
    assert create([stereo[0].image, stereo[1].image[:-4]]) == capi.E_INVALID_ARG  # one image that fails its validation

    batch = Batch(stereo, [0, 1, 1])
    group = new_group(ctx, stereo)
    n, C_ = len(batch.packets), batch.channels

    def call(stream_setup=batch.stream_setup, pk=batch.packets, fmt=None):
        residue = np.full(batch.n_values, 7.0, dtype=np.float32)
        posts = np.full((n * C_, 64), 3, dtype=np.int16)
        counts = np.full(n * C_, 9, dtype=np.uint8)
        rc = group.decode_raw(stream_setup, batch.stream_base, pk, batch.spans, batch.payload, residue, posts, counts, capi.MEM_HOST,
                              residue_format=fmt)
        return rc, bool((residue == 7.0).all() and (posts == 3).all() and (counts == 9).all())

    assert call() == (capi.OK, False)
    bad = batch.stream_setup.copy()
    bad[2] = 2
    assert call(stream_setup=bad) == (capi.E_INVALID_ARG, True)
    for stream in (3, -1):
        pk = batch.packets.copy()
        pk["stream"][n - 1] = stream
        assert call(pk=pk) == (capi.E_INVALID_ARG, True)
    assert not stereo[0].integral
    assert call(fmt=capi.RESIDUE_I16) == (capi.E_INVALID_ARG, True)
    group.close()
