"""vpz_entropy_decode (csrc/entropy.hip) at the edges tests/test_entropy_gpu.py does not reach: launches of 8193 .. 65600 packets
(the zero kernel's stride loop, the last 64-lane and the first 256-lane launch, a partial last workgroup), channels 64..254 (words
1 to 3 of the kernel's channel masks), codes of 31 and 32 bits (the overflow list, the 32-bit peek), the random setups of
synthetic_streams.random_stream, memory the call must leave alone, and one setup reused by calls that shrink and grow.

The reference of every comparison is the CPU front end's decode (itself held to the writer's specification model by
tests/test_front_writer_cpu.py): posts, post counts and residue byte for byte, in float32, and in int16 where the stream is integral."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edge_streams as es  # noqa: E402
from synth_support import check_stream, device_decode  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

BIG = 65600


def both_spaces():
    from vorbispizza_amd import capi
    return (capi.MEM_HOST, capi.MEM_DEVICE)


# ------------------------------------------------------------------------------------------------ batches of one tiled stream
class Tiled:
    """One small stream planned again and again as streams 0, 1, 2 ... of one batch (plan_packets(stream_id=s, residue_base=...),
    spans shifted by the payload base), `pad` values left free behind every stream's residue.  The CPU reference is decoded once."""

    def __init__(self, raw, n_packets, pad=0):
        from vorbispizza_amd import capi
        from vorbispizza_amd.front import OggVorbisFile
        f = OggVorbisFile(raw)
        assert f.gpu_decode_supported
        self.f, self.channels, self.per, self.pad = f, f.channels, f.audio_packets, pad
        self.image = f.entropy_setup()
        self.copies = -(-n_packets // self.per)
        pk, sp, pay, self.bases = [], [], [], []
        res_base = pay_base = 0
        for s in range(self.copies):
            p, spans, payload, used = f.plan_packets(0, min(self.per, n_packets - s * self.per), stream_id=s, residue_base=res_base)
            spans = spans.copy()
            spans[:, 0] += pay_base
            pk.append(p)
            sp.append(spans)
            pay.append(payload)
            self.bases.append(res_base)
            res_base += used + pad
            pay_base += payload.size
        self.packets, self.spans, self.payload = np.concatenate(pk), np.concatenate(sp), np.concatenate(pay)
        self.n_values = res_base
        self.integral = f.residue_is_integral
        halves = np.where(self.packets["flags"] & capi.PKT_BLOCK_FLAG, f.block_size1, f.block_size0) // 2
        self.lens = self.channels * halves.astype(np.int64)
        self.decoded = (self.packets["flags"] & capi.PKT_NOT_DECODED) == 0
        assert self.decoded.any() and not self.decoded.all()  # (the header-edge packets are in)
        self.refs = {}

    def ref(self, i16):
        """(residue, posts, counts) of ONE stream on the CPU, and the mask of the residue values its decoded packets own"""
        if i16 not in self.refs:
            pk, res, posts, counts = self.f.decode_packets(int16=i16)
            own = np.zeros(res.size, dtype=bool)
            for k in range(self.per):
                if self.decoded[k]:
                    o = int(pk["residue_offset"][k])
                    own[o:o + int(self.lens[k])] = True
            self.refs[i16] = (res, posts, counts, own)
        return self.refs[i16]

    def cut(self, n):
        """(packets, spans, residue values) of the batch's first n packets"""
        ends = (self.packets["residue_offset"][:n] + self.lens[:n])[self.decoded[:n]]
        return self.packets[:n], self.spans[:n], int(ends.max())

    def check(self, n, i16, got, what):
        """the first n packets of the batch against the tiled reference"""
        res, posts, counts = got
        rres, rposts, rcounts, own = self.ref(i16)
        C, per = self.channels, self.per
        full, rest = divmod(n, per)
        assert np.array_equal(counts[:full * per * C].reshape(full, rcounts.size), np.broadcast_to(rcounts, (full, rcounts.size))), what
        assert np.array_equal(posts[:full * per * C].reshape(full, rposts.size),
                              np.broadcast_to(rposts.reshape(-1), (full, rposts.size))), what
        assert counts[full * per * C:n * C].tobytes() == rcounts[:rest * C].tobytes(), what
        assert posts[full * per * C:n * C].tobytes() == rposts[:rest * C].tobytes(), what
        stride = rres.size + self.pad
        assert full == 0 or (full - 1) * stride + rres.size <= res.size, what
        tiles = np.lib.stride_tricks.as_strided(res, shape=(full, rres.size), strides=(stride * res.itemsize, res.itemsize))
        assert np.array_equal(tiles[:, own].view(np.uint16 if i16 else np.uint32),
                              np.broadcast_to(rres[own].view(np.uint16 if i16 else np.uint32), (full, int(own.sum())))), what
        for k in range(full * per, n):
            if self.decoded[k]:
                o, r = int(self.packets["residue_offset"][k]), int(self.packets["residue_offset"][k]) - self.bases[full]
                assert res[o:o + int(self.lens[k])].tobytes() == rres[r:r + int(self.lens[k])].tobytes(), (what, k)


_TILED = {}


def tiled(name):
    if name not in _TILED:
        _TILED[name] = Tiled({"mono": es.tile_mono, "three_channels": es.tile_three_channels}[name](), BIG)
    return _TILED[name]


LAUNCHES = [(8193, "device"), (65535, "device"), (65536, "device"), (65600, "device"), (65536, "host")]


@pytest.mark.parametrize("n_packets,space", LAUNCHES)
@pytest.mark.parametrize("name", ["mono", "three_channels"])
def test_large_launches_decode_as_on_the_cpu(ctx, name, n_packets, space):
    """8193: entropy_zero_kernel's grid-stride loop; 65535 / 65536: the last launch of 64 lanes and the first of 256; 65600: a
    256-lane launch whose last workgroup is partial.  The three-channel stream has two submaps, so the decode buffer is
    addressed at 2 * residue_offset up to the end of a 100 MB batch; both streams carry not-decoded packets."""
    from vorbispizza_amd import capi
    from vorbispizza_amd.entropy import EntropySetup
    t = tiled(name)
    assert t.integral and len(t.packets) == BIG
    setup = EntropySetup(ctx, t.image)
    packets, spans, n_values = t.cut(n_packets)
    ms = capi.MEM_HOST if space == "host" else capi.MEM_DEVICE
    for i16 in (False, True):
        got = device_decode(ctx, setup, packets, spans, t.payload, n_values, t.channels, i16, ms)
        t.check(n_packets, i16, got, (name, n_packets, space, i16))
    setup.close()


# ------------------------------------------------------------------------------------------------ channels 64 .. 254
def writer_expectation(exps):
    posts = np.concatenate([e["posts"] for e in exps])
    counts = np.concatenate([e["post_count"] for e in exps])
    return es.expected_residue(exps), posts, counts


def assert_cpu_equals_the_writer(raw, exps, what):
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(raw)
    _, res, posts, counts = f.decode_packets()
    eres, eposts, ecounts = writer_expectation(exps)
    assert np.array_equal(counts, ecounts) and posts.tobytes() == eposts.tobytes() and res.tobytes() == eres.tobytes(), what
    f.close()


@pytest.mark.parametrize("channels", [65, 130, 255])
def test_more_than_64_channels(ctx, channels):
    """three submaps (mux c % 3; residue types 1, 0 and 2; two floors), coupling steps across every 64-channel boundary and
    silent channels at random: no-residue flags, do-not-decode masks and submap membership in every word of Mask256 (at 255
    channels a type-0/1 submap has 85 members: its mask crosses word 0 too)"""
    raw, exps = es.many_channels(channels)
    assert_cpu_equals_the_writer(raw, exps, channels)
    silent = np.concatenate([e["post_count"] for e in exps]) == 0
    assert silent.any() and not silent.all()
    assert check_stream(ctx, "%d channels" % channels, raw, both_spaces())


# ------------------------------------------------------------------------------------------------ long codes
@pytest.mark.parametrize("longest", [31, 32])
def test_codes_of_31_and_32_bits(ctx, longest):
    """Floor posts, class words and residue vectors through the overflow list (codes of 11 .. 32 bits behind a 10-bit prefix
    table), and the peek of 32 bits (an ordered book's max_bits is one more than its longest code, so both streams take it).
    With every code at most 31 bits long the CPU decode is also the writer's expectation.  A 32-bit code is a deliberate
    exception: the front end restates the reference's `(1 << length) - 1` mask, which is 0 at length 32, so such a code never
    matches there and the front end differs from the specification's writer by design -- for that book the device is compared
    with the CPU front end only."""
    raw, exps = es.long_codes(longest)
    if longest <= 31:
        assert_cpu_equals_the_writer(raw, exps, longest)
    assert check_stream(ctx, "codes of up to %d bits" % longest, raw, both_spaces())


# ------------------------------------------------------------------------------------------------ random setups
_RANDOM = {}


def random_raw(seed):
    """(container of synthetic_streams.random_stream(seed), 12 packets; its submap count), built once"""
    if seed not in _RANDOM:
        import synthetic_streams as ss
        st, rng = ss.random_stream(seed)
        _RANDOM[seed] = (bytes(st.build(rng, 12)[0]), len(st.mappings[0].submap_floor))
    return _RANDOM[seed]


@pytest.mark.parametrize("seed", range(40))
def test_random_setups_decode_as_on_the_cpu(ctx, seed):
    """random block sizes 64..4096, residue types 0 / 1 / 2 per submap (a type-2 residue inside a two-submap mapping included);
    a floor-0 setup is not eligible for the device and passes through (the next test counts)"""
    check_stream(ctx, "random_stream(%d)" % seed, random_raw(seed)[0], both_spaces())


def test_enough_random_setups_are_eligible():
    from vorbispizza_amd.front import OggVorbisFile
    eligible = [seed for seed in range(40) if OggVorbisFile(random_raw(seed)[0]).gpu_decode_supported]
    assert len(eligible) >= 25 and sum(random_raw(seed)[1] == 2 for seed in eligible) >= 10


# ------------------------------------------------------------------------------------------------ nothing else is written
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("i16", [False, True])
def test_the_call_writes_its_packets_and_nothing_else(ctx, space, i16):
    """Sentinels everywhere first.  After the call: the gaps between the streams' residues (an odd number of values), the
    residue regions of not-decoded packets and everything behind the batch still hold them; a not-decoded packet's records
    have count 0 and zero posts, as the CPU writes them; no record beyond n_packets * channels is touched."""
    import torch

    from vorbispizza_amd import capi
    from vorbispizza_amd.entropy import EntropySetup
    t = Tiled(es.tile_three_channels(), 3 * 13 + 6, pad=7)
    n, C = len(t.packets), t.channels
    extra_records, tail = 5, 11
    sent_res = np.int16(0x1234) if i16 else np.float32(12345.0)
    residue = np.full(t.n_values + tail, sent_res, dtype=np.int16 if i16 else np.float32)
    posts = np.full((n * C + extra_records, 64), 0x5A5A, dtype=np.int16)
    counts = np.full(n * C + extra_records, 0xEE, dtype=np.uint8)
    setup = EntropySetup(ctx, t.image)
    if space == "host":
        setup.decode(t.packets, t.spans, t.payload, residue, posts, counts, mem_space=capi.MEM_HOST)
    else:
        dev = torch.device("cuda", ctx.device)
        d = [torch.from_numpy(a).to(dev) for a in (t.payload, residue, posts, counts)]
        setup.decode(t.packets, t.spans, d[0], d[1], d[2], d[3], mem_space=capi.MEM_DEVICE)
        ctx.synchronize()
        residue, posts, counts = (x.cpu().numpy() for x in d[1:])
    setup.close()
    t.check(n, i16, (residue, posts, counts), (space, i16))
    written = np.zeros(residue.size, dtype=bool)
    for k in range(n):
        if t.decoded[k]:
            o = int(t.packets["residue_offset"][k])
            written[o:o + int(t.lens[k])] = True
    assert (~written).sum() >= tail + 7 * t.copies and (residue[~written] == sent_res).all()
    assert (posts[n * C:] == 0x5A5A).all() and (counts[n * C:] == 0xEE).all()
    idle = np.repeat(~t.decoded, C)
    assert idle.any() and (counts[:n * C][idle] == 0).all() and not posts[:n * C][idle].any()


# ------------------------------------------------------------------------------------------------ one setup, many calls
def test_one_setup_through_calls_that_shrink_and_grow(ctx):
    """65536 packets, then 7, then 65536 again ... on ONE vpz_entropy_setup, float32 and int16, host and device memory in turn:
    the staging buffers, the class-word cache, the decode buffer and the descriptor buffer are regrown and reused; every result
    is the CPU's, so equal to the first of its kind."""
    from vorbispizza_amd import capi
    from vorbispizza_amd.entropy import EntropySetup
    t = tiled("three_channels")
    setup = EntropySetup(ctx, t.image)
    big, small = 65536, 7
    plan = [(big, False, capi.MEM_DEVICE), (small, True, capi.MEM_HOST), (big, True, capi.MEM_HOST), (small, False, capi.MEM_DEVICE),
            (big, False, capi.MEM_HOST), (small, True, capi.MEM_DEVICE), (big, True, capi.MEM_DEVICE), (small, False, capi.MEM_HOST)]
    first = {}
    for step, (n, i16, ms) in enumerate(plan):
        packets, spans, n_values = t.cut(n)
        got = device_decode(ctx, setup, packets, spans, t.payload, n_values, t.channels, i16, ms)
        t.check(n, i16, got, (step, n, i16, ms))
        if (n, i16) in first:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first[(n, i16)])), step
        else:
            first[(n, i16)] = got
    setup.close()
