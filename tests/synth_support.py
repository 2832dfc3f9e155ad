"""The synth calls' harness: env / run / stream_major_batch / random_xlist (the host paths), the three ROUTES and same_bits over a run's
outputs, damage_audio (hostile input), the entropy decode on the device against the CPU front end (device_decode, check_stream), the
fixture streams of the entropy tests (built once per process) and the int16 conversions."""
import os
import struct
import sys

import numpy as np

import helpers
from helpers import PKT_INTERLEAVED, PKT_NO_FLOOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

ROUTES = (("dual", dict(VPZ_NO_DUAL=None, VPZ_NO_GROUP=None)), ("group", dict(VPZ_NO_DUAL=1, VPZ_NO_GROUP=None)),
          ("separate", dict(VPZ_NO_DUAL=1, VPZ_NO_GROUP=1)))


def same_bits(a, b, what=""):
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3], what
    x, y = (a[0], b[0]) if a[0].dtype == np.int16 else (a[0].view(np.uint32), b[0].view(np.uint32))
    bad = np.nonzero(x != y)[0]
    assert len(bad) == 0, "%s: %d elements differ, first at %d (%r vs %r), last at %d; totals %r" % (
        what, len(bad), bad[0], a[0][bad[0]], b[0][bad[0]], bad[-1], a[1][:6])


def cpu_decode(f, i16):
    packets, residue, posts, counts = f.decode_packets(int16=i16)
    return packets, residue, posts, counts


def device_decode(ctx, setup, packets, spans, payload, n_values, channels, i16, mem_space):
    import torch

    from vorbispizza_amd import capi
    n = len(packets)
    dt = np.int16 if i16 else np.float32
    if mem_space == capi.MEM_HOST:
        residue = np.zeros(max(1, n_values), dtype=dt)
        posts = np.full((n * channels, 64), 0x5A5A, dtype=np.int16)
        counts = np.full(n * channels, 0xEE, dtype=np.uint8)
        setup.decode(packets, spans, payload, residue, posts, counts, mem_space=mem_space)
        return residue, posts, counts
    dev = torch.device("cuda", ctx.device)
    residue = torch.zeros(max(1, n_values), dtype=torch.int16 if i16 else torch.float32, device=dev)
    posts = torch.full((n * channels, 64), 0x5A5A, dtype=torch.int16, device=dev)
    counts = torch.full((n * channels,), 0xEE, dtype=torch.uint8, device=dev)
    setup.decode(packets, spans, torch.from_numpy(payload).to(dev), residue, posts, counts, mem_space=mem_space)
    ctx.synchronize()
    return residue.cpu().numpy(), posts.cpu().numpy(), counts.cpu().numpy()


def assert_same(name, f, packets, ref, got):
    from vorbispizza_amd import capi
    _, rres, rposts, rcounts = ref
    res, posts, counts = got
    assert np.array_equal(counts, rcounts), name
    assert posts.tobytes() == rposts.tobytes(), name
    for k in range(len(packets)):
        if packets["flags"][k] & capi.PKT_NOT_DECODED:
            continue
        o = int(packets["residue_offset"][k])
        n = f.channels * ((f.block_size1 if packets["flags"][k] & capi.PKT_BLOCK_FLAG else f.block_size0) // 2)
        assert res[o:o + n].tobytes() == rres[o:o + n].tobytes(), (name, k)


def check_stream(ctx, name, raw, mem_spaces):
    from vorbispizza_amd import capi
    from vorbispizza_amd.entropy import EntropySetup
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(raw)
    if not f.gpu_decode_supported:
        f.close()
        return False
    setup = EntropySetup(ctx, f.entropy_setup())
    packets, spans, payload, n_values = f.plan_packets()
    for i16 in ([False, True] if f.residue_is_integral else [False]):
        ref = cpu_decode(f, i16)
        assert packets.tobytes() == ref[0].tobytes(), name
        for ms in mem_spaces:
            got = device_decode(ctx, setup, packets, spans, payload, n_values, f.channels, i16, ms)
            assert_same((name, i16, ms), f, packets, ref, got)
    setup.close()
    f.close()
    return True


FIXTURES = ("1test.ogg", "2test.ogg", "3test.ogg", "issue6test.ogg")
# The smallest packets at which the parse of a packet's first bits can go wrong, in place of audio packets 3 ... 9 of ten long
# blocks: nothing to read, each kind of record (type bit set, unused mode number), a header that ends inside the packet, and
# EOS on a degenerate packet.  What the front end wrote for them before the parse became one function (flags per packet,
# vpzh_decode_failures): BLOCK 1, PREV 2, NEXT 4, EOS 8, NOT_DECODED 16, INTERLEAVED 32.
HEADER_EDGE = {
    "stereo_coupled_res2": ([39, 39, 39, 32, 16, 16, 39, 39, 39, 40], (0, -1)),
    "mono_floor1_res1": ([7, 7, 7, 0, 16, 16, 7, 7, 7, 8], (1, 5)),  # (three modes: mode number 3 is unused)
    "three_channels_two_submaps": ([7, 7, 7, 0, 16, 16, 7, 7, 7, 8], (0, -1)),
}


def header_edge_stream(name):
    import synthetic_streams as ss
    import vorbis_writer as vw
    stream, rng = getattr(ss, name)()
    long_mode = next(i for i, (blockflag, _) in enumerate(stream.modes) if blockflag)
    audio = [stream.audio_packet(rng, long_mode, 1, 1)[0] for _ in range(10)]
    mode_bits = vw.ilog(len(stream.modes) - 1)
    unused = (1 << mode_bits) - 1
    audio[3] = b""
    audio[4] = b"\x01"
    audio[5] = bytes([unused << 1]) if unused >= len(stream.modes) else b"\x01\x02"
    audio[6] = audio[6][:1]
    audio[7] = audio[7][:3]
    audio[9] = b""
    granules = [0, 0, 0] + [stream.bs1 // 2 * i for i in range(10)]
    return bytes(vw.ogg_mux(stream.headers() + audio, granules, packets_per_page=2))


def streams():
    """(name, container bytes) of every stream the tests below look at"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostile_setups as hs
    import synthetic_streams as ss
    out = [(n, open(os.path.join(GOLDEN, n), "rb").read()) for n in FIXTURES]
    out += [("header edges:" + name, header_edge_stream(name)) for name in sorted(HEADER_EDGE)]
    for name, make in sorted(ss.ALL.items()):
        st, rng = make()
        ogg, _ = st.build(rng, 24)
        out.append((name, bytes(ogg)))
    for name, (raw, expect) in sorted(hs.crafted().items()):
        if expect == "pcm":
            out.append(("crafted:" + name, raw))
    return out


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def random_xlist(rng, half, count):
    return [0, half] + [int(v) for v in rng.choice(np.arange(1, half), size=count - 2, replace=False)]


def stream_major_batch(n_streams, frames, channels, seed, floor=False, interleaved=False, size0=256, size1=2048, xlists=None,
                       p_ls=0.1, p_sl=0.3, silent_prob=0.1, channel_floors=None, skew=0):
    """channel_floors: ([(x list, multiplier)] * channels of a short block, the same of a long block) -- every channel's posts are
    drawn for ITS floor (tests/channel_cases.py); skew: the first packet's residue_offset (that many floats of 777.0 lie in front of
    it in the residue array: every packet stays inside the buffer, off a multiple of four floats)."""
    from vorbispizza_amd import make_packets
    rng = np.random.default_rng(seed)
    pk = make_packets(n_streams * frames)
    res, posts, counts = ([np.full(skew, 777.0, dtype=np.float32)] if skew else []), [], []
    off, i = skew, 0
    for s in range(n_streams):
        flags = helpers.markov_block_flags(frames, seed=seed * 1000 + s, p_ls=p_ls, p_sl=p_sl, start_long=bool(s & 1))
        for f in range(frames):
            half = (size1 if flags[f] & 1 else size0) // 2
            r = (rng.standard_normal((channels, half)) * (4.0 if floor else 2.0 ** -8)).astype(np.float32)
            if floor:
                r = np.round(r)
            pk[i]["stream"] = s
            pk[i]["flags"] = flags[f] | (0 if floor else PKT_NO_FLOOR) | (PKT_INTERLEAVED if interleaved else 0)
            pk[i]["granule"] = -1
            pk[i]["residue_offset"] = off
            res.append(r.T.reshape(-1) if interleaved else r.reshape(-1))
            off += channels * half
            if floor and channel_floors is not None:
                for xl, mult in channel_floors[flags[f] & 1]:
                    p, c = helpers.random_posts(rng, xl, mult, 1, silent_prob=silent_prob)
                    posts.append(p)
                    counts.append(c)
            elif floor:
                xl = (xlists[1] if flags[f] & 1 else xlists[0]) if xlists else \
                    (helpers.LONG_XLIST if flags[f] & 1 else helpers.SHORT_XLIST)
                p, c = helpers.random_posts(rng, xl, 2, channels, silent_prob=silent_prob)
                posts.append(p)
                counts.append(c)
            i += 1
    res = np.concatenate(res)
    if floor:
        return pk, res, np.concatenate(posts), np.concatenate(counts)
    return pk, res, None, None


def run(ctx, pk, res, posts, counts, n_streams, channels, floors=(), mappings=(), layout=None, splits=1, size0=256,
        size1=2048, fill=0, device_shift=None):
    """fill: what the PCM array holds before the first call (a sentinel shows what the calls wrote); device_shift: the calls are
    device-memory ones (VPZ_MEM_DEVICE), the residue a torch tensor that starts that many floats behind its allocation's base."""
    from vorbispizza_amd import Decoder, capi
    layout = capi.OUT_PLANAR if layout is None else layout
    dec = Decoder(ctx, channels, size0, size1, floors=floors, mappings=mappings, n_streams=n_streams)
    per_stream = len(pk) // n_streams
    cap = per_stream * 1024 + 64
    s16 = layout in (capi.OUT_INTERLEAVED_S16, capi.OUT_PLANAR_S16)
    out = np.full(n_streams * channels * cap, fill, dtype=np.int16 if s16 else np.float32)
    offs = np.arange(n_streams, dtype=np.int64) * channels * cap
    if device_shift is not None:
        import torch
        dev = torch.device("cuda", 0)
        d_res = torch.cat([torch.zeros(device_shift, dtype=torch.float32), torch.from_numpy(res)]).to(dev)[device_shift:]
        d_out = torch.from_numpy(out).to(dev)
    total = np.zeros(n_streams, dtype=np.int64)
    samples = []
    # `splits` calls, each over a slice of every stream's packets (stream-major inside the call)
    idx = np.arange(len(pk)).reshape(n_streams, per_stream)
    cuts = np.linspace(0, per_stream, splits + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        sel = idx[:, a:b].reshape(-1)
        sub = pk[sel].copy()
        sub_posts = None if posts is None else np.ascontiguousarray(posts.reshape(len(pk), channels, 64)[sel].reshape(-1, 64))
        sub_counts = None if counts is None else np.ascontiguousarray(counts.reshape(len(pk), channels)[sel].reshape(-1))
        step_offs = offs + total * (channels if layout in (capi.OUT_INTERLEAVED, capi.OUT_INTERLEAVED_S16) else 1)
        if device_shift is not None:
            w = dec.synth_raw(sub, d_res, None if posts is None else torch.from_numpy(sub_posts).to(dev),
                              None if counts is None else torch.from_numpy(sub_counts).to(dev), d_out, step_offs,
                              cap - int(total.max()), layout, cap, capi.MEM_DEVICE, residue_floats=res.size)
            ctx.synchronize()
        else:
            w = dec.synth_raw(sub, res, sub_posts, sub_counts, out, step_offs, cap - int(total.max()), layout, cap, capi.MEM_HOST)
        samples.append(dec.last_packet_samples(len(sub)))
        total += w
    pos = [dec.position(s) for s in range(n_streams)]
    dec.close()
    if device_shift is not None:
        out = d_out.cpu().numpy()
    return out.copy(), total.copy(), np.concatenate(samples), pos


def _pages(raw):
    """(start, header length, body length, packets completed) of every page"""
    out, pos = [], 0
    while pos + 27 <= len(raw) and raw[pos:pos + 4] == b"OggS":
        nseg = raw[pos + 26]
        lac = raw[pos + 27: pos + 27 + nseg]
        out.append((pos, 27 + nseg, sum(lac), sum(1 for v in lac if v < 255)))
        pos += 27 + nseg + sum(lac)
    return out


def damage_audio(raw, seed, hits):
    import vorbis_writer as vw
    rng = np.random.default_rng(seed)
    pages, done, first_audio = _pages(raw), 0, None
    for i, (_, _, _, completed) in enumerate(pages):
        if done >= 3:
            first_audio = i
            break
        done += completed
    assert first_audio is not None
    data = bytearray(raw)
    touched = set()
    for _ in range(hits):
        i = int(rng.integers(first_audio, len(pages)))
        start, hdr, body, _ = pages[i]
        if body == 0:
            continue
        at = start + hdr + int(rng.integers(0, body))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            data[at] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            data[at] = int(rng.integers(0, 256))
        else:
            n = min(int(rng.integers(1, 24)), start + hdr + body - at)
            data[at:at + n] = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        touched.add(i)
    for i in touched:
        start, hdr, body, _ = pages[i]
        page = bytes(data[start:start + 22]) + b"\0\0\0\0" + bytes(data[start + 26:start + hdr + body])
        data[start + 22:start + 26] = struct.pack("<I", vw._crc(page))
    return bytes(data)


def to_s16(x):  # AssetTest.cs:131-132
    return np.clip((x.astype(np.float32) * np.float32(32768.0)).astype(np.int64), -32768, 32767).astype(np.int16)


def to_s16_wide(x):  # AssetTest.cs:131-132
    return np.clip((x.astype(np.float32) * np.float32(32768.0)).astype(np.int64), -32768, 32767)


def spec_packets(f, pk, res, posts, counts):
    out = []
    C_ = f.channels
    for i in range(len(pk)):
        flags = int(pk["flags"][i])
        if flags & helpers.PKT_NOT_DECODED:
            continue
        half = (f.block_size1 if flags & 1 else f.block_size0) // 2
        off = int(pk["residue_offset"][i])
        r = res[off: off + C_ * half]
        r = r.reshape(half, C_).T if flags & helpers.PKT_INTERLEAVED else r.reshape(C_, half)
        out.append({"flags": flags, "mapping": int(pk["mapping"][i]), "residue": r,
                    "posts": posts[i * C_:(i + 1) * C_], "post_count": counts[i * C_:(i + 1) * C_]})
    return out
