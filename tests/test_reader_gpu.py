"""The VorbisReader / StreamDecoder.Read mirror (vorbispizza_amd/host/vorbis_reader.cpp) against the
oracle, written the way the reference's own asset test is (NVorbis.Tests/AssetTest.cs:72-189): open the
file, call ReadSamples until it returns 0, compare every sample with the truth decoder.  The reference's
tolerance is +-2 LSB of s16 after `(int)(x * 32768f)`; here the truth is the CPU oracle and the bar is
BASELINE's 1e-5 float -- and 0 LSB of s16."""
import os

import numpy as np
import pytest

import helpers
from gpu_context import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_truth(oracle, path, interleave, clip=True):
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(path)
    pk, res, posts, counts = f.decode_packets()
    opk = helpers.packets_for_oracle(f, pk, res, posts, counts)
    ref, pos, clipped = helpers.oracle_decode(oracle, f.channels, f.block_size0, f.block_size1, opk,
                                              floors=f.floors, mappings=f.mappings, clip=clip, interleave=interleave)
    # per-packet sample counts of the oracle run = what each Read call may return at most
    return f, ref, clipped


def to_s16(x):  # AssetTest.cs:131-132
    return np.clip((x * np.float32(32768.0)).astype(np.int64), -32768, 32767)


@pytest.mark.parametrize("name", ["1test.ogg", "2test.ogg", "3test.ogg", "issue6test.ogg"])
@pytest.mark.parametrize("batch", [1, 7, 128])
def test_read_samples_loop_matches_truth(ctx, oracle, name, batch):
    from vorbispizza_amd import capi
    from vorbispizza_amd.front import VorbisReader
    path = os.path.join(GOLDEN, name)
    f, ref, ref_clipped = oracle_truth(oracle, path, interleave=True)
    rdr = VorbisReader(ctx, path, batch_packets=batch)
    assert (rdr.Channels, rdr.SampleRate) == (f.channels, 44100)
    buf = np.zeros(2048 * 8, dtype=np.float32)  # AssetTest.cs:98-100
    chunks, calls, thrown = [], 0, 0
    while True:
        try:
            n = rdr.ReadSamples(buf)
        except capi.SynthError as e:
            # issue6test.ogg's trailing empty packet: `OverlapBuffers` throws out of the Read that reaches it
            # (StreamDecoder.cs:777-778; the reference's harness stops before, AssetTest.cs:107-118) -- that Read fails
            # ONCE, nothing is lost, the next one goes on behind the packet
            assert e.status == capi.E_WINDOW_MISMATCH and name == "issue6test.ogg"
            thrown += 1
            continue
        if n == 0:
            break
        calls += 1
        assert n <= 1472  # never more than one packet's worth (StreamDecoder.cs:436)
        chunks.append(buf[: n * rdr.Channels].reshape(n, rdr.Channels).copy())
    got = np.concatenate(chunks)
    assert got.shape == ref.shape and thrown == (1 if name == "issue6test.ogg" else 0)
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    assert np.abs(to_s16(got) - to_s16(ref)).max() <= 1  # reference criterion is <= 2
    assert rdr.SamplePosition == ref.shape[0] and rdr.IsEndOfStream
    assert rdr.HasClipped == ref_clipped
    assert rdr.ReadSamples(buf) == 0
    # one call per packet that emitted samples
    assert calls <= f.audio_packets
    rdr.Dispose()


def test_planar_read_and_small_buffers(ctx, oracle):
    """Read(buffer, samplesToRead, channelStride) and requests smaller than a packet."""
    from vorbispizza_amd.front import VorbisReader
    path = os.path.join(GOLDEN, "3test.ogg")
    f, ref, _ = oracle_truth(oracle, path, interleave=False, clip=False)
    rdr = VorbisReader(ctx, path, clip_samples=False, batch_packets=16)
    stride = 300
    buf = np.zeros(2 * stride, dtype=np.float32)
    out = [[], []]
    while True:
        n = rdr.ReadSamples(buf, samplesToRead=257, channelStride=stride)
        if n == 0:
            break
        assert n <= 257
        out[0].append(buf[:n].copy())
        out[1].append(buf[stride:stride + n].copy())
    got = np.stack([np.concatenate(out[0]), np.concatenate(out[1])])
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    rdr.Dispose()


def test_bad_container_raises(ctx):
    from vorbispizza_amd.front import FrontError, VorbisReader
    with pytest.raises(FrontError):
        VorbisReader(ctx, b"definitely not ogg" * 8)


@pytest.mark.parametrize("name", ["1test.ogg", "3test.ogg"])
def test_seek_then_read_equals_sequential_decode(ctx, name):
    """StreamDecoder.SeekTo: after a seek the reader hands out exactly the samples a sequential decode has at
    that position (pre-roll packet + target packet, `_prevPacketStart += rollForward`), bit for bit."""
    from vorbispizza_amd.front import VorbisReader
    path = os.path.join(GOLDEN, name)
    r = VorbisReader(ctx, path, batch_packets=16)
    C_ = r.Channels
    buf = np.zeros(C_ * 4096, dtype=np.float32)
    chunks = []
    while True:
        n = r.ReadSamples(buf)
        if n == 0:
            break
        chunks.append(buf[: n * C_].reshape(n, C_).copy())
    full = np.concatenate(chunks)
    total = r.TotalSamples
    assert total == full.shape[0]
    rng = np.random.default_rng(5)
    targets = [0, 1, 127, 128, 1024, total // 2, total - 3000] + [int(v) for v in rng.integers(0, total - 3000, 12)]
    for g in targets:
        r.SeekTo(g)
        assert r.SamplePosition == g and not r.IsEndOfStream
        got = []
        while sum(len(c) for c in got) < 2500:
            n = r.ReadSamples(buf)
            assert n > 0
            got.append(buf[: n * C_].reshape(n, C_).copy())
        got = np.concatenate(got)
        assert np.array_equal(got, full[g: g + len(got)]), g
        assert r.SamplePosition == g + len(got)
    # SeekOrigin.End / Current as the reference computes them (:838, :842)
    r.SeekTo(5000, 2)
    assert r.SamplePosition == total - 5000
    r.SeekTo(1000, 1)
    assert r.SamplePosition == total - 5000 - 1000
    # outside the stream
    from vorbispizza_amd import SynthError
    with pytest.raises(SynthError):
        r.SeekTo(total + 100000)
    with pytest.raises(SynthError):
        r.SeekTo(-5)
    # seeking to the official end lands inside the last packets (the counted length exceeds the last granule).
    # What is left there depends on the position the decoder held BEFORE the seek: the reference's EOS trim
    # (StreamDecoder.cs:658-666) runs during the pre-roll with the stale _currentPosition -- mirrored, not fixed.
    r.SeekTo(total)
    assert r.SamplePosition == total
    while r.ReadSamples(buf):
        pass
    assert r.IsEndOfStream
    r.Dispose()


def test_failed_open_handle_refuses_every_entry_point(ctx):
    """vpzr_open_memory hands a handle back even when it fails (it carries the error text); channels == 0 must not
    reach the `% channels` of the read entry points (round-1 advisor finding)."""
    import ctypes as C
    from vorbispizza_amd import capi, front
    L = front.lib()
    data = np.frombuffer(b"definitely not ogg" * 8, dtype=np.uint8)
    h = C.c_void_p()
    assert L.vpzr_open_memory(ctx._h, data.ctypes.data, data.size, C.byref(h)) != 0 and h
    assert L.vpzr_last_error(h)
    buf = np.zeros(64, dtype=np.float32)
    st = C.c_int(0)
    assert L.vpzr_read_samples(h, buf.ctypes.data, buf.size, C.byref(st)) == 0 and st.value == capi.E_INVALID_ARG
    st = C.c_int(0)
    assert L.vpzr_read_samples_planar(h, buf.ctypes.data, buf.size, 8, 32, C.byref(st)) == 0
    assert st.value == capi.E_INVALID_ARG
    assert L.vpzr_seek_to(h, 0, 0) == capi.E_INVALID_ARG
    assert L.vpzr_channels(h) == 0 and L.vpzr_total_samples(h) == 0
    L.vpzr_close(h)


def test_planar_read_checks_the_last_channel_against_the_buffer(ctx):
    """`buffer.Slice(ch * channelStride + offset, count)` throws in the reference when the stride puts a channel
    outside the span (StreamDecoder.cs:594-638); here it must be an error, not a write past the buffer."""
    from vorbispizza_amd import SynthError, capi
    from vorbispizza_amd.front import VorbisReader
    rdr = VorbisReader(ctx, os.path.join(GOLDEN, "3test.ogg"), batch_packets=4)
    guard = np.full(1024, 7.0, dtype=np.float32)
    buf = guard[:512]
    with pytest.raises(SynthError) as e:
        rdr.ReadSamples(buf, samplesToRead=256, channelStride=300)   # 300 + 256 > 512
    assert e.value.status == capi.E_INVALID_ARG
    with pytest.raises(SynthError):
        rdr.ReadSamples(buf, samplesToRead=16, channelStride=-1)
    assert (guard == 7.0).all()
    assert rdr.ReadSamples(buf, samplesToRead=256, channelStride=256) > 0
    assert (guard[512:] == 7.0).all()
    rdr.Dispose()


def test_a_throwing_packet_surfaces_once_and_the_stream_goes_on(ctx, oracle):
    """An exception out of DecodeNextPacket ("Unused mode index.") costs the reference that packet only: the Read
    that reaches it throws, the next Read continues with the following packet.  The batched reader must neither get
    stuck on the batch nor lose the packets in front of the bad one (round-1 advisor finding)."""
    import synthetic_streams as ss
    import vorbis_writer as vw
    from vorbispizza_amd import SynthError
    from vorbispizza_amd.front import OggVorbisFile, VorbisReader
    stream, rng = ss.mono_floor1_res1(seed=9)
    ogg, exps = stream.build(rng, 12, packets_per_page=1)
    pages, pos = [], 0
    while pos < len(ogg):
        nseg = ogg[pos + 26]
        body = sum(ogg[pos + 27: pos + 27 + nseg])
        pages.append((pos, 27 + nseg, body))
        pos += 27 + nseg + body
    ppos, hdr, body = pages[len(pages) - 12 + 5]
    raw = bytearray(ogg)
    raw[ppos + hdr] |= 0b110  # mode index 3 of 3 modes
    raw[ppos + 22: ppos + 26] = b"\0\0\0\0"
    raw[ppos + 22: ppos + 26] = int(vw._crc(bytes(raw[ppos: ppos + hdr + body]))).to_bytes(4, "little")
    raw = bytes(raw)
    # truth: the oracle over the same packets, the bad one handed over as "not decoded" without EOS
    f = OggVorbisFile(raw)
    pk, res, posts, counts = f.decode_packets()
    assert f.decode_failures() == (1, 5)
    ref, _, _ = helpers.oracle_decode(oracle, f.channels, f.block_size0, f.block_size1,
                                      helpers.packets_for_oracle(f, pk, res, posts, counts),
                                      floors=f.floors, mappings=f.mappings, clip=True, interleave=True)
    for batch in (1, 4, 128):
        rdr = VorbisReader(ctx, raw, batch_packets=batch)
        buf = np.zeros(4096, dtype=np.float32)
        chunks, errors = [], 0
        for _ in range(64):
            try:
                n = rdr.ReadSamples(buf)
            except SynthError as e:
                errors += 1
                assert "mode" in str(e).lower()
                continue
            if n == 0:
                break
            chunks.append(buf[:n].copy())
        got = np.concatenate(chunks)
        assert errors == 1, (batch, errors)
        assert got.shape[0] == ref.shape[0] and np.abs(got - ref[:, 0]).max() <= 1e-5
        rdr.Dispose()


def _oracle_packets(path):
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(path)
    pk, res, posts, counts = f.decode_packets()
    return f, pk, helpers.packets_for_oracle(f, pk, res, posts, counts)


@pytest.mark.parametrize("name", ["1test.ogg", "3test.ogg"])
def test_seek_matches_the_restated_streamdecoder_seekto(ctx, oracle, name):
    """StreamDecoder.SeekTo restated in the oracle (orc_stream_seek_to, StreamDecoder.cs:817-880): ResetDecoder,
    _hasPosition = true, the pre-roll packet and the target packet through ReadNextPacket, `_prevPacketStart +=
    rollForward`.  The reader's seek must hand out the oracle's samples -- including a seek into the last packets,
    where the EOS trim (:658-666) runs on the position the decoder held BEFORE the seek."""
    import ctypes as C
    from vorbispizza_amd.front import VorbisReader
    path = os.path.join(GOLDEN, name)
    f, pk, opk = _oracle_packets(path)
    C_ = f.channels
    # PacketProvider's view: samples every packet adds (PacketInfo.SampleCount; the first one only primes)
    counts = []
    for i in range(len(pk)):
        fl = int(pk["flags"][i])
        info = oracle.packet_info(f.block_size0, f.block_size1, fl & 1, bool(fl & 2), bool(fl & 4))
        counts.append(0 if i == 0 else info.SampleCount)
    cum = np.cumsum(counts)
    total = min(int(cum[-1]), int(f.last_granule))
    rdr = VorbisReader(ctx, path, batch_packets=16)
    buf = np.zeros(C_ * 4096, dtype=np.float32)
    # the reader has decoded a little already: the stale position is not zero
    for _ in range(5):
        rdr.ReadSamples(buf)
    stale = rdr.SamplePosition
    ostream = helpers.OracleStream(oracle, C_, f.block_size0, f.block_size1, f.floors, f.mappings, clip=True, interleave=True)
    for i in range(len(pk)):        # bring the oracle's decoder to the same place (same stale _currentPosition)
        if ostream.position >= stale:
            break
        ostream.feed(opk[i])
    assert ostream.position == stale
    rng = np.random.default_rng(7)
    targets = [total - 1500, total - 200, 5000, total // 3] + [int(v) for v in rng.integers(1, total - 1, 6)]
    for g in targets:
        k = int(np.searchsorted(cum, g, side="right"))    # first packet whose span holds the position
        k = min(k, len(pk) - 1)
        provider_pos = int(cum[k - 1])
        feed = iter(range(k - 1, len(pk)))
        readable = []

        def read_next_packet(_user):
            return ostream.read_next_packet(opk[next(feed)])

        cb = oracle.READ_NEXT_PACKET_FN(read_next_packet)
        ostream.eos_seen = False
        rc = oracle.lib().orc_stream_seek_to(ostream.st, g, provider_pos, int(cum[-1]), cb, None)
        assert rc == 0
        first = ostream.take()
        if first is not None:
            readable.append(first)
        for i in feed:
            got = ostream.feed(opk[i])
            if got is not None:
                readable.append(got)
            if sum(c.shape[1] for c in readable) >= 3000:
                break
        want = np.concatenate(readable, axis=1).T if readable else np.zeros((0, C_), np.float32)
        want_pos = ostream.position
        # the library
        rdr.SeekTo(g)
        assert rdr.SamplePosition == g
        chunks = []
        while sum(len(c) for c in chunks) < len(want):
            n = rdr.ReadSamples(buf)
            if n == 0:
                break
            chunks.append(buf[: n * C_].reshape(n, C_).copy())
        got = np.concatenate(chunks) if chunks else np.zeros((0, C_), np.float32)
        assert got.shape == want.shape, (g, got.shape, want.shape)
        if len(want):
            assert np.abs(got - want).max() <= 1e-5 * max(1.0, float(np.abs(want).max())), g
        assert rdr.SamplePosition == want_pos, (g, rdr.SamplePosition, want_pos)
    ostream.close()
    rdr.Dispose()


def test_position_is_picked_up_again_after_a_resync(ctx, oracle, tmp_path):
    """A dropped page: the front end flags the next packet VPZ_PKT_RESYNC, `_hasPosition` goes false and the position
    comes from the next packet that carries a granule (StreamDecoder.cs:459-463, 718-722)."""
    from vorbispizza_amd import capi
    from vorbispizza_amd.front import OggVorbisFile, VorbisReader
    ogg = bytearray(open(os.path.join(GOLDEN, "3test.ogg"), "rb").read())
    pages, pos = [], 0
    while pos < len(ogg):
        nseg = ogg[pos + 26]
        body = sum(ogg[pos + 27: pos + 27 + nseg])
        pages.append((pos, 27 + nseg + body))
        pos += 27 + nseg + body
    p0, ln = pages[len(pages) // 2]
    ogg[p0 + ln - 1] ^= 0x55
    ogg = bytes(ogg)
    f = OggVorbisFile(ogg)
    pk, res, posts, counts = f.decode_packets()
    assert (pk["flags"] & capi.PKT_RESYNC).any() and f.info.bad_crc_pages >= 1
    ref, ref_pos, _ = helpers.oracle_decode(oracle, f.channels, f.block_size0, f.block_size1,
                                            helpers.packets_for_oracle(f, pk, res, posts, counts), floors=f.floors,
                                            mappings=f.mappings, clip=True, interleave=True)
    for batch in (3, 128):
        rdr = VorbisReader(ctx, ogg, batch_packets=batch)
        buf = np.zeros(2 * 4096, dtype=np.float32)
        chunks = []
        while True:
            n = rdr.ReadSamples(buf)
            if n == 0:
                break
            chunks.append(buf[: 2 * n].reshape(n, 2).copy())
        got = np.concatenate(chunks)
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max()))
        rdr.Dispose()
    # the decoder's own position (the reader counts handed-out samples; the decoder re-bases on the granule)
    from vorbispizza_amd import Decoder
    dec = Decoder(ctx, f.channels, f.block_size0, f.block_size1, floors=f.floors, mappings=f.mappings, clip_samples=True)
    dec.synth(pk, res, posts, counts)
    assert dec.position(0) == ref_pos and ref_pos != ref.shape[0]   # samples were lost: position != count
    dec.close()


def test_chained_file_is_read_stream_by_stream(ctx, oracle):
    """VorbisReader.FindNextStream / SwitchStreams (VorbisReader.cs:191-217) over a chain 3test | 1test | 3test."""
    from vorbispizza_amd import SynthError
    from vorbispizza_amd.front import VorbisReader
    a = open(os.path.join(GOLDEN, "3test.ogg"), "rb").read()
    b = open(os.path.join(GOLDEN, "1test.ogg"), "rb").read()
    want = {}
    for key, data in (("a", a), ("b", b)):
        r = VorbisReader(ctx, data)
        buf = np.zeros(r.Channels * 4096, dtype=np.float32)
        chunks = []
        while True:
            n = r.ReadSamples(buf)
            if n == 0:
                break
            chunks.append(buf[: n * r.Channels].reshape(n, r.Channels).copy())
        want[key] = np.concatenate(chunks)
        r.Dispose()
    rdr = VorbisReader(ctx, a + b + a)
    assert rdr.StreamCount == 1 and rdr.Channels == 2
    outs = []
    index = 0
    while True:
        buf = np.zeros(rdr.Channels * 4096, dtype=np.float32)
        chunks = []
        while True:
            n = rdr.ReadSamples(buf)
            if n == 0:
                break
            chunks.append(buf[: n * rdr.Channels].reshape(n, rdr.Channels).copy())
        outs.append(np.concatenate(chunks))
        if not rdr.FindNextStream():
            break
        index += 1
        changed = rdr.SwitchStreams(index)
        assert changed == (index in (1, 2))          # stereo -> mono -> stereo
    assert rdr.StreamCount == 3 and len(outs) == 3
    for got, key in zip(outs, "aba"):
        assert got.shape == want[key].shape and np.array_equal(got, want[key])
    # streams keep their own position; switching back does not rewind
    assert rdr.SwitchStreams(0) is False           # 3test -> 3test: same channels and rate
    assert rdr.IsEndOfStream and rdr.SamplePosition == len(want["a"])
    assert rdr.SwitchStreams(1) is True and rdr.Channels == 1 and rdr.SwitchStreams(0) is True
    rdr.SeekTo(1000)
    assert rdr.SamplePosition == 1000
    with pytest.raises(SynthError):
        rdr.SwitchStreams(7)
    rdr.Dispose()


@pytest.mark.parametrize("name", ["stereo_floor0", "six_channels_51", "three_channels_two_submaps", "ten_channels",
                                  "mono_floor1_res1", "five_channels", "four_channels_quad"])
def test_seek_in_streams_of_other_shapes(ctx, name):
    """the same property on the spec-based writer's streams: type-0 floors, 5.1, two submaps, ten channels (the
    separate coupling pass), odd channel counts -- every route the reader can end up on seeks like the stereo fast path"""
    import synthetic_streams as ss
    from vorbispizza_amd.front import VorbisReader
    stream, rng = ss.ALL[name]()
    ogg, _ = stream.build(rng, 60)
    r = VorbisReader(ctx, bytes(ogg), batch_packets=9)
    C_ = r.Channels
    buf = np.zeros(C_ * 4096, dtype=np.float32)
    chunks = []
    while True:
        n = r.ReadSamples(buf)
        if n == 0:
            break
        chunks.append(buf[: n * C_].reshape(n, C_).copy())
    full = np.concatenate(chunks)
    total = r.TotalSamples
    assert total == full.shape[0] and total > 2000
    rs = np.random.default_rng(9)
    for g in [0, 1, total // 2, total - 700] + [int(v) for v in rs.integers(0, total - 700, 10)]:
        r.SeekTo(g)
        assert r.SamplePosition == g
        got = []
        while sum(len(c) for c in got) < 600:
            n = r.ReadSamples(buf)
            assert n > 0
            got.append(buf[: n * C_].reshape(n, C_).copy())
        got = np.concatenate(got)
        assert np.array_equal(got.view(np.uint32), full[g: g + len(got)].view(np.uint32)), g
    r.Dispose()


@pytest.mark.parametrize("n_packets", [1, 2, 3, 5])
def test_streams_of_one_two_three_packets(ctx, n_packets):
    """the first packet only primes the overlap (StreamDecoder.cs:679): a one-packet stream is zero samples long, and the
    reader says so instead of waiting for more"""
    import synthetic_streams as ss
    from vorbispizza_amd import Decoder, capi
    from vorbispizza_amd.front import OggVorbisFile, VorbisReader
    stream, rng = ss.ALL["stereo_coupled_res2"]()
    ogg, _ = stream.build(rng, n_packets)
    raw = bytes(ogg)
    f = OggVorbisFile(raw)
    pk, res, posts, counts = f.decode_packets()
    dec = Decoder(ctx, f.channels, f.block_size0, f.block_size1, floors=f.floors, mappings=f.mappings)
    ref = dec.synth(pk, res, posts, counts, out_layout=capi.OUT_INTERLEAVED)[0]
    dec.close()
    r = VorbisReader(ctx, raw, clip_samples=False, batch_packets=2)
    assert r.TotalSamples == ref.shape[0] == int(f.total_samples)
    buf = np.zeros(2 * 4096, dtype=np.float32)
    chunks = []
    while True:
        n = r.ReadSamples(buf)
        if n == 0:
            break
        chunks.append(buf[: n * 2].reshape(n, 2).copy())
    got = np.concatenate(chunks) if chunks else np.zeros((0, 2), dtype=np.float32)
    assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert r.IsEndOfStream and r.SamplePosition == ref.shape[0] and r.ReadSamples(buf) == 0
    if ref.shape[0] > 0:
        r.SeekTo(0)
        assert r.ReadSamples(buf) > 0
    r.Dispose()
