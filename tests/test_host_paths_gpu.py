"""The alternative routes through vpz_decoder_synth give the same bits:

* the host state machine split over the host cores (run_state_machine_parallel, large plain batches) against the
  serial one (StreamDecoder.ReadNextPacket restated packet by packet) -- descriptors, sample counts, positions;
* the fused group mode of the synthesis kernel (Residue2 de-interleave + inverse coupling in LDS) against the
  separate coupling pass through a planar temp (VPZ_NO_GROUP=1);
and batches the parallel pass must refuse (EOS, undecodable packets, unknown position, unsorted streams) still come
out right through the serial fallback."""
import os

import numpy as np
import pytest

import helpers
from helpers import PKT_BLOCK_FLAG, PKT_EOS, PKT_INTERLEAVED, PKT_NEXT_FLAG, PKT_NO_FLOOR, PKT_NOT_DECODED, PKT_PREV_FLAG
from synth_support import env, random_xlist, run, stream_major_batch  # noqa: E402
from gpu_context import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("channels,n_streams,frames", [(2, 1, 700), (2, 37, 40), (1, 5, 333), (3, 16, 64)])
def test_parallel_state_machine_equals_the_serial_one(ctx, channels, n_streams, frames):
    pk, res, _, _ = stream_major_batch(n_streams, frames, channels, seed=channels * 100 + n_streams)
    with env(VPZ_PAR_MIN_PACKETS=1 << 40):
        serial = run(ctx, pk, res, None, None, n_streams, channels, splits=3)
    for threads in (2, 5, 16):
        with env(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=threads):
            par = run(ctx, pk, res, None, None, n_streams, channels, splits=3)
        assert np.array_equal(par[1], serial[1]) and np.array_equal(par[2], serial[2]) and par[3] == serial[3]
        assert np.array_equal(par[0].view(np.uint32), serial[0].view(np.uint32)), threads


def test_parallel_pass_with_floor_and_interleaved_coupled_input(ctx, oracle):
    channels, n_streams, frames = 2, 9, 50
    floors = [(helpers.SHORT_XLIST, 2), (helpers.LONG_XLIST, 2)]
    pk, res, posts, counts = stream_major_batch(n_streams, frames, channels, seed=77, floor=True, interleaved=True)
    pk["mapping"] = pk["flags"] & 1   # mapping 0: short blocks / floor 0, mapping 1: long blocks / floor 1
    mappings = [{"coupling": [(0, 1)], "channel_floor": [0, 0]}, {"coupling": [(0, 1)], "channel_floor": [1, 1]}]
    from vorbispizza_amd import capi
    with env(VPZ_PAR_MIN_PACKETS=1 << 40):
        serial = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=capi.OUT_INTERLEAVED)
    with env(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=7):
        par = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=capi.OUT_INTERLEAVED)
    assert np.array_equal(par[1], serial[1]) and np.array_equal(par[2], serial[2]) and par[3] == serial[3]
    assert np.array_equal(par[0].view(np.uint32), serial[0].view(np.uint32))
    # ... and the oracle agrees with both (stream 4)
    s = 4
    per = frames
    opk = []
    for i in range(s * per, (s + 1) * per):
        half = 1024 if pk["flags"][i] & 1 else 128
        off = int(pk["residue_offset"][i])
        opk.append({"flags": int(pk["flags"][i]), "granule": -1, "mapping": int(pk["mapping"][i]),
                    "residue": res[off: off + channels * half], "posts": posts[i * channels:(i + 1) * channels],
                    "post_count": counts[i * channels:(i + 1) * channels]})
    ref, pos, _ = helpers.oracle_decode(oracle, channels, 256, 2048, opk, floors=floors, mappings=mappings, interleave=True)
    cap = per * 1024 + 64
    got = par[0][s * channels * cap: s * channels * cap + ref.size].reshape(ref.shape)
    assert ref.shape[0] == par[1][s] and np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


def test_batches_the_parallel_pass_must_refuse_take_the_serial_route(ctx, oracle):
    """EOS with a trimming granule, an undecodable packet, a stream whose position is unknown (after a reset), and
    streams interleaved packet by packet: the parallel pass is asked (threshold 1) and has to decline."""
    from vorbispizza_amd import Decoder, capi, make_packets
    frames, channels = 60, 2
    flags = helpers.markov_block_flags(frames, seed=5)
    spec = helpers.gaussian_spectra((frames, channels, 1024), seed=6)
    variants = {"eos": (frames - 1, PKT_EOS, 40000), "undecodable": (20, PKT_NOT_DECODED, -1)}
    for name, (at, flag, gran) in variants.items():
        pk = make_packets(frames)
        opk, chunks, off = [], [], 0
        for f in range(frames):
            half = 1024 if flags[f] & 1 else 128
            fl = int(flags[f]) | PKT_NO_FLOOR | (flag if f == at else 0)
            pk[f]["flags"], pk[f]["granule"], pk[f]["residue_offset"] = fl, (gran if f == at else -1), off
            x = spec[f, :, :half].reshape(-1)
            chunks.append(x)
            off += x.size
            opk.append({"flags": fl, "granule": gran if f == at else -1, "residue": x})
        res = np.concatenate(chunks)
        with env(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4):
            dec = Decoder(ctx, channels, 256, 2048)
            got = dec.synth(pk, res)[0]
            pos = dec.position(0)
            dec.close()
        ref, rpos, _ = helpers.oracle_decode(oracle, channels, 256, 2048, opk)
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-5 and pos == rpos, name
    # unknown position: reset, then a batch with a granule on its third packet
    pk = make_packets(frames)
    pk["flags"] = flags | PKT_NO_FLOOR
    pk["granule"] = -1
    pk["granule"][2] = 5000
    halves = np.where(flags & 1, 1024, 128)
    pk["residue_offset"] = np.concatenate([[0], np.cumsum(halves * channels)[:-1]])
    res = np.concatenate([spec[f, :, :halves[f]].reshape(-1) for f in range(frames)])
    with env(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4):
        dec = Decoder(ctx, channels, 256, 2048)
        dec.reset(0)
        got = dec.synth(pk, res)[0]
        pos_par = dec.position(0)
        dec.close()
    with env(VPZ_PAR_MIN_PACKETS=1 << 40):
        dec = Decoder(ctx, channels, 256, 2048)
        dec.reset(0)
        want = dec.synth(pk, res)[0]
        pos_ser = dec.position(0)
        dec.close()
    assert np.array_equal(got, want) and pos_par == pos_ser and pos_par != got.shape[1]
    # round-robin interleaved streams (not stream-major)
    pk2 = make_packets(2 * frames)
    pk2[0::2] = pk
    pk2[1::2] = pk
    pk2["granule"] = -1
    pk2["stream"][1::2] = 1
    with env(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4):
        dec = Decoder(ctx, channels, 256, 2048, n_streams=2)
        a = dec.synth(pk2, res)
        dec.close()
    assert np.array_equal(a[0], a[1]) and a[0].shape[1] > 0


@pytest.mark.parametrize("channels,steps", [(2, [(0, 1)]), (3, [(0, 1), (2, 0)]), (6, [(0, 1), (2, 3)]), (8, [(7, 0), (1, 6), (0, 1)]),
                                            (4, []), (6, [(0, 2), (3, 4)]), (4, [(3, 0)])])
@pytest.mark.parametrize("interleaved", [True, False])
def test_group_mode_equals_the_separate_coupling_pass(ctx, oracle, channels, steps, interleaved):
    from vorbispizza_amd import capi
    if not steps and not interleaved:
        pytest.skip("nothing to stage")
    n_streams, frames = 3, 30
    floors = [(helpers.SHORT_XLIST, 2), (helpers.LONG_XLIST, 2)]
    pk, res, posts, counts = stream_major_batch(n_streams, frames, channels, seed=channels, floor=True, interleaved=interleaved)
    pk["mapping"] = pk["flags"] & 1
    mappings = [{"coupling": steps, "channel_floor": [0] * channels}, {"coupling": steps, "channel_floor": [1] * channels}]
    outs = {}
    for layout in (capi.OUT_PLANAR, capi.OUT_INTERLEAVED):
        # (VPZ_NO_PAIRS: channel counts and steps the pair route would take -- tests/test_pairs_gpu.py -- stay with group mode here)
        with env(VPZ_NO_GROUP=None, VPZ_NO_PAIRS=1):
            g = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2)
        with env(VPZ_NO_GROUP=1, VPZ_NO_PAIRS=1):
            l = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2)
        assert np.array_equal(g[1], l[1]) and np.array_equal(g[2], l[2])
        assert np.array_equal(g[0].view(np.uint32), l[0].view(np.uint32)), (channels, layout)
        with env(VPZ_NO_GROUP=None, VPZ_NO_PAIRS=None):  # ... and whatever route the decoder picks by itself
            dflt = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2)
        assert np.array_equal(dflt[1], g[1]) and np.array_equal(dflt[0].view(np.uint32), g[0].view(np.uint32)), (channels, layout)
        # ... and group mode where the stereo fast path would otherwise take the batch (two channels)
        with env(VPZ_NO_GROUP=None, VPZ_NO_DUAL=1):
            d = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2)
        assert np.array_equal(d[1], g[1]) and np.array_equal(d[0].view(np.uint32), g[0].view(np.uint32)), (channels, layout)
        outs[layout] = g
    # the oracle, stream 1, planar
    s, per = 1, frames
    opk = []
    for i in range(s * per, (s + 1) * per):
        half = 1024 if pk["flags"][i] & 1 else 128
        off = int(pk["residue_offset"][i])
        opk.append({"flags": int(pk["flags"][i]), "granule": -1, "mapping": int(pk["mapping"][i]),
                    "residue": res[off: off + channels * half], "posts": posts[i * channels:(i + 1) * channels],
                    "post_count": counts[i * channels:(i + 1) * channels]})
    ref, _, _ = helpers.oracle_decode(oracle, channels, 256, 2048, opk, floors=floors, mappings=mappings)
    cap = per * 1024 + 64
    got = outs[capi.OUT_PLANAR][0][s * channels * cap:(s + 1) * channels * cap].reshape(channels, cap)[:, :ref.shape[1]]
    assert outs[capi.OUT_PLANAR][1][s] == ref.shape[1]
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name", ["1test.ogg", "3test.ogg", "issue6test.ogg"])
def test_real_streams_take_the_parallel_pass_and_match_the_serial_one(ctx, name):
    """Real files end with an EOS packet whose granule trims the last block, carry granule positions on every
    page-final packet, start from an unknown position after a reset, and issue6test.ogg ends in a packet the
    reference's OverlapBuffers throws on: the per-stream finalisation of the parallel pass covers all of it."""
    from vorbispizza_amd import Decoder, SynthError, capi
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    pk, res, posts, counts = f.decode_packets()
    copies, n = 5, len(pk)
    pk_all = np.tile(pk, copies)
    pk_all["stream"] = np.repeat(np.arange(copies, dtype=np.int32), n)
    posts_all, counts_all = np.tile(posts, (copies, 1)), np.tile(counts, copies)
    cap = int(f.last_granule) + 4096
    results = {}
    for mode, kv in (("serial", dict(VPZ_PAR_MIN_PACKETS=1 << 40)), ("parallel", dict(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=6))):
        with env(**kv):
            dec = Decoder(ctx, f.channels, f.block_size0, f.block_size1, floors=f.floors, mappings=f.mappings, n_streams=copies)
            for reset_first in (False, True):   # known position 0, then unknown (granule pick-up)
                if reset_first:
                    dec.reset(-1)
                out = np.zeros(copies * cap * f.channels, dtype=np.float32)
                offs = np.arange(copies, dtype=np.int64) * cap * f.channels
                status = 0
                try:
                    w = dec.synth_raw(pk_all, res, posts_all, counts_all, out, offs, cap, capi.OUT_INTERLEAVED, 0, capi.MEM_HOST)
                except SynthError as e:
                    status = e.status
                    assert status == capi.E_WINDOW_MISMATCH
                    w = np.array([int(dec.last_packet_samples(len(pk_all))[s * n:(s + 1) * n].sum()) for s in range(copies)])
                results[(mode, reset_first)] = (out, np.array(w), dec.last_packet_samples(len(pk_all)),
                                                [dec.position(s) for s in range(copies)], status)
            dec.close()
    for reset_first in (False, True):
        a, b = results[("serial", reset_first)], results[("parallel", reset_first)]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4], reset_first
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        # (after a reset the EOS trim runs on the stale position, StreamDecoder.cs:658-666; issue6test.ogg loses its
        # last packet to the window check and never reaches its last granule)
        if not reset_first and name != "issue6test.ogg":
            assert (a[1] == f.last_granule).all() and a[3] == [f.last_granule] * copies
        assert a[4] == (capi.E_WINDOW_MISMATCH if name == "issue6test.ogg" else 0)


@pytest.mark.parametrize("seed", range(10))
def test_random_multi_stream_batches_parallel_compact_vs_serial(ctx, seed):
    """Randomised differential run of the three host routes -- serial; parallel with explicit descriptors
    (VPZ_NO_COMPACT=1); parallel with compact runs -- over the cases the parallel pass settles per stream: EOS on a stream's
    last packet with and without a trimming granule, granules anywhere (position pick-up after a reset), a window
    mismatch on the last packet, several calls with resets in between, 1-3 channels, floors on or off."""
    from vorbispizza_amd import Decoder, SynthError, capi, make_packets
    rng = np.random.default_rng(9000 + seed)
    channels = int(rng.integers(1, 4))
    n_streams = int(rng.integers(1, 7))
    use_floor = bool(rng.integers(0, 2))
    floors = [(helpers.SHORT_XLIST, 2), (helpers.LONG_XLIST, 2)] if use_floor else []
    steps = [(0, 1)] if (use_floor and channels >= 2 and rng.random() < 0.7) else []
    mappings = [{"coupling": steps, "channel_floor": [0] * channels}, {"coupling": steps, "channel_floor": [1] * channels}] \
        if use_floor else []
    calls = []
    for _ in range(int(rng.integers(2, 5))):
        pks, res_parts, posts_parts, counts_parts = [], [], [], []
        off = 0
        for s in range(n_streams):
            frames = int(rng.integers(1, 40))
            flags = helpers.markov_block_flags(frames, seed=int(rng.integers(1 << 30)), start_long=bool(rng.integers(0, 2)))
            if rng.random() < 0.3:                      # contradict the window of the last packet: it gets skipped
                flags[-1] = PKT_BLOCK_FLAG | PKT_NEXT_FLAG if not (flags[-1] & PKT_BLOCK_FLAG) else PKT_BLOCK_FLAG
            gran = np.full(frames, -1, dtype=np.int64)
            gran[rng.random(frames) < 0.2] = rng.integers(0, 40000)
            eos = rng.random() < 0.5
            if eos and rng.random() < 0.7:
                gran[-1] = int(rng.integers(0, 30000))
            for f in range(frames):
                half = 1024 if flags[f] & 1 else 128
                pk = np.zeros(1, dtype=capi.PACKET_DTYPE)
                pk["stream"], pk["granule"], pk["residue_offset"] = s, gran[f], off
                pk["flags"] = int(flags[f]) | (0 if use_floor else PKT_NO_FLOOR) | (PKT_EOS if eos and f == frames - 1 else 0)
                pk["mapping"] = int(flags[f] & 1) if use_floor else 0
                x = rng.standard_normal(channels * half).astype(np.float32) * (3.0 if use_floor else 2.0 ** -8)
                res_parts.append(np.round(x) if use_floor else x)
                off += channels * half
                pks.append(pk)
                if use_floor:
                    p, c = helpers.random_posts(rng, helpers.LONG_XLIST if flags[f] & 1 else helpers.SHORT_XLIST, 2, channels, 0.15)
                    posts_parts.append(p)
                    counts_parts.append(c)
        calls.append((np.concatenate(pks), np.concatenate(res_parts),
                      np.concatenate(posts_parts) if use_floor else None, np.concatenate(counts_parts) if use_floor else None,
                      [s for s in range(n_streams) if rng.random() < 0.3]))
    results = []
    for kv in (dict(VPZ_PAR_MIN_PACKETS=1 << 40), dict(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=3, VPZ_NO_COMPACT=1),
               dict(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=5, VPZ_NO_COMPACT=None)):
        with env(**kv):
            dec = Decoder(ctx, channels, 256, 2048, floors=floors, mappings=mappings, n_streams=n_streams, clip_samples=True)
            trace = []
            for pk, res, posts, counts, resets in calls:
                cap = len(pk) * 1472 + 64
                out = np.zeros(n_streams * channels * cap, dtype=np.float32)
                offs = np.arange(n_streams, dtype=np.int64) * channels * cap
                status = 0
                try:
                    w = dec.synth_raw(pk, res, posts, counts, out, offs, cap, capi.OUT_INTERLEAVED, 0, capi.MEM_HOST)
                except SynthError as e:
                    assert e.status == capi.E_WINDOW_MISMATCH
                    status, w = e.status, None
                trace.append((out, None if w is None else w.copy(), dec.last_packet_samples(len(pk)), status,
                              [dec.position(s) for s in range(n_streams)], [dec.has_clipped(s) for s in range(n_streams)]))
                for s in resets:
                    dec.reset(s)
            dec.close()
        results.append(trace)
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert a[3] == b[3] and a[4] == b[4] and a[5] == b[5]
            assert np.array_equal(a[2], b[2])
            assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.parametrize("size0,size1", [(512, 1024), (256, 1024), (1024, 2048), (512, 512)])
@pytest.mark.parametrize("channels,steps", [(2, [(0, 1)]), (5, [(0, 1), (3, 1), (2, 4)])])
def test_group_mode_with_the_other_block_sizes_and_16_bit_output(ctx, oracle, size0, size1, channels, steps):
    """The general-size instantiations of the fused kernel in group mode (512 / 1024 blocks are what speech-rate and
    low-bitrate streams use), float and 16-bit output, compact runs: bit-equal to the separate coupling pass, and
    within tolerance of the oracle."""
    from vorbispizza_amd import capi
    rng = np.random.default_rng(size0 + size1 + channels)
    xlists = [random_xlist(rng, size0 // 2, 12), random_xlist(rng, size1 // 2, 25)]
    if size0 == size1:
        xlists[1] = xlists[0]             # one block size: every frame uses mapping 0 and its floor
    floors = [(xlists[0], 2), (xlists[1], 2)]
    n_streams, frames = 4, 24
    pk, res, posts, counts = stream_major_batch(n_streams, frames, channels, seed=size0 + channels, floor=True, interleaved=True,
                                                size0=size0, size1=size1, xlists=xlists)
    if size0 == size1:
        pk["flags"] &= ~np.uint8(7)       # equal block sizes: every block is a "short" one
    pk["mapping"] = pk["flags"] & 1
    mappings = [{"coupling": steps, "channel_floor": [0] * channels}, {"coupling": steps, "channel_floor": [1] * channels}]
    outs = {}
    for layout in (capi.OUT_PLANAR, capi.OUT_INTERLEAVED, capi.OUT_INTERLEAVED_S16):
        with env(VPZ_NO_GROUP=None, VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4):
            g = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2, size0=size0,
                    size1=size1)
        with env(VPZ_NO_GROUP=1, VPZ_PAR_MIN_PACKETS=1 << 40):
            l = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2, size0=size0,
                    size1=size1)
        assert np.array_equal(g[1], l[1]) and np.array_equal(g[2], l[2]) and g[3] == l[3]
        assert np.array_equal(g[0], l[0]) if g[0].dtype == np.int16 else np.array_equal(g[0].view(np.uint32), l[0].view(np.uint32))
        outs[layout] = g
    s, per = 2, frames
    opk = []
    for i in range(s * per, (s + 1) * per):
        half = (size1 if pk["flags"][i] & 1 else size0) // 2
        off = int(pk["residue_offset"][i])
        opk.append({"flags": int(pk["flags"][i]), "granule": -1, "mapping": int(pk["mapping"][i]),
                    "residue": res[off: off + channels * half], "posts": posts[i * channels:(i + 1) * channels],
                    "post_count": counts[i * channels:(i + 1) * channels]})
    ref, _, _ = helpers.oracle_decode(oracle, channels, size0, size1, opk, floors=floors, mappings=mappings)
    cap = per * 1024 + 64
    got = outs[capi.OUT_PLANAR][0][s * channels * cap:(s + 1) * channels * cap].reshape(channels, cap)[:, :ref.shape[1]]
    assert outs[capi.OUT_PLANAR][1][s] == ref.shape[1] and ref.shape[1] > 0
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    # the 16-bit samples are the reference conversion of the float ones
    f32 = outs[capi.OUT_INTERLEAVED][0][s * channels * cap: s * channels * cap + ref.size]
    s16 = outs[capi.OUT_INTERLEAVED_S16][0][s * channels * cap: s * channels * cap + ref.size]
    want = np.clip((f32 * np.float32(32768.0)).astype(np.int64), -32768, 32767).astype(np.int16)
    assert np.array_equal(s16, want)


@pytest.mark.parametrize("channels,steps,interleaved_in", [(6, [(0, 1), (2, 3)], True), (5, [], False), (3, [(0, 2)], False)])
def test_interleaved_output_of_many_channels_written_by_the_group(ctx, channels, steps, interleaved_in):
    """`ReadSamples(Span<float>)` of a 5.1 stream: in group mode the waves of a packet write its [samples][channels] block
    together as dense pieces (long block after long block; every other frame geometry scatters as before) -- and a
    batch takes group mode for that alone, coupled or not.  Float and 16-bit, against the run that never groups."""
    from vorbispizza_amd import capi
    n_streams, frames = 3, 40
    pk, res, posts, counts = stream_major_batch(n_streams, frames, channels, seed=900 + channels, floor=True,
                                                interleaved=interleaved_in)
    pk["mapping"] = pk["flags"] & 1
    floors = [(helpers.SHORT_XLIST, 2), (helpers.LONG_XLIST, 2)]
    mappings = [{"coupling": steps, "channel_floor": [0] * channels}, {"coupling": steps, "channel_floor": [1] * channels}]
    assert int((pk["flags"] & 1).sum()) > len(pk) // 2, "the batch must hold runs of long blocks"
    for layout in (capi.OUT_INTERLEAVED, capi.OUT_INTERLEAVED_S16, capi.OUT_PLANAR):
        with env(VPZ_NO_GROUP=None):
            g = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2)
        with env(VPZ_NO_GROUP=1):
            l = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2)
        assert np.array_equal(g[1], l[1]) and np.array_equal(g[2], l[2]) and g[3] == l[3]
        assert np.array_equal(g[0], l[0]) if g[0].dtype == np.int16 else np.array_equal(g[0].view(np.uint32), l[0].view(np.uint32))
        assert np.abs(g[0].astype(np.float64)).max() > 0


@pytest.mark.parametrize("channels,steps,p_sl", [(2, [(0, 1)], 0.08), (2, [(0, 1)], 0.5), (6, [(0, 1), (2, 3)], 0.1), (3, [], 0.15)])
def test_batches_of_short_blocks(ctx, oracle, channels, steps, p_sl):
    """Group mode synthesises up to eight consecutive short blocks of a run in one pass (and the host cuts runs by cost):
    streams with long streaks of short blocks (p_sl small: streaks of a dozen and more, cut into batches of eight and a
    rest), silent channels inside the streaks, every output layout -- against the run that never groups (one block per
    pass), bit for bit, and against the oracle."""
    from vorbispizza_amd import capi
    n_streams, frames = 24, 90     # (24 streams: the host splits the run cutting over its pool)
    pk, res, posts, counts = stream_major_batch(n_streams, frames, channels, seed=4000 + channels, floor=True, interleaved=True,
                                                p_ls=0.25, p_sl=p_sl, silent_prob=0.15)
    pk["mapping"] = pk["flags"] & 1
    short = (pk["flags"] & 1) == 0
    assert short.sum() > len(pk) // 3
    floors = [(helpers.SHORT_XLIST, 2), (helpers.LONG_XLIST, 2)]
    mappings = [{"coupling": steps, "channel_floor": [0] * channels}, {"coupling": steps, "channel_floor": [1] * channels}]
    outs = {}
    for layout in (capi.OUT_PLANAR, capi.OUT_INTERLEAVED, capi.OUT_INTERLEAVED_S16, capi.OUT_PLANAR_S16):
        with env(VPZ_NO_GROUP=None, VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4):
            g = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2)
        with env(VPZ_NO_GROUP=1, VPZ_PAR_MIN_PACKETS=1 << 40):
            l = run(ctx, pk, res, posts, counts, n_streams, channels, floors, mappings, layout=layout, splits=2)
        assert np.array_equal(g[1], l[1]) and np.array_equal(g[2], l[2]) and g[3] == l[3]
        assert np.array_equal(g[0], l[0]) if g[0].dtype == np.int16 else np.array_equal(g[0].view(np.uint32), l[0].view(np.uint32))
        outs[layout] = g
    s_, per = 5, frames
    opk = []
    for i in range(s_ * per, (s_ + 1) * per):
        half = 1024 if pk["flags"][i] & 1 else 128
        off = int(pk["residue_offset"][i])
        opk.append({"flags": int(pk["flags"][i]), "granule": -1, "mapping": int(pk["mapping"][i]),
                    "residue": res[off: off + channels * half], "posts": posts[i * channels:(i + 1) * channels],
                    "post_count": counts[i * channels:(i + 1) * channels]})
    ref, _, _ = helpers.oracle_decode(oracle, channels, 256, 2048, opk, floors=floors, mappings=mappings)
    cap = per * 1024 + 64
    got = outs[capi.OUT_PLANAR][0][s_ * channels * cap:(s_ + 1) * channels * cap].reshape(channels, cap)[:, :ref.shape[1]]
    assert outs[capi.OUT_PLANAR][1][s_] == ref.shape[1] and ref.shape[1] > 0
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max()))


def test_streams_without_packets_in_a_call_parallel_run_cutting(ctx):
    """Multi-stream decoding of files of different lengths: some streams have NO packet in a call (they ended earlier, or
    have not started) -- among them the last stream of a host party's range, whose s_base / s_cnt stay 0 -- while the
    batch takes the wide route of the run cutter (compact runs, group mode, short-block batches, >= 2 streams per party).
    Two calls (the second one after some streams have reached EOS) against the serial route, bit for bit."""
    from vorbispizza_amd import Decoder, capi
    channels, n_streams, frames = 2, 16, 60
    pk, res, posts, counts = stream_major_batch(n_streams, frames, channels, seed=77, floor=True, interleaved=True,
                                                p_ls=0.25, p_sl=0.2, silent_prob=0.1)
    pk["mapping"] = pk["flags"] & 1
    floors = [(helpers.SHORT_XLIST, 2), (helpers.LONG_XLIST, 2)]
    mappings = [{"coupling": [(0, 1)], "channel_floor": [0] * channels}, {"coupling": [(0, 1)], "channel_floor": [1] * channels}]
    idx = np.arange(len(pk)).reshape(n_streams, frames)
    empty_first = {0, 3, 7, 11, 15}          # no packets in call 1 (3, 7, 11, 15 end a party's range of 4 streams)
    ends_in_first = {2, 6, 14}               # EOS on their last packet of call 1; absent from call 2
    half = frames // 2
    sel1 = np.concatenate([idx[s, :half] for s in range(n_streams) if s not in empty_first])
    sel2 = np.concatenate([idx[s, (0 if s in empty_first else half):] for s in range(n_streams) if s not in ends_in_first])
    calls = []
    for sel in (sel1, sel2):
        sub = pk[sel].copy()
        calls.append((sub, np.ascontiguousarray(posts.reshape(len(pk), channels, 64)[sel].reshape(-1, 64)),
                      np.ascontiguousarray(counts.reshape(len(pk), channels)[sel].reshape(-1))))
    for s in ends_in_first:
        last = np.nonzero(calls[0][0]["stream"] == s)[0][-1]
        calls[0][0]["flags"][last] |= PKT_EOS
    cap = 2 * frames * 1024 + 64  # (stream_out_capacity is one number per call: room for a late starter's whole file)
    results = {}
    for mode, kv in (("serial", dict(VPZ_PAR_MIN_PACKETS=1 << 40, VPZ_NO_GROUP=1)),
                     ("wide", dict(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4, VPZ_NO_GROUP=None))):
        with env(**kv):
            dec = Decoder(ctx, channels, 256, 2048, floors=floors, mappings=mappings, n_streams=n_streams)
            out = np.zeros(n_streams * channels * cap, dtype=np.float32)
            offs = np.arange(n_streams, dtype=np.int64) * channels * cap
            total = np.zeros(n_streams, dtype=np.int64)
            per_packet = []
            for sub, p, c in calls:
                w = dec.synth_raw(sub, res, p, c, out, offs + total * channels, cap - int(total.max()),
                                  capi.OUT_INTERLEAVED, 0, capi.MEM_HOST)
                per_packet.append(dec.last_packet_samples(len(sub)))
                total += w
            results[mode] = (out, total.copy(), np.concatenate(per_packet), [dec.position(s) for s in range(n_streams)])
            dec.close()
    a, b = results["serial"], results["wide"]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert a[1][0] > 0 and a[1][2] > 0 and np.abs(a[0]).max() > 0
