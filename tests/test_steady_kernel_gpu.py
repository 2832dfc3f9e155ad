"""steady_stereo_kernel (csrc/steady_stereo.hip): batches of the stereo fast path in which every frame is the
steady state of its stream -- a 2048 block after a 2048 block, long windows on both sides, already floored, planar float32 in and
out -- are overlap-added in the lanes by a kernel of their own; anything else takes synth_dual_kernel.  The two kernels walk the
same runs and do the same arithmetic per sample, so every case here decodes its packets twice, on the default route and under
VPZ_NO_STEADY=1, and compares the PCM BIT FOR BIT; one of the two is held against the C oracle at the bar of
tests/test_chained_route_gpu.py.  Which kernel ran is the `kernel` word of VPZ_HOST_PROFILE's call line.

The shapes are small: VPZ_PLAN_SLOTS=1 with VPZ_DUAL_RUN=R makes choose_run_length settle on runs of R frames (a chained cut takes
the shortest run length >= VPZ_DUAL_RUN that some number of rounds of the slots gives; with one slot every length is one), as in
tests/test_run_lengths_gpu.py.  41 frames in runs of 8 are a stream's start, a first wave that recomputes the block in front of it,
three chained waves, a second workgroup and a run of one frame; runs of 4 and 9 are the floor of the cut and an odd length; 41
frames at VPZ_DUAL_RUN=63 are ONE run of 41 (no run is longer than its stream), so the longest run the plan cuts, 63 frames and 64
staged ones behind a recomputed block, comes from a stream of 315.
StreamDecoder.cs:640-694, 764-791."""
import re

import numpy as np
import pytest

import helpers
from helpers import PKT_BLOCK_FLAG, PKT_EOS, PKT_NEXT_FLAG, PKT_NO_FLOOR, PKT_PREV_FLAG
from synth_support import env

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_chained_route_gpu.py: max |err| <= TOL * max(1, |oracle|max)
_KERNEL = r"\[vpz host\] packets \d+: route (\w+), kernel (\w+),"


@pytest.fixture(scope="module")
def gpu():
    import __graft_entry__ as ge
    ge.build()
    import torch
    from vorbispizza_amd import Context
    c = Context(0)
    yield c, torch
    c.close()


def _cut(R):
    return dict(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4, VPZ_PLAN_SLOTS=1, VPZ_DUAL_RUN=R, VPZ_NO_CHAIN=None, VPZ_NO_DUAL=None)


def _batch(torch, frames_per_stream, seed, scale=2.0 ** -8):
    pk = helpers.all_long_packets(frames_per_stream)
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    res = torch.randn(len(pk) * 2048, generator=g, device="cuda:0", dtype=torch.float32) * scale
    return pk, res


def _decode(gpu, capfd, n_streams, rounds, cap, kv, steady=True, layout=None, clip=False, shift=0):
    """A decoder of n_streams stereo streams created under env(kv) (and VPZ_NO_STEADY=1 unless `steady`) takes `rounds`: a list of
    lists of calls [(packets, residue)]; the state is carried from call to call inside a round and the decoder is reset between
    rounds.  Every stream's PCM area holds `cap` samples per channel and starts `shift` elements off its place; a round starts at
    the head of the areas again.  Returns per round (PCM as the layout has it: [streams, 2, cap] planar, [streams, cap, 2]
    interleaved; samples written; clip flags) and per call (cut line and call line, route, kernel)."""
    ctx, torch = gpu
    from vorbispizza_amd import Decoder, capi
    layout = capi.OUT_PLANAR if layout is None else layout
    s16 = layout in (capi.OUT_INTERLEAVED_S16, capi.OUT_PLANAR_S16)
    planar = layout in (capi.OUT_PLANAR, capi.OUT_PLANAR_S16)
    results, profs = [], []
    with env(VPZ_NO_STEADY=None if steady else 1, **kv):
        dec = Decoder(ctx, 2, 256, 2048, n_streams=n_streams, clip_samples=clip)
        for calls in rounds:
            if s16:
                out = torch.full((n_streams * 2 * cap + shift,), -12345, device="cuda:0", dtype=torch.int16)
            else:
                out = torch.full((n_streams * 2 * cap + shift,), float("nan"), device="cuda:0", dtype=torch.float32)
            written = np.zeros(n_streams, dtype=np.int64)
            for pk, res in calls:
                offs = np.arange(n_streams, dtype=np.int64) * 2 * cap + written * (1 if planar else 2) + shift
                capfd.readouterr()
                with env(VPZ_HOST_PROFILE=1):
                    w = dec.synth_raw(pk, res, None, None, out, offs, cap - int(written.max()), layout, cap, capi.MEM_DEVICE)
                ctx.synchronize()
                err = capfd.readouterr().err
                prof = helpers.host_profile(err)
                words = re.findall(_KERNEL, err)
                assert len(words) == 1, err[-1000:]
                prof["route"], prof["kernel"] = words[0]
                profs.append(prof)
                written += w
            pcm = out[shift:].view(n_streams, 2, cap) if planar else out[shift:].view(n_streams, cap, 2)
            results.append((pcm, written, [dec.has_clipped(s) for s in range(n_streams)]))
            dec.reset()
    dec.close()
    return results, profs


def _same_bits(torch, a, b):
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a.contiguous(), b.contiguous())


def _oracle_stream(oracle, pk, res, s, clip=False):
    """One stream's packets (of one or several calls: [(packets, residue)]) through the oracle: (PCM [2, samples], has clipped)."""
    from vorbispizza_amd import make_packets
    flags, granule, spectra = [], [], []
    for p, r in zip(pk, res):
        mine = np.nonzero(p["stream"] == s)[0]
        r = r.cpu().numpy()
        for i in mine:
            n = 2048 if p["flags"][i] & PKT_BLOCK_FLAG else 256
            flags.append(p["flags"][i])
            granule.append(p["granule"][i])
            spectra.append(r[int(p["residue_offset"][i]):int(p["residue_offset"][i]) + n])
    q = make_packets(len(flags))
    q["flags"] = flags
    q["granule"] = granule
    q["residue_offset"] = np.concatenate([[0], np.cumsum([len(x) for x in spectra])[:-1]]) if spectra else []
    fs = oracle.FlooredStream(2, 256, 2048, q, np.concatenate(spectra) if spectra else np.zeros(1, np.float32), None, None, clip=clip)
    got = int(fs.run())
    return fs.pcm[:, :got], got


def _against_oracle(oracle, rounds_calls, result, n_streams, clip=False):
    pcm, written, _ = result
    worst = 0.0
    for s in range(n_streams):
        ref, got = _oracle_stream(oracle, [c[0] for c in rounds_calls], [c[1] for c in rounds_calls], s, clip)
        assert int(written[s]) == got, (s, int(written[s]), got)
        if got == 0:
            continue
        mine = pcm[s, :, :got].cpu().numpy().astype(np.float64)
        assert np.isfinite(mine).all(), s
        err, peak = float(np.abs(mine - ref).max()), float(np.abs(ref).max())
        assert err <= TOL * max(1.0, peak), "stream %d: max |err| %.3g, peak %.3g over %d samples" % (s, err, peak, got)
        worst = max(worst, err)
    return worst


def _both(gpu, oracle, capfd, n_streams, rounds, cap, R, clip=False):
    """The rounds on the default route and under VPZ_NO_STEADY=1: the route words, the same samples written, the same bits, the same
    clip flags; the default route's first round against the oracle.  Returns (results, profiles) of the default route."""
    _, torch = gpu
    a, pa = _decode(gpu, capfd, n_streams, rounds, cap, _cut(R), steady=True, clip=clip)
    b, pb = _decode(gpu, capfd, n_streams, rounds, cap, _cut(R), steady=False, clip=clip)
    assert [(p["route"], p["kernel"]) for p in pa] == [("stereo", "steady")] * len(pa), pa
    assert [(p["route"], p["kernel"]) for p in pb] == [("stereo", "general")] * len(pb), pb
    for p, q in zip(pa, pb):  # the launch alone picks the kernel: the plan is the same
        assert (p["by"], p["R"], p["runs"], p["chained"]) == (q["by"], q["R"], q["runs"], q["chained"]) and p["by"] == "length", (p, q)
    for (x, wx, cx), (y, wy, cy) in zip(a, b):
        assert np.array_equal(wx, wy) and cx == cy, (wx, wy, cx, cy)
        for s in range(n_streams):
            n = int(wx[s])
            assert _same_bits(torch, x[s, :, :n], y[s, :, :n]), "stream %d: steady_stereo_kernel and synth_dual_kernel differ" % s
            assert bool(torch.isnan(x[s, :, n:]).all()), "stream %d: samples written past the stream's end" % s
    worst = _against_oracle(oracle, rounds[0], a[0], n_streams, clip)
    return a, pa, worst


# (frames, VPZ_DUAL_RUN, the R the cut line must report)
@pytest.mark.parametrize("frames,knob,R", [(41, 8, 8), (41, 4, 4), (41, 9, 9), (41, 63, 41), (315, 63, 63)])
def test_one_all_long_stream(gpu, oracle, capfd, frames, knob, R):
    _, torch = gpu
    pk, res = _batch(torch, [frames], seed=frames + knob)
    a, (prof,), worst = _both(gpu, oracle, capfd, 1, [[(pk, res)]], frames * 1024, knob)
    assert prof["R"] == R and prof["runs"] == -(-frames // R), prof
    assert prof["chained"] == helpers.expected_chained([frames], R), prof
    assert int(a[0][1][0]) == (frames - 1) * 1024
    print("%d frames: R %d, runs %d, chained %d; oracle max |err| %.3g" % (frames, prof["R"], prof["runs"], prof["chained"], worst))


def test_streams_that_end_inside_a_workgroup(gpu, oracle, capfd):
    """17, 8 and 1 frames in one call at R = 8: runs of 8, 8, 1 | 8 | 1 -- stream 0 ends in a chained one-frame run in wave 2,
    stream 1 starts in wave 3 of the same workgroup, stream 2 is only its first frame (it leaves its tail and no sample)."""
    _, torch = gpu
    counts = [17, 8, 1]
    pk, res = _batch(torch, counts, seed=3)
    a, (prof,), worst = _both(gpu, oracle, capfd, 3, [[(pk, res)]], 17 * 1024, 8)
    assert prof["R"] == 8 and prof["runs"] == 5 and prof["chained"] == helpers.expected_chained(counts, 8) == 2, prof
    assert list(a[0][1]) == [16 * 1024, 7 * 1024, 0]
    print("streams of %r frames: %r; oracle max |err| %.3g" % (counts, prof, worst))


def test_two_calls_carry_the_state_and_a_reset_drops_it(gpu, oracle, capfd):
    """24 + 24 frames of one stream in two calls: the first saves its last tail in natural order, the second loads it into the lanes
    (kPreState) and emits from its first frame on.  After a reset the same two calls give the same PCM once more (the state copies'
    epoch: the second round must not see the first round's tail)."""
    _, torch = gpu
    pk1, res1 = _batch(torch, [24], seed=11)
    pk2, res2 = _batch(torch, [24], seed=12)
    calls = [(pk1, res1), (pk2, res2)]
    a, profs, worst = _both(gpu, oracle, capfd, 1, [calls, calls], 48 * 1024, 8)
    assert [p["R"] for p in profs] == [8] * 4 and [p["runs"] for p in profs] == [3] * 4, profs
    assert int(a[0][1][0]) == 47 * 1024 and int(a[1][1][0]) == 47 * 1024
    assert _same_bits(torch, a[0][0][0, :, :47 * 1024], a[1][0][0, :, :47 * 1024]), "the round after the reset differs"
    print("two calls of 24 frames, twice: oracle max |err| %.3g" % worst)


def test_clip_switch(gpu, oracle, capfd):
    """Stream 0 loud enough for some samples beyond +-1 (clipped, flag raised), stream 1 quiet (flag down)."""
    _, torch = gpu
    pk, res = _batch(torch, [20, 12], seed=21)
    res[:20 * 2048] *= 6.0
    res[20 * 2048:] *= 0.5
    a, (prof,), worst = _both(gpu, oracle, capfd, 2, [[(pk, res)]], 20 * 1024, 8, clip=True)
    pcm, written, clipped = a[0]
    assert clipped == [True, False], clipped
    loud = pcm[0, :, :int(written[0])].abs()
    at_limit = int((loud == 0.99999994).sum())
    assert 0 < at_limit < loud.numel() and float(loud.max()) == np.float32(0.99999994), (at_limit, float(loud.max()))
    assert float(pcm[1, :, :int(written[1])].abs().max()) < 0.99
    print("clip: %d samples at the limit; oracle max |err| %.3g" % (at_limit, worst))


def _fallback(gpu, capfd, n_streams, calls, cap, **kw):
    (r,), profs = _decode(gpu, capfd, n_streams, [calls], cap, _cut(8), **kw)
    assert [(p["route"], p["kernel"]) for p in profs] == [("stereo", "general")] * len(profs), profs
    return r


def test_a_short_block_in_the_middle_takes_the_general_kernel(gpu, oracle, capfd):
    from vorbispizza_amd import make_packets
    _, torch = gpu
    n, mid = 21, 10
    LONG = PKT_BLOCK_FLAG | PKT_PREV_FLAG | PKT_NEXT_FLAG
    flags = np.full(n, LONG | PKT_NO_FLOOR, dtype=np.uint8)
    flags[mid - 1] &= ~np.uint8(PKT_NEXT_FLAG)
    flags[mid] = PKT_NO_FLOOR
    flags[mid + 1] &= ~np.uint8(PKT_PREV_FLAG)
    sizes = np.where(flags & PKT_BLOCK_FLAG, 2048, 256)
    pk = make_packets(n)
    pk["flags"] = flags
    pk["granule"] = -1
    pk["residue_offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    g = torch.Generator(device="cuda:0").manual_seed(31)
    res = torch.randn(int(sizes.sum()), generator=g, device="cuda:0", dtype=torch.float32) * 2.0 ** -8
    r = _fallback(gpu, capfd, 1, [(pk, res)], n * 1024)
    rn = _fallback(gpu, capfd, 1, [(pk, res)], n * 1024, steady=False)
    assert np.array_equal(r[1], rn[1]) and _same_bits(torch, r[0][0, :, :int(r[1][0])], rn[0][0, :, :int(r[1][0])])
    _against_oracle(oracle, [(pk, res)], r, 1)


def test_an_eos_trimmed_last_packet_takes_the_general_kernel(gpu, oracle, capfd):
    _, torch = gpu
    frames = 17
    pk, res = _batch(torch, [frames], seed=41)
    pk[-1]["flags"] |= PKT_EOS
    pk[-1]["granule"] = (frames - 2) * 1024 + 300
    r = _fallback(gpu, capfd, 1, [(pk, res)], frames * 1024)
    assert int(r[1][0]) == (frames - 2) * 1024 + 300
    rn = _fallback(gpu, capfd, 1, [(pk, res)], frames * 1024, steady=False)
    assert np.array_equal(r[1], rn[1]) and _same_bits(torch, r[0][0, :, :int(r[1][0])], rn[0][0, :, :int(r[1][0])])
    _against_oracle(oracle, [(pk, res)], r, 1)


def test_other_layouts_and_alignments_take_the_general_kernel_and_give_the_steady_kernels_samples(gpu, oracle, capfd):
    """Interleaved PCM, 16-bit PCM and planar rows off an 8-byte boundary: synth_dual_kernel, as before -- and the samples are the
    ones steady_stereo_kernel writes for the same packets into aligned planar float32 rows (16-bit: `(int)(x * 32768f)` clamped)."""
    from vorbispizza_amd import capi
    _, torch = gpu
    counts = [17, 9]
    cap = 17 * 1024
    pk, res = _batch(torch, counts, seed=51)
    (want, written, _), (prof,) = (lambda r, p: (r[0], p))(*_decode(gpu, capfd, 2, [[(pk, res)]], cap, _cut(8)))
    assert (prof["route"], prof["kernel"]) == ("stereo", "steady"), prof
    _against_oracle(oracle, [(pk, res)], (want, written, None), 2)
    ilv = _fallback(gpu, capfd, 2, [(pk, res)], cap, layout=capi.OUT_INTERLEAVED)
    s16 = _fallback(gpu, capfd, 2, [(pk, res)], cap, layout=capi.OUT_PLANAR_S16)
    odd = _fallback(gpu, capfd, 2, [(pk, res)], cap, shift=1)
    off = _fallback(gpu, capfd, 2, [(pk, res)], cap, steady=False)
    for s in range(2):
        n = int(written[s])
        w = want[s, :, :n]
        assert int(ilv[1][s]) == int(s16[1][s]) == int(odd[1][s]) == int(off[1][s]) == n
        assert _same_bits(torch, ilv[0][s, :n, :].t(), w), ("interleaved", s)
        assert _same_bits(torch, odd[0][s, :, :n], w), ("odd offset", s)
        assert _same_bits(torch, off[0][s, :, :n], w), ("VPZ_NO_STEADY=1", s)
        as16 = (w * 32768.0).to(torch.int64).clamp(-32768, 32767).to(torch.int16)
        assert torch.equal(s16[0][s, :, :n], as16), ("16-bit", s)
