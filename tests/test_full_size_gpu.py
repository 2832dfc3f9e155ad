"""BASELINE.json's full sizes (configs[2], configs[3]) through size-independent properties, device memory all
the way: exact homogeneity (x2 in -> x2 out, bit for bit: every operation on the path is linear in the scale
and powers of two are exact), independence of the batch split, sample counts, and a prefix checked against the
oracle.  The contract line (bench.NorthStarLine) the same way and, every sample, against the oracle."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as ge
    ge.build()
    import torch
    from vorbispizza_amd import Context
    c = Context(0)
    yield c, torch
    c.close()


def _run(ctx, torch, dec, pk, res, posts, counts, samples, channels, splits=()):
    from vorbispizza_amd import capi
    cap = samples + 1024
    out = torch.zeros(channels * cap, device=res.device, dtype=torch.float32)
    dec.reset(-1)
    dec.set_position(0)
    bounds = [0] + list(splits) + [len(pk)]
    done = 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        sub = pk[a:b]
        p_ = None if posts is None else posts[a * channels:b * channels]
        c_ = None if counts is None else counts[a * channels:b * channels]
        # every call writes at the stream's running offset: hand it the tail of the buffer
        view = out[done:]
        w = dec.synth_raw(sub, res, p_, c_, view, None, cap - done, capi.OUT_PLANAR, cap, capi.MEM_DEVICE)
        done += int(w[0])
    ctx.synchronize()
    assert done == samples
    return out.reshape(channels, cap)[:, :samples]


def test_config2_full_size_properties(env, oracle):
    ctx, torch = env
    import bench
    from vorbispizza_amd import Decoder
    dev = torch.device("cuda", 0)
    pk, res, samples, _ = bench.build_synth_ola(torch, dev, 65536)
    dec = Decoder(ctx, 2, 256, 2048)
    y = _run(ctx, torch, dec, pk, res, None, None, samples, 2)
    assert torch.isfinite(y).all() and float(y.abs().max()) < 1.0
    # x2 in -> x2 out, exactly
    y2 = _run(ctx, torch, dec, pk, res * 2.0, None, None, samples, 2)
    assert torch.equal(y2, y * 2.0)
    # the batch split does not matter (state carried across calls == one call)
    y3 = _run(ctx, torch, dec, pk, res, None, None, samples, 2, splits=(1, 30001, 30002, 50000))
    assert torch.equal(y3, y)
    # prefix against the oracle
    n = 300
    opk = [{"flags": int(pk["flags"][f]), "granule": -1, "residue": res[int(pk["residue_offset"][f]):
            int(pk["residue_offset"][f]) + 2 * (1024 if pk["flags"][f] & 1 else 128)].cpu().numpy()} for f in range(n)]
    ref, _, _ = helpers.oracle_decode(oracle, 2, 256, 2048, opk)
    got = y[:, :ref.shape[1]].cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-5
    dec.close()


def test_config3_full_size_properties(env, oracle):
    ctx, torch = env
    import bench
    from vorbispizza_amd import Decoder
    dev = torch.device("cuda", 0)
    pk, res, posts, counts, floors, mappings, samples = bench.build_floor6(torch, dev, 16384)
    dec = Decoder(ctx, 6, 256, 2048, floors=floors, mappings=mappings)
    y = _run(ctx, torch, dec, pk, res, posts, counts, samples, 6)
    assert torch.isfinite(y).all()
    y2 = _run(ctx, torch, dec, pk, res * 2.0, posts, counts, samples, 6)
    assert torch.equal(y2, y * 2.0)
    y3 = _run(ctx, torch, dec, pk, res, posts, counts, samples, 6, splits=(5, 8000, 8001))
    assert torch.equal(y3, y)
    n = 40
    hp, hc = posts[: n * 6].cpu().numpy(), counts[: n * 6].cpu().numpy()
    opk = [{"flags": int(pk["flags"][f]), "granule": -1, "mapping": 0,
            "residue": res[f * 6144:(f + 1) * 6144].cpu().numpy(), "posts": hp[f * 6:(f + 1) * 6],
            "post_count": hc[f * 6:(f + 1) * 6]} for f in range(n)]
    ref, _, _ = helpers.oracle_decode(oracle, 6, 256, 2048, opk, floors=floors, mappings=mappings)
    got = y[:, :ref.shape[1]].cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    # the same batch as `ReadSamples(Span<float>)` delivers it: interleaved, written by a packet's six waves together --
    # the planar result transposed, bit for bit; and as 16-bit samples, the reference conversion of those floats
    from vorbispizza_amd import capi
    cap = samples + 1024
    for layout, dtype in ((capi.OUT_INTERLEAVED, torch.float32), (capi.OUT_INTERLEAVED_S16, torch.int16)):
        out = torch.zeros(6 * cap, device=dev, dtype=dtype)
        dec.reset(-1)
        dec.set_position(0)
        w = dec.synth_raw(pk, res, posts, counts, out, None, cap, layout, 0, capi.MEM_DEVICE)
        ctx.synchronize()
        assert int(w[0]) == samples
        inter = out[: samples * 6].reshape(samples, 6).t()
        if dtype == torch.float32:
            assert torch.equal(inter.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
        else:
            want = torch.clamp((y * 32768.0).to(torch.int32), -32768, 32767).to(torch.int16)
            assert torch.equal(inter, want)
    dec.close()


# ---- the contract line itself: bench.NorthStarLine, one stereo stream of 65 536 all-long N = 2048 frames in ONE call -- the
# chained by-length route (runs of R frames filled in by the context's host pool, every later run of a four-run workgroup
# chained to its neighbour's tail in LDS, thousands of workgroups over several rounds)

@pytest.fixture(scope="module")
def line(env):
    ctx, torch = env
    import bench
    ln = bench.NorthStarLine(torch, ctx, torch.device("cuda", 0), seed=3)
    yield ln
    ln.close()


def _profiled(capfd, fn, **kv):
    """fn() with VPZ_HOST_PROFILE=1 (and kv) in the environment; the route its synth call printed (helpers.host_profile)"""
    from synth_support import env as setenv
    capfd.readouterr()
    with setenv(VPZ_HOST_PROFILE=1, **kv):
        fn()
    return helpers.host_profile(capfd.readouterr().err)


def _synth(ctx, dec, pk, res, out, cap, layout=None):
    from vorbispizza_amd import capi
    layout = capi.OUT_PLANAR if layout is None else layout
    dec.reset(-1)
    w = dec.synth_raw(pk, res, None, None, out, None, cap, layout, cap if layout == capi.OUT_PLANAR else 0, capi.MEM_DEVICE)
    ctx.synchronize()
    return int(w[0])


def _assert_contract_route(prof, frames, threads):
    """The contract batch's route: the stereo kernel, runs of equal length.  threads >= 2: the parallel state machine, enough runs
    for the pool's fill, filled and swept by `threads` pool threads, three of every four chained; one thread: the serial state
    machine (explicit frame descriptors, nothing chained), everything on the calling thread."""
    what = "%r (host threads %d)" % (prof, threads)
    assert prof["route"] == "stereo" and prof["by"] == "length", what
    R = prof["R"]
    if threads >= 2:
        assert prof["pass1"] == "parallel", what
        assert frames // R >= 1024, what
        assert prof["runs"] == -(-frames // R), what
        assert prof["chained"] == helpers.expected_chained([frames], R), what
        assert (prof["fill"], prof["fill_threads"], prof["chain_threads"]) == ("the pool", threads, threads), what
    else:
        assert prof["pass1"] == "serial" and prof["chained"] == 0, what
        assert (prof["fill"], prof["fill_threads"], prof["chain_threads"]) == ("the calling thread", 1, 1), what


def _same_bits(torch, a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _spec_window(spec, res, w0, frames=40):
    """The float64 synthesis of the specification (tests/spec_synthesis.py) for output frames [w0, w0 + frames) of an all-long
    stereo stream, decoded from packet w0 - 1 on: PCM [2, frames * 1024] at samples [(w0 - 1) * 1024, ...).  The packets carry
    their spectra as they are (VPZ_PKT_NO_FLOOR): a floor whose curve is 1.0 everywhere stands in (posts at 255, multiplier 1:
    inverse dB table entry 255 = 10^0, exactly)."""
    spectra = res[(w0 - 1) * 2048:(w0 + frames) * 2048].cpu().numpy().reshape(-1, 2, 1024)
    packets = [{"flags": helpers.ALL_LONG, "mapping": 0, "residue": s, "posts": np.full((2, 2), 255), "post_count": [2, 2]}
               for s in spectra]
    return spec.decode(2, 256, 2048, [([0, 1024], 1)], [{"coupling": [], "channel_floor": [0, 0]}], packets)


def test_north_star_line_full_size(env, line, oracle, capfd):
    """bench.py's timed step, as it is, held to the oracle in every sample and to float64 windows of the specification at the
    boundaries of its runs, workgroups and rounds -- and, bit for bit, to every other cut of the same batch: no chaining, other run
    lengths, other pool sizes (party boundaries inside a workgroup), repeated steps on other inputs, steps after smaller calls,
    the batch split into calls, the interleaved layouts."""
    ctx, torch = env
    import spec_synthesis as spec
    from synth_support import env as setenv
    from vorbispizza_amd import Decoder, capi
    frames, S, cap = len(line.pk), line.samples, line.cap
    assert frames == 65536 and S == (frames - 1) * 1024

    # a) the route of the step as the bench runs it (the default environment: the pool fill when the decoder resolves to >= 2
    # host threads)
    p0 = helpers.resolved_host_threads()
    prof = _profiled(capfd, line.step)
    _assert_contract_route(prof, frames, p0)
    R, runs = prof["R"], prof["runs"]
    y = line.out.view(2, cap)[:, :S]
    ref = y.clone()
    assert int(line.dec.last_written[0]) == S
    ps = line.dec.last_packet_samples(frames)
    assert ps[0] == 0 and (ps[1:] == 1024).all()
    assert bool(torch.isfinite(ref).all())

    # b) every sample against the oracle
    max_err, rms, peak, n = helpers.compare_all_long_with_oracle(oracle, line.pk["flags"], line.pk["granule"], line.residue,
                                                                 ref, chunk=2048, threads=8)
    report = "R %d, runs %d, chained %d, host threads %d: oracle max |err| %.3g, RMS %.3g, peak %.3g over %d x 2 samples" % (
        R, runs, prof["chained"], p0, max_err, rms, peak, n)
    assert n == S and peak > 0.05, report
    assert max_err <= 1e-5 * max(1.0, peak), report

    # c) float64 windows of 40 frames: the head, the tail, and straddling the first run boundary, the first workgroup boundary
    # and the grid's quarter points (the boundaries of its rounds when it takes four)
    starts = [1, frames - 40] + [max(1, min(frames - 40, f - 20)) for f in (R, 4 * R, (runs // 4) * R, (3 * runs // 4) * R)]
    worst = 0.0
    for w0 in starts:
        want = _spec_window(spec, line.residue, w0)
        got = ref[:, (w0 - 1) * 1024:(w0 + 39) * 1024].cpu().numpy().astype(np.float64)
        e = float(np.abs(got - want).max())
        worst = max(worst, e)
        assert e <= 1e-5 * max(1.0, float(np.abs(want).max())), "spec window at frame %d: max |err| %.3g" % (w0, e)
    report += "; float64 windows at frames %r: max |err| %.3g" % (starts, worst)

    # d) bit for bit: other cuts of the same batch, each decoder created under its settings
    alt = torch.empty(2 * cap, device=ref.device, dtype=torch.float32)
    variants = [dict(VPZ_NO_CHAIN=1), dict(VPZ_DUAL_RUN=4), dict(VPZ_DUAL_RUN=13), dict(VPZ_DUAL_RUN=32),
                dict(VPZ_HOST_THREADS=2), dict(VPZ_HOST_THREADS=3), dict(VPZ_HOST_THREADS=7), dict(VPZ_HOST_THREADS=16)]
    for kv in variants:
        with setenv(**kv):
            dec = Decoder(ctx, 2, 256, 2048)
        alt.fill_(float("nan"))
        vp = _profiled(capfd, lambda: _synth(ctx, dec, line.pk, line.residue, alt, cap), **kv)
        dec.close()
        assert _same_bits(torch, alt.view(2, cap)[:, :S], ref), "%r: %r" % (kv, vp)
        if "VPZ_HOST_THREADS" in kv:
            _assert_contract_route(vp, frames, kv["VPZ_HOST_THREADS"])  # (16: the route made certain)
        if "VPZ_NO_CHAIN" in kv:
            assert vp["chained"] == 0, vp
        report += "; %r: R %d, runs %d, chained %d, fill %s" % (kv, vp["R"], vp["runs"], vp["chained"], vp["fill"])

    # repeated steps on one decoder, other inputs in between: A, 2A (exactly twice A), an independent B, A again
    try:
        line.residue.mul_(2.0)
        line.step()
        ctx.synchronize()
        assert _same_bits(torch, y, ref * 2.0), "2A is not twice A"
    finally:
        line.residue.div_(2.0)
    import bench
    _, res_b, s_b, _ = bench.build_synth_ola(torch, ref.device, frames, all_long=True, seed=4)
    assert s_b == S
    assert _synth(ctx, line.dec, line.pk, res_b, line.out, cap) == S
    dec = Decoder(ctx, 2, 256, 2048)
    assert _synth(ctx, dec, line.pk, res_b, alt, cap) == S
    dec.close()
    del res_b
    assert _same_bits(torch, y, alt.view(2, cap)[:, :S]), "B after A differs from B on a fresh decoder"
    assert not torch.equal(y, ref)
    line.step()
    ctx.synchronize()
    assert _same_bits(torch, y, ref), "A after B differs from the first A"

    # smaller calls first (below and around the fill's threshold), then the full step: the first step's bits; the smaller
    # calls give the first step's prefix
    for m in (8191, 4095):
        assert _synth(ctx, line.dec, line.pk[:m], line.residue, alt, cap) == (m - 1) * 1024
        assert _same_bits(torch, alt.view(2, cap)[:, :(m - 1) * 1024], ref[:, :(m - 1) * 1024]), m
    line.step()
    ctx.synchronize()
    assert _same_bits(torch, y, ref), "the full step after 8191- and 4095-frame calls"
    del alt

    # the batch split into calls, the state carried: pieces below and above the fill's threshold, every one saving its state
    y3 = _run(ctx, torch, line.dec, line.pk, line.residue, None, None, S, 2, splits=(1, 30001, 30002, 50000, 65533))
    assert _same_bits(torch, y3, ref), "split calls"
    del y3

    # the other instantiations of the kernel on this route: interleaved float32 (the planar result transposed) and 16-bit
    # samples (the reference conversion of those floats)
    for layout, dtype in ((capi.OUT_INTERLEAVED, torch.float32), (capi.OUT_INTERLEAVED_S16, torch.int16)):
        out = torch.zeros(2 * cap, device=ref.device, dtype=dtype)
        assert _synth(ctx, line.dec, line.pk, line.residue, out, cap, layout) == S
        inter = out[:S * 2].reshape(S, 2).t()
        if dtype == torch.float32:
            assert _same_bits(torch, inter, ref), "interleaved float32"
        else:
            want = torch.clamp((ref * 32768.0).to(torch.int32), -32768, 32767).to(torch.int16)
            assert torch.equal(inter, want), "interleaved 16-bit"
        del out, inter
    print(report)


def test_a_decoder_held_to_one_host_thread_cuts_on_the_calling_thread(env, line, capfd):
    """vpz_decoder_set_host_threads(1) means no pool, and a decoder uses the context's pool only if it has the decoder's party count:
    after a 16-thread decoder of the context has run the contract batch (and left its 16-party pool behind), decoders held to one
    and to three threads fill the runs on the calling thread -- the contract batch, and its first 8 191 frames (fewer packets than
    the parallel state machine takes: runs of 4 frames cut by length, enough of them for the pool's fill) -- and their PCM is the
    16-thread decoder's, bit for bit."""
    ctx, torch = env
    from synth_support import env as setenv
    from vorbispizza_amd import Decoder
    frames, S, cap = len(line.pk), line.samples, line.cap
    with setenv(VPZ_HOST_THREADS=16):
        dec16 = Decoder(ctx, 2, 256, 2048)
    ref = torch.full((2 * cap,), float("nan"), device=line.out.device, dtype=torch.float32)
    prof = _profiled(capfd, lambda: _synth(ctx, dec16, line.pk, line.residue, ref, cap))
    dec16.close()
    _assert_contract_route(prof, frames, 16)
    ref = ref.view(2, cap)[:, :S]
    out = torch.empty(2 * cap, device=ref.device, dtype=torch.float32)
    for threads, m in ((1, frames), (1, 8191), (3, 8191)):
        with setenv(VPZ_HOST_THREADS=None):
            dec = Decoder(ctx, 2, 256, 2048)
        dec.set_host_threads(threads)
        out.fill_(float("nan"))
        p = _profiled(capfd, lambda: _synth(ctx, dec, line.pk[:m], line.residue, out, cap))
        dec.close()
        what = "%d host threads, %d frames: %r" % (threads, m, p)
        assert p["route"] == "stereo" and p["by"] == "length" and p["pass1"] == "serial", what
        assert (p["fill"], p["fill_threads"], p["chain_threads"]) == ("the calling thread", 1, 1), what
        if m < frames:
            assert m // p["R"] >= 1024, what  # (what the pool would have filled)
        n = (m - 1) * 1024
        assert _same_bits(torch, out.view(2, cap)[:, :n], ref[:, :n]), what
