"""The edges of the stereo fast path's chained by-length route (synth_plan.hip plan_runs / chain_runs, synth_dual.hip's deferred pass
for chained runs): all-long stereo streams just below, at and above the run count from which the host pool fills the run records
(frames / R >= 1024), an end-of-stream trim that leaves a last run of one frame, several streams -- one without packets, one of a
single packet -- whose pool shares start in the middle of a stream, and a second call that continues some of them.  Every stream
against the oracle in every sample, and bit for bit against the cut that chains nothing (VPZ_NO_CHAIN=1) and a decoder held to one
host thread on a context that has no pool.  StreamDecoder.cs:640-694, 764-791."""
import numpy as np
import pytest

import helpers
from helpers import PKT_EOS
from synth_support import env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs():
    import __graft_entry__ as ge
    ge.build()
    import torch
    from vorbispizza_amd import Context
    c = Context(0)
    solo = Context(0)  # only decoders held to one host thread run here: it never gets a pool
    yield c, solo, torch
    solo.close()
    c.close()


def _batch(torch, frames_per_stream, seed, first_offset=0):
    pk = helpers.all_long_packets(frames_per_stream, first_offset)
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    res = torch.randn(first_offset + len(pk) * 2048, generator=g, device="cuda:0", dtype=torch.float32) * 2.0 ** -8
    return pk, res


def _decode(ctx, torch, capfd, n_streams, calls, cap, kv, host_threads=None):
    """A decoder of n_streams stereo streams, created under env(kv), takes `calls` ([(packets, residue)]) one after the other with
    the state carried; every stream's PCM goes on where its last call ended.  Returns (PCM [n_streams, 2, cap], samples written per
    stream, the host profile of every call)."""
    from vorbispizza_amd import Decoder, capi
    out = torch.full((n_streams * 2 * cap,), float("nan"), device="cuda:0", dtype=torch.float32)
    written = np.zeros(n_streams, dtype=np.int64)
    profs = []
    with env(**kv):
        dec = Decoder(ctx, 2, 256, 2048, n_streams=n_streams)
        if host_threads is not None:
            dec.set_host_threads(host_threads)
        for pk, res in calls:
            offs = np.arange(n_streams, dtype=np.int64) * 2 * cap + written
            capfd.readouterr()
            with env(VPZ_HOST_PROFILE=1):
                w = dec.synth_raw(pk, res, None, None, out, offs, cap - int(written.max()), capi.OUT_PLANAR, cap, capi.MEM_DEVICE)
            ctx.synchronize()
            profs.append(helpers.host_profile(capfd.readouterr().err))
            written += w
    dec.close()
    return out.view(n_streams, 2, cap), written, profs


def _check_cut(prof, frames_per_stream, trimmed, fill_threads, what):
    """The run records of a cut by length: after the parallel state machine, the runs and the chained ones as computed here; filled
    by the pool when it has `fill_threads` >= 2 parties and there are frames / R >= 1024 runs' worth of frames, on the calling thread
    otherwise."""
    what = "%s: %r" % (what, prof)
    R = prof["R"]
    total = int(sum(frames_per_stream))
    assert prof["route"] == "stereo" and prof["by"] == "length", what
    if prof["pass1"] == "parallel":  # compact runs, three of every four chained
        assert prof["runs"] == len(helpers.by_length_runs(frames_per_stream, R)), what
        assert prof["chained"] == helpers.expected_chained(frames_per_stream, R, trimmed), what
    else:  # explicit frame descriptors (the serial state machine): nothing is chained
        assert prof["chained"] == 0, what
    pool = fill_threads >= 2 and total // R >= 1024
    assert (prof["fill"], prof["fill_threads"]) == (("the pool", fill_threads) if pool else ("the calling thread", 1)), what
    return "pool" if pool else "serial"


def _same_bits(torch, a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_stream(oracle, flags, granule, residue, pcm):
    max_err, rms, peak, n = helpers.compare_all_long_with_oracle(oracle, flags, granule, residue, pcm)
    assert max_err <= 1e-5 * max(1.0, peak), "max |err| %.3g, RMS %.3g, peak %.3g over %d samples" % (max_err, rms, peak, n)
    return max_err


# (4 097, 4 101, 8 193: an EOS granule 300 samples into the last packet's output; where R divides frames - 1, the last run holds
# that one trimmed frame -- 4 101 at R = 4 puts it in the middle of a workgroup, where chain_runs must leave it recomputed)
@pytest.mark.parametrize("frames", [4095, 4096, 4097, 4101, 8191, 8193, 65541])
def test_one_all_long_stream_around_the_pool_fill_threshold(ctxs, oracle, capfd, frames):
    ctx, solo, torch = ctxs
    eos = frames in (4097, 4101, 8193)
    pk, res = _batch(torch, [frames], seed=frames)
    if eos:
        pk[-1]["flags"] |= PKT_EOS
        pk[-1]["granule"] = (frames - 2) * 1024 + 300
    samples = (frames - 2) * 1024 + 300 if eos else (frames - 1) * 1024
    cap = frames * 1024
    trimmed = (0,) if eos else ()
    fills = []
    got, w, (prof,) = _decode(ctx, torch, capfd, 1, [(pk, res)], cap, dict(VPZ_HOST_THREADS=4, VPZ_PAR_MIN_PACKETS=1))
    fills.append(_check_cut(prof, [frames], trimmed, 4, "4 host threads"))
    assert int(w[0]) == samples, (int(w[0]), samples)
    pcm = got[0, :, :samples]
    err = _check_stream(oracle, pk["flags"], pk["granule"], res, pcm)
    nc, w_nc, (p_nc,) = _decode(ctx, torch, capfd, 1, [(pk, res)], cap, dict(VPZ_NO_CHAIN=1, VPZ_HOST_THREADS=4, VPZ_PAR_MIN_PACKETS=1))
    assert p_nc["chained"] == 0, p_nc
    assert np.array_equal(w_nc, w) and _same_bits(torch, nc[0, :, :samples], pcm), "VPZ_NO_CHAIN=1: %r" % p_nc
    one, w_one, (p_one,) = _decode(solo, torch, capfd, 1, [(pk, res)], cap, dict(VPZ_HOST_THREADS=None), host_threads=1)
    fills.append(_check_cut(p_one, [frames], trimmed, 1, "1 host thread"))
    assert np.array_equal(w_one, w) and _same_bits(torch, one[0, :, :samples], pcm), "1 host thread: %r" % p_one
    # (whatever R the chip's size gives, 4 <= R <= 63: 4 095 frames are fewer than 1 024 runs, 65 541 are more)
    if frames == 4095:
        assert fills == ["serial", "serial"], prof
    if frames == 65541:
        assert fills == ["pool", "serial"], prof
    print("%d frames: R %d, runs %d, chained %d, fill %s; oracle max |err| %.3g" % (frames, prof["R"], prof["runs"], prof["chained"],
                                                                                prof["fill"], err))


@pytest.mark.parametrize("threads", [3, 7])
def test_several_streams_through_the_pool_fill(ctxs, oracle, capfd, threads):
    """Six streams, (9 000, 0, 8 193, 1, 12 345, 8 191) packets: stream 1 has none (its segment is empty, the search over the runs'
    first indices meets repeated values), stream 3 a single one (it only primes its overlap); 3 or 7 pool shares start in the middle
    of a stream and of a workgroup.  A second call continues streams 0, 2 and 4; the oracle decodes both calls as one stream."""
    ctx, solo, torch = ctxs
    first = [9000, 0, 8193, 1, 12345, 8191]
    second = [7001, 0, 5000, 0, 6007, 0]
    pk1, res1 = _batch(torch, first, seed=101)
    pk2, res2 = _batch(torch, second, seed=102, first_offset=2048 * 3)  # (the second call's residue does not start at 0)
    cap = (max(first) + max(second)) * 1024  # (the second call's capacity is what is left after the longest first one)
    calls = [(pk1, res1), (pk2, res2)]
    got, w, profs = _decode(ctx, torch, capfd, 6, calls, cap, dict(VPZ_HOST_THREADS=threads, VPZ_PAR_MIN_PACKETS=None))
    for prof, counts in zip(profs, (first, second)):
        assert prof["pass1"] == "parallel", prof
        assert _check_cut(prof, counts, (), threads, "%d host threads" % threads) == "pool"
    want_w = [max(0, a + b - 1) * 1024 for a, b in zip(first, second)]
    assert list(w) == want_w, (list(w), want_w)
    worst = 0.0
    for s in range(6):
        o1 = int(np.nonzero(pk1["stream"] == s)[0][0]) * 2048 if first[s] else 0
        o2 = int(pk2["residue_offset"][np.nonzero(pk2["stream"] == s)[0][0]]) if second[s] else 0
        res = torch.cat([res1[o1:o1 + first[s] * 2048], res2[o2:o2 + second[s] * 2048]])
        n = first[s] + second[s]
        flags = np.full(n, helpers.ALL_LONG | helpers.PKT_NO_FLOOR, dtype=np.uint8)
        worst = max(worst, _check_stream(oracle, flags, np.full(n, -1, dtype=np.int64), res, got[s, :, :int(w[s])]))
    nc, w_nc, p_nc = _decode(ctx, torch, capfd, 6, calls, cap, dict(VPZ_NO_CHAIN=1, VPZ_HOST_THREADS=threads, VPZ_PAR_MIN_PACKETS=None))
    assert all(p["chained"] == 0 for p in p_nc), p_nc
    one, w_one, p_one = _decode(solo, torch, capfd, 6, calls, cap, dict(VPZ_HOST_THREADS=None), host_threads=1)
    for prof, counts in zip(p_one, (first, second)):
        assert _check_cut(prof, counts, (), 1, "1 host thread") == "serial"
    for s in range(6):
        n = int(w[s])
        assert int(w_nc[s]) == n and _same_bits(torch, nc[s, :, :n], got[s, :, :n]), ("VPZ_NO_CHAIN=1", s)
        assert int(w_one[s]) == n and _same_bits(torch, one[s, :, :n], got[s, :, :n]), ("1 host thread", s)
    print("%d host threads: %r; oracle max |err| %.3g" % (threads, [(p["R"], p["runs"], p["chained"], p["fill"]) for p in profs], worst))
