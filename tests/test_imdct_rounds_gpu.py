"""The batched IMDCT kernels past the first round of their persistent grids, and the FAST transforms' error against float64.

Every batched IMDCT kernel runs on a persistent grid: a wave takes a block (or a group of blocks) and steps on by
gridDim.x * blocks-per-workgroup until the batch ends.  The grids are (csrc/imdct_fast.hip resident_groups / grid_for,
csrc/imdct_exact.hip launch_imdct_exact)

    FAST    min(workgroups needed, num_cu * min(occupancy, 2))      blocks per workgroup: BLOCKS_PER_GROUP below
    EXACT   min(count, 4 * num_cu)                                  one block per workgroup

so on a 256-CU MI355X a wave takes a second block only beyond 16 384 (N = 256) ... 2 048 (N = 2048, 4096) blocks, 3 584 at N = 8192
and 1 024 in EXACT mode -- counts the rest of the suite reaches for dense N = 2048 alone.  The capacities here take the launch
code's UPPER bound of two workgroups per CU, whatever occupancy the runtime reports: with count = 3 * cap + tail every case runs
at least three whole rounds and a ragged last one (a whole workgroup, a whole wave group and a partly filled one), where the
pipelined kernels (256, 512, 1024, 2048) clamp their prefetch, skip stores and read a block twice.

1. dense batches through vpz_imdct_batch, every row against the oracle (FAST <= 1e-5, EXACT bit for bit), guard rows around the
   output, device memory and -- once per mode -- host memory;
2. the gathered variants (src_off / dst_off) through the three-pass decoder path, at block counts beyond two rounds per size;
3. an error budget for FAST against the float64 cosine sum (spec_synthesis.imdct), as a multiple K of the oracle's own error.
Mdct.cs:15-19; StreamDecoder.cs:640-694, 764-791."""
import re

import numpy as np
import pytest

import helpers
import spec_synthesis
from helpers import PKT_NO_FLOOR
from synth_support import env, random_xlist
from gpu_context import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_imdct_gpu.py: BASELINE's bar for FAST against the float32 oracle, |PCM| <~ 1

FAST_SIZES = (256, 512, 1024, 2048, 4096, 8192)
EXACT_SIZES = (64, 128) + FAST_SIZES
# channel-blocks a workgroup takes per step (csrc/imdct_fast.hip: kWavesPerGroup = 4 waves of 8, 4, 2, 1, 1 blocks; kWaves8192 = 7)
BLOCKS_PER_GROUP = {256: 32, 512: 16, 1024: 8, 2048: 4, 4096: 4, 8192: 7}
# the last round: one whole workgroup, one whole wave group, a partly filled wave group
TAIL = {256: 43, 512: 23, 1024: 11, 2048: 5, 4096: 5, 8192: 10}
EXACT_TAIL = 5
SENTINEL = 0x7FA5C3E1  # a NaN with a payload: a guard row that was written, or an output element that was not, cannot pass for data


def spectra(count, half, seed):
    return (np.random.default_rng(seed).standard_normal((count, half)) * 2.0 ** -8).astype(np.float32)


def capacity(n, fast):
    """Blocks one round of the grid holds, at most.  Rests on the launch rules: FAST grids are grid_for(work groups,
    resident_groups()) with resident_groups() <= 2 * num_cu (csrc/imdct_fast.hip); launch_imdct_exact takes min(count, 4 * num_cu)
    workgroups of one block (csrc/imdct_exact.hip).  64 and 128 have no FAST kernel: the EXACT one transforms them in either mode."""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if fast and n in BLOCKS_PER_GROUP:
        return 2 * num_cu * BLOCKS_PER_GROUP[n]
    return 4 * num_cu


def tail(n, fast):
    return TAIL[n] if fast and n in TAIL else EXACT_TAIL


def rounds_count(n, fast):
    cap = capacity(n, fast)
    count = 3 * cap + tail(n, fast)
    assert count > 2 * cap  # the premise: some wave takes a third block, whatever the occupancy
    return count, cap


# ---- 1. dense batches of several rounds -----------------------------------------------------------------------------------------

def _first_bad_row(bad, cap, what):
    if bool(bad.any()):
        row = int(bad.nonzero()[0, 0])
        raise AssertionError("%s: %d bad rows, the first is row %d in round %d (cap %d)" % (what, int(bad.sum()), row, row // cap, cap))


def _check_batch(full, count, n, ref, cap, fast, what):
    """`full`: torch float32 [count + 4, n] whose rows [2, 2 + count) the call wrote; ref: torch, same device, [count, n]."""
    import torch
    got = full[2:2 + count]
    if fast:
        err = (got - ref).abs().amax(dim=1)
        print("%s: max |got - ref| %.3g over %d rows" % (what, float(err.max()), count))
        _first_bad_row(~(err <= TOL), cap, what + ", against the oracle at 1e-5")  # (a NaN is a bad row)
        h = n // 2  # the mirrored halves are exact copies, as in Mdct.cs:378-381
        _first_bad_row((got[:, :h] != -torch.flip(got[:, :h], dims=[1])).any(dim=1), cap, what + ", first half against its mirror")
        _first_bad_row((got[:, h:] != torch.flip(got[:, h:], dims=[1])).any(dim=1), cap, what + ", second half against its mirror")
    else:
        _first_bad_row((got.view(torch.int32) != ref.view(torch.int32)).any(dim=1), cap, what + ", against the oracle's bits")
    guards = torch.cat([full[:2], full[2 + count:]]).view(torch.int32)
    assert guards.shape[0] == 4 and bool((guards == SENTINEL).all()), what + ": a guard row was written"


def _run_dense(ctx, oracle, n, fast, host):
    import torch
    from vorbispizza_amd import capi
    mode = capi.IMDCT_FAST if fast else capi.IMDCT_EXACT
    count, cap = rounds_count(n, fast)
    what = "%s N = %d, %d rows, %s memory" % ("FAST" if fast else "EXACT", n, count, "host" if host else "device")
    x = spectra(count, n // 2, 7 * n + int(fast))
    ref = oracle.mdct_reverse(x, n)
    if host:
        full_np = np.full((count + 4, n), SENTINEL, dtype=np.int32).view(np.float32)
        x_in = x.copy()
        ctx.imdct_batch(x_in, n, mode, out=full_np[2:2 + count])
        assert np.array_equal(x_in.view(np.uint32), x.view(np.uint32)), what + ": the input changed"
        _check_batch(torch.from_numpy(full_np), count, n, torch.from_numpy(ref), cap, fast, what)
        del full_np, x_in
    else:
        x_dev = torch.from_numpy(x).cuda()
        full = torch.full((count + 4, n), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        view = full[2:2 + count]  # whole rows: the 16-byte alignment of the float4 stores is kept
        assert view.is_contiguous() and view.data_ptr() % 16 == 0
        ctx.imdct_batch(x_dev, n, mode, out=view)
        ctx.synchronize()
        assert np.array_equal(x_dev.cpu().numpy().view(np.uint32), x.view(np.uint32)), what + ": the input changed"
        ref_dev = torch.from_numpy(ref).cuda()
        _check_batch(full, count, n, ref_dev, cap, fast, what)
        del full, view, x_dev, ref_dev
        torch.cuda.empty_cache()
    del x, ref


@pytest.mark.parametrize("n", FAST_SIZES)
def test_fast_dense_batch_of_several_rounds(ctx, oracle, n):
    """3 * cap + tail rows of per-row seeded spectra, device memory, rows [2, 2 + count) of a guarded tensor: every row is the
    oracle's within 1e-5 and mirrored exactly, the guard rows and the input keep their bits."""
    _run_dense(ctx, oracle, n, fast=True, host=False)


@pytest.mark.parametrize("n", EXACT_SIZES)
def test_exact_dense_batch_of_several_rounds(ctx, oracle, n):
    """The same for the reference's own schedule, one workgroup per block: the oracle's bits in every row."""
    _run_dense(ctx, oracle, n, fast=False, host=False)


@pytest.mark.parametrize("fast,n", [(True, 256), (False, 64)], ids=["fast-256", "exact-64"])
def test_host_memory_batch_of_several_rounds(ctx, oracle, fast, n):
    """VPZ_MEM_HOST: the context's staging buffers grow to the batch, the kernel writes the staged output densely and the copy
    back lands in the caller's rows alone."""
    _run_dense(ctx, oracle, n, fast=fast, host=True)


# ---- 2. the gathered variants, through the three-pass decoder path -----------------------------------------------------------

# block-size pairs no fused kernel takes (synth_supports_sizes / synth_big_supported): the three-pass path by construction
GATHER_PAIRS = [(64, 256), (128, 512), (128, 1024), (128, 2048), (128, 4096), (4096, 8192)]
CHANNELS = 8
FRAMES = 48  # per stream
_CALL_ROUTE = r"\[vpz host\] packets \d+: route (\w+),"  # tests/test_run_lengths_gpu.py


def _stream_flags(seed, p_ls, p_sl):
    fl = helpers.markov_block_flags(FRAMES, seed, p_ls=p_ls, p_sl=p_sl, start_long=bool(seed & 1))
    if fl[0] & 1 and not fl[1] & 1:  # a long first packet with a short successor is legal, but adds nothing here
        fl = helpers.markov_block_flags(FRAMES, seed, p_ls=p_ls, p_sl=p_sl, start_long=False)
        assert not fl[0] & 1
    return fl


def _gather_batch(size0, size1, floored, needs):
    """Streams of FRAMES packets with Markov window switching, as many as it takes for the channel-blocks of EACH size to exceed
    `needs` = (blocks of size0, blocks of size1).  The chain's long -> short rate follows the ratio of the two needs, so that
    neither size is padded by much.  Returns (per stream: packet dicts for helpers.oracle_decode, floors, mappings)."""
    want_long = min(0.9, max(0.5, needs[1] / float(needs[0] + needs[1])))
    p_sl = 0.3
    p_ls = p_sl * (1.0 - want_long) / want_long  # the chain's stationary share of long blocks is p_sl / (p_ls + p_sl)
    rng = np.random.default_rng(size0 * 13 + size1 + int(floored))
    floors, mappings = (), ()
    if floored:  # Floor1 and one coupling step per mapping (mapping 0: short blocks, mapping 1: long blocks)
        floors = [(random_xlist(rng, size0 // 2, 19), 2), (helpers.LONG_XLIST, 2)]
        mappings = [{"coupling": [(0, 1)], "channel_floor": [0] * CHANNELS}, {"coupling": [(1, 0)], "channel_floor": [1] * CHANNELS}]
    streams, blocks = [], [0, 0]
    while blocks[0] <= needs[0] or blocks[1] <= needs[1]:
        flags = _stream_flags(1000 * size1 + len(streams), p_ls, p_sl)
        packets = []
        for fl in flags:
            bf = int(fl) & 1
            half = (size1 if bf else size0) // 2
            blocks[bf] += CHANNELS
            if floored:
                res = (rng.standard_normal((CHANNELS, half)) * 3).round().astype(np.float32)
                res[:, int(half * 0.85):] = 0
                posts, counts = helpers.random_posts(rng, floors[bf][0], floors[bf][1], CHANNELS, silent_prob=0.1)
                packets.append({"flags": int(fl), "mapping": bf, "granule": -1, "residue": res.reshape(-1), "posts": posts,
                                "post_count": counts})
            else:
                res = (rng.standard_normal((CHANNELS, half)) * 2.0 ** -8).astype(np.float32)
                packets.append({"flags": int(fl) | PKT_NO_FLOOR, "mapping": 0, "granule": -1, "residue": res.reshape(-1)})
        streams.append(packets)
    assert blocks[0] > needs[0] and blocks[1] > needs[1], (blocks, needs)
    return streams, floors, mappings, blocks


def _gather_needs(size0, size1):
    """more than 2 * cap + tail channel-blocks of each size, for the kernel that transforms that size in FAST mode"""
    return tuple(2 * capacity(n, True) + tail(n, True) for n in (size0, size1))


def _run_gathered(ctx, oracle, capfd, size0, size1, floored):
    from vorbispizza_amd import Decoder, make_packets
    needs = _gather_needs(size0, size1)
    streams, floors, mappings, blocks = _gather_batch(size0, size1, floored, needs)
    n = len(streams)
    flat = [(s, p) for s in range(n) for p in streams[s]]  # stream-major, residues back to back
    pk = make_packets(len(flat))
    pk["stream"] = [s for s, _ in flat]
    pk["flags"] = [p["flags"] for _, p in flat]
    pk["mapping"] = [p["mapping"] for _, p in flat]
    pk["granule"] = -1
    sizes = np.array([p["residue"].size for _, p in flat], dtype=np.int64)
    pk["residue_offset"] = np.cumsum(sizes) - sizes
    res = np.concatenate([p["residue"] for _, p in flat])
    posts = counts = None
    if floored:
        posts = np.concatenate([p["posts"] for _, p in flat]).astype(np.int16)
        counts = np.concatenate([p["post_count"] for _, p in flat]).astype(np.uint8)
    capacity_ = max(sum(size1 if p["flags"] & 1 else size0 for p in st) for st in streams) + 1
    dec = Decoder(ctx, CHANNELS, size0, size1, floors=floors, mappings=mappings, n_streams=n)
    capfd.readouterr()
    with env(VPZ_HOST_PROFILE=1):
        outs = dec.synth(pk, res, posts, counts, capacity=capacity_)
    routes = re.findall(_CALL_ROUTE, capfd.readouterr().err)
    assert routes == ["generic"], routes
    positions = [dec.position(s) for s in range(n)]
    dec.close()
    # every stream against the oracle: a kernel's block list runs over the streams in order (build_generic_lists), so every round
    # and the ragged last one of both sizes lie in checked streams
    worst = 0.0
    for s in range(n):
        ref, pos, _ = helpers.oracle_decode(oracle, CHANNELS, size0, size1, streams[s], floors=floors, mappings=mappings)
        what = ("stream", s, "of", n)
        assert outs[s].shape == ref.shape and ref.size > 0, (what, outs[s].shape, ref.shape)
        assert positions[s] == pos, (what, positions[s], pos)
        scale = max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(outs[s] - ref).max())
        worst = max(worst, err / scale)
        assert err <= TOL * scale, (what, err, scale)
    print("(%d, %d)%s: %d streams, %d packets, channel-blocks %r for more than %r; worst |err| / scale %.3g"
          % (size0, size1, " floored" if floored else "", n, len(flat), blocks, needs, worst))


@pytest.mark.parametrize("size0,size1", GATHER_PAIRS)
def test_gathered_transforms_of_several_rounds(ctx, oracle, capfd, size0, size1):
    """Already floored packets (VPZ_PKT_NO_FLOOR) of eight channels, many streams in one synth call: both block sizes' gathered
    launches (imdct2048_kernel<true>, imdct256_kernel<true>, the src_off / dst_off branches of the others, the EXACT kernel for 64
    and 128) run more than two rounds and a ragged last one; every stream is the oracle's, sample for sample."""
    _run_gathered(ctx, oracle, capfd, size0, size1, floored=False)


def test_gathered_transforms_behind_floor_and_coupling(ctx, oracle, capfd):
    """(128, 2048) with Floor1 and one coupling step: generic_floor_kernel and the coupling pass at the same frame count."""
    _run_gathered(ctx, oracle, capfd, 128, 2048, floored=True)


# ---- 3. the FAST transforms against float64, measured against the oracle's own error --------------------------------------------

# K is a REGRESSION bar against the reference's error, not a specification: err_fast <= K * err_ref, where err_ref is the error
# of oracle.mdct_reverse (float32, the reference's schedule) against the float64 cosine sum on the same input, computed in the test.
# Twice the largest ratio measured on an MI355X, rounded up to one significant digit, at least 2: inputs are seeded and the kernels
# deterministic, so the margin only has to absorb a legitimate re-association of the sums.
#
# Measured err_fast / err_ref on an MI355X (max error; for the identity batch max error, rms error) -- the FAST transforms, with
# twiddles rounded once from double and fused multiply-adds, sit at a third to six tenths of the reference's own error:
#
#      N      sigma = 2^-8     unit variance     identity (max, rms)
#     256        0.538             0.562           0.336, 0.365
#     512        0.546             0.495           0.361, 0.365
#    1024        0.534             0.501           0.398, 0.319
#    2048        0.555             0.577           0.360, 0.313
#    4096        0.387             0.439           0.391, 0.295
#    8192        0.474             0.414           0.351, 0.288
#
# The largest is 0.577: twice that is 1.2, below the floor of 2.  K * err_ref stays 5 (identity, N = 8192: 2.1e-6) to 190 times
# (sigma = 2^-8, N = 256: 5.4e-8) below the old bar of 1e-5 * max(1, peak), which the test asserts case by case.
K = 2
BUDGET_INPUTS = ("sigma", "unit", "identity")


def _budget_input(n, kind):
    half = n // 2
    if kind == "sigma":
        return spectra(64, half, 3 * n)
    if kind == "unit":
        return np.random.default_rng(3 * n + 1).standard_normal((64, half)).astype(np.float32)
    return np.eye(half, dtype=np.float32)  # one bin per row: every (bin, sample) pair is looked at alone


def _truth(n, kind, x):
    """spec_synthesis.imdct in float64.  It caches its cosine matrix (268 MB at N = 8192): one size at a time here."""
    for k in [k for k in spec_synthesis._COS if k != n]:
        del spec_synthesis._COS[k]
    if kind == "identity":
        # imdct(eye) IS the cached matrix (1.0 * c plus zeros, exact in float64): taken as it is instead of a product of
        # 2 * (N/2)^2 * N flops
        spec_synthesis.imdct(x[:1])
        return spec_synthesis._COS[n]
    return spec_synthesis.imdct(x)


@pytest.fixture(scope="module")
def drop_cosine_cache():
    yield
    for k in [k for k in spec_synthesis._COS if k >= 4096]:
        del spec_synthesis._COS[k]


def _errors(y, truth):
    d = y.astype(np.float64)
    d -= truth
    np.abs(d, out=d)
    return float(d.max()), float(np.sqrt(np.mean(d * d)))


def budget_figures(ctx, oracle, n, kind):
    """(err_ref, err_fast, peak): errors as (max, rms) against the float64 truth"""
    from vorbispizza_amd import capi
    x = _budget_input(n, kind)
    truth = _truth(n, kind, x)
    err_ref = _errors(oracle.mdct_reverse(x, n), truth)
    err_fast = _errors(ctx.imdct_batch(x, n, capi.IMDCT_FAST), truth)
    return err_ref, err_fast, float(np.abs(truth).max())


@pytest.mark.parametrize("n,kind", [(n, kind) for n in FAST_SIZES for kind in BUDGET_INPUTS])
def test_fast_error_budget_against_float64(ctx, oracle, drop_cosine_cache, n, kind):
    err_ref, err_fast, peak = budget_figures(ctx, oracle, n, kind)
    print("N = %d, %s: err_ref max %.3g rms %.3g, err_fast max %.3g rms %.3g, ratios %.3f %.3f, peak %.3g"
          % (n, kind, err_ref[0], err_ref[1], err_fast[0], err_fast[1], err_fast[0] / err_ref[0], err_fast[1] / err_ref[1], peak))
    assert err_ref[0] > 0 and err_ref[1] > 0
    # the new bar is tighter than the old one
    assert K * err_ref[0] < TOL * max(1.0, peak), (n, kind, K, err_ref[0], peak)
    assert err_fast[0] <= K * err_ref[0], (n, kind, "max error", err_fast[0], err_ref[0])
    if kind == "identity":
        assert err_fast[1] <= K * err_ref[1], (n, kind, "rms error", err_fast[1], err_ref[1])


@pytest.mark.parametrize("n", EXACT_SIZES)
def test_exact_is_bit_identical_on_the_identity_batch(ctx, oracle, n):
    """EXACT mode needs no budget: it is held to the oracle's bits, here on one bin per row."""
    from vorbispizza_amd import capi
    x = np.eye(n // 2, dtype=np.float32)
    ref = oracle.mdct_reverse(x, n)
    got = ctx.imdct_batch(x, n, capi.IMDCT_EXACT)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
