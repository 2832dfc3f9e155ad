"""vpz_pcm_loudness (csrc/pcm_loudness.hip) at the limits of its launches: the branches, staging layouts and grid rounds that
tests/test_pcm_loudness_gpu.py never ran, each at the smallest shape that reaches it.

TRUTH and BOUND are those of test_pcm_loudness_gpu.py, unchanged: loudness_truth.step_sums_sequential in numpy.longdouble, computed once
per process in groups of similar length (loudness_cases.truth), and loudness_truth.bound as it stands.  The cases are loudness_cases.py's;
test_loudness_cpu.py holds each to the shape it is named for and the float64 restatement to 0.01 of the bound on them.

THE CASES, and the lines of the kernels each is there for:
  channels_4 .. channels_255   G = 256 / C and `stride` (the host's launch code) from 4 to 255 channels: idle lanes `s < G` false in
                       loudness_pass (5, 7, 9, 31, 33, 85, 86, 129, 255), no padding at 32 and one float at 33, G = 1 from 129 on; rows of
                       2S + 17 and S samples; the weight table's 4, 5 and 7; at 255 channels also the caller's weights, 0 on the loudest
  edges_8, edges_3     `j0 >= count` and `tile = min(G, count - j0)`: steps == G, units == G + 1 (a second workgroup of (a) with a
                       one-sample tail, none of (c)), one sample short of G steps, G + 1 steps, steps == 2G with a tail of 31
  tails_1, tails_6     the `have` clamp of the staging loop and `tn = min(kChunk, len - t0)`: tails of 1, 31, 32, 33 and S - 1 samples;
                       the peak a negative last sample of a tail, and a first sample
  odd_11025_*, odd_44100_5   steps of 1103 and 4410 samples (last chunks of 15 and 26) with idle lanes, tails around the last chunk
  empty_rows, short_rows     `tiles == 0` (hipMemsetAsync of chan_peak, loudness_finish alone) and a launch of loudness_pass<true> in
                       which every workgroup leaves at `j0 >= count`, each inside a scratch allocation that holds stale numbers
  grid                 5 000 descriptors: the `r += gridDim.y` loops of the passes and of loudness_finish, the workgroup-uniform
                       `continue` in front of the barriers, LDS reused across descriptors
  regrowth             loudness_room frees and regrows between calls; a small call inside a large stale allocation
  three_steps, full_row      finish_blocks at max_steps 256 and 257; a row that fills its sums row, the longest tail the call accepts
  shift                the carry's indexing `first + j` across a workgroup boundary: k steps of silence move the sums by k places
  scaling              2^-12 and 2^+12 on the samples are 2^-24 and 2^+24 on the sums, bit for bit
  beyond 2^31          `src + d.src + j0 * S * C` and `sums[row * max_steps + j]` in 64 bits
  non-finite           the rule include/vorbispizza_pcm_loudness.h states: fmaxf drops a NaN from the peak, 0 x NaN passes a weight of 0

Largest error / bound observed on an MI355X (test_zz_the_largest_ratio_of_this_file prints them; the file takes 4.8 s there):
channel counts 4.9e-05 (4 to 255 channels), workgroup edges 9.1e-05, tails 8.0e-05, odd steps 5.1e-05, nothing to do 0, two grid rounds
1.2e-04, scratch regrowth 9.1e-05, sums geometry 6.1e-05, shift 2.8e-05, scaling 3.3e-05, beyond 2^31 4.4e-05: the float64 kernels sit
where the float64 restatement by steps sits (4e-05 to 8e-05 on edges_8, test_loudness_cpu.py), four orders of magnitude inside the bound."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loudness_cases as lc  # noqa: E402
import loudness_truth as lt  # noqa: E402
import loudness_support as first  # noqa: E402
from loudness_support import PEAK_SENTINEL, SENTINEL, check_case, launch, needs_longdouble  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

S = lc.S
WORST = {}


@pytest.fixture(scope="module")
def truth():
    """check_case reads loudness_support.truth(): that table, with this file's cases added to it once"""
    table = first.truth()
    if ("edges_8", 0) not in table:
        table.update(lc.truth())
    return table


def spread(n):
    """destination rows out of order, an unnamed one between every two"""
    return [2 * (n - 1 - i) for i in range(n)]


def run(ctx, group, name, **kw):
    case = lc.cases()[name]
    order = spread(len(case.rows))
    sums, peak = launch(ctx, case, order=order, **kw)
    worst = check_case(case, sums, peak, order)
    WORST[group] = max(WORST.get(group, 0.0), worst)
    print("%s: largest error / bound %.3g" % (name, worst))
    return case, order, sums, peak


@needs_longdouble
@pytest.mark.parametrize("name", ["channels_%d" % c for c in lc.CHANNEL_COUNTS] + ["channels_255_weights"])
def test_channel_counts(ctx, truth, name):
    case, order, sums, peak = run(ctx, "channel counts", name)
    k = lt.kernel_constants(ROOT)
    G = lt.launch_plan(case.channels, k)[0]
    assert lt.tiles_of(2 * S + 17, 8000, case.channels, k)[2] == -(-3 // G)
    if case.weights is not None:  # the loudest channel counts in the peak, not in the sums
        assert case.w[lc.PEAK_CHANNEL] == 0.0 and all(peak[o] == np.abs(r[:, lc.PEAK_CHANNEL]).max() for o, r in zip(order, case.rows))


@needs_longdouble
@pytest.mark.parametrize("name", ["edges_8", "edges_3"])
def test_workgroup_edges(ctx, truth, name):
    run(ctx, "workgroup edges", name)


@needs_longdouble
@pytest.mark.parametrize("name", ["tails_1", "tails_6"])
def test_tails(ctx, truth, name):
    case, order, sums, peak = run(ctx, "tails", name, gap=1)
    assert peak[order[0]] == np.float32(0.95) and case.rows[0][-1].min() == np.float32(-0.95)
    assert peak[order[1]] == np.float32(0.97) and case.rows[1][0, 0] == np.float32(0.97)


@needs_longdouble
@pytest.mark.parametrize("name", ["odd_11025_3", "odd_11025_6", "odd_44100_5"])
def test_steps_that_are_no_multiple_of_32(ctx, truth, name):
    run(ctx, "odd steps", name)


@needs_longdouble
def test_nothing_to_do(ctx, truth):
    """rows of no sample (no pass is launched: the peaks come from the memset) and rows shorter than a step ((c) is launched and every
    workgroup leaves), each right after a larger launch whose numbers lie in the scratch: +0.0 bit for bit in the named rows, exact
    peaks, the sentinel in the others -- check_case holds all three"""
    for name in ("empty_rows", "short_rows"):
        run(ctx, "workgroup edges", "edges_8")
        case, order, sums, peak = run(ctx, "nothing to do", name)
        assert (sums[order].view(np.int64) == 0).all()
        assert list(peak[order]) == [np.abs(r).max() if r.size else 0.0 for r in case.rows]
        assert (sums[1::2] == SENTINEL).all() and (peak[1::2] == PEAK_SENTINEL).all()


@needs_longdouble
def test_more_descriptors_than_the_grid_holds_side_by_side(ctx, truth):
    import types
    k = lt.kernel_constants(ROOT)
    grid, checked_case, checked = lc.cases()["grid"], lc.cases()["grid_checked"], lc.grid_checked_rows()
    n = len(grid.rows)
    assert n == 5000 > k["kLoudMaxGridY"]
    order = np.random.default_rng(9).permutation(lc.GRID_DST)[:n]
    sums, peak = launch(ctx, grid, order=[int(o) for o in order], gap=1, extra_rows=lc.GRID_DST - 1 - int(order.max()), max_steps=4)
    assert sums.shape == (lc.GRID_DST, 4)
    # every peak is exact, every named row holds +0.0 behind its steps, the 100 others keep the sentinel
    want_peak = np.array([np.abs(r).max() if r.size else 0.0 for r in grid.rows], dtype=np.float32)
    assert (peak[order] == want_peak).all()
    steps = np.array([r.shape[0] // S for r in grid.rows])
    behind = np.arange(4)[None, :] >= steps[:, None]
    assert (sums[order][behind].view(np.int64) == 0).all() and (sums[order][~behind] > 0).all()
    rest = np.setdiff1d(np.arange(lc.GRID_DST), order)
    assert rest.size == 100 and (sums[rest] == SENTINEL).all() and (peak[rest] == PEAK_SENTINEL).all()
    # every 7th row and the first and last four against the truth
    assert sum(i >= k["kLoudMaxGridY"] for i in checked) > 100
    worst = check_case(checked_case, sums[order[checked]], peak[order[checked]])
    WORST["two grid rounds"] = worst
    print("grid: largest error / bound %.3g" % worst)
    # a row of the second round alone in a launch: the same bits
    i = max(j for j in range(k["kLoudMaxGridY"], n) if grid.rows[j].shape[0] >= 2 * S)
    alone = types.SimpleNamespace(name="alone", fs=8000, channels=2, weights=None, rows=[grid.rows[i]])
    a_sums, a_peak = launch(ctx, alone, max_steps=4)
    assert a_sums[0].tobytes() == sums[order[i]].tobytes() and a_peak[0].tobytes() == peak[order[i]].tobytes()


@needs_longdouble
def test_the_scratch_is_freed_and_regrown_between_calls(truth):
    """a context of the test's own: tails_6 has 90 units (a scratch of a few KB, a quarter more allocated), edges_3 has 771: loudness_room
    frees and allocates again, and the small launch then runs inside the large allocation, stale numbers and all"""
    from vorbispizza_amd import Context
    own = Context(0)
    try:
        small, large = lc.cases()["tails_6"], lc.cases()["edges_3"]
        assert sum(-(-r.shape[0] // S) for r in large.rows) * 3 == 771 > 2 * sum(-(-r.shape[0] // S) for r in small.rows) * 6 == 180
        before = launch(own, small)
        run(own, "scratch regrowth", "edges_3")
        after = launch(own, small)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        WORST["scratch regrowth"] = max(WORST["scratch regrowth"], check_case(small, *after))
    finally:
        own.close()


@needs_longdouble
def test_the_geometry_of_sums(ctx, truth):
    import torch
    from vorbispizza_amd import capi
    # one and two blocks of loudness_finish: +0.0 from element 3 on (check_case)
    for max_steps in (256, 257):
        case, order, sums, peak = run(ctx, "sums geometry", "three_steps", max_steps=max_steps)
        assert sums.shape[1] == max_steps and (sums[order[0], :3] > 0).all() and (sums[order[0], 3:].view(np.int64) == 0).all()
    # a row that fills its sums row, with the longest tail: every element written, the sentinel row behind it untouched
    case = lc.cases()["full_row"]
    assert case.rows[0].shape[0] == 3 * S + S - 1
    sums, peak = launch(ctx, case, max_steps=3, extra_rows=1)
    WORST["sums geometry"] = max(WORST["sums geometry"], check_case(case, sums, peak))
    assert sums.shape == (2, 3) and (sums[0] > 0).all() and (sums[1] == SENTINEL).all() and peak[1] == PEAK_SENTINEL
    # one sample more is a fourth step: refused, nothing written
    longer = np.concatenate([case.rows[0], case.rows[0][:1]])
    src = torch.from_numpy(longer.reshape(-1)).to("cuda:0")
    d_sums = torch.full((2, 3), SENTINEL, dtype=torch.float64, device="cuda:0")
    d_peak = torch.full((2,), PEAK_SENTINEL, dtype=torch.float32, device="cuda:0")
    with pytest.raises(capi.SynthError) as refused:
        capi.pcm_loudness(ctx, src, 2, 8000, [(0, 4 * S, 0)], max_steps=3, out=(d_sums, d_peak))
    assert refused.value.status == capi.E_INVALID_ARG
    ctx.synchronize()
    assert (d_sums == SENTINEL).all() and (d_peak == PEAK_SENTINEL).all()
    capi.pcm_loudness(ctx, src, 2, 8000, [(0, 4 * S - 1, 0)], max_steps=3, out=(d_sums, d_peak))  # (the same call one sample shorter is good)
    ctx.synchronize()
    assert d_sums[0].cpu().numpy().tobytes() == sums[0].tobytes() and (d_sums[1] == SENTINEL).all()


@needs_longdouble
def test_silence_in_front_moves_the_sums_and_changes_no_bit(ctx, truth):
    """row B is k steps of zeros, then row A: sums_B[:k] is +0.0 and sums_B[k:] is sums_A, at k = 1, 3 and G = 32 (8 channels), where
    B's steps of A lie in another workgroup than A's own"""
    base = lc.cases()["shift"]
    run(ctx, "shift", "shift")
    assert lt.launch_plan(8, lt.kernel_constants(ROOT))[0] == 32
    for k in (1, 3, 32):
        sums, peak = launch(ctx, lc.shifted(base, k), max_steps=3 + k + 2)
        assert (sums[0, :3] > 0).all() and (sums[0, 3:].view(np.int64) == 0).all()
        assert (sums[1, :k].view(np.int64) == 0).all() and sums[1, k: k + 3].tobytes() == sums[0, :3].tobytes(), k
        assert (sums[1, k + 3:].view(np.int64) == 0).all() and peak[0] == peak[1]


@needs_longdouble
def test_a_power_of_two_on_the_samples_is_its_square_on_the_sums(ctx, truth):
    base, order, sums, peak = run(ctx, "scaling", "scaling")
    plain = launch(ctx, base, max_steps=5)
    for e in (-12, 12):
        got_sums, got_peak = launch(ctx, lc.scaled(base, e), max_steps=5)
        assert got_sums[0].tobytes() == np.ldexp(plain[0][0], 2 * e).tobytes() and got_peak[0].tobytes() == np.ldexp(plain[1][0], e).tobytes(), e
        assert (got_sums[0, :3] > 0).all() and (got_sums[1] == SENTINEL).all() and got_peak[1] == PEAK_SENTINEL  # (row 1 is named by nobody)


@needs_longdouble
def test_a_source_beyond_two_to_the_31(ctx, truth):
    import torch
    from vorbispizza_amd import capi
    case = lc.cases()["beyond"]
    tail = np.full(8192, 9.0, dtype=np.float32)
    at = [7, 4001]  # (an odd offset: a stereo window need not start on an even element)
    for a, r in zip(at, case.rows):
        tail[a: a + r.size] = r.reshape(-1)
    assert at[0] + case.rows[0].size < at[1] and at[1] + case.rows[1].size < 8192
    src = torch.empty((1 << 31) + 8192, dtype=torch.float32, device="cuda:0")
    src[1 << 31:] = torch.from_numpy(tail).to("cuda:0")
    sums = torch.full((3, 4), SENTINEL, dtype=torch.float64, device="cuda:0")
    peak = torch.full((3,), PEAK_SENTINEL, dtype=torch.float32, device="cuda:0")
    order = [2, 0]
    capi.pcm_loudness(ctx, src, 2, 8000, [((1 << 31) + a, r.shape[0], o) for a, r, o in zip(at, case.rows, order)], max_steps=4, out=(sums, peak))
    ctx.synchronize()
    del src
    WORST["beyond 2^31"] = max(WORST.get("beyond 2^31", 0.0), check_case(case, sums.cpu().numpy(), peak.cpu().numpy(), order))


@needs_longdouble
def test_sums_beyond_two_to_the_31(ctx, truth):
    import torch
    from vorbispizza_amd import capi
    case = lc.cases()["beyond"]
    max_steps = 300
    dst_rows = (1 << 31) // max_steps + 8
    assert (dst_rows - 3) * max_steps > 1 << 31
    src = torch.from_numpy(np.concatenate([r.reshape(-1) for r in case.rows])).to("cuda:0")
    sums = torch.empty((dst_rows, max_steps), dtype=torch.float64, device="cuda:0")
    peak = torch.empty((dst_rows,), dtype=torch.float32, device="cuda:0")
    sums[-3:] = SENTINEL
    peak[-3:] = PEAK_SENTINEL
    order = [2, 0]
    rows = [(0, case.rows[0].shape[0], dst_rows - 3 + order[0]), (case.rows[0].size, case.rows[1].shape[0], dst_rows - 3 + order[1])]
    capi.pcm_loudness(ctx, src, 2, 8000, rows, max_steps=max_steps, out=(sums, peak))
    ctx.synchronize()
    got, pk = sums[-3:].cpu().numpy(), peak[-3:].cpu().numpy()
    del sums, peak
    WORST["beyond 2^31"] = max(WORST.get("beyond 2^31", 0.0), check_case(case, got, pk, order))


@pytest.mark.parametrize("channel", [1, 5], ids=["weight_1", "lfe_weight_0"])
@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
def test_a_sample_that_is_not_finite(ctx, value, channel):
    """the header's rule: one +Inf, or one NaN, in one channel of row 2 of the crowd, in its third step.  Every other row is the same
    bits as without it; in the row itself the two steps before are the same bits and the sums from the third step on are not finite --
    also where the channel's weight is 0 (0 x NaN); +Inf is the peak, a NaN is not seen by it"""
    import types
    crowd = lc.cases()["crowd"]
    assert crowd.w[5] == 0.0 and crowd.w[1] == 1.0 and crowd.rows[2].shape[0] == 5 * S + 40
    clean_sums, clean_peak = launch(ctx, crowd, max_steps=8)
    rows = [r.copy() for r in crowd.rows]
    rows[2][2 * S + 17, channel] = value
    dirty = types.SimpleNamespace(name="dirty", fs=crowd.fs, channels=crowd.channels, weights=None, rows=rows)
    sums, peak = launch(ctx, dirty, max_steps=8)
    others = [i for i in range(len(rows)) if i != 2]
    assert sums[others].tobytes() == clean_sums[others].tobytes() and peak[others].tobytes() == clean_peak[others].tobytes()
    assert sums[-1].tobytes() == clean_sums[-1].tobytes() and (sums[-1] == SENTINEL).all()  # (the unnamed row)
    assert sums[2, :2].tobytes() == clean_sums[2, :2].tobytes() and np.isfinite(clean_sums[2]).all()
    assert not np.isfinite(sums[2, 2:5]).any() and (sums[2, 5:].view(np.int64) == 0).all()
    if np.isinf(value):
        assert peak[2] == np.inf
    else:
        rest = np.abs(rows[2])
        assert peak[2] == np.nanmax(rest) and np.isnan(rest).sum() == 1


def test_zz_the_largest_ratio_of_this_file():
    """the record lines of the module's docstring come from here (run with -s)"""
    assert WORST and max(WORST.values()) <= 1.0
    for key in sorted(WORST):
        print("largest error / bound  %-24s %.3g" % (key, WORST[key]))
