"""vpz_pcm_logmel at the limits of its tiles and transform sizes: the branches of csrc/pcm_logmel.hip that tests/test_pcm_logmel_gpu.py,
whose transform sizes are all multiples of 8 and whose largest LDS request is 98 KB, does not execute.

The case lists are tests/test_logmel_cpu.py's LIMIT_* (a test without a GPU holds them to a restatement of the launch plan, tile_plan):
  the k loop's tail     n_fft / 2 = 1, 2, 3 mod 4 (n_fft 34, 36, 38, 1022), in the one- and in the two-row-tile kernel; at 1022, where
                        the window is so small over the tail's six samples that noise hides them inside the bound, single samples too;
  the LDS budget        n_fft 1024 at hops 110, 111 (64-frame tiles, 40 859 and 40 850 of 40 960 floats), 112, 113, 757 (32 frames,
                        40 908 floats), 758 (16 frames);
  bin groups            n_fft 62 (cols == nb), 126, 254 (one group per wave), 256 (wave 0 takes a second round), 1024 in 64-frame tiles;
  a partial 64-frame tile with 40 live frames (T = 104): every crowd launch;
  the skew              hops 2, 4, n_fft, n_fft - 1;
  the silent shortcut   both clauses of its condition, each decisive, one sample either side;
  a second descriptor   with all four waves working and wave 0 in a second round;
  one Inf inside a window reaches exactly the frames that cover it;
  scaling by 2^+-12     shifts the power output's exponent by +-24 and changes no other bit (every step is a float32 fmaf).

The truth is tests/test_logmel_cpu.py's float64 restatement and the tolerance its derived bound e_M, as it stands: every checked row gives
error / bound < 1, rows not named and the guards keep the sentinel bit for bit.  A launch of 64-frame tiles is sized from the device
(one row more than gives every CU two workgroups); four of its rows are held to the truth and EVERY row is compared bit for bit with the
same windows sent in launches small enough to take 32-frame tiles -- a result does not depend on the tile.  The truth is never the call
under test.  No case of the lists was left out.

Largest error / bound ratios observed on an MI355X (each test prints its own): 0.072 for the power output, at (36, 6), and 0.157 for log10,
at (32, 2) -- the small transforms with few bins to a band, as in tests/test_pcm_logmel_gpu.py; 0.0041 and 0.016 over the LDS boundaries
of n_fft 1024 (hops 112, 113, 757, 758), 0.0017 in its 64-frame launches (hops 110, 111; 1022 at 110), 0.0018 and 0.010 at (1022, 1022)
(0.0036 and 0.0066 for its single samples, at hops 1022 and 110),
0.059 and 0.125 at (38, 4) in 64-frame tiles, 0.0092 over the 304 checked rows of the second-descriptor launch, 0.023 and 0.127 at the
silent shortcut's edges."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from logmel_truth import (CROWD_T, LIMIT_CROWDS, LIMIT_GROUPS, LIMIT_HOPS, LIMIT_LDS, LIMIT_TAIL, check_log, check_power, crowd_rows,
    frames_of, limit_F, limit_frames, logmel_truth, mel_weights64, silence_value, tile_plan)
from pcm_support import LOGMEL_DST_ROWS as DST_ROWS, FLOOR, SENTINEL, guarded, rows_back  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

MODES = [(False, True), (False, False), (True, True), (True, False)]  # (log, bands_first)
MODE_IDS = ["power-bands_first", "power-frames_first", "log10-bands_first", "log10-frames_first"]
TWO_MODES, TWO_MODE_IDS = [MODES[0], MODES[3]], [MODE_IDS[0], MODE_IDS[3]]


def case_id(case):
    return "%d_%d" % (case[0], case[1])


def spec_for(n_fft, hop, n_mels, log, bands_first, norm="slaney"):
    from vorbispizza_amd import capi
    return capi.LogMelSpec.make(sample_rate=16000, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=0.0, f_max=8000.0, mel_scale="slaney", mel_norm=norm, log=log,
                                floor=FLOOR, bands_first=bands_first)


_W = {}


def weights_for(n_fft, n_mels, norm="slaney"):
    """W of spec_for's bank.  Every bin but 0 and the Nyquist one (which no band of any bank weighs) is live in some band: an error in
    any column of the transform reaches the output"""
    key = (n_fft, n_mels, norm)
    if key not in _W:
        W = mel_weights64(16000, n_fft, n_mels, 0.0, 8000.0, "slaney", norm)
        assert (W[:, 1:-1].sum(axis=0) > 0).all() and (W.sum(axis=1) > 0).all()
        _W[key] = W
    return _W[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def silence_bits(log):
    return silence_value(FLOOR).view(np.uint32) if log else np.uint32(0)


def run(ctx, d_src, rows, dst_rows, F, n_fft, hop, n_mels, log, bands_first, norm="slaney", chunk=None):
    """the rows in one launch (or in launches of at most `chunk` rows) -> [dst_rows][T][n_mels]; the guards keep their sentinel"""
    from vorbispizza_amd import capi
    T = 1 + F // hop
    spec = spec_for(n_fft, hop, n_mels, log, bands_first, norm)
    whole, dst = guarded(dst_rows, n_mels * T)
    view = dst.view((dst_rows, n_mels, T) if bands_first else (dst_rows, T, n_mels))
    for c0 in range(0, len(rows), chunk or len(rows)):
        assert capi.pcm_logmel(ctx, d_src, rows[c0: c0 + (chunk or len(rows))], view, spec, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    return rows_back(whole, dst_rows, n_mels, T, bands_first)


def unnamed_keep_the_sentinel(got, rows):
    rest = np.setdiff1d(np.arange(got.shape[0]), [row for _, _, row in rows])
    assert rest.size > 0 and (bits(got[rest]) == SENTINEL).all()


_CASES = {}


def five_lengths(n_fft, hop, F, n_mels):
    """the source, the descriptors and the float64 truth of five rows of a spec -- L = F (real samples reflect at both ends), F - 1 (the
    reflected tail starts at the one zero), a third (silent tiles behind it), 1, 0 --: computed once, shared by the tests of the spec.
    The rows share one source array at odd offsets and overlap in it."""
    key = (n_fft, hop, F, n_mels)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * hop + n_fft)
        W = weights_for(n_fft, n_mels)
        Ls = [F, F - 1, F // 3, 1, 0]
        src = (rng.standard_normal(3 * F + 64) * 0.5).astype(np.float32)
        order = rng.permutation(DST_ROWS)[: len(Ls)]
        rows = [(1 + 2 * i * (F // 5), L, int(row)) for i, (L, row) in enumerate(zip(Ls, order))]
        assert all(a % 2 == 1 and a + L <= src.size for a, L, _ in rows)
        _CASES[key] = (src, rows, [logmel_truth(src[a: a + L], L, F, n_fft, hop, W) for a, L, _ in rows])
    return _CASES[key]


def hold_to_the_truth(got, rows, truths, log):
    """every named row within the bound (a row of L = 0: the silence value bit for bit) -> the largest error / bound"""
    worst = 0.0
    for (at, L, row), (M, e_M) in zip(rows, truths):
        worst = max(worst, check_log(got[row], M, e_M, FLOOR) if log else check_power(got[row], M, e_M))
        if L == 0:
            assert (bits(got[row]) == silence_bits(log)).all()
    return worst


def five_lengths_against_the_truth(ctx, case, log, bands_first, what):
    import torch
    n_fft, hop, T, n_mels, tile = case
    F = limit_F(case)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert tile_plan(n_fft, hop, T, 5, cu)[0] == tile
    src, rows, truths = five_lengths(n_fft, hop, F, n_mels)
    got = run(ctx, torch.from_numpy(src).to("cuda:0"), rows, DST_ROWS, F, n_fft, hop, n_mels, log, bands_first)
    unnamed_keep_the_sentinel(got, rows)
    worst = hold_to_the_truth(got, rows, truths, log)
    print("error / bound %s (%d, %d) %s %s, %d-frame tiles, %d LDS floats: %.4f" % (
        what, n_fft, hop, "log10" if log else "power", "bands first" if bands_first else "frames first", tile, tile_plan(n_fft, hop, T, 5, cu)[1], worst))
    assert worst < 1.0


# ---- 1. the k loop's tail
@pytest.mark.parametrize("log,bands_first", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", LIMIT_TAIL, ids=case_id)
def test_transform_sizes_that_leave_k_steps_behind_the_blocks_of_four(ctx, case, log, bands_first):
    """n_fft / 2 k-steps go in blocks of four; 34, 36, 38 and 1022 leave one, two, three and three to the loop behind the blocks"""
    five_lengths_against_the_truth(ctx, case, log, bands_first, "tail")


# (frames, each with the place m of its one sample): n_fft 1022's last three k-steps are m = 1016 .. 1021
TAIL_IMPULSES = {(1022, 1022): [(1, 1016), (2, 1017), (3, 1018), (4, 1019), (5, 1020), (6, 1021), (10, 1016), (11, 1018), (12, 1020), (15, 1017), (16, 1019), (17, 1021)],
                 (1022, 110): [(5, 1016), (17, 1017), (29, 1018), (41, 1019), (53, 1020), (96, 1021)]}


@pytest.mark.parametrize("hop", [1022, 110], ids=["1022_1022-16_frame_tiles", "1022_110-64_frame_tiles"])
def test_single_samples_on_the_coefficients_of_the_last_k_steps(ctx, hop):
    """At n_fft 1022 the window is below 3.4e-4 over the six samples of the leftover k-steps: in noise their whole contribution lies
    inside the bound (the random cases above pass with that loop removed).  So a row of zeros with single samples of +-1 more than a
    transform apart, each the ONLY sample of one frame and at one of the places m = 1016 .. 1021: that frame's M is w[m]^2 sum_k W[b][k],
    a thousand bounds from 0.  Hop 1022 in 16-frame tiles; hop 110 in a launch of 64-frame tiles, the frames in both row tiles and in
    the partial last tile, with the crowd's random rows around it."""
    import torch
    n_fft, n_mels = 1022, 40
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    n, T = (5, 19) if hop == 1022 else (crowd_rows(cu), CROWD_T)
    F = limit_frames(hop, T)
    assert tile_plan(n_fft, hop, T, n, cu)[0] == (16 if hop == 1022 else 64) and (n_fft // 2) % 4 == 3
    W = weights_for(n_fft, n_mels)
    x = np.zeros(F, dtype=np.float32)
    for i, (t, m) in enumerate(TAIL_IMPULSES[(n_fft, hop)]):
        x[t * hop - n_fft // 2 + m] = 1.0 if i % 2 == 0 else -1.0
    rng = np.random.default_rng(hop)
    src = np.concatenate([np.zeros(1, np.float32), x, (rng.standard_normal(67 * n + F) * 0.5).astype(np.float32)])
    rows = [(1, F, 1)] + [(F + 2 + 67 * i, F - int(rng.integers(0, F // 2)), 1 + i) for i in range(1, n)]
    X = frames_of(x, F, F, n_fft, hop)
    M, e_M = logmel_truth(x, F, F, n_fft, hop, W)
    for t, m in TAIL_IMPULSES[(n_fft, hop)]:  # on the truth alone: the frame has that one sample, and an output of 0 cannot pass for it
        assert np.nonzero(X[t])[0].tolist() == [m] and m >= n_fft - 2 * ((n_fft // 2) % 4) and (M[t] > 1000 * e_M[t]).all(), (t, m)
    assert {m for _, m in TAIL_IMPULSES[(n_fft, hop)]} == set(range(1016, 1022))
    got = run(ctx, torch.from_numpy(src).to("cuda:0"), rows, n + 2, F, n_fft, hop, n_mels, False, True)
    unnamed_keep_the_sentinel(got, rows)
    worst = check_power(got[1], M, e_M)
    print("error / bound single samples (1022, %d): %.4f" % (hop, worst))
    assert worst < 1.0


# ---- 2. the LDS budget at n_fft 1024
@pytest.mark.parametrize("log,bands_first", TWO_MODES, ids=TWO_MODE_IDS)
@pytest.mark.parametrize("case", LIMIT_LDS, ids=case_id)
def test_hops_either_side_of_a_tile_boundary_of_the_lds(ctx, case, log, bands_first):
    """n_fft 1024: hops 112 and 113 are the first that 64 frames do not fit, 757 the last that 32 fit (40 908 of 40 960 floats), 758 the
    first that takes 16"""
    assert tile_plan(1024, 757, 41, 5, 256) == (32, 40908) and tile_plan(1024, 758, 41, 5, 256)[0] == 16 and tile_plan(1024, 112, 71, 5, 256)[0] == 32
    five_lengths_against_the_truth(ctx, case, log, bands_first, "LDS")


# ---- the launches of 64-frame tiles (1, 2 and 3)
@pytest.mark.parametrize("log,bands_first", TWO_MODES, ids=TWO_MODE_IDS)
@pytest.mark.parametrize("case", LIMIT_CROWDS, ids=case_id)
def test_a_launch_of_64_frame_tiles_gives_the_bits_of_32_frame_tiles(ctx, case, log, bands_first):
    """One row more than gives every CU two workgroups at 64 frames, T = 104: the last 64-frame tile holds 40 frames, its second row tile
    partly live.  (1024, 110) and (1024, 111) ask for 40 859 and 40 850 of the 40 960 floats; 1022 and 38 run the k loop's tail in the
    two-row-tile kernel, 1024 seventeen bin groups, 256 five.  Four rows against the truth; every row bit for bit against the same windows
    in launches of at most CUs / 2 rows, which take 32-frame tiles."""
    import torch
    n_fft, hop, n_mels = case
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    n, T, F = crowd_rows(cu), CROWD_T, limit_frames(hop, CROWD_T)
    chunk = cu // 2
    big, small = tile_plan(n_fft, hop, T, n, cu), tile_plan(n_fft, hop, T, chunk, cu)
    assert big[0] == 64 and small[0] == 32 and T == 1 + F // hop and 32 < T % 64 < 64
    assert n_fft != 1024 or big[1] == {110: 40859, 111: 40850}[hop]  # (of 40 960)
    rng = np.random.default_rng(7 * n_fft + hop)
    W = weights_for(n_fft, n_mels)
    Ls = F - rng.integers(0, F // 2, n)
    Ls[:4] = (F, F - 1, F // 3, 0)
    src = (rng.standard_normal(67 * n + F + 8) * 0.5).astype(np.float32)
    dst_rows = n + 3
    order = rng.permutation(dst_rows)[:n]
    rows = [(1 + 67 * i, int(Ls[i]), int(order[i])) for i in range(n)]  # (the windows lie 67 samples apart in one source: they overlap)
    d_src = torch.from_numpy(src).to("cuda:0")
    got = run(ctx, d_src, rows, dst_rows, F, n_fft, hop, n_mels, log, bands_first)
    unnamed_keep_the_sentinel(got, rows)
    truths = [logmel_truth(src[a: a + L], L, F, n_fft, hop, W) for a, L, _ in rows[:4]]
    worst = hold_to_the_truth(got, rows[:4], truths, log)
    print("error / bound crowd (%d, %d) %s, %d rows, 64-frame tiles, %d LDS floats: %.4f" % (n_fft, hop, "log10" if log else "power", n, big[1], worst))
    assert worst < 1.0
    again = run(ctx, d_src, rows, dst_rows, F, n_fft, hop, n_mels, log, bands_first, chunk=chunk)
    differ = np.nonzero((bits(got) != bits(again)).reshape(dst_rows, -1).any(axis=1))[0]
    assert differ.size == 0, "destination rows that depend on the tile: %s" % differ[:16]


# ---- 3. bin groups
@pytest.mark.parametrize("log,bands_first", TWO_MODES, ids=TWO_MODE_IDS)
@pytest.mark.parametrize("case", LIMIT_GROUPS, ids=case_id)
def test_transform_sizes_at_the_boundaries_of_the_bin_groups(ctx, case, log, bands_first):
    """n_fft 62: one group of exactly 32 bins (no padded column, power rows 33 floats apart); 126: two; 254: one per wave; 256: a fifth,
    which wave 0 takes in a second round.  Hop odd (no skew) and even"""
    five_lengths_against_the_truth(ctx, case, log, bands_first, "groups")


# ---- 4. small and extreme hops
@pytest.mark.parametrize("log,bands_first", TWO_MODES, ids=TWO_MODE_IDS)
@pytest.mark.parametrize("case", LIMIT_HOPS, ids=case_id)
def test_the_smallest_even_hops_and_hops_next_to_the_transform_size(ctx, case, log, bands_first):
    """hop 2 wraps on every k-step (sample i lies at i + i / 2), hop 4 on every second; at hop = n_fft a frame never wraps and
    the frames lie n_fft + 1 apart; hop = n_fft - 1 is the largest odd one, its frames overlapping in one sample"""
    five_lengths_against_the_truth(ctx, case, log, bands_first, "hops")


# ---- 5. the silent shortcut
def silent_edge_case(ctx, F, Ls, frame, silent_frames, log):
    """n_fft 64, hop 16, 32-frame tiles; one row per L, the last two real samples of each of magnitude 0.75, whatever lies behind them in
    the source random.  Ls: {L: whether `frame`'s tile is silent}."""
    import torch
    n_fft, hop, n_mels = 64, 16, 10
    T = 1 + F // hop
    assert tile_plan(n_fft, hop, T, len(Ls), torch.cuda.get_device_properties(0).multi_processor_count)[0] == 32
    rng = np.random.default_rng(F)
    W = weights_for(n_fft, n_mels, None)
    src = (rng.standard_normal(4 * F) * 0.5).astype(np.float32)
    rows = [(1 + i * (F + F % 2), L, 2 * i + 1) for i, L in enumerate(Ls)]  # (windows apart: a row's forced samples lie in no other row)
    for at, L, _ in rows:
        src[at + L - 2: at + L] = (0.75, -0.75)
    assert all(at % 2 == 1 and at + F <= src.size and abs(src[at + L]) > 0 for at, L, _ in rows)
    truths = [logmel_truth(src[at: at + L], L, F, n_fft, hop, W) for at, L, _ in rows]
    # on the truth alone: a frame that must not be silent is far from silent in some band, so the silence value cannot pass for it
    for (at, L, _), (M, e_M) in zip(rows, truths):
        if Ls[L]:
            assert (M[silent_frames] == 0).all() and (e_M[silent_frames] == 0).all(), L
        else:
            assert (M[frame] > 4 * e_M[frame]).any() and (M[frame] - e_M[frame] > 4 * FLOOR).any(), L
    got = run(ctx, torch.from_numpy(src).to("cuda:0"), rows, 2 * len(Ls) + 1, F, n_fft, hop, n_mels, log, True, norm=None)
    unnamed_keep_the_sentinel(got, rows)
    for (at, L, row), (M, e_M) in zip(rows, truths):
        if Ls[L]:
            assert (bits(got[row][silent_frames]) == silence_bits(log)).all(), L
        else:
            assert (bits(got[row][frame]) != silence_bits(log)).any(), L
    worst = hold_to_the_truth(got, rows, truths, log)
    print("error / bound silent edges F %d %s: %.4f" % (F, "log10" if log else "power", worst))
    assert worst < 1.0


@pytest.mark.parametrize("log", [False, True], ids=["power", "log10"])
def test_a_tile_of_zeros_whose_reflected_tail_reaches_a_real_sample_is_not_silent(ctx, log):
    """F = 512, T = 33: the last tile is frame 32 alone, its span the extended samples 480 .. 543, of which 512 .. 543 are the row's
    samples 510 down to 479.  L = 479: all zeros, silent.  L = 480: the tile's own samples are zeros and x[479] reaches frame 32 through
    the reflection alone, at m = 63.  L = 481: x[480] as well."""
    silent_edge_case(ctx, 512, {479: True, 480: False, 481: False}, 32, [32], log)


@pytest.mark.parametrize("log", [False, True], ids=["power", "log10"])
def test_a_tile_that_starts_at_the_first_zero_is_silent_and_one_two_samples_later_is_not(ctx, log):
    """F = 16 * 70 + 5, tiles at frames 0, 32, 64; the middle one's span starts at sample 480.  L = 479 and 480: frames 32 .. 70 are
    silent.  L = 482: frame 32 sees x[481] at m = 1 (481 would show nothing: x[480] meets only the window's exact zero w[0])."""
    silent_edge_case(ctx, 16 * 70 + 5, {479: True, 480: True, 482: False}, 32, list(range(32, 71)), log)


# ---- 6. a second descriptor with all waves working
def test_workgroups_take_a_second_descriptor_with_four_waves_at_work(ctx):
    """2100 rows (the grid's y holds 2048) at n_fft 256 -- five bin groups: every wave computes, wave 0 twice -- in a destination of 2200.
    The source behind every L is NaN and must not reach the output; rows not named keep the sentinel."""
    import torch
    n, dst_rows, F, n_fft, hop, n_mels = 2100, 2200, 200, 256, 64, 20
    T = 1 + F // hop
    rng = np.random.default_rng(6)
    stride = F + 3
    Ls = rng.integers(0, F + 1, n)
    Ls[:4] = (0, 1, F - 1, F)
    src = np.full(1 + n * stride, np.nan, dtype=np.float32)
    for i in range(n):
        src[1 + i * stride: 1 + i * stride + Ls[i]] = rng.standard_normal(Ls[i]) * 0.5
    order = rng.permutation(dst_rows)[:n]
    rows = [(1 + i * stride, int(Ls[i]), int(order[i])) for i in range(n)]
    W = weights_for(n_fft, n_mels)
    got = run(ctx, torch.from_numpy(src).to("cuda:0"), rows, dst_rows, F, n_fft, hop, n_mels, False, True)
    assert T == 4 and not np.isnan(got[order]).any()
    rest = np.setdiff1d(np.arange(dst_rows), order)
    assert rest.size == 100 and (bits(got[rest]) == SENTINEL).all()
    checked = sorted(set(range(0, n, 7)) | set(range(4)))
    assert n > 2048 and sum(i >= 2048 for i in checked) >= 7  # (rows of the grid's second round are among those checked)
    worst = 0.0
    for i in checked:
        at, L, row = rows[i]
        worst = max(worst, check_power(got[row], *logmel_truth(src[at: at + L], L, F, n_fft, hop, W)))
    print("error / bound second descriptor (256, 64): %.4f" % worst)
    assert worst < 1.0


# ---- 7. one Inf inside a window
@pytest.mark.parametrize("n_fft,hop,n_mels", [(400, 160, 80), (34, 5, 6)], ids=["400_160", "34_5"])
def test_one_infinity_reaches_exactly_the_frames_that_cover_it(ctx, n_fft, hop, n_mels):
    """The DFT is a matrix product with frames as rows: an Inf at sample p (the middle of the first tile, far from both reflections) makes
    the frames that cover p non-finite in every band -- Inf, or NaN where it meets a zero coefficient -- and changes no bit of any other
    frame, nor of a second row of the launch whose samples end before p."""
    import torch
    T = 71
    F, p = limit_frames(hop, T), 16 * hop + 2
    t0 = np.arange(T) * hop - n_fft // 2
    covers = (t0 <= p) & (p < t0 + n_fft)
    assert n_fft < p < F - n_fft and 2 <= covers.sum() <= 1 + n_fft // hop and not covers[:8].any() and not covers[31:].any()
    W = weights_for(n_fft, n_mels)
    src = (np.random.default_rng(n_fft).standard_normal(2 * F) * 0.5).astype(np.float32)
    rows = [(1, F, 2), (3, p - 5, 0)]
    assert rows[1][0] + rows[1][1] <= rows[0][0] + p  # (the second row ends before p)
    M, e_M = logmel_truth(src[1: 1 + F], F, F, n_fft, hop, W)
    dirty = src.copy()
    dirty[rows[0][0] + p] = np.inf
    for log in (False, True):
        a = run(ctx, torch.from_numpy(src).to("cuda:0"), rows, 4, F, n_fft, hop, n_mels, log, True)
        b = run(ctx, torch.from_numpy(dirty).to("cuda:0"), rows, 4, F, n_fft, hop, n_mels, log, True)
        unnamed_keep_the_sentinel(b, rows)
        assert np.isfinite(a[[0, 2]]).all()
        assert (check_log(a[2], M, e_M, FLOOR) if log else check_power(a[2], M, e_M)) < 1.0
        assert (bits(a[2][~covers]) == bits(b[2][~covers])).all(), "an Inf reached a frame that does not cover it"
        assert not np.isfinite(b[2][covers]).any(), "a frame that covers the Inf has a finite band"
        assert (bits(a[0]) == bits(b[0])).all(), "an Inf reached a row that ends before it"


# ---- 8. scaling by a power of two
@pytest.mark.parametrize("n_fft,hop,n_mels", [(400, 160, 80), (1022, 110, 40)], ids=["400_160", "1022_110"])
def test_scaling_the_samples_by_a_power_of_two_shifts_the_exponent_only(ctx, n_fft, hop, n_mels):
    """Every step from sample to power output is a float32 multiply-add without an absolute term (the MFMA's k-ordered fmaf chain, re^2 +
    im^2, the band's fmaf chain), so x * 2^+-12 gives the output of x with its exponent shifted by +-24, bit for bit, as long as nothing
    leaves the normal range: by the truth every non-zero M * 2^-24 stays above 2^-120 (and M * 2^24 below 2^120)."""
    import torch
    T = 71
    F = limit_frames(hop, T)
    src, rows, truths = five_lengths(n_fft, hop, F, n_mels)
    for M, e_M in truths:
        assert (M[M > 0] * 2.0 ** -24 > 2.0 ** -120).all() and (M * 2.0 ** 24 < 2.0 ** 120).all()
    named = [row for _, _, row in rows]
    base = run(ctx, torch.from_numpy(src).to("cuda:0"), rows, DST_ROWS, F, n_fft, hop, n_mels, False, True)
    assert hold_to_the_truth(base, rows, truths, False) < 1.0
    for e in (12, -12):
        scaled = np.ldexp(src, e).astype(np.float32)
        assert (np.ldexp(scaled, -e) == src).all()
        got = run(ctx, torch.from_numpy(scaled).to("cuda:0"), rows, DST_ROWS, F, n_fft, hop, n_mels, False, True)
        unnamed_keep_the_sentinel(got, rows)
        want = np.ldexp(np.ascontiguousarray(base[named]), 2 * e).astype(np.float32)
        assert (bits(got[named]) == bits(want)).all(), "x * 2^%d: %d outputs differ in more than the exponent" % (e, int((bits(got[named]) != bits(want)).sum()))
