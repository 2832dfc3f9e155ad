"""vpz_pcm_fbank (csrc/pcm_fbank.hip) at the limits of its launches: the hops, window lengths, bin groups, LDS budgets and grid rounds that
tests/test_pcm_fbank_gpu.py never ran, each at the smallest shape that reaches it.

TRUTH and BOUND are those of test_pcm_fbank_gpu.py, unchanged: fbank_truth.fbank_truth in float64 with check_row, check_power and
check_log and their bound e_M.  The cases are fbank_cases.py's; test_fbank_cpu.py holds each to the shape it is named for.  Every shape
case runs in power and log mode over rows of F, F - 1, F / 3, win and win - 1 samples.

THE CASES, and the lines of the kernel each is there for:
  hops and small windows   hop 2, 3, 6 and win - 1: `step_a` wraps at every k-step and the mean loop's `while (rem >= hop)` twice per term;
                       win 3, 4, 5: mean lanes with no term, `blocks == 0` with and without `if (win & 1)`; win 8 and 9: one look-ahead
                       block that "loads itself again"; win 33: whole blocks plus the odd sample; with remove_dc on and off
  bin groups           nb = 32, 33, 64, 65, 128, 129: `for (k0 = wave * kFbCols; k0 < nb; ...)` and `k < nb` at one full group, a
                       second of one live column, each wave exactly once, a wave's second round; nb 129 also in 64-frame tiles
  empty bands, floor   `cnt == 0` (power 0, log the floor's bits) and `acc <= a.floor` from exact silence
  LDS limits           n_fft 1024 in 64- and 32-frame tiles with the whole budget of 40 960 floats, and one step beyond either
  second round         `r += gridDim.y` with four waves at work: `mean[]`, the span and the power tile written again for the next
                       descriptor behind two barriers; descriptors of `nr <= 0` in front of, behind and (three rounds) between real ones
  long row             more than a thousand tiles of one row
  non-finite           the rule include/vorbispizza_pcm_fbank.h states, in 32- and 64-frame tiles
  scaling              a power of two on the samples, in `scale`, or on the output: the same bytes

Largest error / bound observed on an MI355X (test_zz_the_largest_ratio_of_this_file prints them; the file takes 3.6 s there):
hops and small windows 0.119 power / 0.499 log, bin groups 0.034 / 0.149, empty bands 0.085 / 0.335, silence 0 / 0, LDS limits 0.0064 /
0.0146, rounds of the grid 0.0147, long row 0.192, scaling 0.0047."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fbank_cases as fc  # noqa: E402
import fbank_truth as ft  # noqa: E402
import fbank_cases as first  # noqa: E402
from fbank_cases import launch  # noqa: E402
from pcm_support import SENTINEL, place, signal  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

WORST = {}


def note(key, ratio):
    """test_pcm_fbank_gpu.note, and this file's own record beside it"""
    first.note(key, ratio)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_shape(ctx, key, d, F):
    """test_shapes' rows: a full one, one sample short, a third (pad-only tiles behind it), one frame exactly, one sample short of a frame"""
    win, hop = d["win"], d["hop"]
    T = ft.n_frames(F, win, hop)
    assert T % 16 != 0 and (F - win) % hop != 0
    Ls = [F, F - 1, F // 3, win, win - 1]
    windows = [signal(L, 7 * i + win + hop, d["sample_rate"]) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    order = [4, 0, 5, 2, 6]
    got = launch(ctx, d, src, [(o, L, r) for o, L, r in zip(offs, Ls, order)], 7, F)
    assert got.shape == (7, T, d["n_mels"]) and (got[[1, 3]].view(np.uint32) == SENTINEL).all()
    W, B = ft.mel_weights64(d), ft.operator64(d)
    for w, L, r in zip(windows, Ls, order):
        note(key, ft.check_row(got[r], w, d, W, B))
    return got, order


@pytest.mark.parametrize("log", [False, True], ids=["power", "log"])
@pytest.mark.parametrize("remove_dc", [True, False], ids=["dc_removed", "dc_kept"])
@pytest.mark.parametrize("name", list(fc.SMALL))
def test_hops_and_small_windows(ctx, name, remove_dc, log):
    change, F = fc.small(name)
    run_shape(ctx, "hops and small windows %s" % ("log" if log else "power"), ft.spec_of(log=log, remove_dc=remove_dc, **change), F)


@pytest.mark.parametrize("log", [False, True], ids=["power", "log"])
@pytest.mark.parametrize("name", list(fc.GROUPS))
def test_bin_groups(ctx, name, log):
    change, F = fc.group(name)
    run_shape(ctx, "bin groups %s" % ("log" if log else "power"), ft.spec_of(log=log, **change), F)


def crowded(ctx, key, d, F, num_cu, tile, tile_few, checked=10):
    """max(600, 2 CUs + 8) rows that overlap in the source, 67 samples apart, of all lengths -- the tile asserted through tile_plan;
    `checked` of them against the truth; the same windows in a launch of few rows (another tile): the same bits"""
    import torch
    k = ft.kernel_constants(ROOT)
    win, hop, n_fft = d["win"], d["hop"], d["n_fft"]
    T = ft.n_frames(F, win, hop)
    crowd = fc.crowd_rows(num_cu)
    assert ft.tile_plan(win, hop, n_fft, T, crowd, num_cu, k)[0] == tile and ft.tile_plan(win, hop, n_fft, T, checked, num_cu, k)[0] == tile_few
    host = signal(crowd * 67 + F + 8, win + hop, d["sample_rate"])
    src = torch.from_numpy(host).to("cuda:0")
    rng = np.random.default_rng(win * hop)
    Ls = rng.integers(0, F + 1, crowd)
    Ls[:5] = (F, F - 1, F // 3, win, win - 1)
    order = rng.permutation(crowd + 3)[:crowd]
    rows = [(1 + 67 * i, int(Ls[i]), int(order[i])) for i in range(crowd)]
    big = launch(ctx, d, host, rows, crowd + 3, F, src)
    rest = np.setdiff1d(np.arange(crowd + 3), order)
    assert rest.size == 3 and (big[rest].view(np.uint32) == SENTINEL).all()
    W, B = ft.mel_weights64(d), ft.operator64(d)
    some = list(range(5)) + list(range(5 + 59, crowd, crowd // (checked - 5)))[: checked - 5]
    for i in some:
        a, L, r = rows[i]
        note(key, ft.check_row(big[r], host[a: a + L], d, W, B))
    few = launch(ctx, d, host, [(rows[i][0], rows[i][1], j) for j, i in enumerate(some)], len(some), F, src)
    for j, i in enumerate(some):
        assert few[j].tobytes() == big[rows[i][2]].tobytes(), i


@pytest.mark.parametrize("log", [False, True], ids=["power", "log"])
def test_a_second_round_of_a_wave_in_tiles_of_64(ctx, num_cu, log):
    change, F = fc.group(fc.CROWDED_GROUP)
    crowded(ctx, "bin groups %s" % ("log" if log else "power"), ft.spec_of(log=log, **change), F, num_cu, 64, 32)


@pytest.mark.parametrize("log", [False, True], ids=["power", "log"])
def test_bands_with_no_bin(ctx, log):
    from vorbispizza_amd import capi
    d = ft.spec_of(log=log, **fc.EMPTY_BANDS)
    _, count, _ = capi.fbank_filterbank(capi.FbankSpec.make(**d))
    assert (count == 0).sum() > 200 and (count > 0).any()
    F = 32 + 8 * 70 + 1
    got, order = run_shape(ctx, "empty bands %s" % ("log" if log else "power"), d, F)
    real = got[order[0]][:, count == 0]  # (the full row: every frame is real)
    want = ft.log_floor(d["floor"]).view(np.uint32) if log else 0
    assert real.size > 200 * 71 and (real.view(np.uint32) == want).all()
    assert (got[order[0]][:, count > 0].view(np.uint32) != want).any()


@pytest.mark.parametrize("log", [False, True], ids=["power", "log"])
def test_silence_and_a_constant_are_zero_power_exactly(ctx, log):
    """an all-zero row with and without remove_dc, and a constant row of 0.5 with it: every partial sum of the mean is a multiple of 0.5
    below 2^24 and 200 / 400 is exact, so x - mu is 0 and the power +0.0 bit for bit; the log output is the floor's bits"""
    F = 400 + 160 * 18 + 7
    want = ft.log_floor(ft.DEFAULTS["floor"]).view(np.uint32) if log else 0
    for value, remove_dc in ((0.0, True), (0.0, False), (0.5, True)):
        d = ft.spec_of(n_mels=23, log=log, remove_dc=remove_dc, scale=1.0)
        w = np.full(F, value, dtype=np.float32)
        src, offs = place([w, w[:1000]])
        got = launch(ctx, d, src, [(offs[0], F, 1), (offs[1], 1000, 0)], 2, F)
        assert got.shape[1] == 19 and (got[1].view(np.uint32) == want).all() and (got[0, :4].view(np.uint32) == want).all()
        for r, x in ((1, w), (0, w[:1000])):
            note("silence %s" % ("log" if log else "power"), ft.check_row(got[r], x, d))


@pytest.mark.parametrize("log", [False, True], ids=["power", "log"])
@pytest.mark.parametrize("win_hop", list(fc.LDS_LIMITS), ids=["%d_%d" % wh for wh in fc.LDS_LIMITS])
def test_the_lds_limits_at_n_fft_1024(ctx, num_cu, win_hop, log):
    k = ft.kernel_constants(ROOT)
    T, tile, floats, tile_few = fc.LDS_LIMITS[win_hop]
    change, F = fc.lds_limit(*win_hop)
    d = ft.spec_of(log=log, **change)
    key = "lds limits %s" % ("log" if log else "power")
    assert ft.tile_plan(d["win"], d["hop"], 1024, T, fc.crowd_rows(num_cu), num_cu, k) == (tile, floats) and floats <= k["kFbLdsFloats"]
    if tile == 64 or win_hop == (1024, 112):  # (a crowd: 64 frames are chosen, or are too many for the LDS where the crowd asks for them)
        crowded(ctx, key, d, F, num_cu, tile, tile_few)
    else:
        assert fc.tile_of(change, F, 5, num_cu, k)[0] == tile
        run_shape(ctx, key, d, F)


@pytest.mark.parametrize("n", [2100, 4200], ids=["two_rounds", "three_rounds"])
def test_rounds_of_the_grid_with_four_waves_at_work(ctx, n):
    """(200, 80, 256, 40), remove_dc, T = 3: a workgroup goes on to descriptor i + 2048 (and i + 4096) with all four waves computing;
    real, empty and shorter-than-win descriptors follow one another in one workgroup.  NaN behind every row's L; rows nobody names keep
    the sentinel"""
    k = ft.kernel_constants(ROOT)
    d = ft.spec_of(log=False, scale=1.0, **fc.SECOND_ROUND)
    win, hop, F = d["win"], d["hop"], 397
    assert ft.n_frames(F, win, hop) == 3 and n > k["kFbMaxGridY"] and (n < 2 * k["kFbMaxGridY"]) == (n == 2100)
    rng = np.random.default_rng(3)
    Ls = fc.second_round_lengths(n, F, win, rng)
    stride, dst_rows = F + 3, n + 100
    src = np.full(1 + n * stride, np.nan, dtype=np.float32)
    x = (0.5 * rng.standard_normal((n, F)) + 0.1).astype(np.float32)
    for i in range(n):
        src[1 + i * stride: 1 + i * stride + Ls[i]] = x[i, : Ls[i]]
    order = rng.permutation(dst_rows)[:n]
    got = launch(ctx, d, src, [(1 + i * stride, int(Ls[i]), int(order[i])) for i in range(n)], dst_rows, F)
    assert not np.isnan(got[order]).any()
    rest = np.setdiff1d(np.arange(dst_rows), order)
    assert rest.size == 100 and (got[rest].view(np.uint32) == SENTINEL).all()
    W, B = ft.mel_weights64(d), ft.operator64(d)
    last_round = n - n % k["kFbMaxGridY"]
    checked = sorted(set(range(0, n, 7)) | set(range(8)) | set(range(2048, 2056)) | set(range(last_round, n)))
    for i in checked:
        note("rounds of the grid", ft.check_row(got[order[i]], x[i, : Ls[i]], d, W, B))


def test_a_long_row(ctx, num_cu):
    change, F = fc.LONG_ROW
    d = ft.spec_of(log=False, **change)
    w = signal(F, 12)
    src, offs = place([w])
    got = launch(ctx, d, src, [(offs[0], F, 0)], 1, F)
    assert got.shape == (1, 70000, 1)
    note("long row", ft.check_row(got[0], w, d))


@pytest.mark.parametrize("log", [False, True], ids=["power", "log"])
@pytest.mark.parametrize("remove_dc", [True, False], ids=["dc_removed", "dc_kept"])
@pytest.mark.parametrize("tile", [32, 64])
def test_a_sample_that_is_not_finite(ctx, num_cu, tile, remove_dc, log):
    """the header's rule: one NaN, then one +Inf, at sample p of row 3 of eight.  Exactly the frames t with t * hop <= p < t * hop + win
    are not finite, in every band that has a bin; every other frame of the row -- its neighbours in the same 32-frame MFMA tile among
    them -- and every other row are the same bits as without it"""
    import torch
    from vorbispizza_amd import capi
    k = ft.kernel_constants(ROOT)
    d = ft.spec_of(win=200, hop=80, n_fft=256, n_mels=20, sample_rate=8000, remove_dc=remove_dc, log=log, scale=1.0)
    win, hop = 200, 80
    T = 100 if tile == 32 else 64 * ((2 * num_cu) // 8 + 1) - 23
    F = win + hop * (T - 1) + 5
    assert ft.tile_plan(win, hop, 256, T, 8, num_cu, k)[0] == tile
    _, count, _ = capi.fbank_filterbank(capi.FbankSpec.make(**d))
    assert (count > 0).sum() >= 18
    Ls = [F, F - 1, F // 3, F, win, F - hop, 0, F]
    host = signal(8 * (F + 8), 21, 8000)
    starts = [3 + i * (F + 8) - (i % 2) for i in range(8)]
    rows = [(a, L, r) for a, L, r in zip(starts, Ls, (5, 1, 7, 0, 3, 6, 2, 4))]
    clean = launch(ctx, d, host, rows, 8, F, torch.from_numpy(host).to("cuda:0"))
    assert np.isfinite(clean).all()
    p = 45 * hop + 3
    frames = [t for t in range(T) if t * hop <= p < t * hop + win]
    assert frames == [43, 44, 45]  # (the middle of the tile's second 32 frames)
    hit = np.zeros(clean.shape, dtype=bool)
    hit[0, 43:46, :] = count > 0
    for value in (np.nan, np.inf):
        dirty_host = host.copy()
        dirty_host[starts[3] + p] = value
        dirty = launch(ctx, d, dirty_host, rows, 8, F, torch.from_numpy(dirty_host).to("cuda:0"))
        assert not np.isfinite(dirty[hit]).any() and hit.sum() == 3 * (count > 0).sum()
        assert dirty[~hit].tobytes() == clean[~hit].tobytes()


@pytest.mark.parametrize("e", [12, -12])
def test_a_power_of_two_on_the_samples_in_the_scale_or_on_the_output(ctx, e):
    """power mode, remove_dc on: the input times 2^e with scale 1, the input with scale 2^e, and the input with scale 1 and its output
    times 2^2e on the host are the same bytes (every operation scales exactly; nothing is near underflow)"""
    F = 400 + 160 * 34 + 11
    Ls = [F, F - 161, 1000]
    windows = [signal(L, 60 + i) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    rows = [(o, L, r) for o, L, r in zip(offs, Ls, (2, 0, 1))]
    d = ft.spec_of(n_mels=23, log=False, remove_dc=True, scale=1.0)
    plain = launch(ctx, d, src, rows, 3, F)
    by_input = launch(ctx, d, np.ldexp(src, e).astype(np.float32), rows, 3, F)
    by_scale = launch(ctx, dict(d, scale=2.0 ** e), src, rows, 3, F)
    assert (plain[0, :30] > 0).all() and np.isfinite(plain).all()
    assert by_input.tobytes() == by_scale.tobytes() == np.ldexp(plain, 2 * e).astype(np.float32).tobytes()
    for w, (_, L, r) in zip(windows, rows):
        note("scaling", ft.check_row(by_scale[r], w, dict(d, scale=2.0 ** e)))


def test_zz_the_largest_ratio_of_this_file():
    """the record lines of the module's docstring come from here (run with -s)"""
    assert WORST and max(WORST.values()) < 1.0
    for key in sorted(WORST):
        print("largest error / bound  %-40s %.4f" % (key, WORST[key]))
