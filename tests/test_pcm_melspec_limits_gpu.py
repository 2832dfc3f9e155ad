"""vpz_pcm_melspec (csrc/pcm_melspec.hip) held to its float32 restatement BIT FOR BIT, at every transform size and at the limits of its
launch plan.  tests/test_pcm_melspec_gpu.py holds the kernel to the float64 truth within e_M, where it sits at a fifth of the bound: a
changed rounding, another order of a band's sum or a contracted multiply-add passes there (tests/test_melspec_cpu.py shows it:
test_the_bit_check_tells_what_the_bound_does_not).  Here the power output is melspec_truth.restated_power32 as raw bits -- network32 on
the float32 frames, P = fma32(re, re, im * im), one fma32 chain per band over the library's own bank, k ascending from 0.0 -- and the
log10 output obeys check_log_exact against those values: the silence value's bits at and under float32(floor), 4 u max(1, |v|) above it,
no element exempt.

The cases are melspec_truth.CASES and LIMIT_CASES (tests/test_melspec_cpu.py holds both lists to the plan):
    tile16_last_4096_1638   16-frame tile, 40 954 LDS floats, T 17      tile16_last_8192_819   16-frame tile, 40 957, T 17
    tile8_first_4096_1639    8-frame tile, T 9                          tile8_first_8192_820    8-frame tile, T 9
    tile8_last_4096_3803     8-frame tile, 40 957 (the 4096            full_lds_8192_2048_T7, _T8, _T9
                             kernel's most), T 9                                                8-frame tile, 40 960: the whole 160 KiB
    tile2_first_4096_3804    2-frame tile, T 3, empty bands             tile2_first_8192_2049   2-frame tile, T 3
Rows of L = F, F - 1, F - n_fft / 4, F // 3, 1 and 0, each alone in the source at an odd offset with NaN behind it.

Observed on an MI355X: every power value of every case, in both layouts, equals the restatement in bits; no case failed and none was
left out.  Largest error / bound against the float64 truth over LIMIT_CASES: 0.103 (power, full_lds_8192_2048_T7) and 0.114 (log10,
tile2_first_4096_3804); over CASES 0.162 and 0.182, as tests/test_pcm_melspec_gpu.py has them.  log10f of the restated power: at most
0.688 of the 4 u max(1, |v|) allowed (smallest_2048_hop_1; 0.687 at full_lds_8192_2048_T7), 0.641 with the floor at the median (about
70 % of the values at or under it), 0.697 over the 2 100 rows at 8192."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import melspec_truth as mt  # noqa: E402
from logmel_truth import check_log, check_power, frames_of, silence_value  # noqa: E402
from pcm_support import SENTINEL, guarded, rows_back  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

FLOOR = mt.FLOOR
DST_ROWS = mt.DST_ROWS
ALL_CASES = list(mt.CASES) + list(mt.LIMIT_CASES)


def alone_with_nan_behind(windows):
    """(src, offsets): every window alone in one source array at an odd offset, NaN in front of, between and behind them"""
    offs, at = [], 1
    for w in windows:
        offs.append(at)
        at += len(w) + 3
        at += (at + 1) % 2
    src = np.full(at + 8, np.nan, dtype=np.float32)
    for o, w in zip(offs, windows):
        src[o: o + len(w)] = w
    assert all(o % 2 == 1 for o in offs)
    return src, offs


_SOURCES = {}


def case_source(name):
    """(device source, rows) of a case: case_input's windows, moved apart so that NaN stands behind every L"""
    import torch
    if name not in _SOURCES:
        src, rows = mt.case_input(name)
        placed, offs = alone_with_nan_behind([src[a: a + L] for a, L, _ in rows])
        assert np.isnan(placed).sum() >= 4 * len(rows) and all(np.isnan(placed[o + L]) and np.isnan(placed[o - 1]) for o, (_, L, _) in zip(offs, rows))
        _SOURCES[name] = (placed, [(o, L, row) for o, (_, L, row) in zip(offs, rows)])
    placed, rows = _SOURCES[name]
    return torch.from_numpy(placed).to("cuda:0"), rows


def run(ctx, spec, d_src, rows, dst_rows, F):
    """[row][T][n_mels] float32 of one launch into a guarded destination of sentinels"""
    from vorbispizza_amd import capi
    T, n_mels = 1 + F // spec.hop, spec.n_mels
    bands_first = spec.layout == capi.MEL_BANDS_FIRST
    whole, dst = guarded(dst_rows, n_mels * T)
    assert capi.pcm_melspec(ctx, d_src, rows, dst.view((dst_rows, n_mels, T) if bands_first else (dst_rows, T, n_mels)), spec, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    return rows_back(whole, dst_rows, n_mels, T, bands_first)


def same_bits(got, want, what):
    differ = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert differ[0].size == 0, "%s: first of %d: frame %d band %d, %r against the restated %r" % (
        what, differ[0].size, differ[0][0], differ[1][0], got[differ][0], want[differ][0])


@pytest.mark.parametrize("bands_first", [True, False], ids=["bands_first", "frames_first"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_rows_are_the_restatement_bit_for_bit(ctx, name, bands_first):
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = mt.case_of(name)
    assert mt.tile_plan(n_fft, hop)[0] == tile
    d_src, rows = case_source(name)
    restated, truths = mt.case_restated(name), mt.case_truth(name)
    named = {row for _, _, row in rows}
    silence = silence_value(FLOOR)
    worst = {}
    for log in (False, True):
        got = run(ctx, mt.case_spec(name, log, bands_first, FLOOR), d_src, rows, DST_ROWS, F)
        for r in range(DST_ROWS):
            if r not in named:
                assert (got[r].view(np.uint32) == SENTINEL).all(), r
        assert not np.isnan(got[sorted(named)]).any()
        for (at, L, row), acc32, (M, e_M) in zip(rows, restated, truths):
            if log:
                worst["exact"] = max(worst.get("exact", 0.0), mt.check_log_exact(got[row], acc32, FLOOR))
                worst["log10"] = max(worst.get("log10", 0.0), check_log(got[row], M, e_M, FLOOR))
            else:
                same_bits(got[row], acc32, "%s row %d (L = %d)" % (name, row, L))
                worst["power"] = max(worst.get("power", 0.0), check_power(got[row], M, e_M))
            if L == 0:
                assert (got[row].view(np.uint32) == (silence.view(np.uint32) if log else 0)).all()
    print("error / bound %s: power %.4f, log10 %.4f; log10 against the restated power / (4 u max(1, |v|)) %.4f" % (
        name, worst["power"], worst["log10"], worst["exact"]))
    assert worst["power"] < 1.0 and worst["log10"] < 1.0 and worst["exact"] <= 1.0


@pytest.mark.parametrize("name", ["librosa_2048_512_T17", "tile8_last_4096_3803", "full_lds_8192_2048_T9"])
def test_the_floor_inside_computed_tiles(ctx, name):
    """The floor at the median of the case's restated non-zero power values -- taken from the restatement, never from the launch --, and
    once more at a double next to it that float32 does not represent: acc <= floor picks the silence value for about half of the values
    of tiles that were computed, and every element obeys check_log_exact"""
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = mt.case_of(name)
    d_src, rows = case_source(name)
    restated = mt.case_restated(name)
    values = np.concatenate([acc32.ravel() for acc32 in restated])
    live = np.sort(values[values != 0])
    median = float(live[live.size // 2])  # (one of the values: where the count is even, the upper of the middle two)
    for floor in (median, median * (1 + 2.0 ** -30)):
        assert float(np.float32(floor)) == median and (floor == median or float(np.float32(floor)) != floor)
        share = (values <= np.float32(floor)).mean()
        assert 0.25 <= share <= 0.75, share
        # and the computed tiles themselves are split: frames that see samples, values on either side
        full = restated[0]
        assert (full > 0).all() and 0.25 <= (full <= np.float32(floor)).mean() <= 0.75
        worst = 0.0
        for bands_first in (True, False):
            got = run(ctx, mt.case_spec(name, True, bands_first, floor), d_src, rows, DST_ROWS, F)
            for (at, L, row), acc32 in zip(rows, restated):
                worst = max(worst, mt.check_log_exact(got[row], acc32, floor))
        print("floor %r in %s: %.1f %% at or under it, log10 / (4 u max(1, |v|)) %.4f" % (floor, name, 100 * share, worst))


def test_more_descriptors_than_the_grid_holds_at_8192(ctx):
    """2100 rows of F = 4097 at n_fft 8192, hop 8192 -- one frame per row, the 2-frame tile; the grid's y holds 2048: workgroups of the
    8192 kernel take a second descriptor -- in a destination of 2150 rows, power frames-first and log10 bands-first.  Every named row
    is the restatement (bits / check_log_exact), rows not named keep the sentinel, and NaN stands behind every L."""
    import torch
    from vorbispizza_amd import capi
    n, dst_rows, F, n_fft, hop, n_mels = 2100, 2150, 4097, 8192, 8192, 64
    T = 1 + F // hop
    assert T == 1 and n > mt.kernel_constants()["kMsMaxGridY"] and mt.tile_plan(n_fft, hop)[0] == 2
    rng = np.random.default_rng(8192)
    Ls = rng.integers(0, F + 1, n)
    Ls[:4] = (F, 0, 1, F - 1)
    x = [(rng.standard_normal(L) * 0.5).astype(np.float32) for L in Ls]
    src, offs = alone_with_nan_behind(x)
    order = rng.permutation(dst_rows)[:n]
    rows = [(int(offs[i]), int(Ls[i]), int(order[i])) for i in range(n)]
    rest = np.setdiff1d(np.arange(dst_rows), order)
    assert rest.size == 50
    frames = np.concatenate([frames_of(x[i], int(Ls[i]), F, n_fft, hop) for i in range(n)]).astype(np.float32)
    assert frames.shape == (n, n_fft)
    d_src = torch.from_numpy(src).to("cuda:0")
    make = dict(sample_rate=22050, n_fft=n_fft, hop=hop, n_mels=n_mels, floor=FLOOR)
    first, count, weights = capi.melspec_filterbank(capi.LogMelSpec.make(log=False, **make))
    want = mt.restated_power32(frames, n_fft, first, count, weights)
    assert (want[1] == 0).all() and (want[0] > FLOOR).all()
    for log, bands_first in ((False, False), (True, True)):
        got = run(ctx, capi.LogMelSpec.make(log=log, bands_first=bands_first, **make), d_src, rows, dst_rows, F)
        assert (got[rest].view(np.uint32) == SENTINEL).all()
        named = got[order][:, 0, :]
        assert not np.isnan(named).any()
        if log:
            print("2100 rows at 8192: log10 / (4 u max(1, |v|)) %.4f" % mt.check_log_exact(named, want, FLOOR))
        else:
            same_bits(named, want, "2100 rows at 8192")


@pytest.mark.parametrize("n_fft,hops,tiles", [(4096, (1024, 2048, 4096), (16, 8, 2)), (8192, (512, 1024, 2048, 4096), (16, 8, 8, 2))])
def test_bits_do_not_depend_on_the_tile(ctx, n_fft, hops, tiles):
    """One window of L = F samples in launches whose hops make the plan take the 16-, the 8- and the 2-frame tile (at 8192 the hop 2048
    still takes 8 frames -- with the whole LDS --, so the 2-frame launch is the one at 4096): the frames the launches share -- those at
    the sample positions of the widest hop -- carry the same bits, in every band, and those are the restatement's; among them the
    frames that read no padding on either side"""
    import torch
    from vorbispizza_amd import capi
    n_mels, widest = 128, hops[-1]
    assert tuple(mt.tile_plan(n_fft, h)[0] for h in hops) == tiles and all(widest % h == 0 for h in hops)
    F = widest * 4 + 5
    x = (np.random.default_rng(n_fft + 1).standard_normal(F) * 0.5).astype(np.float32)
    src, offs = alone_with_nan_behind([x])
    d_src = torch.from_numpy(src).to("cuda:0")
    make = dict(sample_rate=44100, n_fft=n_fft, n_mels=n_mels, log=False)
    first, count, weights = capi.melspec_filterbank(capi.LogMelSpec.make(hop=widest, **make))
    want = mt.restated_power32(frames_of(x, F, F, n_fft, widest).astype(np.float32), n_fft, first, count, weights)
    positions = np.arange(want.shape[0]) * widest
    inside = (positions >= n_fft // 2) & (positions + n_fft // 2 <= F)
    assert want.shape[0] == 5 and inside.sum() >= 2 and not inside.all()
    for h in hops:
        got = run(ctx, capi.LogMelSpec.make(hop=h, bands_first=h != hops[1], **make), d_src, [(offs[0], F, 0)], 1, F)[0]
        assert got.shape == (1 + F // h, n_mels) and got.shape[0] > mt.tile_plan(n_fft, h)[0]  # (more than one tile)
        same_bits(got[:: widest // h], want, "n_fft %d hop %d" % (n_fft, h))
