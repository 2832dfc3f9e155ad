"""vpz_pcm_resample at the limits of its ratios and channel counts: every branch of the launch plan, and the long filters EXACTLY.

tests/test_pcm_resample_gpu.py runs friendly ratios; here are the steepest ones (388 taps, a span that fills the LDS stage, one channel to
a pass), every number of channels to a pass, passes with a narrower last one, 255 channels, up = 1024.  The case list is
tests/test_resample_cpu.py's LIMIT_CASES, which a test without a GPU holds to a restatement of the plan.

Three kinds of test:
  random data   the contract of test_every_named_row_is_the_resampled_window_then_zeros (the float64 restatement within the derived bound,
                zero bits behind J, guards and unnamed rows untouched, the layouts bit for bit) for every case of the list;
  impulses      the derived bound is loose where the filter is long -- a dropped outermost tap is 1e-7 of the sum --, so a window of zeros
                with single samples of 1.0 further apart than the filter is long gives back entries of vpz_resample_filter's table, which
                are compared with ==: 1.0 * h and the fused adds of zeros are exact.  The test counts the (phase, tap) pairs it has seen;
  non-finite    what lies around a window is never read, not even as 0 * value: infinities and NaNs around the windows change no bit,
                and one inside a window reaches exactly the outputs whose taps lie on it.
The truth is never the call under test."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pcm_support import (RESAMPLE_DST_ROWS as DST_ROWS, INTERLEAVED, INTERLEAVED_S16, PLANAR, PLANAR_S16, guarded_layout as guarded,
    layout_windows, out_len, random_source, rows_of, run_layouts)
from resample_truth import LIMIT_CASES, filter_table, launch_plan, live_taps, passes_text, resample_truth  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def length_for(J, up, down):
    """the shortest window with at least J outputs (exactly J wherever down >= up)"""
    L = max((J - 1) * down // up, 0)
    while out_len(L, up, down) < J:
        L += 1
    return L


def limit_lengths(up, down):
    """shorter than the filter, around one period of the phases, either side of a tile's edge, two and a half tiles; fewer outputs than
    phases where up is large.  (1024, 1): 0 to 4 samples only, 16 tiles from four source samples"""
    if (up, down) == (1024, 1):
        return [0, 1, 2, 3, 4]
    Ls = [0, 1, 2, down - 1, down, down + 1] + [length_for(J, up, down) for J in (255, 256, 257, 640)]
    if down >= up:
        assert [out_len(L, up, down) for L in Ls[6:]] == [255, 256, 257, 640]
    if up >= 1023:
        Ls.append(length_for(up - 1, up, down))
        assert 768 < out_len(Ls[-1], up, down) < up  # (three tiles and more, and not every phase)
    Ls = list(dict.fromkeys(L for L in Ls if L >= 0))
    assert len(Ls) <= DST_ROWS
    return Ls


def run_once(ctx, src_np, rows, channels, downmix, up, down, frames, layout=PLANAR, guard=5, dst_rows=DST_ROWS):
    """one float32 call -> the destination as [row][frame][channel]; the guards keep their sentinel and the source keeps its bits"""
    import torch
    from vorbispizza_amd import capi
    assert src_np.size % channels == 0 and layout in (PLANAR, INTERLEAVED)
    src = torch.from_numpy(src_np).to("cuda:0").view(-1, channels)
    co = 1 if downmix else channels
    whole, dst, flat = guarded(dst_rows, co, frames, layout, guard)
    assert capi.pcm_resample(ctx, src, rows, dst, layout, up, down, downmix) == capi.OK, ctx.last_error()
    ctx.synchronize()
    img, g0, g1 = rows_of(whole, guard, dst_rows, co, frames, layout)
    assert (g0 == flat[0]).all() and (g1 == flat[0]).all(), "a guard was written"
    assert src.cpu().numpy().reshape(-1).view(np.uint32).tobytes() == src_np.view(np.uint32).tobytes(), "the source was written"
    return np.ascontiguousarray(img)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_case(up, down, channels, downmix):
    """the windows of a case of the list in one source array, non-zero everywhere: (source, descriptors, window lengths)"""
    rng = np.random.default_rng(up * 1000 + down * 10 + channels + downmix)
    Ls = limit_lengths(up, down)
    rows, elems = layout_windows(Ls, channels, rng)
    elems += -elems % channels
    return random_source(elems, seed=up + down + channels), rows, Ls


@pytest.mark.parametrize("up,down,channels,downmix", LIMIT_CASES)
def test_every_branch_of_the_plan_on_random_data(ctx, up, down, channels, downmix):
    src, rows, Ls = random_case(up, down, channels, downmix)
    truths = [resample_truth(src[at: at + L * channels].reshape(L, channels), up, down, downmix) for at, L, _ in rows]
    jmax = max(out_len(L, up, down) for L in Ls)
    worst = 0.0
    for frames, guards in ((jmax, (16, 3, 5, 1)), (jmax + 7, (5, 1, 16, 3))):
        worst = max(worst, run_layouts(ctx, src, rows, channels, downmix, up, down, frames, guards,
                                       (PLANAR, INTERLEAVED, PLANAR_S16, INTERLEAVED_S16), truths))
    if up == down and not downmix:  # the copy, in two passes: the samples' bits
        img = run_once(ctx, src, rows, channels, downmix, up, down, jmax)
        for at, L, row in rows:
            assert img[row, :L].tobytes() == src[at: at + L * channels].tobytes(), L
    pl = launch_plan(up, down, channels, downmix)
    print("up %d down %d channels %d downmix %d (taps %d, span_cap %d, passes %s): largest error / bound %.3f" % (
        up, down, channels, downmix, pl["taps"], pl["span_cap"], passes_text(pl["passes"]), worst))


# ---------------------------------------------------------------------------------------------------------------------------- impulses

def impulse_positions(up, down, count=None):
    """(L, positions): single samples S apart, S > taps and coprime to `down`, the first at sample 0 and the last at sample L - 1.  With
    `count` None there are enough of them that every residue modulo `down` occurs at a position an output of every phase can see: one
    period of the residues, and again those of its positions that lie in front of the first output that could see them"""
    taps = filter_table(up, down)[0]
    S = taps + 1
    while math.gcd(S, down) != 1:
        S += 1
    if count is None:
        count = max(down + (down + 2 * taps + 2) // S + 2, 8)
    pos = np.arange(count, dtype=np.int64) * S
    return int(pos[-1]) + 1, pos


def impulse_truth(L, pos, up, down):
    """what a window of zeros with 1.0 at `pos` resamples to, exactly: (want [J] float32, phase [J], tap [J], hit [J]) -- output j is the
    table's entry coeffs[p][k] where tap k of its span [j * down // up + first[p], + taps) lies on an impulse, and 0 where none does"""
    from vorbispizza_amd import capi
    taps, first, coeffs = capi.resample_filter(up, down)
    assert np.diff(pos).min() > taps and pos[0] == 0 and pos[-1] == L - 1  # (no output sees two of them)
    j = np.arange(out_len(L, up, down), dtype=np.int64)
    p = j % up
    start = j * down // up + first[p]
    i = np.minimum(np.searchsorted(pos, start), len(pos) - 1)  # the first impulse at or behind the span's first sample
    k = pos[i] - start
    hit = (k >= 0) & (k < taps)
    k = np.where(hit, k, 0)
    want = np.where(hit, coeffs[p, k], np.float32(0.0)).astype(np.float32)
    return want, p, k, hit


def impulse_source(channels, windows):
    """windows [(L, positions, channel, amplitude)] -> (source, descriptors): every window is zeros but for its impulses, and EVERY element
    around the windows -- element -1 and element L of each among them -- is 1.0"""
    parts, rows, at = [], [], 0
    for row, (L, pos, channel, amp) in enumerate(windows):
        gap = 3 + (at + 4) % 2  # (an odd element offset)
        parts.append(np.ones(gap, dtype=np.float32))
        at += gap
        x = np.zeros((L, channels), dtype=np.float32)
        x[pos, channel] = amp
        parts.append(x.reshape(-1))
        rows.append((at, L, row))
        at += L * channels
    parts.append(np.ones(channels + 3 + -(at + channels + 3) % channels, dtype=np.float32))
    src = np.concatenate(parts)
    for at, L, _ in rows:
        assert at % 2 == 1 and src[at - 1] == 1.0 and src[at + L * channels] == 1.0
    return src, rows


def run_impulses(ctx, up, down, channels, downmix, windows, layouts=(PLANAR, INTERLEAVED)):
    """-> [(phase, tap, hit)] of the windows, after every output of every window was compared with =="""
    src, rows = impulse_source(channels, windows)
    frames = max(out_len(L, up, down) for L, _, _, _ in windows) + 3
    seen = []
    for layout in layouts:
        img = run_once(ctx, src, rows, channels, downmix, up, down, frames, layout, dst_rows=len(windows))
        seen = []
        for (L, pos, channel, amp), (_, _, row) in zip(windows, rows):
            J = out_len(L, up, down)
            assert not bits(img[row, J:]).any(), "not zero bits behind the samples"
            want = np.zeros((J, img.shape[2]), dtype=np.float32)
            if len(pos):
                want[:, 0 if downmix else channel], p, k, hit = impulse_truth(L, pos, up, down)
                seen.append((p, k, hit))
            wrong = np.argwhere(img[row, :J] != want)  # (==, not bits: -0.0 is 0.0)
            assert wrong.size == 0, (up, down, channels, downmix, layout, row, len(wrong), wrong[:4].tolist(),
                                     [(float(img[row, a, b]), float(want[a, b])) for a, b in wrong[:4]])
    return seen


def pairs_seen(up, down, seen):
    """(seen [up, taps] bool, live [up, taps] bool)"""
    taps = filter_table(up, down)[0]
    got = np.zeros((up, taps), dtype=bool)
    for p, k, hit in seen:
        got[p[hit], k[hit]] = True
    live = np.arange(taps)[None, :] < live_taps(up, down)[:, None]
    return got, live


@pytest.mark.parametrize("up,down", [(1, 32), (31, 991), (5, 48), (1, 12), (160, 441), (3, 1), (1024, 32767), (1024, 1023)])
def test_impulses_give_back_every_entry_of_the_table(ctx, up, down):
    """mono; beside the window of impulses, a window of zeros between 1.0 and 1.0: its row is all zeros"""
    from vorbispizza_amd import capi
    L, pos = impulse_positions(up, down)
    taps, first, coeffs = capi.resample_filter(up, down)
    empty = np.zeros(0, dtype=np.int64)
    seen = run_impulses(ctx, up, down, 1, False, [(L, pos, 0, 1.0), (2 * down + taps + 5, empty, 0, 0.0), (1, empty, 0, 0.0)])
    got, live = pairs_seen(up, down, seen)
    assert (coeffs[live] != 0).all()  # (a live tap that were zero would be seen as nothing)
    full = (got | ~live).all(axis=1)
    print("up %d down %d: %d samples, %d impulses, %d outputs; %d of %d live (phase, tap) pairs seen, %d of %d phases whole" % (
        up, down, L, len(pos), out_len(L, up, down), int((got & live).sum()), int(live.sum()), int(full.sum()), up))
    # every live pair of the table -- at up = 1024 too, where the least that counts is eight whole phases with the first and the last
    assert full.sum() >= min(8, up) and full[0] and full[-1]
    assert (got | ~live).all(), np.argwhere(~got & live)[:8].tolist()


def test_impulses_in_one_channel_of_three_stay_in_it(ctx):
    """(31, 991), three passes of one channel: the impulses in another channel in every window"""
    up, down = 31, 991
    L, pos = impulse_positions(up, down, 40)
    run_impulses(ctx, up, down, 3, False, [(L, pos, c, 1.0) for c in (2, 0, 1)])


@pytest.mark.parametrize("channels", [2, 4])
def test_impulses_mixed_down_from_a_power_of_two_channels(ctx, channels):
    """(1, 32): an impulse of `channels` in one channel is a mean of exactly 1.0"""
    up, down = 1, 32
    L, pos = impulse_positions(up, down)
    seen = run_impulses(ctx, up, down, channels, True, [(L, pos, channels - 1, float(channels)), (2 * down + 5, np.zeros(0, dtype=np.int64), 0, 0.0)])
    got, live = pairs_seen(up, down, seen[:1])
    assert (got | ~live).all()


# -------------------------------------------------------------------------------------------------------------------------- non-finite

NON_FINITE_CASES = [(1, 32, 2, False), (160, 441, 10, False), (5, 48, 7, True)]


@pytest.mark.parametrize("up,down,channels,downmix", NON_FINITE_CASES)
def test_infinities_and_nans_around_the_windows_change_no_bit(ctx, up, down, channels, downmix):
    assert (up, down, channels, downmix) in LIMIT_CASES
    src, rows, Ls = random_case(up, down, channels, downmix)
    frames = max(out_len(L, up, down) for L in Ls) + 1
    inside = np.zeros(src.size, dtype=bool)
    for at, L, _ in rows:
        inside[at: at + L * channels] = True
    sown = src.copy()
    around = np.flatnonzero(~inside)
    sown[around] = np.asarray([np.inf, -np.inf, np.nan], dtype=np.float32)[np.arange(around.size) % 3]
    for at, L, _ in rows:  # in front of every window and behind it, whatever lies between two of them
        assert not np.isfinite(sown[at - 1]) and not np.isfinite(sown[at + L * channels]) and np.isfinite(sown[at: at + L * channels]).all()
    for layout in (PLANAR, INTERLEAVED):
        want = run_once(ctx, src, rows, channels, downmix, up, down, frames, layout)
        got = run_once(ctx, sown, rows, channels, downmix, up, down, frames, layout)
        assert np.isfinite(want[[row for _, _, row in rows]]).all()
        assert bits(got).tobytes() == bits(want).tobytes(), layout


@pytest.mark.parametrize("up,down,channels,downmix", NON_FINITE_CASES)
def test_an_infinity_inside_a_window_reaches_the_outputs_whose_taps_lie_on_it(ctx, up, down, channels, downmix):
    from vorbispizza_amd import capi
    src, rows, Ls = random_case(up, down, channels, downmix)
    frames = max(out_len(L, up, down) for L in Ls) + 1
    taps, first, coeffs = capi.resample_filter(up, down)
    live = live_taps(up, down)
    at, L, row = max(rows, key=lambda r: r[1])  # two and a half tiles
    J = out_len(L, up, down)
    for m0, channel in ((L // 2 + 1, channels - 1), (0, 0), (L - 1, channels // 2)):
        half, inf = src.copy(), src.copy()
        half[at + m0 * channels + channel] = 0.5
        inf[at + m0 * channels + channel] = np.inf
        want = run_once(ctx, half, rows, channels, downmix, up, down, frames)
        got = run_once(ctx, inf, rows, channels, downmix, up, down, frames)
        j = np.arange(J, dtype=np.int64)
        p = j % up
        k = m0 - (j * down // up + first[p])
        touched = (k >= 0) & (k < taps)
        # a live tap with a non-zero coefficient on m0: not finite.  An output that touches m0 only with the zero padding of a short
        # phase is NOT asserted either way: the header's filter, like the published one, multiplies there (0 * Inf).
        reached = touched & (k < live[p]) & (coeffs[p, np.where(touched, k, 0)] != 0)
        # (about taps * up / down outputs see a sample in the middle of a window, half as many its first or last)
        assert reached.sum() >= max(taps * up // down // (1 if 0 < m0 < L - 1 else 3) - 1, 1) and (~touched).sum() > 0
        oc = 0 if downmix else channel
        assert not np.isfinite(got[row, :J, oc][reached]).any(), (m0, np.flatnonzero(reached & np.isfinite(got[row, :J, oc]))[:8].tolist())
        same = np.ones(got.shape, dtype=bool)
        same[row, :J, oc] = ~touched
        assert (bits(got)[same] == bits(want)[same]).all(), (m0, np.argwhere(same & (bits(got) != bits(want)))[:8].tolist())
        assert np.isfinite(want[row, :J]).all()
