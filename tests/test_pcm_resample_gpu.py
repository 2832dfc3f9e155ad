"""vpz_pcm_resample (include/vorbispizza_pcm_resample.h, csrc/pcm_resample.hip) alone: no decoder.

The source is seeded random float32, non-zero EVERYWHERE -- in front of every window, behind it and between windows --, so a tap that
reads a neighbour instead of the definition's zero shows.  The truth is tests/test_resample_cpu.py's float64 restatement and its derived
bound, (T + C + 3) * 2^-24 * B[j] (C the channels mixed down, 1 otherwise); nothing else is tolerated: the zeros behind a row's J samples
are zero bits, the int16 layouts are the project's conversion of the float32 layout's OWN output bit for bit, and the guards on either
side of the destination and the rows no descriptor names keep their sentinel.  Every refusal returns VPZ_E_INVALID_ARG and writes nothing."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from resample_truth import bound, resample_truth, to_s16  # noqa: E402
from pcm_support import (INTERLEAVED, INTERLEAVED_S16, PLANAR, PLANAR_S16, guarded_layout as guarded, layout_windows,  # noqa: E402
    out_len, random_source, rows_of, run_layouts)
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu


# up / down; 1/1 is the copy (and, with a downmix, the mean alone)
RATIOS = [(160, 441), (1, 3), (3, 1), (160, 147), (147, 160), (441, 80), (1, 6), (2, 1), (1, 2), (1, 1)]
MIXES = [(1, False), (2, False), (6, False), (2, True), (6, True)]  # (source channels, downmix)


def lengths(down):
    """shorter than the filter, around one period of the phases, several tiles"""
    return [0, 1, 2, 5, 13, max(down - 1, 0), down, down + 1, 1000, 3001]


@pytest.mark.parametrize("channels,downmix", MIXES)
@pytest.mark.parametrize("up,down", RATIOS)
def test_every_named_row_is_the_resampled_window_then_zeros(ctx, up, down, channels, downmix):
    rng = np.random.default_rng(up * 1000 + down * 10 + channels + downmix)
    Ls = lengths(down)
    rows, elems = layout_windows(Ls, channels, rng)
    elems += -elems % channels
    src = random_source(elems, seed=up + down + channels)
    truths = [resample_truth(src[at: at + L * channels].reshape(L, channels), up, down, downmix) for at, L, _ in rows]
    if (up, down) == (1, 1) and not downmix:  # the copy: the samples' bits
        for (at, L, _), (y, _) in zip(rows, truths):
            assert y.astype(np.float32).tobytes() == src[at: at + L * channels].tobytes()
    jmax = max(out_len(L, up, down) for L in Ls)
    worst = 0.0
    # frames = J of the longest window, J + 1 and J + 7 (one of them odd: rows leave every alignment); guards move the destination too
    for frames, guards in ((jmax, (16, 3, 5, 1)), (jmax + 1, (3, 16, 1, 5)), (jmax + 7, (5, 1, 16, 3))):
        worst = max(worst, run_layouts(ctx, src, rows, channels, downmix, up, down, frames, guards,
                                       (PLANAR, INTERLEAVED, PLANAR_S16, INTERLEAVED_S16), truths))
    # the short windows alone, frames = their own largest J: a row with no zeros behind it at every small size
    small = [(r, t) for r, t in zip(rows, truths) if r[1] <= down + 1 and r[1] < 1000]
    js = sorted({out_len(r[1], up, down) for r, _ in small if r[1] > 0})
    for frames in js[-2:]:
        fit = [(r, t) for r, t in small if out_len(r[1], up, down) <= frames]
        worst = max(worst, run_layouts(ctx, src, [r for r, _ in fit], channels, downmix, up, down, frames, (2, 7, 1, 4),
                                       (INTERLEAVED, PLANAR, INTERLEAVED_S16, PLANAR_S16), [t for _, t in fit]))
    print("up %d down %d channels %d downmix %d: largest error / bound %.3f" % (up, down, channels, downmix, worst))


def test_the_copy_keeps_every_bit_pattern(ctx):
    """up == down without a downmix moves samples: negative zero, denormals, infinities and NaN payloads included (float32 layouts)"""
    import torch
    from vorbispizza_amd import capi
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 32, 2 * 700, dtype=np.uint32)
    for i, v in enumerate([0x80000000, 0x00000001, 0x807FFFFF, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x00000000] * 4):
        bits[(i * 37 + 5) % bits.size] = v
    src = torch.from_numpy(bits.view(np.float32).copy()).to("cuda:0").view(-1, 2)
    for layout in (PLANAR, INTERLEAVED):
        whole, dst, flat = guarded(3, 2, 650, layout, 3)
        assert capi.pcm_resample(ctx, src, [(7 * 2, 649, 1)], dst, layout, 1, 1, False) == capi.OK, ctx.last_error()
        ctx.synchronize()
        img, _, _ = rows_of(whole, 3, 3, 2, 650, layout)
        assert img[1, :649].view(np.uint32).tobytes() == bits[14: 14 + 649 * 2].tobytes()
        assert (img[1, 649:].view(np.uint32) == 0).all() and (img[[0, 2]].view(np.uint32) == 0x5A5A5A5A).all()


def test_more_descriptors_than_the_grid_is_high(ctx):
    """a workgroup takes several descriptors when there are more of them than the grid's second dimension"""
    import torch
    from vorbispizza_amd import capi
    n, channels, frames, up, down = 4500, 2, 7, 1, 2
    rng = np.random.default_rng(3)
    order = rng.permutation(n + 100)[:n]
    rows = [(int(k) * 4 + 2, int(rng.integers(0, 2 * frames + 1)), int(r)) for k, r in enumerate(order)]
    src_np = random_source(n * 4 + 2 + 2 * frames * channels, 9)
    src = torch.from_numpy(src_np).to("cuda:0").view(-1, channels)
    whole, dst, flat = guarded(n + 100, channels, frames, PLANAR, 3)
    assert capi.pcm_resample(ctx, src, rows, dst, PLANAR, up, down, False) == capi.OK, ctx.last_error()
    ctx.synchronize()
    img, g0, g1 = rows_of(whole, 3, n + 100, channels, frames, PLANAR)
    want_named = np.zeros(n + 100, dtype=bool)
    for at, L, row in rows:
        y, B = resample_truth(src_np[at: at + L * channels].reshape(L, channels), up, down)
        J = out_len(L, up, down)
        assert (np.abs(img[row, :J] - y) <= bound(B, up, down)).all() and (img[row, J:].view(np.uint32) == 0).all(), row
        want_named[row] = True
    assert (img[~want_named].view(np.uint32) == 0x5A5A5A5A).all() and (g0 == 0x5A5A5A5A).all() and (g1 == 0x5A5A5A5A).all()


def test_indices_beyond_two_to_the_31(ctx):
    """the last rows of a destination and a window of a source whose element indices do not fit 32 bits"""
    import torch
    from vorbispizza_amd import capi
    channels, frames, up, down = 2, 1024, 160, 441
    dst_rows = (1 << 31) // (channels * frames) + 2
    src = torch.empty(((1 << 31) + 8192) // channels, channels, dtype=torch.float32, device="cuda:0")
    tail = random_source(8192, 4)
    src.view(-1)[1 << 31:] = torch.from_numpy(tail).to("cuda:0")
    wins = [(7, 2000, 2), (2100 * channels, 1024 * 441 // 160 - 900, 0)]  # (offsets inside the tail, rows from the end)
    assert all(at + L * channels <= 8192 and out_len(L, up, down) <= frames for at, L, _ in wins)
    truths = [resample_truth(tail[at: at + L * channels].reshape(L, channels), up, down) for at, L, _ in wins]
    f32 = {}
    for layout in (PLANAR, INTERLEAVED_S16):
        s16 = layout == INTERLEAVED_S16
        dst = torch.empty((dst_rows, channels, frames) if layout == PLANAR else (dst_rows, frames, channels), dtype=torch.int16 if s16 else torch.float32,
                          device="cuda:0")
        dst[-3:] = 23130 if s16 else 7.0
        rows = [((1 << 31) + at, L, dst_rows - 3 + r) for at, L, r in wins]
        assert capi.pcm_resample(ctx, src, rows, dst, layout, up, down, False) == capi.OK, ctx.last_error()
        ctx.synchronize()
        got = dst[-3:].cpu().numpy()
        got = got.transpose(0, 2, 1) if layout == PLANAR else got
        assert (got[1] == (23130 if s16 else 7.0)).all()
        for (at, L, r), (y, B) in zip(wins, truths):
            J = out_len(L, up, down)
            assert (got[r, J:] == 0).all()
            if s16:
                assert got[r, :J].tobytes() == to_s16(f32[r]).tobytes()
            else:
                assert (np.abs(got[r, :J] - y) <= bound(B, up, down)).all()
                f32[r] = got[r, :J].copy()
        del dst


def raw_call(ctx, src_ptr, src_elems, channels, up, down, downmix, rows, dst_ptr, dst_rows, out_channels, frames, layout, n_rows=None, null_rows=False,
             handle=True):
    from vorbispizza_amd import capi
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    return capi.lib().vpz_pcm_resample(ctx._h if handle else None, src_ptr, src_elems, channels, up, down, downmix, desc.shape[0] if n_rows is None else n_rows,
                                       None if null_rows else desc.ctypes.data, dst_ptr, dst_rows, out_channels, frames, layout)


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED_S16])
def test_every_refusal_is_invalid_arg_and_writes_nothing(ctx, layout):
    import torch
    from vorbispizza_amd import capi
    s16 = layout == INTERLEAVED_S16
    channels, frames, dst_rows, guard, up, down = 2, 64, 4, 16, 1, 3
    src_np = random_source(1000, 11)
    src = torch.from_numpy(src_np).to("cuda:0")
    whole, dst, flat = guarded(dst_rows, channels, frames, layout, guard)
    good = dict(src_ptr=src.data_ptr(), src_elems=1000, channels=channels, up=up, down=down, downmix=0, rows=[(3, 10, 1), (41, 64 * 3, 3)],
                dst_ptr=dst.data_ptr(), dst_rows=dst_rows, out_channels=channels, frames=frames, layout=layout)
    elem = 2 if s16 else 4
    pinned = torch.full((dst_rows, channels, frames), 77, dtype=torch.int16 if s16 else torch.float32, pin_memory=True)
    host_src = torch.full((1000,), 0.5, dtype=torch.float32, pin_memory=True)
    refused = {
        "null context": dict(handle=False),
        "null source": dict(src_ptr=None),
        "null destination": dict(dst_ptr=None),
        "null descriptors": dict(null_rows=True),
        "no channels": dict(channels=0, out_channels=0),
        "too many channels": dict(channels=capi.MAX_CHANNELS + 1, out_channels=capi.MAX_CHANNELS + 1),
        "no frames": dict(frames=0),
        "negative descriptor count": dict(n_rows=-1),
        "negative row count": dict(dst_rows=-1),
        "negative source size": dict(src_elems=-1),
        "layout 4": dict(layout=4),
        "layout -1": dict(layout=-1),
        "up above 1024": dict(up=1025, down=1),
        "down above 32 up": dict(up=1, down=33),
        "not in lowest terms": dict(up=2, down=6),
        "up 0": dict(up=0),
        "down 0": dict(down=0),
        "negative up": dict(up=-1),
        "downmix 2": dict(downmix=2),
        "downmix -1": dict(downmix=-1),
        "one output channel without a downmix": dict(out_channels=1),
        "two output channels with a downmix": dict(downmix=1),
        "three output channels": dict(out_channels=3),
        "source starts before the array": dict(rows=[(-1, 10, 1)]),
        "source ends behind the array": dict(rows=[(1000 - 10 * channels + 1, 10, 1)]),
        "source starts behind the array": dict(rows=[(1001, 0, 1)]),
        "one output sample more than frames": dict(rows=[(0, frames * 3 + 1, 1)]),
        "negative samples": dict(rows=[(0, -1, 1)]),
        "row behind the last": dict(rows=[(0, 1, dst_rows)]),
        "negative row": dict(rows=[(0, 1, -1)]),
        "a row named twice": dict(rows=[(0, 1, 2), (8, 3, 0), (16, 2, 2)]),
        "more descriptors than rows": dict(rows=[(0, 1, 0)] * (dst_rows + 1)),
        "destination off its element": dict(dst_ptr=dst.data_ptr() + 1),
        "source off its element": dict(src_ptr=src.data_ptr() + 2, src_elems=999),
        "page-locked host destination": dict(dst_ptr=pinned.data_ptr()),
        "page-locked host source": dict(src_ptr=host_src.data_ptr()),
        # (row 1 alone is named and lies inside the tensor: without the range check the call would succeed)
        "destination longer than its allocation": dict(dst_rows=(1 << 40) // (channels * frames * elem)),
        "source longer than its allocation": dict(src_elems=1 << 38),
    }
    for what, change in refused.items():
        assert raw_call(ctx, **{**good, **change}) == capi.E_INVALID_ARG, what
    ctx.synchronize()
    bits = lambda t: t.cpu().numpy().view(np.uint16 if s16 else np.uint32)  # noqa: E731
    assert bits(whole).tobytes() == flat.tobytes()
    assert (pinned == 77).all()
    # ... and the call they were all made from is a good one: J = frames exactly in row 3
    assert raw_call(ctx, **good) == capi.OK, ctx.last_error()
    ctx.synchronize()
    img, g0, g1 = rows_of(whole, guard, dst_rows, channels, frames, layout)
    assert (g0 == flat[0]).all() and (g1 == flat[0]).all() and (img[[0, 2]].view(g0.dtype) == flat[0]).all()
    for at, L, row in good["rows"]:
        y, B = resample_truth(src_np[at: at + L * channels].reshape(L, channels), up, down)
        J = out_len(L, up, down)
        if s16:  # (a sanity check within one step: run_layouts holds the int16 layouts to the float32 output bit for bit)
            assert (np.abs(img[row, :J].astype(np.float64) - np.clip(np.trunc(y * 32768.0), -32768, 32767)) <= 1).all()
        else:
            assert (np.abs(img[row, :J] - y) <= bound(B, up, down)).all()
        assert (img[row, J:] == 0).all()
    # no descriptors: nothing to do, nothing written
    before = bits(whole).copy()
    assert raw_call(ctx, **{**good, "rows": []}) == capi.OK
    ctx.synchronize()
    assert bits(whole).tobytes() == before.tobytes()
