"""vpz_pcm_fbank (include/vorbispizza_pcm_fbank.h, csrc/pcm_fbank.hip) alone: no decoder.

The truth is tests/fbank_truth.py's float64 restatement of the header's definition -- unfolded: scale, mean, pre-emphasis, window, pad,
rfft, power, dense W, log -- and the tolerance its derived bound e_M, used as it stands.  The real frames of a row lie inside the bound;
every element behind them is pad_value bit for bit; rows no descriptor names and the guards on either side of the destination keep their
sentinel; source elements behind a row's L are NaN and never reach the output; every refusal returns VPZ_E_INVALID_ARG and writes nothing.
The signal is seeded noise plus a tone, written into a device array at odd and aligned offsets.

Largest error / bound ratio observed on an MI355X over the cases of this file (test_zz_the_largest_ratio_of_this_file prints them):
0.138 for the power output and 0.40 for the log, both at (win 2, hop 1, n_fft 32, one band); 0.049 / 0.24 at n_fft 38; 0.0089 / 0.030 at
the Kaldi spec over every option; 0.012 / 0.019 in the DC case; 0.079 in the grid's second round; 0.038 beyond 2^31."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fbank_truth as ft  # noqa: E402
from fbank_truth import refused_specs  # noqa: E402
from fbank_cases import WORST, launch, note  # noqa: E402
from pcm_support import GUARD, SENTINEL, guarded, place, signal  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pad_value", [0.0, -15.9424])
def test_row_lengths(ctx, pad_value):
    """L = 0, 399, 400, 559, 560, F - 1 and F at (400, 160, 512, 23): T_L = 0, 0, 1, 1, 2, 71, 71 of T = 71"""
    d = ft.spec_of(n_mels=23, pad_value=pad_value)
    F = 400 + 160 * 70 + 37
    Ls = [0, 399, 400, 559, 560, F - 1, F]
    assert [ft.n_frames(L, 400, 160) for L in Ls] == [0, 0, 1, 1, 2, 71, 71] and ft.n_frames(F, 400, 160) == 71
    windows = [signal(L, 100 + i) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    assert {o % 2 for o in offs} == {0, 1} and np.isnan(src).sum() > 0
    order = [7, 2, 9, 4, 1, 8, 5]  # (rows 0, 3, 6 and 10 are named by nobody: the guard rows around and between)
    got = launch(ctx, d, src, [(o, L, r) for o, L, r in zip(offs, Ls, order)], 11, F)
    assert (got[[0, 3, 6, 10]].view(np.uint32) == SENTINEL).all()
    W, B = ft.mel_weights64(d), ft.operator64(d)
    pad_bits = np.float32(pad_value).view(np.uint32)
    for w, L, r in zip(windows, Ls, order):
        TL = ft.n_frames(L, 400, 160)
        assert (got[r, TL:].view(np.uint32) == pad_bits).all(), L  # (check_row holds this as well)
        assert not np.isnan(got[r]).any()
        note("row_lengths", ft.check_row(got[r], w, d, W, B))
        assert TL == 0 or (got[r, :TL].view(np.uint32) != pad_bits).any()


# name: (spec changes, F) -- F with a remainder; T is no multiple of a tile
SHAPES = {
    "smallest_2_1_32_1": (dict(win=2, hop=1, n_fft=32, n_mels=1, window="hamming"), 2 + 70 + 0),                    # T = 71
    "widest_1024_1024_1024_256": (dict(win=1024, hop=1024, n_fft=1024, n_mels=256, sample_rate=48000), 1024 * 19 + 100),  # T = 19: 16-frame tiles
    "odd_551_220_1024_80": (dict(win=551, hop=220, n_fft=1024, n_mels=80, sample_rate=22050), 551 + 220 * 40 + 7),   # T = 41
    "full_512_128_512_40": (dict(win=512, hop=128, n_fft=512, n_mels=40), 512 + 128 * 70 + 5),                       # T = 71
    "tail_37_5_38_6": (dict(win=37, hop=5, n_fft=38, n_mels=6, sample_rate=8000, low_freq=100.0), 37 + 5 * 70 + 3),  # 18 pairs: 4 blocks, 2 left, the odd sample
    "tail_35_4_38_6": (dict(win=35, hop=4, n_fft=38, n_mels=6, sample_rate=8000, low_freq=100.0), 35 + 4 * 70 + 1),  # 17 pairs: 1 left, the odd sample; a skewed span
    "tail_30_30_38_6": (dict(win=30, hop=30, n_fft=38, n_mels=6, sample_rate=8000, low_freq=100.0), 30 + 30 * 40 + 9),  # 15 pairs: 3 left; hop = win
}


@pytest.mark.parametrize("log", [False, True], ids=["power", "log"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(ctx, name, log):
    change, F = SHAPES[name]
    d = ft.spec_of(log=log, **change)
    win, hop = d["win"], d["hop"]
    T = ft.n_frames(F, win, hop)
    assert T % 16 != 0 and (hop == 1 or (F - win) % hop != 0)
    # a full row, one sample short, a third (pad-only tiles behind it), one frame exactly, one sample short of a frame
    Ls = [F, F - 1, F // 3, win, win - 1]
    windows = [signal(L, 7 * i + win, d["sample_rate"]) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    order = [4, 0, 5, 2, 6]
    got = launch(ctx, d, src, [(o, L, r) for o, L, r in zip(offs, Ls, order)], 7, F)
    assert got.shape == (7, T, d["n_mels"]) and (got[[1, 3]].view(np.uint32) == SENTINEL).all()
    W, B = ft.mel_weights64(d), ft.operator64(d)
    for w, L, r in zip(windows, Ls, order):
        note("%s %s" % (name, "log" if log else "power"), ft.check_row(got[r], w, d, W, B))


def test_options(ctx):
    """three windows, remove_dc on and off, c 0 and 0.97, power and log, both layouts, scale 1 and 32768, at (400, 160, 512, 23) with
    T = 35 (a whole tile and a partial one)"""
    import torch
    F = 400 + 160 * 34 + 11
    Ls = [F, F - 161, 1000]
    windows = [signal(L, 40 + i) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    d_src = torch.from_numpy(src).to("cuda:0")
    rows = [(o, L, r) for o, L, r in zip(offs, Ls, (2, 0, 1))]
    for window in ft.WINDOWS:
        for remove_dc in (True, False):
            for c in (0.0, 0.97):
                for scale in (1.0, 32768.0):
                    base = ft.spec_of(n_mels=23, window=window, remove_dc=remove_dc, preemphasis=c, scale=scale)
                    W, B = ft.mel_weights64(base), ft.operator64(base)
                    truths = [ft.fbank_truth(w, base, W, B) for w in windows]
                    images = {}
                    for log in (False, True):
                        for frames_first in (True, False):
                            d = dict(base, log=log, frames_first=frames_first)
                            got = launch(ctx, d, src, rows, 3, F, d_src)
                            images[(log, frames_first)] = got
                            for (M, e_M), L, (_, _, r) in zip(truths, Ls, rows):
                                TL = M.shape[0]
                                assert (got[r, TL:].view(np.uint32) == 0).all()
                                ratio = ft.check_log(got[r, :TL], M, e_M, d["floor"]) if log else ft.check_power(got[r, :TL], M, e_M)
                                note("options %s" % ("log" if log else "power"), ratio)
                    for log in (False, True):  # (the layout changes where an element lies, not its bits)
                        assert images[(log, True)].tobytes() == np.ascontiguousarray(images[(log, False)]).tobytes()


def test_a_dc_offset_far_above_the_signal_stays_inside_the_bound(ctx):
    """offset 0.5 under a signal of amplitude 1e-3 with remove_dc: the mean is subtracted before the product, so nothing cancels in the
    accumulators -- what the unfolded mean buys.  The bound is the same formula as everywhere (its mean term is now the largest)."""
    F = 400 + 160 * 40 + 3
    for scale, log in ((1.0, False), (32768.0, True)):
        d = ft.spec_of(n_mels=23, scale=scale, log=log)
        w = (0.5 + 1e-3 * np.random.default_rng(77).standard_normal(F) + 1e-3 * np.sin(2 * np.pi * 440.0 * np.arange(F) / 16000)).astype(np.float32)
        src, offs = place([w])
        got = launch(ctx, d, src, [(offs[0], F, 0)], 1, F)
        M, e_M = ft.fbank_truth(w, d)
        # the signal is there, not lost under the offset: the tone's band stands well above its neighbours' mean
        assert M.max() > 50 * np.median(M)
        note("dc offset %s" % ("log" if log else "power"), ft.check_row(got[0], w, d))


def test_tiles(ctx):
    """T_L one before, at and one after a 32- and a 64-frame boundary, a pad-only row, and ONE WINDOW in three launches that pick 16-, 32-
    and 64-frame tiles (by F and the row count), beside different neighbours: its real frames are the same bits in all three."""
    import torch
    d = ft.spec_of(n_mels=23)
    win, hop, crowd = 400, 160, 600
    F = win + hop * 97 + 13  # T = 98
    k = ft.kernel_constants(ROOT)
    assert ft.tile_plan(win, hop, 512, 98, 8, 256, k)[0] == 32 and ft.tile_plan(win, hop, 512, 98, crowd, 300, k)[0] == 64
    F16 = win + hop * 15 + 50  # T = 16
    assert ft.tile_plan(win, hop, 512, ft.n_frames(F16, win, hop), 8, 256, k)[0] == 16
    TLs = [31, 32, 33, 63, 64, 65, 16, 0]
    Ls = [win + hop * (t - 1) + 7 if t else win - 1 for t in TLs]
    assert [ft.n_frames(L, win, hop) for L in Ls] == TLs
    host = signal(crowd * 67 + F + 8, 5)
    src = torch.from_numpy(host).to("cuda:0")
    starts = [3 + 1000 * i for i in range(len(Ls))]
    rows = [(a, L, r) for a, L, r in zip(starts, Ls, (5, 1, 7, 0, 3, 6, 2, 4))]
    few = launch(ctx, d, host, rows, 8, F, src)
    W, B = ft.mel_weights64(d), ft.operator64(d)
    for a, L, r in rows:
        note("tiles of 32", ft.check_row(few[r], host[a: a + L], d, W, B))
    # the same windows first, then hundreds of others (overlapping in the source, 67 samples apart, of all lengths)
    rng = np.random.default_rng(8)
    many = [(a, L, i) for i, (a, L, _) in enumerate(rows)] + [(i * 67 + 1, int(rng.integers(0, F + 1)), i) for i in range(len(rows), crowd)]
    big = launch(ctx, d, host, many, crowd, F, src)
    for i, (a, L, r) in enumerate(rows):
        assert big[i].tobytes() == few[r].tobytes(), TLs[i]
    for a, L, r in many[len(rows)::97]:
        note("tiles of 64", ft.check_row(big[r], host[a: a + L], d, W, B))
    # the 16-frame window again, in a launch whose rows hold no more than 16 frames
    a16, L16 = starts[6], Ls[6]
    small = launch(ctx, d, host, [(a16 + 400, 2000, 0), (a16, L16, 2), (a16 + 9, win, 1)], 3, F16, src)
    assert small.shape[1] == 16
    assert small[2].tobytes() == few[2, :16].tobytes() == big[6, :16].tobytes()
    note("tiles of 16", ft.check_row(small[0], host[a16 + 400: a16 + 2400], d, W, B))
    # ... and the first frames of a longer window do not depend on the frames behind them
    longer = launch(ctx, d, host, [(a16, L16 + 5000, 0)], 1, F, src)
    assert longer[0, :16].tobytes() == few[2, :16].tobytes() and (few[2, 16:].view(np.uint32) == 0).all()


def test_more_descriptors_than_the_grid_holds_side_by_side(ctx):
    """3000 rows at n_fft 32 (the grid's y holds 2048: workgroups take a second descriptor), in a destination of 3100 rows.  Rows not
    named keep the sentinel bit for bit; the source behind every row's L is NaN and must not reach the output."""
    n, dst_rows, F = 3000, 3100, 32 + 16 * 3 + 5
    d = ft.spec_of(win=32, hop=16, n_fft=32, n_mels=8, log=False, scale=1.0)
    k = ft.kernel_constants(ROOT)
    assert n > k["kFbMaxGridY"]
    rng = np.random.default_rng(3)
    stride = F + 3
    Ls = rng.integers(0, F + 1, n)
    Ls[:4] = (F, 0, 31, F - 1)
    Ls[-3:] = (F, 32, 48)
    src = np.full(1 + n * stride, np.nan, dtype=np.float32)
    x = (0.5 * rng.standard_normal((n, F))).astype(np.float32)
    for i in range(n):
        src[1 + i * stride: 1 + i * stride + Ls[i]] = x[i, : Ls[i]]
    order = rng.permutation(dst_rows)[:n]
    got = launch(ctx, d, src, [(1 + i * stride, int(Ls[i]), int(order[i])) for i in range(n)], dst_rows, F)
    assert not np.isnan(got[order]).any()
    rest = np.setdiff1d(np.arange(dst_rows), order)
    assert rest.size == 100 and (got[rest].view(np.uint32) == SENTINEL).all()
    W, B = ft.mel_weights64(d), ft.operator64(d)
    checked = sorted(set(range(0, n, 7)) | {0, 1, 2, 3, n - 3, n - 2, n - 1})
    assert sum(i >= k["kFbMaxGridY"] for i in checked) > 100  # (rows of the second round)
    for i in checked:
        note("second round", ft.check_row(got[order[i]], x[i, : Ls[i]], d, W, B))


def test_indices_beyond_two_to_the_31(ctx):
    """a window of a source and the last rows of a destination whose element indices do not fit 32 bits"""
    import torch
    from vorbispizza_amd import capi
    F, n_mels = 1000, 8
    d = ft.spec_of(win=32, hop=16, n_fft=32, n_mels=n_mels, log=False, scale=1.0)
    T = ft.n_frames(F, 32, 16)
    dst_rows = (1 << 31) // (n_mels * T) + 8
    src = torch.empty((1 << 31) + 8192, dtype=torch.float32, device="cuda:0")
    tail = signal(8192, 4)
    src[1 << 31:] = torch.from_numpy(tail).to("cuda:0")
    wins = [(7, 1000, 2), (2101, 333, 0)]  # (offsets inside the tail, rows from the end)
    for frames_first in (True, False):
        dst = torch.empty((dst_rows, T, n_mels) if frames_first else (dst_rows, n_mels, T), dtype=torch.float32, device="cuda:0")
        dst[-3:] = 7.0
        assert (dst_rows - 3) * n_mels * T > 1 << 31
        rows = [((1 << 31) + at, L, dst_rows - 3 + r) for at, L, r in wins]
        spec = capi.FbankSpec.make(**dict(d, frames_first=frames_first))
        assert capi.pcm_fbank(ctx, src, rows, dst, spec, F) == capi.OK, ctx.last_error()
        ctx.synchronize()
        got = dst[-3:].cpu().numpy()
        got = got if frames_first else got.transpose(0, 2, 1)
        assert (got[1] == 7.0).all()
        for at, L, r in wins:
            note("beyond 2^31", ft.check_row(got[r], tail[at: at + L], d))
        del dst


def raw_call(ctx, src_ptr, src_elems, frames, spec, rows, dst_ptr, dst_rows, n_rows=None, null_rows=False, handle=True, null_spec=False):
    from vorbispizza_amd import capi
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    return capi.lib().vpz_pcm_fbank(ctx._h if handle else None, src_ptr, src_elems, frames, None if null_spec else C.byref(spec),
                                    desc.shape[0] if n_rows is None else n_rows, None if null_rows else desc.ctypes.data, dst_ptr, dst_rows)


def test_every_refusal_is_invalid_arg_and_writes_nothing(ctx):
    import torch
    from vorbispizza_amd import capi
    F, dst_rows, n_mels = 1000, 4, 80
    T = 1 + (F - 400) // 160
    src = torch.from_numpy(signal(2000, 9)).to("cuda:0")
    whole, dst = guarded(dst_rows, n_mels * T)
    spec = capi.FbankSpec.make()
    good = dict(src_ptr=src.data_ptr(), src_elems=2000, frames=F, spec=spec, rows=[(3, 500, 1), (400, 1000, 3)], dst_ptr=dst.data_ptr(), dst_rows=dst_rows)
    pinned = torch.zeros(dst_rows * n_mels * T, dtype=torch.float32, pin_memory=True)
    host_src = torch.full((2000,), 0.5, dtype=torch.float32, pin_memory=True)
    bad = [("no context", dict(handle=False)), ("null source", dict(src_ptr=None)), ("null destination", dict(dst_ptr=None)), ("null rows", dict(null_rows=True)),
           ("null spec", dict(null_spec=True)), ("frames < win", dict(frames=399, rows=[(3, 100, 1)])), ("frames 0", dict(frames=0, rows=[(3, 0, 1)])),
           ("n_rows < 0", dict(n_rows=-1)), ("dst_rows < 0", dict(dst_rows=-1)), ("src_elems < 0", dict(src_elems=-1)),
           ("samples > frames", dict(rows=[(3, 1001, 1)])), ("samples < 0", dict(rows=[(3, -1, 1)])), ("src < 0", dict(rows=[(-1, 10, 1)])),
           ("span leaves the source", dict(rows=[(1001, 1000, 1)])), ("src behind the source", dict(rows=[(2001, 0, 1)])),
           ("row out of range", dict(rows=[(3, 500, 4)])), ("row < 0", dict(rows=[(3, 500, -1)])),
           ("a row named twice", dict(rows=[(3, 500, 1), (400, 500, 1)])), ("more descriptors than rows", dict(rows=[(0, 1, 0)] * 5)),
           ("destination not aligned", dict(dst_ptr=dst.data_ptr() + 2)), ("source not aligned", dict(src_ptr=src.data_ptr() + 1)),
           # (the rows named lie inside the tensors: without the range checks these two calls would succeed)
           ("destination longer than its allocation", dict(dst_rows=(1 << 40) // (n_mels * T * 4))), ("source longer than its allocation", dict(src_elems=1 << 38)),
           ("destination is host memory", dict(dst_ptr=pinned.data_ptr())), ("source is host memory", dict(src_ptr=host_src.data_ptr())),
           ("frames overflow", dict(frames=1 << 61, rows=[(3, 100, 1)]))]
    bad += [("spec: " + what, dict(spec=s)) for what, s in refused_specs(capi)]
    for what, change in bad:
        assert raw_call(ctx, **dict(good, **change)) == capi.E_INVALID_ARG, what
    ctx.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL).all() and (pinned == 0).all()
    assert raw_call(ctx, **good) == capi.OK, ctx.last_error()  # (the good call is good)
    assert raw_call(ctx, **dict(good, rows=[], n_rows=0)) == capi.OK  # (no descriptor: nothing to do)
    ctx.synchronize()
    body = whole.cpu().numpy().view(np.uint32)[GUARD:-GUARD].reshape(dst_rows, T, n_mels)
    assert (body[[0, 2]] == SENTINEL).all() and np.isfinite(body[[1, 3]].view(np.float32)).all()
    # frames == win is the smallest padded length: one frame
    one_whole, one = guarded(2, n_mels)
    assert raw_call(ctx, **dict(good, frames=400, rows=[(3, 400, 1)], dst_ptr=one.data_ptr(), dst_rows=2)) == capi.OK, ctx.last_error()
    ctx.synchronize()
    body = one_whole.cpu().numpy().view(np.uint32)[GUARD:-GUARD].reshape(2, n_mels)
    assert (body[0] == SENTINEL).all() and np.isfinite(body[1].view(np.float32)).all() and (body[1] != SENTINEL).all()


def test_zz_the_largest_ratio_of_this_file():
    """the record line of the module's docstring comes from here (run with -s)"""
    assert WORST and max(WORST.values()) < 1.0
    for key in sorted(WORST):
        print("largest error / bound  %-40s %.4f" % (key, WORST[key]))
