"""vpz_pcm_stft (include/vorbispizza_pcm_stft.h, csrc/pcm_stft.hip) alone: no decoder.

The truth is tests/stft_truth.py's float64 restatement of the header's definition (numpy.fft.rfft of the float64 windowed frames, held to
torch.stft by tests/test_stft_cpu.py), the tolerance its derived bounds: Re and Im within d = K(n_fft) 2^-24 sum |x| w, K = 38.1, 39.5,
45.2, 46.6, 52.3 at n_fft 512 .. 8192; power within 2 |re| d + 2 |im| d + 2 d^2 + 3 u P; magnitude within sqrt(2) d + 3 u |X|.  Every
element of every named row is held to it -- no log, no floor, none exempt -- for all three outputs and both layouts, and the COMPLEX and
POWER outputs are the float32 restatement's values besides.  The cases are stft_truth.CASES: the smallest shapes at which the kernel can go
wrong.  Rows no descriptor names and the guards on either side of the destination keep their sentinel bit for bit; every refusal returns
VPZ_E_INVALID_ARG and writes nothing.

Largest error / bound observed on an MI355X over the parametrised cases: 0.141 (complex), 0.136 (power) and 0.115 (magnitude), all at
n_fft 512 with F = 257 and hop 1; 0.127 at 2048 / 441; 0.019 at 1024 / 256 and 0.009 at
4096 / 1024.  The same in both layouts: the values are."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stft_truth as st  # noqa: E402
from logmel_truth import frames_of  # noqa: E402
from stft_truth import stft_refused_specs  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD = 64
DST_ROWS = st.DST_ROWS


def guarded(n_floats):
    """a destination of n_floats float32 with GUARD sentinels on either side, every element the sentinel"""
    import torch
    flat = np.full(GUARD + n_floats + GUARD, SENTINEL, dtype=np.uint32)
    whole = torch.from_numpy(flat.view(np.float32).copy()).to("cuda:0")
    return whole, whole[GUARD: GUARD + n_floats]


def as_frames(body, dst_rows, spec):
    """[row][T][n_freq] -- complex64 or float32 -- of a destination's float32 body"""
    from vorbispizza_amd import capi
    a = np.ascontiguousarray(body).reshape((dst_rows,) + spec.row_shape_of)
    if spec.output == capi.STFT_COMPLEX:
        a = a.view(np.complex64)[..., 0]
    return np.ascontiguousarray(a.transpose(0, 2, 1)) if spec.layout == capi.STFT_BINS_FIRST else a


def stft(ctx, d_src, rows, F, dst_rows, n_fft, hop, win_length=None, window="hann", output="complex", bins_first=True):
    """one guarded launch -> [dst_rows][T][n_freq]"""
    from vorbispizza_amd import capi
    spec = capi.StftSpec.make(n_fft=n_fft, hop=hop, win_length=win_length, window=window, output=output, bins_first=bins_first)
    spec.row_shape_of = spec.row_shape(F)
    per_row = int(np.prod(spec.row_shape_of))
    whole, dst = guarded(dst_rows * per_row)
    assert capi.pcm_stft(ctx, d_src, rows, dst.view((dst_rows,) + spec.row_shape_of), spec, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    bits = whole.cpu().numpy().view(np.uint32)
    assert (bits[:GUARD] == SENTINEL).all() and (bits[-GUARD:] == SENTINEL).all()
    return as_frames(bits[GUARD:-GUARD].view(np.float32), dst_rows, spec)


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint32) == SENTINEL).all()


WORST = {}


@pytest.mark.parametrize("bins_first", [True, False], ids=["bins_first", "frames_first"])
@pytest.mark.parametrize("name", list(st.CASES))
def test_rows_against_the_truth_and_the_restatement(ctx, name, bins_first):
    import torch
    n_fft, hop, win_length, window, F, tc, tr = st.CASES[name]
    T = 1 + F // hop
    src, rows = st.case_input(name)
    truths, restated = st.case_truth(name), st.case_restated(name)
    d_src = torch.from_numpy(src).to("cuda:0")
    named = {row for _, _, row in rows}
    for output in st.OUTPUTS:
        got = stft(ctx, d_src, rows, F, DST_ROWS, n_fft, hop, win_length, window, output, bins_first)
        assert got.shape == (DST_ROWS, T, n_fft // 2 + 1)
        for r in range(DST_ROWS):
            if r not in named:
                assert untouched(got[r]), r
        worst = 0.0
        for (at, L, row), (Z, d), want in zip(rows, truths, restated):
            worst = max(worst, st.check_output(output, got[row], Z, d))
            if output != "magnitude":
                assert np.array_equal(got[row], want[output]), (output, row, int((got[row] != want[output]).sum()))
            if L == 0:
                assert (got[row] == 0).all()
        print("error / bound %s %s %s: %.4f" % (name, output, "bins first" if bins_first else "frames first", worst))
        WORST[output] = max(WORST.get(output, 0.0), worst)
        assert worst < 1.0
    print("largest error / bound so far: %s" % WORST)


@pytest.mark.parametrize("n_fft,hop,win_length,window", [(1024, 256, 800, "hamming"), (2048, 512, 2048, "hann"), (512, 100, 511, "hann")])
def test_a_unit_impulse_in_closed_form(ctx, n_fft, hop, win_length, window):
    """x = 1 at sample p of a long row, away from both ends: a frame that covers p at its sample m has X[k] = w[m] e^(-2 pi i m k / n_fft),
    within d = K u w[m]; a frame that does not cover p is zeros exactly"""
    import torch
    F = hop * 40 + 11
    p = hop * 20 + 3
    T = 1 + F // hop
    src = np.zeros(F + 5, dtype=np.float32)
    src[2 + p] = 1.0
    w = st.window64(n_fft, win_length, window)
    m = p - (np.arange(T) * hop - n_fft // 2)
    covers = (m >= 0) & (m < n_fft)
    k = np.arange(n_fft // 2 + 1)
    closed = np.where(covers, w[np.clip(m, 0, n_fft - 1)], 0.0)[:, None] * np.exp(-2j * np.pi * ((m[:, None] * k[None, :]) % n_fft) / n_fft)
    Z, d = st.truth(frames_of(src[2:], F, F, n_fft, hop), n_fft, w)
    assert covers.sum() >= 4 and np.abs(Z - closed).max() <= 1e-12  # (the restatement has the closed form)
    d_src = torch.from_numpy(src).to("cuda:0")
    for bins_first in (True, False):
        for output in st.OUTPUTS:
            got = stft(ctx, d_src, [(2, F, 0)], F, 1, n_fft, hop, win_length, window, output, bins_first)[0]
            assert (got[~covers] == 0).all()
            st.check_output(output, got, closed, d)


def test_more_descriptors_than_the_grid_holds_side_by_side(ctx):
    """2100 rows of F = 257 at n_fft 512, hop 512 -- one frame per row, one of the four a workgroup could carry; the grid's y holds 2048:
    workgroups take a second descriptor -- in a destination of 2150 rows.  Rows not named keep the sentinel bit for bit; the source behind
    every row's L is NaN and must not reach the output."""
    import torch
    n, dst_rows, F, n_fft, hop = 2100, 2150, 257, 512, 512
    assert 1 + F // hop == 1 and n > st.kernel_constants()["kStMaxGridY"]
    rng = np.random.default_rng(3)
    stride = F + 3
    Ls = rng.integers(0, F + 1, n)
    Ls[:4] = (F, 0, 1, F - 1)
    src = np.full(1 + n * stride, np.nan, dtype=np.float32)
    x = np.zeros((n, F), dtype=np.float32)
    for i in range(n):
        x[i, : Ls[i]] = (rng.standard_normal(Ls[i]) * 0.5).astype(np.float32)
        src[1 + i * stride: 1 + i * stride + Ls[i]] = x[i, : Ls[i]]
    order = rng.permutation(dst_rows)[:n]
    rows = [(1 + i * stride, int(Ls[i]), int(order[i])) for i in range(n)]
    w64, (w, t) = st.window64(n_fft), st.tables32(n_fft)
    X = np.concatenate([frames_of(x[i], int(Ls[i]), F, n_fft, hop) for i in range(n)])
    Z, d = st.truth(X, n_fft, w64)
    want = st.outputs32(*st.network32(X.astype(np.float32), n_fft, w, t))
    d_src = torch.from_numpy(src).to("cuda:0")
    for output, bins_first in (("complex", True), ("power", False)):
        got = stft(ctx, d_src, rows, F, dst_rows, n_fft, hop, output=output, bins_first=bins_first)
        assert not np.isnan(got[order]).any()
        rest = np.setdiff1d(np.arange(dst_rows), order)
        assert rest.size == 50 and untouched(got[rest])
        st.check_output(output, got[order, 0], Z, d)
        assert np.array_equal(got[order, 0], want[output])


def test_indices_beyond_two_to_the_31(ctx):
    """the last rows of a destination whose element indices do not fit 32 bits, in both layouts"""
    import torch
    from vorbispizza_amd import capi
    F, n_fft, hop = 2000, 512, 16
    T, NF = 1 + F // hop, n_fft // 2 + 1
    tail = (np.random.default_rng(4).standard_normal(8192) * 0.5).astype(np.float32)
    src = torch.from_numpy(tail).to("cuda:0")
    wins = [(7, 2000, 2), (2101, 333, 0)]  # (rows counted from the third last)
    w64 = st.window64(n_fft)
    for output, bins_first in (("power", True), ("complex", False)):
        spec = capi.StftSpec.make(n_fft=n_fft, hop=hop, output=output, bins_first=bins_first)
        shape = spec.row_shape(F)
        per_row = int(np.prod(shape))
        dst_rows = (1 << 31) // per_row + 8
        dst = torch.empty((dst_rows,) + shape, dtype=torch.float32, device="cuda:0")
        dst[-3:] = 7.0
        assert (dst_rows - 3) * per_row > 1 << 31
        rows = [(at, L, dst_rows - 3 + r) for at, L, r in wins]
        assert capi.pcm_stft(ctx, src, rows, dst, spec, F) == capi.OK, ctx.last_error()
        ctx.synchronize()
        spec.row_shape_of = shape
        got = as_frames(dst[-3:].cpu().numpy(), 3, spec)
        assert (np.ascontiguousarray(got[1]).view(np.float32) == 7.0).all()
        for at, L, r in wins:
            st.check_output(output, got[r], *st.truth(frames_of(tail[at: at + L], L, F, n_fft, hop), n_fft, w64))
        del dst


def test_bits_by_placement(ctx):
    """A window's bits do not depend on where it is placed: the same samples at another source offset, at another destination row and
    among hundreds of other rows carry the same bits, in both layouts"""
    import torch
    n_fft, hop, many = 1024, 256, 301
    F = 256 * 30 + 37
    rng = np.random.default_rng(21)
    host = (rng.standard_normal(6 * F) * 0.5).astype(np.float32)
    L = F - 300
    host[4 * F + 2: 4 * F + 2 + L] = host[2 * F + 5: 2 * F + 5 + L]  # the same window once more, at an even offset
    src = torch.from_numpy(host).to("cuda:0")
    for output, bins_first in (("complex", True), ("complex", False), ("magnitude", True), ("power", False)):
        alone = stft(ctx, src, [(2 * F + 5, L, 0)], F, 1, n_fft, hop, output=output, bins_first=bins_first)[0]
        moved = stft(ctx, src, [(4 * F + 2, L, 3)], F, 5, n_fft, hop, output=output, bins_first=bins_first)[3]
        crowd_rows = [(2 * F + 5, L, many - 7)] + [(i * 67 + 1, F - int(rng.integers(0, 500)), (i * 5) % many) for i in range(many) if (i * 5) % many != many - 7]
        assert len(crowd_rows) == many
        crowd = stft(ctx, src, crowd_rows, F, many, n_fft, hop, output=output, bins_first=bins_first)[many - 7]
        assert alone.tobytes() == moved.tobytes() == crowd.tobytes()
        st.check_output(output, alone, *st.truth(frames_of(host[2 * F + 5: 2 * F + 5 + L], L, F, n_fft, hop), n_fft, st.window64(n_fft)))


@pytest.mark.parametrize("n_fft", st.NFFTS)
def test_bits_by_frame(ctx, n_fft):
    """hop = n_fft / 4, F = 40 hops.  Row A holds one block of n_fft quiet samples exactly under frame 5 and zeros elsewhere, row B the
    same block under frame 18 and loud noise elsewhere: the two frames -- at another t, at another place in their tiles (and, where a
    workgroup carries frames side by side, in another group of lanes), in another row -- carry the same bits in every bin, for every output
    and layout, while their neighbours differ.  (A kernel that packs two real frames into one complex transform fails here.)"""
    import torch
    hop = n_fft // 4
    F, tA, tB = 40 * hop, 5, 18
    k = st.kernel_constants()
    for output in ("complex", "power"):
        tile = st.tile_plan(n_fft, hop, output, True, k)[0]
        assert tile == 1 or tA % tile != tB % tile
    rng = np.random.default_rng(n_fft)
    quiet = (rng.standard_normal(n_fft) * 1e-4).astype(np.float32)
    A = np.zeros(F, dtype=np.float32)
    B = (rng.standard_normal(F) * 0.5).astype(np.float32)
    A[tA * hop - n_fft // 2: tA * hop + n_fft // 2] = quiet
    B[tB * hop - n_fft // 2: tB * hop + n_fft // 2] = quiet
    src = torch.from_numpy(np.concatenate([A, B])).to("cuda:0")
    w, t = st.tables32(n_fft)
    want = st.outputs32(*st.network32(quiet[None, :], n_fft, w, t))
    for output in st.OUTPUTS:
        for bins_first in (True, False):
            got = stft(ctx, src, [(0, F, 2), (F, F, 0)], F, 3, n_fft, hop, output=output, bins_first=bins_first)
            assert untouched(got[1])
            assert got[2, tA].tobytes() == got[0, tB].tobytes()
            assert not np.array_equal(got[2, tA - 1], got[0, tB - 1]) and not np.array_equal(got[2, tA + 1], got[0, tB + 1])
            if output != "magnitude":
                assert np.array_equal(got[2, tA], want[output][0])


def raw_call(ctx, src_ptr, src_elems, frames, spec, rows, dst_ptr, dst_rows, n_rows=None, null_rows=False, handle=True, null_spec=False):
    from vorbispizza_amd import capi
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    return capi.lib().vpz_pcm_stft(ctx._h if handle else None, src_ptr, src_elems, frames, None if null_spec else C.byref(spec),
                                   desc.shape[0] if n_rows is None else n_rows, None if null_rows else desc.ctypes.data, dst_ptr, dst_rows)


def test_every_refusal_is_invalid_arg_and_writes_nothing(ctx):
    import torch
    from vorbispizza_amd import capi
    F, dst_rows = 2500, 4
    spec = capi.StftSpec.make(n_fft=2048, hop=512)
    per_row = int(np.prod(spec.row_shape(F)))
    src = torch.from_numpy((np.random.default_rng(9).standard_normal(8000) * 0.5).astype(np.float32)).to("cuda:0")
    whole, dst = guarded(dst_rows * per_row)
    good = dict(src_ptr=src.data_ptr(), src_elems=8000, frames=F, spec=spec, rows=[(3, 100, 1), (400, 2500, 3)], dst_ptr=dst.data_ptr(), dst_rows=dst_rows)
    pinned = torch.zeros(dst_rows * per_row, dtype=torch.float32, pin_memory=True)
    host_src = torch.full((8000,), 0.5, dtype=torch.float32, pin_memory=True)
    bad = [("no context", dict(handle=False)), ("null source", dict(src_ptr=None)), ("null destination", dict(dst_ptr=None)), ("null rows", dict(null_rows=True)),
           ("null spec", dict(null_spec=True)), ("frames < n_fft / 2 + 1", dict(frames=1024, rows=[(3, 100, 1)])), ("n_rows < 0", dict(n_rows=-1)),
           ("dst_rows < 0", dict(dst_rows=-1)), ("src_elems < 0", dict(src_elems=-1)), ("samples > frames", dict(rows=[(3, 2501, 1)])),
           ("samples < 0", dict(rows=[(3, -1, 1)])), ("src < 0", dict(rows=[(-1, 10, 1)])), ("span leaves the source", dict(rows=[(5501, 2500, 1)])),
           ("src behind the source", dict(rows=[(8001, 0, 1)])), ("row out of range", dict(rows=[(3, 100, 4)])), ("row < 0", dict(rows=[(3, 100, -1)])),
           ("a row named twice", dict(rows=[(3, 100, 1), (400, 100, 1)])), ("more descriptors than rows", dict(rows=[(0, 1, 0)] * 5)),
           ("destination not aligned", dict(dst_ptr=dst.data_ptr() + 2)), ("source not aligned", dict(src_ptr=src.data_ptr() + 1)),
           ("complex destination not aligned to a pair", dict(dst_ptr=dst.data_ptr() + 4, dst_rows=dst_rows - 1, rows=[(3, 100, 1)])),
           # (the rows named lie inside the tensors: without the range checks these two calls would succeed)
           ("destination longer than its allocation", dict(dst_rows=(1 << 40) // (per_row * 4))), ("source longer than its allocation", dict(src_elems=1 << 38)),
           ("destination is host memory", dict(dst_ptr=pinned.data_ptr())), ("source is host memory", dict(src_ptr=host_src.data_ptr())),
           ("frames overflow", dict(frames=1 << 61, rows=[(3, 100, 1)]))]
    specs = stft_refused_specs(capi)
    assert {"n_fft 256", "a reserved word", "win_length < 2", "output 3"} <= {what for what, _ in specs}
    bad += [("spec: " + what, dict(spec=s)) for what, s in specs]
    for what, change in bad:
        assert raw_call(ctx, **dict(good, **change)) == capi.E_INVALID_ARG, what
    ctx.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL).all() and (pinned == 0).all()
    # (a float32 destination at an odd float is fine where no pairs are stored)
    power = capi.StftSpec.make(n_fft=2048, hop=512, output="power")
    assert raw_call(ctx, **dict(good, spec=power, dst_ptr=dst.data_ptr() + 4, rows=[(3, 100, 1)])) == capi.OK, ctx.last_error()
    ctx.synchronize()
    whole.copy_(torch.from_numpy(np.full(whole.numel(), SENTINEL, dtype=np.uint32).view(np.float32)))
    assert raw_call(ctx, **good) == capi.OK, ctx.last_error()  # (the good call is good)
    assert raw_call(ctx, **dict(good, rows=[], n_rows=0)) == capi.OK  # (no descriptor: nothing to do)
    ctx.synchronize()
    spec.row_shape_of = spec.row_shape(F)
    got = as_frames(whole.cpu().numpy()[GUARD:-GUARD], dst_rows, spec)
    assert untouched(got[[0, 2]]) and np.isfinite(got[[1, 3]]).all()
