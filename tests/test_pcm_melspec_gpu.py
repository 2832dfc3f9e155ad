"""vpz_pcm_melspec (include/vorbispizza_pcm_melspec.h, csrc/pcm_melspec.hip) alone: no decoder.

The truth is tests/melspec_truth.py's float64 restatement of the header's definition (numpy.fft.rfft of the float64 windowed frames), the
tolerance its derived bound: re and im within K(n_fft) 2^-24 sum |x| w, K = 45.2, 46.6, 52.3 at n_fft 2048, 4096, 8192, carried into e_P
and e_M and through test_logmel_cpu's check_power / check_log unchanged.  The cases are melspec_truth.CASES: the smallest shapes at
which the kernel can go wrong.  Rows no descriptor names and the guards on either side of the destination keep their sentinel bit for
bit; every refusal returns VPZ_E_INVALID_ARG and writes nothing.

Largest error / bound ratio observed on an MI355X over the parametrised cases: 0.162 (power), at n_fft 8192 with F = 4097 and hop 1, and
0.182 (log10), at the bank with empty bands; 0.149 at the librosa spec (2048 / 512 / 128)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import melspec_truth as mt  # noqa: E402
from logmel_truth import check_log, check_power, mel_weights64, refused_specs, silence_value  # noqa: E402
from melspec_truth import melspec_refused_specs  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

FLOOR = mt.FLOOR
SENTINEL = 0x5A5A5A5A
GUARD = 64
DST_ROWS = mt.DST_ROWS


def make_spec(name, log, bands_first):
    from vorbispizza_amd import capi
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = mt.CASES[name]
    return capi.LogMelSpec.make(sample_rate=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=f_min, f_max=f_max, mel_scale=scale, mel_norm=norm, log=log,
                                floor=FLOOR, bands_first=bands_first)


def guarded(dst_rows, row_elems):
    """a destination of dst_rows * row_elems float32 with GUARD sentinels on either side, every element the sentinel"""
    import torch
    flat = np.full(GUARD + dst_rows * row_elems + GUARD, SENTINEL, dtype=np.uint32)
    whole = torch.from_numpy(flat.view(np.float32).copy()).to("cuda:0")
    return whole, whole[GUARD: GUARD + dst_rows * row_elems]


def rows_back(whole, dst_rows, n_mels, T, bands_first):
    """[row][T][n_mels] float32 of the destination's body, after checking the guards"""
    bits = whole.cpu().numpy().view(np.uint32)
    assert (bits[:GUARD] == SENTINEL).all() and (bits[-GUARD:] == SENTINEL).all()
    body = bits[GUARD:-GUARD].view(np.float32)
    return body.reshape(dst_rows, n_mels, T).transpose(0, 2, 1) if bands_first else body.reshape(dst_rows, T, n_mels)


@pytest.mark.parametrize("bands_first", [True, False], ids=["bands_first", "frames_first"])
@pytest.mark.parametrize("log", [False, True], ids=["power", "log10"])
@pytest.mark.parametrize("name", list(mt.CASES))
def test_rows_against_the_float64_restatement(ctx, name, log, bands_first):
    import torch
    from vorbispizza_amd import capi
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = mt.CASES[name]
    T = 1 + F // hop
    src, rows = mt.case_input(name)
    truths = mt.case_truth(name)
    spec = make_spec(name, log, bands_first)
    whole, dst = guarded(DST_ROWS, n_mels * T)
    d_src = torch.from_numpy(src).to("cuda:0")
    assert capi.pcm_melspec(ctx, d_src, rows, dst.view((DST_ROWS, n_mels, T) if bands_first else (DST_ROWS, T, n_mels)), spec, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    got = rows_back(whole, DST_ROWS, n_mels, T, bands_first)
    named = {row for _, _, row in rows}
    for r in range(DST_ROWS):
        if r not in named:
            assert (got[r].view(np.uint32) == SENTINEL).all(), r
    worst = 0.0
    for (at, L, row), (M, e_M) in zip(rows, truths):
        worst = max(worst, check_log(got[row], M, e_M, FLOOR) if log else check_power(got[row], M, e_M))
        if L == 0:
            assert (got[row].view(np.uint32) == (silence_value(FLOOR).view(np.uint32) if log else 0)).all()
    print("error / bound %s %s: %.4f" % (name, "log10" if log else "power", worst))
    assert worst < 1.0


def test_a_unit_impulse_in_closed_form(ctx):
    """x = 1 at sample p of a long row: a frame that covers p at its sample m has |X[k]| = w[m] for every k, so P[k] = w[m]^2 and
    M[b] = w[m]^2 sum_k W[b][k], within the bound; a frame that does not cover p holds the silence value exactly"""
    import torch
    from vorbispizza_amd import capi
    sr, n_fft, hop, n_mels = 22050, 2048, 512, 128
    F, p = 512 * 20 + 11, 5003
    T = 1 + F // hop
    src = np.zeros(F + 5, dtype=np.float32)
    src[2 + p] = 1.0
    W = mel_weights64(sr, n_fft, n_mels, 0.0, sr / 2.0, "slaney", "slaney")
    w = mt.hann64(n_fft)
    m = p - (np.arange(T) * hop - n_fft // 2)
    covers = (m >= 0) & (m < n_fft)
    closed = np.where(covers, w[np.clip(m, 0, n_fft - 1)] ** 2, 0.0)[:, None] * W.sum(axis=1)[None, :]
    M, e_M = mt.melspec_truth(src[2:], F, F, n_fft, hop, W)
    assert covers.sum() == 4 and np.abs(M - closed).max() <= 1e-12  # (the restatement has the closed form)
    d_src = torch.from_numpy(src).to("cuda:0")
    for log in (False, True):
        spec = capi.LogMelSpec.make(sample_rate=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, log=log, floor=FLOOR)
        whole, dst = guarded(1, n_mels * T)
        assert capi.pcm_melspec(ctx, d_src, [(2, F, 0)], dst.view(1, n_mels, T), spec, F) == capi.OK, ctx.last_error()
        ctx.synchronize()
        got = rows_back(whole, 1, n_mels, T, True)[0]
        assert (got[~covers].view(np.uint32) == (silence_value(FLOOR).view(np.uint32) if log else 0)).all()
        if log:
            check_log(got, closed, e_M, FLOOR)
        else:
            assert (np.abs(got[covers].astype(np.float64) - closed[covers]) <= e_M[covers]).all()


def test_more_descriptors_than_the_grid_holds_side_by_side(ctx):
    """2100 rows of F = 1025 at n_fft 2048, hop 2048 -- one frame per row; the grid's y holds 2048: workgroups take a second descriptor --
    in a destination of 2150 rows.  Rows not named keep the sentinel bit for bit; the source behind every row's L is NaN and must not
    reach the output."""
    import torch
    from vorbispizza_amd import capi
    n, dst_rows, F, n_fft, hop, n_mels = 2100, 2150, 1025, 2048, 2048, 8
    T = 1 + F // hop
    assert T == 1 and n > mt.kernel_constants()["kMsMaxGridY"]
    rng = np.random.default_rng(3)
    stride = F + 3
    Ls = rng.integers(0, F + 1, n)
    Ls[:4] = (F, 0, 1, F - 1)
    src = np.full(1 + n * stride, np.nan, dtype=np.float32)
    x = np.zeros((n, F))
    for i in range(n):
        x[i, : Ls[i]] = (rng.standard_normal(Ls[i]) * 0.5).astype(np.float32)
        src[1 + i * stride: 1 + i * stride + Ls[i]] = x[i, : Ls[i]]
    order = rng.permutation(dst_rows)[:n]
    rows = [(1 + i * stride, int(Ls[i]), int(order[i])) for i in range(n)]
    spec = capi.LogMelSpec.make(sample_rate=22050, n_fft=n_fft, hop=hop, n_mels=n_mels, log=False)
    W = mel_weights64(22050, n_fft, n_mels, 0.0, 11025.0, "slaney", "slaney")
    whole, dst = guarded(dst_rows, n_mels * T)
    assert capi.pcm_melspec(ctx, torch.from_numpy(src).to("cuda:0"), rows, dst.view(dst_rows, n_mels, T), spec, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    got = rows_back(whole, dst_rows, n_mels, T, True)
    assert not np.isnan(got[order]).any()
    rest = np.setdiff1d(np.arange(dst_rows), order)
    assert rest.size == 50 and (got[rest].view(np.uint32) == SENTINEL).all()
    checked = sorted(set(range(0, n, 7)) | set(range(4)) | set(range(2048, 2100)))  # (the rows of the grid's second round among them)
    for i in checked:
        check_power(got[order[i]], *mt.melspec_truth(x[i], int(Ls[i]), F, n_fft, hop, W))


def test_indices_beyond_two_to_the_31(ctx):
    """a window of a source and the last rows of a destination whose element indices do not fit 32 bits"""
    import torch
    from vorbispizza_amd import capi
    F, n_fft, hop, n_mels = 2000, 2048, 16, 8
    T = 1 + F // hop
    dst_rows = (1 << 31) // (n_mels * T) + 8
    src = torch.empty((1 << 31) + 8192, dtype=torch.float32, device="cuda:0")
    tail = (np.random.default_rng(4).standard_normal(8192) * 0.5).astype(np.float32)
    src[1 << 31:] = torch.from_numpy(tail).to("cuda:0")
    wins = [(7, 2000, 2), (2101, 333, 0)]  # (offsets inside the tail, rows from the end)
    W = mel_weights64(22050, n_fft, n_mels, 0.0, 11025.0, "slaney", "slaney")
    for bands_first in (True, False):
        dst = torch.empty((dst_rows, n_mels, T) if bands_first else (dst_rows, T, n_mels), dtype=torch.float32, device="cuda:0")
        dst[-3:] = 7.0
        assert (dst_rows - 3) * n_mels * T > 1 << 31
        rows = [((1 << 31) + at, L, dst_rows - 3 + r) for at, L, r in wins]
        spec = capi.LogMelSpec.make(sample_rate=22050, n_fft=n_fft, hop=hop, n_mels=n_mels, log=False, bands_first=bands_first)
        assert capi.pcm_melspec(ctx, src, rows, dst, spec, F) == capi.OK, ctx.last_error()
        ctx.synchronize()
        got = dst[-3:].cpu().numpy()
        got = got.transpose(0, 2, 1) if bands_first else got
        assert (got[1] == 7.0).all()
        for at, L, r in wins:
            check_power(got[r], *mt.melspec_truth(tail[at: at + L], L, F, n_fft, hop, W))
        del dst


def test_bits_by_placement(ctx):
    """A frame's bits depend on its own n_fft samples only: a window alone, among hundreds, at another destination row, and in a launch
    that picks another tile size (the same n_fft and samples at a hop the plan gives 8-frame tiles, where frames at the same sample
    offsets coincide) carry the same bits."""
    import torch
    from vorbispizza_amd import capi
    n_fft, n_mels, hop, big = 4096, 64, 1024, 2048
    assert mt.tile_plan(n_fft, hop)[0] == 16 and mt.tile_plan(n_fft, big)[0] == 8
    F, many = 1024 * 40 + 37, 301
    T, Tb = 1 + F // hop, 1 + F // big
    rng = np.random.default_rng(21)
    host = (rng.standard_normal(6 * F) * 0.5).astype(np.float32)
    src = torch.from_numpy(host).to("cuda:0")
    spec = capi.LogMelSpec.make(sample_rate=44100, n_fft=n_fft, hop=hop, n_mels=n_mels, floor=FLOOR)
    win = (2 * F + 5, F - 300)
    alone = torch.zeros((1, n_mels, T), dtype=torch.float32, device="cuda:0")
    assert capi.pcm_melspec(ctx, src, [win + (0,)], alone, spec, F) == capi.OK, ctx.last_error()
    crowd = torch.zeros((many, n_mels, T), dtype=torch.float32, device="cuda:0")
    crowd_rows = [win + (many - 7,)] + [(i * 67 + 1, F - int(rng.integers(0, 500)), (i * 5) % many) for i in range(many) if (i * 5) % many != many - 7]
    assert len(crowd_rows) == many
    assert capi.pcm_melspec(ctx, src, crowd_rows, crowd, spec, F) == capi.OK, ctx.last_error()
    other = torch.zeros((1, n_mels, Tb), dtype=torch.float32, device="cuda:0")
    spec_b = capi.LogMelSpec.make(sample_rate=44100, n_fft=n_fft, hop=big, n_mels=n_mels, floor=FLOOR)
    assert capi.pcm_melspec(ctx, src, [win + (0,)], other, spec_b, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    a, c, o = alone[0].cpu().numpy(), crowd[many - 7].cpu().numpy(), other[0].cpu().numpy()
    assert a.view(np.uint32).tobytes() == c.view(np.uint32).tobytes()
    assert o.view(np.uint32).tobytes() == a[:, ::2].copy().view(np.uint32).tobytes() and o.shape[1] == (T + 1) // 2
    W = mel_weights64(44100, n_fft, n_mels, 0.0, 22050.0, "slaney", "slaney")
    for at, L, row in (crowd_rows[0], crowd_rows[150], crowd_rows[300]):
        assert check_log(crowd[row].cpu().numpy().T, *mt.melspec_truth(host[at: at + L], L, F, n_fft, hop, W), FLOOR) < 1.0


@pytest.mark.parametrize("n_fft", mt.NFFTS)
def test_bits_by_frame(ctx, n_fft):
    """hop = n_fft, F = 3 n_fft: frame 1 covers samples [n_fft / 2, 3 n_fft / 2).  Row A holds noise of amplitude 1e-4 there and zeros
    elsewhere, row B the same samples there and noise of amplitude 0.5 elsewhere: frame 1 of both carries the same bits in every band.
    (A kernel that packs two real frames into one complex transform fails here.)"""
    import torch
    from vorbispizza_amd import capi
    hop, F, n_mels = n_fft, 3 * n_fft, 128
    T = 1 + F // hop
    rng = np.random.default_rng(n_fft)
    quiet = (rng.standard_normal(n_fft) * 1e-4).astype(np.float32)
    A = np.zeros(F, dtype=np.float32)
    B = (rng.standard_normal(F) * 0.5).astype(np.float32)
    A[n_fft // 2: 3 * n_fft // 2] = quiet
    B[n_fft // 2: 3 * n_fft // 2] = quiet
    src = torch.from_numpy(np.concatenate([A, B])).to("cuda:0")
    for log in (False, True):
        spec = capi.LogMelSpec.make(sample_rate=44100, n_fft=n_fft, hop=hop, n_mels=n_mels, log=log, floor=1e-30)
        dst = torch.zeros((2, n_mels, T), dtype=torch.float32, device="cuda:0")
        assert capi.pcm_melspec(ctx, src, [(0, F, 0), (F, F, 1)], dst, spec, F) == capi.OK, ctx.last_error()
        ctx.synchronize()
        got = dst.cpu().numpy()
        assert got[0, :, 1].view(np.uint32).tobytes() == got[1, :, 1].view(np.uint32).tobytes()
        assert not np.array_equal(got[0, :, 0], got[1, :, 0]) and not np.array_equal(got[0, :, 2], got[1, :, 2])
        if not log:
            W = mel_weights64(44100, n_fft, n_mels, 0.0, 22050.0, "slaney", "slaney")
            check_power(got[0].T, *mt.melspec_truth(A, F, F, n_fft, hop, W))
            check_power(got[1].T, *mt.melspec_truth(B, F, F, n_fft, hop, W))


def raw_call(ctx, src_ptr, src_elems, frames, spec, rows, dst_ptr, dst_rows, n_rows=None, null_rows=False, handle=True, null_spec=False):
    from vorbispizza_amd import capi
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    return capi.lib().vpz_pcm_melspec(ctx._h if handle else None, src_ptr, src_elems, frames, None if null_spec else C.byref(spec),
                                      desc.shape[0] if n_rows is None else n_rows, None if null_rows else desc.ctypes.data, dst_ptr, dst_rows)


def test_every_refusal_is_invalid_arg_and_writes_nothing(ctx):
    import torch
    from vorbispizza_amd import capi
    F, dst_rows, n_mels = 2500, 4, 128
    T = 1 + F // 512
    src = torch.from_numpy((np.random.default_rng(9).standard_normal(8000) * 0.5).astype(np.float32)).to("cuda:0")
    whole, dst = guarded(dst_rows, n_mels * T)
    spec = capi.LogMelSpec.make(sample_rate=22050, n_fft=2048, hop=512, n_mels=n_mels)
    good = dict(src_ptr=src.data_ptr(), src_elems=8000, frames=F, spec=spec, rows=[(3, 100, 1), (400, 2500, 3)], dst_ptr=dst.data_ptr(), dst_rows=dst_rows)
    pinned = torch.zeros(dst_rows * n_mels * T, dtype=torch.float32, pin_memory=True)
    host_src = torch.full((8000,), 0.5, dtype=torch.float32, pin_memory=True)
    bad = [("no context", dict(handle=False)), ("null source", dict(src_ptr=None)), ("null destination", dict(dst_ptr=None)), ("null rows", dict(null_rows=True)),
           ("null spec", dict(null_spec=True)), ("frames < n_fft / 2 + 1", dict(frames=1024, rows=[(3, 100, 1)])), ("n_rows < 0", dict(n_rows=-1)),
           ("dst_rows < 0", dict(dst_rows=-1)), ("src_elems < 0", dict(src_elems=-1)), ("samples > frames", dict(rows=[(3, 2501, 1)])),
           ("samples < 0", dict(rows=[(3, -1, 1)])), ("src < 0", dict(rows=[(-1, 10, 1)])), ("span leaves the source", dict(rows=[(5501, 2500, 1)])),
           ("src behind the source", dict(rows=[(8001, 0, 1)])), ("row out of range", dict(rows=[(3, 100, 4)])), ("row < 0", dict(rows=[(3, 100, -1)])),
           ("a row named twice", dict(rows=[(3, 100, 1), (400, 100, 1)])), ("more descriptors than rows", dict(rows=[(0, 1, 0)] * 5)),
           ("destination not aligned", dict(dst_ptr=dst.data_ptr() + 2)), ("source not aligned", dict(src_ptr=src.data_ptr() + 1)),
           # (the rows named lie inside the tensors: without the range checks these two calls would succeed)
           ("destination longer than its allocation", dict(dst_rows=(1 << 40) // (n_mels * T * 4))), ("source longer than its allocation", dict(src_elems=1 << 38)),
           ("destination is host memory", dict(dst_ptr=pinned.data_ptr())), ("source is host memory", dict(src_ptr=host_src.data_ptr())),
           ("frames overflow", dict(frames=1 << 61, rows=[(3, 100, 1)]))]
    specs = melspec_refused_specs(capi)
    assert {"n_fft 1024", "a reserved word"} <= {what for what, _ in specs}
    bad += [("spec: " + what, dict(spec=s)) for what, s in specs]
    for what, change in bad:
        assert raw_call(ctx, **dict(good, **change)) == capi.E_INVALID_ARG, what
    ctx.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL).all() and (pinned == 0).all()
    assert raw_call(ctx, **good) == capi.OK, ctx.last_error()  # (the good call is good)
    assert raw_call(ctx, **dict(good, rows=[], n_rows=0)) == capi.OK  # (no descriptor: nothing to do)
    ctx.synchronize()
    got = rows_back(whole, dst_rows, n_mels, T, True)
    assert (got[[0, 2]].view(np.uint32) == SENTINEL).all() and np.isfinite(got[[1, 3]]).all()
