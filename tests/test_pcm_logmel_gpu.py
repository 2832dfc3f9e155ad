"""vpz_pcm_logmel (include/vorbispizza_pcm_logmel.h, csrc/pcm_logmel.hip) alone: no decoder.

The truth is tests/test_logmel_cpu.py's float64 restatement of the header's definition, and the tolerance its derived bound e_M (u = 2^-24,
fmaf chains of length n_fft over once-rounded coefficients, then of a band's live bins); the kernel sums in exactly that order -- m
ascending on the float32 MFMA, k ascending in the band stage --, so the bound is used as it stands.  The power output lies within e_M
and is exactly 0 where e_M is 0; the log10 output follows test_logmel_cpu.check_log.  Rows no descriptor names and the guards on either
side of the destination keep their sentinel bit for bit; every refusal returns VPZ_E_INVALID_ARG and writes nothing.

Largest error / bound ratio observed on an MI355X over the parametrised cases: 0.036 (power) and 0.142 (log10), both at n_fft 32 with one band;
0.0085 and 0.020 at the Whisper spec."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from logmel_truth import check_log, check_power, logmel_truth, mel_weights64, refused_specs, silence_value  # noqa: E402
from pcm_support import LOGMEL_DST_ROWS as DST_ROWS, FLOOR, SENTINEL, guarded, rows_back  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu


# name: (sample_rate, n_fft, hop, n_mels, f_min, f_max, mel_scale, mel_norm, F) -- F so that T = 1 + F // hop is no multiple of the frame
# tile and the last tile is a partial one.  These launches are small, so their tiles are 32 frames (16 at n_fft = hop = 1024, where the LDS
# holds no more); test_a_window_alone_and_among_hundreds_gives_the_same_bits has a launch of 64-frame tiles
SPECS = {
    "whisper_400_160_80": (16000, 400, 160, 80, 0.0, 8000.0, "slaney", "slaney", 160 * 70 + 37),  # T = 71
    "htk_512_128_64": (22050, 512, 128, 64, 20.0, 11025.0, "htk", None, 128 * 75 + 5),            # T = 76
    "odd_96_17_13": (8000, 96, 17, 13, 100.0, 3800.0, "slaney", None, 17 * 70 + 3),               # T = 71
    "widest_1024_1024_256": (48000, 1024, 1024, 256, 0.0, 24000.0, "htk", "slaney", 1024 * 18 + 100),  # T = 19
    "smallest_32_1_1": (16000, 32, 1, 1, 0.0, 8000.0, "slaney", "slaney", 100),                   # T = 101
}


def make_spec(name, log, bands_first):
    from vorbispizza_amd import capi
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F = SPECS[name]
    return capi.LogMelSpec.make(sample_rate=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=f_min, f_max=f_max, mel_scale=scale, mel_norm=norm, log=log,
                                floor=FLOOR, bands_first=bands_first)


def weights_of(name):
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F = SPECS[name]
    return mel_weights64(sr, n_fft, n_mels, f_min, f_max, scale, norm)


_CASES = {}


def case_of(name):
    """the source, the descriptors and the float64 truth of a spec's rows: computed once, shared by its four parametrised tests"""
    if name in _CASES:
        return _CASES[name]
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F = SPECS[name]
    rng = np.random.default_rng(1000 * hop + n_fft)
    W = weights_of(name)
    # L = F (real samples reflect at both ends), F - 1 (the reflected tail starts at the one zero), a third (silent tiles behind it), 1, 0
    Ls = [F, F - 1, F // 3, 1, 0]
    src = (rng.standard_normal(3 * F + 64) * 0.5).astype(np.float32)
    order = rng.permutation(DST_ROWS)[: len(Ls)]
    # (the rows share one source array at odd offsets, and overlap in it)
    rows = [(1 + 2 * i * (F // 5), L, int(row)) for i, (L, row) in enumerate(zip(Ls, order))]
    assert all(a % 2 == 1 and a + L <= src.size for a, L, _ in rows)
    truths = [logmel_truth(src[a: a + L], L, F, n_fft, hop, W) for a, L, _ in rows]
    _CASES[name] = (src, rows, truths)
    return _CASES[name]


RATIOS = {}


@pytest.mark.parametrize("bands_first", [True, False], ids=["bands_first", "frames_first"])
@pytest.mark.parametrize("log", [False, True], ids=["power", "log10"])
@pytest.mark.parametrize("name", list(SPECS))
def test_rows_against_the_float64_restatement(ctx, name, log, bands_first):
    import torch
    from vorbispizza_amd import capi
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F = SPECS[name]
    T = 1 + F // hop
    src, rows, truths = case_of(name)
    spec = make_spec(name, log, bands_first)
    whole, dst = guarded(DST_ROWS, n_mels * T)
    d_src = torch.from_numpy(src).to("cuda:0")
    assert capi.pcm_logmel(ctx, d_src, rows, dst.view((DST_ROWS, n_mels, T) if bands_first else (DST_ROWS, T, n_mels)), spec, F) == capi.OK, ctx.last_error()
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
    RATIOS[(name, log)] = worst
    print("error / bound %s %s: %.4f" % (name, "log10" if log else "power", worst))
    assert worst < 1.0


@pytest.mark.parametrize("name", ["whisper_400_160_80", "odd_96_17_13", "smallest_32_1_1", "widest_1024_1024_256"])
def test_the_smallest_padded_length(ctx, name):
    """F = n_fft / 2 + 1 = L: the reflection reaches the row's other end from both sides"""
    import torch
    from vorbispizza_amd import capi
    sr, n_fft, hop, n_mels = SPECS[name][:4]
    F = n_fft // 2 + 1
    T = 1 + F // hop
    rng = np.random.default_rng(n_fft)
    src = (rng.standard_normal(F + 8) * 0.5).astype(np.float32)
    W = weights_of(name)
    whole, dst = guarded(2, n_mels * T)
    assert capi.pcm_logmel(ctx, torch.from_numpy(src).to("cuda:0"), [(3, F, 1)], dst.view(2, n_mels, T), make_spec(name, False, True), F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    got = rows_back(whole, 2, n_mels, T, True)
    assert (got[0].view(np.uint32) == SENTINEL).all()
    assert check_power(got[1], *logmel_truth(src[3: 3 + F], F, F, n_fft, hop, W)) < 1.0


def test_a_unit_impulse_in_closed_form(ctx):
    """x = 1 at sample p of a long row: a frame that covers p at its sample m has re = w[m] cos, im = w[m] sin, so P[k] = w[m]^2 for every k
    and M[b] = w[m]^2 sum_k W[b][k], within the bound; a frame that does not cover p holds the silence value exactly"""
    import torch
    from vorbispizza_amd import capi
    name = "whisper_400_160_80"
    sr, n_fft, hop, n_mels = SPECS[name][:4]
    F, p = 160 * 40 + 11, 2999
    T = 1 + F // hop
    src = np.zeros(F + 5, dtype=np.float32)
    src[2 + p] = 1.0
    W = weights_of(name)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    m = p - (np.arange(T) * hop - n_fft // 2)
    covers = (m >= 0) & (m < n_fft)
    closed = np.where(covers, w[np.clip(m, 0, n_fft - 1)] ** 2, 0.0)[:, None] * W.sum(axis=1)[None, :]
    M, e_M = logmel_truth(src[2:], F, F, n_fft, hop, W)
    assert covers.sum() in (2, 3) and np.abs(M - closed).max() <= 1e-12  # (the restatement has the closed form)
    d_src = torch.from_numpy(src).to("cuda:0")
    for log in (False, True):
        whole, dst = guarded(1, n_mels * T)
        assert capi.pcm_logmel(ctx, d_src, [(2, F, 0)], dst.view(1, n_mels, T), make_spec(name, log, True), F) == capi.OK, ctx.last_error()
        ctx.synchronize()
        got = rows_back(whole, 1, n_mels, T, True)[0]
        assert (got[~covers].view(np.uint32) == (silence_value(FLOOR).view(np.uint32) if log else 0)).all()
        if log:
            check_log(got, closed, e_M, FLOOR)
        else:
            assert (np.abs(got[covers].astype(np.float64) - closed[covers]) <= e_M[covers]).all()


def test_more_descriptors_than_the_grid_holds_side_by_side(ctx):
    """3000 rows of F = 64 at n_fft 32 (the grid's y holds 2048: workgroups take a second descriptor), in a destination of 3100 rows.  Rows
    not named keep the sentinel bit for bit; the source behind every row's L is NaN and must not reach the output."""
    import torch
    from vorbispizza_amd import capi
    n, dst_rows, F, n_fft, hop, n_mels = 3000, 3100, 64, 32, 16, 8
    T = 1 + F // hop
    rng = np.random.default_rng(3)
    stride = F + 3
    Ls = rng.integers(0, F + 1, n)
    Ls[:4] = (F, 0, 1, F - 1)
    src = np.full(1 + n * stride, np.nan, dtype=np.float32)
    x = np.zeros((n, F))
    for i in range(n):
        x[i, : Ls[i]] = rng.standard_normal(Ls[i]) * 0.5
        src[1 + i * stride: 1 + i * stride + Ls[i]] = x[i, : Ls[i]]
    order = rng.permutation(dst_rows)[:n]
    rows = [(1 + i * stride, int(Ls[i]), int(order[i])) for i in range(n)]
    spec = capi.LogMelSpec.make(sample_rate=16000, n_fft=n_fft, hop=hop, n_mels=n_mels, log=False)
    W = mel_weights64(16000, n_fft, n_mels, 0.0, 8000.0, "slaney", "slaney")
    whole, dst = guarded(dst_rows, n_mels * T)
    assert capi.pcm_logmel(ctx, torch.from_numpy(src).to("cuda:0"), rows, dst.view(dst_rows, n_mels, T), spec, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    got = rows_back(whole, dst_rows, n_mels, T, True)
    assert not np.isnan(got[order]).any()
    rest = np.setdiff1d(np.arange(dst_rows), order)
    assert rest.size == 100 and (got[rest].view(np.uint32) == SENTINEL).all()
    for i in range(0, n, 7):  # (every seventh row against the truth, the first four among them or not: all of them below)
        check_power(got[order[i]], *logmel_truth(x[i], int(Ls[i]), F, n_fft, hop, W))
    for i in range(4):
        check_power(got[order[i]], *logmel_truth(x[i], int(Ls[i]), F, n_fft, hop, W))
    # the rows beyond the grid's first round are among those checked
    assert n > 2048 and any(i >= 2048 for i in range(0, n, 7))


def test_indices_beyond_two_to_the_31(ctx):
    """a window of a source and the last rows of a destination whose element indices do not fit 32 bits"""
    import torch
    from vorbispizza_amd import capi
    F, n_fft, hop, n_mels = 1000, 32, 16, 8
    T = 1 + F // hop
    dst_rows = (1 << 31) // (n_mels * T) + 8
    src = torch.empty((1 << 31) + 8192, dtype=torch.float32, device="cuda:0")
    tail = (np.random.default_rng(4).standard_normal(8192) * 0.5).astype(np.float32)
    src[1 << 31:] = torch.from_numpy(tail).to("cuda:0")
    wins = [(7, 1000, 2), (2101, 333, 0)]  # (offsets inside the tail, rows from the end)
    W = mel_weights64(16000, n_fft, n_mels, 0.0, 8000.0, "slaney", "slaney")
    for bands_first in (True, False):
        dst = torch.empty((dst_rows, n_mels, T) if bands_first else (dst_rows, T, n_mels), dtype=torch.float32, device="cuda:0")
        dst[-3:] = 7.0
        assert (dst_rows - 3) * n_mels * T > 1 << 31
        rows = [((1 << 31) + at, L, dst_rows - 3 + r) for at, L, r in wins]
        spec = capi.LogMelSpec.make(sample_rate=16000, n_fft=n_fft, hop=hop, n_mels=n_mels, log=False, bands_first=bands_first)
        assert capi.pcm_logmel(ctx, src, rows, dst, spec, F) == capi.OK, ctx.last_error()
        ctx.synchronize()
        got = dst[-3:].cpu().numpy()
        got = got.transpose(0, 2, 1) if bands_first else got
        assert (got[1] == 7.0).all()
        for at, L, r in wins:
            check_power(got[r], *logmel_truth(tail[at: at + L], L, F, n_fft, hop, W))
        del dst


def raw_call(ctx, src_ptr, src_elems, frames, spec, rows, dst_ptr, dst_rows, n_rows=None, null_rows=False, handle=True, null_spec=False):
    from vorbispizza_amd import capi
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    return capi.lib().vpz_pcm_logmel(ctx._h if handle else None, src_ptr, src_elems, frames, None if null_spec else C.byref(spec),
                                     desc.shape[0] if n_rows is None else n_rows, None if null_rows else desc.ctypes.data, dst_ptr, dst_rows)


def test_every_refusal_is_invalid_arg_and_writes_nothing(ctx):
    import torch
    from vorbispizza_amd import capi
    F, dst_rows, n_mels = 500, 4, 80
    T = 1 + F // 160
    src = torch.from_numpy((np.random.default_rng(9).standard_normal(2000) * 0.5).astype(np.float32)).to("cuda:0")
    whole, dst = guarded(dst_rows, n_mels * T)
    spec = capi.LogMelSpec.make()
    good = dict(src_ptr=src.data_ptr(), src_elems=2000, frames=F, spec=spec, rows=[(3, 100, 1), (400, 500, 3)], dst_ptr=dst.data_ptr(), dst_rows=dst_rows)
    pinned = torch.zeros(dst_rows * n_mels * T, dtype=torch.float32, pin_memory=True)
    host_src = torch.full((2000,), 0.5, dtype=torch.float32, pin_memory=True)
    bad = [("no context", dict(handle=False)), ("null source", dict(src_ptr=None)), ("null destination", dict(dst_ptr=None)), ("null rows", dict(null_rows=True)),
           ("null spec", dict(null_spec=True)), ("frames < n_fft / 2 + 1", dict(frames=200, rows=[(3, 100, 1)])), ("n_rows < 0", dict(n_rows=-1)),
           ("dst_rows < 0", dict(dst_rows=-1)), ("src_elems < 0", dict(src_elems=-1)), ("samples > frames", dict(rows=[(3, 501, 1)])),
           ("samples < 0", dict(rows=[(3, -1, 1)])), ("src < 0", dict(rows=[(-1, 10, 1)])), ("span leaves the source", dict(rows=[(1501, 500, 1)])),
           ("src behind the source", dict(rows=[(2001, 0, 1)])), ("row out of range", dict(rows=[(3, 100, 4)])), ("row < 0", dict(rows=[(3, 100, -1)])),
           ("a row named twice", dict(rows=[(3, 100, 1), (400, 100, 1)])), ("more descriptors than rows", dict(rows=[(0, 1, 0)] * 5)),
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
    got = rows_back(whole, dst_rows, n_mels, T, True)
    assert (got[[0, 2]].view(np.uint32) == SENTINEL).all() and np.isfinite(got[[1, 3]]).all()


def test_a_window_alone_and_among_hundreds_gives_the_same_bits(ctx):
    """An output is one k-ordered chain per element: it does not depend on what else the launch carries or on how frames fall into tiles.
    The launch picks its tile by its size -- 64 frames when that gives every CU two workgroups, else 32 --, so the window alone and among
    40 others rides in 32-frame tiles and among 600 others in 64-frame ones (two row tiles per wave); the large launch is held to the
    float64 truth on its own as well."""
    import torch
    from vorbispizza_amd import capi
    F, n_mels, many = 160 * 70 + 37, 80, 601
    T = 1 + F // 160
    rng = np.random.default_rng(21)
    host = (rng.standard_normal(42 * F) * 0.5).astype(np.float32)
    src = torch.from_numpy(host).to("cuda:0")
    spec = capi.LogMelSpec.make()
    alone = torch.zeros((1, n_mels, T), dtype=torch.float32, device="cuda:0")
    assert capi.pcm_logmel(ctx, src, [(17 * F + 5, F - 300, 0)], alone, spec, F) == capi.OK, ctx.last_error()
    among = torch.zeros((41, n_mels, T), dtype=torch.float32, device="cuda:0")
    rows = [(i * F + 5, F - 300 if i == 17 else int(rng.integers(0, F)), (i * 7) % 41) for i in range(41)]
    assert capi.pcm_logmel(ctx, src, rows, among, spec, F) == capi.OK, ctx.last_error()
    # (the windows of the large launch overlap in the source: 67 samples apart)
    crowd = torch.zeros((many, n_mels, T), dtype=torch.float32, device="cuda:0")
    crowd_rows = [(17 * F + 5, F - 300, 0)] + [(i * 67 + 1, F - int(rng.integers(0, 500)), i) for i in range(1, many)]
    assert capi.pcm_logmel(ctx, src, crowd_rows, crowd, spec, F) == capi.OK, ctx.last_error()
    # ... and in a shorter padded row, with other tile boundaries: the frames that touch no padding agree bit for bit
    short = torch.zeros((1, n_mels, 1 + 4800 // 160), dtype=torch.float32, device="cuda:0")
    assert capi.pcm_logmel(ctx, src, [(17 * F + 5, 4800, 0)], short, spec, 4800) == capi.OK, ctx.last_error()
    ctx.synchronize()
    a, b, c = alone[0].cpu().numpy(), among[(17 * 7) % 41].cpu().numpy(), crowd[0].cpu().numpy()
    assert a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes() == c.view(np.uint32).tobytes()
    s = short[0].cpu().numpy()
    whole_frames = (4800 - 200) // 160  # frames 0 .. that end before sample 4800
    assert s[:, :whole_frames].view(np.uint32).tobytes() == a[:, :whole_frames].copy().view(np.uint32).tobytes()
    W = weights_of("whisper_400_160_80")
    for at, L, row in (crowd_rows[0], crowd_rows[300], crowd_rows[600]):
        assert check_log(crowd[row].cpu().numpy().T, *logmel_truth(host[at: at + L], L, F, 400, 160, W), FLOOR) < 1.0
