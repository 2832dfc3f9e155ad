"""vpz_pcm_cqt (include/vorbispizza_pcm_cqt.h, csrc/pcm_cqt.hip) alone: no decoder.

The truth is tests/cqt_truth.py's float64 restatement of the header's definition (the direct sum with exact coefficients), the tolerance
its derived bounds: Re and Im within d = (N_k + 2) 2^-24 sum |x| |h_k|; power within 2 |re| d + 2 |im| d + 2 d^2 + 3 u P; magnitude
within sqrt(2) d + 3 u |X|.  Every element of every named row is held to it, none exempt, for all three outputs and both layouts.  The
bound is loose; the sharp check is the float32 restatement (one fused chain per element), whose values the COMPLEX and POWER outputs
must equal bit for bit, the MAGNITUDE being the correctly rounded root of the restated power.  tests/test_cqt_cpu.py holds the
restatement to the bound on every case, so the tolerance is known to admit the reference arithmetic.  The cases are cqt_truth.CASES:
the smallest shapes at which the kernel can go wrong.  Rows no descriptor names and the guards on either side of the destination keep
their sentinel bit for bit; the source outside every window is NaN and never reaches the output; every refusal returns
VPZ_E_INVALID_ARG and writes nothing.

Largest error / bound observed on an MI355X over the parametrised cases: 0.233 (complex), 0.202 (power) and 0.156 (magnitude), all at
N_k = 8, 4, 2; 0.061 at hop 1, 0.022 at the default music spec, 1.4e-05 at N_0 = 65 536.  The same in both layouts: the values are."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cqt_truth as ct  # noqa: E402
from cqt_truth import cqt_refused_specs  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD = 64
DST_ROWS = ct.DST_ROWS


def guarded(n_floats):
    """a destination of n_floats float32 with GUARD sentinels on either side, every element the sentinel"""
    import torch
    flat = np.full(GUARD + n_floats + GUARD, SENTINEL, dtype=np.uint32)
    whole = torch.from_numpy(flat.view(np.float32).copy()).to("cuda:0")
    return whole, whole[GUARD: GUARD + n_floats]


def as_frames(body, dst_rows, spec, shape):
    """[row][T][n_bins] -- complex64 or float32 -- of a destination's float32 body"""
    from vorbispizza_amd import capi
    a = np.ascontiguousarray(body).reshape((dst_rows,) + shape)
    if spec.output == capi.CQT_COMPLEX:
        a = a.view(np.complex64)[..., 0]
    return np.ascontiguousarray(a.transpose(0, 2, 1)) if spec.layout == capi.CQT_BINS_FIRST else a


def cqt(ctx, d_src, rows, F, dst_rows, s, output="complex", bins_first=True):
    """one guarded launch -> [dst_rows][T][n_bins]"""
    from vorbispizza_amd import capi
    spec = capi.CqtSpec.make(output=output, bins_first=bins_first, **s)
    shape = spec.row_shape(F)
    whole, dst = guarded(dst_rows * int(np.prod(shape)))
    assert capi.pcm_cqt(ctx, d_src, rows, dst.view((dst_rows,) + shape), spec, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    bits = whole.cpu().numpy().view(np.uint32)
    assert (bits[:GUARD] == SENTINEL).all() and (bits[-GUARD:] == SENTINEL).all()
    return as_frames(bits[GUARD:-GUARD].view(np.float32), dst_rows, spec, shape)


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint32) == SENTINEL).all()


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


WORST = {}


@pytest.mark.parametrize("bins_first", [True, False], ids=["bins_first", "frames_first"])
@pytest.mark.parametrize("name", list(ct.CASES))
def test_rows_against_the_truth_and_the_restatement(ctx, name, bins_first):
    import torch
    c = ct.CASES[name]
    s, F = c["spec"], c["F"]
    T = 1 + F // s["hop"]
    src, rows = ct.case_input(name)
    truths, restated = ct.case_truth(name), ct.case_restated(name)
    d_src = torch.from_numpy(src).to("cuda:0")
    named = {row for _, _, row in rows}
    for output in ct.OUTPUTS:
        got = cqt(ctx, d_src, rows, F, DST_ROWS, s, output, bins_first)
        assert got.shape == (DST_ROWS, T, s["n_bins"])
        for r in range(DST_ROWS):
            if r not in named:
                assert untouched(got[r]), r
        worst = 0.0
        for (at, L, row), (Z, dr, di), want in zip(rows, truths, restated):
            assert not np.isnan(got[row]).any()  # (the source behind every L is NaN)
            worst = max(worst, ct.check_output(output, got[row], Z, dr, di))
            # COMPLEX and POWER are the restatement's values; MAGNITUDE the correctly rounded root of the restated power (numpy's float32
            # root is)
            assert same_bits(got[row], want[output]), (output, row, int((got[row] != want[output]).sum()))
            if L == 0:
                assert (got[row] == 0).all()
        print("error / bound %s %s %s: %.5f" % (name, output, "bins first" if bins_first else "frames first", worst))
        WORST[output] = max(WORST.get(output, 0.0), worst)
        assert worst < 1.0
    print("largest error / bound so far: %s" % WORST)


def test_a_spec_over_the_longest_kernel_is_refused(ctx):
    """N_0 = 65 536 runs (cqt_truth.CASES); one sample more is outside the limits"""
    import torch
    from vorbispizza_amd import capi
    s = dict(ct.CASES["limit_N0_65536"]["spec"])
    assert ct.bins(s)[1][0] == 65536
    s["f_min"] = ct._f_min_for(65537, s["sample_rate"], s["bins_per_octave"])
    assert ct.bins(s)[1][0] == 65537
    F = 2053
    spec = capi.CqtSpec.make(output="power", **s)
    src = torch.zeros(F, dtype=torch.float32, device="cuda:0")
    whole, dst = guarded(int(np.prod(spec.row_shape(F))))
    assert capi.pcm_cqt(ctx, src, [(0, F, 0)], dst.view((1,) + spec.row_shape(F)), spec, F) == capi.E_INVALID_ARG
    ctx.synchronize()
    assert untouched(whole.cpu().numpy())


def test_more_descriptors_than_the_grid_holds_side_by_side(ctx):
    """2100 rows of F = 270 at the base spec's first 33 bins and hop 270 -- two frames per row; the grid's y holds 2048: workgroups take a
    second descriptor -- in a destination of 2150 rows.  Rows not named keep the sentinel bit for bit; the source behind every row's L is
    NaN and must not reach the output."""
    import torch
    n, dst_rows, F = 2100, 2150, 270
    s = ct.spec_of(n_bins=33, hop=270)
    assert 1 + F // s["hop"] == 2 and n > ct.kernel_constants()["kCqMaxGridY"]
    rng = np.random.default_rng(3)
    stride = F + 3
    Ls = rng.integers(0, F + 1, n)
    Ls[:4] = (F, 0, 1, F - 1)
    src = np.full(1 + n * stride, np.nan, dtype=np.float32)
    for i in range(n):
        src[1 + i * stride: 1 + i * stride + Ls[i]] = (rng.standard_normal(Ls[i]) * 0.5).astype(np.float32)
    order = rng.permutation(dst_rows)[:n]
    rows = [(1 + i * stride, int(Ls[i]), int(order[i])) for i in range(n)]
    want = ct.chains32([(src[a: a + L], L) for a, L, _ in rows], F, s)
    d_src = torch.from_numpy(src).to("cuda:0")
    for output, bins_first in (("complex", True), ("power", False)):
        got = cqt(ctx, d_src, rows, F, dst_rows, s, output, bins_first)
        assert not np.isnan(got[order]).any()
        rest = np.setdiff1d(np.arange(dst_rows), order)
        assert rest.size == 50 and untouched(got[rest])
        for i in (0, 1, 2, 3, 7, 1000, 2047, 2048, 2099):
            assert same_bits(got[order[i]], ct.outputs32(*want[i])[output]), i
        whole = np.stack([ct.outputs32(*w)[output] for w in want])
        assert same_bits(got[order], whole)


def test_indices_beyond_two_to_the_31(ctx):
    """the last rows of a destination whose element indices do not fit 32 bits, in both layouts"""
    import torch
    from vorbispizza_amd import capi
    s = ct.spec_of(hop=4)
    F = 2000
    tail = (np.random.default_rng(4).standard_normal(8192) * 0.5).astype(np.float32)
    src = torch.from_numpy(tail).to("cuda:0")
    wins = [(7, 2000, 2), (2101, 333, 0)]  # (rows counted from the third last)
    want = [ct.outputs32(*w) for w in ct.chains32([(tail[a: a + L], L) for a, L, _ in wins], F, s)]
    for output, bins_first in (("power", True), ("complex", False)):
        spec = capi.CqtSpec.make(output=output, bins_first=bins_first, **s)
        shape = spec.row_shape(F)
        per_row = int(np.prod(shape))
        dst_rows = (1 << 31) // per_row + 8
        dst = torch.empty((dst_rows,) + shape, dtype=torch.float32, device="cuda:0")
        dst[-3:] = 7.0
        assert (dst_rows - 3) * per_row > 1 << 31
        rows = [(at, L, dst_rows - 3 + r) for at, L, r in wins]
        assert capi.pcm_cqt(ctx, src, rows, dst, spec, F) == capi.OK, ctx.last_error()
        ctx.synchronize()
        got = as_frames(dst[-3:].cpu().numpy(), 3, spec, shape)
        assert (np.ascontiguousarray(got[1]).view(np.float32) == 7.0).all()
        for (at, L, r), w in zip(wins, want):
            assert same_bits(got[r], w[output])
        del dst


def test_bits_by_placement(ctx):
    """A window's bits do not depend on where it is placed: the same samples at another source offset, at another destination row, among
    hundreds of other rows, and -- for the frames that touch no padding -- in a longer padded row carry the same bits, in both layouts"""
    import torch
    s = ct.spec_of()
    hop, half = s["hop"], ct.bins(s)[1][0] // 2
    many = 301
    F = hop * 70 + 37
    rng = np.random.default_rng(21)
    host = (rng.standard_normal(6 * F) * 0.5).astype(np.float32)
    L = F - 300
    host[4 * F + 2: 4 * F + 2 + L] = host[2 * F + 5: 2 * F + 5 + L]  # the same window once more, at an even offset
    src = torch.from_numpy(host).to("cuda:0")
    want = ct.outputs32(*ct.chains32([(host[2 * F + 5: 2 * F + 5 + L], L)], F, s)[0])
    T = 1 + F // hop
    inner = [t for t in range(T) if t * hop - half >= 0 and t * hop + half + 1 <= L]  # frames that read samples of the window only
    assert len(inner) > 32
    for output, bins_first in (("complex", True), ("complex", False), ("magnitude", True), ("power", False)):
        alone = cqt(ctx, src, [(2 * F + 5, L, 0)], F, 1, s, output, bins_first)[0]
        moved = cqt(ctx, src, [(4 * F + 2, L, 3)], F, 5, s, output, bins_first)[3]
        crowd_rows = [(2 * F + 5, L, many - 7)] + [(i * 67 + 1, F - int(rng.integers(0, 500)), (i * 5) % many) for i in range(many) if (i * 5) % many != many - 7]
        assert len(crowd_rows) == many
        crowd = cqt(ctx, src, crowd_rows, F, many, s, output, bins_first)[many - 7]
        longer = cqt(ctx, src, [(2 * F + 5, L, 1)], F + 5 * hop + 3, 2, s, output, bins_first)[1]  # (another T: other tiles, another row stride)
        assert same_bits(alone, moved) and same_bits(alone, crowd) and same_bits(alone, want[output])
        assert same_bits(alone[inner], longer[inner])


def raw_call(ctx, src_ptr, src_elems, frames, spec, rows, dst_ptr, dst_rows, n_rows=None, null_rows=False, handle=True, null_spec=False):
    from vorbispizza_amd import capi
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    return capi.lib().vpz_pcm_cqt(ctx._h if handle else None, src_ptr, src_elems, frames, None if null_spec else C.byref(spec),
                                  desc.shape[0] if n_rows is None else n_rows, None if null_rows else desc.ctypes.data, dst_ptr, dst_rows)


def test_every_refusal_is_invalid_arg_and_writes_nothing(ctx):
    import torch
    from vorbispizza_amd import capi
    F, dst_rows = 2500, 4
    s = ct.spec_of()
    spec = capi.CqtSpec.make(output="complex", **s)
    shape = spec.row_shape(F)
    per_row = int(np.prod(shape))
    src = torch.from_numpy((np.random.default_rng(9).standard_normal(8000) * 0.5).astype(np.float32)).to("cuda:0")
    whole, dst = guarded(dst_rows * per_row)
    good = dict(src_ptr=src.data_ptr(), src_elems=8000, frames=F, spec=spec, rows=[(3, 100, 1), (400, 2500, 3)], dst_ptr=dst.data_ptr(), dst_rows=dst_rows)
    pinned = torch.zeros(dst_rows * per_row, dtype=torch.float32, pin_memory=True)
    host_src = torch.full((8000,), 0.5, dtype=torch.float32, pin_memory=True)
    bad = [("no context", dict(handle=False)), ("null source", dict(src_ptr=None)), ("null destination", dict(dst_ptr=None)), ("null rows", dict(null_rows=True)),
           ("null spec", dict(null_spec=True)), ("reflect and frames < N_0 / 2 + 1", dict(frames=269, rows=[(3, 100, 1)])), ("frames < 1", dict(frames=0, rows=[(3, 0, 1)])),
           ("n_rows < 0", dict(n_rows=-1)),
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
    specs = cqt_refused_specs(capi, s)
    assert {"n_bins 513", "a reserved word", "N_0 over 65536", "hop 2049", "the last bin over Nyquist", "output 3"} <= {what for what, _ in specs}
    bad += [("spec: " + what, dict(spec=sp)) for what, sp in specs]
    for what, change in bad:
        assert raw_call(ctx, **dict(good, **change)) == capi.E_INVALID_ARG, what
    ctx.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL).all() and (pinned == 0).all()
    # (a float32 destination at an odd float is fine where no pairs are stored; the zero mode takes the short row)
    power = capi.CqtSpec.make(output="power", **s)
    assert raw_call(ctx, **dict(good, spec=power, dst_ptr=dst.data_ptr() + 4, rows=[(3, 100, 1)])) == capi.OK, ctx.last_error()
    zero = capi.CqtSpec.make(output="power", **dict(s, pad="zero"))
    assert raw_call(ctx, **dict(good, spec=zero, frames=269, rows=[(3, 100, 1)])) == capi.OK, ctx.last_error()
    ctx.synchronize()
    whole.copy_(torch.from_numpy(np.full(whole.numel(), SENTINEL, dtype=np.uint32).view(np.float32)))
    assert raw_call(ctx, **good) == capi.OK, ctx.last_error()  # (the good call is good)
    assert raw_call(ctx, **dict(good, rows=[], n_rows=0)) == capi.OK  # (no descriptor: nothing to do)
    ctx.synchronize()
    got = as_frames(whole.cpu().numpy()[GUARD:-GUARD], dst_rows, spec, shape)
    assert untouched(got[[0, 2]]) and np.isfinite(got[[1, 3]].real).all() and np.isfinite(got[[1, 3]].imag).all()
