"""vpz_feat_post (include/vorbispizza_pcm_featpost.h, csrc/pcm_featpost.hip) alone: no decoder.

The truth is tests/featpost_truth.py's longdouble restatement of the header's definition -- direct window sums, direct delta sums with
exact scales -- and the tolerance its derived bound, used as it stands, for the single stages; a composition is checked bit for bit
against the two single-stage calls it is defined as.  The real frames of a row lie inside the bound; every element behind them is pad_value
bit for bit; rows no descriptor names and the guards on either side of the destination keep their sentinel; source elements behind a row's
real frames are NaN and never reach the output; every refusal returns its status and writes nothing.

Largest error / bound ratio observed on an MI355X over the cases of this file (test_zz_the_largest_ratio_of_this_file prints them):
0.996 over the sliding windows of 4 frames, 0.99 for the row's and the sliding variance at every column count, 0.985 under a mean of 500
times the deviation, 0.96 at the variance floor; 0.35 for the deltas.  The normalised values sit at the bound because its leading term is
their own rounding to float32."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import featpost_truth as pt  # noqa: E402
from featpost_truth import refused_specs  # noqa: E402
from pcm_support import GUARD, SENTINEL, guarded  # noqa: E402
from featpost_cases import LAYOUTS, WORST, batch, by_column_slices, check_rows, feats, launch  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu


STAGES = {
    "deltas": dict(delta_order=2, delta_window=2),
    "row": dict(norm="row"),
    "row_vars": dict(norm="row", norm_vars=True),
    "sliding4": dict(norm="sliding", cmn_window=4, min_window=2),
    "sliding4_center_vars": dict(norm="sliding", cmn_window=4, min_window=2, center=True, norm_vars=True),
}


@pytest.mark.parametrize("frames_first", LAYOUTS)
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_every_kind_of_row_length(ctx, stage, frames_first):
    """n = 0, 1, 2, 3, 63, 64, 65, 129 (none, fewer frames than taps, one chunk less one, one chunk, one more, two and one) in one launch
    at T = 134, permuted into a destination of 11 rows, and each alone at T = n and T = n + 5: pad frames exact, nothing written beyond,
    the same bits in all three launches"""
    d = pt.spec_of(frames_first=frames_first, pad_value=-7.25, **STAGES[stage])
    ns = [0, 1, 2, 3, 63, 64, 65, 129]
    xs = [feats(n, 3, 10 + n) for n in ns]
    order = [9, 4, 0, 7, 2, 10, 5, 3]
    got = launch(ctx, d, batch(xs, 134), [(i, n, r) for i, (n, r) in enumerate(zip(ns, order))], 11)
    assert (got[[1, 6, 8]].view(np.uint32) == SENTINEL).all()
    check_rows(stage, got, xs, d, order)
    for x, r in zip(xs, order):
        n = len(x)
        for T in (n, n + 5):
            if T == 0:
                continue
            alone = launch(ctx, d, batch([x], T), [(0, n, 1)], 3)
            assert (alone[[0, 2]].view(np.uint32) == SENTINEL).all()
            assert (alone[1, :n].view(np.uint32) == got[r, :n].view(np.uint32)).all(), (n, T)
            assert (alone[1, n:] == np.float32(-7.25)).all()


@pytest.mark.parametrize("frames_first", LAYOUTS)
@pytest.mark.parametrize("D", [1, 3, 63, 64, 65, 256])
def test_the_number_of_columns(ctx, D, frames_first):
    """one column, fewer than a wave, a wave less one, a wave, one more, the limit (the sliding kernel takes 32 columns a workgroup: one
    tile, two less one, two, two and one, eight): deltas of order 3 (D_out up to 1024), a variance normalisation of the row and one over
    a sliding window, n = 70 of T = 75 and n = T; and the sliding window behind the deltas against its two single-stage calls (the
    second one per slice of 256 columns: at D = 256 the deltas' tensor has 512)"""
    xs = [feats(70, D, 500 + D), feats(75, D, 600 + D)]
    rows = [(0, 70, 1), (1, 75, 0)]
    sliding = dict(norm="sliding", cmn_window=40, min_window=7, norm_vars=True)
    for name, stage in (("deltas", dict(delta_order=3, delta_window=2)), ("row_vars", dict(norm="row", norm_vars=True)), ("sliding_vars", sliding)):
        d = pt.spec_of(frames_first=frames_first, **stage)
        got = launch(ctx, d, batch(xs, 75), rows, 2)
        check_rows("D %s" % name, got, xs, d, [1, 0])
    d = pt.spec_of(frames_first=frames_first, delta_order=1, deltas_first=True, **sliding)
    between = launch(ctx, dict(d, norm="none"), batch(xs, 75), [(0, 70, 0), (1, 75, 1)], 2)
    two = by_column_slices(ctx, dict(d, delta_order=0), between, rows, 2)
    assert two.shape == (2, 75, 2 * D)
    assert (launch(ctx, d, batch(xs, 75), rows, 2).view(np.uint32) == two.view(np.uint32)).all()


@pytest.mark.parametrize("frames_first", LAYOUTS)
@pytest.mark.parametrize("window", [1, 2, 8])
def test_delta_orders_and_windows(ctx, window, frames_first):
    """orders 1 to 3 at windows 1, 2 and 8 over rows of 1, 2, 5 and 30 frames -- fewer than order * window, where every tap clamps -- and
    of 70; block 0 is the input bit for bit; a one-frame row's deltas are the scales' sum times the frame"""
    ns = [1, 2, 5, 30, 70]
    xs = [feats(n, 4, 70 + n) for n in ns]
    for order in (1, 2, 3):
        d = pt.spec_of(delta_order=order, delta_window=window, frames_first=frames_first)
        got = launch(ctx, d, batch(xs, 70), [(i, n, i) for i, n in enumerate(ns)], 5)
        check_rows("deltas %d" % order, got, xs, d, range(5))
        for i, x in enumerate(xs):
            assert (got[i, :len(x), :4].view(np.uint32) == x.view(np.uint32)).all()


SLIDING = [dict(cmn_window=4, min_window=2), dict(cmn_window=100, min_window=30), dict(cmn_window=100, min_window=100), dict(cmn_window=64, min_window=1)]


@pytest.mark.parametrize("frames_first", LAYOUTS)
@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("center", [False, True])
def test_sliding_windows_across_chunks(ctx, center, norm_vars, frames_first):
    """W = 4 with min_window 2, W = 100 (min_window 30 and 100) and W = 64 over n = 257, 64, 99 and 5: windows inside one chunk, across
    one, two and three boundaries, starting and ending on one, and the edge rules at both ends of the row"""
    ns = [257, 64, 99, 5]
    xs = [feats(n, 3, 900 + n, offset=2.0) for n in ns]
    for w in SLIDING:
        d = pt.spec_of(norm="sliding", center=center, norm_vars=norm_vars, frames_first=frames_first, **w)
        got = launch(ctx, d, batch(xs, 260), [(i, n, 3 - i) for i, n in enumerate(ns)], 4)
        check_rows("sliding W %d" % w["cmn_window"], got, xs, d, [3, 2, 1, 0])


@pytest.mark.parametrize("norm_vars", [False, True])
def test_a_mean_of_500_times_the_deviation(ctx, norm_vars):
    """VPZ_NORM_ROW and a sliding window on rows whose mean is 500 times their deviation: inside the bound, and the bound is below 2^-20 of
    the output's scale -- the float64 sums keep the digits a float32 mean would lose"""
    xs = [feats(n, 5, 33 + n, offset=500.0) for n in (129, 300)]
    for stage in (dict(norm="row"), dict(norm="sliding", cmn_window=100, min_window=30, center=True)):
        d = pt.spec_of(norm_vars=norm_vars, **stage)
        got = launch(ctx, d, batch(xs, 300), [(0, 129, 0), (1, 300, 1)], 2)
        check_rows("dc 500", got, xs, d, [0, 1])
        for x in xs:
            want, bound = pt.truth(x, d)
            assert float(bound.max()) < 2.0 ** -20 * (1.0 if norm_vars else float(np.std(x)))
            assert float(np.abs(want).max()) > 1.0


def test_the_variance_floor_and_the_one_frame_window(ctx):
    """under norm_vars: a constant column ends at the floor (its output is 0 within the bound, |out| < 1e-6, and finite); a one-frame row
    and every frame of a sliding window with c = 1 is +0 bit for bit; a floor above the variance is the divisor"""
    x = feats(100, 3, 5)
    x[:, 1] = np.float32(3.7)
    one = feats(1, 3, 6)
    for stage in (dict(norm="row"), dict(norm="sliding", cmn_window=40, min_window=1, center=True)):
        d = pt.spec_of(norm_vars=True, **stage)
        got = launch(ctx, d, batch([x, one], 100), [(0, 100, 0), (1, 1, 1)], 2)
        check_rows("var floor", got, [x, one], d, [0, 1])
        assert np.isfinite(got[0]).all() and np.abs(got[0, :, 1]).max() < 1e-6
        assert (got[1, 0].view(np.uint32) == 0).all()
    d = pt.spec_of(norm="sliding", norm_vars=True, cmn_window=1, min_window=1, center=True)
    got = launch(ctx, d, batch([x], 100), [(0, 100, 0)], 1)
    assert (got.view(np.uint32) == 0).all()
    d = pt.spec_of(norm="row", norm_vars=True, var_floor=1e4)
    got = launch(ctx, d, batch([x], 100), [(0, 100, 0)], 1)
    check_rows("var floor", got, [x], d, [0])
    assert np.abs(got[0, :, 0].astype(np.float64) - (x[:, 0] - x[:, 0].astype(np.float64).mean()) / 100.0).max() < 1e-6


COMPOSED = [dict(norm="row", norm_vars=True, delta_order=2), dict(norm="sliding", cmn_window=100, min_window=30, center=True, delta_order=2),
            dict(norm="sliding", cmn_window=4, min_window=2, norm_vars=True, delta_order=3, delta_window=1),
            dict(norm="row", delta_order=1, delta_window=8)]


@pytest.mark.parametrize("frames_first", LAYOUTS)
@pytest.mark.parametrize("deltas_first", [False, True])
def test_a_composition_is_its_two_single_stage_calls(ctx, deltas_first, frames_first):
    """both stages in one call against two calls in `order`, the tensor between them float32: the same bits, pad frames included"""
    ns = [129, 0, 1, 3, 64, 200]
    xs = [feats(n, 5, 40 + n, offset=1.5) for n in ns]
    rows = [(i, n, i) for i, n in enumerate(ns)]
    for c in COMPOSED:
        d = pt.spec_of(deltas_first=deltas_first, frames_first=frames_first, pad_value=3.5, **c)
        got = launch(ctx, d, batch(xs, 203), rows, 6)
        only_norm = dict(d, delta_order=0)
        only_deltas = dict(d, norm="none")
        first, second = (only_deltas, only_norm) if deltas_first else (only_norm, only_deltas)
        between = launch(ctx, first, batch(xs, 203), rows, 6)
        assert between.dtype == np.float32
        for i, n in enumerate(ns):
            between[i, n:] = np.nan  # (the second call must not read them)
        two = launch(ctx, second, np.ascontiguousarray(between), rows, 6)
        assert got.shape == two.shape == (6, 203, 5 * (d["delta_order"] + 1))
        assert (got.view(np.uint32) == two.view(np.uint32)).all(), c


def test_the_same_bits_wherever_a_row_sits(ctx):
    """ONE ROW of 150 frames in launches of 1, 3 and 4100 descriptors (the grid's y holds 4096: the last rows are a workgroup's second
    round), at T = 150, 151 and 400, as the first, a middle and the last source and destination row, beside other neighbours, in both
    layouts and with a scratch tensor of the caller's: the same bits, for deltas, the sliding variance normalisation and their
    composition; the neighbours are checked against a launch of their own"""
    import torch
    from vorbispizza_amd import capi
    x = feats(150, 4, 77, offset=3.0)
    for stage in (dict(delta_order=2), dict(norm="sliding", cmn_window=70, min_window=20, norm_vars=True),
                  dict(norm="sliding", cmn_window=70, min_window=20, norm_vars=True, delta_order=2, deltas_first=True),
                  dict(norm="row", delta_order=1)):
        d = pt.spec_of(**stage)
        ref = launch(ctx, d, batch([x], 150), [(0, 150, 0)], 1)[0]
        a, b = feats(151, 4, 78), feats(9, 4, 79)
        got = launch(ctx, d, batch([a, x, b], 151), [(2, 9, 0), (1, 150, 2), (0, 151, 1)], 3)
        assert (got[2, :150].view(np.uint32) == ref.view(np.uint32)).all()
        assert (got[1].view(np.uint32) == launch(ctx, d, batch([a], 151), [(0, 151, 0)], 1)[0].view(np.uint32)).all()
        cf = launch(ctx, dict(d, frames_first=False), batch([b, x], 400), [(1, 150, 0), (0, 9, 1)], 2)
        assert (cf[0, :150].view(np.uint32) == ref.view(np.uint32)).all() and (cf[0, 150:] == 0).all()
        small = [feats(2, 4, 80), feats(3, 4, 81)]
        many = [small[i % 2] for i in range(4099)] + [x]
        rows = [(i, len(m), 4099 - i) for i, m in enumerate(many)]
        big = launch(ctx, d, batch(many, 150), rows, 4100)
        assert (big[0].view(np.uint32) == ref.view(np.uint32)).all()
        pair = launch(ctx, d, batch(small, 150), [(0, 2, 0), (1, 3, 1)], 2)
        for i in (0, 1, 2, 3, 4094, 4095, 4096, 4097, 4098):
            assert (big[4099 - i].view(np.uint32) == pair[i % 2].view(np.uint32)).all(), i
        # the caller's scratch memory, larger than needed, filled with NaN: nothing of it reaches a value
        spec = capi.FeatPostSpec.make(**d)
        need = capi.feat_post_scratch(spec, 1, 150, 4)
        scratch = torch.full((need + 9,), float("nan"), dtype=torch.float64, device="cuda:0")
        dst = torch.zeros((1, 150, spec.out_columns(4)), dtype=torch.float32, device="cuda:0")
        assert capi.feat_post(ctx, torch.from_numpy(batch([x], 150)).to("cuda:0"), [(0, 150, 0)], dst, spec, scratch=scratch) == capi.OK
        ctx.synchronize()
        assert (dst.cpu().numpy()[0].view(np.uint32) == ref.view(np.uint32)).all()
        assert need == 0 or torch.isnan(scratch[need:]).all()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_value_that_is_not_finite_stays_where_it_is_covered(ctx, bad):
    """one NaN / inf at frame 70 of one row of 200: exactly the outputs whose window or non-zero taps cover it are not finite, every other
    output of the row and every other row keep the bits they have without it"""
    x, y = feats(200, 3, 1), feats(130, 3, 2)
    dirty = x.copy()
    dirty[70, 1] = bad
    rows = [(0, 200, 1), (1, 130, 0)]
    for stage in (dict(delta_order=2, delta_window=2), dict(norm="sliding", cmn_window=50, min_window=10, center=True, norm_vars=True),
                  dict(norm="sliding", cmn_window=50, min_window=10), dict(norm="row")):
        d = pt.spec_of(**stage)
        clean = launch(ctx, d, batch([x, y], 200), rows, 2)
        got = launch(ctx, d, batch([dirty, y], 200), rows, 2)
        assert (got[0].view(np.uint32) == clean[0].view(np.uint32)).all()
        hit = np.zeros(got[1].shape, dtype=bool)
        if d["norm"] == "none":
            hit[70, 1] = True
            for i in range(1, d["delta_order"] + 1):
                s, H = pt.scales(i, d["delta_window"]), i * d["delta_window"]
                for t in range(200):
                    hit[t, i * 3 + 1] = any(s[j + H] != 0 and min(max(t + j, 0), 199) == 70 for j in range(-H, H + 1))
        else:
            for t in range(200):
                a, b = pt.window(d, t, 200)
                hit[t, 1] = a <= 70 < b
        assert hit.sum() >= 5
        assert (np.isfinite(got[1]) == ~hit).all()
        assert (got[1][~hit].view(np.uint32) == clean[1][~hit].view(np.uint32)).all()


def test_every_refusal_launches_nothing(ctx):
    """every limit of the spec, D and T outside theirs, descriptors out of range or naming a row twice, a scratch tensor that is missing,
    too small (VPZ_E_CAPACITY), misaligned, host memory or overlapping, source and destination overlapping, null pointers, sizes that
    overflow: the status, and a destination that keeps its sentinel"""
    import torch
    from vorbispizza_amd import capi
    L = capi.lib()
    T, D = 40, 6
    src = torch.from_numpy(batch([feats(40, D, 1), feats(30, D, 2)], T)).to("cuda:0")
    whole, dst = guarded(3, T * D * 3)
    good = capi.FeatPostSpec.make(norm="sliding", cmn_window=10, min_window=5, delta_order=2, deltas_first=True)
    need = capi.feat_post_scratch(good, 2, T, D)
    scratch = torch.zeros(need + 2, dtype=torch.float64, device="cuda:0")
    rows = np.array([(0, 40, 2), (1, 30, 0)], dtype=np.int64)

    def call(spec=good, src_p=src.data_ptr(), src_rows=2, T_=T, D_=D, n_rows=2, rows_=rows, dst_p=dst.data_ptr(), dst_rows=3,
             scr_p=scratch.data_ptr(), scr_elems=need):
        rows_ = None if rows_ is None else np.ascontiguousarray(rows_, dtype=np.int64)
        return L.vpz_feat_post(ctx._h, src_p, src_rows, T_, D_, C.byref(spec) if spec is not None else None, n_rows,
                               None if rows_ is None else rows_.ctypes.data, dst_p, dst_rows, scr_p, scr_elems)

    torch.cuda.synchronize()
    refused = 0
    for what, spec in refused_specs(capi):
        assert call(spec=spec) == capi.E_INVALID_ARG, what
        refused += 1
    host = np.zeros(need, dtype=np.float64)
    cases = [
        ("spec null", dict(spec=None)), ("rows null", dict(rows_=None)), ("src null", dict(src_p=None)), ("dst null", dict(dst_p=None)),
        ("scratch null", dict(scr_p=None)), ("D 0", dict(D_=0)), ("D 257", dict(D_=257)), ("T 0", dict(T_=0)),
        ("src_rows < 0", dict(src_rows=-1)), ("dst_rows < 0", dict(dst_rows=-1)), ("n_rows < 0", dict(n_rows=-1)), ("scratch_elems < 0", dict(scr_elems=-1)),
        ("src_row out of range", dict(rows_=[(2, 40, 2), (1, 30, 0)])), ("src_row negative", dict(rows_=[(-1, 40, 2), (1, 30, 0)])),
        ("real_frames > T", dict(rows_=[(0, 41, 2), (1, 30, 0)])), ("real_frames < 0", dict(rows_=[(0, -1, 2), (1, 30, 0)])),
        ("row out of range", dict(rows_=[(0, 40, 3), (1, 30, 0)])), ("row negative", dict(rows_=[(0, 40, -1), (1, 30, 0)])),
        ("a row named twice", dict(rows_=[(0, 40, 2), (1, 30, 2)])), ("more descriptors than rows", dict(n_rows=2, dst_rows=1)),
        ("sizes overflow", dict(T_=2 ** 61, src_rows=2 ** 40)), ("dst misaligned", dict(dst_p=dst.data_ptr() + 2)),
        ("src misaligned", dict(src_p=src.data_ptr() + 2)), ("scratch misaligned", dict(scr_p=scratch.data_ptr() + 8)),
        ("scratch in host memory", dict(scr_p=host.ctypes.data)), ("src in host memory", dict(src_p=host.ctypes.data, src_rows=0, n_rows=0)),
        ("source and destination overlap", dict(src_p=dst.data_ptr(), src_rows=1, rows_=[(0, 40, 2)], n_rows=1)),
        ("scratch overlaps the destination", dict(scr_p=dst.data_ptr(), scr_elems=need)),
        ("scratch overlaps the source", dict(scr_p=src.data_ptr() - src.data_ptr() % 16, scr_elems=need)),
    ]
    for what, kw in cases:
        assert call(**kw) == capi.E_INVALID_ARG, what
        assert "vpz_feat_post" in ctx.last_error(), what
        refused += 1
    assert call(scr_elems=need - 1) == capi.E_CAPACITY and call(scr_elems=0) == capi.E_CAPACITY
    ctx.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL).all() and (scratch.cpu().numpy() == 0).all()
    assert refused == 27 + len(cases)
    # the Python wrapper validates the destination's shape before the library is called
    with pytest.raises(ValueError):
        capi.feat_post(ctx, src, rows, dst.view(3, T, D * 3)[:, :, :D], good)
    with pytest.raises(ValueError):
        capi.feat_post(ctx, src, rows, dst.view(3, D * 3, T), good)
    # and what is not refused: no descriptors (nothing launched), a normalisation-free spec without scratch memory
    assert call(n_rows=0) == capi.OK
    ctx.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL).all()
    # descriptors without real frames need no scratch memory, and may name a source row the source does not have: pad rows
    assert call(rows_=[(0, 0, 2), (5, 0, 0)], scr_p=None, scr_elems=0) == capi.OK
    ctx.synchronize()
    body = whole.cpu().numpy().view(np.uint32)[GUARD:-GUARD].reshape(3, T, D * 3)
    assert (body[1] == SENTINEL).all() and (body[[0, 2]] == 0).all()
    deltas = capi.FeatPostSpec.make(delta_order=2)
    assert call(spec=deltas, scr_p=None, scr_elems=0) == capi.OK
    ctx.synchronize()
    body = whole.cpu().numpy().view(np.uint32)[GUARD:-GUARD].reshape(3, T, D * 3)
    assert (body[1] == SENTINEL).all() and (body[[0, 2]] != SENTINEL).all()


def test_zz_the_largest_ratio_of_this_file():
    assert WORST, "runs behind the tests above"
    for k in sorted(WORST):
        print("largest error / bound, %s: %.3f" % (k, WORST[k]))
    print("largest error / bound over this file: %.3f" % max(WORST.values()))
    assert max(WORST.values()) <= 1.0
