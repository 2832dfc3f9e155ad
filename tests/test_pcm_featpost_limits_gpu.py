"""vpz_feat_post (include/vorbispizza_pcm_featpost.h, csrc/pcm_featpost.hip) at the limits of what its kernels stage, PINNED BY BITS:
every value of a real frame is compared with tests/featpost_bits.py, the host model of the header's stated arithmetic -- the fused float32
chain, the float64 chunk sums, L + whole chunks + R in that order, one fused step for the variance --, not with another launch.
tests/test_featpost_bits_cpu.py shows that the model tells those orders from others.  Beside the bits, as in
tests/test_pcm_featpost_gpu.py: pad frames are pad_value bit for bit, rows no descriptor names and the guards keep their sentinel, the
source is NaN behind every row's real frames, and a single stage on ordinary input lies inside tests/featpost_truth.py's bound as it stands.

What the first suite left alone, and is run here:
  the longest chain      order 3, window 8: a halo of 24 frames, which the LDS plan is sized for (64 + 48 and 128 + 48 staged frames, 65 472
                         bytes of dynamic LDS), clipped at a row's start, its end, both, and whole on both sides of a middle tile, in the
                         chunk, the apply and the sliding kernel, the third launch of VPZ_POST_NORM_FIRST among them
  width                  D = 33, 129, 256 at order 3 through both two-stage routes: up to 1024 normalised columns (grid z = 4, 8 column
                         tiles), and a third launch that reads block 0 out of a destination of 1024 columns
  Kaldi's own window     cmn_window 600 / min_window 100: up to nine whole chunks a window, 21 chunk sums a row
  the order of the sums  featpost_bits.spiked's rows, on which another order changes the bits
  subnormals             inputs scaled by 2^-140: nothing is flushed

Largest error / bound ratio observed on an MI355X over the single-stage cases of this file (test_zz_the_largest_ratio_of_this_file
prints them): 0.995 at cmn_window 600, 0.989 centred and for the row of 1300 frames; 0.155 for the deltas of order 3 at window 8; on the
subnormal rows 0.240 for the deltas and 0.469 for the row's mean.  Every other case is a composition or a spiked row, where the bits alone
are checked.  The device gave the model's bits in every case of this file; the file takes 9 s with tests/test_pcm_featpost_gpu.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import featpost_bits as fb  # noqa: E402
import featpost_truth as pt  # noqa: E402
from featpost_bits import ROW_SPIKED, SPIKED  # noqa: E402
from pcm_support import SENTINEL  # noqa: E402
from featpost_cases import LAYOUTS, WORST, batch, by_column_slices, check_rows, feats, launch  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

MODEL = {}  # computed once per (input, spec), shared by the layouts
NOTED = set()  # this file's keys of test_pcm_featpost_gpu's table of ratios, which check_rows fills


def spec_key(d):
    return tuple(sorted((k, v) for k, v in d.items() if k not in ("frames_first", "pad_value")))


def model_of(tag, x, d):
    key = (tag, x.shape, spec_key(d))
    if key not in MODEL:
        MODEL[key] = fb.model(x, d)
        MODEL[key].setflags(write=False)
    return MODEL[key]


def check(key, tag, got, xs, d, order, dst_rows, bound=True):
    """every named row: the model's bits on its real frames, pad_value's behind them; every other row: the sentinel; a single stage
    (where `bound`): inside the truth's bound"""
    pad_bits = np.float32(d["pad_value"]).view(np.uint32)
    single = (d["norm"] == "none") != (d["delta_order"] == 0)
    order = list(order)
    for r in sorted(set(range(dst_rows)) - set(order)):
        assert (got[r].view(np.uint32) == SENTINEL).all(), (key, r)
    for i, (x, r) in enumerate(zip(xs, order)):
        n = len(x)
        assert (got[r, n:].view(np.uint32) == pad_bits).all(), (key, n)
        if n == 0:
            continue
        want = model_of((tag, i), x, d)
        differ = got[r, :n].view(np.uint32) != want.view(np.uint32)
        if differ.any():
            t, c = np.argwhere(differ)[0]
            raise AssertionError("%s, n = %d: %d of %d elements differ from the model, the first at frame %d, column %d: %r against %r"
                                 % (key, n, differ.sum(), differ.size, t, c, got[r, t, c], want[t, c]))
    if single and bound:
        NOTED.add(key)
        check_rows(key, got, xs, d, order)


# ---- the longest chain in every kernel
CHAIN_NS = [1, 24, 25, 48, 49, 64, 65, 88, 89, 128, 153, 200]
CHAIN_ORDER = [13, 4, 0, 7, 2, 10, 5, 3, 11, 8, 1, 12]
CHAIN_NORMS = {
    "row": dict(norm="row"),
    "sliding4": dict(norm="sliding", cmn_window=4, min_window=2),
    "sliding70_center": dict(norm="sliding", cmn_window=70, min_window=20, center=True),
    "sliding150": dict(norm="sliding", cmn_window=150, min_window=50),
}


def chain_rows(scale=1.0):
    return [feats(n, 3, 2000 + n, scale=scale) for n in CHAIN_NS]


def run_chain(ctx, key, d, xs, tag, bound=True):
    got = launch(ctx, d, batch(xs, 210), [(i, n, r) for i, (n, r) in enumerate(zip(CHAIN_NS, CHAIN_ORDER))], 14)
    check(key, tag, got, xs, d, CHAIN_ORDER, 14, bound)
    return got


@pytest.mark.parametrize("frames_first", LAYOUTS)
def test_the_longest_chain_alone(ctx, frames_first):
    """deltas of order 3 at window 8, H = 24: rows shorter than the halo (every tap clamps), n = 24, 25, 48, 49 (the halo reaches the
    row's end from inside the first tile), 64, 65, 88, 89 (a second tile of 1, 24 and 25 frames, all halo of the first), 128, 153 (a
    middle tile with 24 frames on either side) and 200; block 0 is the input"""
    xs = chain_rows()
    d = pt.spec_of(delta_order=3, delta_window=8, frames_first=frames_first, pad_value=-7.25)
    got = run_chain(ctx, "chain deltas", d, xs, "chain")
    for x, r in zip(xs, CHAIN_ORDER):
        assert (got[r, :len(x), :3].view(np.uint32) == x.view(np.uint32)).all()


@pytest.mark.parametrize("frames_first", LAYOUTS)
@pytest.mark.parametrize("deltas_first", [False, True])
@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("norm", sorted(CHAIN_NORMS))
def test_the_longest_chain_meets_a_normalisation(ctx, norm, norm_vars, deltas_first, frames_first):
    """the same rows and chain with the row's and three sliding normalisations, mean and variance, in both orders: behind the deltas the
    chunk and the sliding kernel stage the delta view with its halo of 24; in front of them the third launch reads it out of the
    destination"""
    d = pt.spec_of(delta_order=3, delta_window=8, deltas_first=deltas_first, norm_vars=norm_vars, frames_first=frames_first, pad_value=-7.25,
                   **CHAIN_NORMS[norm])
    run_chain(ctx, "chain %s" % norm, d, chain_rows(), "chain")


@pytest.mark.parametrize("frames_first", LAYOUTS)
def test_subnormal_inputs_are_not_flushed(ctx, frames_first):
    """the chain's rows scaled by 2^-140 (every value below float32's normal range): the deltas and the row's mean normalisation are
    the model's bits -- numpy flushes nothing --, inside the bound, whose K * tiny term assumes as much; and most of the first deltas
    and of the normalised values are not zero (the scales of order 2 and 3 take most of theirs below 2^-149)"""
    xs = chain_rows(scale=2.0 ** -140)
    assert all((np.abs(x) < 2.0 ** -126).all() and (x != 0).mean() > 0.9 for x in xs)
    for key, stage, cols in (("subnormal deltas", dict(delta_order=3, delta_window=8), slice(3, 6)), ("subnormal row", dict(norm="row"), slice(0, 3))):
        d = pt.spec_of(frames_first=frames_first, **stage)
        got = run_chain(ctx, key, d, xs, "chain subnormal")
        assert (got[CHAIN_ORDER[-1], :200, cols] != 0).mean() > 0.5


# ---- width through the two-stage routes
WIDE_NORMS = {"row": dict(norm="row"), "sliding40_vars": dict(norm="sliding", cmn_window=40, min_window=7, norm_vars=True)}


@pytest.mark.parametrize("frames_first", LAYOUTS)
@pytest.mark.parametrize("deltas_first", [False, True])
@pytest.mark.parametrize("norm", sorted(WIDE_NORMS))
@pytest.mark.parametrize("D", [33, 129, 256])
def test_wide_tensors_through_the_two_stage_routes(ctx, D, norm, deltas_first, frames_first):
    """D = 33, 129, 256 (a column tile and one column, four and one, eight) at order 3, n = 70 of T = 75 and n = T.  Deltas first: 132,
    516 and 1024 normalised columns, the delta block in the grid's z; and the device against itself -- the deltas call, then the
    normalisation per slice of 256 columns, is the same bits.  Normalisation first: the third launch reads block 0 out of a destination
    of up to 1024 columns, across its 32-column tiles"""
    xs = [feats(70, D, 500 + D), feats(75, D, 600 + D)]
    rows = [(0, 70, 1), (1, 75, 0)]
    d = pt.spec_of(delta_order=3, deltas_first=deltas_first, frames_first=frames_first, pad_value=2.5, **WIDE_NORMS[norm])
    got = launch(ctx, d, batch(xs, 75), rows, 2)
    assert got.shape == (2, 75, 4 * D)
    check("wide %s" % norm, "wide %d" % D, got, xs, d, [1, 0], 2)
    if deltas_first:
        between = launch(ctx, dict(d, norm="none"), batch(xs, 75), [(0, 70, 0), (1, 75, 1)], 2)
        between[0, 70:] = np.nan  # (the second call must not read them)
        two = by_column_slices(ctx, dict(d, delta_order=0), between, rows, 2)
        assert (got.view(np.uint32) == two.view(np.uint32)).all()


# ---- Kaldi's windows
KALDI_NS = [99, 100, 101, 600, 601, 602, 1300]  # (tests/test_featpost_cpu.py's NS without its rows of 1 and 2 frames)
KALDI_ORDER = [8, 3, 0, 6, 2, 7, 4]
KALDI = {
    "W600": dict(norm="sliding", cmn_window=600, min_window=100),
    "W600_center": dict(norm="sliding", cmn_window=600, min_window=100, center=True),
    "row": dict(norm="row"),
}


@pytest.mark.parametrize("frames_first", LAYOUTS)
@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("norm", sorted(KALDI))
def test_kaldis_default_window(ctx, norm, norm_vars, frames_first):
    """cmn_window 600 with min_window 100 -- the spec's defaults --, centred too, and the row, over n = 99, 100, 101 (around
    min_window), 600, 601, 602 (around the window) and 1300 = T, in one launch permuted into nine rows: a window holds up to nine whole
    chunks between its partial ones, a row's sum 21 chunk sums"""
    from featpost_truth import NS
    assert set(KALDI_NS) <= set(NS) and pt.DEFAULTS["cmn_window"] == 600 and pt.DEFAULTS["min_window"] == 100
    xs = [feats(n, 3, 3000 + n, offset=2.0) for n in KALDI_NS]
    d = pt.spec_of(norm_vars=norm_vars, frames_first=frames_first, pad_value=-1.0, **KALDI[norm])
    got = launch(ctx, d, batch(xs, 1300), [(i, n, r) for i, (n, r) in enumerate(zip(KALDI_NS, KALDI_ORDER))], 9)
    check("kaldi %s" % norm, "kaldi", got, xs, d, KALDI_ORDER, 9)


# ---- the order of the sums, made visible
@pytest.mark.parametrize("frames_first", LAYOUTS)
@pytest.mark.parametrize("case", range(len(SPIKED) + len(ROW_SPIKED)), ids=[c[0].replace(" ", "_") for c in SPIKED + ROW_SPIKED])
def test_the_stated_order_of_the_sums(ctx, case, frames_first):
    """the spiked rows of tests/test_featpost_bits_cpu.py, mean only, through the row path and the sliding path at W = 4, 100, 200 and
    300 centred and 600: the header's order and no other gives these bits (the longdouble bound says nothing here: the sums pass 2^43)"""
    name, n, D, seed, far, stage = (SPIKED + ROW_SPIKED)[case]
    x = fb.spiked(n, D, seed, far)
    d = pt.spec_of(frames_first=frames_first, pad_value=1.0, **stage)
    got = launch(ctx, d, batch([x], n + 3), [(0, n, 1)], 3)
    check("spiked", "spiked %s" % name, got, [x], d, [1], 3, bound=False)
    assert np.isfinite(got[1, :n]).all()


@pytest.mark.parametrize("frames_first", LAYOUTS)
def test_a_composition_over_a_spiked_row(ctx, frames_first):
    """add-deltas | apply-cmvn-sliding over a spiked row: the first-order deltas of the pairs, then the centred window of 200 over all
    2 D columns"""
    x = fb.spiked(330, 4, 7)
    d = pt.spec_of(norm="sliding", cmn_window=200, min_window=1, center=True, delta_order=1, deltas_first=True, frames_first=frames_first)
    got = launch(ctx, d, batch([x], 333), [(0, 330, 1)], 3)
    check("spiked", "spiked composed", got, [x], d, [1], 3)
    assert np.isfinite(got[1, :330]).all()


def test_zz_the_largest_ratio_of_this_file():
    assert NOTED, "runs behind the tests above"
    for k in sorted(NOTED):
        print("largest error / bound, %s: %.3f" % (k, WORST[k]))
    print("largest error / bound over this file: %.3f" % max(WORST[k] for k in NOTED))
    assert max(WORST[k] for k in NOTED) <= 1.0
