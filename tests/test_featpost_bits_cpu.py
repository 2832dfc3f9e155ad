"""tests/featpost_bits.py -- the bit-level host model of include/vorbispizza_pcm_featpost.h -- checked on its own, without a device: its
vectorised fused multiply-add against the rational one of tests/test_pcm_mfcc_gpu.py, its single stages inside the longdouble truth's
bound (tests/featpost_truth.py, as it stands), and THAT IT DISCRIMINATES: on featpost_bits.spiked's inputs every other order of the
window's sums than the header's changes the bits of a share of the elements, and so does a delta chain run descending or unfused.  The
shares are conditions (SPIKED and ROW_SPIKED below are the cases tests/test_pcm_featpost_limits_gpu.py runs on the device), not
measurements: a model that passed them by could be any of these orders.

Shares of changed elements, running / descending / R first / chunks first, as printed here:
    near W 100             0.479 / 0.579 / 0.035 / 0          far W 300 centred      0.013 / 0.011 / 0.011 / 0.011
    near W 200 centred     0.739 / 0.592 / 0.228 / 0.055      far W 600              0.018 / 0.012 / 0.018 / 0
    near W 4               0.007 / 0.169 / 0     / 0          far row                0.841 / 0.841 / 0.560 / 0
    near row               0.830 / 0.289 / 0.496 / 0          (a row has no left partial chunk: chunks first is the stated order)"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import featpost_bits as fb  # noqa: E402
import featpost_truth as pt  # noqa: E402
from f32_model import fma32_rational  # noqa: E402
from featpost_bits import ROW_SPIKED, SPIKED  # noqa: E402


def feats(n, D, seed, offset=0.0):
    """tests/test_pcm_featpost_gpu.py's input: seeded noise around a slow ramp per column"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)[:, None]
    return (offset + rng.standard_normal((n, D)) + 0.01 * t * np.cos(np.arange(D))[None, :]).astype(np.float32)


def fma_cases():
    """a, b, c float32: noise times noise plus an addend spread over 16 decades; products that lie exactly midway between two float32
    values (odd integers of 25 bits) with an addend of 0, of +-2^-60 and +-2^-30 (far below the float64 sum's last bit: the tie is
    broken by the error term alone), of +-1 and +-2 (an exact result, no tie), and with both signs of the product"""
    rng = np.random.default_rng(11)
    N = 1500
    a, b = rng.standard_normal(N), rng.standard_normal(N)
    c = rng.standard_normal(N) * 10.0 ** rng.uniform(-8, 8, N)
    odd = rng.integers(2048, 2896, (2, 60)) * 2 + 1  # 4097 .. 5791: the product is odd and in [2^24, 2^25)
    assert ((odd[0] * odd[1] >= 2 ** 24) & (odd[0] * odd[1] < 2 ** 25)).all()
    ta, tb, tc = [], [], []
    for add in (0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -30, -2.0 ** -30, 1.0, -1.0, 2.0, -2.0):
        for sign in (1.0, -1.0):
            ta.append(sign * odd[0]), tb.append(odd[1].astype(np.float64)), tc.append(np.full(60, add))
    cat = lambda head, tail: np.concatenate([head] + tail).astype(np.float32)  # noqa: E731
    return cat(a, ta), cat(b, tb), cat(c, tc), N


def test_the_vectorised_fma_is_the_rational_one():
    a, b, c, N = fma_cases()
    got = fb.fma32(a, b, c)
    assert got.dtype == np.float32
    want = np.array([fma32_rational(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    # the forced ties are ties: a tiny addend of either sign moves the result to the float32 on its side, none leaves the even one
    zero, up, down = (got[N + 120 * k:N + 120 * k + 60] for k in (0, 1, 2))
    assert (up > down).all() and ((zero == up) | (zero == down)).all() and (up - down == 2).all()
    assert (zero.view(np.uint32) & 1 == 0).all()
    # and a product rounded to float32 before the sum (no fused step) is told apart
    unfused = ((a * b).astype(np.float32) + c).astype(np.float32)
    assert (unfused.view(np.uint32) != got.view(np.uint32)).mean() > 0.2
    # the float64 step of the variance, in rationals: a case whose product needs more than 53 bits
    m = 1.0 + 2.0 ** -30
    assert fb.fma64(-m, m, 1.0) == -(2.0 ** -29) - 2.0 ** -60 and -m * m + 1.0 == -(2.0 ** -29)


STAGES = [dict(delta_order=3, delta_window=2), dict(delta_order=3, delta_window=8), dict(norm="row"), dict(norm="row", norm_vars=True),
          dict(norm="sliding"), dict(norm="sliding", norm_vars=True), dict(norm="sliding", cmn_window=100, min_window=30, center=True),
          dict(norm="sliding", cmn_window=100, min_window=30, center=True, norm_vars=True)]


@pytest.mark.parametrize("stage", range(len(STAGES)))
def test_the_single_stages_lie_inside_the_truths_bound(stage):
    """noise plus ramp and the rows whose mean is 500 times their deviation, n = 700 and n = 65 (Kaldi's default window of 600 among
    the sliding ones): error over the longdouble bound, as it stands, at most 1"""
    d = pt.spec_of(**STAGES[stage])
    for n, offset in ((700, 0.0), (700, 500.0), (65, 0.0)):
        x = feats(n, 3, 30 + stage, offset)
        got = fb.model(x, d)
        want, bound = pt.truth(x, d)
        r = pt.ratio(got, want, bound)
        print("model error / bound, n %d offset %g: %.3f" % (n, offset, r))
        assert got.dtype == np.float32 and got.shape == want.shape and r <= 1.0


def test_a_composition_is_the_two_models_in_order():
    x = feats(150, 3, 5)
    d = pt.spec_of(norm="sliding", cmn_window=40, min_window=7, norm_vars=True, delta_order=2)
    only_norm, only_deltas = dict(d, delta_order=0), dict(d, norm="none")
    assert (fb.model(x, d) == fb.deltas(fb.normalise(x, only_norm), only_deltas)).all()
    assert (fb.model(x, dict(d, deltas_first=True)) == fb.normalise(fb.deltas(x, only_deltas), only_norm)).all()
    assert fb.model(x, d).shape == (150, 9) and not (fb.model(x, d) == fb.model(x, dict(d, deltas_first=True))).all()
    assert fb.model(x[:0], d).shape == (0, 9)


def shares(case):
    name, n, D, seed, far, stage = case
    x, d = fb.spiked(n, D, seed, far), pt.spec_of(**stage)
    ref = fb.normalise(x, d)
    assert np.isfinite(ref).all(), name
    out = {o: fb.share(ref, fb.normalise(x, d, o)) for o in fb.ORDERS}
    print("%-20s %s" % (name, "  ".join("%s %.3f" % (o, out[o]) for o in fb.ORDERS)))
    return out


def test_the_model_tells_the_orders_of_the_sums_apart():
    """each of the four other orders changes the bits of at least 1 % of the elements in at least one sliding spiked case; the running
    sum and the R-first order also in a row case; every output is finite"""
    sliding = [shares(c) for c in SPIKED]
    rows = [shares(c) for c in ROW_SPIKED]
    for o in fb.ORDERS:
        assert max(s[o] for s in sliding) >= 0.01, o
    for o in ("running", "r_first"):
        assert max(s[o] for s in rows) >= 0.01, o


def test_the_spiked_input_is_what_it_says():
    for far in (False, True):
        x = fb.spiked(700, 3, 7, far)
        assert x.dtype == np.float32 and (x == fb.spiked(700, 3, 7, far)).all()
        big = np.abs(x) >= 2.0 ** 36
        assert (np.abs(x[~big]) < 8).all() and 0.08 < big.mean() < 0.25
        for c in range(3):
            at = np.nonzero(big[:, c])[0]
            plus, minus = at[x[at, c] > 0], at[x[at, c] < 0]
            assert len(plus) == len(minus) and x[:, c].astype(np.float64)[big[:, c]].sum() == 0
            near = np.array([(x[p + 1:p + 4, c] == -x[p, c]).any() for p in plus])
            wide = np.array([(x[p + 40:p + 100, c] == -x[p, c]).any() for p in plus])
            assert (near | wide).all() and near.all() == (not far)
            gaps = np.diff(plus)
            assert gaps.min() >= 1 and np.median(gaps) >= 5
            exps = np.log2(x[plus, c].astype(np.float64))
            assert (exps == np.round(exps)).all() and exps.min() >= 36 and exps.max() <= 43


def test_the_model_tells_the_delta_chains_apart():
    """on plain noise a descending chain and an unfused multiply-then-add each change more than half of the elements of block 1 at
    window 8, the chain of 16 steps that the device tests run (0.81 and 0.64).  At window 2 block 1 is a chain of four steps, the first
    of them exact in either form, and fewer elements can differ (0.53 and 0.36): there the condition is that some do"""
    x = np.random.default_rng(3).standard_normal((200, 4)).astype(np.float32)
    for w, least in ((8, 0.5), (2, 0.1)):
        d = pt.spec_of(delta_order=3, delta_window=w)
        ref = fb.deltas(x, d)
        assert (ref[:, :4].view(np.uint32) == x.view(np.uint32)).all()
        for other in (dict(descending=True), dict(fused=False)):
            s = fb.share(ref[:, 4:8], fb.deltas(x, d, **other)[:, 4:8])
            print("deltas, window %d, %s: %.3f" % (w, other, s))
            assert s > least
