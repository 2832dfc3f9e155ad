"""vpz_pcm_true_peak (include/vorbispizza_pcm_r128.h, csrc/pcm_truepeak.hip) on the device.

TRUTH: tests/r128_truth.py -- float64, numpy.convolve of the zero-stuffed row with the prototype -- over the cases of tests/r128_cases.py,
computed once per row and never changed.
BOUND (derived at r128_truth.bound): |true_peak - truth| <= (12 + 2) * 2^-24 * max over outputs of sum_k |h[p + k F]| |x[i - k]|; 0 where
F = 1.  The sample peak is exact.  The largest error / bound is printed.
SHAPES: the smallest at which the kernel can go wrong, named from its constants (T = kTpTile elements of a tile): rows around the twelve
taps and around one and two tiles, the peak behind the last sample, at the front and across tile boundaries, 1 to 255 channels with the
peak in the sample a tile boundary cuts, more descriptors than the grid's y, every factor's rates.  tests/test_r128_cpu.py holds each case
to the shape it is named for."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import r128_cases as rc  # noqa: E402
import r128_truth as rt  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SENTINEL, SAMPLE_SENTINEL = -7.25, -3.5
T = rc.T


def launch(ctx, case, order=None, gap=3, extra_rows=1, first=0, fill=9.0, rows=None, sample_peak=True):
    """one vpz_pcm_true_peak launch over the case's rows (or the listed ones): the windows lie in one source array with `gap` elements of
    `fill` in front of each (odd offsets; other members' samples), row i goes to destination row order[i] of extra_rows more rows than
    are named.  -> (true_peak [rows], sample_peak [rows] or None, as numpy), sentinels where nothing was written"""
    import torch
    from vorbispizza_amd import capi
    picked = list(range(len(case.rows))) if rows is None else list(rows)
    n = len(picked)
    order = list(range(n)) if order is None else list(order)
    parts, desc, at = [], [], first
    if first:
        parts.append(np.full(first, fill, dtype=np.float32))
    for i, k in enumerate(picked):
        r = case.rows[k]
        parts.append(np.full(gap, fill, dtype=np.float32))
        at += gap
        desc.append((at, r.shape[0], order[i]))
        parts.append(r.reshape(-1))
        at += r.size
    parts.append(np.full(5, fill, dtype=np.float32))
    src = torch.from_numpy(np.concatenate(parts)).to("cuda:0")
    dst_rows = max(order + [-1]) + 1 + extra_rows
    tp = torch.full((dst_rows + 2,), SENTINEL, dtype=torch.float32, device="cuda:0")
    sp = torch.full((dst_rows + 2,), SAMPLE_SENTINEL, dtype=torch.float32, device="cuda:0") if sample_peak else None
    # (one element of sentinel in front of and behind both outputs)
    capi.pcm_true_peak(ctx, src, case.channels, case.fs, desc, out=(tp[1: 1 + dst_rows], None if sp is None else sp[1: 1 + dst_rows]))
    ctx.synchronize()
    tp, sp = tp.cpu().numpy(), None if sp is None else sp.cpu().numpy()
    assert tp[0] == tp[-1] == SENTINEL and (sp is None or sp[0] == sp[-1] == SAMPLE_SENTINEL)
    return tp[1:-1], None if sp is None else sp[1:-1]


def check(case, tp, sp, order=None, rows=None):
    """every named row against the truth and the bound, unnamed rows untouched; -> the largest error / bound"""
    picked = list(range(len(case.rows))) if rows is None else list(rows)
    order = list(range(len(picked))) if order is None else list(order)
    worst = 0.0
    for i, k in enumerate(picked):
        want_tp, want_sp, bound = rc.truth(case.name, k)
        got_tp, got_sp = float(tp[order[i]]), float(sp[order[i]])
        assert got_sp == want_sp, (case.name, k, got_sp, want_sp)
        assert tp[order[i]].view(np.uint32) >= sp[order[i]].view(np.uint32), (case.name, k)  # (non-negative floats: their bits order them)
        if not np.isfinite(want_tp):
            assert got_tp == want_tp, (case.name, k)
            continue
        err = abs(got_tp - want_tp)
        assert err <= bound, (case.name, k, got_tp, want_tp, err / bound if bound else np.inf)
        worst = max(worst, err / bound if bound else 0.0)
    named = set(order)
    for row in range(len(tp)):
        if row not in named:
            assert tp[row] == SENTINEL and sp[row] == SAMPLE_SENTINEL, row
    return worst


def shuffled(n, seed=7):
    """n rows out of order over n + 2 destination rows: two in between stay unnamed"""
    return [int(v) for v in np.random.default_rng(seed).permutation(n + 2)[:n]]


@pytest.mark.parametrize("name", ["rows", "shapes"] + ["channels_%d" % c for c in rc.CHANNEL_COUNTS]
                         + ["rate_%d" % fs for fs in (44100, 96000, 191999, 192000, 384000)] + ["placement"])
def test_true_peak_and_sample_peak_against_the_truth(ctx, name):
    case = rc.cases()[name]
    order = shuffled(len(case.rows))
    fill = 1e6 if name == "placement" else 9.0  # (what lies around a window is another member: it must not leak into the halo or the tail)
    tp, sp = launch(ctx, case, order=order, fill=fill, gap=5 if name == "placement" else 3)
    worst = check(case, tp, sp, order)
    print("%s: largest error / bound %.3g" % (name, worst))
    if name == "rows":
        assert tp[order[0]] == 0.0 and sp[order[0]] == 0.0  # an empty window
    if name == "shapes":
        for i in range(6):
            assert abs(tp[order[i]] - rc.PAIR_PEAK) < 0.03 and sp[order[i]] == np.float32(rc.PAIR), i  # (a kernel without tail or halo reads 0.5)
        assert tp[order[7]] == sp[order[7]] == np.float32(0.7)
    if name in ("rate_192000", "rate_384000"):
        assert tp[order].tobytes() == sp[order].tobytes()  # F = 1


def test_f_1_and_the_sample_peak_are_pcm_loudness_peak_bits(ctx):
    import torch
    from vorbispizza_amd import capi
    for name in ("rate_192000", "rate_44100", "channels_3"):
        case = rc.cases()[name]
        tp, sp = launch(ctx, case, gap=0, extra_rows=0)
        flat = np.concatenate([r.reshape(-1) for r in case.rows] + [np.full(5, 9.0, dtype=np.float32)])
        at, desc = 0, []
        for i, r in enumerate(case.rows):
            desc.append((at, r.shape[0], i))
            at += r.size
        _, peak = capi.pcm_loudness(ctx, torch.from_numpy(flat).to("cuda:0"), case.channels, case.fs, desc)
        ctx.synchronize()
        assert peak.cpu().numpy().tobytes() == sp.tobytes(), name
        if name == "rate_192000":
            assert tp.tobytes() == sp.tobytes()


def test_more_descriptors_than_the_grid_holds(ctx):
    case = rc.cases()["grid"]
    order = [int(v) for v in np.random.default_rng(9).permutation(rc.GRID_ROWS)]
    tp, sp = launch(ctx, case, order=order, gap=1, extra_rows=3)
    checked = rc.grid_checked_rows()
    worst = 0.0
    for k in checked:
        want_tp, want_sp, bound = rc.truth("grid", k)
        assert float(sp[order[k]]) == want_sp and abs(float(tp[order[k]]) - want_tp) <= bound, k
        worst = max(worst, abs(float(tp[order[k]]) - want_tp) / bound if bound else 0.0)
    print("grid: largest error / bound %.3g over %d rows" % (worst, len(checked)))
    lengths = np.array([r.shape[0] for r in case.rows])
    assert (tp[np.array(order)[lengths == 0]] == 0).all() and (tp[: rc.GRID_ROWS] != SENTINEL).all() and (tp[rc.GRID_ROWS:] == SENTINEL).all()
    assert (tp[: rc.GRID_ROWS].view(np.uint32) >= sp[: rc.GRID_ROWS].view(np.uint32)).all()


def test_a_row_alone_among_others_and_scaled(ctx):
    case = rc.cases()["placement"]
    k = 3  # (more than one tile)
    alone_tp, alone_sp = launch(ctx, case, rows=[k], gap=0, extra_rows=0)
    crowd_tp, crowd_sp = launch(ctx, case, order=shuffled(len(case.rows), 3), gap=7, first=2, fill=1e6)
    at = shuffled(len(case.rows), 3)[k]
    assert alone_tp[0].tobytes() == crowd_tp[at].tobytes() and alone_sp[0].tobytes() == crowd_sp[at].tobytes()
    # without the sample peaks the true peaks are the same bits
    only_tp, none = launch(ctx, case, rows=[k], sample_peak=False)
    assert none is None and only_tp[0].tobytes() == alone_tp[0].tobytes()
    # a power of two on the samples is that power on the peak, bit for bit (every operation a float32 multiply or fused multiply-add)
    scaled = rc.Case("scaled", case.fs, case.channels, [np.ldexp(case.rows[k], -3)])
    s_tp, s_sp = launch(ctx, scaled)
    assert s_tp[0] == np.ldexp(alone_tp[0], -3) and s_sp[0] == np.ldexp(alone_sp[0], -3) and s_tp[0] > 0


def test_non_finite_samples_cost_only_their_row(ctx):
    case = rc.cases()["nonfinite"]
    tp, sp = launch(ctx, case)
    check(case, tp, sp)
    clean_tp, clean_sp = launch(ctx, case, rows=[0, 2])
    assert tp[[0, 2]].tobytes() == clean_tp[:2].tobytes() and sp[[0, 2]].tobytes() == clean_sp[:2].tobytes()
    assert np.isfinite(tp[1]) and tp[1] >= np.float32(0.9) and sp[1] == np.float32(0.9)  # the NaN is passed over
    assert tp[3] == np.inf and sp[3] == np.inf


@pytest.mark.parametrize("fs", rt.SINE_RATES + [192000])
def test_the_faded_sines_on_the_device(ctx, fs):
    case = rc.cases()["sines_%d" % fs]
    tp, sp = launch(ctx, case)
    check(case, tp, sp)
    for i, (div, phase, amp) in enumerate(rt.SINES):
        dev = 20.0 * np.log10(float(tp[i]) / amp)
        print("%d Hz: fs/%d at %.1f degrees, amplitude %.2f: %+.3f dB on the device" % (fs, div, phase, amp, dev))
        if fs < 192000:
            assert rt.TOLERANCE_DB[0] <= dev <= rt.TOLERANCE_DB[1]
        else:
            assert tp[i] == sp[i]


def test_every_refusal_launches_nothing(ctx):
    import torch
    from vorbispizza_amd import capi
    L = capi.lib()
    fs, ch = 8000, 2
    src = torch.full((4000 * ch + 8,), 0.25, dtype=torch.float32, device="cuda:0")
    tp = torch.full((4,), SENTINEL, dtype=torch.float32, device="cuda:0")
    sp = torch.full((4,), SAMPLE_SENTINEL, dtype=torch.float32, device="cuda:0")
    rows = np.array([(3, 4000, 2), (0, 799, 0)], dtype=np.int64)

    def call(**kw):
        a = dict(ctx=ctx._h, src=src.data_ptr(), src_elems=src.numel(), channels=ch, rate=fs, n_rows=len(rows), rows=rows, tp=tp.data_ptr(),
                 sp=sp.data_ptr(), dst_rows=4)
        a.update(kw)
        rr = None if a["rows"] is None else np.ascontiguousarray(a["rows"], dtype=np.int64)
        return L.vpz_pcm_true_peak(a["ctx"], a["src"], a["src_elems"], a["channels"], a["rate"], a["n_rows"], None if rr is None else rr.ctypes.data,
                                   a["tp"], a["sp"], a["dst_rows"])

    def row(k, **kw):
        r = rows.copy()
        for name, v in kw.items():
            r[k, {"src": 0, "samples": 1, "row": 2}[name]] = v
        return r

    host = np.zeros(64, dtype=np.float32)
    refused = [dict(ctx=None), dict(src=None), dict(tp=None), dict(rows=None), dict(channels=0), dict(channels=256), dict(rate=7999), dict(rate=384001),
               dict(n_rows=-1), dict(dst_rows=-1), dict(dst_rows=2), dict(rows=row(0, src=-1)), dict(rows=row(0, src=9)), dict(rows=row(0, samples=-1)),
               dict(rows=row(0, samples=4004)), dict(rows=row(1, row=4)), dict(rows=row(1, row=-1)), dict(rows=row(1, row=2)),
               dict(src=src.data_ptr() + 2), dict(tp=tp.data_ptr() + 2), dict(sp=sp.data_ptr() + 2), dict(src_elems=src.numel() + (1 << 30)),
               dict(dst_rows=1 << 20), dict(src=host.ctypes.data, src_elems=64), dict(tp=host.ctypes.data), dict(sp=host.ctypes.data)]
    for change in refused:
        assert call(**change) == capi.E_INVALID_ARG, change
    ctx.synchronize()
    assert (tp == SENTINEL).all() and (sp == SAMPLE_SENTINEL).all()
    # ... and the call itself is good, with and without the sample peaks: rows 1 and 3 untouched
    assert call(sp=None) == capi.OK
    ctx.synchronize()
    first = tp.cpu().numpy()
    assert first[0] > 0.25 and first[2] > 0.25 and first[1] == first[3] == SENTINEL and (sp == SAMPLE_SENTINEL).all()
    assert call() == capi.OK
    ctx.synchronize()
    got, pk = tp.cpu().numpy(), sp.cpu().numpy()
    assert list(pk) == [0.25, SAMPLE_SENTINEL, 0.25, SAMPLE_SENTINEL] and got[1] == got[3] == SENTINEL
    # (a constant 0.25 that starts and stops abruptly overshoots: the window is a clip of its own)
    want = rt.true_peak(np.full((799, 2), 0.25), fs)
    assert abs(got[0] - want) <= rt.bound(np.full((799, 2), 0.25), fs) and got[0] > 0.25 and got[2] > 0.25
    assert call(n_rows=0) == capi.OK  # (no descriptors: nothing to do, nothing refused)
