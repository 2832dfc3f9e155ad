"""vpz_pcm_normalize (include/vorbispizza_pcm_normalize.h, csrc/pcm_normalize.hip) alone: no decoder, every launch through the C ABI.
Values, sums, peak, offset and gain against the numpy bit model (tests/normalize_truth.py) bit for bit, every value within the header's
derived bound of the longdouble truth; the padding +0.0 by bits, unnamed rows and the guards on either side of the destination a
sentinel; the same window at three offsets and rows gives the same bits; every refusal of the header writes nothing."""
import os
import sys

import numpy as np
import pytest
from gpu_context import ctx  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import normalize_cases as nc  # noqa: E402
import normalize_truth as nt  # noqa: E402

pytestmark = pytest.mark.gpu


def destination(dst_rows, C, frames, planar, s16, guard):
    """(whole flat device tensor, the destination's view inside it): every element a sentinel, `guard` of them on either side"""
    import torch
    body = dst_rows * C * frames
    whole = torch.full((guard + body + guard,), nc.SENTINEL_S16 if s16 else nc.SENTINEL_F32, dtype=torch.int16 if s16 else torch.float32,
                       device="cuda:0")
    return whole, whole[guard:guard + body].view((dst_rows, C, frames) if planar else (dst_rows, frames, C))


def check_untouched(whole, guard, dst_rows, named, s16):
    a = whole.cpu().numpy()
    sent = nc.SENTINEL_S16 if s16 else np.float32(nc.SENTINEL_F32)
    assert (a[:guard] == sent).all() and (a[a.size - guard:] == sent).all(), "a guard was written"
    body = a[guard:a.size - guard].reshape(dst_rows, -1)
    for r in range(dst_rows):
        if r not in named:
            assert (body[r] == sent).all(), ("an unnamed row was written", r)
    return body


def bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run_case(ctx, capi, case, results):
    """one call of a case; returns the largest error / bound of its values (float32 layouts) or 0"""
    import torch
    w = nc.window_of(case)
    src_np, offs = nt.lay_out([w] * len(nc.ROWS), case.frames, nc.GAPS)
    src = torch.from_numpy(src_np if src_np.size else np.zeros(1, dtype=np.float32)).to("cuda:0")
    guard = 3 + case.seed % 5  # moves the destination off the 16-byte boundaries
    whole, dst = destination(nc.DST_ROWS, case.C, case.frames, case.planar, case.s16, guard)
    spec = capi.NormSpec.make(case.mode, channels=case.C, target=case.target, eps=case.eps, ceiling=case.ceiling)
    rows = [(o, case.J, r) for o, r in zip(offs, nc.ROWS)]
    got = capi.pcm_normalize(ctx, src, rows, dst, spec, case.frames, gains=[case.gain] * len(rows), results=results)
    rc, res = got if results else (got, None)
    assert rc == capi.OK, (case.name, ctx.last_error())
    body = check_untouched(whole, guard, nc.DST_ROWS, set(nc.ROWS), case.s16)
    x = np.stack([w] * len(rows))
    kw = nc.spec_args(case)
    want = nt.model(x, **kw)
    expect = nt.expected_rows(want["y"], case.frames, case.planar, case.s16).reshape(len(rows), -1)
    for i, r in enumerate(nc.ROWS):
        assert np.array_equal(bits(body[r]), bits(expect[i])), (case.name, "row", r, int(np.argmax(bits(body[r]) != bits(expect[i]))))
        assert np.array_equal(bits(body[r]), bits(body[nc.ROWS[0]])), (case.name, "the same window, other bits")
    if results:
        for j, key in enumerate(capi.NORM_RESULT_FIELDS):
            assert np.array_equal(bits(res[:, j]), bits(want[key])), (case.name, key, res[:, j], want[key])
        # m and g from the DOWNLOADED statistics: float64 division and square root on the device are numpy's, bit for bit
        m, g = nt.offset_and_gain(res[:, 0], res[:, 1], res[:, 2], case.C * case.J, kw["mode"], case.target, case.eps, case.ceiling, kw["gains"])
        assert np.array_equal(bits(m), bits(res[:, 3])) and np.array_equal(bits(g), bits(res[:, 4])), case.name
    if case.s16:
        return 0.0
    y = body[list(nc.ROWS)].reshape((len(rows), case.C, case.frames) if case.planar else (len(rows), case.frames, case.C))
    y = (y if case.planar else y.transpose(0, 2, 1))[:, :, :case.J]
    ystar, bound, rho = nt.truth(x, **kw)
    assert (rho <= 0.5).all()
    ratio = nt.worst_ratio(y, ystar, bound)
    assert ratio <= 1.0, (case.name, ratio)
    return ratio


@pytest.mark.parametrize("C_", nc.CHANNELS)
def test_every_shape(ctx, C_):  # noqa: F811
    from vorbispizza_amd import capi
    worst = 0.0
    for i, case in enumerate(c for c in nc.shape_cases() if c.C == C_):
        worst = max(worst, run_case(ctx, capi, case, results=i % 2 == 0))
    print("largest error / bound, channels %d: %.4f" % (C_, worst))


def test_every_level_in_every_layout(ctx):  # noqa: F811
    from vorbispizza_amd import capi
    worst = max(run_case(ctx, capi, case, results=True) for case in nc.level_layout_cases())
    worst = max([worst] + [run_case(ctx, capi, case, results=False) for case in nc.level_layout_cases() if nc.plain(case)])
    print("largest error / bound, levels and layouts: %.4f" % worst)


def test_the_special_rows(ctx):  # noqa: F811
    from vorbispizza_amd import capi
    worst = max(run_case(ctx, capi, case, results=True) for case in nc.special_cases())
    print("largest error / bound, special rows: %.4f" % worst)


def big_call(ctx, capi, C, frames, n, planar, s16, mode, j_of):
    """n descriptors over a source [n][C][frames], J = j_of(r), delivered to the rows in reverse; everything against the model"""
    import torch
    rng = np.random.default_rng(n + frames)
    x = rng.uniform(-1.0, 1.0, (n, C, frames)).astype(np.float32)
    J = np.array([j_of(r) for r in range(n)], dtype=np.int64)
    whole, dst = destination(n + 1, C, frames, planar, s16, 5)
    rows = np.stack([np.arange(n, dtype=np.int64) * C * frames, J, n - 1 - np.arange(n, dtype=np.int64)], axis=1)
    spec = capi.NormSpec.make(mode, channels=C, target=0.5)
    rc, res = capi.pcm_normalize(ctx, torch.from_numpy(x).to("cuda:0"), rows, dst, spec, frames, results=True)
    assert rc == capi.OK, ctx.last_error()
    body = check_untouched(whole, 5, n + 1, set(range(n)), s16)[:n][::-1]  # by descriptor
    worst = 0.0
    for j in sorted(set(J.tolist())):
        sel = np.nonzero(J == j)[0]
        want = nt.model(x[sel][:, :, :j], nt.MODES[mode], target=0.5)
        expect = nt.expected_rows(want["y"], frames, planar, s16).reshape(len(sel), -1)
        assert np.array_equal(bits(body[sel]), bits(expect)), (j, "values")
        for k, key in enumerate(capi.NORM_RESULT_FIELDS):
            assert np.array_equal(bits(res[sel, k]), bits(want[key])), (j, key)
        if not s16 and j:
            ystar, bound, rho = nt.truth(x[sel][:, :, :j], nt.MODES[mode], target=0.5)
            got = body[sel].reshape((len(sel), C, frames) if planar else (len(sel), frames, C))
            got = (got if planar else got.transpose(0, 2, 1))[:, :, :j]
            ratio = nt.worst_ratio(got, ystar, bound)
            assert ratio <= 1.0 and (rho <= 0.5).all(), (j, ratio)
            worst = max(worst, ratio)
    return worst


def test_70000_descriptors_pass_every_grid_limit(ctx):  # noqa: F811
    from vorbispizza_amd import capi
    worst = big_call(ctx, capi, 1, 8, 70000, True, False, "meanvar", lambda r: r % 9)
    print("largest error / bound, 70 000 descriptors: %.4f" % worst)


def test_300_descriptors_of_2500_samples(ctx):  # noqa: F811
    from vorbispizza_amd import capi
    worst = big_call(ctx, capi, 2, 2504, 300, False, False, "meanvar", lambda r: 2500)
    print("largest error / bound, 300 descriptors of 2500 samples: %.4f" % worst)


def test_a_second_round_of_the_frames_major_grid(ctx):  # noqa: F811
    from vorbispizza_amd import capi
    big_call(ctx, capi, 3, 9, 4100, False, True, "rms", lambda r: 9 - r % 3)
    big_call(ctx, capi, 2, 8, 4100, False, False, "peak", lambda r: 8 - r % 2)


def test_every_refusal_writes_nothing(ctx):  # noqa: F811
    import ctypes as C
    import torch
    from vorbispizza_amd import capi
    L = capi.lib()
    C_, frames, J, dst_rows = 2, 40, 33, 3
    src = torch.from_numpy(nt.signal("noise", 1, 4 * C_ * frames, 5).reshape(-1)).to("cuda:0")
    need = capi.pcm_normalize_scratch(2, C_, frames)
    scratch = torch.zeros(need, dtype=torch.float64, device="cuda:0")
    result = torch.zeros(2 * 5, dtype=torch.float64, device="cuda:0")
    host = np.zeros(64, dtype=np.float64)

    def call(mode="meanvar", rows=((0, J, 0), (C_ * frames, J, 2)), gains=(1.0, 1.0), layout=capi.OUT_PLANAR, frames_=frames, channels=C_,
             src_=src, src_elems=None, dst_rows_=dst_rows, scratch_=scratch, scratch_doubles=None, result_=None, spec_edit=None, dst_=None,
             n_rows=None, null_rows=False, null_spec=False, **level):
        whole, dst = destination(dst_rows, C_, frames, True, layout in (capi.OUT_PLANAR_S16, capi.OUT_INTERLEAVED_S16), 4)
        spec = capi.NormSpec.make(mode, channels=1, **level)
        spec.channels = channels
        if spec_edit:
            spec_edit(spec)
        desc = (capi.NormRow * max(len(rows), 1))()
        for d, (s, n, r), g in zip(desc, rows, gains):
            d.src, d.samples, d.row, d.gain = s, n, r, g
        p = lambda t: None if t is None else (C.c_void_p(t) if isinstance(t, int) else C.c_void_p(t.data_ptr()))  # noqa: E731
        rc = L.vpz_pcm_normalize(ctx._h, p(src_), src.numel() if src_elems is None else src_elems, frames_,
                                 None if null_spec else C.byref(spec), len(rows) if n_rows is None else n_rows,
                                 None if null_rows else C.cast(desc, C.c_void_p), p(dst if dst_ is None else dst_), dst_rows_, layout,
                                 p(scratch_), (0 if scratch_ is None else scratch_.numel()) if scratch_doubles is None else scratch_doubles,
                                 p(result_))
        ctx.synchronize()
        a = whole.cpu().numpy()
        untouched = bool((a == a[0]).all())
        return rc, untouched

    assert call() == (capi.OK, False) and call(result_=result) == (capi.OK, False)  # the call the refusals are edits of
    assert call(mode="gain", scratch_=None) == (capi.OK, False)  # a plain gain needs no scratch memory
    assert call(rows=((0, 0, 0), (0, 0, 1)), scratch_=None, result_=result) == (capi.OK, False)  # nor do rows without samples
    nan, inf = float("nan"), float("inf")
    refusals = {
        "null spec": dict(null_spec=True), "null rows": dict(null_rows=True), "null source": dict(src_=None),
        "frames 0": dict(frames_=0), "negative rows": dict(n_rows=-1), "negative dst rows": dict(dst_rows_=-1),
        "negative source": dict(src_elems=-1), "layout 4": dict(layout=4), "layout -1": dict(layout=-1),
        "samples above frames": dict(rows=((0, frames + 1, 0),)), "negative samples": dict(rows=((0, -1, 0),)),
        "row out of range": dict(rows=((0, J, dst_rows),)), "negative row": dict(rows=((0, J, -1),)),
        "a row named twice": dict(rows=((0, J, 1), (C_ * frames, J, 1))),
        "more descriptors than rows": dict(rows=((0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 1, 0))),
        "negative src": dict(rows=((-1, J, 0),)),
        "the last channel leaves the source": dict(rows=((src.numel() - frames - J + 1, J, 0),)),
        "src behind the source": dict(rows=((src.numel() + 1, 0, 0),)),
        "the source shorter than said": dict(src_elems=frames + J - 1, rows=((0, J, 0),)),
        "a source claimed longer than its allocation": dict(src_elems=1 << 40),
        "host memory as source": dict(src_=host.ctypes.data), "host memory as scratch": dict(scratch_=host.ctypes.data, scratch_doubles=need),
        "host memory as result": dict(result_=host.ctypes.data), "a misaligned source": dict(src_=src.data_ptr() + 2),
        "a misaligned scratch": dict(scratch_=scratch.data_ptr() + 4, scratch_doubles=need - 1),
        "unknown mode 0": dict(spec_edit=lambda s: setattr(s, "mode", 0)), "unknown mode 5": dict(spec_edit=lambda s: setattr(s, "mode", 5)),
        "channels 0": dict(channels=0), "channels 256": dict(channels=256),
        "peak target 0": dict(mode="peak", target=0.0), "peak target nan": dict(mode="peak", target=nan),
        "rms target inf": dict(mode="rms", target=inf), "rms target negative": dict(mode="rms", target=-0.1),
        "gain 0": dict(mode="gain", gains=(1.0, 0.0)), "gain nan": dict(mode="gain", gains=(nan, 1.0)), "gain inf": dict(mode="gain", gains=(inf, 1.0)),
        "gain negative": dict(mode="gain", gains=(-1.0, 1.0), ceiling=0.5),
        "eps negative": dict(eps=-1e-9), "eps nan": dict(eps=nan), "eps negative in another mode": dict(mode="peak", eps=-1.0),
        "ceiling negative": dict(mode="peak", ceiling=-0.5), "ceiling nan": dict(mode="rms", ceiling=nan),
        "a ceiling with meanvar": dict(ceiling=0.5),
        "a reserved word": dict(spec_edit=lambda s: s.reserved.__setitem__(7, 1)),
        "no scratch": dict(scratch_=None), "scratch too small": dict(scratch_doubles=need - 1),
        "no scratch for a ceiling": dict(mode="gain", ceiling=0.5, scratch_=None),
        "no scratch for a gain's results": dict(mode="gain", scratch_=None, result_=result),
        "the source as destination": dict(dst_=src, dst_rows_=1),
    }
    for name, edit in refusals.items():
        assert call(**edit) == (capi.E_INVALID_ARG, True), (name, ctx.last_error())
    assert L.vpz_pcm_normalize(None, None, 0, 1, None, 0, None, None, 0, 0, None, 0, None) == capi.E_INVALID_ARG
    assert call() == (capi.OK, False)  # and the context still serves
