"""vpz_pcm_mfcc (include/vorbispizza_pcm_mfcc.h, csrc/pcm_fbank.hip) alone: no decoder.

The truth is tests/mfcc_truth.py's float64 restatement of the header's definition on top of tests/fbank_truth.py -- unfolded: the log of
the band sums, an explicit DCT, the lifter behind it, the energy of the scaled, centred frame, a plain float64 mean over the frames --
and the tolerance its derived bound, used as it stands.  The real frames of a row lie inside the bound; every element behind them is
pad_value bit for bit; rows no descriptor names and the guards on either side of the destination keep their sentinel; source elements
behind a row's L are NaN and never reach the output; every refusal returns VPZ_E_INVALID_ARG and writes nothing.  The signal is seeded
noise plus a tone (test_pcm_fbank_gpu.py's), at scale 32768.

Largest error / bound ratio observed on an MI355X over the cases of this file (test_zz_the_largest_ratio_of_this_file prints them):
0.43 over the windows of 2 to 7 samples; 0.18 at the defaults, 0.15 / 0.095 at n_ceps 1, 23 / 256 of 256; 0.30 over the options; 0.20 in
the three tiles; 0.32 for the energy without remove_dc, 0.11 on the all-zero row, 0.005 under the DC offset; 0.072 with the cepstral
mean; 0.19 in the grid's second round."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fbank_cases as fc  # noqa: E402
import fbank_truth as ft  # noqa: E402
import mfcc_truth as mt  # noqa: E402
from mfcc_truth import refused_specs  # noqa: E402
from pcm_support import GUARD, SENTINEL, guarded, place, signal  # noqa: E402
from f32_model import fma32_rational as fma32  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

WORST = {}
LOG_EPS = np.float32(np.log(2.0 ** -23))  # logf(2^-23): the float32 nearest to the logarithm


def launch(ctx, d, src, rows, dst_rows, F, d_src=None):
    """one vpz_pcm_mfcc call of spec dict d -> [dst_rows][T][n_ceps] float32 of the destination's body, the guards checked"""
    import torch
    from vorbispizza_amd import capi
    spec = capi.MfccSpec.make(**d)
    T, n = spec.n_frames(F), d["n_ceps"]
    whole, dst = guarded(dst_rows, n * T)
    d_src = torch.from_numpy(src).to("cuda:0") if d_src is None else d_src
    shape = (dst_rows, T, n) if d["frames_first"] else (dst_rows, n, T)
    assert capi.pcm_mfcc(ctx, d_src, rows, dst.view(shape), spec, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    bits = whole.cpu().numpy().view(np.uint32)
    assert (bits[:GUARD] == SENTINEL).all() and (bits[-GUARD:] == SENTINEL).all()
    body = bits[GUARD:-GUARD].view(np.float32)
    return body.reshape(shape) if d["frames_first"] else body.reshape(shape).transpose(0, 2, 1)


def tables(d):
    fb = mt.fbank_of(d)
    return ft.mel_weights64(fb), ft.operator64(fb)


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("error / bound %s: %.4f" % (key, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("pad_value", [0.0, -15.9424])
def test_the_defaults_at_every_kind_of_row_length(ctx, pad_value):
    """23 bands, 13 cepstra, 16 kHz, win 400, hop 160: L = 0, win - 1, win, win + hop - 1 and F"""
    d = mt.spec_of(pad_value=pad_value)
    F = 400 + 160 * 70 + 37
    Ls = [0, 399, 400, 559, F]
    assert [ft.n_frames(L, 400, 160) for L in Ls] == [0, 0, 1, 1, 71]
    windows = [signal(L, 200 + i) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    order = [5, 2, 7, 4, 1]
    got = launch(ctx, d, src, [(o, L, r) for o, L, r in zip(offs, Ls, order)], 8, F)
    assert got.shape == (8, 71, 13) and (got[[0, 3, 6]].view(np.uint32) == SENTINEL).all()
    W, B = tables(d)
    pad_bits = np.float32(pad_value).view(np.uint32)
    for w, L, r in zip(windows, Ls, order):
        TL = ft.n_frames(L, 400, 160)
        assert (got[r, TL:].view(np.uint32) == pad_bits).all(), L
        note("defaults", mt.check_row(got[r], w, d, W, B))
        assert TL == 0 or (got[r, :TL].view(np.uint32) != pad_bits).any()


@pytest.mark.parametrize("use_energy", [True, False])
@pytest.mark.parametrize("shape", ["1_of_23", "23_of_23", "256_of_256"])
def test_the_number_of_cepstra(ctx, shape, use_energy):
    """one cepstrum, as many as bands, and the largest log-mel tile: 256 bands at n_fft 1024"""
    change = {"1_of_23": dict(n_ceps=1), "23_of_23": dict(n_ceps=23),
              "256_of_256": dict(n_mels=256, n_ceps=256, n_fft=1024, win=800, hop=320, sample_rate=48000)}[shape]
    d = mt.spec_of(use_energy=use_energy, **change)
    win, hop = d["win"], d["hop"]
    F = win + hop * 18 + 5  # T = 19
    Ls = [F, F // 3, win - 1]
    windows = [signal(L, 300 + i, d["sample_rate"]) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    got = launch(ctx, d, src, [(o, L, r) for o, L, r in zip(offs, Ls, (2, 0, 3))], 4, F)
    assert (got[1].view(np.uint32) == SENTINEL).all()
    W, B = tables(d)
    for w, r in zip(windows, (2, 0, 3)):
        note("n_ceps " + shape, mt.check_row(got[r], w, d, W, B))


def test_tiles_and_the_same_bits_wherever_a_row_sits(ctx):
    """T_L around a 32- and a 64-frame boundary (a last tile with nr < nt, tiles with nr = 0), a pad-only row, and ONE WINDOW in three
    launches that pick 16-, 32- and 64-frame tiles beside different neighbours: the same bits in all three, with and without the mean"""
    import torch
    win, hop, crowd = 400, 160, 600
    F = win + hop * 97 + 13  # T = 98
    k = ft.kernel_constants(ROOT)
    assert mt.tile_plan(win, hop, 512, 23, 98, 8, 256, k)[0] == 32 and mt.tile_plan(win, hop, 512, 23, 98, crowd, 300, k)[0] == 64
    F16 = win + hop * 15 + 50  # T = 16
    assert mt.tile_plan(win, hop, 512, 23, 16, 8, 256, k)[0] == 16
    TLs = [31, 32, 33, 63, 64, 65, 16, 0]
    Ls = [win + hop * (t - 1) + 7 if t else win - 1 for t in TLs]
    host = signal(crowd * 67 + F + 8, 6)
    src = torch.from_numpy(host).to("cuda:0")
    starts = [3 + 1000 * i for i in range(len(Ls))]
    rows = [(a, L, r) for a, L, r in zip(starts, Ls, (5, 1, 7, 0, 3, 6, 2, 4))]
    rng = np.random.default_rng(8)
    many = [(a, L, i) for i, (a, L, _) in enumerate(rows)] + [(i * 67 + 1, int(rng.integers(0, F + 1)), i) for i in range(len(rows), crowd)]
    for subtract_mean in (False, True):
        d = mt.spec_of(subtract_mean=subtract_mean)
        W, B = tables(d)
        few = launch(ctx, d, host, rows, 8, F, src)
        for a, L, r in rows:
            note("tiles of 32", mt.check_row(few[r], host[a: a + L], d, W, B))
        big = launch(ctx, d, host, many, crowd, F, src)
        for i, (a, L, r) in enumerate(rows):
            assert big[i].tobytes() == few[r].tobytes(), TLs[i]
        for a, L, r in many[len(rows)::149]:
            note("tiles of 64", mt.check_row(big[r], host[a: a + L], d, W, B))
        a16, L16 = starts[6], Ls[6]
        small = launch(ctx, d, host, [(a16 + 400, 2000, 0), (a16, L16, 2), (a16 + 9, win, 1)], 3, F16, src)
        assert small.shape[1] == 16 and small[2].tobytes() == few[2, :16].tobytes() == big[6, :16].tobytes()
        note("tiles of 16", mt.check_row(small[0], host[a16 + 400: a16 + 2400], d, W, B))


def test_layouts_htk_order_and_the_options_of_the_mel_stage(ctx):
    """both layouts are the same bits; with htk_compat the frame is the plain call's bits rotated (c[0] last) -- all of them with the
    energy, all but the sqrt(2) row without, and that row inside the bound; remove_dc off and on, three windows"""
    import torch
    F = 400 + 160 * 34 + 11  # T = 35
    Ls = [F, F - 161, 1000]
    windows = [signal(L, 50 + i) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    d_src = torch.from_numpy(src).to("cuda:0")
    rows = [(o, L, r) for o, L, r in zip(offs, Ls, (2, 0, 1))]
    for window in ft.WINDOWS:
        for remove_dc in (True, False):
            for use_energy in (True, False):
                base = mt.spec_of(window=window, remove_dc=remove_dc, use_energy=use_energy)
                W, B = tables(base)
                plain = launch(ctx, base, src, rows, 3, F, d_src)
                for w, (_, _, r) in zip(windows, rows):
                    note("options", mt.check_row(plain[r], w, base, W, B))
                other = launch(ctx, dict(base, frames_first=False), src, rows, 3, F, d_src)
                assert np.ascontiguousarray(other).tobytes() == plain.tobytes()
                htk = launch(ctx, dict(base, htk_compat=True), src, rows, 3, F, d_src)
                assert htk[:, :, :-1].tobytes() == plain[:, :, 1:].tobytes()
                for w, (_, _, r) in zip(windows, rows):
                    note("options htk", mt.check_row(htk[r], w, dict(base, htk_compat=True), W, B))
                TL = [ft.n_frames(L, 400, 160) for L in Ls]
                if use_energy:
                    assert htk[:, :, -1].tobytes() == plain[:, :, 0].tobytes()
                else:  # (HTK's C0 is sqrt(2) times Kaldi's)
                    for L, (_, _, r) in zip(TL, rows):
                        ratio = htk[r, :L, -1].astype(np.float64) / plain[r, :L, 0]
                        assert np.abs(ratio - np.sqrt(2.0)).max() < 1e-5


def test_the_energy(ctx):
    """an all-zero row: logf(2^-23)'s bits, and logf(energy_floor)'s with a floor above it; a floor below the energies changes nothing;
    a DC offset of 500 times the signal stays inside the bound, with remove_dc (the mean is not folded) and without"""
    F = 400 + 160 * 40 + 3
    zero = np.zeros(F, dtype=np.float32)
    dc = (0.5 + 1e-3 * np.random.default_rng(78).standard_normal(F) + 1e-3 * np.sin(2 * np.pi * 440.0 * np.arange(F) / 16000)).astype(np.float32)
    src, offs = place([zero, dc])
    rows = [(offs[0], F, 0), (offs[1], F, 1)]
    d = mt.spec_of()
    got = launch(ctx, d, src, rows, 2, F)
    assert (got[0, :, 0].view(np.uint32) == LOG_EPS.view(np.uint32)).all()
    note("energy zero row", mt.check_row(got[0], zero, d))
    note("energy dc", mt.check_row(got[1], dc, d))
    V, _ = mt.mfcc_truth(dc, d)
    assert np.abs(V[:, 0] - np.log(400 * (32768 * 1.4e-3) ** 2)).max() < 1.0  # (the signal's energy, not the offset's)
    floored = dict(d, energy_floor=1000.0)
    got = launch(ctx, floored, src, rows, 2, F)
    assert (got[0, :, 0].view(np.uint32) == np.float32(np.log(1000.0)).view(np.uint32)).all()
    note("energy floor", mt.check_row(got[1], dc, floored))
    low = launch(ctx, dict(d, energy_floor=1e-3), src, rows, 2, F)
    assert low[1].tobytes() == launch(ctx, d, src, rows, 2, F)[1].tobytes()
    assert (low[0, :, 0].view(np.uint32) == np.float32(np.log(float(np.float32(1e-3)))).view(np.uint32)).all()
    raw = dict(d, remove_dc=False)
    got = launch(ctx, raw, src, rows, 2, F)
    note("energy without remove_dc", mt.check_row(got[1], dc, raw))
    assert np.abs(got[1, :, 0] - np.log(400 * (32768 * 0.5) ** 2)).max() < 0.1  # (now the offset's)


@pytest.mark.parametrize("name", ["hop2_2_2_32", "win3_3_2_32", "win3_3_3_32", "win4_4_2_32", "win5_5_2_34", "hop6_7_6_36"])
def test_small_windows_and_hops(ctx, name):
    """the smallest cases of tests/fbank_cases.py: an odd win, an odd hop (no skew) and even hops (a skewed span), where the energy's
    walk through the span wraps like the mean's"""
    change, F = fc.small(name)
    win, hop, n_mels = change["win"], change["hop"], change["n_mels"]
    d = mt.spec_of(n_ceps=n_mels, **change)
    Ls = [F, F - 1, F // 3, win, win - 1]
    windows = [signal(L, 9 * i + win, 8000) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    order = [4, 0, 5, 2, 6]
    got = launch(ctx, d, src, [(o, L, r) for o, L, r in zip(offs, Ls, order)], 7, F)
    assert got.shape == (7, 71, n_mels) and (got[[1, 3]].view(np.uint32) == SENTINEL).all()
    W, B = tables(d)
    for w, r in zip(windows, order):
        note("small " + name, mt.check_row(got[r], w, d, W, B))


@pytest.mark.parametrize("frames_first", [True, False])
def test_the_cepstral_mean(ctx, frames_first):
    """T_L = 0, 1, 63, 64, 65 and 129 -- the edges of the 64 partial sums --: inside the bound, pad frames untouched; a row is the same
    bits alone and as row 3 of 5; without the flag the launch leaves the plain values"""
    win, hop = 400, 160
    TLs = [0, 1, 63, 64, 65, 129]
    Ls = [win - 1 if t == 0 else win + hop * (t - 1) + 3 for t in TLs]
    F = win + hop * 130 + 9  # T = 131
    windows = [signal(L, 400 + i) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    d = mt.spec_of(subtract_mean=True, frames_first=frames_first, pad_value=-3.5)
    rows = [(o, L, r) for o, L, r in zip(offs, Ls, (4, 0, 5, 2, 6, 1))]
    got = launch(ctx, d, src, rows, 7, F)
    assert (got[3].view(np.uint32) == SENTINEL).all()
    W, B = tables(d)
    pad_bits = np.float32(-3.5).view(np.uint32)
    for w, t, (_, _, r) in zip(windows, TLs, rows):
        assert (got[r, t:].view(np.uint32) == pad_bits).all()
        note("cepstral mean", mt.check_row(got[r], w, d, W, B))
        if t > 1:
            assert np.abs(got[r, :t].astype(np.float64).mean(axis=0)).max() < 1e-4
    assert (got[0, 0] == 0).all()  # (one frame: itself the mean)
    plain = launch(ctx, dict(d, subtract_mean=False), src, rows, 7, F)
    assert plain[1, :129].tobytes() != got[1, :129].tobytes() and plain[1, 129:].tobytes() == got[1, 129:].tobytes()
    alone = launch(ctx, d, src, [(offs[4], Ls[4], 0)], 1, F)
    five = launch(ctx, d, src, [(offs[1], Ls[1], 0), (offs[5], Ls[5], 1), (offs[0], Ls[0], 2), (offs[4], Ls[4], 3), (offs[2], Ls[2], 4)], 5, F)
    assert alone[0].tobytes() == five[3].tobytes() == got[6].tobytes()


def test_more_descriptors_than_the_grid_holds_side_by_side(ctx):
    """2100 tiny rows (the grid's y holds 2048: workgroups of both kernels take a second descriptor) in a destination of 2150 rows"""
    n, dst_rows = 2100, 2150
    d = mt.spec_of(win=32, hop=16, n_fft=32, n_mels=8, n_ceps=5, sample_rate=8000, low_freq=100.0, subtract_mean=True)
    F = 32 + 16 * 6 + 5  # T = 7 (second_round_lengths asks for rows of win + 90 samples)
    k = ft.kernel_constants(ROOT)
    assert n > k["kFbMaxGridY"]
    rng = np.random.default_rng(4)
    Ls = fc.second_round_lengths(n, F, 32, rng)
    stride = F + 3
    src = np.full(1 + n * stride, np.nan, dtype=np.float32)
    x = (0.5 * rng.standard_normal((n, F))).astype(np.float32)
    for i in range(n):
        src[1 + i * stride: 1 + i * stride + Ls[i]] = x[i, : Ls[i]]
    order = rng.permutation(dst_rows)[:n]
    got = launch(ctx, d, src, [(1 + i * stride, int(Ls[i]), int(order[i])) for i in range(n)], dst_rows, F)
    assert not np.isnan(got[order]).any()
    rest = np.setdiff1d(np.arange(dst_rows), order)
    assert rest.size == 50 and (got[rest].view(np.uint32) == SENTINEL).all()
    W, B = tables(d)
    checked = sorted(set(range(0, n, 41)) | set(range(6)) | set(range(2048, 2054)) | {n - 1})
    for i in checked:
        note("second round", mt.check_row(got[order[i]], x[i, : Ls[i]], d, W, B))


def raw_call(ctx, src_ptr, src_elems, frames, spec, rows, dst_ptr, dst_rows, n_rows=None, null_rows=False, handle=True, null_spec=False):
    from vorbispizza_amd import capi
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    return capi.lib().vpz_pcm_mfcc(ctx._h if handle else None, src_ptr, src_elems, frames, None if null_spec else C.byref(spec),
                                   desc.shape[0] if n_rows is None else n_rows, None if null_rows else desc.ctypes.data, dst_ptr, dst_rows)


def test_every_refusal_is_invalid_arg_and_writes_nothing(ctx):
    import torch
    from vorbispizza_amd import capi
    F, dst_rows, n = 1000, 4, 13
    T = 1 + (F - 400) // 160
    src = torch.from_numpy(signal(2000, 9)).to("cuda:0")
    whole, dst = guarded(dst_rows, n * T)
    spec = capi.MfccSpec.make(subtract_mean=True)
    good = dict(src_ptr=src.data_ptr(), src_elems=2000, frames=F, spec=spec, rows=[(3, 500, 1), (400, 1000, 3)], dst_ptr=dst.data_ptr(), dst_rows=dst_rows)
    pinned = torch.zeros(dst_rows * n * T, dtype=torch.float32, pin_memory=True)
    host_src = torch.full((2000,), 0.5, dtype=torch.float32, pin_memory=True)
    bad = [("no context", dict(handle=False)), ("null source", dict(src_ptr=None)), ("null destination", dict(dst_ptr=None)), ("null rows", dict(null_rows=True)),
           ("null spec", dict(null_spec=True)), ("frames < win", dict(frames=399, rows=[(3, 100, 1)])), ("frames 0", dict(frames=0, rows=[(3, 0, 1)])),
           ("n_rows < 0", dict(n_rows=-1)), ("dst_rows < 0", dict(dst_rows=-1)), ("src_elems < 0", dict(src_elems=-1)),
           ("samples > frames", dict(rows=[(3, 1001, 1)])), ("samples < 0", dict(rows=[(3, -1, 1)])), ("src < 0", dict(rows=[(-1, 10, 1)])),
           ("span leaves the source", dict(rows=[(1001, 1000, 1)])), ("src behind the source", dict(rows=[(2001, 0, 1)])),
           ("row out of range", dict(rows=[(3, 500, 4)])), ("row < 0", dict(rows=[(3, 500, -1)])),
           ("a row named twice", dict(rows=[(3, 500, 1), (400, 500, 1)])), ("more descriptors than rows", dict(rows=[(0, 1, 0)] * 5)),
           ("destination not aligned", dict(dst_ptr=dst.data_ptr() + 2)), ("source not aligned", dict(src_ptr=src.data_ptr() + 1)),
           ("destination longer than its allocation", dict(dst_rows=(1 << 40) // (n * T * 4))), ("source longer than its allocation", dict(src_elems=1 << 38)),
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
    body = whole.cpu().numpy().view(np.uint32)[GUARD:-GUARD].reshape(dst_rows, T, n)
    assert (body[[0, 2]] == SENTINEL).all() and np.isfinite(body[[1, 3]].view(np.float32)).all()


@pytest.mark.parametrize("subtract_mean", [False, True])
def test_a_sample_that_is_not_finite(ctx, subtract_mean):
    """without the mean: exactly the frames that cover the sample are not finite, in every coefficient; with it: the whole row's real
    frames.  Every other row is the same bits as without the sample"""
    win, hop = 400, 160
    F = win + hop * 40 + 3
    Ls = [F, F - 500, F]
    for bad in (np.inf, -np.inf, np.nan):
        windows = [signal(L, 70 + i) for i, L in enumerate(Ls)]
        src, offs = place(windows)
        rows = [(o, L, r) for r, (o, L) in enumerate(zip(offs, Ls))]
        d = mt.spec_of(subtract_mean=subtract_mean, pad_value=1.5)
        clean = launch(ctx, d, src, rows, 3, F)
        at = 2000
        src[offs[1] + at] = bad
        got = launch(ctx, d, src, rows, 3, F)
        assert got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[2].tobytes()
        TL = ft.n_frames(Ls[1], win, hop)
        covers = np.array([t * hop <= at < t * hop + win for t in range(TL)])
        assert covers.sum() == 2 and not covers[[10, 13]].any()
        finite = np.isfinite(got[1, :TL])
        if subtract_mean:
            assert not finite.any()
        else:
            assert not finite[covers].any() and finite[~covers].all()
            assert got[1, :TL][~covers].tobytes() == clean[1, :TL][~covers].tobytes()
        assert (got[1, TL:] == 1.5).all()


def test_the_cepstra_are_the_stated_chain_over_vpz_pcm_fbank_bit_for_bit(ctx):
    """items 1 and 2 of the definition as bits: the log-mel values are vpz_pcm_fbank's, and a coefficient is the fused chain of
    vpz_mfcc_table's row over them, b ascending -- in the HTK order too; with one band and no lifter C is 1 and the cepstrum is the
    log-mel value itself"""
    import torch
    from fbank_cases import launch as fbank_launch
    from vorbispizza_amd import capi
    F = 400 + 160 * 8 + 11  # T = 9
    Ls = [F, 1000]
    windows = [signal(L, 90 + i) for i, L in enumerate(Ls)]
    src, offs = place(windows)
    rows = [(offs[0], Ls[0], 1), (offs[1], Ls[1], 0)]
    for change in (dict(use_energy=False, htk_compat=True), dict(n_ceps=5), dict(n_mels=1, n_ceps=1, lifter=0.0, use_energy=False)):
        d = mt.spec_of(**change)
        E = fbank_launch(ctx, mt.fbank_of(d), src, rows, 2, F)
        got = launch(ctx, d, src, rows, 2, F)
        table = capi.mfcc_table(capi.MfccSpec.make(**d))
        if d["n_mels"] == 1:
            assert (table == 1.0).all() and got.tobytes() == E.tobytes()
        for r, L in ((1, Ls[0]), (0, Ls[1])):
            for t in range(ft.n_frames(L, 400, 160)):
                for j in range(d["n_ceps"]):
                    if d["use_energy"] and j == 0:
                        continue
                    v = np.float32(0.0)
                    for b in range(d["n_mels"]):
                        v = fma32(table[j, b], E[r, t, b], v)
                    assert v.view(np.uint32) == got[r, t, j].view(np.uint32), (change, r, t, j)


def test_zz_the_largest_ratio_of_this_file():
    """the figure README.md states comes from here (run with -s)"""
    assert WORST and max(WORST.values()) <= 1.0
    for key in sorted(WORST):
        print("largest error / bound  %-40s %.4f" % (key, WORST[key]))
