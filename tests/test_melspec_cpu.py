"""vpz_melspec_twiddles and vpz_melspec_filterbank (include/vorbispizza_pcm_melspec.h, csrc/melspec_tables.hpp) without a device, what a
clean checkout must hold about the new headers and bindings, and what tests/melspec_truth.py states: the truth's spectrum, the bound's
power to tell a right kernel from a wrong one, the check's cap on every GPU case's input, and the launch plan."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import melspec_truth as mt  # noqa: E402
import binding_support as cs  # noqa: E402
from f32_model import U, fma32  # noqa: E402
from logmel_truth import KINDS, check_log, check_power, dft64, frames_of, mel_weights64, refused_specs  # noqa: E402
from binding_support import imports_of  # noqa: E402

# (sample_rate, n_fft, n_mels, f_min, f_max, mel_scale, mel_norm)
BANKS = [(22050, 2048, 128, 0.0, 11025.0, "slaney", "slaney"), (44100, 4096, 128, 20.0, 20000.0, "htk", None), (48000, 8192, 256, 0.0, 24000.0, "htk", "slaney"),
         (44100, 2048, 1, 0.0, 22050.0, "slaney", "slaney"), (44100, 2048, 256, 0.0, 2000.0, "slaney", None)]
# and the bank of every case the GPU tests restate with the library's table
BANKS += sorted({mt.bank_of(c) for c in list(mt.CASES.values()) + list(mt.LIMIT_CASES.values())} - set(BANKS), key=repr)
ALL_CASES = list(mt.CASES) + list(mt.LIMIT_CASES)


def spec_of(bank, **kw):
    from vorbispizza_amd import capi
    sr, n_fft, n_mels, f_min, f_max, scale, norm = bank
    return capi.LogMelSpec.make(sample_rate=sr, n_fft=n_fft, hop=kw.pop("hop", n_fft // 4), n_mels=n_mels, f_min=f_min, f_max=f_max, mel_scale=scale,
                                mel_norm=norm, **kw)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


# ---- the tables
@pytest.mark.parametrize("n_fft", mt.NFFTS)
def test_the_twiddles_are_the_restatement_rounded_once(capi, n_fft):
    """One float32 rounding of the float64 value: |t - v| <= u |v|; on the axes the values are exact, bit for bit (no -0.0)"""
    w, t = capi.melspec_twiddles(n_fft)
    w64, t64 = mt.tables64(n_fft)
    assert w.shape == (n_fft,) and t.shape == (n_fft, 2) and w.dtype == t.dtype == np.float32
    assert (np.abs(w.astype(np.float64) - w64) <= U * np.abs(w64)).all()
    assert (np.abs(t.astype(np.float64) - t64) <= U * np.abs(t64)).all()
    q = n_fft // 4
    assert t[[0, q, 2 * q, 3 * q]].tolist() == [[1.0, 0.0], [0.0, -1.0], [-1.0, 0.0], [0.0, 1.0]]
    assert (t[[0, 2 * q], 1].view(np.uint32) == 0).all() and (t[[q, 3 * q], 0].view(np.uint32) == 0).all() and w[:1].view(np.uint32)[0] == 0 and w[2 * q] == 1.0
    # the restatement's own tables are these bits: network32 runs on what the kernel reads
    assert np.array_equal(w, w64.astype(np.float32)) and np.array_equal(t, t64.astype(np.float32))


@pytest.mark.parametrize("bank", BANKS)
def test_the_filterbank_is_the_restatement_rounded_once(capi, bank):
    first, count, weights = capi.melspec_filterbank(spec_of(bank))
    W = mel_weights64(*bank)
    assert first.shape == count.shape == (bank[2],) and weights.size == int(count.sum())
    at = 0
    for b in range(bank[2]):
        live = np.nonzero(W[b] > 0)[0]
        if live.size == 0:
            assert count[b] == 0 and first[b] == 0
            continue
        assert first[b] == live[0] and count[b] == live[-1] - live[0] + 1 == live.size
        want = W[b, live]
        got = weights[at: at + count[b]].astype(np.float64)
        assert (np.abs(got - want) <= U * want + 8 * 2.0 ** -52 * np.abs(W[b]).max() + 2.0 ** -149).all(), b
        at += count[b]
    if (bank[2] == 256 and bank[1] == 2048) or bank == mt.bank_of(mt.LIMIT_CASES["tile2_first_4096_3804"]):
        assert (count == 0).any() and (count > 0).any()  # (bands narrower than a bin: allowed)


def test_sizing_calls_and_capacities(capi):
    L = capi.lib()
    assert L.vpz_melspec_twiddles(2048, None, 0) == capi.OK
    buf = np.full(3 * 2048 + 1, 7.0, dtype=np.float32)
    assert L.vpz_melspec_twiddles(2048, buf.ctypes.data, 3 * 2048 - 1) == capi.E_CAPACITY and (buf == 7.0).all()
    assert L.vpz_melspec_twiddles(2048, buf.ctypes.data, 3 * 2048) == capi.OK and buf[-1] == 7.0 and buf[2048] == 1.0
    spec = spec_of(BANKS[0])
    total = C.c_int64(-1)
    assert L.vpz_melspec_filterbank(C.byref(spec), None, None, None, 0, C.byref(total)) == capi.OK and total.value > 128
    assert L.vpz_melspec_filterbank(C.byref(spec), None, None, None, 0, None) == capi.OK
    w = np.full(total.value + 1, 7.0, dtype=np.float32)
    assert L.vpz_melspec_filterbank(C.byref(spec), None, None, w.ctypes.data, total.value - 1, None) == capi.E_CAPACITY and (w == 7.0).all()
    assert L.vpz_melspec_filterbank(C.byref(spec), None, None, w.ctypes.data, total.value, None) == capi.OK and w[-1] == 7.0 and (w[:-1] > 0).all()


def test_every_limit_is_refused(capi):
    from melspec_truth import melspec_refused_specs
    L = capi.lib()
    for n_fft in (0, -2048, 1024, 2046, 2047, 2049, 3000, 6144, 8190, 16384):
        assert L.vpz_melspec_twiddles(n_fft, None, 0) == capi.E_INVALID_ARG, n_fft
        with pytest.raises(ValueError):
            capi.melspec_twiddles(n_fft)
    assert L.vpz_melspec_twiddles(2048, None, -1) == capi.E_INVALID_ARG
    for n_fft in mt.NFFTS:
        assert L.vpz_melspec_twiddles(n_fft, None, 0) == capi.OK
    total = C.c_int64(-5)
    specs = melspec_refused_specs(capi)
    assert {"n_fft 1024", "n_fft 2047", "n_fft 3000", "n_fft 16384", "hop < 1", "hop > n_fft", "n_mels < 1", "n_mels > 256", "f_min < 0", "f_min == f_max",
            "f_max > nyquist", "floor 0", "mel_scale", "layout", "a reserved word"} <= {what for what, _ in specs}
    assert [s.hop for what, s in specs if what in ("hop < 1", "hop > n_fft")] == [0, 2049]
    for what, spec in specs:
        assert L.vpz_melspec_filterbank(C.byref(spec), None, None, None, 0, C.byref(total)) == capi.E_INVALID_ARG, what
        with pytest.raises(ValueError):
            capi.melspec_filterbank(spec)
    assert total.value == -5
    assert L.vpz_melspec_filterbank(None, None, None, None, 0, None) == capi.E_INVALID_ARG
    good = capi.LogMelSpec.make(sample_rate=22050, n_fft=2048, hop=512, n_mels=128)
    assert L.vpz_melspec_filterbank(C.byref(good), None, None, None, -1, None) == capi.E_INVALID_ARG
    # at the limits themselves: accepted (a power spec does not look at its floor)
    for kw in (dict(n_fft=2048, hop=2048, n_mels=256), dict(n_fft=8192, hop=1, n_mels=1), dict(n_fft=8192, hop=8192), dict(n_fft=4096, f_min=11024.0),
               dict(log=False, floor=0.0)):
        capi.melspec_filterbank(capi.LogMelSpec.make(**dict(dict(sample_rate=22050, n_fft=2048, hop=512, n_mels=128), **kw)))


def test_the_older_stage_keeps_its_limits(capi):
    """vpz_mel_filterbank and vpz_logmel_dft_table still refuse n_fft = 2048, and the new helpers refuse every n_fft of theirs"""
    L = capi.lib()
    spec = spec_of(BANKS[0])
    assert L.vpz_mel_filterbank(C.byref(spec), None, None, None, 0, None) == capi.E_INVALID_ARG
    assert L.vpz_logmel_dft_table(2048, None, 0) == capi.E_INVALID_ARG
    with pytest.raises(ValueError):
        capi.mel_filterbank(spec)
    old = capi.LogMelSpec.make()
    assert L.vpz_mel_filterbank(C.byref(old), None, None, None, 0, None) == capi.OK
    assert L.vpz_melspec_filterbank(C.byref(old), None, None, None, 0, None) == capi.E_INVALID_ARG
    assert (capi.LOGMEL_MAX_NFFT, capi.MELSPEC_MIN_NFFT, capi.MELSPEC_MAX_NFFT, capi.MELSPEC_MAX_MELS) == (1024, 2048, 8192, 256)
    # every old refusal is still one
    for what, s in refused_specs(capi):
        assert L.vpz_mel_filterbank(C.byref(s), None, None, None, 0, None) == capi.E_INVALID_ARG, what


# ---- the truth
def test_the_truth_spectrum_is_the_dft_and_torch_stft():
    """numpy.fft.rfft of the windowed frames against test_logmel_cpu's dft64 at 2048 (the definition's sums), and against torch.stft in
    float64, center=True, reflect padding, on a row of the padded batch"""
    import torch
    rng = np.random.default_rng(5)
    X = rng.standard_normal((3, 2048)) * 0.5
    cos, sin = dft64(2048)
    re_, im_ = mt.spectrum64(X, 2048)
    assert np.abs(re_ - X @ cos).max() <= 1e-11 and np.abs(im_ - X @ sin).max() <= 1e-11
    for n_fft, hop, F, L in ((2048, 512, 7777, 6500), (4096, 441, 5000, 5000), (8192, 8192, 4097, 4000)):
        x = rng.standard_normal(L) * 0.5
        P, _ = mt.power_truth(frames_of(x, L, F, n_fft, hop), n_fft)
        row = np.zeros(F)
        row[:L] = x
        S = torch.stft(torch.from_numpy(row), n_fft, hop_length=hop, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64), center=True,
                       pad_mode="reflect", return_complex=True)
        want = (S.abs() ** 2).numpy().T
        assert want.shape == P.shape == (1 + F // hop, n_fft // 2 + 1)
        assert np.abs(P - want).max() <= 1e-12 * max(1.0, want.max())


def test_the_bound_is_the_headers_formula():
    text = open(os.path.join(cs.INC, "vorbispizza_pcm_melspec.h")).read()
    assert "K(n_fft) = sqrt(2) * (5 r4 + r2 + 2) + 7" in text and "45.2, 46.6, 52.3" in text
    assert [mt.passes(n) for n in mt.NFFTS] == [(5, 0), (5, 1), (6, 0)]
    assert [round(mt.K(n), 1) for n in mt.NFFTS] == [45.2, 46.6, 52.3]


@pytest.mark.parametrize("n_fft", mt.NFFTS)
def test_the_network_restated_is_the_dft(n_fft):
    """the header's network, step for step in float32 numpy, lies within the bound of the float64 spectrum -- on noise, a tone with noise
    and all-positive noise -- and far inside it (numpy's own float32 rfft reaches 0.52 u S)"""
    rng = np.random.default_rng(n_fft)
    m = np.arange(n_fft)
    X = np.stack([rng.standard_normal(n_fft) * 0.5, np.sin(2 * np.pi * 440.3 * m / 44100.0) * 0.4 + rng.standard_normal(n_fft) * 1e-3,
                  np.abs(rng.standard_normal(n_fft)) * 0.3]).astype(np.float32)
    re_, im_ = mt.network32(X, n_fft)
    r64, i64 = mt.spectrum64(X, n_fft)
    S = (np.abs(X.astype(np.float64)) @ mt.hann64(n_fft))[:, None]
    ratio = np.maximum(np.abs(re_ - r64), np.abs(im_ - i64)) / (U * S)
    print("network32 at %d: largest error %.3f u S, K = %.1f" % (n_fft, ratio.max(), mt.K(n_fft)))
    assert ratio.max() <= mt.K(n_fft) and ratio.max() <= 2.0


def test_every_case_stays_under_the_checks_cap():
    """check_log lets at most 1 % of values lie within e_M of the floor: a condition on the inputs, confirmed here with the truth alone
    (the truth handed to the check as the value: only the cap can fail)"""
    for name in ALL_CASES:
        for (M, e_M) in mt.case_truth(name):
            between = ~((M - e_M > mt.FLOOR) | (M + e_M < mt.FLOOR))
            assert between.sum() <= 0.01 * M.size, (name, int(between.sum()), M.size)
        src, rows = mt.case_input(name)
        assert (np.abs(src) >= 1e-3).all()


# ---- the bound discriminates
def proxy_rows(name, W, w=None, t=None, extend_repeats=False, hop_off=0):
    """the float32 network's M for every row of a case, with the named mistake"""
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = mt.case_of(name)
    src, rows = mt.case_input(name)
    out = []
    for a, L, _ in rows:
        x = src[a: a + L]
        if extend_repeats:  # a reflection that repeats the edge sample
            row = np.zeros(F)
            row[:L] = x
            h = n_fft // 2
            e = np.concatenate([row[:h][::-1], row, row[F - h:][::-1]])
            X = np.stack([e[t_ * hop: t_ * hop + n_fft] for t_ in range(1 + F // hop)])
        elif hop_off:
            e = mt.extend(x, L, F + n_fft, n_fft)  # (room for the longer stride; the first frames see the same samples)
            T = 1 + F // hop
            X = np.stack([e[t_ * (hop + hop_off): t_ * (hop + hop_off) + n_fft] for t_ in range(T)])
        else:
            X = frames_of(x, L, F, n_fft, hop)
        out.append(mt.proxy_mel(X.astype(np.float32), n_fft, W, w, t))
    return out


def passes_the_check(name, Ms):
    try:
        for got, (M, e_M) in zip(Ms, mt.case_truth(name)):
            check_power(got.astype(np.float32), M, e_M)
            check_log(np.log10(np.maximum(got, mt.FLOOR)).astype(np.float32), M, e_M, mt.FLOOR)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("name", ALL_CASES)
def test_the_restated_network_passes_on_every_case(name):
    assert passes_the_check(name, proxy_rows(name, mt.case_weights(name)))


@pytest.mark.parametrize("name", ["librosa_2048_512_T17", "half_4096_2048_T9", "odd_hop_2048_441"])
def test_the_bound_discriminates(name):
    """the same network fails the same check with any one of: one twiddle swapped for its neighbour (a twiddle of the last radix-4 pass
    that has any: a sixteenth of the bins carry it), the symmetric Hann window, a reflection that repeats the edge sample, a hop off by
    one"""
    n_fft = mt.CASES[name][1]
    W = mt.case_weights(name)
    w64, t64 = mt.tables64(n_fft)
    w, t = w64.astype(np.float32), t64.astype(np.float32)
    assert passes_the_check(name, proxy_rows(name, W, w, t))
    swapped = t.copy()
    k = 2 * (n_fft // 2 // 16)  # t[2 p s] at p = 1 of the pass with n = 16, s = H / 16
    swapped[[k, k + 1]] = swapped[[k + 1, k]]
    assert not passes_the_check(name, proxy_rows(name, W, w, swapped))
    symmetric = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / (n_fft - 1))).astype(np.float32)
    assert not passes_the_check(name, proxy_rows(name, W, symmetric, t))
    assert not passes_the_check(name, proxy_rows(name, W, w, t, extend_repeats=True))
    assert not passes_the_check(name, proxy_rows(name, W, w, t, hop_off=1))


# ---- the launch plan
def test_the_launch_plan_fits_and_the_cases_take_their_tiles():
    """csrc/pcm_melspec.hip's constants, restated: at every (n_fft, hop) inside the limits a tile fits the 160 KiB (VPZ_E_UNSUPPORTED cannot
    be reached), no staging or frame index leaves the span, the arrays of a workgroup do not overlap, and every case of
    tests/test_pcm_melspec_gpu.py takes the tile it is meant to"""
    k = mt.kernel_constants()
    assert (k["kMsBlock"], k["kMsLdsFloats"], k["kMsMaxGridY"], k["kMsMelRoom"]) == (256, 40960, 2048, 256)
    tiles = (k["kMsTileA"], k["kMsTileB"], k["kMsTileC"])
    assert tiles == (16, 8, 2)
    most = 0
    for n_fft in mt.NFFTS:
        hop = np.arange(1, n_fft + 1, dtype=np.int64)
        fits = [2 * n_fft + (Tt - 1) * hop + n_fft + Tt * k["kMsMelRoom"] <= k["kMsLdsFloats"] for Tt in tiles]
        assert fits[2].all(), n_fft
        chosen = np.where(fits[0], tiles[0], np.where(fits[1], tiles[1], tiles[2]))
        for h in (1, 2, 441, 512, 819, 820, 1638, 1639, 2048, 3803, 3804, n_fft - 1, n_fft):
            if h <= n_fft:
                Tt, floats = mt.tile_plan(n_fft, h, k)
                assert Tt == chosen[h - 1] and floats <= k["kMsLdsFloats"]
                most = max(most, floats)
                span_cap = (Tt - 1) * h + n_fft
                # the staging writes span[0 .. count), count <= span_cap; frame f reads span[f hop + m], m < n_fft
                assert (Tt - 1) * h + n_fft - 1 < span_cap
                # the arrays: two complex arrays [0, 2 n_fft), the span behind them, the mel tile behind that
                assert floats == 2 * n_fft + span_cap + Tt * k["kMsMelRoom"]
    assert most == 40960  # (n_fft 2048 at hop 2048 with 16 frames and n_fft 8192 at hop 2048 with 8: the whole budget, not a float more)
    assert [max(h for h in range(1, n + 1) if mt.tile_plan(n, h, k)[0] == 16) for n in mt.NFFTS] == [2048, 1638, 819]
    assert [max(h for h in range(1, n + 1) if mt.tile_plan(n, h, k)[0] >= 8) for n in mt.NFFTS] == [2048, 3803, 2048]
    assert mt.tile_plan(8192, 8192, k) == (2, 33280)
    for name, case in mt.CASES.items():
        sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = case
        assert mt.tile_plan(n_fft, hop, k)[0] == tile and F >= n_fft // 2 + 1 and n_mels <= k["kMsMelRoom"], name
    # a T one less than, equal to and one more than each tile size
    Ts = {tile: {1 + c[8] // c[2] for c in mt.CASES.values() if c[9] == tile} for tile in tiles}
    assert all({tile - 1, tile, tile + 1} <= Ts[tile] for tile in tiles), Ts
    # the smallest padded length at every n_fft, with one frame and with hop 1
    assert {(c[1], c[2]) for c in mt.CASES.values() if c[8] == c[1] // 2 + 1} == {(n, h) for n in mt.NFFTS for h in (1, n)}


# what tests/test_pcm_melspec_limits_gpu.py launches: name -> (frames of the tile, LDS floats, T)
LIMIT_PLAN = {"tile16_last_4096_1638": (16, 40954, 17), "tile8_first_4096_1639": (8, 25809, 9), "tile8_last_4096_3803": (8, 40957, 9),
              "tile2_first_4096_3804": (2, 16604, 3), "tile16_last_8192_819": (16, 40957, 17), "tile8_first_8192_820": (8, 32364, 9),
              "full_lds_8192_2048_T7": (8, 40960, 7), "full_lds_8192_2048_T8": (8, 40960, 8), "full_lds_8192_2048_T9": (8, 40960, 9),
              "tile2_first_8192_2049": (2, 27137, 3)}


def test_the_limit_cases_take_their_tiles_and_the_banks_every_trip_of_the_band_loop(capi):
    """LIMIT_CASES against the plan: every case takes the tile it is named for with the LDS floats of the table above -- the last hop of
    a tile size, and the first of the next, at n_fft 4096 and 8192; the whole 160 KiB at 8192 and three floats less at 4096 -- and the
    library's banks of CASES and LIMIT_CASES together give the band loop (kMsAhead = 16 steps issued together, a step beyond the band
    reading its last bin again) every count around its trips"""
    k = mt.kernel_constants()
    assert sorted(mt.LIMIT_CASES) == sorted(LIMIT_PLAN)
    for name, case in mt.LIMIT_CASES.items():
        sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = case
        assert mt.tile_plan(n_fft, hop, k) == LIMIT_PLAN[name][:2] and tile == LIMIT_PLAN[name][0] and 1 + F // hop == LIMIT_PLAN[name][2], name
        assert F >= n_fft // 2 + 1 and F % hop == 5 and n_mels <= k["kMsMelRoom"], name
        assert name.split("_")[0] in ("tile%d" % tile, "full") and "_%d_%d" % (n_fft, hop) in name
    # either side of every change of tile
    for n_fft, last16, last8 in ((4096, 1638, 3803), (8192, 819, 2048)):
        hops = {c[2]: c[9] for c in mt.LIMIT_CASES.values() if c[1] == n_fft}
        assert (hops[last16], hops[last16 + 1], hops[last8], hops[last8 + 1]) == (16, 8, 8, 2)
        assert mt.tile_plan(n_fft, last16 + 1, k)[0] == 8 and mt.tile_plan(n_fft, last8 + 1, k)[0] == 2
    floats = {(c[1], mt.tile_plan(c[1], c[2], k)[1]) for c in mt.LIMIT_CASES.values()}
    assert (8192, 40960) in floats and (4096, 40957) in floats and k["kMsLdsFloats"] == 40960
    # a T one less than, equal to and one more than the tile at the full LDS
    assert {1 + c[8] // c[2] for n, c in mt.LIMIT_CASES.items() if n.startswith("full_lds")} == {7, 8, 9}
    # the banks: both scales, both norms, bin n_fft / 2 live, empty bands, 256 bands where an 8192 launch asks for the most
    cases = mt.LIMIT_CASES.values()
    assert {c[6] for c in cases} == {"htk", "slaney"} and {c[7] for c in cases} == {None, "slaney"} and any(c[5] is None for c in cases)
    most = sorted((mt.tile_plan(c[1], c[2], k)[1], n) for n, c in mt.LIMIT_CASES.items() if c[1] == 8192)[-2:]
    assert all(mt.LIMIT_CASES[n][3] == 256 and mt.LIMIT_CASES[n][5] is None and mt.LIMIT_CASES[n][6] == "htk" and mt.LIMIT_CASES[n][0] == 48000 for _, n in most)
    counts, top_live = set(), set()
    for name in ALL_CASES:
        first, count, weights = capi.melspec_filterbank(mt.case_spec(name))
        counts |= set(count.tolist())
        if mt.case_of(name)[5] is None:
            # f_max at Nyquist: the last band's triangle ends on bin n_fft / 2, where its weight is 0 or what the rounding of the mel
            # points leaves of it -- the bin is live in some banks only
            half = mt.case_of(name)[1] // 2
            assert (first + count).max() in (half, half + 1), name
            if (first + count).max() == half + 1 and name in mt.LIMIT_CASES:
                top_live.add(name)
    assert {"tile16_last_4096_1638", "tile8_last_4096_3803"} <= top_live  # (the kernel reads P[n_fft / 2], which the split pass writes twice)
    assert k["kMsAhead"] == 16
    assert {0, 1, 15, 16, 17, 31, 32, 33} <= counts and max(counts) > 256, sorted(counts)
    first, count, weights = capi.melspec_filterbank(mt.case_spec("tile2_first_4096_3804"))
    assert (count == 0).any() and (count > 0).any()


def test_the_bit_check_tells_what_the_bound_does_not(capi):
    """On a row of LIMIT_CASES: one band's chain summed k descending, and P = re * re + im * im with two roundings, both pass check_power
    against the float64 truth -- at a fraction of the bound -- and both differ from restated_power32 in bits"""
    name = "full_lds_8192_2048_T9"
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = mt.LIMIT_CASES[name]
    src, rows = mt.case_input(name)
    (a, L, _), (M, e_M) = rows[0], mt.case_truth(name)[0]
    assert L == F
    first, count, weights = capi.melspec_filterbank(mt.case_spec(name))
    first, count = first.astype(np.int64), count.astype(np.int64)
    X = frames_of(src[a: a + L], L, F, n_fft, hop).astype(np.float32)
    want = mt.restated_power32(X, n_fft, first, count, weights)
    assert check_power(want, M, e_M) < 1.0
    # one band, k descending
    P = mt.power32(X, n_fft)
    b = int(np.argmax(count))
    start = int(count[:b].sum())
    assert count[b] > 2 * 16
    acc = np.zeros(X.shape[0], dtype=np.float32)
    for i in range(int(count[b]) - 1, -1, -1):
        acc = fma32(weights[start + i], P[:, first[b] + i], acc)
    other = want.copy()
    other[:, b] = acc
    ratio = check_power(other, M, e_M)
    differ = int((other.view(np.uint32) != want.view(np.uint32)).sum())
    print("one chain descending: error / bound %.4f, %d of %d values of the band differ in bits" % (ratio, differ, X.shape[0]))
    assert ratio < 1.0 and differ > 0
    # the power unfused
    re_, im_ = mt.network32(X, n_fft)
    other = mt.band_sums32(re_ * re_ + im_ * im_, first, count, weights)
    ratio = check_power(other, M, e_M)
    differ = int((other.view(np.uint32) != want.view(np.uint32)).sum())
    print("the power unfused: error / bound %.4f, %d of %d values differ in bits" % (ratio, differ, other.size))
    assert ratio < 1.0 and differ > 0


def test_check_log_exact_has_no_exempt_share():
    """the silence value's bits at and under float32(floor), 4 u max(1, |got|) above it, and nothing else"""
    floor = 0.25 * (1 + 2.0 ** -30)  # (float32 rounds it to 0.25)
    acc = np.array([0.0, 0.25, np.nextafter(np.float32(0.25), np.float32(1)), 3.0, 1e-30], dtype=np.float32)
    silence = mt.silence_value(floor)
    good = np.where(acc <= np.float32(0.25), silence, np.log10(np.maximum(acc.astype(np.float64), 1e-300))).astype(np.float32)
    assert silence == np.float32(np.log10(0.25)) and (good[[0, 1, 4]] == silence).all() and good[2] != silence
    assert mt.check_log_exact(good, acc, floor) <= 0.125  # (a correctly rounded log10: half a unit of 4)
    up = np.float32(np.inf)
    # one float32 off the silence value at, and under, the floor; the logarithm of a value under it; five units off a logarithm; a NaN
    for at, value in ((0, np.nextafter(silence, up)), (1, np.nextafter(silence, -up)), (4, np.float32(-30.0)),
                      (3, good[3] + np.float32(5 * 2.0 ** -24)), (3, np.float32("nan"))):
        bad = good.copy()
        bad[at] = value
        with pytest.raises(AssertionError):
            mt.check_log_exact(bad, acc, floor)


# ---- the surface
def test_the_melspec_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_melspec.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmMelspec.cs")
    assert sorted(c) == ["vpz_melspec_filterbank", "vpz_melspec_twiddles", "vpz_pcm_melspec"] == sorted(imports) == sorted(capi.PCM_MELSPEC_EXPORTED_SYMBOLS)
    old = cs.c_functions("vorbispizza_pcm_logmel.h", "vpz_")
    assert c["vpz_pcm_melspec"] == old["vpz_pcm_logmel"] and c["vpz_melspec_filterbank"] == old["vpz_mel_filterbank"]
    assert c["vpz_melspec_twiddles"] == ("i32", ["i32", "ptr", "i64"])
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_MELSPEC_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    # the spec is vpz_logmel_spec: the header declares no struct of its own, and both bindings pass the older one
    structs, defines = cs.c_structs("vorbispizza_pcm_melspec.h")
    assert structs == {} and "vpz_logmel_spec" in open(os.path.join(cs.INC, "vorbispizza_pcm_melspec.h")).read()
    text = cs.strip_cs_comments(open(os.path.join(cs.CS, "GpuPcmMelspec.cs")).read())
    assert text.count("GpuPcmLogMel.LogMelSpec* spec") == 2 and "struct" not in text
    assert dict((n, a) for n, _, a in capi._PCM_MELSPEC_SIGNATURES)["vpz_pcm_melspec"][4] == C.POINTER(capi.LogMelSpec)
    consts = {}
    for m in re.finditer(r"public\s+const\s+int\s+([^;]+);", text):
        for part in m.group(1).split(","):
            key, v = part.split("=")
            consts[cs.norm(key.strip())] = int(v.strip(), 0)
    seen = 0
    for name, value in defines.items():
        if name.startswith("VPZ_MELSPEC_"):
            assert consts[cs.norm(name[4:])] == value == getattr(capi, name[4:]), name
            seen += 1
    assert seen == 3
    # the older headers and their lists did not take the new names
    for name in c:
        assert name not in capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_LOGMEL_EXPORTED_SYMBOLS
        assert name not in cs.c_functions("vorbispizza_synth.h", "vpz_") and name not in old


def test_the_melspec_call_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_melspec.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiMelspec.cs")
    assert sorted(c) == ["vpzm_decode_ranges_melspec"] == sorted(imports) == sorted(multi.MELSPEC_EXPORTED_SYMBOLS)
    # the same signature as the log-mel call
    assert c["vpzm_decode_ranges_melspec"] == cs.c_functions("vorbispizza_multi_logmel.h", "vpzm_")["vpzm_decode_ranges_logmel"]
    assert imports["vpzm_decode_ranges_melspec"] == ("Host",) + c["vpzm_decode_ranges_melspec"]
    fn = multi.lib().vpzm_decode_ranges_melspec
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_decode_ranges_melspec"][1] and KINDS[fn.restype] == "i32"
    assert cs.c_structs("vorbispizza_multi_melspec.h")[0] == {}
    assert sorted(multi.LOGMEL_EXPORTED_SYMBOLS) == ["vpzm_decode_ranges_logmel"]
    sig = inspect.signature(multi.Dispatcher.decode_ranges_melspec)
    old = inspect.signature(multi.Dispatcher.decode_ranges_logmel)
    assert list(sig.parameters) == list(old.parameters) == ["self", "datas", "ranges", "frames", "sample_rate", "n_fft", "hop", "n_mels", "f_min", "f_max", "mel_scale",
                                                            "mel_norm", "log", "floor", "bands_first", "out"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["sample_rate"], d["n_fft"], d["hop"], d["n_mels"], d["f_min"], d["f_max"], d["mel_scale"], d["mel_norm"], d["log"], d["floor"],
            d["bands_first"], d["out"]) == (22050, 2048, 512, 128, 0.0, None, "slaney", "slaney", True, 1e-10, True, None)
    assert (old.parameters["sample_rate"].default, old.parameters["n_fft"].default, old.parameters["hop"].default, old.parameters["n_mels"].default) == (16000, 400, 160, 80)


def test_both_libraries_export_the_new_symbols(capi):
    from vorbispizza_amd import _build, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in capi.PCM_MELSPEC_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert hasattr(H, "vpzm_decode_ranges_melspec") and not hasattr(S, "vpzm_decode_ranges_melspec")
    assert "pcm_melspec.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "melspec_tables.hpp"))
    assert callable(capi.pcm_melspec) and callable(capi.melspec_twiddles) and callable(capi.melspec_filterbank) and callable(multi.Dispatcher.decode_ranges_melspec)


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    for header, body in (("vorbispizza_pcm_melspec.h", "sizeof(vpz_logmel_spec) == 96 && VPZ_MELSPEC_MIN_NFFT == 2048 && VPZ_MELSPEC_MAX_NFFT == 8192 && VPZ_LOGMEL_MAX_NFFT == 1024"),
                         ("vorbispizza_multi_melspec.h", "VPZM_E_RATE == -16 && VPZ_MEL_LOG10 == 1 && VPZ_MELSPEC_MAX_MELS == 256")):
        src = tmp_path / (header + ".c")
        src.write_text('#include "%s"\ntypedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % (header, body))
        exe = tmp_path / (header + ".exe")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


def test_the_melspec_kernels_use_no_scratch_and_say_what_they_take():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = [k for k in kr.analyse(os.path.join(_build.CSRC, "pcm_melspec.hip"), _build.SOURCES["pcm_melspec.hip"]) if "pcm_melspec_kernel" in k["name"]]
    assert len(ks) == 3  # <n_fft 2048, 4096, 8192>
    for k in ks:
        assert k["scratch"] == 0 and k.get("vgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 512 and k["occupancy"] >= 1, k  # (a lane keeps its window values and twiddles in registers)
