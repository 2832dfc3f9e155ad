"""vpz_stft_table (include/vorbispizza_pcm_stft.h, csrc/stft_tables.hpp) without a device, what a clean checkout must hold about the new
headers and bindings, and what tests/stft_truth.py states: the truth against torch.stft, the restated network against the truth on every
GPU case and for all three outputs, what the checks can tell apart, and the launch plan."""
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

import stft_truth as st  # noqa: E402
import binding_support as cs  # noqa: E402
from f32_model import U  # noqa: E402
from logmel_truth import KINDS, frames_of  # noqa: E402
from binding_support import imports_of  # noqa: E402
from stft_truth import stft_refused_specs  # noqa: E402

# (n_fft, win_length, window): centring with an even and an odd remainder, both windows, the limits of win_length
TABLES = [(512, 512, "hann"), (512, 400, "hamming"), (512, 511, "hann"), (512, 2, "hann"), (1024, 1024, "hamming"), (1024, 1001, "hann"), (2048, 2048, "hann"),
          (4096, 4096, "hann"), (4096, 3000, "hamming"), (8192, 8192, "hann"), (8192, 3, "hamming")]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


# ---- the table
@pytest.mark.parametrize("n_fft,win_length,window", TABLES)
def test_the_table_is_the_restatement_rounded_once(capi, n_fft, win_length, window):
    """One float32 rounding of the float64 value; zeros outside the centred window; the twiddles are vpz_melspec_twiddles' bit for bit
    where both stages take the size"""
    w, t = capi.stft_table(n_fft, win_length, window)
    w64, t64 = st.window64(n_fft, win_length, window), st.tables64(n_fft)[1]
    assert w.shape == (n_fft,) and t.shape == (n_fft, 2) and w.dtype == t.dtype == np.float32
    assert (np.abs(w.astype(np.float64) - w64) <= U * np.abs(w64)).all() and (np.abs(t.astype(np.float64) - t64) <= U * np.abs(t64)).all()
    left = (n_fft - win_length) // 2
    assert (w[:left].view(np.uint32) == 0).all() and (w[left + win_length:].view(np.uint32) == 0).all() and (w[left + 1: left + win_length] > 0).all()
    assert w[left] == (np.float32(0.08) if window == "hamming" else 0.0)
    q = n_fft // 4
    assert t[[0, q, 2 * q, 3 * q]].tolist() == [[1.0, 0.0], [0.0, -1.0], [-1.0, 0.0], [0.0, 1.0]]
    assert (t[[0, 2 * q], 1].view(np.uint32) == 0).all() and (t[[q, 3 * q], 0].view(np.uint32) == 0).all()
    # the restatement's own tables are these bits: network32 runs on what the kernel reads
    w32, t32 = st.tables32(n_fft, win_length, window)
    assert np.array_equal(w, w32) and np.array_equal(t, t32)
    if n_fft >= 2048:
        assert np.array_equal(t, capi.melspec_twiddles(n_fft)[1])
        if win_length == n_fft and window == "hann":
            assert np.array_equal(w, capi.melspec_twiddles(n_fft)[0])


@pytest.mark.parametrize("n_fft", [2048, 4096, 8192])
def test_the_mel_stage_reads_the_same_table(capi, n_fft):
    """vpz_melspec_twiddles is vpz_stft_table with hann over the whole transform, bit for bit, window and twiddles: the two kernels'
    networks read one table (csrc/melspec_tables.hpp's twiddle_fill fills both)"""
    (w_mel, t_mel), (w_stft, t_stft) = capi.melspec_twiddles(n_fft), capi.stft_table(n_fft, n_fft, "hann")
    assert w_mel.dtype == w_stft.dtype == t_mel.dtype == t_stft.dtype == np.float32 and w_mel.shape == (n_fft,) and t_mel.shape == (n_fft, 2)
    assert np.array_equal(w_mel.view(np.uint32), w_stft.view(np.uint32)) and np.array_equal(t_mel.view(np.uint32), t_stft.view(np.uint32))


def test_the_windows_are_torchs():
    import torch
    for n_fft, win_length, window in TABLES:
        g = (torch.hamming_window if window == "hamming" else torch.hann_window)(win_length, periodic=True, dtype=torch.float64).numpy()
        left = (n_fft - win_length) // 2
        assert np.abs(st.window64(n_fft, win_length, window)[left: left + win_length] - g).max() <= 1e-15


def test_sizing_calls_and_capacities(capi):
    L = capi.lib()
    assert L.vpz_stft_table(512, 400, capi.STFT_HAMMING, None, 0) == capi.OK
    buf = np.full(3 * 512 + 1, 7.0, dtype=np.float32)
    assert L.vpz_stft_table(512, 512, capi.STFT_HANN, buf.ctypes.data, 3 * 512 - 1) == capi.E_CAPACITY and (buf == 7.0).all()
    assert L.vpz_stft_table(512, 512, capi.STFT_HANN, buf.ctypes.data, 3 * 512) == capi.OK and buf[-1] == 7.0 and buf[256] == 1.0 and buf[512] == 1.0
    assert L.vpz_stft_table(512, 512, capi.STFT_HANN, buf.ctypes.data, 1 << 40) == capi.OK and buf[-1] == 7.0


def test_every_limit_is_refused(capi):
    L = capi.lib()
    for n_fft in (0, -512, 256, 400, 510, 511, 513, 768, 3000, 6144, 8190, 16384):
        assert L.vpz_stft_table(n_fft, 2, 0, None, 0) == capi.E_INVALID_ARG, n_fft
        with pytest.raises(ValueError):
            capi.stft_table(n_fft, 2)
    for wl in (-1, 0, 1, 513, 1 << 20):
        assert L.vpz_stft_table(512, wl, 0, None, 0) == capi.E_INVALID_ARG, wl
    for window in (-1, 2, 7):
        assert L.vpz_stft_table(512, 512, window, None, 0) == capi.E_INVALID_ARG, window
    assert L.vpz_stft_table(512, 512, 0, None, -1) == capi.E_INVALID_ARG
    with pytest.raises(ValueError):
        capi.StftSpec.make(window="povey")
    with pytest.raises(ValueError):
        capi.StftSpec.make(output="log")
    # at the limits themselves: accepted
    for n_fft in st.NFFTS:
        for wl in (2, n_fft):
            for window in (0, 1):
                assert L.vpz_stft_table(n_fft, wl, window, None, 0) == capi.OK
    specs = stft_refused_specs(capi)
    assert {"n_fft 256", "n_fft 400", "n_fft 16384", "hop < 1", "hop > n_fft", "win_length < 2", "win_length > n_fft", "window 2", "output 3", "layout 2",
            "a reserved word"} <= {what for what, _ in specs}
    assert [s.hop for what, s in specs if what in ("hop < 1", "hop > n_fft")] == [0, 2049]
    # (vpz_pcm_stft refuses them in front of every device call: tests/test_pcm_stft_gpu.py; the dispatcher's call without a dispatcher is
    # refused for that alone, so its spec check is the GPU tests' too)


def test_the_older_stages_do_not_change(capi):
    L = capi.lib()
    assert L.vpz_melspec_twiddles(512, None, 0) == capi.E_INVALID_ARG and L.vpz_melspec_twiddles(1024, None, 0) == capi.E_INVALID_ARG
    assert (capi.STFT_MIN_NFFT, capi.STFT_MAX_NFFT, capi.MELSPEC_MIN_NFFT, capi.LOGMEL_MAX_NFFT) == (512, 8192, 2048, 1024)


# ---- the truth
def test_the_truth_is_torch_stft():
    """windowed frames through numpy.fft.rfft against torch.stft in float64, center=True, reflect padding, on a row of the padded batch:
    centring with odd and even win_length, both windows, every size"""
    import torch
    rng = np.random.default_rng(5)
    for (n_fft, win_length, window), hop, F, L in zip(TABLES, (128, 160, 128, 1, 256, 333, 441, 1024, 4096, 8192, 2000),
                                                      (3000, 1607, 1155, 257, 5000, 2222, 7777, 5000, 9000, 4097, 9000),
                                                      (2500, 1607, 1100, 200, 4999, 2222, 6500, 5000, 2049, 4000, 8999)):
        x = rng.standard_normal(L) * 0.5
        Z = st.spectrum64(frames_of(x, L, F, n_fft, hop), st.window64(n_fft, win_length, window))
        row = np.zeros(F)
        row[:L] = x
        g = (torch.hamming_window if window == "hamming" else torch.hann_window)(win_length, periodic=True, dtype=torch.float64)
        S = torch.stft(torch.from_numpy(row), n_fft, hop_length=hop, win_length=win_length, window=g, center=True, pad_mode="reflect", normalized=False,
                       onesided=True, return_complex=True).numpy().T
        assert S.shape == Z.shape == (1 + F // hop, n_fft // 2 + 1)
        assert np.abs(Z - S).max() <= 1e-12 * max(1.0, np.abs(S).max()), (n_fft, win_length, window)


def test_the_bounds_are_the_headers_formulas():
    text = open(os.path.join(cs.INC, "vorbispizza_pcm_stft.h")).read()
    assert "K(n_fft) = sqrt(2) * (5 r4 + r2 + 2) + 7" in text and "38.1, 39.5, 45.2, 46.6, 52.3" in text
    assert "e_P = 2 |re| d + 2 |im| d + 2 d^2 + 3u P" in text and "e = sqrt(2) d + 3u |X|" in text
    assert [st.passes(n) for n in st.NFFTS] == [(4, 0), (4, 1), (5, 0), (5, 1), (6, 0)]
    assert [round(st.K(n), 1) for n in st.NFFTS] == [38.1, 39.5, 45.2, 46.6, 52.3]


def test_the_exact_fma_is_exact():
    """a sum the float64 rounding would carry to a float32 midpoint: 1 + 2^-24 + 2^-60 rounds up, 1 + 2^-24 - 2^-60 down"""
    one, tiny = np.array([1.0], np.float32), np.array([2.0 ** -30], np.float32)
    assert st._fma(tiny, tiny, one + np.float32(0))[0] == 1.0
    a, b = np.array([2.0 ** -12 + 2.0 ** -35], np.float32), np.array([2.0 ** -12], np.float32)  # a b = 2^-24 + 2^-47
    assert st._fma(a, b, one)[0] == np.float32(1.0 + 2.0 ** -23) and st._fma(a, -b, -one)[0] == -np.float32(1.0 + 2.0 ** -23)
    a = np.array([2.0 ** -12 - 2.0 ** -35], np.float32)
    assert st._fma(a, b, one)[0] == 1.0
    # in float64 the three sums are one value: a plain float64 sum cannot tell them apart
    assert (2.0 ** -24 + 2.0 ** -60) + 1.0 == 1.0 + 2.0 ** -24


@pytest.mark.parametrize("n_fft,win_length,window", [(512, 512, "hann"), (512, 400, "hamming"), (1024, 1024, "hann"), (1024, 1001, "hamming"), (2048, 2048, "hann"),
                                                     (4096, 3000, "hamming"), (8192, 8192, "hann")])
def test_the_network_restated_is_the_dft(n_fft, win_length, window):
    """the header's network over a window table, step for step in float32 numpy, lies within the bound of the float64 spectrum -- on noise,
    a tone with noise and all-positive noise -- and far inside it, for all three outputs"""
    rng = np.random.default_rng(n_fft + win_length)
    m = np.arange(n_fft)
    X = np.stack([rng.standard_normal(n_fft) * 0.5, np.sin(2 * np.pi * 440.3 * m / 44100.0) * 0.4 + rng.standard_normal(n_fft) * 1e-3,
                  np.abs(rng.standard_normal(n_fft)) * 0.3]).astype(np.float32)
    w, t = st.tables32(n_fft, win_length, window)
    out = st.outputs32(*st.network32(X, n_fft, w, t))
    Z, d = st.truth(X.astype(np.float64), n_fft, st.window64(n_fft, win_length, window))
    ratios = {o: st.check_output(o, out[o], Z, d) for o in st.OUTPUTS}
    print("network32 at %d / %d %s: largest error / bound %s, K = %.1f" % (n_fft, win_length, window, ratios, st.K(n_fft)))
    assert max(ratios.values()) <= 0.1


@pytest.mark.parametrize("name", list(st.CASES))
def test_the_restated_network_stays_inside_the_bound_on_every_case(name):
    worst = 0.0
    for out, (Z, d) in zip(st.case_restated(name), st.case_truth(name)):
        for o in st.OUTPUTS:
            worst = max(worst, st.check_output(o, out[o], Z, d))
    assert worst < 0.25, worst
    src, rows = st.case_input(name)
    n_fft, hop, win_length, window, F, tc, tr = st.CASES[name]
    assert [L for _, L, _ in rows] == [F, F - 1, F - n_fft // 4, F // 3, 1, 0] and len({r for _, _, r in rows}) == 6 and F >= n_fft // 2 + 1


# ---- what the checks tell apart
def passes_the_bound(out, Z, d):
    try:
        for o in st.OUTPUTS:
            st.check_output(o, out[o], Z, d)
    except AssertionError:
        return False
    return True


def same_values(a, b):
    return all(np.array_equal(a[o], b[o]) for o in ("complex", "power"))


def off_by(t, k, part, ulps):
    out = t.copy()
    out[k, part] = (out[k:k + 1, part].view(np.int32) + ulps).view(np.float32)[0]
    return out


@pytest.mark.parametrize("n_fft", [512, 1024, 4096])
def test_the_checks_discriminate(n_fft):
    """The GPU check of a COMPLEX or POWER row is two-fold: inside the bound of the truth, and the restatement's values.
    One twiddle of the table off by a few ulps -- 3 ulps on t[k] of the split pass -- fails it: the values differ.  The bound alone cannot
    see 3 ulps, and no bound of this form could: a twiddle off by the relative amount r moves an output by at most r S, and K u S is 38 u S
    and more -- the bound starts to see a twiddle at some 40 ulps.  It does see that: on an impulse at an odd sample, where |O[k]| = S,
    t[k] off by 64 ulps leaves the bound at bin k; and it sees every gross mistake -- a twiddle swapped for its neighbour, the symmetric
    window, the hop off by one."""
    H, hop = n_fft // 2, n_fft // 4
    rng = np.random.default_rng(n_fft)
    F = 6 * hop + 3
    x = (rng.standard_normal(F) * 0.25).astype(np.float32)
    X = frames_of(x, F, F, n_fft, hop)
    w, t = st.tables32(n_fft)
    w64 = st.window64(n_fft)
    Z, d = st.truth(X, n_fft, w64)
    right = st.outputs32(*st.network32(X.astype(np.float32), n_fft, w, t))
    assert passes_the_bound(right, Z, d)
    k = H // 2 - 3
    few = st.outputs32(*st.network32(X.astype(np.float32), n_fft, w, off_by(t, k, 1, 3)))
    assert not same_values(few, right) and passes_the_bound(few, Z, d)
    assert (few["complex"][:, [k, H - k]] != right["complex"][:, [k, H - k]]).any() and np.array_equal(np.delete(few["complex"], [k, H - k], axis=1),
                                                                                                    np.delete(right["complex"], [k, H - k], axis=1))
    # the impulse: y[m0] = w[m0] at an odd m0 next to the window's peak -- E = 0, |O[k]| = S
    imp = np.zeros((1, n_fft), dtype=np.float32)
    imp[0, H + 1] = 1.0
    Zi, di = st.truth(imp.astype(np.float64), n_fft, w64)
    assert passes_the_bound(st.outputs32(*st.network32(imp, n_fft, w, t)), Zi, di)
    part = 0 if abs(t[k, 0]) > abs(t[k, 1]) else 1  # (the larger component, in [0.5, 1): an ulp of it is u)
    assert 0.5 <= abs(t[k, part]) < 1.0
    assert passes_the_bound(st.outputs32(*st.network32(imp, n_fft, w, off_by(t, k, part, 3))), Zi, di)
    assert not passes_the_bound(st.outputs32(*st.network32(imp, n_fft, w, off_by(t, k, part, 64))), Zi, di)
    # gross mistakes, on the noise
    swapped = t.copy()
    kk = 2 * (H // 16)  # t[2 p s] at p = 1 of the pass with n = 16, s = H / 16
    swapped[[kk, kk + 1]] = swapped[[kk + 1, kk]]
    assert not passes_the_bound(st.outputs32(*st.network32(X.astype(np.float32), n_fft, w, swapped)), Z, d)
    symmetric = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / (n_fft - 1))).astype(np.float32)
    assert not passes_the_bound(st.outputs32(*st.network32(X.astype(np.float32), n_fft, symmetric, t)), Z, d)
    e = st.extend(x, F, F + n_fft, n_fft)
    Xoff = np.stack([e[i * (hop + 1): i * (hop + 1) + n_fft] for i in range(X.shape[0])])
    assert not passes_the_bound(st.outputs32(*st.network32(Xoff.astype(np.float32), n_fft, w, t)), Z, d)
    # the sign of Im is the definition's (torch's), not the mel stage's
    conj = {o: (v.conj() if o == "complex" else v) for o, v in right.items()}
    assert not passes_the_bound(conj, Z, d)


# ---- the launch plan
def test_the_launch_plan_fits_and_the_cases_take_their_tiles():
    """csrc/pcm_stft.hip's constants, restated: the lanes-per-frame rule; at every spec inside the limits a tile fits the 160 KiB
    (VPZ_E_UNSUPPORTED cannot be reached); the arrays of a workgroup do not overlap; and every case of tests/test_pcm_stft_gpu.py takes the
    bins-first tiles it names"""
    from melspec_truth import kernel_constants as melspec_constants
    k = st.kernel_constants()
    assert (k["kStBlock"], k["kStLdsFloats"], k["kStMaxGridY"], k["kStMaxTile"]) == (256, 40960, 2048, 32)
    assert k["kStLdsFloats"] == melspec_constants()["kMsLdsFloats"]  # (the budget the project already has)
    assert [st.lanes_per_frame(n, k) for n in st.NFFTS] == [64, 128, 256, 256, 256] and [st.side_by_side(n, k) for n in st.NFFTS] == [4, 2, 1, 1, 1]
    text = open(os.path.join(ROOT, "vorbispizza_amd", "csrc", "pcm_stft.hip")).read()
    assert "kLanes = Q < kStBlock ? Q : kStBlock" in text and "G = kStBlock / kLanes" in text and "Q = H / 4" in text
    most = {}
    for n_fft in st.NFFTS:
        G = st.side_by_side(n_fft, k)
        hop = np.arange(1, n_fft + 1, dtype=np.int64)
        for output in ("complex", "power"):
            for bins_first in (True, False):
                c = (2 if output == "complex" else 1) if bins_first else 0
                chosen = np.zeros(n_fft, dtype=np.int64)
                Tt = k["kStMaxTile"]
                while Tt >= G:
                    fits = G * 2 * n_fft + (((Tt - 1) * hop + n_fft + 1) & ~1) + Tt * (n_fft // 2 + 1) * c <= k["kStLdsFloats"]
                    chosen = np.where((chosen == 0) & fits, Tt, chosen)
                    Tt //= 2
                assert (chosen >= G).all(), (n_fft, output, bins_first)  # a tile fits, and it holds whole rounds of side-by-side frames
                for h in {1, 2, 65, 66, 97, 98, 134, 135, 160, 441, 626, 627, 1024, 1227, 1228, 1754, 1755, 4093, 4094, 8190, 8191, n_fft - 1, n_fft}:
                    if h <= n_fft:
                        Tt, floats = st.tile_plan(n_fft, h, output, bins_first, k)
                        assert Tt == chosen[h - 1] and Tt % G == 0 and floats <= k["kStLdsFloats"]
                        span = st.span_floats(n_fft, h, Tt)
                        # the staging writes span[0 .. count), count <= (Tt - 1) hop + n_fft; frame f reads span[f hop + m], m < n_fft; the stage
                        # behind an even span holds pairs
                        assert (Tt - 1) * h + n_fft <= span and span % 2 == 0
                        assert floats == G * 2 * n_fft + span + Tt * (n_fft // 2 + 1) * c
                        most[(n_fft, output, bins_first)] = max(most.get((n_fft, output, bins_first), 0), floats)
    # where the tiles change (the kernel file's plan, worked out): the largest hop of each bins-first tile
    def last(n, output, tile):
        return max((h for h in range(1, n + 1) if st.tile_plan(n, h, output, True, k)[0] >= tile), default=0)
    assert [last(512, o, 32) for o in ("complex", "power")] == [512, 512]
    assert [last(1024, "complex", t) for t in (32, 16)] == [97, 1024] and [last(1024, "power", t) for t in (32, 16)] == [626, 1024]
    assert [last(2048, "complex", t) for t in (32, 16, 8)] == [0, 134, 2048] and [last(2048, "power", t) for t in (32, 16, 8)] == [65, 1227, 2048]
    assert [last(4096, "complex", t) for t in (8, 4, 2)] == [0, 4093, 4096] and [last(4096, "power", t) for t in (16, 8, 4)] == [0, 1754, 4096]
    assert [last(8192, "complex", t) for t in (2, 1)] == [0, 8192] and [last(8192, "power", t) for t in (4, 2, 1)] == [0, 8190, 8192]
    assert [max(h for h in range(1, n + 1) if st.tile_plan(n, h, "complex", False, k)[0] == 32) for n in st.NFFTS] == [512, 1024, 1123, 924, 528]  # frames first
    assert st.tile_plan(8192, 8192, "complex", True, k) == (1, 32770) and most[(8192, "complex", True)] == 32770
    assert max(most.values()) == 40960
    tiles = {}
    for name, (n_fft, hop, win_length, window, F, tc, tr) in st.CASES.items():
        assert st.tile_plan(n_fft, hop, "complex", True, k)[0] == tc, name
        assert st.tile_plan(n_fft, hop, "power", True, k)[0] == st.tile_plan(n_fft, hop, "magnitude", True, k)[0] == tr, name
        T = 1 + F // hop
        tiles.setdefault(tc, set()).add(T)
        tiles.setdefault(tr, set()).add(T)
    # a T one less than, equal to and one more than each tile size the plan can take (no row has T = 0)
    assert sorted(tiles) == [1, 2, 4, 8, 16, 32]
    assert all({tile - 1, tile, tile + 1} - {0} <= Ts for tile, Ts in tiles.items()), tiles
    # the smallest padded length with one frame at every n_fft, and hop 1 at 512 alone
    assert {c[0] for c in st.CASES.values() if c[4] == c[0] // 2 + 1 and c[1] == c[0]} == set(st.NFFTS)
    assert [(c[0], 1 + c[4] // c[1]) for c in st.CASES.values() if c[1] == 1] == [(512, 258)]
    named = {(c[0], c[1], c[2], c[3]) for c in st.CASES.values()}
    assert {(2048, 441, 2048, "hann"), (512, 160, 400, "hamming"), (512, 128, 511, "hann"), (1024, 256, 1024, "hann"), (4096, 1024, 4096, "hann"),
            (8192, 8192, 8192, "hann")} <= named and any(c[2] == 2 and c[0] == 512 for c in st.CASES.values())


# ---- the surface
def test_the_stft_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_stft.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmStft.cs")
    assert sorted(c) == ["vpz_pcm_stft", "vpz_stft_table"] == sorted(imports) == sorted(capi.PCM_STFT_EXPORTED_SYMBOLS)
    assert c["vpz_stft_table"] == ("i32", ["i32", "i32", "i32", "ptr", "i64"])
    assert c["vpz_pcm_stft"] == cs.c_functions("vorbispizza_pcm_melspec.h", "vpz_")["vpz_pcm_melspec"]  # (argument for argument, but for the spec's type)
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_STFT_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    assert dict((n, a) for n, _, a in capi._PCM_STFT_SIGNATURES)["vpz_pcm_stft"][4] == C.POINTER(capi.StftSpec)
    # the struct: the header's fields in order, in C# and in ctypes, 64 bytes
    structs, defines = cs.c_structs("vorbispizza_pcm_stft.h")
    assert list(structs) == ["vpz_stft_spec"]
    fields = structs["vpz_stft_spec"]
    assert fields == [("n_fft", "i32", 0), ("hop", "i32", 0), ("win_length", "i32", 0), ("window", "i32", 0), ("output", "i32", 0), ("layout", "i32", 0),
                      ("reserved", "i32", 10)]
    sharp = cs.cs_structs(os.path.join(cs.CS, "GpuPcmStft.cs"))
    assert list(sharp) == ["StftSpec"] and len(sharp["StftSpec"]) == len(fields)
    for (n0, k0, a0), (n1, k1, a1) in zip(fields, sharp["StftSpec"]):
        assert cs.norm(n0) == cs.norm(n1) and k0 == k1 and a0 == a1, (n0, n1)
    assert C.sizeof(capi.StftSpec) == 64 and [f[0] for f in capi.StftSpec._fields_] == [f[0] for f in fields]
    assert all(t is C.c_int32 for _, t in capi.StftSpec._fields_[:6]) and capi.StftSpec._fields_[6][1]._length_ == 10
    s = capi.StftSpec.make()
    assert (s.n_fft, s.hop, s.win_length, s.window, s.output, s.layout, list(s.reserved)) == (4096, 1024, 4096, 0, 0, 0, [0] * 10)
    s = capi.StftSpec.make(n_fft=512, hop=160, win_length=400, window="hamming", output="magnitude", bins_first=False)
    assert (s.n_fft, s.hop, s.win_length, s.window, s.output, s.layout) == (512, 160, 400, 1, 1, 1) and s.n_freq == 257 and s.row_shape(1600) == (11, 257)
    assert capi.StftSpec.make(n_fft=512, hop=128).row_shape(256) == (257, 3, 2)
    # the constants
    text = cs.strip_cs_comments(open(os.path.join(cs.CS, "GpuPcmStft.cs")).read())
    consts = {}
    for m in re.finditer(r"public\s+const\s+int\s+([^;]+);", text):
        for part in m.group(1).split(","):
            key, v = part.split("=")
            consts[cs.norm(key.strip())] = int(v.strip(), 0)
    seen = 0
    for name, value in defines.items():
        if name.startswith("VPZ_STFT_"):
            assert consts[cs.norm(name[4:])] == value == getattr(capi, name[4:]), name
            seen += 1
    assert seen == 9
    # the older headers and their lists did not take the new names
    for name in c:
        assert name not in capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_LOGMEL_EXPORTED_SYMBOLS + capi.PCM_MELSPEC_EXPORTED_SYMBOLS
        assert name not in cs.c_functions("vorbispizza_synth.h", "vpz_") and name not in cs.c_functions("vorbispizza_pcm_melspec.h", "vpz_")


def test_the_stft_call_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_stft.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiStft.cs")
    assert sorted(c) == ["vpzm_decode_ranges_stft"] == sorted(imports) == sorted(multi.STFT_EXPORTED_SYMBOLS)
    # the resampled call's arguments with the spec in the layout's place
    old = cs.c_functions("vorbispizza_multi_resample.h", "vpzm_")["vpzm_decode_ranges_resampled"]
    assert c["vpzm_decode_ranges_stft"] == ("i32", ["ptr", "i32", "ptr", "ptr", "ptr", "i32", "i32", "i32", "ptr", "i64", "ptr", "ptr", "ptr"])
    assert old[1][:8] == c["vpzm_decode_ranges_stft"][1][:8]
    assert imports["vpzm_decode_ranges_stft"] == ("Host",) + c["vpzm_decode_ranges_stft"]
    fn = multi.lib().vpzm_decode_ranges_stft
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_decode_ranges_stft"][1] and KINDS[fn.restype] == "i32"
    assert cs.c_structs("vorbispizza_multi_stft.h")[0] == {}
    sig = inspect.signature(multi.Dispatcher.decode_ranges_stft)
    assert list(sig.parameters) == ["self", "datas", "ranges", "frames", "sample_rate", "channels", "mono", "n_fft", "hop", "win_length", "window", "output",
                                    "bins_first", "out"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["sample_rate"], d["channels"], d["mono"], d["n_fft"], d["hop"], d["win_length"], d["window"], d["output"], d["bins_first"], d["out"]) == (
        44100, 2, False, 4096, 1024, None, "hann", "complex", True, None)
    # the call without a dispatcher, and with no spec: refused before anything else
    spec = __import__("vorbispizza_amd").capi.StftSpec.make()
    assert fn(None, 0, None, None, None, 44100, 2, 0, C.byref(spec), 4096, None, None, None) == multi.E_ARG
    assert fn(None, 0, None, None, None, 44100, 2, 0, None, 4096, None, None, None) == multi.E_ARG


def test_both_libraries_export_the_new_symbols(capi):
    from vorbispizza_amd import _build, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in capi.PCM_STFT_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert hasattr(H, "vpzm_decode_ranges_stft") and not hasattr(S, "vpzm_decode_ranges_stft")
    assert _build.SOURCES["pcm_stft.hip"] == ["-ffp-contract=off"] and os.path.exists(os.path.join(_build.CSRC, "stft_tables.hpp"))
    assert callable(capi.pcm_stft) and callable(capi.stft_table) and callable(multi.Dispatcher.decode_ranges_stft)


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    for header, body in (("vorbispizza_pcm_stft.h", "sizeof(vpz_stft_spec) == 64 && VPZ_STFT_MIN_NFFT == 512 && VPZ_STFT_MAX_NFFT == 8192 && VPZ_STFT_POWER == 2"),
                         ("vorbispizza_multi_stft.h", "VPZM_E_RATE == -16 && VPZ_STFT_FRAMES_FIRST == 1 && VPZ_STFT_HAMMING == 1 && sizeof(vpz_stft_spec) == 64")):
        src = tmp_path / (header + ".c")
        src.write_text('#include "%s"\ntypedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % (header, body))
        exe = tmp_path / (header + ".exe")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


def test_the_stft_kernels_use_no_scratch_and_say_what_they_take():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = [k for k in kr.analyse(os.path.join(_build.CSRC, "pcm_stft.hip"), _build.SOURCES["pcm_stft.hip"]) if "pcm_stft_kernel" in k["name"]]
    assert len(ks) == 5  # <n_fft 512, 1024, 2048, 4096, 8192>
    for k in ks:
        print("%s: %d VGPRs, %d AGPRs, %d bytes of static LDS (the dynamic request is the launch's: stft_truth.tile_plan), occupancy %d" % (
            k["name"], k["vgprs"], k.get("agprs", 0), k.get("lds", 0), k["occupancy"]))
        assert k["scratch"] == 0 and k.get("vgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 512 and k["occupancy"] >= 1, k  # (a lane keeps its window values and twiddles in registers)
