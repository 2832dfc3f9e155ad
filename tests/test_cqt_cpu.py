"""vpz_pcm_cqt without a GPU: the device-free exports held to tests/cqt_truth.py by bits, the truth held to an independent construction and
to closed forms, every limit refused, the surface (headers, C#, ctypes, Python) in agreement, the tile plan restated, and the float32
restatement inside the bound of the truth on every case of tests/test_pcm_cqt_gpu.py -- so that the GPU tests' tolerance is known to
admit the reference arithmetic."""
import ctypes as C
import inspect
import math
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

import cqt_truth as ct  # noqa: E402
import binding_support as cs  # noqa: E402
from logmel_truth import KINDS  # noqa: E402
from binding_support import imports_of  # noqa: E402
from cqt_truth import cqt_refused_specs, make  # noqa: E402


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


# ---- the exports
@pytest.mark.parametrize("name", list(ct.CASES))
def test_the_exports_are_the_truth(capi, name):
    """f_k exactly, N_k exactly, and every coefficient the truth's double rounded once, by bits"""
    s = ct.CASES[name]["spec"]
    spec = make(capi, s)
    f, n = capi.cqt_bins(spec)
    tf, tn = ct.bins(s)
    assert f.dtype == np.float64 and n.dtype == np.int32
    assert f.tobytes() == np.asarray(tf, dtype=np.float64).tobytes() and list(n) == tn
    assert all(a >= b for a, b in zip(tn, tn[1:])) and tn[-1] >= 2
    for k, (hr, hi) in enumerate(ct.kernels64(s)):
        got_r, got_i = capi.cqt_kernel(spec, k)
        assert got_r.tobytes() == hr.astype(np.float32).tobytes() and got_i.tobytes() == hi.astype(np.float32).tobytes(), k


def test_the_named_lengths():
    """the lengths the header names"""
    for sr, B, n0 in ((22050.0, 12, 11339), (44100.0, 12, 22678), (22050.0, 36, 34683), (44100.0, 24, 46021), (44100.0, 36, 69365)):
        assert ct.bins(dict(ct.DEFAULT, sample_rate=sr, bins_per_octave=B, n_bins=1))[1][0] == n0
    f, n = ct.bins(ct.DEFAULT)
    assert sum(n) == 200481 and (n[0], n[32], n[64]) == (11339, 1786, 282) and n[0] * 84 == 952476
    assert ct.bins(ct.BASE)[1][0] == 539 and ct.bins(ct.BASE)[1][39] == 57
    assert ct.bins(ct.CASES["two_taps"]["spec"])[1] == [8, 4, 2]
    assert ct.bins(ct.CASES["limit_N0_65536"]["spec"])[1][0] == 65536
    nb = ct.bins(ct.BASE)[1]
    assert {v % 2 for v in nb[:32]} == {0, 1} and {v % 2 for v in nb[32:]} == {0, 1}  # both parities inside either block
    assert [ct.bins(ct.CASES["chunk_N0_%d" % v]["spec"])[1][0] for v in (2047, 2048, 2049, 4097)] == [2047, 2048, 2049, 4097]
    assert ct.kernel_constants()["kCqChunk"] == 2048 and ct.kernel_constants()["kCqCols"] == 32


def test_sizing_calls_and_capacities(capi):
    spec = make(capi, ct.spec_of())
    L = capi.lib()
    assert L.vpz_cqt_bins(C.byref(spec), None, None, 0) == capi.OK
    f, n = np.zeros(40), np.zeros(40, dtype=np.int32)
    assert L.vpz_cqt_bins(C.byref(spec), f.ctypes.data, None, 39) == capi.E_CAPACITY
    assert L.vpz_cqt_bins(C.byref(spec), None, n.ctypes.data, 39) == capi.E_CAPACITY
    assert L.vpz_cqt_bins(C.byref(spec), f.ctypes.data, n.ctypes.data, -1) == capi.E_INVALID_ARG
    assert L.vpz_cqt_bins(None, f.ctypes.data, n.ctypes.data, 40) == capi.E_INVALID_ARG
    assert (f == 0).all() and (n == 0).all()
    assert L.vpz_cqt_bins(C.byref(spec), None, n.ctypes.data, 40) == capi.OK and n[0] == 539 and (f == 0).all()
    length = C.c_int32(0)
    assert L.vpz_cqt_kernel(C.byref(spec), 39, None, 0, C.byref(length)) == capi.OK and length.value == 57
    table = np.zeros(2 * 57, dtype=np.float32)
    assert L.vpz_cqt_kernel(C.byref(spec), 39, table.ctypes.data, 2 * 57 - 1, None) == capi.E_CAPACITY and (table == 0).all()
    assert L.vpz_cqt_kernel(C.byref(spec), 39, table.ctypes.data, -1, None) == capi.E_INVALID_ARG
    assert L.vpz_cqt_kernel(C.byref(spec), 40, None, 0, None) == capi.E_INVALID_ARG and L.vpz_cqt_kernel(C.byref(spec), -1, None, 0, None) == capi.E_INVALID_ARG
    assert L.vpz_cqt_kernel(None, 0, None, 0, None) == capi.E_INVALID_ARG
    assert L.vpz_cqt_kernel(C.byref(spec), 39, table.ctypes.data, 2 * 57, None) == capi.OK and table.any()
    with pytest.raises(ValueError):
        capi.cqt_kernel(spec, 40)


def test_every_limit_is_refused(capi):
    L = capi.lib()
    specs = cqt_refused_specs(capi)
    assert len(specs) == 33
    for what, spec in specs:
        assert L.vpz_cqt_bins(C.byref(spec), None, None, 0) == capi.E_INVALID_ARG, what
        assert L.vpz_cqt_kernel(C.byref(spec), 0, None, 0, None) == capi.E_INVALID_ARG, what
        assert L.vpz_pcm_cqt(None, None, 0, 4096, C.byref(spec), 0, None, None, 0) == capi.E_INVALID_ARG, what
        with pytest.raises(ValueError):
            capi.cqt_bins(spec)
    # the edges of the limits are inside them
    for what, kw in (("n_bins 512", dict(n_bins=512, bins_per_octave=96, f_min=50.0)), ("hop 2048", dict(hop=2048)), ("hop 1", dict(hop=1)),
                     ("the last bin at Nyquist", dict(n_bins=49)), ("N_0 65536", ct.CASES["limit_N0_65536"]["spec"]),
                     ("N_k 2", ct.CASES["two_taps"]["spec"]), ("gamma 0", dict(gamma=0.0)), ("bins_per_octave 96", dict(bins_per_octave=96, n_bins=8))):
        spec = make(capi, ct.spec_of(), **kw)
        assert L.vpz_cqt_bins(C.byref(spec), None, None, 0) == capi.OK, what
    assert ct.bins(ct.spec_of(n_bins=49))[0][48] == 4000.0 and ct.bins(ct.spec_of(n_bins=50))[0][49] > 4000.0
    with pytest.raises(ValueError):
        capi.CqtSpec.make(window="blackman")
    with pytest.raises(ValueError):
        capi.CqtSpec.make(pad="edge")


# ---- the truth
def _independent(x, L, F, s):
    """Z by another road: torch.nn.functional.conv1d in float64 over the explicitly padded row, with kernels built in a plain loop from
    the definition's formulas (numpy's functions, another order of evaluation)"""
    import torch
    B, sr = s["bins_per_octave"], s["sample_rate"]
    alpha = 2.0 ** (1.0 / B) - 1.0
    Q = s["filter_scale"] / alpha
    fs = [s["f_min"] * 2.0 ** (k / B) for k in range(s["n_bins"])]
    ns = [int(np.ceil(Q * sr / (f + s["gamma"] / alpha))) for f in fs]
    n0 = ns[0]
    pad = n0 // 2
    row = np.zeros(F)
    row[:L] = x[:L]
    if s["pad"] == "reflect":
        padded = np.concatenate([row[1: pad + 1][::-1], row, row[-pad - 1: -1][::-1]])
    else:
        padded = np.concatenate([np.zeros(pad), row, np.zeros(pad)])
    padded = np.concatenate([padded, np.zeros(2)])  # (beyond the reflection x is zero: the last frame of an odd N_0 reads one such sample when hop divides F)
    W = np.zeros((2 * len(ns), 1, n0 + 1))
    for k, (f, n) in enumerate(zip(fs, ns)):
        j = np.arange(n)
        g = (0.54 - 0.46 * np.cos(2 * np.pi * j / n)) if s["window"] == "hamming" else (0.5 - 0.5 * np.cos(2 * np.pi * j / n))
        sk = (np.sqrt(n) if s["scale"] == "sqrt_length" else 1.0) / g.sum()
        ph = 2 * np.pi * f * (j - n // 2) / sr
        at = pad - n // 2
        W[k, 0, at: at + n] = sk * g * np.cos(ph)
        W[len(ns) + k, 0, at: at + n] = -sk * g * np.sin(ph)
    out = torch.nn.functional.conv1d(torch.from_numpy(padded)[None, None, :], torch.from_numpy(W), stride=s["hop"])[0].numpy()
    T = 1 + F // s["hop"]
    assert out.shape[1] >= T
    return (out[: len(ns), :T] + 1j * out[len(ns):, :T]).T


@pytest.mark.parametrize("name", ["cols_40", "cols_65", "hop_63", "hop_100_above_N39", "two_taps", "reflect_smallest_F", "zero_F1_hop1", "zero_F100", "hamming",
                                  "variable_q", "scale_none", "chunk_N0_2049"])
def test_the_truth_is_a_dense_convolution(name):
    c = ct.CASES[name]
    src, rows = ct.case_input(name)
    for (a, L, _), (Z, dr, di) in zip(rows, ct.case_truth(name)):
        other = _independent(src[a: a + L].astype(np.float64), L, c["F"], c["spec"])
        assert other.shape == Z.shape
        scale = max(np.abs(Z).max(), 1e-300)
        assert np.abs(other - Z).max() <= 1e-12 * scale, (name, L)


def test_a_unit_impulse_in_closed_form():
    """x = 1 at sample p, well inside a row: bin k of frame t reads it at j = p - t hop + floor(N_k / 2) and is h_k[j] where the frame
    covers p, zero elsewhere"""
    s = ct.spec_of()
    hop = s["hop"]
    F = hop * 40 + 11
    p = hop * 20 + 3
    x = np.zeros(F)
    x[p] = 1.0
    Z, dr, di = ct.truth(x, F, F, s)
    f, n = ct.bins(s)
    seen = 0
    for k, (hr, hi) in enumerate(ct.kernels64(s)):
        j = p - np.arange(Z.shape[0]) * hop + n[k] // 2
        covers = (j >= 0) & (j < n[k])
        want = np.where(covers, hr[np.clip(j, 0, n[k] - 1)] + 1j * hi[np.clip(j, 0, n[k] - 1)], 0.0)
        assert np.array_equal(Z[:, k], want)
        seen += int(covers.sum())
    assert seen > 100
    # the restatement has it too: one product, rounded once
    re_, im_ = ct.chains32([(x.astype(np.float32), F)], F, s)[0]
    k = 0
    j = p - np.arange(Z.shape[0]) * hop + n[0] // 2
    covers = (j >= 0) & (j < n[0])
    assert np.array_equal(re_[covers, 0], ct.kernels64(s)[0][0].astype(np.float32)[j[covers]]) and (re_[~covers, 0] == 0).all()


@pytest.mark.parametrize("window", ["hann", "hamming"])
def test_a_unit_cosine_reads_half(window):
    """x = cos(2 pi f_k n / sample_rate), scale none, frames away from the ends: X[t][k] = 0.5 e^(i theta_t) (1 + leak), where the leak is
    the window's transform at 2 f_k against its sum, conjugated onto the other side: |X| = 0.5 |1 + e^(-2 i theta_t) W(2 f_k) / W(0)| with
    W(f) = sum_j g[j] e^(-2 pi i f (j - floor(N / 2)) / sample_rate).  The leak is computed, not assumed small"""
    s = ct.spec_of(scale="none", window=window)
    f, n = ct.bins(s)
    sr, hop = s["sample_rate"], s["hop"]
    F = hop * 30
    a0, a1 = (0.54, 0.46) if window == "hamming" else (0.5, 0.5)
    for k in (0, 7, 20, 39):
        x = np.cos(2 * np.pi * f[k] * np.arange(F) / sr)
        Z = ct.truth(x, F, F, s)[0]
        j = np.arange(n[k])
        g = a0 - a1 * np.cos(2 * np.pi * j / n[k])
        W2 = (g * np.exp(-2j * np.pi * 2 * f[k] * (j - n[k] // 2) / sr)).sum()
        t = np.arange(6, 24)  # (t hop +- N_0 / 2 inside the row)
        theta = 2 * np.pi * f[k] * t * hop / sr
        want = 0.5 * np.exp(1j * theta) * (1 + np.exp(-2j * theta) * W2 / g.sum())
        assert np.abs(Z[t, k] - want).max() <= 1e-12
        assert np.abs(np.abs(Z[t, k]) - 0.5 * np.abs(1 + np.exp(-2j * theta) * W2 / g.sum())).max() <= 1e-12
        assert abs(W2 / g.sum()) < 0.05  # (and small it is: the reading is 0.5 to a few per cent at the most)


def test_the_bounds_are_the_headers_formulas():
    """d = (N_k + 2) u S_k per component, and the two derived bounds of vorbispizza_pcm_stft.h"""
    s = ct.spec_of(n_bins=3)
    rng = np.random.default_rng(5)
    F = 700
    x = rng.standard_normal(F)
    Z, dr, di = ct.truth(x, F, F, s)
    f, n = ct.bins(s)
    hr, hi = ct.kernels64(s)[1]
    t = 5
    seg = np.abs(x[t * 64 - n[1] // 2: t * 64 - n[1] // 2 + n[1]])
    assert math.isclose(dr[t, 1], (n[1] + 2) * 2.0 ** -24 * float(seg @ np.abs(hr)), rel_tol=1e-12)
    assert math.isclose(di[t, 1], (n[1] + 2) * 2.0 ** -24 * float(seg @ np.abs(hi)), rel_tol=1e-12)
    d = np.maximum(dr, di)
    P, eP = ct.power_truth(Z, d)
    assert np.allclose(eP, 2 * np.abs(Z.real) * d + 2 * np.abs(Z.imag) * d + 2 * d * d + 3 * ct.U * P, rtol=1e-15)
    M, eM = ct.magnitude_truth(Z, d)
    assert np.allclose(eM, math.sqrt(2) * d + 3 * ct.U * M, rtol=1e-15)
    text = open(os.path.join(ROOT, "include", "vorbispizza_pcm_cqt.h")).read()
    assert "d = (N_k + 2) u S_k" in text and "finite input only" in text and "Out of scope" in text


@pytest.mark.parametrize("name", list(ct.CASES))
def test_the_restatement_stays_inside_the_bound_on_every_case(name):
    worst = {}
    for (Z, dr, di), r in zip(ct.case_truth(name), ct.case_restated(name)):
        for output in ct.OUTPUTS:
            worst[output] = max(worst.get(output, 0.0), ct.check_output(output, r[output], Z, dr, di))
    print("restatement error / bound %s: %s" % (name, worst))
    assert max(worst.values()) < 1.0


def test_the_end_to_end_bound_admits_the_reference_arithmetic(oracle):
    """tests/test_multi_cqt_gpu.py's end-to-end spec over its synthetic entry, without a device: the window of the stream's whole decode
    (the CPU oracle's: no decoder on the device), resampled in float64 to y; the float32 restatement of the chains over y rounded to
    float32 stays within d = (N_k + 2) u sum |y| |h_k| of the direct sum over y -- the multi test's bound with r = 0"""
    from multi_support import CQT_END_TO_END, end_to_end_entries, out_len, ratio
    from resample_truth import resample_truth
    rate = CQT_END_TO_END["sample_rate"]
    s = dict(ct.DEFAULT, **dict(CQT_END_TO_END, sample_rate=float(rate)))
    assert ct.bins(s)[1][0] == 3372 and ct.bins(s)[1][0] // 2 == 1686
    stream, a, n = end_to_end_entries()[1]
    f = stream.f
    pk, res, posts, counts = f.decode_packets()
    fs = oracle.FlooredStream(f.channels, f.block_size0, f.block_size1, pk, res, posts, counts, floors=f.floors, mappings=f.mappings)
    assert fs.run() == stream.total and stream.channels == 2 and a + n <= stream.total
    up, down = ratio(stream, rate)
    y, _ = resample_truth(fs.pcm[:, a: a + n].T, up, down, False)
    J = out_len(n, up, down)
    assert y.shape == (J, 2) and 2400 <= J <= 2600
    F = J + 3 * s["hop"]
    worst = 0.0
    for c in range(2):
        Z, dr, di = ct.truth_of_a_row_within(y[:, c], np.zeros(J), J, F, s)
        plain = ct.truth(y[:, c], J, F, s)
        assert all(np.array_equal(p, q) for p, q in zip((Z, dr, di), plain))  # (r = 0 is the stage's own truth and bound)
        (re_, im_), = ct.chains32([(y[:, c].astype(np.float32), J)], F, s)
        worst = max(worst, ct.check_output("complex", ct.outputs32(re_, im_)["complex"], Z, dr, di))
        assert (dr == 0).any() and (np.abs(Z) > 1e-3).any()
    print("restatement error / bound, end to end: %.4f" % worst)
    assert worst < 1.0


def test_a_wrong_coefficient_or_order_fails_the_value_check():
    """what the bound cannot see the restatement does: one coefficient off by one ulp, or the chain run in descending j, changes values"""
    s = ct.spec_of(n_bins=3)
    F = 700
    x = (np.random.default_rng(6).standard_normal(F) * 0.25).astype(np.float32)
    re_, im_ = ct.chains32([(x, F)], F, s)[0]
    (k0, half, tab), = ct.block_tables32(s, 32)
    A = ct.frames_of(ct.extend(x, F, F, s, half + 2).astype(np.float32), half + 2, 1 + F // 64, 64, -half, tab.shape[0])
    acc = np.zeros((A.shape[0], 64), dtype=np.float32)
    for m in reversed(range(tab.shape[0])):
        acc = ct._fma(A[:, m, None], tab[None, m, :], acc)
    assert not np.array_equal(acc[:, :3], re_) and np.allclose(acc[:, :3], re_, atol=1e-5)
    off = tab.copy()
    off[half, 0] = np.nextafter(off[half, 0], np.float32(np.inf))
    acc = np.zeros((A.shape[0], 64), dtype=np.float32)
    for m in range(tab.shape[0]):
        acc = ct._fma(A[:, m, None], off[None, m, :], acc)
    assert not np.array_equal(acc[:, 0], re_[:, 0]) and np.array_equal(acc[:, 1:3], re_[:, 1:3])


# ---- the plan
def test_the_tile_plan_fits_and_the_cases_take_their_tiles():
    k = ct.kernel_constants()
    assert k["kCqLdsFloats"] * 4 <= 160 * 1024 and k["kCqChunk"] % 2 == 0 and k["kCqMaxTile"] == 64 and k["kCqMinTile"] == 16
    # every hop inside the limits has a tile, whatever T; the smallest tile fits at the largest hop
    for hop in range(1, 2049):
        for T in (1, 16, 17, 32, 33, 1000):
            Tt, lanes, lds = ct.tile_plan(hop, T, k)
            assert Tt in (16, 32, 64) and lds <= k["kCqLdsFloats"] and lanes == (256 if Tt == 64 else 128)
            assert Tt != 64 or T > 32
    assert ct.tile_plan(512, 65, k)[0] == 64 and ct.tile_plan(512, 32, k)[0] == 32 and ct.tile_plan(2048, 100, k)[0] == 16
    tiles = set()
    for name, c in ct.CASES.items():
        T = 1 + c["F"] // c["spec"]["hop"]
        assert ct.tile_plan(c["spec"]["hop"], T, k)[0] == c["tile"], name
        tiles.add(c["tile"])
    assert tiles == {16, 32, 64}
    # T one under, at and one over every tile size
    for tile, hop in ((32, 64), (64, 64), (16, 1200)):
        assert {1 + c["F"] // c["spec"]["hop"] for c in ct.CASES.values() if c["spec"]["hop"] == hop} >= {tile - 1, tile, tile + 1}
    # the kernel states the same plan: its functions, read as text
    text = open(os.path.join(ROOT, "vorbispizza_amd", "csrc", "pcm_cqt.hip")).read()
    assert "const int count = (Tt - 1) * hop + kCqChunk;" in text and "return count + (hop % 2 == 0 ? count / hop : 0) + 1;" in text
    assert "return span_floats(hop, Tt) + 2 * Tt * kCqStageStride;" in text
    assert "for (int Tt : {kCqMaxTile, 32, kCqMinTile}) {" in text and "if ((Tt == kCqMaxTile && T <= 32) || lds_floats(hop, Tt) > kCqLdsFloats) continue;" in text
    assert "const unsigned lanes = a.Tt > 32 ? 256 : 128;" in text
    assert ct.grid_of(ct.DEFAULT, 22050, 64, k) == (1, 64, 3) and ct.grid_of(ct.DEFAULT, 22050 * 30, 3000, k) == (21, 2048, 3)


# ---- the surface
def test_the_cqt_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_cqt.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmCqt.cs")
    assert sorted(c) == ["vpz_cqt_bins", "vpz_cqt_kernel", "vpz_pcm_cqt"] == sorted(imports) == sorted(capi.PCM_CQT_EXPORTED_SYMBOLS)
    assert c["vpz_cqt_bins"] == ("i32", ["ptr", "ptr", "ptr", "i32"])
    assert c["vpz_cqt_kernel"] == ("i32", ["ptr", "i32", "ptr", "i64", "ptr"])
    assert c["vpz_pcm_cqt"] == cs.c_functions("vorbispizza_pcm_stft.h", "vpz_")["vpz_pcm_stft"]  # (argument for argument, but for the spec's type)
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_CQT_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    assert dict((n, a) for n, _, a in capi._PCM_CQT_SIGNATURES)["vpz_pcm_cqt"][4] == C.POINTER(capi.CqtSpec)
    # the struct: the header's fields in order, in C# and in ctypes, 96 bytes
    structs, defines = cs.c_structs("vorbispizza_pcm_cqt.h")
    assert list(structs) == ["vpz_cqt_spec"]
    fields = structs["vpz_cqt_spec"]
    assert [(n, a) for n, _, a in fields] == [("sample_rate", 0), ("f_min", 0), ("filter_scale", 0), ("gamma", 0), ("n_bins", 0), ("bins_per_octave", 0), ("hop", 0),
                                              ("window", 0), ("scale", 0), ("pad", 0), ("output", 0), ("layout", 0), ("reserved", 8)]
    assert len({kind for _, kind, _ in fields[:4]}) == 1 and {kind for _, kind, _ in fields[4:]} == {"i32"} and fields[0][1] != "i32"
    sharp = cs.cs_structs(os.path.join(cs.CS, "GpuPcmCqt.cs"))
    assert list(sharp) == ["CqtSpec"] and len(sharp["CqtSpec"]) == len(fields)
    for (n0, k0, a0), (n1, k1, a1) in zip(fields, sharp["CqtSpec"]):
        assert cs.norm(n0) == cs.norm(n1) and k0 == k1 and a0 == a1, (n0, n1)
    assert C.sizeof(capi.CqtSpec) == 96 and [f[0] for f in capi.CqtSpec._fields_] == [f[0] for f in fields]
    assert all(t is C.c_double for _, t in capi.CqtSpec._fields_[:4]) and all(t is C.c_int32 for _, t in capi.CqtSpec._fields_[4:12])
    assert capi.CqtSpec._fields_[12][1]._length_ == 8
    # CqtSpec.make's defaults: the music spec
    s = capi.CqtSpec.make()
    assert (s.sample_rate, s.f_min, s.filter_scale, s.gamma) == (22050.0, 32.70319566257483, 1.0, 0.0)
    assert (s.n_bins, s.bins_per_octave, s.hop, s.window, s.scale, s.pad, s.output, s.layout, list(s.reserved)) == (84, 12, 512, 0, 1, 0, 1, 0, [0] * 8)
    assert s.row_shape(22050) == (84, 44) and capi.cqt_bins(s)[1][0] == 11339
    s = capi.CqtSpec.make(sample_rate=8000, f_min=250, n_bins=40, hop=64, window="hamming", scale="none", pad="zero", output="complex", bins_first=False)
    assert (s.window, s.scale, s.pad, s.output, s.layout) == (1, 0, 1, 0, 1) and s.row_shape(640) == (11, 40, 2) and s.n_frames(640) == 11
    # the constants
    text = cs.strip_cs_comments(open(os.path.join(cs.CS, "GpuPcmCqt.cs")).read())
    consts = {}
    for m in re.finditer(r"public\s+const\s+int\s+([^;]+);", text):
        for part in m.group(1).split(","):
            key, v = part.split("=")
            consts[cs.norm(key.strip())] = int(v.strip(), 0)
    seen = 0
    for name, value in defines.items():
        if name.startswith("VPZ_CQT_"):
            assert consts[cs.norm(name[4:])] == value == getattr(capi, name[4:]), name
            seen += 1
    assert seen == 15
    # the older headers and their lists did not take the new names
    for name in c:
        assert name not in capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_STFT_EXPORTED_SYMBOLS
        assert name not in cs.c_functions("vorbispizza_synth.h", "vpz_") and name not in cs.c_functions("vorbispizza_pcm_stft.h", "vpz_")


def test_the_cqt_call_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import capi, multi
    c = cs.c_functions("vorbispizza_multi_cqt.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiCqt.cs")
    assert sorted(c) == ["vpzm_decode_ranges_cqt"] == sorted(imports) == sorted(multi.CQT_EXPORTED_SYMBOLS)
    # the STFT call's signature with the spec's type changed
    assert c["vpzm_decode_ranges_cqt"] == cs.c_functions("vorbispizza_multi_stft.h", "vpzm_")["vpzm_decode_ranges_stft"]
    assert imports["vpzm_decode_ranges_cqt"] == ("Host",) + c["vpzm_decode_ranges_cqt"]
    fn = multi.lib().vpzm_decode_ranges_cqt
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_decode_ranges_cqt"][1] and KINDS[fn.restype] == "i32"
    assert fn.argtypes[8] == C.POINTER(capi.CqtSpec)
    assert cs.c_structs("vorbispizza_multi_cqt.h")[0] == {}
    sig = inspect.signature(multi.Dispatcher.decode_ranges_cqt)
    assert list(sig.parameters) == ["self", "datas", "ranges", "frames", "sample_rate", "channels", "mono", "f_min", "n_bins", "bins_per_octave", "hop",
                                    "filter_scale", "gamma", "window", "scale", "pad", "output", "bins_first", "out"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert [d[k] for k in list(sig.parameters)[4:]] == [22050, 1, True, 32.70319566257483, 84, 12, 512, 1.0, 0.0, "hann", "sqrt_length", "reflect", "magnitude",
                                                       True, None]
    # the call without a dispatcher, with no spec, with a spec outside the limits and with too short a row: refused before anything else
    spec = capi.CqtSpec.make()
    assert fn(None, 0, None, None, None, 22050, 1, 1, C.byref(spec), 22050, None, None, None) == multi.E_ARG
    assert fn(None, 0, None, None, None, 22050, 1, 1, None, 22050, None, None, None) == multi.E_ARG


def test_both_libraries_export_the_new_symbols(capi):
    from vorbispizza_amd import _build, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in capi.PCM_CQT_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert hasattr(H, "vpzm_decode_ranges_cqt") and not hasattr(S, "vpzm_decode_ranges_cqt")
    assert _build.SOURCES["pcm_cqt.hip"] == ["-ffp-contract=off"] and os.path.exists(os.path.join(_build.CSRC, "cqt_tables.hpp"))
    assert callable(capi.pcm_cqt) and callable(capi.cqt_bins) and callable(capi.cqt_kernel) and callable(multi.Dispatcher.decode_ranges_cqt)


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    for header, body in (("vorbispizza_pcm_cqt.h", "sizeof(vpz_cqt_spec) == 96 && VPZ_CQT_MAX_LENGTH == 65536 && VPZ_CQT_MAX_HOP == 2048 && VPZ_CQT_POWER == 2"),
                         ("vorbispizza_multi_cqt.h", "VPZM_E_RATE == -16 && VPZ_CQT_FRAMES_FIRST == 1 && VPZ_CQT_PAD_ZERO == 1 && sizeof(vpz_cqt_spec) == 96")):
        src = tmp_path / (header + ".c")
        src.write_text('#include "%s"\ntypedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % (header, body))
        exe = tmp_path / (header + ".exe")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


def test_the_cqt_kernel_uses_no_scratch_and_says_what_it_takes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = [k for k in kr.analyse(os.path.join(_build.CSRC, "pcm_cqt.hip"), _build.SOURCES["pcm_cqt.hip"]) if "pcm_cqt_kernel" in k["name"]]
    assert len(ks) == 1
    for k in ks:
        print("%s: %d VGPRs, %d AGPRs, %d bytes of static LDS (the dynamic request is the launch's: cqt_truth.tile_plan), occupancy %d" % (
            k["name"], k["vgprs"], k.get("agprs", 0), k.get("lds", 0), k["occupancy"]))
        assert k["scratch"] == 0 and k.get("vgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 128 and k["occupancy"] >= 4, k
