"""THE TRUTH of the constant-Q tests (include/vorbispizza_pcm_cqt.h states the definition), in float64, and what the tests of vpz_pcm_cqt
share: the bins, the kernels, the extended row, the direct sum with its bound per element, a float32 restatement of the kernel's chains, the
tile plan restated from csrc/pcm_cqt.hip's constants, and the case list of tests/test_pcm_cqt_gpu.py (tests/test_cqt_cpu.py holds the
restatement to the bound on every case without a GPU).

f_k, N_k and the coefficients are evaluated with Python's math module, operation for operation as the header writes them, so that they
are the library's doubles and not merely close to them; tests/test_cqt_cpu.py holds the exports to them by bits.

The bounds (u = 2^-24).  With S_k = sum_j |x| |h_k[j]| over a frame, Re and Im lie within d = (N_k + 2) u S_k of the truth (the header
derives it).  Then
    e_P = 2 |re| d + 2 |im| d + 2 d^2 + 3 u P          (power)
    e_M = sqrt(2) d + 3 u |X|                          (magnitude)
Every element is held to its bound: none is exempt.

The restatement computes every fused multiply-add exactly (tests/stft_truth.py's _fma), one chain per (t, k) over j ascending from +0,
vectorised over (t, k) and looping j over a column block's longest kernel, the shorter kernels centre-aligned and padded with zeros as
the device table holds them: its values are the kernel's, and the COMPLEX and POWER outputs are held to them as values."""
import ctypes
import ctypes.util
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from stft_truth import _fma, magnitude_truth, power_truth  # noqa: E402,F401
from kernel_text import constants_of  # noqa: E402


def make(capi, s, **kw):
    return capi.CqtSpec.make(**dict(s, **kw))


def cqt_refused_specs(capi, good=None):
    """(what, spec) for every limit of the definition"""
    good = dict(good or spec_of())
    limit = CASES["limit_N0_65536"]["spec"]
    cases = [("sample_rate 0", dict(sample_rate=0.0)), ("sample_rate < 0", dict(sample_rate=-8000.0)), ("sample_rate NaN", dict(sample_rate=float("nan"))),
             ("f_min 0", dict(f_min=0.0)), ("f_min < 0", dict(f_min=-250.0)), ("the last bin over Nyquist", dict(n_bins=50)),
             ("n_bins 0", dict(n_bins=0)), ("n_bins < 0", dict(n_bins=-1)), ("n_bins 513", dict(n_bins=513, bins_per_octave=96, f_min=50.0)),
             ("bins_per_octave 0", dict(bins_per_octave=0)), ("bins_per_octave 97", dict(bins_per_octave=97)),
             ("filter_scale 0", dict(filter_scale=0.0)), ("filter_scale < 0", dict(filter_scale=-1.0)), ("gamma < 0", dict(gamma=-1.0)),
             ("gamma infinite", dict(gamma=float("inf"))),
             ("N_k < 2", dict(f_min=975.0, n_bins=3, bins_per_octave=1, filter_scale=0.4)),
             ("N_0 over 65536", dict(limit, f_min=_f_min_for(65537, limit["sample_rate"], limit["bins_per_octave"]))),
             ("N_0 69365 (44.1 kHz, 36 to the octave)", dict(sample_rate=44100.0, f_min=32.70319566257483, n_bins=3, bins_per_octave=36)),
             ("hop 0", dict(hop=0)), ("hop < 0", dict(hop=-64)), ("hop 2049", dict(hop=2049))]
    out = [(what, make(capi, good, **kw)) for what, kw in cases]
    for field, value in (("window", 2), ("window", -1), ("scale", 2), ("scale", -1), ("pad", 2), ("pad", -1), ("output", 3), ("output", -1), ("layout", 2),
                         ("layout", -1)):
        s = make(capi, good)
        setattr(s, field, value)
        out.append(("%s %d" % (field, value), s))
    for i in (0, 7):
        s = make(capi, good)
        s.reserved[i] = 1
        out.append(("a reserved word", s))
    return out


U = 2.0 ** -24
OUTPUTS = ("complex", "magnitude", "power")
DEFAULT = dict(sample_rate=22050.0, f_min=32.70319566257483, n_bins=84, bins_per_octave=12, hop=512, filter_scale=1.0, gamma=0.0,
               window="hann", scale="sqrt_length", pad="reflect")
BASE = dict(DEFAULT, sample_rate=8000.0, f_min=250.0, n_bins=40, hop=64)  # N_0 = 539, N_39 = 57


def spec_of(**changes):
    unknown = set(changes) - set(DEFAULT)
    assert not unknown, unknown
    return dict(BASE, **changes)


# ---- the definition
# (2^x is the C library's exp2, as the header says: Python's own power is another function and differs from it in the last place here and there)
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.exp2.restype, _libm.exp2.argtypes = ctypes.c_double, [ctypes.c_double]


def exp2(x):
    return float(_libm.exp2(float(x)))


def bins(s):
    """(f_k, N_k): lists of Python floats and ints"""
    B = float(s["bins_per_octave"])
    alpha = exp2(1.0 / B) - 1.0
    Q = s["filter_scale"] / alpha
    f = [s["f_min"] * exp2(float(k) / B) for k in range(s["n_bins"])]
    return f, [int(math.ceil(Q * s["sample_rate"] / (fk + s["gamma"] / alpha))) for fk in f]


def kernel64(s, f, n):
    """(hr, hi), float64 [n], of a bin at f with n taps: every step in the header's order"""
    two_pi = 2.0 * math.pi
    a0, a1 = (0.54, 0.46) if s["window"] == "hamming" else (0.5, 0.5)
    g = [a0 - a1 * math.cos(two_pi * float(j) / float(n)) for j in range(n)]
    G = 0.0
    for v in g:
        G += v
    sk = math.sqrt(float(n)) / G if s["scale"] == "sqrt_length" else 1.0 / G
    half = n // 2
    hr, hi = np.empty(n), np.empty(n)
    for j in range(n):
        phi = two_pi * f * float(j - half) / s["sample_rate"]
        sg = sk * g[j]
        hr[j], hi[j] = sg * math.cos(phi), -(sg * math.sin(phi))
    return hr, hi


_KERNELS = {}


def kernels64(s):
    """[(hr, hi)] of every bin, computed once per table-shaping part of a spec"""
    key = tuple(s[n] for n in ("sample_rate", "f_min", "n_bins", "bins_per_octave", "filter_scale", "gamma", "window", "scale"))
    if key not in _KERNELS:
        f, n = bins(s)
        _KERNELS[key] = [kernel64(s, fk, nk) for fk, nk in zip(f, n)]
    return _KERNELS[key]


def extend(x, L, F, s, margin):
    """the extended row as float64: element margin + e is x[e], e = -margin .. F - 1 + margin, by the spec's pad mode; positions the
    definition does not name (beyond floor(N_0 / 2) under reflection) are zeros: only a zero coefficient meets them"""
    row = np.zeros(F)
    row[:L] = np.asarray(x[:L], dtype=np.float64)
    out = np.zeros(F + 2 * margin)
    out[margin: margin + F] = row
    if s["pad"] == "reflect":
        reach = bins(s)[1][0] // 2
        assert F >= reach + 1 and margin >= reach
        i = np.arange(1, reach + 1)
        out[margin - i] = row[i]
        out[margin + F - 1 + i] = row[F - 1 - i]
    return out


def frames_of(xe, margin, T, hop, start, length):
    """[T, length]: frame t is xe's samples t * hop + start .. + length"""
    idx = margin + start + np.arange(T)[:, None] * hop + np.arange(length)[None, :]
    return xe[idx]


def truth(x, L, F, s):
    """(Z complex128 [T, n_bins], d_re, d_im float64 [T, n_bins]): the direct sum with the exact coefficients, and d = (N_k + 2) u S_k of
    either component, S_k over that component's own coefficients"""
    f, n = bins(s)
    margin = n[0] // 2 + 2
    xe = extend(x, L, F, s, margin)
    T = 1 + F // s["hop"]
    Z, dr, di = np.zeros((T, len(n)), dtype=np.complex128), np.zeros((T, len(n))), np.zeros((T, len(n)))
    for k, (hr, hi) in enumerate(kernels64(s)):
        X = frames_of(xe, margin, T, s["hop"], -(n[k] // 2), n[k])
        Z[:, k] = X @ hr + 1j * (X @ hi)
        dr[:, k], di[:, k] = (n[k] + 2) * U * (np.abs(X) @ np.abs(hr)), (n[k] + 2) * U * (np.abs(X) @ np.abs(hi))
    return Z, dr, di


def truth_of_a_row_within(y, r, L, F, s):
    """(Z, d_re, d_im) where the row the kernel reads is not y itself but lies within r[j] >= 0 of it (y, r float64 [L]): the transform is
    linear, so the truth over y moves by at most sum_j r |h_k[j]|, and the kernel's own roundings act on magnitudes of at most |y| + r:
    d = (N_k + 2) u sum_j (|y| + r) |h_k[j]| + sum_j r |h_k[j]| of either component.  r = 0 is truth()"""
    f, n = bins(s)
    margin = n[0] // 2 + 2
    y, r = np.asarray(y[:L], dtype=np.float64), np.asarray(r[:L], dtype=np.float64)
    assert (r >= 0).all()
    ye, me, re_ = extend(y, L, F, s, margin), extend(np.abs(y) + r, L, F, s, margin), extend(r, L, F, s, margin)
    T = 1 + F // s["hop"]
    Z, dr, di = np.zeros((T, len(n)), dtype=np.complex128), np.zeros((T, len(n))), np.zeros((T, len(n)))
    for k, (hr, hi) in enumerate(kernels64(s)):
        X, M, R = (frames_of(e, margin, T, s["hop"], -(n[k] // 2), n[k]) for e in (ye, me, re_))
        Z[:, k] = X @ hr + 1j * (X @ hi)
        dr[:, k], di[:, k] = (n[k] + 2) * U * (M @ np.abs(hr)) + R @ np.abs(hr), (n[k] + 2) * U * (M @ np.abs(hi)) + R @ np.abs(hi)
    return Z, dr, di


def check_output(output, got, Z, dr, di):
    """`got` -- complex64 or float32 [T, n_bins] -- within the bound of the truth, every element; exactly zero where the bound is.  Re is
    held to d of hr, Im to d of hi; power and magnitude take the larger of the two as the header's d.  Returns the largest error / bound"""
    d = np.maximum(dr, di)
    if output == "complex":
        er, ei = np.abs(got.real.astype(np.float64) - Z.real), np.abs(got.imag.astype(np.float64) - Z.imag)
        assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
        assert (er <= dr).all() and (ei <= di).all()
        assert (got.real[dr == 0] == 0).all() and (got.imag[di == 0] == 0).all()
        ratios = [(e[t > 0] / t[t > 0]).max() for e, t in ((er, dr), (ei, di)) if (t > 0).any()]
        return float(max(ratios)) if ratios else 0.0
    want, tol = power_truth(Z, d) if output == "power" else magnitude_truth(Z, d)
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all()
    assert (err <= tol).all(), float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else float(err.max())
    assert (got[tol == 0] == 0).all()
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


# ---- the kernel's chains, in float32 numpy
def block_tables32(s, cols):
    """[(first bin, half, table float32 [len, 2 * cols])] per column block: the block's kernels rounded once, centre-aligned in the
    longest (its first bin's), the Re columns, then the Im columns, zeros elsewhere; len is the longest made even"""
    f, n = bins(s)
    ks = kernels64(s)
    out = []
    for k0 in range(0, len(n), cols):
        longest = n[k0]
        half, length = longest // 2, (longest + 1) & ~1
        tab = np.zeros((length, 2 * cols), dtype=np.float32)
        for k in range(k0, min(k0 + cols, len(n))):
            assert n[k] <= longest
            at = half - n[k] // 2
            tab[at: at + n[k], k - k0] = ks[k][0].astype(np.float32)
            tab[at: at + n[k], cols + k - k0] = ks[k][1].astype(np.float32)
        out.append((k0, half, tab))
    return out


def chains32(windows, F, s, cols=None):
    """[(re, im)] float32 [T, n_bins] per (x, L) of `windows`: ONE chain per element over j ascending, from +0, every step one fused
    multiply-add; all windows' frames ride in one array"""
    cols = cols or kernel_constants()["kCqCols"]
    f, n = bins(s)
    margin = n[0] // 2 + 2
    T = 1 + F // s["hop"]
    xes = [extend(x, L, F, s, margin).astype(np.float32) for x, L in windows]
    re_, im_ = np.zeros((len(xes) * T, len(n)), np.float32), np.zeros((len(xes) * T, len(n)), np.float32)
    for k0, half, tab in block_tables32(s, cols):
        A = np.concatenate([frames_of(xe, margin, T, s["hop"], -half, tab.shape[0]) for xe in xes])
        acc = np.zeros((A.shape[0], 2 * cols), dtype=np.float32)
        for m in range(tab.shape[0]):
            acc = _fma(A[:, m, None], tab[None, m, :], acc)
        nb = min(cols, len(n) - k0)
        re_[:, k0: k0 + nb], im_[:, k0: k0 + nb] = acc[:, :nb], acc[:, cols: cols + nb]
    return [(re_[i * T: (i + 1) * T], im_[i * T: (i + 1) * T]) for i in range(len(xes))]


def outputs32(re_, im_):
    """the three outputs of restated chains as the header writes them: complex64, and float32 magnitude and power"""
    P = _fma(re_, re_, im_ * im_)
    Z = np.empty(re_.shape, dtype=np.complex64)
    Z.real, Z.imag = re_, im_
    return {"complex": Z, "power": P, "magnitude": np.sqrt(P)}


# ---- the tile plan, restated
# the constants of csrc/pcm_cqt.hip's plan as the file states them
kernel_constants = constants_of("pcm_cqt.hip", ("kCqCols", "kCqChunk", "kCqLdsFloats", "kCqMaxGridY", "kCqMaxTile", "kCqMinTile",
                                "kCqStageStride"))


def span_floats(hop, Tt, k):
    count = (Tt - 1) * hop + k["kCqChunk"]
    return count + (count // hop if hop % 2 == 0 else 0) + 1


def lds_floats(hop, Tt, k):
    """the span of a chunk of every frame of the tile, then the stage of both components"""
    return span_floats(hop, Tt, k) + 2 * Tt * k["kCqStageStride"]


def tile_plan(hop, T, k=None):
    """(frames of a tile, lanes of a workgroup, LDS floats): the largest tile where the row has more than 32 frames and the LDS holds it,
    else 32, else the smallest; 64 lanes per (32 frames, component); (0, 0, None) where none fits"""
    k = k or kernel_constants()
    for Tt in (k["kCqMaxTile"], 32, k["kCqMinTile"]):
        if (Tt == k["kCqMaxTile"] and T <= 32) or lds_floats(hop, Tt, k) > k["kCqLdsFloats"]:
            continue
        return Tt, 256 if Tt > 32 else 128, lds_floats(hop, Tt, k)
    return 0, 0, None


def grid_of(s, F, n_rows, k=None):
    """(tiles, descriptors side by side, column blocks) of a launch"""
    k = k or kernel_constants()
    T = 1 + F // s["hop"]
    Tt = tile_plan(s["hop"], T, k)[0]
    return -(-T // Tt), min(n_rows, k["kCqMaxGridY"]), -(-s["n_bins"] // k["kCqCols"])


# ---- the cases of tests/test_pcm_cqt_gpu.py
def _f_min_for(n0, sample_rate, B, filter_scale=1.0):
    """an f_min whose N_0 is n0: Q sample_rate / f_min = n0 - 0.5"""
    return filter_scale / (exp2(1.0 / B) - 1.0) * sample_rate / (n0 - 0.5)


def _case(F, Ls=None, tile=None, **changes):
    return dict(spec=spec_of(**changes), F=F, Ls=Ls, tile=tile)


def _cases():
    c = {}
    # columns: the edges of the column blocks (65 bins under Nyquist take 24 to the octave)
    for nb in (1, 32, 33, 40):
        c["cols_%d" % nb] = _case(64 * 9 + 5, n_bins=nb, tile=32)
    for nb in (64, 65):
        c["cols_%d" % nb] = _case(64 * 9 + 5, n_bins=nb, bins_per_octave=24, tile=32)
    # tile boundaries: T one under, at and one over 32 and 64 (hop 64), and 16 (hop 1200: 32 frames do not fit the LDS); two tiles of 32
    # where 64 do not fit (hop 600)
    for T in (31, 32, 33, 63, 64, 65):
        c["tile_T%d" % T] = _case(64 * (T - 1) + 5, Ls=[64 * (T - 1) + 5, 64 * (T - 1) - 100, 700], tile=32 if T <= 32 else 64)
    for T in (15, 16, 17):
        c["tile16_T%d" % T] = _case(1200 * (T - 1) + 5, Ls=[1200 * (T - 1) + 5, 1200 * (T - 1) - 700], hop=1200, n_bins=8, tile=16)
    c["tile32_hop600_T34"] = _case(600 * 33 + 5, Ls=[600 * 33 + 5, 600 * 20], hop=600, n_bins=8, tile=32)
    # hops: odd (no skew), 1, the limit, and one above N_39 = 57 (frames skip samples of the high bins)
    c["hop_63"] = _case(63 * 9 + 5, hop=63, tile=32)
    c["hop_1"] = _case(300, hop=1, n_bins=33, tile=64)
    c["hop_2"] = _case(300, hop=2, n_bins=8, tile=64)
    c["hop_2048"] = _case(2048 * 2 + 5, hop=2048, n_bins=33, tile=16)
    c["hop_100_above_N39"] = _case(100 * 9 + 5, hop=100, tile=32)
    # kernel lengths: N = 8, 4, 2 (B = 1, the last bin just under Nyquist); BASE holds both parities inside a block
    c["two_taps"] = _case(64 * 5 + 3, f_min=975.0, n_bins=3, bins_per_octave=1, filter_scale=0.9, tile=32)
    # staging chunks: N_0 one under, at and one over the chunk, and over two chunks
    for n0 in (2047, 2048, 2049, 4097):
        c["chunk_N0_%d" % n0] = _case(n0 // 2 + 1 + 64 * 3, Ls=[n0 // 2 + 1 + 64 * 3, n0 // 2, 0], f_min=_f_min_for(n0, 8000.0, 12), n_bins=3, tile=32 if n0 < 4000 else 64)  # (T = 20; 36 at 4097)
    # reflect mode at its smallest F (L = F, L < F: zeros are reflected, L = 0)
    c["reflect_smallest_F"] = _case(539 // 2 + 1, tile=32)
    # zero mode: F = 1 (T = 1, and T = 2 at hop 1) and F < N_0 / 2
    c["zero_F1"] = _case(1, Ls=[1, 0], pad="zero", tile=32)
    c["zero_F1_hop1"] = _case(1, Ls=[1, 0], pad="zero", hop=1, tile=32)
    c["zero_F100"] = _case(100, pad="zero", tile=32)
    c["zero_long"] = _case(64 * 9 + 5, pad="zero", tile=32)
    # spec switches
    c["hamming"] = _case(64 * 9 + 5, window="hamming", tile=32)
    c["variable_q"] = _case(64 * 9 + 5, gamma=20.0, tile=32)
    c["scale_none"] = _case(64 * 9 + 5, scale="none", tile=32)
    # the default music spec, one row, T = 65: one tile of 64 and one frame
    c["music_default"] = dict(spec=dict(DEFAULT), F=512 * 64 + 5, Ls=[512 * 64 - 1000], tile=64)
    # the limit: N_0 = 65 536, 3 bins, T = 2 -- no tile could hold this span in LDS
    c["limit_N0_65536"] = dict(spec=dict(DEFAULT, sample_rate=44100.0, f_min=_f_min_for(65536, 44100.0, 36), n_bins=3, bins_per_octave=36,
                                         hop=2048, pad="zero"), F=2048 + 5, Ls=[2048 + 5, 1500], tile=16)
    return c


CASES = _cases()
DST_ROWS = 9


def case_Ls(name):
    c = CASES[name]
    if c["Ls"] is not None:
        return list(c["Ls"])
    F, n0 = c["F"], bins(c["spec"])[1][0]
    return [F, F - 1, max(F - n0 // 4, 0), F // 3, 1, 0]


_INPUTS, _TRUTHS, _RESTATED = {}, {}, {}


def case_input(name):
    """(src float32, rows [(src offset, L, destination row)]) of a case: broadband noise; the rows share one source array at odd offsets,
    the destination rows are named out of order and with gaps, and every element of the source outside the windows is NaN"""
    if name in _INPUTS:
        return _INPUTS[name]
    F, Ls = CASES[name]["F"], case_Ls(name)
    rng = np.random.default_rng(sum(name.encode()) * 1000 + F)
    stride = (F + 6) & ~1
    src = np.full(1 + len(Ls) * stride + 8, np.nan, dtype=np.float32)
    order = rng.permutation(DST_ROWS)[: len(Ls)]
    rows = []
    for i, (L, row) in enumerate(zip(Ls, order)):
        at = 1 + i * stride
        src[at: at + L] = (rng.standard_normal(L) * 0.25).astype(np.float32)
        rows.append((at, L, int(row)))
    assert all(a % 2 == 1 and 0 <= L <= F and a + L <= src.size for a, L, _ in rows)
    _INPUTS[name] = (src, rows)
    return _INPUTS[name]


def case_truth(name):
    """[(Z, d_re, d_im)] of a case's rows, computed once"""
    if name not in _TRUTHS:
        c = CASES[name]
        src, rows = case_input(name)
        _TRUTHS[name] = [truth(src[a: a + L], L, c["F"], c["spec"]) for a, L, _ in rows]
    return _TRUTHS[name]


def case_restated(name):
    """[{output: values}] of a case's rows by the float32 restatement, computed once"""
    if name not in _RESTATED:
        c = CASES[name]
        src, rows = case_input(name)
        _RESTATED[name] = [outputs32(re_, im_) for re_, im_ in chains32([(src[a: a + L], L) for a, L, _ in rows], c["F"], c["spec"])]
    return _RESTATED[name]
