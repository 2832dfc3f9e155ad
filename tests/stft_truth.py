"""THE TRUTH of the STFT tests (include/vorbispizza_pcm_stft.h states the definition), in float64 numpy, and what the tests of vpz_pcm_stft
share: the window, the derived bounds of the three outputs, a float32 restatement of the kernel's own network over a window table, the
launch plan restated from csrc/pcm_stft.hip's constants, and the case list of tests/test_pcm_stft_gpu.py (tests/test_stft_cpu.py holds the
list to the plan without a GPU).

Truth: extend / frames_of are tests/test_logmel_cpu.py's (the signal and the frames are the mel stages', word for word); K, passes and the
twiddles of tables64 are tests/melspec_truth.py's; the spectrum is numpy.fft.rfft of the float64 windowed frames -- Re X and Im X themselves.

The bounds (u = 2^-24).  For a frame with extended samples x[m] and window w[m], S = sum_m |x[m]| w[m]; the kernel's Re and Im lie within
    d = K(n_fft) u S,        K = sqrt(2) (5 r4 + r2 + 2) + 7
of the truth (the header derives it).  Then
    e_P = 2 |re| d + 2 |im| d + 2 d^2 + 3 u P          (power)
    e_M = sqrt(2) d + 3 u |X|                          (magnitude)
Every element is held to its bound: there is no log and no floor, so none is exempt.

The restatement computes every fused multiply-add exactly (the float64 sum rounded to odd before the one rounding to float32), so that its
values are the kernel's and not merely close: the COMPLEX and POWER outputs are held to it as values."""
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from melspec_truth import K, passes, tables64  # noqa: E402,F401
from f32_model import cmul as _cmul, fma32 as _fma, network32, U  # noqa: E402,F401
from logmel_truth import extend, frames_of  # noqa: E402,F401
from kernel_text import constants_of  # noqa: E402


def stft_refused_specs(capi):
    """(what, spec) for every limit of the definition"""
    good = dict(n_fft=2048, hop=512)
    cases = [("n_fft 256", dict(n_fft=256, hop=64)), ("n_fft 400", dict(n_fft=400, hop=100)), ("n_fft 513", dict(n_fft=513)), ("n_fft 3000", dict(n_fft=3000)),
             ("n_fft 16384", dict(n_fft=16384)), ("n_fft 0", dict(n_fft=0, hop=1, win_length=2)), ("n_fft < 0", dict(n_fft=-2048, hop=1, win_length=2)),
             ("hop < 1", dict(hop=0)), ("hop > n_fft", dict(hop=2049)), ("win_length < 2", dict(win_length=1)), ("win_length 0", dict(win_length=0)),
             ("win_length > n_fft", dict(win_length=2049))]
    out = [(what, capi.StftSpec.make(**dict(good, **kw))) for what, kw in cases]
    for field, value in (("window", 2), ("window", -1), ("output", 3), ("output", -1), ("layout", 2), ("layout", -1)):
        s = capi.StftSpec.make(**good)
        setattr(s, field, value)
        out.append(("%s %d" % (field, value), s))
    for i in (0, 9):
        s = capi.StftSpec.make(**good)
        s.reserved[i] = 1
        out.append(("a reserved word", s))
    return out


NFFTS = (512, 1024, 2048, 4096, 8192)
OUTPUTS = ("complex", "magnitude", "power")


def window64(n_fft, win_length=None, window="hann"):
    """w, float64 [n_fft]: the periodic window over win_length, centred in n_fft as torch.stft centres it"""
    win_length = n_fft if win_length is None else win_length
    j = np.arange(win_length)
    a0, a1 = (0.54, 0.46) if window == "hamming" else (0.5, 0.5)
    w = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    w[left: left + win_length] = a0 - a1 * np.cos(2.0 * np.pi * j / win_length)
    return w


def spectrum64(X, w):
    """X[k], complex128 [T, n_fft / 2 + 1], of frames X under the window w"""
    return np.fft.rfft(np.asarray(X, dtype=np.float64) * w, axis=-1)


def truth(X, n_fft, w):
    """(Z, d): the spectrum and the bound of its components, float64 [T, n_fft / 2 + 1] and [T, 1]"""
    return spectrum64(X, w), (K(n_fft) * U * (np.abs(X) @ w))[:, None]


def power_truth(Z, d):
    P = Z.real ** 2 + Z.imag ** 2
    return P, 2 * np.abs(Z.real) * d + 2 * np.abs(Z.imag) * d + 2 * d * d + 3 * U * P


def magnitude_truth(Z, d):
    M = np.abs(Z)
    return M, math.sqrt(2.0) * d + 3 * U * M


def check_output(output, got, Z, d):
    """`got` -- complex64 or float32 [T, n_freq] -- within the bound of the truth, every element; exactly zero where the bound is.  Returns
    the largest error / bound"""
    if output == "complex":
        err = np.maximum(np.abs(got.real.astype(np.float64) - Z.real), np.abs(got.imag.astype(np.float64) - Z.imag))
        tol = np.broadcast_to(d, err.shape)
    else:
        want, tol = power_truth(Z, d) if output == "power" else magnitude_truth(Z, d)
        err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all()
    assert (err <= tol).all(), float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else float(err.max())
    assert (got[tol == 0] == 0).all()
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


# ---- the kernel's own network, in float32 numpy (frames along the first axis): tests/melspec_truth.py's network32 over a window table and
# at every H from 256, with an exact fused multiply-add
def tables32(n_fft, win_length=None, window="hann"):
    """(w, t) in float32: the restatement rounded once (tests/test_stft_cpu.py holds vpz_stft_table to these bits)"""
    return window64(n_fft, win_length, window).astype(np.float32), tables64(n_fft)[1].astype(np.float32)


def outputs32(re_, im_):
    """the three outputs of a restated spectrum: complex64, and float32 magnitude and power"""
    P = _fma(re_, re_, im_ * im_)
    Z = np.empty(re_.shape, dtype=np.complex64)
    Z.real, Z.imag = re_, im_
    return {"complex": Z, "power": P, "magnitude": np.sqrt(P)}


# ---- the launch plan, restated
# the constants of csrc/pcm_stft.hip's plan as the file states them
kernel_constants = constants_of("pcm_stft.hip", ("kStBlock", "kStLdsFloats", "kStMaxGridY", "kStMaxTile"))


def lanes_per_frame(n_fft, k):
    """a frame's transform takes one lane per radix-4 butterfly of a pass, n_fft / 8, a workgroup's at the most"""
    return min(n_fft // 8, k["kStBlock"])


def side_by_side(n_fft, k):
    """frames of a tile a workgroup carries at once: 4, 2, 1, 1, 1"""
    return k["kStBlock"] // lanes_per_frame(n_fft, k)


def span_floats(n_fft, hop, Tt):
    return ((Tt - 1) * hop + n_fft + 1) & ~1


def lds_floats(n_fft, hop, Tt, output, bins_first, k):
    """a pair of complex arrays per frame side by side, the span, and bins-first the stage"""
    stage = Tt * (n_fft // 2 + 1) * (2 if output == "complex" else 1) if bins_first else 0
    return side_by_side(n_fft, k) * 2 * n_fft + span_floats(n_fft, hop, Tt) + stage


def tile_plan(n_fft, hop, output, bins_first=True, k=None):
    """(frames of a tile, LDS floats of the launch): the largest tile that fits, from the spec alone; (0, None) where none does"""
    k = k or kernel_constants()
    Tt = k["kStMaxTile"]
    while Tt >= side_by_side(n_fft, k):
        if lds_floats(n_fft, hop, Tt, output, bins_first, k) <= k["kStLdsFloats"]:
            return Tt, lds_floats(n_fft, hop, Tt, output, bins_first, k)
        Tt //= 2
    return 0, None


# ---- the cases of tests/test_pcm_stft_gpu.py
# name: (n_fft, hop, win_length, window, F, the bins-first tile of the complex output, that of the other two).  Every case carries rows of
# L = F, F - 1 (the right-hand reflection starts at the one zero), F - n_fft / 4 (it reads the zero tail), about a third (silent tiles behind
# it), 1 and 0.
def _smallest(n_fft, tc, tr):
    return (n_fft, n_fft, n_fft, "hann", n_fft // 2 + 1, tc, tr)


CASES = {
    "smallest_512": _smallest(512, 32, 32), "smallest_1024": _smallest(1024, 16, 16), "smallest_2048": _smallest(2048, 8, 8),
    "smallest_4096": _smallest(4096, 2, 4),  # (T = 1: one under the tile of 2)
    "smallest_8192": _smallest(8192, 1, 1),  # (T = 1: at the tile of 1)
    "hop_1_512": (512, 1, 512, "hann", 257, 32, 32),  # T = 258: eight tiles and one of two
    # a T one under, at and one over each tile the plan can take: 32 (512, both kinds), 16 (1024 / 256 complex), 8 (2048 / 441 complex, 4096 /
    # 1024 the other two), 4 (4096 / 1024 complex), 2 (4096 / 4096 complex), 1 (8192 complex)
    "enhance_512_128_T31": (512, 128, 512, "hann", 128 * 30 + 5, 32, 32), "enhance_512_128_T32": (512, 128, 512, "hann", 128 * 31 + 5, 32, 32),
    "enhance_512_128_T33": (512, 128, 512, "hann", 128 * 32 + 5, 32, 32),
    "vocoder_1024_256_T15": (1024, 256, 1024, "hann", 256 * 14 + 5, 16, 32), "vocoder_1024_256_T16": (1024, 256, 1024, "hann", 256 * 15 + 5, 16, 32),
    "vocoder_1024_256_T17": (1024, 256, 1024, "hann", 256 * 16 + 5, 16, 32),
    "odd_hop_2048_441_T7": (2048, 441, 2048, "hann", 441 * 6 + 5, 8, 16), "odd_hop_2048_441_T8": (2048, 441, 2048, "hann", 441 * 7 + 5, 8, 16),
    "odd_hop_2048_441_T9": (2048, 441, 2048, "hann", 441 * 8 + 5, 8, 16),
    "separation_4096_1024_T3": (4096, 1024, 4096, "hann", 1024 * 2 + 5, 4, 8), "separation_4096_1024_T4": (4096, 1024, 4096, "hann", 1024 * 3 + 5, 4, 8),
    "separation_4096_1024_T5": (4096, 1024, 4096, "hann", 1024 * 4 + 5, 4, 8), "separation_4096_1024_T7": (4096, 1024, 4096, "hann", 1024 * 6 + 5, 4, 8),
    "separation_4096_1024_T8": (4096, 1024, 4096, "hann", 1024 * 7 + 5, 4, 8), "separation_4096_1024_T9": (4096, 1024, 4096, "hann", 1024 * 8 + 5, 4, 8),
    "disjoint_4096_4096_T2": (4096, 4096, 4096, "hann", 4096 + 5, 2, 4), "disjoint_4096_4096_T3": (4096, 4096, 4096, "hann", 4096 * 2 + 5, 2, 4),
    # the named spec sets
    "odd_hop_2048_441_T38": (2048, 441, 2048, "hann", 441 * 37 + 5, 8, 16),
    "speech_512_160_400_hamming": (512, 160, 400, "hamming", 160 * 20 + 7, 32, 32),
    "odd_centring_512_128_511": (512, 128, 511, "hann", 128 * 9 + 3, 32, 32),  # left = 0, one zero on the right
    "two_taps_512": (512, 128, 2, "hann", 128 * 5 + 3, 32, 32),                 # w = (0, 1) at m = 255, 256
    "widest_8192_8192_T2": (8192, 8192, 8192, "hann", 8192 + 100, 1, 1),      # the most LDS an 8192 launch asks for (complex, bins first)
}
DST_ROWS = 9


def case_tables(name):
    n_fft, hop, win_length, window, F, tc, tr = CASES[name]
    return tables32(n_fft, win_length, window)


_INPUTS, _TRUTHS, _RESTATED = {}, {}, {}


def case_input(name):
    """(src float32, rows [(src offset, L, destination row)]) of a case: broadband noise; the rows share one source array at odd offsets
    and overlap in it"""
    if name in _INPUTS:
        return _INPUTS[name]
    n_fft, hop, win_length, window, F, tc, tr = CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 1000 + hop)
    Ls = [F, F - 1, F - n_fft // 4, F // 3, 1, 0]
    gap = F // 5
    src = (rng.standard_normal(2 * (len(Ls) - 1) * gap + F + 64) * 0.25).astype(np.float32)
    order = rng.permutation(DST_ROWS)[: len(Ls)]
    rows = [(1 + 2 * i * gap, L, int(row)) for i, (L, row) in enumerate(zip(Ls, order))]
    assert all(a % 2 == 1 and a + L <= src.size for a, L, _ in rows)
    _INPUTS[name] = (src, rows)
    return _INPUTS[name]


def case_frames(name):
    """[X float64 [T, n_fft]] of a case's rows"""
    n_fft, hop, win_length, window, F, tc, tr = CASES[name]
    src, rows = case_input(name)
    return [frames_of(src[a: a + L], L, F, n_fft, hop) for a, L, _ in rows]


def case_truth(name):
    """[(Z, d)] of a case's rows, computed once"""
    if name not in _TRUTHS:
        n_fft, hop, win_length, window, F, tc, tr = CASES[name]
        w = window64(n_fft, win_length, window)
        _TRUTHS[name] = [truth(X, n_fft, w) for X in case_frames(name)]
    return _TRUTHS[name]


def case_restated(name):
    """[{output: values}] of a case's rows by the float32 restatement, computed once"""
    if name not in _RESTATED:
        n_fft = CASES[name][0]
        w, t = case_tables(name)
        _RESTATED[name] = [outputs32(*network32(X.astype(np.float32), n_fft, w, t)) for X in case_frames(name)]
    return _RESTATED[name]
