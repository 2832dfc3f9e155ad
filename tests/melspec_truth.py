"""THE TRUTH of the mel-spectrogram tests (include/vorbispizza_pcm_melspec.h states the definition), in float64 numpy, and what the tests
of vpz_pcm_melspec share: the derived bound, a float32 restatement of the kernel's own network, the launch plan restated from
csrc/pcm_melspec.hip's constants, and the case list of tests/test_pcm_melspec_gpu.py (tests/test_melspec_cpu.py holds the list to the plan
and to the check's cap without a GPU).

Truth: extend / frames_of and mel_weights64 are tests/test_logmel_cpu.py's; the spectrum is numpy.fft.rfft of the float64 windowed frames
(re = Re X, im = -Im X; P does not see the sign).

The bound (u = 2^-24).  For a frame with extended samples x[m] and window w[m], S = sum_m |x[m]| w[m]; the kernel's re and im lie within
    d = K(n_fft) u S,        K = sqrt(2) (5 r4 + r2 + 2) + 7,   r4 / r2 the radix-4 / radix-2 passes of the n_fft/2-point complex transform
(the header derives it: per pass a path's relative perturbation in the modulus is two sums and a product by a once-rounded twiddle,
2u + 3u; the windowing 2u; the split pass mixes two values with moduli adding up to sqrt(2) at the most and adds 6u S; 1 for the second
order).  Then
    e_P = 2 |re| d + 2 |im| d + 2 d^2 + 3 u P
    e_M = e_P W^T + (B + 2) u M        B: the largest live-bin count of a band
and the values go through test_logmel_cpu's check_log / check_power as they stand.

The whole stage restated in float32 (restated_power32): network32 on the float32 frames, P = fma32(re, re, im * im), one fma32 chain per
band over its live bins, k ascending from 0.0, with the bank the library's host code returns.  tests/test_pcm_melspec_limits_gpu.py holds
the kernel to it bit for bit, over CASES and over LIMIT_CASES: the hops on either side of every change of tile at n_fft 4096 and 8192."""
import math
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from f32_model import U  # noqa: E402,F401
from logmel_truth import extend, frames_of, mel_weights64  # noqa: E402,F401
from logmel_truth import refused_specs, silence_value  # noqa: E402
from kernel_text import constants_of  # noqa: E402
import f32_model  # noqa: E402
from f32_model import fma32 as _fma  # noqa: E402


def melspec_refused_specs(capi):
    """(what, spec) for every limit of the definition: logmel_truth's list carried to this stage's transform sizes, and the sizes it
    does not take"""
    good = dict(sample_rate=22050, n_fft=2048, hop=512, n_mels=128)
    out = []
    for what, s in refused_specs(capi):
        if what.startswith("n_fft"):
            continue
        t = capi.LogMelSpec.make(**good)
        scale = 22050.0 / 16000.0
        t.f_min, t.f_max, t.floor = s.f_min * scale, s.f_max * scale, s.floor
        t.sample_rate = s.sample_rate * scale
        t.hop = {160: 512, 0: 0, 401: 2049}[s.hop]
        t.n_mels = {80: 128, 0: 0, 257: 257}[s.n_mels]
        t.mel_scale, t.mel_norm, t.output, t.layout = s.mel_scale, s.mel_norm, s.output, s.layout
        for i in range(9):
            t.reserved[i] = s.reserved[i]
        out.append((what, t))
    for n_fft in (1024, 2047, 2046, 3000, 6144, 16384, 0, -2048):
        out.append(("n_fft %d" % n_fft, capi.LogMelSpec.make(**dict(good, n_fft=n_fft, hop=min(512, max(1, n_fft))))))
    return out


NFFTS = (2048, 4096, 8192)
FLOOR = 1e-10


def passes(n_fft):
    """(radix-4 passes, radix-2 passes) of the n_fft / 2-point complex transform"""
    lg = (n_fft // 2).bit_length() - 1
    return lg // 2, lg % 2


def K(n_fft):
    r4, r2 = passes(n_fft)
    return math.sqrt(2.0) * (5 * r4 + r2 + 2) + 7


def hann64(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def spectrum64(X, n_fft):
    """(re, im), float64 [T, n_fft / 2 + 1], of frames X"""
    Z = np.fft.rfft(np.asarray(X, dtype=np.float64) * hann64(n_fft), axis=-1)
    return Z.real, -Z.imag


def power_truth(X, n_fft):
    """(P, e_P), float64 [T, n_fft / 2 + 1], of frames X"""
    re_, im_ = spectrum64(X, n_fft)
    d = (K(n_fft) * U * (np.abs(X) @ hann64(n_fft)))[:, None]
    P = re_ * re_ + im_ * im_
    return P, 2 * np.abs(re_) * d + 2 * np.abs(im_) * d + 2 * d * d + 3 * U * P


def melspec_truth(x, L, F, n_fft, hop, W):
    """(M, e_M), float64 [T, n_mels], of one row"""
    P, e_P = power_truth(frames_of(x, L, F, n_fft, hop), n_fft)
    B = int((W > 0).sum(axis=1).max())
    M = P @ W.T
    return M, e_P @ W.T + (B + 2) * U * M


# ---- the kernel's own network, in float32 numpy (frames along the first axis)
def tables64(n_fft):
    """(w, t) in float64: the window and t[k] = (cos, -sin)(2 pi k / n_fft), exact on the axes"""
    k = np.arange(n_fft)
    a = 2.0 * np.pi * k / n_fft
    c, s = np.cos(a), -np.sin(a)
    c[[n_fft // 4, 3 * n_fft // 4]] = 0.0
    s[[0, n_fft // 2]] = 0.0
    return hann64(n_fft), np.stack([c, s], axis=1)


def _network32(X, n_fft, w=None, t=None):
    """(re, im), float32 [T, n_fft / 2 + 1]: f32_model.network32 with the library's own tables by default (tables64 rounded once) and
    this stage's sign, (re, -im)"""
    w64, t64 = tables64(n_fft)
    re_, im_ = f32_model.network32(X, n_fft, w64.astype(np.float32) if w is None else w, t64.astype(np.float32) if t is None else t)
    return re_, -im_


network32 = _network32


def proxy_mel(X, n_fft, W, w=None, t=None):
    """M, float64 [T, n_mels]: the network's power through the once-rounded bank (the band sums in float64: no worse than the kernel's)"""
    re_, im_ = network32(X, n_fft, w, t)
    P = _fma(re_, re_, im_ * im_)
    return P.astype(np.float64) @ W.astype(np.float32).astype(np.float64).T


# ---- the whole stage in float32
def band_sums32(P, first, count, weights):
    """[T, n_mels] float32 of the power P [T, n_fft / 2 + 1]: acc = fma32(w[i], P[first + i], acc) over a band's live bins, i ascending"""
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    bins = np.ascontiguousarray(P.T)  # (a step gathers whole bins: rows of this)
    acc = np.zeros((count.size, P.shape[0]), dtype=np.float32)
    for i in range(int(count.max())):
        live = np.nonzero(i < count)[0]
        acc[live] = _fma(weights[start[live] + i][:, None], bins[first[live] + i], acc[live])
    return np.ascontiguousarray(acc.T)


_POOL = []


def power32(X, n_fft):
    """P = fma32(re, re, im * im), float32 [T, n_fft / 2 + 1], of the float32 frames X.  Frames that are equal bit for bit to the first
    all-zero one are restated once; the others in blocks of 64 frames, side by side (numpy leaves the interpreter's lock in its loops)"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    assert X.ndim == 2 and X.shape[1] == n_fft

    def block(Y):
        re_, im_ = network32(Y, n_fft)
        return _fma(re_, re_, im_ * im_)

    P = np.empty((X.shape[0], n_fft // 2 + 1), dtype=np.float32)
    zero = (X.view(np.uint32) == 0).all(axis=1)
    if zero.any():
        P[zero] = block(X[zero][:1])
    rest = np.nonzero(~zero)[0]
    parts = [rest[i: i + 64] for i in range(0, rest.size, 64)]
    if len(parts) > 1 and not _POOL:
        _POOL.append(ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))))
    for at, out in zip(parts, _POOL[0].map(lambda at: block(X[at]), parts) if len(parts) > 1 else [block(X[at]) for at in parts]):
        P[at] = out
    return P


def restated_power32(X, n_fft, first, count, weights):
    """the stage's power output, float32 [T, n_mels], of the float32 frames X [T, n_fft]: network32 with the library's tables, the fused
    power, and the band sums of the library's bank (first, count, weights as vpz_melspec_filterbank returns them)"""
    assert weights.dtype == np.float32
    return band_sums32(power32(X, n_fft), np.asarray(first, dtype=np.int64), np.asarray(count, dtype=np.int64), weights)


def check_log_exact(got, acc32, floor):
    """the log10 mode against the restated power acc32, no element exempt: the silence value's bits where acc32 <= float32(floor), else
    within 4 u max(1, |got|) of log10(acc32) -- what check_log allows log10f, and nothing for the power: that is known by its bits.
    Returns the largest error / bound ratio."""
    got, acc32 = np.asarray(got, dtype=np.float32), np.asarray(acc32, dtype=np.float32)
    assert got.shape == acc32.shape
    below = acc32 <= np.float32(floor)
    assert (got[below].view(np.uint32) == silence_value(floor).view(np.uint32)).all()
    g = got[~below].astype(np.float64)
    err = np.abs(g - np.log10(acc32[~below].astype(np.float64)))
    tol = 4 * U * np.maximum(1.0, np.abs(g))
    assert (err <= tol).all(), float((err / tol).max())  # (a NaN fails here)
    return float((err / tol).max()) if g.size else 0.0


# ---- the launch plan, restated
# the constants of csrc/pcm_melspec.hip's plan as the file states them
kernel_constants = constants_of("pcm_melspec.hip", ("kMsBlock", "kMsLdsFloats", "kMsMaxGridY", "kMsMelRoom", "kMsAhead", "kMsTileA",
                                "kMsTileB", "kMsTileC"))


def lds_floats(n_fft, hop, Tt, k):
    """the two complex arrays, the span, the mel tile"""
    return 2 * n_fft + (Tt - 1) * hop + n_fft + Tt * k["kMsMelRoom"]


def tile_plan(n_fft, hop, k=None):
    """(frames of a tile, LDS floats of the launch): the largest tile that fits, from n_fft and hop alone; (0, None) where none does"""
    k = k or kernel_constants()
    for Tt in (k["kMsTileA"], k["kMsTileB"], k["kMsTileC"]):
        if lds_floats(n_fft, hop, Tt, k) <= k["kMsLdsFloats"]:
            return Tt, lds_floats(n_fft, hop, Tt, k)
    return 0, None


# ---- the cases of tests/test_pcm_melspec_gpu.py
# name: (sample_rate, n_fft, hop, n_mels, f_min, f_max, mel_scale, mel_norm, F, the tile the plan takes).  f_max None: Nyquist, so that the
# bands reach bin n_fft / 2 (live where the rounding of the mel points leaves it a weight: tests/test_melspec_cpu.py).  Every case
# carries rows of L = F, F - 1 (the right-hand reflection starts at the one zero), F - n_fft / 4 (it reads the zero tail), about a third
# (silent tiles behind it), 1 and 0.
def _smallest(n_fft, hop, tile):
    return (44100, n_fft, hop, 16, 0.0, None, "slaney", "slaney", n_fft // 2 + 1, tile)


CASES = {
    "smallest_2048_one_frame": _smallest(2048, 2048, 16), "smallest_2048_hop_1": _smallest(2048, 1, 16),
    "smallest_4096_one_frame": _smallest(4096, 4096, 2), "smallest_4096_hop_1": _smallest(4096, 1, 16),
    "smallest_8192_one_frame": _smallest(8192, 8192, 2), "smallest_8192_hop_1": _smallest(8192, 1, 16),
    "odd_hop_2048_441": (44100, 2048, 441, 128, 0.0, None, "slaney", "slaney", 441 * 37 + 5, 16),        # T = 38: two whole tiles and one of 6
    "disjoint_4096_4096": (48000, 4096, 4096, 128, 20.0, 20000.0, "htk", None, 4096 * 4 + 100, 2),       # T = 5
    "librosa_2048_512_T15": (22050, 2048, 512, 128, 0.0, None, "slaney", "slaney", 512 * 14 + 5, 16),
    "librosa_2048_512_T16": (22050, 2048, 512, 128, 0.0, None, "slaney", "slaney", 512 * 15 + 5, 16),
    "librosa_2048_512_T17": (22050, 2048, 512, 128, 0.0, None, "slaney", "slaney", 512 * 16 + 5, 16),
    "half_4096_2048_T7": (44100, 4096, 2048, 64, 0.0, None, "htk", "slaney", 2048 * 6 + 5, 8),
    "half_4096_2048_T8": (44100, 4096, 2048, 64, 0.0, None, "htk", "slaney", 2048 * 7 + 5, 8),
    "half_4096_2048_T9": (44100, 4096, 2048, 64, 0.0, None, "htk", "slaney", 2048 * 8 + 5, 8),
    "widest_8192_8192_T2": (48000, 8192, 8192, 256, 0.0, None, "htk", "slaney", 8192 * 1 + 100, 2),       # the most LDS a launch asks for
    "widest_8192_8192_T3": (48000, 8192, 8192, 256, 0.0, None, "htk", "slaney", 8192 * 2 + 100, 2),
    "one_band_4096_1024": (44100, 4096, 1024, 1, 0.0, None, "slaney", "slaney", 1024 * 9 + 3, 16),
    "empty_bands_2048_256": (44100, 2048, 1024, 256, 0.0, 2000.0, "slaney", None, 1024 * 6 + 3, 16),       # bands narrower than a bin
}
DST_ROWS = 9

# ---- the cases of tests/test_pcm_melspec_limits_gpu.py, besides CASES: the last hop of a tile size and the first of the next at n_fft 4096
# and 8192 (the 2048 kernel takes 16 frames at every hop), and the 75 % overlap of 8192 that fills the LDS to the float.  F = hop (T - 1) + 5.
# The banks: 256 htk bands up to Nyquist where an 8192 launch asks for the most LDS, both scales and both norms, f_max None in most, and
# one bank with bands narrower than a bin.
_WIDE = (48000, 8192, 2048, 256, 0.0, None, "htk", "slaney")
LIMIT_CASES = {
    "tile16_last_4096_1638": (44100, 4096, 1638, 128, 0.0, None, "slaney", "slaney", 1638 * 16 + 5, 16),   # T = 17: a whole tile and one of 1
    "tile8_first_4096_1639": (48000, 4096, 1639, 64, 20.0, 20000.0, "htk", None, 1639 * 8 + 5, 8),         # T = 9
    "tile8_last_4096_3803": (44100, 4096, 3803, 128, 0.0, None, "slaney", "slaney", 3803 * 8 + 5, 8),      # T = 9; the 4096 kernel's most LDS
    "tile2_first_4096_3804": (44100, 4096, 3804, 128, 0.0, 500.0, "slaney", None, 3804 * 2 + 5, 2),        # T = 3; bands narrower than a bin
    "tile16_last_8192_819": (48000, 8192, 819, 256, 0.0, None, "htk", None, 819 * 16 + 5, 16),             # T = 17
    "tile8_first_8192_820": (22050, 8192, 820, 64, 0.0, None, "slaney", "slaney", 820 * 8 + 5, 8),         # T = 9
    "full_lds_8192_2048_T7": _WIDE + (2048 * 6 + 5, 8),                                                    # the whole 160 KiB
    "full_lds_8192_2048_T8": _WIDE + (2048 * 7 + 5, 8),
    "full_lds_8192_2048_T9": _WIDE + (2048 * 8 + 5, 8),
    "tile2_first_8192_2049": (16000, 8192, 2049, 128, 50.0, 7600.0, "htk", "slaney", 2049 * 2 + 5, 2),     # T = 3
}
assert not set(CASES) & set(LIMIT_CASES)


def case_of(name):
    return CASES[name] if name in CASES else LIMIT_CASES[name]


def bank_of(case):
    """(sample_rate, n_fft, n_mels, f_min, f_max, mel_scale, mel_norm) of a case, f_max resolved: mel_weights64's arguments"""
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = case
    return (sr, n_fft, n_mels, f_min, sr / 2.0 if f_max is None else f_max, scale, norm)


def case_spec(name, log=False, bands_first=True, floor=FLOOR):
    from vorbispizza_amd import capi
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = case_of(name)
    return capi.LogMelSpec.make(sample_rate=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=f_min, f_max=f_max, mel_scale=scale, mel_norm=norm, log=log,
                                floor=floor, bands_first=bands_first)


def case_weights(name):
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = case_of(name)
    return mel_weights64(sr, n_fft, n_mels, f_min, sr / 2.0 if f_max is None else f_max, scale, norm)


_INPUTS = {}


def case_input(name):
    """(src float32, rows [(src offset, L, destination row)]) of a case: broadband noise of amplitude 0.05 .. 0.5, never under 1e-3 in
    magnitude, so that with the floor at 1e-10 the check's cap is a property of the input (test_melspec_cpu confirms it)"""
    if name in _INPUTS:
        return _INPUTS[name]
    sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = case_of(name)
    rng = np.random.default_rng(sum(name.encode()) * 1000 + hop)
    Ls = [F, F - 1, F - n_fft // 4, F // 3, 1, 0]
    gap = F // 5
    src = rng.standard_normal(2 * (len(Ls) - 1) * gap + F + 64) * 0.25
    src = (np.sign(src) * np.maximum(np.abs(src), 1e-3)).astype(np.float32)
    order = rng.permutation(DST_ROWS)[: len(Ls)]
    # (the rows share one source array at odd offsets, and overlap in it)
    rows = [(1 + 2 * i * gap, L, int(row)) for i, (L, row) in enumerate(zip(Ls, order))]
    assert all(a % 2 == 1 and a + L <= src.size for a, L, _ in rows)
    _INPUTS[name] = (src, rows)
    return _INPUTS[name]


_TRUTHS = {}


def case_truth(name):
    """[(M, e_M)] of a case's rows, computed once"""
    if name not in _TRUTHS:
        sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = case_of(name)
        src, rows = case_input(name)
        W = case_weights(name)
        _TRUTHS[name] = [melspec_truth(src[a: a + L], L, F, n_fft, hop, W) for a, L, _ in rows]
    return _TRUTHS[name]


_RESTATED = {}


def case_restated(name):
    """[acc32] of a case's rows, float32 [T, n_mels] each: restated_power32 with the library's bank for the case's spec, computed once"""
    if name not in _RESTATED:
        from vorbispizza_amd import capi
        sr, n_fft, hop, n_mels, f_min, f_max, scale, norm, F, tile = case_of(name)
        src, rows = case_input(name)
        first, count, weights = capi.melspec_filterbank(case_spec(name))
        _RESTATED[name] = [restated_power32(frames_of(src[a: a + L], L, F, n_fft, hop).astype(np.float32), n_fft, first, count, weights)
                           for a, L, _ in rows]
    return _RESTATED[name]
