"""Log-mel's float64 truth, shared by the CPU and GPU tests of vpz_pcm_logmel and by melspec_truth, stft_truth and mfcc_truth: frames_of,
extend, the DFT and mel weights in float64, the power and log checks with their bounds, the silence value, the refused specs, and the
kernel's tile and LDS plan restated from the constants csrc/pcm_logmel.hip states, with the limit cases built on it."""
import ctypes as C
import math
import os
import re

import numpy as np

from f32_model import U
from kernel_text import constants_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}


# ---- the float64 restatement
def dft64(n_fft):
    """(cos, sin), float64 [n_fft, n_fft / 2 + 1]: w[m] cos(2 pi (m k mod n_fft) / n_fft) and the same with sin, w the periodic Hann window"""
    m = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * m / n_fft)
    a = 2.0 * np.pi * ((m * k) % n_fft).astype(np.float64) / n_fft
    return w * np.cos(a), w * np.sin(a)


def hz_to_mel(f, scale):
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def mel_to_hz(m, scale):
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)))


def mel_points(sample_rate, n_mels, f_min, f_max, scale):
    lo, hi = float(hz_to_mel(f_min, scale)), float(hz_to_mel(f_max, scale))
    return mel_to_hz(lo + (hi - lo) * np.arange(n_mels + 2, dtype=np.float64) / (n_mels + 1), scale)


def mel_weights64(sample_rate, n_fft, n_mels, f_min, f_max, scale, norm):
    """W, float64 [n_mels, n_fft / 2 + 1]"""
    pts = mel_points(sample_rate, n_mels, f_min, f_max, scale)
    fk = np.arange(n_fft // 2 + 1, dtype=np.float64) * sample_rate / n_fft
    up = (fk[None, :] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
    down = (pts[2:, None] - fk[None, :]) / (pts[2:] - pts[1:-1])[:, None]
    W = np.maximum(0.0, np.minimum(up, down))
    if norm == "slaney":
        W = W * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return W


def extend(x, L, F, n_fft):
    """the definition's signal of a row: x[0..L), zeros up to F, reflected by n_fft / 2 at both ends without repeating the edge sample"""
    row = np.zeros(F, dtype=np.float64)
    row[:L] = np.asarray(x[:L], dtype=np.float64)
    h = n_fft // 2
    return np.concatenate([row[1:h + 1][::-1], row, row[F - 1 - h:F - 1][::-1]])


def frames_of(x, L, F, n_fft, hop):
    """X, float64 [T, n_fft]: frame t is the extended signal from t * hop (= x[t * hop - n_fft / 2 ...])"""
    e = extend(x, L, F, n_fft)
    T = 1 + F // hop
    return np.stack([e[t * hop: t * hop + n_fft] for t in range(T)])


def power_truth(X, n_fft):
    """(P, e_P), float64 [T, n_fft / 2 + 1], of frames X"""
    cos, sin = dft64(n_fft)
    re, im = X @ cos, X @ sin
    d_re, d_im = (n_fft + 2) * U * (np.abs(X) @ np.abs(cos)), (n_fft + 2) * U * (np.abs(X) @ np.abs(sin))
    P = re * re + im * im
    return P, 2 * np.abs(re) * d_re + 2 * np.abs(im) * d_im + d_re ** 2 + d_im ** 2 + 3 * U * P


def logmel_truth(x, L, F, n_fft, hop, W):
    """(M, e_M), float64 [T, n_mels], of one row"""
    P, e_P = power_truth(frames_of(x, L, F, n_fft, hop), n_fft)
    B = int((W > 0).sum(axis=1).max())
    M = P @ W.T
    return M, e_P @ W.T + (B + 2) * U * M


def silence_value(floor):
    """log10f(floor): the float32 nearest to the decimal logarithm of the float32 floor"""
    return np.float32(math.log10(float(np.float32(floor))))


def check_log(got, M, e_M, floor):
    """the log10 mode's rule: bound where M - e_M > floor, the silence value's bits where M + e_M < floor, at most 1 % between the two.
    Returns the largest error / bound ratio."""
    floor = float(np.float32(floor))
    got = np.asarray(got, dtype=np.float32)
    above, below = M - e_M > floor, M + e_M < floor
    assert (~(above | below)).sum() <= 0.01 * M.size, (int((~(above | below)).sum()), M.size)
    assert (got[below].view(np.uint32) == silence_value(floor).view(np.uint32)).all()
    want = np.log10(M[above])
    tol = e_M[above] / ((M[above] - e_M[above]) * math.log(10.0)) + 4 * U * np.maximum(1.0, np.abs(got[above].astype(np.float64)))
    err = np.abs(got[above].astype(np.float64) - want)
    assert (err <= tol).all(), float((err / tol).max())
    return float((err / tol).max()) if above.any() else 0.0


def check_power(got, M, e_M):
    """within e_M of the truth, exactly 0 where e_M is 0.  Returns the largest error / bound ratio."""
    got = np.asarray(got, dtype=np.float32)
    err = np.abs(got.astype(np.float64) - M)
    assert (err <= e_M).all(), float((err[e_M > 0] / e_M[e_M > 0]).max())
    assert (got[e_M == 0].view(np.uint32) == 0).all()
    return float((err[e_M > 0] / e_M[e_M > 0]).max()) if (e_M > 0).any() else 0.0


# ---- the launch plan, restated, and the case list of tests/test_pcm_logmel_limits_gpu.py
# kLmLdsFloats, kLmAhead, kLmCols, kLmMaxGridY as csrc/pcm_logmel.hip states them
logmel_kernel_constants = constants_of("pcm_logmel.hip", ("kLmLdsFloats", "kLmAhead", "kLmCols", "kLmMaxGridY"))


def lds_plan(n_fft, hop, Tt):
    """(span_cap, pstride) of a tile of Tt frames: the floats of the skewed span, the floats between two rows of the power tile"""
    count = (Tt - 1) * hop + n_fft
    return count + (count // hop if hop % 2 == 0 else 0) + 1, (n_fft // 2 + 1) | 1


def tile_plan(n_fft, hop, T, n_rows, num_cu, k=None):
    """vpz_pcm_logmel's tile choice, restated: (frames of a tile, LDS floats the launch asks for); (0, None) where no tile fits.  64
    frames where the row has more than 32, the launch gives every CU two workgroups at that size and the LDS holds them, else 32, else 16"""
    k = k or logmel_kernel_constants()
    few = ((T + 63) // 64) * n_rows < 2 * num_cu
    for Tt in (64, 32, 16):
        span_cap, pstride = lds_plan(n_fft, hop, Tt)
        if (Tt == 64 and (T <= 32 or few)) or span_cap + Tt * pstride > k["kLmLdsFloats"]:
            continue
        return Tt, span_cap + Tt * pstride
    return 0, None


def crowd_rows(num_cu):
    """the rows of a launch that takes 64-frame tiles where a row has two of them: one more than gives every CU two workgroups"""
    return -(-2 * num_cu // 2) + 1


def limit_frames(hop, T):
    """F with 1 + F // hop = T and a remainder (an odd F where hop allows)"""
    return hop * (T - 1) + min(hop - 1, 5)


# tests/test_pcm_logmel_limits_gpu.py runs every case; test_the_limit_cases_take_the_tiles_they_are_meant_to holds the lists to the plan.
# (n_fft, hop, T, n_mels, the tile a SMALL launch -- five rows -- takes); F = limit_frames(hop, T).  T is never a multiple of 32.
LIMIT_TAIL = [(34, 5, 71, 6, 32), (36, 6, 71, 6, 32), (38, 38, 41, 6, 32), (1022, 1022, 19, 40, 16)]   # pairs % 4 = 1, 2, 3, 3
LIMIT_LDS = [(1024, 112, 71, 40, 32), (1024, 113, 71, 40, 32), (1024, 757, 41, 40, 32), (1024, 758, 41, 40, 16)]
LIMIT_GROUPS = [(62, 15, 71, 10, 32), (62, 16, 71, 10, 32), (126, 31, 71, 20, 32), (126, 32, 71, 20, 32), (254, 63, 71, 32, 32), (254, 64, 71, 32, 32),
                (256, 65, 71, 32, 32), (256, 64, 71, 32, 32)]
# ((1024, 2) with F = 600 exactly)
LIMIT_HOPS = [(32, 2, 71, 6, 32), (1024, 2, 301, 40, 32), (64, 4, 71, 10, 32), (32, 32, 41, 6, 32), (64, 63, 41, 10, 32), (32, 31, 41, 6, 32)]
# launches of crowd_rows(CUs) rows with T = 104: 64-frame tiles, the last one of 40 frames; (n_fft, hop, n_mels)
LIMIT_CROWDS = [(1024, 110, 40), (1024, 111, 40), (1022, 110, 40), (38, 4, 6), (256, 64, 32)]
CROWD_T = 104


def limit_F(case):
    n_fft, hop, T = case[:3]
    return 600 if (n_fft, hop) == (1024, 2) else limit_frames(hop, T)


def refused_specs(capi):
    """(what, spec) for every limit of the definition"""
    good = dict(sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=8000.0)
    cases = [("n_fft odd", dict(n_fft=401)), ("n_fft < 32", dict(n_fft=30, hop=10)), ("n_fft > 1024", dict(n_fft=1026)), ("hop < 1", dict(hop=0)),
             ("hop > n_fft", dict(hop=401)), ("n_mels < 1", dict(n_mels=0)), ("n_mels > 256", dict(n_mels=257)), ("f_min < 0", dict(f_min=-1.0)),
             ("f_min == f_max", dict(f_min=8000.0)), ("f_min > f_max", dict(f_min=5000.0, f_max=4000.0)), ("f_max > nyquist", dict(f_max=8000.5)),
             ("f_max nan", dict(f_max=float("nan"))), ("sample_rate 0", dict(sample_rate=0, f_max=0.0)), ("floor 0", dict(floor=0.0)),
             ("floor < 0", dict(floor=-1.0)), ("floor underflows float32", dict(floor=1e-60)), ("floor nan", dict(floor=float("nan")))]
    out = [(what, capi.LogMelSpec.make(**dict(good, **kw))) for what, kw in cases]
    for field, value in (("mel_scale", 2), ("mel_norm", -1), ("output", 2), ("layout", 2)):
        s = capi.LogMelSpec.make(**good)
        setattr(s, field, value)
        out.append((field, s))
    s = capi.LogMelSpec.make(**good)
    s.reserved[8] = 1
    out.append(("a reserved word", s))
    return out
