"""THE TRUTH of the fbank tests (a helper, not a test): include/vorbispizza_pcm_fbank.h's definition restated in float64 numpy, written
straight from its formulas and UNFOLDED -- scale, mean, pre-emphasis, window, zero padding, numpy.fft.rfft, power, a dense W, log -- where
the library folds steps 1, 3, 4 and 5 into one table.  tests/test_fbank_cpu.py, tests/test_pcm_fbank_gpu.py and
tests/test_multi_fbank_gpu.py import it.  (torchaudio.compliance.kaldi.fbank is the same arithmetic; it is no dependency of this project.)

THE BOUND (u = 2^-24), from the float32 steps that remain in the kernel.  With a[m] = x[m] - mu the exact centred frame, B the folded
operator in float64 (operator64: the unfolded steps applied to unit impulses) and K = 2 ceil(win / 2) the length of the fmaf chain:
    the mean         four chains of at most ceil(win / 4) adds, two adds, one division:  |mu_f - mu| <= d_mu = (ceil(win / 4) + 4) u mean|x|
                     (0 without remove_dc).  It enters every sample of the frame, and every sample ALIKE: the A operand is
                     fl(x - mu_f) = (a[m] + delta)(1 + eps_m) with one delta = mu - mu_f for the frame and |eps_m| <= u, so
                     sum_m fl(x - mu_f) B = re + delta sum_m B[m][k] + sum_m eps_m (a + delta) B
    the chain        d_re[k] = d_mu |sum_m B_cos[m][k]| + (K + 4) u sum_m (|a| + d_mu) |B_cos|
                     (the subtraction's rounding 1, the table's 1, the chain's K, 2 for the terms of second order); d_im likewise with B_sin
    squaring         e_P[k] = 2 |re| d_re + 2 |im| d_im + d_re^2 + d_im^2 + 3 u P
    the bank         e_M[b] = sum_k W[b][k] e_P[k] + (Bmost + 2) u M[b]       Bmost: the largest live-bin count of a band
all evaluated in float64 on the same input.  After the log the bound is relative: the output lies between ln(max(M - e_M, floor)) and
ln(max(M + e_M, floor)), 4 u max(1, |ln|) allowed for logf; where M - e_M > floor that is e_M / (M - e_M) around ln M (check_log)."""
import math

import numpy as np
from kernel_text import constants_of


def make(capi, **kw):
    d = spec_of(**kw)
    return capi.FbankSpec.make(**d), d


def refused_specs(capi):
    """(what, spec) for every limit of the definition"""
    cases = [("n_fft odd", dict(n_fft=513)), ("n_fft < 32", dict(n_fft=30, win=20, hop=10)), ("n_fft > 1024", dict(n_fft=1026)), ("win < 2", dict(win=1, hop=1)),
             ("win > n_fft", dict(win=513)), ("hop < 1", dict(hop=0)), ("hop > win", dict(hop=401)), ("n_mels < 1", dict(n_mels=0)),
             ("n_mels > 256", dict(n_mels=257)), ("low_freq < 0", dict(low_freq=-1.0)), ("low_freq == high", dict(low_freq=8000.0)),
             ("low_freq > high", dict(low_freq=5000.0, high_freq=4000.0)), ("high > nyquist", dict(high_freq=8000.5)),
             ("high offset below low_freq", dict(high_freq=-7990.0)), ("high_freq nan", dict(high_freq=float("nan"))),
             ("low_freq nan", dict(low_freq=float("nan"))), ("sample_rate 0", dict(sample_rate=0)), ("sample_rate inf", dict(sample_rate=float("inf"))),
             ("preemphasis < 0", dict(preemphasis=-0.01)), ("preemphasis > 1", dict(preemphasis=1.01)), ("preemphasis nan", dict(preemphasis=float("nan"))),
             ("scale 0", dict(scale=0.0)), ("scale inf", dict(scale=float("inf"))), ("scale nan", dict(scale=float("nan"))),
             ("scale underflows float32", dict(scale=1e-60)), ("pad_value inf", dict(pad_value=float("-inf"))), ("pad_value nan", dict(pad_value=float("nan"))),
             ("floor 0", dict(floor=0.0)), ("floor < 0", dict(floor=-1.0)), ("floor underflows float32", dict(floor=1e-60)), ("floor nan", dict(floor=float("nan")))]
    out = [(what, make(capi, **kw)[0]) for what, kw in cases]
    for field, value in (("window", 3), ("window", -1), ("remove_dc", 2), ("output", 2), ("layout", 2)):
        s = make(capi)[0]
        setattr(s, field, value)
        out.append((field, s))
    for i in (0, 9):
        s = make(capi)[0]
        s.reserved[i] = 1
        out.append(("a reserved word", s))
    return out


U = 2.0 ** -24
FLT_EPSILON = 2.0 ** -23
WINDOWS = ("hanning", "hamming", "povey")
DEFAULTS = dict(sample_rate=16000, win=400, hop=160, n_fft=512, n_mels=80, low_freq=20.0, high_freq=0.0, preemphasis=0.97, window="povey",
                remove_dc=True, scale=32768.0, log=True, floor=FLT_EPSILON, pad_value=0.0, frames_first=True)


def spec_of(**kw):
    """a spec as a dict with every field of DEFAULTS"""
    assert set(kw) <= set(DEFAULTS), set(kw) - set(DEFAULTS)
    return dict(DEFAULTS, **kw)


def window64(name, win):
    a = 2.0 * np.pi * np.arange(win, dtype=np.float64) / (win - 1)
    if name == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    hann = 0.5 - 0.5 * np.cos(a)
    return hann ** 0.85 if name == "povey" else hann


def n_frames(length, win, hop):
    """T of a padded length, T_L of a row's own length"""
    return 0 if length < win else 1 + (length - win) // hop


def frames_of(x, win, hop):
    """float64 [T_L, win]: frame t is x[t * hop : t * hop + win]"""
    x = np.asarray(x, dtype=np.float64)
    T = n_frames(x.size, win, hop)
    return np.stack([x[t * hop: t * hop + win] for t in range(T)]) if T else np.zeros((0, win))


def spectrum64(Y, spec):
    """steps 3, 4 and 5 of the definition on frames Y [.., win] that steps 1 and 2 have been applied to: (re, im), float64 [.., n_fft / 2]"""
    c, win, n_fft = float(spec["preemphasis"]), spec["win"], spec["n_fft"]
    Z = np.empty_like(Y)
    Z[..., 0] = Y[..., 0] - c * Y[..., 0]
    Z[..., 1:] = Y[..., 1:] - c * Y[..., :-1]
    V = np.zeros(Y.shape[:-1] + (n_fft,))
    V[..., :win] = Z * window64(spec["window"], win)
    S = np.fft.rfft(V, axis=-1)[..., : n_fft // 2]  # (the Nyquist bin is not computed)
    return S.real, -S.imag


def operator64(spec):
    """(B_cos, B_sin), float64 [win, n_fft / 2]: steps 1, 3, 4 and 5 applied to the win unit impulses -- what the library's table folds"""
    return spectrum64(float(spec["scale"]) * np.eye(spec["win"]), spec)


def mel64(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_weights64(spec):
    """W, float64 [n_mels, n_fft / 2]"""
    sr, n_fft, n = float(spec["sample_rate"]), spec["n_fft"], spec["n_mels"]
    high = spec["high_freq"] if spec["high_freq"] > 0 else sr / 2 + spec["high_freq"]
    lo, hi = float(mel64(spec["low_freq"])), float(mel64(high))
    d = (hi - lo) / (n + 1)
    left = lo + np.arange(n, dtype=np.float64) * d
    mk = mel64(np.arange(n_fft // 2, dtype=np.float64) * sr / n_fft)
    return np.maximum(0.0, np.minimum((mk[None, :] - left[:, None]) / d, (left[:, None] + 2 * d - mk[None, :]) / d))


def fbank_truth(x, spec, W=None, B=None):
    """(M, e_M), float64 [T_L, n_mels], of one row's real samples x (float32 values): its real frames only"""
    win, hop = spec["win"], spec["hop"]
    W = mel_weights64(spec) if W is None else W
    X = frames_of(x, win, hop)
    mu = X.mean(axis=1, keepdims=True) if spec["remove_dc"] else np.zeros((X.shape[0], 1))
    Y = float(spec["scale"]) * X
    if spec["remove_dc"]:
        Y = Y - Y.mean(axis=1, keepdims=True)
    re, im = spectrum64(Y, spec)
    P = re * re + im * im
    M = P @ W.T
    # the bound
    Bc, Bs = operator64(spec) if B is None else B
    A = np.abs(X - mu)
    d_mu = (-(-win // 4) + 4) * U * np.abs(X).mean(axis=1, keepdims=True) if spec["remove_dc"] else np.zeros((X.shape[0], 1))
    K = 2 * ((win + 1) // 2)
    d_re = d_mu * np.abs(Bc.sum(axis=0))[None, :] + (K + 4) * U * ((A + d_mu) @ np.abs(Bc))
    d_im = d_mu * np.abs(Bs.sum(axis=0))[None, :] + (K + 4) * U * ((A + d_mu) @ np.abs(Bs))
    e_P = 2 * np.abs(re) * d_re + 2 * np.abs(im) * d_im + d_re ** 2 + d_im ** 2 + 3 * U * P
    most = int((W > 0).sum(axis=1).max())
    return M, e_P @ W.T + (most + 2) * U * M


def log_floor(floor):
    """logf(floor): the float32 nearest to the natural logarithm of the float32 floor"""
    return np.float32(math.log(float(np.float32(floor))))


def check_power(got, M, e_M):
    """within e_M of the truth, exactly 0 where e_M is 0.  Returns the largest error / bound ratio."""
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == M.shape, (got.shape, M.shape)
    err = np.abs(got.astype(np.float64) - M)
    assert (err <= e_M).all(), float((err[e_M > 0] / e_M[e_M > 0]).max())
    assert (got[e_M == 0].view(np.uint32) == 0).all()
    return float((err[e_M > 0] / e_M[e_M > 0]).max()) if (e_M > 0).any() else 0.0


def check_log(got, M, e_M, floor):
    """the log mode's rule, for every element: ln is monotone and the kernel's band sum lies within e_M of M, so the output lies between
    ln(max(M - e_M, floor)) and ln(max(M + e_M, floor)), give or take logf's own 4 u max(1, |value|); where M + e_M < floor it is logf(floor)'s
    bits.  Returns the largest error / bound ratio over the elements with M - e_M > floor, where the bound around ln M is e_M / (M - e_M)."""
    floor = float(np.float32(floor))
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == M.shape, (got.shape, M.shape)
    g = got.astype(np.float64)
    slack = 4 * U * np.maximum(1.0, np.abs(g))
    assert (g >= np.log(np.maximum(M - e_M, floor)) - slack).all() and (g <= np.log(np.maximum(M + e_M, floor)) + slack).all()
    above, below = M - e_M > floor, M + e_M < floor
    assert (got[below].view(np.uint32) == log_floor(floor).view(np.uint32)).all()
    tol = e_M[above] / (M[above] - e_M[above]) + slack[above]
    err = np.abs(g[above] - np.log(M[above]))
    assert (err <= tol).all(), float((err / tol).max())
    return float((err / tol).max()) if above.any() else 0.0


def check_row(got, x, spec, W=None, B=None):
    """a whole row [T, n_mels] of the tensor against the truth of its real samples x: the real frames inside the bound, every element
    behind them pad_value bit for bit.  Returns the largest error / bound ratio."""
    M, e_M = fbank_truth(x, spec, W, B)
    got = np.asarray(got, dtype=np.float32)
    TL = M.shape[0]
    assert got.shape[0] >= TL and got.shape[1] == spec["n_mels"]
    assert (got[TL:].view(np.uint32) == np.float32(spec["pad_value"]).view(np.uint32)).all()
    if TL == 0:
        return 0.0
    return check_log(got[:TL], M, e_M, spec["floor"]) if spec["log"] else check_power(got[:TL], M, e_M)


# ---- the launch plan of vpz_pcm_fbank, restated
# kFbLdsFloats, kFbAhead, kFbCols, kFbMaxGridY, kFbMeans as csrc/pcm_fbank.hip states them
kernel_constants = constants_of("pcm_fbank.hip", ("kFbLdsFloats", "kFbAhead", "kFbCols", "kFbMaxGridY", "kFbMeans"))


def lds_plan(win, hop, n_fft, Tt):
    """(span_cap, pstride) of a tile of Tt frames: the floats of the skewed span, the floats between two rows of the power tile"""
    count = (Tt - 1) * hop + win
    return count + (count // hop if hop % 2 == 0 else 0) + 1, (n_fft // 2) | 1


def tile_plan(win, hop, n_fft, T, n_rows, num_cu, k):
    """vpz_pcm_fbank's tile choice: (frames of a tile, LDS floats the launch asks for); (0, None) where no tile fits.  64 frames where the
    row has more than 32, the launch gives every CU two workgroups at that size and the LDS holds them; else 32 where the row has more
    than 16 and the LDS holds them; else 16"""
    few = ((T + 63) // 64) * n_rows < 2 * num_cu
    for Tt in (64, 32, 16):
        span_cap, pstride = lds_plan(win, hop, n_fft, Tt)
        total = span_cap + k["kFbMeans"] + Tt * pstride
        if (Tt == 64 and (T <= 32 or few)) or (Tt == 32 and T <= 16) or total > k["kFbLdsFloats"]:
            continue
        return Tt, total
    return 0, None
