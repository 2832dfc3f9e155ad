"""THE TRUTH of the MFCC tests (a helper, not a test): include/vorbispizza_pcm_mfcc.h's definition restated in float64 numpy on top of
tests/fbank_truth.py, written straight from its formulas and UNFOLDED -- the log of fbank_truth's band sums, an explicit DCT matrix, the
lifter as a separate multiply behind it, the energy from the scaled, centred frame, the cepstral mean as a plain float64 mean -- where the
library multiplies lifter and DCT into one float32 table and takes the energy from fl(x - mu).  tests/test_mfcc_cpu.py,
tests/test_pcm_mfcc_gpu.py and tests/test_multi_mfcc_gpu.py import it.  (torchaudio.compliance.kaldi.mfcc is the same arithmetic; it is
no dependency of this project.)

THE BOUND (u = 2^-24), from the float32 steps that remain in the kernel.  Nothing below is fitted to the kernel's output.
    the log-mel values   fbank_truth gives (M, e_M).  As check_log takes it, the kernel's E_f[b] lies between ln(max(M - e_M, floor)) and
                         ln(max(M + e_M, floor)), give or take logf's 4 u max(1, |E_f|).  With E = ln(max(M, floor)) and w the larger of
                         the two distances from E to those ends:  dE[b] = w + 4 u max(1, |E| + w)
    the cepstra          the table is C rounded once (1 u), the chain has N = n_mels fused steps (N u), 1 u for the terms of second order:
                             |c_f - c| <= sum_b |C| dE + (N + 2) u sum_b |C| (|E| + dE)
    the energy           a_f[m] = fl(x - mu_f) = (a + delta)(1 + eps), |delta| <= d_mu (fbank_truth's: (ceil(win / 4) + 4) u mean|x|, 0
                         without remove_dc), |eps| <= u, so sum a_f^2 differs from sum a^2 by at most
                             sum (2 |a| d_mu + d_mu^2) + 2 u sum (|a| + d_mu)^2.
                         Every term of the chains is >= 0, so their roundings are relative: ceil(win / 4) fused steps and two adds; the
                         factor fl(fl(scale) fl(scale)) has 3 u and the last multiply 1; 2 u for the second order:
                             e_S = scale^2 [sum (2 |a| d_mu + d_mu^2) + (ceil(win / 4) + 10) u sum (|a| + d_mu)^2]
                         taken through the log like the band sums: e_f lies between ln(max(S - e_S, 2^-23)) and ln(max(S + e_S, 2^-23)),
                         both raised to ln(energy_floor) where there is one, give or take 4 u max(1, |e_f|)
    the cepstral mean    with b[t] the bound of frame t's value v[t] and T_L frames: the float64 sum of the float32 values (at most
                         T_L / 64 + 7 additions of any one term, 2^-53 each, and the division), then one rounding to float32:
                             d_m = mean(b) + (T_L / 64 + 8) 2^-53 mean(|v| + b) + u (|m| + mean(b)),   all times (1 + 2 u)
                         and the subtraction's own rounding:  |out_f - out| <= b[t] + d_m + u (|out| + b[t] + d_m)"""
import math

import numpy as np

import fbank_truth as ft
from fbank_truth import U


def make(capi, **kw):
    d = spec_of(**kw)
    return capi.MfccSpec.make(**d), d


def refused_specs(capi):
    """(what, spec) for every limit of the definition: the mel stage's (fbank_truth's list, inside an MfccSpec) and its own"""
    from fbank_truth import refused_specs as fbank_refused
    out = []
    for what, fb in fbank_refused(capi):
        s = make(capi)[0]
        s.fbank = fb
        out.append(("fbank: " + what, s))
    power = make(capi)[0]
    power.fbank.output = capi.FBANK_POWER
    out.append(("output is not the log", power))
    for what, kw in (("n_ceps < 1", dict(n_ceps=0)), ("n_ceps > n_mels", dict(n_ceps=24)), ("n_ceps > n_mels at one band", dict(n_mels=1, n_ceps=2)),
                     ("lifter < 0", dict(lifter=-1.0)), ("lifter nan", dict(lifter=float("nan"))), ("lifter inf", dict(lifter=float("inf"))),
                     ("energy_floor < 0", dict(energy_floor=-1e-9)), ("energy_floor nan", dict(energy_floor=float("nan"))),
                     ("energy_floor inf", dict(energy_floor=float("inf")))):
        out.append((what, make(capi, **kw)[0]))
    for field in ("use_energy", "htk_compat", "subtract_mean"):
        for value in (2, -1):
            s = make(capi)[0]
            setattr(s, field, value)
            out.append((field, s))
    for i in (0, 11):
        s = make(capi)[0]
        s.reserved[i] = 1
        out.append(("a reserved word", s))
    return out


ENERGY_EPS = 2.0 ** -23
DEFAULTS = dict({k: v for k, v in ft.DEFAULTS.items() if k != "log"}, n_mels=23, n_ceps=13, lifter=22.0, use_energy=True, energy_floor=0.0,
                htk_compat=False, subtract_mean=False)


def spec_of(**kw):
    """a spec as a dict with every field of DEFAULTS"""
    assert set(kw) <= set(DEFAULTS), set(kw) - set(DEFAULTS)
    return dict(DEFAULTS, **kw)


def fbank_of(d):
    """the mel stage's spec, as fbank_truth takes it"""
    return ft.spec_of(log=True, **{k: d[k] for k in ft.DEFAULTS if k != "log"})


def dct64(n_ceps, N):
    """Kaldi's ComputeDctMatrix, float64 [n_ceps, N]"""
    b = np.arange(N, dtype=np.float64)
    D = np.sqrt(2.0 / N) * np.cos(np.pi * np.arange(n_ceps, dtype=np.float64)[:, None] * (b[None, :] + 0.5) / N)
    D[0] = math.sqrt(1.0 / N)
    return D


def lifter64(n_ceps, Q):
    i = np.arange(n_ceps, dtype=np.float64)
    return 1.0 + 0.5 * Q * np.sin(np.pi * i / Q) if Q > 0 else np.ones(n_ceps)


def stored_order(d):
    """the coefficient a frame's j-th stored value holds"""
    n = d["n_ceps"]
    return list(range(1, n)) + [0] if d["htk_compat"] else list(range(n))


def matrix64(d):
    """C in the order of the coefficients (not the stored one), float64 [n_ceps, n_mels]: the DCT, then the lifter, then HTK's sqrt(2)"""
    C = dct64(d["n_ceps"], d["n_mels"])
    C = lifter64(d["n_ceps"], float(d["lifter"]))[:, None] * C
    if d["htk_compat"] and not d["use_energy"]:
        C[0] = C[0] * math.sqrt(2.0)
    return C


def log_interval(S, e_S, floor):
    """(value, half-width) of logf(max(S_f, floor)) for S_f within e_S of S"""
    v = np.log(np.maximum(S, floor))
    w = np.maximum(np.log(np.maximum(S + e_S, floor)) - v, v - np.log(np.maximum(S - e_S, floor)))
    return v, w + 4 * U * np.maximum(1.0, np.abs(v) + w)


def energy_truth(x, d):
    """(e, bound), float64 [T_L], of one row's real samples: the log energy of item 3"""
    win, hop, scale = d["win"], d["hop"], float(d["scale"])
    X = ft.frames_of(x, win, hop)
    mu = X.mean(axis=1, keepdims=True) if d["remove_dc"] else np.zeros((X.shape[0], 1))
    Y = scale * X
    if d["remove_dc"]:
        Y = Y - Y.mean(axis=1, keepdims=True)
    S = (Y * Y).sum(axis=1)
    A = np.abs(X - mu)
    q = -(-win // 4)
    d_mu = (q + 4) * U * np.abs(X).mean(axis=1, keepdims=True) if d["remove_dc"] else np.zeros((X.shape[0], 1))
    e_S = scale * scale * ((2 * A * d_mu + d_mu ** 2).sum(axis=1) + (q + 10) * U * ((A + d_mu) ** 2).sum(axis=1))
    ef = float(np.float32(d["energy_floor"]))
    lo = max(ENERGY_EPS, ef) if ef > 0 else ENERGY_EPS  # (ln is monotone: a floor under the log's value is a floor under its argument)
    return log_interval(S, e_S, lo)


def mfcc_truth(x, d, W=None, B=None):
    """(V, b), float64 [T_L, n_ceps] in the STORED order, of one row's real samples x (float32 values), without the cepstral mean: the
    values and their bounds"""
    fb = fbank_of(d)
    M, e_M = ft.fbank_truth(x, fb, W, B)
    E, dE = log_interval(M, e_M, float(np.float32(d["floor"])))
    N = d["n_mels"]
    D, l = dct64(d["n_ceps"], N), lifter64(d["n_ceps"], float(d["lifter"]))
    c = (E @ D.T) * l[None, :]
    Ca = np.abs(D) * np.abs(l)[:, None]
    if d["htk_compat"] and not d["use_energy"]:
        c[:, 0] *= math.sqrt(2.0)
        Ca[0] *= math.sqrt(2.0)
    b = dE @ Ca.T + (N + 2) * U * ((np.abs(E) + dE) @ Ca.T)
    if d["use_energy"]:
        c[:, 0], b[:, 0] = energy_truth(x, d)
    order = stored_order(d)
    return c[:, order], b[:, order]


def cmn_truth(V, b):
    """item 5 on (V, b) of mfcc_truth: (out, bound)"""
    TL = V.shape[0]
    if TL == 0:
        return V, b
    m, mb = V.mean(axis=0, keepdims=True), b.mean(axis=0, keepdims=True)
    d_m = (mb + (TL // 64 + 8) * 2.0 ** -53 * (np.abs(V) + b).mean(axis=0, keepdims=True) + U * (np.abs(m) + mb)) * (1 + 2 * U)
    out = V - m
    return out, b + d_m + U * (np.abs(out) + b + d_m)


def row_truth(x, d, W=None, B=None):
    """(values, bounds) of a row's real frames, the cepstral mean included where the spec asks for it"""
    V, b = mfcc_truth(x, d, W, B)
    return cmn_truth(V, b) if d["subtract_mean"] else (V, b)


def check_row(got, x, d, W=None, B=None):
    """a whole row [T, n_ceps] of the tensor against the truth of its real samples x: the real frames inside the bound, every element
    behind them pad_value bit for bit.  Returns the largest error / bound ratio."""
    V, b = row_truth(x, d, W, B)
    got = np.asarray(got, dtype=np.float32)
    TL = V.shape[0]
    assert got.shape[0] >= TL and got.shape[1] == d["n_ceps"], (got.shape, V.shape)
    assert (got[TL:].view(np.uint32) == np.float32(d["pad_value"]).view(np.uint32)).all()
    if TL == 0:
        return 0.0
    err = np.abs(got[:TL].astype(np.float64) - V)
    assert np.isfinite(got[:TL]).all() and (b > 0).all()
    ratio = float((err / b).max())
    assert ratio <= 1.0, ratio
    return ratio


# ---- the launch plan of vpz_pcm_mfcc, restated
def mfcc_lds_plan(win, hop, n_fft, n_mels, Tt, k):
    """(floats of the launch's LDS, estride): fbank's span and power tile, the means and the energies (kFbMeans each), and the log-mel
    tile [Tt][n_mels | 1] behind the power tile -- room of its own"""
    span_cap, pstride = ft.lds_plan(win, hop, n_fft, Tt)
    estride = n_mels | 1
    return span_cap + 2 * k["kFbMeans"] + Tt * pstride + Tt * estride, estride


def tile_plan(win, hop, n_fft, n_mels, T, n_rows, num_cu, k):
    """vpz_pcm_mfcc's tile choice: vpz_pcm_fbank's rule over mfcc_lds_plan -> (frames of a tile, LDS floats); (0, None): none fits"""
    few = ((T + 63) // 64) * n_rows < 2 * num_cu
    for Tt in (64, 32, 16):
        total, _ = mfcc_lds_plan(win, hop, n_fft, n_mels, Tt, k)
        if (Tt == 64 and (T <= 32 or few)) or (Tt == 32 and T <= 16) or total > k["kFbLdsFloats"]:
            continue
        return Tt, total
    return 0, None
