"""THE TRUTH of the feature post-processing tests (a helper, not a test): include/vorbispizza_pcm_featpost.h's definition restated in
numpy.longdouble, written straight from its formulas -- the delta scales by repeated convolution, a delta as the direct sum over its taps
with those scales, a window's S1 and S2 as direct sums over [a, b) -- where the library rounds the scales to float32, runs a fused float32
chain and adds float64 chunk sums in a stated order.  tests/test_featpost_cpu.py, tests/test_pcm_featpost_gpu.py and
tests/test_multi_featpost_gpu.py import it.  (Kaldi's add-deltas / apply-cmvn / apply-cmvn-sliding are the same arithmetic; neither
Kaldi nor torchaudio is a dependency of this project.)

THE BOUNDS, per element (u = 2^-24, v = 2^-53, tiny = 2^-149 for a result below float32's normal range).  Nothing is fitted to the
library's output; x is float32 and exact.
    deltas      block i has K = 2 i w + 1 taps.  The scale is rounded once (u), the chain has at most K fused steps (K u), 1 u for the terms
                of second order:        |d_f - d| <= (K + 2) u sum_j |s_j x_j| + K tiny.      Block 0 is a copy: the bound is 0.
    mean only   S1 is a float64 sum of c exact terms: at most c - 1 roundings touch any one term, whatever the order, then the division:
                |m_f - m| <= dm = (c + 1) v (sum over the window of |x|) / c.  The subtraction rounds once in float64, the result once to
                float32:               |out_f - out| <= u |out| + dm + v (|out| + dm), all times (1 + 2 u), + tiny
    variance    S2's terms are exact squares >= 0, so its c roundings are relative; S2 / c, the fused -m m + S2 / c and the square of the
                computed mean:          dv = (c + 4) v (S2 / c + m^2) + 2 |m| dm + dm^2
                The floor is 1-Lipschitz, so the floored variance V_f lies in [V_lo, V_hi] = [max(V - dv, floor), V + dv].  With
                xd = x - m and dx = dm + v (|xd| + dm) the quotient before its own roundings differs from q = xd / sqrt(V) by at most
                    e_q = dx / sqrt(V_lo) + |xd| (1 / sqrt(V_lo) - 1 / sqrt(V))
                (the lower end is the farther one: 1 / sqrt is convex), which is |out| dv / (2 V) to first order.  Square root, division
                and the float32 rounding:   |out_f - out| <= e_q + (u + 3 v)(|q| + e_q), all times (1 + 2 u), + tiny
                c == 1: out is 0 and the library's x - m is exactly 0: the bound is 0."""
from fractions import Fraction

import numpy as np


def make(capi, **kw):
    d = spec_of(**kw)
    return capi.FeatPostSpec.make(**d), d


# ---- the window
NS = (1, 2, 99, 100, 101, 600, 601, 602, 1300)


# ---- limits, refusals, the scratch size
def refused_specs(capi):
    """(what, spec) for every limit of the definition"""
    out = []
    base = dict(norm="sliding", delta_order=2)
    for what, kw in (("cmn_window < 1", dict(cmn_window=0, min_window=0)), ("cmn_window > 2^20", dict(cmn_window=(1 << 20) + 1)),
                     ("min_window < 1", dict(min_window=0)), ("min_window > cmn_window", dict(cmn_window=50, min_window=51)),
                     ("delta_order < 0", dict(delta_order=-1)), ("delta_order > 3", dict(delta_order=4)),
                     ("delta_window < 1", dict(delta_window=0)), ("delta_window > 8", dict(delta_window=9)),
                     ("var_floor 0", dict(var_floor=0.0)), ("var_floor < 0", dict(var_floor=-1e-10)), ("var_floor nan", dict(var_floor=float("nan"))),
                     ("var_floor inf", dict(var_floor=float("inf"))), ("pad_value nan", dict(pad_value=float("nan"))),
                     ("pad_value inf", dict(pad_value=float("-inf"))), ("a spec that does nothing", dict(norm="none", delta_order=0))):
        out.append((what, make(capi, **dict(base, **kw))[0]))
    for field, values in (("norm", (-1, 3)), ("norm_vars", (-1, 2)), ("center", (-1, 2)), ("order", (-1, 2)), ("layout", (-1, 2))):
        for value in values:
            s = make(capi, **base)[0]
            setattr(s, field, value)
            out.append((field, s))
    for i in (0, 10):
        s = make(capi, **base)[0]
        s.reserved[i] = 1
        out.append(("a reserved word", s))
    return out


LD =np.longdouble
U = LD(2.0) ** -24
V = LD(2.0) ** -53
TINY = LD(2.0) ** -149
CHUNK = 64

DEFAULTS = dict(norm="none", norm_vars=False, center=False, cmn_window=600, min_window=100, var_floor=1e-10, delta_order=0, delta_window=2,
                deltas_first=False, pad_value=0.0, frames_first=True)


def spec_of(**kw):
    """a spec as a dict with every field of DEFAULTS (the names of capi.FeatPostSpec.make)"""
    assert set(kw) <= set(DEFAULTS), set(kw) - set(DEFAULTS)
    return dict(DEFAULTS, **kw)


def scales(i, w):
    """s_i as longdouble [2 i w + 1]: s_0 = [1], s_i = s_(i-1) convolved with j / sum j^2, j = -w .. w -- in exact fractions (a tap that is
    0 is 0), each divided once"""
    Z = sum(j * j for j in range(-w, w + 1))
    s = [Fraction(1)]
    for _ in range(i):
        nxt = [Fraction(0)] * (len(s) + 2 * w)
        for k, v in enumerate(s):
            for j in range(-w, w + 1):
                nxt[k + j + w] += v * Fraction(j, Z)
        s = nxt
    return np.array([LD(f.numerator) / LD(f.denominator) for f in s], dtype=LD)


def window(d, t, n):
    """[a, b) of frame t of a row of n real frames: the header's item 2, in Python integers"""
    if d["norm"] == "row":
        return 0, n
    W, center = d["cmn_window"], d["center"]
    if center:
        a = t - W // 2
        b = a + W
    else:
        a, b = t - W, t + 1
    if a < 0:
        b -= a
        a = 0
    if not center:
        b = max(t + 1, d["min_window"])
    if b > n:
        a -= b - n
        b = n
        a = max(a, 0)
    return a, b


def deltas(x, d):
    """x: float32 [n, D] -> (truth longdouble [n, D_out], bound longdouble [n, D_out])"""
    n, D = x.shape
    order, w = d["delta_order"], d["delta_window"]
    xl = x.astype(LD)
    out, bound = [xl], [np.zeros((n, D), dtype=LD)]
    t = np.arange(n)
    for i in range(1, order + 1):
        s, H = scales(i, w), i * w
        acc, mag = np.zeros((n, D), dtype=LD), np.zeros((n, D), dtype=LD)
        for j in range(-H, H + 1):
            term = s[j + H] * xl[np.clip(t + j, 0, n - 1)] if n else xl
            acc, mag = acc + term, mag + np.abs(term)
        K = 2 * H + 1
        out.append(acc)
        bound.append((K + 2) * U * mag + K * TINY)
    return np.concatenate(out, axis=1), np.concatenate(bound, axis=1)


def normalise(x, d):
    """x: float32 [n, D] -> (truth longdouble [n, D], bound longdouble [n, D]) of the normalisation alone"""
    n, D = x.shape
    xl = x.astype(LD)
    out, bound = np.zeros((n, D), dtype=LD), np.zeros((n, D), dtype=LD)
    floor = LD(d["var_floor"])
    for t in range(n):
        a, b = window(d, t, n)
        c = b - a
        seg = xl[a:b]
        S1, S2, A1 = seg.sum(axis=0), (seg * seg).sum(axis=0), np.abs(seg).sum(axis=0)
        m = S1 / c
        xd = xl[t] - m
        dm = (c + 1) * V * A1 / c
        if not d["norm_vars"]:
            out[t] = xd
            bound[t] = (U * np.abs(xd) + dm + V * (np.abs(xd) + dm)) * (1 + 2 * U) + TINY
        elif c == 1:
            out[t], bound[t] = 0, 0
        else:
            var = np.maximum(S2 / c - m * m, floor)
            dv = (c + 4) * V * (S2 / c + m * m) + 2 * np.abs(m) * dm + dm * dm
            vlo = np.maximum(var - dv, floor)
            dx = dm + V * (np.abs(xd) + dm)
            q = xd / np.sqrt(var)
            eq = dx / np.sqrt(vlo) + np.abs(xd) * (1 / np.sqrt(vlo) - 1 / np.sqrt(var))
            out[t] = q
            bound[t] = (eq + (U + 3 * V) * (np.abs(q) + eq)) * (1 + 2 * U) + TINY
    return out, bound


def truth(x, d):
    """one SINGLE-STAGE spec (deltas alone, or a normalisation alone) over the real frames x: float32 [n, D] -> (truth, bound)"""
    assert (d["norm"] == "none") != (d["delta_order"] == 0), "the truth is of single stages: compositions are checked bit for bit"
    return deltas(x, d) if d["norm"] == "none" else normalise(x, d)


def ratio(got, want, bound):
    """largest |got - want| / bound over the elements; where the bound is 0 the value is exact (ratio 0) or the ratio is inf"""
    if got.size == 0:
        return 0.0
    err = np.abs(got.astype(LD) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))
