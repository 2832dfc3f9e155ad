"""What vpz_true_peak_filter, vpz_pcm_true_peak, vpz_loudness_range and vpz_loudness_maxima must compute, restated in numpy from
include/vorbispizza_pcm_r128.h alone -- no code of the library is used here, so the library is checked AGAINST this file, not by it.

The true peak is taken in float64 by numpy.convolve of the zero-stuffed row with the prototype h (whose exact zeros are set, not computed:
sin(pi k) is not 0 in double), numpy.fmax over the magnitudes.  `true_peak_by_phases` is the header's own sum, output by output: the form
for rows with non-finite samples, where a zero coefficient must not meet a NaN; on finite rows the two agree to the last few bits.
The bound of the device tests is derived at `bound` below."""
import os
import re

import numpy as np
from kernel_text import constants_of

TAPS = 12


def factor_of(fs):
    return 4 if fs < 96000 else 2 if fs < 192000 else 1


def prototype(F):
    """float64 [12 F + 1]: the Hann-windowed sinc of the header"""
    N = TAPS * F + 1
    j = np.arange(N)
    m = j - (TAPS // 2) * F
    t = m / F
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.sin(np.pi * t) / (np.pi * t) * 0.5 * (1.0 - np.cos(2.0 * np.pi * j / (N - 1)))
    h[m % F == 0] = 0.0
    h[(TAPS // 2) * F] = 1.0
    return h


def oversampled(x, F, h=None):
    """x: float [L] of one channel -> float64 [(L + 12) F]: y of the header (the F positions behind i = L + 10 are zeros)"""
    x = np.asarray(x, dtype=np.float64)
    h = prototype(F) if h is None else h
    if len(x) == 0:
        return np.zeros(0)
    z = np.zeros(len(x) * F)
    z[::F] = x
    return np.convolve(z, h)


def true_peak(x, fs):
    """x: float [L] or [L, channels] -> the true peak in float64, 0 for an empty window"""
    x = np.asarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    F, best = factor_of(fs), 0.0
    for ch in range(x.shape[1]):
        y = np.abs(oversampled(x[:, ch], F))
        if y.size:
            best = float(np.fmax(best, np.fmax.reduce(y)))
    return best


def true_peak_by_phases(x, fs, dtype=np.float64):
    """the same from the header's sums: y[i F] = x[i - 6], y[i F + p] = sum_k h[p + k F] x[i - k], k ascending; NaN outputs passed over.
    -> (peak, the output index i F + p of its first occurrence, channel)"""
    x = np.asarray(x, dtype=dtype)
    x = x[:, None] if x.ndim == 1 else x
    F, L = factor_of(fs), x.shape[0]
    h = prototype(F).astype(dtype)
    best = (0.0, -1, -1)
    if L == 0:
        return best
    for ch in range(x.shape[1]):
        pad = np.concatenate([np.zeros(TAPS - 1, dtype=dtype), x[:, ch], np.zeros(TAPS - 1, dtype=dtype)])  # pad[11 + i] = x[i]
        i = np.arange(L + TAPS - 1)
        Y = np.zeros((L + TAPS - 1, F), dtype=dtype)
        Y[:, 0] = pad[TAPS - 1 + i - TAPS // 2]
        with np.errstate(invalid="ignore"):
            for p in range(1, F):
                acc = h[p] * pad[TAPS - 1 + i]
                for k in range(1, TAPS):
                    acc = acc + h[p + k * F] * pad[TAPS - 1 + i - k]
                Y[:, p] = acc
        flat = np.abs(Y).reshape(-1)
        if np.isnan(flat).all():
            continue
        at = int(np.nanargmax(flat))
        if flat[at] > best[0]:
            best = (float(flat[at]), at, ch)
    return best


def bound(x, fs):
    """The device tests' bound on |true_peak - truth|:  (12 + 2) * 2^-24 * max over outputs of sum_k |h[p + k F]| |x[i - k]|.
    A maximum moves by no more than its terms do.  The device's output is a chain of one multiply and eleven fused multiply-adds, k
    ascending: twelve roundings, each relative 2^-24 to a partial sum no larger than sum |h| |x|; every coefficient is the float32 nearest
    to h, one more relative 2^-24 of the same sum; one more covers the products of those.  The identity phase is exact, and so is F = 1:
    the bound is then 0."""
    x = np.asarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    F = factor_of(fs)
    if F == 1 or x.shape[0] == 0:
        return 0.0
    h = np.abs(prototype(F))
    h[(TAPS // 2) * F] = 0.0  # (the identity phase has no rounding)
    most = max(float(oversampled(np.abs(x[:, ch]), F, h).max()) for ch in range(x.shape[1]))
    return (TAPS + 2) * 2.0 ** -24 * most


# ---- range and maxima
def block_levels(sums, S, length):
    """-> (p, l) of every block of `length` steps, hop one step; the sum of a block taken i ascending"""
    sums = np.asarray(sums, dtype=np.float64)
    n = len(sums) - length + 1
    if n < 1:
        return np.zeros(0), np.zeros(0)
    total = np.zeros(n)
    for i in range(length):
        total = total + sums[i: i + n]
    p = total / (float(length) * S)
    with np.errstate(divide="ignore", invalid="ignore"):
        return p, -0.691 + 10.0 * np.log10(p)


def _mean(p):
    """the mean with the sum taken in order (numpy's own sum is pairwise)"""
    return float(np.cumsum(p)[-1]) / len(p)


def loudness_range(sums, S):
    """-> (range LU, low, high, blocks kept): EBU Tech 3342 as the header states it"""
    p, l = block_levels(sums, S, 30)
    with np.errstate(invalid="ignore"):
        absolute = l > -70.0
    if not absolute.any():
        return 0.0, -np.inf, -np.inf, 0
    threshold = -0.691 + 10.0 * np.log10(_mean(p[absolute])) - 20.0
    with np.errstate(invalid="ignore"):
        kept = absolute & (l > threshold)
    if not kept.any():
        return 0.0, -np.inf, -np.inf, 0
    v = np.sort(l[kept])
    m = len(v)
    low, high = v[int(np.floor(0.10 * (m - 1) + 0.5))], v[int(np.floor(0.95 * (m - 1) + 0.5))]
    return float(high - low), float(low), float(high), m


def loudness_maxima(sums, S):
    """-> (maximum momentary, maximum short-term): -inf without a block or a finite level; NaN levels passed over"""
    out = []
    for length in (4, 30):
        l = block_levels(sums, S, length)[1]
        l = l[~np.isnan(l)]
        out.append(float(l.max()) if l.size else -np.inf)
    return tuple(out)


# ---- the launch plan of vpz_pcm_true_peak, restated
# kTpBlock, kTpTile, kTpTaps, kTpMaxGridY as csrc/pcm_truepeak.hip states them
kernel_constants = constants_of("pcm_truepeak.hip", ("kTpBlock", "kTpTile", "kTpTaps", "kTpMaxGridY"))


def launch_plan(samples, channels, k):
    """(output elements, tiles, LDS bytes) of one row: a tile is kTpTile consecutive ELEMENTS (position * channels + channel) of the
    row's (L + 11) * channels, staged with a halo of 11 * channels in front; eight more floats hold the waves' maxima; an empty window
    has no tile"""
    elems = (samples + k["kTpTaps"] - 1) * channels if samples > 0 else 0
    lds = ((k["kTpTaps"] - 1) * channels + k["kTpTile"] + 2 * (k["kTpBlock"] // 64)) * 4
    return elems, -(-elems // k["kTpTile"]), lds


def tile_of(sample, channel, channels, k):
    """the tile that computes output position `sample` of `channel`"""
    return (sample * channels + channel) // k["kTpTile"]


# ---- signals
def faded_sine(fs, hz, phase_deg, amplitude, seconds=0.5, fade=0.02):
    """float32 [samples]: amplitude * sin(2 pi hz n / fs + phase) under raised-cosine fades of `fade` seconds at both ends"""
    n = int(round(seconds * fs))
    t = np.arange(n)
    x = amplitude * np.sin(2.0 * np.pi * hz * t / fs + np.deg2rad(phase_deg))
    m = int(round(fade * fs))
    ramp = 0.5 * (1.0 - np.cos(np.pi * (np.arange(m) + 0.5) / m))
    env = np.ones(n)
    env[:m] = ramp
    env[n - m:] = ramp[::-1]
    return (x * env).astype(np.float32)


# (rate divisor, phase in degrees, amplitude): the shapes of EBU Tech 3341's true-peak cases
SINES = [(4, 0.0, 0.5), (4, 45.0, 0.5), (6, 60.0, 0.5), (8, 67.5, 0.5), (4, 45.0, 1.41)]
SINE_RATES = [48000, 44100, 8000, 96000]
TOLERANCE_DB = (-0.4, 0.2)  # EBU's
