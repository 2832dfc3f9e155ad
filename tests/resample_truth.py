"""The resampler's truth, shared by the CPU and GPU tests of vpz_pcm_resample and of the dispatcher's resampled batches: the ratio rules, the
filter table and the float64 resampling restated, the bound, the project's int16 conversion, the limit cases and the kernel's launch plan
restated from the constants csrc/pcm_resample.hip states.  The tables are computed once per process (_tables)."""
import math
import os
import re

import numpy as np
from kernel_text import constants_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def ratio_of(fs, ft):
    g = math.gcd(fs, ft)
    return ft // g, fs // g  # (up, down)


def ratio_ok(up, down):
    return 1 <= up <= 1024 and 1 <= down <= 32 * up and math.gcd(up, down) == 1


def tap_live(n, up, down):
    """|s * u| < 6 for u = n / up, s = 0.99 * min(up, down) / down -- in integers"""
    return abs(n) * 99 * min(up, down) < 600 * up * down


_tables = {}


def filter_table(up, down):
    """(taps, first[up], h[up, taps] float64): output j of phase p = j % up starts at source sample j * down // up + first[p]"""
    if (up, down) in _tables:
        return _tables[(up, down)]
    assert ratio_ok(up, down)
    if up == down:
        out = (1, np.zeros(1, dtype=np.int64), np.ones((1, 1)))
    else:
        s = 0.99 * min(up, down) / down
        first, live = [], []
        for p in range(up):
            r = p * down % up
            d = -(600 * down // (99 * min(up, down)) + 2)
            while not tap_live(d * up - r, up, down):
                d += 1
            first.append(d)
            while tap_live(d * up - r, up, down):
                d += 1
            live.append(d - first[-1])
        taps = max(live)
        h = np.zeros((up, taps))
        for p in range(up):
            r = p * down % up
            n = (first[p] + np.arange(live[p], dtype=np.int64)) * up - r
            x = s * n.astype(np.float64) / up
            h[p, :live[p]] = s * np.sinc(x) * np.cos(np.pi * x / 12.0) ** 2  # (np.sinc(x) = sin(pi x) / (pi x), 1 at 0)
        out = (taps, np.asarray(first, dtype=np.int64), h)
    _tables[(up, down)] = out
    return out


def resample_truth(x, up, down, downmix=False):
    """x [L, C] (any float type) -> (y [J, Co], B [J, Co]) in float64, J = ceil(L * up / down), Co = 1 with downmix; the window is a clip of
    its own, zero outside [0, L).  B[j] = sum |x[m] * h| over the taps (and the channels, divided by C, for a downmix)."""
    x = np.asarray(x, dtype=np.float64)
    L, ch = x.shape
    J = -(-L * up // down)
    taps, first, h = filter_table(up, down)
    y, B = np.zeros((J, ch)), np.zeros((J, ch))
    if up == down:
        y, B = x.copy(), np.abs(x)
    else:
        reach = int(max(0, -first.min())) + 1
        padded = np.zeros((L + 2 * reach + taps + down + 2, ch))
        padded[reach: reach + L] = x
        for p in range(min(up, J)):
            js = np.arange(p, J, up, dtype=np.int64)
            at = js * down // up + first[p] + reach
            idx = at[:, None] + np.arange(taps)[None, :]
            assert idx.min() >= 0 and idx.max() < padded.shape[0]
            prod = padded[idx] * h[p][None, :, None]  # [outputs, taps, channels]
            y[js] = prod.sum(axis=1)
            B[js] = np.abs(prod).sum(axis=1)
    if downmix:
        y, B = y.mean(axis=1, keepdims=True), B.sum(axis=1, keepdims=True) / ch
    return y, B


def bound(B, up, down, mixed_channels=1):
    """the derived tolerance (the module's docstring)"""
    return (filter_table(up, down)[0] + mixed_channels + 3) * 2.0 ** -24 * B


def to_s16(y):
    """the project's one conversion of a float32 sample: (int)(x * 32768f) clamped"""
    v = np.asarray(y, dtype=np.float32) * np.float32(32768.0)
    return np.clip(np.trunc(v.astype(np.float64)), -32768, 32767).astype(np.int16)


def live_taps(up, down):
    """live[up]: the live taps of every phase; table entries behind them are the zero padding of a short phase"""
    taps, first, _ = filter_table(up, down)
    if up == down:
        return np.ones(1, dtype=np.int64)
    live = [sum(tap_live((int(first[p]) + k) * up - p * down % up, up, down) for k in range(taps)) for p in range(up)]
    return np.asarray(live, dtype=np.int64)


# (up, down, source channels, downmix): tests/test_pcm_resample_limits_gpu.py runs every one; test_the_limit_cases_take_every_branch_of_the_plan
# holds the list to the plan.  (1, 6) with seven channels is the list's one case of five channels to a pass; (5, 48) with seven mixed
# down is there for the non-finite tests, which rerun it.
LIMIT_CASES = [(1, 32, 1, False), (1, 32, 2, False), (1, 32, 6, False), (1, 32, 6, True),
               (31, 991, 2, False), (31, 991, 3, False), (31, 991, 2, True),
               (1024, 32767, 2, False), (1024, 32767, 2, True),
               (1, 12, 5, False), (5, 48, 5, False), (5, 48, 7, False), (5, 48, 7, True), (1, 8, 6, False), (1, 6, 7, False),
               (160, 441, 9, False), (160, 441, 10, False), (160, 441, 17, False), (160, 441, 255, False), (160, 441, 255, True),
               (1024, 1023, 2, False), (1024, 1023, 8, False), (1023, 1024, 2, False), (1023, 1024, 8, False),
               (1024, 1, 2, False), (1, 1, 10, False), (1, 1, 255, True)]


# kRsBlock, kRsLds, kRsMaxPass, kRsMaxTaps as csrc/pcm_resample.hip states them
kernel_constants = constants_of("pcm_resample.hip", ("kRsBlock", "kRsLds", "kRsMaxPass", "kRsMaxTaps"))


def launch_plan(up, down, channels, downmix, k=None):
    """vpz_pcm_resample's launch plan, restated: the floats between two staged channels, the channels of every pass, the dynamic LDS"""
    k = k or kernel_constants()
    taps, first, _ = filter_table(up, down)
    out_channels = 1 if downmix else channels
    span_cap = (k["kRsBlock"] - 1) * down // up + 2 + taps
    per_pass = max(1, min(out_channels, k["kRsMaxPass"], k["kRsLds"] // span_cap))
    passes = [min(per_pass, out_channels - c0) for c0 in range(0, out_channels, per_pass)]
    return dict(taps=taps, first=first, span_cap=span_cap, per_pass=per_pass, passes=passes, lds_bytes=4 * per_pass * (span_cap + k["kRsBlock"]))


def passes_text(passes):
    """[8, 8, 8, 7] -> '3 x 8 + 7'"""
    head = [n for n in passes if n == passes[0]]
    parts = ["%d x %d" % (len(head), head[0]) if len(head) > 3 else " + ".join(str(n) for n in head)] + [str(n) for n in passes[len(head):]]
    return " + ".join(parts)
