"""vpz_pcm_loudness on the device, shared by tests/test_pcm_loudness_gpu.py, tests/test_pcm_loudness_limits_gpu.py, tests/test_loudness_cpu.py and
tests/loudness_cases.py: Case (rows of one launch, crest factor 4 or less), the first cases and their longdouble truth (one table per
process), the launch into sentinel-filled outputs and check_case, which holds sums and peak to truth and bound."""
import numpy as np
import pytest

import loudness_truth as lt


LONGDOUBLE_BITS = np.finfo(np.longdouble).nmant
needs_longdouble = pytest.mark.skipif(LONGDOUBLE_BITS < 63, reason="numpy.longdouble has %d mantissa bits on this machine: float64 would be "
                                      "compared against itself" % LONGDOUBLE_BITS)
SENTINEL, PEAK_SENTINEL = -7.25, -3.5


def noise(rng, n, channels):
    """uniform in [-1, 1): crest factor sqrt(3)"""
    return rng.uniform(-1.0, 1.0, size=(n, channels))


def tone(n, fs, hz):
    return np.sin(2.0 * np.pi * hz * np.arange(n) / fs)[:, None]


def crest(x):
    return float(np.abs(x).max() / np.sqrt(np.mean(np.square(x, dtype=np.float64)))) if x.size else 0.0


class Case:
    """rows of one launch: float32 [L, channels] each, one rate, one channel count"""

    def __init__(self, name, fs, channels, rows, weights=None):
        self.name, self.fs, self.channels, self.weights = name, fs, channels, weights
        self.rows = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, channels) for r in rows]
        for r in self.rows:  # (the bound's premise, channel by channel: every channel is a signal of its own)
            assert r.shape[0] < lt.step_of(fs) or max(crest(r[:, ch]) for ch in range(channels)) <= 4.0, name

    @property
    def w(self):
        return lt.weights_of(self.channels) if self.weights is None else np.asarray(self.weights, dtype=np.float64)


def build_cases():
    rng = np.random.default_rng(1770)
    cases = []
    S = 800
    # lengths around a step, at 8 000 Hz, stereo
    cases.append(Case("lengths", 8000, 2, [0.4 * noise(rng, L, 2) + 0.3 * tone(L, 8000, 440.0) for L in (0, S - 1, S, S + 1, 4 * S, 7 * S + 123)]))
    # 70 steps: more units of one channel than a 64-lane wave; under a DC offset (the state-carry case) and as the gate case (a loud half,
    # then 26 dB less: every block far from both gates)
    n = 70 * S
    dc = 0.5 + 0.1 * noise(rng, n, 1) + 0.1 * tone(n, 8000, 20.0)
    envelope = np.where(np.arange(n) < 35 * S, 1.0, 0.05)[:, None]
    gated = envelope * (0.3 * noise(rng, n, 1) + 0.5 * tone(n, 8000, 997.0))
    cases.append(Case("dc_70_steps", 8000, 1, [dc, gated]))
    # 40 steps of 8 channels take two workgroups of (a) and (c): 256 / 8 = 32 steps each
    cases.append(Case("two_workgroups", 8000, 8, [0.5 * noise(rng, 40 * S + 5, 8)]))
    # every rate's own step
    for fs in (11025, 44100, 48000):
        L = 7 * lt.step_of(fs) + 123
        cases.append(Case("rate_%d" % fs, fs, 2, [0.3 * noise(rng, L, 2) + 0.4 * tone(L, fs, 1000.0)]))
    L = 2 * 38400 + 5
    cases.append(Case("rate_384000", 384000, 1, [0.3 * noise(rng, L, 1) + 0.4 * tone(L, 384000, 1000.0)]))
    # channel counts: 6 has an LFE of weight 0 that is the loudest channel and holds the peak; 3 takes the caller's weights
    for channels, weights in ((1, None), (2, None), (6, None), (8, None), (3, [0.5, 2.0, 0.0])):
        rows = []
        for L in (4 * S + 17, 2 * S):
            x = 0.2 * noise(rng, L, channels) + 0.2 * tone(L, 8000, 300.0)
            x[:, -1] *= 2.4
            rows.append(x)
        cases.append(Case("channels_%d" % channels, 8000, channels, rows, weights))
    # a burst that goes silent in the middle of its third step, then six silent steps
    burst = 0.6 * noise(rng, 9 * S, 1)
    burst[2 * S + S // 2:] = 0.0
    cases.append(Case("burst", 8000, 1, [burst]))
    return {c.name: c for c in cases}


_cases, _truth = {}, {}


def cases():
    if not _cases:
        _cases.update(build_cases())
    return _cases


def truth():
    """{(case, row): (per-channel step sums in longdouble [steps, channels], weighted [steps])}, computed once in one run over time"""
    if not _truth:
        signals, rates, keys = [], [], []
        for c in cases().values():
            for i, r in enumerate(c.rows):
                for ch in range(c.channels):
                    signals.append(r[:, ch])
                    rates.append(c.fs)
                    keys.append((c.name, i, ch))
        sums = lt.step_sums_sequential(signals, rates, np.longdouble)
        for c in cases().values():
            for i, r in enumerate(c.rows):
                per = np.stack([sums[keys.index((c.name, i, ch))] for ch in range(c.channels)], axis=1)
                _truth[(c.name, i)] = (per, lt.weighted(per, c.w.astype(np.longdouble)))
    return _truth


def launch(ctx, case, order=None, gap=3, extra_rows=1, max_steps=None, first=0):
    """one vpz_pcm_loudness launch over the case's rows: the windows lie in one source array with `gap` junk elements in front of each
    (odd offsets), row i goes to destination row order[i] of extra_rows more rows than the case has.
    -> (sums [rows, max_steps] float64, peak [rows] float32, as numpy)"""
    import torch
    from vorbispizza_amd import capi
    n = len(case.rows)
    order = list(range(n)) if order is None else list(order)
    parts, desc, at = [], [], first
    if first:
        parts.append(np.full(first, 9.0, dtype=np.float32))
    for i, r in enumerate(case.rows):
        parts.append(np.full(gap, 9.0, dtype=np.float32))
        at += gap
        desc.append((at, r.shape[0], order[i]))
        parts.append(r.reshape(-1))
        at += r.size
    parts.append(np.full(5, 9.0, dtype=np.float32))
    src = torch.from_numpy(np.concatenate(parts)).to("cuda:0")
    S = lt.step_of(case.fs)
    if max_steps is None:
        max_steps = max([1] + [r.shape[0] // S for r in case.rows]) + 2
    dst_rows = max(order + [-1]) + 1 + extra_rows
    sums = torch.full((dst_rows, max_steps), SENTINEL, dtype=torch.float64, device="cuda:0")
    peak = torch.full((dst_rows,), PEAK_SENTINEL, dtype=torch.float32, device="cuda:0")
    capi.pcm_loudness(ctx, src, case.channels, case.fs, desc, weights=case.weights, max_steps=max_steps, out=(sums, peak))
    ctx.synchronize()
    return sums.cpu().numpy(), peak.cpu().numpy()


def check_case(case, sums, peak, order=None):
    """every named row against the truth and the bound; -> the largest error / bound"""
    S = lt.step_of(case.fs)
    order = list(range(len(case.rows))) if order is None else list(order)
    worst = 0.0
    for i, r in enumerate(case.rows):
        row, n = order[i], r.shape[0] // S
        want = truth()[(case.name, i)][1]
        assert len(want) == n
        got = sums[row]
        assert (got[n:].view(np.int64) == 0).all(), (case.name, i)  # +0.0 behind the steps, bit for bit
        assert peak[row] == (np.abs(r).max() if r.size else 0.0), (case.name, i)
        if n == 0:
            continue
        err = np.abs(got[:n].astype(np.longdouble) - want).astype(np.float64)
        bound = lt.bound(case.fs, want.astype(np.float64))
        assert (bound > 0).all()
        ratio = err / bound
        assert (ratio <= 1.0).all(), (case.name, i, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
    named = set(order)
    for row in range(sums.shape[0]):
        if row not in named:  # an unnamed row is not touched
            assert (sums[row] == SENTINEL).all() and peak[row] == PEAK_SENTINEL
    return worst
