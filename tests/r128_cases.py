"""The cases of tests/test_pcm_true_peak_gpu.py: rows of one launch each, the smallest shapes at which csrc/pcm_truepeak.hip can go wrong,
named from its own constants (tests/r128_truth.py reads them).  tests/test_r128_cpu.py asserts, without a device, that every case is the
shape it is named for and that the truth alone meets the conditions of its device test.  Built once, never changed."""
import os

import numpy as np

import r128_truth as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = rt.kernel_constants(ROOT)
T = K["kTpTile"]  # elements of a tile: samples of a mono row
PAIR = 0.5        # two neighbouring samples of 0.5 interpolate to 0.62577 half way between them
PAIR_PEAK = 0.62577
QUIET = 0.02
ROW_LENGTHS = (0, 1, 2, 11, 12, 13, T - 1, T, T + 1, 2 * T + 5)
CHANNEL_COUNTS = (1, 2, 3, 6, 8, 33, 255)
GRID_ROWS = 5000


class Case:
    """rows of one launch: float32 [L, channels] each, one rate, one channel count"""

    def __init__(self, name, fs, channels, rows):
        self.name, self.fs, self.channels = name, fs, channels
        self.rows = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, channels) for r in rows]


def crest(x):
    return float(np.abs(x).max() / np.sqrt(np.mean(np.square(x, dtype=np.float64)))) if x.size else 0.0


def noise(rng, n, channels, amplitude=0.5):
    """uniform in [-amplitude, amplitude): crest factor sqrt(3)"""
    return amplitude * rng.uniform(-1.0, 1.0, size=(n, channels))


def with_pair(rng, n, channels, at, channel, value=PAIR):
    """quiet noise with `value` at samples at, at + 1 of `channel`"""
    x = noise(rng, n, channels, QUIET)
    x[at: at + 2, channel] = value
    return x


def build_cases():
    rng = np.random.default_rng(3341)
    cases = []
    # rows around the taps and around a tile, mono: a tile is T samples
    cases.append(Case("rows", 8000, 1, [noise(rng, L, 1) for L in ROW_LENGTHS]))
    # the peak behind the last sample, at the front, across the tile boundaries (inputs on both sides; the output in the tile behind, its
    # inputs in the halo; the output the last of a tile), negative, and a row whose true peak is its sample peak (an impulse)
    n = 2 * T + 50
    impulse = noise(rng, 300, 1, 0.001)
    impulse[150] = 0.7
    cases.append(Case("shapes", 8000, 1, [with_pair(rng, 300, 1, 298, 0), with_pair(rng, 300, 1, 0, 0), with_pair(rng, n, 1, T - 1, 0),
                                          with_pair(rng, n, 1, 2 * T - 1, 0), with_pair(rng, n, 1, T - 7, 0), with_pair(rng, n, 1, T - 6, 0),
                                          with_pair(rng, 300, 1, 100, 0, -PAIR), impulse]))
    # channel counts: the pair in the last channel and in channel 0, in the sample a tile boundary falls into (or begins with)
    for channels in CHANNEL_COUNTS:
        s = T // channels
        n = 2 * s + 30
        cases.append(Case("channels_%d" % channels, 8000, channels, [with_pair(rng, n, channels, s, channels - 1), with_pair(rng, n, channels, s, 0),
                                                                      noise(rng, n, channels)]))
    # rates: F = 4, 2, 2, 1, 1
    for fs in (44100, 96000, 191999, 192000, 384000):
        cases.append(Case("rate_%d" % fs, fs, 2, [noise(rng, 3000, 2), noise(rng, 17, 2)]))
    # more descriptors than the grid's y holds
    lengths = rng.integers(0, 41, size=GRID_ROWS)
    lengths[[0, 7, GRID_ROWS - 1]] = (40, 0, 33)
    cases.append(Case("grid", 8000, 2, [noise(rng, int(L), 2) for L in lengths]))
    # placement: rows of every kind out of order, other members' samples (1e6) around every window
    cases.append(Case("placement", 8000, 2, [noise(rng, int(L), 2) for L in (700, 0, 5, T // 2 + 3, 64, T // 2 - 11, 1, 2500)]))
    # non-finite samples and their clean neighbours
    clean_a, clean_b = noise(rng, 500, 2), noise(rng, 2 * T // 2 + 9, 2)
    nan_row, inf_row = noise(rng, 600, 2), noise(rng, 600, 2)
    nan_row[300, 1] = np.nan
    nan_row[10, 0] = 0.9  # (far from the NaN: the row's peak survives it)
    inf_row[17, 0] = np.inf
    cases.append(Case("nonfinite", 8000, 2, [clean_a, nan_row, clean_b, inf_row]))
    # the faded sines of EBU Tech 3341's true-peak cases, one launch per rate
    for fs in rt.SINE_RATES + [192000]:
        cases.append(Case("sines_%d" % fs, fs, 1, [rt.faded_sine(fs, fs / div, phase, amp) for div, phase, amp in rt.SINES]))
    return {c.name: c for c in cases}


_cases, _truth = {}, {}


def cases():
    if not _cases:
        _cases.update(build_cases())
    return _cases


def grid_checked_rows():
    return sorted(set(range(0, GRID_ROWS, 7)) | {0, GRID_ROWS - 1})


def truth(name, i):
    """(true peak, sample peak, bound) of row i of a case, float64; a row with non-finite samples by the header's own sums"""
    key = (name, i)
    if key not in _truth:
        case = cases()[name]
        r = case.rows[i]
        if np.isfinite(r).all():
            _truth[key] = (rt.true_peak(r, case.fs), float(np.abs(r).max()) if r.size else 0.0, rt.bound(r, case.fs))
        else:
            finite = np.where(np.isfinite(r), r, 0.0)
            _truth[key] = (rt.true_peak_by_phases(r, case.fs)[0], float(np.fmax.reduce(np.abs(r).reshape(-1))), rt.bound(finite, case.fs))
    return _truth[key]
