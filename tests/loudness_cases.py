"""vpz_pcm_loudness at the limits of its launches: ONE case list, used by test_loudness_cpu.py (is every case the shape it is named for, and
does the reference alone meet the conditions?) and by test_pcm_loudness_limits_gpu.py (does the device compute them?).

A case is loudness_support.Case: rows of one launch, noise plus a tone, every channel's crest factor 4 or less (Case asserts it).
EXPECT states, in numbers written down here and not computed, what each case is there for: G and the idle lanes of its channel count, and
per row (units, steps, workgroups of (a), workgroups of (c), samples behind the last whole step); test_loudness_cpu.py holds the cases to
them through loudness_truth.launch_plan and tiles_of.  The truth of all cases is one table, computed once per process in groups of similar
length (numpy.longdouble, one sample after the other)."""
import types

import numpy as np

import loudness_truth as lt
from loudness_support import Case, noise, tone

S = 800                      # the step at 8 000 Hz
CHANNEL_COUNTS = (4, 5, 7, 9, 31, 32, 33, 64, 85, 86, 128, 129, 255)
PEAK_CHANNEL = 200           # of the 255-channel case with the caller's weights: the loudest channel, weight 0
GRID_ROWS, GRID_DST = 5000, 5100


def sig(rng, L, channels, fs=8000, hz=440.0):
    """noise plus tone: |x| <= 0.7, rms about 0.31"""
    return 0.4 * noise(rng, L, channels) + 0.3 * tone(L, fs, hz)


def _rng(*key):
    return np.random.default_rng([1770, 2] + list(key))


def _channels(c, weights=False):
    rng = _rng(1, c, int(weights))
    rows = [sig(rng, 2 * S + 17, c), sig(rng, S, c)]
    w = None
    if weights:
        for r in rows:
            r[:, PEAK_CHANNEL] *= 1.3
        w = rng.uniform(0.5, 2.0, c)
        w[PEAK_CHANNEL] = 0.0
    return Case("channels_%d%s" % (c, "_weights" if weights else ""), 8000, c, rows, w)


def _tails(c):
    rng = _rng(3, c)
    rows = [sig(rng, 2 * S + t, c) for t in (1, 31, 32, 33, S - 1)]
    rows[0][-1, c - 1] = -0.95  # the largest |x| is negative and the last sample of a one-sample tail
    rows[1][0, 0] = 0.97        # the largest |x| is the first sample
    return Case("tails_%d" % c, 8000, c, rows)


def _odd(fs, c, tails, whole):
    rng = _rng(4, fs, c)
    s = lt.step_of(fs)
    return Case("odd_%d_%d" % (fs, c), fs, c, [sig(rng, whole * s + t, c, fs) for t in tails])


def _grid():
    rng = _rng(5)
    lengths = rng.integers(0, 2 * S + 6, GRID_ROWS)
    lengths[:4] = (2 * S + 5, 0, S - 1, S)
    lengths[-4:] = (S + 1, 2 * S, 1, 2 * S + 5)
    return Case("grid", 8000, 2, [sig(rng, int(L), 2) for L in lengths])


def grid_checked_rows():
    return sorted(set(range(0, GRID_ROWS, 7)) | set(range(4)) | set(range(GRID_ROWS - 4, GRID_ROWS)))


def build_cases():
    out = [_channels(c) for c in CHANNEL_COUNTS] + [_channels(255, weights=True)]
    rng = _rng(2)
    out.append(Case("edges_8", 8000, 8, [sig(rng, L, 8) for L in (32 * S, 32 * S + 1, 31 * S + 799, 33 * S, 64 * S + 31)]))
    out.append(Case("edges_3", 8000, 3, [sig(rng, L, 3) for L in (85 * S, 85 * S + 1, 86 * S)]))
    out += [_tails(1), _tails(6)]
    out += [_odd(11025, 3, (14, 15, 16), 2), _odd(11025, 6, (14, 15, 16), 2), _odd(44100, 5, (26,), 1)]
    rng = _rng(6)
    out.append(Case("empty_rows", 8000, 2, [sig(rng, 0, 2) for _ in range(4)]))
    out.append(Case("short_rows", 8000, 2, [sig(rng, L, 2) for L in (1, 31, S - 1, 400)]))
    grid = _grid()
    out.append(grid)
    out.append(Case("grid_checked", 8000, 2, [grid.rows[i] for i in grid_checked_rows()]))
    out.append(Case("three_steps", 8000, 1, [sig(rng, 3 * S + 5, 1)]))
    out.append(Case("full_row", 8000, 2, [sig(rng, 3 * S + S - 1, 2)]))
    out.append(Case("beyond", 8000, 2, [sig(rng, 2 * S + 100, 2), sig(rng, S + 5, 2)]))
    out.append(Case("scaling", 8000, 5, [sig(rng, 3 * S + 40, 5)]))
    out.append(Case("shift", 8000, 8, [sig(rng, 3 * S + 40, 8)]))
    out.append(Case("crowd", 8000, 6, [sig(rng, int(L), 6) for L in (3 * S + 7, S - 3, 5 * S + 40, 0, 2 * S, 4 * S + 1, S, 6 * S + 31)]))
    return {c.name: c for c in out}


NO_TRUTH = ("grid",)  # (its checked rows are the case grid_checked)
_cases, _truth = {}, {}


def cases():
    if not _cases:
        _cases.update(build_cases())
    return _cases


def shifted(case, k):
    """the case's row 0 behind k steps of silence, as something `launch` takes (no Case: silence in front raises the crest factor, and
    the shifted row is held to its twin's bits, not to the bound)"""
    row = case.rows[0]
    rows = [row, np.concatenate([np.zeros((k * lt.step_of(case.fs), case.channels), dtype=np.float32), row])]
    return types.SimpleNamespace(name="%s_by_%d" % (case.name, k), fs=case.fs, channels=case.channels, weights=case.weights, rows=rows)


def scaled(case, e):
    """the case's rows times 2^e: exact in float32"""
    return types.SimpleNamespace(name="%s_2^%d" % (case.name, e), fs=case.fs, channels=case.channels, weights=case.weights,
                                 rows=[np.ldexp(r, e).astype(np.float32) for r in case.rows])


def truth_of(some, limit_bytes=400 << 20):
    """{(case, row): (per-channel step sums in longdouble [steps, channels], weighted [steps])} of these cases.  The signals run in groups
    of similar length -- a group ends where a signal is shorter than half its longest, or the padded [time, signals] array would pass
    limit_bytes -- so a short signal never rides along a long one's loop over time."""
    entries = [(r.shape[0], c, i, ch) for c in some for i, r in enumerate(c.rows) for ch in range(c.channels)]
    entries.sort(key=lambda e: -e[0])
    size = np.dtype(np.longdouble).itemsize
    out, per, at = {}, {}, 0
    while at < len(entries):
        longest, end = entries[at][0], at + 1
        while end < len(entries) and 2 * entries[end][0] >= longest and longest * (end - at + 1) * size <= limit_bytes:
            end += 1
        group = entries[at:end]
        sums = lt.step_sums_sequential([c.rows[i][:, ch] for _, c, i, ch in group], [c.fs for _, c, _, _ in group], np.longdouble)
        for (_, c, i, ch), s in zip(group, sums):
            per[(c.name, i, ch)] = s
        at = end
    for c in some:
        for i in range(len(c.rows)):
            p = np.stack([per[(c.name, i, ch)] for ch in range(c.channels)], axis=1)
            out[(c.name, i)] = (p, lt.weighted(p, c.w.astype(np.longdouble)))
    return out


def truth():
    """of every case but NO_TRUTH, computed once"""
    if not _truth:
        _truth.update(truth_of([c for c in cases().values() if c.name not in NO_TRUTH]))
    return _truth


# ---- what each case is there for: name -> (G, idle lanes, S % 32, [(units, steps, workgroups of (a), of (c), tail)] per row)
def _chan(c, G, idle):
    # 2S + 17: three units, two steps; S: one of each
    return (G, idle, 0, [(3, 2, -(-3 // G), -(-2 // G), 17), (1, 1, 1, 1, 0)])


EXPECT = {
    "channels_4": _chan(4, 64, 0), "channels_5": _chan(5, 51, 1), "channels_7": _chan(7, 36, 4), "channels_9": _chan(9, 28, 4),
    "channels_31": _chan(31, 8, 8), "channels_32": _chan(32, 8, 0), "channels_33": _chan(33, 7, 25), "channels_64": _chan(64, 4, 0),
    "channels_85": _chan(85, 3, 1), "channels_86": _chan(86, 2, 84), "channels_128": _chan(128, 2, 0), "channels_129": _chan(129, 1, 127),
    "channels_255": _chan(255, 1, 1), "channels_255_weights": _chan(255, 1, 1),
    # steps == G; units == G + 1 (the second workgroup of (a) holds a one-sample tail, that of (c) nothing); one sample short of G
    # steps; G + 1 steps; steps == 2G and a tail of 31
    "edges_8": (32, 0, 0, [(32, 32, 1, 1, 0), (33, 32, 2, 1, 1), (32, 31, 1, 1, 799), (33, 33, 2, 2, 0), (65, 64, 3, 2, 31)]),
    "edges_3": (85, 1, 0, [(85, 85, 1, 1, 0), (86, 85, 2, 1, 1), (86, 86, 2, 2, 0)]),
    "tails_1": (256, 0, 0, [(3, 2, 1, 1, t) for t in (1, 31, 32, 33, 799)]),
    "tails_6": (42, 4, 0, [(3, 2, 1, 1, t) for t in (1, 31, 32, 33, 799)]),
    # a last chunk of 15 samples and tails one under, at and one over it; of 26 samples
    "odd_11025_3": (85, 1, 15, [(3, 2, 1, 1, t) for t in (14, 15, 16)]),
    "odd_11025_6": (42, 4, 15, [(3, 2, 1, 1, t) for t in (14, 15, 16)]),
    "odd_44100_5": (51, 1, 26, [(2, 1, 1, 1, 26)]),
    "empty_rows": (128, 0, 0, [(0, 0, 0, 0, 0)] * 4),  # tiles == 0: no pass is launched
    "short_rows": (128, 0, 0, [(1, 0, 1, 0, t) for t in (1, 31, 799, 400)]),  # (c) is launched and every workgroup leaves
    "three_steps": (256, 0, 0, [(4, 3, 1, 1, 5)]),
    "full_row": (128, 0, 0, [(4, 3, 1, 1, 799)]),
    "beyond": (128, 0, 0, [(3, 2, 1, 1, 100), (2, 1, 1, 1, 5)]),
    "scaling": (51, 1, 0, [(4, 3, 1, 1, 40)]),
    "shift": (32, 0, 0, [(4, 3, 1, 1, 40)]),
}
