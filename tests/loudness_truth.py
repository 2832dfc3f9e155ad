"""What vpz_pcm_loudness and vpz_loudness_gate must compute, restated in numpy from include/vorbispizza_pcm_loudness.h alone -- no code of
the library is used here, so the library's coefficients, steps and gate are checked AGAINST this file, not by it.

Two forms of the same recurrence:
  step_sums_sequential  one sample after the other, vectorised over signals, in a dtype of the caller's (numpy.longdouble: the truth of
                        the device tests; the Python loop runs over time, so it is for short signals);
  step_sums_chunked     float64, every step from zero state, the exact carry s[j+1] = P s[j] + z[j], every step again from its entering
                        state -- the loop runs over the samples of ONE step, vectorised over the steps, which is what makes the
                        80-second sequences of EBU Tech 3341 affordable in numpy.  It is also the shape of the device kernels.
The bound of the device tests is derived at `bound` below."""
import numpy as np
from kernel_text import constants_of

SHELF = dict(f0=1681.974450955533, G=3.999843853973347, Q=0.7071752369554196, vb_exp=0.4996667741545416)
HIGHPASS = dict(f0=38.13547087602444, Q=0.5003270373238773)
# BS.1770-4's table for 48 000 Hz: b0 b1 b2 a1 a2 of the shelf, a1 a2 of the high-pass (its numerator is 1, -2, 1)
PUBLISHED_48K = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621]
WEIGHTS = {1: [1], 2: [1, 1], 3: [1, 1, 1], 4: [1, 1, 1.41, 1.41], 5: [1, 1, 1, 1.41, 1.41], 6: [1, 1, 1, 1.41, 1.41, 0],
           7: [1, 1, 1, 1.41, 1.41, 1, 0], 8: [1, 1, 1, 1.41, 1.41, 1, 1, 0]}


def step_of(fs):
    return (int(fs) + 5) // 10


def weights_of(channels):
    return np.array(WEIGHTS.get(channels, [1] * channels), dtype=np.float64)


def coefficients(fs):
    """float64 [2, 5]: b0 b1 b2 a1 a2 of the shelf, then of the high-pass"""
    K, Q = np.tan(np.pi * SHELF["f0"] / fs), SHELF["Q"]
    Vh = 10.0 ** (SHELF["G"] / 20.0)
    Vb = Vh ** SHELF["vb_exp"]
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K, Q = np.tan(np.pi * HIGHPASS["f0"] / fs), HIGHPASS["Q"]
    a0 = 1.0 + K / Q + K * K
    return np.array([shelf, [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]], dtype=np.float64)


def pole_radius(fs):
    """|pole| of the high-pass: sqrt(a2) of a complex pair, the larger root of a real one"""
    a1, a2 = coefficients(fs)[1, 3:]
    disc = a1 * a1 - 4.0 * a2
    return float(np.sqrt(a2)) if disc < 0 else float((abs(a1) + np.sqrt(disc)) / 2.0)


def _advance(c, x, s):
    """one sample of the two stages in transposed direct form II; c: [2, 5] (or [2, 5, signals]), s: list of four arrays; -> y"""
    y1 = c[0][0] * x + s[0]
    s[0] = c[0][1] * x - c[0][3] * y1 + s[1]
    s[1] = c[0][2] * x - c[0][4] * y1
    y2 = c[1][0] * y1 + s[2]
    s[2] = c[1][1] * y1 - c[1][3] * y2 + s[3]
    s[3] = c[1][2] * y1 - c[1][4] * y2
    return y2


def step_sums_sequential(signals, rates, dtype=np.longdouble):
    """signals: a list of 1-D float arrays (one channel each), rates: their sample rates.  -> a list of arrays in `dtype`: the sum of y^2
    over every whole step of each signal, filtered from zero state.  All signals advance together (a signal past its end gets zeros)."""
    n = len(signals)
    longest = max([len(x) for x in signals] + [0])
    X = np.zeros((longest, n), dtype=dtype)
    for i, x in enumerate(signals):
        X[: len(x), i] = np.asarray(x).astype(dtype)
    c = np.stack([coefficients(fs) for fs in rates], axis=-1).astype(dtype)  # [2, 5, n]
    S = np.array([step_of(fs) for fs in rates])
    steps = np.array([len(x) // step_of(fs) for x, fs in zip(signals, rates)])
    sums = np.zeros((int(steps.max()) if n else 0, n), dtype=dtype)
    s = [np.zeros(n, dtype=dtype) for _ in range(4)]
    acc = np.zeros(n, dtype=dtype)
    left = S.copy()  # samples to the end of each signal's current step
    at = np.zeros(n, dtype=np.int64)
    idx = np.arange(n)
    for t in range(longest):
        y = _advance(c, X[t], s)
        acc += y * y
        left -= 1
        done = left == 0
        if done.any():
            keep = done & (at < steps)
            sums[at[keep], idx[keep]] = acc[keep]
            acc[done] = 0
            at[done] += 1
            left[done] = S[done]
    return [sums[: steps[i], i].copy() for i in range(n)]


def transition(fs):
    """float64 [4, 4]: what S samples of silence make of a state"""
    c = coefficients(fs)
    s = [np.eye(4)[k].copy() for k in range(4)]  # s[k][i]: component k of the state that started as unit vector i
    for _ in range(step_of(fs)):
        _advance(c, 0.0, s)
    return np.array(s)


def step_sums_chunked(x, fs):
    """x: float [samples] or [samples, channels] -> float64 [steps, channels]: the same sums in float64, by steps (see the module text)"""
    x = np.asarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    S, C = step_of(fs), x.shape[1]
    n = x.shape[0] // S
    c = coefficients(fs)
    X = x[: n * S].reshape(n, S, C)
    z = [np.zeros((n, C)) for _ in range(4)]
    for t in range(S):
        _advance(c, X[:, t, :], z)
    P = transition(fs)
    enter = np.zeros((4, n, C))
    s = np.zeros((4, C))
    for j in range(n):
        enter[:, j, :] = s
        s = P @ s + np.array([z[k][j] for k in range(4)])
    s = [enter[k].copy() for k in range(4)]
    acc = np.zeros((n, C))
    for t in range(S):
        y = _advance(c, X[:, t, :], s)
        acc += y * y
    return acc


def weighted(sums_per_channel, w):
    """[steps, channels] -> [steps]: sum_c w[c] * sums, c ascending"""
    out = np.zeros(sums_per_channel.shape[0], dtype=sums_per_channel.dtype)
    for ch in range(sums_per_channel.shape[1]):
        out = out + w[ch] * sums_per_channel[:, ch]
    return out


def block_levels(sums, S):
    """-> (p, l) of every 400 ms block of the step sums"""
    sums = np.asarray(sums, dtype=np.float64)
    if len(sums) < 4:
        return np.zeros(0), np.zeros(0)
    p = (sums[:-3] + sums[1:-2] + sums[2:-1] + sums[3:]) / (4.0 * S)
    with np.errstate(divide="ignore"):
        return p, -0.691 + 10.0 * np.log10(p)


def _mean(p):
    """the mean with the sum taken in order (numpy's own sum is pairwise)"""
    return float(np.cumsum(p)[-1]) / len(p)


def gate(sums, S):
    """-> (integrated LUFS or -inf, blocks kept, the relative threshold or None, the levels)"""
    p, l = block_levels(sums, S)
    absolute = l > -70.0
    if not absolute.any():
        return -np.inf, 0, None, l
    threshold = -0.691 + 10.0 * np.log10(_mean(p[absolute])) - 10.0
    kept = absolute & (l > threshold)
    if not kept.any():
        return -np.inf, 0, threshold, l
    return float(-0.691 + 10.0 * np.log10(_mean(p[kept]))), int(kept.sum()), threshold, l


def bound(fs, truth):
    """The device tests' bound on |sums[j] - truth[j]|:  64 * 2^-53 * (1 / (1 - r)^2 + S) * max_{i <= j} truth[i].
    Every float64 operation of the recurrence adds a relative 2^-53 of a value no larger than the state; the high-pass, with poles of
    radius r, carries such an error on with a gain whose worst case is 1 / (1 - r)^2 (a double pole at r: sum_k (k + 1) r^k), relative to
    the signal that made the state.  Summing S squares adds S roundings of the running sum.  A quiet step behind a loud one still carries
    the loud one's rounding, hence the running maximum.  64 covers the constant number of operations per sample and the crest factor of
    the input, which the tests keep at 4 or less."""
    r, S = pole_radius(fs), step_of(fs)
    truth = np.asarray(truth, dtype=np.float64)
    return 64.0 * 2.0 ** -53 * (1.0 / (1.0 - r) ** 2 + S) * np.maximum.accumulate(truth) if len(truth) else truth


def relative_bound(fs):
    r, S = pole_radius(fs), step_of(fs)
    return 64.0 * 2.0 ** -53 * (1.0 / (1.0 - r) ** 2 + S)


# ---- the launch plan of vpz_pcm_loudness, restated
# kLoudBlock, kChunk, kLoudMaxGridY as csrc/pcm_loudness.hip states them
kernel_constants = constants_of("pcm_loudness.hip", ("kLoudBlock", "kChunk", "kLoudMaxGridY"))


def launch_plan(channels, k):
    """(G, stride, lds_bytes) of passes (a) and (c): G = kLoudBlock / channels steps to a workgroup, lane = step * channels + channel;
    a step's chunk of kChunk * channels floats lies at a pitch of `stride` floats in LDS, the least one >= kChunk * channels that is
    `channels` modulo 32"""
    G = k["kLoudBlock"] // channels
    stride = k["kChunk"] * channels
    stride += (channels - stride) % 32
    return G, stride, G * stride * 4


def tiles_of(samples, fs, channels, k):
    """(units, steps, workgroups of (a) that hold a unit, of (c) that hold a step, samples behind the last whole step) of one row"""
    S, G = step_of(fs), launch_plan(channels, k)[0]
    units, steps = -(-samples // S), samples // S
    return units, steps, -(-units // G), -(-steps // G), samples - steps * S


def sine(fs, seconds_and_dbfs, hz=1000.0, channels=2):
    """float32 [samples, channels]: a sine of `hz` whose per-channel peak level follows [(seconds, dBFS), ...], phase running through"""
    total = sum(int(round(sec * fs)) for sec, _ in seconds_and_dbfs)
    amp = np.concatenate([np.full(int(round(sec * fs)), 10.0 ** (db / 20.0)) for sec, db in seconds_and_dbfs])
    x = amp * np.sin(2.0 * np.pi * hz * np.arange(total) / fs)
    return np.repeat(x.astype(np.float32)[:, None], channels, axis=1)


EBU_3341 = {  # case: ([(seconds, dBFS)], target LUFS)
    1: ([(20, -23.0)], -23.0),
    2: ([(20, -33.0)], -33.0),
    3: ([(10, -36.0), (60, -23.0), (10, -36.0)], -23.0),
    4: ([(10, -72.0), (10, -36.0), (60, -23.0), (10, -36.0), (10, -72.0)], -23.0),
}
