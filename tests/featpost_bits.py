"""THE BITS of the feature post-processing tests (a helper, not a test): include/vorbispizza_pcm_featpost.h's definition as a host model
that gives the float32 BITS the header promises, written from the header's text and not from the kernels -- where tests/featpost_truth.py
restates the same definition in longdouble with a bound, and so cannot tell one order of the sums from another.
tests/test_featpost_bits_cpu.py holds the model to the truth's bound and shows that it tells the orders apart;
tests/test_pcm_featpost_limits_gpu.py compares the device with it bit for bit.

Item 1, deltas.  The scales are featpost_truth.scales(i, w) rounded to float32; the chain runs j ascending from an accumulator of 0, every
step one float32 fused multiply-add, a zero scale skipped.  fma32 is vectorised: the product of two float32 is exact in float64, TwoSum
gives the error of the float64 sum exactly, and the sum is rounded once to float32 -- which is the fused result unless the float64 sum
lies exactly midway between two float32 values while the error is not zero; then the error's sign decides.  (Round to nearest is
monotonic, and the midpoint is a float64: a float64 sum on one side of it has its exact value on the same side.)
Item 3, normalisation.  Float64 chunk sums, frames ascending (a float32 square is exact in float64, so `s2 + x * x` is the fused step); a
window's sums are L, the whole chunks with k ascending, R, with e = min(b, 64 * ceil(a / 64)); m = S1 / c; v = fma(-m, m, S2 / c) in exact
rationals (one per window and column), rounded once.  numpy's float64 division and square root are correctly rounded, its conversion to
float32 rounds to nearest even, and it flushes no subnormal.
Item 4, composition: the two models in `order`, the tensor between them float32; at any D (the host has no limit of 256 columns).

ORDERS other than the stated one stand beside it (`order=` of normalise) for the test that the model discriminates:
    "running"       one running sum over [a, b), ascending from 0
    "descending"    the partial chunks L and R summed with their frames descending
    "r_first"       the parts added R, L, whole chunks
    "chunks_first"  the parts added whole chunks, L, R
and for the deltas `descending=True` (j from + i w down) and `fused=False` (a float32 product, then a float32 sum).

spiked(n, D, seed, far) is an input on which the order of float64 sums reaches the float32 output: noise with cancelling pairs +M, -M,
M = 2^36 .. 2^43, so that a window holding both halves of a pair has partial sums near M, where a float64 rounds at 2^-17 .. 2^-10, and a
result near 1."""
from fractions import Fraction

import numpy as np

import featpost_truth as pt
from f32_model import fma32


# (name, n, D, seed, far, the sliding spec): the spiked cases, mean only
SPIKED = [
    ("near W 100", 330, 4, 7, False, dict(norm="sliding", cmn_window=100, min_window=30)),
    ("near W 200 centred", 330, 4, 7, False, dict(norm="sliding", cmn_window=200, min_window=1, center=True)),
    ("near W 4", 330, 4, 7, False, dict(norm="sliding", cmn_window=4, min_window=2)),
    ("far W 300 centred", 700, 3, 7, True, dict(norm="sliding", cmn_window=300, min_window=1, center=True)),
    ("far W 600", 700, 3, 7, True, dict(norm="sliding", cmn_window=600, min_window=100)),
]
ROW_SPIKED = [("near row", 330, 4, 7, False, dict(norm="row")), ("far row", 700, 3, 7, True, dict(norm="row"))]


F32, F64 = np.float32, np.float64
CHUNK = pt.CHUNK
ORDERS = ("running", "descending", "r_first", "chunks_first")


def fma64(a, b, c):
    """Python floats -> fl64(a * b + c), one rounding, in exact rationals (a Fraction's float() is correctly rounded)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def scales32(i, w):
    return pt.scales(i, w).astype(F32)


def deltas(x, d, descending=False, fused=True):
    """x: float32 [n, D] -> float32 [n, D * (order + 1)]: item 1"""
    n, D = x.shape
    x = np.ascontiguousarray(x, dtype=F32)
    out = [x]
    t = np.arange(n)
    for i in range(1, d["delta_order"] + 1):
        s, H = scales32(i, d["delta_window"]), i * d["delta_window"]
        acc = np.zeros((n, D), dtype=F32)
        for j in (range(H, -H - 1, -1) if descending else range(-H, H + 1)):
            if s[j + H] == 0 or n == 0:
                continue
            tap = x[np.clip(t + j, 0, n - 1)]
            acc = fma32(s[j + H], tap, acc) if fused else ((s[j + H] * tap).astype(F32) + acc).astype(F32)
        out.append(acc)
    return np.concatenate(out, axis=1)


def windows(d, n):
    """a, b of every frame of a row of n real frames: int64 [n] each"""
    ab = np.array([pt.window(d, t, n) for t in range(n)], dtype=np.int64).reshape(n, 2)
    return ab[:, 0], ab[:, 1]


def _span_sums(X, Q, lo, hi, descending=False):
    """per frame t the float64 sums of X and Q over [lo[t], hi[t]) from an accumulator of 0, ascending (or descending): [n, D] each"""
    s1, s2 = np.zeros((len(lo), X.shape[1])), np.zeros((len(lo), X.shape[1]))
    for k in range(int((hi - lo).max()) if len(lo) else 0):
        idx = hi - 1 - k if descending else lo + k
        live = np.nonzero(lo + k < hi)[0]
        s1[live] += X[idx[live]]
        s2[live] += Q[idx[live]]
    return s1, s2


def window_sums(x, d, order=None):
    """x: float32 [n, D] -> S1, S2 float64 [n, D] of every frame's window in the header's order (or one of ORDERS), and c int64 [n]"""
    n, D = x.shape
    X = x.astype(F64)
    Q = X * X  # exact
    a, b = windows(d, n)
    if order == "running":
        return _span_sums(X, Q, a, b) + (b - a,)
    e = np.minimum(b, (a + CHUNK - 1) // CHUNK * CHUNK)
    nwhole = np.maximum(b // CHUNK - e // CHUNK, 0)  # (e is a chunk boundary wherever this is not 0)
    u = e + nwhole * CHUNK
    # the whole chunks' sums, frames ascending
    nck = (n + CHUNK - 1) // CHUNK
    starts = np.arange(nck, dtype=np.int64) * CHUNK
    C1, C2 = _span_sums(X, Q, starts, np.minimum(starts + CHUNK, n))
    desc = order == "descending"
    L1, L2 = _span_sums(X, Q, a, e, desc)
    R1, R2 = _span_sums(X, Q, u, b, desc)
    S1, S2 = np.zeros((n, D)), np.zeros((n, D))

    def add_chunks():
        for k in range(int(nwhole.max())):
            live = np.nonzero(k < nwhole)[0]
            S1[live] += C1[e[live] // CHUNK + k]
            S2[live] += C2[e[live] // CHUNK + k]

    def add(P1, P2, lo, hi):  # (what is empty is left out)
        live = np.nonzero(hi > lo)[0]
        S1[live] += P1[live]
        S2[live] += P2[live]

    if order == "r_first":
        add(R1, R2, u, b), add(L1, L2, a, e), add_chunks()
    elif order == "chunks_first":
        add_chunks(), add(L1, L2, a, e), add(R1, R2, u, b)
    else:
        assert order in (None, "descending"), order
        add(L1, L2, a, e), add_chunks(), add(R1, R2, u, b)
    return S1, S2, b - a


def normalise(x, d, order=None):
    """x: float32 [n, D] -> float32 [n, D]: items 2 and 3"""
    n, D = x.shape
    x = np.ascontiguousarray(x, dtype=F32)
    if n == 0:
        return x.copy()
    S1, S2, c = window_sums(x, d, order)
    cf = c.astype(F64)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = S1 / cf
        xd = x.astype(F64) - m
        if not d["norm_vars"]:
            return xd.astype(F32)
        q = S2 / cf
        v = np.array([fma64(-mm, mm, qq) if np.isfinite(mm) and np.isfinite(qq) else np.nan
                      for mm, qq in zip(m.ravel().tolist(), q.ravel().tolist())], dtype=F64).reshape(n, D)
        floor = F64(d["var_floor"])
        v = np.where(v >= floor, v, floor)
        return np.where(cf == 1, xd * 0.0, xd / np.sqrt(v)).astype(F32)


def model(x, d, order=None):
    """the real frames x: float32 [n, D] -> float32 [n, D_out]: the whole spec, item 4 included"""
    if d["norm"] == "none":
        return deltas(x, d)
    if d["delta_order"] == 0:
        return normalise(x, d, order)
    if d["deltas_first"]:
        return normalise(deltas(x, d), d, order)
    return deltas(normalise(x, d, order), d)


def spiked(n, D, seed, far=False):
    """seeded N(0, 1) float32 [n, D]; per column, every 5 to 19 frames a cancelling pair +M, -M with M = 2^k, k = 36 .. 43, written over
    it, the second half 1 to 3 frames behind the first -- with `far`, every fourth pair 40 to 99 frames behind, across a chunk boundary.
    A pair is written only where both frames are inside the row and still noise, so every pair cancels"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D)).astype(F32)
    for c in range(D):
        taken = np.zeros(n, dtype=bool)
        t, pairs = int(rng.integers(0, 5)), 0
        while t < n:
            lag = int(rng.integers(40, 100)) if far and pairs % 4 == 3 else int(rng.integers(1, 4))
            M = F32(2.0 ** int(rng.integers(36, 44)))
            if t + lag < n and not taken[t] and not taken[t + lag]:
                x[t, c], x[t + lag, c] = M, -M
                taken[t] = taken[t + lag] = True
            pairs += 1
            t += int(rng.integers(5, 20))
    return x


def share(a, b):
    """the share of elements whose bits differ"""
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())
