"""What the normalisation tests share (include/vorbispizza_pcm_normalize.h states the definition): the numpy BIT MODEL of vpz_pcm_normalize
-- the stated summation order in float64, m and g, the two float32 operations, the int16 conversion --, the numpy.longdouble two-pass
TRUTH with the header's derived bound, and the layout of a call's source array.  Batches are [R, C, J] float32: R windows of C channels
and J real samples each."""
import numpy as np

CHUNK = 1024
MEANVAR, PEAK, RMS, GAIN = 1, 2, 3, 4
MODES = {"meanvar": MEANVAR, "peak": PEAK, "rms": RMS, "gain": GAIN}
U, W = 2.0 ** -53, 2.0 ** -24
SLAB = 1 << 21  # float64 elements the model works on at a time


def _chunk_sums(seg):
    """seg: float64 [..., 1024], chunks padded with +0.0 (which changes no sum): lane l adds samples 256 t + 4 l + i, t then i ascending,
    from 0; the lanes fold by halves"""
    q = seg.reshape(seg.shape[:-1] + (4, 64, 4))
    acc = np.zeros(seg.shape[:-1] + (64,), dtype=np.float64)
    for t in range(4):
        for i in range(4):
            acc = acc + q[..., t, :, i]
    off = 32
    while off >= 1:
        acc = acc[..., :off] + acc[..., off:2 * off]
        off //= 2
    return acc[..., 0]


def sums(x):
    """(S1, S2, P) of every window of x [R, C, J] in the header's order; float64 [R]"""
    x = np.asarray(x, dtype=np.float32)
    R, C, J = x.shape
    S1, S2, P = np.zeros(R), np.zeros(R), np.zeros(R)
    if J == 0 or R == 0:
        return S1, S2, P
    nq = (J + CHUNK - 1) // CHUNK
    step = max(1, SLAB // (C * nq * CHUNK))
    for r0 in range(0, R, step):
        part = x[r0:r0 + step]
        pad = np.zeros((part.shape[0], C, nq * CHUNK), dtype=np.float64)
        pad[:, :, :J] = part
        pad = pad.reshape(part.shape[0], C, nq, CHUNK)
        c1, c2 = _chunk_sums(pad), _chunk_sums(pad * pad)
        a1, a2 = np.zeros(part.shape[0]), np.zeros(part.shape[0])
        for c in range(C):  # ascending by chunk inside a channel, the channels ascending, one accumulator
            for k in range(nq):
                a1 = a1 + c1[:, c, k]
                a2 = a2 + c2[:, c, k]
        S1[r0:r0 + step], S2[r0:r0 + step] = a1, a2
        P[r0:r0 + step] = np.abs(part).reshape(part.shape[0], -1).max(axis=1).astype(np.float64)
    return S1, S2, P


def offset_and_gain(S1, S2, P, N, mode, target=1.0, eps=1e-7, ceiling=0.0, gains=None):
    """m and g of item 2 from downloaded or modelled statistics, float64 [R] holding float32 values"""
    S1, S2, P = (np.asarray(v, dtype=np.float64) for v in (S1, S2, P))
    R = S1.shape[0]
    m, g = np.zeros(R), np.ones(R)
    live = (P > 0) & (N > 0)
    if not live.any():
        return m, g
    Nf = np.float64(max(N, 1))
    with np.errstate(all="ignore"):
        if mode == MEANVAR:
            mm = S1 / Nf
            v = S2 / Nf - mm * mm
            v = np.where(v > 0, v, 0.0)
            gg = 1.0 / np.sqrt(v + np.float64(eps))
        elif mode == PEAK:
            mm, gg = np.zeros(R), np.float64(target) / P
        elif mode == RMS:
            mm, gg = np.zeros(R), np.float64(target) / np.sqrt(S2 / Nf)
        else:
            mm, gg = np.zeros(R), np.ones(R) if gains is None else np.asarray(gains, dtype=np.float64).copy()
        if ceiling > 0:
            gg = np.where(gg * P > ceiling, np.float64(ceiling) / P, gg)
    m[live], g[live] = mm[live], gg[live]
    return m.astype(np.float32).astype(np.float64), g.astype(np.float32).astype(np.float64)


def model(x, mode, target=1.0, eps=1e-7, ceiling=0.0, gains=None):
    """the stage, bit for bit: {y float32 [R, C, J], sum, sum_sq, peak, mean, gain float64 [R]}"""
    x = np.asarray(x, dtype=np.float32)
    R, C, J = x.shape
    S1, S2, P = sums(x)
    m, g = offset_and_gain(S1, S2, P, C * J, mode, target, eps, ceiling, gains)
    with np.errstate(all="ignore"):
        y = (x - m.astype(np.float32)[:, None, None]) * g.astype(np.float32)[:, None, None]
    assert y.dtype == np.float32
    return {"y": y, "sum": S1, "sum_sq": S2, "peak": P, "mean": m, "gain": g}


def plain_gain(x, gains):
    """VPZ_NORM_GAIN without ceiling or result array: no statistics, y = fl32(x * fl32(gain)) -- also for a silent window"""
    x = np.asarray(x, dtype=np.float32)
    return x * np.asarray(gains, dtype=np.float64).astype(np.float32)[:, None, None]


def to_s16(y):
    """the library's one conversion: (int)(y * 32768f) clamped, NaN as 0"""
    with np.errstate(all="ignore"):
        v = (np.asarray(y, dtype=np.float32) * np.float32(32768.0)).astype(np.float64)
    v = np.where(np.isnan(v), 0.0, np.trunc(v))
    return np.clip(v, -32768, 32767).astype(np.int16)


def truth(x, mode, target=1.0, eps=1e-7, ceiling=0.0, gains=None):
    """(y*, bound, rho): the longdouble two-pass restatement -- the mean first, then sum (x - mean)^2 --, the header's bound on |y - y*|
    per element and rho per window (the bound is claimed for rho <= 1 / 2)"""
    L = np.longdouble
    x = np.asarray(x, dtype=np.float32)
    R, C, J = x.shape
    xl = x.astype(L)
    N = C * J
    P = np.abs(xl).reshape(R, -1).max(axis=1) if N else np.zeros(R, dtype=L)
    live = (P > 0) & (N > 0)
    Ps = np.where(live, P, L(1))
    mu = xl.reshape(R, -1).sum(axis=1) / L(max(N, 1)) if N else np.zeros(R, dtype=L)
    var = ((xl - mu[:, None, None]) ** 2).reshape(R, -1).sum(axis=1) / L(max(N, 1)) if N else np.zeros(R, dtype=L)
    e2 = (xl ** 2).reshape(R, -1).sum(axis=1) / L(max(N, 1)) if N else np.zeros(R, dtype=L)
    K = C * ((J + CHUNK - 1) // CHUNK)
    d = 22 + K
    rho = np.zeros(R, dtype=L)
    if mode == MEANVAR:
        g = 1 / np.sqrt(var + L(eps))
        rho = (3 * d + 5) * L(U) * P * P / (var + L(eps)) if eps > 0 or (var > 0).all() else np.full(R, np.inf, dtype=L)
        e_g = rho + 3 * L(U) + L(W)
        dm = (d + 1) * L(U) * P + L(W) * np.abs(mu)
    else:
        mu = np.zeros(R, dtype=L)
        dm = np.zeros(R, dtype=L)
        if mode == PEAK:
            g, e_g = L(target) / Ps, np.full(R, 2 * L(U) + L(W))
        elif mode == RMS:
            g, e_g = L(target) / np.sqrt(np.where(live, e2, L(1))), np.full(R, (d + 4) * L(U) + L(W))
        else:
            g = np.ones(R, dtype=L) if gains is None else np.asarray(gains, dtype=np.float64).astype(L)
            e_g = np.full(R, 2 * L(U) + L(W))
        if ceiling > 0:
            g = np.where(g * P > L(ceiling), L(ceiling) / Ps, g)
    g = np.where(live, g, L(1))
    mu = np.where(live, mu, L(0))
    dm = np.where(live, dm, L(0))
    dev = np.abs(xl - mu[:, None, None])
    grow = ((1 + L(W)) ** 2 * (1 + e_g) - 1)[:, None, None]
    bound = g[:, None, None] * ((dev + dm[:, None, None]) * grow + dm[:, None, None]) + L(2.0) ** -150
    return (xl - mu[:, None, None]) * g[:, None, None], bound, rho


def worst_ratio(y, ystar, bound):
    """largest |y - y*| / bound over the elements (0 where there are none)"""
    if np.asarray(y).size == 0:
        return 0.0
    return float(np.max(np.abs(np.asarray(y).astype(np.longdouble) - ystar) / bound))


def signal(kind, C, J, seed):
    """a window [C, J] float32 of one of the tests' kinds"""
    rng = np.random.default_rng(seed)
    t = np.arange(C * J, dtype=np.float64).reshape(C, J)
    if kind == "noise":
        x = rng.uniform(-1.0, 1.0, (C, J))
    elif kind == "zero":
        x = np.zeros((C, J))
    elif kind == "constant":
        x = np.full((C, J), 0.3)
    elif kind == "outlier":  # one sample of 1e4 among values of 1e-4
        x = rng.uniform(-1e-4, 1e-4, (C, J))
        if C * J:
            x.reshape(-1)[(C * J) // 3] = 1e4
    elif kind == "dc":  # full scale, a DC offset of 0.9 and a ripple of 1e-4: the cancellation case of the one-pass variance
        x = 0.9 + 1e-4 * np.sin(0.37 * t)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def lay_out(windows, frames, gaps):
    """the source array of a call: planar windows [C, J] as [C][frames] blocks -- the samples behind J are NaN, so that a read past a
    window's end shows --, window i `gaps[i]` NaN elements behind the one before; returns (float32 array, [src offsets])"""
    parts, offs, at = [], [], 0
    for w, gap in zip(windows, gaps):
        C, J = w.shape
        parts.append(np.full(gap, np.nan, dtype=np.float32))
        at += gap
        offs.append(at)
        block = np.full((C, frames), np.nan, dtype=np.float32)
        block[:, :J] = w
        parts.append(block.reshape(-1))
        at += C * frames
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32), offs


def expected_rows(y, frames, planar, s16):
    """model values [R, C, J] as destination rows [R, C, frames] or [R, frames, C], padded with zeros, float32 or int16"""
    R, C, J = y.shape
    full = np.zeros((R, C, frames), dtype=np.float32)
    full[:, :, :J] = y
    out = to_s16(full) if s16 else full
    return np.ascontiguousarray(out if planar else out.transpose(0, 2, 1))
