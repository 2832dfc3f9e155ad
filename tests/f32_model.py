"""The float32 model the restatements are written in: the unit roundoff, ONE exactly rounded vectorised fused multiply-add, the complex
product as the headers write it, and the rational reference that holds the vectorised one (tests/test_featpost_bits_cpu.py and
test_fma32_is_the_exact_one of tests/test_pcm_context_state_gpu.py)."""
import numpy as np

U = 2.0 ** -24


def fma32(a, b, c):
    """float32 fused multiply-add, correctly rounded, element by element: the float32 product is exact in float64; the float64 sum is
    rounded to odd (TwoSum gives what it lost), so that the second rounding, to float32, is the only one that counts.  A sum that is
    not finite stays as float64 made it."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = (e != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def cmul(tr, ti, vr, vi):
    """t * v as the headers write it"""
    return fma32(vr, tr, -(vi * ti)), fma32(vr, ti, vi * tr)


def network32(X, n_fft, w, t):
    """(re, im) = (Re X, Im X), float32 [T, n_fft / 2 + 1]: the real FFT network of the melspec and STFT headers, step for step on
    float32 frames X, with the float32 tables w [n_fft] and t [n_fft, 2]"""
    H = n_fft // 2
    X = np.asarray(X, dtype=np.float32)
    y = X * w[None, :]
    zr, zi = y[:, 0::2].copy(), y[:, 1::2].copy()
    n, s = H, 1
    while n >= 4:
        q4 = n // 4
        ar, ai = zr.reshape(-1, 4, q4, s), zi.reshape(-1, 4, q4, s)  # in[q + s (p + j n/4)] as [T, j, p, q]
        a_r, b_r, c_r, d_r = ar[:, 0], ar[:, 1], ar[:, 2], ar[:, 3]
        a_i, b_i, c_i, d_i = ai[:, 0], ai[:, 1], ai[:, 2], ai[:, 3]
        apc_r, apc_i, amc_r, amc_i = a_r + c_r, a_i + c_i, a_r - c_r, a_i - c_i
        bpd_r, bpd_i, bmd_r, bmd_i = b_r + d_r, b_i + d_i, b_r - d_r, b_i - d_i
        p = np.arange(q4)
        t1, t2, t3 = t[2 * p * s][None, :, None, :], t[4 * p * s][None, :, None, :], t[6 * p * s][None, :, None, :]
        o0r, o0i = apc_r + bpd_r, apc_i + bpd_i
        o1r, o1i = cmul(t1[..., 0], t1[..., 1], amc_r + bmd_i, amc_i - bmd_r)
        o2r, o2i = cmul(t2[..., 0], t2[..., 1], apc_r - bpd_r, apc_i - bpd_i)
        o3r, o3i = cmul(t3[..., 0], t3[..., 1], amc_r - bmd_i, amc_i + bmd_r)
        zr = np.stack([o0r, o1r, o2r, o3r], axis=2).reshape(-1, H)  # out[q + s (4p + j)] as [T, p, j, q]
        zi = np.stack([o0i, o1i, o2i, o3i], axis=2).reshape(-1, H)
        n, s = n // 4, s * 4
    if n == 2:
        ar, ai = zr.reshape(-1, 2, s), zi.reshape(-1, 2, s)
        zr = np.concatenate([ar[:, 0] + ar[:, 1], ar[:, 0] - ar[:, 1]], axis=1)
        zi = np.concatenate([ai[:, 0] + ai[:, 1], ai[:, 0] - ai[:, 1]], axis=1)
    k = np.arange(H // 2 + 1)
    m = (H - k) % H
    half = np.float32(0.5)
    Er, Ei = (zr[:, k] + zr[:, m]) * half, (zi[:, k] - zi[:, m]) * half
    Or, Oi = (zi[:, k] + zi[:, m]) * half, (zr[:, m] - zr[:, k]) * half
    tr, ti = cmul(t[k, 0][None, :], t[k, 1][None, :], Or, Oi)
    re_, im_ = np.zeros((X.shape[0], H + 1), np.float32), np.zeros((X.shape[0], H + 1), np.float32)
    re_[:, H - k], im_[:, H - k] = Er - tr, -(Ei - ti)  # conj(E - t O)
    re_[:, k], im_[:, k] = Er + tr, Ei + ti            # (bin H / 2 is its own mirror: E + t O stands)
    return re_, im_


def fma32_rational(a, b, c):
    """one float32 fused multiply-add: the exact a * b + c (rationals), rounded once"""
    from fractions import Fraction
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = np.float32(float(exact))  # (rounded twice: at most one float32 off; the neighbours decide)
    best = min((near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))),
               key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)
