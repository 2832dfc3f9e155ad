"""The PCM stages' harness, shared by the tests/test_pcm_*_gpu.py and tests/test_pcm_*_limits_gpu.py families: sentinel-guarded destinations
(`guarded` for float32 rows, `guarded_layout` for the resampler's four layouts), source placement, signals, the layout constants and the
resampler's run over all layouts.  What differs in substance between kinds stays with the kind."""
import numpy as np

from resample_truth import bound, to_s16


SENTINEL = 0x5A5A5A5A
GUARD = 64


def signal(n, seed, sample_rate=16000, amplitude=0.3):
    """seeded noise plus a tone, float32"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    return (amplitude * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 440.0 * t / sample_rate + 0.3)).astype(np.float32)


def place(windows, gap=3):
    """one source array for these windows (float32 arrays): window i at an offset that is odd for odd i and a multiple of 4 for even i,
    NaN between and behind them (what lies at or behind src + L must not be read).  -> (src, offsets)"""
    offs, at = [], 0
    for i, w in enumerate(windows):
        at += gap
        at += (-at) % 4 if i % 2 == 0 else (at + 1) % 2
        offs.append(at)
        at += len(w)
    src = np.full(at + gap, np.nan, dtype=np.float32)
    for o, w in zip(offs, windows):
        src[o: o + len(w)] = w
    return src, offs


def guarded(dst_rows, row_elems):
    """a destination of dst_rows * row_elems float32 with GUARD sentinels on either side, every element the sentinel"""
    import torch
    flat = np.full(GUARD + dst_rows * row_elems + GUARD, SENTINEL, dtype=np.uint32)
    whole = torch.from_numpy(flat.view(np.float32).copy()).to("cuda:0")
    return whole, whole[GUARD: GUARD + dst_rows * row_elems]


FLOOR = 1e-10
LOGMEL_DST_ROWS = 9


def rows_back(whole, dst_rows, n_mels, T, bands_first):
    """[row][T][n_mels] float32 of the destination's body, after checking the guards"""
    bits = whole.cpu().numpy().view(np.uint32)
    assert (bits[:GUARD] == SENTINEL).all() and (bits[-GUARD:] == SENTINEL).all()
    body = bits[GUARD:-GUARD].view(np.float32)
    return body.reshape(dst_rows, n_mels, T).transpose(0, 2, 1) if bands_first else body.reshape(dst_rows, T, n_mels)


INTERLEAVED, PLANAR, INTERLEAVED_S16, PLANAR_S16 = 0, 1, 2, 3
RESAMPLE_DST_ROWS = 13


def out_len(L, up, down):
    return -(-L * up // down)


def random_source(n, seed):
    """n float32 in +-1.25 (so that the int16 conversion clamps now and then), none of them zero"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.25, 1.25, n).astype(np.float32)
    a[a == 0] = np.float32(0.5)
    assert (a != 0).all()
    return a


def layout_windows(Ls, channels, rng):
    """every window from an ODD element offset, at least 9 elements of other data in front of it and behind it"""
    rows, at = [], 0
    order = rng.permutation(RESAMPLE_DST_ROWS)[: len(Ls)]
    for L, row in zip(Ls, order):
        at += 9 + int(rng.integers(0, 5))
        at += 1 - at % 2
        rows.append((at, L, int(row)))
        at += L * channels
    return rows, at + 11


def guarded_layout(dst_rows, channels, frames, layout, guard):
    import torch
    s16 = layout in (INTERLEAVED_S16, PLANAR_S16)
    body = dst_rows * channels * frames
    flat = np.full(guard + body + guard, 0x5A5A if s16 else 0x5A5A5A5A, dtype=np.uint16 if s16 else np.uint32)
    whole = torch.from_numpy(flat.view(np.int16 if s16 else np.float32).copy()).to("cuda:0")
    shape = (dst_rows, channels, frames) if layout in (PLANAR, PLANAR_S16) else (dst_rows, frames, channels)
    return whole, whole[guard: guard + body].view(shape), flat


def rows_of(whole, guard, dst_rows, channels, frames, layout):
    """the destination as [row][frame][channel] numpy (float32 or int16), and the two guards' bits"""
    a = whole.cpu().numpy()
    body = a[guard: a.size - guard]
    img = body.reshape(dst_rows, channels, frames).transpose(0, 2, 1) if layout in (PLANAR, PLANAR_S16) else body.reshape(dst_rows, frames, channels)
    bits = a.view(np.uint16 if a.dtype == np.int16 else np.uint32)
    return img, bits[:guard], bits[a.size - guard:]


def run_layouts(ctx, src_np, rows, channels, downmix, up, down, frames, guards, layouts, truths):
    """one call per layout over the same descriptors; the float32 outputs against the truth, the int16 ones against the float32 ones"""
    import torch
    from vorbispizza_amd import capi
    src = torch.from_numpy(src_np).to("cuda:0").view(-1, channels) if src_np.size % channels == 0 else None
    assert src is not None
    co = 1 if downmix else channels
    named = {row for _, _, row in rows}
    f32 = {}
    worst = 0.0
    for layout, guard in zip(layouts, guards):
        whole, dst, flat = guarded_layout(RESAMPLE_DST_ROWS, co, frames, layout, guard)
        assert capi.pcm_resample(ctx, src, rows, dst, layout, up, down, downmix) == capi.OK, ctx.last_error()
        ctx.synchronize()
        img, g0, g1 = rows_of(whole, guard, RESAMPLE_DST_ROWS, co, frames, layout)
        sent = flat[0]
        assert (g0 == sent).all() and (g1 == sent).all(), "a guard was written"
        bits = img.view(np.uint16 if img.dtype == np.int16 else np.uint32)
        for r in range(RESAMPLE_DST_ROWS):
            if r not in named:
                assert (bits[r] == sent).all(), ("an unnamed row was written", r)
        for (at, L, row), (y, B) in zip(rows, truths):
            J = out_len(L, up, down)
            assert (bits[row, J:] == 0).all(), ("not zero bits behind the samples", layout, L, row)
            if layout in (INTERLEAVED, PLANAR):
                err = np.abs(img[row, :J].astype(np.float64) - y)
                tol = bound(B, up, down, channels if downmix else 1)
                if J:
                    worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
                assert (err <= tol).all(), (layout, channels, downmix, up, down, L, int(np.argmax(err - tol)), float(err.max()))
                f32.setdefault((row, L), img[row, :J].copy())
            else:
                assert (row, L) in f32, "the int16 layouts come after a float32 one"
                assert img[row, :J].tobytes() == to_s16(f32[(row, L)]).tobytes(), ("int16 is not the conversion of the float32 output", layout, L)
        # the float32 layouts agree bit for bit with each other (the same arithmetic, another store)
        for (at, L, row) in rows:
            if layout in (INTERLEAVED, PLANAR):
                assert img[row, :out_len(L, up, down)].tobytes() == f32[(row, L)].tobytes()
    assert (torch.from_numpy(src_np).to("cuda:0") == src.view(-1)).all()
    return worst
