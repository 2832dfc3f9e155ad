"""vpz_pcm_pack (include/vorbispizza_pcm_pack.h, csrc/pcm_pack.hip) alone: no decoder.  The source is a torch tensor of seeded random BIT
patterns (float32: -0.0, denormals, NaN payloads and infinities among them; int16: the extremes), the expected destination is built with
numpy and compared as raw bits.  Guard elements on either side of the destination and the rows no descriptor names hold a sentinel
that must survive; the guards' sizes also move the destination off every 16-byte boundary, so whole tiles, partial first and last
tiles, aligned and unaligned sources all occur.  Every refusal of the header returns VPZ_E_INVALID_ARG and writes nothing."""
import os
import sys

import numpy as np
import pytest
from gpu_context import ctx  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

LAYOUTS = {"interleaved": 0, "planar": 1, "interleaved_s16": 2, "planar_s16": 3}
FRAMES = (1, 7, 64, 1023, 1024, 1025)


def is_s16(layout):
    return layout in (2, 3)


def source(n, s16, seed):
    """n elements of random bits as a numpy integer array (uint32 / uint16), the notable patterns sown in"""
    rng = np.random.default_rng(seed)
    if s16:
        a = rng.integers(0, 1 << 16, n, dtype=np.uint16)
        notable = [0x8000, 0x7FFF, 0xFFFF, 0x0000, 0x0001]
    else:
        a = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        notable = [0x80000000, 0x00000001, 0x807FFFFF, 0x007FFFFF, 0x7FC00001, 0xFF800000, 0x00000000]
    for i, v in enumerate(notable * 8):
        a[(i * 37 + 5) % n] = v
    return a


def to_device(bits, s16):
    import torch
    return torch.from_numpy(bits.view(np.int16 if s16 else np.float32).copy()).to("cuda:0")


def bits_of(t, s16):
    import torch
    return t.view(torch.int16 if s16 else torch.int32).cpu().numpy().view(np.uint16 if s16 else np.uint32)


def sentinel(s16):
    return np.uint16(0x5A5A) if s16 else np.uint32(0x5A5A5A5A)


def guarded(dst_rows, channels, frames, layout, guard):
    """(whole flat device tensor, the destination view inside it, the flat numpy image of a correct call's start: all sentinel)"""
    import torch
    s16 = is_s16(layout)
    body = dst_rows * channels * frames
    flat = np.full(guard + body + guard, sentinel(s16))
    whole = to_device(flat, s16)
    shape = (dst_rows, channels, frames) if layout in (1, 3) else (dst_rows, frames, channels)
    view = whole[guard: guard + body].view(shape)
    assert view.data_ptr() == whole.data_ptr() + guard * whole.element_size() and isinstance(view, torch.Tensor)
    return whole, view, flat


def expect(flat, guard, src_bits, rows, channels, frames, layout):
    body = channels * frames
    for src, samples, row in rows:
        img = np.zeros((frames, channels), dtype=src_bits.dtype)
        img[:samples] = src_bits[src: src + samples * channels].reshape(samples, channels)
        if layout in (1, 3):
            img = img.T
        flat[guard + row * body: guard + (row + 1) * body] = img.reshape(-1)
    return flat


def descriptors(frames, channels, seed):
    """eight windows over twelve rows, out of order and with gaps: samples 0, 1, frames - 1, frames (where they fit), each from an odd
    source offset and from a multiple of 8 elements"""
    rng = np.random.default_rng(seed)
    counts = (0, 1, frames - 1, frames)  # (frames >= 1: they all fit)
    picked = list(rng.permutation(12)[:8])
    rows, at = [], 0
    for i, row in enumerate(picked):
        samples, odd = counts[i % 4], i < 4
        at = (at + 7) // 8 * 8 + (int(rng.integers(0, 4)) * 2 + 1 if odd else 0)
        rows.append((at, samples, int(row)))
        at += samples * channels
    return rows, at + 8


@pytest.mark.parametrize("channels", [1, 2, 6])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_named_row_is_the_window_then_zeros(ctx, layout, channels):
    from vorbispizza_amd import capi
    lay, s16 = LAYOUTS[layout], is_s16(LAYOUTS[layout])
    seen = set()
    for frames in FRAMES:
        for guard in (16, 3, 5):  # (elements: the destination at a 16-byte boundary, and off it by an odd number of elements)
            rows, src_elems = descriptors(frames, channels, seed=frames * 10 + guard)
            seen |= {(s == frames, s == 0, a % 8 == 0, a % 2 == 1) for a, s, _ in rows}
            src_bits = source(src_elems, s16, seed=frames + channels)
            src = to_device(src_bits, s16)
            whole, dst, flat = guarded(12, channels, frames, lay, guard)
            assert capi.pcm_pack(ctx, src, rows, dst, lay) == capi.OK, ctx.last_error()
            ctx.synchronize()
            want = expect(flat, guard, src_bits, rows, channels, frames, lay)
            got = bits_of(whole, s16)
            assert got.tobytes() == want.tobytes(), (layout, channels, frames, guard, np.flatnonzero(got != want)[:8])
            assert bits_of(src, s16).tobytes() == src_bits.tobytes()
    # whole and empty windows, from odd offsets and from multiples of 8 elements
    assert {(True, False, True, False), (True, False, False, True), (False, True, True, False), (False, True, False, True)} <= seen, seen


def test_more_descriptors_than_the_grid_is_high(ctx):
    """a workgroup takes several descriptors when there are more of them than the grid's second dimension"""
    from vorbispizza_amd import capi
    n, channels, frames = 4500, 2, 7
    rng = np.random.default_rng(3)
    order = rng.permutation(n + 100)[:n]
    rows = [(int(k) * 3 + 1, int(rng.integers(0, frames + 1)), int(r)) for k, r in enumerate(order)]
    src_bits = source(n * 3 + 1 + frames * channels, False, 9)
    whole, dst, flat = guarded(n + 100, channels, frames, 1, 3)
    assert capi.pcm_pack(ctx, to_device(src_bits, False), rows, dst, 1) == capi.OK, ctx.last_error()
    ctx.synchronize()
    assert bits_of(whole, False).tobytes() == expect(flat, 3, src_bits, rows, channels, frames, 1).tobytes()


def test_indices_beyond_two_to_the_31(ctx):
    """the last row of a destination and a window of a source whose element indices do not fit 32 bits"""
    import torch
    from vorbispizza_amd import capi
    channels, frames = 2, 1024
    dst_rows = (1 << 31) // (channels * frames) + 2
    src_elems = (1 << 31) + 4096
    src = torch.empty(src_elems, dtype=torch.int16, device="cuda:0")
    tail = source(4096, True, 4)
    src[1 << 31:] = to_device(tail, True)
    for lay in (3, 2):
        dst = torch.empty((dst_rows, channels, frames) if lay == 3 else (dst_rows, frames, channels), dtype=torch.int16, device="cuda:0")
        dst[-3:] = 0x5A5A
        rows = [((1 << 31) + 3, 1000, dst_rows - 1), ((1 << 31) + 2048, frames, dst_rows - 3)]
        assert capi.pcm_pack(ctx, src, rows, dst, lay) == capi.OK, ctx.last_error()
        ctx.synchronize()
        want = expect(np.full(3 * channels * frames, sentinel(True)), 0, tail, [(3, 1000, 2), (2048, frames, 0)], channels, frames, lay)
        assert bits_of(dst[-3:], True).tobytes() == want.tobytes(), lay
        del dst


def raw_call(ctx, src_ptr, src_elems, channels, rows, dst_ptr, dst_rows, frames, layout, n_rows=None, null_rows=False, handle=True):
    from vorbispizza_amd import capi
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    return capi.lib().vpz_pcm_pack(ctx._h if handle else None, src_ptr, src_elems, channels, desc.shape[0] if n_rows is None else n_rows,
                                   None if null_rows else desc.ctypes.data, dst_ptr, dst_rows, frames, layout)


@pytest.mark.parametrize("layout", ["planar", "interleaved_s16"])
def test_every_refusal_is_invalid_arg_and_writes_nothing(ctx, layout):
    import torch
    from vorbispizza_amd import capi
    lay, s16 = LAYOUTS[layout], is_s16(LAYOUTS[layout])
    channels, frames, dst_rows, guard = 2, 64, 4, 16
    src_bits = source(1000, s16, 11)
    src = to_device(src_bits, s16)
    whole, dst, flat = guarded(dst_rows, channels, frames, lay, guard)
    good = dict(src_ptr=src.data_ptr(), src_elems=1000, channels=channels, rows=[(3, 10, 1), (40, 64, 3)], dst_ptr=dst.data_ptr(),
                dst_rows=dst_rows, frames=frames, layout=lay)
    elem = 2 if s16 else 4
    pinned = torch.full((dst_rows, channels, frames), 77, dtype=torch.int16 if s16 else torch.float32, pin_memory=True)
    assert pinned.is_pinned() and not pinned.is_cuda
    host_src = torch.full((1000,), 3, dtype=torch.int16 if s16 else torch.float32, pin_memory=True)
    refused = {
        "null context": dict(handle=False),
        "null source": dict(src_ptr=None),
        "null destination": dict(dst_ptr=None),
        "null descriptors": dict(null_rows=True),
        "no channels": dict(channels=0),
        "too many channels": dict(channels=capi.MAX_CHANNELS + 1),
        "no frames": dict(frames=0),
        "negative descriptor count": dict(n_rows=-1),
        "negative row count": dict(dst_rows=-1),
        "negative source size": dict(src_elems=-1),
        "layout 4": dict(layout=4),
        "layout -1": dict(layout=-1),
        "source starts before the array": dict(rows=[(-1, 10, 1)]),
        "source ends behind the array": dict(rows=[(1000 - 10 * channels + 1, 10, 1)]),
        "source starts behind the array": dict(rows=[(1001, 0, 1)]),
        "more samples than frames": dict(rows=[(0, frames + 1, 1)]),
        "negative samples": dict(rows=[(0, -1, 1)]),
        "row behind the last": dict(rows=[(0, 1, dst_rows)]),
        "negative row": dict(rows=[(0, 1, -1)]),
        "a row named twice": dict(rows=[(0, 1, 2), (8, 3, 0), (16, 2, 2)]),
        "more descriptors than rows": dict(rows=[(0, 1, 0)] * (dst_rows + 1)),
        "destination off its element": dict(dst_ptr=dst.data_ptr() + 1),
        "source off its element": dict(src_ptr=src.data_ptr() + elem // 2, src_elems=999),
        "page-locked host destination": dict(dst_ptr=pinned.data_ptr()),
        "page-locked host source": dict(src_ptr=host_src.data_ptr()),
        # (row 1 alone is named and lies inside the tensor: without the range check the call would succeed)
        "destination longer than its allocation": dict(dst_rows=(1 << 40) // (channels * frames * elem)),
        "source longer than its allocation": dict(src_elems=1 << 38),
    }
    for what, change in refused.items():
        assert raw_call(ctx, **{**good, **change}) == capi.E_INVALID_ARG, what
    ctx.synchronize()
    assert bits_of(whole, s16).tobytes() == flat.tobytes()
    assert (pinned == 77).all()
    # ... and the call they were all made from is a good one
    assert raw_call(ctx, **good) == capi.OK, ctx.last_error()
    ctx.synchronize()
    assert bits_of(whole, s16).tobytes() == expect(flat, guard, src_bits, good["rows"], channels, frames, lay).tobytes()
    # no descriptors: nothing to do, nothing written
    before = bits_of(whole, s16).copy()
    assert raw_call(ctx, **{**good, "rows": []}) == capi.OK
    ctx.synchronize()
    assert bits_of(whole, s16).tobytes() == before.tobytes()
