"""vpz_feat_post on the device, shared by tests/test_pcm_featpost_gpu.py and tests/test_pcm_featpost_limits_gpu.py: the layouts, the
feature batches, the launch into a guarded destination, and the row check with its record of the worst error / bound."""
import numpy as np

import featpost_truth as pt
from pcm_support import GUARD, SENTINEL, guarded


WORST = {}
LAYOUTS = [True, False]


def feats(n, D, seed, offset=0.0, scale=1.0):
    """seeded noise around a slow ramp per column, float32 [n, D]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)[:, None]
    return (offset + scale * (rng.standard_normal((n, D)) + 0.01 * t * np.cos(np.arange(D))[None, :])).astype(np.float32)


def batch(xs, T):
    """the source tensor [len(xs), T, D] of these rows' real frames, NaN behind them (what lies behind a row's n must not be read)"""
    D = xs[0].shape[1]
    src = np.full((len(xs), T, D), np.nan, dtype=np.float32)
    for i, x in enumerate(xs):
        src[i, :len(x)] = x
    return src


def launch(ctx, d, src, rows, dst_rows, want_rc=None):
    """one vpz_feat_post call of spec dict d over src [src_rows, T, D] (frames first here; laid out as d says on the device) ->
    [dst_rows, T, D_out] float32 of the destination's body, the guards checked"""
    import torch
    from vorbispizza_amd import capi
    spec = capi.FeatPostSpec.make(**d)
    src_rows, T, D = src.shape
    Do = spec.out_columns(D)
    ff = d["frames_first"]
    whole, dst = guarded(dst_rows, T * Do)
    d_src = torch.from_numpy(np.ascontiguousarray(src if ff else src.transpose(0, 2, 1))).to("cuda:0")
    shape = (dst_rows, T, Do) if ff else (dst_rows, Do, T)
    rc = capi.feat_post(ctx, d_src, rows, dst.view(shape), spec)
    assert rc == (capi.OK if want_rc is None else want_rc), ctx.last_error()
    ctx.synchronize()
    bits = whole.cpu().numpy().view(np.uint32)
    assert (bits[:GUARD] == SENTINEL).all() and (bits[-GUARD:] == SENTINEL).all()
    body = bits[GUARD:-GUARD].view(np.float32).reshape(shape)
    return body if ff else body.transpose(0, 2, 1)


def by_column_slices(ctx, d, src, rows, dst_rows):
    """the normalisation d (no deltas) of src [src_rows, T, any number of columns], one call per slice of 256 columns -- a call's source
    has 256 at the most, and a column's values depend on no other column -- put side by side again"""
    assert d["delta_order"] == 0
    return np.concatenate([launch(ctx, d, np.ascontiguousarray(src[:, :, c:c + 256]), rows, dst_rows) for c in range(0, src.shape[2], 256)], axis=2)


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("error / bound %s: %.4f" % (key, ratio))
    assert ratio <= 1.0


def check_rows(key, got, xs, d, order):
    """every row of `order` against the truth of its real frames; pad frames exact"""
    pad_bits = np.float32(d["pad_value"]).view(np.uint32)
    for x, r in zip(xs, order):
        n = len(x)
        assert (got[r, n:].view(np.uint32) == pad_bits).all(), (key, n)
        if n:
            want, bound = pt.truth(x, d)
            note(key, pt.ratio(got[r, :n], want, bound))
