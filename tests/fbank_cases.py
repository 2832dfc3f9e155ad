"""vpz_pcm_fbank at the limits of its launches: ONE case list, used by test_fbank_cpu.py (is every case the shape it is named for?) and by
test_pcm_fbank_limits_gpu.py (does the device compute it?).

A shape case is (spec changes, F): F leaves a remainder and T = 71, 40 or 19 is no multiple of 16.  EXPECT states in numbers written
down here, not computed, what each case is there for in csrc/pcm_fbank.hip: (blocks, left, odd) = (pairs / kFbAhead whole look-ahead
blocks, pairs % kFbAhead k-steps behind them, win & 1 the odd sample), skew (an even hop), the rounds `k0 += 128` gives each of the four
waves, and for the cases at the LDS limit the tile and the floats fbank_truth.tile_plan gives (CROWD_CUS stands for a device's CU count
where no device is; the device test takes the real one)."""
import fbank_truth as ft
import numpy as np
from pcm_support import GUARD, SENTINEL, guarded


WORST = {}


def launch(ctx, d, src, rows, dst_rows, F, d_src=None):
    """one vpz_pcm_fbank call of spec dict d -> [dst_rows][T][n_mels] float32 of the destination's body, the guards checked"""
    import torch
    from vorbispizza_amd import capi
    spec = capi.FbankSpec.make(**d)
    T, n_mels = spec.n_frames(F), d["n_mels"]
    whole, dst = guarded(dst_rows, n_mels * T)
    d_src = torch.from_numpy(src).to("cuda:0") if d_src is None else d_src
    shape = (dst_rows, T, n_mels) if d["frames_first"] else (dst_rows, n_mels, T)
    assert capi.pcm_fbank(ctx, d_src, rows, dst.view(shape), spec, F) == capi.OK, ctx.last_error()
    ctx.synchronize()
    bits = whole.cpu().numpy().view(np.uint32)
    assert (bits[:GUARD] == SENTINEL).all() and (bits[-GUARD:] == SENTINEL).all()
    body = bits[GUARD:-GUARD].view(np.float32)
    return body.reshape(shape) if d["frames_first"] else body.reshape(shape).transpose(0, 2, 1)


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("error / bound %s: %.4f" % (key, ratio))
    assert ratio < 1.0


CROWD_CUS = 256


def crowd_rows(num_cu):
    """rows of a launch that gives every CU two workgroups at one 64-frame tile a row"""
    return max(600, 2 * num_cu + 8)


def _small(win, hop, n_fft, n_mels):
    # (a Hanning or Povey window of two points is two zeros)
    change = dict(win=win, hop=hop, n_fft=n_fft, n_mels=n_mels, sample_rate=8000, low_freq=100.0, window="hamming" if win == 2 else "povey")
    return change, win + hop * 70 + 1


# hops and small windows: name -> ((win, hop, n_fft, n_mels), (blocks, left, odd), skew, rounds of the four waves)
SMALL = {
    "hop2_2_2_32": ((2, 2, 32, 1), (0, 1, 0), 1, (1, 0, 0, 0)),     # hop 2 = win: every k-step wraps in step_a
    "win3_3_2_32": ((3, 2, 32, 2), (0, 1, 1), 1, (1, 0, 0, 0)),     # hop = win - 1; mean lane 3 has no term; blocks == 0, the odd sample
    "win3_3_3_32": ((3, 3, 32, 2), (0, 1, 1), 0, (1, 0, 0, 0)),     # hop 3: not skewed
    "win4_4_2_32": ((4, 2, 32, 3), (0, 2, 0), 1, (1, 0, 0, 0)),     # blocks == 0 without the odd sample; one term to a mean lane
    "win5_5_2_34": ((5, 2, 34, 3), (0, 2, 1), 1, (1, 0, 0, 0)),     # the mean loop wraps twice per term at hop 2
    "hop6_7_6_36": ((7, 6, 36, 4), (0, 3, 1), 1, (1, 0, 0, 0)),     # hop 6 = win - 1
    "win8_8_2_32": ((8, 2, 32, 3), (1, 0, 0), 1, (1, 0, 0, 0)),     # exactly one look-ahead block: it loads itself again
    "win9_9_8_32": ((9, 8, 32, 3), (1, 0, 1), 1, (1, 0, 0, 0)),     # one block and the odd sample; hop = win - 1
    "win33_33_32_64": ((33, 32, 64, 5), (4, 0, 1), 1, (1, 0, 0, 0)),  # whole blocks plus the odd sample, no leftover pair; nb = 32: one full group
    "win33_33_2_64": ((33, 2, 64, 5), (4, 0, 1), 1, (1, 0, 0, 0)),
    "hop62_63_62_64": ((63, 62, 64, 8), (7, 3, 1), 1, (1, 0, 0, 0)),
    "hop64_64_64_64": ((64, 64, 64, 8), (8, 0, 0), 1, (1, 0, 0, 0)),
}
# bin groups: name -> ((win, hop, n_fft, n_mels), rounds of the four waves); win = n_fft - 1 or n_fft
GROUPS = {
    "nb32_63_20_64": ((63, 20, 64, 10), (1, 0, 0, 0)),       # one full group
    "nb33_66_22_66": ((66, 22, 66, 10), (1, 1, 0, 0)),       # a second group of one live column
    "nb64_127_40_128": ((127, 40, 128, 10), (1, 1, 0, 0)),
    "nb65_130_43_130": ((130, 43, 130, 10), (1, 1, 1, 0)),
    "nb128_255_80_256": ((255, 80, 256, 10), (1, 1, 1, 1)),  # each wave exactly once
    "nb129_258_86_258": ((258, 86, 258, 10), (2, 1, 1, 1)),  # a wave's second round, with one live column
}
CROWDED_GROUP = "nb129_258_86_258"  # ... also in 64-frame tiles
# the LDS limits at n_fft 1024: (win, hop) -> (T, tile in a crowded launch, LDS floats of it, tile in a launch of few rows)
LDS_LIMITS = {
    (944, 113): (40, 64, 40960, 32),
    (1024, 111): (40, 64, 40914, 32),
    (1024, 112): (40, 32, 21017, 32),   # 64 frames no longer fit
    (1012, 757): (40, 32, 40960, 32),
    (1024, 755): (40, 32, 40910, 32),
    (1024, 756): (19, 16, 20653, 16),   # 32 frames no longer fit
}
LDS_N_MELS = 23
EMPTY_BANDS = dict(win=32, hop=8, n_fft=32, n_mels=256, sample_rate=16000, low_freq=0.0)
SECOND_ROUND = dict(win=200, hop=80, n_fft=256, n_mels=40, remove_dc=True)  # T = 3; nb = 128: four waves at work
LONG_ROW = (dict(win=2, hop=1, n_fft=32, n_mels=1, window="hamming"), 70001)


def small(name):
    return _small(*SMALL[name][0])


def group(name):
    win, hop, n_fft, n_mels = GROUPS[name][0]
    return dict(win=win, hop=hop, n_fft=n_fft, n_mels=n_mels, sample_rate=8000, low_freq=100.0), win + hop * 70 + 1


def lds_limit(win, hop):
    T = LDS_LIMITS[(win, hop)][0]
    return dict(win=win, hop=hop, n_fft=1024, n_mels=LDS_N_MELS), win + hop * (T - 1) + 1


def chain_of(win, k):
    """(blocks, left, odd) of the k loop"""
    pairs = win // 2
    return pairs // k["kFbAhead"], pairs % k["kFbAhead"], win & 1


def rounds_of(n_fft, k):
    """how often each of the four waves goes through `for (k0 = wave * kFbCols; k0 < nb; k0 += 4 * kFbCols)`"""
    return tuple(len(range(w * k["kFbCols"], n_fft // 2, 4 * k["kFbCols"])) for w in range(4))


def second_round_lengths(n, F, win, rng):
    """lengths of n > kFbMaxGridY rows, of all kinds, with these pairs (i, i + 2048) in one workgroup: real and empty, empty and real,
    real and shorter than win, shorter than win and real, both real with different lengths; with a third round (n > 4096): real,
    shorter than win, real, and empty, real, empty"""
    Ls = rng.integers(0, F + 1, n)
    pairs = [(F, 0), (0, F), (F, win - 1), (win - 1, F), (F, win + 90), (win, F - 1)]
    for i, (a, b) in enumerate(pairs):
        Ls[i], Ls[i + 2048] = a, b
    if n > 4096 + 8:
        for i, (a, b, c) in enumerate([(F, win - 1, F - 3), (0, F, 0), (F, 0, win), (win - 1, win - 1, F)]):
            Ls[i], Ls[i + 2048], Ls[i + 4096] = a, b, c
    return Ls


def tile_of(change, F, n_rows, num_cu, k):
    d = ft.spec_of(**change)
    return ft.tile_plan(d["win"], d["hop"], d["n_fft"], ft.n_frames(F, d["win"], d["hop"]), n_rows, num_cu, k)
