"""vpz_decoder_synth at the limits of channel count and coupling tables (the cases: channel_cases.CASES; test_channel_cases_cpu.py
shows with the oracle alone that each would notice a skipped step and that its routes follow from the rules):
  counts   7 (group mode; tile width 512), 9 (tile width 256), 31 / 32 (coupling_tile_kernel's last counts, 32 on the pair route
           too), 33 (coupling_kernel's first), 64 (32 pairs, more than 32 runs in a call; coupling_kernel), 254 (the pair route's
           last count; a chain of 253 dependent steps), 255 (the ABI's maximum);
  limits   the staged step table full and one pair too long (one mapping of 128 / 129 steps, 32 / 33 padded lists, stereo and group
           mode), the pairs' own table (254 channels, 128 / 129 pair-steps), 65 / 255 / 256 mappings of four channels -- decoder-wide
           offsets beyond the 8 bits of a frame's offset field --, 256 steps in one mapping;
  floors   a floor per channel: four floors (floor1_unwrap_kernel's LDS copy full) and five (its memory instantiation), other post
           counts and multipliers side by side in a pair;
  align    packets 1, 2, 3 floats off a multiple of four; device-memory calls whose residue pointer is.
Every case, on every route it lists: the word VPZ_HOST_PROFILE=1 prints is the one the case names; planar and interleaved float32
PCM (and both int16 layouts where the case says so) are the same bits on all its routes -- one of them always the separate
coupling pass with the one-channel kernel --, samples written, per-packet samples and positions too; the int16 PCM is to_s16 of the
float32 PCM; nothing is written outside a stream's span (the array is filled with a sentinel first); and the second stream meets
the oracle at the bar of test_pairs_gpu.py, 1e-5 * max(1, |ref|max).  Two calls per stream: every channel's state crosses a call."""
import re

import numpy as np
import pytest

import channel_cases as cc
from synth_support import env, run, same_bits, to_s16
from gpu_context import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 12345


def decode(ctx, b, kv, layout, capfd, device_shift=None):
    """The case's batch in two calls under the route's environment.  Returns run()'s tuple, the route words the calls printed and
    the runs each cut."""
    c = b.case
    capfd.readouterr()
    with env(**dict(kv, VPZ_HOST_PROFILE=1)):
        got = run(ctx, b.pk, b.res, b.posts, b.counts, c["n_streams"], c["channels"], c["floors"], c["maps"], layout=layout,
                  splits=2, fill=SENTINEL, device_shift=device_shift)
    err = capfd.readouterr().err
    words = re.findall(r"\[vpz host\] packets \d+: route (\w+)", err)
    runs = [int(n) for n in re.findall(r"\[vpz host\] cut: [^\n]*? (\d+) runs for ", err)]
    return got, words, runs


def written_mask(c, total, layout):
    """True where the calls may have written: `total[s]` samples of every channel of stream s, in the layout's places."""
    from vorbispizza_amd import capi
    C, cap = c["channels"], c["frames"] * 1024 + 64
    mask = np.zeros((c["n_streams"], C * cap), dtype=bool)
    for s in range(c["n_streams"]):
        if layout in (capi.OUT_PLANAR, capi.OUT_PLANAR_S16):
            mask[s].reshape(C, cap)[:, :int(total[s])] = True
        else:
            mask[s, :int(total[s]) * C] = True
    return mask.reshape(-1)


@pytest.mark.parametrize("case_id", cc.IDS)
def test_channel_limits(ctx, oracle, capfd, case_id):
    from vorbispizza_amd import capi
    b, ref = cc.built(case_id)
    c = b.case
    C, cap = c["channels"], c["frames"] * 1024 + 64
    layouts = [capi.OUT_PLANAR, capi.OUT_INTERLEAVED] + ([capi.OUT_INTERLEAVED_S16, capi.OUT_PLANAR_S16] if c["s16"] else [])
    first = c["routes"][0][0]
    outs, report = {}, []
    for layout in layouts:
        for name, kv, word in c["routes"]:
            got, words, runs = decode(ctx, b, kv, layout, capfd)
            outs[(name, layout)] = got
            report.append((name, layout, words, word, runs))
    for shift, kv, word in c["device"]:
        for layout in layouts[:2]:
            got, words, runs = decode(ctx, b, kv, layout, capfd, device_shift=shift)
            outs[("device+%d" % shift, layout)] = got
            report.append(("device+%d" % shift, layout, words, word, runs))
    twin = cc.built(case_id, 0)[0] if c["skew"] else None   # the same packets on a multiple of four floats, the plainest route
    if twin is not None:
        assert np.array_equal(twin.res, b.res[c["skew"]:]) and np.array_equal(twin.pk["residue_offset"] + c["skew"], b.pk["residue_offset"])
        for layout in layouts:
            outs[("unskewed", layout)] = decode(ctx, twin, cc.PLAIN[1], layout, capfd)[0]
    # (after the runs: capfd takes what is printed before a run with the run's own lines)
    # ---- route
    for name, layout, words, word, runs in report:
        print("%s %s layout %d: route %s, runs %r" % (case_id, name, layout, words, runs))
        assert words == [word] * 2, (name, layout, words, word)
        if name == first and c["min_runs"]:
            assert len(runs) == 2 and min(runs) > c["min_runs"], (name, runs)
    # ---- bits, and nothing beyond
    for (name, layout), got in outs.items():
        same_bits(got, outs[(first, layout)], "%s: %s vs %s, layout %d" % (case_id, name, first, layout))
        mask = written_mask(c, got[1], layout)
        assert (got[0][~mask] == SENTINEL).all(), (name, layout, "written outside a stream's span")
        assert (got[1] > 0).all() and got[2].sum() == got[1].sum()
        if got[0].dtype == np.float32:
            assert np.isfinite(got[0]).all() and not (got[0][mask] == SENTINEL).any(), (name, layout)
    # ---- the 16-bit samples are the reference conversion of the float ones
    for s16, f32 in ((capi.OUT_INTERLEAVED_S16, capi.OUT_INTERLEAVED), (capi.OUT_PLANAR_S16, capi.OUT_PLANAR)):
        if s16 in layouts:
            mask = written_mask(c, outs[(first, f32)][1], f32)
            assert np.array_equal(outs[(first, s16)][0][mask], to_s16(outs[(first, f32)][0][mask])), s16
    # ---- truth
    s = cc.TRUTH_STREAM
    got = outs[(first, capi.OUT_PLANAR)]
    assert got[1][s] == ref.shape[1] and ref.shape[1] > 0
    pcm = got[0][s * C * cap:(s + 1) * C * cap].reshape(C, cap)[:, :ref.shape[1]]
    peak = float(np.abs(ref).max())
    err = float(np.abs(pcm.astype(np.float64) - ref).max())
    print("%s: |got - ref|max = %.3g, |ref|max = %.3g (the bar: %g * max(1, |ref|max))" % (case_id, err, peak, cc.TOL))
    assert err <= cc.TOL * max(1.0, peak), (err, peak)
    # ... and the interleaved layout, at the same bar
    ilv = outs[(first, capi.OUT_INTERLEAVED)][0][s * C * cap: s * C * cap + ref.size].reshape(ref.shape[1], C).T
    assert float(np.abs(ilv.astype(np.float64) - ref).max()) <= cc.TOL * max(1.0, peak)
