"""The case list of the normalisation tests: the smallest shapes at which vpz_pcm_normalize's kernels can go wrong.  A case is one call:
the SAME window laid out three times -- at an aligned offset, one element further, two further -- and delivered to rows 3, 0 and 4 of a
destination of five, so that every case also asks that a row's bits do not depend on where it lies; rows 1 and 2 keep a sentinel."""
import collections

import normalize_truth as nt

Case = collections.namedtuple("Case", "name kind C J frames mode target eps ceiling gain planar s16 seed")

J_VALUES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17)  # around a wave, around a chunk, several chunks and a tail
CHANNELS = (1, 2, 3, 8)
# mode, target (gain: the rows' one gain) and ceiling: every mode without one, and PEAK / RMS / GAIN with one that is taken on noise of
# amplitude 1 (0.15) and one that is not (0.6)
LEVELS = [("meanvar", 0.0, 0.0)] + [(m, t, c) for m, t in (("peak", 0.5), ("rms", 0.1), ("gain", 0.4)) for c in (0.0, 0.15, 0.6)]
LAYOUTS = [(True, False), (False, False), (True, True), (False, True)]  # (planar, int16)
ROWS, DST_ROWS, GAPS = (3, 0, 4), 5, (0, 1, 2)
SENTINEL_F32, SENTINEL_S16 = 777.0, 12345


def _case(name, kind, C, J, frames, level, layout, seed):
    mode, target, ceiling = level
    return Case(name, kind, C, J, frames, mode, target, 1e-7, ceiling, target if mode == "gain" else 1.0, layout[0], layout[1], seed)


def shape_cases():
    """every J x channels x (frames == J, frames == J + 5), the 40 combinations of level and layout dealt round"""
    out, i = [], 0
    for C in CHANNELS:
        for J in J_VALUES:
            for frames in (max(J, 1), J + 5):
                k = (7 * i) % (len(LEVELS) * len(LAYOUTS))  # (7 and 40 share no factor: 72 shapes meet every combination)
                level, layout = LEVELS[k % len(LEVELS)], LAYOUTS[k // len(LEVELS)]
                out.append(_case("C%d-J%d-F%d-%s-c%g-%s%s" % (C, J, frames, level[0], level[2], "planar" if layout[0] else "inter",
                                                             "-s16" if layout[1] else ""), "noise", C, J, frames, level, layout, 1000 + i))
                i += 1
    return out


def special_cases():
    """the rows the definition singles out, in every mode: silence (g = 1), a constant, one sample of 1e4 among 1e-4, the cancellation case"""
    out, i = [], 0
    for kind in ("zero", "constant", "outlier", "dc"):
        for level in (LEVELS[0], LEVELS[1], LEVELS[5], LEVELS[8]):  # meanvar; peak; rms with the low ceiling; gain
            layout = LAYOUTS[i % len(LAYOUTS)]
            out.append(_case("%s-%s-c%g-%s%s" % (kind, level[0], level[2], "planar" if layout[0] else "inter", "-s16" if layout[1] else ""),
                             kind, 2, 3 * 1024 + 17, 3 * 1024 + 22, level, layout, 2000 + i))
            i += 1
    return out


def level_layout_cases():
    """all 40 combinations of level and layout at one shape with an odd channel count and a tail"""
    return [_case("all-%s-c%g-%s%s" % (level[0], level[2], "planar" if layout[0] else "inter", "-s16" if layout[1] else ""), "noise", 3, 1025,
                  1030, level, layout, 3000 + i) for i, (level, layout) in enumerate((lv, ly) for lv in LEVELS for ly in LAYOUTS)]


def all_cases():
    return shape_cases() + special_cases() + level_layout_cases()


def window_of(case):
    return nt.signal(case.kind, case.C, case.J, case.seed)


def spec_args(case):
    """the keyword arguments of nt.model / nt.truth for a case's three descriptors"""
    return dict(mode=nt.MODES[case.mode], target=case.target, eps=case.eps, ceiling=case.ceiling,
                gains=[case.gain] * len(ROWS) if case.mode == "gain" else None)


def plain(case):
    """VPZ_NORM_GAIN without a ceiling: the call that needs no statistics (unless the result array is asked for)"""
    return case.mode == "gain" and case.ceiling == 0.0
