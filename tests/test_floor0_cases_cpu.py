"""The inputs of test_floor0_limits_gpu.py, checked with the oracle alone (no GPU): are they fit to test with?  For every case
of floor0_cases.CASES -- the list the GPU file runs --
  C1  the oracle's PCM is finite and its peak lies in [1, 100] (the bar 1e-5 * max(1, peak) is relative to the signal);
  C2  the test has teeth: a mutation of the INPUTS that amounts to what a wrong index in the kernels would read -- (a) the late
      coefficients j >= 64 replaced by j - 64, (b) the last coefficient by the one before it, (c) the other type-0 floor's
      configuration, (d) record r with the data of record r - 8192 -- moves the oracle's PCM by at least 100 bars;
  C3  every 256-wide round of bark indices the case's floors have is hit by some bin, at every block size the floor is used at.
The worst ratios are recorded in DESIGN.md (the Floor0 limits)."""
import numpy as np
import pytest

import floor0_cases as fc


@pytest.mark.parametrize("case_id", fc.IDS)
def test_oracle_pcm_is_finite_and_of_signal_size(oracle, case_id):
    b, ref = fc.built(case_id)
    assert ref.shape[0] == b.case["channels"] and ref.shape[1] > 0
    assert np.isfinite(ref).all()
    peak = float(np.abs(ref).max())
    print("%s: peak %.3f, scale %g, amp %.3g ... %.3g" % (case_id, peak, b.scale, b.amps[b.amps > 0].min(), b.amps.max()))
    assert 1.0 <= peak <= 100.0
    # every type-0 channel carries signal of that size, not only the loudest one
    for ch in range(b.case["channels"]):
        if any(isinstance(b.floors[cf[ch]], dict) for cf in b.case["maps"]):
            assert float(np.abs(ref[ch]).max()) >= 1e-2 * peak, ch


@pytest.mark.parametrize("case_id", fc.IDS)
def test_mutated_inputs_move_the_oracle_by_a_hundred_bars(oracle, case_id):
    b, ref = fc.built(case_id)
    muts = b.mutations()
    c = b.case
    assert ("a" in muts) == any(f["order"] > 64 for f in c["floors"] if isinstance(f, dict))
    assert ("c" in muts) == (sum(isinstance(f, dict) for f in c["floors"]) == 2)
    assert ("d" in muts) == (c["group"] == "D")
    bar = fc.TOL * max(1.0, float(np.abs(ref).max()))
    for name, kw in sorted(muts.items()):
        whole = kw["first"] == 0 and kw["last"] == b.n
        base = ref if whole else b.oracle(oracle, first=kw["first"], last=kw["last"])
        moved = b.oracle(oracle, **kw)
        assert moved.shape == base.shape
        # (two equal LSP frequencies put the curve far above 0 dB: a PCM that overflows has moved)
        ratio = float(np.abs(moved.astype(np.float64) - base).max()) / bar if np.isfinite(moved).all() else np.inf
        print("%s: mutation (%s) moves the oracle by %.3g bars" % (case_id, name, ratio))
        assert ratio >= fc.TEETH, (name, ratio)


@pytest.mark.parametrize("case_id", fc.IDS)
def test_every_round_of_bark_indices_is_hit(oracle, case_id):
    b, _ = fc.built(case_id)
    c = b.case
    two_sizes = c["size0"] != c["size1"]
    seen = 0
    for m, channel_floor in enumerate(c["maps"]):
        is_long = m if two_sizes else 0
        assert (b.mapping == m).any(), "the case has no packet of mapping %d" % m
        for fi in channel_floor:
            fl = c["floors"][fi]
            if not isinstance(fl, dict):
                continue
            n = b.half[is_long]
            assert fl["bark_map_size"] <= n, "the oracle refuses a bark map larger than half a block"
            bark = oracle.floor0_bark_map(fl["order"], fl["rate"], fl["bark_map_size"], n)[:n]
            assert bark.min() >= 0 and bark.max() < fl["bark_map_size"]
            rounds = (fl["bark_map_size"] + 255) // 256
            assert set(np.unique(bark // 256)) == set(range(rounds)), (fi, n)
            assert bark[n - 1] == 0 and bark[n - 2] == bark.max()  # (Floor0.cs:82-95: the last bin keeps index 0)
            seen += 1
    assert seen > 0


def test_groups_a_b_d_are_the_fast_paths_and_group_c_is_not():
    """synth_dual_supported (stereo, 256 / 2048 blocks) and kFloor0MaxBark put groups A, B and D on the stereo fast path and no
    case of group C; a coefficient row holds the largest order (vpz_decoder_set_floor0_data refuses less)."""
    assert len(set(fc.IDS)) == len(fc.IDS)
    for c in fc.CASES:
        assert fc.fast_path(c) == (c["group"] != "C"), c["id"]
        assert c["stride"] >= max(f["order"] for f in c["floors"] if isinstance(f, dict)), c["id"]


def test_the_large_batch_makes_wavefronts_take_a_second_record(oracle):
    """Case D: more records than floor0_curve_kernel's grid has wavefronts, and among the pairs (r, r + 8192) one wavefront gets:
    a type-1 record in front of a type-0 one, both floor changes, a silent record first and a silent record second."""
    b, _ = fc.built("D-8400-records")
    n1 = int(b.bounds[1]) * 2
    assert n1 > fc.GRID_WAVES
    is0 = np.array([isinstance(b.floors[f], dict) for f in b.rec_floor[:n1]])
    r = np.arange(n1 - fc.GRID_WAVES)
    first, second = r, r + fc.GRID_WAVES
    live = is0 & (b.amps[:n1] > 0)
    assert (~is0[first] & live[second]).any()
    for fa, fb in ((0, 1), (1, 0)):
        assert (live[first] & live[second] & (b.rec_floor[first] == fa) & (b.rec_floor[second] == fb)).any()
    assert (is0[first] & ~live[first] & live[second]).any() and (live[first] & is0[second] & ~live[second]).any()
