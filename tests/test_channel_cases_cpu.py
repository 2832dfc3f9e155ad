"""The inputs of test_channel_limits_gpu.py, checked with the oracle and a few lines of arithmetic (no GPU): does every case of
channel_cases.CASES hold what it claims?
  C1  the oracle's PCM of the stream the GPU file compares is finite, every channel carries signal, the stream has both block
      sizes and at least one silent record;
  C2  the test has teeth: the same packets decoded with the coupling removed, with the first listed step of every mapping removed,
      with the last one removed (a route that skipped a step), or -- where nothing is coupled -- read as planar (a route that
      skipped the de-interleave) move the oracle's PCM by at least a hundred bars;
  C3  the word each route must print is the one the rules of vpz_decoder_create and SynthPlan::dual_usable / group_usable give,
      restated in channel_cases.expected_route, for both output layouts;
  C4  the arithmetic the limit cases lean on: the padded step-pair totals, the pair route's totals and firsts, the mapping whose
      decoder-wide offset first reaches 256, the runs of the 64-channel grid case."""
import numpy as np
import pytest

import channel_cases as cc

TEETH = 100.0


@pytest.mark.parametrize("case_id", cc.IDS)
def test_every_channel_carries_signal_and_a_record_is_silent(oracle, case_id):
    b, ref = cc.built(case_id)
    c = b.case
    C, per, s = c["channels"], c["frames"], cc.TRUTH_STREAM
    assert ref.shape[0] == C and ref.shape[1] > 0 and np.isfinite(ref).all()
    peak = float(np.abs(ref).max())
    quietest = float(np.abs(ref).max(axis=1).min())
    print("%s: peak %.3g, the quietest channel's peak %.3g" % (case_id, peak, quietest))
    assert peak >= 1e-3 and quietest >= 1e-3 * peak
    flags = b.pk["flags"][s * per:(s + 1) * per]
    assert (flags & 1).any() and not (flags & 1).all(), "both block sizes"
    assert c["n_streams"] >= 2 and c["frames"] >= 4
    counts = b.counts[s * per * C:(s + 1) * per * C]
    assert (counts == 0).any() and (counts > 0).sum() > counts.size // 2
    # every packet lies inside the residue array, `skew` floats off a multiple of four
    off = b.pk["residue_offset"].astype(np.int64)
    size = C * np.where(b.pk["flags"] & 1, 1024, 128)
    assert (off >= 0).all() and (off + size <= b.res.size).all()
    assert (off % 4 == b.skew).all() and b.skew == c["skew"]   # (half a block is a multiple of four bins, whatever the channel count)
    # every mapping a spread case has on the truth stream's block sizes is named by some packet of the batch's top end
    if c["pick"] == "spread":
        used = set(int(m) for m in b.pk["mapping"])
        assert len(c["maps"]) - 1 in used and len(c["maps"]) - 2 in used
        assert all((int(m) & 1) == (int(f) & 1) for m, f in zip(b.pk["mapping"], b.pk["flags"]))


@pytest.mark.parametrize("case_id", [c["id"] for c in cc.CASES if c["skew"] == 0])
def test_a_skipped_step_moves_the_oracle_by_a_hundred_bars(oracle, case_id):
    b, ref = cc.built(case_id)
    c = b.case
    bar = cc.TOL * max(1.0, float(np.abs(ref).max()))
    s = cc.TRUTH_STREAM
    variants = {}
    if any(m["coupling"] for m in c["maps"]):
        variants["no coupling"] = dict(maps=[dict(m, coupling=[]) for m in c["maps"]])
        variants["first step dropped"] = dict(maps=[dict(m, coupling=m["coupling"][1:]) for m in c["maps"]])
        variants["last step dropped"] = dict(maps=[dict(m, coupling=m["coupling"][:-1]) for m in c["maps"]])
    if c["interleaved"]:
        variants["not de-interleaved"] = dict(interleaved=False)
    assert variants
    for name, kw in variants.items():
        moved = b.oracle(oracle, s, **kw)
        assert moved.shape == ref.shape
        ratio = float(np.abs(moved.astype(np.float64) - ref).max()) / bar
        print("%s: %s moves the oracle by %.3g bars" % (case_id, name, ratio))
        assert ratio >= TEETH, (name, ratio)


@pytest.mark.parametrize("case_id", cc.IDS)
def test_the_words_of_the_routes_follow_from_the_rules(case_id):
    c = cc.BY_ID[case_id]
    names = [r[0] for r in c["routes"]]
    assert len(set(names)) == len(names) and len(names) >= 2
    # one of the routes is always the plainest: the separate pass and the one-channel kernel
    assert c["routes"][-1] is cc.PLAIN
    for name, kv, word in c["routes"]:
        for out_interleaved in (False, True):
            assert cc.expected_route(c, kv, out_interleaved) == word, (name, out_interleaved)
    for shift, kv, word in c["device"]:
        for out_interleaved in (False, True):
            assert cc.expected_route(c, kv, out_interleaved, device_shift=shift) == word, (shift, out_interleaved)
    # the kernels behind the word "separate": coupling_tile_kernel up to 32 channels (width 1024 / 512 / 256), coupling_kernel beyond
    assert cc.expected_route(c, cc.PLAIN[1], False) == "separate"


def test_the_ids_are_unique_and_every_count_of_the_issue_is_there():
    assert len(set(cc.IDS)) == len(cc.IDS)
    counts = {c["channels"] for c in cc.CASES}
    assert {7, 9, 31, 32, 33, 64, 254, 255} <= counts
    words = lambda C: {r[2] for c in cc.CASES if c["channels"] == C for r in c["routes"]}
    assert "pairs" in words(32) and "pairs" in words(64) and "pairs" in words(254) and "group" in words(7)
    for C in (7, 33, 64, 255):
        assert any(c["s16"] for c in cc.CASES if c["channels"] == C), C
    # the alignment cases: every skew on the four setups, the unskewed ones with device-memory calls off the boundary
    for skew in (1, 2, 3):
        assert sum(1 for c in cc.CASES if c["skew"] == skew) == 4
    assert sum(len(c["device"]) for c in cc.CASES) >= 4
    # a skew of 2 keeps the planar stereo kernel and the pairs, and drops the Residue2 stereo kernel and group mode
    first = lambda i: cc.BY_ID[i]["routes"][0][2]
    assert (first("align2-stereo-planar"), first("align2-pairs-c6")) == ("stereo", "pairs")
    assert (first("align2-stereo-residue2"), first("align2-group-c6")) == ("separate", "separate")
    for skew in (1, 3):
        assert {first("align%d-%s" % (skew, n)) for n in ("stereo-planar", "stereo-residue2", "group-c6", "pairs-c6")} == {"separate"}


def test_the_step_tables_sit_on_their_limits_and_one_past():
    table = lambda i: cc.step_table(cc.BY_ID[i]["maps"])
    # one mapping of 128 / 129 steps
    assert table("lim-stereo-128-steps")[1:] == (128, 128) and table("lim-stereo-129-steps")[1:] == (129, 129)
    # 32 / 33 padded lists: the 32nd ends at pair 128, the 33rd starts there
    for kind in ("stereo", "group"):
        first, size, most = table("lim-%s-32-mappings" % kind)
        assert first == [4 * m for m in range(32)] and size == cc.MAX_STEP_PAIRS and most == 4
        assert {len(m["coupling"]) for m in cc.BY_ID["lim-%s-32-mappings" % kind]["maps"]} == {2, 3, 4}
        first, size, most = table("lim-%s-33-mappings" % kind)
        assert first[32] == cc.MAX_STEP_PAIRS and size > cc.MAX_STEP_PAIRS
    for i in ("lim-stereo-128-steps", "lim-stereo-32-mappings", "lim-group-32-mappings"):
        assert cc.wide_steps_fit(cc.BY_ID[i]["maps"]), i
    for i in ("lim-stereo-129-steps", "lim-stereo-33-mappings", "lim-group-33-mappings", "lim-256-steps", "lim-256-steps-stereo",
              "lim-pairs-65-mappings", "lim-pairs-255-mappings", "lim-256-mappings", "c254-chain"):
        assert not cc.wide_steps_fit(cc.BY_ID[i]["maps"]), i
    # the steps of the group cases are no pairs
    assert cc.pair_table(6, cc.BY_ID["lim-group-32-mappings"]["maps"]) is None
    # VPZ_MAX_COUPLING steps in one mapping: one more than the 8 bits of a frame's count
    assert table("lim-256-steps")[2] == 256 and table("lim-256-steps-stereo")[2] == 256
    # 253 dependent steps keep 254 channels off the pair route
    c = cc.BY_ID["c254-chain"]
    assert len(c["maps"][0]["coupling"]) == 253 and cc.pair_table(254, c["maps"]) is None


def test_the_pair_tables_sit_on_their_limits_and_one_past():
    c = cc.BY_ID["lim-pairs-254-128-steps"]
    pairs, firsts, total = cc.pair_table(254, c["maps"])
    assert len(pairs) == 127 and total == cc.MAX_STEP_PAIRS and max(firsts) <= 255
    assert [len(m["coupling"]) for m in c["maps"]] == [64, 64]
    coupled = {tuple(sorted(p)) for m in c["maps"] for p in m["coupling"]}
    assert {(1, 200), (130, 131), (3, 4)} <= coupled                       # distant, beyond channel 127, adjacent-odd
    assert any(a >= 128 and b >= 128 for a, b in pairs if tuple(sorted((a, b))) not in coupled)   # lone channels beyond 127 too
    assert any(mag > ang for m in c["maps"] for mag, ang in m["coupling"])  # the angle in front of the magnitude
    c = cc.BY_ID["lim-pairs-254-129-steps"]
    assert [len(m["coupling"]) for m in c["maps"]] == [64, 65] and cc.pair_table(254, c["maps"]) is None
    # 65 mappings of one step: 65 steps in the pairs' table; the decoder-wide offset reaches 256 at mapping 64, and packets name it
    c = cc.BY_ID["lim-pairs-65-mappings"]
    pairs, firsts, total = cc.pair_table(4, c["maps"])
    assert pairs == [(0, 1), (2, 3)] and total == 65 and all(len(m["coupling"]) == 1 for m in c["maps"])
    first = cc.step_table(c["maps"])[0]
    assert [m for m, f in enumerate(first) if f >= cc.OFFSET_FIELD] == [64] and first[64] == 256
    b, _ = cc.built("lim-pairs-65-mappings")
    per = c["frames"]
    truth = b.pk["mapping"][cc.TRUTH_STREAM * per:(cc.TRUTH_STREAM + 1) * per]
    assert (truth == 64).sum() >= 2 and (b.pk["mapping"] == 64).sum() >= 4
    # 255 mappings, 128 of them coupled: the pairs' table full, offsets up to 508, packets at mappings 253 and 254
    c = cc.BY_ID["lim-pairs-255-mappings"]
    pairs, firsts, total = cc.pair_table(4, c["maps"])
    assert total == cc.MAX_STEP_PAIRS and len(c["maps"]) == 255
    first = cc.step_table(c["maps"])[0]
    assert min(m for m, f in enumerate(first) if f is not None and f >= cc.OFFSET_FIELD) == 127 + 64 and first[254] == 508
    b, _ = cc.built("lim-pairs-255-mappings")
    truth = b.pk["mapping"][cc.TRUTH_STREAM * per:(cc.TRUTH_STREAM + 1) * per]
    assert (truth == 254).any() and (truth == 253).any()
    # 256 mappings: one more than the pair route takes
    c = cc.BY_ID["lim-256-mappings"]
    assert len(c["maps"]) == 256 and cc.pair_table(4, c["maps"]) is None and cc.pair_table(4, c["maps"][:255]) is None
    b, _ = cc.built("lim-256-mappings")
    assert (b.pk["mapping"] == 255).any()


def test_the_grid_case_cuts_more_than_32_runs_in_every_call():
    """synth_pairs_kernel's grid: groups of 8 chunks x n_pairs workgroups, four runs to a chunk -- the second group starts with
    run 33.  A run never crosses a stream, so a call with packets of 34 streams cuts at least 34."""
    c = cc.BY_ID["c64-pairs-grid"]
    assert c["channels"] // 2 == 32 and c["min_runs"] == 32
    b, _ = cc.built("c64-pairs-grid")
    per = c["frames"]
    for a, e in ((0, per // 2), (per // 2, per)):    # the two calls of run(..., splits=2)
        streams = {int(s) for i, s in enumerate(b.pk["stream"]) if a <= i % per < e}
        assert len(streams) == c["n_streams"] > c["min_runs"]
    assert c["routes"][0][1]["VPZ_DUAL_RUN"] == 4


def test_the_per_channel_floors_differ_inside_a_pair():
    for n, count in (("4", 4), ("5", 5)):
        for kind in ("stereo", "c6", "c33"):
            c = cc.BY_ID["floors%s-%s" % (n, kind)]
            assert len(c["floors"]) == count
            used = {f for m in c["maps"] for f in m["channel_floor"]}
            assert used == set(range(count)) or (kind == "stereo" and used == set(range(4)))
            for m in c["maps"]:
                a, b_ = c["floors"][m["channel_floor"][0]], c["floors"][m["channel_floor"][1]]
                assert len(a[0]) != len(b_[0]) and a[1] != b_[1]      # other post counts, other multipliers
