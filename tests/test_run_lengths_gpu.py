"""The synth kernels at the run lengths large batches give them.  A wavefront synthesises a RUN of R consecutive blocks of one
channel (synth_plan.hip choose_run_length: R = ceil(channel-blocks / (k * resident slots)), at least 4), and an MI355X has several
thousand resident slots: every batch of a few hundred channel-blocks is cut at R = 4.  VPZ_PLAN_SLOTS=n (tests) replaces the slot
count, so the batches here -- tens of frames -- are cut into runs of 5, a middle value, r_max - 1 and r_max frames, r_max being
the kernels' descriptor areas:

    synth_big_kernel                          kMaxRunLengthBig = 32      csrc/synth_desc.hpp:51
    synth_kernel, general variant             kMaxRunLengthGeneral = 16  csrc/synth_desc.hpp:50
    synth_kernel, standard sizes, group mode  kMaxRunLength = 32         csrc/synth_desc.hpp:49
    stereo kernel and pair route              kMaxRunLengthDual = 63     csrc/synth_desc.hpp:52

Every case decodes the same packets (a) with the knob, (b) without it (R = 4) and (c) through the oracle: the cut line of
VPZ_HOST_PROFILE=1 must report the intended R, rule, route and run count; (a) and (b) agree bit for bit (a block's samples do not
depend on where the runs are cut); (a) meets the oracle at the bar of the route's existing oracle test; positions and clip flags
are the oracle's.  Streams of r_max, r_max + 1 and 2 R + 1 frames (a run that starts its stream with r_max staged frames, one that
recomputes its predecessor with r_max + 1, a one-frame last run) share a call, and therefore workgroups; a second call on the same
decoder continues every stream from the state a run of the first call saved, and one stream ends in an EOS-trimmed packet.

How the two calls are made is a reading of "split one batch inside a run-length multiple and off it": the knob is read once per
decoder and R follows from a call's work, so both calls must hold the same work to be cut at the same R -- the second call gives
every stream another of the first call's sequences (stream 0 goes on after r_max frames, a multiple of R at R = r_max, stream 1
after r_max + 1, off it), which makes the batch twice as long as one split would.  The 8192 cases at R = 32 therefore hold more
than the 2 M samples a case should; the oracle takes 0.3 s for the largest.

For cuts by COST the R of a case's id is what the cut line reports, not the frames per run: the target starts at 8 R eighths of a
pass and fit_target raises it by up to 24 (while target / 8 < r_max) when the runs do not fit slots / channels -- with these slot
counts they never do -- so "R5" is cut at 64 eighths and the stereo "R62" at 504 like "R63"; a run holds as many frames as that
cost buys, up to r_max.  The restated rule (helpers.by_cost_runs) takes the target and the skew threshold from the cut line: it
checks the walk and the run count, not how the target was chosen.  What ran at r_max and r_max + 1 staged frames is what the
closing test counts.
StreamDecoder.cs:640-694, 764-791; Mapping.cs:166-195."""
import re

import numpy as np
import pytest

import helpers
from helpers import PKT_BLOCK_FLAG, PKT_EOS, PKT_INTERLEAVED, PKT_NEXT_FLAG, PKT_NO_FLOOR, PKT_PREV_FLAG
from synth_support import env, random_xlist
from gpu_context import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-5        # tests/test_synth_gpu.py: TOL * max(1, |ref|max), the bar of every oracle test of these routes
TOL_CURVE = 2e-6  # tests/test_synth_gpu.py test_floor_curve_is_bit_exact, relative to max(1, |ref|max)

R_MAX = {"big": 32, "general": 16, "standard": 32, "dual": 63}  # csrc/synth_desc.hpp:51, :50, :49, :52
R_LIST = {k: (5, v // 2, v - 1, v) for k, v in R_MAX.items()}
ALL_LONG = PKT_BLOCK_FLAG | PKT_PREV_FLAG | PKT_NEXT_FLAG
PARALLEL = dict(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4)  # the parallel host pass: compact run descriptors, cuts by cost
# every switch a case may set, cleared where it does not: a case's route is its own
SWITCHES = ("VPZ_NO_BIG", "VPZ_NO_DUAL", "VPZ_NO_GROUP", "VPZ_NO_PAIRS", "VPZ_PAIRS", "VPZ_NO_COMPACT", "VPZ_PAR_MIN_PACKETS",
            "VPZ_HOST_THREADS", "VPZ_DUAL_RUN", "VPZ_NO_CHAIN", "VPZ_PLAN_SLOTS")

# what the cases' cut lines reported: (group of cases, R) and (group, R, staged frames of a run); the last test reads it (it
# needs the whole file to have run in its process: not under -k, --lf or a split over workers)
REACHED = set()


def case(ident, kernel, R, channels, size0, size1, kind, **kw):
    c = dict(id=ident, kernel=kernel, R=R, channels=channels, size0=size0, size1=size1, kind=kind, in_layout="planar", out="planar",
             i16=False, clip=False, kv={}, by="length", route="separate", all_long=False, lens=None, stretch=False, control=False)
    c.update(kw)
    return pytest.param(c, id=ident)


# ---- the batch of a case ------------------------------------------------------------------------------------------------------

def _flags(c, n, seed):
    if c["size0"] == c["size1"]:
        return np.zeros(n, dtype=np.uint8)  # one block size: every block is a "short" one (block flag 0)
    if c["all_long"]:
        return np.full(n, ALL_LONG, dtype=np.uint8)
    # (the last two blocks long: the EOS trim compares the granule with the position plus the previous block's TAIL,
    # StreamDecoder.cs:654-666, which is what the last packet emits only after a long block)
    head = helpers.markov_block_flags(n - 2, seed=seed, p_ls=0.15, p_sl=0.3)
    after_long = PKT_PREV_FLAG if head[-1] & PKT_BLOCK_FLAG else 0
    return np.concatenate([head, [PKT_BLOCK_FLAG | after_long | PKT_NEXT_FLAG, ALL_LONG]]).astype(np.uint8)


def _stretch_flags(n):
    """a stream with 45 short blocks in a row: at a target of 32 passes the frame cap ends their run, not the cost"""
    bf = np.ones(n, dtype=np.uint8)
    bf[6:51] = 0
    prev = np.concatenate([[1], bf[:-1]])
    nxt = np.concatenate([bf[1:], [1]])
    return (bf * PKT_BLOCK_FLAG | prev * PKT_PREV_FLAG * bf | nxt * PKT_NEXT_FLAG * bf).astype(np.uint8)


def _setup(c):
    """floors and mappings of a case (mapping 0: short blocks, mapping 1: long blocks)"""
    C_, h0, h1 = c["channels"], c["size0"] // 2, c["size1"] // 2
    if c["kind"] == "nofloor":
        return (), ()
    if c["kind"] == "curve":
        return [(helpers.LONG_XLIST, 2)], [{"coupling": [], "channel_floor": [0]}]
    rng = np.random.default_rng(c["size0"] * 11 + c["size1"])
    if (c["size0"], c["size1"]) == (256, 2048):
        f1 = [(helpers.SHORT_XLIST, 2), (helpers.LONG_XLIST, 2)]
    else:
        f1 = [(random_xlist(rng, h0, min(19, h0 // 2)), 2), (random_xlist(rng, h1, min(61, h1 // 2)), 1)]
    steps = {1: ([], []), 2: ([(0, 1)], [(1, 0)]), 3: ([(0, 1)], [(1, 0), (2, 1)]), 6: ([(0, 1), (2, 3)], [(0, 1), (2, 3)]),
             8: ([(7, 0), (1, 6), (0, 1)], [(7, 0), (1, 6), (0, 1)]), 10: ([(0, 1), (9, 2)], [(2, 9), (5, 4)])}[C_]
    if c["kind"] == "floor0":  # channel 0 has a type-0 floor, the others the block size's type-1 floor
        f0 = {"order": 9, "rate": 44100, "bark_map_size": 64, "amp_bits": 6, "amp_ofs": 100}
        return [f0] + f1, [{"coupling": steps[0], "channel_floor": [0] + [1] * (C_ - 1)},
                           {"coupling": steps[1], "channel_floor": [0] + [2] * (C_ - 1)}]
    return f1, [{"coupling": steps[0], "channel_floor": [0] * C_}, {"coupling": steps[1], "channel_floor": [1] * C_}]


def _packets(c, floors, flags, seed):
    """One stream's packets of one call, as the oracle takes them (helpers.OracleStream)."""
    rng = np.random.default_rng(seed)
    C_ = c["channels"]
    out = []
    for f, fl in enumerate(flags):
        bf = int(fl) & 1
        half = (c["size1"] if bf else c["size0"]) // 2
        if c["kind"] == "curve":  # test_floor_curve_is_bit_exact: a flat residue, the floor curve alone shapes the spectrum
            posts, counts = helpers.random_posts(rng, helpers.LONG_XLIST, 2, 1)
            out.append({"flags": int(fl), "mapping": 0, "granule": -1, "residue": np.full(half, 2.0 ** -10, dtype=np.float32),
                        "posts": posts, "post_count": counts})
            continue
        no_floor = c["kind"] == "nofloor" or (c["kind"] == "mixed" and f % 5 == 4)
        ilv = c["in_layout"] == "interleaved" or (c["in_layout"] == "alternate" and f % 2 == 1 and not no_floor)
        # small integers (exact under the floor multiply in float32); already floored spectra are scaled down to PCM size
        res = (rng.standard_normal((C_, half)) * 3).round().astype(np.float32)
        res[:, int(half * 0.85):] = 0
        if no_floor:
            res = (res * 2.0 ** -8).astype(np.float32)
        pk = {"flags": int(fl) | (PKT_INTERLEAVED if ilv else 0) | (PKT_NO_FLOOR if no_floor else 0), "mapping": bf, "granule": -1,
              "residue": (res.T.reshape(-1) if ilv else res.reshape(-1)).copy()}
        if c["kind"] != "nofloor":
            xl, mult = floors[-2 + bf]
            posts, counts = helpers.random_posts(rng, xl, mult, C_, silent_prob=0.1)
            if f == 3:
                counts[C_ - 1] = 0  # a silent channel (ExecuteChannel false, Mapping.cs:185)
            pk["posts"], pk["post_count"] = posts, counts
        if c["kind"] == "floor0":
            f0 = floors[0]
            coeff = np.zeros((C_, 32), dtype=np.float32)
            coeff[0, :f0["order"]] = np.sort(rng.uniform(0.05, 3.0, f0["order"]))
            amp = np.zeros(C_, dtype=np.float32)
            if f != 5:  # (frame 5: the type-0 channel is silent)
                amp[0] = helpers.floor0_safe_amp(coeff[0, :f0["order"]], f0["bark_map_size"], 100.0) * rng.uniform(0.3, 1.0)
            pk["post_count"][0] = 1 if amp[0] != 0 else 0
            pk["f0_amp"], pk["f0_coeff"] = amp, coeff
        out.append(pk)
    return out


def _slots_for(work, R):
    """the slot count for which ceil(work / slots) == R (then one round of runs of R is the cheapest cut: k (R_k + 1) > R + 1)"""
    for n in range(1, work + 1):
        if -(-work // n) == R:
            return n
    return None


def _work(c, seqs):
    if c["by"] == "length":
        return sum(len(s) for s in seqs) * c["channels"]
    dual = c["route"] in ("stereo", "pairs")
    units = sum(helpers.cost_codes([(int(f) | _layout_bits(c), int(f) & 1) for f in s], dual)[1] for s in seqs)
    return (units + 7) // 8 * c["channels"]


def _layout_bits(c):
    return (PKT_INTERLEAVED if c["in_layout"] == "interleaved" else 0) | (PKT_NO_FLOOR if c["kind"] == "nofloor" else 0)


def _batch(c, oracle):
    """The case's streams: flag sequences of r_max, r_max + 1 and 2 R + 1 frames (and, where no slot count gives R for that
    much work, a short fourth one); call k gives stream s the sequence (s + k) mod n -- both calls hold the same work, so one slot
    count cuts both at R -- with data of its own.  Stream 1 ends, in the second call, with the 2 R + 1 sequence: its last run is
    one frame, and an EOS granule trims that frame by 37 samples.  Returns (calls: [per stream: packets], slots, oracle results)."""
    r_max, R = R_MAX[c["kernel"]], c["R"]
    base = list(c["lens"] or (r_max, r_max + 1, 2 * R + 1))
    for extra in [0] + list(range(3, 3 * R)):
        lens = base + ([extra] if extra else [])
        seqs = [_flags(c, n, seed=1000 * R + 10 * len(c["id"]) + i) for i, n in enumerate(lens)]
        if c["stretch"]:
            seqs[2] = _stretch_flags(lens[2])
        slots = _slots_for(_work(c, seqs), R)
        if slots is not None:
            break
    assert slots is not None, "no slot count cuts this batch at R = %d" % R
    floors, mappings = _setup(c)
    n = len(seqs)
    calls = [[_packets(c, floors, seqs[(s + k) % n], seed=7919 * R + 100 * k + s) for s in range(n)] for k in range(2)]
    kw = dict(floors=floors, mappings=mappings, clip=c["clip"])
    natural = helpers.oracle_decode(oracle, c["channels"], c["size0"], c["size1"], calls[0][1] + calls[1][1], **kw)[0].shape[1]
    calls[1][1][-1]["flags"] |= PKT_EOS
    calls[1][1][-1]["granule"] = natural - 37
    refs = [helpers.oracle_decode(oracle, c["channels"], c["size0"], c["size1"], calls[0][s] + calls[1][s], **kw) for s in range(n)]
    assert refs[1][0].shape[1] == natural - 37
    return calls, slots, refs


# ---- decoding it --------------------------------------------------------------------------------------------------------------

_CALL_ROUTE = r"\[vpz host\] packets \d+: route (\w+),"


def _decode(ctx, capfd, c, calls, kv):
    """A fresh decoder under env(kv) takes the calls one after the other.  Returns (per stream: PCM [channels, samples], per
    stream (position, has_clipped), per call: its host profile -- for the three-pass path, which cuts no runs, the route alone)."""
    from vorbispizza_amd import Decoder, capi, make_packets
    floors, mappings = _setup(c)
    C_, n = c["channels"], len(calls[0])
    layout = {"planar": capi.OUT_PLANAR, "interleaved": capi.OUT_INTERLEAVED, "planar_s16": capi.OUT_PLANAR_S16,
              "interleaved_s16": capi.OUT_INTERLEAVED_S16}[c["out"]]
    settings = dict.fromkeys(SWITCHES)
    settings.update(c["kv"])
    settings.update(kv)
    parts, profs = [[] for _ in range(n)], []
    with env(**settings):
        dec = Decoder(ctx, C_, c["size0"], c["size1"], floors=floors, mappings=mappings, n_streams=n, clip_samples=c["clip"])
        for call in calls:
            flat = [(s, p) for s in range(n) for p in call[s]]  # stream-major, residues back to back
            pk = make_packets(len(flat))
            off = 0
            for i, (s, p) in enumerate(flat):
                pk[i]["stream"], pk[i]["flags"], pk[i]["mapping"], pk[i]["granule"], pk[i]["residue_offset"] = \
                    s, p["flags"], p["mapping"], p["granule"], off
                off += p["residue"].size
            res = np.concatenate([p["residue"] for _, p in flat])
            if c["i16"]:
                assert np.array_equal(res, np.round(res))
                res = res.astype(np.int16)
            posts = counts = None
            if c["kind"] != "nofloor":
                posts = np.concatenate([p["posts"] for _, p in flat]).astype(np.int16)
                counts = np.concatenate([p["post_count"] for _, p in flat]).astype(np.uint8)
            if c["kind"] == "floor0":
                dec.set_floor0_data(np.concatenate([p["f0_amp"] for _, p in flat]), np.concatenate([p["f0_coeff"] for _, p in flat]))
            capfd.readouterr()
            with env(VPZ_HOST_PROFILE=1):
                outs = dec.synth(pk, res, posts, counts, out_layout=layout)
            err = capfd.readouterr().err
            if re.search(r"\[vpz host\] cut:", err):
                profs.append(helpers.host_profile(err))
            else:
                routes = re.findall(_CALL_ROUTE, err)
                assert len(routes) == 1, err[-2000:]
                profs.append({"route": routes[0]})
            for s in range(n):
                parts[s].append(outs[s].T if "interleaved" in c["out"] else outs[s])
        state = [(dec.position(s), dec.has_clipped(s)) for s in range(n)]
        dec.close()
    return [np.concatenate(p, axis=1) for p in parts], state, profs


def _check_shape(c, calls, profs, group):
    """The cut lines say what the case is about: R, the rule, the route, and the run count the rule gives."""
    r_max, R = R_MAX[c["kernel"]], c["R"]
    dual = c["route"] in ("stereo", "pairs")
    for call, prof in zip(calls, profs):
        what = "%s: %r" % (c["id"], prof)
        assert prof["route"] == c["route"], what
        assert (prof["R"], prof["by"]) == (R, c["by"]), what
        # compact runs exist only behind the parallel host pass (and explicit ones, VPZ_NO_COMPACT=1, are written by it too where
        # the case asks for it): a pass that declined the batch would quietly make the case another one
        assert prof["pass1"] == ("parallel" if "VPZ_PAR_MIN_PACKETS" in c["kv"] else "serial"), what
        if c["by"] == "length":
            runs = [(s, j, cnt) for s, j, cnt in helpers.by_length_runs([len(p) for p in call], R)]
        else:
            pkts = [[(p["flags"], p["mapping"]) for p in stream] for stream in call]
            cut = helpers.by_cost_runs(pkts, prof["target"], r_max, dual, prof["heavy"])
            runs = [(s, j, cnt) for s, j, cnt, _, _ in cut]
            if c["stretch"]:
                # the 45 short blocks: the frame cap ends a run that the cost target (8 R eighths at least) would let go on
                assert prof["target"] >= 8 * R and any(capped and cnt == r_max and units < prof["target"] - 8
                                                       for _, _, cnt, units, capped in cut), (what, cut)
        assert prof["runs"] == len(runs), (what, len(runs))
        assert max(cnt for _, _, cnt in runs) <= r_max
        REACHED.add((group, R))
        for s, j, cnt in runs:  # a stream's first run starts from nothing or the saved state, the others recompute a block
            REACHED.add((group, R, cnt + (1 if j > 0 else 0)))


def _to_s16(x):  # tests/test_s16_gpu.py (AssetTest.cs:131-132)
    return np.clip((x.astype(np.float32) * np.float32(32768.0)).astype(np.int64), -32768, 32767).astype(np.int16)


def _run_case(ctx, oracle, capfd, c, group):
    calls, slots, refs = _batch(c, oracle)
    a, state_a, profs = _decode(ctx, capfd, c, calls, dict(VPZ_PLAN_SLOTS=slots))
    if c["control"]:  # the three-pass path cuts no runs: the knob has nothing to change
        assert [p["route"] for p in profs] == ["generic", "generic"], profs
    else:
        _check_shape(c, calls, profs, group)
    b, state_b, profs_b = _decode(ctx, capfd, c, calls, dict(VPZ_PLAN_SLOTS=None))
    assert all(p["route"] == profs[0]["route"] and p.get("R", 4) == 4 for p in profs_b), profs_b
    assert state_a == state_b
    a_float = None
    if "s16" in c["out"]:  # the same cut with float PCM
        a_float, state_f, profs_f = _decode(ctx, capfd, dict(c, out=c["out"][:-4]), calls, dict(VPZ_PLAN_SLOTS=slots))
        assert state_f == state_a and [p.get("R") for p in profs_f] == [p.get("R") for p in profs]
    worst = 0.0
    for s, (ref, pos, clipped) in enumerate(refs):
        what = (c["id"], "stream", s)
        assert a[s].shape == b[s].shape == ref.shape, (what, a[s].shape, b[s].shape, ref.shape)
        if a[s].dtype == np.int16:
            assert np.array_equal(a[s], b[s]), what
        else:
            assert np.array_equal(a[s].view(np.uint32), b[s].view(np.uint32)), (what, "runs of R against runs of 4")
        assert np.isfinite(ref).all() and ref.size > 0
        scale = max(1.0, float(np.abs(ref).max()))
        if a[s].dtype == np.int16:
            # tests/test_s16_gpu.py: 16-bit PCM is the reference's conversion of the float PCM of the same decode, bit for bit;
            # that float PCM meets the oracle at the float bar
            assert np.array_equal(a[s], _to_s16(a_float[s])), (what, "s16 against the conversion of the float decode")
        for got in ([a_float[s]] if a[s].dtype == np.int16 else [a[s]]):
            assert got.shape == ref.shape
            err = float(np.abs(got - ref).max())
            worst = max(worst, err / scale)
            assert err <= (TOL_CURVE if c["kind"] == "curve" else TOL) * scale, (what, err, scale)
        assert state_a[s] == (pos, clipped), (what, state_a[s], pos, clipped)
    print("%s: slots %d, cuts %r; oracle max |err| / scale %.3g" % (c["id"], slots, [(p.get("R"), p.get("runs")) for p in profs], worst))
    return calls, a, state_a


# ---- the routes ---------------------------------------------------------------------------------------------------------------

BIG = [
    case("512-4096-R5-mixed-planar", "big", 5, 3, 512, 4096, "mixed", in_layout="alternate", route="big"),
    case("4096-4096-R16-mixed-interleaved", "big", 16, 3, 4096, 4096, "mixed", in_layout="alternate", out="interleaved", route="big"),
    case("1024-8192-R31-mixed-s16", "big", 31, 3, 1024, 8192, "mixed", in_layout="alternate", out="planar_s16", clip=True, route="big"),
    case("8192-8192-R32-floor-planar", "big", 32, 3, 8192, 8192, "floor", in_layout="interleaved", route="big"),
    case("1024-8192-R32-nofloor-interleaved", "big", 32, 3, 1024, 8192, "nofloor", out="interleaved", route="big"),
    case("512-4096-R32-mixed-s16", "big", 32, 3, 512, 4096, "mixed", in_layout="alternate", out="planar_s16", route="big"),
    case("512-4096-R32-floor0-in-front", "big", 32, 3, 512, 4096, "floor0", route="big"),
    case("4096-4096-R31-int16-residue", "big", 31, 3, 4096, 4096, "floor", i16=True, route="big"),
    case("8192-8192-R5-mixed-clip", "big", 5, 3, 8192, 8192, "mixed", in_layout="alternate", clip=True, route="big"),
    case("4096-8192-three-pass-control", "big", 5, 3, 4096, 8192, "mixed", in_layout="alternate", route="generic", control=True),
]


@pytest.mark.parametrize("c", BIG)
def test_synth_big_at_long_runs(ctx, oracle, capfd, c):
    """synth_big_kernel: up to 33 staged frames (66 descriptor words, the copy loop's second trip), at 8192 the tail through
    global memory 32 times in a row; floored and coupled, planar / Residue2 / already floored packets, every output layout, a type-0
    floor applied in front, int16 residue.  Also against the three-pass path (VPZ_NO_BIG=1) under the rule of
    test_the_fused_kernel_for_4096_and_8192_blocks_equals_the_three_pass_path: the same values, and the only bit patterns that may
    differ are zeros, +0.0 here.  (4096, 8192) is not the big kernel's: the control, on the three-pass path either way."""
    calls, a, state = _run_case(ctx, oracle, capfd, c, "big")
    want, want_state, profs = _decode(ctx, capfd, c, calls, dict(VPZ_NO_BIG=1))
    assert all(p["route"] == "generic" for p in profs), profs
    assert [clipped for _, clipped in state] == [clipped for _, clipped in want_state]
    for s in range(len(a)):
        assert a[s].shape == want[s].shape and np.array_equal(a[s], want[s]), (c["id"], s)
        if a[s].dtype != np.int16:
            differing = a[s].view(np.uint32) != want[s].view(np.uint32)
            assert (a[s][differing] == 0).all() and not np.signbit(a[s][differing]).any(), (c["id"], s)


GENERAL = [
    case("512-1024-1ch-R5-nofloor", "general", 5, 1, 512, 1024, "nofloor"),
    case("256-1024-2ch-R8-floor-coupled", "general", 8, 2, 256, 1024, "floor", in_layout="interleaved", kv=dict(VPZ_NO_DUAL=1), route="group"),
    case("1024-2048-3ch-R15-floor-coupled", "general", 15, 3, 1024, 2048, "floor", in_layout="interleaved", out="interleaved", route="group"),
    case("512-512-3ch-R16-nofloor", "general", 16, 3, 512, 512, "nofloor"),
    case("512-1024-3ch-R16-floor-coupled", "general", 16, 3, 512, 1024, "floor", route="group"),
    case("256-1024-1ch-R16-floor", "general", 16, 1, 256, 1024, "floor"),
    case("1024-2048-2ch-R16-nofloor", "general", 16, 2, 1024, 2048, "nofloor", kv=dict(VPZ_NO_DUAL=1), out="interleaved"),
    case("512-512-2ch-R15-floor-coupled", "general", 15, 2, 512, 512, "floor", kv=dict(VPZ_NO_DUAL=1, VPZ_NO_GROUP=1)),
]


@pytest.mark.parametrize("c", GENERAL)
def test_the_general_variant_at_long_runs(ctx, oracle, capfd, c):
    """synth_kernel's general variant (512 / 1024 in the mix): 17 staged frames; 1, 2 and 3 channels, already floored and
    Floor1 + coupling (in group mode, and through the separate coupling pass)."""
    _run_case(ctx, oracle, capfd, c, "general")


def _plain(name, R, channels, kind, descriptors, **kw):
    """`descriptors`: "compact" (the parallel host pass writes two bytes per frame) or "explicit" (VPZ_NO_COMPACT=1: FrameDescs)"""
    kv = dict(PARALLEL, VPZ_NO_COMPACT=None if descriptors == "compact" else 1, **kw.pop("kv", {}))
    return case("%s-R%d-%s" % (name, R, descriptors), "standard", R, channels, 256, 2048, kind, kv=kv, **kw)


PLAIN = [
    _plain("1ch-exact-floor-curve", 5, 1, "curve", "compact", all_long=True),
    _plain("1ch-exact-floor-curve", 32, 1, "curve", "explicit", all_long=True),
    _plain("1ch-exact-floor-curve", 31, 1, "curve", "compact", all_long=True),
    _plain("1ch-exact-floor-curve", 16, 1, "curve", "explicit", all_long=True),
    _plain("3ch-already-floored", 16, 3, "nofloor", "compact"),
    _plain("3ch-already-floored", 31, 3, "nofloor", "explicit"),
    _plain("3ch-already-floored", 32, 3, "nofloor", "compact"),
    _plain("3ch-already-floored", 5, 3, "nofloor", "explicit"),
    _plain("3ch-already-floored", 32, 3, "nofloor", "explicit"),
    # ten channels: beyond group mode's eight and, with VPZ_NO_PAIRS=1, not the pair route's -- the batch needs the separate coupling
    # pass, and behind it no run is compact (synth_plan.hip: compact only where no coupling is needed or the fused routes take it).
    # Explicit descriptors either way: written by the parallel host pass, and by the serial one.
    case("10ch-coupling-pass-R32-parallel-host-pass", "standard", 32, 10, 256, 2048, "floor", kv=dict(PARALLEL, VPZ_NO_PAIRS=1)),
    case("10ch-coupling-pass-R16-parallel-host-pass", "standard", 16, 10, 256, 2048, "floor", kv=dict(PARALLEL, VPZ_NO_PAIRS=1)),
    case("10ch-coupling-pass-R5-serial-host-pass", "standard", 5, 10, 256, 2048, "floor", kv=dict(VPZ_NO_PAIRS=1)),
    case("10ch-coupling-pass-R31-serial-host-pass", "standard", 31, 10, 256, 2048, "floor", kv=dict(VPZ_NO_PAIRS=1)),
]


@pytest.mark.parametrize("c", PLAIN)
def test_one_wave_per_channel_at_long_runs(ctx, oracle, capfd, c):
    """synth_kernel, 256 / 2048, waves on their own: one channel with the exact floor curve of test_floor_curve_is_bit_exact (and
    its bar) and three channels already floored, each with compact runs and with explicit descriptors (VPZ_NO_COMPACT=1); ten
    channels behind coupling_tile_kernel, where descriptors are always explicit."""
    _run_case(ctx, oracle, capfd, c, "plain")  # (the cut lines' pass1 field says that the parallel pass wrote the descriptors)


GROUP = [
    case("256-2048-3ch-R5-all-long-planar", "standard", 5, 3, 256, 2048, "floor", in_layout="interleaved", all_long=True, route="group"),
    case("256-2048-6ch-R16-all-long-interleaved", "standard", 16, 6, 256, 2048, "floor", in_layout="interleaved", all_long=True,
         out="interleaved", kv=dict(VPZ_NO_PAIRS=1), route="group"),
    case("256-2048-8ch-R31-all-long-s16", "standard", 31, 8, 256, 2048, "floor", in_layout="interleaved", all_long=True,
         out="interleaved_s16", kv=dict(VPZ_NO_PAIRS=1), route="group"),
    case("256-2048-8ch-R32-all-long-planar", "standard", 32, 8, 256, 2048, "floor", all_long=True, kv=dict(VPZ_NO_PAIRS=1), route="group"),
    # (512 in the mix: the general variant's group mode, 17 staged frames)
    case("512-2048-3ch-R16-interleaved", "general", 16, 3, 512, 2048, "floor", in_layout="interleaved", out="interleaved", route="group"),
    case("512-2048-6ch-R15-planar-s16", "general", 15, 6, 512, 2048, "floor", in_layout="interleaved", out="planar_s16",
         kv=dict(VPZ_NO_PAIRS=1), route="group"),
    case("256-2048-3ch-R32-all-long-compact", "standard", 32, 3, 256, 2048, "floor", in_layout="interleaved", all_long=True,
         kv=PARALLEL, route="group"),
]


@pytest.mark.parametrize("c", GROUP)
def test_group_mode_cut_by_length_at_long_runs(ctx, oracle, capfd, c):
    """Group mode outside the 6 channels at 256 / 2048 of the full-size test: 3, 6 and 8 channels -- with 3, a full run shares its
    workgroup with a partial run of another stream, whose idle iterations keep the barriers matched -- all-long streams at
    256 / 2048 and window switching at 512 / 2048, every output layout."""
    _run_case(ctx, oracle, capfd, c, "group-length")


GROUP_COST = [case("256-2048-6ch-R%d-%s" % (R, out), "standard", R, 6, 256, 2048, "floor", in_layout="interleaved", out=out, by="cost",
                   kv=dict(PARALLEL, VPZ_NO_PAIRS=1), route="group", stretch=R == 32, lens=(32, 33, 65) if R == 32 else None)
              for R, out in ((5, "interleaved"), (16, "planar"), (31, "interleaved_s16"), (32, "interleaved"))]


@pytest.mark.parametrize("c", GROUP_COST)
def test_group_mode_cut_by_cost_at_long_runs(ctx, oracle, capfd, c):
    """Group mode with short blocks riding in batches: runs of equal cost, up to the 32-frame cap -- at R = 32 a stream with 45
    short blocks in a row, whose runs the cap ends."""
    _run_case(ctx, oracle, capfd, c, "group-cost")


DUAL = [case("%s-R%d-%s-%s" % (route, R, kind, lay), "dual", R, ch, 256, 2048, kind, in_layout=lay, out=out, by="cost",
             kv=dict(PARALLEL, **kv), route=route, lens=(63, 64, 127))
        for (route, ch, kv), rows in (
            (("stereo", 2, {}), ((5, "nofloor", "planar", "planar"), (31, "floor", "interleaved", "interleaved"),
                                 (62, "floor", "planar", "planar_s16"), (63, "floor", "interleaved", "planar"),
                                 (63, "nofloor", "planar", "interleaved"))),
            (("pairs", 6, dict(VPZ_PAIRS=1)), ((5, "floor", "interleaved", "planar"), (31, "floor", "planar", "interleaved"),
                                               (62, "nofloor", "planar", "planar"), (63, "floor", "interleaved", "interleaved"))))
        for R, kind, lay, out in rows]


@pytest.mark.parametrize("c", DUAL)
def test_the_stereo_kernel_and_the_pair_route_cut_by_cost_at_long_runs(ctx, oracle, capfd, c):
    """Streams of 63, 64 and 127 frames with window switching: runs cut by cost up to 63 frames -- 64 staged ones, a lane each,
    the last lane used."""
    _run_case(ctx, oracle, capfd, c, c["route"])


def test_every_run_length_of_every_route_was_reached():
    """What the cases above reported on their cut lines: every route at 5, r_max / 2, r_max - 1 and r_max, and at r_max a run that
    starts its stream (r_max staged frames) and one that recomputes its predecessor (r_max + 1).  A planner change that drops one of
    these shapes shows here.  (Reads what the tests above left in REACHED: run the file as a whole.)"""
    want = set()
    for group, kernel in (("big", "big"), ("general", "general"), ("plain", "standard"), ("group-length", "standard"),
                          ("group-cost", "standard"), ("stereo", "dual"), ("pairs", "dual")):
        r_max = R_MAX[kernel]
        want |= {(group, R) for R in R_LIST[kernel]} | {(group, r_max, r_max), (group, r_max, r_max + 1)}
    assert not want - REACHED, sorted(want - REACHED)
