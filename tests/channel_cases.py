"""vpz_decoder_synth at the limits of channel count and coupling tables: ONE case list, used by test_channel_cases_cpu.py (do the
cases hold what they claim?  the oracle and a few lines of arithmetic, no GPU) and by test_channel_limits_gpu.py (does the device
compute them, on the route each case names?).

A case: the channel count, the floors, the mappings (coupling steps, a floor per channel), the input layout, a skew of the packets'
residue offsets, and the routes to run it on -- (name, environment, the word VPZ_HOST_PROFILE=1 must print).  Mapping m belongs to
the short blocks when m is even and to the long ones when it is odd; a case with more than two mappings spreads its packets over
them (`pick`).  Every case: 2 streams (the grid case: 34) of 14 packets (the grid case: 8), 256 / 2048 blocks with window
switching, a tenth of the records silent, two calls per stream.

The rules of vpz_decoder_create and SynthPlan::dual_usable / group_usable are restated here in Python (step_table, pair_table,
expected_route): the CPU file checks every case's words against them, the GPU file checks the words against the library."""
import functools

import numpy as np

import helpers

TOL = 1e-5                      # the bar of test_pairs_gpu.py / test_dual_gpu.py: |got - ref|max <= TOL * max(1, |ref|max)
MAX_STEP_PAIRS = 128            # kGroupMaxStepPairs: the step pairs the fused kernels stage in LDS
PAD = 4                         # a mapping's list starts on a multiple of four pairs (the kernels read four steps at once)
OFFSET_FIELD = 256              # a frame's flag word has 8 bits for the place of its mapping's first step (and 8 for the count)
TILE_CHANNELS = 32              # kCouplingTileChannels: coupling_tile_kernel up to here, coupling_kernel beyond
GROUP_CHANNELS = 8              # kGroupMaxChannels

F_SA, F_LA = (helpers.SHORT_XLIST, 2), (helpers.LONG_XLIST, 2)
# other post counts (11 / 17 / 7 against 19 / 29) and multipliers: what two records side by side in a pair may differ in
F_SB = ([0, 128, 64, 32, 96, 16, 48, 80, 112, 8, 24], 3)
F_LB = ([0, 1024, 512, 256, 768, 128, 384, 640, 896, 64, 192, 320, 448, 576, 704, 832, 960], 1)
F_SC = ([0, 128, 100, 50, 25, 75, 10], 4)
FLOORS2 = [F_SA, F_LA]
FLOORS4 = [F_SA, F_LA, F_SB, F_LB]          # kPrepFloorsInLds = 4: the LDS copy of floor1_unwrap_kernel is full
FLOORS5 = [F_SA, F_LA, F_SB, F_LB, F_SC]    # ... and one more: its instantiation that reads the floors from memory

HOSTS = {  # the host pass: serial (explicit descriptors), parallel with compact runs where the batch allows, parallel with explicit ones
    "serial": dict(VPZ_PAR_MIN_PACKETS=1 << 40, VPZ_HOST_THREADS=None, VPZ_NO_COMPACT=None),
    "compact": dict(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4, VPZ_NO_COMPACT=None),
    "explicit": dict(VPZ_PAR_MIN_PACKETS=1, VPZ_HOST_THREADS=4, VPZ_NO_COMPACT=1),
}


def route(name, word, host="serial", pairs=None, no_pairs=None, no_group=None, no_dual=None, dual_run=None):
    """(name, environment, word): every switch a route depends on is named, set or unset (the style of test_pairs_gpu.ROUTES)."""
    kv = dict(VPZ_PAIRS=pairs, VPZ_NO_PAIRS=no_pairs, VPZ_NO_GROUP=no_group, VPZ_NO_DUAL=no_dual, VPZ_DUAL_RUN=dual_run)
    kv.update(HOSTS[host])
    return (name, kv, word)


PLAIN = route("plain", "separate", no_pairs=1, no_group=1, no_dual=1)   # the separate coupling pass + the one-channel kernel
DEFAULT_SEPARATE = route("default", "separate", host="compact")         # the decoder's own choice, where that is the separate pass too


def maps2(channels, steps0, steps1=None, floors0=None, floors1=None):
    return [{"coupling": list(steps0), "channel_floor": list(floors0 or [0] * channels)},
            {"coupling": list(steps0 if steps1 is None else steps1), "channel_floor": list(floors1 or [1] * channels)}]


def many_maps(channels, steps_of):
    """steps_of: the coupling steps of mappings 0, 1, 2, ...; floor 0 for the even (short) ones, floor 1 for the odd (long) ones."""
    return [{"coupling": list(st), "channel_floor": [m & 1] * channels} for m, st in enumerate(steps_of)]


def chain(channels):
    return [(c, c + 1) for c in range(channels - 1)]


def _case(id, channels, maps, routes, floors=FLOORS2, interleaved=False, skew=0, s16=False, n_streams=2, frames=14, device=(),
          min_runs=0):
    """routes[0] is the route compared with the oracle; device: [(shift in floats, environment, word)] device-memory calls whose
    residue pointer lies that far off its allocation; min_runs: every call of routes[0] must cut more runs than this."""
    return dict(id=id, channels=channels, maps=maps, routes=list(routes), floors=list(floors), interleaved=interleaved, skew=skew,
                s16=s16, n_streams=n_streams, frames=frames, device=list(device), min_runs=min_runs,
                pick="parity" if len(maps) <= 2 else "spread")


def _count_cases():
    out = []
    # 7: group mode at a count no test has (div_magic, the cooperative interleaved store); tile width 512 behind VPZ_NO_GROUP=1
    st7 = [(0, 1), (2, 3), (5, 4), (6, 0)]
    out.append(_case("c7-group", 7, maps2(7, st7, [(6, 5), (1, 2)]), [route("group", "group", host="compact"),
                                                                    route("tile512", "separate", no_group=1), PLAIN],
                     interleaved=True, s16=True))
    # 9: the first odd count past group mode: coupling_tile_kernel at width 256, a chain of dependent steps
    out.append(_case("c9-chain", 9, maps2(9, chain(9)), [DEFAULT_SEPARATE, PLAIN], interleaved=True))
    # 31, 32: the tile kernel's last counts; adjacent-odd, distant and both-ways steps; 32 also on the pair route
    st31 = [(3, 4), (1, 30), (10, 11), (11, 10), (29, 28)]
    out.append(_case("c31-tile", 31, maps2(31, st31, [(30, 0), (4, 3)]), [DEFAULT_SEPARATE, PLAIN]))
    out.append(_case("c31-tile-ilv-chain", 31, maps2(31, chain(31)), [DEFAULT_SEPARATE, PLAIN], interleaved=True))
    out.append(_case("c32-ilv-uncoupled", 32, maps2(32, []), [route("pairs", "pairs", host="compact", pairs=1), PLAIN],
                     interleaved=True))       # de-interleave only: 32 x 257 floats of LDS in the tile kernel
    even32 = [(c, c + 1) for c in range(0, 32, 2)]
    out.append(_case("c32-pairs", 32, maps2(32, even32, [(c + 1, c) for c in range(0, 32, 4)]),
                     [route("pairs", "pairs", host="compact", pairs=1), route("pairs-serial", "pairs", pairs=1), PLAIN]))
    # 33: coupling_kernel's first count; odd, so never pairs
    st33 = [(3, 4), (1, 32), (20, 21), (21, 20), (32, 0)]
    out.append(_case("c33-fallback-ilv", 33, maps2(33, st33, [(32, 31), (0, 16)]), [DEFAULT_SEPARATE, PLAIN], interleaved=True, s16=True))
    out.append(_case("c33-fallback-chain", 33, maps2(33, chain(33)), [DEFAULT_SEPARATE, PLAIN]))
    # 64: 32 pairs, more than 32 runs in a call (the grid's second group of 8 chunks x n_pairs); coupling_kernel behind VPZ_NO_PAIRS=1
    st64 = [(c, c + 1) for c in range(0, 64, 2)]
    out.append(_case("c64-pairs-grid", 64, maps2(64, st64, [(1, 0), (63, 62), (31, 30)]),
                     [route("pairs", "pairs", host="compact", pairs=1, dual_run=4), route("no-pairs", "separate", no_pairs=1), PLAIN],
                     n_streams=34, frames=8, s16=True, min_runs=32))
    # 254: the pair route's last count -- see _limit_cases; and a chain that keeps it off the pair route: 253 dependent steps
    out.append(_case("c254-chain", 254, maps2(254, chain(254)), [DEFAULT_SEPARATE, PLAIN], interleaved=True))
    # 255: the ABI's maximum
    st255 = [(1, 200), (130, 131), (254, 0), (3, 4), (4, 3)]
    out.append(_case("c255-max", 255, maps2(255, st255, [(253, 254), (200, 1)]), [DEFAULT_SEPARATE, PLAIN], s16=True))
    return out


def pairs254(n0, n1):
    """254 channels: the first n0 of these coupled pairs in the short blocks' mapping, the last n1 in the long blocks' -- among them
    distant ones, (1, 200) and (130, 131) beyond channel 127, adjacent-odd ones, the angle in front of the magnitude."""
    special = [(1, 200), (130, 131), (3, 4), (253, 252), (129, 2), (201, 128)]
    used = {c for p in special for c in p}
    free = [c for c in range(254) if c not in used]
    rest = [(free[2 * i + 1], free[2 * i]) if i & 1 else (free[2 * i], free[2 * i + 1]) for i in range(70)]
    pool = (special + rest)[:65]
    return maps2(254, pool[:n0], pool[65 - n1:])


def _limit_cases():
    out = []
    alt = lambda n: [((0, 1), (1, 0))[i & 1] for i in range(n)]
    stereo = [route("stereo", "stereo", host="compact"), PLAIN]
    # stereo, ONE mapping of 128 / 129 steps (the short blocks' mapping is uncoupled): the staged table full, and one step too many
    out.append(_case("lim-stereo-128-steps", 2, maps2(2, [], alt(128)), stereo))
    out.append(_case("lim-stereo-129-steps", 2, maps2(2, [], alt(129)), [DEFAULT_SEPARATE, PLAIN]))
    # stereo, 32 / 33 mappings of 2 ... 4 steps: the padded lists fill the table / the 33rd starts at pair 128
    sizes = [2, 3, 4]
    out.append(_case("lim-stereo-32-mappings", 2, many_maps(2, [alt(4 if m == 31 else sizes[m % 3]) for m in range(32)]), stereo,
                     interleaved=True))
    out.append(_case("lim-stereo-33-mappings", 2, many_maps(2, [alt(sizes[m % 3]) for m in range(33)]), [DEFAULT_SEPARATE, PLAIN],
                     interleaved=True))
    # group mode, 6 channels, steps that are no pairs: the same two sides
    g6 = lambda n: [(0, 1), (1, 2), (3, 4), (5, 3)][:n]
    out.append(_case("lim-group-32-mappings", 6, many_maps(6, [g6(4 if m == 31 else sizes[m % 3]) for m in range(32)]),
                     [route("group", "group", host="compact"), PLAIN], interleaved=True))
    out.append(_case("lim-group-33-mappings", 6, many_maps(6, [g6(sizes[m % 3]) for m in range(33)]), [DEFAULT_SEPARATE, PLAIN],
                     interleaved=True))
    # the pair route at 254 channels: 64 + 64 pair-steps fill the pairs' own table; 64 + 65 do not
    out.append(_case("lim-pairs-254-128-steps", 254, pairs254(64, 64),
                     [route("pairs", "pairs", host="compact", pairs=1), route("pairs-serial", "pairs", pairs=1), PLAIN]))
    out.append(_case("lim-pairs-254-129-steps", 254, pairs254(64, 65), [route("default", "separate", host="compact", pairs=1), PLAIN]))
    # ... and the Residue2 vector read by columns: 8 bytes where a pair's channels are adjacent, 4 + 4 for (1, 200)
    out.append(_case("lim-pairs-254-residue2", 254, pairs254(64, 64), [route("pairs", "pairs", host="compact", pairs=1), PLAIN],
                     interleaved=True))
    # the pair route, 4 channels, 65 mappings of one step: the decoder-wide table reaches pair 256 at mapping 64 -- beyond the
    # 8 bits of a frame's offset field, which the pairs (a table of their own: 65 steps) never look at
    one = lambda m: [[(0, 1)], [(1, 0)], [(2, 3)]][m % 3]
    pair_routes = [route("pairs-serial", "pairs", pairs=1), route("pairs-explicit", "pairs", host="explicit", pairs=1),
                   route("pairs-compact", "pairs", host="compact", pairs=1), PLAIN]
    out.append(_case("lim-pairs-65-mappings", 4, many_maps(4, [one(m) for m in range(65)]), pair_routes))
    # ... 255 mappings, the last 128 coupled: the pairs' table full, the top of the 8-bit mapping field, decoder-wide offsets up to 508
    out.append(_case("lim-pairs-255-mappings", 4, many_maps(4, [one(m) if m >= 127 else [] for m in range(255)]), pair_routes))
    # ... 256 mappings: the most vpz_decoder_create takes, one more than the pair route does
    out.append(_case("lim-256-mappings", 4, many_maps(4, [one(m) for m in range(256)]),
                     [route("default", "separate", host="compact", pairs=1), PLAIN]))
    # VPZ_MAX_COUPLING = 256 steps in one mapping: beyond the 8 bits of a frame's step count, the separate pass takes them all
    long_chain = [chain(9)[i % 8] if (i // 8) % 2 == 0 else chain(9)[7 - i % 8][::-1] for i in range(256)]
    out.append(_case("lim-256-steps", 9, maps2(9, long_chain, chain(9)), [DEFAULT_SEPARATE, PLAIN], interleaved=True))
    out.append(_case("lim-256-steps-stereo", 2, maps2(2, alt(256), alt(3)), [DEFAULT_SEPARATE, PLAIN]))
    return out


def _floor_cases():
    out = []
    for name, floors, short in (("4", FLOORS4, (0, 2)), ("5", FLOORS5, (0, 2, 4))):
        fl = lambda C: dict(floors0=[short[c % len(short)] for c in range(C)], floors1=[(1, 3)[c & 1] for c in range(C)])
        out.append(_case("floors%s-stereo" % name, 2, maps2(2, [(0, 1)], [(1, 0)], **fl(2)),
                         [route("stereo", "stereo", host="compact"), PLAIN], floors=floors, interleaved=True))
        out.append(_case("floors%s-c6" % name, 6, maps2(6, [(0, 1), (2, 3)], [(1, 0), (5, 4)], **fl(6)),
                         [route("pairs", "pairs", host="compact", pairs=1), route("group", "group", no_pairs=1), PLAIN], floors=floors,
                         interleaved=True))
        out.append(_case("floors%s-c33" % name, 33, maps2(33, [(0, 1), (32, 2)], [(1, 0)], **fl(33)), [DEFAULT_SEPARATE, PLAIN],
                         floors=floors))
    return out


def _alignment_cases():
    """residue_offset off a multiple of four floats by 1, 2, 3: the stereo and pair kernels read 8 bytes (planar packets, and the
    pairs in either layout), the stereo kernel's Residue2 loads and group mode 16; everything else goes to the separate pass, which
    reads element by element.  Skew 0: the host-memory call is aligned, a device-memory call whose pointer is not takes the same
    decision on the address."""
    out = []
    m2, m6 = maps2(2, [(0, 1)], [(1, 0), (0, 1)]), maps2(6, [(0, 1), (2, 3)], [(1, 0), (5, 4)])
    dflt = dict(VPZ_PAIRS=None, VPZ_NO_PAIRS=None, VPZ_NO_GROUP=None, VPZ_NO_DUAL=None, VPZ_DUAL_RUN=None, **HOSTS["compact"])
    for skew in (0, 1, 2, 3):
        w8, w16 = ("separate" if skew & 1 else None), ("separate" if skew & 3 else None)
        dev = [(1, dflt, "separate")] if skew == 0 else []
        out.append(_case("align%d-stereo-planar" % skew, 2, m2, [route("fast", w8 or "stereo", host="compact"), PLAIN], skew=skew,
                         device=dev + ([(2, dflt, "stereo")] if skew == 0 else [])))
        out.append(_case("align%d-stereo-residue2" % skew, 2, m2, [route("fast", w16 or "stereo", host="compact"), PLAIN], skew=skew,
                         interleaved=True, device=dev))
        out.append(_case("align%d-group-c6" % skew, 6, m6, [route("fast", w16 or "group", host="compact", no_pairs=1), PLAIN], skew=skew,
                         interleaved=True, device=[(s, dict(k, VPZ_NO_PAIRS=1), w) for s, k, w in dev]))
        out.append(_case("align%d-pairs-c6" % skew, 6, m6, [route("fast", w8 or "pairs", host="compact", pairs=1), PLAIN], skew=skew,
                         interleaved=bool(skew & 2), device=[(s, dict(k, VPZ_PAIRS=1), w) for s, k, w in dev]))
    return out


CASES = _count_cases() + _limit_cases() + _floor_cases() + _alignment_cases()
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]


# ---- the rules restated ------------------------------------------------------------------------------------------------------

def step_table(maps):
    """vpz_decoder_create's decoder-wide table: (first pair of every mapping's list, None where it has no steps; pairs in all --
    the lists of coupled mappings start on multiples of PAD pairs, the last one is not padded; most steps any mapping has)."""
    first, size = [], 0
    for m in maps:
        n = len(m["coupling"])
        if n:
            size = (size + PAD - 1) // PAD * PAD
        first.append(size if n else None)
        size += n
    return first, size, max([len(m["coupling"]) for m in maps] or [0])


def wide_steps_fit(maps):
    """group mode and the stereo kernel: the whole table staged in LDS, count and first pair of a mapping in 8 bits each"""
    first, size, most = step_table(maps)
    return size <= MAX_STEP_PAIRS and most <= 255 and all(f is None or f < OFFSET_FIELD for f in first)


def pair_table(channels, maps):
    """The pair route's setup: None where the steps of all mappings do not join the channels two by two, else (the pairs, the first
    step of every (pair, mapping) list in the pairs' own table, the steps in it)."""
    if channels < 4 or channels > 254 or channels & 1 or len(maps) > 255:
        return None
    partner = [-1] * channels
    for m in maps:
        for mag, ang in m["coupling"]:
            if partner[mag] < 0 and partner[ang] < 0:
                partner[mag], partner[ang] = ang, mag
            elif partner[mag] != ang or partner[ang] != mag:
                return None
    pairs, lone = [], -1
    for c in range(channels):
        if partner[c] > c:
            pairs.append((c, partner[c]))
        elif partner[c] < 0:
            if lone < 0:
                lone = c
            else:
                pairs.append((lone, c))
                lone = -1
    if lone >= 0:
        return None
    firsts, total = [], 0
    for a, b in pairs:
        for m in maps:
            cnt = sum(1 for mag, _ in m["coupling"] if mag in (a, b))
            if cnt > 255 or total > 255:
                return None
            firsts.append(total)
            total += cnt
    return (pairs, firsts, total) if total <= MAX_STEP_PAIRS else None


def expected_route(c, kv, out_interleaved, skew=None, device_shift=None):
    """The word of the call line: vpz_decoder_create's group_ok / dual_ok / pairs, then SynthPlan::dual_usable and plan_frames'
    use_group, for a floored batch of one input layout."""
    on = lambda k: bool(kv.get(k))
    skew = c["skew"] if skew is None else skew
    C, maps, ilv = c["channels"], c["maps"], c["interleaved"]
    fit = wide_steps_fit(maps)
    group_ok = 2 <= C <= GROUP_CHANNELS and fit and not on("VPZ_NO_GROUP")
    stereo_ok = C == 2 and fit and not on("VPZ_NO_DUAL")
    pairs = pair_table(C, maps) is not None and not (on("VPZ_NO_DUAL") or on("VPZ_NO_PAIRS") or on("VPZ_NO_GROUP"))
    need_coupling = ilv or any(m["coupling"] for m in maps)
    addr = 0 if device_shift is None else 4 * device_shift
    wide = ilv and not pairs
    dual = (stereo_ok or pairs) and addr % (16 if wide else 8) == 0 and skew % (4 if wide else 2) == 0
    if dual and pairs and not on("VPZ_PAIRS") and (ilv or out_interleaved):
        dual = False
    if dual:
        return "pairs" if pairs else "stereo"
    if group_ok and (need_coupling or (out_interleaved and C > 2)) and skew % 4 == 0 and addr % 16 == 0:
        return "group"
    return "separate"


# ---- the inputs --------------------------------------------------------------------------------------------------------------

class Built:
    """A case's batch as stream_major_batch makes it (pk, res, posts, counts) with the packets' mappings set."""

    def __init__(self, c, skew=None):
        from synth_support import stream_major_batch
        self.case = c
        C = c["channels"]
        maps, floors = c["maps"], c["floors"]
        for m, mp in enumerate(maps):   # every mapping of a block size names the same floors: the posts are drawn per block size
            assert mp["channel_floor"] == maps[m & 1]["channel_floor"], (c["id"], m)
        per_size = tuple([floors[f] for f in maps[b]["channel_floor"]] for b in (0, 1))
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c["id"])) % 100000
        # the first seed from there on that gives streams 0 and 1 both block sizes in both calls (stream_major_batch's own draw)
        def switches(sd):
            for s in (0, 1):
                bf = helpers.markov_block_flags(c["frames"], seed=sd * 1000 + s, p_ls=0.15, p_sl=0.3, start_long=bool(s & 1)) & 1
                for part in (bf[:c["frames"] // 2], bf[c["frames"] // 2:]):
                    if part.all() or not part.any():
                        return False
            return True
        while not switches(seed):
            seed += 1
        self.skew = c["skew"] if skew is None else skew
        self.pk, self.res, self.posts, self.counts = stream_major_batch(
            c["n_streams"], c["frames"], C, seed=seed, floor=True, interleaved=c["interleaved"], p_ls=0.15, p_sl=0.3,
            silent_prob=0.1, channel_floors=per_size, skew=self.skew)
        for s in range(c["n_streams"]):   # the one silent record every stream has, whatever the draw (ExecuteChannel false)
            rec = (s * c["frames"] + 3) * C + (s + 1) % C
            self.counts[rec], self.posts[rec] = 0, 0
        is_long = (self.pk["flags"] & 1).astype(np.int64)
        if c["pick"] == "parity":
            self.pk["mapping"] = is_long
        else:
            # the k-th packet of a block size: the size's LAST mapping when k is even, the others from the top down when it is odd
            seen = [0, 0]
            for i in range(len(self.pk)):
                b = int(is_long[i])
                mine = list(range(b, len(maps), 2))[::-1]
                k = seen[b]
                seen[b] += 1
                self.pk["mapping"][i] = mine[0] if k % 2 == 0 else mine[(1 + k // 2) % len(mine)]

    def opk(self, stream, interleaved=None):
        """One stream's packets as helpers.oracle_decode takes them (interleaved: what the flags say about the residue's layout)."""
        c = self.case
        C, per = c["channels"], c["frames"]
        out = []
        for i in range(stream * per, (stream + 1) * per):
            fl = int(self.pk["flags"][i])
            if interleaved is not None:
                fl = (fl & ~helpers.PKT_INTERLEAVED) | (helpers.PKT_INTERLEAVED if interleaved else 0)
            half = 1024 if fl & 1 else 128
            off = int(self.pk["residue_offset"][i])
            out.append({"flags": fl, "granule": -1, "mapping": int(self.pk["mapping"][i]), "residue": self.res[off: off + C * half],
                        "posts": self.posts[i * C:(i + 1) * C], "post_count": self.counts[i * C:(i + 1) * C]})
        return out

    def oracle(self, orc, stream, maps=None, interleaved=None):
        c = self.case
        return helpers.oracle_decode(orc, c["channels"], 256, 2048, self.opk(stream, interleaved), floors=c["floors"],
                                     mappings=c["maps"] if maps is None else maps)[0]


TRUTH_STREAM = 1   # (not the first: the stream stride of the saved state and of the output matters)


@functools.lru_cache(maxsize=None)
def built(case_id, skew=None):
    """The case's inputs and the oracle's PCM of stream TRUTH_STREAM, computed once per process and shared (read-only)."""
    import oracle as orc
    b = Built(BY_ID[case_id], skew)
    ref = b.oracle(orc, TRUTH_STREAM)
    ref.setflags(write=False)
    return b, ref
