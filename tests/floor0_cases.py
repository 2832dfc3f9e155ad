"""The Floor0 kernels at the limits of order, bark map and grid: ONE case list, used by test_floor0_cases_cpu.py (are the inputs
fit to test with?  the oracle alone) and by test_floor0_limits_gpu.py (does the device compute them?).

Inputs the reference can carry.  Sorted uniform LSP frequencies (np.sort(rng.uniform(0.05, 3.0, order)), the rest of the suite)
break down at high order: two roots fall next to each other somewhere, floor0_safe_amp drops to 1e-5 ... 1e-13 and the oracle's
cosf / expf move away from the same float32 arithmetic on correctly rounded functions (1e-4 of the peak at order 254).  Here the
frequencies sit on an evenly spaced grid with jitter, theta_j = (j + 0.5) pi / order + u_j 0.3 pi / order, u_j uniform in [-1, 1]
(sorted, float32), and amp = floor0_safe_amp * U, U in [0.9, 1.0]: the curve peaks near 0 dB at every order.  Residues are small
integers, nonzero up to the last bin (bin n - 2 carries the largest bark index, bin n - 1 index 0: Floor0.cs:82-95), times a power
of two that puts the case's oracle PCM peak into [1, 100]: 1e-5 * max(1, |ref|max) is then a bar relative to the signal."""
import functools

import numpy as np

import helpers
from helpers import PKT_BLOCK_FLAG, PKT_NEXT_FLAG, PKT_PREV_FLAG

TOL = 1e-5          # the bar of test_floor0_matches_oracle: |got - ref|max <= TOL * max(1, |ref|max)
TEETH = 100.0       # a mutation of the inputs must move the oracle's PCM by this many bars
GRID_WAVES = 8192   # floor0_curve_kernel's persistent grid: kCurveGroupsMax * kCurveWaves wavefronts, one record each per round
RATE, AMP_BITS, AMP_OFS = 44100, 6, 100


def f0(order, bark):
    return {"order": order, "rate": RATE, "bark_map_size": bark, "amp_bits": AMP_BITS, "amp_ofs": AMP_OFS}


F1S, F1L = (helpers.SHORT_XLIST, 2), (helpers.LONG_XLIST, 2)
STEREO = [(0, 1)]


def _case(id, group, floors, maps, stride, sizes=(256, 2048), channels=2, calls=(7, 5), coupling=None, seed=0, long_rule=None,
          silent=None, windows=None):
    """floors: type-0 dicts and type-1 (x list, multiplier) pairs; maps: channel_floor of mapping 0 (short blocks) and, where the
    block sizes differ, of mapping 1 (long blocks); calls: packets per synth call; silent: {(packet, channel): amp} beyond the
    one amp = 0 record every case has; windows: {mutation: (first packet, last + 1)} to run C2 on a part of a large case."""
    if coupling is None:
        coupling = [STEREO if channels == 2 else []] * len(maps)
    return dict(id=id, group=group, floors=floors, maps=maps, stride=stride, size0=sizes[0], size1=sizes[1], channels=channels,
                calls=tuple(calls), coupling=coupling, seed=seed, long_rule=long_rule, silent=silent or {}, windows=windows or {})


def _order_cases():
    # A: 256 / 2048, bark 64 (the oracle holds for short blocks: bark_map_size <= blocksize / 2); every order % 4 class below and
    # above the 64-coefficient prefetch; strides equal to the order, order + 1, 64, 256
    strides = {1: 1, 2: 3, 3: 64, 4: 256, 5: 5, 7: 8, 63: 64, 64: 64, 65: 66, 66: 256, 67: 67, 128: 129, 254: 256, 255: 255}
    out = [_case("A-order%d-stride%d" % (o, s), "A", [f0(o, 64)], [[0, 0], [0, 0]], s) for o, s in strides.items()]
    # two type-0 floors swapped between the channels by block size: a short-order record follows a long-order one in a wave's row
    out.append(_case("A-orders65+7-swapped", "A", [f0(65, 64), f0(7, 64)], [[0, 1], [1, 0]], 65))
    # silence by sign: amp = -0.0 and amp = -1.0 give zeros like amp = 0 (the kernels' a <= 0 / a > 0, the oracle's amp <= 0); the
    # records keep post_count 1, so the kernels' own test of the amplitude is what silences them
    out.append(_case("A-order16-silent-by-sign", "A", [f0(16, 64)], [[0, 0], [0, 0]], 16, silent={(5, 0): -0.0, (8, 1): -1.0}))
    return out


def _bark_cases():
    # B: 2048 / 2048 (the stereo fast path takes it, the oracle holds up to bark 1024); channel 0 order 16, channel 1 order 65
    return [_case("B-bark%d" % b, "B", [f0(16, b), f0(65, b)], [[0, 1]], 65 if b % 2 else 256, sizes=(2048, 2048))
            for b in (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 1023, 1024)]


def _separate_cases():
    # C: floor0_apply_kernel on the routes that have no fused twin
    return [
        _case("C-mono-order65", "C", [f0(65, 128)], [[0], [0]], 65, channels=1),
        _case("C-three-channels-floors010", "C", [f0(67, 100), F1S, F1L], [[0, 1, 0], [0, 2, 0]], 67, channels=3,
              coupling=[[(0, 1), (2, 1)], [(1, 0), (2, 1)]]),
        _case("C-4096-bark1025-order255", "C", [f0(255, 1025)], [[0, 0]], 255, sizes=(4096, 4096), calls=(5, 3)),
        _case("C-4096-bark2048-order255", "C", [f0(255, 2048)], [[0, 0]], 256, sizes=(4096, 4096), calls=(5, 3)),
        _case("C-128-4096-order7", "C", [f0(7, 64)], [[0, 0], [0, 0]], 7, sizes=(128, 4096), calls=(7, 5)),
    ]


def _grid_case():
    # D: 4200 stereo packets = 8400 records in one call: 208 wavefronts take a second record, r + 8192, with the prefetched header,
    # amplitude and coefficients of it.  One long frame in sixteen, and the pattern shifts by three after 4096 packets, so that
    # records r and r + 8192 differ in block size: type-1 records skipped, the floor changing inside a wave's sequence
    return [_case("D-8400-records", "D", [f0(65, 64), f0(7, 128), F1S], [[0, 2], [1, 0]], 65, calls=(4200, 8),
                  long_rule=lambda p: (p + 3 * (p // 4096)) % 16 == 0,
                  silent={(5, 0): 0.0, (4176, 0): 0.0, (16, 1): 0.0, (4109 + 16 * 3, 1): 0.0},
                  windows={"a": (0, 128), "b": (0, 128), "c": (0, 128), "d": (4096, 4200)})]


CASES = _order_cases() + _bark_cases() + _separate_cases() + _grid_case()
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]


def fast_path(c):
    """Does the stereo fast path take the setup (floor0_curve_kernel + floor0_multiply_x2 instead of floor0_apply_kernel)?"""
    plain = (256, 2048)
    return (c["channels"] == 2 and c["size0"] in plain and c["size1"] in plain and
            all(f["bark_map_size"] <= 1024 for f in c["floors"] if isinstance(f, dict)))


def route(c, fused):
    """The route of the case's synth calls as VPZ_HOST_PROFILE=1 names it: the stereo fast path (floor0_curve_kernel + the lookup in
    the pass), or floor0_apply_kernel on the planar temp in front of the one-channel, the big or the any-size kernels."""
    if fused and fast_path(c):
        return "stereo"
    if c["size1"] >= 4096:
        return "big" if c["size0"] >= 256 else "generic"
    return "separate"


def lsp_frequencies(rng, order):
    j = np.arange(order)
    theta = (j + 0.5) * np.pi / order + rng.uniform(-1.0, 1.0, order) * 0.3 * np.pi / order
    return np.sort(theta).astype(np.float32)


class Built:
    """A case's inputs: floors / mappings as Decoder and oracle_decode take them, the packets as oracle dicts (opk) and as the
    ABI's arrays (flags, mapping, residue_offset; res, posts, counts, amps, coeffs [records, stride])."""

    def __init__(self, c, scale=1.0):
        self.case, self.scale = c, scale
        C_, h = c["channels"], (c["size0"] // 2, c["size1"] // 2)
        rng = np.random.default_rng([c["seed"], len(c["id"])] + [ord(ch) for ch in c["id"]])
        n = sum(c["calls"])
        two_sizes = c["size0"] != c["size1"]
        if not two_sizes:
            bf = np.zeros(n, dtype=np.uint8)
        elif c["long_rule"] is not None:
            bf = np.array([1 if c["long_rule"](p) else 0 for p in range(n)], dtype=np.uint8)
        else:
            bf = (rng.random(n) < 0.5).astype(np.uint8)
            bf[:4] = (1, 0, 0, 1)  # (both block sizes, whatever the seed)
        prev, nxt = np.concatenate([[1], bf[:-1]]), np.concatenate([bf[1:], [1]])
        self.flags = (bf * PKT_BLOCK_FLAG | prev * PKT_PREV_FLAG * bf | nxt * PKT_NEXT_FLAG * bf).astype(np.uint8)
        self.mapping = bf.astype(np.int32) if two_sizes else np.zeros(n, dtype=np.int32)
        self.floors = list(c["floors"])
        self.mappings = [{"coupling": list(c["coupling"][m]), "channel_floor": list(cf)} for m, cf in enumerate(c["maps"])]
        stride = c["stride"]
        self.amps = np.zeros(n * C_, dtype=np.float32)
        self.coeffs = np.zeros((n * C_, stride), dtype=np.float32)
        self.posts = np.zeros((n * C_, 64), dtype=np.int16)
        self.counts = np.zeros(n * C_, dtype=np.uint8)
        self.rec_floor = np.zeros(n * C_, dtype=np.int32)
        silent = dict(c["silent"])
        first0 = [ch for ch in range(C_) if isinstance(self.floors[c["maps"][int(self.mapping[3])][ch]], dict)][0]
        silent.setdefault((3, first0), 0.0)  # the one silent type-0 record every case has
        res, offs, off = [], np.zeros(n, dtype=np.int64), 0
        for p in range(n):
            half = h[int(bf[p])]
            r = np.round(rng.standard_normal((C_, half)) * 3.0)
            tail = r[:, -4:]
            tail[tail == 0] = 2.0  # nonzero up to the last bin: the highest bark indices are looked at
            res.append((r * scale).astype(np.float32).reshape(-1))
            offs[p] = off
            off += C_ * half
            for ch in range(C_):
                rec = p * C_ + ch
                fi = c["maps"][int(self.mapping[p])][ch]
                fl = self.floors[fi]
                self.rec_floor[rec] = fi
                if not isinstance(fl, dict):
                    posts, counts = helpers.random_posts(rng, fl[0], fl[1], 1)
                    self.posts[rec], self.counts[rec] = posts[0], counts[0]
                    continue
                co = lsp_frequencies(rng, fl["order"])
                self.coeffs[rec, :fl["order"]] = co
                amp = helpers.floor0_safe_amp(co, fl["bark_map_size"], float(fl["amp_ofs"])) * rng.uniform(0.9, 1.0)
                if (p, ch) in silent:
                    amp = silent[(p, ch)]
                self.amps[rec] = amp
                # (post_count = Amp != 0 is the caller's word; the records silenced by sign keep 1: the kernels test the amplitude)
                self.counts[rec] = 0 if (amp == 0 and not np.signbit(amp)) else 1
        self.res, self.residue_offset, self.n, self.half = np.concatenate(res), offs, n, h
        self.bounds = np.concatenate([[0], np.cumsum(c["calls"])]).astype(int)

    def opk(self, amps=None, coeffs=None, first=0, last=None):
        """The packets [first, last) as helpers.oracle_decode takes them, with other Floor0 data where a mutation asks for it."""
        C_ = self.case["channels"]
        amps = self.amps if amps is None else amps
        coeffs = self.coeffs if coeffs is None else coeffs
        last = self.n if last is None else last
        out = []
        for p in range(first, last):
            half = self.half[int(self.flags[p]) & 1]
            a = int(self.residue_offset[p])
            out.append({"flags": int(self.flags[p]), "mapping": int(self.mapping[p]), "granule": -1, "residue": self.res[a:a + C_ * half],
                        "posts": self.posts[p * C_:(p + 1) * C_], "post_count": self.counts[p * C_:(p + 1) * C_],
                        "f0_amp": amps[p * C_:(p + 1) * C_], "f0_coeff": coeffs[p * C_:(p + 1) * C_]})
        return out

    def oracle(self, orc, floors=None, **kw):
        c = self.case
        return helpers.oracle_decode(orc, c["channels"], c["size0"], c["size1"], self.opk(**kw),
                                     floors=self.floors if floors is None else floors, mappings=self.mappings)[0]

    # ---- C2: mutations of the INPUTS, each what a wrong index in the kernels would amount to
    def type0(self):
        return [i for i, f in enumerate(self.floors) if isinstance(f, dict)]

    def mutations(self):
        """{name: (keyword arguments for oracle(), window)} for the mutations that apply to this case."""
        c, out = self.case, {}
        orders = [self.floors[i]["order"] for i in self.type0()]
        win = lambda k: dict(zip(("first", "last"), c["windows"].get(k, (0, self.n))))
        rec_order = np.array([self.floors[f]["order"] if isinstance(self.floors[f], dict) else 0 for f in self.rec_floor])
        if max(orders) > 64:  # (a) the late coefficients, j >= 64, read from where the prefetched ones are
            co = self.coeffs.copy()
            co[:, 64:] = self.coeffs[:, :self.coeffs.shape[1] - 64]
            out["a"] = dict(coeffs=co, **win("a"))
        if max(orders) >= 2:  # (b) the last coefficient replaced by the one before it
            co = self.coeffs.copy()
            rows = np.nonzero(rec_order >= 2)[0]
            co[rows, rec_order[rows] - 1] = self.coeffs[rows, rec_order[rows] - 2]
            out["b"] = dict(coeffs=co, **win("b"))
        if len(self.type0()) == 2:  # (c) a record decoded with the other type-0 floor's configuration
            i, j = self.type0()
            fl = list(self.floors)
            fl[i], fl[j] = dict(self.floors[j]), dict(self.floors[i])
            out["c"] = dict(floors=fl, **win("c"))
        if self.bounds[1] * c["channels"] > GRID_WAVES:  # (d) record r with the amplitude and coefficients of record r - 8192
            am, co = self.amps.copy(), self.coeffs.copy()
            n1 = self.bounds[1] * c["channels"]
            am[GRID_WAVES:n1], co[GRID_WAVES:n1] = self.amps[:n1 - GRID_WAVES], self.coeffs[:n1 - GRID_WAVES]
            out["d"] = dict(amps=am, coeffs=co, **win("d"))
        return out


@functools.lru_cache(maxsize=None)
def built(case_id):
    """The case's inputs and its oracle PCM, computed once per process and shared (treat both as read-only)."""
    import oracle as orc
    c = BY_ID[case_id]
    b = Built(c)
    peak = float(np.abs(b.oracle(orc)).max())
    if np.isfinite(peak) and peak > 0:  # a power of two (exact in float32) that puts the peak at 8 ... 16
        b = Built(c, scale=2.0 ** (3 - int(np.floor(np.log2(peak)))))
    ref = b.oracle(orc)
    ref.setflags(write=False)
    return b, ref
