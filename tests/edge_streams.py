"""Streams of the specification-based writer (tests/vorbis_writer.py) at edges that neither the fixtures nor
tests/synthetic_streams.py reach: residues that ACCUMULATE across the submaps of a mapping (the reference reuses one decode
buffer for every submap without clearing it, Mapping.cs:132-163), mappings of 65 / 130 / 255 channels, codes of 31 and 32
bits, and small streams with not-decoded packets to tile into very large batches.  Shared by tests/test_residue_i16_cpu.py,
tests/test_residue_i16_gpu.py and tests/test_entropy_edges_gpu.py."""
import numpy as np

import vorbis_writer as vw
from hostile_setups import _floor1_with_posts, _plain_residue


# ---------------------------------------------------------------------------------- accumulating submaps
def value_book(m, dims=2):
    """an integer lattice {-m, 0, +m}: nine entries of two dimensions, or three entries of one"""
    kw = dict(minv=vw.float32_pack(m, 788, negative=True), delta=vw.float32_pack(m, 788), value_bits=2, mults=[0, 1, 2])
    if dims == 2:
        return vw.Codebook(2, [4] * 8 + [1], 1, **kw)
    return vw.Codebook(1, [2, 2, 1], 1, **kw)


def accumulating_stream(mux, m, types=None, dims=2, seed=5, packets=30):
    """Block sizes 64/64, one mode, one mapping of len(mux) channels whose submap s holds the channels with mux == s.  Every
    submap uses the same floor and a residue over bins 0..32 (partition size 4, two classes, cascade [0, 1]) whose one value
    book is value_book(m, dims); types[s] is the residue type of submap s (default: all type 1).  A type-2 residue covers its
    submap's interleaved vector.  Returns (container bytes, the writer's expectations, the Stream)."""
    channels, submaps = len(mux), max(mux) + 1
    types = [1] * submaps if types is None else list(types)
    assert len(types) == submaps and sorted(set(mux)) == list(range(submaps))
    rng = np.random.default_rng(seed)
    books = []
    floor = _floor1_with_posts(rng, books, 32, 6, 1)
    books.append(value_book(m, dims))
    books.append(vw.Codebook(1, [1, 1]))
    vb, cb = len(books) - 2, len(books) - 1
    residues, index, sub_res = [], {}, []
    for s in range(submaps):
        members = sum(1 for c in mux if c == s)
        key = (types[s], members if types[s] == 2 else 1)
        if key not in index:
            index[key] = len(residues)
            residues.append(vw.Residue(types[s], 0, 32 * key[1], 4, cb, [0, 1], [[None] * 8, [vb] + [None] * 7]))
        sub_res.append(index[key])
    maps = [vw.Mapping(channels, [], list(mux), [0] * submaps, sub_res)]
    st = vw.Stream(channels, 44100, 6, 6, books, [floor], residues, maps, [(0, 0)])
    ogg, exps = st.build(rng, packets)
    return bytes(ogg), exps, st


# (N one-channel submaps, M): the table of the bug report -- what the per-residue rule said, and the largest |sum| a decode met
TABLE = [(2, 8000), (3, 8000), (5, 8000), (16, 8000), (16, 1000)]

# name -> (keyword arguments of accumulating_stream, is the stream integral by the rule as built -- see EXPECT_WHY)
SHAPES = {
    # type 0 sums an entry's dimensions into ONE bin: a vector adds up to entry_l1 = 2 m there
    "type0_x16_m4000": (dict(mux=list(range(16)), m=4000, types=[0] * 16), False),
    "type0_x16_m250": (dict(mux=list(range(16)), m=250, types=[0] * 16), True),
    # submaps of 3, 2 and 1 channels: row 0 takes three residues, row 1 two, row 2 one
    "mixed_sizes_m16000": (dict(mux=[0, 0, 0, 1, 1, 2], m=16000, dims=1), False),
    "mixed_sizes_m2700": (dict(mux=[0, 0, 0, 1, 1, 2], m=2700, dims=1), True),
    # sixteen submaps of which the first four have two channels: row 0 takes sixteen residues, row 1 four
    "mixed_sizes_x16_m8000": (dict(mux=list(range(16)) + [0, 1, 2, 3], m=8000), False),
    # a type-2 submap overwrites the rows it covers: 1, 1, [2], 1 is two sums of two, not one of four
    "type2_resets_m10000": (dict(mux=[0, 1, 2, 3], m=10000, types=[1, 1, 2, 1], dims=1), True),
    "type2_then_four_m16000": (dict(mux=[0, 1, 2, 3, 4], m=16000, types=[1, 2, 1, 1, 1], dims=1), False),
}
EXPECT_WHY = """one decode of these residues (one stage) adds to a bin at most A = m for type 1 / 2 and A = entry_l1 = 2 m for type 0 with
the two-dimensional book; a row's bound is the sum of A over the type-0/1 submaps that reach it since the last type-2 submap
that covers it, and the stream is integral when every row stays below 32768 (and every residue alone passes
2 * entry_l1 * stages < 32768, which all of these do)"""
# ... and for TABLE: 2 * 8000 and 3 * 8000 stay below 32768, 5 * 8000 and 16 * 8000 do not, 16 * 1000 does
# (None: either answer is sound -- five sums of 8000 could reach 40000 in principle; 30 packets get to 32000)
TABLE_INTEGRAL = {(2, 8000): True, (3, 8000): True, (5, 8000): None, (16, 8000): False, (16, 1000): True}


def expected_residue(exps):
    """the writer's expectation of decode_packets()[1] for an all-decoded stream: planar [channel][half] per packet"""
    return np.concatenate([e["residue"].reshape(-1) for e in exps]).astype(np.float32)


# ---------------------------------------------------------------------------------- many channels
def many_channels(channels, seed=0, packets=12):
    """64/64, three submaps (mux c % 3) with residue types 1, 0 and 2 (the type-2 residue over its members' interleaved
    vector), floors 0, 1, 0, and coupling steps that straddle every 64-channel boundary.  Returns (bytes, expectations)."""
    rng = np.random.default_rng(7000 + channels + seed)
    books = []
    floors = [_floor1_with_posts(rng, books, 32, 6, 1), _floor1_with_posts(rng, books, 32, 11, 3)]
    mux = [c % 3 for c in range(channels)]
    members2 = sum(1 for c in mux if c == 2)
    residues = [_plain_residue(rng, books, 1, 0, 32, 4), _plain_residue(rng, books, 0, 0, 32, 4),
                _plain_residue(rng, books, 2, 0, 32 * members2, 4)]
    coupling = [(c, c + 1) for c in (0, 62, 63, 64, 126, 127, 128, 190, 191, 192, channels - 2) if 0 <= c and c + 1 < channels]
    coupling = sorted(set(coupling))
    maps = [vw.Mapping(channels, coupling, mux, [0, 1, 0], [0, 1, 2])]
    st = vw.Stream(channels, 44100, 6, 6, books, floors, residues, maps, [(0, 0)])
    ogg, exps = st.build(rng, packets)
    return bytes(ogg), exps


# ---------------------------------------------------------------------------------- long codes
class AnyPostFloor1(vw.Floor1):
    """vw.Floor1 whose packets draw a post from EVERY entry of a subclass book (vw.Floor1 keeps to the first six so that
    the curve stays in range; here only the entropy decode is looked at)"""

    def write_packet(self, bw, books, rng, silent):
        if silent:
            bw.write(0, 1)
            return 0, []
        bw.write(1, 1)
        rng_range = self.RANGES[self.multiplier - 1]
        ybits = vw.ilog(rng_range - 1)
        posts = [int(rng.integers(rng_range)), int(rng.integers(rng_range))]
        bw.write(posts[0], ybits)
        bw.write(posts[1], ybits)
        for cls in self.partition_class:
            assert self.class_subclasses[cls] == 0
            for _ in range(self.class_dims[cls]):
                book = books[self.subclass_books[cls][0]]
                e = int(rng.choice(book.used))
                book.write_entry(bw, e)
                posts.append(e)
        return len(posts), posts


def long_codes(longest, seed=0, packets=40):
    """mono 64/64.  The floor's subclass book is ordered with lengths 1 .. longest-1, longest, longest; the type-1 residue's
    value book (one dimension, the integers -16 ..) has those lengths permuted; its 32-entry class book has five dimensions
    and lengths 1..31, 31.  Every code longer than the 10-bit prefix table goes through the overflow list, and with
    longest == 32 the floor book's peek is the 32-bit one.  Returns (bytes, expectations)."""
    rng = np.random.default_rng(8000 + longest + seed)
    lengths = list(range(1, longest)) + [longest, longest]
    books = [vw.Codebook(1, lengths, ordered=True)]
    floor = AnyPostFloor1([0, 0], [3], [0], [0], [[0]], 2, 5, [int(v) for v in rng.choice(np.arange(1, 32), size=6, replace=False)])
    n = len(lengths)
    books.append(vw.Codebook(1, [int(v) for v in rng.permutation(lengths)], 1, minv=vw.float32_pack(16, 788, negative=True),
                             delta=vw.float32_pack(1, 788), value_bits=6, mults=list(range(n))))
    books.append(vw.Codebook(5, list(range(1, 32)) + [31]))
    residue = vw.Residue(1, 0, 32, 4, 2, [1, 1], [[1] + [None] * 7, [1] + [None] * 7])
    st = vw.Stream(1, 8000, 6, 6, books, [floor], [residue], [vw.Mapping(1, [], [0], [0], [0])], [(0, 0)])
    ogg, exps = st.build(rng, packets)
    return bytes(ogg), exps


# ---------------------------------------------------------------------------------- small streams to tile
def _integer_residue(books, rtype, end, partition_size):
    """two classes, the second with two stages of integer books (values -3 .. 4 in pairs, -1 .. 1 in fours)"""
    base = len(books)
    books.append(vw.Codebook(2, [4] * 16, 1, minv=vw.float32_pack(3, 788, negative=True), delta=vw.float32_pack(1, 788), value_bits=3,
                             mults=[0, 1, 2, 7]))
    books.append(vw.Codebook(4, [6] * 47 + [7] * 34, 1, minv=vw.float32_pack(1, 788, negative=True), delta=vw.float32_pack(1, 788),
                             value_bits=2, mults=[0, 1, 2]))
    books.append(vw.Codebook(2, [2, 2, 2, 2]))
    return vw.Residue(rtype, 0, end, partition_size, base + 2, [0, 3], [[None] * 8, [base, base + 1] + [None] * 6])


def with_header_edges(st, rng, packets):
    """a container of `packets` random audio packets of `st` of which five are replaced by the smallest packets at which
    the parse of a packet's first bits goes wrong (tests/test_entropy_plan_cpu.py, HEADER_EDGE): nothing to read, the type
    bit set, a header that ends inside the packet.  They come out as VPZ_PKT_NOT_DECODED records or as short decodes."""
    seq = [int(rng.integers(len(st.modes))) for _ in range(packets)]
    audio, total, grans = [], 0, [0, 0, 0]
    for i, mi in enumerate(seq):
        bf = st.modes[mi][0]
        prev = st.modes[seq[i - 1]][0] if i else 1
        nxt = st.modes[seq[i + 1]][0] if i + 1 < packets else 1
        audio.append(st.audio_packet(rng, mi, prev, nxt)[0])
        if i:
            total += ((st.bs1 if st.modes[seq[i - 1]][0] else st.bs0) + (st.bs1 if bf else st.bs0)) // 4
        grans.append(total)
    audio[3] = b""
    audio[4] = b"\x01"
    audio[5] = b"\x01\x02"
    audio[6] = audio[6][:1]
    audio[7] = audio[7][:3]
    return bytes(vw.ogg_mux(st.headers() + audio, grans, packets_per_page=2))


def tile_mono(seed=0, packets=17):
    """mono, 64/64, residue type 1, integer books"""
    rng = np.random.default_rng(9000 + seed)
    books = []
    floor = _floor1_with_posts(rng, books, 32, 7, 2)
    residue = _integer_residue(books, 1, 32, 8)
    st = vw.Stream(1, 8000, 6, 6, books, [floor], [residue], [vw.Mapping(1, [], [0], [0], [0])], [(0, 0)])
    return with_header_edges(st, rng, packets)


def tile_three_channels(seed=0, packets=13):
    """three channels in two submaps (mux 0, 0, 1: residue 1 on the pair, residue 2 on the third), 64/128, integer books"""
    rng = np.random.default_rng(9100 + seed)
    books = []
    floors = [_floor1_with_posts(rng, books, 32, 6, 1), _floor1_with_posts(rng, books, 64, 9, 2)]
    residues = [_integer_residue(books, 1, 32, 8), _integer_residue(books, 2, 32, 4),
                _integer_residue(books, 1, 64, 8), _integer_residue(books, 2, 64, 8)]
    maps = [vw.Mapping(3, [(0, 1)], [0, 0, 1], [0, 0], [0, 1]), vw.Mapping(3, [(2, 0)], [0, 0, 1], [1, 1], [2, 3])]
    st = vw.Stream(3, 8000, 6, 7, books, floors, residues, maps, [(0, 0), (1, 1)])
    return with_header_edges(st, rng, packets)
