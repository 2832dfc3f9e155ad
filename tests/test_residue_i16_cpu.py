"""ABI v5, host side: the residue as 16-bit integers (vpzh_residue_is_integral / vpzh_decode_range_i16, vorbispizza_front.h).  A residue
value is a sum of codebook values (Residue0.cs:144-205); libvorbis' residue books are integer lattices, so for the reference's
fixtures every value is an integer and the int16 form is the float32 one, value for value."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", ["1test.ogg", "2test.ogg", "3test.ogg", "issue6test.ogg"])
def test_the_fixtures_residues_are_integers_and_the_int16_form_is_the_float_one(name):
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(os.path.join(GOLDEN, name))
    assert f.residue_is_integral
    pk, res, posts, counts = f.decode_packets()
    pk16, res16, posts16, counts16 = f.decode_packets(int16=True)
    assert res16.dtype == np.int16 and res.dtype == np.float32
    assert np.array_equal(res16.astype(np.float32), res)
    assert np.array_equal(pk, pk16) and np.array_equal(posts, posts16) and np.array_equal(counts, counts16)


def test_a_stream_with_fractional_codebook_values_is_not_integral_and_is_refused():
    import __graft_entry__ as ge
    ge.build()
    import synthetic_streams as ss
    from vorbispizza_amd.front import FrontError, OggVorbisFile
    seen = {True: 0, False: 0}
    for name in ("stereo_coupled_res2", "mono_floor1_res1", "six_channels_51"):
        stream, rng = ss.ALL[name]()
        ogg, _ = stream.build(rng, 8)
        f = OggVorbisFile(bytes(ogg))
        pk, res, _, _ = f.decode_packets()
        integral_values = bool(np.array_equal(res, np.round(res)) and np.abs(res).max(initial=0) < 32768)
        seen[f.residue_is_integral] += 1
        if f.residue_is_integral:
            assert integral_values  # (the setup header's word holds for what was decoded)
            assert np.array_equal(f.decode_packets(int16=True)[1].astype(np.float32), res)
        else:
            with pytest.raises(FrontError):
                f.decode_packets(int16=True)
    assert seen[False] > 0, "the spec-based writer's books are random floats: at least one stream must come out non-integral"


# ---- residues that accumulate across the submaps of a mapping.  decode_packet keeps the reference's quirk (Mapping.cs:132-163): one
# decode buffer for every submap, never cleared, so a type-0/1 submap adds to what earlier submaps left in row k and a type-2 submap
# overwrites the rows it covers.  A bound per residue is not a bound on the sum: (16, 8000) below passed it and wrapped 155 int16 values.
def _accumulating_cases():
    import edge_streams as es
    cases = {"%d_submaps_m%d" % nm: (dict(mux=list(range(nm[0])), m=nm[1]), es.TABLE_INTEGRAL[nm]) for nm in es.TABLE}
    cases.update(es.SHAPES)
    return cases


_BUILT = {}


def _accumulating(name):
    """(open stream, float decode, the writer's expectation) of a case, built once"""
    if name not in _BUILT:
        import __graft_entry__ as ge
        ge.build()
        import edge_streams as es
        from vorbispizza_amd.front import OggVorbisFile
        raw, exps, _ = es.accumulating_stream(**_accumulating_cases()[name][0])
        f = OggVorbisFile(raw)
        assert f.audio_packets == 30 and not (f.decode_packets()[0]["flags"] & 16).any()
        _BUILT[name] = (f, f.decode_packets()[1], es.expected_residue(exps))
    return _BUILT[name]


ACCUMULATING = sorted(_accumulating_cases())


@pytest.mark.parametrize("name", ACCUMULATING)
def test_the_int16_decode_of_accumulating_submaps_is_the_float_decode_or_is_refused(name):
    """The float decode is the writer's expectation; where the front end says integral the int16 decode is the float one value for
    value, and where it does not decode_packets(int16=True) refuses.  The answer itself is the rule as built
    (edge_streams.EXPECT_WHY): sixteen submaps of +-8000 are not integral."""
    from vorbispizza_amd.front import FrontError
    f, res, expected = _accumulating(name)
    assert res.tobytes() == expected.tobytes()
    want = _accumulating_cases()[name][1]
    assert want is None or f.residue_is_integral == want
    if f.residue_is_integral:
        res16 = f.decode_packets(int16=True)[1]
        assert res16.dtype == np.int16 and np.array_equal(res16.astype(np.float32), res)
    else:
        with pytest.raises(FrontError):
            f.decode_packets(int16=True)


@pytest.mark.parametrize("name", ACCUMULATING)
def test_an_integral_stream_s_expected_residue_fits_int16(name):
    """independent of the front end's rule: what the WRITER's model of the decode (vorbis_writer.Stream.audio_packet) expects of
    30 packets stays inside int16 whenever the front end says integral"""
    f, _, expected = _accumulating(name)
    peak = float(np.abs(expected).max())
    print(name, "integral", f.residue_is_integral, "largest |expected residue|", peak)
    if f.residue_is_integral:
        assert peak < 32768 and np.array_equal(expected, np.round(expected))


def test_the_accumulating_cases_do_leave_int16():
    """... and the cases are not vacuous: the sums of the non-integral ones of these do leave the int16 range"""
    for name in ("16_submaps_m8000", "type0_x16_m4000", "mixed_sizes_m16000", "mixed_sizes_x16_m8000", "type2_then_four_m16000"):
        assert float(np.abs(_accumulating(name)[2]).max()) >= 32768, name


# the answers of the parent of the accumulation rule (a bound per residue only): the new rule may be conservative for mappings of
# several submaps, but it must not change any of these
INTEGRAL_BEFORE = {
    "1test.ogg": True, "2test.ogg": True, "3test.ogg": True, "issue6test.ogg": True,
    "mono_floor1_res1": False, "stereo_coupled_res2": False, "three_channels_two_submaps": False, "stereo_floor0": False,
    "six_channels_51": False, "four_channels_quad": False, "three_channels_chained": False, "five_channels": False,
    "ten_channels": False,
    "crafted:eight_channels_coupled_in_a_ring": False, "crafted:floor1_64_posts_multiplier_4": False,
    "crafted:floor1_x_lists_at_the_ends": False, "crafted:forty_channels_sixteen_submaps": False,
    "crafted:residue_ranges_beyond_the_block": False, "crafted:twelve_modes_twenty_four_floors": False,
}


def test_the_listed_streams_keep_their_answer():
    import __graft_entry__ as ge
    ge.build()
    import hostile_setups as hs
    import synthetic_streams as ss
    from vorbispizza_amd.front import OggVorbisFile
    got = {name: OggVorbisFile(os.path.join(GOLDEN, name)).residue_is_integral for name in INTEGRAL_BEFORE if name.endswith(".ogg")}
    for name, make in ss.ALL.items():
        stream, rng = make()
        got[name] = OggVorbisFile(bytes(stream.build(rng, 8)[0])).residue_is_integral
    for name, (raw, expect) in hs.crafted().items():
        if expect == "pcm":
            got["crafted:" + name] = OggVorbisFile(raw).residue_is_integral
    assert got == INTEGRAL_BEFORE


def test_one_submap_and_all_type_2_mappings_answer_as_the_residue_alone():
    """the accumulation rule does not reach a mapping of one submap, and type-2 submaps overwrite: four type-2 submaps of +-8000
    (2 * entry_l1 = 32000 per residue, the most the per-residue bound lets through) are integral like one, and so is one type-1 submap
    of five channels"""
    import __graft_entry__ as ge
    ge.build()
    import edge_streams as es
    from vorbispizza_amd.front import OggVorbisFile
    for kw in (dict(mux=[0, 1, 2, 3], m=8000, types=[2, 2, 2, 2]), dict(mux=[0, 0, 1, 1, 1], m=8000, types=[2, 2]),
               dict(mux=[0] * 5, m=8000), dict(mux=[0], m=8191)):
        raw, exps, _ = es.accumulating_stream(packets=10, **kw)
        f = OggVorbisFile(raw)
        assert f.residue_is_integral, kw
        res = f.decode_packets()[1]
        assert res.tobytes() == es.expected_residue(exps).tobytes()
        assert np.array_equal(f.decode_packets(int16=True)[1].astype(np.float32), res)
    raw, _, _ = es.accumulating_stream(mux=[0], m=8192, packets=2)
    assert not OggVorbisFile(raw).residue_is_integral  # (2 * entry_l1 = 32768: the per-residue bound, unchanged)
