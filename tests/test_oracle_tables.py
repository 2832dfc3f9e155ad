"""Checks the oracle's constant tables against the reference's source text.  tests/golden/reference_constants.npz holds
the literals of that text as float32 (inverse_dB_table of Floor1.cs, LowerClip / UpperClip of Utils.cs), parsed out of
it by `tools/make_golden_fixtures.py --reference`; reading the reference as text is study, not execution."""
import ctypes as C
import os

import numpy as np

REF = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_constants.npz"))


def test_inverse_db_table_matches_reference_literals(oracle):
    vals = REF["inverse_db_table"]
    assert vals.dtype == np.float32 and vals.shape == (256,)
    assert np.array_equal(vals.view(np.uint32), oracle.inverse_db_table().view(np.uint32))


def test_clip_constants_match_reference(oracle):
    lower, upper = REF["clip"]
    assert lower == np.float32(-0.99999994) and upper == np.float32(0.99999994)
    # ... and they are where the oracle clips
    clipped = C.c_int(0)
    for x, want in ((2.0, upper), (-2.0, lower), (0.5, np.float32(0.5))):
        got = np.float32(oracle.lib().orc_clip_value(x, C.byref(clipped)))
        assert got.view(np.uint32) == want.view(np.uint32), (x, got, want)
    assert clipped.value == 1
