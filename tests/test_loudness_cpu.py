"""vpz_loudness_filter, vpz_loudness_weights and vpz_loudness_gate (include/vorbispizza_pcm_loudness.h, csrc/pcm_loudness.hip) without a
device, every refusal of the host entry points, the known answers of EBU Tech 3341, and what a clean checkout must hold about the new
headers and bindings.

The truth is tests/loudness_truth.py: the header's definition restated in numpy.  The known-answer tests feed ITS float64 step sums -- the
chunked form, held here to the sequential one -- to the library's gate: the sequences are 20 to 100 seconds long and are not shortened
(shortened ones read -23.18 where the target is -23.0)."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loudness_truth as lt  # noqa: E402
import binding_support as cs  # noqa: E402
from binding_support import imports_of  # noqa: E402

KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


# ---- filter, steps, weights
def test_the_filter_at_48k_is_the_published_table(capi):
    c = capi.loudness_filter(48000)
    assert c.shape == (2, 5) and c.dtype == np.float64
    got = list(c[0]) + list(c[1, 3:])
    worst = max(abs(g - p) / abs(p) for g, p in zip(got, lt.PUBLISHED_48K))
    print("largest relative distance from BS.1770's table: %.3g" % worst)
    assert worst <= 1e-12
    assert list(c[1, :3]) == [1.0, -2.0, 1.0]  # (not normalised)


@pytest.mark.parametrize("fs", [8000, 11025, 16000, 22050, 44100, 48000, 96000, 192000, 384000, 12345])
def test_the_filter_of_a_rate_is_the_headers_formula(capi, fs):
    got, want = capi.loudness_filter(fs), lt.coefficients(fs)
    assert (np.abs(got - want) <= 4 * 2.0 ** -52 * np.abs(want)).all()
    assert 0.9 < lt.pole_radius(fs) < 1.0


def test_the_step_rule(capi):
    assert [capi.loudness_step(fs) for fs in (8000, 11025, 44100, 48000, 384000)] == [800, 1103, 4410, 4800, 38400]
    assert [lt.step_of(fs) for fs in (8000, 11025, 44100)] == [800, 1103, 4410]


def test_the_weight_table(capi):
    for channels in range(1, 9):
        assert list(capi.loudness_weights(channels)) == lt.WEIGHTS[channels], channels
    assert list(capi.loudness_weights(6)) == [1, 1, 1, 1.41, 1.41, 0]
    for channels in (9, 10, 255):
        assert list(capi.loudness_weights(channels)) == [1.0] * channels
    for channels in (0, -1, 256):
        with pytest.raises(ValueError):
            capi.loudness_weights(channels)
    assert capi.lib().vpz_loudness_weights(2, None) == capi.E_INVALID_ARG


def test_rates_outside_the_limits_are_refused(capi):
    assert (capi.LOUDNESS_MIN_RATE, capi.LOUDNESS_MAX_RATE) == (8000, 384000)
    for fs in (7999, 384001, 0, -48000):
        with pytest.raises(ValueError):
            capi.loudness_filter(fs)
    capi.loudness_filter(8000)
    capi.loudness_filter(384000)
    assert capi.lib().vpz_loudness_filter(48000, None) == capi.E_INVALID_ARG


# ---- the gate
def sums_at(level, S, steps):
    """step sums that put every block at `level` LUFS"""
    return np.full(steps, S * 10.0 ** ((level + 0.691) / 10.0))


def test_fewer_than_four_steps_give_minus_infinity(capi):
    for steps in (0, 1, 2, 3):
        assert capi.loudness_gate(sums_at(-20.0, 4800, steps), 4800) == (-np.inf, 0)
    lufs, kept = capi.loudness_gate(sums_at(-20.0, 4800, 4), 4800)
    assert kept == 1 and abs(lufs + 20.0) < 1e-12
    assert capi.loudness_gate(np.zeros(10), 4800) == (-np.inf, 0)  # (silence: nothing passes the absolute gate)


def test_the_gate_refuses_what_the_header_says(capi):
    L = capi.lib()
    sums = np.ones(8)
    lufs, kept = C.c_double(), C.c_int64()
    assert L.vpz_loudness_gate(sums.ctypes.data, 8, 4800, C.byref(lufs), C.byref(kept)) == capi.OK
    assert L.vpz_loudness_gate(sums.ctypes.data, 8, 4800, C.byref(lufs), None) == capi.OK  # (blocks_kept is optional)
    assert L.vpz_loudness_gate(sums.ctypes.data, 8, 4800, None, C.byref(kept)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_gate(None, 8, 4800, C.byref(lufs), C.byref(kept)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_gate(sums.ctypes.data, -1, 4800, C.byref(lufs), C.byref(kept)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_gate(sums.ctypes.data, 8, 0, C.byref(lufs), C.byref(kept)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_gate(None, 0, 4800, C.byref(lufs), C.byref(kept)) == capi.OK and lufs.value == -np.inf and kept.value == 0


def test_the_absolute_gate_alone_changes_the_answer(capi):
    """twenty steps at -65 LUFS, then twenty at -75: the relative threshold is -75 (ten below the mean of what passed, the -65 blocks), so
    without the absolute gate the blocks near -75 -- those ABOVE the -75 threshold because they overlap a louder step -- would count"""
    S = 4800
    sums = np.concatenate([sums_at(-65.0, S, 20), sums_at(-75.0, S, 20)])
    want, kept, threshold, levels = lt.gate(sums, S)
    lufs, blocks = capi.loudness_gate(sums, S)
    assert (lufs, blocks) == (want, kept)
    below_absolute = (levels <= -70.0) & (levels > threshold)
    assert below_absolute.any()  # blocks only the absolute gate removes
    p, _ = lt.block_levels(sums, S)
    without = -0.691 + 10.0 * np.log10(p[levels > threshold].mean())
    assert abs(without - lufs) > 0.05


def test_the_relative_gate_alone_changes_the_answer(capi):
    """-20 LUFS and -40 LUFS, both far above -70: the relative threshold, about -33, removes the quiet half (the three blocks across the
    change are partly loud: two of them stay, which is why the value is a little under -20)"""
    S = 800
    sums = np.concatenate([sums_at(-20.0, S, 30), sums_at(-40.0, S, 30)])
    want, kept, threshold, levels = lt.gate(sums, S)
    lufs, blocks = capi.loudness_gate(sums, S)
    assert (lufs, blocks) == (want, kept) and (levels > -70.0).all() and 0 < blocks < len(levels)
    p, _ = lt.block_levels(sums, S)
    ungated = -0.691 + 10.0 * np.log10(p.mean())
    assert lufs > ungated + 2.0 and abs(lufs + 20.0) < 0.5


def test_a_block_exactly_at_minus_70_is_not_kept(capi):
    """a power whose level evaluates to exactly -70.0 (found by stepping through the neighbouring doubles), and its upper neighbour"""
    S = 4096  # (a power of two: the step sums below are exact, and so is the block's power)
    level = lambda p: -0.691 + 10.0 * np.log10(p)  # noqa: E731
    p = 10.0 ** ((-70.0 + 0.691) / 10.0)
    for _ in range(1000):
        if level(p) == -70.0:
            break
        p = np.nextafter(p, np.inf if level(p) < -70.0 else -np.inf)
    assert level(p) == -70.0
    above = p
    while level(above) == -70.0:
        above = np.nextafter(above, np.inf)
    # four equal steps whose block power is exactly p: sums = p * S each
    for power, kept in ((p, 0), (above, 1)):
        s = power * S
        assert (s + s + s + s) / (4.0 * S) == power
        lufs, blocks = capi.loudness_gate([s, s, s, s], S)
        assert blocks == kept and (lufs == -np.inf) == (kept == 0)


# ---- the restatement, and the known answers
def test_the_chunked_restatement_is_the_sequential_one():
    """float64 by steps against numpy.longdouble sample by sample, inside the device tests' bound"""
    rng = np.random.default_rng(11)
    for fs in (8000, 11025):
        S = lt.step_of(fs)
        x = (0.5 + 0.1 * rng.standard_normal((9 * S + 77, 2)) + 0.2 * np.sin(2 * np.pi * 20.0 * np.arange(9 * S + 77) / fs)[:, None]).astype(np.float32)
        seq = lt.step_sums_sequential([x[:, 0], x[:, 1]], [fs, fs])
        chunked = lt.step_sums_chunked(x, fs)
        assert chunked.shape == (9, 2)
        for ch in range(2):
            truth = seq[ch].astype(np.float64)
            err = np.abs(chunked[:, ch] - seq[ch]).astype(np.float64)
            assert (err <= lt.bound(fs, truth)).all(), (fs, ch, float((err / lt.bound(fs, truth)).max()))


@pytest.mark.parametrize("fs", [48000, 8000])
@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_ebu_tech_3341(capi, case, fs):
    """a stereo 1 kHz sine at the stated per-channel peak levels, within 0.1 LU of the target"""
    parts, target = lt.EBU_3341[case]
    x = lt.sine(fs, parts)
    sums = lt.weighted(lt.step_sums_chunked(x, fs), lt.weights_of(2))
    lufs, kept = capi.loudness_gate(sums, lt.step_of(fs))
    print("EBU Tech 3341 case %d at %d Hz: %.3f LUFS (target %.1f), %d blocks" % (case, fs, lufs, target, kept))
    assert abs(lufs - target) <= 0.1
    assert (lufs, kept) == lt.gate(sums, lt.step_of(fs))[:2]


def test_a_full_scale_997_hz_mono_sine_reads_minus_3_01(capi):
    fs = 48000
    x = lt.sine(fs, [(20, 0.0)], hz=997.0, channels=1)
    sums = lt.weighted(lt.step_sums_chunked(x, fs), lt.weights_of(1))
    lufs, _ = capi.loudness_gate(sums, lt.step_of(fs))
    print("997 Hz, 0 dBFS, mono: %.4f LUFS" % lufs)
    assert abs(lufs + 3.01) <= 0.01


# ---- the surface
def test_the_loudness_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_loudness.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmLoudness.cs")
    names = ["vpz_loudness_filter", "vpz_loudness_gate", "vpz_loudness_weights", "vpz_pcm_loudness"]
    assert sorted(c) == names == sorted(imports) == sorted(capi.PCM_LOUDNESS_EXPORTED_SYMBOLS)
    # (`double coeffs[10]` is a pointer parameter: the header's parser reads an array declarator as its element)
    assert c["vpz_loudness_filter"] == ("i32", ["i32", "f64"]) and "double coeffs[10]" in open(os.path.join(cs.INC, "vorbispizza_pcm_loudness.h")).read()
    c["vpz_loudness_filter"] = ("i32", ["i32", "ptr"])
    assert c["vpz_loudness_weights"] == ("i32", ["i32", "ptr"])
    assert c["vpz_pcm_loudness"] == ("i32", ["ptr", "ptr", "i64", "i32", "i32", "ptr", "i32", "ptr", "ptr", "ptr", "i64", "i64"])
    assert c["vpz_loudness_gate"] == ("i32", ["ptr", "i64", "i32", "ptr", "ptr"])
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_LOUDNESS_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    structs, defines = cs.c_structs("vorbispizza_pcm_loudness.h")
    assert structs == {} and defines["VPZ_LOUDNESS_MIN_RATE"] == capi.LOUDNESS_MIN_RATE and defines["VPZ_LOUDNESS_MAX_RATE"] == capi.LOUDNESS_MAX_RATE
    text = cs.strip_cs_comments(open(os.path.join(cs.CS, "GpuPcmLoudness.cs")).read())
    assert "LoudnessMinRate = 8000" in text and "LoudnessMaxRate = 384000" in text
    # the older headers and their lists did not take the new names
    older = (capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_RESAMPLE_EXPORTED_SYMBOLS
             + capi.PCM_LOGMEL_EXPORTED_SYMBOLS + capi.PCM_FBANK_EXPORTED_SYMBOLS)
    for name in c:
        assert name not in older
        assert name not in cs.c_functions("vorbispizza_synth.h", "vpz_") and name not in cs.c_functions("vorbispizza_pcm_fbank.h", "vpz_")
    # what is out of scope is said where a caller reads it
    header = open(os.path.join(cs.INC, "vorbispizza_pcm_loudness.h")).read()
    for word in ("true peak", "loudness range", "short-term", "int16", "gain", "vpzr_"):
        assert word in header, word


def test_the_measure_call_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_loudness.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiLoudness.cs")
    assert sorted(c) == ["vpzm_measure_loudness"] == sorted(imports) == sorted(multi.LOUDNESS_EXPORTED_SYMBOLS)
    assert c["vpzm_measure_loudness"] == ("i32", ["ptr", "i32", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"])
    assert imports["vpzm_measure_loudness"] == ("Host",) + c["vpzm_measure_loudness"]
    fn = multi.lib().vpzm_measure_loudness
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_measure_loudness"][1] and KINDS[fn.restype] == "i32"
    structs, _ = cs.c_structs("vorbispizza_multi_loudness.h")
    cs_fields = cs.cs_structs(os.path.join(cs.CS, "VorbisPizzaMultiLoudness.cs"))["Loudness"]
    py_fields = [(n, {"<f8": "f64", "<i8": "i64"}[multi.LOUDNESS_DTYPE[n].str], 0) for n in multi.LOUDNESS_DTYPE.names]
    assert sorted(structs) == ["vpzm_loudness"] and len(structs["vpzm_loudness"]) == len(cs_fields) == len(py_fields) == 4
    for (n0, k0, a0), (n1, k1, a1), (n2, k2, a2) in zip(structs["vpzm_loudness"], cs_fields, py_fields):
        assert cs.norm(n0) == cs.norm(n1) == cs.norm(n2) and k0 == k1 == k2 and a0 == a1 == a2 == 0, (n0, n1, n2)
    assert multi.LOUDNESS_DTYPE.itemsize == 32
    sig = inspect.signature(multi.Dispatcher.measure_loudness)
    assert list(sig.parameters) == ["self", "datas", "ranges"] and sig.parameters["ranges"].default is None


def test_both_libraries_export_the_new_symbols(capi):
    from vorbispizza_amd import _build, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in capi.PCM_LOUDNESS_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert hasattr(H, "vpzm_measure_loudness") and not hasattr(S, "vpzm_measure_loudness")
    assert "pcm_loudness.hip" in _build.SOURCES
    sig = inspect.signature(capi.pcm_loudness)
    assert list(sig.parameters)[:7] == ["ctx", "src", "channels", "sample_rate", "rows", "weights", "max_steps"]
    assert callable(capi.loudness_filter) and callable(capi.loudness_weights) and callable(capi.loudness_gate) and callable(multi.Dispatcher.measure_loudness)


# ---- the launch plan of vpz_pcm_loudness, and the cases of tests/test_pcm_loudness_limits_gpu.py
def test_the_launch_plan_at_every_channel_count():
    """G, the LDS pitch and its bytes as csrc/pcm_loudness.hip computes them, at 1..255 channels; and the comment's bank claim: lane
    (s, c) reads lds[s * stride + t * C + c], and the live lanes of every aligned group of 32 fall on 32 different banks at every t"""
    k = lt.kernel_constants(ROOT)
    assert (k["kLoudBlock"], k["kChunk"], k["kLoudMaxGridY"]) == (256, 32, 4096)
    most = {}
    for channels in range(1, 256):
        G, stride, lds_bytes = lt.launch_plan(channels, k)
        assert stride >= 32 * channels and stride - 32 * channels < 32 and stride % 32 == channels % 32 and G >= 1, channels
        assert G == 256 // channels and lds_bytes == 4 * G * stride <= 34 * 1024, channels
        most[channels] = lds_bytes
        lane = np.arange(256)
        s, c = lane // channels, lane % channels
        for t in (0, 1, 31):
            bank = (s * stride + t * channels + c) % 32
            for first in range(0, 256, 32):
                live = bank[first: first + 32][s[first: first + 32] < G]
                assert len(set(live.tolist())) == len(live), (channels, t, first)
    assert max(most.values()) == most[16] == 33792
    assert lt.launch_plan(32, k)[1] == 32 * 32 and lt.launch_plan(33, k)[1] == 32 * 33 + 1  # (no padding; one float of it)
    assert lt.launch_plan(129, k)[0] == 1 and lt.launch_plan(128, k)[0] == 2


def test_every_limit_case_is_the_shape_it_is_named_for():
    """Case's constructor has held every channel of every row to a crest factor of 4 (building the list is that check); here each case's
    G, idle lanes, step modulo 32 and, row by row, units, steps, the workgroups of (a) and (c) and the tail, against the numbers
    loudness_cases.EXPECT writes down"""
    import loudness_cases as lc
    k = lt.kernel_constants(ROOT)
    cases = lc.cases()
    assert set(lc.EXPECT) | {"grid", "grid_checked", "crowd"} == set(cases)
    assert {"channels_%d" % c for c in lc.CHANNEL_COUNTS} <= set(lc.EXPECT) and lc.CHANNEL_COUNTS == (4, 5, 7, 9, 31, 32, 33, 64, 85, 86, 128, 129, 255)
    for name, (G, idle, s32, rows) in lc.EXPECT.items():
        case = cases[name]
        assert lt.launch_plan(case.channels, k)[0] == G and 256 - G * case.channels == idle and lt.step_of(case.fs) % 32 == s32, name
        assert [lt.tiles_of(r.shape[0], case.fs, case.channels, k) for r in case.rows] == rows, name
        if case.weights is None and case.channels > 8:
            assert (case.w == 1.0).all()
    # the lengths the cases are named for
    S = lc.S
    assert [r.shape[0] for r in cases["edges_8"].rows] == [32 * S, 32 * S + 1, 31 * S + 799, 33 * S, 64 * S + 31]
    assert [r.shape[0] for r in cases["edges_3"].rows] == [85 * S, 85 * S + 1, 86 * S]
    assert lt.step_of(11025) == 1103 and lt.step_of(44100) == 4410
    for name in ("tails_1", "tails_6"):
        a, b = cases[name].rows[:2]
        assert a[-1].min() == -np.abs(a).max() and (np.abs(a[:-1]) < np.abs(a).max()).all()  # negative, the last sample of the tail
        assert np.abs(b[0]).max() == np.abs(b).max() and (np.abs(b[1:]) < np.abs(b).max()).all()  # the first sample
    heavy = cases["channels_255_weights"]
    assert heavy.w[lc.PEAK_CHANNEL] == 0.0 and (np.delete(heavy.w, lc.PEAK_CHANNEL) > 0).all()
    assert all(np.abs(r[:, lc.PEAK_CHANNEL]).max() == np.abs(r).max() for r in heavy.rows)
    # the weight table's entries that had never run: 1.41 without an LFE, and 7's own LFE place
    assert list(cases["channels_4"].w) == [1, 1, 1.41, 1.41] and list(cases["channels_5"].w) == [1, 1, 1, 1.41, 1.41]
    assert list(cases["channels_7"].w) == [1, 1, 1, 1.41, 1.41, 1, 0]
    # two grid rounds: more descriptors than the grid's y holds, lengths of every kind, checked rows in the second round
    grid, checked = cases["grid"], lc.grid_checked_rows()
    lengths = np.array([r.shape[0] for r in grid.rows])
    assert len(grid.rows) == lc.GRID_ROWS > k["kLoudMaxGridY"] and lengths.max() == 2 * S + 5 and lengths.min() == 0
    assert sum(i >= k["kLoudMaxGridY"] for i in checked) > 100 and len(cases["grid_checked"].rows) == len(checked)
    assert (lengths < S).sum() > 1000 and (lengths >= 2 * S).sum() > 10
    assert all(r.shape[0] == 0 for r in cases["empty_rows"].rows) and all(0 < r.shape[0] < S for r in cases["short_rows"].rows)
    # finish_blocks: one block at max_steps 256, two at 257
    assert [-(-m // k["kLoudBlock"]) for m in (256, 257)] == [1, 2]


def test_the_float64_restatement_meets_the_bound_with_room_on_the_limit_cases():
    """before any device run: step_sums_chunked -- float64, the shape of the kernels -- lies within 0.01 of the bound of the longdouble
    truth on a multi-workgroup case and on the 255-channel case, so a device result outside the bound is the device's doing"""
    import loudness_cases as lc
    from loudness_support import LONGDOUBLE_BITS
    assert LONGDOUBLE_BITS >= 63, "numpy.longdouble has %d mantissa bits here: float64 would be compared against itself" % LONGDOUBLE_BITS
    some = [lc.cases()[n] for n in ("edges_8", "channels_255_weights")]
    truth = lc.truth_of(some)
    for case in some:
        for i, r in enumerate(case.rows):
            per, want = truth[(case.name, i)]
            got = lt.weighted(lt.step_sums_chunked(r, case.fs), case.w)
            assert got.shape == want.shape and len(want) == r.shape[0] // lc.S
            bound = lt.bound(case.fs, want.astype(np.float64))
            ratio = np.abs(got.astype(np.longdouble) - want).astype(np.float64) / bound
            print("%s row %d: float64 by steps, largest error / bound %.3g" % (case.name, i, ratio.max()))
            assert (ratio <= 0.01).all(), (case.name, i, float(ratio.max()))


def test_the_shift_and_scaling_identities_hold_on_the_restatements():
    """k steps of silence in front of a row move its sums by k places and change no bit (zero state stays zero state); a power of two
    on the samples is its square on the sums, bit for bit (every operation a float64 multiply or add, nothing near underflow)"""
    import loudness_cases as lc
    base = lc.cases()["shift"]
    for k in (1, 3, 32):
        a, b = lc.shifted(base, k).rows
        sa, sb = lt.step_sums_chunked(a, base.fs), lt.step_sums_chunked(b, base.fs)
        assert sb.shape[0] == sa.shape[0] + k and (sb[:k].view(np.int64) == 0).all() and sb[k:].tobytes() == sa.tobytes(), k
        if k < 32:
            seq = lt.step_sums_sequential([a[:, 0], b[:, 0]], [base.fs] * 2, np.float64)
            assert (seq[1][:k].view(np.int64) == 0).all() and seq[1][k:].tobytes() == seq[0].tobytes(), k
    base = lc.cases()["scaling"]
    want = lt.weighted(lt.step_sums_chunked(base.rows[0], base.fs), base.w)
    for e in (-12, 12, -60, 60):
        row = lc.scaled(base, e).rows[0] if abs(e) == 12 else np.ldexp(base.rows[0].astype(np.float64), e)
        got = lt.weighted(lt.step_sums_chunked(row, base.fs), base.w)
        assert got.tobytes() == np.ldexp(want, 2 * e).tobytes(), e
    assert (lc.scaled(base, -12).rows[0].astype(np.float64) == np.ldexp(base.rows[0].astype(np.float64), -12)).all()  # (exact in float32)


def test_the_loudness_kernels_use_no_scratch_and_say_what_they_take():
    import shutil
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = [k for k in kr.analyse(os.path.join(_build.CSRC, "pcm_loudness.hip"), _build.SOURCES["pcm_loudness.hip"]) if "loudness_" in k["name"]]
    assert len(ks) == 4 and sum("loudness_pass" in k["name"] for k in ks) == 2  # (a) and (c), the carry, the finish
    assert sum("loudness_carry" in k["name"] for k in ks) == 1 and sum("loudness_finish" in k["name"] for k in ks) == 1
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 512 and k["occupancy"] >= 1, k
