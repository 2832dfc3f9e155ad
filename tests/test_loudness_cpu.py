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
import test_csharp_binding_cpu as cs  # noqa: E402
from test_mixed_setups_cpu import imports_of  # noqa: E402

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
