"""vpz_true_peak_filter, vpz_loudness_range and vpz_loudness_maxima (include/vorbispizza_pcm_r128.h, csrc/pcm_truepeak.hip) without a
device, the known answers of EBU Tech 3341's true-peak shapes and EBU Tech 3342's range shapes, what a clean checkout must hold about the
new headers and bindings, and the cases of tests/test_pcm_true_peak_gpu.py held to the shapes they are named for.

The truth is tests/r128_truth.py: the header's definition restated in numpy.  The range tests feed tests/loudness_truth.py's float64 step
sums (the chunked form) to the library's functions."""
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
import r128_truth as rt  # noqa: E402
import binding_support as cs  # noqa: E402
from binding_support import imports_of  # noqa: E402

KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


# ---- the surface
def test_the_r128_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_r128.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmR128.cs")
    names = ["vpz_loudness_maxima", "vpz_loudness_range", "vpz_pcm_true_peak", "vpz_true_peak_filter"]
    assert sorted(c) == names == sorted(imports) == sorted(capi.PCM_R128_EXPORTED_SYMBOLS)
    # (`double h[49]` is a pointer parameter: the header's parser reads an array declarator as its element)
    assert c["vpz_true_peak_filter"] == ("i32", ["i32", "ptr", "f64"]) and "double h[49]" in open(os.path.join(cs.INC, "vorbispizza_pcm_r128.h")).read()
    c["vpz_true_peak_filter"] = ("i32", ["i32", "ptr", "ptr"])
    assert c["vpz_pcm_true_peak"] == ("i32", ["ptr", "ptr", "i64", "i32", "i32", "i32", "ptr", "ptr", "ptr", "i64"])
    assert c["vpz_loudness_range"] == ("i32", ["ptr", "i64", "i32", "ptr", "ptr", "ptr", "ptr"])
    assert c["vpz_loudness_maxima"] == ("i32", ["ptr", "i64", "i32", "ptr", "ptr"])
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_R128_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    structs, defines = cs.c_structs("vorbispizza_pcm_r128.h")
    assert structs == {} and defines["VPZ_TRUE_PEAK_TAPS"] == capi.TRUE_PEAK_TAPS == rt.TAPS and defines["VPZ_TRUE_PEAK_MAX_COEFFS"] == capi.TRUE_PEAK_MAX_COEFFS == 49
    text = cs.strip_cs_comments(open(os.path.join(cs.CS, "GpuPcmR128.cs")).read())
    assert "TruePeakTaps = 12" in text and "TruePeakMaxCoeffs = 49" in text
    # the older headers and their lists did not take the new names
    older = (capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_RESAMPLE_EXPORTED_SYMBOLS
             + capi.PCM_LOGMEL_EXPORTED_SYMBOLS + capi.PCM_FBANK_EXPORTED_SYMBOLS + capi.PCM_LOUDNESS_EXPORTED_SYMBOLS)
    for name in c:
        assert name not in older
        assert name not in cs.c_functions("vorbispizza_synth.h", "vpz_") and name not in cs.c_functions("vorbispizza_pcm_loudness.h", "vpz_")
    # the new header says that it supplies what the loudness header leaves out, and what stays out of scope
    header = open(os.path.join(cs.INC, "vorbispizza_pcm_r128.h")).read()
    for word in ("supplies what that one leaves out", "int16", "gain", "per-channel", "vpzr_"):
        assert word in header, word
    for word in ("true peak", "loudness range", "short-term"):  # (still listed there: the older header is unchanged)
        assert word in open(os.path.join(cs.INC, "vorbispizza_pcm_loudness.h")).read().split("Out of scope")[1]


def test_the_measure_call_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_r128.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiR128.cs")
    assert sorted(c) == ["vpzm_measure_r128"] == sorted(imports) == sorted(multi.R128_EXPORTED_SYMBOLS)
    assert c["vpzm_measure_r128"] == ("i32", ["ptr", "i32", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"])
    assert c["vpzm_measure_r128"] == cs.c_functions("vorbispizza_multi_loudness.h", "vpzm_")["vpzm_measure_loudness"]
    assert imports["vpzm_measure_r128"] == ("Host",) + c["vpzm_measure_r128"]
    fn = multi.lib().vpzm_measure_r128
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_measure_r128"][1] and KINDS[fn.restype] == "i32"
    structs, _ = cs.c_structs("vorbispizza_multi_r128.h")
    cs_fields = cs.cs_structs(os.path.join(cs.CS, "VorbisPizzaMultiR128.cs"))["R128"]
    py_fields = [(n, {"<f8": "f64", "<i8": "i64"}[multi.R128_DTYPE[n].str], 0) for n in multi.R128_DTYPE.names]
    assert sorted(structs) == ["vpzm_r128"] and len(structs["vpzm_r128"]) == len(cs_fields) == len(py_fields) == 11
    for (n0, k0, a0), (n1, k1, a1), (n2, k2, a2) in zip(structs["vpzm_r128"], cs_fields, py_fields):
        assert cs.norm(n0) == cs.norm(n1) == cs.norm(n2) and k0 == k1 == k2 and a0 == a1 == a2 == 0, (n0, n1, n2)
    assert [n for n, _, _ in py_fields] == ["integrated", "range", "range_low", "range_high", "momentary_max", "short_term_max", "true_peak", "sample_peak",
                                            "steps", "blocks_kept", "range_blocks"]
    assert multi.R128_DTYPE.itemsize == 88 and multi.LOUDNESS_DTYPE.itemsize == 32
    sig = inspect.signature(multi.Dispatcher.measure_r128)
    assert list(sig.parameters) == ["self", "datas", "ranges"] and sig.parameters["ranges"].default is None
    assert "vpzm_measure_r128" not in multi.LOUDNESS_EXPORTED_SYMBOLS + multi.BATCH_EXPORTED_SYMBOLS
    header = open(os.path.join(cs.INC, "vorbispizza_multi_r128.h")).read()
    assert "supplies what that one leaves out" in header


def test_both_libraries_export_the_new_symbols(capi):
    from vorbispizza_amd import _build, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in capi.PCM_R128_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert hasattr(H, "vpzm_measure_r128") and not hasattr(S, "vpzm_measure_r128")
    assert "pcm_truepeak.hip" in _build.SOURCES
    sig = inspect.signature(capi.pcm_true_peak)
    assert list(sig.parameters) == ["ctx", "src", "channels", "sample_rate", "rows", "out"] and sig.parameters["out"].default is None
    assert callable(capi.true_peak_filter) and callable(capi.loudness_range) and callable(capi.loudness_maxima) and callable(multi.Dispatcher.measure_r128)


# ---- the filter
@pytest.mark.parametrize("fs,F", [(8000, 4), (44100, 4), (48000, 4), (95999, 4), (96000, 2), (191999, 2), (192000, 1), (384000, 1)])
def test_the_factor_rule_and_the_prototype(capi, fs, F):
    got_F, h = capi.true_peak_filter(fs)
    assert got_F == F == rt.factor_of(fs) and h.shape == (12 * F + 1,) and h.dtype == np.float64
    want = rt.prototype(F)
    assert np.abs(h - want).max() <= 4 * 2.0 ** -52
    assert (h == h[::-1]).all() or np.abs(h - h[::-1]).max() <= 2.0 ** -52  # symmetric (to the last bit of sin and cos)
    # the identity phase is exact: 1 in the middle, exact zeros at every other multiple of F
    ident = h[::F]
    assert ident[6] == 1.0 and (np.delete(ident, 6) == 0.0).all() and (np.delete(ident, 6).view(np.int64) == 0).all()
    assert (np.delete(h, np.arange(0, 12 * F + 1, F)) != 0).all() or F == 1


def test_the_one_phase_of_2_is_the_middle_phase_of_4(capi):
    _, h4 = capi.true_peak_filter(48000)
    _, h2 = capi.true_peak_filter(96000)
    assert np.array_equal(h2[1::2].astype(np.float32), h4[2::4].astype(np.float32))  # the device coefficients, bit for bit
    assert np.abs(h2[1::2] - h4[2::4]).max() <= 2.0 ** -52 and len(h2[1::2]) == 12
    assert abs(2 * 0.5 * h4[22] - 0.62577) < 1e-5  # (two samples of 0.5: the number the pair cases read)


def test_rates_outside_the_limits_are_refused(capi):
    for fs in (7999, 384001, 0, -48000):
        with pytest.raises(ValueError):
            capi.true_peak_filter(fs)
    L, f, h = capi.lib(), C.c_int32(), np.zeros(49)
    assert L.vpz_true_peak_filter(48000, None, h.ctypes.data) == capi.E_INVALID_ARG
    assert L.vpz_true_peak_filter(48000, C.addressof(f), None) == capi.E_INVALID_ARG
    h[:] = 7.0
    assert L.vpz_true_peak_filter(96000, C.addressof(f), h.ctypes.data) == capi.OK and f.value == 2 and (h[25:] == 0).all() and h[12] == 1.0


# ---- the true peak of the truth on EBU Tech 3341's shapes
@pytest.mark.parametrize("fs", rt.SINE_RATES)
def test_the_truth_reads_the_faded_sines_within_ebus_tolerance(fs):
    for div, phase, amp in rt.SINES:
        x = rt.faded_sine(fs, fs / div, phase, amp)
        tp = rt.true_peak(x, fs)
        dev = 20.0 * np.log10(tp / amp)
        print("%d Hz: fs/%d at %.1f degrees, amplitude %.2f: %+.3f dB (sample peak %+.3f dB)" % (fs, div, phase, amp, dev, 20 * np.log10(np.abs(x).max() / amp)))
        assert rt.TOLERANCE_DB[0] <= dev <= rt.TOLERANCE_DB[1]
        assert tp >= np.abs(x).max()
        by_phases = rt.true_peak_by_phases(x, fs)[0]
        assert abs(by_phases - tp) <= 1e-12  # the two forms of the truth
    # the sample peak alone misses the tolerance at 45 degrees: the case is no formality
    x = rt.faded_sine(fs, fs / 4, 45.0, 0.5)
    assert 20.0 * np.log10(np.abs(x).max() / 0.5) < -2.9


def test_at_192000_hz_the_true_peak_is_the_sample_peak():
    for div, phase, amp in rt.SINES:
        x = rt.faded_sine(192000, 192000 / div, phase, amp)
        assert rt.true_peak(x, 192000) == float(np.abs(x).max()) and rt.bound(x, 192000) == 0.0


def test_an_abrupt_onset_overshoots_and_the_clip_rule_counts_it():
    """why the sines are faded: a sine that starts at full level at 67.5 degrees legitimately reads above its amplitude"""
    fs, n = 48000, 24000
    x = (0.5 * np.sin(2 * np.pi * np.arange(n) / 8 + np.deg2rad(67.5))).astype(np.float32)
    assert 20.0 * np.log10(rt.true_peak(x, fs) / 0.5) > 0.4


# ---- range and maxima
def sums_at(level, S, steps):
    return np.full(steps, S * 10.0 ** ((level + 0.691) / 10.0))


EBU_3342 = [([(20, -20.0), (20, -30.0)], 10.0), ([(20, -20.0), (20, -15.0)], 5.0), ([(20, -40.0), (20, -20.0)], 20.0),
            ([(20, -50.0), (20, -35.0), (20, -20.0), (20, -35.0), (20, -50.0)], 15.0)]
_sums = {}


def ebu_sums(fs, case):
    if (fs, case) not in _sums:
        _sums[(fs, case)] = lt.weighted(lt.step_sums_chunked(lt.sine(fs, EBU_3342[case][0]), fs), lt.weights_of(2))
    return _sums[(fs, case)]


@pytest.mark.parametrize("fs", [48000, 44100])
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_ebu_tech_3342(capi, case, fs):
    """a stereo 1 kHz sine at the stated per-channel peak levels: the range within 1 LU of the target"""
    sums, S = ebu_sums(fs, case), lt.step_of(fs)
    lra, low, high, kept = capi.loudness_range(sums, S)
    print("EBU Tech 3342 shape %d at %d Hz: LRA %.4f LU (target %.0f), %.3f .. %.3f LUFS, %d blocks" % (case + 1, fs, lra, EBU_3342[case][1], low, high, kept))
    assert abs(lra - EBU_3342[case][1]) <= 1.0
    want = rt.loudness_range(sums, S)
    assert kept == want[3] and np.abs(np.array([lra, low, high]) - np.array(want[:3])).max() <= 1e-12
    if fs == 48000:
        assert kept == (627 if case == 3 else 371)
    mom, short = capi.loudness_maxima(sums, S)
    assert np.abs(np.array([mom, short]) - np.array(rt.loudness_maxima(sums, S))).max() <= 1e-12
    loudest = max(db for _, db in EBU_3342[case][0])
    assert abs(short - loudest) < 0.1 and abs(mom - loudest) < 0.1  # (a stereo 1 kHz sine of per-channel peak level d dBFS reads d LUFS: EBU Tech 3341)


def test_range_and_maxima_equal_the_truth_on_noise(capi):
    rng = np.random.default_rng(3342)
    for S, n in ((800, 30), (800, 31), (4410, 200), (4800, 999)):
        sums = S * 10.0 ** (rng.uniform(-6.0, -1.0, size=n))
        got, want = capi.loudness_range(sums, S), rt.loudness_range(sums, S)
        assert got[3] == want[3] and np.abs(np.array(got[:3]) - np.array(want[:3])).max() <= 1e-12, (S, n)
        assert np.abs(np.array(capi.loudness_maxima(sums, S)) - np.array(rt.loudness_maxima(sums, S))).max() <= 1e-12


@pytest.mark.parametrize("m,lo,hi", [(1, 0, 0), (2, 0, 1), (11, 1, 10), (21, 2, 19)])
def test_the_percentile_index_rule(capi, m, lo, hi):
    """m kept blocks of distinct levels: low = v[floor(0.10 (m-1) + 0.5)], high = v[floor(0.95 (m-1) + 0.5)].  m + 29 steps whose level
    rises slowly give exactly m blocks, all kept, all different; the indices the rule picks are written out above"""
    assert (int(np.floor(0.10 * (m - 1) + 0.5)), int(np.floor(0.95 * (m - 1) + 0.5))) == (lo, hi)
    S = 800
    # m blocks exactly: m + 29 steps whose 3 s levels rise slowly (all within 20 LU, all above -70)
    sums = S * 10.0 ** ((np.linspace(-30.0, -25.0, m + 29) + 0.691) / 10.0)
    _, l = rt.block_levels(sums, S, 30)
    v = np.sort(l)
    lra, low, high, kept = capi.loudness_range(sums, S)
    assert kept == m == len(v)
    assert abs(low - v[lo]) <= 1e-12 and abs(high - v[hi]) <= 1e-12 and abs(lra - (v[hi] - v[lo])) <= 1e-12
    if m > 2:
        assert v[lo] != v[lo + 1] and v[hi] != v[hi - 1]  # (a neighbouring index would read another level)


def test_too_few_steps_silence_and_nan(capi):
    S = 4800
    for steps in (0, 1, 29):
        assert capi.loudness_range(sums_at(-20.0, S, steps), S) == (0.0, -np.inf, -np.inf, 0)
    lra, low, high, kept = capi.loudness_range(sums_at(-20.0, S, 30), S)
    assert kept == 1 and lra == 0.0 and abs(low + 20.0) < 1e-12 and low == high
    assert capi.loudness_range(np.zeros(100), S) == (0.0, -np.inf, -np.inf, 0)  # (silence: nothing passes the absolute gate)
    assert capi.loudness_maxima(np.zeros(100), S) == (-np.inf, -np.inf)
    assert capi.loudness_maxima(sums_at(-20.0, S, 3), S) == (-np.inf, -np.inf)
    mom, short = capi.loudness_maxima(sums_at(-20.0, S, 4), S)
    assert abs(mom + 20.0) < 1e-12 and short == -np.inf
    # a NaN step: the blocks that hold it fail both comparisons and are not kept; the maxima pass them over
    sums = np.concatenate([sums_at(-20.0, S, 40), sums_at(-26.0, S, 40)])
    sums[50] = np.nan
    got, want = capi.loudness_range(sums, S), rt.loudness_range(sums, S)
    assert got[3] == want[3] == (80 - 29) - 30 and np.abs(np.array(got[:3]) - np.array(want[:3])).max() <= 1e-12
    assert np.abs(np.array(capi.loudness_maxima(sums, S)) - np.array(rt.loudness_maxima(sums, S))).max() <= 1e-12
    assert abs(capi.loudness_maxima(sums, S)[0] + 20.0) < 1e-9
    all_nan = np.full(40, np.nan)
    assert capi.loudness_range(all_nan, S) == (0.0, -np.inf, -np.inf, 0) and capi.loudness_maxima(all_nan, S) == (-np.inf, -np.inf)


def test_range_and_maxima_refuse_what_the_header_says(capi):
    L = capi.lib()
    sums = np.ones(40)
    a, b, c, k = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
    p = C.addressof
    assert L.vpz_loudness_range(sums.ctypes.data, 40, 4800, p(a), p(b), p(c), p(k)) == capi.OK and k.value == 11
    assert L.vpz_loudness_range(sums.ctypes.data, 40, 4800, p(a), None, None, None) == capi.OK  # (all but the range are optional)
    assert L.vpz_loudness_range(sums.ctypes.data, 40, 4800, None, p(b), p(c), p(k)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_range(None, 40, 4800, p(a), p(b), p(c), p(k)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_range(sums.ctypes.data, -1, 4800, p(a), p(b), p(c), p(k)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_range(sums.ctypes.data, 40, 0, p(a), p(b), p(c), p(k)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_range(None, 0, 4800, p(a), p(b), p(c), p(k)) == capi.OK and (a.value, b.value, k.value) == (0.0, -np.inf, 0)
    assert L.vpz_loudness_maxima(sums.ctypes.data, 40, 4800, p(a), p(b)) == capi.OK
    assert L.vpz_loudness_maxima(sums.ctypes.data, 40, 4800, p(a), None) == capi.OK and L.vpz_loudness_maxima(sums.ctypes.data, 40, 4800, None, p(b)) == capi.OK
    assert L.vpz_loudness_maxima(sums.ctypes.data, 40, 4800, None, None) == capi.E_INVALID_ARG
    assert L.vpz_loudness_maxima(None, 40, 4800, p(a), p(b)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_maxima(sums.ctypes.data, -1, 4800, p(a), p(b)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_maxima(sums.ctypes.data, 40, 0, p(a), p(b)) == capi.E_INVALID_ARG
    assert L.vpz_loudness_maxima(None, 0, 4800, p(a), p(b)) == capi.OK and (a.value, b.value) == (-np.inf, -np.inf)


# ---- the launch plan of vpz_pcm_true_peak, and the cases of tests/test_pcm_true_peak_gpu.py
def test_the_launch_plan():
    k = rt.kernel_constants(ROOT)
    assert (k["kTpBlock"], k["kTpTile"], k["kTpTaps"], k["kTpMaxGridY"]) == (256, 4096, 12, 4096)
    assert k["kTpTile"] % k["kTpBlock"] == 0 and k["kTpBlock"] % 64 == 0
    assert rt.launch_plan(0, 2, k)[:2] == (0, 0) and rt.launch_plan(1, 1, k)[:2] == (12, 1)
    T = k["kTpTile"]
    assert rt.launch_plan(T - 11, 1, k)[1] == 1 and rt.launch_plan(T - 10, 1, k)[1] == 2  # (the tail counts: L + 11 positions)
    assert max(rt.launch_plan(1, c, k)[2] for c in range(1, 256)) == rt.launch_plan(1, 255, k)[2] == (11 * 255 + T + 8) * 4 <= 28 * 1024
    # consecutive lanes read consecutive floats at every tap: 32 different banks in every group of 32, whatever the channel count
    for channels in (1, 2, 3, 255):
        lane = np.arange(32)
        for tap in range(12):
            assert len(set(((11 * channels + lane - tap * channels) % 32).tolist())) == 32


def test_every_case_is_the_shape_it_is_named_for():
    import r128_cases as rc
    k, T = rc.K, rc.T
    cases = rc.cases()
    assert [r.shape[0] for r in cases["rows"].rows] == [0, 1, 2, 11, 12, 13, T - 1, T, T + 1, 2 * T + 5]
    assert [rt.launch_plan(r.shape[0], 1, k)[1] for r in cases["rows"].rows] == [0, 1, 1, 1, 1, 1, 2, 2, 2, 3]
    assert all(rc.crest(r) <= 4.0 for r in cases["rows"].rows if r.shape[0] >= 11)
    # the peak shapes: where the truth's peak lies (output index i * 4 + p), and that the sample peak alone would miss it
    shapes = cases["shapes"]
    where = []
    for i, r in enumerate(shapes.rows):
        peak, at, _ = rt.true_peak_by_phases(r, shapes.fs)
        assert abs(peak - rc.truth("shapes", i)[0]) <= 1e-12
        where.append(divmod(at, 4))
        if i < 7:
            assert abs(peak - rc.PAIR_PEAK) < 0.03 and np.abs(r).max() == np.float32(rc.PAIR) and peak > 0.6, i
    L = shapes.rows[0].shape[0]
    assert where[0] == (L + 4, 2) and where[0][0] >= L        # behind the last sample: a kernel that stops at i < L reads 0.5
    assert where[1] == (6, 2)                                   # the first two samples
    assert where[2] == (T + 5, 2) and rt.tile_of(T + 5, 0, 1, k) == 1 and rt.tile_of(T - 1, 0, 1, k) == 0   # inputs T-1 | T
    assert where[3] == (2 * T + 5, 2) and rt.tile_of(2 * T + 5, 0, 1, k) == 2
    assert where[4] == (T - 1, 2)                               # the output is the last position of tile 0
    assert where[5] == (T, 2)                                   # the output is the first of tile 1, both inputs in its halo
    assert shapes.rows[6].min() == -np.float32(rc.PAIR) and shapes.rows[6].max() < 0.1
    assert rc.truth("shapes", 7)[0] == rc.truth("shapes", 7)[1] == float(np.float32(0.7))  # an impulse: true peak = sample peak
    # channel counts: the pair sits in the sample the first tile boundary falls into, in the last channel and in channel 0
    assert rc.CHANNEL_COUNTS == (1, 2, 3, 6, 8, 33, 255)
    for channels in rc.CHANNEL_COUNTS:
        case = cases["channels_%d" % channels]
        s = T // channels
        a, b, c = case.rows
        assert a[s, channels - 1] == a[s + 1, channels - 1] == np.float32(rc.PAIR) and b[s, 0] == b[s + 1, 0] == np.float32(rc.PAIR)
        assert rt.tile_of(s, 0, channels, k) == (1 if T % channels == 0 else 0) and rt.tile_of(s - 1, channels - 1, channels, k) == 0
        assert rt.tile_of(s + 1, channels - 1, channels, k) == 1
        assert rt.launch_plan(a.shape[0], channels, k)[1] >= 3 and rc.crest(c) <= 4.0
        for i in (0, 1):
            assert abs(rc.truth(case.name, i)[0] - rc.PAIR_PEAK) < 0.03 and rc.truth(case.name, i)[1] == float(np.float32(rc.PAIR))
    assert T % 3 == 1 and T % 255 != 0 and T % 33 != 0  # a tile boundary in the middle of a sample
    # rates
    assert [rt.factor_of(fs) for fs in (44100, 96000, 191999, 192000, 384000)] == [4, 2, 2, 1, 1]
    for fs in (192000, 384000):
        for i in range(2):
            tp, sp, bound = rc.truth("rate_%d" % fs, i)
            assert tp == sp and bound == 0.0
    # the grid: more descriptors than its y holds, checked rows in the second round, every length from 0 to 40
    grid = cases["grid"]
    lengths = np.array([r.shape[0] for r in grid.rows])
    assert len(grid.rows) == rc.GRID_ROWS > k["kTpMaxGridY"] and lengths.min() == 0 and lengths.max() == 40 and len(set(lengths.tolist())) == 41
    checked = rc.grid_checked_rows()
    assert checked[0] == 0 and checked[-1] == rc.GRID_ROWS - 1 and sum(i >= k["kTpMaxGridY"] for i in checked) > 100
    # non-finite rows: the NaN row keeps a finite peak beside the NaN, the Inf row reads +Inf
    tp, sp, _ = rc.truth("nonfinite", 1)
    assert np.isfinite(tp) and tp >= sp == float(np.float32(0.9))
    assert rc.truth("nonfinite", 3)[0] == np.inf and rc.truth("nonfinite", 3)[1] == np.inf
    # every finite row of every case: true peak >= sample peak, and a bound that is small beside it
    for case in cases.values():
        for i in (range(len(case.rows)) if case.name != "grid" else checked[:50]):
            tp, sp, bound = rc.truth(case.name, i)
            assert tp >= sp and (bound <= 4e-6 * max(tp, 1e-30) * 8 or not np.isfinite(tp)), (case.name, i)


def test_the_truth_meets_the_device_tests_conditions():
    """float32 arithmetic in the header's order, in numpy, stands inside the bound on the pair cases and a noise case -- so a device
    result outside the bound is the device's doing; and the faded sines at every rate read within EBU's tolerance in float32 too"""
    import r128_cases as rc
    for name, rows in (("shapes", range(8)), ("channels_3", range(3)), ("rate_96000", range(2))):
        case = rc.cases()[name]
        for i in rows:
            tp, _, bound = rc.truth(name, i)
            got = rt.true_peak_by_phases(case.rows[i], case.fs, np.float32)[0]
            assert abs(got - tp) <= bound, (name, i, abs(got - tp) / bound)
    for fs in rt.SINE_RATES:
        case = rc.cases()["sines_%d" % fs]
        for i, (div, phase, amp) in enumerate(rt.SINES):
            dev = 20.0 * np.log10(rt.true_peak_by_phases(case.rows[i], fs, np.float32)[0] / amp)
            assert rt.TOLERANCE_DB[0] <= dev <= rt.TOLERANCE_DB[1]


def test_the_true_peak_kernels_use_no_scratch_and_say_what_they_take():
    import shutil
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = [k for k in kr.analyse(os.path.join(_build.CSRC, "pcm_truepeak.hip"), _build.SOURCES["pcm_truepeak.hip"]) if "true_peak_" in k["name"]]
    assert len(ks) == 4 and sum("true_peak_tiles" in k["name"] for k in ks) == 3 and sum("true_peak_finish" in k["name"] for k in ks) == 1
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 64 and k["occupancy"] == 8, k
