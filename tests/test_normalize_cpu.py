"""vpz_pcm_normalize and vpzm_decode_ranges_normalized without a device: the headers, the bindings, the Python surface, and the numpy bit
model (tests/normalize_truth.py) held to the longdouble two-pass truth within the header's derived bound on the GPU tests' case list."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import binding_support as cs  # noqa: E402
import normalize_cases as nc  # noqa: E402
import normalize_truth as nt  # noqa: E402
from binding_support import imports_of  # noqa: E402

KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


def _compile_and_run(tmp_path, name, text):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    src, exe = tmp_path / (name + ".c"), tmp_path / (name + ".exe")
    src.write_text(text)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


# ---- the surface
def test_the_stage_header_is_plain_c(tmp_path):
    body = ("sizeof(vpz_norm_row) == 32 && offsetof(vpz_norm_row, gain) == 24 && sizeof(vpz_norm_spec) == 64 && "
            "offsetof(vpz_norm_spec, mode) == 24 && offsetof(vpz_norm_spec, channels) == 28 && offsetof(vpz_norm_spec, reserved) == 32 && "
            "sizeof(vpz_norm_result) == 40 && offsetof(vpz_norm_result, gain) == 32 && VPZ_NORM_CHUNK == 1024 && "
            "VPZ_NORM_MEANVAR == 1 && VPZ_NORM_PEAK == 2 && VPZ_NORM_RMS == 3 && VPZ_NORM_GAIN == 4")
    _compile_and_run(tmp_path, "normalize", '#include <stddef.h>\n#include "vorbispizza_pcm_normalize.h"\n#include "vorbispizza_pcm_featpost.h"\n'
                     'typedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % body)


def test_the_call_header_is_plain_c(tmp_path):
    body = ("sizeof(vpzm_norm_spec) == 64 && offsetof(vpzm_norm_spec, mode) == 24 && offsetof(vpzm_norm_spec, reserved) == 28 && "
            "sizeof(vpzm_norm_out) == 32 && offsetof(vpzm_norm_out, loudness) == 24 && VPZM_NORM_MEANVAR == VPZ_NORM_MEANVAR && "
            "VPZM_NORM_PEAK == VPZ_NORM_PEAK && VPZM_NORM_RMS == VPZ_NORM_RMS && VPZM_NORM_GAIN == VPZ_NORM_GAIN && VPZM_NORM_LOUDNESS == 5 && "
            "VPZM_E_ARG < 0")
    _compile_and_run(tmp_path, "multi_normalize", '#include <stddef.h>\n#include "vorbispizza_multi_normalize.h"\n'
                     'typedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % body)


def test_the_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_normalize.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmNormalize.cs")
    assert sorted(c) == ["vpz_pcm_normalize", "vpz_pcm_normalize_scratch"] == sorted(imports) == sorted(capi.PCM_NORMALIZE_EXPORTED_SYMBOLS)
    assert c["vpz_pcm_normalize"] == ("i32", ["ptr", "ptr", "i64", "i64", "ptr", "i32", "ptr", "ptr", "i64", "i32", "ptr", "i64", "ptr"])
    assert c["vpz_pcm_normalize_scratch"] == ("i32", ["i32", "i32", "i64", "ptr"])
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_NORMALIZE_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    structs, defines = cs.c_structs("vorbispizza_pcm_normalize.h")
    cs_structs = cs.cs_structs(os.path.join(cs.CS, "GpuPcmNormalize.cs"))
    assert sorted(structs) == ["vpz_norm_result", "vpz_norm_row", "vpz_norm_spec"] and sorted(cs_structs) == ["NormResult", "NormRow", "NormSpec"]
    for c_name, cs_name in (("vpz_norm_result", "NormResult"), ("vpz_norm_row", "NormRow"), ("vpz_norm_spec", "NormSpec")):
        assert [(cs.norm(n), k, a) for n, k, a in cs_structs[cs_name]] == [(cs.norm(n), k, a) for n, k, a in structs[c_name]], c_name
    assert structs["vpz_norm_row"] == [("src", "i64", 0), ("samples", "i64", 0), ("row", "i64", 0), ("gain", "f64", 0)]
    assert [n for n, _, _ in structs["vpz_norm_result"]] == list(capi.NORM_RESULT_FIELDS)
    for py, c_name in ((capi.NormSpec, "vpz_norm_spec"), (capi.NormRow, "vpz_norm_row")):
        fields = [(n, {C.c_double: "f64", C.c_int64: "i64"}.get(t, "i32"), getattr(t, "_length_", 0)) for n, t in py._fields_]
        assert fields == structs[c_name], c_name
    assert C.sizeof(capi.NormSpec) == 64 and C.sizeof(capi.NormRow) == 32
    # the constants: header, C# and Python
    text = cs.strip_cs_comments(open(os.path.join(cs.CS, "GpuPcmNormalize.cs")).read())
    consts = {}
    for m in re.finditer(r"public\s+const\s+int\s+([^;]+);", text):
        for part in m.group(1).split(","):
            k, v = part.split("=")
            consts[cs.norm(k.strip())] = int(v.strip(), 0)
    mine = {k: v for k, v in defines.items() if k.startswith("VPZ_")}
    assert sorted(mine) == ["VPZ_NORM_CHUNK", "VPZ_NORM_GAIN", "VPZ_NORM_MEANVAR", "VPZ_NORM_PEAK", "VPZ_NORM_RMS"]
    for name, value in mine.items():
        assert consts[cs.norm(name[4:])] == value == getattr(capi, name[4:]), name
    assert capi.NORM_MODES == {"meanvar": 1, "peak": 2, "rms": 3, "gain": 4} == nt.MODES and nt.CHUNK == capi.NORM_CHUNK
    # the feature post-processing's VPZ_NORM_* keep their values beside the new ones
    assert cs.c_structs("vorbispizza_pcm_featpost.h")[1]["VPZ_NORM_SLIDING"] == 2
    # the older headers and their lists did not take the new names
    older = (capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_RESAMPLE_EXPORTED_SYMBOLS
             + capi.PCM_LOGMEL_EXPORTED_SYMBOLS + capi.PCM_FBANK_EXPORTED_SYMBOLS + capi.PCM_MFCC_EXPORTED_SYMBOLS + capi.PCM_FEATPOST_EXPORTED_SYMBOLS)
    for name in c:
        assert name not in older


def test_the_call_binding_matches_its_header(tmp_path, capi):
    from vorbispizza_amd import multi, normalize
    c = cs.c_functions("vorbispizza_multi_normalize.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiNormalize.cs")
    assert sorted(c) == ["vpzm_decode_ranges_normalized"] == sorted(imports) == sorted(normalize.EXPORTED_SYMBOLS)
    # the resampled call's parameters with the spec and the per-entry output behind them
    ret, params = cs.c_functions("vorbispizza_multi_resample.h", "vpzm_")["vpzm_decode_ranges_resampled"]
    assert c["vpzm_decode_ranges_normalized"] == (ret, params + ["ptr", "ptr"])
    assert imports["vpzm_decode_ranges_normalized"] == ("Host",) + c["vpzm_decode_ranges_normalized"]
    fn = multi.lib().vpzm_decode_ranges_normalized
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_decode_ranges_normalized"][1] and KINDS[fn.restype] == "i32"
    structs, defines = cs.c_structs("vorbispizza_multi_normalize.h")
    cs_structs = cs.cs_structs(os.path.join(cs.CS, "VorbisPizzaMultiNormalize.cs"))
    assert sorted(structs) == ["vpzm_norm_out", "vpzm_norm_spec"] and sorted(cs_structs) == ["NormOut", "NormSpec"]
    for c_name, cs_name in (("vpzm_norm_out", "NormOut"), ("vpzm_norm_spec", "NormSpec")):
        assert [(cs.norm(n), k, a) for n, k, a in cs_structs[cs_name]] == [(cs.norm(n), k, a) for n, k, a in structs[c_name]], c_name
    assert structs["vpzm_norm_out"] == [("gain", "f64", 0), ("mean", "f64", 0), ("peak", "f64", 0), ("loudness", "f64", 0)]
    assert structs["vpzm_norm_spec"] == [("target", "f64", 0), ("eps", "f64", 0), ("ceiling", "f64", 0), ("mode", "i32", 0), ("reserved", "i32", 9)]
    for py, c_name in ((normalize.MultiNormSpec, "vpzm_norm_spec"), (normalize.MultiNormOut, "vpzm_norm_out")):
        fields = [(n, {C.c_double: "f64"}.get(t, "i32"), getattr(t, "_length_", 0)) for n, t in py._fields_]
        assert fields == structs[c_name], c_name
    assert normalize.MODES == {"meanvar": 1, "peak": 2, "rms": 3, "gain": 4, "loudness": 5}
    assert {k: defines["VPZM_NORM_" + k.upper()] for k in normalize.MODES} == normalize.MODES


def test_the_library_exports_the_new_symbols_and_no_others(capi):
    from vorbispizza_amd import _build, front, normalize
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in normalize.EXPORTED_SYMBOLS:
        assert hasattr(H, name) and not hasattr(S, name), name
    for name in capi.PCM_NORMALIZE_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert _build.SOURCES["pcm_normalize.hip"] == ["-ffp-contract=off"] and os.path.exists(os.path.join(_build.CSRC, "pcm_normalize.hip"))
    # what the two libraries define with "normal" in its name is exactly the new entry points
    for path, want in ((capi.LIB_PATH, capi.PCM_NORMALIZE_EXPORTED_SYMBOLS), (_build.HOST_LIB_PATH, normalize.EXPORTED_SYMBOLS)):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = [line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith(("vpz_", "vpzm_"))]
        assert sorted(n for n in names if "normal" in n) == sorted(want), path


def test_the_python_surface(capi):
    from vorbispizza_amd import multi, normalize
    s = capi.NormSpec.make()
    assert (s.mode, s.channels, s.target, s.eps, s.ceiling, list(s.reserved)) == (capi.NORM_MEANVAR, 1, 0.0, 1e-7, 0.0, [0] * 8)
    assert [capi.NormSpec.make(m).target for m in ("peak", "rms", "gain")] == [1.0, 0.1, 1.0]
    s = capi.NormSpec.make("rms", channels=2, target=0.25, ceiling=0.9)
    assert (s.mode, s.channels, s.target, s.ceiling) == (capi.NORM_RMS, 2, 0.25, 0.9)
    with pytest.raises(ValueError):
        capi.NormSpec.make("loudness")  # (the dispatcher's mode, not the stage's)
    assert str(inspect.signature(capi.NormSpec.make)) == "(mode='meanvar', channels=1, target=None, eps=1e-07, ceiling=0.0)"
    assert str(inspect.signature(capi.pcm_normalize)) == "(ctx, src, rows, dst, spec, frames, gains=None, results=False)"
    assert str(inspect.signature(capi.pcm_normalize_scratch)) == "(n_rows, channels, frames)"
    assert str(inspect.signature(normalize.decode_ranges_normalized)) == (
        "(dispatcher, datas, ranges, channels, frames, sample_rate, mono=False, mode='meanvar', target=None, eps=1e-07, ceiling=0.0, "
        "planar=True, s16=False, out=None)")
    assert normalize.DEFAULT_TARGETS == {"meanvar": 0.0, "peak": 1.0, "rms": 0.1, "loudness": -23.0, "gain": 1.0}
    for fn in (capi.pcm_normalize, capi.pcm_normalize_scratch, normalize.decode_ranges_normalized, capi.NormSpec):
        assert fn.__doc__ and len(fn.__doc__) > 40
    # the dispatcher's public methods stay what they were: the entry point is the module's function, its helper is underscore-named
    assert not hasattr(multi.Dispatcher, "decode_ranges_normalized") and hasattr(multi.Dispatcher, "_decode_ranges_normalized")


def test_the_scratch_size(capi):
    assert capi.pcm_normalize_scratch(0, 1, 1) == 0
    assert capi.pcm_normalize_scratch(1, 1, 1) == 3 + 2 == capi.pcm_normalize_scratch(1, 1, 1024)
    assert capi.pcm_normalize_scratch(1, 1, 1025) == 6 + 2
    assert capi.pcm_normalize_scratch(7, 3, 3 * 1024 + 17) == 7 * (3 * 3 * 4 + 2)
    for bad in ((-1, 1, 8), (1, 0, 8), (1, 256, 8), (1, 1, 0), (2 ** 31 - 1, 255, 2 ** 62)):
        with pytest.raises(ValueError):
            capi.pcm_normalize_scratch(*bad)
    assert capi.lib().vpz_pcm_normalize_scratch(1, 1, 8, None) == capi.E_INVALID_ARG


# ---- the bit model against the truth
def _batch(case):
    w = nc.window_of(case)
    return np.stack([w] * len(nc.ROWS))


@pytest.mark.parametrize("C_", nc.CHANNELS)
def test_the_model_is_within_the_derived_bound_of_the_truth(C_):
    worst = 0.0
    for case in [c for c in nc.all_cases() if c.C == C_ or (C_ == 2 and c.C not in nc.CHANNELS)]:
        x, kw = _batch(case), nc.spec_args(case)
        got = nt.model(x, **kw)
        ystar, bound, rho = nt.truth(x, **kw)
        assert (rho <= 0.5).all(), (case.name, rho)
        ratio = nt.worst_ratio(got["y"], ystar, bound)
        assert ratio <= 1.0, (case.name, ratio)
        worst = max(worst, ratio)
        if nc.plain(case):  # the launch without statistics gives the same values
            assert np.array_equal(nt.plain_gain(x, kw["gains"]).view(np.uint32), got["y"].view(np.uint32)), case.name
        if case.s16:  # within 1 of the truth's conversion wherever the bound is below an int16 step
            want = np.clip(np.trunc(np.asarray(ystar * 32768, dtype=np.float64)), -32768, 32767)
            fine = np.asarray(bound * 32768 < 1)
            assert (np.abs(nt.to_s16(got["y"]).astype(np.float64) - want)[fine] <= 1).all(), case.name
    print("largest error / bound, channels %d: %.4f" % (C_, worst))
    assert worst > 0.01  # the bound is of the error's size, not a blanket


def test_the_bound_discriminates():
    # one float32 step on the gain, or a mean that is off by one float32 step, is outside the bound
    case = [c for c in nc.special_cases() if c.name.startswith("dc-meanvar")][0]
    x, kw = _batch(case), nc.spec_args(case)
    got = nt.model(x, **kw)
    ystar, bound, _ = nt.truth(x, **kw)
    assert nt.worst_ratio(got["y"], ystar, bound) <= 1.0
    off = (x - np.nextafter(got["mean"].astype(np.float32), np.float32(2))[:, None, None]) * got["gain"].astype(np.float32)[:, None, None]
    assert nt.worst_ratio(off, ystar, bound) > 1.0
    case = [c for c in nc.level_layout_cases() if c.mode == "peak" and c.ceiling == 0.0][0]
    x, kw = _batch(case), nc.spec_args(case)
    got = nt.model(x, **kw)
    ystar, bound, _ = nt.truth(x, **kw)
    off = x * np.nextafter(np.nextafter(got["gain"].astype(np.float32), np.float32(9)), np.float32(9))[:, None, None]
    assert nt.worst_ratio(got["y"], ystar, bound) <= 1.0 < nt.worst_ratio(off, ystar, bound)


def test_the_int16_conversion():
    y = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 0.99999, 3.0e-5, -3.0e-5, 3.1e-5, 1e30, -1e30, np.inf, -np.inf, np.nan, 32767.5 / 32768],
                 dtype=np.float32)
    assert nt.to_s16(y).tolist() == [0, 0, 16384, -16384, 32767, -32768, 32767, 0, 0, 1, 32767, -32768, 32767, -32768, 0, 32767]


def test_the_special_rows():
    for case in nc.special_cases():
        x, kw = _batch(case), nc.spec_args(case)
        got = nt.model(x, **kw)
        if case.kind == "zero":
            assert (got["gain"] == 1.0).all() and (got["mean"] == 0.0).all() and (got["y"].view(np.uint32) == 0).all(), case.name
        if case.kind == "constant" and case.mode == "meanvar":  # the sum of N equal float32 values is exact: every value is +0.0
            assert (got["mean"] == np.float64(np.float32(0.3))).all() and (got["y"].view(np.uint32) == 0).all(), case.name
        if case.kind == "dc" and case.mode == "meanvar":  # the one-pass variance has lost digits, and the bound says how many
            _, _, rho = nt.truth(x, **kw)
            assert 1e-9 < float(rho[0]) < 1e-5, float(rho[0])


def test_the_models_bits_do_not_depend_on_where_a_window_lies():
    for case in nc.level_layout_cases()[:8] + nc.shape_cases()[-4:]:
        w = nc.window_of(case)
        src, offs = nt.lay_out([w] * 3, case.frames, nc.GAPS)
        assert offs[0] % 4 == 0 and len({o % 4 for o in offs}) >= 2  # one window starts on a 16-byte boundary, one does not
        back = np.stack([np.stack([src[o + c * case.frames:o + c * case.frames + case.J] for c in range(case.C)]) for o in offs])
        got = nt.model(back, **nc.spec_args(case))
        for r in (1, 2):
            assert np.array_equal(got["y"][r].view(np.uint32), got["y"][0].view(np.uint32)), case.name
            for key in ("sum", "sum_sq", "peak", "mean", "gain"):
                assert got[key][r].view(np.uint64) == got[key][0].view(np.uint64), (case.name, key)
        # and a window's bits are its own: in a batch with other windows, in another order, nothing moves
        other = nt.signal("noise", case.C, case.J, 99)
        mixed = nt.model(np.stack([other, w]), **dict(nc.spec_args(case), gains=[case.gain] * 2 if case.mode == "gain" else None))
        assert np.array_equal(mixed["y"][1].view(np.uint32), got["y"][0].view(np.uint32)), case.name


def test_the_order_of_the_sums_is_the_stated_one():
    # a window whose sum depends on the order: the model is not numpy's pairwise sum nor a running sum, and a chunk is 1024 samples
    x = nt.signal("outlier", 1, 2 * 1024 + 5, 7)[None]
    S1, S2, P = nt.sums(x)
    assert P[0] == 1e4
    lanes = np.zeros(64)
    seg = np.zeros(1024)
    total = 0.0
    for q in range(3):
        seg[:] = 0.0
        part = x[0, 0, 1024 * q:1024 * (q + 1)].astype(np.float64)
        seg[:part.size] = part
        for lane in range(64):
            acc = 0.0
            for t in range(4):
                for i in range(4):
                    acc += seg[256 * t + 4 * lane + i]
            lanes[lane] = acc
        fold = lanes.copy()
        for off in (32, 16, 8, 4, 2, 1):
            fold[:off] = fold[:off] + fold[off:2 * off]
        total += fold[0]
    assert np.float64(total).view(np.uint64) == S1[0].view(np.uint64)


def test_the_ceiling_rule_takes_both_branches():
    taken = {m: set() for m in ("peak", "rms", "gain")}
    for case in nc.level_layout_cases() + nc.shape_cases():
        if case.ceiling == 0.0 or case.J == 0:
            continue
        x, kw = _batch(case), nc.spec_args(case)
        got, free = nt.model(x, **kw), nt.model(x, **dict(kw, ceiling=0.0))
        g, g0, P = got["gain"][0], free["gain"][0], got["peak"][0]
        if g != g0:
            assert g < g0 and g == np.float64(np.float32(np.float64(case.ceiling) / P)), case.name
            assert np.float64(g0) * P > case.ceiling * (1 - 1e-6)
        else:
            assert g * P <= case.ceiling * (1 + 1e-6), case.name
        taken[case.mode].add(bool(g != g0))
    assert all(v == {True, False} for v in taken.values()), taken
    # MEANVAR takes no ceiling, and the delivered peak stays at the ceiling to a float32 step
    case = [c for c in nc.level_layout_cases() if c.mode == "peak" and c.ceiling == 0.15][0]
    got = nt.model(_batch(case), **nc.spec_args(case))
    assert abs(float(np.abs(got["y"]).max()) - 0.15) <= 0.15 * 2.0 ** -23
