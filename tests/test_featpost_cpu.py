"""The host side of vpz_feat_post (include/vorbispizza_pcm_featpost.h, csrc/pcm_featpost.hip) without a device: the delta scales, a
frame's window against a Python restatement, the scratch size, every refusal of the spec, what a clean checkout must hold about the new
header and its bindings, and the truth's own bound.

The truth is tests/featpost_truth.py: the header's definition in numpy.longdouble."""
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

import featpost_truth as pt  # noqa: E402
import binding_support as cs  # noqa: E402
from binding_support import imports_of  # noqa: E402
from featpost_truth import NS, make, refused_specs  # noqa: E402

KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


# ---- the delta scales
def test_the_closed_forms_of_the_header(capi):
    s = make(capi, delta_order=2, delta_window=2)[0]
    assert (capi.feat_delta_scales(s, 0) == np.float32([1])).all()
    assert (capi.feat_delta_scales(s, 1) == (np.float64([-2, -1, 0, 1, 2]) / 10).astype(np.float32)).all()
    assert (capi.feat_delta_scales(s, 2) == (np.float64([4, 4, 1, -4, -10, -4, 1, 4, 4]) / 100).astype(np.float32)).all()


@pytest.mark.parametrize("w", [1, 2, 3, 8])
def test_the_scales_are_the_convolution_rounded_once(capi, w):
    """orders 0 to 3 at windows 1 to 8 against the longdouble convolution: the float32 nearest to it (the value is a ratio of integers, so
    the longdouble is within 2^-63 of it: no double rounding at these sizes); odd orders antisymmetric, even ones symmetric; a delta of a
    constant is 0 and the first delta of a ramp is its slope"""
    s = make(capi, delta_order=3, delta_window=w)[0]
    for i in range(4):
        got = capi.feat_delta_scales(s, i)
        want = pt.scales(i, w)
        assert got.dtype == np.float32 and got.shape == (2 * i * w + 1,)
        assert (got == want.astype(np.float32)).all(), (i, w)
        assert (got == (-got[::-1] if i % 2 else got[::-1])).all()
        if i:
            assert abs(float(want.sum())) < 1e-17
    k = np.arange(-w, w + 1).astype(np.longdouble)
    assert abs(float((pt.scales(1, w) * k).sum()) - 1.0) < 1e-17
    if w == 1:
        assert (capi.feat_delta_scales(s, 1) == np.float32([-0.5, 0, 0.5])).all()
        assert (capi.feat_delta_scales(s, 2) == np.float32([0.25, 0, -0.5, 0, 0.25])).all()
    if w == 8:
        assert capi.feat_delta_scales(s, 3).shape == (49,) and capi.feat_delta_scales(s, 1)[-1] == np.float32(8 / 408)


def test_scales_capacities_and_orders(capi):
    L = capi.lib()
    s = make(capi, delta_order=2, delta_window=3)[0]
    buf = np.full(14, 7.0, dtype=np.float32)
    assert L.vpz_feat_delta_scales(C.byref(s), 2, None, 0) == capi.OK
    assert L.vpz_feat_delta_scales(C.byref(s), 2, buf.ctypes.data, 12) == capi.E_CAPACITY and (buf == 7.0).all()
    assert L.vpz_feat_delta_scales(C.byref(s), 2, buf.ctypes.data, 13) == capi.OK and buf[13] == 7.0 and buf[6] != 7.0
    for i in (-1, 3):
        assert L.vpz_feat_delta_scales(C.byref(s), i, None, 0) == capi.E_INVALID_ARG
        with pytest.raises(ValueError):
            capi.feat_delta_scales(s, i)
    assert L.vpz_feat_delta_scales(C.byref(s), 1, None, -1) == capi.E_INVALID_ARG and L.vpz_feat_delta_scales(None, 0, None, 0) == capi.E_INVALID_ARG


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("W", [1, 2, 300, 600])
def test_the_window_of_every_frame(capi, W, center):
    """every t of every n at min_window 1, 100 (where W allows it) and W: the library's [a, b) is the restatement's, 0 <= a < b <= n,
    t lies inside, c = min(n, W) with center and c <= W + 1 without, and both ends move by 0 or 1 from one frame to the next"""
    L = capi.lib()
    a, b = C.c_int64(0), C.c_int64(0)
    for minw in sorted({1, min(100, W), W}):
        s, d = make(capi, norm="sliding", center=center, cmn_window=W, min_window=minw)
        for n in NS:
            before = (0, 0)
            for t in range(n):
                assert L.vpz_feat_cmn_window(C.byref(s), t, n, C.byref(a), C.byref(b)) == capi.OK
                got = (a.value, b.value)
                assert got == pt.window(d, t, n), (n, W, minw, center, t)
                assert 0 <= got[0] < got[1] <= n and got[0] <= t < got[1]
                c = got[1] - got[0]
                assert c == min(n, W) if center else (c <= max(W + 1, minw) and c >= min(n, minw, t + 1))
                assert t == 0 or (0 <= got[0] - before[0] <= 1 and 0 <= got[1] - before[1] <= 1)
                before = got
    if not center and W == 300:  # the steady window of the uncentred rule has W + 1 frames
        assert capi.feat_cmn_window(make(capi, norm="sliding", cmn_window=300, min_window=100)[0], 700, 1300) == (400, 701)


def test_the_window_of_a_row_and_its_refusals(capi):
    L = capi.lib()
    row = make(capi, norm="row")[0]
    assert [capi.feat_cmn_window(row, t, 77) for t in (0, 40, 76)] == [(0, 77)] * 3
    a, b = C.c_int64(5), C.c_int64(5)
    none = make(capi, delta_order=1)[0]
    for spec, t, n in ((row, -1, 5), (row, 5, 5), (row, 0, 0), (none, 0, 5)):
        assert L.vpz_feat_cmn_window(C.byref(spec), t, n, C.byref(a), C.byref(b)) == capi.E_INVALID_ARG
        with pytest.raises(ValueError):
            capi.feat_cmn_window(spec, t, n)
    assert L.vpz_feat_cmn_window(C.byref(row), 0, 5, None, C.byref(b)) == capi.E_INVALID_ARG
    assert L.vpz_feat_cmn_window(C.byref(row), 0, 5, C.byref(a), None) == capi.E_INVALID_ARG
    assert L.vpz_feat_cmn_window(None, 0, 5, C.byref(a), C.byref(b)) == capi.E_INVALID_ARG and (a.value, b.value) == (5, 5)


def accepted_specs(capi):
    """at the limits themselves"""
    return [make(capi, **kw)[0] for kw in (
        dict(norm="row"), dict(delta_order=1), dict(delta_order=3, delta_window=8), dict(delta_order=1, delta_window=1),
        dict(norm="sliding", cmn_window=1, min_window=1), dict(norm="sliding", cmn_window=1 << 20, min_window=1 << 20),
        dict(norm="sliding", norm_vars=True, center=True, delta_order=3, deltas_first=True, frames_first=False, var_floor=5e-324, pad_value=-1e38))]


def test_every_limit_is_refused_by_every_entry_point(capi):
    L = capi.lib()
    cases = refused_specs(capi)
    assert len(cases) == 15 + 10 + 2
    buf = np.full(8, 7.0, dtype=np.float32)
    a, b, elems = C.c_int64(5), C.c_int64(5), C.c_int64(5)
    for what, spec in cases:
        assert L.vpz_feat_delta_scales(C.byref(spec), 0, buf.ctypes.data, 8) == capi.E_INVALID_ARG, what
        assert L.vpz_feat_cmn_window(C.byref(spec), 0, 5, C.byref(a), C.byref(b)) == capi.E_INVALID_ARG, what
        assert L.vpz_feat_post_scratch(C.byref(spec), 4, 100, 13, C.byref(elems)) == capi.E_INVALID_ARG, what
        with pytest.raises(ValueError):
            capi.feat_post_scratch(spec, 4, 100, 13)
    assert (buf == 7.0).all() and (a.value, b.value, elems.value) == (5, 5, 5)
    for spec in accepted_specs(capi):
        assert L.vpz_feat_post_scratch(C.byref(spec), 4, 100, 13, C.byref(elems)) == capi.OK
    # vpz_feat_post without a context (its other refusals need a device: tests/test_pcm_featpost_gpu.py)
    good = make(capi, norm="row")[0]
    assert L.vpz_feat_post(None, None, 0, 10, 13, C.byref(good), 0, None, None, 0, None, 0) == capi.E_INVALID_ARG


def test_the_scratch_size(capi):
    """2 float64 per (descriptor, chunk of 64 frames, normalised column); none without a normalisation; the deltas' columns count only
    behind the deltas; sizes beyond 63 bits of bytes, D outside 1 .. 256, T < 1 and a negative count are refused"""
    L = capi.lib()
    ceil = lambda T: (T + 63) // 64  # noqa: E731
    for T in (1, 63, 64, 65, 3000):
        assert capi.feat_post_scratch(make(capi, norm="row")[0], 7, T, 13) == 2 * 7 * ceil(T) * 13
        assert capi.feat_post_scratch(make(capi, norm="sliding", delta_order=2)[0], 7, T, 13) == 2 * 7 * ceil(T) * 13
        assert capi.feat_post_scratch(make(capi, norm="sliding", delta_order=2, deltas_first=True)[0], 7, T, 13) == 2 * 7 * ceil(T) * 39
        assert capi.feat_post_scratch(make(capi, delta_order=3)[0], 7, T, 13) == 0
    row = make(capi, norm="row")[0]
    assert capi.feat_post_scratch(row, 0, 100, 256) == 0 and capi.feat_post_scratch(row, 1, 1, 1) == 2
    assert capi.feat_post_scratch(row, 2 ** 31 - 1, 64 * 2 ** 20, 256) == 2 * (2 ** 31 - 1) * 2 ** 20 * 256  # 2^60 elements: 2^63 bytes less some
    elems = C.c_int64(5)
    for n_rows, T, D in ((-1, 100, 13), (1, 0, 13), (1, 100, 0), (1, 100, 257), (2 ** 31 - 1, 64 * 2 ** 21, 256)):
        assert L.vpz_feat_post_scratch(C.byref(row), n_rows, T, D, C.byref(elems)) == capi.E_INVALID_ARG, (n_rows, T, D)
    assert L.vpz_feat_post_scratch(C.byref(row), 1, 100, 13, None) == capi.E_INVALID_ARG and elems.value == 5
    # the bound the header gives: O(rows * ceil(T / 64) * D) doubles, an eighth of the tensor's bytes at most past the last chunk
    assert capi.feat_post_scratch(make(capi, norm="sliding", delta_order=2, deltas_first=True)[0], 64, 3000, 13) * 8 <= 64 * 3008 * 39 * 4 // 8


def test_the_spec_helper_has_kaldis_defaults(capi):
    s = capi.FeatPostSpec.make()
    assert (s.norm, s.norm_vars, s.center, s.cmn_window, s.min_window, s.var_floor, s.delta_order, s.delta_window, s.order, s.layout, s.pad_value) == \
        (capi.NORM_NONE, 0, 0, 600, 100, 1e-10, 0, 2, capi.POST_NORM_FIRST, capi.FEAT_FRAMES_FIRST, 0.0)
    made = inspect.signature(capi.FeatPostSpec.make)
    assert {k: p.default for k, p in made.parameters.items() if k != "cls"} == pt.DEFAULTS
    assert capi.FeatPostSpec.make(delta_order=2).out_columns(13) == 39
    with pytest.raises(ValueError):
        capi.FeatPostSpec.make(norm="global")


# ---- the surface
def test_the_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_featpost.h", "vpz_")
    imports = imports_of(tmp_path, "GpuFeatPost.cs")
    assert sorted(c) == ["vpz_feat_cmn_window", "vpz_feat_delta_scales", "vpz_feat_post", "vpz_feat_post_scratch"] == sorted(imports) \
        == sorted(capi.PCM_FEATPOST_EXPORTED_SYMBOLS)
    assert c["vpz_feat_post"] == ("i32", ["ptr", "ptr", "i64", "i64", "i32", "ptr", "i32", "ptr", "ptr", "i64", "ptr", "i64"])
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_FEATPOST_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    structs, defines = cs.c_structs("vorbispizza_pcm_featpost.h")
    cs_structs = cs.cs_structs(os.path.join(cs.CS, "GpuFeatPost.cs"))
    assert sorted(structs) == ["vpz_feat_post_spec", "vpz_feat_row"] and sorted(cs_structs) == ["FeatPostSpec", "FeatRow"]
    py_spec = [(n, {C.c_double: "f64"}.get(t, "i32"), getattr(t, "_length_", 0)) for n, t in capi.FeatPostSpec._fields_]
    assert len(structs["vpz_feat_post_spec"]) == len(cs_structs["FeatPostSpec"]) == len(py_spec) == 12
    for (n0, k0, a0), (n1, k1, a1), (n2, k2, a2) in zip(structs["vpz_feat_post_spec"], cs_structs["FeatPostSpec"], py_spec):
        assert cs.norm(n0) == cs.norm(n1) == cs.norm(n2) and k0 == k1 == k2 and a0 == a1 == a2, (n0, n1, n2)
    assert structs["vpz_feat_row"] == [("src_row", "i64", 0), ("real_frames", "i64", 0), ("row", "i64", 0)]
    assert [(cs.norm(n), k, a) for n, k, a in cs_structs["FeatRow"]] == [(cs.norm(n), k, a) for n, k, a in structs["vpz_feat_row"]]
    assert C.sizeof(capi.FeatPostSpec) == 2 * 8 + 9 * 4 + 11 * 4 == 96 and capi.PACK_ROW_DTYPE.itemsize == 24
    # the constants: header, C# and Python
    text = cs.strip_cs_comments(open(os.path.join(cs.CS, "GpuFeatPost.cs")).read())
    consts = {}
    for m in re.finditer(r"public\s+const\s+int\s+([^;]+);", text):
        for part in m.group(1).split(","):
            k, v = part.split("=")
            shifted = re.fullmatch(r"\s*(\d+)\s*<<\s*(\d+)\s*", v)
            consts[cs.norm(k.strip())] = int(shifted.group(1)) << int(shifted.group(2)) if shifted else int(v.strip(), 0)
    mine = {k: v for k, v in defines.items() if k.startswith("VPZ_")}
    assert len(mine) == 11 and "VPZ_FEAT_MAX_CMN_WINDOW" not in mine  # (an expression: the parser takes literals)
    for name, value in dict(mine, VPZ_FEAT_MAX_CMN_WINDOW=1 << 20).items():
        assert consts[cs.norm(name[4:])] == value == getattr(capi, name[4:]), name
    fb = cs.c_structs("vorbispizza_pcm_fbank.h")[1]
    assert (mine["VPZ_FEAT_COLUMNS_FIRST"], mine["VPZ_FEAT_FRAMES_FIRST"]) == (fb["VPZ_FBANK_BANDS_FIRST"], fb["VPZ_FBANK_FRAMES_FIRST"])
    # the older headers and their lists did not take the new names
    older = (capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_RESAMPLE_EXPORTED_SYMBOLS
             + capi.PCM_LOGMEL_EXPORTED_SYMBOLS + capi.PCM_FBANK_EXPORTED_SYMBOLS + capi.PCM_MFCC_EXPORTED_SYMBOLS)
    for name in c:
        assert name not in older and name not in cs.c_functions("vorbispizza_pcm_mfcc.h", "vpz_")


def test_the_call_binding_matches_its_header(tmp_path, capi):
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_featpost.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiFeatPost.cs")
    assert sorted(c) == ["vpzm_decode_ranges_fbank_post", "vpzm_decode_ranges_mfcc_post"] == sorted(imports) == sorted(multi.FEATPOST_EXPORTED_SYMBOLS)
    # the existing calls' parameters with the post spec behind the feature spec
    for name, header, old in (("vpzm_decode_ranges_fbank_post", "vorbispizza_multi_fbank.h", "vpzm_decode_ranges_fbank"),
                              ("vpzm_decode_ranges_mfcc_post", "vorbispizza_multi_mfcc.h", "vpzm_decode_ranges_mfcc")):
        ret, params = cs.c_functions(header, "vpzm_")[old]
        assert c[name] == (ret, params[:6] + ["ptr"] + params[6:]) and len(c[name][1]) == 11
        assert imports[name] == ("Host",) + c[name]
        fn = getattr(multi.lib(), name)
        assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c[name][1] and KINDS[fn.restype] == "i32"
    assert cs.c_structs("vorbispizza_multi_featpost.h")[0] == {}
    text = open(os.path.join(cs.CS, "VorbisPizzaMultiFeatPost.cs")).read()
    assert "GpuFeatPost.FeatPostSpec* post, long frames" in text and "GpuPcmMfcc.MfccSpec* spec" in text and "GpuPcmFbank.FbankSpec* spec" in text
    # the Python methods: the feature spec's names pass through, `post` None is the call without it
    for method, rest in ((multi.Dispatcher.decode_ranges_fbank_post, "fbank"), (multi.Dispatcher.decode_ranges_mfcc_post, "mfcc")):
        sig = inspect.signature(method)
        assert list(sig.parameters) == ["self", "datas", "ranges", "frames", "post", "out", rest]
        assert sig.parameters["post"].default is None and sig.parameters["out"].default is None
        assert sig.parameters[rest].kind is inspect.Parameter.VAR_KEYWORD
    # the calls without a post spec keep their signatures
    assert "post" not in inspect.signature(multi.Dispatcher.decode_ranges_mfcc).parameters
    assert "post" not in inspect.signature(multi.Dispatcher.decode_ranges_fbank).parameters


def test_the_library_exports_the_new_symbols(capi):
    from vorbispizza_amd import _build, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in multi.FEATPOST_EXPORTED_SYMBOLS:
        assert hasattr(H, name) and not hasattr(S, name), name
    for name in capi.PCM_FEATPOST_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert "pcm_featpost.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "pcm_featpost.hip"))
    assert callable(capi.feat_post) and callable(capi.feat_delta_scales) and callable(capi.feat_cmn_window)


def test_the_new_header_is_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    body = ("sizeof(vpz_feat_post_spec) == 96 && sizeof(vpz_feat_row) == 24 && sizeof(vpz_feat_row) == sizeof(vpz_pack_row) && "
            "VPZ_FEAT_MAX_CMN_WINDOW == 1048576 && VPZ_NORM_SLIDING == 2")
    src = tmp_path / "featpost.c"
    src.write_text('#include "vorbispizza_pcm_featpost.h"\n#include "vorbispizza_pcm_pack.h"\ntypedef char holds[(%s) ? 1 : -1];\n'
                   'int main(void) { return (int)sizeof(holds) - 1; }\n' % body)
    exe = tmp_path / "featpost.exe"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
    src.write_text('#include "vorbispizza_multi_featpost.h"\ntypedef char holds[(sizeof(vpz_feat_post_spec) == 96 && VPZM_E_ARG < 0 && '
                   'VPZ_FEAT_FRAMES_FIRST == VPZ_FBANK_FRAMES_FIRST && VPZ_FEAT_COLUMNS_FIRST == VPZ_FBANK_BANDS_FIRST) ? 1 : -1];\n'
                   'int main(void) { return (int)sizeof(holds) - 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_the_kernels_use_no_scratch_and_say_what_they_take():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = kr.analyse(os.path.join(_build.CSRC, "pcm_featpost.hip"), _build.SOURCES["pcm_featpost.hip"])
    names = ("featpost_chunk_kernel", "featpost_apply_kernel", "featpost_slide_kernel")
    assert sorted(name for k in ks for name in names if name in k["name"]) == sorted(names) and len(ks) == 3
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k.get("vgpr_spill", 0) == 0, k
        # LDS, 33 floats a frame (32 columns and one of padding): a tile's or a region's source frames with a halo of 24 to either side
        # beside the values -- the chunk kernel's one chunk, the sliding kernel's four chunks and its tile (two workgroups of it on a
        # CU; dynamic, so the kernel itself reports none, and without the delta view the launch asks for the values alone: three), the
        # apply kernel's 32 sums
        kind = k["name"].split("featpost_")[1].split("_kernel")[0]
        assert k["lds"] == {"chunk": 4 * 33 * (64 + 112), "slide": 0, "apply": 4 * 33 * 112 + 16 * 32}[kind], k
        text = open(os.path.join(_build.CSRC, "pcm_featpost.hip")).read()
        assert "return sizeof(float) * kSlStride * (size_t)(kSlRows + (view ? kRegionStage : 0));" in text
        assert 4 * 33 * (320 + 176) <= 65536  # (what a launch may ask for without raising the kernel's limit)
        assert k["vgprs"] + k.get("agprs", 0) <= 128 and k["occupancy"] >= 2, k


# ---- the truth itself
def proxy(x, d):
    """a float32 / float64 proxy of the definition with OTHER orders than the library's: the delta as a float32 multiply and add per step,
    descending; the window sums as numpy's pairwise float64 sums"""
    n, D = x.shape
    if d["norm"] == "none":
        out = [x]
        t = np.arange(n)
        for i in range(1, d["delta_order"] + 1):
            s, H = pt.scales(i, d["delta_window"]).astype(np.float32), i * d["delta_window"]
            acc = np.zeros((n, D), np.float32)
            for j in range(H, -H - 1, -1):
                acc = acc + s[j + H] * x[np.clip(t + j, 0, n - 1)]
            out.append(acc)
        return np.concatenate(out, axis=1)
    out = np.zeros((n, D), np.float32)
    for t in range(n):
        a, b = pt.window(d, t, n)
        seg = x[a:b].astype(np.float64)
        m = seg.sum(axis=0) / (b - a)
        if not d["norm_vars"]:
            out[t] = x[t] - m
        elif b - a == 1:
            out[t] = 0
        else:
            out[t] = (x[t] - m) / np.sqrt(np.maximum((seg * seg).sum(axis=0) / (b - a) - m * m, d["var_floor"]))
    return out


CASES = [dict(delta_order=3, delta_window=2), dict(delta_order=2, delta_window=8), dict(norm="row"), dict(norm="row", norm_vars=True),
         dict(norm="sliding", cmn_window=30, min_window=10), dict(norm="sliding", cmn_window=30, min_window=10, norm_vars=True, center=True)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_bound_discriminates(case):
    """a proxy in the library's number formats but other orders stays inside the bound -- on noise, and on a column whose mean is 500 times
    its deviation, where the bound stays below 2^-20 of the deviation (not vacuous) --; one scale 1e-5 off, or a mean taken in float32,
    leaves it on most elements"""
    d = pt.spec_of(**CASES[case])
    rng = np.random.default_rng(40 + case)
    noise = rng.standard_normal((150, 5)).astype(np.float32)
    dc = (500.0 + rng.standard_normal((150, 5))).astype(np.float32)
    for x in (noise, dc):
        want, bound = pt.truth(x, d)
        r = pt.ratio(proxy(x, d), want, bound)
        print("proxy error / bound %.3f" % r)
        assert r <= 1.0
    want, bound = pt.truth(dc, d)
    if d["norm"] == "none":
        assert (bound[:, :5] == 0).all() and (want[:, :5] == dc).all()
        want, bound = pt.truth(noise, d)
        off = proxy(noise, d)[:, 5:10].astype(np.float64) * (1 + 1e-5)
        assert (np.abs(off - want[:, 5:10]) > bound[:, 5:10]).mean() > 0.5
    else:
        scale = 1.0 if d["norm_vars"] else float(np.std(dc))
        assert float(bound.max()) < 2.0 ** -20 * scale
        m32 = dc - dc.mean(axis=0, dtype=np.float32) if d["norm"] == "row" and not d["norm_vars"] else None
        if m32 is not None:
            assert (np.abs(m32 - want) > bound).mean() > 0.5
