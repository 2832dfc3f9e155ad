"""vpz_mfcc_table (include/vorbispizza_pcm_mfcc.h, csrc/mfcc_tables.hpp) without a device, every refusal of the spec, what a clean
checkout must hold about the new headers and bindings, and the launch plan of vpz_pcm_mfcc.

The truth is tests/mfcc_truth.py: the header's definition in float64, unfolded (an explicit DCT, the lifter behind it)."""
import ctypes as C
import inspect
import math
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

import fbank_truth as ft  # noqa: E402
import mfcc_truth as mt  # noqa: E402
import binding_support as cs  # noqa: E402
from fbank_truth import U  # noqa: E402
from binding_support import imports_of  # noqa: E402
from mfcc_truth import make, refused_specs  # noqa: E402

KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


# ---- the table
@pytest.mark.parametrize("use_energy", [False, True])
@pytest.mark.parametrize("htk_compat", [False, True])
@pytest.mark.parametrize("lifter", [22.0, 0.0, 5.5])
def test_the_table_is_the_double_restatement_rounded_once(capi, lifter, htk_compat, use_energy):
    """within one float32 ulp (2 u |v|) of the unfolded float64 value -- DCT, then lifter, then sqrt(2) --, in the stored order: rows 0 and
    n_ceps - 1, the sqrt(2) row and Q = 0 among them"""
    for n_mels, n_ceps in ((23, 13), (23, 23), (23, 1), (256, 256), (1, 1), (40, 2)):
        spec, d = make(capi, n_mels=n_mels, n_ceps=n_ceps, lifter=lifter, htk_compat=htk_compat, use_energy=use_energy,
                       **(dict(n_fft=1024, win=1024, hop=512, sample_rate=48000) if n_mels == 256 else {}))
        table = capi.mfcc_table(spec)
        assert table.shape == (n_ceps, n_mels) and table.dtype == np.float32
        want = mt.matrix64(d)[mt.stored_order(d)]
        assert (np.abs(table.astype(np.float64) - want) <= 2 * U * np.abs(want) + 2.0 ** -60).all(), (n_mels, n_ceps)
        c0 = n_ceps - 1 if htk_compat else 0  # where C[0] is stored
        flat = math.sqrt(1.0 / n_mels) * (math.sqrt(2.0) if htk_compat and not use_energy else 1.0)
        assert np.abs(table[c0].astype(np.float64) - flat).max() <= 2 * U * flat
        if n_ceps > 1:
            i = n_ceps - 1
            last = n_ceps - 2 if htk_compat else n_ceps - 1  # where C[n_ceps - 1] is stored
            lift = 1.0 + 0.5 * lifter * math.sin(math.pi * i / lifter) if lifter > 0 else 1.0
            row = lift * math.sqrt(2.0 / n_mels) * np.cos(math.pi * i * (np.arange(n_mels) + 0.5) / n_mels)
            assert np.abs(table[last].astype(np.float64) - row).max() <= 2 * U * np.abs(row).max() + 2.0 ** -60


def test_the_dct_is_orthonormal_and_a_constant_has_one_cepstrum(capi):
    for N in (1, 2, 23, 80, 256):
        D = mt.dct64(N, N)
        assert np.abs(D @ D.T - np.eye(N)).max() < 1e-12
        spec, d = make(capi, n_mels=N, n_ceps=N, lifter=0.0, use_energy=False, **(dict(n_fft=1024, win=1024, hop=512) if N > 128 else {}))
        c = capi.mfcc_table(spec).astype(np.float64) @ np.full(N, -3.25)
        assert abs(c[0] - math.sqrt(N) * -3.25) < 1e-5 * math.sqrt(N) and (N == 1 or np.abs(c[1:]).max() < 1e-4)


def test_sizing_calls_and_capacities(capi):
    L = capi.lib()
    spec, _ = make(capi)
    n = 13 * 23
    assert L.vpz_mfcc_table(C.byref(spec), None, 0) == capi.OK
    buf = np.full(n + 1, 7.0, dtype=np.float32)
    assert L.vpz_mfcc_table(C.byref(spec), buf.ctypes.data, n - 1) == capi.E_CAPACITY and (buf == 7.0).all()
    assert L.vpz_mfcc_table(C.byref(spec), buf.ctypes.data, n) == capi.OK and buf[-1] == 7.0 and (buf[:-1] != 7.0).all()


def test_every_limit_is_refused(capi):
    L = capi.lib()
    buf = np.full(8, 7.0, dtype=np.float32)
    cases = refused_specs(capi)
    assert len(cases) > 50
    for what, spec in cases:
        assert L.vpz_mfcc_table(C.byref(spec), None, 0) == capi.E_INVALID_ARG, what
        assert L.vpz_mfcc_table(C.byref(spec), buf.ctypes.data, 1 << 40) == capi.E_INVALID_ARG, what
        with pytest.raises(ValueError):
            capi.mfcc_table(spec)
    assert (buf == 7.0).all()
    good = make(capi)[0]
    assert L.vpz_mfcc_table(None, None, 0) == capi.E_INVALID_ARG and L.vpz_mfcc_table(C.byref(good), None, -1) == capi.E_INVALID_ARG
    # vpz_pcm_mfcc without a context (its other refusals need a device: tests/test_pcm_mfcc_gpu.py)
    assert L.vpz_pcm_mfcc(None, None, 0, 400, C.byref(good), 0, None, None, 0) == capi.E_INVALID_ARG
    # at the limits themselves: accepted
    for kw in (dict(n_ceps=1), dict(n_ceps=23), dict(n_mels=256, n_ceps=256, n_fft=1024), dict(n_mels=1, n_ceps=1), dict(lifter=0.0), dict(lifter=1e6),
               dict(energy_floor=1e30), dict(use_energy=False, htk_compat=True, subtract_mean=True), dict(n_fft=32, win=2, hop=1)):
        capi.mfcc_table(make(capi, **kw)[0])


def test_the_spec_helper_has_kaldis_defaults(capi):
    s = capi.MfccSpec.make()
    assert [s.n_frames(F) for F in (0, 399, 400, 559, 560, 16000)] == [0, 0, 1, 1, 2, 98]
    f = s.fbank
    assert (f.sample_rate, f.win, f.hop, f.n_fft, f.n_mels, f.low_freq, f.high_freq, f.preemphasis, f.window, f.remove_dc, f.scale, f.output, f.floor,
            f.pad_value, f.layout) == (16000.0, 400, 160, 512, 23, 20.0, 0.0, 0.97, capi.FBANK_POVEY, 1, 32768.0, capi.FBANK_LOG, 2.0 ** -23, 0.0,
                                       capi.FBANK_FRAMES_FIRST)
    assert (s.n_ceps, s.lifter, s.use_energy, s.energy_floor, s.htk_compat, s.subtract_mean) == (13, 22.0, 1, 0.0, 0, 0)
    made = inspect.signature(capi.MfccSpec.make)
    assert {k: p.default for k, p in made.parameters.items() if k != "cls"} == mt.DEFAULTS


# ---- the surface
def flattened(tmp_path, path, old, new):
    """a copy of a header or binding with its nested fbank spec as 128 bytes, for the parsers of test_csharp_binding_cpu.py"""
    text = open(path).read()
    assert text.count(old) == 1, (path, old)
    out = tmp_path / os.path.basename(path)
    out.write_text(text.replace(old, new))
    return str(out)


def test_the_mfcc_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_mfcc.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmMfcc.cs")
    assert sorted(c) == ["vpz_mfcc_table", "vpz_pcm_mfcc"] == sorted(imports) == sorted(capi.PCM_MFCC_EXPORTED_SYMBOLS)
    # vpz_pcm_fbank's parameters, the spec of the other kind in the same place
    assert c["vpz_pcm_mfcc"] == cs.c_functions("vorbispizza_pcm_fbank.h", "vpz_")["vpz_pcm_fbank"]
    assert c["vpz_mfcc_table"] == ("i32", ["ptr", "ptr", "i64"])
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_MFCC_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    header = flattened(tmp_path, os.path.join(cs.INC, "vorbispizza_pcm_mfcc.h"), "vpz_fbank_spec fbank;", "uint8_t fbank[128];")
    structs, defines = cs.c_structs(header)
    assert sorted(structs) == ["vpz_mfcc_spec"] and not [k for k in defines if k.startswith("VPZ_")]
    binding = flattened(tmp_path, os.path.join(cs.CS, "GpuPcmMfcc.cs"), "public GpuPcmFbank.FbankSpec Fbank;", "public fixed byte Fbank[128];")
    cs_fields = cs.cs_structs(binding)["MfccSpec"]
    py_fields = [(n, {C.c_double: "f64", C.c_int32: "i32", capi.FbankSpec: "u8"}.get(t, "i32"), C.sizeof(t) if t is capi.FbankSpec else getattr(t, "_length_", 0))
                 for n, t in capi.MfccSpec._fields_]
    assert len(structs["vpz_mfcc_spec"]) == len(cs_fields) == len(py_fields) == 8
    for (n0, k0, a0), (n1, k1, a1), (n2, k2, a2) in zip(structs["vpz_mfcc_spec"], cs_fields, py_fields):
        assert cs.norm(n0) == cs.norm(n1) == cs.norm(n2) and k0 == k1 == k2 and a0 == a1 == a2, (n0, n1, n2)
    assert C.sizeof(capi.MfccSpec) == 128 + 2 * 8 + 4 * 4 + 12 * 4 == 208 and capi.MfccSpec.lifter.offset == 128
    # the older headers and their lists did not take the new names
    for name in c:
        assert name not in (capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_RESAMPLE_EXPORTED_SYMBOLS
                            + capi.PCM_LOGMEL_EXPORTED_SYMBOLS + capi.PCM_FBANK_EXPORTED_SYMBOLS)
        assert name not in cs.c_functions("vorbispizza_synth.h", "vpz_") and name not in cs.c_functions("vorbispizza_pcm_fbank.h", "vpz_")


def test_the_mfcc_call_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_mfcc.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiMfcc.cs")
    assert sorted(c) == ["vpzm_decode_ranges_mfcc"] == sorted(imports) == sorted(multi.MFCC_EXPORTED_SYMBOLS)
    # the fbank call's parameters, the spec of the other kind in the same place
    assert c["vpzm_decode_ranges_mfcc"] == cs.c_functions("vorbispizza_multi_fbank.h", "vpzm_")["vpzm_decode_ranges_fbank"]
    assert imports["vpzm_decode_ranges_mfcc"] == ("Host",) + c["vpzm_decode_ranges_mfcc"]
    fn = multi.lib().vpzm_decode_ranges_mfcc
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_decode_ranges_mfcc"][1] and KINDS[fn.restype] == "i32"
    assert cs.c_structs("vorbispizza_multi_mfcc.h")[0] == {}
    sig = inspect.signature(multi.Dispatcher.decode_ranges_mfcc)
    assert list(sig.parameters) == ["self", "datas", "ranges", "frames"] + list(mt.DEFAULTS) + ["out"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert {k: d[k] for k in mt.DEFAULTS} == mt.DEFAULTS and d["out"] is None


def test_both_libraries_export_the_new_symbols(capi):
    from vorbispizza_amd import _build, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in capi.PCM_MFCC_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert hasattr(H, "vpzm_decode_ranges_mfcc") and not hasattr(S, "vpzm_decode_ranges_mfcc")
    assert os.path.exists(os.path.join(_build.CSRC, "mfcc_tables.hpp"))
    assert callable(capi.pcm_mfcc) and callable(capi.mfcc_table) and callable(multi.Dispatcher.decode_ranges_mfcc)


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    for header, body in (("vorbispizza_pcm_mfcc.h", "sizeof(vpz_mfcc_spec) == 208 && sizeof(vpz_fbank_spec) == 128 && VPZ_FBANK_LOG == 1"),
                         ("vorbispizza_multi_mfcc.h", "VPZM_E_RATE == -16 && sizeof(vpz_mfcc_spec) == 208 && VPZ_FBANK_FRAMES_FIRST == 1")):
        src = tmp_path / (header + ".c")
        src.write_text('#include "%s"\ntypedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % (header, body))
        exe = tmp_path / (header + ".exe")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


def test_the_kernels_use_no_scratch_and_say_what_they_take():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = kr.analyse(os.path.join(_build.CSRC, "pcm_fbank.hip"), _build.SOURCES["pcm_fbank.hip"])
    count = {name: len([k for k in ks if name in k["name"]]) for name in ("pcm_mfcc_kernel", "pcm_cmn_kernel", "pcm_fbank_kernel")}
    assert count == {"pcm_mfcc_kernel": 2, "pcm_cmn_kernel": 1, "pcm_fbank_kernel": 2} and len(ks) == 5
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k.get("vgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 512 and k["occupancy"] >= 1, k


# ---- the launch plan
def test_a_tile_of_sixteen_frames_fits_at_any_spec():
    """mfcc_lds_plan restated (tests/mfcc_truth.py) against the source's statement of it, and swept over the limits: n_fft 32 / 1024,
    win 2 / n_fft, hop 1 / win, n_mels 1 / 256 (n_ceps takes no LDS): 16 frames always fit, so VPZ_E_UNSUPPORTED cannot be reached"""
    k = ft.kernel_constants(ROOT)
    text = open(os.path.join(ROOT, "vorbispizza_amd", "csrc", "pcm_fbank.hip")).read()
    body = text[text.index("int mfcc_lds_plan("):]
    body = body[: body.index("\n}")]
    assert "lds_plan(s, Tt, span_cap, pstride);" in body and "*estride = s.n_mels | 1;" in body
    assert "return *span_cap + 2 * kFbMeans + Tt * *pstride + Tt * *estride;" in body
    assert "*en = mean + kFbMeans, *pw = CEP ? en + kFbMeans : en, *et = pw + a.Tt * a.pstride" in text
    largest = 0
    for n_fft in (32, 1024):
        for win in (2, n_fft):
            for hop in (1, win):
                for n_mels in (1, 256):
                    for n_ceps in (1, n_mels):
                        total, estride = mt.mfcc_lds_plan(win, hop, n_fft, n_mels, 16, k)
                        span_cap, pstride = ft.lds_plan(win, hop, n_fft, 16)
                        assert total == span_cap + 128 + 16 * pstride + 16 * estride and estride % 2 == 1 and estride >= n_mels
                        assert total <= k["kFbLdsFloats"], (n_fft, win, hop, n_mels)
                        largest = max(largest, total)
                        assert mt.tile_plan(win, hop, n_fft, n_mels, 1000, 1000, 256, k)[0] in (64, 32, 16)
    assert largest == 16 * 1024 + 16 + 1 + 128 + 16 * 513 + 16 * 257  # (win = hop = n_fft = 1024, 256 bands)
    # the defaults: the tiles of vpz_pcm_fbank at the same launch sizes
    assert [mt.tile_plan(400, 160, 512, 23, T, n, 256, k)[0] for T, n in ((16, 1), (17, 1), (98, 5), (98, 255), (98, 256), (32, 1000), (33, 1000))] == \
        [16, 32, 32, 32, 64, 32, 64]
    # the log-mel tile costs frames where the LDS decides: n_fft = win = 1024 with 256 bands
    assert [mt.tile_plan(1024, hop, 1024, 256, 104, 600, 256, k)[0] for hop in (1, 111, 112, 755, 756, 1024)] == [32, 32, 32, 16, 16, 16]


# ---- the truth itself
def proxy32(x, d, C32, centre_first=True):
    """a float32 proxy of the stated orders: the log-mel values from the float64 band sums rounded to float32, the chain as a float32
    multiply and add per step (no better than the fused one), the energy as four float32 chains over fl(x - mu)"""
    fb = mt.fbank_of(d)
    M, _ = ft.fbank_truth(x, fb)
    E = np.log(np.maximum(M, d["floor"])).astype(np.float32)
    c = np.zeros((E.shape[0], C32.shape[0]), np.float32)
    for b in range(E.shape[1]):
        c = c + C32[None, :, b] * E[:, b:b + 1]
    if d["use_energy"]:
        X = ft.frames_of(x, d["win"], d["hop"]).astype(np.float32)
        s = [np.zeros(X.shape[0], np.float32) for _ in range(4)]
        for q in range(4):
            for j in range(q, d["win"], 4):
                s[q] = s[q] + X[:, j]
        mu = ((s[0] + s[1]) + (s[2] + s[3])) / np.float32(d["win"])
        A = X - mu[:, None] if centre_first else X
        s = [np.zeros(X.shape[0], np.float32) for _ in range(4)]
        for q in range(4):
            for j in range(q, d["win"], 4):
                s[q] = s[q] + A[:, j] * A[:, j]
        S = np.float32(d["scale"]) * np.float32(d["scale"]) * ((s[0] + s[1]) + (s[2] + s[3]))
        c[:, 0] = np.log(np.maximum(S, np.float32(2.0 ** -23)))
    return c


def test_the_bound_discriminates():
    """the float32 proxy stays far inside the bound on plain noise and under a DC offset of 500 times the signal; one table row 5 % off
    leaves it on most outputs of that row, and so does an energy taken before the mean is removed, under the DC offset"""
    rng = np.random.default_rng(12)
    d = mt.spec_of(win=96, hop=17, n_fft=128, n_mels=13, n_ceps=9, sample_rate=8000, low_freq=100.0, high_freq=-200.0, scale=32768.0)
    C32 = mt.matrix64(d).astype(np.float32)
    noise = (0.5 * rng.standard_normal(900)).astype(np.float32)
    dc = (0.5 + 1e-3 * rng.standard_normal(900)).astype(np.float32)
    for x in (noise, dc):
        V, b = mt.mfcc_truth(x, d)
        worst = float((np.abs(proxy32(x, d, C32) - V) / b).max())
        print("proxy error / bound %.3f" % worst)
        assert worst <= 0.5
        out, ob = mt.cmn_truth(V, b)
        p = proxy32(x, d, C32).astype(np.float64)
        assert (np.abs((p - p.mean(axis=0)).astype(np.float32) - out) <= 0.5 * ob).all()
    off = C32.copy()
    off[5] *= np.float32(1.05)
    V, b = mt.mfcc_truth(noise, d)
    assert (np.abs(proxy32(noise, d, off)[:, 5] - V[:, 5]) > b[:, 5]).mean() > 0.5
    assert (np.abs(proxy32(noise, d, off)[:, 4] - V[:, 4]) <= b[:, 4]).all()
    V, b = mt.mfcc_truth(dc, d)
    assert (np.abs(proxy32(dc, d, C32, centre_first=False)[:, 0] - V[:, 0]) > b[:, 0]).mean() > 0.5
