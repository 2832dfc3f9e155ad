"""vpz_fbank_table and vpz_fbank_filterbank (include/vorbispizza_pcm_fbank.h, csrc/fbank_tables.hpp) without a device, every refusal of
the host entry points, what a clean checkout must hold about the new headers and bindings, and the launch plan of vpz_pcm_fbank.

The truth is tests/fbank_truth.py: the header's definition in float64, unfolded.  The library's folded table is held to that unfolded
operator applied to unit impulses, within one float32 rounding; the mel bank to the dense W."""
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

import fbank_truth as ft  # noqa: E402
import binding_support as cs  # noqa: E402
from fbank_truth import make, refused_specs, U  # noqa: E402
from binding_support import imports_of  # noqa: E402

KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}
# (sample_rate, n_fft, n_mels, low_freq, high_freq)
BANKS = [(16000, 512, 23, 20.0, 0.0), (16000, 512, 80, 20.0, 0.0), (16000, 512, 23, 20.0, -400.0), (16000, 512, 80, 20.0, -400.0),
         (8000, 256, 40, 0.0, 0.0)]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


# ---- the tables
@pytest.mark.parametrize("scale", [1.0, 32768.0])
@pytest.mark.parametrize("c", [0.0, 0.97, 1.0])
@pytest.mark.parametrize("window", ft.WINDOWS)
def test_the_table_is_the_unfolded_operator_on_unit_impulses(capi, window, c, scale):
    """|t - v| <= u |v| for one float32 rounding of the float64 value v.  v itself is the sum of at most three products of a window value
    with a cos or sin, each a few float64 roundings of a value of magnitude <= 1 (the library reduces the angle in integers, rfft does not
    evaluate one at all): 16 * 2^-52 * scale is allowed for that."""
    for win, n_fft in ((2, 32), (2, 1024), (400, 400), (400, 512), (551, 552), (551, 1024), (1024, 1024)):
        spec, d = make(capi, win=win, hop=max(1, win // 3), n_fft=n_fft, window=window, preemphasis=c, scale=scale, n_mels=4, sample_rate=48000)
        table = capi.fbank_table(spec)
        assert table.shape == (win, 2, n_fft // 2) and table.dtype == np.float32
        for got, want in zip((table[:, 0], table[:, 1]), ft.operator64(d)):
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= U * np.abs(want) + 16 * 2.0 ** -52 * scale).all(), (win, n_fft, float(err.max()))
        assert (table[:, 1, 0].view(np.uint32) << 1 == 0).all()  # (bin 0 has no sin part)
        assert win == 2 or np.abs(table).max() > 0.01 * scale  # (a Hanning window of two points is two zeros)


def test_the_table_in_closed_form_at_two_points(capi):
    """win 2, Hamming (w = 0.08, 0.08 at both ends -- cos(0) and cos(2 pi)): z[0] = (1 - c) y[0], z[1] = y[1] - c y[0], so
    B[0][k] = w (1 - c) - c w cos(2 pi k / n_fft), B[1][k] = w cos(2 pi k / n_fft)"""
    c, n_fft = 0.5, 32
    spec, d = make(capi, win=2, hop=1, n_fft=n_fft, window="hamming", preemphasis=c, scale=1.0, n_mels=1)
    table = capi.fbank_table(spec).astype(np.float64)
    k = np.arange(n_fft // 2)
    w = 0.54 - 0.46
    assert np.abs(table[0, 0] - (w * (1 - c) - c * w * np.cos(2 * np.pi * k / n_fft))).max() < 1e-8
    assert np.abs(table[1, 0] - w * np.cos(2 * np.pi * k / n_fft)).max() < 1e-8
    assert np.abs(table[0, 1] + c * w * np.sin(2 * np.pi * k / n_fft)).max() < 1e-8
    assert np.abs(table[1, 1] - w * np.sin(2 * np.pi * k / n_fft)).max() < 1e-8


@pytest.mark.parametrize("bank", BANKS)
def test_the_filterbank_is_the_dense_w_rounded_once(capi, bank):
    sr, n_fft, n_mels, low, high = bank
    spec, d = make(capi, sample_rate=sr, n_fft=n_fft, win=min(400, n_fft), hop=100, n_mels=n_mels, low_freq=low, high_freq=high)
    first, count, weights = capi.fbank_filterbank(spec)
    W = ft.mel_weights64(d)
    assert W.shape == (n_mels, n_fft // 2) and first.shape == count.shape == (n_mels,) and weights.size == int(count.sum())
    at = 0
    for b in range(n_mels):
        live = np.nonzero(W[b] > 0)[0]
        assert live.size > 0, b
        assert first[b] == live[0] and count[b] == live[-1] - live[0] + 1 == live.size  # (every band's live bins are contiguous)
        got = weights[at: at + count[b]].astype(np.float64)
        # one float32 rounding, of a float64 value that two evaluations may state a few of its own roundings apart (mel values of up
        # to 3000 divided by a band width d of 30 and more: 2^-52 * 3000 / 30 * a few)
        assert (np.abs(got - W[b, live]) <= U * W[b, live] + 2.0 ** -40).all(), b
        assert (got > 0).all()
        at += count[b]
    if low > 0:
        assert (first > 0).all()  # (bin 0 has weight 0 in every band)
    if high < 0:  # (nothing at or above nyquist + high_freq)
        assert ((first + count - 1) * sr / n_fft < sr / 2 + high).all()
    # Kaldi's bank against its closed form at one point: band b peaks where mel(f) = left + d
    lo, hi = ft.mel64(low), ft.mel64(sr / 2 + high if high <= 0 else high)
    dd = (hi - lo) / (n_mels + 1)
    b = n_mels // 2
    k = int(np.argmax(W[b]))
    assert abs(ft.mel64(k * sr / n_fft) - (lo + (b + 1) * dd)) <= ft.mel64((k + 1) * sr / n_fft) - ft.mel64((k - 1) * sr / n_fft)


def test_a_band_with_no_bin_under_it_is_allowed(capi):
    spec, d = make(capi, sample_rate=16000, n_fft=32, win=32, hop=8, n_mels=40, low_freq=0.0)
    first, count, weights = capi.fbank_filterbank(spec)
    W = ft.mel_weights64(d)
    assert (count == 0).any() and (count > 0).any() and ((W > 0).sum(axis=1) == count).all() and (first[count == 0] == 0).all()


def test_sizing_calls_and_capacities(capi):
    L = capi.lib()
    spec, _ = make(capi)
    n = 400 * 512
    assert L.vpz_fbank_table(C.byref(spec), None, 0) == capi.OK
    buf = np.full(n + 1, 7.0, dtype=np.float32)
    assert L.vpz_fbank_table(C.byref(spec), buf.ctypes.data, n - 1) == capi.E_CAPACITY and (buf == 7.0).all()
    assert L.vpz_fbank_table(C.byref(spec), buf.ctypes.data, n) == capi.OK and buf[-1] == 7.0 and (buf[:-1] != 7.0).all()
    total = C.c_int64(-1)
    assert L.vpz_fbank_filterbank(C.byref(spec), None, None, None, 0, C.byref(total)) == capi.OK and total.value > 80
    assert L.vpz_fbank_filterbank(C.byref(spec), None, None, None, 0, None) == capi.OK
    w = np.full(total.value + 1, 7.0, dtype=np.float32)
    assert L.vpz_fbank_filterbank(C.byref(spec), None, None, w.ctypes.data, total.value - 1, None) == capi.E_CAPACITY and (w == 7.0).all()
    assert L.vpz_fbank_filterbank(C.byref(spec), None, None, w.ctypes.data, total.value, None) == capi.OK and w[-1] == 7.0 and (w[:-1] > 0).all()


def test_every_limit_is_refused(capi):
    L = capi.lib()
    total = C.c_int64(-5)
    buf = np.full(8, 7.0, dtype=np.float32)
    for what, spec in refused_specs(capi):
        assert L.vpz_fbank_filterbank(C.byref(spec), None, None, None, 0, C.byref(total)) == capi.E_INVALID_ARG, what
        assert L.vpz_fbank_table(C.byref(spec), None, 0) == capi.E_INVALID_ARG, what
        assert L.vpz_fbank_table(C.byref(spec), buf.ctypes.data, 1 << 40) == capi.E_INVALID_ARG, what
        with pytest.raises(ValueError):
            capi.fbank_filterbank(spec)
        with pytest.raises(ValueError):
            capi.fbank_table(spec)
    assert total.value == -5 and (buf == 7.0).all()
    good = make(capi)[0]
    assert L.vpz_fbank_filterbank(None, None, None, None, 0, None) == capi.E_INVALID_ARG and L.vpz_fbank_table(None, None, 0) == capi.E_INVALID_ARG
    assert L.vpz_fbank_filterbank(C.byref(good), None, None, None, -1, None) == capi.E_INVALID_ARG and L.vpz_fbank_table(C.byref(good), None, -1) == capi.E_INVALID_ARG
    # vpz_pcm_fbank without a context (its other refusals need a device: tests/test_pcm_fbank_gpu.py)
    assert L.vpz_pcm_fbank(None, None, 0, 400, C.byref(good), 0, None, None, 0) == capi.E_INVALID_ARG
    # at the limits themselves: accepted (a power spec does not look at its floor)
    for kw in (dict(n_fft=32, win=2, hop=1, n_mels=256), dict(n_fft=1024, win=1024, hop=1024, n_mels=1, sample_rate=48000), dict(low_freq=7999.0),
               dict(high_freq=8000.0), dict(log=False, floor=0.0), dict(preemphasis=0.0), dict(preemphasis=1.0), dict(win=551, n_fft=552, hop=551),
               dict(scale=-1.0), dict(pad_value=-15.9424)):
        capi.fbank_filterbank(make(capi, **kw)[0])
        capi.fbank_table(make(capi, **kw)[0])
    with pytest.raises(ValueError):
        capi.FbankSpec.make(window="blackman")
    with pytest.raises(ValueError):
        capi.FbankSpec.make(window=None)


def test_the_spec_helper_counts_frames(capi):
    s = capi.FbankSpec.make()
    assert [s.n_frames(F) for F in (0, 399, 400, 559, 560, 16000)] == [0, 0, 1, 1, 2, 98]
    assert [ft.n_frames(F, 400, 160) for F in (0, 399, 400, 559, 560, 16000)] == [0, 0, 1, 1, 2, 98]
    assert (s.sample_rate, s.win, s.hop, s.n_fft, s.n_mels, s.low_freq, s.high_freq, s.preemphasis, s.window, s.remove_dc, s.scale, s.output,
            s.floor, s.pad_value, s.layout) == (16000.0, 400, 160, 512, 80, 20.0, 0.0, 0.97, capi.FBANK_POVEY, 1, 32768.0, capi.FBANK_LOG,
                                                2.0 ** -23, 0.0, capi.FBANK_FRAMES_FIRST)


# ---- the surface
def test_the_fbank_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_fbank.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmFbank.cs")
    assert sorted(c) == ["vpz_fbank_filterbank", "vpz_fbank_table", "vpz_pcm_fbank"] == sorted(imports) == sorted(capi.PCM_FBANK_EXPORTED_SYMBOLS)
    assert c["vpz_pcm_fbank"] == ("i32", ["ptr", "ptr", "i64", "i64", "ptr", "i32", "ptr", "ptr", "i64"])
    assert c["vpz_fbank_table"] == ("i32", ["ptr", "ptr", "i64"]) and c["vpz_fbank_filterbank"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "i64", "ptr"])
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_FBANK_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    structs, defines = cs.c_structs("vorbispizza_pcm_fbank.h")
    assert sorted(structs) == ["vpz_fbank_spec"]
    cs_fields = cs.cs_structs(os.path.join(cs.CS, "GpuPcmFbank.cs"))["FbankSpec"]
    py_fields = [(n, {C.c_double: "f64", C.c_int32: "i32"}.get(t, "i32"), getattr(t, "_length_", 0)) for n, t in capi.FbankSpec._fields_]
    assert len(structs["vpz_fbank_spec"]) == len(cs_fields) == len(py_fields) == 16
    for (n0, k0, a0), (n1, k1, a1), (n2, k2, a2) in zip(structs["vpz_fbank_spec"], cs_fields, py_fields):
        assert cs.norm(n0) == cs.norm(n1) == cs.norm(n2) and k0 == k1 == k2 and a0 == a1 == a2, (n0, n1, n2)
    assert C.sizeof(capi.FbankSpec) == 7 * 8 + 8 * 4 + 10 * 4 == 128
    text = cs.strip_cs_comments(open(os.path.join(cs.CS, "GpuPcmFbank.cs")).read())
    consts = {}
    for m in re.finditer(r"public\s+const\s+int\s+([^;]+);", text):
        for part in m.group(1).split(","):
            k, v = part.split("=")
            consts[cs.norm(k.strip())] = int(v.strip(), 0)
    seen = 0
    for name, value in defines.items():
        if name.startswith("VPZ_FBANK_"):
            assert consts[cs.norm(name[4:])] == value == getattr(capi, name[4:]), name
            seen += 1
    assert seen == 10
    assert (capi.FBANK_HANNING, capi.FBANK_HAMMING, capi.FBANK_POVEY, capi.FBANK_POWER, capi.FBANK_LOG, capi.FBANK_BANDS_FIRST,
            capi.FBANK_FRAMES_FIRST) == (0, 1, 2, 0, 1, 0, 1)
    # the older headers and their lists did not take the new names
    for name in c:
        assert name not in (capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_RESAMPLE_EXPORTED_SYMBOLS
                            + capi.PCM_LOGMEL_EXPORTED_SYMBOLS)
        assert name not in cs.c_functions("vorbispizza_synth.h", "vpz_") and name not in cs.c_functions("vorbispizza_pcm_logmel.h", "vpz_")


def test_the_fbank_call_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import capi, multi
    c = cs.c_functions("vorbispizza_multi_fbank.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiFbank.cs")
    assert sorted(c) == ["vpzm_decode_ranges_fbank"] == sorted(imports) == sorted(multi.FBANK_EXPORTED_SYMBOLS)
    # the log-mel call's parameters, the spec of the other kind in the same place
    assert c["vpzm_decode_ranges_fbank"] == cs.c_functions("vorbispizza_multi_logmel.h", "vpzm_")["vpzm_decode_ranges_logmel"]
    assert imports["vpzm_decode_ranges_fbank"] == ("Host",) + c["vpzm_decode_ranges_fbank"]
    fn = multi.lib().vpzm_decode_ranges_fbank
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_decode_ranges_fbank"][1] and KINDS[fn.restype] == "i32"
    assert cs.c_structs("vorbispizza_multi_fbank.h")[0] == {}
    assert sorted(cs.c_functions("vorbispizza_multi_logmel.h", "vpzm_")) == ["vpzm_decode_ranges_logmel"] == sorted(multi.LOGMEL_EXPORTED_SYMBOLS)
    sig = inspect.signature(multi.Dispatcher.decode_ranges_fbank)
    assert list(sig.parameters) == ["self", "datas", "ranges", "frames"] + list(ft.DEFAULTS) + ["out"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert {k: d[k] for k in ft.DEFAULTS} == ft.DEFAULTS and d["out"] is None
    assert ft.DEFAULTS["floor"] == capi.FLT_EPSILON == float(np.finfo(np.float32).eps)
    made = inspect.signature(capi.FbankSpec.make)
    assert {k: p.default for k, p in made.parameters.items() if k != "cls"} == ft.DEFAULTS


def test_both_libraries_export_the_new_symbols(capi):
    from vorbispizza_amd import _build, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in capi.PCM_FBANK_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert hasattr(H, "vpzm_decode_ranges_fbank") and not hasattr(S, "vpzm_decode_ranges_fbank")
    assert "pcm_fbank.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "fbank_tables.hpp"))
    assert callable(capi.pcm_fbank) and callable(capi.fbank_table) and callable(capi.fbank_filterbank) and callable(multi.Dispatcher.decode_ranges_fbank)


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    for header, body in (("vorbispizza_pcm_fbank.h", "sizeof(vpz_fbank_spec) == 128 && sizeof(vpz_pack_row) == 24 && VPZ_FBANK_MAX_NFFT == 1024 && VPZ_FBANK_POVEY == 2"),
                         ("vorbispizza_multi_fbank.h", "VPZM_E_RATE == -16 && VPZ_FBANK_LOG == 1 && VPZ_FBANK_FRAMES_FIRST == 1")):
        src = tmp_path / (header + ".c")
        src.write_text('#include "%s"\ntypedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % (header, body))
        exe = tmp_path / (header + ".exe")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


def test_the_fbank_kernels_use_no_scratch_and_say_what_they_take():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = [k for k in kr.analyse(os.path.join(_build.CSRC, "pcm_fbank.hip"), _build.SOURCES["pcm_fbank.hip"]) if "pcm_fbank_kernel" in k["name"]]
    assert len(ks) == 2  # <one / two 32-frame row tiles>
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k.get("vgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 512 and k["occupancy"] >= 1, k


# ---- the truth itself
def test_the_folded_operator_equals_the_unfolded_chain():
    """the restatement's two routes agree: frames through scale, pre-emphasis, window, pad and rfft, and the same frames times operator64"""
    rng = np.random.default_rng(2)
    for kw in (dict(), dict(win=551, hop=220, n_fft=1024, sample_rate=22050, window="hamming"), dict(win=37, hop=5, n_fft=38, preemphasis=1.0, window="hanning")):
        d = ft.spec_of(**kw)
        Y = rng.standard_normal((5, d["win"]))
        re, im = ft.spectrum64(d["scale"] * Y, d)
        Bc, Bs = ft.operator64(d)
        assert np.abs(re - Y @ Bc).max() <= 1e-9 * d["scale"] and np.abs(im - Y @ Bs).max() <= 1e-9 * d["scale"]


def test_the_bound_discriminates():
    """a float32 proxy of the kernel -- the stated mean order, the subtraction, a float32 multiply and add per step (no better than the
    fused chain) -- stays far inside e_M, on plain noise and on frames whose DC dwarfs their signal; on the noise, one table row 5 % off
    leaves the bound on most outputs: it both holds and catches a wrong table.  (Under a DC of 500 times the signal the mean's own
    rounding is most of the bound, as it is most of the error: such a case shows that the bound holds, not that it is tight.)"""
    rng = np.random.default_rng(11)
    d = ft.spec_of(win=96, hop=17, n_fft=128, n_mels=13, sample_rate=8000, low_freq=100.0, high_freq=-200.0, scale=1.0, log=False)
    W = ft.mel_weights64(d)
    Bc, Bs = (t.astype(np.float32) for t in ft.operator64(d))

    def centred(x):
        X = ft.frames_of(x, 96, 17).astype(np.float32)
        s = [np.zeros(X.shape[0], np.float32) for _ in range(4)]
        for q in range(4):
            for j in range(q, 96, 4):
                s[q] = s[q] + X[:, j]
        return X - (((s[0] + s[1]) + (s[2] + s[3])) / np.float32(96))[:, None]

    def proxy(A, Bc, Bs):
        re, im = np.zeros((A.shape[0], Bc.shape[1]), np.float32), np.zeros((A.shape[0], Bc.shape[1]), np.float32)
        for m in range(96):
            re += A[:, m:m + 1] * Bc[m:m + 1]
            im += A[:, m:m + 1] * Bs[m:m + 1]
        return (re * re + im * im).astype(np.float64) @ W.astype(np.float32).astype(np.float64).T

    noise, dc = (0.5 * rng.standard_normal(600)).astype(np.float32), (0.5 + 1e-3 * rng.standard_normal(600)).astype(np.float32)
    for x in (noise, dc):
        M, e_M = ft.fbank_truth(x, d, W)
        worst = float((np.abs(proxy(centred(x), Bc, Bs) - M) / e_M).max())
        print('proxy error / bound %.3f' % worst)
        assert worst <= 0.5
    Bc[48] *= np.float32(1.05)
    Bs[48] *= np.float32(1.05)
    M, e_M = ft.fbank_truth(noise, d, W)
    assert (np.abs(proxy(centred(noise), Bc, Bs) - M) > e_M).mean() > 0.5


# ---- the launch plan
def test_a_tile_fits_and_no_index_leaves_the_span_at_any_spec():
    """every even n_fft in 32..1024 with win and hop at the limits (and a sweep of every win <= n_fft, hop <= win at four n_fft): 16
    frames always fit, so VPZ_E_UNSUPPORTED cannot be reached inside the limits; at each tile size the largest skewed index written by
    the staging and the largest read by a frame lie inside span_cap"""
    k = ft.kernel_constants(ROOT)
    assert (k["kFbLdsFloats"], k["kFbAhead"], k["kFbCols"], k["kFbMaxGridY"], k["kFbMeans"]) == (40960, 4, 32, 2048, 64)
    largest = 0

    def sweep(n_fft, wins):
        nonlocal largest
        for win in wins:
            hop = np.arange(1, win + 1, dtype=np.int64)
            skew = (hop % 2 == 0).astype(np.int64)
            pstride = (n_fft // 2) | 1
            for Tt in (64, 32, 16):
                count = (Tt - 1) * hop + win
                span_cap = count + skew * (count // hop) + 1
                assert (count - 1 + skew * ((count - 1) // hop) < span_cap).all()  # the staging's last write
                assert ((Tt - 1) * (hop + skew) + (win - 1) + skew * ((win - 1) // hop) < span_cap).all()  # the last frame's last sample
                if Tt == 16:
                    total = span_cap + k["kFbMeans"] + Tt * pstride
                    assert (total <= k["kFbLdsFloats"]).all(), (n_fft, win)
                    largest = max(largest, int(total.max()))
            for h in (1, 2, win - 1, win):
                if h >= 1:
                    for Tt in (64, 32, 16):
                        c = (Tt - 1) * h + win
                        assert ft.lds_plan(win, h, n_fft, Tt) == (c + (c // h if h % 2 == 0 else 0) + 1, pstride)
                    assert ft.tile_plan(win, h, n_fft, 1000, 1000, 256, k)[0] in (64, 32, 16)

    for n_fft in range(32, 1025, 2):
        sweep(n_fft, (2, 3, n_fft - 1, n_fft))
    for n_fft in (32, 38, 512, 1024):
        sweep(n_fft, range(2, n_fft + 1))
    assert largest == 16 * 1024 + 16 + 1 + 64 + 16 * 513  # (win = hop = n_fft = 1024)
    # the tile by the launch's size at the default spec: 16 frames for a short row, 32 for few rows, 64 for a crowd
    assert [ft.tile_plan(400, 160, 512, T, n, 256, k)[0] for T, n in ((16, 1), (17, 1), (98, 5), (98, 255), (98, 256), (32, 1000), (33, 1000))] == \
        [16, 32, 32, 32, 64, 32, 64]
    # and where the LDS decides: n_fft = win = 1024
    assert [ft.tile_plan(1024, hop, 1024, 104, 600, 256, k)[0] for hop in (1, 111, 112, 755, 756, 1024)] == [64, 64, 32, 32, 16, 16]


# ---- the cases of tests/test_pcm_fbank_limits_gpu.py
def test_every_limit_case_is_the_shape_it_is_named_for(capi):
    """each case of fbank_cases.py against the numbers written down there: the k loop's whole blocks, leftover pairs and odd sample, the
    skew, the bin groups and the waves' rounds, and tile and LDS floats through tile_plan"""
    import fbank_cases as fc
    k = ft.kernel_constants(ROOT)
    assert [v[0] for v in fc.SMALL.values()] == [(2, 2, 32, 1), (3, 2, 32, 2), (3, 3, 32, 2), (4, 2, 32, 3), (5, 2, 34, 3), (7, 6, 36, 4), (8, 2, 32, 3),
                                                  (9, 8, 32, 3), (33, 32, 64, 5), (33, 2, 64, 5), (63, 62, 64, 8), (64, 64, 64, 8)]
    for name, ((win, hop, n_fft, n_mels), chain, skew, rounds) in fc.SMALL.items():
        change, F = fc.small(name)
        T = ft.n_frames(F, win, hop)
        assert T == 71 and T % 16 != 0 and (F - win) % hop != 0, name
        assert fc.chain_of(win, k) == chain and (hop % 2 == 0) == bool(skew) and fc.rounds_of(n_fft, k) == rounds, name
        tile, floats = fc.tile_of(change, F, 5, fc.CROWD_CUS, k)
        assert tile == 32 and floats <= k["kFbLdsFloats"], name
        capi.FbankSpec.make(**ft.spec_of(**change))
    assert {v[0][1] for v in fc.SMALL.values()} >= {2, 3, 6} and all((w - 1, w) in [(v[0][1], v[0][0]) for v in fc.SMALL.values()] for w in (3, 7, 9, 33, 63))
    # a mean lane with no term at win 3; one term each at win 4; a fifth sample to lane 0 at win 5
    assert [len(range(3, w, 4)) for w in (3, 4, 5)] == [0, 1, 1] and len(range(0, 5, 4)) == 2
    assert [v[0][2] // 2 for v in fc.GROUPS.values()] == [32, 33, 64, 65, 128, 129]
    for name, ((win, hop, n_fft, n_mels), rounds) in fc.GROUPS.items():
        change, F = fc.group(name)
        assert win in (n_fft - 1, n_fft) and fc.rounds_of(n_fft, k) == rounds and -(-(n_fft // 2) // k["kFbCols"]) == sum(rounds), name
        assert ft.n_frames(F, win, hop) == 71 and (F - win) % hop != 0 and fc.tile_of(change, F, 5, fc.CROWD_CUS, k)[0] == 32, name
    change, F = fc.group(fc.CROWDED_GROUP)
    assert fc.tile_of(change, F, fc.crowd_rows(fc.CROWD_CUS), fc.CROWD_CUS, k)[0] == 64 and fc.GROUPS[fc.CROWDED_GROUP][1][0] == 2
    # the LDS limits at n_fft 1024
    assert list(fc.LDS_LIMITS) == [(944, 113), (1024, 111), (1024, 112), (1012, 757), (1024, 755), (1024, 756)]
    for (win, hop), (T, tile, floats, tile_few) in fc.LDS_LIMITS.items():
        change, F = fc.lds_limit(win, hop)
        assert ft.n_frames(F, win, hop) == T and T % 16 != 0 and (F - win) % hop != 0
        for cus in (64, 256, 304):
            assert fc.tile_of(change, F, fc.crowd_rows(cus), cus, k) == (tile, floats), (win, hop, cus)
        assert fc.tile_of(change, F, 5, fc.CROWD_CUS, k)[0] == tile_few
        assert floats <= k["kFbLdsFloats"]
    assert [v[2] for v in fc.LDS_LIMITS.values()].count(k["kFbLdsFloats"]) == 2  # (the budget exactly, at 64 and at 32 frames)
    # one frame more of hop, or one sample more of win, and the tile no longer fits
    assert ft.lds_plan(944, 113, 1024, 64)[0] + 64 + 64 * 513 == 40960 and ft.lds_plan(1012, 757, 1024, 32)[0] + 64 + 32 * 513 == 40960
    assert ft.tile_plan(945, 113, 1024, 40, 600, 256, k)[0] == 32 and ft.tile_plan(1013, 757, 1024, 40, 600, 256, k)[0] == 16
    # most of 256 bands have no bin at n_fft 32
    first, count, _ = capi.fbank_filterbank(capi.FbankSpec.make(**ft.spec_of(**fc.EMPTY_BANDS)))
    assert (count == 0).sum() > 200 and (count > 0).sum() >= 8
    # the second round: four waves at work, one 16-frame tile a row; the long row: more than a thousand tiles
    d = ft.spec_of(**fc.SECOND_ROUND)
    assert fc.rounds_of(d["n_fft"], k) == (1, 1, 1, 1) and ft.tile_plan(200, 80, 256, 3, 2100, fc.CROWD_CUS, k)[0] == 16
    for n in (2100, 4200):
        Ls = fc.second_round_lengths(n, 397, 200, np.random.default_rng(3))
        assert n > k["kFbMaxGridY"] and (Ls[0], Ls[2048]) == ((397, 0) if n == 2100 else (397, 199)) and (Ls == 0).any() and (Ls < 200).sum() > 100
    change, F = fc.LONG_ROW
    tile, _ = fc.tile_of(change, F, 1, fc.CROWD_CUS, k)
    assert tile == 64 and -(-ft.n_frames(F, 2, 1) // tile) > 1000  # (so many tiles of one row are a crowd by themselves)
