"""vpz_logmel_dft_table and vpz_mel_filterbank (include/vorbispizza_pcm_logmel.h, csrc/logmel_tables.hpp) without a device, and what a
clean checkout must hold about the new headers and bindings.

THE TRUTH of the log-mel tests is written here, in float64 numpy, from the formulas of the header's definition -- not from the library's
tables: dft64 (window and DFT matrix), mel_weights64 (the filterbank), extend (zero extension and reflection), logmel_truth (M and the
derived bound e_M).  tests/test_pcm_logmel_gpu.py and tests/test_multi_logmel_gpu.py import them.

The bound (u = 2^-24; the kernel's sums are fmaf chains of length n_fft over once-rounded coefficients, m ascending, then of a band's
live bins, k ascending):
    d_re[k] = (n_fft + 2) u sum_m |x w cos|        d_im likewise with sin
    e_P[k]  = 2 |re| d_re + 2 |im| d_im + d_re^2 + d_im^2 + 3 u P
    e_M[b]  = sum_k W[b][k] e_P[k] + (B + 2) u M[b]        B: the largest live-bin count of a band
all evaluated in float64 on the same input.

THE LAUNCH PLAN of vpz_pcm_logmel is restated here as well (lds_plan, tile_plan), with the case lists of
tests/test_pcm_logmel_limits_gpu.py, LIMIT_*: a test without a GPU holds the lists to the plan -- a changed constant in pcm_logmel.hip
fails here, not as a quietly weaker GPU test -- and a sweep over every n_fft and hop holds the plan's index arithmetic."""
import ctypes as C
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

import binding_support as cs  # noqa: E402
from binding_support import imports_of  # noqa: E402
from f32_model import U  # noqa: E402
from logmel_truth import (CROWD_T, KINDS, LIMIT_CROWDS, LIMIT_GROUPS, LIMIT_HOPS, LIMIT_LDS, LIMIT_TAIL, crowd_rows, dft64,  # noqa: E402
    frames_of, lds_plan, limit_F, logmel_kernel_constants, logmel_truth, mel_points, mel_weights64, power_truth,
    refused_specs, tile_plan)


# (sample_rate, n_fft, n_mels, f_min, f_max, mel_scale, mel_norm)
BANKS = [(16000, 400, 80, 0.0, 8000.0, "slaney", "slaney"), (22050, 512, 64, 20.0, 11025.0, "htk", None), (8000, 96, 13, 100.0, 3800.0, "slaney", None),
         (48000, 1024, 256, 0.0, 24000.0, "htk", "slaney"), (16000, 32, 1, 0.0, 8000.0, "slaney", "slaney"), (16000, 32, 40, 0.0, 8000.0, "slaney", "slaney")]


def spec_of(bank, **kw):
    from vorbispizza_amd import capi
    sr, n_fft, n_mels, f_min, f_max, scale, norm = bank
    return capi.LogMelSpec.make(sample_rate=sr, n_fft=n_fft, hop=kw.pop("hop", max(1, n_fft // 4)), n_mels=n_mels, f_min=f_min, f_max=f_max, mel_scale=scale,
                                mel_norm=norm, **kw)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


# ---- the tables
@pytest.mark.parametrize("n_fft", [32, 34, 96, 400, 512, 1024])
def test_the_dft_table_is_the_restatement_rounded_once(capi, n_fft):
    """One float32 rounding of the float64 value: |t - v| <= u |v|.  The float64 values themselves carry the error of cos and sin at a
    rounded multiple of pi / 2 (1.2e-16 where the exact value is 0), which the library's table does not: 2^-52 w[m] is allowed for it."""
    table = capi.logmel_dft_table(n_fft)
    cos, sin = dft64(n_fft)
    assert table.shape == (n_fft, 2, n_fft // 2 + 1) and table.dtype == np.float32
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft))[:, None]
    for got, want in ((table[:, 0], cos), (table[:, 1], sin)):
        assert (np.abs(got.astype(np.float64) - want) <= U * np.abs(want) + 2.0 ** -52 * w).all()
    # the sin columns of k = 0 and of k = n_fft / 2 are zeros, bit for bit (no -0.0 either)
    assert (table[:, 1, 0].view(np.uint32) == 0).all() and (table[:, 1, n_fft // 2].view(np.uint32) == 0).all()
    assert (table[0].view(np.uint32) == 0).all()  # (w[0] = 0)
    assert np.abs(table[n_fft // 2, 0, 1] + 1.0) == 0  # (w = 1, cos(pi) = -1)


@pytest.mark.parametrize("bank", BANKS)
def test_the_filterbank_is_the_restatement_rounded_once(capi, bank):
    first, count, weights = capi.mel_filterbank(spec_of(bank))
    W = mel_weights64(*bank)
    assert first.shape == count.shape == (bank[2],) and weights.size == int(count.sum())
    at = 0
    for b in range(bank[2]):
        live = np.nonzero(W[b] > 0)[0]
        if live.size == 0:
            assert count[b] == 0 and first[b] == 0
            continue
        assert first[b] == live[0] and count[b] == live[-1] - live[0] + 1 == live.size  # (a triangle's live bins are consecutive)
        want = W[b, live]
        got = weights[at: at + count[b]].astype(np.float64)
        # one float32 rounding, of a float64 value that two evaluations may state a few of its own roundings apart
        assert (np.abs(got - want) <= U * want + 8 * 2.0 ** -52 * np.abs(W[b]).max() + 2.0 ** -149).all(), b
        at += count[b]


def test_sizing_calls_and_capacities(capi):
    L = capi.lib()
    assert L.vpz_logmel_dft_table(400, None, 0) == capi.OK
    buf = np.full(400 * 402 + 1, 7.0, dtype=np.float32)
    assert L.vpz_logmel_dft_table(400, buf.ctypes.data, 400 * 402 - 1) == capi.E_CAPACITY and (buf == 7.0).all()
    assert L.vpz_logmel_dft_table(400, buf.ctypes.data, 400 * 402) == capi.OK and buf[-1] == 7.0
    spec = spec_of(BANKS[0])
    total = C.c_int64(-1)
    assert L.vpz_mel_filterbank(C.byref(spec), None, None, None, 0, C.byref(total)) == capi.OK and total.value > 80
    assert L.vpz_mel_filterbank(C.byref(spec), None, None, None, 0, None) == capi.OK
    w = np.full(total.value + 1, 7.0, dtype=np.float32)
    assert L.vpz_mel_filterbank(C.byref(spec), None, None, w.ctypes.data, total.value - 1, None) == capi.E_CAPACITY and (w == 7.0).all()
    assert L.vpz_mel_filterbank(C.byref(spec), None, None, w.ctypes.data, total.value, None) == capi.OK and w[-1] == 7.0 and (w[:-1] > 0).all()


def test_every_limit_is_refused(capi):
    L = capi.lib()
    for n_fft in (0, -2, 30, 31, 33, 1025, 1026, 2048):
        assert L.vpz_logmel_dft_table(n_fft, None, 0) == capi.E_INVALID_ARG, n_fft
    assert L.vpz_logmel_dft_table(400, None, -1) == capi.E_INVALID_ARG
    for n_fft in (32, 1024):
        assert L.vpz_logmel_dft_table(n_fft, None, 0) == capi.OK
    total = C.c_int64(-5)
    for what, spec in refused_specs(capi):
        assert L.vpz_mel_filterbank(C.byref(spec), None, None, None, 0, C.byref(total)) == capi.E_INVALID_ARG, what
        with pytest.raises(ValueError):
            capi.mel_filterbank(spec)
    assert total.value == -5
    assert L.vpz_mel_filterbank(None, None, None, None, 0, None) == capi.E_INVALID_ARG
    good = capi.LogMelSpec.make()
    assert L.vpz_mel_filterbank(C.byref(good), None, None, None, -1, None) == capi.E_INVALID_ARG
    # at the limits themselves: accepted (a power spec does not look at its floor)
    for kw in (dict(n_fft=32, hop=32, n_mels=256), dict(n_fft=1024, hop=1, n_mels=1), dict(f_min=7999.0), dict(log=False, floor=0.0)):
        capi.mel_filterbank(capi.LogMelSpec.make(**kw))
    with pytest.raises(ValueError):
        capi.logmel_dft_table(30)
    with pytest.raises(ValueError):
        capi.LogMelSpec.make(mel_scale="bark")


def test_slaney_bands_have_equal_area_and_an_empty_band_is_allowed(capi):
    """A Slaney-normalised triangle has area 1 in Hz.  Its bins sample it df = sample_rate / n_fft apart; the trapezoid sum of a piecewise
    linear function is exact but in the cells that hold its three kinks, where it misses by at most df^2 / 8 times the change of slope:
    in all df * peak / 2 when both sides are at least a bin wide -- so df * sum(W) is within a bin at the peak, df * peak, of 1."""
    bank = (16000, 1024, 20, 0.0, 8000.0, "slaney", "slaney")
    first, count, weights = capi.mel_filterbank(spec_of(bank))
    pts, df = mel_points(bank[0], bank[2], bank[3], bank[4], bank[5]), bank[0] / bank[1]
    assert (np.diff(pts) >= df).all() and (count >= 4).all()
    at = 0
    for b in range(bank[2]):
        area = df * float(weights[at: at + count[b]].astype(np.float64).sum())
        assert abs(area - 1.0) <= df * 2.0 / (pts[b + 2] - pts[b]), (b, area)
        at += count[b]
    # bands narrower than a bin: no bin under some of them, count 0, and the call succeeds
    first, count, weights = capi.mel_filterbank(spec_of(BANKS[5]))
    W = mel_weights64(*BANKS[5])
    assert (count == 0).any() and (count > 0).any() and ((W > 0).sum(axis=1) == count).all() and (first[count == 0] == 0).all()
    # the two scales differ
    a = capi.mel_filterbank(spec_of((16000, 400, 40, 0.0, 8000.0, "htk", None)))
    b = capi.mel_filterbank(spec_of((16000, 400, 40, 0.0, 8000.0, "slaney", None)))
    assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def test_the_restatement_agrees_with_torch_stft():
    """a second opinion on P: torch.stft in float64, center=True, reflect padding, on a row of the padded batch"""
    import torch
    rng = np.random.default_rng(5)
    for n_fft, hop, F, L in ((400, 160, 1777, 1500), (96, 17, 300, 300), (32, 1, 17, 9)):
        x = rng.standard_normal(L) * 0.5
        P, _ = power_truth(frames_of(x, L, F, n_fft, hop), n_fft)
        row = np.zeros(F)
        row[:L] = x
        S = torch.stft(torch.from_numpy(row), n_fft, hop_length=hop, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64), center=True,
                       pad_mode="reflect", return_complex=True)
        want = (S.abs() ** 2).numpy().T
        assert want.shape == P.shape == (1 + F // hop, n_fft // 2 + 1)
        assert np.abs(P - want).max() <= 1e-12 * max(1.0, want.max())


# ---- the surface
def test_the_logmel_binding_matches_its_header(tmp_path, capi):
    c = cs.c_functions("vorbispizza_pcm_logmel.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmLogMel.cs")
    assert sorted(c) == ["vpz_logmel_dft_table", "vpz_mel_filterbank", "vpz_pcm_logmel"] == sorted(imports) == sorted(capi.PCM_LOGMEL_EXPORTED_SYMBOLS)
    assert c["vpz_pcm_logmel"] == ("i32", ["ptr", "ptr", "i64", "i64", "ptr", "i32", "ptr", "ptr", "i64"])
    assert c["vpz_logmel_dft_table"] == ("i32", ["i32", "ptr", "i64"]) and c["vpz_mel_filterbank"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "i64", "ptr"])
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_LOGMEL_SIGNATURES:
        assert ([KINDS.get(a, "ptr") for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    structs, defines = cs.c_structs("vorbispizza_pcm_logmel.h")
    assert sorted(structs) == ["vpz_logmel_spec"]
    cs_fields = cs.cs_structs(os.path.join(cs.CS, "GpuPcmLogMel.cs"))["LogMelSpec"]
    py_fields = [(n, {C.c_double: "f64", C.c_int32: "i32"}.get(t, "i32"), getattr(t, "_length_", 0)) for n, t in capi.LogMelSpec._fields_]
    assert len(structs["vpz_logmel_spec"]) == len(cs_fields) == len(py_fields) == 12
    for (n0, k0, a0), (n1, k1, a1), (n2, k2, a2) in zip(structs["vpz_logmel_spec"], cs_fields, py_fields):
        assert cs.norm(n0) == cs.norm(n1) == cs.norm(n2) and k0 == k1 == k2 and a0 == a1 == a2, (n0, n1, n2)
    assert C.sizeof(capi.LogMelSpec) == 4 * 8 + 7 * 4 + 9 * 4
    text = cs.strip_cs_comments(open(os.path.join(cs.CS, "GpuPcmLogMel.cs")).read())
    consts = {}
    for m in re.finditer(r"public\s+const\s+int\s+([^;]+);", text):
        for part in m.group(1).split(","):
            k, v = part.split("=")
            consts[cs.norm(k.strip())] = int(v.strip(), 0)
    seen = 0
    for name, value in defines.items():
        if name.startswith("VPZ_MEL_") or name.startswith("VPZ_LOGMEL_"):
            assert consts[cs.norm(name[4:])] == value == getattr(capi, name[4:]), name
            seen += 1
    assert seen == 11
    # the older headers and their lists did not take the new names
    for name in c:
        assert name not in capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS + capi.PCM_RESAMPLE_EXPORTED_SYMBOLS
        assert name not in cs.c_functions("vorbispizza_synth.h", "vpz_") and name not in cs.c_functions("vorbispizza_pcm_resample.h", "vpz_")


def test_the_logmel_call_binding_matches_its_header(tmp_path):
    import inspect
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_logmel.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiLogMel.cs")
    assert sorted(c) == ["vpzm_decode_ranges_logmel"] == sorted(imports) == sorted(multi.LOGMEL_EXPORTED_SYMBOLS)
    res = cs.c_functions("vorbispizza_multi_resample.h", "vpzm_")["vpzm_decode_ranges_resampled"]
    # the resampled call's parameters with the spec in the place of rate, channels and downmix, and no layout
    assert c["vpzm_decode_ranges_logmel"] == (res[0], res[1][:5] + ["ptr"] + res[1][8:9] + res[1][10:])
    assert imports["vpzm_decode_ranges_logmel"] == ("Host",) + c["vpzm_decode_ranges_logmel"]
    fn = multi.lib().vpzm_decode_ranges_logmel
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_decode_ranges_logmel"][1] and KINDS[fn.restype] == "i32"
    assert cs.c_structs("vorbispizza_multi_logmel.h")[0] == {}
    assert sorted(cs.c_functions("vorbispizza_multi_resample.h", "vpzm_")) == ["vpzm_decode_ranges_resampled"] == sorted(multi.RESAMPLE_EXPORTED_SYMBOLS)
    sig = inspect.signature(multi.Dispatcher.decode_ranges_logmel)
    assert list(sig.parameters) == ["self", "datas", "ranges", "frames", "sample_rate", "n_fft", "hop", "n_mels", "f_min", "f_max", "mel_scale", "mel_norm",
                                    "log", "floor", "bands_first", "out"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["sample_rate"], d["n_fft"], d["hop"], d["n_mels"], d["f_min"], d["f_max"], d["mel_scale"], d["mel_norm"], d["log"], d["floor"],
            d["bands_first"], d["out"]) == (16000, 400, 160, 80, 0.0, None, "slaney", "slaney", True, 1e-10, True, None)


def test_both_libraries_export_the_new_symbols(capi):
    from vorbispizza_amd import _build, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in capi.PCM_LOGMEL_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert hasattr(H, "vpzm_decode_ranges_logmel") and not hasattr(S, "vpzm_decode_ranges_logmel")
    assert "pcm_logmel.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "logmel_tables.hpp"))
    assert callable(capi.pcm_logmel) and callable(capi.logmel_dft_table) and callable(capi.mel_filterbank) and callable(multi.Dispatcher.decode_ranges_logmel)


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    for header, body in (("vorbispizza_pcm_logmel.h", "sizeof(vpz_logmel_spec) == 96 && sizeof(vpz_pack_row) == 24 && VPZ_LOGMEL_MAX_NFFT == 1024"),
                         ("vorbispizza_multi_logmel.h", "VPZM_E_RATE == -16 && VPZ_MEL_LOG10 == 1")):
        src = tmp_path / (header + ".c")
        src.write_text('#include "%s"\ntypedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % (header, body))
        exe = tmp_path / (header + ".exe")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


def test_the_logmel_kernels_use_no_scratch_and_say_what_they_take():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = [k for k in kr.analyse(os.path.join(_build.CSRC, "pcm_logmel.hip"), _build.SOURCES["pcm_logmel.hip"]) if "pcm_logmel_kernel" in k["name"]]
    assert len(ks) == 2  # <one / two 32-frame row tiles>
    for k in ks:
        assert k["scratch"] == 0 and k.get("vgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 512 and k["occupancy"] >= 1, k


def test_the_bound_discriminates():
    """a float32 sequential-sum proxy of the kernel stays far inside e_M, and one window coefficient 5 % off leaves it on most outputs: the
    bound both holds and catches a wrong table"""
    rng = np.random.default_rng(11)
    n_fft, hop, F = 96, 17, 600
    W = mel_weights64(8000, n_fft, 13, 100.0, 3800.0, "slaney", None)
    x = rng.standard_normal(F) * 0.5
    M, e_M = logmel_truth(x, F, F, n_fft, hop, W)
    X = frames_of(x, F, F, n_fft, hop).astype(np.float32)
    cos, sin = (t.astype(np.float32) for t in dft64(n_fft))

    def proxy(cos, sin):
        re, im = np.zeros((X.shape[0], cos.shape[1]), np.float32), np.zeros((X.shape[0], cos.shape[1]), np.float32)
        for m in range(n_fft):  # (a float32 product and a float32 add per step: no better than the fused chain)
            re += X[:, m:m + 1] * cos[m:m + 1]
            im += X[:, m:m + 1] * sin[m:m + 1]
        return ((re * re + im * im).astype(np.float64) @ W.astype(np.float32).astype(np.float64).T)

    assert (np.abs(proxy(cos, sin) - M) <= 0.1 * e_M).all()
    cos[n_fft // 2] *= np.float32(1.05)
    sin[n_fft // 2] *= np.float32(1.05)
    assert (np.abs(proxy(cos, sin) - M) > e_M).mean() > 0.5


# ---- the launch plan
def test_the_limit_cases_take_the_tiles_they_are_meant_to():
    """tests/test_pcm_logmel_limits_gpu.py's lists against the restated plan at 256 CUs: the tile of every case, the LDS requests next
    to the budget, every length of the k loop's tail"""
    k, cu = logmel_kernel_constants(), 256
    assert (k["kLmLdsFloats"], k["kLmAhead"], k["kLmCols"], k["kLmMaxGridY"]) == (40960, 4, 32, 2048)
    for case in LIMIT_TAIL + LIMIT_LDS + LIMIT_GROUPS + LIMIT_HOPS:
        n_fft, hop, T, n_mels, tile = case
        F = limit_F(case)
        assert T == 1 + F // hop and T % 32 != 0 and F >= n_fft // 2 + 1, case
        assert tile_plan(n_fft, hop, T, 5, cu, k)[0] == tile, case
    n = crowd_rows(cu)
    assert n == 257 and CROWD_T % 64 == 40  # (the last 64-frame tile holds 40 frames: the second row tile is partly live)
    for n_fft, hop, n_mels in LIMIT_CROWDS:
        assert tile_plan(n_fft, hop, CROWD_T, n, cu, k)[0] == 64, (n_fft, hop)
        assert tile_plan(n_fft, hop, CROWD_T, n - 1, cu, k)[0] == 64 and tile_plan(n_fft, hop, CROWD_T, n - 2, cu, k)[0] == 32  # (the threshold)
        assert tile_plan(n_fft, hop, CROWD_T, cu // 2, cu, k)[0] == 32, (n_fft, hop)
    # the boundaries of the LDS at n_fft 1024: 64 frames up to hop 111, 32 up to 757
    want = {110: (64, 40859), 111: (64, 40850), 112: (32, None), 113: (32, None), 757: (32, 40908), 758: (16, None)}
    for hop, (tile, floats) in want.items():
        got = tile_plan(1024, hop, CROWD_T, n, cu, k)
        assert got[0] == tile and (floats is None or got[1] == floats), (hop, got)
        assert got[1] <= k["kLmLdsFloats"]
    for hop in range(1, 1025):
        assert tile_plan(1024, hop, CROWD_T, n, cu, k)[0] == (64 if hop <= 111 else 32 if hop <= 757 else 16), hop
    assert {(hop, tile) for n_fft, hop, T, n_mels, tile in LIMIT_LDS} == {(112, 32), (113, 32), (757, 32), (758, 16)}
    assert {hop for n_fft, hop, n_mels in LIMIT_CROWDS if n_fft == 1024} == {110, 111}
    requests = [tile_plan(n_fft, hop, CROWD_T, n, cu, k)[1] for n_fft, hop, n_mels in LIMIT_CROWDS]
    requests += [tile_plan(c[0], c[1], c[2], 5, cu, k)[1] for c in LIMIT_LDS]
    assert sum(r > 40800 for r in requests) >= 4 and max(requests) == 40908  # (1024 and 1022 at hop 110, 1024 at 111 and at 757)
    # the k loop's tail: n_fft / 2 steps in blocks of kLmAhead
    assert {(c[0] // 2) % k["kLmAhead"] for c in LIMIT_TAIL} == {1, 2, 3}
    assert {(n_fft // 2) % k["kLmAhead"] for n_fft, hop, n_mels in LIMIT_CROWDS} >= {3}  # (the tail in the two-row-tile kernel as well)
    # bin groups of 32: one exactly (cols == nb), a whole number, one per wave, one more than the waves, and 17
    groups = {n_fft: -(-(n_fft // 2 + 1) // k["kLmCols"]) for n_fft in (62, 126, 254, 256, 1024)}
    assert groups == {62: 1, 126: 2, 254: 4, 256: 5, 1024: 17} and {c[0] for c in LIMIT_GROUPS} == {62, 126, 254, 256}
    assert (62 // 2 + 1) % k["kLmCols"] == 0 and lds_plan(62, 15, 32)[1] == 33
    assert all({c[1] % 2 for c in LIMIT_GROUPS if c[0] == n_fft} == {0, 1} for n_fft in (62, 126, 254, 256))  # (hop odd and even)


def test_a_tile_fits_and_no_index_leaves_the_span_at_any_spec():
    """every even n_fft in 32..1024 with every hop in 1..n_fft: 16 frames always fit (VPZ_E_UNSUPPORTED cannot be reached inside the
    limits), and at each tile size the largest skewed index written by the staging and the largest read by a frame lie inside span_cap"""
    k = logmel_kernel_constants()
    largest = 0
    for n_fft in range(32, 1025, 2):
        hop = np.arange(1, n_fft + 1, dtype=np.int64)
        skew = (hop % 2 == 0).astype(np.int64)
        for Tt in (64, 32, 16):
            count = (Tt - 1) * hop + n_fft
            span_cap = count + skew * (count // hop) + 1
            pstride = (n_fft // 2 + 1) | 1
            assert (count - 1 + skew * ((count - 1) // hop) < span_cap).all()
            assert ((Tt - 1) * (hop + skew) + (n_fft - 1) + skew * ((n_fft - 1) // hop) < span_cap).all()
            if Tt == 16:
                assert (span_cap + Tt * pstride <= k["kLmLdsFloats"]).all(), n_fft
                largest = max(largest, int((span_cap + Tt * pstride).max()))
        for h in (1, 2, n_fft - 1, n_fft):  # (the vector form above is the scalar restatement)
            for Tt in (64, 32, 16):
                c = (Tt - 1) * h + n_fft
                assert lds_plan(n_fft, h, Tt) == (c + (c // h if h % 2 == 0 else 0) + 1, (n_fft // 2 + 1) | 1)
            assert tile_plan(n_fft, h, 1000, 1000, 256, k)[0] in (64, 32, 16)
    assert largest == 24609  # (n_fft = hop = 1024)
