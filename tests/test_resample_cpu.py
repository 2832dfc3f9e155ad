"""include/vorbispizza_pcm_resample.h and include/vorbispizza_multi_resample.h without a GPU.

THE TRUTH of every resampling test of the suite is here: `resample_truth`, a numpy float64 restatement of the definition in
vorbispizza_pcm_resample.h (the support of a tap decided in Python integers, a coefficient in float64).  This module holds it to the
table-and-strided-convolution form of the published algorithm (torchaudio.functional.resample at its defaults, restated in numpy), holds
vpz_resample_filter to it, checks what the filter does to a sine below and above the new Nyquist rate, and checks the bindings, the
export lists and the refused ratios against the headers.

The tolerance of the GPU tests, `bound`, is derived, not measured: coefficients rounded once to float32 plus a float32 multiply-accumulate
over T taps, plus C - 1 adds and a scale where C channels are mixed down, give |y - truth| <= (T + C + 3) * 2^-24 * B[j] with
B[j] = sum |x * h| (divided by C for a downmix); C counts as 1 where nothing is mixed.

The kernel's launch plan is restated here too (`launch_plan`, its constants read out of csrc/pcm_resample.hip), together with the case list
of tests/test_pcm_resample_limits_gpu.py, `LIMIT_CASES`: a test without a GPU holds the list to the plan's branches, and a sweep over
ratios up to the limits holds the two facts the kernel's staging counts on."""
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
from binding_support import imports_of, vpzm_statuses  # noqa: E402
from resample_truth import (LIMIT_CASES, filter_table, kernel_constants, launch_plan, passes_text, ratio_of, ratio_ok,  # noqa: E402
    resample_truth, tap_live)

KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}
# (up, down): the ratios of the project's fixtures to 16 000 Hz and back, up- and downsampling, one and many phases, the widest filter
RATIOS = [(160, 441), (1, 3), (3, 1), (160, 147), (147, 160), (441, 80), (1, 6), (2, 1), (1, 2), (320, 441)]
MEASURED_TAPS = {(160, 441): 34, (1, 3): 37, (160, 147): 13, (441, 80): 13, (1, 6): 73}


def strided_convolution_form(x, orig, new):
    """the published algorithm in its own terms: a table [new][2 * width + orig] and a convolution of stride `orig` (orig, new reduced)"""
    lpw, rolloff = 6, 0.99
    base = min(orig, new) * rolloff
    width = math.ceil(lpw * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64) / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx[None, :]
    t = np.clip(t * base, -lpw, lpw)
    window = np.cos(t * np.pi / lpw / 2) ** 2
    t = t * np.pi
    kernel = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t)) * window * (base / orig)
    padded = np.concatenate([np.zeros(width), np.asarray(x, dtype=np.float64), np.zeros(width + orig)])
    frames = (len(padded) - kernel.shape[1]) // orig + 1
    views = np.lib.stride_tricks.as_strided(padded, (frames, kernel.shape[1]), (padded.strides[0] * orig, padded.strides[0]))
    out = views @ kernel.T  # [frames, new]
    return out.reshape(-1)[: -(-new * len(x) // orig)]


@pytest.mark.parametrize("fs,ft", [(44100, 16000), (48000, 16000), (44100, 48000), (8000, 44100), (22050, 16000), (96000, 16000)])
def test_the_restatement_is_the_published_algorithm(fs, ft):
    up, down = ratio_of(fs, ft)
    rng = np.random.default_rng(fs + ft)
    for L in (1, 2, 13, down - 1, down, down + 1, 1000):
        x = rng.uniform(-1, 1, L)
        y, B = resample_truth(x[:, None], up, down)
        want = strided_convolution_form(x, down, up)
        assert y.shape == (len(want), 1) == (-(-L * up // down), 1)
        assert np.abs(y[:, 0] - want).max() <= 1e-12, (fs, ft, L)
        assert (np.abs(y) <= B + 1e-15).all()


def test_the_tap_counts_and_the_one_to_one_case():
    for ratio, taps in MEASURED_TAPS.items():
        assert filter_table(*ratio)[0] == taps, ratio
    for up, down in RATIOS:
        taps, first, h = filter_table(up, down)
        s = 0.99 * min(up, down) / down
        assert taps <= 2 * math.ceil(6 / s) and h.shape == (up, taps) and first.shape == (up,)
        assert first.max() - first.min() <= 1  # (what the kernel's staged span counts on)
    x = np.random.default_rng(1).uniform(-1, 1, (50, 3))
    y, B = resample_truth(x, 1, 1)
    assert (y == x).all() and (B == np.abs(x)).all()  # (a copy: the formula at 1:1 is not the identity, the definition says copy)
    y, _ = resample_truth(x, 1, 1, downmix=True)
    assert np.allclose(y[:, 0], x.mean(axis=1), rtol=0, atol=1e-16)


def test_a_sine_below_the_new_nyquist_rate_passes_and_one_above_it_does_not():
    up, down = ratio_of(44100, 16000)
    m = np.arange(4410)
    y, _ = resample_truth(np.sin(2 * np.pi * 1000 * m / 44100)[:, None], up, down)
    j = np.arange(len(y))
    assert len(y) == 1600
    err = np.abs(y[:, 0] - np.sin(2 * np.pi * 1000 * j / 16000))[40:-40].max()
    print("1 kHz through 44 100 -> 16 000: largest error 40 samples from the edges %.3g" % err)
    assert err <= 1e-3
    y, _ = resample_truth(np.sin(2 * np.pi * 12000 * m / 44100)[:, None], up, down)
    left = np.abs(y[40:-40, 0]).max()
    print("12 kHz through 44 100 -> 16 000: largest sample 40 samples from the edges %.3g" % left)
    assert left <= 5e-3


def test_the_library_filter_is_the_restatement():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    for up, down in RATIOS + [(1, 1), (1, 32), (1024, 1), (1023, 32735), (33, 1)]:
        taps, first, coeffs = capi.resample_filter(up, down)
        want_taps, want_first, h = filter_table(up, down)
        assert taps == want_taps and first.tolist() == want_first.tolist(), (up, down)
        assert taps <= 388  # (kRsMaxTaps: what the kernel's LDS stage is sized for at the steepest ratio)
        rounded = h.astype(np.float32)
        assert coeffs.shape == rounded.shape
        assert (np.abs(coeffs.astype(np.float64) - rounded.astype(np.float64)) <= np.spacing(np.abs(rounded)).astype(np.float64)).all(), (up, down)
        assert ((coeffs == 0) == (rounded == 0)).all() or np.abs(h[(coeffs == 0) != (rounded == 0)]).max() < 1e-30
    # (33, 1): a tap exactly at the support's edge (|n| * 99 == 600 * 33) is not live in either
    assert not tap_live(200, 33, 1) and tap_live(199, 33, 1)


def test_the_refused_ratios_and_the_size_query():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    L = capi.lib()
    taps = C.c_int32(-1)
    for up, down in [(1025, 1), (1, 33), (3, 97), (2, 2), (4, 6), (0, 1), (1, 0), (-1, 3), (3, -1)]:
        assert not ratio_ok(up, down)
        assert L.vpz_resample_filter(up, down, C.byref(taps), None, None, 0) == capi.E_INVALID_ARG, (up, down)
        with pytest.raises(ValueError):
            capi.resample_filter(up, down)
    assert taps.value == -1
    assert L.vpz_resample_filter(1, 3, None, None, None, 0) == capi.E_INVALID_ARG
    assert L.vpz_resample_filter(1, 3, C.byref(taps), None, None, -1) == capi.E_INVALID_ARG
    for up, down in [(1024, 1), (1, 32), (3, 96 - 1), (1, 1)]:
        assert ratio_ok(up, down) and L.vpz_resample_filter(up, down, C.byref(taps), None, None, 0) == capi.OK and taps.value >= 1
    # a table that does not fit: the size, VPZ_E_CAPACITY, nothing written
    buf = np.full(37, 7.0, dtype=np.float32)
    assert L.vpz_resample_filter(1, 3, C.byref(taps), None, buf.ctypes.data, 36) == capi.E_CAPACITY and taps.value == 37 and (buf == 7.0).all()
    assert L.vpz_resample_filter(1, 3, C.byref(taps), None, buf.ctypes.data, 37) == capi.OK and buf[18] == np.float32(0.33)


def test_the_resample_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import capi
    c = cs.c_functions("vorbispizza_pcm_resample.h", "vpz_")
    imports = imports_of(tmp_path, "GpuPcmResample.cs")
    assert sorted(c) == ["vpz_pcm_resample", "vpz_resample_filter"] == sorted(imports) == sorted(capi.PCM_RESAMPLE_EXPORTED_SYMBOLS)
    pack = cs.c_functions("vorbispizza_pcm_pack.h", "vpz_pcm_")["vpz_pcm_pack"][1]
    # vpz_pcm_pack's parameters with the ratio and the downmix behind `channels` and out_channels in front of `frames`
    assert c["vpz_pcm_resample"] == ("i32", pack[:4] + ["i32", "i32", "i32"] + pack[4:8] + ["i32"] + pack[8:])
    assert c["vpz_resample_filter"] == ("i32", ["i32", "i32", "ptr", "ptr", "ptr", "i64"])
    for name, (ret, params) in c.items():
        assert imports[name] == ("Synth", ret, params), name
    for name, restype, argtypes in capi._PCM_RESAMPLE_SIGNATURES:
        assert ([KINDS[a] for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    structs, defines = cs.c_structs("vorbispizza_pcm_resample.h")
    assert structs == {}  # (vpz_pack_row serves)
    assert defines["VPZ_RESAMPLE_MAX_UP"] == capi.RESAMPLE_MAX_UP == 1024 and defines["VPZ_RESAMPLE_MAX_DOWN_PER_UP"] == capi.RESAMPLE_MAX_DOWN_PER_UP == 32
    text = open(os.path.join(cs.CS, "GpuPcmResample.cs")).read()
    assert "MaxUp = 1024" in text and "MaxDownPerUp = 32" in text and "GpuPcmPack.PackRow* rows" in text
    # the older headers and their lists did not take the new names
    for name in c:
        assert name not in capi.EXPORTED_SYMBOLS + capi.PCM_EXPORTED_SYMBOLS + capi.PCM_PACK_EXPORTED_SYMBOLS
        assert name not in cs.c_functions("vorbispizza_synth.h", "vpz_") and name not in cs.c_functions("vorbispizza_pcm_pack.h", "vpz_")
    assert callable(capi.pcm_resample) and callable(capi.resample_filter)


def test_the_resampled_call_binding_matches_its_header(tmp_path):
    import inspect
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_resample.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiResample.cs")
    assert sorted(c) == ["vpzm_decode_ranges_resampled"] == sorted(imports) == sorted(multi.RESAMPLE_EXPORTED_SYMBOLS)
    batch = cs.c_functions("vorbispizza_multi_batch.h", "vpzm_")["vpzm_decode_ranges_batch"]
    # the batch call's parameters with the rate in front of `channels` and the downmix behind it
    assert c["vpzm_decode_ranges_resampled"] == (batch[0], batch[1][:5] + ["i32"] + batch[1][5:6] + ["i32"] + batch[1][6:])
    assert imports["vpzm_decode_ranges_resampled"] == ("Host",) + c["vpzm_decode_ranges_resampled"]
    fn = multi.lib().vpzm_decode_ranges_resampled
    assert [KINDS.get(a, "ptr") for a in fn.argtypes] == c["vpzm_decode_ranges_resampled"][1] and KINDS[fn.restype] == "i32"
    assert cs.c_structs("vorbispizza_multi_resample.h")[0] == {}
    # the older headers keep their functions, the Python call keeps its defaults
    assert sorted(cs.c_functions("vorbispizza_multi_batch.h", "vpzm_")) == ["vpzm_batch_partition", "vpzm_decode_ranges_batch"] == sorted(multi.BATCH_EXPORTED_SYMBOLS)
    assert len(cs.c_functions("vorbispizza_multi.h", "vpzm_")) == 5
    sig = inspect.signature(multi.Dispatcher.decode_ranges_batch)
    assert sig.parameters["sample_rate"].default is None and sig.parameters["mono"].default is False
    assert list(sig.parameters)[:8] == ["self", "datas", "ranges", "channels", "frames", "planar", "s16", "out"]


def test_the_rate_status_collides_with_no_other():
    from vorbispizza_amd import multi
    st = vpzm_statuses()
    assert st["VPZM_E_RATE"] == multi.E_RATE == -16 and st["VPZM_E_CHANNELS"] == -15
    assert len(set(st.values())) == len(st) and min(st.values()) == -16, st  # (the next free value)
    assert "ERate = -16" in open(os.path.join(cs.CS, "VorbisPizzaMultiResample.cs")).read()


def test_both_libraries_export_the_new_symbols():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import _build, capi, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in capi.PCM_RESAMPLE_EXPORTED_SYMBOLS:
        assert hasattr(S, name), name
    assert hasattr(H, "vpzm_decode_ranges_resampled") and not hasattr(S, "vpzm_decode_ranges_resampled")
    assert "pcm_resample.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "resample_filter.hpp"))


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    for header, body in (("vorbispizza_pcm_resample.h", "sizeof(vpz_pack_row) == 24 && VPZ_RESAMPLE_MAX_UP == 1024"),
                         ("vorbispizza_multi_resample.h", "VPZM_E_RATE == -16 && VPZM_E_CHANNELS == -15")):
        src = tmp_path / (header + ".c")
        src.write_text('#include "%s"\ntypedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % (header, body))
        exe = tmp_path / (header + ".exe")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


def test_the_resample_kernels_use_no_scratch_and_say_what_they_take():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc: a tool, not hardware -- nothing to skip for"
    ks = [k for k in kr.analyse(os.path.join(_build.CSRC, "pcm_resample.hip"), _build.SOURCES["pcm_resample.hip"]) if "pcm_resample_kernel" in k["name"]]
    assert len(ks) == 4  # <float32 / int16, planar / interleaved>
    for k in ks:
        print(k)
        # (the LDS is dynamic, sized per ratio by the launch: at most 42 KiB, 8 KiB at 160 / 441 stereo; no static part)
        assert k.get("scratch", 0) == 0 and k["vgprs"] <= 128 and k["lds"] == 0, k


def test_the_limit_cases_take_every_branch_of_the_plan():
    """the case list of tests/test_pcm_resample_limits_gpu.py against the plan: a changed constant in pcm_resample.hip fails HERE, and the
    list is what to look at then"""
    k = kernel_constants()
    assert k == {"kRsBlock": 256, "kRsLds": 8704, "kRsMaxPass": 8, "kRsMaxTaps": 388}, k
    plans = [(case, launch_plan(*case, k=k)) for case in LIMIT_CASES]
    for (up, down, channels, downmix), pl in plans:
        print("(%d, %d) %d channels%s: taps %d span_cap %d per_pass %d passes %s LDS %d bytes" % (
            up, down, channels, " mixed down" if downmix else "", pl["taps"], pl["span_cap"], pl["per_pass"],
            passes_text(pl["passes"]), pl["lds_bytes"]))
        assert pl["taps"] <= k["kRsMaxTaps"] and pl["span_cap"] <= k["kRsLds"] and pl["lds_bytes"] <= 43008  # (42 KiB)
    assert {pl["per_pass"] for _, pl in plans} >= {1, 2, 3, 4, 5, 8}
    assert any(len(pl["passes"]) > 2 for _, pl in plans)
    assert any(len(pl["passes"]) > 1 and pl["passes"][-1] < pl["passes"][0] for _, pl in plans)
    assert any(len(pl["passes"]) > 1 and pl["passes"][-1] == pl["passes"][0] for _, pl in plans)  # (... and one whose last pass is full)
    assert any(len(pl["passes"]) == 1 and pl["passes"][0] == k["kRsMaxPass"] for _, pl in plans)
    assert any(pl["taps"] == k["kRsMaxTaps"] for _, pl in plans)
    assert any(pl["span_cap"] > 0.98 * k["kRsLds"] for _, pl in plans)
    assert any(case[0] == 1024 for case, _ in plans)
    assert any(pl["first"].max() != pl["first"].min() and pl["per_pass"] == 1 and not case[3] and case[2] > 1 for case, pl in plans)
    assert max(case[2] for case, _ in plans) == 255  # (VPZ_MAX_CHANNELS)


def sweep_ratios():
    """for every `up` of the sweep: the steepest coprime down <= 32 * up, down = 1, down = up + 1 and down = up - 1"""
    out = []
    for up in list(range(1, 65)) + [127, 128, 255, 256, 257, 511, 512, 1023, 1024]:
        steepest = next(d for d in range(32 * up, 0, -1) if math.gcd(up, d) == 1)
        for down in (steepest, 1, up + 1, up - 1):
            if down >= 1 and ratio_ok(up, down) and (up, down) not in out:
                out.append((up, down))
    return out


def test_what_the_staging_counts_on_holds_up_to_the_limits():
    """a phase's first tap is first_min or one more, no filter is longer than kRsMaxTaps, and one channel's span of a tile fits kRsLds"""
    k = kernel_constants()
    ratios = sweep_ratios()
    assert len(ratios) > 250 and (1024, 32767) in ratios and (1, 32) in ratios and (1024, 1) in ratios and (1024, 1023) in ratios
    most = 0
    for up, down in ratios:
        taps, first, _ = filter_table(up, down)
        assert first.max() - first.min() <= 1, (up, down)
        assert taps <= k["kRsMaxTaps"] == 388, (up, down, taps)
        assert (k["kRsBlock"] - 1) * down // up + 2 + taps <= k["kRsLds"] == 8704, (up, down)
        most = max(most, taps)
    print("%d ratios, the largest tap count %d" % (len(ratios), most))
    assert most == 388
