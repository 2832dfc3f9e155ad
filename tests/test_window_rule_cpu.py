"""vpzh_window (include/vorbispizza_front.h) and the two headers of the windowed batch decode -- include/vorbispizza_pcm.h and
include/vorbispizza_multi_ranges.h -- without a GPU: the window rule against a brute-force answer from vpzh_seek for EVERY start of
three streams, the headers as plain C, every declared symbol exported, the Python and C# bindings name by name.  The compute is in
tests/test_multi_ranges_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import binding_support as cs  # noqa: E402
from binding_support import imports_of  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def stream(name):
    import synthetic_streams as ss
    if name.endswith(".ogg"):
        return open(os.path.join(GOLDEN, name), "rb").read()
    st, rng = getattr(ss, name)()
    return bytes(st.build(rng, 12)[0])


@pytest.fixture(scope="module", params=["stereo_coupled_res2", "mono_floor1_res1", "1test.ogg"])
def opened(request):
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(stream(request.param))
    yield request.param, f
    f.close()


def counted_length(f):
    """the largest position vpzh_seek accepts: the counted length, which the last page's granule may cut short"""
    from vorbispizza_amd.front import FrontError
    n = int(f.total_samples)
    while True:
        try:
            f.seek(n + 1)
        except FrontError:
            return n
        n += 1


def residue_values_of(f):
    """residue values of every audio packet, from the records' offsets"""
    pk = f.decode_packets()[0]
    offs = [int(o) for o in pk["residue_offset"]] + [int(f.info.residue_floats)]
    return [offs[i + 1] - offs[i] for i in range(len(pk))]


def test_every_window_is_what_two_seeks_say(opened):
    name, f = opened
    total = int(f.total_samples)
    values = residue_values_of(f)
    assert len(values) == f.audio_packets and total > 0
    for start in range(total + 1):
        first, roll = f.seek(start)
        position = start - roll  # (the counted position the pre-roll packet ends at: where seek(position) rolls 0 ...)
        assert f.seek(position)[1] == 0
        for count in (0, 1, 5, -1, total + 100):
            w = f.window(start, count)
            samples = total - start if count < 0 else min(count, total - start)
            assert w["samples"] == samples and start + w["samples"] <= total, (name, start, count, w)
            assert (w["first_packet"], w["roll_forward"], w["position"]) == (first, roll, position), (name, start, count, w)
            if samples == 0:
                assert w["n_packets"] == 0 and w["residue_values"] == 0, (name, start, count, w)
                continue
            last = f.seek(start + samples - 1)[0] + 1  # the packet that holds the window's last sample
            assert w["n_packets"] == last - first + 1 >= 2, (name, start, count, w)
            assert first + w["n_packets"] <= f.audio_packets
            assert w["residue_values"] == sum(values[first: first + w["n_packets"]]), (name, start, count, w)
    assert f.window(total, 10)["n_packets"] == 0 and f.window(total, -1)["samples"] == 0
    assert f.window(0, -1)["samples"] == total and f.window(0, -1)["n_packets"] == f.audio_packets


def test_a_window_is_bounded_by_the_granule_capped_total(opened):
    from vorbispizza_amd.front import FrontError
    name, f = opened
    total, counted = int(f.total_samples), counted_length(f)
    if name == "1test.ogg":
        assert (total, counted) == (17318, 17856)  # the last page's granule trims 538 samples
    else:
        assert total == counted
    for bad in [-1, -100] + list(range(total + 1, counted + 2)):
        with pytest.raises(FrontError):
            f.window(bad, 1)
        with pytest.raises(FrontError):
            f.window(bad, -1)
    for pos in range(total + 1, counted + 1):  # (seek takes what window refuses)
        f.seek(pos)


def test_null_arguments_are_refused(opened):
    from vorbispizza_amd import front
    L = front.lib()
    out = [C.c_int64() for _ in range(6)]
    refs = [C.byref(v) for v in out]
    assert L.vpzh_window(None, 0, 1, *refs) == -3  # VPZH_E_ARG
    for i in range(6):
        holed = list(refs)
        holed[i] = None
        assert L.vpzh_window(opened[1]._h, 0, 1, *holed) == -3


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    for header, body in (("vorbispizza_pcm.h", "sizeof(uint64_t) == 8"),
                         ("vorbispizza_multi_ranges.h", "sizeof(vpzm_range) == 16 && VPZM_E_RANGE == -14")):
        src = tmp_path / (header + ".c")
        src.write_text('#include "%s"\ntypedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % (header, body))
        exe = tmp_path / (header + ".exe")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


def test_every_declared_symbol_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi, front, multi
    pcm = cs.c_functions("vorbispizza_pcm.h", "vpz_pcm_")
    ranges = cs.c_functions("vorbispizza_multi_ranges.h", "vpzm_")
    assert sorted(pcm) == ["vpz_pcm_download"] == sorted(capi.PCM_EXPORTED_SYMBOLS)
    assert sorted(ranges) == ["vpzm_decode_ranges"] == sorted(multi.RANGES_EXPORTED_SYMBOLS)
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    for name in pcm:
        assert hasattr(S, name), name
    for name in list(ranges) + ["vpzh_window"]:
        assert hasattr(H, name), name
    assert "vpzh_window" in cs.c_functions("vorbispizza_front.h", "vpzh_")
    # the existing headers and bindings did not take the new names
    assert len(cs.c_functions("vorbispizza_multi.h", "vpzm_")) == 5 and "vpz_pcm_download" not in capi.EXPORTED_SYMBOLS


KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}


def test_the_pcm_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import capi
    c = cs.c_functions("vorbispizza_pcm.h", "vpz_pcm_")
    imports = imports_of(tmp_path, "GpuPcmDownload.cs")
    assert sorted(c) == ["vpz_pcm_download"] == sorted(imports) and len(c["vpz_pcm_download"][1]) == 4
    for name, (ret, params) in c.items():
        lib, cs_ret, cs_params = imports[name]
        assert lib == "Synth" and cs_params == params and cs_ret == ret, (name, (ret, params), (cs_ret, cs_params))
    for name, restype, argtypes in capi._PCM_SIGNATURES:
        assert ([KINDS[a] for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    # ... with the parameters of the copy it is the asynchronous form of
    assert c["vpz_pcm_download"] == cs.c_functions("vorbispizza_synth.h", "vpz_")["vpz_memcpy_d2h"]


def test_the_ranges_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_ranges.h", "vpzm_")
    text = open(os.path.join(cs.CS, "VorbisPizzaMultiRanges.cs")).read()
    imports = imports_of(tmp_path, "VorbisPizzaMultiRanges.cs")
    assert sorted(c) == ["vpzm_decode_ranges"] == sorted(imports)
    ret, params = c["vpzm_decode_ranges"]
    assert len(params) == 11 and imports["vpzm_decode_ranges"] == ("Host", ret, params)
    # one parameter more than vpzm_decode_library, the ranges after the sizes
    lib_params = cs.c_functions("vorbispizza_multi.h", "vpzm_")["vpzm_decode_library"][1]
    assert params == lib_params[:4] + ["ptr"] + lib_params[4:]
    cstructs, defines = cs.c_structs("vorbispizza_multi_ranges.h")
    css = cs.cs_structs(os.path.join(cs.CS, "VorbisPizzaMultiRanges.cs"))
    assert sorted(cstructs) == ["vpzm_range"] and sorted(css) == ["Range"]
    for (n0, k0, a0), (n1, k1, a1) in zip(cstructs["vpzm_range"], css["Range"]):
        assert cs.norm(n0) == cs.norm(n1) and k0 == k1 == "i64" and a0 == a1 == 0
    assert list(multi.RANGE_DTYPE.names) == [f[0] for f in cstructs["vpzm_range"]] == ["start", "count"] and multi.RANGE_DTYPE.itemsize == 16
    assert defines["VPZM_E_RANGE"] == multi.E_RANGE == -14 and "ERange = -14" in text
    assert callable(multi.Dispatcher.decode_ranges)


def test_bad_arguments_are_refused_without_a_device():
    from vorbispizza_amd import capi, multi
    L = multi.lib()
    assert L.vpzm_decode_ranges(None, 0, None, None, None, 0, None, None, None, None, None) == multi.E_ARG
    S = capi.lib()
    assert S.vpz_pcm_download(None, None, None, 0) == capi.E_INVALID_ARG
