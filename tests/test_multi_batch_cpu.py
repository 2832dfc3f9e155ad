"""include/vorbispizza_pcm_pack.h and include/vorbispizza_multi_batch.h without a GPU: the C# files against their headers (the helpers of
tests/test_csharp_binding_cpu.py), the Python signatures against the headers, the new status, the partition rule and the exports."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import binding_support as cs  # noqa: E402
from binding_support import imports_of, vpzm_statuses  # noqa: E402

KINDS = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_int: "i32", None: "void"}


def test_the_pack_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import capi
    c = cs.c_functions("vorbispizza_pcm_pack.h", "vpz_pcm_")
    imports = imports_of(tmp_path, "GpuPcmPack.cs")
    assert sorted(c) == ["vpz_pcm_pack"] == sorted(imports) == sorted(capi.PCM_PACK_EXPORTED_SYMBOLS)
    ret, params = c["vpz_pcm_pack"]
    assert params == ["ptr", "ptr", "i64", "i32", "i32", "ptr", "ptr", "i64", "i64", "i32"] and ret == "i32"
    assert imports["vpz_pcm_pack"] == ("Synth", ret, params)
    for name, restype, argtypes in capi._PCM_PACK_SIGNATURES:
        assert ([KINDS[a] for a in argtypes], KINDS[restype]) == (c[name][1], c[name][0]), name
    cstructs, _ = cs.c_structs("vorbispizza_pcm_pack.h")
    css = cs.cs_structs(os.path.join(cs.CS, "GpuPcmPack.cs"))
    assert sorted(cstructs) == ["vpz_pack_row"] and sorted(css) == ["PackRow"]
    assert len(cstructs["vpz_pack_row"]) == len(css["PackRow"]) == 3
    for (n0, k0, a0), (n1, k1, a1) in zip(cstructs["vpz_pack_row"], css["PackRow"]):
        assert cs.norm(n0) == cs.norm(n1) and k0 == k1 == "i64" and a0 == a1 == 0
    assert list(capi.PACK_ROW_DTYPE.names) == [f[0] for f in cstructs["vpz_pack_row"]] == ["src", "samples", "row"]
    assert capi.PACK_ROW_DTYPE.itemsize == 24
    # the product header and its binding did not take the new name
    assert "vpz_pcm_pack" not in capi.EXPORTED_SYMBOLS and "vpz_pcm_pack" not in capi.PCM_EXPORTED_SYMBOLS
    assert "vpz_pcm_pack" not in cs.c_functions("vorbispizza_synth.h", "vpz_") and "vpz_pcm_pack" not in cs.c_functions("vorbispizza_pcm.h", "vpz_")


def test_the_batch_binding_matches_its_header(tmp_path):
    from vorbispizza_amd import multi
    c = cs.c_functions("vorbispizza_multi_batch.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiBatch.cs")
    assert sorted(c) == ["vpzm_batch_partition", "vpzm_decode_ranges_batch"] == sorted(imports) == sorted(multi.BATCH_EXPORTED_SYMBOLS)
    for name, (ret, params) in c.items():
        assert imports[name] == ("Host", ret, params), (name, (ret, params), imports[name])
    assert c["vpzm_batch_partition"] == ("i32", ["ptr", "i32", "i32", "ptr", "ptr"])
    # the ranges call's parameters up to the ranges, then channels, frames and the layout, the groups' pieces, results and stats
    ranges = cs.c_functions("vorbispizza_multi_ranges.h", "vpzm_")["vpzm_decode_ranges"][1]
    assert c["vpzm_decode_ranges_batch"][1] == ranges[:5] + ["i32", "i64", "i32", "ptr"] + ranges[-2:]
    L = multi.lib()
    for name, (ret, params) in c.items():
        fn = getattr(L, name)
        assert [KINDS.get(a, "ptr") for a in fn.argtypes] == params and KINDS[fn.restype] == ret, name
    assert callable(multi.Dispatcher.decode_ranges_batch) and callable(multi.Dispatcher.batch_partition)
    assert cs.c_structs("vorbispizza_multi_batch.h")[0] == {}  # (no struct of its own: the ranges', the results' and the stats' serve)
    assert len(cs.c_functions("vorbispizza_multi.h", "vpzm_")) == 5 and sorted(cs.c_functions("vorbispizza_multi_ranges.h", "vpzm_")) == ["vpzm_decode_ranges"]


def test_the_channels_status_collides_with_no_other():
    from vorbispizza_amd import multi
    st = vpzm_statuses()
    assert st["VPZM_E_CHANNELS"] == multi.E_CHANNELS == -15 and len(st) >= 9
    assert len(set(st.values())) == len(st), st
    text = open(os.path.join(cs.CS, "VorbisPizzaMultiBatch.cs")).read()
    assert "EChannels = -15" in text
    py = [multi.E_ARG, multi.E_DEVICE, multi.E_NOMEM, multi.E_OPEN, multi.E_CAPACITY, multi.E_SYNTH, multi.E_SETUP, multi.E_RANGE, multi.E_CHANNELS]
    assert len(set(py)) == len(py) and set(py) <= set(st.values())


def partition_rule():
    """the body of `partition` in host/vorbis_multi.cpp, restated in Python: lo and hi as functions of (n, g, D)"""
    text = open(os.path.join(ROOT, "vorbispizza_amd", "host", "vorbis_multi.cpp")).read()
    body = re.search(r"static void partition\(int32_t n, int g, int D, int32_t \*lo, int32_t \*hi\)\s*\{(.*?)\n\}", text, flags=re.S).group(1)
    rules = {}
    for which, expr in re.findall(r"\*(lo|hi) = \(int32_t\)\((.*?)\);", body):
        expr = expr.replace("(int64_t)", "")
        assert re.fullmatch(r"[nDg\s\d\+\*/\(\)]+", expr), expr
        rules[which] = eval("lambda n, g, D: " + expr.replace("/", "//"))
    assert sorted(rules) == ["hi", "lo"]
    # ... and it is the only statement: decode_call and vpzm_batch_partition both call it, nothing else divides by the group count
    assert text.count("partition(n, d, D, &lo, &hi)") == 1 and text.count("partition(n, group, (int)m->groups.size(), lo, hi)") == 1
    assert len(re.findall(r"\* *\(?d *\+ *1\)? */ *D", text)) == 0
    return rules


def test_the_partition_rule():
    from vorbispizza_amd import sharding
    rules = partition_rule()
    for D in range(1, 9):
        for n in range(0, 41):
            cuts = [(rules["lo"](n, g, D), rules["hi"](n, g, D)) for g in range(D)]
            assert cuts == [(n * g // D, n * (g + 1) // D) for g in range(D)]
            assert cuts[0][0] == 0 and cuts[-1][1] == n and all(cuts[g][1] == cuts[g + 1][0] for g in range(D - 1))
            if n % D == 0:  # (the sizes shard_range gives)
                assert [tuple(sharding.shard_range(n, D, g)) for g in range(D)] == cuts


def test_both_libraries_export_the_new_symbols():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi, front, multi
    S, H = C.CDLL(capi.LIB_PATH), front.lib()
    assert hasattr(S, "vpz_pcm_pack") and not hasattr(S, "vpzm_decode_ranges_batch")
    for name in multi.BATCH_EXPORTED_SYMBOLS:
        assert hasattr(H, name), name
    assert "pcm_pack.hip" in __import__("vorbispizza_amd._build", fromlist=["SOURCES"]).SOURCES


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    for header, body in (("vorbispizza_pcm_pack.h", "sizeof(vpz_pack_row) == 24"),
                         ("vorbispizza_multi_batch.h", "VPZM_E_CHANNELS == -15 && VPZM_E_RANGE == -14")):
        src = tmp_path / (header + ".c")
        src.write_text('#include "%s"\ntypedef char holds[(%s) ? 1 : -1];\nint main(void) { return (int)sizeof(holds) - 1; }\n' % (header, body))
        exe = tmp_path / (header + ".exe")
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", cs.INC, str(src), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0
