"""include/vorbispizza_entropy_group.h and include/vorbispizza_multi_mixed.h without a GPU: plain C, their C# and Python bindings
name by name, the kernels of csrc/entropy.hip counted, null handles refused.  The compute is in tests/test_entropy_group_gpu.py
and tests/test_multi_mixed_gpu.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import binding_support as cs  # noqa: E402
from binding_support import imports_of  # noqa: E402


def test_the_new_headers_are_plain_c(tmp_path):
    assert shutil.which("gcc"), "the check needs a C compiler (gcc): a tool, not hardware -- nothing to skip for"
    src = tmp_path / "headers.c"
    src.write_text('#include "vorbispizza_entropy_group.h"\n#include "vorbispizza_multi_mixed.h"\n'
                   'typedef char counts_are_64_bytes[sizeof(vpzm_call_counts) == 64 ? 1 : -1];\n'
                   'int main(void) { return (int)sizeof(counts_are_64_bytes) - 1; }\n')
    exe = tmp_path / "headers"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
    from vorbispizza_amd import multi
    assert C.sizeof(multi.CallCounts) == 64


def test_the_group_binding_matches_its_header(tmp_path):
    c = cs.c_functions("vorbispizza_entropy_group.h", "vpz_entropy_group_")
    imports = imports_of(tmp_path, "GpuEntropyGroup.cs")
    assert sorted(c) == ["vpz_entropy_group_create", "vpz_entropy_group_decode", "vpz_entropy_group_destroy"] == sorted(imports)
    assert len(c["vpz_entropy_group_decode"][1]) == 16
    for name, (ret, params) in c.items():
        lib, cs_ret, cs_params = imports[name]
        assert lib == "Synth" and cs_params == params and cs_ret == ret, (name, (ret, params), (cs_ret, cs_params))
    _, defines = cs.c_structs("vorbispizza_entropy_group.h")
    assert defines["VPZ_ENTROPY_GROUP_MAX_SETUPS"] == 256
    assert "MaxSetups = 256" in open(os.path.join(cs.CS, "GpuEntropyGroup.cs")).read()
    # ... and the ctypes signatures have the header's kinds
    from vorbispizza_amd import entropy
    kinds = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_int: "i32", C.POINTER(C.c_void_p): "ptr", None: "void"}
    assert sorted(entropy.GROUP_EXPORTED_SYMBOLS) == sorted(c)
    for name, restype, argtypes in entropy._GROUP_SIGNATURES:
        assert ([kinds[a] for a in argtypes], kinds[restype]) == (c[name][1], c[name][0]), name
    assert entropy.GROUP_MAX_SETUPS == 256


def test_the_mixed_dispatcher_binding_matches_its_header(tmp_path):
    c = cs.c_functions("vorbispizza_multi_mixed.h", "vpzm_")
    imports = imports_of(tmp_path, "VorbisPizzaMultiMixed.cs")
    assert sorted(c) == ["vpzm_last_call_counts", "vpzm_set_mixed_setups"] == sorted(imports)
    for name, (ret, params) in c.items():
        lib, cs_ret, cs_params = imports[name]
        assert lib == "Host" and cs_params == params and cs_ret == ret, (name, (ret, params), (cs_ret, cs_params))
    cstructs, _ = cs.c_structs("vorbispizza_multi_mixed.h")
    css = cs.cs_structs(os.path.join(cs.CS, "VorbisPizzaMultiMixed.cs"))
    assert sorted(cstructs) == ["vpzm_call_counts"] and sorted(css) == ["CallCounts"]
    cf, sf = cstructs["vpzm_call_counts"], css["CallCounts"]
    assert len(cf) == len(sf) == 6
    for (n0, k0, a0), (n1, k1, a1) in zip(cf, sf):
        assert cs.norm(n0) == cs.norm(n1) and k0 == k1 and a0 == a1, ((n0, k0, a0), (n1, k1, a1))
    from vorbispizza_amd import multi
    assert [f[0] for f in multi.CallCounts._fields_] == [f[0] for f in cf]
    assert sorted(multi.MIXED_EXPORTED_SYMBOLS) == sorted(c)
    # the existing headers and bindings did not take the new names
    assert len(cs.c_functions("vorbispizza_multi.h", "vpzm_")) == 5 and len(cs.c_functions("vorbispizza_entropy.h", "vpz_entropy_")) == 4


def test_mixed_setups_is_the_dispatchers_last_keyword():
    from vorbispizza_amd import multi
    params = list(inspect.signature(multi.Dispatcher.__init__).parameters.values())
    assert params[-1].name == "mixed_setups" and params[-1].default is False
    assert [p.name for p in params[1:-1]] == ["device_ids", "host_threads", "streams_per_call", "contexts_per_device", "clip_samples",
                                              "slots_per_device", "float_residue", "gpu_entropy"]
    assert callable(multi.Dispatcher.call_counts)


def test_the_kernels_of_the_entropy_unit():
    """two entropy_group_kernel instantiations next to the two each of entropy_decode_kernel and entropy_zero_kernel, none with
    scratch or LDS, and the group kernel at no fewer waves per SIMD than the kernel it restates"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from vorbispizza_amd import _build
    assert shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc()), "the check needs hipcc, as the build does"
    import kernel_resources as kr
    ks = kr.analyse(os.path.join(_build.CSRC, "entropy.hip"), _build.SOURCES["entropy.hip"])
    by = {}
    for k in ks:
        for name in ("entropy_group_kernel", "entropy_decode_kernel", "entropy_zero_kernel"):
            if name in k["demangled"]:
                by.setdefault(name, []).append(k)
    assert {name: len(v) for name, v in by.items()} == {"entropy_group_kernel": 2, "entropy_decode_kernel": 2, "entropy_zero_kernel": 2}
    assert len(ks) == 6
    for k in ks:
        assert k.get("scratch", 1) == 0 and k.get("lds", 1) == 0, k["demangled"]
    assert min(k["occupancy"] for k in by["entropy_decode_kernel"]) >= 4
    assert min(k["occupancy"] for k in by["entropy_group_kernel"]) >= min(k["occupancy"] for k in by["entropy_decode_kernel"])


def test_null_handles_are_refused_without_a_device():
    from vorbispizza_amd import entropy, multi
    L = multi.lib()
    counts = multi.CallCounts()
    assert L.vpzm_set_mixed_setups(None, 1) == multi.E_ARG
    assert L.vpzm_last_call_counts(None, C.byref(counts)) == multi.E_ARG
    E = entropy.lib()
    h = C.c_void_p()
    assert E.vpz_entropy_group_create(None, None, None, 1, C.byref(h)) == -1 and not h.value  # VPZ_E_INVALID_ARG
    assert E.vpz_entropy_group_decode(None, 0, None, None, 0, None, None, None, 0, 0, None, 0, None, None, 0, 0) == -1
    E.vpz_entropy_group_destroy(None)
