"""The shape of the test tree itself: no module imports a test module, the support modules (every tests/*.py that is neither a test module
nor conftest.py) import only each other, the package, numpy / torch / pytest and the standard library, without a cycle, and the helpers
that every kind used to carry a copy of are defined once.  The expectations are literals, not read off the tree."""
import ast
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIRD_PARTY = {"numpy", "torch", "pytest"}
PROJECT = {"vorbispizza_amd", "oracle", "__graft_entry__"}
ONCE = ("ctx", "kernel_constants", "fma32", "_fma", "network32")


def modules():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    assert len(paths) > 100
    return {p: ast.parse(open(p).read()) for p in paths}


def imported(tree):
    """the top-level name of every module imported anywhere in the file"""
    out = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            out |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            out.add(node.module.split(".")[0])
    return out


def support():
    return {os.path.basename(p)[:-3]: t for p, t in modules().items()
            if os.path.dirname(p).endswith("tests") and not os.path.basename(p).startswith(("test_", "conftest"))}


def test_no_module_imports_a_test_module():
    bad = [(os.path.relpath(p, ROOT), m) for p, t in modules().items() for m in sorted(imported(t)) if m.startswith("test_")]
    assert bad == []


def test_support_modules_import_only_each_other_the_package_and_the_libraries_without_a_cycle():
    mods = support()
    assert {"helpers", "gpu_context", "multi_support", "pcm_support", "synth_support", "binding_support", "logmel_truth", "resample_truth",
            "f32_model"} <= set(mods)
    allowed = set(sys.stdlib_module_names) | THIRD_PARTY | PROJECT | set(mods)
    graph = {}
    for name, tree in mods.items():
        assert imported(tree) <= allowed, (name, sorted(imported(tree) - allowed))
        graph[name] = imported(tree) & set(mods)
    done, on_path = set(), []

    def visit(name):
        assert name not in on_path, "a cycle: %s" % " -> ".join(on_path[on_path.index(name):] + [name])
        if name not in done:
            on_path.append(name)
            for other in sorted(graph[name]):
                visit(other)
            on_path.pop()
            done.add(name)

    for name in sorted(graph):
        visit(name)


def test_the_shared_helpers_are_defined_once():
    where = {name: [] for name in ONCE}
    for p, tree in modules().items():
        if os.path.dirname(p).endswith("tests"):
            for st in tree.body:
                if isinstance(st, (ast.FunctionDef, ast.AsyncFunctionDef)) and st.name in where:
                    where[st.name].append(os.path.basename(p))
    assert where == {"ctx": ["gpu_context.py"], "kernel_constants": ["kernel_text.py"], "fma32": ["f32_model.py"], "_fma": [],
                     "network32": ["f32_model.py"]}
