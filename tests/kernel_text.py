"""What the tests read out of the kernels' source text: the integer constants a .hip file states, which the restated launch plans of the
truth modules start from; the members of a struct and the body of a function, for tests/test_context_teardown_cpu.py."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vorbispizza_amd", "csrc")


def kernel_constants(path_under_csrc, names):
    """{name: value} of the `constexpr int name = value;` lines of one file, each of them stated exactly once"""
    text = open(os.path.join(CSRC, path_under_csrc)).read()
    out = {}
    for name in names:
        found = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert len(found) == 1, name
        out[name] = int(found[0])
    return out


def source_text(path_under_csrc):
    """a file of csrc without its comments"""
    text = open(os.path.join(CSRC, path_under_csrc)).read()
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def braced(text, at):
    """the text between the brace at or behind `at` and the brace that closes it"""
    start = text.index("{", at)
    depth = 0
    for i in range(start, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[start + 1: i]
    raise AssertionError("a brace is not closed")


def struct_body(text, name):
    """the body of `struct name {...}` in comment-free text, the bodies of the structs nested in it taken out"""
    found = [m for m in re.finditer(r"\bstruct\s+%s\b[^;{]*\{" % name, text)]
    assert len(found) == 1, name
    body = braced(text, found[0].start())
    while True:
        inner = re.search(r"\bstruct\s+\w+[^;{]*\{", body)
        if inner is None:
            return body
        end = body.index("{", inner.start()) + len(braced(body, inner.start())) + 2
        body = body[: inner.start()] + body[end:]


def function_body(text, name):
    """the body of the one definition of `name` in comment-free text (a call or a declaration has no brace behind its parentheses)"""
    found = [m for m in re.finditer(r"\b%s\s*\([^;{}]*\)\s*\{" % name, text)]
    assert len(found) == 1, name
    return braced(text, found[0].start())


def members_of_type(body, type_pattern):
    """the names of a struct body's members whose type matches: `type a, b{...};` declares both"""
    names = []
    for statement in body.split(";"):
        m = re.match(r"\s*(%s)\s+(.*)" % type_pattern, statement, flags=re.S)
        if m:
            declarators = re.sub(r"\{[^{}]*\}", "", m.group(2))  # (brace initialisers)
            names += [re.match(r"\s*(\w+)", part).group(1) for part in declarators.split(",")]
    return names


def constants_of(path_under_csrc, names):
    """a kind's reader of its own file: called with nothing, or with the repository root that some callers still hand over"""
    return lambda root=None: kernel_constants(path_under_csrc, names)
