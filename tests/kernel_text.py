"""What the tests read out of the kernels' source text: the integer constants a .hip file states, which the restated launch plans of the
truth modules start from."""
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


def constants_of(path_under_csrc, names):
    """a kind's reader of its own file: called with nothing, or with the repository root that some callers still hand over"""
    return lambda root=None: kernel_constants(path_under_csrc, names)
