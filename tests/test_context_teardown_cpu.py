"""What a context owns it also gives back: every std::map and every Scratch record of struct Context (csrc/vpz_internal.hpp) is named in
free_pcm_state or in vpz_context_destroy (csrc/vpz_context.hip), as the comment on free_pcm_state asks of a stage that adds one.  Read
from the source text (tests/kernel_text.py): a map that a new stage adds and no teardown names leaks its tables with every context, and
nothing else in the suite would see it.  The member counts are literals; the check is shown to fail on the struct with one more map."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from kernel_text import function_body, members_of_type, source_text, struct_body  # noqa: E402

MAPS = ["tables", "resample_tables", "logmel_dft", "logmel_banks", "fbank_tables", "fbank_banks", "mfcc_tables", "stft_tables", "cqt_tables",
        "loudness_rates"]
SCRATCH = ["stage_in", "stage_out", "loud_scratch", "tp_scratch"]


def kept(struct):
    """(the maps, the Scratch records) of a struct body"""
    return members_of_type(struct, r"std::map\s*<.*>"), members_of_type(struct, r"Scratch")


def not_given_back(struct, teardown):
    """the maps and Scratch records of the struct body that no teardown body names as a member of the context"""
    maps, scratch = kept(struct)
    return [name for name in maps + scratch if not any(re.search(r"->\s*%s\b" % name, body) for body in teardown)]


def tree():
    context = source_text("vpz_context.hip")
    return struct_body(source_text("vpz_internal.hpp"), "Context"), [function_body(context, "free_pcm_state"), function_body(context, "vpz_context_destroy")]


def test_every_map_and_scratch_record_of_the_context_is_given_back():
    struct, teardown = tree()
    maps, scratch = kept(struct)
    assert maps == MAPS and scratch == SCRATCH  # (ten maps, four records: a new one is added here and to free_pcm_state)
    assert not_given_back(struct, teardown) == []
    # the eight maps of device tables go through free_tables, which frees every record's one allocation
    for name in MAPS[1:-1]:
        assert "free_tables(ctx->%s);" % name in teardown[0], name
    assert "vpz::free_pcm_state(ctx);" in teardown[1]


def test_the_check_sees_a_member_that_no_teardown_names():
    struct, teardown = tree()
    more = struct + "\n    std::map<std::array<int, 2>, LogmelDft> chroma_tables;\n    Scratch chroma_scratch{nullptr, 0, true};\n"
    assert kept(more) == (MAPS + ["chroma_tables"], SCRATCH + ["chroma_scratch"])
    assert not_given_back(more, teardown) == ["chroma_tables", "chroma_scratch"]
    # a member whose name another member's begins with is not named by it
    assert not_given_back(struct + "\n    std::map<int, LogmelDft> stft;\n", teardown) == ["stft"]
    assert not_given_back(more, teardown + ["free_tables(ctx->chroma_tables); hipFree(ctx->chroma_scratch.p);"]) == []
    # and a teardown that drops one line misses exactly that map
    assert not_given_back(struct, [teardown[0].replace("free_tables(ctx->cqt_tables);", ""), teardown[1]]) == ["cqt_tables"]
