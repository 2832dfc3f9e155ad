"""vpzm_options.gpu_entropy and the two statistics it brought (include/vorbispizza_multi.h): the option took the first of
the two reserved words, the statistics were appended -- nothing a caller built against the earlier structs reads or writes
has moved.  Layouts as the C compiler has them against the ctypes mirror; no device needed.  The behaviour is
tests/test_multi_entropy_gpu.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the layout before the option existed (x86-64 / C alignment): what older callers were compiled with
OPTIONS_BEFORE = {"host_threads": 0, "streams_per_call": 4, "contexts_per_device": 8, "clip_samples": 12, "slots_per_device": 16,
                  "float_residue": 20}
STATS_BEFORE = {"wall_s": 0, "device_wall_s": 8, "device_decode_s": 136, "device_synth_s": 264, "device_streams": 392,
                "device_samples": 520, "threads_per_device": 648, "pinned_mib": 652}
STATS_SIZE_BEFORE = 656


def test_the_option_took_a_reserved_word_and_nothing_moved():
    from vorbispizza_amd import multi
    for name, off in OPTIONS_BEFORE.items():
        assert getattr(multi.Options, name).offset == off, name
    assert multi.Options.gpu_entropy.offset == 24 and multi.Options.gpu_entropy.size == 4
    assert multi.Options.reserved.offset == 28 and multi.Options.reserved.size == 4
    assert C.sizeof(multi.Options) == 32


def test_the_statistics_were_appended():
    from vorbispizza_amd import multi
    for name, off in STATS_BEFORE.items():
        assert getattr(multi.Stats, name).offset == off, name
    # two int64 arrays after pinned_mib (an int32 at 652: the struct was 656 bytes, 8-aligned already)
    assert multi.Stats.device_gpu_entropy_streams.offset == STATS_SIZE_BEFORE
    assert multi.Stats.device_gpu_entropy_streams.size == 16 * 8
    assert multi.Stats.device_payload_bytes.offset == STATS_SIZE_BEFORE + 128
    assert C.sizeof(multi.Stats) == STATS_SIZE_BEFORE + 256
    assert [f[0] for f in multi.Stats._fields_][-2:] == ["device_gpu_entropy_streams", "device_payload_bytes"]


def test_the_c_compiler_agrees(tmp_path):
    from vorbispizza_amd import multi
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "vorbispizza_multi.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(vpzm_options), offsetof(vpzm_options, gpu_entropy), offsetof(vpzm_options, reserved),
           sizeof(vpzm_stats), offsetof(vpzm_stats, pinned_mib), offsetof(vpzm_stats, device_gpu_entropy_streams),
           offsetof(vpzm_stats, device_payload_bytes));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 24, 28, STATS_SIZE_BEFORE + 256, 652, STATS_SIZE_BEFORE, STATS_SIZE_BEFORE + 128]
    assert got[0] == C.sizeof(multi.Options) and got[3] == C.sizeof(multi.Stats)


def test_the_dispatcher_takes_the_argument_and_defaults_to_off():
    from vorbispizza_amd import multi
    p = inspect.signature(multi.Dispatcher.__init__).parameters
    assert "gpu_entropy" in p and p["gpu_entropy"].default is False


def test_the_plan_counts_the_packets_it_gives_up():
    """vpzh_plan_range marks a packet with an unused mode number "not decoded" -- the one failure a setup the device can decode
    has -- and vpzh_decode_failures then reports what it reports after the host's own decode of the same container: the
    dispatcher's skipped_packets of a device-decoded stream come from there."""
    import sys

    import numpy as np
    sys.path.insert(0, os.path.dirname(__file__))
    import synthetic_streams as ss
    from synth_support import damage_audio
    from vorbispizza_amd.front import OggVorbisFile
    stream, rng = ss.ALL["mono_floor1_res1"]()  # (three modes in a two-bit field: mode number 3 is unused)
    ogg, _ = stream.build(rng, 24)
    seen = 0
    for seed, hits in ((6, 16), (24, 4), (1, 4)):
        f = OggVorbisFile(damage_audio(bytes(ogg), seed, hits))
        assert f.gpu_decode_supported
        decoded = f.decode_packets()[0]
        want = f.decode_failures()
        planned = f.plan_packets()[0]
        assert f.decode_failures() == want, (seed, hits)
        assert np.array_equal(decoded, planned)
        seen += want[0]
    assert seen >= 2  # (seeds 6 and 24 each hit a mode field)
