"""The host half of the GPU entropy decode (vorbispizza_front.h / vorbispizza_entropy.h), no GPU needed: which setups the
device can decode, the setup image, and the plan -- packet records byte for byte what the CPU decode writes, the payload
spans holding each packet's bytes.  Also the new header as C99, its C# binding and the kernels' resources."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from synth_support import HEADER_EDGE, header_edge_stream, streams  # noqa: E402
GOLDEN = os.path.join(ROOT, "tests", "golden")


def ogg_packets(raw):
    """Every packet of the first logical stream of an undamaged container (page lacing joined), headers included."""
    out, pending, pos, serial = [], b"", 0, None
    while pos + 27 <= len(raw):
        assert raw[pos:pos + 4] == b"OggS"
        nseg = raw[pos + 26]
        lacing = raw[pos + 27:pos + 27 + nseg]
        ser = struct.unpack_from("<I", raw, pos + 14)[0]
        body = pos + 27 + nseg
        size = sum(lacing)
        if serial is None:
            serial = ser
        if ser == serial:
            at = body
            for lv in lacing:
                pending += raw[at:at + lv]
                at += lv
                if lv < 255:
                    out.append(pending)
                    pending = b""
        pos = body + size
    return out


@pytest.fixture(scope="module")
def front():
    sys.path.insert(0, ROOT)
    from vorbispizza_amd import front
    front.lib()
    return front


def test_eligibility_follows_the_setup(front):
    """Supported exactly when every floor is type 1 (the writer's streams all tile their residue partitions); an unsupported
    stream says why and has no setup image."""
    seen = {True: 0, False: 0}
    for name, raw in streams():
        f = front.OggVorbisFile(raw)
        floor0 = any(isinstance(fl, dict) for fl in f.floors)
        assert f.gpu_decode_supported == (not floor0), name
        seen[f.gpu_decode_supported] += 1
        if floor0:
            assert "floor of type 0" in f.last_error()
            with pytest.raises(front.FrontError):
                f.entropy_setup()
        else:
            img = f.entropy_setup()
            magic, version, total = struct.unpack_from("<III", img, 0)
            assert (magic, version, total) == (0x45505A56, 1, len(img)), name
            channels, bs0, bs1 = struct.unpack_from("<iii", img, 12)
            assert (channels, bs0, bs1) == (f.channels, f.block_size0, f.block_size1), name
        f.close()
    assert seen[True] >= 15 and seen[False] >= 1


def test_hostile_setups_are_either_supported_or_say_why(front):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostile_setups as hs
    reasons = ("floor of type 0", "do not tile", "master book", "class book")
    for name, seed, raw in hs.committed_cases():
        try:
            f = front.OggVorbisFile(raw)
        except front.FrontError:
            continue
        if f.gpu_decode_supported:
            assert len(f.entropy_setup()) > 0, (name, seed)
            assert not any(isinstance(fl, dict) for fl in f.floors)
        else:
            assert any(r in f.last_error() for r in reasons), (name, seed, f.last_error())
        f.close()


@pytest.mark.parametrize("cut", [(0, None), (0, 1), (1, 7), (5, 40), ("last", 1)])
def test_plan_records_equal_the_cpu_decode(front, cut):
    for name, raw in streams():
        f = front.OggVorbisFile(raw)
        if not f.gpu_decode_supported:
            continue
        n = f.audio_packets
        first, count = cut
        first = n - 1 if first == "last" else min(first, n)
        count = n - first if count is None else min(count, n - first)
        stream_id, base = 3, 1000
        packets, spans, payload, used = f.plan_packets(first, count, stream_id, base)
        ref = front.capi.make_packets(count)
        res = np.zeros(max(1, count * f.channels * f.block_size1 // 2), dtype=np.float32)
        posts = np.zeros((count * f.channels, 64), dtype=np.int16)
        counts = np.zeros(count * f.channels, dtype=np.uint8)
        ref_used = C.c_int64()
        rc = front.lib().vpzh_decode_range_ex(f._h, first, count, stream_id, base, ref.ctypes.data, res.ctypes.data, posts.ctypes.data,
                                              counts.ctypes.data, C.byref(ref_used), None, None, 0)
        assert rc == 0
        assert packets.tobytes() == ref.tobytes(), (name, cut)
        assert used == ref_used.value, (name, cut)
        f.close()


@pytest.mark.parametrize("name", sorted(HEADER_EDGE))
def test_header_edge_packets_give_the_written_down_records(front, name):
    flags, failures = HEADER_EDGE[name]
    f = front.OggVorbisFile(header_edge_stream(name))
    assert f.audio_packets == 10 and f.gpu_decode_supported
    planned = f.plan_packets()[0]
    assert list(planned["flags"]) == flags
    assert f.decode_failures() == failures  # (as the plan counts them ...
    decoded = f.decode_packets()[0]
    assert decoded.tobytes() == planned.tobytes() and list(decoded["flags"]) == flags
    assert f.decode_failures() == failures  # ... and as the decode does)
    f.close()


def test_payload_spans_reproduce_the_packets(front):
    for name, raw in streams():
        f = front.OggVorbisFile(raw)
        if not f.gpu_decode_supported:
            continue
        audio = ogg_packets(raw)[3:]
        assert len(audio) == f.audio_packets, name
        packets, spans, payload, _ = f.plan_packets()
        for k, (off, size) in enumerate(spans):
            assert payload[off:off + size].tobytes() == audio[k], (name, k)
        end = int(spans[-1][0] + spans[-1][1])
        assert payload.size >= end + 8 and not payload[end:].any(), name
        # a range starts its own payload at 0
        _, spans2, payload2, _ = f.plan_packets(2, 3)
        assert spans2[0][0] == 0 and payload2[:spans2[0][1]].tobytes() == audio[2]
        f.close()


def test_equal_setup_headers_give_identical_images(front):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synthetic_streams as ss
    st, _ = ss.stereo_coupled_res2()
    a, _ = st.build(np.random.default_rng(10), 12)
    b, _ = st.build(np.random.default_rng(11), 17)
    assert bytes(a) != bytes(b)
    fa, fb = front.OggVorbisFile(bytes(a)), front.OggVorbisFile(bytes(b))
    assert fa.entropy_setup() == fb.entropy_setup()
    # ... and the same across two opens of one file
    raw = open(os.path.join(GOLDEN, "3test.ogg"), "rb").read()
    assert front.OggVorbisFile(raw).entropy_setup() == front.OggVorbisFile(raw).entropy_setup()


def test_plan_refuses_a_small_payload_and_writes_nothing(front):
    f = front.OggVorbisFile(open(os.path.join(GOLDEN, "1test.ogg"), "rb").read())
    need = C.c_int64()
    assert front.lib().vpzh_plan_range(f._h, 0, f.audio_packets, 0, 0, None, None, None, 0, C.byref(need), None) == 0
    buf = np.full(need.value - 1, 0xAB, dtype=np.uint8)
    packets = front.capi.make_packets(f.audio_packets)
    assert front.lib().vpzh_plan_range(f._h, 0, f.audio_packets, 0, 0, packets.ctypes.data, None, buf.ctypes.data, buf.size,
                                       C.byref(need), None) == -3
    assert (buf == 0xAB).all() and not packets.tobytes().strip(b"\0")
    assert front.lib().vpzh_plan_range(f._h, 0, f.audio_packets + 1, 0, 0, None, None, None, 0, None, None) == -3


def test_entropy_header_compiles_as_c99(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "entropy.c"
    src.write_text('#include <stddef.h>\n#include "vorbispizza_entropy.h"\n#include "vorbispizza_front.h"\n'
                   "typedef char hdr[sizeof(vpz_entropy_image_header) == 80 ? 1 : -1];\n"
                   "typedef char span[sizeof(vpz_entropy_span) == 16 ? 1 : -1];\n"
                   "int main(void) { return (int)sizeof(hdr) + (int)sizeof(span) - 2; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "entropy.o")], check=True, capture_output=True)


def test_the_csharp_binding_matches_the_entropy_header():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from binding_support import CS, c_functions, cs_imports
    c = c_functions("vorbispizza_entropy.h", "vpz_entropy_")
    front_syms = c_functions("vorbispizza_front.h", "vpzh_")
    host = {n: front_syms[n] for n in ("vpzh_gpu_decode_supported", "vpzh_get_entropy_setup", "vpzh_plan_range")}
    cs = cs_imports(os.path.join(CS, "GpuEntropyDecode.cs"))
    assert len(c) == 4 and len(c["vpz_entropy_decode"][1]) == 13
    assert sorted(cs) == sorted(list(c) + list(host))
    for name, (ret, params) in list(c.items()) + list(host.items()):
        lib, cs_ret, cs_params = cs[name]
        assert lib == ("Host" if name.startswith("vpzh_") else "Synth"), name
        assert cs_params == params and cs_ret == ret, (name, (ret, params), (cs_ret, cs_params))


def test_the_entropy_kernels_use_no_scratch():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from vorbispizza_amd import _build
    if not (shutil.which(_build._hipcc()) or os.path.exists(_build._hipcc())):
        pytest.skip("no hipcc")
    import kernel_resources as kr
    units = dict((os.path.basename(s), e) for s, e in kr.all_units())
    assert "entropy.hip" in units
    ks = kr.analyse(os.path.join(_build.CSRC, "entropy.hip"), units["entropy.hip"])
    names = [k["demangled"] for k in ks]
    assert sum("entropy_decode_kernel" in n for n in names) == 2 and sum("entropy_zero_kernel" in n for n in names) == 2
    for k in ks:
        assert k.get("scratch", 1) == 0, k["demangled"]


def test_an_ordered_book_with_32_bit_codes_gives_an_image_the_device_accepts(front):
    """An ordered book's max_bits is one more than its longest code (33 with 32-bit codes; the count of Codebook.cs:60-66); the
    device peeks 32 bits at most (vpz_entropy_setup_create refuses more), and decode_scalar compares 32 bits only: the image
    says min(max_bits, 32) for a stream that vpzh_gpu_decode_supported accepts."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_streams as es
    seen = []
    for longest in (31, 32):
        f = front.OggVorbisFile(es.long_codes(longest, packets=2)[0])
        assert f.gpu_decode_supported
        img = f.entropy_setup()
        book_count = struct.unpack_from("<i", img, 32)[0]
        books = struct.unpack_from("<I", img, 52)[0]
        assert book_count == 3
        bits = [struct.unpack_from("<i", img, books + 48 * k + 8)[0] for k in range(book_count)]
        assert all(0 < b <= 32 for b in bits), bits
        seen.append(bits[0])
        f.close()
    assert seen == [32, 32]  # (the ordered floor book: 31 + 1, and 32 + 1 held to 32)
