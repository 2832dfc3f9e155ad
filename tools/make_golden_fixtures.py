#!/usr/bin/env python3
"""Writes the small golden vectors of SURVEY.md section 8c into tests/golden/ (committed; data only).

Source of the numbers: the CPU oracle (oracle/vorbis_synth_oracle.c -- the restatement of the reference's
arithmetic) and the C++ front end (bit-exact entropy stage) run HERE on seeded inputs and on the reference's own
.ogg fixtures.  The reference itself cannot run in this pipeline (C#, no .NET) and holds no vectors of its own, so
these files freeze the oracle as it was when tests/test_spec_crosscheck_cpu.py tied it to the specification-derived
float64 synthesis; tests/test_golden_vectors_cpu.py fails if a later edit of the oracle moves a single bit, and
tests/test_golden_vectors_gpu.py holds the HIP path to them without needing any oracle code on the GPU box.

    python tools/make_golden_fixtures.py        # rewrites tests/golden/*.npz
    python tools/make_golden_fixtures.py --front-records COMMIT
                                                # writes tests/golden/front_records.json alone: what the C++ front end, built
                                                # from COMMIT, writes for the four .ogg fixtures (tests/test_front_cpu.py)
    python tools/make_golden_fixtures.py --reference NVORBIS_DIR
                                                # writes tests/golden/reference_constants.npz alone: the constant tables
                                                # of the reference's source text (NVORBIS_DIR: its NVorbis/ folder), which
                                                # tests/test_oracle_tables.py holds the oracle to
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("1test.ogg", "2test.ogg", "3test.ogg", "issue6test.ogg")


def main():
    import helpers
    import oracle
    from vorbispizza_amd.front import OggVorbisFile

    # ---- IMDCT, N = 256 and 2048: seeded N(0, 1) spectra -> Mdct.Reverse outputs (Mdct.cs:15-19)
    vec = {}
    for n, rows in ((256, 8), (2048, 4)):
        x = np.random.default_rng(n).standard_normal((rows, n // 2)).astype(np.float32)
        vec["spectra_%d" % n] = x
        vec["pcm_%d" % n] = oracle.mdct_reverse(x, n)
    np.savez_compressed(os.path.join(OUT, "imdct_vectors.npz"), **vec)

    # ---- window switching + overlap-add: every PacketInfo geometry of Mode.cs:30-66 at least once
    L, P, N = helpers.PKT_BLOCK_FLAG, helpers.PKT_PREV_FLAG, helpers.PKT_NEXT_FLAG
    #                 long pl/nl  long pl/ns  short short long ps/ns short long ps/nl  long pl/nl
    flags = np.array([L | P | N, L | P, 0, 0, L, 0, L | N, L | P | N], dtype=np.uint8)
    spectra = helpers.gaussian_spectra((len(flags), 2, 1024), seed=11)
    pcm = oracle.synth_stream_planar(2, 256, 2048, flags, spectra)
    infos = np.array([[getattr(oracle.packet_info(256, 2048, f & 1, bool(f & 2), bool(f & 4)), k)
                       for k in ("Length", "LeftUseSize1", "LeftStart", "LeftEnd", "RightStart", "RightEnd")]
                      for f in flags], dtype=np.int32)
    np.savez_compressed(os.path.join(OUT, "window_ola_sequence.npz"), flags=flags, spectra=spectra, pcm=pcm,
                        packet_info=infos)

    # ---- inverse coupling: the four sign quadrants, zeros of either sign, equal magnitudes (Mapping.cs:198-269)
    m = np.array([3.0, 3.0, -3.0, -3.0, 0.0, -0.0, 0.0, 2.0, -2.0, 5.0, -5.0, 1.5, -1.5, 0.0, -0.0, 7.0], dtype=np.float32)
    a = np.array([1.0, -1.0, 1.0, -1.0, 2.0, 2.0, -2.0, 0.0, -0.0, 5.0, -5.0, -1.5, 1.5, 0.0, -0.0, -0.0], dtype=np.float32)
    mv, av = oracle.apply_coupling(m, a, vector_form=True)
    ms, as_ = oracle.apply_coupling(m, a, vector_form=False)
    np.savez_compressed(os.path.join(OUT, "coupling_quadrants.npz"), magnitude=m, angle=a, out_magnitude_vector=mv,
                        out_angle_vector=av, out_magnitude_scalar=ms, out_angle_scalar=as_)

    # ---- Floor1: the 29-post long floor of 3test.ogg, posts of its first long packets -> finalY, flags, curve
    f = OggVorbisFile(os.path.join(OUT, "3test.ogg"))
    pk, res, posts, counts = f.decode_packets()
    long_floor = next(i for i, fl in enumerate(f.floors) if len(fl[0]) == 29)
    xlist, mult = f.floors[long_floor]
    of = oracle.floor1_init(xlist, mult)
    rows = [i * 2 + c for i in range(len(pk)) if pk["flags"][i] & 1 for c in range(2) if counts[i * 2 + c]][:16]
    raw = posts[rows].astype(np.int16)
    fy, fl, cur = zip(*[oracle.floor1_indices(of, raw[r].astype(np.int32), 29, 1024) for r in range(len(rows))])
    np.savez_compressed(os.path.join(OUT, "floor1_3test_long.npz"), x_list=np.array(xlist, np.int32),
                        multiplier=np.int32(mult), raw_posts=raw, final_y=np.array(fy, np.int32)[:, :29],
                        step_flags=np.array(fl, np.uint8)[:, :29], table_index=np.array(cur, np.int32),
                        inverse_db_table=oracle.inverse_db_table())

    # ---- the first 4096 PCM samples per channel of every reference fixture, and the decoded lengths
    pcm_head = {}
    for name in FIXTURES:
        f = OggVorbisFile(os.path.join(OUT, name))
        pk, res, posts, counts = f.decode_packets()
        ref, pos, clipped = helpers.oracle_decode(oracle, f.channels, f.block_size0, f.block_size1,
                                                  helpers.packets_for_oracle(f, pk, res, posts, counts),
                                                  floors=f.floors, mappings=f.mappings, clip=True)
        key = name.replace(".ogg", "")
        pcm_head[key + "_pcm"] = ref[:, :4096]
        # a window around the loudest sample too (these files start, and some of them continue, with silence)
        mid = int(np.clip(int(np.abs(ref).max(axis=0).argmax()) - 1024, 0, ref.shape[1] - 2048))
        pcm_head[key + "_meta"] = np.array([f.channels, f.sample_rate, f.audio_packets, ref.shape[1], pos, int(clipped), mid],
                                           dtype=np.int64)
        pcm_head[key + "_mid"] = ref[:, mid: mid + 2048]
    np.savez_compressed(os.path.join(OUT, "fixture_pcm_heads.npz"), **pcm_head)
    for n in sorted(os.listdir(OUT)):
        if n.endswith(".npz"):
            print("%-28s %7d bytes" % (n, os.path.getsize(os.path.join(OUT, n))))


def front_records(front, path):
    """Digests of everything the front end writes for one fixture: a whole-file decode (stream_id 0, residue_base 0) as
    float and, where the residue is integral, as int16; and the packet records of the range first=5, count=40 (cut to the
    file's length: 1test.ogg has 25 packets) from vpzh_decode_range_ex and from vpzh_plan_range."""
    import ctypes as C

    def sha(a):
        return hashlib.sha256(a.tobytes()).hexdigest()

    f = front.OggVorbisFile(path)
    pk, res, posts, counts = f.decode_packets()
    out = {"packets": sha(pk), "posts": sha(posts), "post_counts": sha(counts), "residue_f32": sha(res),
           "residue_floats": int(f.info.residue_floats), "total_samples": int(f.total_samples),
           "decode_failures": list(f.decode_failures())}
    if f.residue_is_integral:
        pk16, res16, posts16, counts16 = f.decode_packets(int16=True)
        assert (sha(pk16), sha(posts16), sha(counts16)) == (out["packets"], out["posts"], out["post_counts"])
        out["residue_i16"] = sha(res16)
    first = 5
    count = min(40, f.audio_packets - first)
    pk_r = front.capi.make_packets(count)
    res_r = np.zeros(count * f.channels * f.block_size1 // 2, dtype=np.float32)
    posts_r = np.zeros((count * f.channels, 64), dtype=np.int16)
    counts_r = np.zeros(count * f.channels, dtype=np.uint8)
    assert front.lib().vpzh_decode_range_ex(f._h, first, count, 0, 0, pk_r.ctypes.data, res_r.ctypes.data, posts_r.ctypes.data,
                                            counts_r.ctypes.data, None, None, None, 0) == 0
    out["range_5_40_decode_packets"] = sha(pk_r)
    out["range_5_40_plan_packets"] = sha(f.plan_packets(first, count)[0])
    f.close()
    return out


def write_front_records(commit):
    from vorbispizza_amd import front
    rec = {"generated_at_commit": commit, "fixtures": {n: front_records(front, os.path.join(OUT, n)) for n in FIXTURES}}
    path = os.path.join(OUT, "front_records.json")
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%-28s %7d bytes" % (os.path.basename(path), os.path.getsize(path)))


def reference_constants(src_dir):
    """inverse_dB_table (Floor1.cs) and LowerClip / UpperClip (Utils.cs) as float32, read from the reference's source text."""
    src = open(os.path.join(src_dir, "Floor1.cs")).read()
    body = re.search(r"inverse_dB_table =\s*\{(.*?)\};", src, re.S).group(1)
    table = np.array([np.float32(t.strip().rstrip("f")) for t in body.replace("\n", " ").split(",") if t.strip()],
                     dtype=np.float32)
    assert table.shape == (256,)
    src = open(os.path.join(src_dir, "Utils.cs")).read()
    clip = np.array([np.float32(re.search(r"%s = (\S+)f;" % k, src).group(1)) for k in ("LowerClip", "UpperClip")],
                    dtype=np.float32)
    path = os.path.join(OUT, "reference_constants.npz")
    np.savez_compressed(path, inverse_db_table=table, clip=clip)
    print("%-28s %7d bytes" % (os.path.basename(path), os.path.getsize(path)))


if __name__ == "__main__":
    if "--reference" in sys.argv:
        reference_constants(sys.argv[sys.argv.index("--reference") + 1])
    elif "--front-records" in sys.argv:
        write_front_records(sys.argv[sys.argv.index("--front-records") + 1])
    else:
        main()
