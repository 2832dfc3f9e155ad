"""vpz_entropy_decode (vorbispizza_entropy.h) against the CPU front end: the device's posts, post counts and residue are
byte for byte what vpzh_decode_range_ex / vpzh_decode_range_i16 write -- on the fixtures, the writer's floor-1 streams,
the crafted setups and damaged audio -- and decode_to_pcm's PCM is the PCM of the CPU-decoded residue through the same
vpz_decoder_synth route."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from synth_support import FIXTURES, GOLDEN, check_stream, device_decode, streams  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def fixture(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def test_every_eligible_stream_decodes_as_on_the_cpu(ctx):
    from vorbispizza_amd import capi
    done = 0
    for name, raw in streams():
        done += check_stream(ctx, name, raw, (capi.MEM_HOST, capi.MEM_DEVICE))
    assert done >= 15


def test_damaged_audio_decodes_as_on_the_cpu(ctx):
    """truncated packets, Huffman misses, early residue stops: 60 seeds over the two long fixtures and a writer stream"""
    from synth_support import damage_audio

    from vorbispizza_amd import capi
    import synthetic_streams as ss
    st, rng = ss.stereo_coupled_res2()
    ogg, _ = st.build(rng, 40)
    sources = [fixture("3test.ogg"), fixture("issue6test.ogg"), bytes(ogg)]
    for seed in range(60):
        raw = damage_audio(sources[seed % 3], seed, 6 + seed % 13)
        assert check_stream(ctx, "damaged %d" % seed, raw, (capi.MEM_HOST,) if seed % 4 else (capi.MEM_DEVICE,))


def test_a_batch_of_several_streams_of_one_setup(ctx):
    """one call over three streams of 3test's setup (the file and two damaged copies), payloads and residues back to back"""
    from synth_support import damage_audio

    from vorbispizza_amd import capi
    from vorbispizza_amd.entropy import EntropySetup
    from vorbispizza_amd.front import OggVorbisFile
    raws = [fixture("3test.ogg"), damage_audio(fixture("3test.ogg"), 7, 10), damage_audio(fixture("3test.ogg"), 8, 20)]
    files = [OggVorbisFile(r) for r in raws]
    images = {f.entropy_setup() for f in files}
    assert len(images) == 1
    setup = EntropySetup(ctx, images.pop())
    for i16 in (False, True):
        pk_all, sp_all, pay_all, refs = [], [], [], []
        res_base, pay_base = 0, 0
        for s, f in enumerate(files):
            pk, sp, pay, used = f.plan_packets(stream_id=s, residue_base=res_base)
            sp = sp.copy()
            sp[:, 0] += pay_base
            pk_all.append(pk)
            sp_all.append(sp)
            pay_all.append(pay)
            _, r, po, co = f.decode_packets(stream_id=s, int16=i16)
            refs.append((r, po, co))
            res_base += used
            pay_base += pay.size
        packets, spans, payload = np.concatenate(pk_all), np.concatenate(sp_all), np.concatenate(pay_all)
        for ms in (capi.MEM_HOST, capi.MEM_DEVICE):
            res, posts, counts = device_decode(ctx, setup, packets, spans, payload, res_base, 2, i16, ms)
            assert np.array_equal(counts, np.concatenate([r[2] for r in refs]))
            assert posts.tobytes() == np.concatenate([r[1] for r in refs]).tobytes()
            flat = np.concatenate([r[0] for r in refs])
            for k in range(len(packets)):
                if packets["flags"][k] & capi.PKT_NOT_DECODED:
                    continue
                o = int(packets["residue_offset"][k])
                n = 2 * ((2048 if packets["flags"][k] & capi.PKT_BLOCK_FLAG else 256) // 2)
                assert res[o:o + n].tobytes() == flat[o:o + n].tobytes(), (i16, ms, k)
    setup.close()


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_decode_to_pcm_equals_the_cpu_residue_through_the_same_route(ctx, layout):
    import torch

    from vorbispizza_amd import capi
    from vorbispizza_amd.entropy import decode_to_pcm
    from vorbispizza_amd.front import OggVorbisFile
    dev = torch.device("cuda", ctx.device)
    for name in FIXTURES:
        raw = fixture(name)
        got = decode_to_pcm(ctx, raw, out_layout=layout)
        f = OggVorbisFile(raw)
        packets, residue, posts, counts = f.decode_packets()
        dec = capi.Decoder(ctx, f.channels, f.block_size0, f.block_size1, f.floors, f.mappings)
        per = int(np.where(packets["flags"] & capi.PKT_BLOCK_FLAG, f.block_size1, f.block_size0).sum()) + 1
        s16 = layout in (capi.OUT_INTERLEAVED_S16, capi.OUT_PLANAR_S16)
        pcm = torch.zeros(f.channels * per, dtype=torch.int16 if s16 else torch.float32, device=dev)
        w = int(dec.synth_raw(packets, torch.from_numpy(residue).to(dev), torch.from_numpy(posts).to(dev),
                              torch.from_numpy(counts).to(dev), pcm, None, per, layout, per, capi.MEM_DEVICE,
                              on_mismatch="ignore")[0])
        ctx.synchronize()
        ref = pcm.view(f.channels, per)[:, :w] if layout in (capi.OUT_PLANAR, capi.OUT_PLANAR_S16) else pcm[: w * f.channels].view(w, f.channels)
        assert got.shape == ref.shape and w > 0, name
        assert got.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes(), (name, layout)
        dec.close()
        f.close()


def test_argument_errors_write_nothing(ctx):
    import ctypes as C

    from vorbispizza_amd import capi, entropy
    from vorbispizza_amd.entropy import EntropySetup
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(fixture("1test.ogg"))
    image = bytearray(f.entropy_setup())
    # a bad image version, a truncated image, an offset out of range
    for bad in (image[:4] + b"\x02" + image[5:], image[:-4], image[:60] + b"\xff\xff\xff\x7f" + image[64:]):
        h = C.c_void_p()
        buf = np.frombuffer(bytes(bad), dtype=np.uint8)
        assert entropy.lib().vpz_entropy_setup_create(ctx._h, buf.ctypes.data, buf.size, C.byref(h)) == capi.E_INVALID_ARG
        assert not h.value
    assert entropy.lib().vpz_entropy_version() == 1
    setup = EntropySetup(ctx, bytes(image))
    packets, spans, payload, n_values = f.plan_packets()
    n, ch = len(packets), f.channels

    def call(pk=packets, sp=spans, values=n_values, records=n * ch, fmt=None):
        residue = np.full(max(1, n_values), 7.0, dtype=np.float32)
        posts = np.full((n * ch, 64), 3, dtype=np.int16)
        counts = np.full(n * ch, 9, dtype=np.uint8)
        rc = setup.decode_raw(pk, sp, payload, residue, posts, counts, capi.MEM_HOST, residue_format=fmt, residue_values=values,
                              n_records=records)
        untouched = (residue == 7.0).all() and (posts == 3).all() and (counts == 9).all()
        return rc, untouched

    assert call()[0] == capi.OK
    bad_span = spans.copy()
    bad_span[3, 1] = payload.size  # beyond the payload
    assert call(sp=bad_span) == (capi.E_INVALID_ARG, True)
    bad_span = spans.copy()
    bad_span[-1, 0] = payload.size - bad_span[-1, 1] - 7  # 7 bytes of padding left, 8 needed
    assert call(sp=bad_span) == (capi.E_INVALID_ARG, True)
    assert call(values=n_values - 1) == (capi.E_INVALID_ARG, True)  # the last decoded packet's residue does not fit
    assert call(records=n * ch - 1) == (capi.E_INVALID_ARG, True)
    bad_pk = packets.copy()
    bad_pk["mapping"][0] = 200
    assert call(pk=bad_pk) == (capi.E_INVALID_ARG, True)
    assert call(fmt=5) == (capi.E_INVALID_ARG, True)
    setup.close()
    f.close()
