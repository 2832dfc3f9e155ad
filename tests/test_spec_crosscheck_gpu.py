"""The HIP path against the specification-derived float64 synthesis (tests/spec_synthesis.py) -- NO oracle code in
the loop.  The CPU suite pins the oracle to the specification (test_spec_crosscheck_cpu.py) and the other GPU tests
hold the kernels to the oracle; this file closes the triangle directly, so that a misreading shared by the restatement
and the kernels (e.g. of StreamDecoder.cs:764-791) cannot hide behind their agreement.  The reference's own acceptance
test is the model: decode a fixture, compare as 16-bit samples within a small band (NVorbis.Tests/AssetTest.cs:131-161,
band 2; here 1) -- plus BASELINE's float criterion, 1e-5 x max(1, peak)."""
import os

import numpy as np
import pytest

import spec_synthesis as spec
from synth_support import spec_packets, to_s16_wide as to_s16
from gpu_context import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", ["1test.ogg", "2test.ogg", "3test.ogg", "issue6test.ogg"])
def test_gpu_pcm_matches_the_specification_derived_synthesis(ctx, name):
    from vorbispizza_amd import Decoder, capi
    from vorbispizza_amd.front import OggVorbisFile
    f = OggVorbisFile(os.path.join(GOLDEN, name))
    pk, res, posts, counts = f.decode_packets()
    packets = spec_packets(f, pk, res, posts, counts)
    if name == "issue6test.ogg":
        packets = packets[:-1]  # the trailing empty packet: skipped by the window check (see the CPU version of this test)
    want = spec.decode(f.channels, f.block_size0, f.block_size1, f.floors, f.mappings, packets,
                       total_samples=int(f.last_granule))
    cap = int(f.audio_packets) * (f.block_size1 // 2) + f.block_size1
    C_ = f.channels

    # float32, planar, un-clipped: BASELINE's criterion
    dec = Decoder(ctx, C_, f.block_size0, f.block_size1, floors=f.floors, mappings=f.mappings, clip_samples=False)
    out = np.zeros(C_ * cap, dtype=np.float32)
    w = dec.synth_raw(pk, res, posts, counts, out, None, cap, capi.OUT_PLANAR, cap, capi.MEM_HOST, on_mismatch="ignore")
    assert dec.last_mismatches() == (1 if name == "issue6test.ogg" else 0)
    status = dec.last_packet_status(len(pk))
    assert [int(i) for i in np.nonzero(status)[0]] == ([len(pk) - 1] if name == "issue6test.ogg" else [])
    n = int(w[0])
    got = out.reshape(C_, cap)[:, :n]
    assert abs(n - want.shape[1]) <= (63 if name == "issue6test.ogg" else 0) and n >= want.shape[1]
    m = min(n, want.shape[1])
    peak = float(np.abs(want).max())
    assert peak > 0.05
    d = float(np.abs(got[:, :m].astype(np.float64) - want[:, :m]).max())
    assert d <= 1e-5 * max(1.0, peak), (name, d, peak)
    dec.close()

    # 16-bit samples straight from the store epilogue (VPZ_OUT_INTERLEAVED_S16, clipping on as VorbisReader sets it):
    # the reference's own acceptance criterion
    dec = Decoder(ctx, C_, f.block_size0, f.block_size1, floors=f.floors, mappings=f.mappings, clip_samples=True)
    out16 = np.zeros(C_ * cap, dtype=np.int16)
    w = dec.synth_raw(pk, res, posts, counts, out16, None, cap, capi.OUT_INTERLEAVED_S16, 0, capi.MEM_HOST,
                      on_mismatch="ignore")
    assert int(w[0]) == n
    got16 = out16[: n * C_].reshape(n, C_).T.astype(np.int64)
    want16 = to_s16(np.clip(want[:, :m], -0.99999994, 0.99999994))
    assert np.abs(got16[:, :m] - want16).max() <= 1, name
    dec.close()


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("name", ["stereo_coupled_res2", "three_channels_chained", "four_channels_quad", "five_channels", "six_channels_51",
                                  "ten_channels"])
def test_gpu_matches_the_specification_on_synthetic_multichannel_streams(ctx, name, layout):
    """... and the same for what the fixtures do not hold (they are mono and stereo): 3 / 4 / 6 channels from the spec-based
    writer -- group mode with real Residue2 vectors, the libvorbis 5.1 coupling (0,2), (3,4), chained steps, silent channels
    inside coupled pairs, batches of short blocks -- straight against the specification-derived synthesis, no oracle code."""
    import synthetic_streams as ss
    from vorbispizza_amd import Decoder, capi
    from vorbispizza_amd.front import OggVorbisFile
    stream, rng = ss.ALL[name]()
    ogg, _ = stream.build(rng, 40)
    f = OggVorbisFile(ogg)
    pk, res, posts, counts = f.decode_packets()
    want = spec.decode(f.channels, f.block_size0, f.block_size1, f.floors, f.mappings, spec_packets(f, pk, res, posts, counts),
                       total_samples=int(f.last_granule))
    C_ = f.channels
    cap = int(f.last_granule) + f.block_size1
    dec = Decoder(ctx, C_, f.block_size0, f.block_size1, floors=f.floors, mappings=f.mappings, clip_samples=False)
    out = np.zeros(C_ * cap, dtype=np.float32)
    if layout == "planar":
        w = dec.synth_raw(pk, res, posts, counts, out, None, cap, capi.OUT_PLANAR, cap, capi.MEM_HOST)
        got = out.reshape(C_, cap)[:, : int(w[0])]
    else:
        w = dec.synth_raw(pk, res, posts, counts, out, None, cap, capi.OUT_INTERLEAVED, 0, capi.MEM_HOST)
        got = out[: int(w[0]) * C_].reshape(int(w[0]), C_).T
    assert int(w[0]) == want.shape[1] == f.last_granule
    peak = float(np.abs(want).max())
    d = float(np.abs(got.astype(np.float64) - want).max())
    assert peak > 0.05 and d <= 1e-5 * max(1.0, peak), (name, d, peak)
    dec.close()
    if layout == "interleaved":
        # ... and as the 16-bit samples of the store epilogue, clipping on (the reference's own acceptance criterion)
        dec = Decoder(ctx, C_, f.block_size0, f.block_size1, floors=f.floors, mappings=f.mappings, clip_samples=True)
        out16 = np.zeros(C_ * cap, dtype=np.int16)
        w = dec.synth_raw(pk, res, posts, counts, out16, None, cap, capi.OUT_INTERLEAVED_S16, 0, capi.MEM_HOST)
        n = int(w[0])
        assert n == want.shape[1]
        got16 = out16[: n * C_].reshape(n, C_).T.astype(np.int64)
        assert np.abs(got16 - to_s16(np.clip(want, -0.99999994, 0.99999994))).max() <= 1, name
        dec.close()
