"""What a context keeps from one call to the next (csrc/device_table.hpp, Scratch in csrc/vpz_internal.hpp): the device tables built on
first use, each under its key; the scratch memory that grows and is reused; the launch plan vpz_pcm_fbank and vpz_pcm_mfcc share.

No truth of its own: every expectation but the last test's is BIT EQUALITY with the same call on a freshly created context, which is
destroyed afterwards -- the truth tests of each entry point hold the values themselves.  A key that lost a field would hand call A the
table call B built, and the bits would be B's; a scratch buffer that grew wrongly would be read or written behind its end.  The shapes
are the smallest that reach the state: 2 rows of win + 3 * hop samples (4 frames) at the smallest n_fft, white noise of a fixed seed."""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fbank_truth as ft  # noqa: E402
import mfcc_truth as mt  # noqa: E402
from f32_model import fma32  # noqa: E402

pytestmark = pytest.mark.gpu

# the smallest n_fft the headers allow, with 4 bands
FBANK = dict(sample_rate=8000, win=32, hop=16, n_fft=32, n_mels=4, low_freq=100.0, high_freq=0.0)
MFCC = dict(FBANK, n_ceps=3)
LOGMEL = dict(sample_rate=8000, n_fft=32, hop=16, n_mels=4, f_min=0.0, f_max=4000.0, mel_scale="slaney", mel_norm="slaney")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import capi
    return capi


@pytest.fixture(scope="module")
def noise(capi):
    """white noise of a fixed seed: the float32 host array and its device copy"""
    import torch
    host = (0.3 * np.random.default_rng(20261020).standard_normal(1 << 18)).astype(np.float32)
    return host, torch.from_numpy(host).to("cuda:0")


@contextlib.contextmanager
def fresh():
    from vorbispizza_amd import Context
    c = Context(0)
    try:
        yield c
    finally:
        c.close()


def two_rows(F):
    """a whole row at an odd offset and a shorter one behind it, into rows 1 and 0"""
    return [(3, F, 1), (F + 8, F - 5, 0)]


def run_fbank(capi, c, d, src, rows=None, F=None, dst_rows=2):
    import torch
    spec = capi.FbankSpec.make(**ft.spec_of(**d))
    F = spec.win + 3 * spec.hop if F is None else F
    dst = torch.full((dst_rows, spec.n_frames(F), spec.n_mels), float("nan"), dtype=torch.float32, device="cuda:0")
    assert capi.pcm_fbank(c, src, two_rows(F) if rows is None else rows, dst, spec, F) == capi.OK, c.last_error()
    c.synchronize()
    return dst.cpu().numpy()


def run_mfcc(capi, c, d, src, rows=None, F=None, dst_rows=2):
    import torch
    spec = capi.MfccSpec.make(**mt.spec_of(**d))
    F = spec.fbank.win + 3 * spec.fbank.hop if F is None else F
    dst = torch.full((dst_rows, spec.n_frames(F), spec.n_ceps), float("nan"), dtype=torch.float32, device="cuda:0")
    assert capi.pcm_mfcc(c, src, two_rows(F) if rows is None else rows, dst, spec, F) == capi.OK, c.last_error()
    c.synchronize()
    return dst.cpu().numpy()


def run_logmel(capi, c, d, src):
    import torch
    spec = capi.LogMelSpec.make(**d)
    F = spec.n_fft + 3 * spec.hop
    dst = torch.full((2, spec.n_mels, spec.n_frames(F)), float("nan"), dtype=torch.float32, device="cuda:0")
    assert capi.pcm_logmel(c, src, two_rows(F), dst, spec, F) == capi.OK, c.last_error()
    c.synchronize()
    return dst.cpu().numpy()


def run_resample(capi, c, ratio, src):
    import torch
    up, down = ratio
    L, F = 300, 300 * up // down + 1
    dst = torch.full((2, 1, F), float("nan"), dtype=torch.float32, device="cuda:0")
    assert capi.pcm_resample(c, src.view(-1, 1), [(3, L, 1), (400, L - 7, 0)], dst, capi.OUT_PLANAR, up, down) == capi.OK, c.last_error()
    c.synchronize()
    return dst.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def alternate(run, A, B):
    """A, B, A on one context: each the bits of the same call on a context of its own -- and A's are not B's there"""
    with fresh() as c:
        a = run(c, A)
    with fresh() as c:
        b = run(c, B)
    assert not same(a, b), "the two specs agree on a fresh context: the pair shows nothing"
    assert not np.isnan(a).all() and not np.isnan(b).all()
    with fresh() as c:
        got = [run(c, A), run(c, B), run(c, A)]
    assert same(got[0], a), "the first call"
    assert same(got[1], b), "the second call has the first one's table"
    assert same(got[2], a), "the third call has the second one's table"


def tables_differ(x, y):
    """what two table calls returned (an array or a tuple of arrays) is not the same"""
    x, y = (x, y) if isinstance(x, tuple) else ((x,), (y,))
    return any(not same(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


FBANK_TABLE_FIELDS = {"win": dict(win=30), "n_fft": dict(n_fft=34), "window": dict(window="hamming"), "preemphasis": dict(preemphasis=0.5),
                      "scale": dict(scale=1.0)}
FBANK_BANK_FIELDS = {"sample_rate": dict(sample_rate=16000), "n_fft": dict(n_fft=34), "n_mels": dict(n_mels=5), "low_freq": dict(low_freq=600.0),
                     "high_freq": dict(high_freq=3000.0)}
CEPSTRAL_FIELDS = {"n_mels": dict(n_mels=5), "n_ceps": dict(n_ceps=4), "lifter": dict(lifter=0.0), "htk_compat": dict(htk_compat=True),
                   "use_energy": dict(use_energy=False)}
LOGMEL_BANK_FIELDS = {"sample_rate": dict(sample_rate=16000, f_max=4000.0), "n_fft": dict(n_fft=34), "n_mels": dict(n_mels=5), "f_min": dict(f_min=500.0),
                      "f_max": dict(f_max=3000.0), "mel_scale": dict(mel_scale="htk"), "mel_norm": dict(mel_norm=None)}


@pytest.mark.parametrize("field", sorted(FBANK_TABLE_FIELDS))
def test_the_fbank_table_key_keeps_every_field(capi, noise, field):
    A, B = FBANK, dict(FBANK, **FBANK_TABLE_FIELDS[field])
    ta, tb = (capi.fbank_table(capi.FbankSpec.make(**ft.spec_of(**d))) for d in (A, B))
    assert tables_differ(ta, tb)  # (vpz_fbank_table decides it: the pair is a pair of two tables)
    alternate(lambda c, d: run_fbank(capi, c, d, noise[1]), A, B)


@pytest.mark.parametrize("field", sorted(FBANK_BANK_FIELDS))
def test_the_fbank_bank_key_keeps_every_field(capi, noise, field):
    A, B = FBANK, dict(FBANK, **FBANK_BANK_FIELDS[field])
    ba, bb = (capi.fbank_filterbank(capi.FbankSpec.make(**ft.spec_of(**d))) for d in (A, B))
    assert tables_differ(ba, bb)  # (vpz_fbank_filterbank decides it)
    alternate(lambda c, d: run_fbank(capi, c, d, noise[1]), A, B)


@pytest.mark.parametrize("field", sorted(CEPSTRAL_FIELDS))
def test_the_cepstral_key_keeps_every_field(capi, noise, field):
    A, B = MFCC, dict(MFCC, **CEPSTRAL_FIELDS[field])
    if field != "use_energy":  # (the energy takes c[0]'s place in the kernel: vpz_mfcc_table does not show it)
        ca, cb = (capi.mfcc_table(capi.MfccSpec.make(**mt.spec_of(**d))) for d in (A, B))
        assert tables_differ(ca, cb)
    alternate(lambda c, d: run_mfcc(capi, c, d, noise[1]), A, B)


@pytest.mark.parametrize("field", sorted(LOGMEL_BANK_FIELDS))
def test_the_logmel_keys_keep_every_field(capi, noise, field):
    """the seven fields of the bank's key; n_fft is the DFT table's key too"""
    A, B = LOGMEL, dict(LOGMEL, **LOGMEL_BANK_FIELDS[field])
    ba, bb = (capi.mel_filterbank(capi.LogMelSpec.make(**d)) for d in (A, B))
    assert tables_differ(ba, bb)  # (vpz_mel_filterbank decides it)
    if field == "n_fft":
        assert capi.logmel_dft_table(A["n_fft"]).shape != capi.logmel_dft_table(B["n_fft"]).shape
    alternate(lambda c, d: run_logmel(capi, c, d, noise[1]), A, B)


def test_the_resample_key_keeps_both_fields_in_their_order(capi, noise):
    """(2, 3), (3, 2) and (2, 1), twice over on one context"""
    ratios = [(2, 3), (3, 2), (2, 1)]
    alone = []
    for r in ratios:
        with fresh() as c:
            alone.append(run_resample(capi, c, r, noise[1]))
    filters = [capi.resample_filter(*r) for r in ratios]
    for i in range(3):
        for j in range(i + 1, 3):
            assert tables_differ(filters[i][1:], filters[j][1:]) and not same(alone[i], alone[j])
    with fresh() as c:
        for k in range(6):
            assert same(run_resample(capi, c, ratios[k % 3], noise[1]), alone[k % 3]), (k, ratios[k % 3])


def loudness_calls(fs, host):
    """(channels, rows, source) of the three calls: 1 mono row of one step, 3 stereo rows of 40 steps, the first again"""
    S = (fs + 5) // 10
    small = (1, [(5, S, 0)], host[: S + 5])
    big = (2, [(2, 40 * S, 2), (80 * S + 10, 40 * S, 0), (160 * S + 18, 40 * S, 1)], host[: 240 * S + 32])
    return [small, big, small]


def run_loudness(capi, c, fs, call):
    import torch
    channels, rows, x = call
    sums, peak = capi.pcm_loudness(c, torch.from_numpy(x).to("cuda:0"), channels, fs, rows)
    c.synchronize()
    return np.concatenate([sums.cpu().numpy().view(np.uint8).reshape(-1), peak.cpu().numpy().view(np.uint8).reshape(-1)])


def run_true_peak(capi, c, fs, call):
    import torch
    channels, rows, x = call
    tp, sp = capi.pcm_true_peak(c, torch.from_numpy(x).to("cuda:0"), channels, fs, rows)
    c.synchronize()
    return np.concatenate([tp.cpu().numpy().view(np.uint8), sp.cpu().numpy().view(np.uint8)])


@pytest.mark.parametrize("entry", ["loudness", "true_peak"])
def test_scratch_grows_and_is_reused(capi, noise, entry):
    run = run_loudness if entry == "loudness" else run_true_peak
    calls = loudness_calls(8000, noise[0])
    alone = []
    for call in calls[:2]:
        with fresh() as c:
            alone.append(run(capi, c, 8000, call))
    assert alone[0].any() and alone[1].any()
    with fresh() as c:
        got = [run(capi, c, 8000, call) for call in calls]
    assert same(got[0], alone[0]) and same(got[1], alone[1]) and same(got[2], alone[0])


def test_the_loudness_rate_is_its_constants_key(capi, noise):
    """two rates inside the header's limits, A, B, A: 8000 and 8010 Hz (steps of 800 and 801 samples)"""
    def run(c, fs):
        S = (fs + 5) // 10
        return run_loudness(capi, c, fs, (2, [(2, 4 * S + 7, 0), (8 * S + 20, 3 * S, 1)], noise[0][: 14 * S + 32]))
    assert tables_differ(capi.loudness_filter(8000), capi.loudness_filter(8010))
    alternate(run, 8000, 8010)


def test_staging_memory_grows_and_is_reused(capi):
    """host-memory calls: vpz_decoder_synth over one short packet pair, a larger batch, the pair again -- one decoder, reset in between
    -- and vpz_imdct_batch over 1, 9 and 1 blocks"""
    import synthetic_streams as ss
    from vorbispizza_amd import Decoder
    from vorbispizza_amd.front import OggVorbisFile
    stream, rng = ss.mono_floor1_res1()
    batches = []
    for n in (2, 12):
        f = OggVorbisFile(stream.build(rng, n)[0])
        batches.append((f, f.decode_packets()))
    f0 = batches[0][0]
    order = [0, 1, 0]
    spectra = [(np.random.default_rng(5 + n).standard_normal((n, 128)) * 2.0 ** -8).astype(np.float32) for n in (1, 9)]

    def synth(dec, k):
        pk, res, posts, counts = batches[k][1]
        dec.reset()
        dec.set_position(0)  # (a new decoder's state: the stream starts over)
        return dec.synth(pk, res, posts, counts)[0]

    def decoder(c):
        return Decoder(c, f0.channels, f0.block_size0, f0.block_size1, floors=f0.floors, mappings=f0.mappings)

    alone, blocks = [], []
    for k in (0, 1):
        with fresh() as c:
            dec = decoder(c)
            alone.append(synth(dec, k))
            dec.close()
            blocks.append(c.imdct_batch(spectra[k], 256))
    assert alone[0].size and alone[1].shape[1] > alone[0].shape[1] and np.abs(alone[1]).max() > 0
    with fresh() as c:
        dec = decoder(c)
        for k in order:
            assert same(synth(dec, k), alone[k]), k
            assert same(c.imdct_batch(spectra[k], 256), blocks[k]), k
        dec.close()


def test_fma32_is_the_exact_one():
    from f32_model import fma32_rational as one
    rng = np.random.default_rng(11)
    a, b = rng.standard_normal(300).astype(np.float32), rng.standard_normal(300).astype(np.float32)
    c = (rng.standard_normal(300) * 2.0 ** rng.integers(-30, 30, 300)).astype(np.float32)
    a[:3], b[:3], c[:3] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), [np.float32(2.0 ** -24), np.float32(-1.0), np.float32(2.0 ** 24)]
    got = fma32(a, b, c)
    for i in range(300):
        assert got[i].view(np.uint32) == one(a[i], b[i], c[i]).view(np.uint32), i


def test_fbank_and_mfcc_share_one_plan(capi, noise):
    """T = 1, 16, 17, 32, 33 and 65 frames at 2 rows -- 16-, 32-frame tiles on either side of their thresholds, 65 the 32 tile of a
    launch too small for 64 -- and 65 frames at 2 * num_cu rows of `win` samples each, which takes the 64 tile: at each, a coefficient
    of vpz_pcm_mfcc is the fused chain of vpz_mfcc_table's row over vpz_pcm_fbank's output, b ascending, bit for bit"""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    k = ft.kernel_constants(ROOT)
    d = dict(MFCC, use_energy=False, pad_value=-2.5)
    win, hop, n_fft, n_mels, n_ceps = d["win"], d["hop"], d["n_fft"], d["n_mels"], d["n_ceps"]
    table = capi.mfcc_table(capi.MfccSpec.make(**mt.spec_of(**d)))
    fb = {key: d[key] for key in ft.DEFAULTS if key in d}
    shapes = [(T, 2, tile) for T, tile in ((1, 16), (16, 16), (17, 32), (32, 32), (33, 32), (65, 32))] + [(65, 2 * num_cu, 64)]
    with fresh() as c:
        for T, n_rows, tile in shapes:
            assert ft.tile_plan(win, hop, n_fft, T, n_rows, num_cu, k)[0] == tile == mt.tile_plan(win, hop, n_fft, n_mels, T, n_rows, num_cu, k)[0]
            F = win + (T - 1) * hop + 3
            rows = [(3, F, 1), (F + 8, F - 5, 0)] if n_rows == 2 else [(7 * i, win, i) for i in range(n_rows)]
            E = run_fbank(capi, c, fb, noise[1], rows, F, n_rows)
            got = run_mfcc(capi, c, d, noise[1], rows, F, n_rows)
            assert E.shape == (n_rows, T, n_mels) and got.shape == (n_rows, T, n_ceps)
            real = np.zeros((n_rows, T), dtype=bool)
            for _, L, r in rows:
                real[r, : ft.n_frames(L, win, hop)] = True
            assert (E[~real] == -2.5).all() and (got[~real] == -2.5).all() and np.isfinite(E[real]).all()
            v = np.zeros((n_rows, T, n_ceps), dtype=np.float32)
            for b in range(n_mels):
                v = fma32(np.broadcast_to(table[:, b], v.shape), np.broadcast_to(E[:, :, b, None], v.shape), v)
            assert v[real].tobytes() == got[real].tobytes(), (T, n_rows)
