"""What a context keeps from one call to the next (csrc/device_table.hpp, Scratch in csrc/vpz_internal.hpp): the device tables built on
first use, each under its key; the scratch memory that grows and is reused; the launch plan vpz_pcm_fbank and vpz_pcm_mfcc share.

No truth of its own: every expectation but test_fbank_and_mfcc_share_one_plan's is BIT EQUALITY with the same call on a freshly created context, which is
destroyed afterwards -- the truth tests of each entry point hold the values themselves.  A key that lost a field would hand call A the
table call B built, and the bits would be B's; a scratch buffer that grew wrongly would be read or written behind its end.  The shapes
are the smallest that reach the state: 2 rows of win + 3 * hop samples (4 frames) at the smallest n_fft, white noise of a fixed seed.

vpz_pcm_stft, vpz_pcm_cqt and vpz_pcm_melspec (the second half of the file) keep two maps of their own -- stft_tables, cqt_tables -- and
melspec writes into log-mel's two.  ONE RULE for every pair (A, B) of theirs: every table of B is no larger than the matching table of A
(no_larger, asserted on the host through the exports before the first launch), so that a key that lost a field shows as wrong bits and
never as a read behind an allocation."""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cqt_truth as ct  # noqa: E402
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


# ---- vpz_pcm_stft, vpz_pcm_cqt and vpz_pcm_melspec: stft_tables, cqt_tables, and melspec's entries in logmel_dft and logmel_banks
# (hop = n_fft / 4 and F = n_fft / 2 + 1 + 3 hop unless a spec or a call says otherwise; the CQT's N_0 = 539 and F = 64 * 9 + 5 = 581)
STFT = dict(n_fft=1024, win_length=1024, window="hann", output="complex", bins_first=True)
CQT = dict(ct.spec_of(n_bins=3, hop=64), output="complex", bins_first=True)
CQT_F = 64 * 9 + 5
MELSPEC = dict(sample_rate=8000, n_fft=2048, n_mels=4, f_min=0.0, f_max=4000.0, mel_scale="slaney", mel_norm="slaney")


def stage_of(capi, kind, d, F=None):
    """(the launch, its spec, F, a destination row's shape) of one spec of a stage"""
    d = dict(d)
    if kind == "cqt":
        spec, F = capi.CqtSpec.make(**d), CQT_F if F is None else F
        return capi.pcm_cqt, spec, F, spec.row_shape(F)
    d.setdefault("hop", d["n_fft"] // 4)
    spec = capi.StftSpec.make(**d) if kind == "stft" else capi.LogMelSpec.make(**d)
    F = spec.n_fft // 2 + 1 + 3 * spec.hop if F is None else F
    if kind == "stft":
        return capi.pcm_stft, spec, F, spec.row_shape(F)
    T = spec.n_frames(F)
    return capi.pcm_melspec, spec, F, (spec.n_mels, T) if spec.layout == capi.MEL_BANDS_FIRST else (T, spec.n_mels)


def destination(capi, kind, d, F=None, dst_rows=2):
    import torch
    return torch.full((dst_rows,) + stage_of(capi, kind, d, F)[3], float("nan"), dtype=torch.float32, device="cuda:0")


def enqueue(capi, c, kind, d, src, dst, rows=None, F=None):
    """one launch on the context's stream, not synchronised"""
    call, spec, F, _ = stage_of(capi, kind, d, F)
    assert call(c, src, two_rows(F) if rows is None else rows, dst, spec, F) == capi.OK, c.last_error()


def run_stage(capi, c, kind, d, src, rows=None, F=None, dst_rows=2):
    dst = destination(capi, kind, d, F, dst_rows)
    enqueue(capi, c, kind, d, src, dst, rows, F)
    c.synchronize()
    return dst.cpu().numpy()


def run_stft(capi, c, d, src, **kw):
    return run_stage(capi, c, "stft", d, src, **kw)


def run_cqt(capi, c, d, src, **kw):
    return run_stage(capi, c, "cqt", d, src, **kw)


def run_melspec(capi, c, d, src, **kw):
    return run_stage(capi, c, "melspec", d, src, **kw)


def stft_table_of(capi, d):
    return capi.stft_table(d["n_fft"], d["win_length"], d["window"])


def cqt_tables_of(capi, d):
    """(f_k, N_k, hr_0, hi_0, hr_1, ...) of a spec, and the floats a lane reads down one column of its device table: the sum of len_b, a
    column block's longest kernel made even (csrc/pcm_cqt.hip lays every block out 2 * kCqCols columns wide, whatever n_bins)"""
    spec = capi.CqtSpec.make(**d)
    f, n = capi.cqt_bins(spec)
    kernels = tuple(x for k in range(spec.n_bins) for x in capi.cqt_kernel(spec, k))
    return (f, n) + kernels, sum((int(n[b]) + 1) & ~1 for b in range(0, spec.n_bins, ct.kernel_constants()["kCqCols"]))


def melspec_bank_of(capi, d):
    """(first, count, weights), and (n_mels, total weights)"""
    bank = capi.melspec_filterbank(capi.LogMelSpec.make(**dict(d, hop=d["n_fft"] // 4)))
    return bank, (d["n_mels"], bank[2].size)


def in_turn(run, specs, order):
    """the specs in `order` on one context: each call the bits of the same call on a context of its own -- and no two specs agree there"""
    alone = []
    for d in specs:
        with fresh() as c:
            alone.append(run(c, d))
    assert all(np.isfinite(a).all() for a in alone)
    assert all(not same(alone[i], alone[j]) for i in range(len(specs)) for j in range(i)), "two specs agree on a fresh context"
    with fresh() as c:
        for at, k in enumerate(order):
            assert same(run(c, specs[k]), alone[k]), (at, k)


# B's change to A, one field of the key each.  n_fft: win_length <= n_fft, so both specs carry 512 and n_fft changes alone
STFT_KEY_PAIRS = {"n_fft": (dict(win_length=512), dict(n_fft=512, win_length=512)), "win_length": ({}, dict(win_length=800)), "window": ({}, dict(window="hamming"))}


@pytest.mark.parametrize("field", sorted(STFT_KEY_PAIRS))
def test_the_stft_table_key_keeps_every_field(capi, noise, field):
    A, B = (dict(STFT, **change) for change in STFT_KEY_PAIRS[field])
    assert [k for k in ("n_fft", "win_length", "window") if A[k] != B[k]] == [field]
    ta, tb = stft_table_of(capi, A), stft_table_of(capi, B)
    assert tables_differ(ta, tb)  # (vpz_stft_table decides it)
    assert sum(x.size for x in tb) <= sum(x.size for x in ta)
    alternate(lambda c, d: run_stft(capi, c, d, noise[1]), A, B)


# (A's change, B's change) to CQT: the one field in which the two differ, A the larger table but for n_bins.  n_bins 3 -> 4: a block's
# table is 32 columns wide whatever n_bins, and the columns of the first three bins are the same in both, so a key without n_bins shows
# only where the LATER call has the bin the earlier one lacks -- its column is zeros in the earlier call's table, inside the allocation
CQT_KEY_PAIRS = {"sample_rate": (dict(sample_rate=8010.0), dict(sample_rate=8000.0)), "f_min": (dict(f_min=250.0), dict(f_min=260.0)),
                 "filter_scale": (dict(filter_scale=1.0), dict(filter_scale=0.9)), "gamma": (dict(gamma=0.0), dict(gamma=20.0)),
                 "n_bins": (dict(n_bins=3), dict(n_bins=4)), "bins_per_octave": (dict(bins_per_octave=24), dict(bins_per_octave=12)),
                 "window": (dict(window="hann"), dict(window="hamming")), "scale": (dict(scale="sqrt_length"), dict(scale="none"))}
CQT_KEY = ("sample_rate", "f_min", "filter_scale", "gamma", "n_bins", "bins_per_octave", "window", "scale")


@pytest.mark.parametrize("field", sorted(CQT_KEY_PAIRS))
def test_the_cqt_table_key_keeps_every_field(capi, noise, field):
    A, B = (dict(CQT, **change) for change in CQT_KEY_PAIRS[field])
    assert [k for k in CQT_KEY if A[k] != B[k]] == [field] and all(A[k] == B[k] for k in A if k not in CQT_KEY)
    (ta, floats_a), (tb, floats_b) = cqt_tables_of(capi, A), cqt_tables_of(capi, B)
    assert tables_differ(ta, tb)  # (vpz_cqt_bins and vpz_cqt_kernel decide it)
    assert floats_b <= floats_a and CQT_F >= int(ta[1][0]) // 2 + 1  # (and the row holds the reflection of the longer kernel: N_0 = 1093 at 24 to the octave)
    alternate(lambda c, d: run_cqt(capi, c, d, noise[1]), A, B)


# (A's change, B's change) to MELSPEC: the seven fields of the bank's key, B's bank the smaller (or as large); n_fft is the twiddles' key too
MELSPEC_BANK_PAIRS = {"sample_rate": ({}, dict(sample_rate=16000)), "n_fft": (dict(n_fft=4096), {}), "n_mels": (dict(n_mels=5), {}), "f_min": ({}, dict(f_min=500.0)),
                      "f_max": ({}, dict(f_max=3000.0)), "mel_scale": (dict(mel_scale="htk"), {}), "mel_norm": ({}, dict(mel_norm=None))}


@pytest.mark.parametrize("field", sorted(MELSPEC_BANK_PAIRS))
def test_the_melspec_keys_keep_every_field(capi, noise, field):
    A, B = (dict(MELSPEC, **change) for change in MELSPEC_BANK_PAIRS[field])
    assert [k for k in sorted(MELSPEC_BANK_PAIRS) if A[k] != B[k]] == [field]
    (ba, size_a), (bb, size_b) = melspec_bank_of(capi, A), melspec_bank_of(capi, B)
    assert tables_differ(ba, bb)  # (vpz_melspec_filterbank decides it)
    assert size_b[0] <= size_a[0] and size_b[1] <= size_a[1]
    ta, tb = capi.melspec_twiddles(A["n_fft"]), capi.melspec_twiddles(B["n_fft"])
    assert tables_differ(ta, tb) == (field == "n_fft") and sum(x.size for x in tb) <= sum(x.size for x in ta)  # (vpz_melspec_twiddles)
    alternate(lambda c, d: run_melspec(capi, c, d, noise[1]), A, B)


def test_melspec_and_logmel_share_two_maps_without_meeting(capi, noise):
    """vpz_pcm_logmel at n_fft 1024 and vpz_pcm_melspec at 2048 with the other six fields of the bank's key the same, in turn, twice: both
    write into logmel_dft and logmel_banks"""
    old, new = dict(LOGMEL, n_fft=1024, hop=256), dict(MELSPEC, hop=512)
    assert all(old[k] == new[k] for k in MELSPEC_BANK_PAIRS if k != "n_fft")
    runs = [lambda c: run_logmel(capi, c, old, noise[1]), lambda c: run_melspec(capi, c, new, noise[1])]
    in_turn(lambda c, run: run(c), runs, (0, 1, 0, 1))


def test_what_is_not_in_the_stft_key_is_the_launchs(capi, noise):
    """hop, output and layout over one table"""
    B = dict(STFT, hop=96, output="power", bins_first=False)
    assert not tables_differ(stft_table_of(capi, STFT), stft_table_of(capi, B))
    in_turn(lambda c, d: run_stft(capi, c, d, noise[1]), [STFT, B], (0, 1, 0))


def test_what_is_not_in_the_cqt_key_is_the_launchs(capi, noise):
    """hop, output, layout and pad over one table (CqtTable::n0, which the table keeps, feeds the reflection's reach)"""
    B = dict(CQT, hop=48, output="magnitude", bins_first=False, pad="zero")
    assert not tables_differ(cqt_tables_of(capi, CQT)[0], cqt_tables_of(capi, B)[0])
    in_turn(lambda c, d: run_cqt(capi, c, d, noise[1]), [CQT, B], (0, 1, 0))


def test_what_is_not_in_the_melspec_keys_is_the_launchs(capi, noise):
    """hop, log or power, the floor and the layout over one table and one bank: A in decibels, B the power at another hop in the other
    layout, C is A with the median of A's powers as its floor, so that half of the elements lie under it"""
    A = dict(MELSPEC, hop=512, log=True, floor=1e-10, bands_first=True)
    B = dict(A, hop=300, log=False, floor=1e-3, bands_first=False)
    with fresh() as c:
        power = run_melspec(capi, c, dict(A, log=False), noise[1])
    floor = np.float32(np.median(power.astype(np.float64)))
    C = dict(A, floor=float(floor))
    with fresh() as c:
        a, floored = run_melspec(capi, c, A, noise[1]), run_melspec(capi, c, C, noise[1])
    under = power <= floor
    assert under.any() and not under.all() and np.unique(floored[under]).size == 1 and (a[under] <= floored[under]).all()
    assert same(a[~under], floored[~under]) and not same(a, floored)
    in_turn(lambda c, d: run_melspec(capi, c, d, noise[1]), [A, B, C], (0, 1, 2, 0, 2, 1))


def test_the_new_maps_only_grow(capi, noise):
    """24 CQT specs (f_min 250, 252, ..) and 12 STFT specs (win_length 512, 500, ..) on one context, then the first of each again: the
    repeat carries the first call's bits, the last spec of each kind its own, and those are a fresh context's"""
    cqts = [dict(CQT, f_min=250.0 + 2 * i) for i in range(24)]
    stfts = [dict(STFT, n_fft=512, win_length=512 - 12 * i) for i in range(12)]
    alone = {}
    for kind, d in (("cqt", cqts[0]), ("cqt", cqts[-1]), ("stft", stfts[0]), ("stft", stfts[-1])):
        with fresh() as c:
            alone[(kind, id(d))] = run_stage(capi, c, kind, d, noise[1])
    with fresh() as c:
        got = {}
        for kind, specs in (("cqt", cqts), ("stft", stfts)):
            for d in specs:
                got[(kind, id(d))] = run_stage(capi, c, kind, d, noise[1])
        assert len({a.tobytes() for a in got.values()}) == 36  # (36 specs, 36 tables)
        for kind, d in (("cqt", cqts[0]), ("stft", stfts[0])):
            assert same(run_stage(capi, c, kind, d, noise[1]), got[(kind, id(d))]), kind
    for key, a in alone.items():
        assert same(got[key], a), key[0]


# (the first call's spec, the 200-row call's): the second table is the smaller
QUEUED = {"stft": (STFT, dict(STFT, n_fft=512, win_length=512)), "cqt": (CQT, dict(CQT, f_min=260.0)), "melspec": (dict(MELSPEC, n_fft=4096), MELSPEC)}


@pytest.mark.parametrize("kind", sorted(QUEUED))
def test_calls_queued_back_to_back(capi, noise, kind):
    """2 rows, 200 rows of a new spec -- upload_rows's descriptor buffer grows (66 at first) and a table is built while the first kernel
    may still run --, and the first call again into a destination of its own; one synchronise behind the three"""
    X, Y = QUEUED[kind]
    F = stage_of(capi, kind, Y)[2]
    many = [(7 * i, F, i) for i in range(200)]
    with fresh() as c:
        x = run_stage(capi, c, kind, X, noise[1])
    with fresh() as c:
        y = run_stage(capi, c, kind, Y, noise[1], rows=many, dst_rows=200)
    assert np.isfinite(x).all() and np.isfinite(y).all() and not same(y[0], y[199])
    with fresh() as c:
        dsts = [destination(capi, kind, X), destination(capi, kind, Y, dst_rows=200), destination(capi, kind, X)]
        enqueue(capi, c, kind, X, noise[1], dsts[0])
        enqueue(capi, c, kind, Y, noise[1], dsts[1], rows=many)
        enqueue(capi, c, kind, X, noise[1], dsts[2])
        c.synchronize()
        got = [d.cpu().numpy() for d in dsts]
    assert same(got[0], x) and same(got[1], y) and same(got[2], x)


# ((spec, F) of context 1, of context 2): the least and the most dynamic LDS a launch of the stage asks for -- STFT 512 / 128 power frames
# first against stft_truth's widest_8192_8192_T2; melspec 2048 against 8192 at hop 8192; the CQT at hop 1 against hop 2048
TWO_CONTEXTS = {"stft": ((dict(STFT, n_fft=512, win_length=512, hop=128, output="power", bins_first=False), None),
                         (dict(STFT, n_fft=8192, win_length=8192, hop=8192), 8192 + 100)),
                "melspec": ((MELSPEC, None), (dict(MELSPEC, n_fft=8192, hop=8192), 8192 + 100)),
                "cqt": ((dict(CQT, hop=1), 300), (dict(CQT, hop=2048), 2048 * 2 + 5))}


@pytest.mark.parametrize("kind", sorted(TWO_CONTEXTS))
def test_two_contexts_alive_at_once(capi, noise, kind):
    """the launchers set the kernel's hipFuncAttributeMaxDynamicSharedMemorySize to the whole budget so that two contexts never lower it
    under each other: context 1's small launch, context 2's large one, and both again"""
    calls = TWO_CONTEXTS[kind]
    alone = []
    for d, F in calls:
        with fresh() as c:
            alone.append(run_stage(capi, c, kind, d, noise[1], F=F))
    assert np.isfinite(alone[0]).all() and np.isfinite(alone[1]).all()
    with fresh() as c1, fresh() as c2:
        for at in range(4):
            d, F = calls[at % 2]
            assert same(run_stage(capi, (c1, c2)[at % 2], kind, d, noise[1], F=F), alone[at % 2]), at
