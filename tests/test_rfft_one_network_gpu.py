"""vpz_pcm_stft and vpz_pcm_melspec run ONE real-FFT network (csrc/pcm_stft.hip and csrc/pcm_melspec.hip each carry its passes;
csrc/real_fft.hpp says why): the STFT's power output, pushed through the band-sum half of the mel stage's float32 restatement -- per band
one fma32 chain over the once-rounded weights, k ascending from 0.0 -- is the mel stage's power output bit for bit.  A change to the
network's rounding made in one kernel only fails here, whatever the float32 model of the tests says.

n_fft 2048 with hann over the whole transform (the one table both stages read, tests/test_stft_cpu.py), one row of F = 1025 samples, the
smallest legal padded length, 128 bands: hop 2048 gives T = 1; hop 64 gives T = 17, one more than the mel stage's tile of 16, so both
kernels take a second tile."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from melspec_truth import band_sums32  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

N_FFT, F, N_MELS, SAMPLE_RATE = 2048, 1025, 128, 22050


@pytest.mark.parametrize("hop,T", [(2048, 1), (64, 17)])
def test_the_stft_power_through_the_band_sums_is_the_mel_power(ctx, hop, T):
    import torch
    from vorbispizza_amd import capi
    assert T == 1 + F // hop
    src = (np.random.default_rng(2048 + hop).standard_normal(F + 3) * 0.25).astype(np.float32)
    d_src = torch.from_numpy(src).to("cuda:0")
    rows = [(3, F, 0)]

    stft = capi.StftSpec.make(n_fft=N_FFT, hop=hop, win_length=N_FFT, window="hann", output="power", bins_first=False)
    P = torch.full((1, T, N_FFT // 2 + 1), float("nan"), dtype=torch.float32, device="cuda:0")
    assert capi.pcm_stft(ctx, d_src, rows, P, stft, F) == capi.OK, ctx.last_error()

    mel = capi.LogMelSpec.make(sample_rate=SAMPLE_RATE, n_fft=N_FFT, hop=hop, n_mels=N_MELS, log=False, bands_first=False)
    M = torch.full((1, T, N_MELS), float("nan"), dtype=torch.float32, device="cuda:0")
    assert capi.pcm_melspec(ctx, d_src, rows, M, mel, F) == capi.OK, ctx.last_error()
    ctx.synchronize()

    first, count, weights = capi.melspec_filterbank(mel)
    assert count.min() > 0 and weights.dtype == np.float32  # (every band is a chain of its own)
    P, M = P.cpu().numpy()[0], M.cpu().numpy()[0]
    assert np.isfinite(P).all() and (P > 0).any() and np.isfinite(M).all()
    want = band_sums32(P, first.astype(np.int64), count.astype(np.int64), weights)
    differ = np.nonzero(want.view(np.uint32) != M.view(np.uint32))
    assert differ[0].size == 0, "first of %d: frame %d band %d, %r against %r" % (
        differ[0].size, differ[0][0], differ[1][0], want[differ][0], M[differ][0])
