"""vpzm_decode_ranges_cqt (include/vorbispizza_multi_cqt.h): the window batch as per-channel constant-Q spectrograms.

The call is vpzm_decode_ranges_resampled into the lane's temporary followed by vpz_pcm_cqt, so on the fixture streams it must equal
decode_ranges_resampled followed by capi.pcm_cqt bit for bit -- on the host route and with gpu_entropy, with one and two groups, mono
and stereo (two rows per entry); the statuses are the STFT call's, the rows of an entry that delivered nothing are zeros in all its
channels, VPZM_FAIL_DELIVERY ends members as VPZM_E_SYNTH with zero rows, and a spec outside the limits is VPZM_E_ARG.  The stage's
own values are tests/test_pcm_cqt_gpu.py's business; one test here holds the whole chain to the float64 truth end to end (its docstring
states the bound)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cqt_truth as ct  # noqa: E402
from cqt_truth import cqt_refused_specs  # noqa: E402
from multi_support import (bits_of_any as bits, channels_of, CQT_END_TO_END, end_to_end_entries, FIELDS, logmel_by_hand, logmel_call,  # noqa: E402
    LOGMEL_VARIANTS, MELSPEC_VARIANTS, melspec_by_hand, melspec_call, mixed_entries, most_outputs, OPTIONS, out_len, RATE, ratio,
    refused_entries_by_channel as refused_entries, resampled_call, streams)
from resample_truth import bound, resample_truth  # noqa: E402
from gpu_context import ctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

OWN = 44100  # the rate of the stereo and six-channel fixture streams
# both channels of a stereo batch as complex frames, bins first, reflected (N_0 = 3371: a row of 2100 samples holds its reflection); the
# default music spec on the mixed-down signal at 22.05 kHz, magnitudes, frames first, in the zero mode (N_0 = 11 339 is longer than the
# shortest windows)
VARIANTS = [dict(sample_rate=OWN, channels=2, mono=False, f_min=220.0, n_bins=30, bins_per_octave=12, hop=512, window="hann", scale="sqrt_length", pad="reflect",
                 output="complex", bins_first=True),
            dict(sample_rate=22050, channels=1, mono=True, f_min=32.70319566257483, n_bins=84, bins_per_octave=12, hop=512, window="hamming", scale="none",
                 pad="zero", output="magnitude", bins_first=False)]
IDS = ["stereo_44100_30_bins_complex_bins_first", "mono_22050_music_magnitude_frames_first"]


def shape_of(n, frames, spec):
    T, nb = 1 + frames // spec["hop"], spec["n_bins"]
    return (n, channels_of(spec)) + ((nb, T) if spec["bins_first"] else (T, nb))


def dtype_of(spec):
    import torch
    return torch.complex64 if spec["output"] == "complex" else torch.float32


def make_spec(spec):
    from vorbispizza_amd import capi
    return capi.CqtSpec.make(**{k: v for k, v in spec.items() if k not in ("channels", "mono")})


def reach(spec):
    """the shortest row of the spec's pad mode"""
    from vorbispizza_amd import capi
    return int(capi.cqt_bins(make_spec(spec))[1][0]) // 2 + 1 if spec["pad"] == "reflect" else 1


def cqt_call(entries, frames, spec, device_ids=(0,), dispatcher=None, out=None, **opt):
    """-> (the spectrograms as one tensor, results, stats)"""
    import torch
    from vorbispizza_amd import multi
    opt.setdefault("host_threads", 4)
    opt.setdefault("streams_per_call", 16)
    d = dispatcher or multi.Dispatcher(list(device_ids), **opt)
    try:
        parts, whole, results, stats = d.decode_ranges_cqt([s.data for s, _, _ in entries], [(a, n) for _, a, n in entries], frames, out=out, **spec)
    finally:
        if dispatcher is None:
            d.close()
    if whole is None:
        whole = torch.cat(list(parts))
    assert tuple(whole.shape) == shape_of(len(entries), frames, spec) and whole.dtype == dtype_of(spec)
    return whole, results, stats


def by_hand(ctx, entries, frames, spec, **opt):
    """capi.pcm_cqt over the planar resampled batch of the same entries, every channel a row, results["samples"] as L: what the call must
    equal"""
    import torch
    from vorbispizza_amd import capi
    Cn = channels_of(spec)
    batch, results, _ = resampled_call(entries, spec["sample_rate"], Cn, frames, True, False, spec["mono"], **opt)
    shape = shape_of(len(entries), frames, spec)
    dst = torch.full((len(entries) * Cn,) + shape[2:] + ((2,) if spec["output"] == "complex" else ()), 7.0, dtype=torch.float32, device="cuda:0")
    rows = [((k * Cn + c) * frames, int(results["samples"][k]), k * Cn + c) for k in range(len(entries)) for c in range(Cn)]
    assert capi.pcm_cqt(ctx, batch.reshape(-1), rows, dst, make_spec(spec), frames) == capi.OK, ctx.last_error()
    ctx.synchronize()
    if spec["output"] == "complex":
        dst = torch.view_as_complex(dst)
    return dst.view(shape), results


def frames_for(entries, spec, more=5):
    return max(most_outputs(entries, spec["sample_rate"]), reach(spec)) + more


@pytest.mark.parametrize("variant", [0, 1], ids=IDS)
@pytest.mark.parametrize("route", ["host", "device"])
def test_the_call_is_pcm_cqt_of_the_resampled_batch(ctx, route, variant):
    import torch
    from vorbispizza_amd import multi
    spec = VARIANTS[variant]
    entries = mixed_entries()  # (1, 2 and 6 channels; 44 100, 48 000, 22 050, 8 000 and 16 000 Hz: entries at other rates than the call's)
    frames = frames_for(entries, spec)
    want, want_results = by_hand(ctx, entries, frames, spec, **OPTIONS[route])
    got, results, _ = cqt_call(entries, frames, spec, **OPTIONS[route])
    assert torch.equal(bits(got), bits(want))
    for field in FIELDS:
        assert np.array_equal(results[field], want_results[field]), field
    assert (results["status"] == 0).sum() >= 10 and (results["samples"] > 0).any() and (results["samples"] == 0).any()
    assert torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all()
    other = np.array([s.channels != 2 for s, _, _ in entries])
    if spec["mono"]:
        assert (results["status"] != multi.E_CHANNELS).all()
    else:  # a stream of another channel count costs its entry, and its rows are zeros in both channels
        assert other.any() and (results["status"][other] == multi.E_CHANNELS).all() and (results["status"][~other] != multi.E_CHANNELS).all()
        assert not bits(got[torch.from_numpy(other).to(got.device)]).any()
        live = torch.from_numpy((results["samples"] > 1000)).to(got.device)
        assert live.any() and (got[live].abs().amax(dim=(2, 3)) > 0).all()  # both channels of every entry that delivered a window of some length


def test_one_and_two_groups_and_both_routes_carry_the_same_bits(ctx):
    import torch
    for spec in VARIANTS:
        entries = mixed_entries()[::2]
        frames = frames_for(entries, spec, 1)
        one, one_results = by_hand(ctx, entries, frames, spec, gpu_entropy=False)
        for groups in (1, 2):
            for gpu_entropy in (False, True):
                got, results, _ = cqt_call(entries, frames, spec, device_ids=[0] * groups, streams_per_call=5, gpu_entropy=gpu_entropy, host_threads=2 * groups)
                assert torch.equal(bits(got), bits(one)), (groups, gpu_entropy)
                for field in FIELDS:
                    if field != "device_slot":
                        assert np.array_equal(results[field], one_results[field]), field


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_refused_entry_costs_only_itself_and_leaves_zero_rows_in_all_its_channels(ctx, gpu_entropy):
    """the STFT call's entries and statuses (tests/test_multi_stft_gpu.py's refused_entries), in a row of J = 2100 samples"""
    import torch
    for spec in VARIANTS:
        entries, J, status, samples = refused_entries(spec)
        assert J >= reach(spec)
        want, _ = by_hand(ctx, entries, J, spec, gpu_entropy=gpu_entropy, streams_per_call=2)
        got, results, _ = cqt_call(entries, J, spec, device_ids=(0, 0), host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
        assert list(results["status"]) == status and list(results["samples"]) == samples
        assert torch.equal(bits(got), bits(want))
        img = bits(got).cpu().numpy().reshape(len(entries), channels_of(spec), -1)
        dead = [k for k in range(len(entries)) if samples[k] == 0]
        live = [k for k in range(len(entries)) if samples[k] > 0]
        assert not img[dead].any() and img[live].any(axis=2).all()  # every channel of a dead entry is zeros, every channel of a live one is not


@pytest.mark.parametrize("gpu_entropy", [False, True])
def test_a_failed_cqt_launch_costs_its_members_e_synth_and_leaves_zero_rows(ctx, monkeypatch, gpu_entropy):
    """the entries of the test above under VPZM_FAIL_DELIVERY (check_failed_delivery of multi_support.py): the resample launches into
    the lane's temporary are made, the CQT launch is not"""
    from multi_support import check_failed_delivery, sentinel_out
    from vorbispizza_amd import multi
    d = multi.Dispatcher([0, 0], host_threads=3, streams_per_call=2, gpu_entropy=gpu_entropy)
    try:
        for spec in VARIANTS:
            entries, J, _, _ = refused_entries(spec)
            check_failed_delivery(monkeypatch, d, lambda: cqt_call(entries, J, spec, dispatcher=d, out=sentinel_out(
                d, len(entries), lambda rows: shape_of(rows, J, spec), dtype_of(spec), 77.0))[:2], 0, step="vpz_pcm_cqt")
    finally:
        d.close()


def test_a_spec_outside_the_limits_is_refused(ctx):
    import torch
    from vorbispizza_amd import capi, multi
    s = streams()["stereo_coupled_res2_12"]
    entries = [(s, a, n) for a, n in s.windows()[:6]]
    spec = VARIANTS[0]
    frames = frames_for(entries, spec, 0)
    T, nb = 1 + frames // spec["hop"], spec["n_bins"]
    d = multi.Dispatcher([0, 0], host_threads=2)
    try:
        got, _, _ = cqt_call(entries, frames, spec, dispatcher=d)
        with pytest.raises(ValueError):
            d.decode_ranges_cqt([e[0].data for e in entries], [(a, n) for _, a, n in entries], frames, **dict(spec, window="povey"))
        with pytest.raises(ValueError):
            d.decode_ranges_cqt([e[0].data for e in entries], [(a, n) for _, a, n in entries], frames,
                                out=[torch.zeros((3, 2, nb, T), dtype=torch.float32, device="cuda:0")] * 2, **spec)
        with pytest.raises(multi.MultiError):
            d.decode_ranges_cqt([e[0].data for e in entries], [(a, n) for _, a, n in entries], frames, **dict(spec, n_bins=100))  # (over Nyquist)
        # the library's own refusals: VPZM_E_ARG
        n_e = len(entries)
        ptrs = (C.c_void_p * n_e)(*[e[0].data.ctypes.data for e in entries])
        sizes = (C.c_uint64 * n_e)(*[e[0].data.size for e in entries])
        rng = np.array([(x, c) for _, x, c in entries], dtype=np.int64)
        res = np.zeros(n_e, dtype=multi.RESULT_DTYPE)
        whole = torch.zeros((n_e, 2, nb, T), dtype=torch.complex64, device="cuda:0")
        dst = (C.c_void_p * 2)(whole[:3].data_ptr(), whole[3:].data_ptr())
        ok = make_spec(spec)
        args = lambda **kw: [kw.get(k, v) for k, v in (("m", d._h), ("n", n_e), ("data", ptrs), ("size", sizes), ("ranges", rng.ctypes.data),  # noqa: E731
                                                       ("rate", OWN), ("channels", 2), ("downmix", 0), ("spec", C.byref(ok)), ("frames", frames), ("dst", dst),
                                                       ("results", res.ctypes.data), ("stats", None))]
        L = multi.lib()
        assert L.vpzm_decode_ranges_cqt(*args()) == multi.OK
        assert torch.equal(bits(whole), bits(got))
        changes = [dict(spec=None), dict(frames=0), dict(frames=reach(spec) - 1), dict(dst=None), dict(m=None), dict(results=None), dict(ranges=None), dict(n=-1),
                   dict(rate=0), dict(channels=0), dict(channels=256), dict(downmix=2), dict(downmix=-1), dict(downmix=1)]  # (downmix 1 needs channels 1)
        changes += [dict(spec=C.byref(sp)) for _, sp in cqt_refused_specs(capi)]
        for change in changes:
            assert L.vpzm_decode_ranges_cqt(*args(**change)) == multi.E_ARG, change
        assert L.vpzm_decode_ranges_cqt(*args(frames=reach(spec))) == multi.OK  # (the entries that need more are refused one by one)
        zero = make_spec(dict(spec, pad="zero"))
        assert L.vpzm_decode_ranges_cqt(*args(spec=C.byref(zero), frames=reach(spec) - 1)) == multi.OK  # (the zero mode takes the shorter row)
    finally:
        d.close()


def test_the_calls_in_turn_on_one_dispatcher(ctx):
    """the lane's temporary -- mono rows for the older feature calls, planar channels of another row layout for this one -- and the
    context's table caches serve call after call: the log-mel call, the melspec call and the plain batch still deliver their old bits
    beside both CQT variants, twice round"""
    import torch
    from vorbispizza_amd import multi
    entries = mixed_entries()[::3]
    frames = max(frames_for(entries, spec, 0) for spec in VARIANTS)
    wants = [by_hand(ctx, entries, frames, spec)[0] for spec in VARIANTS]
    old_want = logmel_by_hand(ctx, entries, frames, LOGMEL_VARIANTS[0])[0]
    mel_want = melspec_by_hand(ctx, entries, frames, MELSPEC_VARIANTS[0])[0]
    stereo = resampled_call(entries, RATE, 2, frames, True, False, False)[0]
    d = multi.Dispatcher([0, 0], host_threads=4, streams_per_call=4, gpu_entropy=True)
    try:
        for _ in range(2):
            for spec, want in zip(VARIANTS, wants):
                assert torch.equal(bits(cqt_call(entries, frames, spec, dispatcher=d)[0]), bits(want))
                assert torch.equal(bits(logmel_call(entries, frames, LOGMEL_VARIANTS[0], dispatcher=d)[0]), bits(old_want))
                assert torch.equal(bits(melspec_call(entries, frames, MELSPEC_VARIANTS[0], dispatcher=d)[0]), bits(mel_want))
                assert torch.equal(bits(resampled_call(entries, RATE, 2, frames, True, False, False, dispatcher=d)[0]), bits(stereo))
    finally:
        d.close()


def test_a_fixture_window_against_the_float64_truth_end_to_end(ctx):
    """One window of a recorded stream (golden/3test.ogg, stereo) and one of the synthetic stereo stream, through decode, resample to
    22 050 Hz and the complex CQT of both channels (48 bins from 110 Hz, hop 256, reflected: N_0 = 3372), against the float64
    restatements of both definitions over the host's stream-by-stream whole decode of the same window.  The row holds the longest window's
    output samples and three hops of padding, so the last frames of the high bins lie wholly in zeros.

    THE BOUND, derived and not measured.  The resampled row the kernel reads differs from its float64 truth y by at most
    r[j] = bound(B, up, down, 1) (tests/test_resample_cpu.py, the resample's documented bound).  The CQT is linear in the row, so Re moves
    by at most sum_j r |hr_k[j]|; on top come the kernel's own roundings on the row it read, whose magnitudes are at most |y| + r.  So Re
    lies within d_re = (N_k + 2) u sum_j (|y| + r) |hr_k[j]| + sum_j r |hr_k[j]| of cqt_truth's direct sum over y, and Im the same with
    hi_k (cqt_truth.truth_of_a_row_within); tests/test_cqt_cpu.py holds the float32 restatement of the chains to the same d with r = 0.

    Largest error / bound observed on an MI355X: 0.0143 (the restatement's on the synthetic entry alone, without a device: 0.0143)."""
    rate, hop = CQT_END_TO_END["sample_rate"], CQT_END_TO_END["hop"]
    s = dict(ct.DEFAULT, **dict(CQT_END_TO_END, sample_rate=float(rate)))
    spec = dict(CQT_END_TO_END, channels=2, mono=False, output="complex", bins_first=True)
    assert ct.bins(s)[1][0] == 3372
    entries = end_to_end_entries()
    frames = most_outputs(entries, rate) + 3 * hop
    assert frames >= reach(spec)
    got, results, _ = cqt_call(entries, frames, spec, gpu_entropy=False)
    img = got.cpu().numpy().transpose(0, 1, 3, 2)  # [row][channel][T][n_bins]
    worst = 0.0
    for k, (stream, a, n) in enumerate(entries):
        up, down = ratio(stream, rate)
        m = stream.f.window(a, n)["samples"]
        J = out_len(m, up, down)
        assert results["status"][k] == 0 and results["samples"][k] == J and m == n and stream.channels == 2
        y, B = resample_truth(stream.truth(ctx, False)[a: a + m], up, down, False)
        r = bound(B, up, down, 1)
        for c in range(2):
            Z, dr, di = ct.truth_of_a_row_within(y[:, c], r[:, c], J, frames, s)
            er, ei = np.abs(img[k, c].real.astype(np.float64) - Z.real), np.abs(img[k, c].imag.astype(np.float64) - Z.imag)
            assert np.isfinite(img[k, c].real).all() and np.isfinite(img[k, c].imag).all()
            assert (er <= dr).all() and (ei <= di).all(), (k, c, float((er / np.maximum(dr, 1e-300)).max()), float((ei / np.maximum(di, 1e-300)).max()))
            assert (img[k, c].real[dr == 0] == 0).all() and (img[k, c].imag[di == 0] == 0).all()
            assert (dr == 0).any() and (di == 0).any() and (np.abs(Z) > 1e-3).any()
            worst = max(worst, float((er[dr > 0] / dr[dr > 0]).max()), float((ei[di > 0] / di[di > 0]).max()))
        assert not np.array_equal(img[k, 0], img[k, 1])  # (two channels, not one twice)
    print("end to end: largest error / bound %.4f" % worst)
