#!/usr/bin/env python3
"""The 1024-stream job through the in-process dispatcher under several thread / slot / sub-batch settings (one GPU, N groups).

    dispatcher_probe.py [--gpu-entropy | --mixed | --ab] [--setups K] [--reps N] [--s16-only] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --ranges SAMPLES [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --ranges SAMPLES --batch [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --pack-kernel
    dispatcher_probe.py --ranges SAMPLES --batch --resample RATE [--mono] [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --resample-kernel
    dispatcher_probe.py --ranges SAMPLES --batch --resample RATE --logmel [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --logmel-kernel
    dispatcher_probe.py --ranges SAMPLES --batch --resample RATE --melspec [--nfft N --hop H] [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --melspec-kernel
    dispatcher_probe.py --ranges SAMPLES --batch --resample RATE --stft [--nfft N --hop H] [--mono] [--stft-output complex|magnitude|power] [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --stft-kernel
    dispatcher_probe.py --ranges SAMPLES --batch --resample 22050 --cqt [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --cqt-kernel
    dispatcher_probe.py --ranges SAMPLES --batch --resample RATE --fbank [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --fbank-kernel
    dispatcher_probe.py --ranges SAMPLES --batch --resample RATE --mfcc [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --mfcc-kernel
    dispatcher_probe.py --ranges SAMPLES --batch --resample RATE --mfcc --post [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --post-kernel
    dispatcher_probe.py --loudness [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --loudness-kernel
    dispatcher_probe.py --r128 [--gpu-entropy] [--reps N] groups,threads,streams_per_call,contexts,slots ...
    dispatcher_probe.py --r128-kernel

--gpu-entropy: the dispatchers are created with vpzm_options.gpu_entropy (eligible streams entropy-decoded on the device).
--mixed: ... and with mixed_setups (vpzm_set_mixed_setups: streams of different setups share device-decoded sub-batches).
--ab: for every setting TWO dispatchers in this process, the option off and on, take the job in turn, --reps times each
(default 5): medians and extremes of both, and the PCM of the two compared.  The option is gpu_entropy; with --mixed it is
mixed_setups, gpu_entropy on in both.
--setups K: the mixed-library job instead of the two fixtures' -- STREAMS streams drawn round-robin from K stereo 256/2048 setups of
the writer (tests/synthetic_streams.py: stereo_coupled_res2(2 + 10 k), --setup-packets packets each, default 300) and the two
fixtures.  Building them takes seconds each: with VPZ_PROBE_CACHE=DIR they are kept there.
A line "counts" follows every result: sub_batches, device-decoded and mixed ones, decoders_created of the last call (a build
without vpzm_last_call_counts, taken through VPZ_LIB_DIR, prints none).
--ranges SAMPLES: one window of SAMPLES samples per stream at a seeded random start, 16-bit PCM, into a dense [streams][SAMPLES][2] array.
The A/B: vpzm_decode_library of the whole streams followed by slicing on the host (the slicing timed with it) against vpzm_decode_ranges,
two dispatchers in this process taking turns, --reps times each (default 5), the pair of series run twice; the two dense arrays are
compared.  Every line gives the median and the extremes of its series: a difference inside the extremes is no difference.
--ranges SAMPLES --batch: the same windows delivered as a device tensor [streams][2][SAMPLES], int16.  The A/B: vpzm_decode_ranges into
page-locked memory (every window placed in its padded row there), torch.from_numpy(...).to(device) and the transposition to planar on the
device, against vpzm_decode_ranges_batch; two dispatchers taking turns as above, the two tensors compared.
--pack-kernel: vpz_pcm_pack alone for one sub-batch of 64 one-second stereo windows (44 100 samples from odd offsets of areas a block
apart), every layout, timed with the context's event timer: median of 20 launches and the bytes it moves.
--ranges SAMPLES --batch --resample RATE: the same windows as a float32 device tensor at RATE Hz ([streams][2][J], or [streams][1][J] with
--mono).  The A/B: what a loader does without the call -- vpzm_decode_ranges_batch at the source rate, then torch conv1d with the same
coefficient table (vpz_resample_filter) at stride = down, a reshape and the channels' mean on the device -- against
vpzm_decode_ranges_resampled; two dispatchers taking turns as above, the largest difference of the two tensors printed.
--resample-kernel: vpz_pcm_resample alone for the same 64 windows, 44 100 -> 16 000 Hz, every layout and the mono mix.
--ranges SAMPLES --batch --resample RATE --logmel: the same windows as log-mel features of the Whisper spec (n_fft 400, hop 160, 80 Slaney
bands, floor 1e-10), a float32 device tensor [streams][80][T].  The A/B: what a loader does without the call -- decode_ranges_batch at
RATE Hz, mono, then on the device torch.stft (center, reflect, periodic Hann), abs() ** 2, a matmul with the same filterbank
(vpz_mel_filterbank as a dense matrix), clamp and log10 -- against decode_ranges_logmel; two dispatchers taking turns as above, the
largest difference of the two tensors printed.  With VPZM_PROFILE=1 the library prints the log-mel launch's own time per sub-batch.
--logmel-kernel: vpz_pcm_logmel alone, the Whisper spec, 64 windows of one second and of thirty, both layouts, the context's event timer.
--ranges SAMPLES --batch --resample RATE --melspec: the same windows as mel spectrograms of a music front end (n_fft 2048, hop 512 -- or
--nfft / --hop --, 128 Slaney bands, log10) -- what a loader does without the call, decode_ranges_batch(mono) + torch.stft, power, matmul with the
same bank (vpz_melspec_filterbank as a dense matrix), clamp and log10 -- against decode_ranges_melspec; two dispatchers taking turns as
above.  Both legs are held to one truth: the same chain in float64 (torch, on the float32 rows the batch call delivers).
--melspec-kernel: vpz_pcm_melspec alone, 64 windows of one second and of thirty at 44 100 Hz, at 2048 / 512 / 128 and 4096 / 1024 / 128, the
context's event timer; the time, and the HBM bytes that must move (PCM read plus mel write) against it.
--ranges SAMPLES --batch --resample RATE --stft: the same windows as STFT spectrograms of every channel (or, with --mono, of the mixed-down
one) at --nfft / --hop, periodic Hann, --stft-output complex (the default), magnitude or power, in torch's order -- what a loader does
without the call, decode_ranges_batch at RATE Hz + torch.stft with the same window (and abs() or abs() ** 2) -- against
decode_ranges_stft; two dispatchers taking turns as above.  Both legs are held to one truth: torch.stft in float64 on the float32 rows
the batch call delivers.
--stft-kernel: vpz_pcm_stft alone, 64 stereo windows (128 rows) of one second and of thirty at 44 100 Hz, at 4096 / 1024 complex, 1024 / 256
magnitude and 2048 / 512 power, both layouts, the context's event timer; the time, the bytes it stores per second, and vpz_pcm_melspec on
the same rows at the same n_fft and hop where it takes the size.
--ranges SAMPLES --batch --resample RATE --cqt: the same windows as constant-Q spectrograms of the mixed-down signal at the default music spec
(84 bins from 32.70 Hz, 12 to the octave, hop 512, magnitude, bins first; RATE is the spec's sample rate) -- what a loader does without the
call, decode_ranges_batch(mono) at RATE Hz, then one float32 torch.nn.functional.conv1d over the reflect-padded rows with the same kernels
(vpz_cqt_kernel's) zero-padded to N_0 and stride hop, then the magnitude -- against decode_ranges_cqt; two dispatchers taking turns as above.
--cqt-kernel: vpz_pcm_cqt alone, 64 mono rows of one second and of thirty at the default spec, magnitude, bins first, the context's event
timer; the time, and the multiply-add rate over sum N_k (what the definition needs) and over the padded block lengths (what the kernel
runs), each as a fraction of the 157 TFLOP/s float32 matrix peak.
--ranges SAMPLES --batch --resample RATE --fbank: the same windows as Kaldi filterbank features (win 400, hop 160, n_fft 512, 80 bands, Povey
window, pre-emphasis 0.97, per-frame mean removal, scale 32768, natural log), a float32 device tensor [streams][T][80].  The A/B: what a
loader does without the call -- decode_ranges_batch at RATE Hz, mono, then on the device the eight torch ops unfold, mean, pre-emphasis,
window, pad, rfft, power, matmul (vpz_fbank_filterbank as a dense matrix) and log -- against decode_ranges_fbank; two dispatchers taking
turns as above, the largest difference of the two tensors printed.  With VPZM_PROFILE=1 the library prints the fbank launch's own time.
--fbank-kernel: vpz_pcm_fbank alone, that spec, 64 windows of one second and of thirty, both layouts, the context's event timer.
--ranges SAMPLES --batch --resample RATE --mfcc: the same windows as Kaldi MFCC features (13 cepstra of 23 bands, lifter 22, C0 replaced by
the raw log energy, cepstral mean subtraction), a float32 device tensor [streams][T][13].  The A/B: what a loader does without the call
-- decode_ranges_fbank with 23 bands, a SECOND decode through decode_ranges_batch at RATE Hz, mono, for the energy, then on the device
unfold, mean and square-sum on that PCM, a matmul with the liftered DCT (vpz_mfcc_table), the column overwrite, the mean over the frames
and the subtraction -- against decode_ranges_mfcc; two dispatchers taking turns as above, the largest difference of the two tensors
printed.  With VPZM_PROFILE=1 the library prints the MFCC launches' own time.
--mfcc-kernel: vpz_pcm_mfcc alone (with and without subtract_mean) next to vpz_pcm_fbank at the same mel spec (23 bands), 64 windows of one
second and of thirty, the context's event timer: medians of 10 with their extremes.
--ranges SAMPLES --batch --resample RATE --mfcc --post: the same windows as Kaldi MFCC features (the defaults, no cepstral mean) with
add-deltas | apply-cmvn-sliding --cmn-window=300 --center=true behind them (deltas of order 2, window 2, then the sliding mean over all 39
columns), a float32 device tensor [streams][T][39].  The A/B: what a loader does without the call -- decode_ranges_mfcc, then on the
device the mask of the pad frames, one replicate-padded conv1d per order with the convolved scales (vpz_feat_delta_scales; right for rows
that fill T, which all of this job's do), a float64 cumsum and the window's ends per row with the edge rules, two gathers, the mean and
the subtraction -- against decode_ranges_mfcc_post; two dispatchers taking turns as above, the largest difference of the two tensors
printed.
--post-kernel: vpz_feat_post alone (that spec, its two stages alone, and the other order) next to vpz_pcm_mfcc at the same shapes, 64 rows
of one second and of thirty at 13 columns, the context's event timer: medians of 10 with their extremes, and the bytes per second
against the source tensor's read plus the destination's write.
--loudness: the whole streams measured for programme loudness (BS.1770).  The A/B: what a scanner has to do first without the call --
vpzm_decode_library of the whole streams into float32 page-locked memory, to which its host scan (two IIR filters and a gated mean over
all of it) could only add -- against measure_loudness, which brings no PCM down; two dispatchers taking turns as above.  The records of
the first two streams are printed.  With VPZM_PROFILE=1 the library prints the loudness launches' own time per sub-batch.
--loudness-kernel: vpz_pcm_loudness alone, 64 stereo rows of one second and of 200 seconds at 44 100 Hz, the context's event timer.
--r128: the whole streams measured for everything an EBU R 128 scanner reports (measure_r128: the integrated loudness, the range, the
maxima, the true peak).  Three dispatchers taking turns: decode_library into float32 page-locked memory, measure_loudness and
measure_r128 -- the cost of the added numbers, and what a host scanner must do first.  The records of the first two streams are
printed.  With VPZM_PROFILE=1 the library prints the loudness and the true-peak launches' own time per sub-batch.
--r128-kernel: vpz_pcm_true_peak alone and vpz_pcm_loudness beside it, the same rows as --loudness-kernel, the context's event timer:
the median of 5 with its extremes, GB/s against 8 TB/s and multiply-adds per second against the float32 vector peak (157.3 TFLOP/s).
--ranges SAMPLES --batch --resample RATE [--mono] --normalize MODE (meanvar, peak, rms or loudness): the window batch delivered normalised
(vorbispizza_amd.normalize.decode_ranges_normalized) against what a loader does without the call: decode_ranges_batch at the same rate,
then the torch chain -- a mask from results["samples"], the masked mean and variance (or peak, or RMS) and the scale --, with a
measure_loudness call in front of it for the loudness mode (the second decode that the call saves).  Both legs' first rows are held to
the longdouble truth of tests/normalize_truth.py with the header's bound; two dispatchers taking turns as above.
--normalize-kernel: vpz_pcm_normalize alone, 64 mono rows of one second and of thirty at 16 000 Hz from odd offsets, the context's event
timer: the median of 10 with its extremes, and the bytes moved (a float32 row is read twice and written once: 12 B per sample) per
second against 8 TB/s."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import bench
from vorbispizza_amd import multi
ap = argparse.ArgumentParser()
ap.add_argument("--gpu-entropy", action="store_true")
ap.add_argument("--ab", action="store_true")
ap.add_argument("--mixed", action="store_true")
ap.add_argument("--setups", type=int, default=0)
ap.add_argument("--setup-packets", type=int, default=300)
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--s16-only", action="store_true")
ap.add_argument("--ranges", type=int, default=0)
ap.add_argument("--batch", action="store_true")
ap.add_argument("--pack-kernel", action="store_true")
ap.add_argument("--resample", type=int, default=0)
ap.add_argument("--mono", action="store_true")
ap.add_argument("--resample-kernel", action="store_true")
ap.add_argument("--logmel", action="store_true")
ap.add_argument("--logmel-kernel", action="store_true")
ap.add_argument("--melspec", action="store_true")
ap.add_argument("--melspec-kernel", action="store_true")
ap.add_argument("--stft", action="store_true")
ap.add_argument("--stft-kernel", action="store_true")
ap.add_argument("--stft-output", default="complex")
ap.add_argument("--cqt", action="store_true")
ap.add_argument("--cqt-kernel", action="store_true")
ap.add_argument("--nfft", type=int, default=2048)
ap.add_argument("--hop", type=int, default=512)
ap.add_argument("--fbank", action="store_true")
ap.add_argument("--fbank-kernel", action="store_true")
ap.add_argument("--mfcc", action="store_true")
ap.add_argument("--mfcc-kernel", action="store_true")
ap.add_argument("--post", action="store_true")
ap.add_argument("--post-kernel", action="store_true")
ap.add_argument("--loudness", action="store_true")
ap.add_argument("--loudness-kernel", action="store_true")
ap.add_argument("--r128", action="store_true")
ap.add_argument("--r128-kernel", action="store_true")
ap.add_argument("--normalize", default="")
ap.add_argument("--normalize-kernel", action="store_true")
ap.add_argument("settings", nargs="*")
args = ap.parse_args()
streams = int(os.environ.get("STREAMS", "1024"))
raws = [np.frombuffer(open(os.path.join(ROOT, "tests", "golden", n), "rb").read(), dtype=np.uint8) for n, _ in bench.REAL_FIXTURES]
caps1 = [smp + 2048 for _, smp in bench.REAL_FIXTURES]


def writer_stream(k, packets):
    """stereo_coupled_res2(2 + 10 k) with `packets` packets, as a uint8 array (kept under VPZ_PROBE_CACHE when that is set)"""
    cache = os.environ.get("VPZ_PROBE_CACHE")
    path = os.path.join(cache, "stereo_%d_%d.ogg" % (2 + 10 * k, packets)) if cache else None
    if path and os.path.exists(path):
        return np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
    import synthetic_streams as ss
    st, rng = ss.stereo_coupled_res2(2 + 10 * k)
    raw = bytes(st.build(rng, packets)[0])
    if path:
        os.makedirs(cache, exist_ok=True)
        open(path, "wb").write(raw)
    return np.frombuffer(raw, dtype=np.uint8)


if args.setups:
    from vorbispizza_amd.front import OggVorbisFile
    raws += [writer_stream(k, args.setup_packets) for k in range(args.setups)]
    for r in raws[2:]:
        f = OggVorbisFile(r.tobytes())
        assert f.gpu_decode_supported and f.channels == 2
        caps1.append(int(f.total_samples) + 2048)
        f.close()
    pick = [2 + i % args.setups for i in range(streams - 2)] + [0, 1]
else:
    pick = [i % 2 for i in range(streams)]
datas = [raws[i] for i in pick]
caps = np.array([caps1[i] for i in pick], dtype=np.int64)
offs = np.concatenate([[0], np.cumsum(caps * 2)[:-1]]).astype(np.int64)


def counts_line(d):
    if not hasattr(multi.lib(), "vpzm_last_call_counts"):
        return ""
    c = d.call_counts()
    return "\n    counts: %d sub-batches (%d device-decoded, %d mixed, at most %d setups in one), %d decoders created in the last call" % (
        c.sub_batches, c.device_decoded_sub_batches, c.mixed_sub_batches, c.max_setups_per_sub_batch, c.decoders_created)


def describe(walls):
    return "median %.1f ms (min %.1f, max %.1f)" % (statistics.median(walls) * 1e3, min(walls) * 1e3, max(walls) * 1e3)


def ranges_job(samples):
    import time
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    starts = np.array([int(rng.integers(0, totals[i] - samples - 64)) for i in pick], dtype=np.int64)  # (issue6test.ogg ends 63 samples short)
    windows = [(int(a), samples) for a in starts]
    n = len(datas)
    whole = torch.empty(int((caps * 2).sum()), dtype=torch.int16, pin_memory=True).numpy()
    dense = [torch.empty(n * samples * 2, dtype=torch.int16, pin_memory=True).numpy() for _ in range(2)]
    d_offs, d_caps = np.arange(n, dtype=np.int64) * samples * 2, np.full(n, samples, dtype=np.int64)

    def by_library(d):
        t0 = time.perf_counter()
        res, st = d.decode_library(datas, whole, offs, caps, s16=True)
        out = dense[0].reshape(n, samples * 2)
        for k in range(n):  # the host's slicing: what a caller of the whole decode does to get its windows
            out[k] = whole[offs[k] + starts[k] * 2: offs[k] + (starts[k] + samples) * 2]
        return time.perf_counter() - t0, res, st

    def by_ranges(d):
        t0 = time.perf_counter()
        res, st = d.decode_ranges(datas, windows, dense[1], d_offs, d_caps, s16=True)
        return time.perf_counter() - t0, res, st

    def series(legs, reps):
        walls = [[] for _ in legs]
        for _ in range(reps):
            for i, leg in enumerate(legs):
                wall, res, st = leg()
                assert (res["status"] == 0).all()
                walls[i].append(wall)
        return walls

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "s16 groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        _, res_lib, _ = by_library(ds[0])  # (one pass each that does not count: slots, decoders and device arrays are allocated in it)
        _, res, st = by_ranges(ds[1])
        assert (res["samples"] == samples).all() and np.array_equal(dense[0], dense[1]), "the windows differ from the slices of the whole decode"
        print("%s:\n    packets decoded: %d of %d (%.1f %%), pinned %d MiB, %d streams on the device" % (
            what, int(res["packets"].sum()), int(res_lib["packets"].sum()), 100.0 * res["packets"].sum() / res_lib["packets"].sum(), st.pinned_mib,
            int(sum(st.device_gpu_entropy_streams))), flush=True)
        for run in (1, 2):
            walls = series([lambda: by_library(ds[0]), lambda: by_ranges(ds[1])], args.reps or 5)
            print("    A/B run %d: decode_library + host slicing %s; decode_ranges %s" % (run, describe(walls[0]), describe(walls[1])), flush=True)
        for d in ds:
            d.close()


def batch_job(samples):
    import time
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    n = len(datas)
    padded = torch.zeros((n, samples, 2), dtype=torch.int16, pin_memory=True)  # (frames = SAMPLES: a row is one window, placed by its offset)
    d_offs, d_caps = np.arange(n, dtype=np.int64) * samples * 2, np.full(n, samples, dtype=np.int64)
    out = [None, None]

    def by_ranges_and_upload(d):
        t0 = time.perf_counter()
        res, st = d.decode_ranges(datas, windows, padded.numpy().reshape(-1), d_offs, d_caps, s16=True)
        out[0] = torch.from_numpy(padded.numpy()).to("cuda:0", non_blocking=True).permute(0, 2, 1).contiguous()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res, st

    def by_batch(d):
        t0 = time.perf_counter()
        _, out[1], res, st = d.decode_ranges_batch(datas, windows, 2, samples, planar=True, s16=True)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "s16 groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_ranges_and_upload(ds[0]), lambda: by_batch(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders and device arrays are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all() and (res["samples"] == samples).all()
        assert torch.equal(out[0], out[1]), "the batch differs from the uploaded windows"
        print("%s:\n    a tensor of %.1f MB, pinned %d MiB, %d streams on the device" % (
            what, out[1].numel() * 2 / 1e6, st.pinned_mib, int(sum(st.device_gpu_entropy_streams))), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_ranges + upload %s; decode_ranges_batch %s" % (run, describe(walls[0]), describe(walls[1])), flush=True)
        for d in ds:
            d.close()


def pack_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n, samples, area = 64, 44100, 44100 + 2 * 2048
    rows = [(k * area * 2 + 2 * (2 * k + 1) + 1 - 1, samples, k) for k in range(n)]  # (an odd number of samples into every area)
    for name, lay, dtype in (("planar f32", capi.OUT_PLANAR, torch.float32), ("interleaved f32", capi.OUT_INTERLEAVED, torch.float32),
                             ("planar s16", capi.OUT_PLANAR_S16, torch.int16), ("interleaved s16", capi.OUT_INTERLEAVED_S16, torch.int16)):
        src = (torch.rand(n * area * 2, device="cuda:0") * 2000 - 1000).to(dtype)
        planar = lay in (capi.OUT_PLANAR, capi.OUT_PLANAR_S16)
        dst = torch.empty((n, 2, samples) if planar else (n, samples, 2), dtype=dtype, device="cuda:0")
        times = []
        for _ in range(21):
            ctx.timer_start()
            assert capi.pcm_pack(ctx, src, rows, dst, lay) == capi.OK, ctx.last_error()
            times.append(ctx.timer_stop())
        want = torch.stack([src[a: a + samples * 2].view(samples, 2) for a, _, _ in rows])
        assert torch.equal(dst, want.permute(0, 2, 1) if planar else want)
        moved = 2 * dst.numel() * dst.element_size()  # (read once, written once)
        ms = statistics.median(times[1:])
        print("vpz_pcm_pack %-16s 64 windows of 44100 stereo samples: median %.1f us (min %.1f, max %.1f) for %.2f MB read + written = %.0f GB/s" % (
            name, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3, moved / 1e6, moved / ms / 1e6), flush=True)
    ctx.close()


def conv_table(up, down):
    """vpz_resample_filter's table as ONE conv1d weight [up][1][W] for stride = down: phase p's taps start floor(p * down / up) + first_tap[p]
    samples from the frame's first source sample; -> (weight on the device, the padding in front)"""
    from vorbispizza_amd import capi
    taps, first, coeffs = capi.resample_filter(up, down)
    off = np.arange(up, dtype=np.int64) * down // up + first
    lo, width = int(off.min()), int((off + taps).max() - off.min())
    weight = np.zeros((up, 1, width), dtype=np.float32)
    for p in range(up):
        weight[p, 0, off[p] - lo: off[p] - lo + taps] = coeffs[p]
    return torch.from_numpy(weight).to("cuda:0"), -lo


def resample_job(samples, rate):
    import math, time
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    n, out = len(datas), [None, None]
    state = {}

    def by_batch_and_torch(d):
        t0 = time.perf_counter()
        _, whole, res, st = d.decode_ranges_batch(datas, windows, 2, samples, planar=True, s16=False)
        if "weight" not in state:  # (every stream of the set has one rate: one ratio, one table, built once like the library's)
            fs = int(res["sample_rate"][0])
            assert (res["sample_rate"] == fs).all()
            g = math.gcd(fs, rate)
            state["up"], state["down"] = rate // g, fs // g
            state["weight"], state["front"] = conv_table(state["up"], state["down"])
        up, down, w = state["up"], state["down"], state["weight"]
        J = -(-samples * up // down)
        x = torch.nn.functional.pad(whole.view(n * 2, 1, samples), (state["front"], w.shape[2] + down))
        y = torch.nn.functional.conv1d(x, w, stride=down).transpose(1, 2).reshape(n, 2, -1)[:, :, :J]
        out[0] = y.mean(dim=1, keepdim=True) if args.mono else y.contiguous()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res, st

    def by_resampled(d):
        t0 = time.perf_counter()
        J = -(-samples * state["up"] // state["down"])
        _, out[1], res, st = d.decode_ranges_batch(datas, windows, 1 if args.mono else 2, J, planar=True, s16=False, sample_rate=rate, mono=args.mono)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "f32 groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples to %d Hz%s" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples, rate, ", mono" if args.mono else "")
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_batch_and_torch(ds[0]), lambda: by_resampled(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders, device arrays and tables are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all()
        assert out[0].shape == out[1].shape
        print("%s:\n    ratio %d / %d, a tensor of %.1f MB, largest difference of the two tensors %.3g (largest sample %.3g), %d streams on the device" % (
            what, state["up"], state["down"], out[1].numel() * 4 / 1e6, float((out[0] - out[1]).abs().max()), float(out[1].abs().max()),
            int(sum(st.device_gpu_entropy_streams))), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_ranges_batch + torch conv1d %s; decode_ranges_resampled %s" % (run, describe(walls[0]), describe(walls[1])), flush=True)
        for d in ds:
            d.close()


def resample_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n, samples, area, up, down = 64, 44100, 44100 + 2 * 2048, 160, 441
    J = -(-samples * up // down)
    rows = [(k * area * 2 + 2 * (2 * k + 1), samples, k) for k in range(n)]
    src = (torch.rand(n * area, 2, device="cuda:0") * 2 - 1)
    for name, lay, dtype, mono in (("planar f32", capi.OUT_PLANAR, torch.float32, False), ("interleaved f32", capi.OUT_INTERLEAVED, torch.float32, False),
                                   ("planar s16", capi.OUT_PLANAR_S16, torch.int16, False), ("interleaved s16", capi.OUT_INTERLEAVED_S16, torch.int16, False),
                                   ("mono f32", capi.OUT_PLANAR, torch.float32, True), ("mono s16", capi.OUT_PLANAR_S16, torch.int16, True)):
        co = 1 if mono else 2
        planar = lay in (capi.OUT_PLANAR, capi.OUT_PLANAR_S16)
        dst = torch.empty((n, co, J) if planar else (n, J, co), dtype=dtype, device="cuda:0")
        times = []
        for _ in range(21):
            ctx.timer_start()
            assert capi.pcm_resample(ctx, src, rows, dst, lay, up, down, mono) == capi.OK, ctx.last_error()
            times.append(ctx.timer_stop())
        moved = n * samples * 2 * 4 + dst.numel() * dst.element_size()  # (the windows read once, the rows written once)
        ms = statistics.median(times[1:])
        print("vpz_pcm_resample %-16s 64 windows of 44100 stereo samples to 16000 Hz: median %.1f us (min %.1f, max %.1f) for %.2f MB read + written = %.0f GB/s" % (
            name, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3, moved / 1e6, moved / ms / 1e6), flush=True)
    ctx.close()


def dense_filterbank(spec):
    """vpz_mel_filterbank as a dense [n_mels][n_fft / 2 + 1] float32 matrix on the device"""
    from vorbispizza_amd import capi
    first, count, weights = capi.mel_filterbank(spec)
    W, at = np.zeros((spec.n_mels, spec.n_fft // 2 + 1), dtype=np.float32), 0
    for b in range(spec.n_mels):
        W[b, first[b]: first[b] + count[b]] = weights[at: at + count[b]]
        at += count[b]
    return torch.from_numpy(W).to("cuda:0")


def logmel_job(samples, rate):
    import math, time
    from vorbispizza_amd import capi
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    n, out = len(datas), [None, None]
    spec = capi.LogMelSpec.make(sample_rate=rate)
    W, window = dense_filterbank(spec), torch.hann_window(spec.n_fft, periodic=True, device="cuda:0")
    fs = 44100  # (both fixtures)
    J = -(-samples * (rate // math.gcd(fs, rate)) // (fs // math.gcd(fs, rate)))

    def by_batch_and_torch(d):
        t0 = time.perf_counter()
        _, whole, res, st = d.decode_ranges_batch(datas, windows, 1, J, planar=True, s16=False, sample_rate=rate, mono=True)
        S = torch.stft(whole.view(n, J), spec.n_fft, hop_length=spec.hop, window=window, center=True, pad_mode="reflect", return_complex=True)
        out[0] = torch.log10(torch.clamp(torch.matmul(W, S.abs() ** 2), min=spec.floor))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res, st

    def by_logmel(d):
        t0 = time.perf_counter()
        _, out[1], res, st = d.decode_ranges_logmel(datas, windows, J, sample_rate=rate)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples to %d Hz, log-mel 400/160/80" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples, rate)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_batch_and_torch(ds[0]), lambda: by_logmel(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders, device arrays and tables are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all() and (res["samples"] == J).all()
        assert out[0].shape == out[1].shape
        print("%s:\n    rows of %d samples, a tensor of %.1f MB (the complex spectrogram it replaces: %.1f MB), largest difference of the two tensors %.3g (log10 units)" % (
            what, J, out[1].numel() * 4 / 1e6, n * (spec.n_fft // 2 + 1) * out[1].shape[2] * 8 / 1e6, float((out[0] - out[1]).abs().max())), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_ranges_batch(mono) + torch stft/power/matmul/log %s; decode_ranges_logmel %s" % (run, describe(walls[0]), describe(walls[1])),
                  flush=True)
        for d in ds:
            d.close()


def logmel_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n = 64
    for samples in (16000, 480000):
        src = (torch.rand(n * (samples + 3), device="cuda:0") * 2 - 1)
        rows = [(k * (samples + 3) + 1, samples, k) for k in range(n)]
        for name, bands_first in (("bands first", True), ("frames first", False)):
            spec = capi.LogMelSpec.make(bands_first=bands_first)
            T = spec.n_frames(samples)
            dst = torch.empty((n, 80, T) if bands_first else (n, T, 80), dtype=torch.float32, device="cuda:0")
            times = []
            for _ in range(11):
                ctx.timer_start()
                assert capi.pcm_logmel(ctx, src, rows, dst, spec, samples) == capi.OK, ctx.last_error()
                times.append(ctx.timer_stop())
            ms = statistics.median(times[1:])
            flop = 2.0 * n * T * 400 * 402
            print("vpz_pcm_logmel %-12s 64 windows of %6d samples (T = %4d): median %.1f us (min %.1f, max %.1f); %.2f GFLOP of DFT = %.1f TFLOP/s; %.1f MB out, "
                  "%.1f MB of spectrogram not written" % (name, samples, T, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3, flop / 1e9, flop / ms / 1e9,
                                                          dst.numel() * 4 / 1e6, n * 201 * T * 8 / 1e6), flush=True)
    ctx.close()


def melspec_job(samples, rate):
    import math, time
    from vorbispizza_amd import capi
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    n, out = len(datas), [None, None]
    spec = capi.LogMelSpec.make(sample_rate=rate, n_fft=args.nfft, hop=args.hop, n_mels=128)
    first, count, weights = capi.melspec_filterbank(spec)
    Wh, at = np.zeros((spec.n_mels, spec.n_fft // 2 + 1), dtype=np.float32), 0
    for b in range(spec.n_mels):
        Wh[b, first[b]: first[b] + count[b]] = weights[at: at + count[b]]
        at += count[b]
    W, window = torch.from_numpy(Wh).to("cuda:0"), torch.hann_window(spec.n_fft, periodic=True, device="cuda:0")
    fs = 44100  # (both fixtures)
    J = -(-samples * (rate // math.gcd(fs, rate)) // (fs // math.gcd(fs, rate)))
    state = {}

    def by_batch_and_torch(d):
        t0 = time.perf_counter()
        _, whole, res, st = d.decode_ranges_batch(datas, windows, 1, J, planar=True, s16=False, sample_rate=rate, mono=True)
        S = torch.stft(whole.view(n, J), spec.n_fft, hop_length=spec.hop, window=window, center=True, pad_mode="reflect", return_complex=True)
        out[0] = torch.log10(torch.clamp(torch.matmul(W, S.abs() ** 2), min=spec.floor))
        torch.cuda.synchronize()
        state["rows"] = whole
        return time.perf_counter() - t0, res, st

    def by_melspec(d):
        t0 = time.perf_counter()
        _, out[1], res, st = d.decode_ranges_melspec(datas, windows, J, sample_rate=rate, n_fft=spec.n_fft, hop=spec.hop, n_mels=spec.n_mels)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples to %d Hz, mel %d/%d/%d" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples, rate, spec.n_fft, spec.hop, spec.n_mels)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_batch_and_torch(ds[0]), lambda: by_melspec(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders, device arrays and tables are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all() and (res["samples"] == J).all()
        assert out[0].shape == out[1].shape
        # one truth for both legs: the same chain in float64 on the rows the batch call delivered (eight rows are enough to say)
        rows64 = state["rows"].view(n, J)[:8].double()
        S64 = torch.stft(rows64, spec.n_fft, hop_length=spec.hop, window=torch.hann_window(spec.n_fft, periodic=True, device="cuda:0", dtype=torch.float64),
                         center=True, pad_mode="reflect", return_complex=True)
        truth = torch.log10(torch.clamp(torch.matmul(W.double(), S64.abs() ** 2), min=float(np.float32(spec.floor))))
        print("%s:\n    rows of %d samples, a tensor of %.1f MB (the complex spectrogram it replaces: %.1f MB), largest difference of the two tensors %.3g; against the "
              "float64 chain: torch %.3g, decode_ranges_melspec %.3g (log10 units)" % (
                  what, J, out[1].numel() * 4 / 1e6, n * (spec.n_fft // 2 + 1) * out[1].shape[2] * 8 / 1e6, float((out[0] - out[1]).abs().max()),
                  float((out[0][:8].double() - truth).abs().max()), float((out[1][:8].double() - truth).abs().max())), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_ranges_batch(mono) + torch stft/power/matmul/log %s; decode_ranges_melspec %s" % (run, describe(walls[0]), describe(walls[1])),
                  flush=True)
        for d in ds:
            d.close()


def melspec_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n, rate = 64, 44100
    for n_fft, hop in ((2048, 512), (4096, 1024)):
        for samples in (rate, 30 * rate):
            src = (torch.rand(n * (samples + 3), device="cuda:0") * 2 - 1)
            rows = [(k * (samples + 3) + 1, samples, k) for k in range(n)]
            for name, bands_first in (("bands first", True), ("frames first", False)):
                spec = capi.LogMelSpec.make(sample_rate=rate, n_fft=n_fft, hop=hop, n_mels=128, bands_first=bands_first)
                T = spec.n_frames(samples)
                dst = torch.empty((n, 128, T) if bands_first else (n, T, 128), dtype=torch.float32, device="cuda:0")
                for run in (1, 2):
                    times = []
                    for _ in range(6):
                        ctx.timer_start()
                        assert capi.pcm_melspec(ctx, src, rows, dst, spec, samples) == capi.OK, ctx.last_error()
                        times.append(ctx.timer_stop())
                    ms = statistics.median(times[1:])
                    moved = n * samples * 4 + dst.numel() * 4  # (the PCM read once, the mel frames written once)
                    print("vpz_pcm_melspec %d/%d/128 %-12s 64 windows of %7d samples (T = %4d) run %d: median of 5 %.1f us (min %.1f, max %.1f); %.1f MB must move = "
                          "%.0f GB/s; %.1f MB of spectrogram not written" % (n_fft, hop, name, samples, T, run, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3,
                                                                             moved / 1e6, moved / ms / 1e6, n * (n_fft // 2 + 1) * T * 8 / 1e6), flush=True)
    ctx.close()


def stft_job(samples, rate):
    import math, time
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    n, out = len(datas), [None, None]
    n_fft, hop, output, Cn = args.nfft, args.hop, args.stft_output, 1 if args.mono else 2
    window = torch.hann_window(n_fft, periodic=True, device="cuda:0")
    fs = 44100  # (both fixtures, stereo)
    J = -(-samples * (rate // math.gcd(fs, rate)) // (fs // math.gcd(fs, rate)))
    state = {}

    def of(S):
        return S if output == "complex" else S.abs() if output == "magnitude" else S.abs() ** 2

    def by_batch_and_torch(d):
        t0 = time.perf_counter()
        _, whole, res, st = d.decode_ranges_batch(datas, windows, Cn, J, planar=True, s16=False, sample_rate=rate, mono=args.mono)
        S = torch.stft(whole.view(n * Cn, J), n_fft, hop_length=hop, window=window, center=True, pad_mode="reflect", return_complex=True)
        out[0] = of(S).view(n, Cn, n_fft // 2 + 1, -1)
        torch.cuda.synchronize()
        state["rows"] = whole
        return time.perf_counter() - t0, res, st

    def by_stft(d):
        t0 = time.perf_counter()
        _, out[1], res, st = d.decode_ranges_stft(datas, windows, J, sample_rate=rate, channels=Cn, mono=args.mono, n_fft=n_fft, hop=hop, output=output)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples to %d Hz, stft %d/%d %s of %d channel%s" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples, rate, n_fft, hop, output, Cn, "s" if Cn > 1 else "")
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_batch_and_torch(ds[0]), lambda: by_stft(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders, device arrays and tables are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all() and (res["samples"] == J).all()
        assert out[0].shape == out[1].shape and out[0].dtype == out[1].dtype
        # one truth for both legs: torch.stft in float64 on the rows the batch call delivered (eight entries are enough to say)
        rows64 = state["rows"].view(n * Cn, J)[:8 * Cn].double()
        truth = of(torch.stft(rows64, n_fft, hop_length=hop, window=torch.hann_window(n_fft, periodic=True, device="cuda:0", dtype=torch.float64), center=True,
                              pad_mode="reflect", return_complex=True)).view(8, Cn, n_fft // 2 + 1, -1)
        wide = torch.complex128 if output == "complex" else torch.float64
        print("%s:\n    rows of %d samples, a tensor of %.1f MB, largest difference of the two tensors %.3g; against the float64 chain: torch %.3g, "
              "decode_ranges_stft %.3g (largest |X| %.3g)" % (
                  what, J, out[1].numel() * out[1].element_size() / 1e6, float((out[0] - out[1]).abs().max()), float((out[0][:8].to(wide) - truth).abs().max()),
                  float((out[1][:8].to(wide) - truth).abs().max()), float(truth.abs().max())), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_ranges_batch + torch.stft %s; decode_ranges_stft %s" % (run, describe(walls[0]), describe(walls[1])), flush=True)
        for d in ds:
            d.close()


def stft_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n, rate = 128, 44100  # (64 stereo windows: a channel is a row)
    for n_fft, hop, output in ((4096, 1024, "complex"), (1024, 256, "magnitude"), (2048, 512, "power")):
        for samples in (rate, 30 * rate):
            src = (torch.rand(n * (samples + 3), device="cuda:0") * 2 - 1)
            rows = [(k * (samples + 3) + 1, samples, k) for k in range(n)]
            for name, bins_first in (("bins first", True), ("frames first", False)):
                spec = capi.StftSpec.make(n_fft=n_fft, hop=hop, output=output, bins_first=bins_first)
                T = spec.n_frames(samples)
                dst = torch.empty((n,) + spec.row_shape(samples), dtype=torch.float32, device="cuda:0")
                for run in (1, 2):
                    times = []
                    for _ in range(6):
                        ctx.timer_start()
                        assert capi.pcm_stft(ctx, src, rows, dst, spec, samples) == capi.OK, ctx.last_error()
                        times.append(ctx.timer_stop())
                    ms = statistics.median(times[1:])
                    print("vpz_pcm_stft %d/%d %-9s %-12s 128 rows of %7d samples (T = %4d) run %d: median of 5 %.1f us (min %.1f, max %.1f); stores %.1f MB = %.0f GB/s"
                          % (n_fft, hop, output, name, samples, T, run, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3, dst.numel() * 4 / 1e6,
                             dst.numel() * 4 / ms / 1e6), flush=True)
                del dst
            if n_fft >= 2048:  # the mel stage on the same rows: the same transforms, a 128-band tile stored in the spectrogram's place
                mel = capi.LogMelSpec.make(sample_rate=rate, n_fft=n_fft, hop=hop, n_mels=128)
                T = mel.n_frames(samples)
                dst = torch.empty((n, 128, T), dtype=torch.float32, device="cuda:0")
                times = []
                for _ in range(6):
                    ctx.timer_start()
                    assert capi.pcm_melspec(ctx, src, rows, dst, mel, samples) == capi.OK, ctx.last_error()
                    times.append(ctx.timer_stop())
                print("vpz_pcm_melspec %d/%d/128 on the same 128 rows of %7d samples: median of 5 %.1f us (min %.1f, max %.1f)" % (
                    n_fft, hop, samples, statistics.median(times[1:]) * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3), flush=True)
                del dst
    ctx.close()


def cqt_job(samples, rate):
    import math, time
    from vorbispizza_amd import capi
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    n, out = len(datas), [None, None]
    spec = capi.CqtSpec.make(sample_rate=rate)
    freqs, lengths = capi.cqt_bins(spec)
    n0, nb, hop = int(lengths[0]), spec.n_bins, spec.hop
    fs = 44100  # (both fixtures, stereo)
    J = -(-samples * (rate // math.gcd(fs, rate)) // (fs // math.gcd(fs, rate)))
    assert J >= n0 // 2 + 1, "windows shorter than the reflection of the lowest bin"
    T = spec.n_frames(J)
    # the dense bank a loader builds: every kernel centre-aligned in N_0, zeros elsewhere (Re rows, then Im rows)
    dense = np.zeros((2 * nb, 1, n0), dtype=np.float32)
    for k in range(nb):
        hr, hi = capi.cqt_kernel(spec, k)
        at = n0 // 2 - hr.size // 2
        dense[k, 0, at: at + hr.size], dense[nb + k, 0, at: at + hr.size] = hr, hi
    bank = torch.from_numpy(dense).to("cuda:0")
    print("the dense bank: %d x %d = %d coefficients, %d of them live (%.1f %% zeros)" % (2 * nb, n0, 2 * nb * n0, 2 * int(lengths.sum()),
                                                                                        100.0 * (1 - lengths.sum() / (nb * n0))), flush=True)
    state = {}

    def by_batch_and_torch(d):
        t0 = time.perf_counter()
        _, whole, res, st = d.decode_ranges_batch(datas, windows, 1, J, planar=True, s16=False, sample_rate=rate, mono=True)
        x = torch.nn.functional.pad(whole.view(n, 1, J), (n0 // 2, n0 // 2), mode="reflect")
        x = torch.nn.functional.pad(x, (0, 1))  # (beyond the reflection x is zero: an odd N_0 reads one such sample when hop divides J)
        y = torch.nn.functional.conv1d(x, bank, stride=hop)[:, :, :T]
        out[0] = torch.sqrt(y[:, :nb] ** 2 + y[:, nb:] ** 2).view(n, 1, nb, T)
        torch.cuda.synchronize()
        state["rows"] = whole
        return time.perf_counter() - t0, res, st

    def by_cqt(d):
        t0 = time.perf_counter()
        _, out[1], res, st = d.decode_ranges_cqt(datas, windows, J, sample_rate=rate)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples to %d Hz, cqt %d bins, hop %d, magnitude" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples, rate, nb, hop)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_batch_and_torch(ds[0]), lambda: by_cqt(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders, device arrays and tables are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all() and (res["samples"] == J).all()
        assert out[0].shape == out[1].shape and out[0].dtype == out[1].dtype
        # one truth for both legs: the same convolution in float64 on the rows the batch call delivered (four entries are enough to say)
        x64 = torch.nn.functional.pad(torch.nn.functional.pad(state["rows"].view(n, 1, J)[:4].double(), (n0 // 2, n0 // 2), mode="reflect"), (0, 1))
        wide = torch.from_numpy(np.stack([np.concatenate(capi_cqt_kernel64(spec, k, n0)) for k in range(nb)])).to("cuda:0")
        y64 = torch.nn.functional.conv1d(x64, wide.view(nb, 2, n0).transpose(0, 1).reshape(2 * nb, 1, n0), stride=hop)[:, :, :T]
        truth = torch.sqrt(y64[:, :nb] ** 2 + y64[:, nb:] ** 2).view(4, 1, nb, T)
        print("%s:\n    rows of %d samples, a tensor of %.1f MB, largest difference of the two tensors %.3g; against the float64 chain: torch %.3g, "
              "decode_ranges_cqt %.3g (largest |X| %.3g)" % (
                  what, J, out[1].numel() * out[1].element_size() / 1e6, float((out[0] - out[1]).abs().max()), float((out[0][:4].double() - truth).abs().max()),
                  float((out[1][:4].double() - truth).abs().max()), float(truth.abs().max())), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_ranges_batch(mono) + conv1d + magnitude %s; decode_ranges_cqt %s" % (run, describe(walls[0]), describe(walls[1])), flush=True)
        for d in ds:
            d.close()


def capi_cqt_kernel64(spec, k, n0):
    """bin k's float32 coefficients widened to float64 and centre-aligned in n0: (hr, hi)"""
    from vorbispizza_amd import capi
    hr, hi = capi.cqt_kernel(spec, k)
    a, b = np.zeros(n0), np.zeros(n0)
    at = n0 // 2 - hr.size // 2
    a[at: at + hr.size], b[at: at + hr.size] = hr, hi
    return a, b


def cqt_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n, rate = 64, 22050
    spec = capi.CqtSpec.make()
    freqs, lengths = capi.cqt_bins(spec)
    live = int(lengths.sum())
    padded = sum(32 * ((int(lengths[k0]) + 1) & ~1) for k0 in range(0, spec.n_bins, 32))
    print("the default spec: sum N_k = %d, padded block lengths x 32 columns = %d (%.2f x), dense %d" % (live, padded, padded / live, spec.n_bins * int(lengths[0])), flush=True)
    for samples in (rate, 30 * rate):
        src = (torch.rand(n * (samples + 3), device="cuda:0") * 2 - 1)
        rows = [(k * (samples + 3) + 1, samples, k) for k in range(n)]
        T = spec.n_frames(samples)
        dst = torch.empty((n,) + spec.row_shape(samples), dtype=torch.float32, device="cuda:0")
        for run in (1, 2):
            times = []
            for _ in range(6):
                ctx.timer_start()
                assert capi.pcm_cqt(ctx, src, rows, dst, spec, samples) == capi.OK, ctx.last_error()
                times.append(ctx.timer_stop())
            ms = statistics.median(times[1:])
            # a multiply-add is two operations; Re and Im are two sums
            rate_live, rate_padded = 2 * 2 * n * T * live / ms / 1e9, 2 * 2 * n * T * padded / ms / 1e9
            print("vpz_pcm_cqt 84 bins hop 512 magnitude bins first, 64 rows of %7d samples (T = %4d) run %d: median of 5 %.1f us (min %.1f, max %.1f); "
                  "%.2f TFLOP/s over sum N_k = %.1f %% of 157, %.2f TFLOP/s over the padded blocks = %.1f %%"
                  % (samples, T, run, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3, rate_live, rate_live / 157 * 100, rate_padded, rate_padded / 157 * 100), flush=True)
        del dst
    ctx.close()


def fbank_job(samples, rate):
    import math, time
    from vorbispizza_amd import capi
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    n, out = len(datas), [None, None]
    spec = capi.FbankSpec.make(sample_rate=rate)
    first, count, weights = capi.fbank_filterbank(spec)
    Wh, at = np.zeros((spec.n_mels, spec.n_fft // 2 + 1), dtype=np.float32), 0  # (a zero column for the Nyquist bin rfft returns)
    for b in range(spec.n_mels):
        Wh[b, first[b]: first[b] + count[b]] = weights[at: at + count[b]]
        at += count[b]
    W = torch.from_numpy(Wh.T.copy()).to("cuda:0")
    m = torch.arange(spec.win, dtype=torch.float64)
    window = ((0.5 - 0.5 * torch.cos(2 * math.pi * m / (spec.win - 1))) ** 0.85).to(torch.float32).to("cuda:0")
    fs = 44100  # (both fixtures)
    J = -(-samples * (rate // math.gcd(fs, rate)) // (fs // math.gcd(fs, rate)))

    def by_batch_and_torch(d):
        t0 = time.perf_counter()
        _, whole, res, st = d.decode_ranges_batch(datas, windows, 1, J, planar=True, s16=False, sample_rate=rate, mono=True)
        y = whole.view(n, J).unfold(1, spec.win, spec.hop) * spec.scale                            # unfold (and the scale)
        y = y - y.mean(dim=2, keepdim=True)                                                        # mean
        z = y - spec.preemphasis * torch.cat([y[:, :, :1], y[:, :, :-1]], dim=2)                   # pre-emphasis
        z = torch.nn.functional.pad(z * window, (0, spec.n_fft - spec.win))                        # window, pad
        S = torch.fft.rfft(z, dim=2)                                                               # rfft
        out[0] = torch.log(torch.clamp(torch.matmul(S.abs() ** 2, W), min=spec.floor))             # power, matmul, log
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res, st

    def by_fbank(d):
        t0 = time.perf_counter()
        _, out[1], res, st = d.decode_ranges_fbank(datas, windows, J, sample_rate=rate)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples to %d Hz, fbank 400/160/512/80" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples, rate)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_batch_and_torch(ds[0]), lambda: by_fbank(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders, device arrays and tables are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all() and (res["samples"] == J).all()
        assert out[0].shape == out[1].shape
        T = out[1].shape[1]
        print("%s:\n    rows of %d samples, a tensor of %.1f MB (the framed batch it replaces: %.1f MB, the complex spectrogram: %.1f MB), largest difference of "
              "the two tensors %.3g (natural-log units)" % (what, J, out[1].numel() * 4 / 1e6, n * T * spec.n_fft * 4 / 1e6, n * (spec.n_fft // 2 + 1) * T * 8 / 1e6,
                                                            float((out[0] - out[1]).abs().max())), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_ranges_batch(mono) + the eight torch ops %s; decode_ranges_fbank %s" % (run, describe(walls[0]), describe(walls[1])),
                  flush=True)
        for d in ds:
            d.close()


def fbank_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n = 64
    for samples in (16000, 480000):
        src = (torch.rand(n * (samples + 3), device="cuda:0") * 2 - 1)
        rows = [(k * (samples + 3) + 1, samples, k) for k in range(n)]
        for name, frames_first in (("frames first", True), ("bands first", False)):
            spec = capi.FbankSpec.make(frames_first=frames_first)
            T = spec.n_frames(samples)
            dst = torch.empty((n, T, 80) if frames_first else (n, 80, T), dtype=torch.float32, device="cuda:0")
            times = []
            for _ in range(11):
                ctx.timer_start()
                assert capi.pcm_fbank(ctx, src, rows, dst, spec, samples) == capi.OK, ctx.last_error()
                times.append(ctx.timer_stop())
            ms = statistics.median(times[1:])
            flop = 2.0 * n * T * 400 * 512
            print("vpz_pcm_fbank %-12s 64 windows of %6d samples (T = %4d): median %.1f us (min %.1f, max %.1f); %.2f GFLOP of the folded product = %.1f TFLOP/s; "
                  "%.1f MB out, %.1f MB of framed batch and %.1f MB of spectrogram not written" % (
                      name, samples, T, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3, flop / 1e9, flop / ms / 1e9, dst.numel() * 4 / 1e6,
                      n * T * 512 * 4 / 1e6, n * 257 * T * 8 / 1e6), flush=True)
    ctx.close()


def mfcc_job(samples, rate):
    import math, time
    from vorbispizza_amd import capi
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    n, out = len(datas), [None, None]
    spec = capi.MfccSpec.make(sample_rate=rate, subtract_mean=True)
    fb = spec.fbank
    Ct = torch.from_numpy(capi.mfcc_table(spec).T.copy()).to("cuda:0")  # [23][13]
    fs = 44100  # (both fixtures)
    J = -(-samples * (rate // math.gcd(fs, rate)) // (fs // math.gcd(fs, rate)))

    def by_fbank_batch_and_torch(d):
        t0 = time.perf_counter()
        _, E, res, st = d.decode_ranges_fbank(datas, windows, J, sample_rate=rate, n_mels=fb.n_mels)
        _, whole, res2, _ = d.decode_ranges_batch(datas, windows, 1, J, planar=True, s16=False, sample_rate=rate, mono=True)  # (the second decode)
        y = whole.view(n, J).unfold(1, fb.win, fb.hop) * fb.scale                                  # unfold (and the scale)
        y = y - y.mean(dim=2, keepdim=True)                                                        # mean
        e = torch.log(torch.clamp((y * y).sum(dim=2), min=2.0 ** -23))                             # square-sum (and the log)
        c = torch.matmul(E, Ct)                                                                    # matmul with the DCT, the lifter in it
        c[:, :, 0] = e                                                                             # column overwrite
        out[0] = c - c.mean(dim=1, keepdim=True)                                                   # mean over frames, subtraction
        torch.cuda.synchronize()
        assert (res2["status"] == 0).all()
        return time.perf_counter() - t0, res, st

    def by_mfcc(d):
        t0 = time.perf_counter()
        _, out[1], res, st = d.decode_ranges_mfcc(datas, windows, J, sample_rate=rate, subtract_mean=True)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples to %d Hz, mfcc 400/160/512/23/13 with the mean" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples, rate)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_fbank_batch_and_torch(ds[0]), lambda: by_mfcc(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders, device arrays and tables are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all() and (res["samples"] == J).all()
        assert out[0].shape == out[1].shape
        print("%s:\n    rows of %d samples, a tensor of %.1f MB (the framed batch it replaces: %.1f MB), largest difference of the two tensors %.3g" % (
            what, J, out[1].numel() * 4 / 1e6, n * out[1].shape[1] * fb.win * 4 / 1e6, float((out[0] - out[1]).abs().max())), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_ranges_fbank + decode_ranges_batch(mono) + the torch chain %s; decode_ranges_mfcc %s" % (
                run, describe(walls[0]), describe(walls[1])), flush=True)
        for d in ds:
            d.close()


def mfcc_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n = 64
    for samples in (16000, 480000):
        src = (torch.rand(n * (samples + 3), device="cuda:0") * 2 - 1)
        rows = [(k * (samples + 3) + 1, samples, k) for k in range(n)]
        fspec = capi.FbankSpec.make(n_mels=23)
        T = fspec.n_frames(samples)
        calls = [("vpz_pcm_fbank, 23 bands", lambda dst: capi.pcm_fbank(ctx, src, rows, dst, fspec, samples), 23)]
        for name, mean in (("vpz_pcm_mfcc 23 / 13", False), ("vpz_pcm_mfcc 23 / 13 with the mean", True)):
            mspec = capi.MfccSpec.make(subtract_mean=mean)
            calls.append((name, lambda dst, mspec=mspec: capi.pcm_mfcc(ctx, src, rows, dst, mspec, samples), 13))
        for name, call, width in calls:
            dst = torch.empty((n, T, width), dtype=torch.float32, device="cuda:0")
            times = []
            for _ in range(11):
                ctx.timer_start()
                assert call(dst) == capi.OK, ctx.last_error()
                times.append(ctx.timer_stop())
            print("%-36s 64 windows of %6d samples (T = %4d): median %.1f us (min %.1f, max %.1f)" % (
                name, samples, T, statistics.median(times[1:]) * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3), flush=True)
    ctx.close()


POST = dict(norm="sliding", cmn_window=300, min_window=100, center=True, delta_order=2, delta_window=2, deltas_first=True)


def post_job(samples, rate):
    import math, time
    from vorbispizza_amd import capi
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    import featpost_truth as pt
    n, out, kept = len(datas), [None, None], {}
    spec = capi.MfccSpec.make(sample_rate=rate)
    post = capi.FeatPostSpec.make(**POST)
    W, w, order = post.cmn_window, post.delta_window, post.delta_order
    kernels = [torch.from_numpy(capi.feat_delta_scales(post, i).copy()).to("cuda:0") for i in range(1, order + 1)]
    fs = 44100  # (both fixtures)
    J = -(-samples * (rate // math.gcd(fs, rate)) // (fs // math.gcd(fs, rate)))

    def by_mfcc_and_torch(d):
        t0 = time.perf_counter()
        _, E, res, st = d.decode_ranges_mfcc(datas, windows, J, sample_rate=rate)
        T, D = E.shape[1], E.shape[2]
        nf = torch.from_numpy(np.array([spec.n_frames(int(x)) for x in res["samples"]], dtype=np.int64)).to("cuda:0")
        t = torch.arange(T, device="cuda:0")
        mask = (t[None, :] < nf[:, None])[:, :, None]                                              # mask
        x = (E * mask).transpose(1, 2).reshape(n * D, 1, T)
        blocks = [x]
        for i, k in enumerate(kernels, 1):                                                         # replicate pad, conv1d: per order
            blocks.append(torch.nn.functional.conv1d(torch.nn.functional.pad(x, (i * w, i * w), mode="replicate"), k.view(1, 1, -1)))
        y = torch.cat([b.view(n, D, T) for b in blocks], dim=1).transpose(1, 2)                    # [n][T][39]
        cs = torch.nn.functional.pad(torch.cumsum(y.double(), dim=1), (0, 0, 1, 0))                # cumsum (float64), a zero in front
        a = (t - W // 2)[None, :].expand(n, T)                                                     # the window's ends per row, edge rules
        b = a + W
        b = torch.where(a < 0, b - a, b)
        a = a.clamp(min=0)
        over = (b - nf[:, None]).clamp(min=0)
        a, b = (a - over).clamp(min=0), torch.minimum(b, nf[:, None]).clamp(min=1)
        S1 = cs.gather(1, b[:, :, None].expand(n, T, y.shape[2])) - cs.gather(1, a[:, :, None].expand(n, T, y.shape[2]))   # two gathers
        out[0] = ((y - S1 / (b - a).clamp(min=1)[:, :, None]) * mask).float()                      # mean, subtraction, mask
        kept["E"], kept["y"], kept["nf"] = E, y, nf
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res, st

    def by_post(d):
        t0 = time.perf_counter()
        _, out[1], res, st = d.decode_ranges_mfcc_post(datas, windows, J, post=post, sample_rate=rate)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples to %d Hz, mfcc 400/160/512/23/13, deltas 2 / 2, sliding mean 300 centred" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples, rate)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_mfcc_and_torch(ds[0]), lambda: by_post(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders, device arrays and tables are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all() and (res["samples"] == J).all()
        assert out[0].shape == out[1].shape
        # leg 1 held to the truth (tests/featpost_truth.py) on a sample of its rows, as the composition is defined: its float32 deltas
        # against the truth of the MFCC frames, its normalised values against the truth of ITS OWN float32 deltas
        worst = [0.0, 0.0]
        for k in sorted({0, 1, n // 3, n // 2, n - 2, n - 1}):
            f = int(kept["nf"][k])
            E_k, y_k, o_k = (t[k, :f].cpu().numpy() for t in (kept["E"], kept["y"], out[0]))
            want, bound = pt.deltas(E_k, pt.spec_of(delta_order=order, delta_window=w))
            worst[0] = max(worst[0], pt.ratio(y_k, want, bound))
            want, bound = pt.normalise(np.ascontiguousarray(y_k), pt.spec_of(norm="sliding", cmn_window=W, min_window=post.min_window, center=True))
            worst[1] = max(worst[1], pt.ratio(o_k, want, bound))
        print("%s:\n    rows of %d samples, a tensor of %.1f MB, largest difference of the two tensors %.3g (largest value %.3g); the torch chain against the "
              "truth's bound on 6 rows: largest error / bound %.3f for its deltas, %.3f for its normalised values" % (
                  what, J, out[1].numel() * 4 / 1e6, float((out[0] - out[1]).abs().max()), float(out[1].abs().max()), worst[0], worst[1]), flush=True)
        assert max(worst) <= 1.0, "the torch chain leaves the truth's bound: it does not compute what the call computes"
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_ranges_mfcc + the torch chain %s; decode_ranges_mfcc_post %s" % (run, describe(walls[0]), describe(walls[1])), flush=True)
        for d in ds:
            d.close()


def post_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n, D = 64, 13
    for samples in (16000, 480000):
        pcm = (torch.rand(n * (samples + 3), device="cuda:0") * 2 - 1)
        prows = [(k * (samples + 3) + 1, samples, k) for k in range(n)]
        mspec = capi.MfccSpec.make()
        T = mspec.n_frames(samples)
        src = torch.empty((n, T, D), dtype=torch.float32, device="cuda:0")
        rows = [(k, T, k) for k in range(n)]
        calls = [("vpz_pcm_mfcc 23 / 13", lambda dst: capi.pcm_mfcc(ctx, pcm, prows, dst, mspec, samples), D, None)]
        for name, kw in (("deltas 2 / 2, then sliding mean 300", POST), ("deltas 2 / 2 alone", dict(delta_order=2)),
                         ("sliding mean 300 alone", dict(norm="sliding", cmn_window=300, min_window=100, center=True)),
                         ("sliding mean 300, then deltas 2 / 2", dict(POST, deltas_first=False)),
                         ("row mean and variance, then deltas", dict(norm="row", norm_vars=True, delta_order=2))):
            ps = capi.FeatPostSpec.make(**kw)
            scratch = torch.empty(max(capi.feat_post_scratch(ps, n, T, D), 1), dtype=torch.float64, device="cuda:0")
            calls.append(("vpz_feat_post " + name, lambda dst, ps=ps, scratch=scratch: capi.feat_post(ctx, src, rows, dst, ps, scratch=scratch),
                          ps.out_columns(D), ps))
        for name, call, width, ps in calls:
            dst = src if ps is None else torch.empty((n, T, width), dtype=torch.float32, device="cuda:0")
            times = []
            for _ in range(11):
                ctx.timer_start()
                assert call(dst) == capi.OK, ctx.last_error()
                times.append(ctx.timer_stop())
            ms = statistics.median(times[1:])
            moved = "" if ps is None else "; %.1f MB read + %.1f MB written = %.2f TB/s" % (
                src.numel() * 4 / 1e6, dst.numel() * 4 / 1e6, (src.numel() + dst.numel()) * 4 / ms / 1e9)
            print("%-52s 64 rows of %6d samples (T = %4d): median %.1f us (min %.1f, max %.1f)%s" % (
                name, samples, T, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3, moved), flush=True)
    ctx.close()


def loudness_job():
    import time
    n = len(datas)
    pcm = torch.empty(int((caps * 2).sum()), dtype=torch.float32, pin_memory=True).numpy()
    rec = [None]

    def by_library(d):
        t0 = time.perf_counter()
        res, st = d.decode_library(datas, pcm, offs, caps, s16=False)
        return time.perf_counter() - t0, res, st

    def by_loudness(d):
        t0 = time.perf_counter()
        res, integrated, peak, steps, kept, st = d.measure_loudness(datas)
        rec[0] = (integrated, peak, steps, kept)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d whole streams" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_library(ds[0]), lambda: by_loudness(ds[1])]
        samples = []
        for leg in legs:  # (one pass each that does not count: slots, decoders and device arrays are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all()
            samples.append(res["samples"].copy())
        assert np.array_equal(samples[0], samples[1]), "the samples measured are not the samples decoded"
        integrated, peak, steps, kept = rec[0]
        assert np.isfinite(integrated).all() and (integrated[2:] == integrated[pick[2:]]).all() and (peak[2:] == peak[pick[2:]]).all()
        print("%s:\n    %.1f MB of float32 PCM stay on the device, %.1f kB of step sums and peaks come down; the two fixtures: %.2f LUFS (peak %.4f, %d steps, "
              "%d blocks kept) and %.2f LUFS (peak %.4f, %d steps, %d blocks kept)" % (
                  what, int(samples[1].sum()) * 2 * 4 / 1e6, (int(steps.sum()) * 8 + n * 4) / 1e3, integrated[0], peak[0], steps[0], kept[0], integrated[1],
                  peak[1], steps[1], kept[1]), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_library into float32 host memory %s; measure_loudness %s" % (run, describe(walls[0]), describe(walls[1])), flush=True)
        for d in ds:
            d.close()


def loudness_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n, fs = 64, 44100
    for samples in (44100, 200 * 44100):
        src = (torch.rand(n * (samples + 3) * 2, device="cuda:0") * 2 - 1)
        rows = [((k * (samples + 3) + 1) * 2, samples, k) for k in range(n)]
        steps = samples // capi.loudness_step(fs)
        out = (torch.empty((n, steps), dtype=torch.float64, device="cuda:0"), torch.empty((n,), dtype=torch.float32, device="cuda:0"))
        times = []
        for _ in range(11):
            ctx.timer_start()
            capi.pcm_loudness(ctx, src, 2, fs, rows, max_steps=steps, out=out)
            times.append(ctx.timer_stop())
        ms = statistics.median(times[1:])
        read = 2.0 * n * samples * 2 * 4  # (the two passes read every sample once each)
        print("vpz_pcm_loudness 64 stereo rows of %8d samples (%4d steps): median %.1f us (min %.1f, max %.1f); %.1f MB read twice = %.0f GB/s; %.1f kB out" % (
            samples, steps, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3, read / 2e6, read / ms / 1e6, (out[0].numel() * 8 + n * 4) / 1e3), flush=True)
    ctx.close()


def normalize_job(samples, rate, mode):
    """--normalize MODE: normalize.decode_ranges_normalized against what a loader does without it"""
    import time
    import normalize_truth as nt
    from vorbispizza_amd import normalize
    totals = [smp for _, smp in bench.REAL_FIXTURES]
    rng = np.random.default_rng(7)
    windows = [(int(rng.integers(0, totals[i] - samples - 64)), samples) for i in pick]
    n, C_, out, kept = len(datas), 1 if args.mono else 2, [None, None], {}
    target = normalize.DEFAULT_TARGETS[mode]
    J = -(-samples * rate // 44100)  # (the set's streams are at 44 100 Hz)

    def by_batch_and_torch(d):
        t0 = time.perf_counter()
        gain = None
        if mode == "loudness":  # measure first: the second decode that the call saves
            _, integrated, _, _, _, _ = d.measure_loudness(datas, windows)
            g = np.where(np.isfinite(integrated), 10.0 ** ((target - np.where(np.isfinite(integrated), integrated, target)) / 20.0), 1.0)
            gain = torch.from_numpy(g.astype(np.float32)).to("cuda:0")
            kept["loudness"] = integrated
        _, x, res, st = d.decode_ranges_batch(datas, windows, C_, J, planar=True, s16=False, sample_rate=rate, mono=args.mono)
        count = torch.from_numpy(res["samples"].astype(np.int64)).to("cuda:0")
        mask = (torch.arange(J, device="cuda:0")[None, :] < count[:, None])[:, None, :].to(torch.float32)
        N = (count * C_).clamp(min=1).to(torch.float32)[:, None, None]
        if mode == "meanvar":
            mean = (x * mask).sum(dim=(1, 2), keepdim=True) / N
            var = (((x - mean) * mask) ** 2).sum(dim=(1, 2), keepdim=True) / N
            y = (x - mean) / torch.sqrt(var + 1e-7) * mask
        elif mode == "peak":
            y = x * (target / (x * mask).abs().amax(dim=(1, 2), keepdim=True).clamp(min=1e-30)) * mask
        elif mode == "rms":
            y = x * (target / torch.sqrt(((x * mask) ** 2).sum(dim=(1, 2), keepdim=True) / N).clamp(min=1e-30)) * mask
        else:
            y = x * gain[:, None, None] * mask
        out[0] = y
        kept["x"], kept["count"] = x, res["samples"]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res, st

    def by_normalized(d):
        t0 = time.perf_counter()
        _, out[1], res, st = normalize.decode_ranges_normalized(d, datas, windows, C_, J, rate, mono=args.mono, mode=mode)
        kept["results"] = res
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "f32 groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d streams, windows of %d samples to %d Hz%s, %s" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n, samples, rate, ", mono" if args.mono else "", mode)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(2)]
        legs = [lambda: by_batch_and_torch(ds[0]), lambda: by_normalized(ds[1])]
        for leg in legs:  # (one pass each that does not count: slots, decoders, device arrays and tables are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all()
        # both legs against the same truth (tests/normalize_truth.py: longdouble, two passes, the header's bound), on the first rows
        rows = slice(0, 16)
        x = kept["x"][rows].cpu().numpy()
        res = kept["results"]
        assert (kept["count"] == J).all() and np.array_equal(res["samples"], kept["count"])
        if mode == "loudness":
            assert np.array_equal(res["loudness"].view(np.uint64), kept["loudness"].view(np.uint64)), "the loudness is not measure_loudness's"
            kw = dict(mode=nt.GAIN, gains=res["gain"][rows])
        else:
            kw = dict(mode=nt.MODES[mode], target=target)
        ystar, bound, _ = nt.truth(x, **kw)
        ratios = [nt.worst_ratio(out[i][rows].cpu().numpy(), ystar, bound) for i in (0, 1)]
        print("%s:\n    a tensor of %.1f MB; error / derived bound on the first 16 rows: torch chain %.3g, the call %.3g; largest difference of the two tensors "
              "%.3g (largest value %.3g), %d streams on the device" % (
                  what, out[1].numel() * 4 / 1e6, ratios[0], ratios[1], float((out[0] - out[1]).abs().max()), float(out[1].abs().max()),
                  int(sum(st.device_gpu_entropy_streams))), flush=True)
        for run in (1, 2):
            walls = [[], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: %sdecode_ranges_batch + torch chain %s; decode_ranges_normalized %s" % (
                run, "measure_loudness + " if mode == "loudness" else "", describe(walls[0]), describe(walls[1])), flush=True)
        for d in ds:
            d.close()


def normalize_kernel_job():
    """--normalize-kernel: vpz_pcm_normalize alone, 64 mono rows of one second and of thirty at 16 000 Hz, the context's event timer"""
    import ctypes as C
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n = 64
    for samples in (16000, 30 * 16000):
        src = (torch.rand(n * samples + 8, device="cuda:0") * 2 - 1)
        desc = (capi.NormRow * n)()
        for k in range(n):
            desc[k].src, desc[k].samples, desc[k].row, desc[k].gain = k * samples + 1, samples, k, 0.5  # (odd offsets: unaligned sources)
        scratch = torch.empty(capi.pcm_normalize_scratch(n, 1, samples), dtype=torch.float64, device="cuda:0")
        for name, mode, lay, dtype in (("meanvar f32", "meanvar", capi.OUT_PLANAR, torch.float32), ("meanvar s16", "meanvar", capi.OUT_PLANAR_S16, torch.int16),
                                       ("peak f32", "peak", capi.OUT_PLANAR, torch.float32), ("plain gain f32", "gain", capi.OUT_PLANAR, torch.float32)):
            dst = torch.empty((n, 1, samples), dtype=dtype, device="cuda:0")
            spec = capi.NormSpec.make(mode, channels=1)
            times = []
            for _ in range(11):
                ctx.timer_start()
                rc = capi.lib().vpz_pcm_normalize(ctx._h, C.c_void_p(src.data_ptr()), src.numel(), samples, C.byref(spec), n, C.cast(desc, C.c_void_p),
                                                  C.c_void_p(dst.data_ptr()), n, lay, C.c_void_p(scratch.data_ptr()), scratch.numel(), None)
                assert rc == capi.OK, ctx.last_error()
                times.append(ctx.timer_stop())
            passes = 1 if mode == "gain" else 2  # (a plain gain reads its rows once)
            moved = n * samples * (4 * passes + dst.element_size())
            ms = statistics.median(times[1:])
            print("vpz_pcm_normalize %-14s 64 mono rows of %6d samples: median %.1f us (min %.1f, max %.1f) for %.2f MB moved (read %s, written once) = %.0f GB/s, "
                  "%.1f %% of 8 TB/s" % (name, samples, ms * 1e3, min(times[1:]) * 1e3, max(times[1:]) * 1e3, moved / 1e6, "twice" if passes == 2 else "once",
                                        moved / ms / 1e6, 100.0 * moved / ms / 1e6 / 8000.0), flush=True)
    ctx.close()


def r128_job():
    import time
    n = len(datas)
    pcm = torch.empty(int((caps * 2).sum()), dtype=torch.float32, pin_memory=True).numpy()
    rec = [None, None]

    def by_library(d):
        t0 = time.perf_counter()
        res, st = d.decode_library(datas, pcm, offs, caps, s16=False)
        return time.perf_counter() - t0, res, st

    def by_loudness(d):
        t0 = time.perf_counter()
        res, integrated, peak, steps, kept, st = d.measure_loudness(datas)
        rec[0] = (integrated, peak, steps, kept)
        return time.perf_counter() - t0, res, st

    def by_r128(d):
        t0 = time.perf_counter()
        res, rec[1], st = d.measure_r128(datas)
        return time.perf_counter() - t0, res, st

    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "groups %d threads %3d streams/call %2d contexts %d slots %d gpu_entropy %s, %d whole streams" % (
            groups, thr, spc, ctxs, slots, "on" if args.gpu_entropy else "off", n)
        ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                               gpu_entropy=args.gpu_entropy) for _ in range(3)]
        legs = [lambda: by_library(ds[0]), lambda: by_loudness(ds[1]), lambda: by_r128(ds[2])]
        samples = []
        for leg in legs:  # (one pass each that does not count: slots, decoders and device arrays are allocated in it)
            _, res, st = leg()
            assert (res["status"] == 0).all()
            samples.append(res["samples"].copy())
        assert np.array_equal(samples[0], samples[1]) and np.array_equal(samples[0], samples[2]), "the samples measured are not the samples decoded"
        (integrated, peak, steps, kept), r = rec
        assert integrated.tobytes() == r["integrated"].tobytes() and peak.tobytes() == r["sample_peak"].tobytes(), "measure_r128 is not measure_loudness's bits"
        assert np.array_equal(steps, r["steps"]) and np.array_equal(kept, r["blocks_kept"]) and (r["true_peak"] >= r["sample_peak"]).all()
        assert r[2:].tobytes() == r[pick[2:]].tobytes()
        print("%s:\n    %.1f MB of float32 PCM stay on the device, %.1f kB of step sums and peaks come down" % (
            what, int(samples[2].sum()) * 2 * 4 / 1e6, (int(r["steps"].sum()) * 8 + n * 8) / 1e3), flush=True)
        for k in (0, 1):
            print("    fixture %d: %.2f LUFS, range %.2f LU (%.2f .. %.2f, %d blocks), momentary max %.2f, short-term max %.2f, true peak %.4f (%.2f dBTP), "
                  "sample peak %.4f" % (k, r["integrated"][k], r["range"][k], r["range_low"][k], r["range_high"][k], r["range_blocks"][k], r["momentary_max"][k],
                                        r["short_term_max"][k], r["true_peak"][k], 20 * np.log10(r["true_peak"][k]), r["sample_peak"][k]), flush=True)
        for run in (1, 2):
            walls = [[], [], []]
            for _ in range(args.reps or 5):
                for i, leg in enumerate(legs):
                    walls[i].append(leg()[0])
            print("    A/B run %d: decode_library into float32 host memory %s; measure_loudness %s; measure_r128 %s" % (
                run, describe(walls[0]), describe(walls[1]), describe(walls[2])), flush=True)
        for d in ds:
            d.close()


def r128_kernel_job():
    from vorbispizza_amd import Context, capi
    ctx = Context(0)
    n, fs = 64, 44100
    for samples in (44100, 200 * 44100):
        src = (torch.rand(n * (samples + 3) * 2, device="cuda:0") * 2 - 1)
        rows = [((k * (samples + 3) + 1) * 2, samples, k) for k in range(n)]
        steps = samples // capi.loudness_step(fs)
        loud = (torch.empty((n, steps), dtype=torch.float64, device="cuda:0"), torch.empty((n,), dtype=torch.float32, device="cuda:0"))
        peaks = (torch.empty((n,), dtype=torch.float32, device="cuda:0"), torch.empty((n,), dtype=torch.float32, device="cuda:0"))
        calls = {"vpz_pcm_true_peak": lambda: capi.pcm_true_peak(ctx, src, 2, fs, rows, out=peaks),
                 "vpz_pcm_loudness": lambda: capi.pcm_loudness(ctx, src, 2, fs, rows, max_steps=steps, out=loud)}
        times = {name: [] for name in calls}
        for _ in range(6):  # (the first of each does not count; the two take turns)
            for name, call in calls.items():
                ctx.timer_start()
                call()
                times[name].append(ctx.timer_stop())
        read = n * samples * 2 * 4.0
        fma = n * (samples + 11) * 2 * 36.0
        ms = statistics.median(times["vpz_pcm_true_peak"][1:])
        print("vpz_pcm_true_peak 64 stereo rows of %8d samples: median of 5 %.1f us (min %.1f, max %.1f); %.1f MB read once = %.0f GB/s (%.1f %% of 8 TB/s); "
              "%.2f G multiply-adds = %.2f T/s (%.1f %% of the float32 vector peak)" % (
                  samples, ms * 1e3, min(times["vpz_pcm_true_peak"][1:]) * 1e3, max(times["vpz_pcm_true_peak"][1:]) * 1e3, read / 1e6, read / ms / 1e6,
                  read / ms / 1e6 / 8000 * 100, fma / 1e9, fma / ms / 1e9, 2 * fma / ms / 1e9 / 157.3 * 100), flush=True)
        ms = statistics.median(times["vpz_pcm_loudness"][1:])
        print("vpz_pcm_loudness  64 stereo rows of %8d samples: median of 5 %.1f us (min %.1f, max %.1f); %.1f MB read twice = %.0f GB/s" % (
            samples, ms * 1e3, min(times["vpz_pcm_loudness"][1:]) * 1e3, max(times["vpz_pcm_loudness"][1:]) * 1e3, read / 1e6, 2 * read / ms / 1e6), flush=True)
    ctx.close()


if args.normalize_kernel:
    normalize_kernel_job()
    sys.exit(0)
if args.ranges and args.batch and args.resample and args.normalize:
    normalize_job(args.ranges, args.resample, args.normalize)
    sys.exit(0)
if args.r128_kernel:
    r128_kernel_job()
    sys.exit(0)
if args.r128:
    r128_job()
    sys.exit(0)
if args.loudness_kernel:
    loudness_kernel_job()
    sys.exit(0)
if args.loudness:
    loudness_job()
    sys.exit(0)
if args.fbank_kernel:
    fbank_kernel_job()
    sys.exit(0)
if args.ranges and args.batch and args.resample and args.fbank:
    fbank_job(args.ranges, args.resample)
    sys.exit(0)
if args.mfcc_kernel:
    mfcc_kernel_job()
    sys.exit(0)
if args.post_kernel:
    post_kernel_job()
    sys.exit(0)
if args.ranges and args.batch and args.resample and args.mfcc and args.post:
    post_job(args.ranges, args.resample)
    sys.exit(0)
if args.ranges and args.batch and args.resample and args.mfcc:
    mfcc_job(args.ranges, args.resample)
    sys.exit(0)
if args.logmel_kernel:
    logmel_kernel_job()
    sys.exit(0)
if args.melspec_kernel:
    melspec_kernel_job()
    sys.exit(0)
if args.ranges and args.batch and args.resample and args.melspec:
    melspec_job(args.ranges, args.resample)
    sys.exit(0)
if args.stft_kernel:
    stft_kernel_job()
    sys.exit(0)
if args.ranges and args.batch and args.resample and args.stft:
    stft_job(args.ranges, args.resample)
    sys.exit(0)
if args.cqt_kernel:
    cqt_kernel_job()
    sys.exit(0)
if args.ranges and args.batch and args.resample and args.cqt:
    cqt_job(args.ranges, args.resample)
    sys.exit(0)
if args.ranges and args.batch and args.resample and args.logmel:
    logmel_job(args.ranges, args.resample)
    sys.exit(0)
if args.pack_kernel:
    pack_kernel_job()
    sys.exit(0)
if args.resample_kernel:
    resample_kernel_job()
    sys.exit(0)
if args.ranges and args.batch and args.resample:
    resample_job(args.ranges, args.resample)
    sys.exit(0)
if args.ranges:
    (batch_job if args.batch else ranges_job)(args.ranges)
    sys.exit(0)

for s16 in ((True,) if args.s16_only else (False, True)):
    pcm = torch.empty(int((caps * 2).sum()), dtype=torch.int16 if s16 else torch.float32, pin_memory=True).numpy()
    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "%s groups %d threads %3d streams/call %2d contexts %d slots %d" % ("s16" if s16 else "f32", groups, thr, spc, ctxs, slots)
        if args.ab:
            ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                                   gpu_entropy=g or args.mixed, **({"mixed_setups": g} if args.mixed else {})) for g in (False, True)]
            walls, sums, lines = ([], []), [None, None], ["", ""]
            for d in ds:  # (one pass each that does not count: slots, decoders and device arrays are allocated in it)
                d.decode_library(datas, pcm, offs, caps, s16=s16)
            for _ in range(args.reps or 5):
                for i, d in enumerate(ds):
                    pcm[:] = 0
                    res, st = d.decode_library(datas, pcm, offs, caps, s16=s16)
                    assert (res["status"] == 0).all()
                    walls[i].append(st.wall_s)
                    sums[i] = (int(pcm.view(np.uint16).astype(np.uint64).sum()), int(res["samples"].sum()), st.pinned_mib,
                               int(sum(st.device_gpu_entropy_streams)), int(sum(st.device_payload_bytes)), st.device_decode_s[0])
            for i, d in enumerate(ds):
                lines[i] = counts_line(d)
                d.close()
            assert sums[0][:2] == sums[1][:2], "the two dispatchers' PCM differs"
            name = "mixed_setups" if args.mixed else "gpu_entropy"
            print("%s:\n    %s off: %s, host decode until %.1f ms, pinned %d MiB%s\n    %s on:  %s, plan until %.1f ms, pinned %d MiB, "
                  "%d streams on the device, %.1f MB of packet bytes%s" % (what, name, describe(walls[0]), sums[0][5] * 1e3, sums[0][2], lines[0], name,
                                                                         describe(walls[1]), sums[1][5] * 1e3, sums[1][2], sums[1][3], sums[1][4] / 1e6,
                                                                         lines[1]), flush=True)
            continue
        d = multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                             gpu_entropy=args.gpu_entropy or args.mixed, **({"mixed_setups": True} if args.mixed else {}))
        best, walls = None, []
        for _ in range(args.reps or 3):
            res, st = d.decode_library(datas, pcm, offs, caps, s16=s16)
            assert (res["status"] == 0).all() or os.environ.get("VPZM_NO_SYNTH")
            walls.append(st.wall_s)
            if best is None or st.wall_s < best[0]:
                best = (st.wall_s, st.device_decode_s[0], st.device_synth_s[0])
        line = counts_line(d)
        d.close()
        tot = int(res["samples"].sum()) * 2
        print("%s%s: %.1f ms = %.2f Gsamples/s (decode until %.1f, synth sum %.1f; %s)%s"
              % (what, " mixed_setups" if args.mixed else " gpu_entropy" if args.gpu_entropy else "", best[0] * 1e3, tot / best[0] / 1e9, best[1] * 1e3,
                 best[2] * 1e3, describe(walls[1:] or walls), line), flush=True)
    del pcm
