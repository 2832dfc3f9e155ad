#!/usr/bin/env python3
"""The 1024-stream job through the in-process dispatcher under several thread / slot / sub-batch settings (one GPU, N groups).

    dispatcher_probe.py [--gpu-entropy | --ab] [--reps N] [--s16-only] groups,threads,streams_per_call,contexts,slots ...

--gpu-entropy: the dispatchers are created with vpzm_options.gpu_entropy (eligible streams entropy-decoded on the device).
--ab: for every setting TWO dispatchers in this process, the option off and on, take the job in turn, --reps times each
(default 5): medians and extremes of both, and the PCM of the two compared."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import bench
from vorbispizza_amd import multi
ap = argparse.ArgumentParser()
ap.add_argument("--gpu-entropy", action="store_true")
ap.add_argument("--ab", action="store_true")
ap.add_argument("--reps", type=int, default=0)
ap.add_argument("--s16-only", action="store_true")
ap.add_argument("settings", nargs="+")
args = ap.parse_args()
streams = int(os.environ.get("STREAMS", "1024"))
raws = [np.frombuffer(open(os.path.join(ROOT, "tests", "golden", n), "rb").read(), dtype=np.uint8) for n, _ in bench.REAL_FIXTURES]
caps1 = [smp + 2048 for _, smp in bench.REAL_FIXTURES]
datas = [raws[i % 2] for i in range(streams)]
caps = np.array([caps1[i % 2] for i in range(streams)], dtype=np.int64)
offs = np.concatenate([[0], np.cumsum(caps * 2)[:-1]]).astype(np.int64)


def describe(walls):
    return "median %.1f ms (min %.1f, max %.1f)" % (statistics.median(walls) * 1e3, min(walls) * 1e3, max(walls) * 1e3)


for s16 in ((True,) if args.s16_only else (False, True)):
    pcm = torch.empty(int((caps * 2).sum()), dtype=torch.int16 if s16 else torch.float32, pin_memory=True).numpy()
    for groups, thr, spc, ctxs, slots in [tuple(int(x) for x in a.split(",")) for a in args.settings]:
        what = "%s groups %d threads %3d streams/call %2d contexts %d slots %d" % ("s16" if s16 else "f32", groups, thr, spc, ctxs, slots)
        if args.ab:
            ds = [multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                                   gpu_entropy=g) for g in (False, True)]
            walls, sums = ([], []), [None, None]
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
            for d in ds:
                d.close()
            assert sums[0][:2] == sums[1][:2], "the two dispatchers' PCM differs"
            print("%s:\n    gpu_entropy off: %s, host decode until %.1f ms, pinned %d MiB\n    gpu_entropy on:  %s, plan until %.1f ms, pinned %d MiB, "
                  "%d streams on the device, %.1f MB of packet bytes" % (what, describe(walls[0]), sums[0][5] * 1e3, sums[0][2], describe(walls[1]),
                                                                           sums[1][5] * 1e3, sums[1][2], sums[1][3], sums[1][4] / 1e6), flush=True)
            continue
        d = multi.Dispatcher([0] * groups, host_threads=thr, streams_per_call=spc, contexts_per_device=ctxs, slots_per_device=slots,
                             gpu_entropy=args.gpu_entropy)
        best, walls = None, []
        for _ in range(args.reps or 3):
            res, st = d.decode_library(datas, pcm, offs, caps, s16=s16)
            assert (res["status"] == 0).all() or os.environ.get("VPZM_NO_SYNTH")
            walls.append(st.wall_s)
            if best is None or st.wall_s < best[0]:
                best = (st.wall_s, st.device_decode_s[0], st.device_synth_s[0])
        d.close()
        tot = int(res["samples"].sum()) * 2
        print("%s%s: %.1f ms = %.2f Gsamples/s (decode until %.1f, synth sum %.1f; %s)"
              % (what, " gpu_entropy" if args.gpu_entropy else "", best[0] * 1e3, tot / best[0] / 1e9, best[1] * 1e3, best[2] * 1e3,
                 describe(walls[1:] or walls)), flush=True)
    del pcm
