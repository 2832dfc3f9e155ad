#!/usr/bin/env python3
"""The GPU entropy decode (vpz_entropy_decode) against the CPU's (vpzh_decode_many), over the bench's real-stream mix:
copies of 3test.ogg and issue6test.ogg (half each), 128 and 1024 streams.  Per size it reports

  * the host time of vpzh_plan_range over the batch (the files already opened: paging and setup headers are the same
    work on either path),
  * the vpz_entropy_decode time from events on the context stream (the residue-zeroing pass and the decode kernel),
    median of `--steps` runs after `--warmup`, and the rate in M samples/s (decoded samples per channel),
  * the payload bytes the device path moves to the GPU against the residue / post bytes the CPU path moves,
  * in the same run, vpzh_decode_many over the same containers on vpzh_default_threads() threads (wall clock),

and checks the device's result against the CPU's for the first stream of each fixture.  One JSON line per size.

  python tools/kbench_entropy.py [--streams 128 1024] [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURES = ("3test.ogg", "issue6test.ogg")


def run(n_streams, steps, warmup, ctx, torch):
    from vorbispizza_amd import capi, front
    from vorbispizza_amd.entropy import EntropySetup
    dev = torch.device("cuda", ctx.device)
    raws = [open(os.path.join(ROOT, "tests", "golden", n), "rb").read() for n in FIXTURES]
    files = [front.OggVorbisFile(raws[s % 2]) for s in range(n_streams)]
    images = [files[0].entropy_setup(), files[1].entropy_setup()]
    setups = [EntropySetup(ctx, img) for img in images]  # the two fixtures have two setups: one batch each

    # ---- plan on the host
    t0 = time.perf_counter()
    plans = [[], []]
    for s, f in enumerate(files):
        plans[s % 2].append(f.plan_packets(stream_id=s))
    t_plan = time.perf_counter() - t0

    batches = []
    for which in range(2):
        pk_all, sp_all, pay_all, res_base, pay_base = [], [], [], 0, 0
        for pk, sp, pay, used in plans[which]:
            pk = pk.copy()
            pk["residue_offset"] += res_base
            sp = sp.copy()
            sp[:, 0] += pay_base
            pk_all.append(pk)
            sp_all.append(sp)
            pay_all.append(pay)
            res_base += used
            pay_base += pay.size
        packets, spans, payload = np.concatenate(pk_all), np.concatenate(sp_all), np.concatenate(pay_all)
        ch = files[which].channels
        batches.append(dict(packets=packets, spans=spans, d_payload=torch.from_numpy(payload).to(dev), payload_bytes=payload.size,
                            residue=torch.empty(res_base, dtype=torch.float32, device=dev), values=res_base,
                            posts=torch.empty((len(packets) * ch, 64), dtype=torch.int16, device=dev),
                            counts=torch.empty(len(packets) * ch, dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()

    def decode_all():
        for which in range(2):
            b = batches[which]
            setups[which].decode(b["packets"], b["spans"], b["d_payload"], b["residue"], b["posts"], b["counts"], mem_space=capi.MEM_DEVICE)

    for _ in range(warmup):
        decode_all()
    ctx.synchronize()
    times = []
    for _ in range(steps):
        ctx.timer_start()
        decode_all()
        times.append(ctx.timer_stop())
    ms = statistics.median(times)

    # ---- check: the first stream of each fixture against the CPU
    for which in range(2):
        f = files[which]
        pk, res, posts, counts = f.decode_packets()
        b = batches[which]
        n = len(pk)
        assert np.array_equal(b["counts"][: n * f.channels].cpu().numpy(), counts)
        assert b["posts"][: n * f.channels].cpu().numpy().tobytes() == posts.tobytes()
        assert b["residue"][: res.size].cpu().numpy().tobytes() == res.tobytes()

    # ---- the CPU path over the same containers
    datas = [np.frombuffer(raws[s % 2], dtype=np.uint8) for s in range(n_streams)]
    n_pk = [f.audio_packets for f in files]
    n_val = [int(f.info.residue_floats) for f in files]
    pbase = np.concatenate([[0], np.cumsum(n_pk)[:-1]]).astype(np.int64)
    rbase = np.concatenate([[0], np.cumsum(n_val)[:-1]]).astype(np.int64)
    packets = capi.make_packets(int(sum(n_pk)))
    residue = np.empty(int(sum(n_val)), dtype=np.float32)
    posts = np.empty((int(sum(n_pk)) * 2, 64), dtype=np.int16)
    counts = np.empty(int(sum(n_pk)) * 2, dtype=np.uint8)
    threads = front.lib().vpzh_default_threads()
    front.decode_many(datas[:2], pbase[:2], rbase[:2], packets, residue, posts, counts, threads=threads)  # (warm the setup cache)
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        front.decode_many(datas, pbase, rbase, packets, residue, posts, counts, threads=threads)
        cpu.append(time.perf_counter() - t0)
    t_cpu = statistics.median(cpu)

    samples = sum(f.total_samples for f in files)
    n_packets = sum(len(b["packets"]) for b in batches)
    payload_bytes = sum(b["payload_bytes"] for b in batches)
    residue_bytes = 4 * sum(b["values"] for b in batches) + n_packets * 2 * (64 * 2 + 1)
    for s in setups:
        s.close()
    for f in files:
        f.close()
    return {
        "streams": n_streams, "packets": n_packets, "samples_per_channel": samples,
        "plan_host_ms": round(t_plan * 1e3, 3),
        "gpu_entropy_decode_ms": round(ms, 3), "gpu_entropy_decode_ms_all": [round(t, 3) for t in times],
        "gpu_msamples_per_s": round(samples / (ms * 1e-3) / 1e6, 1),
        "payload_bytes": payload_bytes, "cpu_path_residue_and_post_bytes": residue_bytes,
        "cpu_decode_many_ms": round(t_cpu * 1e3, 3), "cpu_threads": threads,
        "speedup_vs_cpu": round(t_cpu * 1e3 / ms, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch

    from vorbispizza_amd import Context
    ctx = Context(0)
    for n in args.streams:
        print(json.dumps(run(n, args.steps, args.warmup, ctx, torch)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
