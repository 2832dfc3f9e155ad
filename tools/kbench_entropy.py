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

Group mode (--group K): the same packets two ways, taken in turn in one process -- as ONE vpz_entropy_group_decode launch over
streams drawn round-robin from K stereo 256/2048 setups of the writer (tests/synthetic_streams.py, --group-packets packets each),
and as K vpz_entropy_decode launches, one per setup, back to back on the same stream.  Medians of --steps, one JSON line per size;
the two results are compared byte for byte.

  python tools/kbench_entropy.py [--streams 128 1024] [--steps 5] [--warmup 2] [--group 32 [--group-packets 200]]
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


def run_group(n_streams, n_setups, n_packets, steps, warmup, ctx, torch):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synthetic_streams as ss

    from vorbispizza_amd import capi, front
    from vorbispizza_amd.entropy import EntropyGroup, EntropySetup
    dev = torch.device("cuda", ctx.device)
    files = []
    for k in range(n_setups):
        st, rng = ss.stereo_coupled_res2(2 + 10 * k)
        files.append(front.OggVorbisFile(bytes(st.build(rng, n_packets)[0])))
        assert files[-1].gpu_decode_supported
    images = [f.entropy_setup() for f in files]
    plans = [f.plan_packets() for f in files]
    # the batch: stream s is a copy of setup s % K, residues and payloads back to back
    pk_all, sp_all, pay_all, res_base, pay_base = [], [], [], 0, 0
    for s in range(n_streams):
        pk, sp, pay, used = plans[s % n_setups]
        pk, sp = pk.copy(), sp.copy()
        pk["stream"] = s
        pk["residue_offset"] += res_base
        sp[:, 0] += pay_base
        pk_all.append(pk)
        sp_all.append(sp)
        pay_all.append(pay)
        res_base += used
        pay_base += pay.size
    packets, spans, payload = np.concatenate(pk_all), np.concatenate(sp_all), np.concatenate(pay_all)
    owner = np.repeat(np.arange(n_streams) % n_setups, [len(plans[s % n_setups][0]) for s in range(n_streams)])
    d_payload = torch.from_numpy(payload).to(dev)
    n = len(packets)

    def outputs():
        return (torch.zeros(res_base, dtype=torch.float32, device=dev), torch.zeros((n * 2, 64), dtype=torch.int16, device=dev),
                torch.zeros(n * 2, dtype=torch.uint8, device=dev))

    out_group, out_single = outputs(), outputs()
    group = EntropyGroup(ctx, images)
    singles = [EntropySetup(ctx, img) for img in images]
    stream_setup = (np.arange(n_streams) % n_setups).astype(np.uint8)
    stream_base = np.zeros(n_streams, dtype=np.uint8)
    # per setup: its packets, in batch order; the records of packet k of a per-setup call are k * 2 + c of that call's arrays
    per = []
    for k in range(n_setups):
        at = np.flatnonzero(owner == k)
        per.append(dict(packets=np.ascontiguousarray(packets[at]), spans=np.ascontiguousarray(spans[at]), at=at,
                        posts=torch.zeros((len(at) * 2, 64), dtype=torch.int16, device=dev),
                        counts=torch.zeros(len(at) * 2, dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()

    def as_group():
        group.decode(stream_setup, stream_base, packets, spans, d_payload, *out_group, mem_space=capi.MEM_DEVICE)

    def per_setup():
        for k in range(n_setups):
            singles[k].decode(per[k]["packets"], per[k]["spans"], d_payload, out_single[0], per[k]["posts"], per[k]["counts"],
                              mem_space=capi.MEM_DEVICE)

    for _ in range(warmup):
        as_group()
        per_setup()
    ctx.synchronize()
    t_group, t_single = [], []
    for _ in range(steps):  # (in turn)
        ctx.timer_start()
        as_group()
        t_group.append(ctx.timer_stop())
        ctx.timer_start()
        per_setup()
        t_single.append(ctx.timer_stop())
    # the two ways wrote the same bytes
    assert out_group[0].cpu().numpy().tobytes() == out_single[0].cpu().numpy().tobytes()
    posts, counts = out_group[1].cpu().numpy().reshape(n, 2, 64), out_group[2].cpu().numpy().reshape(n, 2)
    for k in range(n_setups):
        assert posts[per[k]["at"]].tobytes() == per[k]["posts"].cpu().numpy().tobytes()
        assert counts[per[k]["at"]].tobytes() == per[k]["counts"].cpu().numpy().tobytes()
    group.close()
    for x in singles:
        x.close()
    for f in files:
        f.close()
    g, o = statistics.median(t_group), statistics.median(t_single)
    return {"mode": "group", "streams": n_streams, "setups": n_setups, "packets": n, "payload_bytes": int(payload.size),
            "one_group_launch_ms": round(g, 3), "one_group_launch_ms_all": [round(t, 3) for t in t_group],
            "per_setup_launches_ms": round(o, 3), "per_setup_launches_ms_all": [round(t, 3) for t in t_single],
            "per_setup_over_group": round(o / g, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--group", type=int, default=0, help="group mode: this many setups (1 .. 256)")
    ap.add_argument("--group-packets", type=int, default=200)
    args = ap.parse_args()
    import torch

    from vorbispizza_amd import Context
    ctx = Context(0)
    for n in args.streams:
        if args.group:
            print(json.dumps(run_group(n, args.group, args.group_packets, args.steps, args.warmup, ctx, torch)), flush=True)
        else:
            print(json.dumps(run(n, args.steps, args.warmup, ctx, torch)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
