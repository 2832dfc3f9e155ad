#!/usr/bin/env python3
"""What the host link gives on this box: pinned host <-> device copies of the sizes the end-to-end leg moves (one sub-batch of
16 real stereo streams: ~54 MB of residue in, ~54 MB of float PCM out), alone, both directions at once, and on two streams.
`pcie_probe.py job`: the floor of the 1 024-stream job with the entropy decode on the device -- 1.7 GB of 16-bit PCM down while
88 MB of packet bytes go up, in pieces of a sub-batch's size on four streams."""
import sys
import time
import torch

dev = torch.device("cuda", 0)
if sys.argv[1:] == ["job"]:
    down, up, pieces = 1700 * 10**6, 88 * 10**6, 16
    h_out = torch.empty(down // 2, dtype=torch.int16, pin_memory=True)
    d_out = torch.zeros(down // 2, dtype=torch.int16, device=dev)
    h_in = torch.empty(up, dtype=torch.uint8, pin_memory=True).zero_()
    d_in = torch.empty(up, dtype=torch.uint8, device=dev)
    streams = [torch.cuda.Stream() for _ in range(4)]
    for with_up in (False, True):
        times = []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(pieces):
                with torch.cuda.stream(streams[i % 4]):
                    if with_up:
                        d_in[i * up // pieces:(i + 1) * up // pieces].copy_(h_in[i * up // pieces:(i + 1) * up // pieces], non_blocking=True)
                    a, b = i * (down // 2) // pieces, (i + 1) * (down // 2) // pieces
                    h_out[a:b].copy_(d_out[a:b], non_blocking=True)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        t = sorted(times[1:])[len(times[1:]) // 2]
        print("1.7 GB of 16-bit PCM down%s: median %.1f ms (%.1f GB/s down)" % (", 88 MB of packet bytes up" if with_up else " alone", t * 1e3, down / 1e9 / t), flush=True)
    sys.exit(0)
for mb in (8, 54, 428):
    n = mb * (1 << 20) // 4
    h_in = torch.empty(n, dtype=torch.float32, pin_memory=True).normal_()
    h_out = torch.empty(n, dtype=torch.float32, pin_memory=True)
    d_in = torch.empty(n, dtype=torch.float32, device=dev)
    d_out = torch.empty(n, dtype=torch.float32, device=dev).normal_()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def timed(fn, reps=10):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    t_h2d = timed(lambda: d_in.copy_(h_in, non_blocking=True))
    t_d2h = timed(lambda: h_out.copy_(d_out, non_blocking=True))

    def both():
        with torch.cuda.stream(s1):
            d_in.copy_(h_in, non_blocking=True)
        with torch.cuda.stream(s2):
            h_out.copy_(d_out, non_blocking=True)
    t_both = timed(both)
    gb = n * 4 / 1e9
    print("%4d MB: H2D %.1f GB/s, D2H %.1f GB/s, both at once %.1f GB/s each way (%.2f ms)" % (mb, gb / t_h2d, gb / t_d2h, gb / t_both, t_both * 1e3), flush=True)
