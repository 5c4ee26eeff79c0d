#!/usr/bin/env python3
"""The measurements of profiles/dedup.md, one JSON line each.

    python tools/dedup_bench.py stat           the duplicate statistic at 3 x 1088 x 1920 against a device-to-device copy of the same size
    python tools/dedup_bench.py loop           frames/s of the 1080p `-t 2` driver loop: a clip without repeats with and without --dedup, a
                                               clip on twos with and without it (five runs each, interleaved; medians)
    python tools/dedup_bench.py parent DIR     the flag-off loop with the drba_amd package of another checkout (DIR holds drba_amd/ and
                                               include/, with a built library): the parent commit's figure in the same session
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1]
sys.path.insert(0, os.path.abspath(sys.argv[2]) if mode == "parent" else ROOT)
sys.path.insert(1, ROOT)
import torch
import drba_amd
from drba_amd import ops
from drba_amd import infer as drv
from drba_amd.utils import synth
dev = torch.device("cuda:0")
out = {"mode": mode, "drba_amd": os.path.dirname(drba_amd.__file__)}
H, W = 1080, 1920


def ev_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


if mode == "stat":
    n = 3 * 1088 * 1920
    xs = [torch.rand(1, 3, 1088, 1920, device=dev) for _ in range(16)]  # 16 x 25 MB: every call reads 50 MB it has not read for 350 MB
    dst = [torch.empty_like(xs[0]) for _ in range(2)]
    big_src = [torch.rand(2 * n, device=dev) for _ in range(4)]
    big_dst = [torch.empty(2 * n, device=dev) for _ in range(4)]
    stat = lambda i: ops._dup_stats_enqueue(xs[(2 * i) % 16], xs[(2 * i + 1) % 16], 5 / 255)
    copy = lambda i: big_dst[i % 4].copy_(big_src[i % 4])
    for f in (stat, copy):
        ev_time(f, 8)
    ts = sorted(ev_time(stat, 40) for _ in range(5))
    tc = sorted(ev_time(copy, 40) for _ in range(5))
    same = lambda i: ops._dup_stats_enqueue(xs[0], xs[1], 5 / 255)
    ev_time(same, 8)
    tw = sorted(ev_time(same, 40) for _ in range(5))
    out.update(stat_s=ts, copy_s=tc, stat_same_pair_s=tw, bytes=8 * n, stat_GBps=8 * n / ts[2] / 1e9, copy_GBps_copied=8 * n / tc[2] / 1e9,
               copy_GBps_traffic=16 * n / tc[2] / 1e9, stat_same_pair_GBps=8 * n / tw[2] / 1e9, result=ops.dup_stats(xs[0], xs[1], 5 / 255))
    # host cost of one asynchronous test (launches + pinned copy + event)
    t = time.perf_counter()
    for i in range(200):
        ops.dup_stats_async(xs[0], xs[1], 5 / 255)
    torch.cuda.synchronize()
    out["async_host_s"] = (time.perf_counter() - t) / 200
else:
    import bench
    from drba_amd import tune
    wdir = tune._default_weights("rife")
    model = drv.load_model("rife", 1.0, weights=wdir if (wdir and os.path.isdir(wdir)) else tune._synthetic_weights("rife"))
    to_inp, to_out = bench._dev_hooks()
    N = 42
    base = [torch.from_numpy(f).to(dev) for f in synth.make_clip(N, H, W, seed=977, offsets=[24 * k + 8 * (k % 2) for k in range(N)])]

    class Clip:
        def __init__(self, twos):
            self.twos = twos
        def __len__(self):
            return N
        def __getitem__(self, k):
            return base[k // 2] if self.twos else base[k]

    def leg(twos, dedup):
        io = bench._DevIO(Clip(twos), 24.0)
        kept = []
        kw = dict(dedup=True, on_kept=kept.append) if dedup else {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = drv.interpolate_stream(model, io, 48.0, times=2, to_inp=to_inp, to_out=to_out, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        return n / dt, len(kept)

    legs = [("plain", False, False)] if mode == "parent" else [("plain", False, False), ("dedup", False, True), ("twos_dedup", True, True), ("twos_plain", True, False)]
    for name, twos, dd in legs:  # warm-up: tuning, allocator
        leg(twos, dd), leg(twos, dd)
    res = {name: [] for name, _, _ in legs}
    for _ in range(5):
        for name, twos, dd in legs:
            fps, nk = leg(twos, dd)
            res[name].append(round(fps, 1))
            out[name + "_kept"] = nk
    out["frames_per_s"] = res
    out["median"] = {k: statistics.median(v) for k, v in res.items()}
    out["source_frames"] = N
print(json.dumps(out))
