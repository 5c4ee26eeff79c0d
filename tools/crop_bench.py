#!/usr/bin/env python3
"""The measurements of profiles/crop.md, one JSON line each.

    python tools/crop_bench.py stat           the active-picture statistic on a 1080 x 1920 x 3 uint8 frame and on its 1080 x 1920 luma
                                              plane, each against a device-to-device copy of the same number of bytes
    python tools/crop_bench.py loop           frames/s of the 1080p `-t 2` driver loop over a 1440 x 1080 picture pillarboxed into 1920 x 1080:
                                              without the flag, with --crop 1440:1080:240:0, and on the bare 1440 x 1080 clip (five runs
                                              each, interleaved; medians)
    python tools/crop_bench.py parent DIR     the flag-off loop with the drba_amd package of another checkout (DIR holds drba_amd/ and
                                              include/, with a built library): the parent commit's figure in the same session
    python tools/crop_bench.py scan           frames/s of `--crop auto`'s first pass over a Y4M file and an .npz of the pillarboxed clip
"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1]
sys.path.insert(0, os.path.abspath(sys.argv[2]) if mode == "parent" else ROOT)
sys.path.insert(1, ROOT)
import numpy as np
import torch
import drba_amd
from drba_amd import ops
from drba_amd import infer as drv
from drba_amd.utils import synth
dev = torch.device("cuda:0")
out = {"mode": mode, "drba_amd": os.path.dirname(drba_amd.__file__)}
H, W, PW, X0 = 1080, 1920, 1440, 240


def ev_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def pillarboxed(n):
    """n frames of 1080 x 1920: a moving 1440 x 1080 picture between two black bars of 240 columns; and the bare picture"""
    bare = synth.make_clip(n, H, PW, seed=977, offsets=[24 * k + 8 * (k % 2) for k in range(n)])
    full = np.zeros((n, H, W, 3), np.uint8)
    full[:, :, X0:X0 + PW] = np.stack(bare)
    return full, np.stack(bare)


if mode == "stat":
    for name, shape in (("packed", (H, W, 3)), ("luma", (H, W))):
        n = int(np.prod(shape))
        # 64 frames of 6.2 MB (2.1 MB for luma) walked in turn: 400 MB (133 MB) between two reads of a frame
        xs = [torch.randint(0, 256, shape, dtype=torch.uint8, device=dev) for _ in range(64)]
        src = [torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev) for _ in range(64)]
        dst = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(4)]
        stat = lambda i: ops._edge_max_enqueue(xs[i % 64])
        copy = lambda i: dst[i % 4].copy_(src[i % 64])
        same = lambda i: ops._edge_max_enqueue(xs[0])
        for f in (stat, copy, same):
            ev_time(f, 8)
        ts, tc, tw = (sorted(ev_time(f, 64) for _ in range(5)) for f in (stat, copy, same))
        out[name] = dict(bytes=n, stat_s=ts, copy_s=tc, stat_same_frame_s=tw, stat_GBps=n / ts[2] / 1e9, copy_GBps_copied=n / tc[2] / 1e9,
                         stat_over_copy=ts[2] / tc[2])
        t = time.perf_counter()
        for i in range(200):
            ops.edge_max_async(xs[0])
        torch.cuda.synchronize()
        out[name]["async_host_s"] = (time.perf_counter() - t) / 200
        # the kernels' own durations (the library's launch trace: an event pair on each dispatch packet), frames walked as above
        ops.trace_begin()
        for i in range(64):
            stat(i)
        torch.cuda.synchronize()
        by = {}
        for r in ops.trace_end():
            by.setdefault(r["name"], []).append(r["ms"] * 1e3)
        out[name]["kernel_us_median"] = {k: round(statistics.median(v), 2) for k, v in by.items()}
        del xs, src, dst
elif mode == "scan":
    from drba_amd import crop, y4m
    N = 48
    full, _ = pillarboxed(N)
    tmp = tempfile.mkdtemp(prefix="crop_bench_")
    npz, y4 = os.path.join(tmp, "c.npz"), os.path.join(tmp, "c.y4m")
    np.savez(npz, frames=full, fps=np.float64(24.0))
    luma = np.clip(16.0 + 219.0 * full.astype(np.float32).mean(axis=3) / 255.0, 0, 255).astype(np.uint8)  # (a stand-in luma: the scan reads Y only)
    with open(y4, "wb") as f:
        wr = y4m.Writer(f, y4m.Header(W, H, (24, 1), interlace="p", chroma="420mpeg2"))
        for k in range(N):
            wr.write_frame(y4m.YuvFrame.from_planes(luma[k], np.full((H // 2, W // 2), 128, np.uint8), np.full((H // 2, W // 2), 128, np.uint8)))
        wr.flush()
    for name, path, align in (("npz", npz, (1, 1)), ("y4m", y4, (2, 2))):
        crop.scan(path, align=align)
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            box = crop.scan(path, align=align)
            ts.append(time.perf_counter() - t)
        # the same pass without the statistic: opening the clip and touching every frame
        from drba_amd.evaluate import ClipSource
        tr = []
        for _ in range(5):
            t = time.perf_counter()
            for fr in ClipSource(path):
                pass
            tr.append(time.perf_counter() - t)
        out[name] = dict(frames=N, box=str(box), scan_s=sorted(ts), read_only_s=sorted(tr), scan_frames_per_s=N / statistics.median(ts),
                         read_only_frames_per_s=N / statistics.median(tr))
    for p in (npz, y4):
        os.remove(p)
    os.rmdir(tmp)
else:
    import bench
    from drba_amd import tune
    wdir = tune._default_weights("rife")
    model = drv.load_model("rife", 1.0, weights=wdir if (wdir and os.path.isdir(wdir)) else tune._synthetic_weights("rife"))
    N = 42
    full_np, bare_np = pillarboxed(N)
    full, bare = [torch.from_numpy(f).to(dev) for f in full_np], [torch.from_numpy(f).to(dev) for f in bare_np]
    plain = bench._dev_hooks()
    if mode != "parent":
        from drba_amd import crop
        box = crop.parse("1440:1080:240:0", frame_size=(H, W))
        win = box.window
        cropped = (lambda fr, size: ops.to_inp(fr, size, window=win)), (lambda x, size: ops.to_out(x, size, window=win))

    def leg(clip, hooks, kw):
        io = bench._DevIO(clip, 24.0)
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = drv.interpolate_stream(model, io, 48.0, times=2, to_inp=hooks[0], to_out=hooks[1], **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert tuple(io.last.shape) == tuple(clip[0].shape)
        return n / dt

    legs = [("full_no_flag", full, plain, {})]
    if mode != "parent":
        legs += [("full_crop", full, cropped, {"crop": box}), ("bare_1440", bare, plain, {})]
    for name, clip, hooks, kw in legs:  # warm-up: tuning, allocator
        leg(clip, hooks, kw), leg(clip, hooks, kw)
    res = {name: [] for name, *_ in legs}
    for _ in range(5):
        for name, clip, hooks, kw in legs:
            res[name].append(round(leg(clip, hooks, kw), 1))
    out["frames_per_s"] = res
    out["median"] = {k: statistics.median(v) for k, v in res.items()}
    out["source_frames"] = N
print(json.dumps(out))
