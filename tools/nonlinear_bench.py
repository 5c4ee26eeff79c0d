"""What a non-linear DRBA step costs: the 1080p RIFE driver loop at `-t 2`, warm, in three readings.

    python tools/nonlinear_bench.py [--parent-tree DIR] [--rounds 2] [--blocks 5] [--steps 40] [--warmup 24] [--json OUT]

  linear      this tree, drba_amd.infer.interpolate_stream(..., linear=True): the ceiling
  nonlinear   this tree, linear=False (infer.py --nonlinear)
  parent      DIR -- a built checkout of the parent commit -- with every inference_ts_drba call of its driver loop switched to
              linear=False by this tool (the parent's driver has no switch): the yardstick for the gain.  Left out without DIR.

The clip is bench.py's config 1 construction: synth.make_clip(8, 1080, 1920, seed=1234) resident in HBM, cycled with a roll so
the content keeps moving; frames in and out through the device to_inp / to_out kernels (decode / encode are outside the metric).
Every reading is a process of its own (a tree brings its own library); the readings alternate, `--rounds` times over, so that a
drift of the box shows as spread and not as a difference.  Inside a process: W warm-up iterations, then `--blocks` blocks of K
iterations, each block between two device synchronisations; a reading is the median block, its spread the blocks' range.
bench.py is not involved and stays the project's yardstick; this tool answers one question beside it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--blocks", type=int, default=5)
    p.add_argument("--steps", type=int, default=40, help="driver-loop iterations per timed block")
    p.add_argument("--warmup", type=int, default=24)
    p.add_argument("--size", default="1080x1920", help="source HxW (the readings that count are at 1080x1920)")
    p.add_argument("--json", dest="json_path", default=None)
    p.add_argument("--leg", default=None, choices=("linear", "nonlinear", "parent"), help="(internal) run one reading in this process")
    p.add_argument("--tree", default=HERE, help="(internal) the tree the reading imports drba_amd from")
    return p.parse_args(argv)


class _Clip:
    """Frame k of bench.py's config 1 clip: 8 base frames in HBM, cycled, rolled by 3 columns per cycle."""

    def __init__(self, n, h, w, dev):
        import torch

        from drba_amd.utils import synth
        self.n = n
        self.base = [torch.from_numpy(f).to(dev) for f in synth.make_clip(8, h, w, seed=1234)]

    def frame(self, k):
        import torch
        f = self.base[k % 8]
        return torch.roll(f, (k // 8) * 3, dims=1) if k >= 8 else f


class _IO:
    def __init__(self, clip, fps):
        self.src_fps, self.total_frames_count, self.clip, self.k, self.written = fps, clip.n, clip, 0, 0

    def read_frame(self):
        if self.k >= self.clip.n:
            return None
        self.k += 1
        return self.clip.frame(self.k - 1)

    def write_frame(self, x):
        self.written += 1


def run_leg(args):
    """One reading in this process -> the JSON object printed on the last line."""
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    from drba_amd import infer as drv
    from drba_amd import ops
    from drba_amd.models.rife import RIFE
    from drba_amd.utils import synth
    if not torch.cuda.is_available():
        raise SystemExit("nonlinear_bench: no GPU -- a time is measured on the device or not at all")
    assert os.path.abspath(drv.__file__).startswith(os.path.abspath(args.tree)), (drv.__file__, args.tree)
    dev = torch.device("cuda:0")
    h, w = (int(v) for v in args.size.split("x"))
    kw = {}
    if args.leg == "parent":
        # the parent's driver loop passes linear=True literally: every call is switched here
        orig = RIFE.inference_ts_drba

        def forced(self, I0, I1, I2, ts, reuse=None, linear=False, lookahead=None):
            return orig(self, I0, I1, I2, ts, reuse, False, lookahead)
        RIFE.inference_ts_drba = forced
    else:
        kw["linear"] = args.leg == "linear"
    model = RIFE(weights=synth.ifnet_state_dict(seed=0), scale=1.0, device=dev)
    W_, K, B = args.warmup, args.steps, args.blocks
    clip = _Clip(W_ + K * B + 4, h, w, dev)
    io = _IO(clip, 24.0)
    marks, stats0 = [], {}

    def on_step(idx):  # idx loop iterations are complete
        j = idx - W_
        if j >= 0 and j % K == 0 and j // K <= B:
            torch.cuda.synchronize()
            marks.append((time.perf_counter(), io.written))
            if j == 0:
                stats0.update(model.stats)

    drv.interpolate_stream(model, io, 48.0, times=2, to_inp=lambda f, size: ops.to_inp(f, size), to_out=lambda x, size: ops.to_out(x, size),
                           on_step=on_step, **kw)
    torch.cuda.synchronize()
    assert len(marks) == B + 1, len(marks)
    ms = [(marks[i + 1][0] - marks[i][0]) / K * 1e3 for i in range(B)]
    frames = [marks[i + 1][1] - marks[i][1] for i in range(B)]
    assert all(f == 2 * K for f in frames), frames  # -t 2: two written frames per iteration
    path = {k: v - stats0.get(k, 0) for k, v in model.stats.items()}
    return {"leg": args.leg, "size": [h, w], "steps_per_block": K, "warmup": W_, "ms_per_step_blocks": [round(v, 4) for v in ms],
            "ms_per_step": round(statistics.median(ms), 4), "block_min": round(min(ms), 4), "block_max": round(max(ms), 4),
            "path": path, "device": torch.cuda.get_device_name(0)}


def main(argv=None):
    args = parse(argv)
    if args.leg:
        print(json.dumps(run_leg(args)))
        return 0
    legs = [("linear", HERE), ("nonlinear", HERE)] + ([("parent", os.path.abspath(args.parent_tree))] if args.parent_tree else [])
    readings = {name: [] for name, _ in legs}
    for r in range(args.rounds):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--tree", tree, "--blocks", str(args.blocks), "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--size", args.size]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, timeout=900)
            if p.returncode != 0:  # a reading that failed ends the run: nothing more is started on the device
                sys.stderr.write(p.stderr[-3000:])
                return p.returncode or 1
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            readings[name].append(rec)
            print(f"round {r} {name}: {rec['ms_per_step']} ms/step (blocks {rec['block_min']} .. {rec['block_max']}), path {rec['path']}", flush=True)
    summary = {}
    for name, recs in readings.items():
        blocks = [v for rec in recs for v in rec["ms_per_step_blocks"]]
        summary[name] = {"ms_per_step": round(statistics.median(blocks), 4), "min": min(blocks), "max": max(blocks),
                         "per_process_medians": [rec["ms_per_step"] for rec in recs], "frames_per_s": round(2e3 / statistics.median(blocks), 1)}
    out = {"command": "nonlinear_bench", "rounds": args.rounds, "summary": summary, "readings": readings}
    print(json.dumps(out))
    if args.json_path:
        with open(args.json_path, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
