#!/usr/bin/env python3
"""What the per-frame driver does, recorded with fakes (host code only: no GPU): every call interpolate_stream and
interpolate_shard make on the model, the conversion hooks, the scene test and the writer, over a grid of clips, schedules,
model surfaces and world sizes.  tests/test_driver_calls.py replays the grid on the tree and compares, so a change of the
driver that moves one call, one timestep or one announced frame shows.

    python tools/driver_calls.py [out.json]      (default: tests/golden/driver_calls.json)
    python tools/driver_calls.py --dump CASE     (the full recording of one case on stdout)

The file keeps a digest per run; when the test reports one, --dump on the two commits shows the calls that differ.

Regenerate the file only from a commit whose driver is known good (the bit-exact reference traces of tests/test_schedule.py
and the GPU suite pass); the file names the commit it was made from."""
import hashlib
import json
import os
import subprocess
import sys
import weakref

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "driver_calls.json")
SRC_FPS = 24.0

# name -> (source frames, cuts: k = a cut between frames k and k + 1)
CLIPS = {
    "n2": (2, ()), "n3": (3, ()), "n4": (4, ()), "n5": (5, ()), "n14": (14, ()),
    "n14_cut6": (14, (6,)),
    "n20_cuts3_4_12": (20, (3, 4, 12)),  # iteration 3 (centred on frame 4) has a cut on both sides
    "n18_cut8": (18, (8,)),              # 16 iterations over 4 ranks: the cut is iteration 8's right pair, the first of rank 2
}
SCHEDULES = {"t2": (2, 60.0), "fps60": (-1, 60.0)}  # name -> (times, dst_fps)
# name -> (supports_lookahead, prefetch hooks, GROUP): read-ahead depths 0, 1, 3 and 7
SURFACES = {"plain": (False, False, None), "lookahead": (True, False, None), "group1": (True, True, 1), "group4": (True, True, 4)}


def worlds(n):
    """1 .. 4 and one world with more ranks than the clip has loop iterations."""
    return sorted({1, 2, 3, 4, max(n - 2, 0) + 1})


class Inp:
    """Stand-in for a network-size frame tensor (weakly referencable, as tensors are)."""
    is_cuda = False

    def __init__(self, k):
        self.k = k


class Recorder:
    """The fakes of one run over one shared event list: the model, to_inp, check_scene, to_out, the writer and on_step."""

    def __init__(self, surface, cuts):
        self.events, self.made, self.n_calls = [], [], 0
        self.cuts = set(cuts)
        look, prefetch, group = SURFACES[surface]
        self.model = _LookModel(self) if look else _PlainModel(self)
        if prefetch:
            self.model.GROUP = group
            self.model.prefetch_frame = lambda x: self.events.append(["prefetch_frame", x.k])
            self.model.prefetch_pair = lambda a, b: self.events.append(["prefetch_pair", a.k, b.k])

    def to_inp(self, raw, size):
        x = Inp(int(raw[0, 0, 0]))
        self.events.append(["inp", x.k])
        self.made.append(weakref.ref(x))
        return x

    def to_out(self, x, size):
        return x if isinstance(x, str) else f"copy{x.k}"  # a source frame passed through, or a generated frame's tag

    def check_scene(self, a, b, thr):
        assert b.k == a.k + 1, (a.k, b.k)
        self.events.append(["scene", a.k])
        return a.k in self.cuts

    def alive(self):  # (frames hold no references, so they are in no cycle: a dropped one is gone at once)
        return sum(1 for r in self.made if r() is not None)

    def call(self, *entry):
        self.n_calls += 1
        self.events.append(list(entry))
        return self.n_calls

    def model_calls(self):
        return [e for e in self.events if e[0] in ("ts", "drba", "calc_flow")]


class _PlainModel:
    """The reference models' surface.  A generated frame is named by what it depends on -- the centre frame, the timestep and
    the frame pair the carried `reuse` was made from (cold steps: none) -- so a shard with a wrong entering state emits other
    frames than the sequential run, as with the real models."""
    scale, pad_size = 1.0, 16

    def __init__(self, rec):
        self.rec = rec

    def calc_flow(self, a, b):
        no = self.rec.call("calc_flow", a.k, b.k)
        return ("flow", a.k, b.k, no), ("flow", b.k, a.k, no), ("feat", a.k), ("feat", b.k)

    def inference_ts(self, I0, I1, ts):
        self.rec.call("ts", I0.k, I1.k, [float(t) for t in ts])
        return [I0 if t == 0 else I1 if t == 1 else f"ts{I0.k}-{I1.k}@{float(t)!r}" for t in ts]

    def _drba(self, I0, I1, I2, ts, reuse, linear, lookahead):
        # reuse: None, the one a DRBA call returned, or parallel.warm_reuse's (flow_ba, flow_ab, fb, fa) of calc_flow
        if reuse is None:
            pair, by = None, None
        elif reuse[0] == "reuse":
            pair, by = reuse[1], reuse[2]
        else:
            pair, by = [reuse[1][1], reuse[1][2]], reuse[0][3]
        look = None
        if lookahead is not None:
            look = [x.k if isinstance(x, Inp) else [float(t) for t in x] for x in lookahead]
        no = self.rec.call("drba", I0.k, I1.k, I2.k, [float(t) for t in ts], by, bool(linear), look)
        tag = "cold" if pair is None else f"{pair[0]}-{pair[1]}"
        out = [I0 if t == 0 else I1 if t == 1 else I2 if t == 2 else f"drba{I1.k}@{float(t)!r}/{tag}" for t in ts]
        return out, ("reuse", [I1.k, I2.k], no)

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False):
        return self._drba(I0, I1, I2, ts, reuse, linear, None)


class _LookModel(_PlainModel):
    supports_lookahead = True

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, lookahead=None):
        return self._drba(I0, I1, I2, ts, reuse, linear, lookahead)


class _IO:
    """VideoFI_IO's read/write surface; the source must not be asked again once it has returned None."""

    def __init__(self, frames, rec):
        self.src_fps, self.total_frames_count = SRC_FPS, len(frames)
        self._it, self.rec = iter(list(frames) + [None]), rec

    def read_frame(self):
        return next(self._it)

    def write_frame(self, x):
        self.rec.events.append(["write", x])


def make_frames(n):
    return [np.full((16, 16, 3), k, dtype=np.uint8) for k in range(n)]


def run_sequential(clip, schedule, surface):
    """-> {"events": everything in call order, "written": frames returned, "max_alive": most network inputs alive at an on_step}"""
    from drba_amd import infer
    (n, cuts), (times, dst_fps) = CLIPS[clip], SCHEDULES[schedule]
    rec, alive = Recorder(surface, cuts), []

    def on_step(idx):
        rec.events.append(["step", idx])
        alive.append(rec.alive())

    written = infer.interpolate_stream(rec.model, _IO(make_frames(n), rec), dst_fps, times=times, enable_scdet=bool(cuts),
                                       to_inp=rec.to_inp, to_out=rec.to_out, check_scene=rec.check_scene, on_step=on_step)
    return {"events": rec.events, "written": written, "max_alive": max(alive)}


def run_shard(clip, schedule, surface, rank, world):
    """-> {"model": the model calls, "emitted": [[frame, ...] per emission]} and, for the property checks (not stored),
    "events", "max_alive" (most network inputs alive at an emission).  The run without a sink must return the same frames."""
    from drba_amd import parallel
    (n, cuts), (times, dst_fps) = CLIPS[clip], SCHEDULES[schedule]
    frames = make_frames(n)
    rec, emitted, alive = Recorder(surface, cuts), [], []

    def sink(fr):
        emitted.append(list(fr))
        alive.append(rec.alive())

    kw = dict(times=times, enable_scdet=bool(cuts), to_inp=rec.to_inp, to_out=rec.to_out, check_scene=rec.check_scene)
    rest = parallel.interpolate_shard(rec.model, frames, SRC_FPS, dst_fps, rank, world, sink=sink, **kw)
    assert rest == [], rest
    rec2 = Recorder(surface, cuts)
    kw.update(to_inp=rec2.to_inp, to_out=rec2.to_out, check_scene=rec2.check_scene)
    returned = parallel.interpolate_shard(rec2.model, frames, SRC_FPS, dst_fps, rank, world, **kw)
    assert returned == [x for e in emitted for x in e], (returned, emitted)
    assert rec2.model_calls() == rec.model_calls()
    return {"model": rec.model_calls(), "emitted": emitted, "events": rec.events, "max_alive": max(alive, default=0)}


def grid():
    for clip in CLIPS:
        for schedule in SCHEDULES:
            for surface in SURFACES:
                yield clip, schedule, surface


def digest(x):
    """SHA-256 (first 24 hex digits) of the canonical JSON of a recording; floats are written with repr, so exactly."""
    return hashlib.sha256(json.dumps(x, separators=(",", ":"), sort_keys=True).encode()).hexdigest()[:24]


def summarise(seq, shards):
    """What the file keeps of a case: digests of the sequential event list and of each world's per-rank [model calls,
    emissions], with the counts that say where to look when one differs."""
    return {"sequential": digest(seq["events"]), "events": len(seq["events"]), "written": seq["written"], "max_alive": seq["max_alive"],
            "shards": {str(w): digest([[s["model"], s["emitted"]] for s in runs]) for w, runs in shards.items()}}


def run_case(clip, schedule, surface):
    """-> (run_sequential(...), {world: [run_shard(...) per rank]})"""
    shards = {w: [run_shard(clip, schedule, surface, r, w) for r in range(w)] for w in worlds(CLIPS[clip][0])}
    return run_sequential(clip, schedule, surface), shards


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--dump":  # the full recording of one case ("n14/t2/group4"), to diff two commits with
        seq, shards = run_case(*sys.argv[2].split("/"))
        json.dump({"sequential": seq, "shards": {str(w): [{"model": s["model"], "emitted": s["emitted"]} for s in runs]
                                                 for w, runs in shards.items()}}, sys.stdout, indent=1)
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "drba_amd"], capture_output=True, text=True,
                           check=True).stdout.strip()
    cases = {"/".join(c): summarise(*run_case(*c)) for c in grid()}
    with open(path, "w") as f:  # one line per case
        f.write('{"made_from": %s,\n "cases": {\n' % json.dumps({"commit": head, "drba_amd_modified": bool(dirty),
                                                               "by": "python tools/driver_calls.py"}))
        f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(cases.items())))
        f.write("\n }}\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(cases)} cases) from {head}")
