"""Rehearsal: run the driver loop over a short synthetic clip so that the conv autotuner meets -- and, with the store of
drba_amd.tunecache on, keeps -- the launch shapes a real clip of that frame size and schedule will ask for.

    python -m drba_amd.tune -m rife --size 1080x1920 -fps 60 -s          # fills the store for that size and schedule
    python -m drba_amd.tune --list | --clear                             # no device needed

A new launch shape can appear in the middle of a clip: the first scene cut runs inference_ts at batch 1 and 2, a cold
calc_flow and the shorter groups of steps on either side of the cut, and each first use stalls the three-stream pipeline
once per candidate configuration.  infer.py does not rehearse on its own (a rehearsal costs a few dozen steps: nothing for
an episode, too much for a 16-frame clip); this command populates the store once per machine, build and frame size, and
the command line's own runs add whatever they meet.
"""
import argparse
import json
import math
import os
import sys
from fractions import Fraction

MAX_FRAMES = 64  # source frames of a rehearsal clip, at most
# Where the scenes of the rehearsal clip start, with scene detection on.  Frame 2 is a scene of its own: the iteration centred on it
# has a cut on both sides, the one before it a cut on the right, the one after it a cut on the left.  From frame 3 on the scenes
# are 13, 14, 15 and 16 frames long: the driver announces frames to the model only up to a cut, so the last steps in front of
# one run as a shorter group or as single steps depending on where the cut falls in the group phase (RIFE.GROUP = 4) -- the
# four spacings cover every phase.  The last scene (61 .. 63) is the cold restart with nothing to look ahead to, and the tail.
SCDET_CUTS = (2, 3, 16, 30, 45, 61)


def schedule_period(src_fps, dst_fps, times):
    """Source frames after which calc_t's timesteps repeat (1 for an integer `-t`)."""
    if times != -1:
        return 1
    return Fraction(dst_fps / src_fps).limit_denominator(1000).denominator


def plan_clip(src_fps, dst_fps, times, enable_scdet, group=4):
    """-> (number of source frames, frames at which a new scene starts)."""
    if enable_scdet:
        return MAX_FRAMES, SCDET_CUTS
    # head, the cold step, at least two whole groups at every phase of the timestep schedule, the ramp-down and the tail
    phase = math.lcm(schedule_period(src_fps, dst_fps, times), max(int(group), 1))
    return min(MAX_FRAMES, max(24, 2 * phase + 2 * group + 4)), ()


class DeviceClip:
    """A clip of uint8 HWC frames resident on the device: two synthetic scenes (drba_amd.utils.synth.make_clip, 8 frames
    each) that alternate at every planted cut.  Within a scene the base frames are walked 0 .. 7, 6 .. 1, 0 ..: consecutive
    frames are always neighbours of the base clip, so the scene test sees no cut but the planted ones."""

    def __init__(self, n, h, w, device, cuts=(), seed=977):
        import torch

        from drba_amd.utils import synth
        self.n, self.cuts = int(n), tuple(cuts)
        self.scenes = [[torch.from_numpy(f).to(device) for f in synth.make_clip(min(n, 8), h, w, seed=sd)]
                       for sd in ((seed, seed + 7919) if self.cuts else (seed,))]

    def __len__(self):
        return self.n

    def __getitem__(self, k):
        if not 0 <= k < self.n:
            raise IndexError(k)
        src = self.scenes[sum(1 for c in self.cuts if k >= c) % len(self.scenes)]
        if len(src) == 1:
            return src[0]
        period = 2 * len(src) - 2
        j = k % period
        return src[j if j < len(src) else period - j]


class _DiscardIO:
    """VideoFI_IO's read / write surface over a DeviceClip; written frames are dropped."""

    def __init__(self, clip, fps):
        self.src_fps, self.total_frames_count = fps, len(clip)
        self.clip, self.k, self.written = clip, 0, 0

    def read_frame(self):
        if self.k >= len(self.clip):
            return None
        self.k += 1
        return self.clip[self.k - 1]

    def write_frame(self, x):
        self.written += 1


class _Recorder:
    """Hands every call to the model and notes which frames it was made on: the driver's decisions, as it acted on them."""

    def __init__(self, m):
        self.m, self.calls = m, []
        self.scale, self.pad_size = m.scale, m.pad_size
        self.supports_lookahead = bool(getattr(m, "supports_lookahead", False))

    def inference_ts(self, I0, I1, ts):
        self.calls.append(("ts", I0._drba_rehearsal_idx, I1._drba_rehearsal_idx))
        return self.m.inference_ts(I0, I1, ts)

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, **kw):
        self.calls.append(("drba", I1._drba_rehearsal_idx))
        return self.m.inference_ts_drba(I0, I1, I2, ts, reuse, linear, **kw)

    def __getattr__(self, name):  # the optional driver hooks, present only if the model has them
        if name in ("prefetch_frame", "prefetch_pair", "GROUP", "stats", "intake_stream"):
            return getattr(self.m, name)
        raise AttributeError(name)


def observed_cuts(segments, n):
    """The scene decisions the driver acted on, read off the model calls of each loop iteration (`segments`: the calls between two
    on_step marks; segment 0 is the head, segment c the iteration centred on frame c, the last one the tail).
    -> (sorted frames k with a cut between k - 1 and k, {branch: count})."""
    cuts, branches = set(), dict.fromkeys(("head", "head_cut", "drba", "cut_left", "cut_right", "cut_both", "tail"), 0)
    if len(segments) != n:  # head + (n - 2) iterations + tail
        raise RuntimeError(f"rehearsal: {len(segments)} driver steps for {n} source frames")
    if any(c[0] == "ts" for c in segments[0]):
        branches["head"] += 1
    else:
        branches["head_cut"] += 1
        cuts.add(1)
    for c in range(1, n - 1):
        kinds = [(k[0], k[1]) for k in segments[c]]
        if kinds == [("drba", c)]:
            branches["drba"] += 1
        elif kinds == [("ts", c)]:       # inference_ts(I1, I2): the left pair is unusable
            branches["cut_left"] += 1
            cuts.add(c)
        elif kinds == [("ts", c - 1)]:   # inference_ts(I0, I1): the right pair is unusable
            branches["cut_right"] += 1
            cuts.add(c + 1)
        elif not kinds:
            branches["cut_both"] += 1
            cuts.update((c, c + 1))
        else:
            raise RuntimeError(f"rehearsal: unexpected model calls {segments[c]} in the iteration centred on frame {c}")
    branches["tail"] += 1
    return sorted(cuts), branches


def _model_state_reset(model, stats):
    """Drop what a run of the driver loop leaves on the model (the model knows what it carries: reset_stream_state) and put the
    counters back."""
    reset = getattr(model, "reset_stream_state", None)
    if reset is not None:
        reset()
    if stats is not None:
        model.stats = stats


def rehearse(model, frame_hw, src_fps=24.0, dst_fps=60.0, times=-1, enable_scdet=False, scdet_threshold=0.3, retune=False):
    """Run drba_amd.infer.interpolate_stream over a synthetic clip of `frame_hw` = (H, W) source frames that stays on the
    device, with a sink that drops the frames, so that every launch shape the loop can ask for with this schedule has been
    tuned.  With scene detection the clip carries planted cuts (SCDET_CUTS) and the real scene test decides; the decisions the
    driver acted on must be exactly the planted ones -- RuntimeError otherwise: a rehearsal whose clip produced a false cut or
    missed a planted one has tuned the wrong shapes.  With `-fps` the batch sizes follow the phase of calc_t: the clip holds
    every phase of one period of the schedule against the group phase as far as MAX_FRAMES source frames allow; what the
    rehearsal does not reach is tuned on first use like any other shape.

    retune: stored winners are not read, every shape met is tuned afresh and its entry replaced (shapes this process has already
    tuned are kept: use a fresh process, as `python -m drba_amd.tune --retune` does).

    The model carries no state from the call: no steps computed ahead, no pending side-stream work, `model.stats` as before.
    -> {"frames", "cuts", "branches", "written", "path": the difference of model.stats, "tune": that of ops.tune_stats()}"""
    import torch

    from drba_amd import infer as drv
    from drba_amd import ops
    h, w = int(frame_hw[0]), int(frame_hw[1])
    group = int(getattr(model, "GROUP", 1)) if hasattr(model, "prefetch_frame") else 1
    n, cuts = plan_clip(src_fps, dst_fps, times, enable_scdet, group)
    device = getattr(model, "device", None) or ops.default_device()
    stats0 = dict(model.stats) if isinstance(getattr(model, "stats", None), dict) else None
    before, ignore0 = ops.tune_stats(), ops.TUNE_IGNORE_HITS
    rec, io = _Recorder(model), _DiscardIO(DeviceClip(n, h, w, device, cuts), float(src_fps))
    count, marks = [0], []

    def to_inp(frame_u8, dst_size):
        x = ops.to_inp(frame_u8, dst_size)
        x._drba_rehearsal_idx = count[0]  # frames are converted in the order they are read
        count[0] += 1
        return x

    ops.TUNE_IGNORE_HITS = bool(retune) or ignore0
    det0 = ops.deterministic()  # a rehearsal IS the timing: it runs with the deterministic mode off and puts it back
    if det0:
        ops.set_deterministic(False)
    try:
        with torch.cuda.device(device):
            drv.interpolate_stream(rec, io, dst_fps, times=times, enable_scdet=enable_scdet, scdet_threshold=scdet_threshold,
                                   to_inp=to_inp, to_out=lambda x, size: ops.to_out(x, size),
                                   on_step=lambda idx: marks.append(len(rec.calls)))
            torch.cuda.synchronize(device)
    finally:
        ops.TUNE_IGNORE_HITS = ignore0
        if det0:
            ops.set_deterministic(True)
        stats1 = dict(model.stats) if stats0 is not None else {}
        _model_state_reset(model, stats0)
    segments = [rec.calls[a:b] for a, b in zip([0] + marks, marks)]
    seen, branches = observed_cuts(segments, n)
    if seen != sorted(cuts):
        raise RuntimeError(f"rehearsal at {h}x{w}: the scene test cut at frames {seen}, planted were {sorted(cuts)}; the shapes tuned "
                           "are not the ones a clip with these cuts runs")
    after = ops.tune_stats()
    return {"frames": n, "cuts": list(cuts), "branches": branches, "written": io.written,
            "path": {k: v - stats0.get(k, 0) for k, v in stats1.items()},  # which paths the model's calls took (RIFE.stats)
            "tune": {k: after[k] - before[k] for k in after}}


def _synthetic_weights(model_type):
    from drba_amd.utils import synth
    if model_type == "rife":
        return synth.ifnet_state_dict(0)
    if model_type == "gmfss_union":
        return synth.gmfss_union_state_dicts(0)
    raise FileNotFoundError(f"no weights on disk for -m {model_type} and no synthetic state dicts for it: pass --weights DIR")


def _default_weights(model_type):
    return {"rife": "weights/train_log_rife_426_heavy", "gmfss": "weights/train_log_gmfss",
            "gmfss_union": "weights/train_log_gmfss_union"}.get(model_type)


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m drba_amd.tune", description="Fill the conv autotuner's store by a rehearsal")
    p.add_argument("-m", "--model_type", dest="model_type", type=str, default="rife")
    p.add_argument("--size", type=str, default=None, help="source frame size HxW, e.g. 1080x1920")
    p.add_argument("-scale", "--scale", dest="scale", type=float, default=1.0)
    p.add_argument("--src-fps", dest="src_fps", type=float, default=24.0)
    p.add_argument("-fps", "--dst_fps", dest="dst_fps", type=float, default=60)
    p.add_argument("-t", "--times", dest="times", type=int, default=-1)
    p.add_argument("-s", "--enable_scdet", dest="enable_scdet", action="store_true", default=False)
    p.add_argument("-st", "--scdet_threshold", dest="scdet_threshold", type=float, default=0.3)
    p.add_argument("--weights", type=str, default=None, help="weight directory (default: the model's, synthetic if absent)")
    p.add_argument("--retune", action="store_true", help="ignore stored winners: tune every shape afresh and replace its entry")
    p.add_argument("--list", dest="list_", action="store_true", help="print the entries of every identity file in the directory")
    p.add_argument("--clear", action="store_true", help="remove the files the store wrote in the directory")
    return p.parse_args(argv)


def _this_identity():
    """The identity of this process, or None without a device / a built library."""
    from drba_amd import tunecache
    try:
        import torch
        if tunecache.identity_provider is tunecache.device_identity and not torch.cuda.is_available():
            return None
        return tunecache.identity_provider(None)
    except Exception:  # noqa: BLE001 (no device, no library: the listing goes on without the mark)
        return None


def main(argv=None):
    from drba_amd import tunecache
    args = parse_args(argv)
    tunecache.default_on()  # a command line: on unless DRBA_TUNE_CACHE=0
    d = tunecache.directory()
    if args.list_ or args.clear:
        if d is None:
            print(json.dumps({"store": None, "note": "DRBA_TUNE_CACHE=0: the store is off"}))
            return 0
        if args.clear:
            gone = tunecache.clear(d)
            print(json.dumps({"store": d, "removed": [os.path.basename(p) for p in gone]}))
            return 0
        mine = _this_identity()
        files = [{"file": os.path.basename(p), "this_process": mine is not None and ident == mine, "identity": ident,
                  "bytes": os.path.getsize(p), "entries": ent} for p, ident, ent in tunecache.list_files(d)]
        print(json.dumps({"store": d, "files": files}))
        return 0
    if args.size is None:
        raise SystemExit("--size HxW is required for a rehearsal")
    h, w = (int(v) for v in args.size.lower().split("x"))
    if d is None:
        raise SystemExit("DRBA_TUNE_CACHE=0: the store is off, a rehearsal would keep nothing")
    from drba_amd import infer as drv
    from drba_amd import ops
    wdir = args.weights or _default_weights(args.model_type)
    synthetic = args.weights is None and not (wdir and os.path.isdir(wdir))
    model = drv.load_model(args.model_type, scale=args.scale, weights=_synthetic_weights(args.model_type) if synthetic else wdir)
    store = tunecache.active(getattr(model.device, "index", None))
    n0 = len(store)
    dst_fps = args.dst_fps if args.times == -1 else args.src_fps * args.times
    rep = rehearse(model, (h, w), args.src_fps, dst_fps, args.times, args.enable_scdet, args.scdet_threshold, retune=args.retune)
    store = tunecache.Store(store.dir, store.identity)  # read back from disk: what the next process will find
    print(json.dumps({"store": store.path, "entries_before": n0, "entries_after": len(store),
                      "bytes": os.path.getsize(store.path) if os.path.exists(store.path) else 0,
                      "weights": "synthetic (drba_amd.utils.synth)" if synthetic else wdir, "model": args.model_type,
                      "size": [h, w], "retune": bool(args.retune), "rehearsal": rep, "decisions_checked": True,
                      "tune_stats": ops.tune_stats()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
