"""Picture quality of finished clips, as commands.

    python -m drba_amd.evaluate compare A B [--json PATH] [--max-lsb N] [--min-psnr X] [--min-ssim X]
    python -m drba_amd.evaluate holdout -m rife -i CLIP [-k 3] [-scale 1.0] [-s] [-st 0.3] [--plain] [--weights DIR] [--json PATH]

`compare` reads two clips frame by frame (the sources infer.py reads: .npz, .npy + .json, a container when OpenCV is
installed) and prints one JSON line: PSNR, ssim_matlab, the largest difference in LSB and the number of differing bytes, per
clip; `--json` adds the per-frame lists.  A gate that is given and violated makes the exit status 1, so "the outputs of two
builds agree within 1 LSB" is `compare a.npz b.npz --max-lsb 1`.

`holdout` measures what an interpolator is judged by: every K-th frame of a clip is kept, the driver loop of infer.py
(drba_amd.infer.interpolate_stream at `-t K`) fills the gaps, and every emission is compared with the original frame at its
position.  K is odd: an even K puts every emission half-way between two original frames.  `--plain` replaces each DRBA step by
plain inference_ts on the pair the timestep lies in -- the baseline DRBA's "preserves the original pace" is a claim against.

16-bit clips (uint16 frames; `maxval` from the .npz entry or the .json sidecar, 65535 when absent) are measured in their own
steps: the reports carry "depth": 16 and "maxval", the PSNR peak is maxval, `--max-lsb` counts 16-bit steps, and `holdout` emits
at 16 bits.  Two clips of different depth or maxval are refused.

Non-finite JSON numbers are written as the strings "inf" / "-inf" / "nan" (float() reads them back).
"""
import argparse
import json
import math
import os
import sys

import numpy as np

from drba_amd import metrics


# ----------------------------------------------------------------------------------------------------------------- sources
class ClipSource:
    """The frames of a clip, opened the way tools.VideoFI_IO opens its input: .npz {frames, fps}, .npy (+ .json {"fps"}), anything
    else through cv2.VideoCapture when OpenCV is installed.  len() is None for a container (known when it has been read)."""

    def __init__(self, path):
        self.path, self._frames, self._cap = path, None, None
        self.depth, self.maxval = 8, 255
        if not os.path.exists(path):
            raise FileNotFoundError(f"can't find the clip {path}")
        ext = os.path.splitext(path)[1].lower()
        maxval = None
        if ext == ".npz":
            z = np.load(path)
            self._frames, self.fps = z["frames"], (float(z["fps"]) if "fps" in z.files else 24.0)
            maxval = int(z["maxval"]) if "maxval" in z.files else None
        elif ext == ".npy":
            self._frames = np.load(path, mmap_mode="r")
            side = os.path.splitext(path)[0] + ".json"
            meta = json.load(open(side)) if os.path.exists(side) else {}
            self.fps = float(meta["fps"]) if "fps" in meta else 24.0
            maxval = int(meta["maxval"]) if "maxval" in meta else None
        else:
            try:
                import cv2  # noqa: WPS433 (optional dependency)
            except ImportError as e:
                raise RuntimeError(f"decoding {ext or 'this input'} needs OpenCV, which is not installed; use a .npz/.npy clip") from e
            self._cap = cv2.VideoCapture(path)
            self.fps = float(self._cap.get(cv2.CAP_PROP_FPS))
        if self._frames is not None and (self._frames.ndim != 4 or self._frames.shape[3] != 3 or
                                         self._frames.dtype not in (np.uint8, np.uint16)):
            raise ValueError(f"{path}: frames must be uint8 or uint16 [N,H,W,3], got {self._frames.dtype} {self._frames.shape}")
        if self._frames is not None and self._frames.dtype == np.uint16:  # samples in [0, maxval], 65535 unless the clip says
            if maxval is not None and not 255 < maxval <= 65535:
                raise ValueError(f"{path}: maxval of a 16-bit clip must satisfy 255 < maxval <= 65535, got {maxval}")
            self.depth, self.maxval = 16, (65535 if maxval is None else maxval)

    def __len__(self):
        if self._frames is None:
            raise TypeError("the length of a container is known once it has been read")
        return len(self._frames)

    @property
    def random_access(self):
        return self._frames is not None

    def __iter__(self):
        if self._frames is not None:
            for k in range(len(self._frames)):
                yield np.ascontiguousarray(self._frames[k])
            return
        ok, fr = self._cap.read()
        while ok:
            yield fr
            ok, fr = self._cap.read()


def _jsonable(v):
    if isinstance(v, float) and not math.isfinite(v):
        return "nan" if math.isnan(v) else ("inf" if v > 0 else "-inf")
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, np.generic):
        return _jsonable(v.item())
    return v


# ----------------------------------------------------------------------------------------------------------------- compare
def compare(a, b, backend=None):
    """The metrics of clip `b` against clip `a` (two ClipSources, or anything that iterates uint8 [H,W,3] frames).
    ValueError when the frame counts or the frame sizes differ (both values are named).  Two uint16 clips (ClipSource.depth 16)
    are compared in their own steps, the peak being their maxval; clips of different depth or maxval are refused, both named."""
    da, db = getattr(a, "depth", None), getattr(b, "depth", None)
    if da is not None and db is not None and (da, getattr(a, "maxval", None)) != (db, getattr(b, "maxval", None)):
        raise ValueError(f"the clips differ in depth: {da}-bit frames with maxval {getattr(a, 'maxval', None)} against {db}-bit "
                         f"frames with maxval {getattr(b, 'maxval', None)}; convert one of them first")
    if getattr(a, "random_access", True) and getattr(b, "random_access", True) and hasattr(a, "__len__") and len(a) != len(b):
        raise ValueError(f"the clips differ in length: {len(a)} frames against {len(b)}")
    cm = metrics.ClipMetrics(backend=backend, maxval=getattr(a, "maxval", None) if da == 16 else None)
    ia, ib = iter(a), iter(b)
    na = nb = 0
    size = None
    while True:
        fa, fb = next(ia, None), next(ib, None)
        na, nb = na + (fa is not None), nb + (fb is not None)
        if fa is None or fb is None:
            if fa is not None or fb is not None:  # a container ended early: count the rest of the longer one
                na += sum(1 for _ in ia)
                nb += sum(1 for _ in ib)
                raise ValueError(f"the clips differ in length: {na} frames against {nb}")
            break
        if tuple(fa.shape) != tuple(fb.shape):
            raise ValueError(f"the clips differ in frame size: {tuple(fa.shape[:2])} against {tuple(fb.shape[:2])} (frame {na - 1})")
        size = [int(fa.shape[0]), int(fa.shape[1])]
        cm.add(fa, fb)
    res = cm.result()
    res["size"] = size
    if da == 16:  # (the report of two 8-bit clips is what it was)
        res["depth"], res["maxval"] = 16, int(a.maxval)
    return res


GATES = (("max_lsb", "max_lsb", lambda v, lim: v <= lim), ("min_psnr", "min_psnr", lambda v, lim: v >= lim),
         ("min_ssim", "min_ssim", lambda v, lim: v >= lim))


def apply_gates(summary, limits):
    """{gate: {"limit", "value", "ok"}} for the gates that were given (limits: {"max_lsb" | "min_psnr" | "min_ssim": value or None}).
    A NaN value fails its gate."""
    out = {}
    for gate, key, ok in GATES:
        lim = limits.get(gate)
        if lim is not None:
            v = summary[key]
            out[gate] = {"limit": lim, "value": v, "ok": bool(ok(v, lim))}
    return out


def compare_report(res, limits, a_name=None, b_name=None):
    """The JSON object of `compare` (without the per-frame lists) and whether every given gate holds."""
    summary = dict(res["summary"])
    ps = res["per_frame"]["psnr"]
    summary["min_psnr"] = min(ps) if ps else math.inf
    gates = apply_gates(summary, limits)
    ok = all(g["ok"] for g in gates.values())
    rep = {"command": "compare", "a": a_name, "b": b_name, "frames": res["frames"], "size": res.get("size"), "peak": res["peak"]}
    rep.update(summary)
    if "depth" in res:  # 16-bit clips: max_lsb (and its gate) and total_differing are in the clips' own steps and samples
        rep.update({"depth": res["depth"], "maxval": res["maxval"]})
    rep.update({"gates": gates, "ok": ok})
    return rep, ok


# ----------------------------------------------------------------------------------------------------------------- hold-out
class PlainSteps:
    """A model whose DRBA step is plain interpolation: each timestep of inference_ts_drba goes to inference_ts on the pair it
    lies in ((I0, I1) below 1, (I1, I2) from 1 on).  No look-ahead hooks: the driver runs it step by step."""

    def __init__(self, m):
        self.m, self.scale, self.pad_size = m, m.scale, m.pad_size

    def inference_ts(self, I0, I1, ts):
        return self.m.inference_ts(I0, I1, ts)

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, **kw):
        ts = np.asarray(ts, dtype=np.float64)
        left, right = ts[ts < 1], ts[ts >= 1] - 1
        out = list(self.m.inference_ts(I0, I1, left)) if len(left) else []
        if len(right):
            out.extend(self.m.inference_ts(I1, I2, right))
        return out, None


def holdout_plan(n_frames, k):
    """-> (m, half): the first m k + 1 frames are used, frames 0, k, .., m k are kept; emission j of the run stands at original
    frame j - half.  ValueError with the reason when k or the clip does not allow the procedure."""
    k = int(k)
    if k < 3:
        raise ValueError(f"-k {k}: at least 3 (every k-th frame is kept, the k - 1 between two kept ones are held out)")
    if k % 2 == 0:
        raise ValueError(f"-k {k}: an even k puts every emission at a half-integer position between two original frames; use an odd k")
    m = (int(n_frames) - 1) // k
    if m < 2:
        raise ValueError(f"a hold-out at -k {k} needs at least {2 * k + 1} frames (three kept ones), the clip has {n_frames}")
    return m, (k - 1) // 2


class _HoldoutIO:
    """VideoFI_IO's read / write surface: reads the kept frames, compares every emission with the original at its position as it
    is written (nothing is stored) and notes which original each emission was paired with."""

    def __init__(self, frames, k, m, half, fps, kept, held):
        self.frames, self.k, self.m, self.half = frames, k, m, half
        self.src_fps, self.total_frames_count = float(fps), m + 1
        self.kept, self.held = kept, held
        self.i = self.j = 0
        self.pairs, self.skipped = [], []

    def read_frame(self):
        if self.i > self.m:
            return None
        self.i += 1
        return np.ascontiguousarray(self.frames[(self.i - 1) * self.k])

    def write_frame(self, x):
        j, p = self.j, self.j - self.half
        self.j += 1
        if p < 0 or p > self.m * self.k:
            self.skipped.append(j)  # the copies the run emits before the first and after the last frame: no original there
            return
        (self.kept if p % self.k == 0 else self.held).add(x, np.ascontiguousarray(self.frames[p]))
        self.pairs.append((j, p))


def holdout(model, frames, k=3, fps=24.0, enable_scdet=False, scdet_threshold=0.3, plain=False, backend=None, to_inp=None,
            to_out=None, check_scene=None, maxval=None, linear=True):
    """Keep every k-th frame of `frames` (uint8 [N,H,W,3], indexable), let interpolate_stream fill the gaps at `times = k`
    and compare every emission with the original frame at its position.  -> {"k", "m", "frames_used", "emissions",
    "pairs": [(emission, original)], "kept": ClipMetrics.result() + "positions", "held_out": the same}.
    to_inp / to_out / check_scene / backend: the hooks of interpolate_stream and of drba_amd.metrics (defaults: the device
    ones, with the emitted frames staying on the device).
    uint16 frames (samples in [0, maxval], 65535 unless given): the default hooks read and emit 16 bits at that maxval and the
    emissions are compared with the 16-bit originals in their own steps; the result carries "depth": 16 and "maxval".
    linear=False: every DRBA step of the run with the non-linear DistanceRatioMap (infer.py --nonlinear); not together with
    `plain`, whose steps have no DistanceRatioMap at all.  The result carries "linear"."""
    from drba_amd import infer as drv
    if plain and not linear:
        raise ValueError("--nonlinear and --plain exclude each other: a plain step is inference_ts, it has no DistanceRatioMap to retime")
    m, half = holdout_plan(len(frames), k)
    deep = getattr(frames, "dtype", None) == np.uint16
    if maxval is not None and not deep:
        raise ValueError("maxval belongs to uint16 frames")
    mv = (65535 if maxval is None else int(maxval)) if deep else None
    device_out = to_out is None
    if device_out:
        from drba_amd import ops
        if deep:
            to_out = lambda x, size: ops.to_out(x, size, depth=16, maxval=mv)  # noqa: E731  (uint16 on the device: compared there)
        else:
            to_out = lambda x, size: ops.to_out(x, size)  # noqa: E731  (uint8 on the device: compared there)
    if to_inp is None and deep:
        from drba_amd.models.utils import tools
        to_inp = lambda fr, size: tools.to_inp(fr, size, maxval=mv)  # noqa: E731
    backend = backend or metrics.default_backend()
    kept, held = metrics.ClipMetrics(backend=backend, maxval=mv), metrics.ClipMetrics(backend=backend, maxval=mv)
    io = _HoldoutIO(frames, int(k), m, half, fps, kept, held)
    run = PlainSteps(model) if plain else model
    written = drv.interpolate_stream(run, io, float(fps) * int(k), times=int(k), enable_scdet=enable_scdet,
                                     scdet_threshold=scdet_threshold, to_inp=to_inp, to_out=to_out, check_scene=check_scene,
                                     linear=bool(linear))
    if written != int(k) * (m + 1) or len(io.skipped) != 2 * half:
        raise RuntimeError(f"hold-out at k = {k}: the run emitted {written} frames ({len(io.skipped)} without an original), "
                           f"expected {int(k) * (m + 1)} ({2 * half})")
    out = {"k": int(k), "m": m, "frames_used": m * int(k) + 1, "emissions": written, "plain": bool(plain), "linear": bool(linear),
           "pairs": io.pairs}
    if deep:
        out.update({"depth": 16, "maxval": mv})
    for name, cm in (("kept", kept), ("held_out", held)):
        res = cm.result()  # (has waited for every kernel behind the frames)
        res["positions"] = [p for _, p in io.pairs if (p % int(k) == 0) == (name == "kept")]
        out[name] = res
    if device_out:
        ops.check_overflow()  # what tools.to_out asks per frame: an overflow of the two-term fp16 kernels raises
    return out


def holdout_report(res):
    """The JSON object of `holdout` without the per-frame lists."""
    rep = {"command": "holdout", "k": res["k"], "m": res["m"], "frames_used": res["frames_used"], "emissions": res["emissions"],
           "plain": res["plain"], "linear": res["linear"]}
    if "depth" in res:
        rep.update({"depth": res["depth"], "maxval": res["maxval"]})
    for name in ("kept", "held_out"):
        r = res[name]
        s = dict(r["summary"])
        s.update({"frames": r["frames"], "positions": r["positions"]})
        rep[name] = s
    return rep


# ----------------------------------------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m drba_amd.evaluate", description="PSNR / SSIM of finished clips")
    sub = p.add_subparsers(dest="command", required=True)
    c = sub.add_parser("compare", help="compare two clips frame by frame")
    c.add_argument("a")
    c.add_argument("b")
    c.add_argument("--json", dest="json_path", type=str, default=None, help="also write the report with the per-frame lists here")
    c.add_argument("--max-lsb", dest="max_lsb", type=float, default=None, help="gate: the largest difference allowed, in the clips' own steps (bytes, or 16-bit samples)")
    c.add_argument("--min-psnr", dest="min_psnr", type=float, default=None, help="gate: the lowest per-frame PSNR allowed")
    c.add_argument("--min-ssim", dest="min_ssim", type=float, default=None, help="gate: the lowest per-frame SSIM allowed")
    h = sub.add_parser("holdout", help="hold frames out of a clip and compare what the driver loop puts in their place")
    h.add_argument("-m", "--model_type", dest="model_type", type=str, default="rife")
    h.add_argument("-i", "--input", dest="input", type=str, required=True)
    h.add_argument("-k", dest="k", type=int, default=3, help="keep every k-th frame (odd, >= 3)")
    h.add_argument("-scale", "--scale", dest="scale", type=float, default=1.0)
    h.add_argument("-s", "--enable_scdet", dest="enable_scdet", action="store_true", default=False)
    h.add_argument("-st", "--scdet_threshold", dest="scdet_threshold", type=float, default=0.3)
    h.add_argument("--plain", action="store_true", help="plain inference_ts in place of every DRBA step (the baseline)")
    h.add_argument("--nonlinear", action="store_true", help="every DRBA step with the non-linear DistanceRatioMap (linear=False); not with --plain")
    h.add_argument("--deterministic", action="store_true", help="bit-reproducible run (infer.py --deterministic): the same clip and command give the same figures")
    h.add_argument("--weights", type=str, default=None, help="weight directory (default: the model's, synthetic if absent)")
    h.add_argument("--json", dest="json_path", type=str, default=None)
    return p.parse_args(argv)


def _write_json(path, rep, extra):
    if path:
        full = dict(rep)
        full.update(extra)
        with open(path, "w") as f:
            json.dump(_jsonable(full), f)


def main(argv=None, backend=None):
    args = parse_args(argv)
    try:
        if args.command == "compare":
            res = compare(ClipSource(args.a), ClipSource(args.b), backend=backend)
            rep, ok = compare_report(res, {"max_lsb": args.max_lsb, "min_psnr": args.min_psnr, "min_ssim": args.min_ssim},
                                     args.a, args.b)
            print(json.dumps(_jsonable(rep)))
            _write_json(args.json_path, rep, {"per_frame": res["per_frame"]})
            return 0 if ok else 1
        src = ClipSource(args.input)
        if not src.random_access:
            raise ValueError("a hold-out needs random access to the clip: use a .npz / .npy source")
        holdout_plan(len(src), args.k)  # refuse before a model is loaded
        if args.plain and args.nonlinear:
            raise ValueError("--nonlinear and --plain exclude each other: a plain step is inference_ts, it has no DistanceRatioMap to retime")
        from drba_amd import infer as drv
        from drba_amd import tune, tunecache
        tunecache.default_on()  # a command line: the conv autotuner's winners are kept across runs unless DRBA_TUNE_CACHE=0
        drv.apply_deterministic(args)
        wdir = args.weights or tune._default_weights(args.model_type)
        synthetic = args.weights is None and not (wdir and os.path.isdir(wdir))
        model = drv.load_model(args.model_type, scale=args.scale,
                               weights=tune._synthetic_weights(args.model_type) if synthetic else wdir)
        res = holdout(model, src._frames, args.k, fps=src.fps, enable_scdet=args.enable_scdet,
                      scdet_threshold=args.scdet_threshold, plain=args.plain, backend=backend, linear=not args.nonlinear,
                      **({"maxval": src.maxval} if src.depth == 16 else {}))
        rep = holdout_report(res)
        rep.update({"model": args.model_type, "scale": args.scale, "input": args.input,
                    "weights": "synthetic (drba_amd.utils.synth): the figures say nothing about quality" if synthetic else wdir})
        print(json.dumps(_jsonable(rep)))
        _write_json(args.json_path, rep, {"pairs": res["pairs"], "per_frame": {n: res[n]["per_frame"] for n in ("kept", "held_out")}})
        return 0
    except (ValueError, FileNotFoundError, RuntimeError) as e:
        print(f"evaluate {args.command}: {e}", file=sys.stderr)
        return 2


if __name__ == "__main__":
    sys.exit(main())
