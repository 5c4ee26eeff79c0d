"""Picture quality of finished clips, as commands.

    python -m drba_amd.evaluate compare A B [--json PATH] [--max-lsb N] [--min-psnr X] [--min-ssim X]
    python -m drba_amd.evaluate holdout -m rife -i CLIP [-k 3] [-scale 1.0] [-s] [-st 0.3] [--plain] [--nonlinear] [--deterministic]
                                        [--yuv-matrix bt709|bt601] [--yuv-range source|limited|full] [--fit resize|pad] [--weights DIR]
                                        [--dedup [--dedup-hi X] [--dedup-lo X] [--dedup-frac X] [--dedup-max N]] [--json PATH]
    python -m drba_amd.evaluate dups CLIP [-m rife] [-scale 1.0] [--fit resize|pad] [--dedup-hi X] [--dedup-lo X] [--dedup-frac X]
                                          [--dedup-max N] [--yuv-matrix bt709|bt601] [--yuv-range source|limited|full] [--json PATH]
    python -m drba_amd.evaluate bars CLIP [--crop-limit 0.094]

`compare` reads two clips frame by frame (the sources infer.py reads: .npz, .npy + .json, a .y4m stream -- below --, a container
when OpenCV is installed) and prints one JSON line: PSNR, ssim_matlab, the largest difference in LSB and the number of differing bytes, per
clip; `--json` adds the per-frame lists.  A gate that is given and violated makes the exit status 1, so "the outputs of two
builds agree within 1 LSB" is `compare a.npz b.npz --max-lsb 1`.

`holdout` measures what an interpolator is judged by: every K-th frame of a clip is kept, the driver loop of infer.py
(drba_amd.infer.interpolate_stream at `-t K`) fills the gaps, and every emission is compared with the original frame at its
position.  K is odd: an even K puts every emission half-way between two original frames.  `--plain` replaces each DRBA step by
plain inference_ts on the pair the timestep lies in -- the baseline DRBA's "preserves the original pace" is a claim against.

16-bit clips (uint16 frames; `maxval` from the .npz entry or the .json sidecar, 65535 when absent) are measured in their own
steps: the reports carry "depth": 16 and "maxval", the PSNR peak is maxval, `--max-lsb` counts 16-bit steps, and `holdout` emits
at 16 bits.  Two clips of different depth or maxval are refused.

YUV4MPEG2 clips (a `.y4m` path; `-` is a stream on stdin, for `compare` only: it cannot seek) are measured on the planes as they
stand in the stream, one frame in memory at a time, nothing converted: `compare a.y4m b.y4m` reports per frame and per clip the
PSNR of Y, of U and of V, `psnr` -- the squared error pooled over all samples of the three planes, the 4:1:1 weighting 4:2:0 has
by construction --, the single-channel 2-D SSIM of luma (drba_ssim2d: `ssim_matlab`'s window runs across three colour channels and
has no meaning on one plane), the largest difference in the clips' own steps and the differing samples; the peak is 255, or 1023
for C420p10.  `--max-lsb` gates max_lsb, `--min-psnr` the lowest per-frame pooled `psnr`, `--min-ssim` the lowest `ssim_y`; the
report carries "pixfmt": "yuv420", "depth" (8, or 16 for 10-bit samples, as tools.VideoFI_IO names them), "maxval", "chroma" (the C
tags of both sides: two 4:2:0 sitings may be compared, the samples are taken as they are) and "color_range".  Refused, both sides
named: different sizes, depths or XCOLORRANGE (no tag = limited), and a Y4M clip against an array clip.  `compare a.y4m b.y4m
--max-lsb 0` is the reproducibility gate of `infer.py --deterministic` on Y4M outputs.
A clip may be planar 4:2:2 or 4:4:4 (C422, C422p10, C444, C444p10): the per-plane figures use that layout's plane sizes, the report's
"pixfmt" names it ("yuv422", "yuv444"), and two clips of different layouts are refused, both C tags named.
`holdout -i clip.y4m` reads the kept frames through a random-access index of the file (one scan of the FRAME lines), converts
them on the device (`--yuv-matrix`, `--yuv-range` as in infer.py), emits packed Y, U, V planes at the clip's depth that stay on
the device, and compares each with the original's planes, uploaded when its turn comes: memory does not grow with the clip.
Kept frames pass through to_out(to_inp(frame)), which filters their chroma ("Pass-through frames"): their PSNR is
finite, and the report says so in "kept_passthrough".

`holdout --fit pad` pads the kept frames to the network size and crops the emissions (infer.py --fit pad) instead of resizing both
ways: the scores then carry no resampling loss, a kept frame of an array clip or the luma of an in-gamut Y4M one comes back as it
went in.  The report names the mode in "fit".

`dups` is how the thresholds of `infer.py --dedup` are picked for a noisy encode: for every source pair of a clip (.npz, .npy, .y4m) it
prints the duplicate statistic of the two network inputs -- `max_block`, `n_above / n_blocks` (drba_amd.ops.dup_stats; the frames are
converted as infer.py converts them for the model named by -m / -scale / --fit) -- and the decision, then the runs of repeats and how many
frames the filter keeps, and one JSON line with the kept indices.  `holdout --dedup` runs the hold-out with the filter on.

`bars` is what `infer.py --crop auto` does before it runs, as a command: for every frame of a clip (.npz, .npy, .y4m; `-` is a Y4M
stream on stdin) the box of its active picture as W:H:X:Y, or `empty` (drba_amd.crop: ffmpeg cropdetect's rule on the row and column
maxima, taken on the device -- of a planar clip, on luma), then the union over the clip as `crop=W:H:X:Y` -- the string `--crop` takes
-- and the share of the frame it covers.  The union is grown outward to the clip's own chroma alignment; a run whose sink has a
coarser layout validates the box again.

Non-finite JSON numbers are written as the strings "inf" / "-inf" / "nan" (float() reads them back).
"""
import argparse
import json
import math
import os
import sys

import numpy as np

from drba_amd import frames as _frames
from drba_amd import metrics


# ----------------------------------------------------------------------------------------------------------------- sources
class ClipSource:
    """The frames of a clip, opened the way tools.VideoFI_IO opens its input: .npz {frames, fps}, .npy (+ .json {"fps"}), anything
    else through cv2.VideoCapture when OpenCV is installed.  len() is None for a container (known when it has been read).
    A .y4m path, or `-` for stdin, is a YUV4MPEG2 clip (_open_y4m): .pixfmt is "yuv420" ("bgr" otherwise) and the frames are
    y4m.YuvFrames."""

    def __init__(self, path):
        self.path, self._frames, self._cap, self._y4m = path, None, None, None
        self.depth, self.maxval, self.pixfmt = 8, 255, "bgr"
        if path == "-":  # a YUV4MPEG2 stream on stdin: sequential only
            self._open_y4m(sys.stdin.buffer, seekable=False)
            return
        if not os.path.exists(path):
            raise FileNotFoundError(f"can't find the clip {path}")
        ext = os.path.splitext(path)[1].lower()
        maxval = None
        if ext == ".y4m":
            self._open_y4m(open(path, "rb"), seekable=True)
        elif ext in (".npz", ".npy"):
            self._frames, fps, maxval = _frames.open_array_clip(path)
            self.fps = 24.0 if fps is None else fps
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

    def _open_y4m(self, f, seekable):
        """A YUV4MPEG2 clip: frames are y4m.YuvFrames (planar 4:2:0, never converted here).  A seekable file is indexed in one scan of
        its FRAME lines (y4m.IndexedReader: len() and frame(k)); a pipe is read in order.  Either way one frame is in memory at a
        time.  depth / maxval as tools.VideoFI_IO names them: 8 / 255, or 16 / 1023 for C420p10."""
        from drba_amd import y4m
        self._y4m = y4m.IndexedReader(f, accept=y4m.ACCEPT_ALL) if seekable and f.seekable() else y4m.Reader(f, accept=y4m.ACCEPT_ALL)
        self._indexed = isinstance(self._y4m, y4m.IndexedReader)
        hdr = self.header = self._y4m.header
        self.layout, self.pixfmt = hdr.layout, "yuv" + hdr.layout  # "yuv420" | "yuv422" | "yuv444"
        self.fps = float(hdr.fps)
        self.size = (hdr.height, hdr.width)
        self.chroma, self.color_range = hdr.chroma, hdr.color_range
        if hdr.depth > 8:
            self.depth, self.maxval = 16, hdr.maxval

    def __len__(self):
        if self._y4m is not None and self._indexed:
            return len(self._y4m)
        if self._frames is None:
            raise TypeError("the length of a container or of a stream is known once it has been read")
        return len(self._frames)

    @property
    def random_access(self):
        return self._frames is not None or (self._y4m is not None and self._indexed)

    def frame(self, k):
        """frame k of a clip with random access: a contiguous array, or a y4m.YuvFrame read when it is asked for"""
        if self._y4m is not None and self._indexed:
            return self._y4m.read_frame(k)
        if self._frames is None:
            raise TypeError("this clip has no random access")
        return np.ascontiguousarray(self._frames[k])

    def __iter__(self):
        if self._y4m is not None:
            yield from self._y4m
            return
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
    are compared in their own steps, the peak being their maxval; clips of different depth or maxval are refused, both named.
    Two YUV4MPEG2 clips go to compare_yuv; one against an array clip is refused."""
    if any(getattr(c, "pixfmt", None) in _frames.YUV_PIXFMTS for c in (a, b)):
        return compare_yuv(a, b, backend=backend)
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


def _side(clip):
    """how a refusal names one side: the path and what it holds"""
    name = getattr(clip, "path", None) or type(clip).__name__
    if getattr(clip, "pixfmt", None) in _frames.YUV_PIXFMTS:
        h, w = clip.size
        bits = 10 if clip.depth == 16 else 8
        lay = _frames.YUV_PIXFMTS[clip.pixfmt]
        tag = "" if lay == "420" else f" C{clip.chroma},"  # (what a 4:2:0 refusal says is what it always said)
        return f"{name} (planar 4:{lay[1]}:{lay[2]},{tag} {w}x{h}, {bits}-bit, XCOLORRANGE={clip.color_range or 'none'})"
    return f"{name} (packed BGR frames)"


def compare_yuv(a, b, backend=None):
    """compare for two YUV4MPEG2 clips (ClipSources of .y4m paths or stdin), plane by plane on the samples as they stand in the
    streams -- nothing is converted --: metrics.YuvClipMetrics' figures (PSNR of Y, U, V and of the three planes pooled, the 2-D
    SSIM of luma, the largest difference in the clips' own steps, differing samples) plus "pixfmt", "depth", "maxval", "chroma" (the
    C tags of the two sides; different 4:2:0 sitings are allowed, the samples are compared as they are) and "color_range".
    ValueError naming both sides: a Y4M clip against an array clip, different frame sizes, depths or XCOLORRANGE (a stream
    without the tag is limited range, as infer.py reads it), different lengths."""
    ya, yb = getattr(a, "pixfmt", None) in _frames.YUV_PIXFMTS, getattr(b, "pixfmt", None) in _frames.YUV_PIXFMTS
    if not (ya and yb):
        raise ValueError(f"one clip is YUV4MPEG2 and the other is not: {_side(a)} against {_side(b)}; convert one of them first")
    if a.pixfmt != b.pixfmt:
        raise ValueError(f"the clips differ in chroma layout: C{a.chroma or '420jpeg'} against C{b.chroma or '420jpeg'} "
                         f"({_side(a)} against {_side(b)}); convert one of them first")
    if tuple(a.size) != tuple(b.size):
        raise ValueError(f"the clips differ in frame size: {_side(a)} against {_side(b)}")
    if (a.depth, a.maxval) != (b.depth, b.maxval):
        raise ValueError(f"the clips differ in depth: {_side(a)} against {_side(b)}; convert one of them first")
    if (a.color_range or "LIMITED") != (b.color_range or "LIMITED"):
        raise ValueError(f"the clips differ in sample range: {_side(a)} against {_side(b)}; convert one of them first")
    if a.random_access and b.random_access and len(a) != len(b):
        raise ValueError(f"the clips differ in length: {len(a)} frames of {a.path} against {len(b)} of {b.path}")
    cm = metrics.YuvClipMetrics(backend=backend, maxval=a.maxval)
    ia, ib = iter(a), iter(b)
    na = nb = 0
    while True:
        fa, fb = next(ia, None), next(ib, None)
        na, nb = na + (fa is not None), nb + (fb is not None)
        if fa is None or fb is None:
            if fa is not None or fb is not None:  # a stream ended early: count the rest of the longer one
                na += sum(1 for _ in ia)
                nb += sum(1 for _ in ib)
                raise ValueError(f"the clips differ in length: {na} frames of {a.path} against {nb} of {b.path}")
            break
        cm.add(fa, fb)
    res = cm.result()
    res.update({"size": [int(a.size[0]), int(a.size[1])], "pixfmt": a.pixfmt, "depth": a.depth, "maxval": int(a.maxval),
                "chroma": [a.chroma, b.chroma], "color_range": a.color_range or b.color_range})
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
    if res.get("pixfmt") in _frames.YUV_PIXFMTS:  # YUV4MPEG2 clips: the summary above already carries the per-plane figures
        rep.update({"pixfmt": res["pixfmt"], "chroma": res["chroma"], "color_range": res["color_range"]})
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


KEPT_PASSTHROUGH = "to_out(to_inp(frame))"  # what a kept frame of a YUV4MPEG2 hold-out is: converted in and out, chroma filtered


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


def _frame_at(frames, p):
    """frame p of an indexable array of frames, or of a ClipSource with random access (a YUV4MPEG2 clip: read now, not kept)"""
    return frames.frame(p) if hasattr(frames, "frame") else np.ascontiguousarray(frames[p])


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
        return _frame_at(self.frames, (self.i - 1) * self.k)

    def write_frame(self, x):
        j, p = self.j, self.j - self.half
        self.j += 1
        if p < 0 or p > self.m * self.k:
            self.skipped.append(j)  # the copies the run emits before the first and after the last frame: no original there
            return
        (self.kept if p % self.k == 0 else self.held).add(x, _frame_at(self.frames, p))
        self.pairs.append((j, p))


def holdout(model, frames, k=3, fps=24.0, enable_scdet=False, scdet_threshold=0.3, plain=False, backend=None, to_inp=None,
            to_out=None, check_scene=None, maxval=None, linear=True, yuv_matrix="bt709", yuv_range="source", fit="resize", dedup=None,
            check_dup=None):
    """Keep every k-th frame of `frames` (uint8 [N,H,W,3], indexable, or a ClipSource with random access), let interpolate_stream fill the gaps at `times = k`
    and compare every emission with the original frame at its position.  -> {"k", "m", "frames_used", "emissions",
    "pairs": [(emission, original)], "kept": ClipMetrics.result() + "positions", "held_out": the same}.
    to_inp / to_out / check_scene / backend: the hooks of interpolate_stream and of drba_amd.metrics (defaults: the device
    ones, with the emitted frames staying on the device).
    uint16 frames (samples in [0, maxval], 65535 unless given): the default hooks read and emit 16 bits at that maxval and the
    emissions are compared with the 16-bit originals in their own steps; the result carries "depth": 16 and "maxval".
    linear=False: every DRBA step of the run with the non-linear DistanceRatioMap (infer.py --nonlinear); not together with
    `plain`, whose steps have no DistanceRatioMap at all.  The result carries "linear".
    A YUV4MPEG2 clip (`frames` a ClipSource of a seekable .y4m file): the kept frames are read through its random-access reader and
    given to the model as y4m.YuvFrames (tools.to_inp converts on the device, `yuv_matrix` / `yuv_range` as in infer.py); every
    emission leaves as packed Y, U, V planes (ops.to_out_yuv, on the device) and is compared plane by plane
    (metrics.YuvClipMetrics) with the original's planes, read and uploaded when its turn comes -- nothing is stored, memory does
    not grow with the clip.  The kept frames pass through to_out(to_inp(frame)): their chroma is interpolated up and averaged
    down again ("Pass-through frames"), so unlike those of an array clip they do not come back identical and
    their PSNR is finite; the result says so in "kept_passthrough", beside "pixfmt", "depth" and "maxval".
    fit="pad": the default hooks pad the frames to the network size and crop the emissions instead of resizing both ways (infer.py
    --fit pad), so the figures carry no resampling loss; hooks that are given are the caller's.  The result carries "fit".
    dedup / check_dup: interpolate_stream's (infer.py --dedup) -- repeats among the KEPT frames are dropped and the steps retimed; the
    emissions and what they are compared with stay the same.  The result carries "dedup_kept", the kept indices among the kept frames."""
    from drba_amd import infer as drv
    if fit not in ("resize", "pad"):
        raise ValueError(f"fit must be resize or pad, got {fit!r}")
    if plain and not linear:
        raise ValueError("--nonlinear and --plain exclude each other: a plain step is inference_ts, it has no DistanceRatioMap to retime")
    m, half = holdout_plan(len(frames), k)
    fmt = _frames.source_format(frames, maxval, yuv_matrix, yuv_range)  # (refuses a maxval given for frames that are not uint16)
    yuv = fmt.pixfmt in _frames.YUV_PIXFMTS
    deep = not yuv and fmt.depth == 16
    mv = fmt.maxval if yuv or deep else None
    device_out = to_out is None
    # the emissions are what the clip's frames are -- uint8, uint16 or packed planes at the clip's own depth -- and by default stay on
    # the device, where they are compared
    inp, out = _frames.hooks(fmt, fmt, fit, on_device=True)
    to_inp, to_out = to_inp or inp, to_out or out
    backend = backend or metrics.default_backend()
    if yuv:
        kept, held = metrics.YuvClipMetrics(backend=backend, maxval=mv), metrics.YuvClipMetrics(backend=backend, maxval=mv)
    else:
        kept, held = metrics.ClipMetrics(backend=backend, maxval=mv), metrics.ClipMetrics(backend=backend, maxval=mv)
    io = _HoldoutIO(frames, int(k), m, half, fps, kept, held)
    run = PlainSteps(model) if plain else model
    dedup_kept = []
    written = drv.interpolate_stream(run, io, float(fps) * int(k), times=int(k), enable_scdet=enable_scdet,
                                     scdet_threshold=scdet_threshold, to_inp=to_inp, to_out=to_out, check_scene=check_scene,
                                     linear=bool(linear), dedup=dedup, check_dup=check_dup, on_kept=dedup_kept.append)
    if written != int(k) * (m + 1) or len(io.skipped) != 2 * half:
        raise RuntimeError(f"hold-out at k = {k}: the run emitted {written} frames ({len(io.skipped)} without an original), "
                           f"expected {int(k) * (m + 1)} ({2 * half})")
    out = {"k": int(k), "m": m, "frames_used": m * int(k) + 1, "emissions": written, "plain": bool(plain), "linear": bool(linear),
           "fit": fit, "pairs": io.pairs}
    if dedup:
        out["dedup_kept"] = dedup_kept
    if deep:
        out.update({"depth": 16, "maxval": mv})
    if yuv:
        out.update({"pixfmt": fmt.pixfmt, "depth": frames.depth, "maxval": mv, "chroma": frames.chroma, "yuv_matrix": yuv_matrix,
                    "full_range": fmt.full_range, "kept_passthrough": KEPT_PASSTHROUGH})
    for name, cm in (("kept", kept), ("held_out", held)):
        res = cm.result()  # (has waited for every kernel behind the frames)
        res["positions"] = [p for _, p in io.pairs if (p % int(k) == 0) == (name == "kept")]
        out[name] = res
    if device_out:
        from drba_amd import ops
        ops.check_overflow()  # what tools.to_out asks per frame: an overflow of the two-term fp16 kernels raises
    return out


def holdout_report(res):
    """The JSON object of `holdout` without the per-frame lists."""
    rep = {"command": "holdout", "k": res["k"], "m": res["m"], "frames_used": res["frames_used"], "emissions": res["emissions"],
           "plain": res["plain"], "linear": res["linear"], "fit": res.get("fit", "resize")}
    if "depth" in res:
        rep.update({"depth": res["depth"], "maxval": res["maxval"]})
    if "dedup_kept" in res:
        rep["dedup_kept"] = res["dedup_kept"]
    if res.get("pixfmt") in _frames.YUV_PIXFMTS:
        rep.update({k: res[k] for k in ("pixfmt", "chroma", "yuv_matrix", "full_range", "kept_passthrough")})
    for name in ("kept", "held_out"):
        r = res[name]
        s = dict(r["summary"])
        s.update({"frames": r["frames"], "positions": r["positions"]})
        rep[name] = s
    return rep


# ----------------------------------------------------------------------------------------------------------------- repeats
PAD_SIZE = {"rife": 64, "gmfss": 64, "gmfss_union": 128}  # the models' pad_size: the network size follows from it without loading one


def dups(src, settings=None, model_type="rife", scale=1.0, fit="resize", yuv_matrix="bt709", yuv_range="source", stats=None, to_inp=None,
         out=None):
    """The duplicate statistic of every source pair of a ClipSource, on the network inputs infer.py would make for the model, and what
    the --dedup filter does with them.  Prints one line per pair and the runs of repeats to `out` (None: nothing); -> {"pairs":
    [{"pair", "max_block", "n_above", "n_blocks", "dup"}], "runs": [[first repeated frame, length]], "kept": [...], "frames"}.
    stats(a, b, lo) -> (max_block, n_above, n_blocks) and to_inp(frame, size): the device's unless given."""
    from drba_amd import dedup as _dedup
    from drba_amd.models.utils import tools
    s = settings or _dedup.Settings()
    if model_type not in PAD_SIZE:
        raise ValueError(f"model_type must be one of {sorted(PAD_SIZE)}, got {model_type!r}")
    if stats is None:
        from drba_amd import ops
        stats = ops.dup_stats
    if to_inp is None:
        fmt = _frames.source_format(src, yuv_matrix=yuv_matrix, yuv_range=yuv_range)
        to_inp, _ = _frames.hooks(fmt, fmt, fit)
    pairs, prev, size = [], None, None
    for k, fr in enumerate(src):
        if size is None:
            size = tools.get_valid_net_inp_size(fr, scale, div=PAD_SIZE[model_type])["dst_size"]
        x = to_inp(fr, size)
        if prev is not None:
            mx, na, nb = stats(prev, x, s.lo)
            d = bool(_dedup.is_dup(mx, na, nb, hi=s.hi, frac=s.frac))
            pairs.append({"pair": [k - 1, k], "max_block": mx, "n_above": na, "n_blocks": nb, "dup": d})
            if out is not None:
                print(f"{k - 1:6d} -> {k:<6d} max_block {mx:.5f} ({mx * 255:6.2f}/255)  n_above {na} / {nb} ({na / nb:.3f})  "
                      f"{'repeat' if d else 'new'}", file=out)
        prev = x
    n = len(pairs) + 1 if prev is not None else 0
    kept = _dedup.kept_indices([p["dup"] for p in pairs], s.max_run) if n else []
    runs, k = [], 1
    while k < n:
        if pairs[k - 1]["dup"]:
            j = k
            while j < n and pairs[j - 1]["dup"]:
                j += 1
            runs.append([k, j - k])
            k = j
        else:
            k += 1
    if out is not None:
        for first, length in runs:
            print(f"frames {first} .. {first + length - 1}: {length} repeat{'s' if length > 1 else ''} of frame {first - 1}"
                  + (f" (at most {s.max_run} in a row are dropped)" if length > s.max_run else ""), file=out)
        print(f"{len(kept)} of {n} frames kept (hi {s.hi:.5f}, lo {s.lo:.5f}, frac {s.frac}, max {s.max_run})", file=out)
    return {"pairs": pairs, "runs": runs, "kept": kept, "frames": n}


# ----------------------------------------------------------------------------------------------------------------- bars
def bars(src, limit=None, stat=None, out=None):
    """The active picture of every frame of a ClipSource and of the clip (drba_amd.crop).  Prints one line per frame -- its box as
    W:H:X:Y, or `empty` -- then `crop=W:H:X:Y` of the union, grown outward to the clip's chroma alignment, and the share of the frame
    it covers, to `out` (None: nothing); -> {"boxes": [str | None], "crop": str | None, "share": float | None, "frames", "size"}.
    stat(frame) -> (row_max, col_max): the device's (ops.edge_max) unless given."""
    from drba_amd import crop as _crop
    limit = _crop.LIMIT if limit is None else limit
    sized, boxes = _crop._sized(src), []
    for k, box in enumerate(_crop.frame_boxes(sized, limit, stat)):
        boxes.append(box)
        if out is not None:
            print(f"{k:6d} {'empty' if box is None else box}", file=out)
    u = _crop.union(boxes)
    if u is not None:
        u = _crop.aligned(u, sized.size, _crop.alignment_of(getattr(src, "pixfmt", "bgr")))
    share = None if u is None else u.w * u.h / float(sized.size[0] * sized.size[1])
    if out is not None:
        if u is None:
            print(f"no picture above the limit in {len(boxes)} frames: nothing to crop", file=out)
        else:
            print(f"crop={u}  {100.0 * share:.1f}% of the {sized.size[1]}x{sized.size[0]} frame"
                  + ("  (the whole frame: nothing to crop)" if _crop.whole(u, sized.size) else ""), file=out)
    return {"boxes": [None if b is None else str(b) for b in boxes], "crop": None if u is None else str(u), "share": share,
            "frames": len(boxes), "size": None if sized.size is None else list(sized.size)}


# ----------------------------------------------------------------------------------------------------------------- command line
def _dedup_flags(p):
    from drba_amd import dedup as _dedup
    p.add_argument("--dedup-hi", dest="dedup_hi", type=float, default=_dedup.HI, help="as in infer.py (default 12/255)")
    p.add_argument("--dedup-lo", dest="dedup_lo", type=float, default=_dedup.LO, help="as in infer.py (default 5/255)")
    p.add_argument("--dedup-frac", dest="dedup_frac", type=float, default=_dedup.FRAC, help="as in infer.py (default 0.33)")
    p.add_argument("--dedup-max", dest="dedup_max", type=int, default=_dedup.MAX_RUN, help="as in infer.py (default 3)")


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
    h.add_argument("--yuv-matrix", dest="yuv_matrix", type=str, default="bt709", choices=("bt709", "bt601"),
                   help="YCbCr matrix of a .y4m clip (default bt709), as in infer.py")
    h.add_argument("--yuv-range", dest="yuv_range", type=str, default="source", choices=("source", "limited", "full"),
                   help="sample range of a .y4m clip: the header's XCOLORRANGE (default; limited when it has none) or the one named, as in infer.py")
    h.add_argument("--fit", dest="fit", type=str, default="resize", choices=("resize", "pad"),
                   help="how a frame gets to the network size and back, as in infer.py: resize (default) or pad (no resampling)")
    h.add_argument("--weights", type=str, default=None, help="weight directory (default: the model's, synthetic if absent)")
    h.add_argument("--dedup", action="store_true", help="drop repeated frames among the kept ones and retime the steps (infer.py --dedup)")
    _dedup_flags(h)
    h.add_argument("--json", dest="json_path", type=str, default=None)
    d = sub.add_parser("dups", help="the duplicate statistic of every source pair of a clip and what --dedup does with it")
    d.add_argument("clip")
    d.add_argument("-m", "--model_type", dest="model_type", type=str, default="rife", help="the model whose network size the frames are brought to")
    d.add_argument("-scale", "--scale", dest="scale", type=float, default=1.0)
    d.add_argument("--fit", dest="fit", type=str, default="resize", choices=("resize", "pad"))
    d.add_argument("--yuv-matrix", dest="yuv_matrix", type=str, default="bt709", choices=("bt709", "bt601"))
    d.add_argument("--yuv-range", dest="yuv_range", type=str, default="source", choices=("source", "limited", "full"))
    _dedup_flags(d)
    d.add_argument("--json", dest="json_path", type=str, default=None)
    b = sub.add_parser("bars", help="the active picture of every frame of a clip and the box `infer.py --crop` takes")
    b.add_argument("clip")
    b.add_argument("--crop-limit", dest="crop_limit", type=float, default=None,
                   help="a row or column is picture when a sample of it exceeds this, on the [0, 1] scale (default 24/255, as in infer.py)")
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
        if args.command == "dups":
            from drba_amd import dedup as _dedup
            res = dups(ClipSource(args.clip), _dedup.Settings(args.dedup_hi, args.dedup_lo, args.dedup_frac, args.dedup_max), args.model_type,
                       args.scale, args.fit, args.yuv_matrix, args.yuv_range, out=sys.stdout)
            rep = {"command": "dups", "input": args.clip, "frames": res["frames"], "kept": res["kept"], "runs": res["runs"]}
            print(json.dumps(_jsonable(rep)))
            _write_json(args.json_path, rep, {"pairs": res["pairs"]})
            return 0
        if args.command == "bars":
            bars(ClipSource(args.clip), args.crop_limit, out=sys.stdout)
            return 0
        src = ClipSource(args.input)
        if not src.random_access:
            raise ValueError("a hold-out needs random access to the clip: use a .npz / .npy source"
                             + (" or a seekable .y4m file" if src.pixfmt in _frames.YUV_PIXFMTS else ""))
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
        # (the clip itself says what its frames are -- depth, maxval, 4:2:0 --: frames.source_format, which holdout asks)
        res = holdout(model, src, args.k, fps=src.fps, enable_scdet=args.enable_scdet, scdet_threshold=args.scdet_threshold,
                      plain=args.plain, backend=backend, linear=not args.nonlinear, fit=args.fit, dedup=drv.dedup_of(args),
                      yuv_matrix=args.yuv_matrix, yuv_range=args.yuv_range)
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
