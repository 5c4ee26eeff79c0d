"""What the driver knows about a clip's frames, and the two hooks built from it.

`FrameFormat` describes one end of a run; `hooks` turns the two ends' formats and `--fit` into the `to_inp(frame, size)` /
`to_out(x, size)` pair `infer.interpolate_stream` takes.  infer.inference, infer.inference_sharded, evaluate.holdout and evaluate.dups
get their hooks here, so a new frame property (another chroma layout, a transfer function, an alpha plane) is a field of `FrameFormat`,
a line in `inp_keywords` / `out_keywords`, and whoever fills the field in (tools.VideoFI_IO, source_format).

`hooks(..., crop=box)` (--crop) adds `window` to both keyword sets; without a box nothing is added.

The rule of the keyword sets: A DEFAULT IS LEFT OUT.  A plain 8-bit BGR resize run calls tools.to_inp(frame, size) and
tools.to_out(x, size) with no keyword at all, as the reference does, and every keyword appears only for the frames that need it
(two exceptions are kept as they always were: a 16-bit BGR sink names `rgb` even when it is False, and a planar sink names all five
of its keywords).  Stand-ins with closed signatures rely on it.  The chroma layout follows the rule: a 4:2:0 end says nothing about
it, a 4:2:2 or 4:4:4 sink says `pixfmt="yuv422"` / `"yuv444"` to tools.to_out and `layout="422"` / `"444"` to ops.to_out_yuv; a source
frame (y4m.YuvFrame) carries its own layout.

Nothing here touches the GPU, and nothing that does is imported when the module is loaded.
"""
import json
import os
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class FrameFormat:
    """One end of a run.  depth 8 | 16 is the sample type (uint8 | uint16; a 10-bit planar clip is depth 16 with maxval 1023),
    maxval the largest sample (255 at depth 8); matrix / full_range name the YCbCr conversion of a planar end, whose chroma layout
    the pixfmt names; rgb (a sink only): the sink takes RGB order, not BGR."""
    pixfmt: str = "bgr"  # "bgr" | "yuv420" | "yuv422" | "yuv444"
    depth: int = 8
    maxval: int = 255
    matrix: str = "bt709"
    full_range: bool = False
    rgb: bool = False


YUV_PIXFMTS = {"yuv420": "420", "yuv422": "422", "yuv444": "444"}  # a planar pixfmt -> its chroma layout (y4m.LAYOUTS)


def open_array_clip(path):
    """-> (frames, fps or None, maxval or None) of a .npz {frames, fps, maxval} or a .npy (memory-mapped) + .json sidecar {"fps",
    "maxval"}.  The defaults and the checks are the caller's."""
    if os.path.splitext(path)[1].lower() == ".npz":
        z = np.load(path)
        frames, meta = z["frames"], {k: z[k] for k in ("fps", "maxval") if k in z.files}
    else:
        frames = np.load(path, mmap_mode="r")
        side = os.path.splitext(path)[0] + ".json"
        meta = json.load(open(side)) if os.path.exists(side) else {}
    return frames, (float(meta["fps"]) if "fps" in meta else None), (int(meta["maxval"]) if "maxval" in meta else None)


def full_range(yuv_range, tag, tag_wins):
    """Is a 4:2:0 clip full range?  yuv_range: --yuv-range (source | limited | full); tag: the stream header's XCOLORRANGE ("FULL" |
    "LIMITED" | None).  With `source` the tag decides, and a clip without one is limited.  When the flag names a range AND the header
    carries a tag, the callers differ: tools.VideoFI_IO (infer.py) reads the clip by its tag (tag_wins=True), evaluate's holdout and
    dups by the flag (tag_wins=False)."""
    if yuv_range not in ("source", "limited", "full"):
        raise ValueError(f"yuv_range must be source, limited or full, got {yuv_range!r}")
    if tag is not None and (tag_wins or yuv_range == "source"):
        return tag == "FULL"
    return yuv_range == "full"


def source_format(clip, maxval=None, yuv_matrix="bt709", yuv_range="source"):
    """The format of what evaluate reads: an evaluate.ClipSource (array clip or YUV4MPEG2), or a bare [N,H,W,3] array, whose
    `maxval` (65535 unless given) belongs to uint16 frames only."""
    if getattr(clip, "pixfmt", None) in YUV_PIXFMTS:
        if maxval is not None:
            raise ValueError("maxval belongs to uint16 frames")
        return FrameFormat(clip.pixfmt, clip.depth, int(clip.maxval), yuv_matrix, full_range(yuv_range, clip.color_range, tag_wins=False))
    if getattr(clip, "depth", 16 if getattr(clip, "dtype", None) == np.uint16 else 8) != 16:
        if maxval is not None:
            raise ValueError("maxval belongs to uint16 frames")
        return FrameFormat()
    return FrameFormat(depth=16, maxval=int(getattr(clip, "maxval", 65535) if maxval is None else maxval))


def _fit_keywords(fit):
    if fit not in ("resize", "pad"):
        raise ValueError(f"fit must be resize or pad, got {fit!r}")
    return {} if fit == "resize" else {"fit": fit}


def inp_keywords(fmt, fit):
    """What tools.to_inp is told about a source frame.  A planar frame (y4m.YuvFrame) carries its own depth, maxval and layout."""
    if fmt.pixfmt in YUV_PIXFMTS:
        return {"matrix": fmt.matrix, "full_range": fmt.full_range, **_fit_keywords(fit)}
    if fmt.depth == 16:
        return {"maxval": fmt.maxval, **_fit_keywords(fit)}
    return _fit_keywords(fit)


def out_keywords(fmt, fit, on_device=False):
    """What tools.to_out is told about the sink's frames; on_device: what ops.to_out -- ops.to_out_yuv for a planar sink -- is told
    (the frame stays on the device: no `rgb`, and the entry says the pixel format; a layout other than 4:2:0 is named)."""
    mv = fmt.maxval if fmt.depth == 16 else None
    if fmt.pixfmt in YUV_PIXFMTS:
        kw = {"matrix": fmt.matrix, "full_range": fmt.full_range, "depth": fmt.depth, "maxval": mv}
        layout = YUV_PIXFMTS[fmt.pixfmt]
        said = ({} if layout == "420" else {"layout": layout}) if on_device else {"pixfmt": fmt.pixfmt}
        return {**kw, **said, **_fit_keywords(fit)}
    if fmt.depth == 16:
        return {**({} if on_device else {"rgb": fmt.rgb}), "depth": 16, "maxval": mv, **_fit_keywords(fit)}
    return {**({"rgb": True} if fmt.rgb and not on_device else {}), **_fit_keywords(fit)}


def _crop_keywords(crop):
    """--crop: the box (drba_amd.crop.Box, or anything with .window = (x, y, w, h)) as the `window` keyword; no box, no keyword"""
    return {} if crop is None else {"window": tuple(int(v) for v in crop.window)}


def hooks(src_format, sink_format, fit, on_device=False, crop=None):
    """-> (to_inp, to_out) for interpolate_stream: tools.to_inp / tools.to_out with the keywords of the two formats (looked up on
    the module at every call: a test may replace them).  on_device: to_out leaves the finished frame on the device (ops.to_out /
    ops.to_out_yuv) -- what a hold-out compares there and a frame-sharded run gathers from there.
    crop (--crop; a drba_amd.crop.Box): both hooks name `window`: to_inp reads that rectangle of the source frame, to_out writes it
    into a frame of the size it is given -- the source's -- whose remainder is black.  The sizes stay the caller's: interpolate_stream
    computes the network size from the box (its `crop`) and hands to_out the frame size."""
    from drba_amd.models.utils import tools
    win = _crop_keywords(crop)
    kin, kout = {**inp_keywords(src_format, fit), **win}, {**out_keywords(sink_format, fit, on_device), **win}

    def to_inp(frame, size):
        return tools.to_inp(frame, size, **kin)

    where, entry = tools, "to_out"
    if on_device:
        from drba_amd import ops as where
        entry = "to_out_yuv" if sink_format.pixfmt in YUV_PIXFMTS else "to_out"

    def to_out(x, size):
        return getattr(where, entry)(x, size, **kout)

    return to_inp, to_out
