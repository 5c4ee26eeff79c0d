"""--crop: the active picture of a clip with letterbox / pillarbox bars, as a box the frame hooks read and write a window by.

A `Box` is ffmpeg's crop=W:H:X:Y.  One frame's box follows from the statistic `ops.edge_max` (active_area.hip; `edge_max_numpy` is
its numpy reference): the largest sample of every row and of every pixel column.  A row or column is PICTURE when its maximum exceeds
`threshold = floor(limit * maxval)` (ffmpeg cropdetect's rule; `--crop-limit`, 24/255 by default, on the [0, 1] scale), and the box
runs from the first to the last such row and column; a frame with no sample above the threshold is EMPTY and has no box.  A clip's
box is the union over its frames, grown OUTWARD to the chroma alignment of the two ends and clamped to the frame: never rounded
into the picture.  `scan` does that for a whole clip, on the device; everything else here is host arithmetic.

Nothing here touches the GPU when the module is loaded.
"""
import math
from dataclasses import dataclass

import numpy as np

LIMIT = 24.0 / 255.0  # cropdetect's default limit, on the [0, 1] scale

_SUBSAMPLING = {"bgr": (1, 1), "yuv420": (2, 2), "yuv422": (2, 1), "yuv444": (1, 1)}  # pixfmt -> (horizontal, vertical)


@dataclass(frozen=True)
class Box:
    """crop=W:H:X:Y, ffmpeg's order: a w x h rectangle whose top-left pixel is (x, y)."""
    w: int
    h: int
    x: int
    y: int

    @property
    def window(self):
        """(x, y, w, h): the `window` keyword of the frame conversions"""
        return (self.x, self.y, self.w, self.h)

    @property
    def size(self):
        """(h, w): what the network size is computed from"""
        return (self.h, self.w)

    def __str__(self):
        return f"{self.w}:{self.h}:{self.x}:{self.y}"

    def contains(self, other):
        return (self.x <= other.x and self.y <= other.y and self.x + self.w >= other.x + other.w and
                self.y + self.h >= other.y + other.h)

    def inside(self, frame_size):
        fh, fw = int(frame_size[0]), int(frame_size[1])
        return self.x >= 0 and self.y >= 0 and self.w >= 1 and self.h >= 1 and self.x + self.w <= fw and self.y + self.h <= fh


def parse(text, frame_size=None):
    """"W:H:X:Y" -> Box; a leading "crop=" is accepted, so a line of `ffmpeg -vf cropdetect` pastes in.  ValueError for anything but four
    non-negative integers with W, H >= 1, and -- frame_size = (H, W) given -- for a box that does not lie inside the frame."""
    s = str(text).strip()
    if s.startswith("crop="):
        s = s[len("crop="):]
    parts = s.split(":")
    if len(parts) != 4 or not all(p.isascii() and p.isdigit() for p in parts):
        raise ValueError(f"a crop box is W:H:X:Y, four non-negative integers (ffmpeg's crop=), got {text!r}")
    w, h, x, y = (int(p) for p in parts)
    if w < 1 or h < 1:
        raise ValueError(f"a crop box needs W, H >= 1, got {text!r}")
    box = Box(w, h, x, y)
    if frame_size is not None and not box.inside(frame_size):
        raise ValueError(f"the crop box {box} does not lie inside the {int(frame_size[1])}x{int(frame_size[0])} frame")
    return box


def threshold_of(limit, maxval):
    """floor(limit * maxval): samples ABOVE it are picture (24 of 255 at the default limit, 96 of 1023)"""
    if not 0.0 <= float(limit) < 1.0:
        raise ValueError(f"--crop-limit is a fraction of the sample range, 0 <= limit < 1, got {limit!r}")
    return int(math.floor(float(limit) * int(maxval) + 1e-9))


def box_of(row_max, col_max, threshold):
    """The box of one frame from its row and column maxima: first to last row / column whose maximum is > threshold; None for an
    empty frame (no sample above the threshold)."""
    rows = np.flatnonzero(np.asarray(row_max).astype(np.int64) > int(threshold))
    cols = np.flatnonzero(np.asarray(col_max).astype(np.int64) > int(threshold))
    if rows.size == 0 or cols.size == 0:
        return None
    return Box(int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1), int(cols[0]), int(rows[0]))


def union(boxes):
    """The smallest box holding every box of `boxes`; empty frames (None) are ignored, all empty -> None."""
    boxes = [b for b in boxes if b is not None]
    if not boxes:
        return None
    x0, y0 = min(b.x for b in boxes), min(b.y for b in boxes)
    x1, y1 = max(b.x + b.w for b in boxes), max(b.y + b.h for b in boxes)
    return Box(x1 - x0, y1 - y0, x0, y0)


def alignment_of(*formats):
    """(ax, ay) a box must be aligned to for frames of these formats (frames.FrameFormat, or pixfmt names): per axis the larger chroma
    subsampling -- 2, 2 for 4:2:0, 2, 1 for 4:2:2, 1, 1 for 4:4:4 and packed frames."""
    subs = [_SUBSAMPLING[getattr(f, "pixfmt", f)] for f in formats]
    return max(s[0] for s in subs), max(s[1] for s in subs)


def aligned(box, frame_size, align):
    """`box` grown OUTWARD to multiples of align = (ax, ay) and clamped to the frame (H, W): the result always contains the box, and
    its far edges are aligned unless they are the frame's own (an odd frame edge)."""
    fh, fw = int(frame_size[0]), int(frame_size[1])
    ax, ay = int(align[0]), int(align[1])
    x0, y0 = (box.x // ax) * ax, (box.y // ay) * ay
    x1, y1 = min(-(-(box.x + box.w) // ax) * ax, fw), min(-(-(box.y + box.h) // ay) * ay, fh)
    return Box(x1 - x0, y1 - y0, x0, y0)


def validate(box, frame_size, align):
    """An explicit box is trusted, but it must be usable: inside the frame, x, y multiples of the alignment, w, h too unless the box
    reaches the frame's right / bottom edge.  ValueError names the required multiple."""
    fh, fw = int(frame_size[0]), int(frame_size[1])
    if not box.inside(frame_size):
        raise ValueError(f"the crop box {box} does not lie inside the {fw}x{fh} frame")
    for name, at, ext, full, m in (("X and W", box.x, box.w, fw, int(align[0])), ("Y and H", box.y, box.h, fh, int(align[1]))):
        if at % m or (ext % m and at + ext != full):
            raise ValueError(f"the crop box {box}: {name} must be multiples of {m} for the chroma layout of these frames (the extent may "
                             f"be odd only where the box reaches the frame's edge); the aligned box is crop={aligned(box, frame_size, align)}")
    return box


def whole(box, frame_size):
    return box is not None and box.x == 0 and box.y == 0 and (box.h, box.w) == (int(frame_size[0]), int(frame_size[1]))


def edge_max_numpy(frame, group=None):
    """The reference of ops.edge_max: frame [H,W,c] (group c unless given) or a plane [rows,cols] (group 1) -> (row_max [rows],
    col_max [cols / group]) as int64 arrays."""
    a = np.asarray(frame)
    if a.ndim == 3:
        group = a.shape[2] if group is None else int(group)
        a = a.reshape(a.shape[0], -1)
    else:
        group = 1 if group is None else int(group)
    if a.ndim != 2 or a.shape[1] % group:
        raise ValueError(f"edge_max_numpy takes [H,W,c] or [rows,cols] with cols a multiple of group, got {np.asarray(frame).shape}")
    a = a.astype(np.int64)
    return a.max(axis=1), a.reshape(a.shape[0], -1, group).max(axis=(0, 2))


def _device_stat(device=None):
    """frame -> (row_max, col_max) on the device: a packed frame as it stands, of a planar one the luma plane only (only that plane
    is uploaded).  One frame ahead: the statistic of frame k is read while frame k + 1 is on its way."""
    import torch

    from drba_amd import ops
    device = ops.default_device() if device is None else device

    def enqueue(fr):
        if hasattr(fr, "planes"):  # y4m.YuvFrame
            t = torch.from_numpy(np.ascontiguousarray(fr.planes()[0])).to(device, non_blocking=True)
        else:
            t = torch.from_numpy(np.ascontiguousarray(fr)).to(device, non_blocking=True)
        return ops.edge_max_async(t)

    def collect(job):
        host, ev, rows = job
        ev.synchronize()
        a = host.numpy()
        return a[:rows], a[rows:]

    return enqueue, collect


def frame_boxes(source, limit=LIMIT, stat=None, device=None):
    """Yields the box (or None: empty) of every frame of `source`, an iterable of frames that knows its .maxval (evaluate.ClipSource;
    255 when it does not say).  stat(frame) -> (row_max, col_max) replaces the device (tests: edge_max_numpy on the frame or its luma)."""
    thr = threshold_of(limit, getattr(source, "maxval", 255))
    if stat is not None:
        for fr in source:
            yield box_of(*stat(fr), thr)
        return
    enqueue, collect = _device_stat(device)
    pending = None
    for fr in source:
        job = enqueue(fr)
        if pending is not None:
            yield box_of(*collect(pending), thr)
        pending = job
    if pending is not None:
        yield box_of(*collect(pending), thr)


def scan(source, limit=LIMIT, align=(1, 1), stat=None, device=None, on_frame=None):
    """The box of a clip: every frame of `source` (a path of a .npz / .npy / .y4m clip, or an evaluate.ClipSource) read once, the
    statistic on the device, the union of the frames' boxes grown outward to `align` and clamped to the frame.  None when every frame
    is empty or the box is the whole frame: there is nothing to crop.  on_frame(k, box) fires per frame."""
    if isinstance(source, str):
        from drba_amd.evaluate import ClipSource
        source = ClipSource(source)
    size, boxes = None, []
    src_iter = _sized(source)
    for k, box in enumerate(frame_boxes(src_iter, limit, stat, device)):
        boxes.append(box)
        if on_frame is not None:
            on_frame(k, box)
    size = src_iter.size
    u = union(boxes)
    if u is None or size is None:
        return None
    u = aligned(u, size, align)
    return None if whole(u, size) else u


class _sized:
    """An iterable of frames that remembers the frame size it saw (and refuses a clip whose size changes)."""

    def __init__(self, source):
        self.source, self.size = source, None
        self.maxval = getattr(source, "maxval", 255)

    def __iter__(self):
        for fr in self.source:
            s = (int(fr.shape[0]), int(fr.shape[1]))
            if self.size is None:
                self.size = s
            elif s != self.size:
                raise ValueError(f"the frame size changes inside the clip: {self.size} then {s}")
            yield fr
