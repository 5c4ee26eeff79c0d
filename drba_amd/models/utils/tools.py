"""Host-side utilities of the DRBA driver, same names as the reference's models/utils/tools.py.

Pure host logic (sizes, timestep mapping, weight-key conversion, frame IO) lives here in
Python like the reference.  Anything that touches pixels on the hot path (resize,
distance, scene check) dispatches to the HIP library through drba_amd.ops; there is no
CPU fallback in this module.
"""
import math
import weakref
import os
import subprocess
import sys
import threading
from queue import Queue

import numpy as np
import torch

from drba_amd import frames as _frames
from drba_amd import ops as _ops
from drba_amd import y4m as _y4m


def check_cupy_env():
    """The reference switches between a cupy/CUDA and a torch splat here (tools.py:14-24).
    This build has exactly one backend (the HIP library); there is no cupy path."""
    return False


# ----------------------------------------------------------------------------- sizes / conversion
def get_valid_net_inp_size(img, scale, div=64):
    """Network input size: each side rounded up so that side*scale is a multiple of `div`.
    How a frame gets to that size is to_inp's `fit`: resized to it (the default, as the reference does) or
    replicate-padded at the bottom and right (fit="pad"); the size is the same either way.  Float arithmetic
    then int(), as in reference tools.py:41-56, so 1080 -> 1088 (div 64), 1152 (div 128); 2160@0.5 -> 2176."""
    src_h, src_w = int(img.shape[0]), int(img.shape[1])

    def round_up(v):
        if v * scale % div != 0:
            return int((v * scale // div + 1) * div / scale)
        return v

    return {"src_size": (src_h, src_w), "dst_size": (round_up(src_h), round_up(src_w))}


def convert(param):
    """Keep only keys carrying the DataParallel 'module.' prefix, with it stripped (tools.py:83-88)."""
    return {k.replace("module.", ""): v for k, v in param.items() if "module." in k}


def load_weights(path):
    """torch.load of a checkpoint file the way the reference reads it (map_location='cpu': its shipped pickles carry CUDA-tagged
    storages) but with weights_only=True: a state dict of tensors unpickles, arbitrary code in a downloaded .pkl does not run
    (the reference's plain torch.load executes whatever the file holds, rife.py:19 / GMFSS.py:50-53)."""
    return torch.load(path, map_location="cpu", weights_only=True)


def _is_u16(img):
    return img.dtype == (torch.uint16 if torch.is_tensor(img) else np.uint16)


def _check_depth(depth, maxval):
    if depth not in (8, 16):
        raise ValueError(f"depth must be 8 or 16, got {depth!r}")
    if depth == 8 and maxval is not None:
        raise ValueError("maxval belongs to 16-bit frames (depth=16)")


def to_tensor(img, device=None, maxval=None):
    """uint8 HWC -> fp32 [1,3,H,W] in [0,1] on the GPU (tools.py:33-34).  Channel order is kept.  A uint16 frame is divided by
    `maxval` (65535 unless given) instead of 255."""
    device = _ops.default_device() if device is None else device
    t = torch.from_numpy(np.ascontiguousarray(img)).to(device, non_blocking=True)
    if _is_u16(t):
        return _ops.u16hwc_to_f32nchw(t, maxval)
    return _ops.u8hwc_to_f32nchw(t)


def to_cv2(img, depth=8, maxval=None):
    """fp32 [1,3,H,W] -> uint8 HWC with (x*255.) truncation, no clamp/round (tools.py:37-38).  depth=16: uint16 HWC, x * maxval
    rounded to nearest even and saturated (ops.to_out)."""
    _check_depth(depth, maxval)
    if depth == 16:
        return _ops.f32nchw_to_u16hwc(img, maxval).cpu().numpy()
    return _ops.f32nchw_to_u8hwc(img).cpu().numpy()


def resize(tensor, size):
    """Bilinear, align_corners=False, explicit output size (tools.py:71-72)."""
    return _ops.resize_bilinear(tensor, size)


def _fit_kw(fit):
    """`fit` as the ops entries take it; the default is left out, so a resize call is the call it always was"""
    if fit not in _ops.FITS:
        raise ValueError(f"fit must be one of {_ops.FITS}, got {fit!r}")
    return {} if fit == "resize" else {"fit": fit}


def _window_kw(window):
    """`window` as the ops entries take it; the default is left out, as `fit`"""
    return {} if window is None else {"window": tuple(int(v) for v in window)}


def to_inp(npInp, dst_size, device=None, maxval=None, matrix="bt709", full_range=False, fit="resize", window=None):
    """resize(to_tensor(npInp), dst_size) (tools.py:59-60) as one kernel on the uploaded uint8 frame (the full-size
    fp32 frame of the reference is never materialised); bit-exact with the two-step form.  A uint16 frame goes through the
    16-bit kernel with its `maxval` (65535 unless given).  A planar frame (y4m.YuvFrame: 4:2:0, 4:2:2 or 4:4:4) is uploaded as it
    stands -- half the bytes of a BGR frame at 4:2:0 -- and converted with `matrix` / `full_range` inside the kernel
    (ops.to_inp_yuv); the frame knows its own depth and layout.  fit="pad" (not in the reference): the frame is replicate-padded to `dst_size` at the bottom and right instead of
    resized (ops.to_inp).  window=(x, y, w, h) (--crop, not in the reference): the whole frame is uploaded as it stands and that
    rectangle of it is converted as if it were the frame (ops.to_inp / ops.to_inp_yuv: no copy in between)."""
    fit_kw = {**_fit_kw(fit), **_window_kw(window)}
    device = _ops.default_device() if device is None else device
    if isinstance(npInp, _y4m.YuvFrame):
        if maxval not in (None, npInp.maxval):
            raise ValueError(f"a {npInp.depth}-bit planar frame has maxval {npInp.maxval}, got {maxval}")
        planes = torch.from_numpy(npInp.data if npInp.data.flags.writeable else npInp.data.copy()).to(device, non_blocking=True)
        return _ops.to_inp_yuv(planes, npInp.shape[:2], dst_size, matrix=matrix, full_range=full_range,
                               maxval=None if npInp.depth == 8 else npInp.maxval, **fit_kw,
                               **({} if npInp.layout == "420" else {"layout": npInp.layout}))
    if torch.is_tensor(npInp):
        u8 = npInp.to(device, non_blocking=True)
    else:
        u8 = torch.from_numpy(np.ascontiguousarray(npInp)).to(device, non_blocking=True)
    if _is_u16(u8):
        return _ops.to_inp(u8, dst_size, maxval=maxval, **fit_kw)
    if maxval is not None:
        raise ValueError("maxval belongs to 16-bit frames (uint16)")
    return _ops.to_inp(u8, dst_size, **fit_kw)


def to_out(tenInp, src_size, rgb=False, depth=8, maxval=None, pixfmt="bgr", matrix="bt709", full_range=False, fit="resize",
           window=None):
    """to_cv2(resize(tenInp, src_size)) (tools.py:63-64) as one kernel + the D2H copy.  rgb=True returns the frame in RGB
    order (the flip the reference's writer thread does on the host, tools.py:202, done on the device instead).  depth=16
    returns a uint16 frame scaled to `maxval` (65535 unless given), rounded and saturated (ops.to_out).  pixfmt="yuv420" returns
    the frame as planar 4:2:0 instead, one 1-D array holding Y, U, V (ops.to_out_yuv; at depth 16 scaled to 1023 unless given);
    "yuv422" and "yuv444" the same with those chroma layouts.
    fit="pad" (not in the reference): the top-left `src_size` window of tenInp is converted as it stands -- the counterpart of
    to_inp(..., fit="pad") -- instead of the resize.
    window=(x, y, w, h) (--crop, not in the reference): the frame returned is still `src_size`; tenInp is converted to that rectangle
    of it and everything outside is the format's black (ops.to_out / ops.to_out_yuv)."""
    _check_depth(depth, maxval)
    fit_kw = {**_fit_kw(fit), **_window_kw(window)}
    if pixfmt != "bgr" and pixfmt not in _frames.YUV_PIXFMTS:
        raise ValueError(f"pixfmt must be bgr, yuv420, yuv422 or yuv444, got {pixfmt!r}")
    if pixfmt in _frames.YUV_PIXFMTS:
        if rgb:
            raise ValueError("rgb=True belongs to packed frames (pixfmt='bgr')")
        layout_kw = {} if pixfmt == "yuv420" else {"layout": _frames.YUV_PIXFMTS[pixfmt]}
        frame = _ops.to_out_yuv(tenInp, src_size, matrix=matrix, full_range=full_range, depth=depth, maxval=maxval, **fit_kw,
                                **layout_kw).cpu().numpy()
    elif depth == 16:
        frame = _ops.to_out(tenInp, src_size, rgb=rgb, depth=16, maxval=maxval, **fit_kw).cpu().numpy()
    else:
        frame = _ops.to_out(tenInp, src_size, rgb=rgb, **fit_kw).cpu().numpy()
    # the copy has waited for every kernel behind this frame: had one of the two-term fp16 kernels overflowed on the way, its
    # status byte is set by now -- raise here rather than hand the frame to the writer (ops.check_overflow: a host memory read)
    _ops.check_overflow(tenInp.device)
    return frame


def distance_calculator(_x):
    """sqrt(u^2 + v^2) per pixel in fp32 (tools.py:77-80)."""
    return _ops.flow_distance(_x)


def check_scene(x1, x2, scdet_threshold=0.3):
    """Scene cut test: SSIM(32x32 thumbnails, 3-D 11^3 gaussian) < threshold (tools.py:27-30).
    Returns a Python bool (the reference returns a 0-dim bool tensor used in `if`)."""
    return _ops.ssim_thumb32(x1, x2) < scdet_threshold


class SceneChecks:
    """check_scene for frame pairs announced ahead of their use (not in the reference, same decisions): submit(key, x1, x2)
    enqueues the test when the driver has both frames, cut(key, x1, x2) returns the bool -- waiting only for that test's own
    event -- and remembers it (the drivers ask for the same pair in several iterations).  `key` identifies the pair for
    the caller (frame indices, or object ids).  Only the decision is kept once it is known, with WEAK references to the
    two frames as the identity guard (an id can be recycled once a frame is gone: a dead or different referent is a miss):
    a remembered pair must not keep its frames -- and the encoder features hung on them, 270 MB per 1080p frame -- alive.
    A pending test holds its frames only until it is collected; the last 32 decisions are kept."""

    def __init__(self, scdet_threshold=0.3):
        self.thr, self.pending, self.done = scdet_threshold, {}, {}

    def submit(self, key, x1, x2):
        if key not in self.pending and not self._known(key, x1, x2):
            self.pending[key] = (_ops.ssim_thumb32_async(x1, x2), x1, x2)
            while len(self.pending) > 32:  # tests nobody asked for (a driver that stopped early): do not pin their frames
                self.pending.pop(next(iter(self.pending)))

    def _known(self, key, x1, x2):
        d = self.done.get(key)
        return d is not None and d[1]() is x1 and d[2]() is x2

    def cut(self, key, x1, x2):
        if self._known(key, x1, x2):
            return self.done[key][0]
        self.done.pop(key, None)
        p = self.pending.pop(key, None)
        if p is None or p[1] is not x1 or p[2] is not x2:
            p = (_ops.ssim_thumb32_async(x1, x2), x1, x2)
        (host, ev), _, _ = p
        ev.synchronize()
        res = float(host.item()) < self.thr
        self.done[key] = (res, weakref.ref(x1), weakref.ref(x2))
        while len(self.done) > 32:
            self.done.pop(next(iter(self.done)))
        return res


# ----------------------------------------------------------------------------- timestep mapping
class TMapper:
    """Maps a source-frame interval to the output timestamps that fall inside it (tools.py:120-134)."""

    def __init__(self, src=-1.0, dst=0.0, times=-1):
        self.times = dst / src if times == -1 else times
        self.now_step = -1

    def get_range_timestamps(self, _min, _max, lclose=True, rclose=False, normalize=True):
        first = math.ceil(_min * self.times)
        last = math.ceil(_max * self.times)
        if not lclose:
            first += 1
        if rclose:
            last += 1
        if first >= last:
            return []
        if normalize:
            return [((i / self.times) - _min) / (_max - _min) for i in range(first, last)]
        return [i / self.times for i in range(first, last)]


def calc_t(idx, times, t_mapper):
    """Timesteps (in [0.5, 1.5), relative to frame idx-... see driver) for one centre frame.

    Integer `times` (reference infer.py:76-87): odd -> [..., 1, ...] symmetric about 1,
    even -> (i + 0.5)/times mirrored about 1.  Otherwise (infer.py:89-91) the output
    timestamps inside [idx-0.5, idx+0.5) from TMapper, shifted by -idx, rounded to 4
    decimals, +1.  float64 throughout; must be bit-identical to the reference.
    """
    if times != -1:
        if times % 2:
            half = [(i + 1) / times for i in range((times - 1) // 2)]
            return np.array(list(reversed([1 - t for t in half])) + [1] + [t + 1 for t in half])
        half = [(i + 0.5) / times for i in range(times // 2)]
        return np.array(list(reversed([1 - t for t in half])) + [t + 1 for t in half])
    stamps = np.array(t_mapper.get_range_timestamps(idx - 0.5, idx + 0.5, lclose=True, rclose=False, normalize=False))
    return np.round(stamps - idx, 4) + 1


# ----------------------------------------------------------------------------- frame source / sink
def out_layout(out_chroma, output_path, src_layout):
    """--out-chroma (source | 420 | 422 | 444) -> the chroma layout of a Y4M sink ("420" | "422" | "444"), None for any other sink,
    which refuses a value other than `source` (ValueError).  `source`: src_layout when the source is a Y4M stream (None otherwise:
    4:2:0, as before the flag existed)."""
    if out_chroma not in ("source",) + tuple(_y4m.LAYOUTS):
        raise ValueError(f"out_chroma must be source, 420, 422 or 444, got {out_chroma!r}")
    if not (output_path == "-" or os.path.splitext(output_path)[1].lower() == ".y4m"):
        if out_chroma != "source":
            raise ValueError(f"--out-chroma {out_chroma} needs a YUV4MPEG2 sink (a .y4m path or -), not {output_path}: the other sinks "
                             "take packed frames, and the encoder pipe stays yuv420p")
        return None
    return (src_layout or "420") if out_chroma == "source" else out_chroma


class VideoFI_IO:
    """Frame source/sink with the reference's interface (tools.py:156-213): read_frame(),
    write_frame(), finish_writing(), .src_fps, .total_frames_count, .width, .height.

    Containers: when OpenCV and an ffmpeg binary exist the reference's path is used
    (cv2.VideoCapture decode, rawvideo rgb24 pipe into ffmpeg libx264 -qp 16, audio copied).
    Neither exists on the MI355X image, so the native formats are:
      input : .npz  {frames: uint8 [N,H,W,3] BGR, fps: float}  or .npy (+ optional .json {"fps"})
      output: .npz  {frames, fps}  or .npy;  anything else -> raw rgb24 bytes (ffmpeg's pipe format)
    `hwaccel` selects a hardware encoder when ffmpeg is present (h264_vaapi/h264_amf on AMD
    instead of the reference's h264_nvenc).

    16-bit frames (not in the reference): a .npz / .npy source may hold uint16 [N,H,W,3] frames with samples in [0, maxval]
    (.npz entry `maxval` / .json {"maxval"}, 65535 when absent; 1023 for 10-bit data); a container source stays 8-bit.
    .depth (8 | 16) and .maxval describe the source, .out_depth / .out_maxval what the sink takes: `out_depth` 8 or 16, or None
    for the source's depth (a 16-bit sink of an 8-bit source is scaled to 65535, otherwise to the source's maxval).  At depth 16
    the .npz / .npy sink stores uint16 frames (.npz: with `maxval`), the raw sink and the encoder pipe take rgb48le bytes --
    little-endian, RGB order, always scaled to 65535 -- and the encoder is libx264 at yuv420p10le; `hwaccel` is refused there
    (h264_vaapi encodes 8 bits).

    YUV4MPEG2 (not in the reference; drba_amd/y4m.py): a `.y4m` path, or `-` for stdin / stdout, selects the Y4M source or sink,
    each independently of the other end.  The source reads one planar 4:2:0 frame at a time behind the bounded read queue (frames
    are y4m.YuvFrame objects; .pixfmt is "yuv420", .depth 8, or 16 with .maxval 1023 for C420p10) and the sink writes each frame
    as it arrives (.out_pixfmt "yuv420": frames are the 1-D Y, U, V arrays of to_out(..., pixfmt="yuv420"); out_depth 16 writes
    C420p10, .out_maxval 1023).  `yuv_matrix` (bt709 | bt601) and `yuv_range` (source | limited | full) describe the conversion the
    hooks perform: .yuv_full_range for the way in (the header's XCOLORRANGE; without one, what `yuv_range` says, limited by
    default), .out_full_range for the way out (`yuv_range`, or the way in's when it is `source`).  The sink's header carries the
    source's C tag, A, I and X tags through and the exact frame rate (y4m.output_fps).

    Chroma layouts: a Y4M source may be 4:2:0, 4:2:2 or 4:4:4 (C422, C422p10, C444, C444p10: .pixfmt "yuv422" / "yuv444", frames
    carry their layout).  `out_chroma` (source | 420 | 422 | 444) names the Y4M sink's layout: `source` is the source's when it is a
    Y4M stream and 4:2:0 otherwise; .out_pixfmt and the sink header's C tag follow it (C444p10 at out_depth 16).  Any other sink
    refuses a value other than `source`: the encoder pipe stays yuv420p.

    .src_format / .sink_format say all of the above about the two ends as one drba_amd.frames.FrameFormat each: what the frame hooks
    are built from (frames.hooks).
    """

    def __init__(self, input_path, output_path, dst_fps=60, times=-1, hwaccel=False, src_fps=None, out_depth=None,
                 yuv_matrix="bt709", yuv_range="source", out_chroma="source"):
        self.input_path, self.output_path = input_path, output_path
        self.out_layout = out_layout(out_chroma, output_path, None)  # (refuses before anything is opened)
        self._cv2 = None
        self._y4m_in = self._y4m_out = None
        self.depth, self.maxval = 8, 255
        self.pixfmt = "bgr"
        if yuv_matrix not in _ops.YUV_MATRICES:
            raise ValueError(f"yuv_matrix must be one of {sorted(_ops.YUV_MATRICES)}, got {yuv_matrix!r}")
        self.yuv_matrix = yuv_matrix
        self.yuv_full_range = _frames.full_range(yuv_range, None, tag_wins=True)  # (refuses an unknown yuv_range)
        src_ratio = None
        ext = os.path.splitext(input_path)[1].lower()
        if input_path == "-" or ext == ".y4m":
            self._y4m_in = _y4m.Reader(sys.stdin.buffer if input_path == "-" else open(input_path, "rb"), accept=_y4m.ACCEPT_ALL)
            hdr = self._y4m_in.header
            self.pixfmt = "yuv" + hdr.layout
            if hdr.depth > 8:
                self.depth, self.maxval = 16, hdr.maxval
            self.yuv_full_range = _frames.full_range(yuv_range, hdr.color_range, tag_wins=True)
            src_ratio = (hdr.fps_num, hdr.fps_den)
            self.src_fps = float(src_fps if src_fps is not None else hdr.fps)
            self.total_frames_count = float(self._y4m_in.frame_count_estimate())
            self.height, self.width = hdr.height, hdr.width
        elif ext in (".npz", ".npy"):
            self._frames, fps, maxval = _frames.open_array_clip(input_path)
            if self._frames.dtype == np.uint16:
                self.depth, self.maxval = 16, _ops._maxval(maxval)
            self.src_fps = float(src_fps if src_fps is not None else (fps if fps is not None else 24.0))
            self.total_frames_count = float(len(self._frames))
            self.height, self.width = int(self._frames.shape[1]), int(self._frames.shape[2])
        else:
            try:
                import cv2  # noqa: WPS433 (optional dependency, absent on the GPU image)
            except ImportError as e:
                raise RuntimeError(f"decoding {ext or 'this input'} needs OpenCV, which is not installed; "
                                   "use a .npz/.npy clip") from e
            self._cv2 = cv2.VideoCapture(input_path)
            self.src_fps = self._cv2.get(cv2.CAP_PROP_FPS)
            self.total_frames_count = self._cv2.get(7)
            self.width = int(self._cv2.get(cv2.CAP_PROP_FRAME_WIDTH))
            self.height = int(self._cv2.get(cv2.CAP_PROP_FRAME_HEIGHT))
        self.dst_fps = times * self.src_fps if times != -1 else dst_fps
        if out_depth not in (None, 8, 16):
            raise ValueError(f"out_depth must be 8, 16 or None (the source's depth), got {out_depth!r}")
        self.out_depth = self.depth if out_depth is None else int(out_depth)
        self.out_maxval = 255 if self.out_depth == 8 else (self.maxval if self.depth == 16 else 65535)
        if hwaccel and self.out_depth == 16:  # before a frame is read or an encoder is started
            raise ValueError("-hw at 16-bit output: the hardware encoder (h264_vaapi) takes 8-bit frames, there is no 10-bit "
                             "hardware encode here; drop -hw (libx264 at yuv420p10le) or write 8 bits (--out-depth 8)")

        oext = os.path.splitext(output_path)[1].lower()
        self._sink_frames = [] if oext in (".npz", ".npy") else None
        self._ffmpeg = None
        self._raw = None
        self.out_pixfmt = "bgr"
        self.out_full_range = self.yuv_full_range if yuv_range == "source" else yuv_range == "full"
        if output_path == "-" or oext == ".y4m":
            self.out_layout = out_layout(out_chroma, output_path, self._y4m_in.header.layout if self._y4m_in is not None else None)
            self.out_pixfmt = "yuv" + self.out_layout
            if self.out_depth == 16:
                self.out_maxval = 1023  # 10 bits is what the format and the encoders carry
            self._y4m_out = _y4m.Writer(sys.stdout.buffer if output_path == "-" else open(output_path, "wb"),
                                        self._y4m_header(src_ratio, src_fps, dst_fps, times, yuv_range))
        elif self._sink_frames is None:
            if _have_ffmpeg() and oext not in (".raw", ".rgb"):
                self._ffmpeg = self._spawn_ffmpeg(hwaccel)
            else:
                self._raw = open(output_path, "wb")
        # sinks that want RGB bytes (the ffmpeg pipe and the raw file, tools.py:202): the driver can hand over frames that
        # are already RGB (to_out(..., rgb=True) flips on the device) by setting frames_are_rgb
        self.wants_rgb = self._sink_frames is None and self._y4m_out is None
        self.frames_are_rgb = False
        # the two ends as the frame hooks are built from them (drba_amd.frames.hooks)
        self.src_format = _frames.FrameFormat(self.pixfmt, self.depth, self.maxval, yuv_matrix, self.yuv_full_range)
        self.sink_format = _frames.FrameFormat(self.out_pixfmt, self.out_depth, self.out_maxval, yuv_matrix, self.out_full_range,
                                               rgb=self.wants_rgb)
        self._sink_error = None
        self.read_buffer = Queue(maxsize=100)
        # the Y4M sink writes each frame as it arrives and may be a pipe into an encoder that is slower than this pipeline: its
        # queue is bounded like the read queue, so that memory does not grow with the clip (write_frame then waits for the sink)
        self.write_buffer = Queue(maxsize=100 if self._y4m_out is not None else -1)
        self._closed = threading.Event()
        threading.Thread(target=self._reader, daemon=True).start()
        self._writer_thread = threading.Thread(target=self._writer, daemon=True)
        self._writer_thread.start()

    def _y4m_header(self, src_ratio, src_fps, dst_fps, times, yuv_range):
        """The sink's header: the source's tags where it is a Y4M stream (its C tag unchanged while the depth class stays, A, I, the
        other X tags), C420p10 at 16-bit output, C420jpeg for any other source; the exact frame rate; XCOLORRANGE when the source
        carried one or `yuv_range` names one."""
        src = self._y4m_in.header if self._y4m_in is not None else None
        if src_fps is not None or src_ratio is None:
            src_ratio = self.src_fps
        num, den = _y4m.output_fps(src_ratio, dst_fps, times)
        chroma = _y4m.chroma_tag(self.out_layout, 10 if self.out_depth == 16 else 8,
                                 like=src.chroma if src is not None and src.depth == 8 else None)
        color_range = None
        if yuv_range != "source" or (src is not None and src.color_range is not None):
            color_range = "FULL" if self.out_full_range else "LIMITED"
        return _y4m.Header(self.width, self.height, (num, den), interlace=src.interlace if src is not None else "p",
                           aspect=src.aspect if src is not None else None, chroma=chroma, color_range=color_range,
                           extra=src.extra if src is not None else ())

    def _ffmpeg_cmd(self, hwaccel):
        """The reference's pipe (tools.py:176-186): rawvideo rgb24 in, libx264 -qp 16 -preset medium, audio copied from the
        source container.  -hw selects h264_vaapi (the reference's h264_nvenc has no AMD counterpart), which needs the
        device + upload filter and takes neither -preset nor a software pixel format.  A .npz/.npy source has no audio
        stream to map, so the second input is only added for real containers."""
        container = self._cv2 is not None
        cmd = ["ffmpeg", "-y"]
        if hwaccel:
            cmd += ["-vaapi_device", "/dev/dri/renderD128"]
        cmd += ["-f", "rawvideo", "-pix_fmt", "rgb24" if self.out_depth == 8 else "rgb48le", "-r", f"{self.dst_fps}", "-s", f"{self.width}x{self.height}", "-i", "pipe:0"]
        if container:
            cmd += ["-i", self.input_path, "-map", "0:v", "-map", "1:a?"]
        if hwaccel:
            cmd += ["-vf", "format=nv12,hwupload", "-c:v", "h264_vaapi", "-qp", "16"]
        else:
            cmd += ["-c:v", "libx264", "-pix_fmt", "yuv420p" if self.out_depth == 8 else "yuv420p10le", "-qp", "16", "-preset", "medium"]
        cmd += ["-movflags", "+faststart"]
        if container:
            cmd += ["-c:a", "aac", "-b:a", "320k"]
        return cmd + [f"{self.output_path}"]

    def _spawn_ffmpeg(self, hwaccel):
        return subprocess.Popen(self._ffmpeg_cmd(hwaccel), stdin=subprocess.PIPE)

    def _reader(self):
        if self._y4m_in is not None:
            try:
                fr = self._y4m_in.read_frame()  # one frame ahead of the bounded queue, never more
                while fr is not None:
                    self.read_buffer.put(fr)
                    fr = self._y4m_in.read_frame()
            except Exception as e:  # a truncated stream: hand the error to the reading side instead of dying silently
                self.read_buffer.put(e)
                return
        elif self._cv2 is not None:
            ok, fr = self._cv2.read()
            while ok:
                self.read_buffer.put(fr)
                ok, fr = self._cv2.read()
        else:
            for k in range(len(self._frames)):
                self.read_buffer.put(np.ascontiguousarray(self._frames[k]))
        self.read_buffer.put(None)

    def _writer(self):
        while True:
            item = self.write_buffer.get()
            if item is None:
                break
            if self._sink_frames is not None:
                self._sink_frames.append(item)
            elif self._y4m_out is not None:
                if self._sink_error is None:
                    try:
                        self._y4m_out.write_frame(item)  # each frame as it arrives: nothing is kept
                    except (BrokenPipeError, OSError, TypeError, ValueError) as e:
                        self._sink_error = e
            elif self._sink_error is None:
                # BGR -> RGB as the reference's pipe, unless the driver already flipped on the device
                rgb = np.ascontiguousarray(item if self.frames_are_rgb else item[:, :, ::-1])
                try:
                    if self.out_depth == 16:
                        rgb = self._rgb48le(rgb)
                    if self._ffmpeg is not None and self._ffmpeg.poll() is not None:
                        raise BrokenPipeError(f"ffmpeg exited with code {self._ffmpeg.returncode}")
                    (self._ffmpeg.stdin if self._ffmpeg is not None else self._raw).write(rgb)
                except (BrokenPipeError, OSError, TypeError) as e:  # keep draining the queue; close() re-raises
                    self._sink_error = e
        if self._sink_frames is not None:
            dtype = np.uint8 if self.out_depth == 8 else np.uint16
            arr = np.stack(self._sink_frames) if self._sink_frames else np.zeros((0, self.height, self.width, 3), dtype)
            if self.out_depth == 16 and arr.dtype != dtype:
                self._sink_error = TypeError(f"the sink takes {np.dtype(dtype).name} frames (out_depth {self.out_depth}), got {arr.dtype}")
            elif self.output_path.lower().endswith(".npz"):
                extra = {} if self.out_depth == 8 else {"maxval": np.int64(self.out_maxval)}
                np.savez(self.output_path, frames=arr, fps=np.float64(self.dst_fps), **extra)
            else:
                np.save(self.output_path, arr)
        elif self._y4m_out is not None:
            try:
                self._y4m_out.flush()
                if self.output_path != "-":
                    self._y4m_out.f.close()
            except OSError as e:
                self._sink_error = self._sink_error or e
        elif self._ffmpeg is not None:
            try:
                self._ffmpeg.stdin.close()
            except OSError:
                pass
            if self._ffmpeg.wait() != 0 and self._sink_error is None:
                self._sink_error = RuntimeError(f"ffmpeg exited with code {self._ffmpeg.returncode}")
        else:
            self._raw.close()
        self._closed.set()

    def _rgb48le(self, rgb):
        """uint16 RGB frame with samples in [0, out_maxval] -> rgb48le: full range (v * 65535 / maxval, rounded), little-endian."""
        if rgb.dtype != np.uint16:
            raise TypeError(f"the 16-bit sink takes uint16 frames, got {rgb.dtype}")
        if self.out_maxval != 65535:
            mv = np.uint32(self.out_maxval)
            rgb = (np.minimum(rgb, self.out_maxval).astype(np.uint32) * np.uint32(65535) + mv // np.uint32(2)) // mv
        return np.ascontiguousarray(rgb.astype("<u2"))

    def write_frame(self, x):
        self.write_buffer.put(x)

    def read_frame(self):
        fr = self.read_buffer.get()
        if isinstance(fr, Exception):
            raise fr
        return fr

    def finish_writing(self):
        return self.write_buffer.empty() or self._closed.is_set()

    def close(self):
        """Flush and close the sink (the reference never terminates its writer thread; this does)."""
        self.write_buffer.put(None)
        self._writer_thread.join()
        if self._sink_error is not None:
            raise RuntimeError(f"writing {self.output_path} failed: {self._sink_error}") from self._sink_error


def _have_ffmpeg():
    from shutil import which
    return which("ffmpeg") is not None
