"""DRBA command line and per-frame driver loop (same CLI as the reference's infer.py).

    python infer.py -m rife -i in.npz -o out.npz [-fps 60 | -t 2] [-s] [-st 0.3] [-hw] [-scale 1.0] [--out-depth source|8|16]
                    [--nonlinear] [--yuv-matrix bt709|bt601] [--yuv-range source|limited|full] [--deterministic] [--fit resize|pad]
                    [--dedup [--dedup-hi 0.047] [--dedup-lo 0.0196] [--dedup-frac 0.33] [--dedup-max 3]] [--out-chroma source|420|422|444]
                    [--crop off|auto|W:H:X:Y] [--crop-limit 0.094]

`--out-depth` is not in the reference: a .npz / .npy clip may hold uint16 frames, and the written frames are 8 or 16 bits deep
(default: as the source, so an 8-bit clip is handled exactly as before).  `--nonlinear` is not in the reference either: its driver
always asks the model for linear=True (infer.py:143) although the model entry point defaults to the non-linear DistanceRatioMap
(get_drm_t); with the flag every DRBA step of the clip runs with linear=False.

`--deterministic` (not in the reference): the written bytes depend on the clip, the command, the build, the device model and the
stored kernel configurations only -- two runs write the same file (drba_amd.ops.set_deterministic).  A frame-sharded
run is reproducible too, but not promised to equal the sequential one.

A `.y4m` path, or `-` for stdin / stdout, at either end selects the YUV4MPEG2 source or sink (drba_amd/y4m.py; planar 4:2:0 at 8
or 10 bits, converted inside the to_inp / to_out kernels): `ffmpeg -i a.mkv -f yuv4mpegpipe - | python infer.py -m rife -i - -o - -t 2
| x264 --demuxer y4m -o b.264 -`.  `--yuv-matrix` and `--yuv-range` name the conversion; on a Y4M sink `--out-depth 16` writes
C420p10.  Nothing is printed to stdout.  A Y4M source may also be planar 4:2:2 or 4:4:4 (C422, C422p10, C444, C444p10), and
`--out-chroma` names the Y4M sink's layout: `source` (default) writes the source's when it is a Y4M stream and 4:2:0 otherwise, so a
4:2:0 clip and every run without a Y4M sink are what they were; `--out-chroma 444` keeps the full-resolution colour of the generated
frames (`-f yuv4mpegpipe -pix_fmt yuv444p10le` in, `--out-chroma 444 --out-depth 16` out).  With any other sink a value but `source`
is refused before the model is built.

`--fit pad` (not in the reference, whose frames are always resized to the network size and back): the frame sits at the top left
of the network tensor, the bottom and right margins repeat its last row and column and are cropped away on the way out -- no
resampling in either direction, so a frame the driver only copies (a scene cut, the head and the tail) comes back with the
source's bytes.  The network sizes are those of `resize`.  Scene detection runs on the padded network input, so its decisions may
differ from `resize` mode for a pair near the threshold.  The default, `resize`, is unchanged.

`--dedup` (not in the reference, whose README leaves repeated frames to a separate tool): a source frame that repeats its predecessor
(ffmpeg mpdecimate's rule, tested on the device: drba_amd.ops.dup_stats) is dropped before the model sees it, at most `--dedup-max` in a
row, and the steps are retimed across the gaps (drba_amd/dedup.py): the clip written has the same frames at the same instants, but the
motion of a drawing held for two frames is spread over both instead of being packed into the interval where it changes.  With every
source and sink; `python -m drba_amd.evaluate dups clip` prints the figures the thresholds are chosen from.

`--crop` (not in the reference): letterbox / pillarbox bars stay out of the network.  `--crop W:H:X:Y` (ffmpeg's crop=, as `ffmpeg -vf
cropdetect` prints it; a leading `crop=` is accepted) names the active picture; `--crop auto` finds it first, in one pass over the clip
(drba_amd/crop.py: cropdetect's rule on the row and column maxima of every frame, `--crop-limit` on the [0, 1] scale, the union over
the clip grown outward to the chroma alignment) -- for sources that can be opened twice, .npz / .npy / .y4m files; for stdin and
containers it is refused before the model is built (`python -m drba_amd.evaluate bars clip` prints the box to pass explicitly).  The
hooks then read and write that window of every frame (drba_amd.frames.hooks(..., crop=box)), the network size follows from the box
(1440x1080 inside 1920x1080 runs at 1440x1088), and the written frames keep the source's size with exact black outside the box.  The
scene test and `--dedup` see the cropped network input, so their decisions may differ from an uncropped run.  Not in the frame-sharded
run.

The driver logic is host-side Python like the reference; the model calls it makes run on
the HIP library.  `interpolate_stream` is the loop of reference infer.py:58-174 (drba_amd/driver.py) with the
module globals turned into arguments, so tests can drive it with any model object.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

from drba_amd import crop as _crop
from drba_amd import dedup as _dedup
from drba_amd import driver
from drba_amd import frames as _frames
from drba_amd.models.utils import tools as _tools


def parse_args(argv=None):
    """Same flags, defaults and dest names as reference infer.py:18-36."""
    p = argparse.ArgumentParser(description="Interpolation a video with DRBA")
    p.add_argument("-m", "--model_type", dest="model_type", type=str, default="rife",
                   help="model network type, current support rife/gmfss/gmfss_union")
    p.add_argument("-i", "--input", dest="input", type=str, default="input.mp4", help="absolute path of input video")
    p.add_argument("-o", "--output", dest="output", type=str, default="output.mp4", help="absolute path of output video")
    p.add_argument("-fps", "--dst_fps", dest="dst_fps", type=float, default=60, help="interpolate to ? fps")
    p.add_argument("-t", "--times", dest="times", type=int, default=-1, help="interpolate to ?x fps")
    p.add_argument("-s", "--enable_scdet", dest="enable_scdet", action="store_true", default=False,
                   help="enable scene change detection")
    p.add_argument("-st", "--scdet_threshold", dest="scdet_threshold", type=float, default=0.3,
                   help="ssim scene detection threshold")
    p.add_argument("-hw", "--hwaccel", dest="hwaccel", action="store_true", default=False,
                   help="enable hardware acceleration encode")
    p.add_argument("-scale", "--scale", dest="scale", type=float, default=1.0,
                   help="flow scale, generally use 1.0 with 1080P and 0.5 with 4K resolution")
    p.add_argument("--out-depth", dest="out_depth", type=str, default="source", choices=("source", "8", "16"),
                   help="bits per sample of the written frames: the source's (default), 8, or 16 (uint16 .npz / .npy, rgb48le raw, "
                        "libx264 yuv420p10le; not with -hw, not in the frame-sharded run)")
    p.add_argument("--nonlinear", dest="nonlinear", action="store_true", default=False,
                   help="run every DRBA step with the non-linear DistanceRatioMap (inference_ts_drba(..., linear=False))")
    p.add_argument("--yuv-matrix", dest="yuv_matrix", type=str, default="bt709", choices=("bt709", "bt601"),
                   help="YCbCr matrix of a .y4m source / sink (default bt709)")
    p.add_argument("--yuv-range", dest="yuv_range", type=str, default="source", choices=("source", "limited", "full"),
                   help="sample range of a .y4m source / sink: the source header's XCOLORRANGE (default; limited when it has none or "
                        "the source is not Y4M), limited or full; a Y4M source that carries the tag is always read by it")
    p.add_argument("--deterministic", dest="deterministic", action="store_true", default=False,
                   help="bit-reproducible output: the splats sum in an order fixed by the data and no timing picks a kernel "
                        "configuration (stored winners of `python -m drba_amd.tune` are still used)")
    p.add_argument("--fit", dest="fit", type=str, default="resize", choices=("resize", "pad"),
                   help="how a frame gets to the network size and back: resize (default, the reference's behaviour) or pad -- "
                        "replicate padding at the bottom and right, cropped away on the way out, no resampling")
    p.add_argument("--out-chroma", dest="out_chroma", type=str, default="source", choices=("source", "420", "422", "444"),
                   help="chroma layout of a .y4m sink: the source's when it is a Y4M stream, else 4:2:0 (default), or 4:2:0 / 4:2:2 / "
                        "4:4:4 (C444p10 with --out-depth 16); refused with any other sink")
    p.add_argument("--dedup", dest="dedup", action="store_true", default=False,
                   help="drop repeated source frames (drawings on twos, threes, fours) and interpolate across the gaps: the same "
                        "frames at the same instants are written (ffmpeg mpdecimate's rule; not in the frame-sharded run)")
    p.add_argument("--dedup-hi", dest="dedup_hi", type=float, default=_dedup.HI,
                   help="a frame is no repeat if one 8x8 block differs from the previous source frame by more than this on average, "
                        "on the [0, 1] scale (default 12/255)")
    p.add_argument("--dedup-lo", dest="dedup_lo", type=float, default=_dedup.LO,
                   help="... or if more than --dedup-frac of the blocks differ by more than this (default 5/255)")
    p.add_argument("--dedup-frac", dest="dedup_frac", type=float, default=_dedup.FRAC, help="see --dedup-lo (default 0.33)")
    p.add_argument("--dedup-max", dest="dedup_max", type=int, default=_dedup.MAX_RUN,
                   help="at most this many frames in a row are dropped; the next one is kept whatever the test says (default 3)")
    p.add_argument("--crop", dest="crop", type=str, default="off",
                   help="keep letterbox / pillarbox bars out of the network: off (default), auto (one pass over the clip finds the active "
                        "picture first; .npz / .npy / .y4m files) or W:H:X:Y, ffmpeg's crop= as cropdetect prints it.  The written frames "
                        "keep the source's size, exact black outside the box (not in the frame-sharded run)")
    p.add_argument("--crop-limit", dest="crop_limit", type=float, default=_crop.LIMIT,
                   help="--crop auto: a row or column is picture when a sample of it exceeds this, on the [0, 1] scale (default 24/255, "
                        "cropdetect's limit)")
    return p.parse_args(argv)


RESCANNABLE = (".npz", ".npy", ".y4m")  # sources --crop auto can read twice


def crop_of(args):
    """--crop as the driver takes it: None (off), "auto", or a drba_amd.crop.Box (ValueError for anything else).  A namespace built
    without the flag means off."""
    v = getattr(args, "crop", "off")
    if v is None or v == "off":
        return None
    if isinstance(v, _crop.Box) or v == "auto":
        return v
    return _crop.parse(v)


def crop_limit_of(args):
    """--crop-limit, checked (0 <= limit < 1).  A namespace built without the flag means 24/255."""
    v = getattr(args, "crop_limit", _crop.LIMIT)
    _crop.threshold_of(v, 255)
    return float(v)


def check_crop(args):
    """What can be refused about --crop without reading a frame, before the model is built: a malformed box or limit, and `auto` for a
    source that cannot be opened twice.  -> crop_of(args)."""
    c = crop_of(args)
    crop_limit_of(args)
    if c == "auto" and (args.input == "-" or os.path.splitext(args.input)[1].lower() not in RESCANNABLE):
        raise ValueError(f"--crop auto reads the clip twice, which it can do for {' / '.join(RESCANNABLE)} files, not for "
                         f"{'stdin' if args.input == '-' else args.input}: run `python -m drba_amd.evaluate bars CLIP` on a copy or an "
                         "excerpt of the clip (or ffmpeg's cropdetect) and pass the box it prints as --crop W:H:X:Y")
    return c


def _resolve_crop(args, c, size, src_pixfmt, sink_pixfmt):
    """auto -> the scan's box (None, and one line on stderr, when there is nothing to crop); an explicit box -> itself, validated."""
    align = _crop.alignment_of(src_pixfmt, sink_pixfmt)
    if c == "auto":
        box = _crop.scan(args.input, crop_limit_of(args), align)
        if box is None:
            print(f"--crop auto: no bars found in {args.input} (every frame empty, or the picture fills the frame): running without a "
                  "crop", file=sys.stderr)
        return box
    return _crop.validate(c, size, align)


def plan_crop(args):
    """main() calls this before the model is built: check_crop, and for a source whose size can be read from the file (.npz / .npy /
    .y4m) the box itself -- `auto` scanned, an explicit one validated against the frame size and the chroma alignment of the two ends
    -- stored back as args.crop (a Box, or "off").  An explicit box on a stream or a container is validated when its header has been
    read (inference)."""
    c = check_crop(args)
    ext = os.path.splitext(args.input)[1].lower()
    if c is None or args.input == "-" or ext not in RESCANNABLE:
        return c
    if ext == ".y4m":
        from drba_amd import y4m
        with open(args.input, "rb") as f:
            hdr = y4m.Reader(f, accept=y4m.ACCEPT_ALL).header
        size, src_pixfmt, src_layout = (hdr.height, hdr.width), "yuv" + hdr.layout, hdr.layout
    else:
        frames, _, _ = _frames.open_array_clip(args.input)
        size, src_pixfmt, src_layout = (int(frames.shape[1]), int(frames.shape[2])), "bgr", None
    layout = _tools.out_layout(getattr(args, "out_chroma", "source"), args.output, src_layout)
    box = _resolve_crop(args, c, size, src_pixfmt, "bgr" if layout is None else "yuv" + layout)
    args.crop = "off" if box is None else box
    return box


def crop_box(args, video_io):
    """--crop for an opened clip -> a drba_amd.crop.Box or None: what inference hands the hooks and the loop."""
    c = check_crop(args)
    if c is None:
        return None
    return _resolve_crop(args, c, (video_io.height, video_io.width), video_io.src_format.pixfmt, video_io.sink_format.pixfmt)


def dedup_of(args):
    """--dedup and its settings as interpolate_stream takes them: None (off) or a drba_amd.dedup.Settings.  A namespace built without
    the flags means off / the defaults."""
    if not getattr(args, "dedup", False):
        return None
    return _dedup.Settings(getattr(args, "dedup_hi", _dedup.HI), getattr(args, "dedup_lo", _dedup.LO),
                           getattr(args, "dedup_frac", _dedup.FRAC), getattr(args, "dedup_max", _dedup.MAX_RUN))


def fit_of(args):
    """--fit as the hooks take it.  A namespace built without the flag means resize."""
    v = getattr(args, "fit", "resize")
    if v not in ("resize", "pad"):
        raise ValueError(f"--fit must be resize or pad, got {v!r}")
    return v


def apply_deterministic(args):
    """--deterministic: switch the mode on (process wide) before anything runs.  A namespace built without the flag leaves it alone."""
    if getattr(args, "deterministic", False):
        from drba_amd import ops
        ops.set_deterministic(True)


def out_chroma_of(args):
    """--out-chroma as VideoFI_IO takes it, checked against the sink (tools.out_layout: ValueError for a sink that is not Y4M and a
    value other than source).  A namespace built without the flag means source."""
    v = getattr(args, "out_chroma", "source")
    _tools.out_layout(v, args.output, None)
    return v


def out_depth_of(args):
    """--out-depth as VideoFI_IO takes it: None (the source's depth), 8 or 16.  A namespace built without the flag means None."""
    v = getattr(args, "out_depth", "source")
    if v in (None, "source"):
        return None
    if str(v) not in ("8", "16"):
        raise ValueError(f"--out-depth must be source, 8 or 16, got {v!r}")
    return int(v)


def load_model(model_type, scale=1.0, device=None, weights=None):
    """Model factory (reference infer.py:39-55); unknown type -> ValueError."""
    kw = {} if device is None else {"device": device}
    if model_type == "rife":
        from drba_amd.models.rife import RIFE
        return RIFE(weights=weights or r"weights/train_log_rife_426_heavy", scale=scale, **kw)
    if model_type == "gmfss":
        from drba_amd.models.gmfss import GMFSS
        return GMFSS(weights=weights or r"weights/train_log_gmfss", scale=scale, **kw)
    if model_type == "gmfss_union":
        from drba_amd.models.gmfss_union import GMFSS_UNION
        return GMFSS_UNION(weights=weights or r"weights/train_log_gmfss_union", scale=scale, **kw)
    raise ValueError(f"model_type must in {model_type}")


def interpolate_stream(model, video_io, dst_fps, times=-1, enable_scdet=False, scdet_threshold=0.3,
                       to_inp=None, to_out=None, check_scene=None, on_step=None, linear=True, dedup=None, check_dup=None, on_kept=None,
                       crop=None):
    """Run the whole clip: drba_amd.driver.run from a cold start, head and tail included.  Returns the number of frames written.
    linear=False: every DRBA step with the non-linear DistanceRatioMap (--nonlinear).
    dedup (--dedup; None: off, True: the defaults, a drba_amd.dedup.Settings or a dict of its fields): repeated source frames are
    dropped before the model sees them and the steps are retimed across the gaps -- the same number of frames at the same instants is
    written (drba_amd.dedup).  check_dup(a, b) -> bool replaces the device test; on_kept(k) fires for every kept source index k, in
    order; on_step then fires once per source frame the finished steps have passed (a progress bar counts source frames).
    crop (--crop; a drba_amd.crop.Box, with hooks built for it: frames.hooks(..., crop=box)): the network size is computed from the box
    instead of the frame; to_out is still given the frame's size, which is the size of what it writes."""
    to_inp = to_inp or _tools.to_inp
    to_out = to_out or _tools.to_out
    src_fps = video_io.src_fps
    if dst_fps <= src_fps:
        raise ValueError(f"dst fps should be greater than src fps, but got dst_fps={dst_fps} and src_fps={src_fps}")

    written = 0

    def emit(frames):
        nonlocal written
        for x in frames:
            video_io.write_frame(to_out(x, src_size))
            written += 1

    def sizes(raw):  # the frame's size, and the network size of what the model sees of it
        s = _tools.get_valid_net_inp_size(raw, model.scale, div=model.pad_size)
        if crop is not None:
            s["dst_size"] = _tools.get_valid_net_inp_size(SimpleNamespace(shape=tuple(crop.size)), model.scale, div=model.pad_size)["dst_size"]
        return s

    mapper = _tools.TMapper(src_fps, dst_fps, times)
    cuts = driver.SceneCuts(enable_scdet, scdet_threshold, check_scene)
    settings = _dedup.settings_of(dedup)
    if settings is not None:
        size = {}

        def convert(raw):
            if not size:
                size.update(sizes(raw))
            return to_inp(raw, size["dst_size"])

        def intake():  # the stream driver.run takes its frames in on, when the model offers one (decided once the first frame is here)
            if not (getattr(model, "supports_lookahead", False) and getattr(model, "prefetch_frame", None) is not None):
                return None
            offer = getattr(model, "intake_stream", None)
            import torch
            if offer is None or not torch.cuda.is_available():
                return None
            dev = getattr(model, "device", None)
            return offer(torch.device("cuda", torch.cuda.current_device()) if dev is None else dev)

        kept = driver.KeptFrames(lambda k: video_io.read_frame(), convert, settings, check_dup=check_dup, stream=intake, on_kept=on_kept)
        pair = [kept.next(), kept.next()]
        src_size = size["src_size"]
        sched = _dedup.Retimed(lambda idx: _tools.calc_t(idx, times, mapper), kept.kept, lambda: kept.total)
        passed = -1

        def step(idx):  # step s of the driver (head 0, iteration u: u + 1, the tail last) has passed source frame k_s, the tail all
            nonlocal passed
            upto = kept.kept[idx] if idx < len(kept.kept) - 1 or kept.total is None else kept.total - 1
            if on_step is not None:
                for j in range(passed + 1, upto + 1):
                    on_step(j)
            passed = max(passed, upto)

        driver.run(model, lambda k: kept.next(), pair, 0, to_inp=lambda x: x, emit=emit, cuts=cuts, ts_of=sched.ts_of, on_step=step,
                   linear=linear, even_of=sched.even_of)
        return written

    i0, i1 = video_io.read_frame(), video_io.read_frame()
    size = sizes(i0)
    src_size, dst_size = size["src_size"], size["dst_size"]
    driver.run(model, lambda k: video_io.read_frame(), [to_inp(i0, dst_size), to_inp(i1, dst_size)], 0,
               to_inp=lambda raw: to_inp(raw, dst_size), emit=emit, cuts=cuts,
               ts_of=lambda idx: _tools.calc_t(idx, times, mapper), on_step=on_step, linear=linear)
    return written


def inference(model, args):
    apply_deterministic(args)
    depth_kw = {} if out_depth_of(args) is None else {"out_depth": out_depth_of(args)}
    for flag, dflt in (("yuv_matrix", "bt709"), ("yuv_range", "source")):  # a namespace built without the flags means the defaults
        if getattr(args, flag, dflt) != dflt:
            depth_kw[flag] = getattr(args, flag)
    if out_chroma_of(args) != "source":
        depth_kw["out_chroma"] = out_chroma_of(args)
    video_io = _tools.VideoFI_IO(args.input, args.output, dst_fps=args.dst_fps, times=args.times, hwaccel=args.hwaccel, **depth_kw)
    try:
        from tqdm import tqdm
        bar = tqdm(total=video_io.total_frames_count)
        step = lambda _i: bar.update(1)  # noqa: E731
    except ImportError:
        bar, step = None, None
    if video_io.sink_format.rgb:  # encoder pipe / raw sink: BGR -> RGB inside the to_out kernel, not on the host
        video_io.frames_are_rgb = True
    # the hooks carry what the two ends' frames are (depth and maxval, planar 4:2:0, RGB order) and --fit: the loop between them
    # never looks at a frame, and a plain 8-bit resize run makes the calls it always made
    try:
        box = crop_box(args, video_io)  # --crop: None, the box given, or the one a scan of the clip finds
    except ValueError:
        video_io.close()
        raise
    to_inp, to_out = _frames.hooks(video_io.src_format, video_io.sink_format, fit_of(args), **({} if box is None else {"crop": box}))
    n = interpolate_stream(model, video_io, args.dst_fps, times=args.times, enable_scdet=args.enable_scdet,
                           scdet_threshold=args.scdet_threshold, to_inp=to_inp, to_out=to_out, on_step=step,
                           linear=not getattr(args, "nonlinear", False), dedup=dedup_of(args), **({} if box is None else {"crop": box}))
    while not video_io.finish_writing():
        time.sleep(0.01)
    video_io.close()
    if bar is not None:
        bar.close()
    return n


def inference_sharded(model, args, rank, world, to_inp=None, to_out=None, check_scene=None, device=None, chunk=4):
    """ONE clip frame-sharded over the ranks of a torch.distributed job (not in the reference, which has no parallelism;
    BASELINE.json configs[4]).  Every rank opens the clip (random access: .npz / .npy sources), runs its contiguous share
    of the driver loop with the one-frame halo of drba_amd.parallel.interpolate_shard, and the finished uint8 frames
    stream to rank 0 -- the writer -- through StreamedGather (the only collective: RCCL over xGMI on the GPUs).  The file
    rank 0 writes equals the single-process run's.  Returns the number of frames written (rank 0), 0 elsewhere."""
    import numpy as np

    from drba_amd import parallel
    # every rank sees the same flag: all of them refuse here, before the clip is opened, the gather exists or any collective runs
    if dedup_of(args) is not None:
        raise ValueError("the frame-sharded run does not take --dedup (which frames are kept decides every rank's share of the clip "
                         "and its schedule): run --dedup on one GPU")
    if crop_of(args) is not None:
        raise ValueError("the frame-sharded run does not take --crop (the ranks' hooks and the gather carry whole frames): run --crop on "
                         "one GPU")
    apply_deterministic(args)
    if os.path.splitext(args.input)[1].lower() not in (".npz", ".npy"):
        raise RuntimeError("the frame-sharded run needs random access to the clip: use a .npz / .npy source")
    frames, fps, _ = _frames.open_array_clip(args.input)
    fps = 24.0 if fps is None else fps
    # every rank sees the same clip and the same flag: all of them refuse here, before the gather exists and before any collective
    if frames.dtype == np.uint16 or out_depth_of(args) == 16:
        raise ValueError(f"the frame-sharded run carries 8-bit frames only (the gather to the writer moves uint8): {args.input} holds "
                         f"{frames.dtype} frames, --out-depth is {getattr(args, 'out_depth', 'source')}; run 16-bit clips on one GPU")
    counts = parallel.emission_counts(len(frames), fps, args.dst_fps, args.times, world)
    sg = parallel.StreamedGather(rank, world, counts, chunk=chunk, device=device, frame_shape=tuple(frames[0].shape))
    # the default hooks of the shard: 8-bit BGR frames and --fit, as in inference (hooks the caller gives are the caller's).  On the
    # GPUs finished frames stay on the device until the gather has moved them (tools.to_out would copy each one to the host only
    # for StreamedGather to copy it back): the uint8 frame is written straight into the send path
    bgr8 = _frames.FrameFormat()
    inp, out = _frames.hooks(bgr8, bgr8, fit_of(args), on_device=world > 1 and device is not None and device.type == "cuda")
    to_inp, to_out = to_inp or inp, to_out or out
    parallel.interpolate_shard(model, frames, fps, args.dst_fps, rank, world, times=args.times, enable_scdet=args.enable_scdet,
                               scdet_threshold=args.scdet_threshold, to_inp=to_inp, to_out=to_out, check_scene=check_scene,
                               sink=sg.push, linear=not getattr(args, "nonlinear", False))
    allf = sg.finish()
    if rank != 0:
        return 0
    video_io = _tools.VideoFI_IO(args.input, args.output, dst_fps=args.dst_fps, times=args.times, hwaccel=args.hwaccel)
    for f in allf:
        video_io.write_frame(f.cpu().numpy() if hasattr(f, "cpu") else f)
    while not video_io.finish_writing():
        time.sleep(0.01)
    video_io.close()
    return len(allf)


def main(argv=None):
    """`python infer.py ...` = the reference CLI.  Under torch.distributed.run (WORLD_SIZE > 1, one rank per GPU) the same
    command line shards the clip over the ranks: `python -m torch.distributed.run --nproc-per-node 8 infer.py -m rife ...`."""
    args = parse_args(argv)
    if args.input != "-" and not os.path.exists(args.input):
        raise FileNotFoundError(f"can't find the video file {args.input}")
    # the command line keeps the conv autotuner's winners across runs unless DRBA_TUNE_CACHE=0 (drba_amd/tunecache.py; the library
    # alone leaves the store off); nothing is written before the first winner is stored
    from drba_amd import tunecache
    tunecache.default_on()
    out_chroma_of(args)  # refuses --out-chroma with a sink that is not Y4M before the model is built
    apply_deterministic(args)  # before the model is built: nothing it does at load is timed in this mode
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != 1 and check_crop(args) is not None:  # every rank, before the process group exists
        raise ValueError("the frame-sharded run does not take --crop: run --crop on one GPU")
    if world == 1:
        plan_crop(args)  # refuses what --crop can be refused for, and finds / validates the box of a file source, before the model is built
        model = load_model(args.model_type, scale=args.scale)
        return inference(model, args)
    import torch
    import torch.distributed as dist
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(local)
    dist.init_process_group(backend="nccl")  # RCCL over xGMI
    try:
        model = load_model(args.model_type, scale=args.scale, device=torch.device("cuda", local))
        return inference_sharded(model, args, rank, world, device=torch.device("cuda", local))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
