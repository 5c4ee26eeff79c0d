"""CPU: --crop without a device -- the box arithmetic of drba_amd/crop.py (parse, the box rule, union, outward alignment, the numpy
reference of the statistic, a scan with that reference), the flags and their refusals, the keyword the hooks carry, the C entries'
argument checks, and a host round trip through interpolate_stream with stand-in conversions."""
import argparse
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

from drba_amd import _lib, crop, evaluate, frames
from drba_amd import infer as drv
from drba_amd.crop import Box
from drba_amd.models.utils import tools


# ------------------------------------------------------------------------------------------------------------------------ parse
def test_parse_takes_ffmpegs_order_and_cropdetects_line():
    assert crop.parse("1440:1080:240:0") == Box(1440, 1080, 240, 0)
    assert crop.parse("crop=1440:1080:240:0") == Box(1440, 1080, 240, 0)
    b = crop.parse(" crop=100:60:6:4 ", frame_size=(70, 118))
    assert (b.w, b.h, b.x, b.y) == (100, 60, 6, 4) and b.window == (6, 4, 100, 60) and b.size == (60, 100) and str(b) == "100:60:6:4"


@pytest.mark.parametrize("text", ["", "auto?", "1440:1080:240", "1440:1080:240:0:1", "1440x1080+240+0", "1440:1080:-240:0", "-4:8:0:0",
                                  "0:1080:0:0", "1440:0:0:0", "a:b:c:d", "1.5:2:0:0", "crop=", "crop=:::"])
def test_parse_rejects_malformed_and_negative_boxes(text):
    with pytest.raises(ValueError, match="crop box"):
        crop.parse(text)


@pytest.mark.parametrize("text", ["1440:1080:481:0", "1440:1081:240:0", "1921:1080:0:0", "8:8:1920:0", "8:8:0:1080"])
def test_parse_rejects_a_box_outside_the_frame(text):
    assert crop.parse(text) is not None  # well-formed in itself
    with pytest.raises(ValueError, match="does not lie inside the 1920x1080 frame"):
        crop.parse(text, frame_size=(1080, 1920))


# ------------------------------------------------------------------------------------------------------------------ the box rule
def _maxima(h, w, rows, cols, value, floor=0):
    r, c = np.full(h, floor, np.int64), np.full(w, floor, np.int64)
    r[rows[0]:rows[1]] = value
    c[cols[0]:cols[1]] = value
    return r, c


def test_box_rule_first_to_last_row_and_column_above_the_threshold():
    r, c = _maxima(20, 30, (4, 15), (6, 27), 200, floor=16)
    assert crop.box_of(r, c, 24) == Box(21, 11, 6, 4)
    r[9], c[12] = 0, 0  # a dark row and column INSIDE the picture change nothing
    assert crop.box_of(r, c, 24) == Box(21, 11, 6, 4)
    r[17] = 25  # one more row above the threshold, past a gap: the box runs to it
    assert crop.box_of(r, c, 24) == Box(21, 14, 6, 4)


def test_threshold_is_bar_threshold_plus_one_is_picture():
    assert crop.threshold_of(crop.LIMIT, 255) == 24 and crop.threshold_of(crop.LIMIT, 1023) == 96 and crop.threshold_of(crop.LIMIT, 65535) == 6168
    assert crop.threshold_of(0.0, 255) == 0
    for bad in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError, match="crop-limit"):
            crop.threshold_of(bad, 255)
    r, c = _maxima(8, 8, (2, 6), (2, 6), 24)
    assert crop.box_of(r, c, 24) is None  # a sample EQUAL to the threshold is bar
    r, c = _maxima(8, 8, (2, 6), (2, 6), 25)
    assert crop.box_of(r, c, 24) == Box(4, 4, 2, 2)


def test_empty_frame_and_picture_touching_each_edge():
    assert crop.box_of(np.zeros(8), np.zeros(12), 24) is None
    assert crop.box_of(np.full(8, 24), np.full(12, 24), 24) is None
    for rows, cols, want in (((0, 3), (4, 8), Box(4, 3, 4, 0)), ((5, 8), (4, 8), Box(4, 3, 4, 5)), ((2, 6), (0, 5), Box(5, 4, 0, 2)),
                             ((2, 6), (7, 12), Box(5, 4, 7, 2)), ((0, 8), (0, 12), Box(12, 8, 0, 0))):
        assert crop.box_of(*_maxima(8, 12, rows, cols, 255), 24) == want


def test_union_ignores_empty_frames():
    a, b = Box(10, 8, 4, 2), Box(6, 12, 12, 0)
    assert crop.union([a]) == a
    assert crop.union([None, a, None, b, None]) == Box(14, 12, 4, 0)
    assert crop.union([None, None]) is None and crop.union([]) is None


def _luma_clip(boxes, h=24, w=40, bar=16, pic=180):
    """frames [N,h,w,3] uint8, each black (`bar`) with `pic` inside its box (None: an empty frame)"""
    out = np.full((len(boxes), h, w, 3), bar, np.uint8)
    for k, b in enumerate(boxes):
        if b is not None:
            out[k, b.y:b.y + b.h, b.x:b.x + b.w] = pic
    return out


class _Clip(list):
    maxval, pixfmt = 255, "bgr"


def test_scan_gives_the_union_none_for_all_empty_and_none_for_the_whole_frame():
    stat = crop.edge_max_numpy
    clip = _Clip(_luma_clip([Box(10, 8, 6, 4), None, Box(12, 6, 8, 5)]))
    seen = []
    assert crop.scan(clip, stat=stat, on_frame=lambda k, b: seen.append((k, b))) == Box(14, 8, 6, 4)
    assert seen == [(0, Box(10, 8, 6, 4)), (1, None), (2, Box(12, 6, 8, 5))]
    assert crop.scan(_Clip(_luma_clip([None, None, None])), stat=stat) is None  # all frames empty
    assert crop.scan(_Clip(_luma_clip([Box(40, 24, 0, 0)])), stat=stat) is None  # the union is the frame
    assert crop.scan(_Clip(_luma_clip([Box(40, 10, 0, 0), Box(12, 24, 3, 0)])), stat=stat) is None  # ... only as a union
    assert crop.scan(_Clip(_luma_clip([Box(39, 24, 0, 0)])), stat=stat) == Box(39, 24, 0, 0)
    assert crop.scan(_Clip(_luma_clip([Box(39, 24, 0, 0)])), stat=stat, align=(2, 2)) is None  # grown outward to the whole frame
    assert crop.scan(_Clip(_luma_clip([Box(9, 7, 7, 5)])), stat=stat, align=(2, 2)) == Box(10, 8, 6, 4)
    assert crop.scan(_Clip(_luma_clip([Box(10, 8, 6, 4)], bar=30)), stat=stat, limit=0.2) == Box(10, 8, 6, 4)  # limit 0.2: 51


def test_edge_max_numpy_reference():
    rng = np.random.default_rng(0)
    f = rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    r, c = crop.edge_max_numpy(f)
    assert np.array_equal(r, f.reshape(5, -1).max(axis=1)) and np.array_equal(c, f.max(axis=(0, 2))) and c.shape == (7,)
    r, c = crop.edge_max_numpy(f[:, :, 0])
    assert np.array_equal(r, f[:, :, 0].max(axis=1)) and np.array_equal(c, f[:, :, 0].max(axis=0))
    r, c = crop.edge_max_numpy(f.reshape(5, 21), group=3)
    assert np.array_equal(c, f.max(axis=(0, 2)))
    with pytest.raises(ValueError):
        crop.edge_max_numpy(f.reshape(5, 21), group=4)


# -------------------------------------------------------------------------------------------------------------------- alignment
F8 = frames.FrameFormat()


def _fmt(pixfmt):
    return frames.FrameFormat(pixfmt)


def test_alignment_is_the_larger_subsampling_of_the_two_ends():
    assert crop.alignment_of(F8, F8) == (1, 1) and crop.alignment_of("bgr") == (1, 1)
    assert crop.alignment_of(_fmt("yuv420"), _fmt("yuv420")) == (2, 2)
    assert crop.alignment_of(_fmt("yuv422"), _fmt("yuv422")) == (2, 1)
    assert crop.alignment_of(_fmt("yuv444"), _fmt("yuv444")) == (1, 1)
    assert crop.alignment_of(_fmt("yuv444"), _fmt("yuv420")) == (2, 2) and crop.alignment_of(F8, _fmt("yuv420")) == (2, 2)
    assert crop.alignment_of(_fmt("yuv422"), F8) == (2, 1) and crop.alignment_of(_fmt("yuv444"), _fmt("yuv422")) == (2, 1)


def test_aligned_grows_outward_and_clamps_at_an_odd_frame_edge():
    b = Box(9, 7, 7, 5)  # x 7..16, y 5..12
    assert crop.aligned(b, (24, 40), (2, 2)) == Box(10, 8, 6, 4)      # 4:2:0: both axes
    assert crop.aligned(b, (24, 40), (2, 1)) == Box(10, 7, 6, 5)      # 4:2:2: x only
    assert crop.aligned(b, (24, 40), (1, 1)) == b                     # 4:4:4 and packed: none
    assert crop.aligned(Box(8, 6, 6, 4), (24, 40), (2, 2)) == Box(8, 6, 6, 4)  # already aligned
    # an odd frame: the box's far edge would be rounded past the frame's own, and is clamped to it
    assert crop.aligned(Box(30, 18, 9, 5), (23, 39), (2, 2)) == Box(31, 19, 8, 4)
    assert crop.aligned(Box(30, 17, 9, 5), (23, 39), (2, 2)) == Box(31, 18, 8, 4)


def test_aligned_box_always_contains_the_box():
    for fh, fw in ((23, 39), (24, 40), (7, 5)):
        for ax, ay in ((1, 1), (2, 1), (2, 2), (4, 2)):
            for x in range(0, fw, 3):
                for y in range(0, fh, 3):
                    for w in (1, 2, 5, fw - x):
                        for h in (1, 3, 4, fh - y):
                            if x + w > fw or y + h > fh:
                                continue
                            b = Box(w, h, x, y)
                            a = crop.aligned(b, (fh, fw), (ax, ay))
                            assert a.contains(b) and a.inside((fh, fw)), (b, a)
                            assert a.x % ax == 0 and a.y % ay == 0
                            assert (a.x + a.w) % ax == 0 or a.x + a.w == fw
                            assert (a.y + a.h) % ay == 0 or a.y + a.h == fh
                            crop.validate(a, (fh, fw), (ax, ay))  # what the scan returns is what an explicit box must be


def test_validate_names_the_multiple():
    crop.validate(Box(100, 60, 8, 6), (72, 120), (2, 2))
    crop.validate(Box(111, 65, 8, 6), (71, 119), (2, 2))  # odd extents that reach the frame's edges
    with pytest.raises(ValueError, match="X and W must be multiples of 2"):
        crop.validate(Box(100, 60, 7, 6), (72, 120), (2, 2))
    with pytest.raises(ValueError, match="Y and H must be multiples of 2.*crop=100:62:8:6"):
        crop.validate(Box(100, 61, 8, 6), (72, 120), (2, 2))
    crop.validate(Box(100, 61, 8, 5), (72, 120), (2, 1))
    with pytest.raises(ValueError, match="does not lie inside"):
        crop.validate(Box(100, 60, 30, 6), (72, 120), (1, 1))


# ------------------------------------------------------------------------------------------------------------------- the flags
def test_cli_flags_parse_and_a_bare_namespace_means_off():
    a = drv.parse_args(["-i", "x.npz", "-o", "y.npz"])
    assert a.crop == "off" and drv.crop_of(a) is None and a.crop_limit == 24 / 255 == crop.LIMIT
    assert drv.crop_of(argparse.Namespace()) is None and drv.crop_limit_of(argparse.Namespace()) == crop.LIMIT
    a = drv.parse_args(["-i", "x.npz", "-o", "y.npz", "--crop", "auto", "--crop-limit", "0.05", "-s", "--dedup", "--nonlinear",
                        "--deterministic", "--fit", "pad", "--out-depth", "16"])
    assert drv.crop_of(a) == "auto" and drv.crop_limit_of(a) == 0.05
    a = drv.parse_args(["-i", "-", "-o", "-", "--crop", "crop=1440:1080:240:0"])
    assert drv.crop_of(a) == Box(1440, 1080, 240, 0) and drv.check_crop(a) == Box(1440, 1080, 240, 0)  # explicit: any source
    with pytest.raises(ValueError, match="crop box"):
        drv.crop_of(drv.parse_args(["-i", "x.npz", "-o", "y.npz", "--crop", "on"]))
    with pytest.raises(ValueError, match="crop-limit"):
        drv.check_crop(drv.parse_args(["-i", "x.npz", "-o", "y.npz", "--crop", "auto", "--crop-limit", "1.5"]))


@pytest.mark.parametrize("inp", ["-", "film.mkv"])
def test_auto_is_refused_for_sources_that_cannot_be_read_twice_before_a_model_is_built(tmp_path, monkeypatch, inp):
    if inp != "-":
        inp = str(tmp_path / inp)
        open(inp, "wb").close()
    built = []
    monkeypatch.setattr(drv, "load_model", lambda *a, **k: built.append(a) or object())
    monkeypatch.setenv("DRBA_TUNE_CACHE", "0")
    with pytest.raises(ValueError, match=r"python -m drba_amd\.evaluate bars.*--crop W:H:X:Y"):
        drv.main(["-m", "rife", "-i", inp, "-o", str(tmp_path / "out.y4m"), "-t", "2", "--crop", "auto"])
    assert not built and not os.path.exists(str(tmp_path / "out.y4m"))


def test_explicit_misaligned_box_is_refused_before_a_model_is_built(tmp_path, monkeypatch):
    from tests import metrics_yuv_common as myc
    inp = str(tmp_path / "in.y4m")
    myc.write_clip(inp, myc.random_clip(3, 72, 120, 8, seed=1))
    built = []
    monkeypatch.setattr(drv, "load_model", lambda *a, **k: built.append(a) or object())
    monkeypatch.setenv("DRBA_TUNE_CACHE", "0")
    with pytest.raises(ValueError, match="X and W must be multiples of 2"):
        drv.main(["-m", "rife", "-i", inp, "-o", str(tmp_path / "out.y4m"), "-t", "2", "--crop", "100:60:7:6"])
    with pytest.raises(ValueError, match="does not lie inside the 120x72 frame"):
        drv.main(["-m", "rife", "-i", inp, "-o", str(tmp_path / "out.y4m"), "-t", "2", "--crop", "100:60:30:6"])
    # a packed source into a 4:2:0 sink: the sink's layout asks for the multiple
    npz = str(tmp_path / "in.npz")
    np.savez(npz, frames=np.zeros((3, 72, 120, 3), np.uint8), fps=np.float64(24.0))
    with pytest.raises(ValueError, match="Y and H must be multiples of 2"):
        drv.main(["-m", "rife", "-i", npz, "-o", str(tmp_path / "out.y4m"), "-t", "2", "--crop", "100:60:8:7"])
    a = drv.parse_args(["-m", "rife", "-i", npz, "-o", str(tmp_path / "out.npz"), "-t", "2", "--crop", "100:59:7:7"])
    assert drv.plan_crop(a) == Box(100, 59, 7, 7) and a.crop == Box(100, 59, 7, 7)  # packed at both ends: no multiple is asked
    assert not built and not os.path.exists(str(tmp_path / "out.y4m"))


def test_sharded_run_refuses_crop(tmp_path):
    inp = str(tmp_path / "in.npz")
    np.savez(inp, frames=np.zeros((4, 16, 16, 3), dtype=np.uint8), fps=np.float64(24.0))
    for flag in ("auto", "8:8:4:4"):
        a = drv.parse_args(["-i", inp, "-o", str(tmp_path / "out.npz"), "-t", "2", "--crop", flag])
        for rank in (0, 1):
            with pytest.raises(ValueError, match="--crop"):
                drv.inference_sharded(object(), a, rank, 2)
    assert not os.path.exists(str(tmp_path / "out.npz"))


# ------------------------------------------------------------------------------------------------------------------- the hooks
def test_hooks_pass_window_only_with_a_box(monkeypatch):
    seen = []

    def closed_inp(frame, size):  # closed signatures: any keyword is a TypeError
        seen.append(("in", {}))
        return torch.zeros(1, 3, *size)

    def closed_out(x, size):
        seen.append(("out", {}))
        return np.zeros((*size, 3), np.uint8)

    monkeypatch.setattr(tools, "to_inp", closed_inp)
    monkeypatch.setattr(tools, "to_out", closed_out)
    to_inp, to_out = frames.hooks(F8, F8, "resize")
    to_out(to_inp(np.zeros((8, 8, 3), np.uint8), (32, 32)), (8, 8))
    to_inp, to_out = frames.hooks(F8, F8, "resize", crop=None)
    to_out(to_inp(np.zeros((8, 8, 3), np.uint8), (32, 32)), (8, 8))
    assert seen == [("in", {}), ("out", {})] * 2

    def open_inp(frame, size, **kw):
        seen.append(("in", kw))
        return torch.zeros(1, 3, *size)

    def open_out(x, size, **kw):
        seen.append(("out", kw))
        return np.zeros((*size, 3), np.uint8)

    del seen[:]
    monkeypatch.setattr(tools, "to_inp", open_inp)
    monkeypatch.setattr(tools, "to_out", open_out)
    to_inp, to_out = frames.hooks(F8, frames.FrameFormat("yuv422", 16, 1023), "pad", crop=Box(100, 60, 8, 6))
    to_out(to_inp(np.zeros((72, 120, 3), np.uint8), (64, 128)), (72, 120))
    assert seen[0] == ("in", {"fit": "pad", "window": (8, 6, 100, 60)})
    assert seen[1] == ("out", {"matrix": "bt709", "full_range": False, "depth": 16, "maxval": 1023, "pixfmt": "yuv422", "fit": "pad",
                               "window": (8, 6, 100, 60)})


def test_crop_loads_without_the_gpu_modules():
    import ast
    top = [n for n in ast.parse(open(crop.__file__).read()).body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name if isinstance(n, ast.Import) else n.module for n in top for a in n.names}
    assert names == {"math", "dataclasses", "numpy"}


# ------------------------------------------------------------------------------------------------------------- the C entries
def test_edge_max_and_window_entries_check_their_arguments():
    lib = _lib.load()
    buf = (C.c_uint32 * 256)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 1)
    for fn in (lib.drba_edge_max_u8, lib.drba_edge_max_u16):
        for args in ((None, 4, 12, 12, 3, p, p), (p, 4, 12, 12, 3, None, p), (p, 4, 12, 12, 3, p, None),   # null pointers
                     (p, 0, 12, 12, 3, p, p), (p, 4, 0, 12, 3, p, p), (p, -1, 12, 12, 3, p, p), (p, 4, 12, 12, 0, p, p),  # sizes
                     (p, 4, 12, 11, 3, p, p),                                                               # pitch < cols
                     (p, 4, 12, 12, 5, p, p), (p, 4, 13, 13, 3, p, p),                                      # cols % g != 0
                     (p, 4, 12, 12, 3, odd, p)):                                                            # a misaligned result
            assert fn(*args, None) == -1, args
    assert lib.drba_edge_max_u16(odd, 4, 12, 12, 3, p, p, None) == -1  # a misaligned u16 pointer
    f = C.c_float
    for fn, args in ((lib.drba_to_inp_win_x4, (p, 23, p, None, 8, 8, 8, 8, f(1), f(1))),       # pitch < 3 * Win
                     (lib.drba_to_inp16_win_x4, (p, 23, p, None, 8, 8, 8, 8, f(1), f(1), f(1023))),
                     (lib.drba_to_inp_pad_win_x4, (p, 0, p, None, 8, 8, 8, 8)),
                     (lib.drba_to_inp16_pad_win_x4, (odd, 24, p, None, 8, 8, 8, 8, f(1023))),   # a misaligned u16 frame
                     (lib.drba_to_out_win, (p, p, 23, 8, 8, 8, 8, f(1), f(1), 0)),
                     (lib.drba_to_out16_win, (p, p, 24, 8, 8, 8, 8, f(1), f(1), 0, f(100))),    # maxval
                     (lib.drba_to_out_crop_win, (p, p, 23, 8, 8, 8, 8, 0)),
                     (lib.drba_to_out16_crop_win, (p, None, 24, 8, 8, 8, 8, 0, f(1023)))):
        assert fn(*args, None) == -1, fn


def test_edge_max_has_no_cpu_fallback():
    from drba_amd import ops
    with pytest.raises(_lib.DrbaHipError):
        ops.edge_max(torch.zeros(4, 4, 3, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------ host round trip
class _Copy:  # "interpolates" by repeating the nearer frame: only the plumbing is under test
    scale, pad_size, supports_lookahead = 1.0, 64, False

    def inference_ts(self, I0, I1, ts):
        return [I0 if t < 0.5 else I1 for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, **kw):
        return [I0 if t < 0.5 else (I1 if t < 1.5 else I2) for t in ts], None


def _host_conversions(monkeypatch, fit):
    """tools.to_inp / tools.to_out on the host with the window semantics of the device's: the rectangle as if it were the frame"""
    import oracle
    sizes = []

    def place(t, size):
        if fit == "resize":
            return oracle.ops.resize(t, size)
        out = torch.zeros(1, 3, *size)
        out[:, :, :t.shape[2], :t.shape[3]] = t
        return out

    def to_inp(fr, size, window=None, **kw):
        assert kw == ({} if fit == "resize" else {"fit": fit})
        if window is not None:
            x, y, w, h = window
            fr = fr[y:y + h, x:x + w]
        sizes.append(tuple(size))
        return place(torch.from_numpy(np.ascontiguousarray(fr).transpose(2, 0, 1)).unsqueeze(0).float() / 255.0, size)

    def to_out(t, size, window=None, **kw):
        frame = np.zeros((*size, 3), np.uint8)
        x, y, w, h = (0, 0, size[1], size[0]) if window is None else window
        part = oracle.ops.resize(t, (h, w)) if fit == "resize" else t[:, :, :h, :w]
        frame[y:y + h, x:x + w] = (part[0].numpy().transpose(1, 2, 0) * 255.0 + 0.5).astype(np.uint8)
        return frame

    monkeypatch.setattr(tools, "to_inp", to_inp)
    monkeypatch.setattr(tools, "to_out", to_out)
    return sizes


@pytest.mark.parametrize("fit", ["resize", "pad"])
def test_host_round_trip_writes_source_sized_frames_with_black_bars(monkeypatch, fit):
    from drba_amd.utils import synth
    from tests.clip_common import ListIO
    box = Box(100, 60, 10, 6)
    inner = synth.make_clip(5, 60, 100, seed=3)
    clip = np.full((5, 72, 120, 3), 9, np.uint8)  # bars that are NOT black on the way in
    clip[:, 6:66, 10:110] = inner
    sizes = _host_conversions(monkeypatch, fit)
    to_inp, to_out = frames.hooks(F8, F8, fit, crop=box)
    sink = ListIO(list(clip), 24.0)
    n = drv.interpolate_stream(_Copy(), sink, 48.0, times=2, to_inp=to_inp, to_out=to_out, crop=box)
    assert n == len(sink.written) == 10
    assert set(sizes) == {(64, 128)}, "the network size follows from the 100x60 box, not from the 120x72 frame (128x128)"
    for fr in sink.written:
        assert fr.shape == (72, 120, 3) and fr.dtype == np.uint8  # the source's shape
        outside = fr.copy()
        outside[6:66, 10:110] = 0
        assert not outside.any(), "exact black outside the box"
    if fit == "pad":  # no resampling: the copied frames come back inside the box as they went in
        assert np.array_equal(sink.written[0][6:66, 10:110], inner[0])
    # the same clip without the box runs at the frame's network size
    del sizes[:]
    to_inp, to_out = frames.hooks(F8, F8, fit)
    drv.interpolate_stream(_Copy(), ListIO(list(clip), 24.0), 48.0, times=2, to_inp=to_inp, to_out=to_out)
    assert set(sizes) == {(128, 128)}
    # with --dedup the box decides the size as well
    del sizes[:]
    to_inp, to_out = frames.hooks(F8, F8, fit, crop=box)
    drv.interpolate_stream(_Copy(), ListIO(list(clip), 24.0), 48.0, times=2, to_inp=to_inp, to_out=to_out, crop=box, dedup=True,
                           check_dup=lambda a, b: False)
    assert set(sizes) == {(64, 128)}


def test_inference_resolves_auto_through_the_scan_and_says_when_there_is_nothing_to_crop(tmp_path, monkeypatch, capsys):
    """infer.inference with --crop auto: the scan (here with the numpy statistic in the device's place) gives the box the hooks and the
    loop get; a clip without bars runs as without the flag, with one line on stderr."""
    inner = np.random.default_rng(2).integers(40, 256, size=(4, 60, 100, 3), dtype=np.uint8)
    clip = np.zeros((4, 72, 120, 3), np.uint8)
    clip[:, 6:66, 10:110] = inner
    barred, full = str(tmp_path / "barred.npz"), str(tmp_path / "full.npz")
    np.savez(barred, frames=clip, fps=np.float64(24.0))
    np.savez(full, frames=inner, fps=np.float64(24.0))
    real_scan = crop.scan
    monkeypatch.setattr(crop, "scan", lambda src, limit, align, **kw: real_scan(src, limit, align, stat=crop.edge_max_numpy))
    windows, sizes = [], []

    def to_inp(fr, size, **kw):
        windows.append(kw.get("window"))
        sizes.append(tuple(size))
        return torch.zeros(1, 3, *size)

    monkeypatch.setattr(tools, "to_inp", to_inp)
    monkeypatch.setattr(tools, "to_out", lambda x, size, **kw: np.zeros((*size, 3), np.uint8))
    out = str(tmp_path / "out.npz")
    assert drv.inference(_Copy(), drv.parse_args(["-i", barred, "-o", out, "-t", "2", "--crop", "auto"])) == 8
    assert set(windows) == {(10, 6, 100, 60)} and set(sizes) == {(64, 128)}
    assert np.load(out)["frames"].shape == (8, 72, 120, 3)  # the sink's size and frame count are the source's
    assert "no bars" not in capsys.readouterr().err
    del windows[:], sizes[:]
    assert drv.inference(_Copy(), drv.parse_args(["-i", full, "-o", out, "-t", "2", "--crop", "auto"])) == 8
    assert set(windows) == {None} and set(sizes) == {(64, 128)}
    assert "--crop auto: no bars found" in capsys.readouterr().err


def test_evaluate_bars_prints_every_frame_and_the_union(tmp_path):
    clip = _luma_clip([Box(10, 8, 6, 4), None, Box(12, 6, 8, 5)])
    path = str(tmp_path / "c.npz")
    np.savez(path, frames=clip, fps=np.float64(24.0))
    text = io.StringIO()
    res = evaluate.bars(evaluate.ClipSource(path), stat=crop.edge_max_numpy, out=text)
    lines = text.getvalue().splitlines()
    assert [ln.split() for ln in lines[:3]] == [["0", "10:8:6:4"], ["1", "empty"], ["2", "12:6:8:5"]]
    assert lines[3].startswith("crop=14:8:6:4  11.7% of the 40x24 frame")
    assert res == {"boxes": ["10:8:6:4", None, "12:6:8:5"], "crop": "14:8:6:4", "share": 14 * 8 / (40 * 24), "frames": 3, "size": [24, 40]}
    a = evaluate.parse_args(["bars", path, "--crop-limit", "0.2"])
    assert (a.command, a.clip, a.crop_limit) == ("bars", path, 0.2)
