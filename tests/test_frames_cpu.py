"""CPU: drba_amd/frames.py -- the keyword sets every frame hook carries, the full-range rule and the array-clip reader.

The tables below were recorded from the commit before frames.py existed, by running that commit's infer.inference, evaluate.holdout
and evaluate.dups under the recorders of this file (open **kw signatures); the tests make the same runs and compare the keyword dicts
with `==`: a keyword more, a keyword less or a default spelled out is a failure."""
import json

import numpy as np
import pytest
import torch

from drba_amd import evaluate, frames, ops, y4m
from drba_amd import infer as drv
from drba_amd.models.utils import tools
from tests import depth16_common as d16
from tests import metric_checks as mc
from tests import metrics_yuv_common as myc
from tests import yuv_common as yc


# ---------------------------------------------------------------------------------------------------------------- the recorders
class _Copy:  # "interpolates" by repeating the nearer frame: only the plumbing is under test
    scale, pad_size, supports_lookahead = 1.0, 32, False

    def inference_ts(self, I0, I1, ts):
        return [I0 if t < 0.5 else I1 for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, **kw):
        return [I0 if t < 0.5 else (I1 if t < 1.5 else I2) for t in ts], None


def _blank(size, kw):
    """the frame a way out with these keywords returns: packed planes or [H,W,3], uint8 or uint16"""
    h, w = size
    dtype = np.uint16 if kw.get("depth", 8) == 16 else np.uint8
    if "matrix" in kw:  # (only a 4:2:0 way out names a matrix)
        return np.zeros(h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2), dtype)
    return np.zeros((h, w, 3), dtype)


@pytest.fixture()
def calls(monkeypatch):
    """tools.to_inp / tools.to_out and ops.to_out / ops.to_out_yuv replaced by recorders -> {"to_inp": [kw], "to_out": [(entry, kw)]}"""
    seen = {"to_inp": [], "to_out": []}

    def to_inp(fr, size, **kw):
        seen["to_inp"].append(dict(kw))
        return torch.zeros(1, 3, *size)

    def way_out(entry):
        def to_out(x, size, **kw):
            seen["to_out"].append((entry, dict(kw)))
            return _blank(size, kw)
        return to_out

    monkeypatch.setattr(tools, "to_inp", to_inp)
    monkeypatch.setattr(tools, "to_out", way_out("tools.to_out"))
    monkeypatch.setattr(ops, "to_out", way_out("ops.to_out"))
    monkeypatch.setattr(ops, "to_out_yuv", way_out("ops.to_out_yuv"))
    monkeypatch.setattr(ops, "check_overflow", lambda *a: None)
    return seen


def _one(records):
    """every call of a run carries the same keywords: that one set"""
    assert records and all(r == records[0] for r in records), records
    return records[0]


def _y4m_clip(path, n, h, w, bits, color_range=None):
    myc.write_clip(path, myc.random_clip(n, h, w, bits, seed=bits), color_range=color_range)
    return path


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    d, rng, shape = tmp_path_factory.mktemp("frames_src"), np.random.default_rng(3), (4, 30, 44, 3)
    p = {k: str(d / name) for k, name in (("u8", "in8.npz"), ("u16", "in16.npz"), ("y8", "in8.y4m"), ("y10", "in10.y4m"))}
    np.savez(p["u8"], frames=rng.integers(0, 256, size=shape, dtype=np.uint8), fps=np.float64(24.0))
    np.savez(p["u16"], frames=rng.integers(0, 1024, size=shape, dtype=np.uint16), fps=np.float64(24.0), maxval=np.int64(1023))
    _y4m_clip(p["y8"], 4, 30, 44, 8)
    _y4m_clip(p["y10"], 4, 30, 44, 10)
    return p


# --------------------------------------------------------------------------------------------------------------- infer.inference
YUV = {"matrix": "bt709", "full_range": False}
# source -> the keywords of tools.to_inp
INFERENCE_IN = {"u8": {}, "u16": {"maxval": 1023}, "y8": YUV, "y10": YUV}
# (sink, --out-depth) -> source -> the keywords of tools.to_out
INFERENCE_OUT = {
    ("out.npz", None): {"u8": {}, "u16": {"rgb": False, "depth": 16, "maxval": 1023}, "y8": {},
                        "y10": {"rgb": False, "depth": 16, "maxval": 1023}},
    ("out.npz", "16"): {"u8": {"rgb": False, "depth": 16, "maxval": 65535}, "u16": {"rgb": False, "depth": 16, "maxval": 1023},
                        "y8": {"rgb": False, "depth": 16, "maxval": 65535}, "y10": {"rgb": False, "depth": 16, "maxval": 1023}},
    ("out.raw", None): {"u8": {"rgb": True}, "u16": {"rgb": True, "depth": 16, "maxval": 1023}, "y8": {"rgb": True},
                        "y10": {"rgb": True, "depth": 16, "maxval": 1023}},
    ("out.raw", "16"): {"u8": {"rgb": True, "depth": 16, "maxval": 65535}, "u16": {"rgb": True, "depth": 16, "maxval": 1023},
                        "y8": {"rgb": True, "depth": 16, "maxval": 65535}, "y10": {"rgb": True, "depth": 16, "maxval": 1023}},
    ("out.y4m", None): {"u8": {"depth": 8, "maxval": None, "pixfmt": "yuv420", **YUV},
                        "u16": {"depth": 16, "maxval": 1023, "pixfmt": "yuv420", **YUV},
                        "y8": {"depth": 8, "maxval": None, "pixfmt": "yuv420", **YUV},
                        "y10": {"depth": 16, "maxval": 1023, "pixfmt": "yuv420", **YUV}},
    ("out.y4m", "16"): {s: {"depth": 16, "maxval": 1023, "pixfmt": "yuv420", **YUV} for s in ("u8", "u16", "y8", "y10")},
}
PAD = {"fit": "pad"}  # what --fit pad adds to every set above; --fit resize adds nothing


def _inference(tmp_path, calls, inp, sink, out_depth, fit, more=()):
    del calls["to_inp"][:], calls["to_out"][:]
    argv = ["-m", "rife", "-i", inp, "-o", str(tmp_path / sink), "-t", "2", "--fit", fit, *more]
    assert drv.inference(_Copy(), drv.parse_args(argv + (["--out-depth", out_depth] if out_depth else []))) == 8
    assert len(calls["to_inp"]) == 4 and len(calls["to_out"]) == 8
    entry, kw = _one(calls["to_out"])
    assert entry == "tools.to_out"
    return _one(calls["to_inp"]), kw


@pytest.mark.parametrize("sink,out_depth", list(INFERENCE_OUT), ids=[f"{s}-{d or 'source'}" for s, d in INFERENCE_OUT])
def test_inference_makes_the_calls_it_made(tmp_path, calls, sources, sink, out_depth):
    for src, path in sources.items():
        for fit, extra in (("resize", {}), ("pad", PAD)):
            kin, kout = _inference(tmp_path, calls, path, sink, out_depth, fit)
            assert kin == {**INFERENCE_IN[src], **extra}, (src, fit)
            assert kout == {**INFERENCE_OUT[sink, out_depth][src], **extra}, (src, fit)


def test_inference_names_the_conversion_the_flags_name(tmp_path, calls, sources):
    kin, kout = _inference(tmp_path, calls, sources["y8"], "out.y4m", None, "resize", ["--yuv-matrix", "bt601", "--yuv-range", "full"])
    assert kin == {"matrix": "bt601", "full_range": True}
    assert kout == {"depth": 8, "maxval": None, "pixfmt": "yuv420", "matrix": "bt601", "full_range": True}


def test_video_io_describes_both_ends(tmp_path, sources):
    io = tools.VideoFI_IO(sources["y10"], str(tmp_path / "o.raw"), times=2, out_depth=8, yuv_matrix="bt601")
    try:
        assert io.src_format == frames.FrameFormat("yuv420", 16, 1023, "bt601", False)
        assert io.sink_format == frames.FrameFormat("bgr", 8, 255, "bt601", False, rgb=True)
        assert (io.depth, io.maxval, io.pixfmt, io.out_depth, io.out_maxval, io.out_pixfmt, io.wants_rgb) == (16, 1023, "yuv420", 8, 255, "bgr", True)
    finally:
        io.close()
    with pytest.raises(AttributeError):  # a frozen record
        io.src_format.depth = 8


# ------------------------------------------------------------------------------------------------------------ evaluate.holdout
# clip -> (the keywords of tools.to_inp, the device entry of the way out, its keywords)
HOLDOUT = {
    "u8": ({}, "ops.to_out", {}),
    "u16": ({"maxval": 65535}, "ops.to_out", {"depth": 16, "maxval": 65535}),
    "u16-1023": ({"maxval": 1023}, "ops.to_out", {"depth": 16, "maxval": 1023}),
    "y8": (YUV, "ops.to_out_yuv", {**YUV, "depth": 8, "maxval": None}),
    "y10": (YUV, "ops.to_out_yuv", {**YUV, "depth": 16, "maxval": 1023}),
}


def _holdout_clip(tmp_path, kind, color_range=None):
    """-> (what holdout takes, its keywords, the metrics back-end): 7 frames of 10 x 14 (below the SSIM window: nothing to compute)"""
    rng = np.random.default_rng(5)
    if kind == "u8":
        return rng.integers(0, 256, size=(7, 10, 14, 3), dtype=np.uint8), {}, mc.NumpyBackend()
    if kind.startswith("u16"):
        kw = {"maxval": 1023} if kind == "u16-1023" else {}
        return rng.integers(0, 1024, size=(7, 10, 14, 3), dtype=np.uint16), kw, d16.NumpyBackend16()
    path = _y4m_clip(str(tmp_path / f"{kind}.y4m"), 7, 10, 14, 8 if kind == "y8" else 10, color_range)
    return evaluate.ClipSource(path), {}, myc.NumpyYuvBackend()


def _holdout(calls, clip, fit="resize", **kw):
    del calls["to_inp"][:], calls["to_out"][:]
    res = evaluate.holdout(_Copy(), clip, 3, fit=fit, **kw)
    assert len(calls["to_inp"]) == 3 and len(calls["to_out"]) == 9
    return res, _one(calls["to_inp"]), _one(calls["to_out"])


@pytest.mark.parametrize("kind", list(HOLDOUT))
def test_holdout_default_hooks_make_the_calls_they_made(tmp_path, calls, kind):
    clip, kw, be = _holdout_clip(tmp_path, kind)
    for fit, extra in (("resize", {}), ("pad", PAD)):
        _, kin, (entry, kout) = _holdout(calls, clip, fit, backend=be, **kw)
        assert (kin, entry, kout) == ({**HOLDOUT[kind][0], **extra}, HOLDOUT[kind][1], {**HOLDOUT[kind][2], **extra}), fit


def test_holdout_leaves_the_callers_hooks_alone(tmp_path, calls):
    clip, _, be = _holdout_clip(tmp_path, "u16")
    mine = []
    evaluate.holdout(_Copy(), clip, 3, fit="pad", backend=be, to_inp=lambda fr, size: mine.append("in") or torch.zeros(1, 3, *size),
                     to_out=lambda x, size: mine.append("out") or np.zeros((*size, 3), np.uint16))
    assert mine.count("in") == 3 and mine.count("out") == 9 and not calls["to_inp"] and not calls["to_out"]
    with pytest.raises(ValueError, match="maxval belongs to uint16 frames"):
        evaluate.holdout(_Copy(), _holdout_clip(tmp_path, "u8")[0], 3, backend=mc.NumpyBackend(), maxval=1023)


# --------------------------------------------------------------------------------------------------------------- evaluate.dups
# clip -> the keywords of tools.to_inp
DUPS = {"u8": {}, "u16": {"maxval": 1023}, "y8": YUV, "y10": YUV}


def _dups(calls, path, fit="resize", **kw):
    del calls["to_inp"][:]
    res = evaluate.dups(evaluate.ClipSource(path), fit=fit, stats=lambda a, b, lo: (0.0, 0, 1), **kw)
    assert res["frames"] == len(calls["to_inp"])
    return _one(calls["to_inp"])


def test_dups_makes_the_calls_it_made(calls, sources):
    for src, path in sources.items():
        assert _dups(calls, path) == DUPS[src] and _dups(calls, path, "pad") == {**DUPS[src], **PAD}, src
    assert _dups(calls, sources["y8"], yuv_matrix="bt601", yuv_range="full") == {"matrix": "bt601", "full_range": True}


# ----------------------------------------------------------------------------------------------------------- the full-range rule
# (XCOLORRANGE of the header, --yuv-range) -> (infer.py: the way in, the way out; evaluate holdout / dups: both ways).  The two differ
# where the flag names a range and the header carries the other one: infer.py reads the clip by its tag, evaluate by the flag.
FULL_RANGE = {
    (None, "source"): (False, False, False), (None, "limited"): (False, False, False), (None, "full"): (True, True, True),
    ("LIMITED", "source"): (False, False, False), ("LIMITED", "limited"): (False, False, False), ("LIMITED", "full"): (False, True, True),
    ("FULL", "source"): (True, True, True), ("FULL", "limited"): (True, False, False), ("FULL", "full"): (True, True, True),
}


@pytest.mark.parametrize("tag", [None, "LIMITED", "FULL"])
def test_full_range_rule_of_both_callers(tmp_path, calls, tag):
    clip, _, be = _holdout_clip(tmp_path, "y8", color_range=tag)
    for flag in ("source", "limited", "full"):
        way_in, way_out, ev = FULL_RANGE[tag, flag]
        io = tools.VideoFI_IO(clip.path, str(tmp_path / "o.y4m"), times=2, yuv_range=flag)
        try:
            assert (io.yuv_full_range, io.out_full_range) == (way_in, way_out), flag
            assert (io.src_format.full_range, io.sink_format.full_range) == (way_in, way_out), flag
        finally:
            io.close()
        assert frames.full_range(flag, tag, tag_wins=True) is way_in and frames.full_range(flag, tag, tag_wins=False) is ev, flag
        res, kin, (_, kout) = _holdout(calls, clip, backend=be, yuv_range=flag)
        assert (res["full_range"], kin["full_range"], kout["full_range"]) == (ev, ev, ev), flag
        assert _dups(calls, clip.path, yuv_range=flag)["full_range"] is ev, flag
    with pytest.raises(ValueError, match="yuv_range must be source, limited or full"):
        frames.full_range("video", tag, tag_wins=True)


# ------------------------------------------------------------------------------------------------------------ open_array_clip
def test_open_array_clip(tmp_path):
    fr = np.random.default_rng(1).integers(0, 1024, size=(3, 6, 8, 3), dtype=np.uint16)
    full, bare = str(tmp_path / "full.npz"), str(tmp_path / "bare.npz")
    np.savez(full, frames=fr, fps=np.float64(30.0), maxval=np.int64(1023))
    np.savez(bare, frames=fr)
    got, fps, maxval = frames.open_array_clip(full)
    assert np.array_equal(got, fr) and (fps, maxval) == (30.0, 1023) and type(fps) is float and type(maxval) is int
    got, fps, maxval = frames.open_array_clip(bare)
    assert np.array_equal(got, fr) and fps is None and maxval is None
    for name, meta, want in (("side.npy", {"fps": 25, "maxval": 4095}, (25.0, 4095)), ("half.npy", {"fps": 12.5}, (12.5, None)),
                             ("alone.NPY", None, (None, None))):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            np.save(f, fr)
        if meta is not None:
            json.dump(meta, open(path[:-4] + ".json", "w"))
        got, fps, maxval = frames.open_array_clip(path)
        assert isinstance(got, np.memmap) and np.array_equal(got, fr) and (fps, maxval) == want, name


def test_the_callers_keep_their_own_defaults(tmp_path):
    u16, u8 = str(tmp_path / "a.npy"), str(tmp_path / "b.npz")
    np.save(u16, np.zeros((3, 6, 8, 3), np.uint16))
    np.savez(u8, frames=np.zeros((3, 6, 8, 3), np.uint8), fps=np.float64(50.0))
    src = evaluate.ClipSource(u16)
    assert (src.fps, src.depth, src.maxval) == (24.0, 16, 65535) and frames.source_format(src) == frames.FrameFormat(depth=16, maxval=65535)
    io = tools.VideoFI_IO(u16, str(tmp_path / "o.npy"), times=2)
    try:
        assert (io.src_fps, io.depth, io.maxval) == (24.0, 16, 65535) and io.src_format == frames.FrameFormat(depth=16, maxval=65535)
    finally:
        io.close()
    src = evaluate.ClipSource(u8)
    assert (src.fps, src.depth, src.maxval) == (50.0, 8, 255) and frames.source_format(src) == frames.FrameFormat()
    json.dump({"maxval": 70000}, open(u16[:-4] + ".json", "w"))
    with pytest.raises(ValueError, match="255 < maxval <= 65535"):
        evaluate.ClipSource(u16)


def test_frames_loads_without_the_gpu_modules():
    import ast
    top = [n for n in ast.parse(open(frames.__file__).read()).body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name if isinstance(n, ast.Import) else n.module for n in top for a in n.names}
    assert names == {"json", "os", "dataclasses", "numpy"}  # tools, ops and torch are imported where a hook is built
