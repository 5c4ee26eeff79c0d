"""CPU: planar 4:2:2 and 4:4:4 -- the C422 / C422p10 / C444 / C444p10 tags through drba_amd/y4m.py (strict by default, `accept=` for a
caller that converts them), plane sizes at odd sizes, the fp64 restatement of tests/yuv_layouts_common.py, the keyword sets of
frames.hooks, --out-chroma, evaluate compare's refusal of mixed layouts, the argument checks of the layout entries and a whole clip
through the driver on CPU hooks."""
import ctypes as C
import io
import itertools

import numpy as np
import pytest

from drba_amd import _lib, evaluate, frames, y4m
from tests import metrics_yuv_common as myc
from tests import yuv_common as yc
from tests import yuv_layouts_common as yl

TAGS = [("422", "422", 8), ("422p10", "422", 10), ("444", "444", 8), ("444p10", "444", 10)]


# ------------------------------------------------------------------------------------------------------------------- headers
@pytest.mark.parametrize("tag,layout,bits", TAGS)
def test_header_parse_format_and_round_trip_with_accept(tag, layout, bits):
    line = f"YUV4MPEG2 W71 H45 F24000:1001 Ip A1:1 C{tag} XCOLORRANGE=FULL XKEEP=me\n".encode()
    h = y4m.parse_header(line, accept=y4m.ACCEPT_ALL)
    assert (h.width, h.height, h.chroma, h.layout, h.depth, h.maxval) == (71, 45, tag, layout, bits, (1 << bits) - 1)
    wc = 36 if layout == "422" else 71
    assert h.frame_bytes == (45 * 71 + 2 * 45 * wc) * (2 if bits == 10 else 1)
    assert h.format() == line and y4m.parse_header(h.format(), accept=y4m.ACCEPT_ALL) == h
    assert y4m.parse_header(line, accept=(tag,)).chroma == tag  # a caller may name less than everything
    # the bare parser is strict, and so is a caller that accepts another tag only; both name the tag
    for kw in ({}, {"accept": y4m.ACCEPT_420}, {"accept": tuple(t for t, _, _ in TAGS if t != tag)}):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.parse_header(line, **kw)
        assert "C" + tag in str(e.value)
    for reader in (y4m.Reader, y4m.IndexedReader):
        with pytest.raises(y4m.Y4MError, match="C" + tag):
            reader(io.BytesIO(line))


def test_420_is_what_it_was_and_the_rest_stays_refused():
    h = y4m.parse_header(b"YUV4MPEG2 W71 H45 F25:1 C420mpeg2\n", accept=y4m.ACCEPT_ALL)
    assert (h.layout, h.depth, h.frame_bytes) == ("420", 8, 45 * 71 + 2 * 23 * 36)
    assert y4m.parse_header(b"YUV4MPEG2 W6 H4 F25:1\n").layout == "420"
    for tag in ("444alpha", "mono", "mono16", "411", "420paldv", "420p12", "420p16", "422p12", "444p12", "444p16", "422p16"):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.parse_header(f"YUV4MPEG2 W6 H4 F25:1 C{tag}\n".encode(), accept=y4m.ACCEPT_ALL)
        assert "C" + tag in str(e.value)
    with pytest.raises(y4m.Y4MError, match="It"):
        y4m.parse_header(b"YUV4MPEG2 W6 H4 F25:1 It C444\n", accept=y4m.ACCEPT_ALL)
    with pytest.raises(ValueError, match="C444alpha"):
        y4m.parse_header(b"YUV4MPEG2 W6 H4 F25:1\n", accept=("444alpha",))  # nobody can promise to convert it
    assert y4m.chroma_tag("444", 8) == "444" and y4m.chroma_tag("444", 10) == "444p10" and y4m.chroma_tag("422", 10, like="422") == "422p10"
    assert y4m.chroma_tag("420", 8, like="420mpeg2") == "420mpeg2" and y4m.chroma_tag("420", 8, like="444") == "420jpeg"
    assert y4m.chroma_tag("420", 10, like="420mpeg2") == "420p10" and y4m.chroma_tag("420", 8) == "420jpeg"


# -------------------------------------------------------------------------------------------------------------------- frames
def test_plane_sizes_and_frames_at_odd_sizes():
    assert y4m.plane_sizes(45, 71) == y4m.plane_sizes(45, 71, "420") == ((45, 71), (23, 36))
    assert y4m.plane_sizes(45, 71, "422") == ((45, 71), (45, 36)) and y4m.plane_sizes(45, 71, "444") == ((45, 71), (45, 71))
    with pytest.raises(y4m.Y4MError):
        y4m.plane_sizes(4, 4, "411")
    for (tag, layout, bits), size in itertools.product(TAGS, ((5, 7), (45, 71), (4, 6))):
        f = yl.random_frame(*size, bits, seed=3, layout=layout)
        (h, w), (hc, wc) = y4m.plane_sizes(*size, layout)
        assert f.layout == layout and f.shape == (h, w, 3) and f.data.size == h * w + 2 * hc * wc
        y, u, v = f.planes()
        assert y.shape == (h, w) and u.shape == v.shape == (hc, wc)
        g = y4m.YuvFrame.from_planes(y, u, v, depth=bits, layout=layout)
        assert g.layout == layout and np.array_equal(g.data, f.data)
        assert np.array_equal(np.concatenate([p.reshape(-1) for p in (y, u, v)]), f.data)
        if layout != "444" or size[0] * size[1] * 3 != h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2):
            with pytest.raises(y4m.Y4MError, match="4:" + layout[1] + ":" + layout[2]):
                y4m.YuvFrame(f.data[:-1], h, w, bits, layout)
    with pytest.raises(y4m.Y4MError):
        y4m.YuvFrame(np.zeros(12, np.uint8), 2, 2, 8, "411")


@pytest.mark.parametrize("tag,layout,bits", TAGS)
def test_reader_indexed_reader_and_writer_round_trip(tag, layout, bits):
    fr = [yl.random_frame(5, 7, bits, seed=s, layout=layout) for s in range(3)]
    hdr = y4m.Header(7, 5, (30000, 1001), interlace="p", chroma=tag)
    raw = yl.y4m_bytes(fr, hdr)
    assert len(raw) == len(hdr.format()) + 3 * (6 + hdr.frame_bytes)
    r = y4m.Reader(io.BytesIO(raw), accept=y4m.ACCEPT_ALL)
    got = list(r)
    assert r.header == hdr and r.frame_count_estimate() == 3 and len(got) == 3
    assert all(g.layout == layout and g.depth == bits and np.array_equal(g.data, f.data) for g, f in zip(got, fr))
    ir = y4m.IndexedReader(io.BytesIO(raw), accept=y4m.ACCEPT_ALL)
    assert len(ir) == 3 and np.array_equal(ir.read_frame(2).data, fr[2].data) and ir.read_frame(0).layout == layout
    with pytest.raises(y4m.Y4MError, match="truncated"):
        list(y4m.Reader(io.BytesIO(raw[:-1]), accept=y4m.ACCEPT_ALL))
    w = y4m.Writer(io.BytesIO(), hdr)
    with pytest.raises(ValueError, match="bytes"):  # a 4:2:0 frame of the same size is not a frame of this stream
        w.write_frame(yc.random_frame(5, 7, bits, 0))


# --------------------------------------------------------------------------------------------------------------- restatement
def test_restatement_sanity():
    """4:2:0 through the layout-aware restatement is yuv_common's; 4:4:4 up then down is the identity; 4:2:2 planes built by repeating
    each 4:2:0 chroma row twice give the 4:2:0 way-in result where the picture is vertically constant."""
    f0 = yc.random_frame(45, 71, 8, 1)
    assert np.array_equal(yl.to_inp_ref(f0, (64, 128), 8, layout="420").numpy(), yc.to_inp_ref(f0, (64, 128), 8).numpy())
    x = yl.planted_net_frame((64, 128), seed=7)
    assert np.array_equal(yl.to_out_ref(x, (45, 71), 10, "bt601", True, "420"), yc.to_out_ref(x, (45, 71), 10, "bt601", True))
    c = np.random.default_rng(0).integers(0, 256, size=(9, 13)).astype(np.float64)
    assert np.array_equal(yl.box(yl.upsample(c, 9, 13, "444"), "444"), c)
    for bits, full, matrix in itertools.product((8, 10), (False, True), ("bt709", "bt601")):
        f = yl.in_gamut_frame(45, 71, bits, seed=bits, layout="444")
        x = yl.to_inp_ref(f, (45, 71), bits, matrix, full, "444")
        assert np.array_equal(yl.to_out_ref(x, (45, 71), bits, matrix, full, "444"), f.data)  # fp64: far below half a step
    m = (1 << 8) - 1
    rng = np.random.default_rng(5)
    y = np.repeat(rng.integers(0, m + 1, size=(1, 71)), 46, axis=0)
    u, v = (np.repeat(rng.integers(0, m + 1, size=(1, 36)), 23, axis=0) for _ in range(2))
    a = yc.to_bgr_unclamped((y, u, v), 8)
    b = yl.to_bgr_unclamped((y, np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0)), 8, layout="422")
    assert np.array_equal(a, b)


def test_restatement_planted_values_and_window_share():
    """The way-out inputs of tests/test_gpu_yuv_layouts.py against the restatement alone: the share of samples inside the tie window
    stays under the cap for exactly those inputs, layouts and conversions, and the rule holds inside the planted blocks."""
    geoms = [((45, 71), (64, 128)), ((60, 64), (64, 64)), ((60, 66), (64, 66))]
    for layout in ("422", "444"):
        cases = [(geoms[0], b, f, m) for b, f, m in itertools.product((8, 10), (False, True), ("bt709", "bt601"))]
        cases += [(g, b, False, "bt709") for g in geoms[1:] for b in (8, 10)]
        for (src, net), bits, full, matrix in cases:
            x = yl.planted_net_frame(net, seed=7)
            share = yl.compare_out(None, x, src, bits, matrix, full, layout)[3]
            assert share <= yl.TIE_SHARE_MAX, (layout, src, bits, full, matrix, share)
            if src == (45, 71):
                yp, up, vp = yl.split(yl.to_out_ref(x, src, bits, matrix, full, layout), src, layout)
                for colour, code in yl.planted_codes(bits, full).items():
                    (ly, lx), (cy, cx) = yl.PLANTED["resized"][layout][colour]
                    assert (int(yp[ly, lx]), int(up[cy, cx]), int(vp[cy, cx])) == code, (layout, bits, full, matrix, colour)
        for (src, net), bits, (full, matrix) in itertools.product(geoms[:2], (8, 10), ((False, "bt709"), (True, "bt709"), (False, "bt601"))):
            x = yl.planted_net_frame(net, seed=7)  # the crop cases
            share = yl.compare_out(None, x, src, bits, matrix, full, layout, crop=True)[3]
            assert share <= yl.TIE_SHARE_MAX, (layout, src, bits, full, matrix, share)
            if src == (45, 71):
                yp, up, vp = yl.split(yl.to_out_crop_ref(x, src, bits, matrix, full, layout), src, layout)
                (ly, lx), (cy, cx) = yl.PLANTED["window"][layout]["black"]
                assert (int(yp[ly, lx]), int(up[cy, cx]), int(vp[cy, cx])) == yl.planted_codes(bits, full)["black"]


# ------------------------------------------------------------------------------------------------------------------ host glue
def test_hooks_keyword_sets_for_the_new_pixfmts(monkeypatch):
    from drba_amd.models.utils import tools
    with pytest.raises(ValueError, match="pixfmt"):
        tools.to_out(None, (2, 2), pixfmt="yuv411")
    for layout in ("422", "444"):
        fmt = frames.FrameFormat("yuv" + layout, 16, 1023, "bt601", True)
        assert frames.inp_keywords(fmt, "resize") == {"matrix": "bt601", "full_range": True}  # the frame carries its layout
        assert frames.inp_keywords(fmt, "pad") == {"matrix": "bt601", "full_range": True, "fit": "pad"}
        five = {"matrix": "bt601", "full_range": True, "depth": 16, "maxval": 1023}
        assert frames.out_keywords(fmt, "resize") == {**five, "pixfmt": "yuv" + layout}
        assert frames.out_keywords(fmt, "pad", on_device=True) == {**five, "layout": layout, "fit": "pad"}
        calls = []
        monkeypatch.setattr(tools, "to_inp", lambda fr, size, **kw: calls.append(("in", kw)))
        monkeypatch.setattr(tools, "to_out", lambda x, size, **kw: calls.append(("out", kw)))
        to_inp, to_out = frames.hooks(fmt, frames.FrameFormat("yuv" + layout), "resize")
        to_inp(None, (2, 2)), to_out(None, (2, 2))
        assert calls == [("in", {"matrix": "bt601", "full_range": True}),
                         ("out", {"matrix": "bt709", "full_range": False, "depth": 8, "maxval": None, "pixfmt": "yuv" + layout})]
    # 4:2:0 says nothing about its layout, on the device either
    assert frames.out_keywords(frames.FrameFormat("yuv420"), "resize", on_device=True) == {"matrix": "bt709", "full_range": False, "depth": 8,
                                                                                          "maxval": None}


def test_out_chroma_parsing_and_refusals(tmp_path):
    from drba_amd import infer as drv
    from drba_amd.models.utils import tools
    assert drv.parse_args(["-i", "a.y4m", "-o", "b.y4m"]).out_chroma == "source"
    for v in ("420", "422", "444"):
        a = drv.parse_args(["-i", "a.y4m", "-o", "b.y4m", "--out-chroma", v])
        assert a.out_chroma == v and drv.out_chroma_of(a) == v
        assert drv.out_chroma_of(drv.parse_args(["-i", "a.y4m", "-o", "-", "--out-chroma", v])) == v
        for sink in ("out.npz", "out.npy", "out.mp4", "out.raw"):
            with pytest.raises(ValueError, match="--out-chroma " + v):
                drv.out_chroma_of(drv.parse_args(["-i", "a.y4m", "-o", sink, "--out-chroma", v]))
    with pytest.raises(SystemExit):
        drv.parse_args(["--out-chroma", "411"])
    import argparse
    assert drv.out_chroma_of(argparse.Namespace(output="x.npz")) == "source"  # a namespace built without the flag
    # main() refuses before a model is built: load_model would raise on the unknown type first if it were reached
    src = str(tmp_path / "in.y4m")
    open(src, "wb").write(yl.y4m_bytes([yl.random_frame(16, 24, 8, 0, "444")], yl.header_for(16, 24, 8, "444")))
    with pytest.raises(ValueError, match="--out-chroma 444"):
        drv.main(["-m", "no-such-model", "-i", src, "-o", str(tmp_path / "out.npz"), "--out-chroma", "444"])
    assert tools.out_layout("source", "o.y4m", None) == "420" and tools.out_layout("source", "o.y4m", "444") == "444"
    assert tools.out_layout("422", "-", "444") == "422" and tools.out_layout("source", "o.npz", "444") is None


def test_sink_header_follows_the_layout_and_depth(tmp_path):
    from drba_amd.models.utils import tools
    paths = {}
    for tag, layout, bits in TAGS + [("420mpeg2", "420", 8)]:
        paths[tag] = str(tmp_path / f"in_{tag}.y4m")
        f = yl.random_frame(16, 24, bits, 0, layout) if layout != "420" else yc.random_frame(16, 24, bits, 0)
        open(paths[tag], "wb").write(yl.y4m_bytes([f], y4m.Header(24, 16, (25, 1), chroma=tag)))

    def header_of(inp, **kw):
        out = str(tmp_path / "o.y4m")
        io_ = tools.VideoFI_IO(inp, out, times=2, **kw)
        io_.close()
        return io_, y4m.Reader(open(out, "rb"), accept=y4m.ACCEPT_ALL).header

    for tag, layout, bits in TAGS:  # source: the source's layout and tag
        io_, h = header_of(paths[tag])
        assert (io_.pixfmt, io_.out_pixfmt, h.chroma) == ("yuv" + layout, "yuv" + layout, tag)
        assert (io_.src_format.pixfmt, io_.sink_format.pixfmt, io_.sink_format.maxval) == ("yuv" + layout, "yuv" + layout, (1 << bits) - 1)
    io_, h = header_of(paths["420mpeg2"])
    assert (io_.out_pixfmt, h.chroma) == ("yuv420", "420mpeg2")
    io_, h = header_of(paths["420mpeg2"], out_chroma="444", out_depth=16)
    assert (io_.pixfmt, io_.out_pixfmt, h.chroma, h.depth, io_.out_maxval) == ("yuv420", "yuv444", "444p10", 10, 1023)
    io_, h = header_of(paths["444p10"], out_chroma="422")
    assert (io_.out_pixfmt, h.chroma) == ("yuv422", "422p10")
    io_, h = header_of(paths["444"], out_chroma="420")
    assert (io_.out_pixfmt, h.chroma) == ("yuv420", "420jpeg")
    io_, h = header_of(paths["444"], out_chroma="444", out_depth=16)
    assert h.chroma == "444p10"
    npz = str(tmp_path / "in.npz")
    np.savez(npz, frames=np.zeros((2, 16, 24, 3), np.uint8), fps=np.float64(24.0))
    assert header_of(npz)[1].chroma == "420jpeg" and header_of(npz, out_chroma="422")[1].chroma == "422"
    with pytest.raises(ValueError, match="out-chroma"):
        tools.VideoFI_IO(paths["444"], str(tmp_path / "o.npz"), times=2, out_chroma="444")
    with pytest.raises(ValueError, match="out_chroma"):
        tools.VideoFI_IO(paths["444"], str(tmp_path / "o.y4m"), times=2, out_chroma="411")


def test_compare_measures_layouts_and_refuses_mixed_ones(tmp_path, capsys):
    import json
    be = myc.NumpyYuvBackend()
    clips = {}
    for tag, layout, bits in TAGS:
        clips[tag] = str(tmp_path / f"{tag}.y4m")
        myc.write_clip(clips[tag], [yl.random_frame(14, 22, bits, 70 + i, layout) for i in range(3)], chroma=tag)
    clips["420"] = str(tmp_path / "420.y4m")
    myc.write_clip(clips["420"], myc.random_clip(3, 14, 22, 8, seed=61))
    for a, b in (("444", "420"), ("420", "422"), ("422", "444"), ("422p10", "444p10")):
        assert evaluate.main(["compare", clips[a], clips[b]], backend=be) == 2
        err = capsys.readouterr().err
        assert "chroma layout" in err and "C" + (a if a != "420" else "420jpeg") in err and "C" + (b if b != "420" else "420jpeg") in err, err
    src = evaluate.ClipSource(clips["422p10"])
    assert (src.pixfmt, src.layout, src.depth, src.maxval, len(src)) == ("yuv422", "422", 16, 1023, 3)
    assert frames.source_format(src, yuv_matrix="bt601").pixfmt == "yuv422"
    # the refusal happens before anything is measured; the stand-in back end measures 4:2:0 only, so the figures are checked on the GPU


def test_layout_entries_validate_their_arguments_without_a_gpu():
    """Every malformed argument is DRBA_EINVAL (-1) before any launch: null planes, a stride below the plane width, a misaligned
    16-bit plane, maxval outside (255, 65535], an unknown matrix, an unknown layout, a pad target below the frame."""
    lib = _lib.load()
    H, W = 16, 24
    buf = (C.c_uint16 * (3 * H * W + 8))()
    base = C.addressof(buf)
    x = (C.c_float * (3 * H * W + 4))()
    xp = C.c_void_p((C.addressof(x) + 15) & ~15)

    def planes(layout, es, off=0):
        wc = W if layout == 444 else W // 2
        hc = H // 2 if layout == 420 else H
        return [C.c_void_p(base + off), C.c_void_p(base + off + H * W * es), C.c_void_p(base + off + (H * W + hc * wc) * es)], wc

    def call(name, layout, pl=None, strides=None, size=(H, W, H, W), matrix=0, maxval=1023.0, tensor=xp):
        deep, out, fit = "16" in name, "to_out" in name, ("pad" in name or "crop" in name)
        p, wc = planes(layout, 2 if deep else 1)
        p = p if pl is None else pl
        strides = (W, wc) if strides is None else strides
        tail = ([] if fit else [1.0, 1.0]) + [matrix, 0, layout] + ([maxval] if deep else []) + [None]
        if out:
            return getattr(lib, name)(tensor, *p, *strides, *size, *tail)
        return getattr(lib, name)(*p, *strides, tensor, None, *size, *tail)

    names = ["drba_to_inp_yuv_x4", "drba_to_inp16_yuv_x4", "drba_to_out_yuv", "drba_to_out16_yuv", "drba_to_inp_yuv_pad_x4",
             "drba_to_inp16_yuv_pad_x4", "drba_to_out_yuv_crop", "drba_to_out16_yuv_crop"]
    assert all(n in _lib.SIGNATURES for n in names)
    for name, layout in itertools.product(names, (420, 422, 444)):
        deep = "16" in name
        for k in range(3):  # a null plane
            pl, _ = planes(layout, 2 if deep else 1)
            pl[k] = None
            assert call(name, layout, pl=pl) == -1, (name, layout, k)
        assert call(name, layout, tensor=None) == -1
        wc = W if layout == 444 else W // 2
        assert call(name, layout, strides=(W - 1, wc)) == -1 and call(name, layout, strides=(W, wc - 1)) == -1
        for k in range(4):
            size = [H, W, H, W]
            size[k] = 0
            assert call(name, layout, size=tuple(size)) == -1
        for matrix in (2, -1):
            assert call(name, layout, matrix=matrix) == -1
        if deep:
            for maxval in (255.0, 70000.0, float("nan")):
                assert call(name, layout, maxval=maxval) == -1
            assert call(name, layout, pl=planes(layout, 2, off=1)[0]) == -1  # a misaligned 16-bit plane
        if "pad" in name:
            assert call(name, layout, size=(H, W, H - 1, W)) == -1 and call(name, layout, size=(H, W, H, W - 1)) == -1
        if "crop" in name:
            assert call(name, layout, size=(H, W, H + 1, W)) == -1 and call(name, layout, size=(H, W, H, W + 1)) == -1
    for name, layout in itertools.product(names, (0, 411, 440, -422, 4440)):  # an unknown layout, every other argument well formed
        p, wc = planes(444, 2 if "16" in name else 1)
        deep, out, fit = "16" in name, "to_out" in name, ("pad" in name or "crop" in name)
        tail = ([] if fit else [1.0, 1.0]) + [0, 0, layout] + ([1023.0] if deep else []) + [None]
        args = [xp, *p, W, wc, H, W, H, W, *tail] if out else [*p, W, wc, xp, None, H, W, H, W, *tail]
        assert getattr(lib, name)(*args) == -1, (name, layout)


# ---------------------------------------------------------------------------------------------------------------- whole clip
def test_whole_clip_444_to_444_on_the_cpu(tmp_path):
    """6 frames of 64 x 96, C444 source to C444 sink through VideoFI_IO and interpolate_stream with the CPU oracle and the
    restatement's hooks, -t 2: frame count, header, bytes per frame; the head and tail copies equal the restatement's
    to_out(to_inp(frame))."""
    import oracle
    from drba_amd import infer as drv
    from drba_amd.models.utils import tools
    from drba_amd.utils import synth
    size = (64, 96)
    src_frames = yl.clip_from_bgr(synth.make_clip(6, *size, seed=11), 8, "444")
    hdr = yl.header_for(*size, 8, "444", fps=(24000, 1001), aspect="1:1", extra=("FOO=1",))
    inp, out = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    open(inp, "wb").write(yl.y4m_bytes(src_frames, hdr))
    io_ = tools.VideoFI_IO(inp, out, times=2)
    assert (io_.pixfmt, io_.out_pixfmt, io_.width, io_.height, io_.total_frames_count) == ("yuv444", "yuv444", 96, 64, 6.0)
    to_inp, to_out, check = yl.cpu_hooks(8, 8, "444", "444")
    n = drv.interpolate_stream(oracle.rife.RifeOracle(synth.ifnet_state_dict(seed=0), 1.0), io_, io_.dst_fps, times=2,
                               to_inp=to_inp, to_out=to_out, check_scene=check)
    io_.close()
    raw = open(out, "rb").read()
    with pytest.raises(y4m.Y4MError, match="C444"):
        y4m.Reader(io.BytesIO(raw))
    r = y4m.Reader(io.BytesIO(raw), accept=y4m.ACCEPT_ALL)
    got = list(r)
    assert n == 12 and len(got) == 12 and all(g.layout == "444" for g in got)
    assert r.header.format() == hdr.format().replace(b"F24000:1001", b"F48000:1001") and hdr.frame_bytes == 3 * 64 * 96
    assert len(raw) == len(r.header.format()) + 12 * (6 + hdr.frame_bytes)
    net = tools.get_valid_net_inp_size(src_frames[0], 1.0, div=64)["dst_size"]
    assert net == (64, 128)  # the width is resized on the way in and back on the way out
    for k, src in ((0, src_frames[0]), (-1, src_frames[-1])):
        assert np.array_equal(got[k].data, to_out(to_inp(src, net), size))
