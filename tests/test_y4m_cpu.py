"""CPU: YUV4MPEG2 streams (drba_amd/y4m.py) -- header round trips and refusals, the streaming reader on a pipe, odd sizes, a
truncated frame, the exact output frame rate --, a whole clip Y4M -> Y4M through interpolate_stream with the CPU oracle and the
restatement's hooks, and properties of the restatement of the YCbCr conversion itself (tests/yuv_common.py)."""
import io
import itertools
import os
import threading

import numpy as np
import pytest

from drba_amd import y4m
from tests import yuv_common as yc


# ------------------------------------------------------------------------------------------------------------------- headers
@pytest.mark.parametrize("chroma,interlace,aspect,rng,extra", list(itertools.product(
    (None, "420", "420jpeg", "420mpeg2", "420p10"), (None, "p", "?"), (None, "1:1", "0:0", "128:117"), (None, "FULL", "LIMITED"),
    ((), ("YSCSS=420JPEG", "FOO=bar")))))
def test_header_round_trips(chroma, interlace, aspect, rng, extra):
    parts = ["YUV4MPEG2", "W71", "H45", "F24000:1001"]
    parts += ["I" + interlace] if interlace else []
    parts += ["A" + aspect] if aspect else []
    parts += ["C" + chroma] if chroma else []
    parts += ["XCOLORRANGE=" + rng] if rng else []
    parts += ["X" + x for x in extra]
    line = (" ".join(parts) + "\n").encode()
    h = y4m.parse_header(line)
    assert (h.width, h.height, h.fps_num, h.fps_den) == (71, 45, 24000, 1001)
    assert (h.chroma, h.interlace, h.aspect, h.color_range, h.extra) == (chroma, interlace, aspect, rng, tuple(extra))
    assert h.depth == (10 if chroma == "420p10" else 8) and h.maxval == (1023 if chroma == "420p10" else 255)
    assert h.frame_bytes == (45 * 71 + 2 * 23 * 36) * (2 if chroma == "420p10" else 1)
    assert h.format() == line and y4m.parse_header(h.format()) == h


def test_header_fields_in_any_order_and_missing_rate():
    h = y4m.parse_header(b"YUV4MPEG2 C420mpeg2 H4 XFOO W6 Ip F30:1\n")
    assert (h.width, h.height, h.chroma, h.extra, h.fps) == (6, 4, "420mpeg2", ("FOO",), 30)
    for line in (b"YUV4MPEG2 W6 H4 F0:0\n", b"YUV4MPEG2 W6 H4\n"):
        with pytest.warns(UserWarning, match="24/1"):
            h = y4m.parse_header(line)
        assert (h.fps_num, h.fps_den) == (24, 1)


@pytest.mark.parametrize("field,needle", [
    ("It", "It"), ("Ib", "Ib"), ("Im", "Im"), ("C420paldv", "C420paldv"), ("C422", "C422"), ("C422p10", "C422p10"), ("C444", "C444"),
    ("C444alpha", "C444alpha"), ("Cmono", "Cmono"), ("Cmono16", "Cmono16"), ("C420p12", "C420p12"), ("C420p16", "C420p16"),
    ("C420p9", "C420p9"), ("C411", "C411"), ("Cfoo", "Cfoo"), ("XCOLORRANGE=WIDE", "XCOLORRANGE=WIDE")])
def test_header_refusals_name_the_tag(field, needle):
    with pytest.raises(y4m.Y4MError) as e:
        y4m.parse_header(f"YUV4MPEG2 W6 H4 F25:1 {field}\n".encode())
    assert needle in str(e.value)


def test_header_refuses_other_streams():
    for line, needle in ((b"RIFF....AVI \n", "YUV4MPEG2"), (b"YUV4MPEG2 H4 F25:1\n", "W or H"), (b"YUV4MPEG2 W0 H4 F25:1\n", "size"),
                         (b"YUV4MPEG2 Wx H4\n", "Wx")):
        with pytest.raises(y4m.Y4MError, match=needle):
            y4m.parse_header(line)
    with pytest.raises(y4m.Y4MError, match="empty"):
        y4m.Reader(io.BytesIO(b""))
    with pytest.raises(y4m.Y4MError, match="header"):
        y4m.Reader(io.BytesIO(b"YUV4MPEG2 W6 H4"))


# -------------------------------------------------------------------------------------------------------------------- frames
def test_odd_sizes_and_frame_header_parameters():
    assert y4m.plane_sizes(45, 71) == ((45, 71), (23, 36))
    frames = [yc.random_frame(45, 71, 8, seed=s) for s in range(3)]
    hdr = y4m.Header(71, 45, (25, 1), chroma="420mpeg2")
    raw = yc.y4m_bytes(frames, hdr)
    assert len(raw) == len(hdr.format()) + 3 * (6 + 45 * 71 + 2 * 23 * 36)
    raw = raw.replace(b"FRAME\n", b"FRAME Ip XANY=thing\n", 2)  # frame headers may carry parameters: read up to the newline
    r = y4m.Reader(io.BytesIO(raw))
    assert r.header == hdr and r.frame_count_estimate() in (3, 4)
    got = list(r)
    assert len(got) == 3 and all(np.array_equal(a.data, b.data) for a, b in zip(got, frames))
    y, u, v = got[0].planes()
    assert got[0].shape == (45, 71, 3) and y.shape == (45, 71) and u.shape == v.shape == (23, 36)
    assert r.read_frame() is None


@pytest.mark.parametrize("bits", [8, 10])
def test_truncated_last_frame_raises(bits):
    frames = [yc.random_frame(8, 12, bits, seed=s) for s in range(2)]
    raw = yc.y4m_bytes(frames, y4m.Header(12, 8, (25, 1), chroma="420p10" if bits == 10 else "420jpeg"))
    r = y4m.Reader(io.BytesIO(raw[:-5]))
    first = r.read_frame()
    assert np.array_equal(first.data, frames[0].data) and first.depth == bits and first.data.dtype == (np.uint8 if bits == 8 else np.uint16)
    with pytest.raises(y4m.Y4MError, match="truncated"):
        r.read_frame()
    with pytest.raises(y4m.Y4MError, match="FRAME"):
        list(y4m.Reader(io.BytesIO(raw.replace(b"FRAME\n", b"FRAMF\n"))))


def test_writer_checks_the_frame_it_is_given():
    w = y4m.Writer(io.BytesIO(), y4m.Header(12, 8, (25, 1), chroma="420p10"))
    with pytest.raises(TypeError):
        w.write_frame(yc.random_frame(8, 12, 8, 0))
    with pytest.raises(ValueError):
        w.write_frame(yc.random_frame(8, 14, 10, 0))
    w.write_frame(yc.random_frame(8, 12, 10, 0).data)
    assert w.frames_written == 1


def test_streaming_from_a_pipe_reads_no_further_than_asked():
    """A non-seekable source fed by a thread: the reader delivers each frame as soon as it is complete, and VideoFI_IO's reader
    thread stays behind its bounded queue: with 3 slots it is never more than 3 queued + 1 in hand ahead of the consumer."""
    from drba_amd.models.utils import tools
    n, bits = 12, 8
    frames = [yc.random_frame(16, 24, bits, seed=s) for s in range(n)]
    hdr = y4m.Header(24, 16, (30000, 1001), chroma="420mpeg2", color_range="FULL")
    raw = yc.y4m_bytes(frames, hdr)
    rfd, wfd = os.pipe()
    fed = []

    def feed():
        with os.fdopen(wfd, "wb", buffering=0) as w:
            w.write(raw[:len(hdr.format())])
            per = 6 + hdr.frame_bytes
            for k in range(n):
                a = len(hdr.format()) + k * per
                w.write(raw[a:a + 7])       # short writes: the reader must assemble a frame from several reads
                w.write(raw[a + 7:a + per])
                fed.append(k)

    t = threading.Thread(target=feed, daemon=True)
    t.start()
    with os.fdopen(rfd, "rb") as f:
        assert not f.seekable()
        r = y4m.Reader(f)
        assert r.header == hdr and r.frame_count_estimate() == 0
        got = list(r)
    t.join(10)
    assert len(got) == n and all(np.array_equal(a.data, b.data) for a, b in zip(got, frames))

    # the bounded queue: a reader over an in-memory stream that counts the frames taken from it
    class Counting(io.BytesIO):
        def seekable(self):
            return False

    src = Counting(raw)
    io_ = tools.VideoFI_IO.__new__(tools.VideoFI_IO)
    from queue import Queue
    io_._y4m_in, io_._cv2, io_.read_buffer = y4m.Reader(src), None, Queue(maxsize=3)
    th = threading.Thread(target=io_._reader, daemon=True)
    th.start()
    out = []
    while True:
        fr = io_.read_frame()  # (blocks until the reader thread has delivered: no waiting on a clock)
        if fr is None:
            break
        out.append(fr)
        # whatever the interleaving, the reader is never further ahead than the queue's slots plus the frame in its hand
        assert io_._y4m_in.frames_read <= len(out) + 3 + 1, (io_._y4m_in.frames_read, len(out))
    th.join(10)
    assert len(out) == n and all(np.array_equal(a.data, b.data) for a, b in zip(out, frames))


def test_output_frame_rate_is_exact():
    assert y4m.output_fps((24000, 1001), 60, times=2) == (48000, 1001)
    assert y4m.output_fps((24000, 1001), 60, times=3) == (72000, 1001)
    assert y4m.output_fps((50, 2), 0, times=2) == (100, 2)          # (num * N) : den of the pair as written
    assert y4m.output_fps((24000, 1001), 60) == (60, 1)
    from fractions import Fraction
    assert y4m.output_fps((24000, 1001), 59.94) == (Fraction(59.94).limit_denominator(1001).numerator, Fraction(59.94).limit_denominator(1001).denominator)
    assert y4m.output_fps((24000, 1001), 60000 / 1001) == (60000, 1001)
    assert y4m.output_fps(24.0, 0, times=2) == (48, 1) and y4m.output_fps(23.976023976023978, 0, times=2) == (48000, 1001)


# ------------------------------------------------------------------------------------------------- the restatement's properties
@pytest.mark.parametrize("bits,full,matrix", list(itertools.product((8, 10), (False, True), ("bt709", "bt601"))))
def test_restatement_round_trip_properties(bits, full, matrix):
    size = (45, 71)
    # luma returns bit for bit for an in-gamut frame without resize
    f = yc.in_gamut_frame(*size, bits, seed=bits)
    bgr = yc.to_bgr_unclamped(f, bits, matrix, full)
    assert float(bgr.min()) > 0.0 and float(bgr.max()) < 1.0
    back = yc.split(yc.to_out_ref(yc.to_inp_ref(f, size, bits, matrix, full), size, bits, matrix, full), size)
    assert np.array_equal(back[0], f.planes()[0])
    # ... its chroma is the source's filtered by (1/8, 3/4, 1/8) per axis (edge samples repeated)
    for got, src in zip(back[1:], f.planes()[1:]):
        p = np.pad(src.astype(np.float64), 1, mode="edge")
        hz = p[:, :-2] / 8 + p[:, 1:-1] * 0.75 + p[:, 2:] / 8
        want = hz[:-2] / 8 + hz[1:-1] * 0.75 + hz[2:] / 8
        if size[1] % 2:  # an odd width: the last chroma column's block repeats its one luma column, whose taps are (1/4, 3/4)
            want, got = want[:, :-1], got[:, :-1]
        if size[0] % 2:
            want, got = want[:-1], got[:-1]
        assert np.abs(got.astype(np.float64) - want).max() <= 0.5 + 1e-9
    # a frame with flat chroma returns its chroma bit for bit
    f = yc.in_gamut_frame(*size, bits, seed=3, flat_chroma=True)
    back = yc.split(yc.to_out_ref(yc.to_inp_ref(f, size, bits, matrix, full), size, bits, matrix, full), size)
    assert all(np.array_equal(a, b) for a, b in zip(back, f.planes()))
    # every legal luma value with neutral chroma returns itself
    f = yc.legal_luma_frame(33, 34, bits, full)
    back = yc.split(yc.to_out_ref(yc.to_inp_ref(f, (33, 34), bits, matrix, full), (33, 34), bits, matrix, full), (33, 34))
    assert all(np.array_equal(a, b) for a, b in zip(back, f.planes()))
    vals = np.unique(f.planes()[0])
    assert vals.size == ((1 << bits) if full else 219 * (1 << (bits - 8)) + 1)


def test_restatement_planted_values_and_window_share():
    """The seed of the way-out frame of tests/test_gpu_yuv.py against the restatement alone: the share of samples whose unrounded
    value lies in the tie window stays under the bar, and the rule holds inside the planted blocks."""
    for bits, full, matrix in itertools.product((8, 10), (False, True), ("bt709", "bt601")):
        x = yc.planted_net_frame((64, 128), seed=7)
        unr = np.concatenate([p.reshape(-1) for p in yc.to_out_unrounded(x, (45, 71), bits, matrix, full)])
        share = float((np.abs(unr - np.floor(unr) - 0.5) <= yc.TIE_WINDOW_STEPS).mean())
        assert share <= yc.TIE_SHARE_MAX, (bits, full, matrix, share)
        yp, up, vp = yc.split(yc.to_out_ref(x, (45, 71), bits, matrix, full), (45, 71))
        want = yc.planted_codes(bits, full)
        assert (int(yp[17, 26]), int(up[8, 13]), int(vp[8, 13])) == want["black"], (bits, full, matrix)
        assert (int(yp[31, 26]), int(up[15, 13]), int(vp[15, 13])) == want["white"], (bits, full, matrix)


# ---------------------------------------------------------------------------------------------------------------- whole clip
@pytest.mark.parametrize("bits", [8, 10])
def test_whole_clip_y4m_to_y4m_on_the_cpu(bits, tmp_path):
    """A 5-frame clip, Y4M source to Y4M sink through VideoFI_IO and interpolate_stream with the CPU oracle and the restatement's
    hooks, -t 2: frame count, header, bytes per frame; the head and tail copies equal the restatement's to_out(to_inp(frame))."""
    import oracle
    from drba_amd import infer as drv
    from drba_amd.models.utils import tools
    from drba_amd.utils import synth
    size = (64, 96)
    src_frames = yc.clip_from_bgr(synth.make_clip(5, *size, seed=11), bits)
    tag = "420p10" if bits == 10 else "420mpeg2"
    hdr = y4m.Header(size[1], size[0], (24000, 1001), interlace="p", aspect="1:1", chroma=tag, extra=("FOO=1",))
    inp, out = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    with open(inp, "wb") as f:
        f.write(yc.y4m_bytes(src_frames, hdr))
    io_ = tools.VideoFI_IO(inp, out, times=2)
    assert (io_.pixfmt, io_.out_pixfmt, io_.width, io_.height) == ("yuv420", "yuv420", 96, 64)
    assert (io_.depth, io_.maxval, io_.out_depth, io_.out_maxval) == ((16, 1023, 16, 1023) if bits == 10 else (8, 255, 8, 255))
    assert io_.total_frames_count == 5.0 and io_.src_fps == pytest.approx(24000 / 1001) and not io_.wants_rgb
    assert io_.yuv_full_range is False and io_.out_full_range is False
    to_inp, to_out, check = yc.cpu_hooks(bits, bits)
    n = drv.interpolate_stream(oracle.rife.RifeOracle(synth.ifnet_state_dict(seed=0), 1.0), io_, io_.dst_fps, times=2,
                               to_inp=to_inp, to_out=to_out, check_scene=check)
    io_.close()
    raw = open(out, "rb").read()
    r = y4m.Reader(io.BytesIO(raw))
    got = list(r)
    assert n == 10 and len(got) == 10
    assert r.header.format() == hdr.format().replace(b"F24000:1001", b"F48000:1001")
    assert len(raw) == len(r.header.format()) + 10 * (6 + hdr.frame_bytes)
    net = tools.get_valid_net_inp_size(src_frames[0], 1.0, div=64)["dst_size"]
    assert net == (64, 128)  # the width is resized on the way in and back on the way out
    for k, src in ((0, src_frames[0]), (-1, src_frames[-1])):
        assert np.array_equal(got[k].data, to_out(to_inp(src, net), size))


def test_sink_header_follows_the_flags(tmp_path):
    from drba_amd.models.utils import tools
    f8 = yc.random_frame(16, 24, 8, 0)
    inp = str(tmp_path / "in.y4m")
    with open(inp, "wb") as f:
        f.write(yc.y4m_bytes([f8], y4m.Header(24, 16, (25, 1), chroma="420mpeg2", color_range="FULL")))

    def header_of(**kw):
        out = str(tmp_path / "o.y4m")
        io_ = tools.VideoFI_IO(kw.pop("inp", inp), out, **kw)
        io_.close()
        return io_, y4m.Reader(open(out, "rb")).header

    io_, h = header_of(times=2)
    assert (h.chroma, h.color_range, h.fps_num, h.fps_den) == ("420mpeg2", "FULL", 50, 1) and io_.yuv_full_range and io_.out_full_range
    io_, h = header_of(times=2, yuv_range="limited")
    assert h.color_range == "LIMITED" and io_.yuv_full_range and not io_.out_full_range  # the source is read by its own tag
    io_, h = header_of(dst_fps=59.94, out_depth=16)
    assert (h.chroma, h.depth, io_.out_maxval) == ("420p10", 10, 1023) and (h.fps_num, h.fps_den) == y4m.output_fps(25, 59.94)
    npz = str(tmp_path / "in.npz")
    np.savez(npz, frames=np.zeros((2, 16, 24, 3), np.uint8), fps=np.float64(24000 / 1001))
    io_, h = header_of(inp=npz, times=2)
    assert (h.chroma, h.color_range, h.interlace, h.fps_num, h.fps_den) == ("420jpeg", None, "p", 48000, 1001) and io_.pixfmt == "bgr"
    io_, h = header_of(inp=npz, times=2, yuv_range="full", out_depth=16)
    assert (h.chroma, h.color_range) == ("420p10", "FULL") and io_.out_full_range
    with pytest.raises(ValueError):
        tools.VideoFI_IO(npz, str(tmp_path / "o.y4m"), yuv_matrix="bt2020")
