"""YUV4MPEG2 (.y4m) streams: header parse and format, a streaming reader, a random-access reader and a writer.  Pure Python, no GPU.

The format is one text line, `YUV4MPEG2 W.. H.. F.. I.. A.. C.. X..`, then per frame the line `FRAME[ params]` and the three
planes Y, U, V.  Progressive planar 4:2:0 at 8 or 10 bits is taken (C420, C420jpeg, C420mpeg2, C420p10): Y is H x W, U and V
are ceil(H/2) x ceil(W/2), 10-bit samples are little-endian uint16 -- and, by a caller that says it can convert them (`accept=`:
the parser is strict by default), planar 4:2:2 (C422, C422p10: U and V are H x ceil(W/2)) and 4:4:4 (C444, C444p10: H x W).  A frame travels through the pipeline as a YuvFrame: the packed
plane bytes as they stand in the stream plus the geometry; the colour conversion happens on the device (ops.to_inp_yuv /
ops.to_out_yuv), never here.  The reader reads any file object, pipes included, one frame at a time; IndexedReader gives len() and
read_frame(k) on a seekable one.
"""
import warnings
from fractions import Fraction

import numpy as np

MAGIC = b"YUV4MPEG2"
CHROMA_8 = ("420", "420jpeg", "420mpeg2")  # all read with the one centre-sited filter pair; the tag is carried through
CHROMA_10 = ("420p10",)
ACCEPT_420 = CHROMA_8 + CHROMA_10  # what parse_header, Reader and IndexedReader take unless told otherwise
CHROMA_WIDE = {"422": ("422", 8), "422p10": ("422", 10), "444": ("444", 8), "444p10": ("444", 10)}  # tag -> (layout, bits)
ACCEPT_ALL = ACCEPT_420 + tuple(CHROMA_WIDE)  # ... and what a caller that converts every layout passes as `accept`
LAYOUTS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}  # layout -> (horizontal, vertical) subsampling factor of U and V
MAX_LINE = 4096


class Y4MError(ValueError):
    pass


def plane_sizes(height, width, layout="420"):
    """-> ((H, W), (Hc, Wc)): odd sizes are legal, chroma rounds up along the axes the layout subsamples"""
    if layout not in LAYOUTS:
        raise Y4MError(f"unknown chroma layout {layout!r}: one of {sorted(LAYOUTS)}")
    sx, sy = LAYOUTS[layout]
    return (int(height), int(width)), ((int(height) + sy - 1) // sy, (int(width) + sx - 1) // sx)


def layout_of(tag):
    """the chroma layout of a C tag (without the C; None: no tag, 4:2:0) -> "420" | "422" | "444" (a key of LAYOUTS)"""
    return CHROMA_WIDE[tag][0] if tag in CHROMA_WIDE else "420"


def chroma_tag(layout, depth, like=None):
    """the C tag a sink of `layout` writes at 8 bits or at 10 (depth > 8); `like`: a source's tag, kept where it names the same layout
    and depth class (C420mpeg2 stays C420mpeg2)"""
    if layout not in LAYOUTS:
        raise Y4MError(f"unknown chroma layout {layout!r}: one of {sorted(LAYOUTS)}")
    if depth > 8:
        return layout + "p10"
    if like is not None and like in CHROMA_8 + tuple(t for t, (_, b) in CHROMA_WIDE.items() if b == 8) and layout_of(like) == layout:
        return like
    return "420jpeg" if layout == "420" else layout


class Header:
    """The stream header.  `chroma` is the C tag without the C (`420mpeg2`), None when the stream had none (then `420jpeg` is meant
    and no tag is written back); `color_range` is "FULL" / "LIMITED" / None (XCOLORRANGE); `extra` the other X tags, verbatim."""

    def __init__(self, width, height, fps=(24, 1), interlace="p", aspect=None, chroma="420jpeg", color_range=None, extra=()):
        self.width, self.height = int(width), int(height)
        self.fps_num, self.fps_den = int(fps[0]), int(fps[1])
        self.interlace, self.aspect, self.chroma, self.color_range, self.extra = interlace, aspect, chroma, color_range, tuple(extra)
        if self.width <= 0 or self.height <= 0:
            raise Y4MError(f"y4m: bad frame size {self.width}x{self.height}")
        if self.fps_num <= 0 or self.fps_den <= 0:
            raise Y4MError(f"y4m: bad frame rate F{self.fps_num}:{self.fps_den}")
        _check_chroma(self.chroma, ACCEPT_ALL)  # a header is built for a sink too: every tag the writer can carry

    @property
    def depth(self):
        """bits per sample: 8 or 10"""
        return 10 if self.chroma in CHROMA_10 or CHROMA_WIDE.get(self.chroma, ("", 8))[1] == 10 else 8

    @property
    def layout(self):
        """the chroma layout, "420" | "422" | "444", from the C tag"""
        return layout_of(self.chroma)

    @property
    def maxval(self):
        return (1 << self.depth) - 1

    @property
    def fps(self):
        return Fraction(self.fps_num, self.fps_den)

    @property
    def frame_bytes(self):
        (h, w), (hc, wc) = plane_sizes(self.height, self.width, self.layout)
        return (h * w + 2 * hc * wc) * (2 if self.depth > 8 else 1)

    def format(self):
        parts = [MAGIC.decode(), f"W{self.width}", f"H{self.height}", f"F{self.fps_num}:{self.fps_den}"]
        if self.interlace is not None:
            parts.append("I" + self.interlace)
        if self.aspect is not None:
            parts.append("A" + self.aspect)
        if self.chroma is not None:
            parts.append("C" + self.chroma)
        if self.color_range is not None:
            parts.append("XCOLORRANGE=" + self.color_range)
        parts += ["X" + x for x in self.extra]
        return (" ".join(parts) + "\n").encode("ascii")

    def __eq__(self, other):
        return isinstance(other, Header) and self.format() == other.format()

    def __repr__(self):
        return f"Header({self.format()[:-1].decode()!r})"


def _check_chroma(tag, accept=ACCEPT_420):
    if tag is None or tag in accept:
        return
    if tag == "420paldv":
        raise Y4MError("y4m: C420paldv is not supported (its chroma samples are co-sited with alternate luma lines)")
    if tag.startswith("420"):
        raise Y4MError(f"y4m: C{tag} is not supported: 4:2:0 is read at 8 bits (C420, C420jpeg, C420mpeg2) or 10 (C420p10)")
    if tag in CHROMA_WIDE:  # a stream this reader's caller did not ask for (parse_header's `accept`)
        raise Y4MError(f"y4m: C{tag} is not supported here: only planar 4:2:0 is read (C420, C420jpeg, C420mpeg2, C420p10)")
    if tag.startswith(("422", "444", "411", "mono")):
        raise Y4MError(f"y4m: C{tag} is not supported: planar 4:2:0, 4:2:2 and 4:4:4 are read at 8 or 10 bits, without alpha")
    raise Y4MError(f"y4m: unknown colour space tag C{tag}")


def parse_header(line, accept=ACCEPT_420):
    """The first line of a stream (bytes, with or without its newline) -> Header.  `accept`: the C tags (without the C) the caller can
    convert -- 4:2:0 only unless it says more (ACCEPT_ALL: 4:2:2 and 4:4:4 too); any other tag is refused by name."""
    accept = tuple(accept)
    for t in accept:
        if t not in ACCEPT_ALL:
            raise ValueError(f"y4m: accept names C{t}, which no reader here can carry (one of {ACCEPT_ALL})")
    if isinstance(line, str):
        line = line.encode("ascii")
    fields = line.rstrip(b"\n").decode("ascii", "replace").split(" ")
    if fields[0] != MAGIC.decode():
        raise Y4MError(f"y4m: the stream does not start with {MAGIC.decode()} (got {fields[0][:16]!r})")
    width = height = None
    fps, interlace, aspect, chroma, color_range, extra = None, None, None, None, None, []
    for f in fields[1:]:
        if not f:
            continue
        key, val = f[0], f[1:]
        if key == "W":
            width = _int(val, f)
        elif key == "H":
            height = _int(val, f)
        elif key == "F":
            num, _, den = val.partition(":")
            fps = (_int(num, f), _int(den or "1", f))
        elif key == "I":
            if val in ("t", "b", "m"):
                raise Y4MError(f"y4m: I{val}: interlaced streams are not supported, only progressive ones (Ip)")
            if val not in ("p", "?"):
                raise Y4MError(f"y4m: unknown interlacing tag I{val}")
            interlace = val
        elif key == "A":
            aspect = val
        elif key == "C":
            _check_chroma(val, accept)
            chroma = val
        elif key == "X":
            if val.startswith("COLORRANGE="):
                color_range = val[len("COLORRANGE="):].upper()
                if color_range not in ("FULL", "LIMITED"):
                    raise Y4MError(f"y4m: unknown colour range {f}")
            else:
                extra.append(val)
        else:
            raise Y4MError(f"y4m: unknown header field {f!r}")
    if width is None or height is None:
        raise Y4MError("y4m: the header lacks W or H")
    if fps is None or fps[0] == 0 or fps[1] == 0:
        warnings.warn("y4m: the stream gives no frame rate (F0:0 or none): 24/1 is assumed")
        fps = (24, 1)
    return Header(width, height, fps, interlace, aspect, chroma, color_range, extra)


def _int(s, field):
    try:
        return int(s)
    except ValueError:
        raise Y4MError(f"y4m: bad header field {field!r}") from None


class YuvFrame:
    """One planar frame: `data` holds Y, then U, then V as they stand in the stream (a 1-D uint8 array for 8-bit samples, a
    1-D uint16 array for 10-bit ones); `layout` ("420" | "422" | "444") says how large U and V are (plane_sizes).  `.shape` is
    (H, W, 3) -- the size a frame-shaped consumer asks for -- although no such array exists."""

    def __init__(self, data, height, width, depth=8, layout="420"):
        if depth not in (8, 10):
            raise Y4MError(f"a YuvFrame holds 8- or 10-bit samples, got {depth}")
        if layout not in LAYOUTS:
            raise Y4MError(f"a YuvFrame is 4:2:0, 4:2:2 or 4:4:4 (layout one of {sorted(LAYOUTS)}), got {layout!r}")
        dtype = np.uint8 if depth == 8 else np.dtype("<u2")
        if not isinstance(data, np.ndarray):
            data = np.frombuffer(data, dtype=dtype)
        self.height, self.width, self.depth, self.layout = int(height), int(width), int(depth), layout
        (h, w), (hc, wc) = plane_sizes(height, width, layout)
        if data.dtype != dtype or data.ndim != 1 or data.size != h * w + 2 * hc * wc:
            raise Y4MError(f"a {w}x{h} {depth}-bit 4:{layout[1]}:{layout[2]} frame is {h * w + 2 * hc * wc} {np.dtype(dtype).name} samples, "
                           f"got {data.dtype} x {data.shape}")
        self.data = data

    @property
    def shape(self):
        return (self.height, self.width, 3)

    @property
    def maxval(self):
        return (1 << self.depth) - 1

    def planes(self):
        """-> (y [H,W], u [Hc,Wc], v [Hc,Wc]) views"""
        (h, w), (hc, wc) = plane_sizes(self.height, self.width, self.layout)
        d = self.data
        return d[:h * w].reshape(h, w), d[h * w:h * w + hc * wc].reshape(hc, wc), d[h * w + hc * wc:].reshape(hc, wc)

    @classmethod
    def from_planes(cls, y, u, v, depth=8, layout="420"):
        dtype = np.uint8 if depth == 8 else np.dtype("<u2")
        return cls(np.concatenate([np.asarray(p, dtype=dtype).reshape(-1) for p in (y, u, v)]), y.shape[0], y.shape[1], depth, layout)


def _read_exact(f, n):
    """n bytes of a file object that may return short reads (a pipe); fewer only at the end of the stream"""
    buf = bytearray(n)
    view, got = memoryview(buf), 0
    readinto = getattr(f, "readinto", None)
    while got < n:
        if readinto is not None:
            k = readinto(view[got:])
        else:
            chunk = f.read(n - got)
            k = len(chunk)
            view[got:got + k] = chunk
        if not k:
            break
        got += k
    return buf if got == n else bytes(buf[:got])


def _read_line(f):
    """up to and including the newline, never past it (the stream need not be seekable or buffered)"""
    readline = getattr(f, "readline", None)
    if readline is not None:
        return readline(MAX_LINE)
    out = bytearray()
    while len(out) < MAX_LINE:
        c = f.read(1)
        if not c:
            break
        out += c
        if c == b"\n":
            break
    return bytes(out)


class Reader:
    """Frames of a stream, one read_frame() at a time; nothing is read ahead of the frame asked for."""

    def __init__(self, fileobj, accept=ACCEPT_420):
        self.f = fileobj
        line = _read_line(fileobj)
        if not line.endswith(b"\n"):
            raise Y4MError("y4m: the stream ends inside its header" if line else "y4m: the stream is empty")
        self.header_bytes = len(line)
        self.header = parse_header(line, accept)
        self.frames_read = 0

    def read_frame(self):
        """-> YuvFrame, or None at the end of the stream; a truncated frame raises"""
        line = _read_line(self.f)
        if not line:
            return None
        if not (line.endswith(b"\n") and (line[:-1] == b"FRAME" or line.startswith(b"FRAME "))):  # a frame header may carry parameters
            raise Y4MError(f"y4m: frame {self.frames_read}: expected a FRAME line, got {bytes(line[:24])!r}")
        h = self.header
        data = _read_exact(self.f, h.frame_bytes)
        if len(data) != h.frame_bytes:
            raise Y4MError(f"y4m: frame {self.frames_read} is truncated: {len(data)} of {h.frame_bytes} bytes")
        self.frames_read += 1
        return YuvFrame(data, h.height, h.width, h.depth, h.layout)

    def frame_count_estimate(self):
        """the number of frames from the file size (frame headers without parameters), 0 for a stream that cannot seek"""
        try:
            if not self.f.seekable():
                return 0
            pos = self.f.tell()
            end = self.f.seek(0, 2)
            self.f.seek(pos)
        except (OSError, AttributeError, ValueError):
            return 0
        return max(0, (end - self.header_bytes) // (len(b"FRAME\n") + self.header.frame_bytes))

    def __iter__(self):
        return iter(self.read_frame, None)


class IndexedReader:
    """Random access to the frames of a seekable stream: len() and read_frame(k).  One scan at construction reads each `FRAME...\\n`
    line and seeks over the payload -- a frame header may carry parameters, so the offsets are not assumed uniform -- and keeps one
    integer per frame; no payload is read before its frame is asked for.  A file object that cannot seek raises Y4MError, and so does
    a truncated last frame, as in Reader."""

    def __init__(self, fileobj, accept=ACCEPT_420):
        seekable = getattr(fileobj, "seekable", None)
        if not (callable(seekable) and seekable() and hasattr(fileobj, "seek") and hasattr(fileobj, "tell")):
            raise Y4MError("y4m: random access needs a seekable stream (a file, not a pipe)")
        self.f = fileobj
        start = fileobj.tell()
        head = Reader(fileobj, accept)
        self.header, self.header_bytes = head.header, head.header_bytes
        end = fileobj.seek(0, 2)
        size, pos, self._offsets = self.header.frame_bytes, start + head.header_bytes, []
        while pos < end:
            fileobj.seek(pos)
            line = _read_line(fileobj)
            k = len(self._offsets)
            if not (line.endswith(b"\n") and (line[:-1] == b"FRAME" or line.startswith(b"FRAME "))):
                raise Y4MError(f"y4m: frame {k}: expected a FRAME line, got {bytes(line[:24])!r}")
            pos += len(line)
            if pos + size > end:
                raise Y4MError(f"y4m: frame {k} is truncated: {end - pos} of {size} bytes")
            self._offsets.append(pos)
            pos += size

    def __len__(self):
        return len(self._offsets)

    def read_frame(self, k):
        """-> frame k as a YuvFrame (IndexError outside 0 .. len() - 1)"""
        if not 0 <= int(k) < len(self._offsets):
            raise IndexError(f"y4m: frame {k} of {len(self._offsets)}")
        h = self.header
        self.f.seek(self._offsets[int(k)])
        data = _read_exact(self.f, h.frame_bytes)
        if len(data) != h.frame_bytes:  # (the file shrank after the scan)
            raise Y4MError(f"y4m: frame {k} is truncated: {len(data)} of {h.frame_bytes} bytes")
        return YuvFrame(data, h.height, h.width, h.depth, h.layout)

    def __iter__(self):
        return (self.read_frame(k) for k in range(len(self._offsets)))


class Writer:
    """The header at once, then each frame as it is handed over."""

    def __init__(self, fileobj, header):
        self.f, self.header, self.frames_written = fileobj, header, 0
        fileobj.write(header.format())

    def write_frame(self, frame):
        data = frame.data if isinstance(frame, YuvFrame) else frame
        if isinstance(data, np.ndarray):
            want = np.uint8 if self.header.depth == 8 else np.uint16
            if data.dtype != want:
                raise TypeError(f"the y4m sink takes {np.dtype(want).name} samples at {self.header.depth} bits, got {data.dtype}")
            data = np.ascontiguousarray(data.astype(data.dtype.newbyteorder("<"), copy=False)).reshape(-1).view(np.uint8)
        if len(data) != self.header.frame_bytes:
            raise ValueError(f"a frame of this stream is {self.header.frame_bytes} bytes, got {len(data)}")
        self.f.write(b"FRAME\n")
        self.f.write(data)
        self.frames_written += 1

    def flush(self):
        self.f.flush()


def output_fps(src_fps, dst_fps, times=-1):
    """The exact F ratio of the output: with an integer factor (num * times) : den of the source's ratio, otherwise
    Fraction(dst_fps).limit_denominator(1001).  `src_fps`: a Fraction, a (num, den) pair or a float."""
    if times != -1:
        if isinstance(src_fps, tuple):  # the header's own pair, not reduced
            return int(src_fps[0]) * int(times), int(src_fps[1])
        if not isinstance(src_fps, Fraction):
            src_fps = Fraction(src_fps).limit_denominator(1001)
        return src_fps.numerator * int(times), src_fps.denominator
    r = Fraction(dst_fps).limit_denominator(1001)
    return r.numerator, r.denominator
