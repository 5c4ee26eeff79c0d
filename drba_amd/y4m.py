"""YUV4MPEG2 (.y4m) streams: header parse and format, a streaming reader, a random-access reader and a writer.  Pure Python, no GPU.

The format is one text line, `YUV4MPEG2 W.. H.. F.. I.. A.. C.. X..`, then per frame the line `FRAME[ params]` and the three
planes Y, U, V.  Only progressive planar 4:2:0 at 8 or 10 bits is taken (C420, C420jpeg, C420mpeg2, C420p10): Y is H x W, U and V
are ceil(H/2) x ceil(W/2), 10-bit samples are little-endian uint16.  A frame travels through the pipeline as a YuvFrame: the packed
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
MAX_LINE = 4096


class Y4MError(ValueError):
    pass


def plane_sizes(height, width):
    """-> ((H, W), (Hc, Wc)): odd sizes are legal, chroma rounds up"""
    return (int(height), int(width)), ((int(height) + 1) // 2, (int(width) + 1) // 2)


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
        _check_chroma(self.chroma)

    @property
    def depth(self):
        """bits per sample: 8 or 10"""
        return 10 if self.chroma in CHROMA_10 else 8

    @property
    def maxval(self):
        return (1 << self.depth) - 1

    @property
    def fps(self):
        return Fraction(self.fps_num, self.fps_den)

    @property
    def frame_bytes(self):
        (h, w), (hc, wc) = plane_sizes(self.height, self.width)
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


def _check_chroma(tag):
    if tag is None or tag in CHROMA_8 or tag in CHROMA_10:
        return
    if tag == "420paldv":
        raise Y4MError("y4m: C420paldv is not supported (its chroma samples are co-sited with alternate luma lines)")
    if tag.startswith("420"):
        raise Y4MError(f"y4m: C{tag} is not supported: 4:2:0 is read at 8 bits (C420, C420jpeg, C420mpeg2) or 10 (C420p10)")
    if tag.startswith(("422", "444", "411", "mono")):
        raise Y4MError(f"y4m: C{tag} is not supported: only planar 4:2:0 is read (C420, C420jpeg, C420mpeg2, C420p10)")
    raise Y4MError(f"y4m: unknown colour space tag C{tag}")


def parse_header(line):
    """The first line of a stream (bytes, with or without its newline) -> Header"""
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
            _check_chroma(val)
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
    """One planar 4:2:0 frame: `data` holds Y, then U, then V as they stand in the stream (a 1-D uint8 array for 8-bit samples, a
    1-D uint16 array for 10-bit ones).  `.shape` is (H, W, 3) -- the size a frame-shaped consumer asks for -- although no such array
    exists."""

    def __init__(self, data, height, width, depth=8):
        if depth not in (8, 10):
            raise Y4MError(f"a YuvFrame holds 8- or 10-bit samples, got {depth}")
        dtype = np.uint8 if depth == 8 else np.dtype("<u2")
        if not isinstance(data, np.ndarray):
            data = np.frombuffer(data, dtype=dtype)
        self.height, self.width, self.depth = int(height), int(width), int(depth)
        (h, w), (hc, wc) = plane_sizes(height, width)
        if data.dtype != dtype or data.ndim != 1 or data.size != h * w + 2 * hc * wc:
            raise Y4MError(f"a {w}x{h} {depth}-bit 4:2:0 frame is {h * w + 2 * hc * wc} {np.dtype(dtype).name} samples, got {data.dtype} x {data.shape}")
        self.data = data

    @property
    def shape(self):
        return (self.height, self.width, 3)

    @property
    def maxval(self):
        return (1 << self.depth) - 1

    def planes(self):
        """-> (y [H,W], u [Hc,Wc], v [Hc,Wc]) views"""
        (h, w), (hc, wc) = plane_sizes(self.height, self.width)
        d = self.data
        return d[:h * w].reshape(h, w), d[h * w:h * w + hc * wc].reshape(hc, wc), d[h * w + hc * wc:].reshape(hc, wc)

    @classmethod
    def from_planes(cls, y, u, v, depth=8):
        dtype = np.uint8 if depth == 8 else np.dtype("<u2")
        return cls(np.concatenate([np.asarray(p, dtype=dtype).reshape(-1) for p in (y, u, v)]), y.shape[0], y.shape[1], depth)


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

    def __init__(self, fileobj):
        self.f = fileobj
        line = _read_line(fileobj)
        if not line.endswith(b"\n"):
            raise Y4MError("y4m: the stream ends inside its header" if line else "y4m: the stream is empty")
        self.header_bytes = len(line)
        self.header = parse_header(line)
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
        return YuvFrame(data, h.height, h.width, h.depth)

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

    def __init__(self, fileobj):
        seekable = getattr(fileobj, "seekable", None)
        if not (callable(seekable) and seekable() and hasattr(fileobj, "seek") and hasattr(fileobj, "tell")):
            raise Y4MError("y4m: random access needs a seekable stream (a file, not a pipe)")
        self.f = fileobj
        start = fileobj.tell()
        head = Reader(fileobj)
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
        return YuvFrame(data, h.height, h.width, h.depth)

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
