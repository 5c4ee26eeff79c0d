"""Picture metrics on finished frames: exact frame differences, PSNR and the RIFE lineage's `ssim_matlab` at full size.

    from drba_amd import metrics
    metrics.psnr(a, b), metrics.ssim(a, b), metrics.frame_error(a, b)       # one pair, Python numbers
    cm = metrics.ClipMetrics(); cm.add(a, b) ...; cm.result()               # a clip: nothing waits until result()

A frame is a uint8 [H,W,3] array (numpy or torch: what to_out emits; [N,H,W,3] is N frames), a uint16 one of the same shapes
(what to_out emits at depth=16; samples in [0, maxval], `maxval` 65535 unless given) or an fp32 [N,3,H,W] tensor; host
inputs are uploaded.  The arithmetic runs in metrics.hip (drba_ssim3d, drba_frame_error_u8 / _u16 / _f32): SSIM is the value of
the definition with the blurs accumulated in fp64 -- on flat content the reference's fp32 evaluation of the same formula is off
in the third decimal -- and the differences of bytes and of 16-bit samples are exact integers.  A uint16 frame is converted to
fp32 / maxval on the device (drba_u16hwc_to_f32nchw) for its SSIM, which then runs at val_range 1.

The back end is an argument (the way interpolate_stream takes to_inp / to_out / check_scene): tests drive the host logic with
a numpy stand-in.  The product has one back end, HipBackend; without a GPU it raises, there is no CPU fallback.

A back end provides
    prepare(x)                      -> (frame in the back end's form, "u8" | "u16" | "f32", (N, H, W))
    slots(capacity)                 -> result slots for `capacity` frames
    measure(slots, k, a, b, kind, shape, val_range, want_ssim)   enqueue the metrics of N pairs into slots k .. k + N - 1;
                                       "u16" pairs are measured with the further keyword maxval=
    collect(slots_list, counts)     -> rows (sum_sq, sum_abs, max_abs, count, ssim) of Python numbers, one per frame;
                                       count = differing bytes (u8) / samples (u16) or non-finite differences (f32); the one
                                       synchronisation
and, for planar 4:2:0 frames (YUV4MPEG2 clips; YuvClipMetrics, psnr_yuv, ssim_y), beside them and without touching them
    prepare(x, size)                -> (1-D packed Y, U, V samples, "yuv8" | "yuv16", (1, H, W)); x a y4m.YuvFrame (size from it) or
                                       a 1-D uint8 / uint16 array or tensor with size = (H, W): what ops.to_out_yuv returns
    slots_yuv(capacity)             -> result slots: per frame three 4-word error rows (Y, U, V) and one SSIM double
    measure_yuv(slots, k, a, b, kind, shape, maxval, want_ssim)   enqueue the plane errors (drba_frame_error_u8 / _u16, once per
                                       plane at its offset inside the packed frame) and the 2-D SSIM of luma (drba_ssim2d)
    collect_yuv(slots_list, counts) -> rows ((sum_sq, sum_abs, max_abs, differing) of Y, of U, of V, ssim_y); the one synchronisation
"""
import ctypes as C
import math

import numpy as np

from drba_amd import _lib, y4m


class HipBackend:
    """metrics.hip on the current device and stream."""

    def __init__(self, device=None):
        from drba_amd import ops
        self.ops = ops
        self.device = ops.default_device() if device is None else device

    def prepare(self, x, size=None, layout="420"):
        import torch
        if size is not None or isinstance(x, y4m.YuvFrame):
            return self._prepare_yuv(x, size, layout)
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if not torch.is_tensor(x):
            raise TypeError(f"a frame is a numpy array or a torch tensor, not {type(x).__name__}")
        if x.dtype == torch.uint8 and x.dim() in (3, 4) and x.shape[-1] == 3:
            x = x.to(self.device, non_blocking=True).contiguous()
            n = 1 if x.dim() == 3 else int(x.shape[0])
            return x, "u8", (n, int(x.shape[-3]), int(x.shape[-2]))
        if x.dtype == torch.uint16 and x.dim() in (3, 4) and x.shape[-1] == 3:
            x = x.to(self.device, non_blocking=True).contiguous()
            n = 1 if x.dim() == 3 else int(x.shape[0])
            return x, "u16", (n, int(x.shape[-3]), int(x.shape[-2]))
        if x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3:
            x = x.to(self.device, non_blocking=True).contiguous()
            return x, "f32", (int(x.shape[0]), int(x.shape[2]), int(x.shape[3]))
        raise TypeError(f"a frame is uint8 / uint16 [H,W,3] / [N,H,W,3] or fp32 [N,3,H,W], got {x.dtype} {tuple(x.shape)}")

    def slots(self, capacity):
        import torch
        # [capacity x 4 error words][capacity SSIM doubles], 8 bytes each: one tensor, one copy back
        return torch.zeros(int(capacity) * 5, dtype=torch.int64, device=self.device)

    def _planar16(self, x, shape, maxval):
        """uint16 [N,H,W,3] (or [H,W,3]) on the device -> fp32 [N,3,H,W] / maxval, frame by frame (no synchronisation)"""
        import torch
        lib, ops = _lib.load(), self.ops
        n, h, w = shape
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=x.device)
        for i in range(n):
            src = C.c_void_p(x.data_ptr() + 6 * h * w * i)
            _lib.check(lib.drba_u16hwc_to_f32nchw(src, ops._p(out[i]), h, w, float(maxval), ops._stream()), "drba_u16hwc_to_f32nchw")
        return out

    def measure(self, slots, k, a, b, kind, shape, val_range, want_ssim=True, maxval=None):
        lib, ops = _lib.load(), self.ops
        n, h, w = shape
        cap = slots.numel() // 5
        if k < 0 or k + n > cap:
            raise IndexError(f"slots {k} .. {k + n - 1} of {cap}")
        per_item = 3 * h * w
        err = C.c_void_p(slots.data_ptr() + 32 * k)
        ws = ops._workspace(self.device, max(lib.drba_frame_error_ws_floats(n, per_item), lib.drba_ssim3d_ws_floats(n, h, w)))
        fn = {"u8": lib.drba_frame_error_u8, "u16": lib.drba_frame_error_u16, "f32": lib.drba_frame_error_f32}[kind]
        _lib.check(fn(ops._p(a), ops._p(b), err, ops._p(ws), n, per_item, ops._stream()), "drba_frame_error_" + kind)
        if want_ssim:
            out = C.c_void_p(slots.data_ptr() + 8 * (4 * cap + k))
            if kind == "u16":  # planar fp32 / maxval on the device, then the fp32 form at range 1 unless another was asked for
                mv = ops._maxval(maxval)
                a, b, kind, val_range = self._planar16(a, shape, mv), self._planar16(b, shape, mv), "f32", (val_range or 1.0)
            _lib.check(lib.drba_ssim3d(ops._p(a), ops._p(b), out, ops._p(ws), n, h, w, 1 if kind == "u8" else 0,
                                       float(val_range or 0.0), ops._stream()), "drba_ssim3d")

    def collect(self, slots_list, counts):
        import torch
        if not slots_list:
            return []
        caps = [s.numel() // 5 for s in slots_list]
        parts = [torch.cat([s[:4 * c].view(c, 4)[:n].reshape(-1), s[4 * c:4 * c + n]]) for s, c, (n, _) in zip(slots_list, caps, counts)]
        host = (torch.cat(parts) if len(parts) > 1 else parts[0]).cpu().numpy()  # the one synchronisation
        rows, at = [], 0
        for n, kinds in counts:
            err, ssim = host[at:at + 4 * n].reshape(n, 4), host[at + 4 * n:at + 5 * n].view(np.float64)
            at += 5 * n
            for i in range(n):
                if kinds[i] in ("u8", "u16"):
                    e = err[i].view(np.uint64)
                    rows.append((int(e[0]), int(e[1]), int(e[2]), int(e[3]), float(ssim[i])))
                else:
                    e = err[i].view(np.float64)
                    rows.append((float(e[0]), float(e[1]), float(e[2]), int(err[i].view(np.uint64)[3]), float(ssim[i])))
        return rows

    # ---- planar 4:2:0 frames: per-plane errors and the 2-D SSIM of luma (drba_ssim2d) -------------------------------------------
    def _prepare_yuv(self, x, size, layout="420"):
        import torch
        if isinstance(x, y4m.YuvFrame):
            if x.layout != layout:
                raise ValueError(f"the frame is 4:{x.layout[1]}:{x.layout[2]}, the layout given is {layout!r}")
            x, size = torch.from_numpy(x.data if x.data.flags.writeable else x.data.copy()), x.shape[:2]
        elif isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if not (torch.is_tensor(x) and x.dim() == 1 and x.dtype in (torch.uint8, torch.uint16)) or size is None:
            raise TypeError("a planar 4:2:0 frame is a y4m.YuvFrame, or a 1-D uint8 / uint16 array of packed Y, U, V planes with its (H, W)")
        h, w = int(size[0]), int(size[1])
        ny, nc = yuv_samples((h, w), layout)
        if x.numel() != ny + 2 * nc:
            raise ValueError(f"a {w}x{h} 4:{layout[1]}:{layout[2]} frame is {ny + 2 * nc} samples, got {x.numel()}")
        return x.to(self.device, non_blocking=True).contiguous(), "yuv8" if x.dtype == torch.uint8 else "yuv16", (1, h, w)

    def slots_yuv(self, capacity):
        import torch
        # [capacity x 3 planes x 4 error words][capacity SSIM doubles], 8 bytes each: one tensor, one copy back
        return torch.zeros(int(capacity) * YUV_WORDS, dtype=torch.int64, device=self.device)

    def measure_yuv(self, slots, k, a, b, kind, shape, maxval, want_ssim=True, layout="420"):
        lib, ops = _lib.load(), self.ops
        _, h, w = shape
        cap = slots.numel() // YUV_WORDS
        if not 0 <= k < cap:
            raise IndexError(f"slot {k} of {cap}")
        ny, nc = yuv_samples((h, w), layout)
        es = a.element_size()
        fn = lib.drba_frame_error_u8 if kind == "yuv8" else lib.drba_frame_error_u16
        ws = ops._workspace(self.device, max(lib.drba_frame_error_ws_floats(1, ny), lib.drba_ssim2d_ws_floats(1, h, w)))
        for plane, (at, n) in enumerate(((0, ny), (ny, nc), (ny + nc, nc))):  # each plane at its offset inside the packed frame
            err = C.c_void_p(slots.data_ptr() + 32 * (3 * k + plane))
            _lib.check(fn(C.c_void_p(a.data_ptr() + at * es), C.c_void_p(b.data_ptr() + at * es), err, ops._p(ws), 1, n, ops._stream()),
                       "drba_frame_error_" + ("u8" if kind == "yuv8" else "u16"))
        if want_ssim:
            out = C.c_void_p(slots.data_ptr() + 8 * (12 * cap + k))
            _lib.check(lib.drba_ssim2d(ops._p(a), ops._p(b), out, ops._p(ws), 1, h, w, w, ny + 2 * nc, 1 if kind == "yuv8" else 2,
                                       float(maxval), ops._stream()), "drba_ssim2d")

    def collect_yuv(self, slots_list, counts):
        import torch
        if not slots_list:
            return []
        caps = [s.numel() // YUV_WORDS for s in slots_list]
        parts = [torch.cat([s[:12 * n], s[12 * c:12 * c + n]]) for s, c, n in zip(slots_list, caps, counts)]
        host = (torch.cat(parts) if len(parts) > 1 else parts[0]).cpu().numpy()  # the one synchronisation
        rows, at = [], 0
        for n in counts:
            err, ssim = host[at:at + 12 * n].view(np.uint64).reshape(n, 3, 4), host[at + 12 * n:at + 13 * n].view(np.float64)
            at += 13 * n
            rows += [tuple(tuple(int(v) for v in err[i, p]) for p in range(3)) + (float(ssim[i]),) for i in range(n)]
        return rows


YUV_WORDS = 13  # result words of a planar frame: three 4-word error rows (Y, U, V) and one SSIM double


def yuv420_samples(size):
    """(H, W) -> (samples of Y, of U (= of V)) of a packed planar 4:2:0 frame"""
    (h, w), (hc, wc) = y4m.plane_sizes(*size)
    return h * w, hc * wc


def yuv_samples(size, layout="420"):
    """yuv420_samples for a chroma layout: "420" | "422" | "444" (y4m.plane_sizes)"""
    (h, w), (hc, wc) = y4m.plane_sizes(*size, layout)
    return h * w, hc * wc


def _layout_kw(layout):
    """what a back end is told about the layout: nothing for 4:2:0 (a default is left out: back ends written for 4:2:0 keep working)"""
    return {} if layout == "420" else {"layout": layout}


def default_backend():
    return HipBackend()


def psnr_of_mse(mse, peak):
    """10 log10(peak^2 / mse); inf for mse = 0."""
    return math.inf if mse == 0 else 10.0 * math.log10(float(peak) ** 2 / mse)


def default_peak(kind, maxval=None):
    """255 for bytes, `maxval` (65535 unless given) for 16-bit samples, 1 for fp32 frames"""
    if kind == "u16":
        return float(65535 if maxval is None else maxval)
    return 255.0 if kind == "u8" else 1.0


def _pair(backend, a, b):
    a, ka, sa = backend.prepare(a)
    b, kb, sb = backend.prepare(b)
    if ka != kb or sa != sb:
        raise ValueError(f"the two frames differ in form: {ka} {sa} against {kb} {sb}")
    return a, b, ka, sa


def _maxval_kw(kind, maxval):
    """the keyword a back end's measure() gets for "u16" pairs (and only for them: "u8" / "f32" calls are what they were)"""
    if kind != "u16":
        if maxval is not None:
            raise ValueError(f"maxval belongs to uint16 frames, these are {kind}")
        return {}
    if maxval is not None and (int(maxval) != maxval or not 255 < int(maxval) <= 65535):
        raise ValueError(f"maxval of a 16-bit frame must be an integer with 255 < maxval <= 65535, got {maxval!r}")
    return {"maxval": 65535 if maxval is None else int(maxval)}


def _one_shot(a, b, val_range, want_ssim, backend, maxval=None):
    backend = backend or default_backend()
    a, b, kind, shape = _pair(backend, a, b)
    slots = backend.slots(shape[0])
    backend.measure(slots, 0, a, b, kind, shape, val_range, want_ssim, **_maxval_kw(kind, maxval))
    return backend.collect([slots], [(shape[0], [kind] * shape[0])]), kind, shape


def _scalar(values):
    return values[0] if len(values) == 1 else values


def frame_error(a, b, backend=None):
    """{"sum_sq", "sum_abs", "max_abs", "n", and "differing" (uint8 / uint16 frames: samples with d != 0; exact integers
    throughout, in the frames' own steps) or "nonfinite" (fp32 frames: the sums and the maximum run over the finite differences)};
    a list of them for N > 1 frames."""
    rows, kind, (n, h, w) = _one_shot(a, b, None, False, backend)
    name = "differing" if kind in ("u8", "u16") else "nonfinite"
    return _scalar([{"sum_sq": r[0], "sum_abs": r[1], "max_abs": r[2], name: r[3], "n": 3 * h * w} for r in rows])


def psnr(a, b, peak=None, backend=None, maxval=None):
    """10 log10(peak^2 / mse), inf for identical frames.  peak: 255 for uint8 frames, `maxval` (65535 unless given) for uint16
    ones, 1 for fp32 ones unless given."""
    rows, kind, (n, h, w) = _one_shot(a, b, None, False, backend, maxval)
    peak = default_peak(kind, maxval) if peak is None else peak
    return _scalar([psnr_of_mse(r[0] / (3.0 * h * w), peak) for r in rows])


def ssim(a, b, val_range=None, backend=None, maxval=None):
    """ssim_matlab (3-D 11^3 gaussian window, replicate padding) at full size.  val_range None: inferred from `a` per frame by
    the reference's rule (uint8 frames are scaled to [0, 1]: range 1; uint16 frames are divided by `maxval`, 65535 unless
    given: range 1)."""
    rows, _, _ = _one_shot(a, b, val_range, True, backend, maxval)
    return _scalar([r[4] for r in rows])


def summarise(mse, ssim_values, max_lsb, differing, peak, nonfinite=None):
    """-> {"frames", "peak", "per_frame": {...lists}, "summary": {...}} from per-frame figures (host arithmetic only).
    mean_psnr is taken over the frames with a finite PSNR (inf when there is none); psnr_of_mean_mse is the PSNR of the clip
    as one signal; the worst frame is the one with the lowest PSNR (ties: the lower SSIM, then the earlier frame)."""
    mse = [float(v) for v in mse]
    ps = [psnr_of_mse(v, peak) for v in mse]
    ss = [float(v) for v in ssim_values]
    n = len(mse)
    finite = [v for v in ps if math.isfinite(v)]
    worst = min(range(n), key=lambda i: (ps[i], ss[i], i)) if n else None
    per = {"psnr": ps, "ssim": ss, "max_lsb": list(max_lsb), "differing": [int(v) for v in differing]}
    if nonfinite is not None:
        per["nonfinite"] = [int(v) for v in nonfinite]
    summary = {"mean_psnr": (sum(finite) / len(finite)) if finite else math.inf,
               "psnr_of_mean_mse": psnr_of_mse(sum(mse) / n, peak) if n else math.inf,
               "mean_ssim": (sum(ss) / n) if n else math.nan, "min_ssim": min(ss) if n else math.nan,
               "max_lsb": max(max_lsb) if n else 0, "total_differing": int(sum(differing)), "worst_frame": worst}
    return {"frames": n, "peak": peak, "per_frame": per, "summary": summary}


class ClipMetrics:
    """Metrics of a clip, frame by frame.  add(a, b) enqueues the kernels of one pair (or of N pairs) on the current stream
    into result slots allocated ahead -- it never waits for the device --; result() synchronises once and returns
    {"frames", "peak", "per_frame": the lists "psnr", "ssim", "max_lsb", "differing", "summary": summarise()'s figures}.  max_lsb is max |d| in 8-bit steps
    (fp32 frames: max |d| * 255 / peak); fp32 frames report their non-finite differences under "nonfinite", not "differing".
    uint16 frames (samples in [0, maxval], 65535 unless given): max_lsb and differing are in 16-bit steps and samples, the peak is
    maxval unless `peak` is given."""

    def __init__(self, backend=None, capacity=256, val_range=None, peak=None, maxval=None):
        self.backend = backend or default_backend()
        self.capacity, self.val_range, self.peak, self.maxval = int(capacity), val_range, peak, maxval
        self._slots, self._cap, self._used, self._kinds, self._elems = [], [], [], [], []

    def __len__(self):
        return sum(self._used)

    def add(self, a, b):
        a, b, kind, (n, h, w) = _pair(self.backend, a, b)
        if not self._slots or self._used[-1] + n > self._cap[-1]:
            cap = max(self.capacity, n)
            self._slots.append(self.backend.slots(cap))
            self._used.append(0)
            self._kinds.append([])
            self._cap.append(cap)
        kw = _maxval_kw(kind, self.maxval) if kind == "u16" else {}  # (a clip's maxval does not hinder its 8-bit or fp32 pairs)
        self.backend.measure(self._slots[-1], self._used[-1], a, b, kind, (n, h, w), self.val_range, True, **kw)
        self._used[-1] += n
        self._kinds[-1] += [kind] * n
        self._elems += [3 * h * w] * n

    def result(self):
        rows = self.backend.collect(self._slots, list(zip(self._used, self._kinds)))
        kinds = [k for ks in self._kinds for k in ks]
        peak = self.peak if self.peak is not None else default_peak(kinds[0] if kinds else "u8", self.maxval)
        lsb = [r[2] if k in ("u8", "u16") else r[2] * 255.0 / peak for r, k in zip(rows, kinds)]
        return summarise([r[0] / e for r, e in zip(rows, self._elems)], [r[4] for r in rows], lsb,
                         [r[3] if k in ("u8", "u16") else 0 for r, k in zip(rows, kinds)], peak,
                         nonfinite=[r[3] if k == "f32" else 0 for r, k in zip(rows, kinds)])


# ------------------------------------------------------------------------------------------------- planar 4:2:0 clips
PLANES = ("y", "u", "v")


def _yuv_layout(a, b, layout):
    """the one layout of a pair: a YuvFrame's own, or the one given for packed planes (4:2:0 unless said)"""
    for x in (a, b):
        if isinstance(x, y4m.YuvFrame):
            if layout is not None and layout != x.layout:
                raise ValueError(f"the two frames differ in chroma layout: C{x.layout} against C{layout}")
            layout = x.layout
    return "420" if layout is None else layout


def _yuv_size(a, b, size):
    for x in (a, b):
        if isinstance(x, y4m.YuvFrame):
            if size is not None and tuple(size) != x.shape[:2]:
                raise ValueError(f"the frame is {x.shape[:2]}, the size given is {tuple(size)}")
            size = x.shape[:2]
    if size is None:
        raise ValueError("packed Y, U, V planes need their (H, W): pass size=")
    return int(size[0]), int(size[1])


def _yuv_pair(backend, a, b, size, layout="420"):
    size = _yuv_size(a, b, size)
    a, ka, sa = backend.prepare(a, size, **_layout_kw(layout))
    b, kb, sb = backend.prepare(b, size, **_layout_kw(layout))
    if ka != kb or sa != sb:
        raise ValueError(f"the two frames differ in form: {ka} {sa} against {kb} {sb}")
    return a, b, ka, sa


def _yuv_maxval(kind, maxval):
    """255 for 8-bit samples; 16-bit ones: `maxval`, 1023 (10 bits, what YUV4MPEG2 carries) unless given"""
    if kind == "yuv8":
        if maxval not in (None, 255):
            raise ValueError(f"8-bit samples have maxval 255, got {maxval!r}")
        return 255
    if maxval is not None and (int(maxval) != maxval or not 255 < int(maxval) <= 65535):
        raise ValueError(f"maxval of 16-bit samples must be an integer with 255 < maxval <= 65535, got {maxval!r}")
    return 1023 if maxval is None else int(maxval)


def summarise_yuv(rows, samples, peak):
    """-> {"frames", "peak", "per_frame", "summary"} from collect_yuv's rows and the (Y, U (= V)) sample counts per frame: host
    arithmetic on exact integers.  `psnr` pools the squared error of the three planes over all their samples -- the 4:1:1 weighting
    4:2:0 has by construction, 2:1:1 for 4:2:2 and 1:1:1 for 4:4:4 --; the summary follows summarise(), for the pooled figure and with _y / _u / _v for each plane."""
    n = len(rows)
    sq = [[r[p][0] for r in rows] for p in range(3)]
    cnt = [[s[0] for s in samples], [s[1] for s in samples], [s[1] for s in samples]]
    per = {"psnr_" + name: [psnr_of_mse(sq[p][i] / cnt[p][i], peak) for i in range(n)] for p, name in enumerate(PLANES)}
    pooled_sq = [sq[0][i] + sq[1][i] + sq[2][i] for i in range(n)]
    pooled_n = [cnt[0][i] + cnt[1][i] + cnt[2][i] for i in range(n)]
    per["psnr"] = [psnr_of_mse(pooled_sq[i] / pooled_n[i], peak) for i in range(n)]
    per["ssim_y"] = [float(r[3]) for r in rows]
    per["max_lsb"] = [max(r[p][2] for p in range(3)) for r in rows]
    per["differing"] = [sum(r[p][3] for p in range(3)) for r in rows]

    def mean_finite(ps):
        finite = [v for v in ps if math.isfinite(v)]
        return (sum(finite) / len(finite)) if finite else math.inf

    ps, ss = per["psnr"], per["ssim_y"]
    summary = {"mean_psnr": mean_finite(ps), "psnr_of_mean_mse": psnr_of_mse(sum(pooled_sq) / sum(pooled_n), peak) if n else math.inf}
    for p, name in enumerate(PLANES):
        summary["mean_psnr_" + name] = mean_finite(per["psnr_" + name])
        summary["psnr_of_mean_mse_" + name] = psnr_of_mse(sum(sq[p]) / sum(cnt[p]), peak) if n else math.inf
    summary.update({"mean_ssim": (sum(ss) / n) if n else math.nan, "min_ssim": min(ss) if n else math.nan,
                    "max_lsb": max(per["max_lsb"]) if n else 0, "total_differing": int(sum(per["differing"])),
                    "worst_frame": min(range(n), key=lambda i: (ps[i], ss[i], i)) if n else None})
    return {"frames": n, "peak": peak, "per_frame": per, "summary": summary}


class YuvClipMetrics:
    """ClipMetrics for planar 4:2:0 frames: add(a, b) takes two y4m.YuvFrames, or 1-D arrays / tensors of packed Y, U, V planes
    (what ops.to_out_yuv returns: they stay on the device) with size=(H, W) -- one of the two being a YuvFrame gives the size --,
    enqueues three plane errors and the 2-D SSIM of luma and never waits; result() synchronises once.
    Per frame: psnr_y / psnr_u / psnr_v, psnr (pooled over the samples of the three planes), ssim_y, max_lsb (the largest
    difference of the three planes, in the clip's own steps) and differing (samples).  The peak is maxval: 255, or for 16-bit
    samples `maxval` (1023 unless given)."""

    def __init__(self, backend=None, capacity=256, maxval=None):
        self.backend = backend or default_backend()
        self.capacity, self.maxval = int(capacity), maxval
        self._slots, self._used, self._samples, self._kind, self._layout = [], [], [], None, None

    def __len__(self):
        return sum(self._used)

    def add(self, a, b, size=None, layout=None):
        """layout: the chroma layout of packed planes ("420" unless given); a YuvFrame carries its own"""
        layout = _yuv_layout(a, b, layout)
        a, b, kind, (_, h, w) = _yuv_pair(self.backend, a, b, size, layout)
        if self._kind not in (None, kind):
            raise ValueError(f"a clip has one sample depth: {self._kind} so far, now {kind}")
        if self._layout not in (None, layout):
            raise ValueError(f"a clip has one chroma layout: {self._layout} so far, now {layout}")
        self._layout = layout
        mv = _yuv_maxval(kind, self.maxval)
        if not self._slots or self._used[-1] == self.capacity:
            self._slots.append(self.backend.slots_yuv(self.capacity))
            self._used.append(0)
        self.backend.measure_yuv(self._slots[-1], self._used[-1], a, b, kind, (1, h, w), mv, True, **_layout_kw(layout))
        self._kind = kind
        self._used[-1] += 1
        self._samples.append(yuv_samples((h, w), layout))

    def result(self):
        rows = self.backend.collect_yuv(self._slots, list(self._used))
        return summarise_yuv(rows, self._samples, float(_yuv_maxval(self._kind or "yuv8", self.maxval)))


def _one_shot_yuv(a, b, size, want_ssim, backend, maxval, layout=None):
    backend = backend or default_backend()
    layout = _yuv_layout(a, b, layout)
    a, b, kind, shape = _yuv_pair(backend, a, b, size, layout)
    mv = _yuv_maxval(kind, maxval)
    slots = backend.slots_yuv(1)
    backend.measure_yuv(slots, 0, a, b, kind, shape, mv, want_ssim, **_layout_kw(layout))
    return backend.collect_yuv([slots], [1])[0], yuv_samples(shape[1:], layout), float(mv)


def psnr_yuv(a, b, size=None, backend=None, maxval=None, layout=None):
    """{"psnr_y", "psnr_u", "psnr_v", "psnr"} of one pair of planar frames (peak = maxval; inf for identical planes); layout: of packed
    planes, 4:2:0 unless given"""
    row, samples, peak = _one_shot_yuv(a, b, size, False, backend, maxval, layout)
    per = summarise_yuv([row], [samples], peak)["per_frame"]
    return {k: per[k][0] for k in ("psnr_y", "psnr_u", "psnr_v", "psnr")}


def ssim_y(a, b, size=None, backend=None, maxval=None):
    """The single-channel 2-D ssim (11 x 11 gaussian window, replicate padding) of the luma planes of one pair of 4:2:0 frames"""
    return _one_shot_yuv(a, b, size, True, backend, maxval)[0][3]
