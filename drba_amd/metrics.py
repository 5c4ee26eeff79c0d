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
"""
import ctypes as C
import math

import numpy as np

from drba_amd import _lib


class HipBackend:
    """metrics.hip on the current device and stream."""

    def __init__(self, device=None):
        from drba_amd import ops
        self.ops = ops
        self.device = ops.default_device() if device is None else device

    def prepare(self, x):
        import torch
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
