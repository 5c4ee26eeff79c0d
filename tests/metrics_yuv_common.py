"""Shared pieces of the YUV4MPEG2 metric tests (tests/test_metrics_yuv_cpu.py, tests/test_gpu_metrics_yuv.py): the float64 truth of
the single-channel 2-D ssim, the plane pairs it is asked on, a numpy stand-in for the planar back-end methods of drba_amd.metrics
(with and without a planted defect: the rows CAN fail) and small clips on disk.

SSIM.  The truth is the definition of pytorch_msssim's ssim() on one channel (window 11 x 11 of gaussian(11, 1.5), replicate
padding 5 on both axes, C1 = 0.01^2, C2 = 0.03^2 at L = 1, the mean over all H W positions) evaluated in float64 with a DENSE
11 x 11 convolution of the reference's fp32 window widened (not the separable form the kernel uses), on the fp32 inputs
(float)s / (float)maxval widened.  The bar is tests/metric_checks.SSIM_TOL (2e-5), the project's bar for the fp64-accumulating
SSIM kernel.  tests/golden/ssim2d_reference.npz holds the values of the reference's own ssim() on a few of these pairs.
"""
import io
import os

import numpy as np
import torch
import torch.nn.functional as F

from drba_amd import metrics, y4m
from tests import metric_checks as mc
from tests import yuv_common as yc

SSIM_TOL = mc.SSIM_TOL
SSIM2D_SHAPES = ((11, 11), (11, 40), (40, 11), (13, 37), (mc.TILE_H + 1, mc.TILE_W + 1), (45, 70))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim2d_reference.npz")


# ------------------------------------------------------------------------------------------------------------------- SSIM
def window_2d():
    """pytorch_msssim/__init__.py:9-18 at one channel: the fp32 outer product of the normalised fp32 1-D gaussian, [1,1,11,11]"""
    g = torch.Tensor([float(np.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2))) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)


def as_unit(plane, maxval):
    """integer plane [H,W] -> fp32 torch [1,1,H,W]: (float)s / (float)maxval, the division in fp32"""
    return torch.from_numpy((np.asarray(plane).astype(np.float32) / np.float32(maxval))[None, None])


def ssim_formula(x, y, window, L=1.0):
    """the map's mean for [1,1,H,W] inputs, in the dtype of its arguments"""
    def blur(v):
        return F.conv2d(F.pad(v, (5, 5, 5, 5), mode="replicate"), window)

    mu1, mu2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    m = ((2 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return float(m.mean())


def ssim2d_truth(p, q, maxval):
    """float64, dense window, from the fp32 inputs widened"""
    return ssim_formula(as_unit(p, maxval).double(), as_unit(q, maxval).double(), window_2d().double())


def ssim2d_fp32(p, q, maxval):
    """the same formula evaluated in fp32 (what an fp32-accumulating kernel computes, up to its summation order)"""
    return ssim_formula(as_unit(p, maxval), as_unit(q, maxval), window_2d())


def _dtype(maxval):
    return np.uint8 if maxval == 255 else np.uint16


def noisy_planes(h, w, maxval, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(0, maxval + 1, (h, w))
    q = np.clip(p + np.rint(rng.standard_normal((h, w)) * 0.05 * maxval).astype(np.int64), 0, maxval)
    return p.astype(_dtype(maxval)), q.astype(_dtype(maxval))


def flat_planes(h, w, maxval):
    """a constant near the top of the range and the same constant plus a one-step checker: sigma^2 is a quarter of a squared step,
    1e-6 of C2 at 8 bits -- the content on which blur(a a) - blur(a)^2 cancels in fp32"""
    c = (maxval * 237) // 255
    p = np.full((h, w), c, np.int64)
    q = p + ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1)
    return p.astype(_dtype(maxval)), q.astype(_dtype(maxval))


_cases = None


def ssim2d_cases():
    """[(name, p, q, maxval, truth)]: computed once, shared by every test that needs them"""
    global _cases
    if _cases is None:
        _cases = []
        for maxval in (255, 1023):
            for k, (h, w) in enumerate(SSIM2D_SHAPES):
                for kind, (p, q) in (("noisy", noisy_planes(h, w, maxval, 300 + k)), ("flat", flat_planes(h, w, maxval))):
                    _cases.append((f"{h}x{w} maxval={maxval} {kind}", p, q, maxval, ssim2d_truth(p, q, maxval)))
    return _cases


def check_ssim2d(fn):
    """fn(p, q, maxval) -> float for integer planes [H,W]; rows (name, err, tol, extra) with the pass rule err <= tol"""
    rows = []
    for name, p, q, maxval, truth in ssim2d_cases():
        got = float(fn(p, q, maxval))
        err = abs(got - truth) if np.isfinite(got) else float("inf")
        rows.append((name, err, SSIM_TOL, f"truth={truth:.9f} fp32_formula_err={abs(ssim2d_fp32(p, q, maxval) - truth):.2e}"))
    return rows


def golden_pairs():
    """the plane pairs of tests/golden/ssim2d_reference.npz, regenerated: [(key, p, q, maxval)] (the fixture stores them too; its
    generator, tests/golden/make_ssim2d_reference.py, takes them from here)"""
    out = []
    for maxval in (255, 1023):
        for k, (h, w) in enumerate(((13, 37), (17, 33), (45, 70))):
            out.append((f"noisy_{maxval}_{h}x{w}", *noisy_planes(h, w, maxval, 400 + k), maxval))
        out.append((f"flat_{maxval}_17x33", *flat_planes(17, 33, maxval), maxval))
    return out


# ---------------------------------------------------------------------------------------- a numpy back end for the host logic
def plane_rows(a, b, size):
    """packed planes -> ((sum_sq, sum_abs, max_abs, differing) of Y, of U, of V) in numpy int64"""
    out = []
    for pa, pb in zip(yc.split(a, size), yc.split(b, size)):
        d = np.abs(pa.astype(np.int64) - pb.astype(np.int64))
        out.append((int((d * d).sum()), int(d.sum()), int(d.max()), int((d != 0).sum())))
    return tuple(out)


class NumpyYuvBackend(mc.NumpyBackend):
    """the planar methods of drba_amd.metrics' back-end protocol on the host (tests only).  swap_uv plants a defect: the rows of U
    and V change places."""

    def __init__(self, swap_uv=False):
        super().__init__()
        self.swap_uv = swap_uv

    def prepare(self, x, size=None):
        if size is None and not isinstance(x, y4m.YuvFrame):
            return super().prepare(x)
        if isinstance(x, y4m.YuvFrame):
            x, size = x.data, x.shape[:2]
        x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        assert x.ndim == 1 and x.dtype in (np.uint8, np.uint16), (x.dtype, x.shape)
        return x, "yuv8" if x.dtype == np.uint8 else "yuv16", (1, int(size[0]), int(size[1]))

    def slots_yuv(self, capacity):
        return [None] * int(capacity)

    def measure_yuv(self, slots, k, a, b, kind, shape, maxval, want_ssim=True):
        _, h, w = shape
        self.pairs.append((a, b))
        ry, ru, rv = plane_rows(a, b, (h, w))
        if self.swap_uv:
            ru, rv = rv, ru
        ss = float("nan")
        if want_ssim and h >= 11 and w >= 11:
            ss = ssim2d_truth(yc.split(a, (h, w))[0], yc.split(b, (h, w))[0], maxval)
        slots[k] = (ry, ru, rv, ss)

    def collect_yuv(self, slots_list, counts):
        return [s[i] for s, n in zip(slots_list, counts) for i in range(n)]


def expected_figures(fa, fb, size, maxval):
    """numpy int64 / float64 figures of lists of packed frames -> the per_frame dict YuvClipMetrics must report (without ssim_y)"""
    per = {k: [] for k in ("psnr_y", "psnr_u", "psnr_v", "psnr", "max_lsb", "differing")}
    for a, b in zip(fa, fb):
        d = [np.abs(pa.astype(np.int64) - pb.astype(np.int64)).reshape(-1) for pa, pb in zip(yc.split(a, size), yc.split(b, size))]
        for name, dp in zip("yuv", d):
            per["psnr_" + name].append(metrics.psnr_of_mse(float((dp * dp).sum()) / dp.size, float(maxval)))
        allp = np.concatenate(d)  # the PSNR of the concatenated samples
        per["psnr"].append(metrics.psnr_of_mse(float((allp * allp).sum()) / allp.size, float(maxval)))
        per["max_lsb"].append(int(allp.max()))
        per["differing"].append(int((allp != 0).sum()))
    return per


# ------------------------------------------------------------------------------------------------------------------ clips
def random_clip(n, h, w, bits, seed):
    return [yc.random_frame(h, w, bits, seed + i) for i in range(n)]


def write_clip(path, frames, chroma=None, color_range=None, fps=(24, 1), frame_params=None):
    """frames (YuvFrames) -> a .y4m file; frame_params {index: b"Ixyz"}: FRAME lines that carry parameters"""
    f0 = frames[0]
    chroma = chroma or ("420p10" if f0.depth == 10 else "420jpeg")
    hdr = y4m.Header(f0.width, f0.height, fps, chroma=chroma, color_range=color_range)
    buf = io.BytesIO()
    buf.write(hdr.format())
    for i, f in enumerate(frames):
        par = (frame_params or {}).get(i)
        buf.write(b"FRAME" + (b" " + par if par else b"") + b"\n")
        buf.write(np.ascontiguousarray(f.data).view(np.uint8).tobytes())
    data = buf.getvalue()
    if path is not None:
        with open(path, "wb") as fh:
            fh.write(data)
    return data
