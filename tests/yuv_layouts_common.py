"""Shared pieces of the planar 4:2:2 / 4:4:4 tests (tests/test_y4m_layouts_cpu.py, tests/test_gpu_yuv_layouts.py): the fp64 numpy
restatement of tests/yuv_common.py with the chroma layout as an argument, frames built for the checks, and whole-clip hooks.

There is no reference for these frames; the restatement, written from the definition in INTEGRATION.md ("Planar YUV 4:2:2 and
4:4:4"), is the truth.  Colour conversion, ranges, clamps, NaN -> 0, round-half-even and saturation are those of 4:2:0
(yuv_common: consts, MATRICES, quantise).  A layout subsamples chroma by (sx, sy): 4:2:0 (2, 2), 4:2:2 (2, 1), 4:4:4 (1, 1).

    up(c):  along a subsampled axis the bilinear taps at s = p/2 - 0.25 clamped (yuv_common.chroma_taps); along a full-resolution
            axis the sample itself
    box(c): the mean over the sx x sy luma block of a chroma sample, a pixel past an odd edge repeating the edge pixel

`layout="420"` gives yuv_common's own figures (tests/test_y4m_layouts_cpu.py checks that).
"""
import numpy as np
import torch

from drba_amd import y4m
from tests import depth16_common as d16
from tests import fit_pad_common as fpc
from tests.yuv_common import (CLIP_TOL_STEPS, MATRICES, TIE_SHARE_MAX, TIE_WINDOW_STEPS, TO_INP_TOL, chroma_taps, consts,  # noqa: F401
                              planted_codes, planted_net_frame, quantise, y4m_bytes)

LAYOUTS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
TAGS = {("422", 8): "422", ("422", 10): "422p10", ("444", 8): "444", ("444", 10): "444p10", ("420", 8): "420jpeg", ("420", 10): "420p10"}


def upsample(c, H, W, layout):
    """chroma plane [Hc, Wc] -> [H, W], fp64"""
    sx, sy = LAYOUTS[layout]
    c = np.asarray(c, dtype=np.float64)
    if sx == 2:
        x0, x1, wx0, wx1 = chroma_taps(W, c.shape[1])
        c = c[:, x0] * wx0 + c[:, x1] * wx1
    if sy == 2:
        y0, y1, wy0, wy1 = chroma_taps(H, c.shape[0])
        c = c[y0] * wy0[:, None] + c[y1] * wy1[:, None]
    assert c.shape == (H, W), (c.shape, H, W, layout)
    return c


def box(c, layout):
    """[H, W] -> [ceil(H/sy), ceil(W/sx)]: the mean of each block, edges replicated"""
    sx, sy = LAYOUTS[layout]
    H, W = c.shape
    Hc, Wc = (H + sy - 1) // sy, (W + sx - 1) // sx
    p = np.pad(c, ((0, sy * Hc - H), (0, sx * Wc - W)), mode="edge")
    return sum(p[dy::sy, dx::sx] for dy in range(sy) for dx in range(sx)) / float(sx * sy)


def planes_of(frame):
    return frame.planes() if isinstance(frame, y4m.YuvFrame) else frame


def to_bgr_unclamped(frame, bits, matrix="bt709", full=False, layout="444"):
    y, u, v = (np.asarray(p, dtype=np.float64) for p in planes_of(frame))
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    m, yo, ysc, co, csc = consts(bits, full)
    H, W = y.shape
    Y = (y - yo) / ysc
    Cb, Cr = upsample((u - co) / csc, H, W, layout), upsample((v - co) / csc, H, W, layout)
    R = Y + 2.0 * (1.0 - kr) * Cr
    B = Y + 2.0 * (1.0 - kb) * Cb
    G = (Y - kr * R - kb * B) / kg
    return np.stack([B, G, R])


def to_inp_ref(frame, dst, bits, matrix="bt709", full=False, layout="444"):
    """-> fp64 torch tensor [1, 3, *dst]"""
    bgr = np.clip(to_bgr_unclamped(frame, bits, matrix, full, layout), 0.0, 1.0)
    return d16.resize(torch.from_numpy(bgr).unsqueeze(0), tuple(dst))


def to_inp_pad_ref(frame, dst, bits, matrix="bt709", full=False, layout="444"):
    """fit = pad: the conversion at the frame's own size, edge-padded (a margin pixel is the converted pixel of the clamped coordinate)"""
    (h, w), _ = y4m.plane_sizes(*planes_of(frame)[0].shape, layout)
    return fpc.pad_planes(to_inp_ref(frame, (h, w), bits, matrix, full, layout), dst)


def to_out_unrounded(x, src, bits, matrix="bt709", full=False, layout="444"):
    """fp32 (or fp64) [1, 3, h, w] -> the three planes as fp64 codes before rounding and saturation"""
    r = d16.resize(x, tuple(src))[0].numpy().astype(np.float64)
    r = np.clip(np.where(np.isnan(r), 0.0, r), 0.0, 1.0)
    B, G, R = r
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    Y = kr * R + kg * G + kb * B
    Cb, Cr = (B - Y) / (2.0 * (1.0 - kb)), (R - Y) / (2.0 * (1.0 - kr))
    m, yo, ysc, co, csc = consts(bits, full)
    return yo + ysc * Y, co + csc * box(Cb, layout), co + csc * box(Cr, layout)


def to_out_ref(x, src, bits, matrix="bt709", full=False, layout="444"):
    """-> 1-D array: Y, U, V packed (uint8 at 8 bits, uint16 at 10)"""
    return np.concatenate([p.reshape(-1) for p in quantise(to_out_unrounded(x, src, bits, matrix, full, layout), bits)])


def to_out_crop_ref(x, src, bits, matrix="bt709", full=False, layout="444"):
    """fit = pad: the restatement of the window (the chroma mean sees the window alone)"""
    return to_out_ref(fpc.crop(x, src), src, bits, matrix, full, layout)


def split(packed, size, layout):
    (h, w), (hc, wc) = y4m.plane_sizes(*size, layout)
    packed = np.asarray(packed)
    assert packed.shape == (h * w + 2 * hc * wc,), (packed.shape, size, layout)
    return packed[:h * w].reshape(h, w), packed[h * w:h * w + hc * wc].reshape(hc, wc), packed[h * w + hc * wc:].reshape(hc, wc)


def frame_of(packed, size, bits, layout):
    return y4m.YuvFrame(np.ascontiguousarray(packed), size[0], size[1], bits, layout)


def compare_out(got, x, src, bits, matrix, full, layout, crop=False):
    """yuv_common.compare_out for a layout -> (max |d| in steps, samples that differ, those OUTSIDE the tie window, share inside it);
    got=None: the restatement alone (the share)"""
    xs = fpc.crop(x, src) if crop else x
    unr = np.concatenate([p.reshape(-1) for p in to_out_unrounded(xs, src, bits, matrix, full, layout)])
    near = np.abs(unr - np.floor(unr) - 0.5) <= TIE_WINDOW_STEPS
    if got is None:
        return 0, 0, 0, float(near.mean())
    want = np.concatenate([p.reshape(-1) for p in quantise(split(unr, src, layout), bits)])
    d = np.abs(np.asarray(got).astype(np.int64) - want.astype(np.int64))
    return int(d.max()), int((d != 0).sum()), int(((d != 0) & ~near).sum()), float(near.mean())


def cpu_hooks(bits_in, bits_out, layout_in, layout_out, matrix="bt709", full=False):
    """to_inp / to_out / check_scene for interpolate_stream on the CPU (fp32 tensors between them)"""
    import oracle
    return ((lambda fr, size: to_inp_ref(fr, size, bits_in, matrix, full, layout_in).float()),
            (lambda x, size: to_out_ref(x, size, bits_out, matrix, full, layout_out)), oracle.scdet.check_scene)


# ---------------------------------------------------------------------------------------------------------------- test frames
def _dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


def random_frame(h, w, bits, seed, layout):
    """uniform samples in all three planes, the extremes 0 and m planted at the corners of each (yuv_common.random_frame)"""
    m = (1 << bits) - 1
    rng = np.random.default_rng(seed)
    _, (hc, wc) = y4m.plane_sizes(h, w, layout)
    planes = [rng.integers(0, m + 1, size=s).astype(_dtype(bits)) for s in ((h, w), (hc, wc), (hc, wc))]
    for k, p in enumerate(planes):
        p[0, 0], p[0, -1], p[-1, 0], p[-1, -1] = (0, m, m, 0) if k != 1 else (m, 0, 0, m)
    return y4m.YuvFrame.from_planes(*planes, depth=bits, layout=layout)


def in_gamut_frame(h, w, bits, seed, layout, flat_chroma=False):
    """yuv_common.in_gamut_frame for a layout: every pixel's RGB strictly inside [0, 1] for both matrices and ranges (interpolated
    chroma stays inside the range its samples span)"""
    k = 1 << (bits - 8)
    rng = np.random.default_rng(seed)
    _, (hc, wc) = y4m.plane_sizes(h, w, layout)
    y = rng.integers(80 * k, 180 * k + 1, size=(h, w))
    if flat_chroma:
        u, v = np.full((hc, wc), 100 * k + 1), np.full((hc, wc), 150 * k - 1)
    else:
        u, v = rng.integers(108 * k, 148 * k + 1, size=(hc, wc)), rng.integers(108 * k, 148 * k + 1, size=(hc, wc))
    return y4m.YuvFrame.from_planes(y, u, v, depth=bits, layout=layout)


def picture_as(frame444, layout):
    """a 4:4:4 frame -> the same picture in `layout`, its chroma the rounded block mean"""
    y, u, v = frame444.planes()
    q = [np.rint(box(p.astype(np.float64), layout)).astype(p.dtype) for p in (u, v)]
    return y4m.YuvFrame.from_planes(y, q[0], q[1], depth=frame444.depth, layout=layout)


def clip_from_bgr(frames, bits, layout, matrix="bt709", full=False):
    """HWC BGR frames (uint8, or uint16 with samples in [0, 65535]) -> YuvFrames through the restatement's way out"""
    out = []
    for f in frames:
        peak = 255.0 if f.dtype == np.uint8 else 65535.0
        x = torch.from_numpy(np.ascontiguousarray(f).astype(np.float32).transpose(2, 0, 1).copy()).unsqueeze(0) / peak
        out.append(frame_of(to_out_ref(x, f.shape[:2], bits, matrix, full, layout), f.shape[:2], bits, layout))
    return out


def header_for(h, w, bits, layout, fps=(24, 1), **kw):
    return y4m.Header(w, h, fps, interlace="p", chroma=TAGS[(layout, bits)], **kw)


# sample positions whose every tap lies inside planted_net_frame's blocks, per geometry kind and layout: luma (row, col) and the
# chroma sample that covers it.  resized: (45, 71) <- (64, 128), output row 17 reads net rows 24, 25 and column 26 / 27 net columns
# 47 .. 49 (rows 31 -> 44, 45); window: the (45, 71) window of the net frame itself.
PLANTED = {
    "resized": {"422": {"black": ((17, 26), (17, 13)), "white": ((31, 26), (31, 13))},
                "444": {"black": ((17, 26), (17, 26)), "white": ((31, 26), (31, 26))}},
    "window": {"422": {"black": ((25, 45), (25, 22)), "white": ((44, 45), (44, 22))},
               "444": {"black": ((25, 45), (25, 45)), "white": ((44, 45), (44, 45))}},
}
