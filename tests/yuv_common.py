"""Shared pieces of the planar 4:2:0 tests (tests/test_y4m_cpu.py, tests/test_gpu_yuv.py): the CPU restatement of the YCbCr
conversions in numpy fp64, frames built for the checks, and whole-clip hooks.

There is no reference for these frames; the restatement below, written from the definition in INTEGRATION.md ("Planar YUV
4:2:0"), is the truth.  Notation: b bits per sample (8 | 10), m = 2^b - 1, k = 2^(b-8); (Kr, Kb) = (0.2126, 0.0722) bt709,
(0.299, 0.114) bt601; limited range Y' = (y - 16k) / 219k, Cb = (u - 128k) / 224k; full range Y' = y / m, Cb = (u - 128k) / m.

    to_inp = resize(clamp01(rgb(Y', up(Cb), up(Cr))), dst)      up: bilinear taps at s = x/2 - 0.25 clamped, both axes
    to_out = round_half_even(code(Y', mean2x2(Cb), mean2x2(Cr))) of clamp01(resize(x, src)), NaN -> 0, saturated to [0, m]

with `resize` = tests.depth16_common.resize (the loop ATen runs on frames), channel order BGR.
"""
import numpy as np
import torch

from drba_amd import y4m
from tests import depth16_common as d16

MATRICES = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}
TO_INP_TOL = 2e-6        # fp32 kernel vs fp64 restatement: ~16 roundings on magnitudes <= 2, 16 * 2 * 6e-8
TIE_WINDOW_STEPS = 2e-3  # way out: one step of difference is allowed where the unrounded fp64 value is this close to a half-integer
TIE_SHARE_MAX = 0.01     # ... and at most this share of the samples may lie in that window (0.4 % for uniform values)
CLIP_TOL_STEPS = 1       # whole clip: 1e-3 of a frame is 0.22 steps of 219 and 0.88 of 876; |round(a) - round(b)| <= ceil(|a - b|)


def consts(bits, full):
    """-> (m, y_off, y_scale, c_off, c_scale): code = off + scale * value"""
    m, k = (1 << bits) - 1, 1 << (bits - 8)
    if full:
        return m, 0.0, float(m), 128.0 * k, float(m)
    return m, 16.0 * k, 219.0 * k, 128.0 * k, 224.0 * k


def chroma_taps(n, nc):
    s = np.clip(np.arange(n, dtype=np.float64) / 2 - 0.25, 0.0, nc - 1.0)
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, nc - 1)
    w1 = s - i0
    return i0, i1, 1.0 - w1, w1


def upsample(c, H, W):
    """chroma plane [Hc, Wc] -> [H, W], fp64"""
    y0, y1, wy0, wy1 = chroma_taps(H, c.shape[0])
    x0, x1, wx0, wx1 = chroma_taps(W, c.shape[1])
    top = c[y0][:, x0] * wx0 + c[y0][:, x1] * wx1
    bot = c[y1][:, x0] * wx0 + c[y1][:, x1] * wx1
    return top * wy0[:, None] + bot * wy1[:, None]


def planes_of(frame):
    return frame.planes() if isinstance(frame, y4m.YuvFrame) else frame


def to_bgr_unclamped(frame, bits, matrix="bt709", full=False):
    """(y, u, v) integer planes (or a YuvFrame) -> fp64 [3, H, W], BGR, before the clamp"""
    y, u, v = (np.asarray(p, dtype=np.float64) for p in planes_of(frame))
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    m, yo, ysc, co, csc = consts(bits, full)
    H, W = y.shape
    Y = (y - yo) / ysc
    Cb, Cr = upsample((u - co) / csc, H, W), upsample((v - co) / csc, H, W)
    R = Y + 2.0 * (1.0 - kr) * Cr
    B = Y + 2.0 * (1.0 - kb) * Cb
    G = (Y - kr * R - kb * B) / kg
    return np.stack([B, G, R])


def to_inp_ref(frame, dst, bits, matrix="bt709", full=False):
    """-> fp64 torch tensor [1, 3, *dst]"""
    bgr = np.clip(to_bgr_unclamped(frame, bits, matrix, full), 0.0, 1.0)
    return d16.resize(torch.from_numpy(bgr).unsqueeze(0), tuple(dst))


def to_out_unrounded(x, src, bits, matrix="bt709", full=False):
    """fp32 (or fp64) [1, 3, h, w] -> the three planes as fp64 codes before rounding and saturation"""
    r = d16.resize(x, tuple(src))[0].numpy().astype(np.float64)
    r = np.clip(np.where(np.isnan(r), 0.0, r), 0.0, 1.0)
    B, G, R = r
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    Y = kr * R + kg * G + kb * B
    Cb, Cr = (B - Y) / (2.0 * (1.0 - kb)), (R - Y) / (2.0 * (1.0 - kr))
    H, W = Y.shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2

    def box(c):
        p = np.pad(c, ((0, 2 * Hc - H), (0, 2 * Wc - W)), mode="edge")
        return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) / 4.0

    m, yo, ysc, co, csc = consts(bits, full)
    return yo + ysc * Y, co + csc * box(Cb), co + csc * box(Cr)


def quantise(planes, bits):
    m = (1 << bits) - 1
    dtype = np.uint8 if bits == 8 else np.uint16
    return [np.clip(np.rint(p), 0, m).astype(dtype) for p in planes]  # np.rint: half to even


def to_out_ref(x, src, bits, matrix="bt709", full=False):
    """-> 1-D array: Y, U, V packed (uint8 at 8 bits, uint16 at 10)"""
    return np.concatenate([p.reshape(-1) for p in quantise(to_out_unrounded(x, src, bits, matrix, full), bits)])


def split(packed, size):
    """1-D packed frame -> (y, u, v) planes"""
    (h, w), (hc, wc) = y4m.plane_sizes(*size)
    packed = np.asarray(packed)
    assert packed.shape == (h * w + 2 * hc * wc,), (packed.shape, size)
    return packed[:h * w].reshape(h, w), packed[h * w:h * w + hc * wc].reshape(hc, wc), packed[h * w + hc * wc:].reshape(hc, wc)


def frame_of(packed, size, bits):
    return y4m.YuvFrame(np.ascontiguousarray(packed), size[0], size[1], bits)


def cpu_hooks(bits_in, bits_out, matrix="bt709", full=False):
    """to_inp / to_out / check_scene for interpolate_stream on the CPU, planar 4:2:0 at both ends (fp32 tensors between them)"""
    import oracle
    return ((lambda fr, size: to_inp_ref(fr, size, bits_in, matrix, full).float()),
            (lambda x, size: to_out_ref(x, size, bits_out, matrix, full)), oracle.scdet.check_scene)


# ---------------------------------------------------------------------------------------------------------------- test frames
def random_frame(h, w, bits, seed):
    """uniform samples in all three planes, the extremes 0 and m planted at the corners of each"""
    m = (1 << bits) - 1
    rng = np.random.default_rng(seed)
    (_, _), (hc, wc) = y4m.plane_sizes(h, w)
    planes = [rng.integers(0, m + 1, size=s).astype(np.uint8 if bits == 8 else np.uint16) for s in ((h, w), (hc, wc), (hc, wc))]
    for k, p in enumerate(planes):
        p[0, 0], p[0, -1], p[-1, 0], p[-1, -1] = (0, m, m, 0) if k != 1 else (m, 0, 0, m)
    return y4m.YuvFrame.from_planes(*planes, depth=bits)


def in_gamut_frame(h, w, bits, seed, flat_chroma=False):
    """luma well inside its range and little chroma: every pixel's RGB lies strictly inside [0, 1] for both matrices and ranges"""
    k = 1 << (bits - 8)
    rng = np.random.default_rng(seed)
    (_, _), (hc, wc) = y4m.plane_sizes(h, w)
    y = rng.integers(80 * k, 180 * k + 1, size=(h, w))
    if flat_chroma:
        u, v = np.full((hc, wc), 100 * k + 1), np.full((hc, wc), 150 * k - 1)
    else:
        u, v = rng.integers(108 * k, 148 * k + 1, size=(hc, wc)), rng.integers(108 * k, 148 * k + 1, size=(hc, wc))
    return y4m.YuvFrame.from_planes(y, u, v, depth=bits)


def legal_luma_frame(h, w, bits, full):
    """every legal luma code (0 .. m full range, 16k .. 235k limited), repeated to fill h x w, over neutral chroma"""
    m, k = (1 << bits) - 1, 1 << (bits - 8)
    vals = np.arange(0, m + 1) if full else np.arange(16 * k, 235 * k + 1)
    assert h * w >= vals.size
    (_, _), (hc, wc) = y4m.plane_sizes(h, w)
    return y4m.YuvFrame.from_planes(np.resize(vals, (h, w)), np.full((hc, wc), 128 * k), np.full((hc, wc), 128 * k), depth=bits)


def planted_net_frame(net, seed):
    """fp32 [1, 3, *net] uniform in [-0.01, 1.01] with blocks and single samples of NaN, +inf, -0.5 and 1.5 (tests/test_gpu_depth16.py):
    rows 20:30 x columns 40:56 hold (B, G, R) = (NaN, -0.5, NaN) -> (0, 0, 0), rows 40:50 x the same columns (+inf, 1.5, +inf) ->
    (1, 1, 1); single samples elsewhere.  (Black and white have integer codes at every depth and range.  A block of a saturated
    COLOUR would put a whole block of samples on a tie or next to one -- Cr of pure red is exactly 1/2, 0.587 * 1023 = 600.501 --
    and use up the share of samples the comparison may allow a step to.)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, 3, net[0], net[1], generator=g) * 1.02 - 0.01
    x[0, 0, 20:30, 40:56], x[0, 1, 20:30, 40:56], x[0, 2, 20:30, 40:56] = float("nan"), -0.5, float("nan")
    x[0, 0, 40:50, 40:56], x[0, 1, 40:50, 40:56], x[0, 2, 40:50, 40:56] = float("inf"), 1.5, float("inf")
    x[0, 1, 3, 7], x[0, 2, 50, 9], x[0, 0, 63, net[1] - 1], x[0, 2, 0, 0] = float("nan"), float("inf"), -0.5, 1.5
    return x


def planted_codes(bits, full):
    """the (y, u, v) codes of black and white from the definition: {"black": ..., "white": ...}"""
    m, yo, ysc, co, csc = consts(bits, full)
    return {"black": (int(yo), int(co), int(co)), "white": (int(yo + ysc), int(co), int(co))}


def compare_out(got, x, src, bits, matrix, full):
    """The way-out rule of the tests: got (1-D packed) against the restatement -> (max |d| in steps, samples that differ, samples that
    differ OUTSIDE the tie window, share of samples inside the window)."""
    unr = np.concatenate([p.reshape(-1) for p in to_out_unrounded(x, src, bits, matrix, full)])
    want = np.concatenate([p.reshape(-1) for p in quantise(split_unrounded(unr, src), bits)])
    d = np.abs(np.asarray(got).astype(np.int64) - want.astype(np.int64))
    near = np.abs(unr - np.floor(unr) - 0.5) <= TIE_WINDOW_STEPS
    return int(d.max()), int((d != 0).sum()), int(((d != 0) & ~near).sum()), float(near.mean())


def split_unrounded(unr, src):
    return split(unr, src)


def y4m_bytes(frames, header):
    import io
    buf = io.BytesIO()
    w = y4m.Writer(buf, header)
    for f in frames:
        w.write_frame(f)
    return buf.getvalue()


def clip_from_bgr(frames, bits, matrix="bt709", full=False):
    """HWC BGR frames (uint8, or uint16 with samples in [0, 65535]) -> YuvFrames through the restatement's way out"""
    out = []
    for f in frames:
        peak = 255.0 if f.dtype == np.uint8 else 65535.0
        x = torch.from_numpy(np.ascontiguousarray(f).astype(np.float32).transpose(2, 0, 1).copy()).unsqueeze(0) / peak
        out.append(frame_of(to_out_ref(x, f.shape[:2], bits, matrix, full), f.shape[:2], bits))
    return out
