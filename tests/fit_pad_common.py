"""Shared pieces of the fit = pad tests (tests/test_fit_pad_cpu.py, tests/test_gpu_fit_pad.py): the CPU restatement of the mode
and whole-clip hooks built on it.

    to_inp = edge_pad(to_unit(frame), dst)        bottom and right, np.pad(..., mode="edge"); no interpolation
    to_out = quantise(x[:, :, :h, :w])            the top-left `src` window as it stands

with the unit conversions and quantisers the resize-mode restatements use: / 255. and trunc(x * 255.) for bytes
(tests/clip_common.py), / maxval and round-half-even with saturation for 16-bit samples (tests/depth16_common.py), the fp64 colour
code of tests/yuv_common.py for planar 4:2:0.  The 16-bit and planar ways out go through those restatements at the window's own
size, where nothing is resampled and ATen's copy of an unchanged axis makes a non-finite sample NaN -> 0.
"""
import numpy as np
import torch

from tests import depth16_common as d16
from tests import yuv_common as yc


def _margins(src, dst):
    (h, w), (ho, wo) = src, dst
    assert ho >= h and wo >= w, (src, dst)
    return ho - h, wo - w


def pad_planes(x, dst):
    """[..., H, W] (numpy or torch) -> [..., *dst], the last row and column repeated"""
    t = torch.is_tensor(x)
    a = x.numpy() if t else np.asarray(x)
    dh, dw = _margins(a.shape[-2:], dst)
    out = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(0, dh), (0, dw)], mode="edge")
    return torch.from_numpy(out) if t else out


def crop(x, src):
    assert x.shape[2] >= src[0] and x.shape[3] >= src[1], (tuple(x.shape), src)
    return x[:, :, :src[0], :src[1]].contiguous()


# ----------------------------------------------------------------------------------------------------------------- packed frames
def to_inp8(frame, dst):
    """uint8 [H,W,3] -> fp32 [1,3,*dst]"""
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(frame)).transpose(2, 0, 1).copy()).unsqueeze(0).float() / 255.0
    return pad_planes(x, dst)


def to_out8(x, src, rgb=False):
    """fp32 [1,3,h,w] -> uint8 [*src,3], the reference's truncation"""
    out = (crop(x, src)[0].numpy().transpose(1, 2, 0) * 255.0).astype(np.uint8)
    return np.ascontiguousarray(out[:, :, ::-1]) if rgb else out


def to_inp16(frame, dst, maxval=65535):
    return pad_planes(d16.planar16(frame, maxval), dst)


def to_out16(x, src, maxval=65535, rgb=False):
    """the 16-bit restatement of the window at its own size: no resampling happens there, and ATen's copy of an unchanged axis
    turns a non-finite sample into NaN -> 0, which is the rule the device's unresized conversion has"""
    return d16.to_out16_ref(crop(x, src), src, maxval, rev=rgb)


# ----------------------------------------------------------------------------------------------------------------- planar 4:2:0
def to_inp_yuv(frame, dst, bits, matrix="bt709", full=False):
    """YuvFrame -> fp64 [1,3,*dst]: yc.to_inp_ref at the frame's own size (no resize happens there), edge-padded in fp64"""
    return pad_planes(yc.to_inp_ref(frame, frame.shape[:2], bits, matrix, full), dst)


def to_out_yuv(x, src, bits, matrix="bt709", full=False):
    """-> 1-D packed Y, U, V: yc.to_out_ref of the window (the chroma mean sees the window alone)"""
    return yc.to_out_ref(crop(x, src), src, bits, matrix, full)


# ------------------------------------------------------------------------------------------------------------------- clip hooks
def cpu_hooks8():
    import oracle
    return to_inp8, to_out8, oracle.scdet.check_scene


def cpu_hooks16(maxval=65535):
    import oracle
    return (lambda fr, size: to_inp16(fr, size, maxval)), (lambda x, size: to_out16(x, size, maxval)), oracle.scdet.check_scene


def cpu_hooks_yuv(bits_in, bits_out, matrix="bt709", full=False):
    import oracle
    return ((lambda fr, size: to_inp_yuv(fr, size, bits_in, matrix, full).float()),
            (lambda x, size: to_out_yuv(x, size, bits_out, matrix, full)), oracle.scdet.check_scene)


def all_codes_frame(h, w, seed):
    """random uint8 [h,w,3] with every code 0 .. 255 planted in each channel"""
    assert h * w >= 256
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    for c in range(3):
        f.reshape(-1, 3)[rng.permutation(h * w)[:256], c] = np.arange(256, dtype=np.uint8)
    return f
