"""GPU: fit = pad -- the eight pad / crop entries of frame_io.hip against the PARENT kernels (the existing conversions at an unchanged
size, replicate-padded or fed the cropped window: padding adds no arithmetic, so the comparison is bit for bit), both kernel forms
read from the launch trace, the exact round trip, the argument checks, copied frames coming back as the source's bytes, whole clips
against the CPU oracle driver with the CPU pad hooks of tests/fit_pad_common.py, and the command lines."""
import ctypes as C
import io
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from drba_amd import _lib, ops, y4m
from drba_amd.models.utils import tools
from drba_amd.utils import synth
from tests import fit_pad_common as fpc
from tests import yuv_common as yc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _traced(fn):
    ops.trace_begin()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        recs = ops.trace_end()
    return out, [r["name"] for r in recs]


def _forms(names, direction):
    """the forms of the pad / crop launches of one direction; a resize kernel in their place fails the comparison"""
    mark = "pad" if direction == "to_inp" else "crop"
    return [("rows" if "rows" in n else "general") if mark in n else "resize:" + n for n in names if direction in n]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _replicate(x, net):
    """the yardstick of the way in: the parent's unresized conversion, its last row and column repeated"""
    h, w = x.shape[2:]
    return F.pad(x.cpu(), (0, net[1] - w, 0, net[0] - h), mode="replicate")


# (src size, net size, the kernel form both directions must take)
GEOMETRIES = [((45, 71), (64, 128), "general"), ((60, 64), (64, 64), "rows"), ((60, 66), (64, 66), "general"), ((64, 64), (64, 64), "rows")]
GIDS = [f"{g[0][0]}x{g[0][1]}" for g in GEOMETRIES]
PACKED = [(np.uint8, None), (np.uint16, 1023), (np.uint16, 65535)]
PIDS = ["u8", "u16-1023", "u16-65535"]
ALL = list(itertools.product((8, 10), (False, True), ("bt709", "bt601")))
YUV_CASES = [(GEOMETRIES[0], b, f, m) for b, f, m in ALL] + [(g, b, False, "bt709") for g in GEOMETRIES[1:] for b in (8, 10)]
YUV_IDS = [f"{g[0][0]}x{g[0][1]}-{b}bit-{'full' if f else 'limited'}-{m}" for g, b, f, m in YUV_CASES]


def _packed_frame(src, dtype, maxval, seed):
    peak = 255 if maxval is None else maxval
    f = np.random.default_rng(seed).integers(0, peak + 1, size=(src[0], src[1], 3)).astype(dtype)
    f[0, 0], f[-1, -1], f[0, -1], f[-1, 0] = (0, peak, peak // 2), (peak, 0, 1), (peak, peak, peak), (0, 0, 0)
    return f


def _depth_kw(bits):
    return {"depth": 8} if bits == 8 else {"depth": 16, "maxval": 1023}


def _out_kw(maxval):
    return {} if maxval is None else {"depth": 16, "maxval": maxval}


# ------------------------------------------------------------------------------------------------------------------------ way in
@pytest.mark.parametrize("dtype,maxval", PACKED, ids=PIDS)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GIDS)
def test_to_inp_pad_is_the_parents_conversion_replicate_padded(dev, geometry, dtype, maxval):
    src, net, form = geometry
    f = _packed_frame(src, dtype, maxval, seed=src[1])
    t = torch.from_numpy(f).to(dev)
    got, names = _traced(lambda: ops.to_inp(t, net, maxval=maxval, fit="pad"))
    assert _forms(names, "to_inp") == [form] and all(("16" in n) == (maxval is not None) for n in names if "to_inp" in n), names
    want = _replicate(ops.to_inp(t, src, maxval=maxval), net)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, net[0], net[1])
    assert _same_bits(got.cpu(), want), float((got.cpu() - want).abs().max())
    x4 = ops._x4_of(got)
    assert x4 is not None and tuple(x4.shape) == (net[0], net[1], 4)
    assert _same_bits(x4[:, :, :3].cpu(), got[0].permute(1, 2, 0).cpu()) and not bool(x4[:, :, 3].any())
    assert torch.equal(tools.to_inp(f, net, maxval=maxval, fit="pad"), got)  # the host-frame entry
    ref = fpc.to_inp8(f, net) if maxval is None else fpc.to_inp16(f, net, maxval)
    assert torch.equal(got.cpu(), ref)  # ... and the CPU restatement the whole-clip hooks are built on


@pytest.mark.parametrize("geometry,bits,full,matrix", YUV_CASES, ids=YUV_IDS)
def test_to_inp_yuv_pad_is_the_parents_conversion_replicate_padded(dev, geometry, bits, full, matrix):
    src, net, form = geometry
    f = yc.random_frame(src[0], src[1], bits, seed=src[1] + bits)
    planes = torch.from_numpy(f.data).to(dev)
    mv = None if bits == 8 else 1023
    got, names = _traced(lambda: ops.to_inp_yuv(planes, src, net, matrix=matrix, full_range=full, maxval=mv, fit="pad"))
    assert _forms(names, "to_inp") == [form] and all(("16" in n) == (bits == 10) for n in names if "to_inp" in n), names
    want = _replicate(ops.to_inp_yuv(planes, src, src, matrix=matrix, full_range=full, maxval=mv), net)
    assert _same_bits(got.cpu(), want), float((got.cpu() - want).abs().max())
    x4 = ops._x4_of(got)
    assert x4 is not None and tuple(x4.shape) == (net[0], net[1], 4)
    assert _same_bits(x4[:, :, :3].cpu(), got[0].permute(1, 2, 0).cpu()) and not bool(x4[:, :, 3].any())
    err = float((got.cpu().double() - fpc.to_inp_yuv(f, net, bits, matrix, full)).abs().max())
    print(f"to_inp_yuv pad {src}->{net} {bits} bit {'full' if full else 'limited'} {matrix} [{form}]: max |d| = {err:.3e} (bar {yc.TO_INP_TOL:.0e})")
    assert err <= yc.TO_INP_TOL, err
    assert torch.equal(tools.to_inp(f, net, matrix=matrix, full_range=full, fit="pad"), got)


# ----------------------------------------------------------------------------------------------------------------------- way out
def _spoil_margin(x, src):
    y = x.clone()
    y[:, :, src[0]:, :], y[:, :, :, src[1]:] = 0.9, float("nan")
    return y


@pytest.mark.parametrize("maxval", [1023, 65535])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GIDS)
def test_to_out16_crop_is_the_parents_conversion_of_the_window(dev, geometry, maxval):
    """planted NaN, +-inf, -0.5 and 1.5: NaN -> 0, -0.5 -> 0, 1.5 -> maxval, and an infinity -> 0 as in the parent's unresized form
    (ATen's copy of an unchanged axis makes it NaN)."""
    src, net, form = geometry
    x = yc.planted_net_frame(net, seed=7)
    for rev in (False, True):
        got, names = _traced(lambda: ops.to_out(x.to(dev), src, rgb=rev, depth=16, maxval=maxval, fit="pad"))
        assert _forms(names, "to_out") == [form] and all("16" in n for n in names if "to_out" in n), names
        want = ops.to_out(x[:, :, :src[0], :src[1]].contiguous().to(dev), src, rgb=rev, depth=16, maxval=maxval)
        assert got.dtype == torch.uint16 and tuple(got.shape) == (src[0], src[1], 3)
        g = got.cpu().numpy()
        assert np.array_equal(g, want.cpu().numpy())
        assert np.array_equal(g, fpc.to_out16(x, src, maxval, rgb=rev))
        assert g[25, 45].tolist() == [0, 0, 0] and g[3, 7, 1] == 0           # NaN, -0.5, NaN; a single NaN
        assert g[42, 45].tolist() == [0, maxval, 0] and g[0, 0, 0 if rev else 2] == maxval  # inf, 1.5, inf; a single 1.5
        assert np.array_equal(ops.to_out(_spoil_margin(x, src).to(dev), src, rgb=rev, depth=16, maxval=maxval, fit="pad").cpu().numpy(), g)
    assert np.array_equal(tools.to_out(x.to(dev), src, depth=16, maxval=maxval, fit="pad"), ops.to_out(x.to(dev), src, depth=16, maxval=maxval, fit="pad").cpu().numpy())


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GIDS)
def test_to_out_crop_is_the_parents_conversion_of_the_window_and_reads_the_pixel_alone(dev, geometry):
    src, net, form = geometry
    g_ = torch.Generator().manual_seed(src[1])
    x = torch.rand(1, 3, net[0], net[1], generator=g_) * 1.02 - 0.01
    assert bool(torch.isfinite(x).all()) and float(x.min()) < 0.0 and float(x.max()) > 1.0
    win = x[:, :, :src[0], :src[1]].contiguous()
    for rev in (False, True):
        got, names = _traced(lambda: ops.to_out(x.to(dev), src, rgb=rev, fit="pad"))
        assert _forms(names, "to_out") == [form] and not [n for n in names if "16" in n], names
        assert got.dtype == torch.uint8 and tuple(got.shape) == (src[0], src[1], 3)
        g = got.cpu().numpy()
        assert np.array_equal(g, ops.to_out(win.to(dev), src, rgb=rev).cpu().numpy())
        assert np.array_equal(ops.to_out(_spoil_margin(x, src).to(dev), src, rgb=rev, fit="pad").cpu().numpy(), g)
    assert np.array_equal(tools.to_out(x.to(dev), src, fit="pad"), ops.to_out(x.to(dev), src, fit="pad").cpu().numpy())
    # a planted pair: the pixel (5, 10) is 0.5, its right and lower neighbours are +inf.  The parent's unresized form weighs the
    # neighbour with 0 (0 * inf = NaN reaches the pixel); the crop reads the pixel alone
    y = x.clone()
    y[0, :, 5, 10], y[0, :, 5, 11], y[0, :, 6, 10] = 0.5, float("inf"), float("inf")
    got = ops.to_out(y.to(dev), src, fit="pad").cpu().numpy()
    assert got[5, 10].tolist() == [127, 127, 127]
    parent = ops.to_out(y[:, :, :src[0], :src[1]].contiguous().to(dev), src).cpu().numpy()
    assert parent[5, 10].tolist() != [127, 127, 127]
    keep = np.ones(src, bool)
    keep[4:7, 9:12] = False
    assert np.array_equal(got[keep], parent[keep])


@pytest.mark.parametrize("geometry,bits,full,matrix", YUV_CASES, ids=YUV_IDS)
def test_to_out_yuv_crop_is_the_parents_conversion_of_the_window(dev, geometry, bits, full, matrix):
    src, net, form = geometry
    x = yc.planted_net_frame(net, seed=7)
    kw = dict(matrix=matrix, full_range=full, **_depth_kw(bits))
    got, names = _traced(lambda: ops.to_out_yuv(x.to(dev), src, fit="pad", **kw))
    assert _forms(names, "to_out") == [form] and all(("16" in n) == (bits == 10) for n in names if "to_out" in n), names
    (h, w), (hc, wc) = y4m.plane_sizes(*src)
    assert got.dim() == 1 and got.numel() == h * w + 2 * hc * wc and got.dtype == (torch.uint8 if bits == 8 else torch.uint16)
    g = got.cpu().numpy()
    assert np.array_equal(g, ops.to_out_yuv(x[:, :, :h, :w].contiguous().to(dev), src, **kw).cpu().numpy())
    yp, up, vp = yc.split(g, src)
    assert (int(yp[25, 45]), int(up[12, 22]), int(vp[12, 22])) == yc.planted_codes(bits, full)["black"]  # NaN and -0.5 -> the code of 0
    assert int(g.max()) <= (1 << bits) - 1
    # the margin is never read: not by the luma, and not by the chroma mean at an odd edge (45 and 71 are odd)
    assert np.array_equal(ops.to_out_yuv(_spoil_margin(x, src).to(dev), src, fit="pad", **kw).cpu().numpy(), g)
    assert np.array_equal(tools.to_out(x.to(dev), src, pixfmt="yuv420", matrix=matrix, full_range=full, depth=8 if bits == 8 else 16,
                                       maxval=None if bits == 8 else 1023, fit="pad"), g)


# -------------------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GIDS)
def test_round_trip_gives_the_frame_back_byte_for_byte(dev, geometry):
    src, net, _ = geometry
    f = fpc.all_codes_frame(*src, seed=5)
    for rev in (False, True):
        back = ops.to_out(ops.to_inp(torch.from_numpy(f).to(dev), net, fit="pad"), src, rgb=rev, fit="pad").cpu().numpy()
        assert np.array_equal(back, f[:, :, ::-1] if rev else f)
    for maxval in (1023, 65535):
        f16 = _packed_frame(src, np.uint16, maxval, seed=maxval)
        x = ops.to_inp(torch.from_numpy(f16).to(dev), net, maxval=maxval, fit="pad")
        assert np.array_equal(ops.to_out(x, src, depth=16, maxval=maxval, fit="pad").cpu().numpy(), f16)
    for bits, full, matrix in ALL:
        mv = None if bits == 8 else 1023

        def trip(fr):
            x = ops.to_inp_yuv(torch.from_numpy(fr.data).to(dev), src, net, matrix=matrix, full_range=full, maxval=mv, fit="pad")
            return yc.split(ops.to_out_yuv(x, src, matrix=matrix, full_range=full, fit="pad", **_depth_kw(bits)).cpu().numpy(), src)

        fr = yc.in_gamut_frame(*src, bits, seed=bits)
        assert np.array_equal(trip(fr)[0], fr.planes()[0])
        fr = yc.in_gamut_frame(*src, bits, seed=3, flat_chroma=True)
        assert all(np.array_equal(a, b) for a, b in zip(trip(fr), fr.planes()))


# --------------------------------------------------------------------------------------------------------------- argument checks
def test_entry_points_validate_their_arguments(dev):
    lib = _lib.load()
    H, W, Hc, Wc, Ho, Wo = 16, 24, 8, 12, 32, 32
    st = ops._stream()
    img8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    img16 = torch.zeros(H * W * 3 + 8, dtype=torch.uint16, device=dev)
    p8 = torch.zeros(H * W + 2 * Hc * Wc, dtype=torch.uint8, device=dev)
    p16 = torch.zeros(H * W + 2 * Hc * Wc + 8, dtype=torch.uint16, device=dev)
    net = torch.zeros((1, 3, Ho, Wo), dtype=torch.float32, device=dev)
    x4 = torch.zeros(Ho * Wo * 4 + 4, dtype=torch.float32, device=dev)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None  # noqa: E731

    def planes(t, off=0):
        es, b = t.element_size(), t.data_ptr() + off
        return [C.c_void_p(b), C.c_void_p(b + H * W * es), C.c_void_p(b + (H * W + Hc * Wc) * es)]

    def inp8(img=img8, out=net, o4=None, size=(H, W, Ho, Wo)):
        return lib.drba_to_inp_pad_x4(P(img), P(out), o4, *size, st)

    def inp16(img=P(img16), out=net, o4=None, size=(H, W, Ho, Wo), maxval=1023.0):
        return lib.drba_to_inp16_pad_x4(img, P(out), o4, *size, maxval, st)

    def out8(src=net, dst=img8, size=(Ho, Wo, H, W)):
        return lib.drba_to_out_crop(P(src), P(dst), *size, 0, st)

    def out16(src=net, dst=P(img16), size=(Ho, Wo, H, W), maxval=1023.0):
        return lib.drba_to_out16_crop(P(src), dst, *size, 0, maxval, st)

    def yinp8(pl=None, out=net, o4=None, size=(H, W, Ho, Wo), matrix=0, strides=(W, Wc)):
        return lib.drba_to_inp_yuv420_pad_x4(*(planes(p8) if pl is None else pl), *strides, P(out), o4, *size, matrix, 0, st)

    def yinp16(pl=None, out=net, o4=None, size=(H, W, Ho, Wo), matrix=0, maxval=1023.0):
        return lib.drba_to_inp16_yuv420_pad_x4(*(planes(p16) if pl is None else pl), W, Wc, P(out), o4, *size, matrix, 0, maxval, st)

    def yout8(pl=None, src=net, size=(Ho, Wo, H, W), matrix=0, strides=(W, Wc)):
        return lib.drba_to_out_yuv420_crop(P(src), *(planes(p8) if pl is None else pl), *strides, *size, matrix, 0, st)

    def yout16(pl=None, src=net, size=(Ho, Wo, H, W), matrix=0, maxval=1023.0):
        return lib.drba_to_out16_yuv420_crop(P(src), *(planes(p16) if pl is None else pl), W, Wc, *size, matrix, 0, maxval, st)

    ways_in, ways_out = (inp8, inp16, yinp8, yinp16), (out8, out16, yout8, yout16)
    assert all(f() == 0 for f in ways_in + ways_out)
    assert all(f(o4=P(x4)) == 0 for f in ways_in)
    # null pointers
    assert inp8(img=None) == -1 and inp16(img=None) == -1 and out8(dst=None) == -1 and out16(dst=None) == -1
    assert all(f(out=None) == -1 for f in ways_in) and all(f(src=None) == -1 for f in ways_out)
    for k in range(3):
        for t, fi, fo in ((p8, yinp8, yout8), (p16, yinp16, yout16)):
            pl = planes(t)
            pl[k] = None
            assert fi(pl=pl) == -1 and fo(pl=pl) == -1
    # a destination smaller than the source on the way in, a frame larger than the tensor on the way out, a zero size
    for size in ((H, W, H - 1, Wo), (H, W, Ho, W - 1), (0, W, Ho, Wo), (H, 0, Ho, Wo)):
        assert all(f(size=size) == -1 for f in ways_in), size
    for size in ((H - 1, Wo, H, W), (Ho, W - 1, H, W), (Ho, Wo, 0, W), (Ho, Wo, H, 0)):
        assert all(f(size=size) == -1 for f in ways_out), size
    assert all(f(size=(H, W, H, W)) == 0 for f in ways_in) and all(f(size=(H, W, H, W)) == 0 for f in ways_out)  # nothing to pad
    # a misaligned out_x4, a bad maxval, a misaligned 16-bit pointer, a short stride, an unknown matrix
    assert all(f(o4=P(x4, 4)) == -1 for f in ways_in)
    for maxval in (255.0, 70000.0, float("nan")):
        assert inp16(maxval=maxval) == -1 and out16(maxval=maxval) == -1 and yinp16(maxval=maxval) == -1 and yout16(maxval=maxval) == -1
    assert inp16(img=P(img16, 1)) == -1 and out16(dst=P(img16, 1)) == -1
    assert yinp16(pl=planes(p16, off=1)) == -1 and yout16(pl=planes(p16, off=1)) == -1
    assert yinp8(strides=(W - 1, Wc)) == -1 and yout8(strides=(W, Wc - 1)) == -1
    for matrix in (2, -1):
        assert yinp8(matrix=matrix) == -1 and yout8(matrix=matrix) == -1 and yinp16(matrix=matrix) == -1 and yout16(matrix=matrix) == -1
    torch.cuda.synchronize()
    # the Python surface
    f = np.zeros((H, W, 3), np.uint8)
    pk = torch.zeros(H * W + 2 * Hc * Wc, dtype=torch.uint8, device=dev)
    for call in (lambda fit: ops.to_inp(img8, (Ho, Wo), fit=fit), lambda fit: ops.to_out(net, (H, W), fit=fit),
                 lambda fit: ops.to_inp_yuv(pk, (H, W), (Ho, Wo), fit=fit), lambda fit: ops.to_out_yuv(net, (H, W), fit=fit),
                 lambda fit: tools.to_inp(f, (Ho, Wo), fit=fit), lambda fit: tools.to_out(net, (H, W), fit=fit)):
        with pytest.raises(ValueError, match="fit"):
            call("stretch")
    for call in (lambda: ops.to_inp(img8, (H - 1, Wo), fit="pad"), lambda: ops.to_out(net, (Ho + 1, W), fit="pad"),
                 lambda: ops.to_inp_yuv(pk, (H, W), (Ho, W - 2), fit="pad"), lambda: ops.to_out_yuv(net, (H, Wo + 2), fit="pad")):
        with pytest.raises(ValueError, match="pad"):
            call()


# --------------------------------------------------------------------------------------------------- what the mode is for: copies
class _Copy:  # repeats the nearer frame: with a cut between every pair the driver copies, and the tail copies through this
    scale, pad_size, supports_lookahead = 1.0, 64, False

    def inference_ts(self, I0, I1, ts):
        return [I0 if t < 0.5 else I1 for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False):
        raise AssertionError("a DRBA step ran although every pair is a scene cut")


def test_copied_frames_are_the_sources_bytes(dev):
    """5 frames of 45 x 71 (network size 64 x 128), a cut between every pair: every written frame is a copy.  With the pad hooks it is
    one of the source frames byte for byte; with the default (resize) hooks it is not."""
    from drba_amd import infer as drv
    from tests.clip_common import ListIO
    frames = [fpc.all_codes_frame(45, 71, seed=k) for k in range(5)]

    def run(**hooks):
        io_ = ListIO(frames, 24.0)
        n = drv.interpolate_stream(_Copy(), io_, 48.0, times=2, enable_scdet=True, check_scene=lambda *a: True, **hooks)
        assert n == len(io_.written) == 10
        return io_.written

    pad = run(to_inp=lambda fr, size: tools.to_inp(fr, size, fit="pad"), to_out=lambda x, size: tools.to_out(x, size, fit="pad"))
    assert all(any(np.array_equal(w, f) for f in frames) for w in pad)
    assert [next(k for k, f in enumerate(frames) if np.array_equal(w, f)) for w in pad] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    resized = run()
    assert not any(any(np.array_equal(w, f) for f in frames) for w in resized)


# -------------------------------------------------------------------------------------------------------------------- whole clip
SRC, NET = (120, 180), (128, 192)  # the network size is the smallest the whole-clip tests use; the source leaves both margins


def _rife(dev):
    from drba_amd.models.rife import RIFE
    return RIFE(weights=synth.ifnet_state_dict(seed=0), scale=1.0, device=dev)


def test_whole_clip_packed_against_the_cpu_oracle_driver(dev):
    """RIFE on synthetic weights, 6 frames of 120 x 180 (network size 128 x 192), -t 2, pad hooks at both ends, against the CPU oracle
    driver with the CPU pad hooks.  The bar is the one of the resize-mode clip tests (tests/test_gpu_cli.py): never more than 1 LSB,
    fewer than 2e-3 of the bytes differing."""
    import oracle
    from drba_amd import infer as drv
    from tests.clip_common import ListIO
    frames = [np.ascontiguousarray(f[:SRC[0], :SRC[1]]) for f in synth.make_clip(6, NET[0], NET[1], seed=1234)]
    io_ = ListIO(frames, 24.0)
    n = drv.interpolate_stream(_rife(dev), io_, 48.0, times=2, to_inp=lambda fr, size: tools.to_inp(fr, size, fit="pad"),
                               to_out=lambda x, size: tools.to_out(x, size, fit="pad"))
    ref_io = ListIO(frames, 24.0)
    to_inp, to_out, check = fpc.cpu_hooks8()
    drv.interpolate_stream(oracle.rife.RifeOracle(synth.ifnet_state_dict(seed=0), 1.0), ref_io, 48.0, times=2, to_inp=to_inp, to_out=to_out,
                           check_scene=check)
    got, want = np.stack(io_.written), np.stack(ref_io.written)
    assert n == 12 and got.shape == want.shape == (12, SRC[0], SRC[1], 3) and got.dtype == np.uint8
    assert np.array_equal(got[0], frames[0]) and np.array_equal(got[-1], frames[-1])  # the head and tail copies: the source's bytes
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print(f"whole clip, packed 8 bit, pad: max |d| = {int(d.max())} LSB (bar 1), differing bytes {float((d > 0).mean()):.2e} (bar 2e-3)")
    assert d.max() <= 1, f"max diff {d.max()} LSB"
    assert (d > 0).mean() < 2e-3, f"{(d > 0).mean():.2e} of the bytes differ"


@pytest.mark.parametrize("bits", [8, 10])
def test_whole_clip_y4m_against_the_cpu_oracle_driver(dev, bits):
    """The same clip as planar 4:2:0 at 8 and 10 bits, pad hooks, against the CPU oracle driver with the fp64 pad hooks: the bar of the
    resize-mode test (tests/test_gpu_yuv.py), yc.CLIP_TOL_STEPS."""
    import oracle
    from drba_amd import infer as drv
    from tests.clip_common import ListIO
    clip = synth.make_clip(6, NET[0], NET[1], seed=1234) if bits == 8 else synth.make_clip16(6, NET[0], NET[1], seed=1234)
    frames = yc.clip_from_bgr([np.ascontiguousarray(f[:SRC[0], :SRC[1]]) for f in clip], bits)
    mv = None if bits == 8 else 1023
    io_ = ListIO(frames, 24.0)
    n = drv.interpolate_stream(_rife(dev), io_, 48.0, times=2, to_inp=lambda fr, size: tools.to_inp(fr, size, fit="pad"),
                               to_out=lambda x, size: tools.to_out(x, size, pixfmt="yuv420", depth=8 if bits == 8 else 16, maxval=mv,
                                                                   fit="pad"))
    ref_io = ListIO(frames, 24.0)
    to_inp, to_out, check = fpc.cpu_hooks_yuv(bits, bits)
    drv.interpolate_stream(oracle.rife.RifeOracle(synth.ifnet_state_dict(seed=0), 1.0), ref_io, 48.0, times=2, to_inp=to_inp, to_out=to_out,
                           check_scene=check)
    got, want = np.stack(io_.written), np.stack(ref_io.written)
    assert n == 12 and got.shape == want.shape == (12, SRC[0] * SRC[1] * 3 // 2) and got.dtype == want.dtype
    assert np.array_equal(yc.split(got[0], SRC)[0], frames[0].planes()[0])  # the head copy's luma (in gamut: the clip came from RGB)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(f"whole clip {bits} bit, pad: max |d| = {int(d.max())} step (bar {yc.CLIP_TOL_STEPS}), differing samples {float((d != 0).mean()):.4%}")
    assert int(d.max()) <= yc.CLIP_TOL_STEPS, int(d.max())


# ----------------------------------------------------------------------------------------------------------------- command lines
def test_command_lines_with_fit(dev, tmp_path):
    """One child process: infer.py --fit pad on an 8-bit .npz clip, a 16-bit one and a Y4M stream, `evaluate holdout --fit pad`, and
    --fit resize against no flag under --deterministic (the same bytes).  7 frames of 120 x 180, -t 2."""
    wdir = tmp_path / "w"
    wdir.mkdir()
    torch.save({"module." + k: v for k, v in synth.ifnet_state_dict(0).items()}, str(wdir / "flownet.pkl"))
    bgr = [np.ascontiguousarray(f[:SRC[0], :SRC[1]]) for f in synth.make_clip(7, NET[0], NET[1], seed=21)]
    b16 = [np.ascontiguousarray(f[:SRC[0], :SRC[1]]) for f in synth.make_clip16(4, NET[0], NET[1], seed=9)]
    f8 = yc.clip_from_bgr(bgr[:4], 8)
    hdr = y4m.Header(SRC[1], SRC[0], (24, 1), interlace="p", chroma="420jpeg")
    pz, pz16, py = str(tmp_path / "clip.npz"), str(tmp_path / "clip16.npz"), str(tmp_path / "clip.y4m")
    np.savez(pz, frames=np.stack(bgr), fps=np.float64(24.0))
    np.savez(pz16, frames=np.stack(b16), fps=np.float64(24.0))
    open(py, "wb").write(yc.y4m_bytes(f8, hdr))
    outs = {k: str(tmp_path / k) for k in ("out.npz", "out16.npz", "out.y4m", "det_flag.npz", "det_plain.npz")}
    jobs = [(pz, outs["out.npz"], ["--fit", "pad"]), (pz16, outs["out16.npz"], ["--fit", "pad"]), (py, outs["out.y4m"], ["--fit", "pad"]),
            (pz, outs["det_flag.npz"], ["--fit", "resize", "--deterministic"]), (pz, outs["det_plain.npz"], ["--deterministic"])]
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import drba_amd.infer as I\n"
        "from drba_amd import evaluate\n"
        "for inp, out, extra in %r:\n"
        "    a = I.parse_args(['-m', 'rife', '-i', inp, '-o', out, '-t', '2'] + extra)\n"
        "    I.apply_deterministic(a)  # before the model is built, as main() does\n"
        "    print('written', I.inference(I.load_model('rife', 1.0, weights=%r), a), file=sys.stderr)\n"
        "sys.exit(evaluate.main(['holdout', '-m', 'rife', '-i', %r, '--weights', %r, '--fit', 'pad']))\n"
        % (ROOT, jobs, str(wdir), pz, str(wdir)))
    env = dict(os.environ, DRBA_TUNE_CACHE="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [ln for ln in r.stderr.decode().splitlines() if ln.startswith("written")] == ["written 14", "written 8", "written 8", "written 14",
                                                                                         "written 14"]
    z = np.load(outs["out.npz"])
    assert z["frames"].shape == (14, SRC[0], SRC[1], 3) and z["frames"].dtype == np.uint8 and float(z["fps"]) == 48.0
    assert np.array_equal(z["frames"][0], bgr[0]) and np.array_equal(z["frames"][-1], bgr[-1])  # the copies: the source's bytes
    z = np.load(outs["out16.npz"])
    assert z["frames"].shape == (8, SRC[0], SRC[1], 3) and z["frames"].dtype == np.uint16
    assert np.array_equal(z["frames"][0], b16[0]) and np.array_equal(z["frames"][-1], b16[-1])
    rd = y4m.Reader(io.BytesIO(open(outs["out.y4m"], "rb").read()))
    fr = list(rd)
    assert (rd.header.height, rd.header.width) == SRC and len(fr) == 8 and fr[0].depth == 8
    assert np.array_equal(fr[0].planes()[0], f8[0].planes()[0])
    rep = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert rep["command"] == "holdout" and rep["fit"] == "pad" and rep["kept"]["max_lsb"] == 0 and rep["kept"]["frames"] == 3
    a, b = np.load(outs["det_flag.npz"])["frames"], np.load(outs["det_plain.npz"])["frames"]
    assert a.shape == (14, SRC[0], SRC[1], 3) and np.array_equal(a, b)
    assert not np.array_equal(a[0], bgr[0])  # ... and resize mode does not give the copied frame back
