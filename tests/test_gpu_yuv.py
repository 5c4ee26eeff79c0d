"""GPU: planar YCbCr 4:2:0 frames -- the conversion kernels (frame_io.hip: drba_to_inp_yuv420_x4, drba_to_out_yuv420 and their
16-bit siblings) against the fp64 restatement of tests/yuv_common.py in both kernel forms (the form a call took is read from the
launch trace), the round-trip properties on the device, the argument checks of the four entries, a whole Y4M clip through
interpolate_stream against the CPU oracle driver, and the command lines."""
import ctypes as C
import io
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from drba_amd import _lib, ops, y4m
from drba_amd.models.utils import tools
from drba_amd.utils import synth
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
    return [("rows" if "rows" in n else "general") for n in names if "yuv" in n and direction in n]


# (src size, net size, the kernel form both directions must take)
GEOMETRIES = [((45, 71), (64, 128), "general"), ((60, 64), (64, 64), "rows"), ((60, 66), (64, 66), "general"), ((64, 64), (64, 64), "rows")]
ALL = list(itertools.product((8, 10), (False, True), ("bt709", "bt601")))
CASES = [(GEOMETRIES[0], b, f, m) for b, f, m in ALL] + [(g, b, False, "bt709") for g in GEOMETRIES[1:] for b in (8, 10)]
IDS = [f"{g[0][0]}x{g[0][1]}-{b}bit-{'full' if f else 'limited'}-{m}" for g, b, f, m in CASES]


def _depth_kw(bits):
    return {"depth": 8} if bits == 8 else {"depth": 16, "maxval": 1023}


@pytest.mark.parametrize("geometry,bits,full,matrix", CASES, ids=IDS)
def test_to_inp_yuv_against_the_restatement(dev, geometry, bits, full, matrix):
    """Every fp32 value within 2e-6 of the fp64 restatement (the extremes 0 and m planted at the corners of all three planes), the
    [H,W,4] copy equal to the planar result bit for bit with a zero fourth lane, the form read from the launch trace."""
    src, net, form = geometry
    f = yc.random_frame(src[0], src[1], bits, seed=src[1] + bits)
    want = yc.to_inp_ref(f, net, bits, matrix, full)
    planes = torch.from_numpy(f.data).to(dev)
    got, names = _traced(lambda: ops.to_inp_yuv(planes, src, net, matrix=matrix, full_range=full, maxval=None if bits == 8 else 1023))
    assert _forms(names, "to_inp") == [form] and all(("16" in n) == (bits == 10) for n in names if "yuv" in n), names
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, net[0], net[1])
    err = float((got.cpu().double() - want).abs().max())
    print(f"to_inp_yuv {src}->{net} {bits} bit {'full' if full else 'limited'} {matrix} [{form}]: max |d| = {err:.3e} (bar {yc.TO_INP_TOL:.0e})")
    assert err <= yc.TO_INP_TOL, err
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    x4 = ops._x4_of(got)
    assert x4 is not None and tuple(x4.shape) == (net[0], net[1], 4)
    assert torch.equal(x4[:, :, :3], got[0].permute(1, 2, 0)) and not bool(x4[:, :, 3].any())
    assert torch.equal(tools.to_inp(f, net, matrix=matrix, full_range=full), got)  # the host-frame entry


@pytest.mark.parametrize("geometry,bits,full,matrix", CASES, ids=IDS)
def test_to_out_yuv_against_the_restatement(dev, geometry, bits, full, matrix):
    """A frame uniform in [-0.01, 1.01] with blocks and single samples of NaN, +inf, -0.5 and 1.5: every sample equal to the
    restatement's except where the fp64 unrounded value lies within 2e-3 steps of a half-integer (one step allowed there), never
    more than one step, at most 1 % of the samples inside that window; inside the planted blocks the rule itself."""
    src, net, form = geometry
    x = yc.planted_net_frame(net, seed=7)
    got, names = _traced(lambda: ops.to_out_yuv(x.to(dev), src, matrix=matrix, full_range=full, **_depth_kw(bits)))
    assert _forms(names, "to_out") == [form] and all(("16" in n) == (bits == 10) for n in names if "yuv" in n), names
    (h, w), (hc, wc) = y4m.plane_sizes(*src)
    assert got.dim() == 1 and got.numel() == h * w + 2 * hc * wc and got.dtype == (torch.uint8 if bits == 8 else torch.uint16)
    g = got.cpu().numpy()
    worst, differing, outside, share = yc.compare_out(g, x, src, bits, matrix, full)
    print(f"to_out_yuv {net}->{src} {bits} bit {'full' if full else 'limited'} {matrix} [{form}]: max |d| = {worst} step, {differing} samples "
          f"differ, {outside} of them outside the tie window, {share:.3%} of the samples inside it")
    assert worst <= 1, worst
    assert outside == 0, outside
    assert share <= yc.TIE_SHARE_MAX, share
    assert int(g.max()) <= (1 << bits) - 1
    assert np.array_equal(tools.to_out(x.to(dev), src, pixfmt="yuv420", matrix=matrix, full_range=full,
                                       depth=8 if bits == 8 else 16, maxval=None if bits == 8 else 1023), g)
    if src == (45, 71):  # every tap of these samples lies inside a planted block (tests/test_y4m_cpu.py checks the restatement there)
        yp, up, vp = yc.split(g, src)
        want = yc.planted_codes(bits, full)
        assert (int(yp[17, 26]), int(up[8, 13]), int(vp[8, 13])) == want["black"]   # NaN and -0.5 -> the code of 0
        assert (int(yp[31, 26]), int(up[15, 13]), int(vp[15, 13])) == want["white"]  # +inf and 1.5 -> the code of 1


@pytest.mark.parametrize("bits,full", list(itertools.product((8, 10), (False, True))))
def test_round_trip_properties_on_the_device(dev, bits, full):
    """Through ops.to_inp_yuv / ops.to_out_yuv without resize, both forms: luma returns bit for bit for an in-gamut frame, flat
    chroma returns bit for bit, every legal luma value over neutral chroma returns itself."""
    mv = None if bits == 8 else 1023

    def trip(f, matrix):
        size = f.shape[:2]
        x = ops.to_inp_yuv(torch.from_numpy(f.data).to(dev), size, size, matrix=matrix, full_range=full, maxval=mv)
        return yc.split(ops.to_out_yuv(x, size, matrix=matrix, full_range=full, **_depth_kw(bits)).cpu().numpy(), size)

    for matrix in ("bt709", "bt601"):
        for size in ((45, 71), (48, 64)):  # general, rows
            f = yc.in_gamut_frame(*size, bits, seed=bits)
            assert np.array_equal(trip(f, matrix)[0], f.planes()[0])
            f = yc.in_gamut_frame(*size, bits, seed=3, flat_chroma=True)
            assert all(np.array_equal(a, b) for a, b in zip(trip(f, matrix), f.planes()))
        for size in ((33, 34), (32, 32)):
            f = yc.legal_luma_frame(*size, bits, full)
            assert all(np.array_equal(a, b) for a, b in zip(trip(f, matrix), f.planes()))


def test_entry_points_validate_their_arguments(dev):
    lib = _lib.load()
    H, W, Hc, Wc = 16, 24, 8, 12
    p8 = torch.zeros(H * W + 2 * Hc * Wc, dtype=torch.uint8, device=dev)
    p16 = torch.zeros(H * W + 2 * Hc * Wc + 8, dtype=torch.uint16, device=dev)
    x = torch.zeros((1, 3, H, W), dtype=torch.float32, device=dev)
    st = ops._stream()

    def planes(t, off=0):
        es, b = t.element_size(), t.data_ptr() + off
        return [C.c_void_p(b), C.c_void_p(b + H * W * es), C.c_void_p(b + (H * W + Hc * Wc) * es)]

    def inp8(pl=None, size=(H, W, H, W), matrix=0, strides=(W, Wc), out=x):
        pl = planes(p8) if pl is None else pl
        return lib.drba_to_inp_yuv420_x4(*pl, *strides, C.c_void_p(out.data_ptr() if out is not None else 0), None, *size, 1.0, 1.0, matrix, 0, st)

    def out8(pl=None, size=(H, W, H, W), matrix=0, strides=(W, Wc), src=x):
        pl = planes(p8) if pl is None else pl
        return lib.drba_to_out_yuv420(C.c_void_p(src.data_ptr() if src is not None else 0), *pl, *strides, *size, 1.0, 1.0, matrix, 0, st)

    def inp16(pl=None, maxval=1023.0, matrix=0):
        pl = planes(p16) if pl is None else pl
        return lib.drba_to_inp16_yuv420_x4(*pl, W, Wc, C.c_void_p(x.data_ptr()), None, H, W, H, W, 1.0, 1.0, matrix, 0, maxval, st)

    def out16(pl=None, maxval=1023.0, matrix=0):
        pl = planes(p16) if pl is None else pl
        return lib.drba_to_out16_yuv420(C.c_void_p(x.data_ptr()), *pl, W, Wc, H, W, H, W, 1.0, 1.0, matrix, 0, maxval, st)

    assert inp8() == 0 and out8() == 0 and inp16() == 0 and out16() == 0
    for k in range(3):  # a null plane
        pl = planes(p8)
        pl[k] = None
        assert inp8(pl=pl) == -1 and out8(pl=pl) == -1
        pl = planes(p16)
        pl[k] = None
        assert inp16(pl=pl) == -1 and out16(pl=pl) == -1
    assert inp8(out=None) == -1 and out8(src=None) == -1
    for k in range(4):  # a zero size
        size = [H, W, H, W]
        size[k] = 0
        assert inp8(size=tuple(size)) == -1 and out8(size=tuple(size)) == -1
    assert inp8(strides=(W - 1, Wc)) == -1 and out8(strides=(W, Wc - 1)) == -1  # a stride shorter than its row
    for matrix in (2, -1):
        assert inp8(matrix=matrix) == -1 and out8(matrix=matrix) == -1 and inp16(matrix=matrix) == -1 and out16(matrix=matrix) == -1
    for maxval in (255.0, 70000.0, float("nan")):
        assert inp16(maxval=maxval) == -1 and out16(maxval=maxval) == -1
    assert inp16(pl=planes(p16, off=1)) == -1 and out16(pl=planes(p16, off=1)) == -1  # a misaligned 16-bit pointer
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.to_out_yuv(x, (H, W), matrix="bt2020")
    with pytest.raises(_lib.DrbaHipError):
        ops.to_inp_yuv(p8[:-1], (H, W), (H, W))


# ---------------------------------------------------------------------------------------------------------------- whole clip
@pytest.mark.parametrize("bits", [8, 10])
def test_whole_clip_y4m_against_the_cpu_oracle_driver(dev, bits):
    """RIFE on synthetic weights, a 6-frame 128 x 192 clip built from synth.make_clip / make_clip16 through the restatement, -t 2,
    planar 4:2:0 in and out, against the CPU oracle driver with the restatement's hooks.  The bar is 1 step: the project's 1e-3
    frame tolerance is 0.22 steps of 219 and 0.88 of 876, and |round(a) - round(b)| <= ceil(|a - b|).  The measured maximum and the
    share of differing samples are printed (profiles/yuv420.md records them); no tighter number is fixed."""
    import oracle
    from drba_amd import infer as drv
    from drba_amd.models.rife import RIFE
    from tests.clip_common import ListIO
    src = synth.make_clip(6, 128, 192, seed=1234) if bits == 8 else synth.make_clip16(6, 128, 192, seed=1234)
    frames = yc.clip_from_bgr(src, bits)
    sd = synth.ifnet_state_dict(seed=0)
    mv = None if bits == 8 else 1023
    io_ = ListIO(frames, 24.0)
    n = drv.interpolate_stream(RIFE(weights=sd, scale=1.0, device=dev), io_, 48.0, times=2,
                               to_inp=lambda fr, size: tools.to_inp(fr, size),
                               to_out=lambda x, size: tools.to_out(x, size, pixfmt="yuv420", depth=8 if bits == 8 else 16, maxval=mv))
    ref_io = ListIO(frames, 24.0)
    to_inp, to_out, check = yc.cpu_hooks(bits, bits)
    drv.interpolate_stream(oracle.rife.RifeOracle(sd, 1.0), ref_io, 48.0, times=2, to_inp=to_inp, to_out=to_out, check_scene=check)
    got, want = np.stack(io_.written), np.stack(ref_io.written)
    assert n == 12 and got.shape == want.shape == (12, 128 * 192 * 3 // 2) and got.dtype == want.dtype
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    # the pass-through emissions (head and tail copies): luma unchanged (in gamut: the clip came from RGB), chroma filtered
    for k, f in ((0, frames[0]), (-1, frames[-1])):
        gy, gu, gv = yc.split(got[k], (128, 192))
        sy_, su, sv = f.planes()
        mse = float(np.mean(np.concatenate([(gu.astype(np.float64) - su).reshape(-1), (gv.astype(np.float64) - sv).reshape(-1)]) ** 2))
        psnr = float("inf") if mse == 0 else 10 * np.log10(((1 << bits) - 1) ** 2 / mse)
        print(f"pass-through frame {k}: luma samples changed {int((gy != sy_).sum())} of {gy.size}, chroma PSNR {psnr:.2f} dB")
    print(f"whole clip {bits} bit: max |d| = {int(d.max())} step (bar {yc.CLIP_TOL_STEPS}), differing samples {float((d != 0).mean()):.4%}")
    assert int(d.max()) <= yc.CLIP_TOL_STEPS, int(d.max())


# -------------------------------------------------------------------------------------------------------------- command lines
def test_command_lines_with_y4m(dev, tmp_path):
    """One child process: infer.py y4m -> y4m (8 bits, C420mpeg2 and XCOLORRANGE carried), y4m p10 -> y4m, npz -> y4m with --out-depth
    16 (C420p10) and --yuv-range full, y4m p10 -> npz (uint16 frames, maxval 1023), and -i - / -o - through the child's own pipes
    (nothing but the stream on stdout).  4 frames of 128 x 192, -t 2 ."""
    wdir = tmp_path / "w"
    wdir.mkdir()
    torch.save({"module." + k: v for k, v in synth.ifnet_state_dict(0).items()}, str(wdir / "flownet.pkl"))
    bgr = synth.make_clip(4, 128, 192, seed=21)
    f8, f10 = yc.clip_from_bgr(bgr, 8), yc.clip_from_bgr(bgr, 10)
    h8 = y4m.Header(192, 128, (24000, 1001), interlace="p", aspect="1:1", chroma="420mpeg2", color_range="LIMITED", extra=("KEEP=me",))
    h10 = y4m.Header(192, 128, (25, 1), interlace="p", chroma="420p10")
    p8, p10, pz = str(tmp_path / "in8.y4m"), str(tmp_path / "in10.y4m"), str(tmp_path / "in8.npz")
    open(p8, "wb").write(yc.y4m_bytes(f8, h8))
    open(p10, "wb").write(yc.y4m_bytes(f10, h10))
    np.savez(pz, frames=np.stack(bgr), fps=np.float64(24.0))
    outs = {k: str(tmp_path / f"out_{k}") for k in ("8.y4m", "10.y4m", "npz16.y4m", "10.npz")}
    jobs = [(p8, outs["8.y4m"], ["-t", "2"]), (p10, outs["10.y4m"], ["-t", "2"]),
            (pz, outs["npz16.y4m"], ["-t", "2", "--out-depth", "16", "--yuv-range", "full"]), (p10, outs["10.npz"], ["-t", "2"]),
            ("-", "-", ["-t", "2", "--yuv-range", "full", "--yuv-matrix", "bt601"])]
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import drba_amd.infer as I\n"
        "m = I.load_model('rife', 1.0, weights=%r)\n"
        "for inp, out, extra in %r:\n"
        "    print('written', I.inference(m, I.parse_args(['-m', 'rife', '-i', inp, '-o', out] + extra)), file=sys.stderr)\n"
        % (ROOT, str(wdir), jobs))
    env = dict(os.environ, DRBA_TUNE_CACHE="0")
    r = subprocess.run([sys.executable, "-c", code], input=yc.y4m_bytes(f8, h8), capture_output=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [ln for ln in r.stderr.decode().splitlines() if ln.startswith("written")] == ["written 8"] * 5

    def read(path_or_bytes):
        rd = y4m.Reader(io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, bytes) else open(path_or_bytes, "rb"))
        return rd.header, list(rd)

    h, fr = read(outs["8.y4m"])
    assert h.format() == h8.format().replace(b"F24000:1001", b"F48000:1001") and len(fr) == 8 and fr[0].depth == 8
    assert np.array_equal(fr[0].planes()[0], f8[0].planes()[0])  # the head copy's luma: in gamut, no resize at this size
    h, fr = read(outs["10.y4m"])
    assert h.format() == h10.format().replace(b"F25:1", b"F50:1") and len(fr) == 8 and fr[0].depth == 10
    assert np.array_equal(fr[-1].planes()[0], f10[-1].planes()[0])
    h, fr = read(outs["npz16.y4m"])
    assert (h.chroma, h.color_range, h.fps_num, h.fps_den, h.interlace) == ("420p10", "FULL", 48, 1, "p") and len(fr) == 8 and fr[0].depth == 10
    assert int(fr[0].data.max()) <= 1023 and int(fr[0].planes()[0].max()) > 255
    z = np.load(outs["10.npz"])
    assert z["frames"].dtype == np.uint16 and z["frames"].shape == (8, 128, 192, 3) and int(z["maxval"]) == 1023 and float(z["fps"]) == 50.0
    assert int(z["frames"].max()) <= 1023
    # the pipe: stdout holds the stream and nothing else; the source's LIMITED tag rules the way in, --yuv-range the way out
    h, fr = read(r.stdout)
    assert h.format() == h8.format().replace(b"F24000:1001", b"F48000:1001").replace(b"LIMITED", b"FULL")
    assert len(fr) == 8 and len(r.stdout) == len(h.format()) + 8 * (6 + h.frame_bytes)
