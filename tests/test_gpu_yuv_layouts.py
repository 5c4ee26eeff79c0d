"""GPU: planar YCbCr 4:2:2 and 4:4:4 frames -- the layout-aware conversion kernels (frame_io.hip: the drba_to_*_yuv* entries that take
a layout) against the fp64 restatement of tests/yuv_layouts_common.py in both kernel forms (read from the launch trace), the pad and
crop forms against their resize siblings bit for bit, the round trips the layouts exist for, a whole clip through interpolate_stream
against the CPU oracle driver, and the command lines."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from drba_amd import ops, y4m
from drba_amd.models.utils import tools
from drba_amd.utils import synth
from tests import yuv_common as yc
from tests import yuv_layouts_common as yl

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


def _forms(names, direction, layout):
    return [("rows" if "rows" in n else "general") for n in names if "yuv" + layout in n and direction in n]


def _named(names, bits):
    return all(("16" in n) == (bits == 10) for n in names if "yuv" in n)


# (src size, net size, the kernel form both directions must take)
GEOMETRIES = [((45, 71), (64, 128), "general"), ((60, 64), (64, 64), "rows"), ((60, 66), (64, 66), "general")]
ALL = list(itertools.product((8, 10), (False, True), ("bt709", "bt601")))
CASES = [(lay, g, b, f, m) for lay in ("422", "444")
         for g, b, f, m in [(GEOMETRIES[0], b, f, m) for b, f, m in ALL] + [(g, b, False, "bt709") for g in GEOMETRIES[1:] for b in (8, 10)]]
IDS = [f"{lay}-{g[0][0]}x{g[0][1]}-{b}bit-{'full' if f else 'limited'}-{m}" for lay, g, b, f, m in CASES]
PAD_GEOMETRIES = GEOMETRIES[:2]


def _depth_kw(bits):
    return {"depth": 8} if bits == 8 else {"depth": 16, "maxval": 1023}


def _mv(bits):
    return None if bits == 8 else 1023


@pytest.mark.parametrize("layout,geometry,bits,full,matrix", CASES, ids=IDS)
def test_to_inp_yuv_layouts_against_the_restatement(dev, layout, geometry, bits, full, matrix):
    """Every fp32 value within 2e-6 of the fp64 restatement (0 and m planted at the corners of all three planes), the [H,W,4] copy
    equal to the planar result bit for bit, the form read from the launch trace, tools.to_inp equal to ops.to_inp_yuv."""
    src, net, form = geometry
    f = yl.random_frame(src[0], src[1], bits, seed=src[1] + bits, layout=layout)
    want = yl.to_inp_ref(f, net, bits, matrix, full, layout)
    planes = torch.from_numpy(f.data).to(dev)
    got, names = _traced(lambda: ops.to_inp_yuv(planes, src, net, matrix=matrix, full_range=full, maxval=_mv(bits), layout=layout))
    assert _forms(names, "to_inp", layout) == [form] and _named(names, bits), names
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, net[0], net[1])
    err = float((got.cpu().double() - want).abs().max())
    print(f"to_inp_yuv {layout} {src}->{net} {bits} bit {'full' if full else 'limited'} {matrix} [{form}]: max |d| = {err:.3e} (bar {yl.TO_INP_TOL:.0e})")
    assert err <= yl.TO_INP_TOL, err
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    x4 = ops._x4_of(got)
    assert x4 is not None and tuple(x4.shape) == (net[0], net[1], 4)
    assert torch.equal(x4[:, :, :3], got[0].permute(1, 2, 0)) and not bool(x4[:, :, 3].any())
    assert torch.equal(tools.to_inp(f, net, matrix=matrix, full_range=full), got)  # the host-frame entry: the frame carries its layout


@pytest.mark.parametrize("layout,geometry,bits,full,matrix", CASES, ids=IDS)
def test_to_out_yuv_layouts_against_the_restatement(dev, layout, geometry, bits, full, matrix):
    """yuv_common's way-out rule: never more than one step, no difference outside the tie window, at most 1 % of the samples inside
    it (a condition: tests/test_y4m_layouts_cpu.py asserts it of the restatement alone for these inputs); the planted blocks."""
    src, net, form = geometry
    x = yl.planted_net_frame(net, seed=7)
    got, names = _traced(lambda: ops.to_out_yuv(x.to(dev), src, matrix=matrix, full_range=full, layout=layout, **_depth_kw(bits)))
    assert _forms(names, "to_out", layout) == [form] and _named(names, bits), names
    (h, w), (hc, wc) = y4m.plane_sizes(*src, layout)
    assert got.dim() == 1 and got.numel() == h * w + 2 * hc * wc and got.dtype == (torch.uint8 if bits == 8 else torch.uint16)
    g = got.cpu().numpy()
    worst, differing, outside, share = yl.compare_out(g, x, src, bits, matrix, full, layout)
    print(f"to_out_yuv {layout} {net}->{src} {bits} bit {'full' if full else 'limited'} {matrix} [{form}]: max |d| = {worst} step, {differing} "
          f"samples differ, {outside} of them outside the tie window, {share:.3%} of the samples inside it")
    assert worst <= 1, worst
    assert outside == 0, outside
    assert share <= yl.TIE_SHARE_MAX, share
    assert int(g.max()) <= (1 << bits) - 1
    assert np.array_equal(tools.to_out(x.to(dev), src, pixfmt="yuv" + layout, matrix=matrix, full_range=full, depth=8 if bits == 8 else 16,
                                       maxval=_mv(bits)), g)
    if src == (45, 71):
        yp, up, vp = yl.split(g, src, layout)
        for colour, code in yl.planted_codes(bits, full).items():
            (ly, lx), (cy, cx) = yl.PLANTED["resized"][layout][colour]
            assert (int(yp[ly, lx]), int(up[cy, cx]), int(vp[cy, cx])) == code, colour


PAD_CASES = [(lay, g, b) for lay in ("422", "444") for g in PAD_GEOMETRIES for b in (8, 10)]
PAD_IDS = [f"{lay}-{g[0][0]}x{g[0][1]}-{b}bit" for lay, g, b in PAD_CASES]
# (full range, matrix) of the pad / crop cases.  Full-range bt601 is not among them: where an axis is not resized ATen's copy turns the
# planted +inf into NaN -> 0, the (+inf, 1.5, +inf) block becomes pure green, and 0.587 * 1023 = 600.501 puts the whole block inside
# the tie window (yuv_common.planted_net_frame says so of saturated colours): the restatement alone is over the 1 % cap there.
PAD_CONVERSIONS = ((False, "bt709"), (True, "bt709"), (False, "bt601"))


def _replicate(x, net):
    return torch.from_numpy(np.pad(x.cpu().numpy(), ((0, 0), (0, 0), (0, net[0] - x.shape[2]), (0, net[1] - x.shape[3])), mode="edge"))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _spoil_margin(x, src):
    y = x.clone()
    y[:, :, src[0]:, :], y[:, :, :, src[1]:] = 0.9, float("nan")
    return y


@pytest.mark.parametrize("layout,geometry,bits", PAD_CASES, ids=PAD_IDS)
def test_to_inp_yuv_layouts_pad_is_the_resize_sibling_replicate_padded(dev, layout, geometry, bits):
    """fit="pad": inside the frame the values of the resize entry at an unchanged size bit for bit (torch.equal on the bits), the
    margins the converted pixel of the clamped coordinate, the restatement within 2e-6."""
    src, net, form = geometry
    for full, matrix in PAD_CONVERSIONS:
        f = yl.random_frame(src[0], src[1], bits, seed=src[1] + bits, layout=layout)
        planes = torch.from_numpy(f.data).to(dev)
        kw = dict(matrix=matrix, full_range=full, maxval=_mv(bits), layout=layout)
        got, names = _traced(lambda: ops.to_inp_yuv(planes, src, net, fit="pad", **kw))
        assert _forms(names, "to_inp", layout) == [form] and _named(names, bits) and all("pad" in n for n in names if "yuv" in n), names
        want = _replicate(ops.to_inp_yuv(planes, src, src, **kw), net)
        assert _same_bits(got.cpu(), want), float((got.cpu() - want).abs().max())
        x4 = ops._x4_of(got)
        assert _same_bits(x4[:, :, :3].cpu(), got[0].permute(1, 2, 0).cpu()) and not bool(x4[:, :, 3].any())
        err = float((got.cpu().double() - yl.to_inp_pad_ref(f, net, bits, matrix, full, layout)).abs().max())
        print(f"to_inp_yuv {layout} pad {src}->{net} {bits} bit [{form}]: max |d| = {err:.3e} (bar {yl.TO_INP_TOL:.0e})")
        assert err <= yl.TO_INP_TOL, err
        assert torch.equal(tools.to_inp(f, net, matrix=matrix, full_range=full, fit="pad"), got)


@pytest.mark.parametrize("layout,geometry,bits", PAD_CASES, ids=PAD_IDS)
def test_to_out_yuv_layouts_crop_is_the_resize_sibling_of_the_window(dev, layout, geometry, bits):
    """fit="pad" on the way out: the resize entry given the window alone, bit for bit; the restatement of the window under the
    way-out rule; the margin is never read, not by the chroma mean at an odd last column either (71 is odd)."""
    src, net, form = geometry
    x = yl.planted_net_frame(net, seed=7)
    for full, matrix in PAD_CONVERSIONS:
        kw = dict(matrix=matrix, full_range=full, layout=layout, **_depth_kw(bits))
        got, names = _traced(lambda: ops.to_out_yuv(x.to(dev), src, fit="pad", **kw))
        assert _forms(names, "to_out", layout) == [form] and _named(names, bits) and all("crop" in n for n in names if "yuv" in n), names
        g = got.cpu().numpy()
        assert np.array_equal(g, ops.to_out_yuv(x[:, :, :src[0], :src[1]].contiguous().to(dev), src, **kw).cpu().numpy())
        worst, differing, outside, share = yl.compare_out(g, x, src, bits, matrix, full, layout, crop=True)
        print(f"to_out_yuv {layout} crop {net}->{src} {bits} bit [{form}]: max |d| = {worst} step, {differing} differ, {outside} outside the "
              f"window, {share:.3%} inside it")
        assert worst <= 1 and outside == 0 and share <= yl.TIE_SHARE_MAX, (worst, outside, share)
        yp, up, vp = yl.split(g, src, layout)
        (ly, lx), (cy, cx) = yl.PLANTED["window"][layout]["black"]
        assert (int(yp[ly, lx]), int(up[cy, cx]), int(vp[cy, cx])) == yl.planted_codes(bits, full)["black"]
        assert np.array_equal(ops.to_out_yuv(_spoil_margin(x, src).to(dev), src, fit="pad", **kw).cpu().numpy(), g)
        assert np.array_equal(tools.to_out(x.to(dev), src, pixfmt="yuv" + layout, matrix=matrix, full_range=full,
                                           depth=8 if bits == 8 else 16, maxval=_mv(bits), fit="pad"), g)


@pytest.mark.parametrize("bits,full", list(itertools.product((8, 10), (False, True))))
def test_round_trips_without_resize(dev, bits, full):
    """What the layouts exist for.  4:4:4: to_out(to_inp(f)) returns all three planes of an in-gamut frame with random chroma bit for
    bit (the fp32 round trip errs by a few 1e-7 x 896 steps, far below half a step).  4:2:2: luma bit for bit, flat chroma bit for
    bit.  The control: the same picture as 4:2:0 does not return its chroma.  Both matrices, both forms, resize and pad entries."""
    def trip(f, matrix, layout, fit):
        size = f.shape[:2]
        x = ops.to_inp_yuv(torch.from_numpy(f.data).to(dev), size, size, matrix=matrix, full_range=full, maxval=_mv(bits), layout=layout, fit=fit)
        back = ops.to_out_yuv(x, size, matrix=matrix, full_range=full, layout=layout, fit=fit, **_depth_kw(bits))
        return yl.split(back.cpu().numpy(), size, layout)

    for matrix, size, fit in itertools.product(("bt709", "bt601"), ((45, 71), (48, 64)), ("resize", "pad")):  # general, rows
        f = yl.in_gamut_frame(*size, bits, seed=bits, layout="444")
        assert all(np.array_equal(a, b) for a, b in zip(trip(f, matrix, "444", fit), f.planes())), (matrix, size, fit)
        f2 = yl.in_gamut_frame(*size, bits, seed=bits, layout="422")
        assert np.array_equal(trip(f2, matrix, "422", fit)[0], f2.planes()[0])
        f2 = yl.in_gamut_frame(*size, bits, seed=3, layout="422", flat_chroma=True)
        assert all(np.array_equal(a, b) for a, b in zip(trip(f2, matrix, "422", fit), f2.planes()))
        f0 = yl.picture_as(f, "420")  # the control
        back = trip(f0, matrix, "420", fit)
        assert np.array_equal(back[0], f0.planes()[0]) and not np.array_equal(back[1], f0.planes()[1])


# ---------------------------------------------------------------------------------------------------------------- whole clip
@pytest.mark.parametrize("layout,bits", [("444", 8), ("422", 10)])
def test_whole_clip_against_the_cpu_oracle_driver(dev, layout, bits):
    """RIFE on synthetic weights, a 6-frame 128 x 192 clip, -t 2, the layout in and out, against the CPU oracle driver with the
    restatement's hooks, within CLIP_TOL_STEPS (yuv_common: the derivation)."""
    import oracle
    from drba_amd import infer as drv
    from drba_amd.models.rife import RIFE
    from tests.clip_common import ListIO
    src = synth.make_clip(6, 128, 192, seed=1234) if bits == 8 else synth.make_clip16(6, 128, 192, seed=1234)
    frames = yl.clip_from_bgr(src, bits, layout)
    sd = synth.ifnet_state_dict(seed=0)
    io_ = ListIO(frames, 24.0)
    n = drv.interpolate_stream(RIFE(weights=sd, scale=1.0, device=dev), io_, 48.0, times=2,
                               to_inp=lambda fr, size: tools.to_inp(fr, size),
                               to_out=lambda x, size: tools.to_out(x, size, pixfmt="yuv" + layout, depth=8 if bits == 8 else 16, maxval=_mv(bits)))
    ref_io = ListIO(frames, 24.0)
    to_inp, to_out, check = yl.cpu_hooks(bits, bits, layout, layout)
    drv.interpolate_stream(oracle.rife.RifeOracle(sd, 1.0), ref_io, 48.0, times=2, to_inp=to_inp, to_out=to_out, check_scene=check)
    got, want = np.stack(io_.written), np.stack(ref_io.written)
    (h, w), (hc, wc) = y4m.plane_sizes(128, 192, layout)
    assert n == 12 and got.shape == want.shape == (12, h * w + 2 * hc * wc) and got.dtype == want.dtype
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(f"whole clip {layout} {bits} bit: max |d| = {int(d.max())} step (bar {yl.CLIP_TOL_STEPS}), differing samples {float((d != 0).mean()):.4%}")
    assert int(d.max()) <= yl.CLIP_TOL_STEPS, int(d.max())
    if layout == "444":  # the pass-through emissions (head and tail copies) return the source's bytes: in gamut, nothing resampled
        assert np.array_equal(got[0], frames[0].data) and np.array_equal(got[-1], frames[-1].data)


# -------------------------------------------------------------------------------------------------------------- command lines
def test_command_lines_with_layouts(dev, tmp_path):
    """One child process runs infer.py four times and evaluate compare twice: C444 in -> C444 out; C420 in with --out-chroma 444
    --out-depth 16 -> C444p10; C422p10 with --fit pad -s --dedup --deterministic (and --nonlinear) twice -> the same bytes
    (evaluate compare --max-lsb 0 exits 0); compare of a 4:4:4 clip with itself names the layout and reports infinite PSNR on all
    planes.  A second, short child: --out-chroma 444 -o out.npz exits non-zero before a model is built."""
    wdir = tmp_path / "w"
    wdir.mkdir()
    torch.save({"module." + k: v for k, v in synth.ifnet_state_dict(0).items()}, str(wdir / "flownet.pkl"))
    bgr = synth.make_clip(4, 128, 192, seed=21)
    clips = {"444": (yl.clip_from_bgr(bgr, 8, "444"), yl.header_for(128, 192, 8, "444", fps=(24000, 1001), aspect="1:1", extra=("KEEP=me",))),
             "420": (yc.clip_from_bgr(bgr, 8), y4m.Header(192, 128, (25, 1), interlace="p", chroma="420mpeg2")),
             "422p10": (yl.clip_from_bgr(bgr, 10, "422"), yl.header_for(128, 192, 10, "422", fps=(25, 1)))}
    paths = {k: str(tmp_path / f"in_{k}.y4m") for k in clips}
    for k, (fr, hdr) in clips.items():
        open(paths[k], "wb").write(yl.y4m_bytes(fr, hdr))
    outs = {k: str(tmp_path / f"out_{k}.y4m") for k in ("444", "420to444p10", "422a", "422b")}
    rep = str(tmp_path / "self.json")
    hard = ["-t", "2", "--fit", "pad", "-s", "--dedup", "--deterministic", "--nonlinear"]
    jobs = [(paths["444"], outs["444"], ["-t", "2"]), (paths["420"], outs["420to444p10"], ["-t", "2", "--out-chroma", "444", "--out-depth", "16"]),
            (paths["422p10"], outs["422a"], hard), (paths["422p10"], outs["422b"], hard)]
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import drba_amd.infer as I\n"
        "import drba_amd.evaluate as E\n"
        "m = I.load_model('rife', 1.0, weights=%r)\n"
        "for inp, out, extra in %r:\n"
        "    print('written', I.inference(m, I.parse_args(['-m', 'rife', '-i', inp, '-o', out] + extra)), file=sys.stderr)\n"
        "print('same', E.main(['compare', %r, %r, '--max-lsb', '0']), file=sys.stderr)\n"
        "print('self', E.main(['compare', %r, %r, '--json', %r]), file=sys.stderr)\n"
        % (ROOT, str(wdir), jobs, outs["422a"], outs["422b"], outs["444"], outs["444"], rep))
    env = dict(os.environ, DRBA_TUNE_CACHE="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stderr.decode().splitlines()
    assert [ln for ln in lines if ln.startswith("written")] == ["written 8"] * 4, lines[-10:]
    assert "same 0" in lines and "self 0" in lines, lines[-10:]

    def read(path):
        rd = y4m.Reader(open(path, "rb"), accept=y4m.ACCEPT_ALL)
        return rd.header, list(rd)

    h, fr = read(outs["444"])
    assert h.format() == clips["444"][1].format().replace(b"F24000:1001", b"F48000:1001") and len(fr) == 8
    assert (fr[0].layout, fr[0].depth) == ("444", 8) and np.array_equal(fr[0].data, clips["444"][0][0].data)  # the head copy: the source's bytes
    h, fr = read(outs["420to444p10"])
    assert (h.chroma, h.layout, h.depth, h.fps_num, h.fps_den) == ("444p10", "444", 10, 50, 1) and len(fr) == 8
    assert os.path.getsize(outs["420to444p10"]) == len(h.format()) + 8 * (6 + 2 * 3 * 128 * 192) and h.frame_bytes == 2 * 3 * 128 * 192
    assert int(fr[0].data.max()) <= 1023 and int(fr[0].planes()[0].max()) > 255
    h, fr = read(outs["422a"])
    assert (h.chroma, h.layout, h.depth) == ("422p10", "422", 10) and len(fr) == 8 and h.frame_bytes == 2 * 2 * 128 * 192
    assert open(outs["422a"], "rb").read() == open(outs["422b"], "rb").read()
    report = json.load(open(rep))
    assert report["pixfmt"] == "yuv444" and report["chroma"] == ["444", "444"] and report["frames"] == 8, report
    planes = ("mean_psnr_y", "mean_psnr_u", "mean_psnr_v", "psnr_of_mean_mse_y", "psnr_of_mean_mse_u", "psnr_of_mean_mse_v")
    assert all(report[k] == "inf" for k in planes) and report["total_differing"] == 0 and report["max_lsb"] == 0, report
    assert all(p == "inf" for k in ("psnr_y", "psnr_u", "psnr_v") for p in report["per_frame"][k]) and abs(report["mean_ssim"] - 1.0) < 1e-9
    # refused before a model is built: no weights are given, nothing is loaded
    bad = subprocess.run([sys.executable, "-m", "drba_amd.infer", "-m", "rife", "-i", paths["444"], "-o", str(tmp_path / "out.npz"), "-t", "2",
                          "--out-chroma", "444"], capture_output=True, timeout=300, cwd=ROOT, env=env)
    assert bad.returncode != 0 and b"--out-chroma" in bad.stderr, bad.stderr[-1000:]
