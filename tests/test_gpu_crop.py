"""GPU: --crop on the device -- the active-picture statistic (active_area.hip: drba_edge_max_u8 / _u16) against its numpy reference,
element for element; the windowed conversions against the same conversions of a contiguous copy of the window, bit for bit (way in)
and byte for byte (way out, black outside the rectangle); and the command line: a clip embedded in black frames and run with
`--crop auto --deterministic` writes, inside the box, the bytes the bare clip writes without the flag -- packed 8-bit at both fits,
4:2:0 Y4M, 10-bit packed, with -s and with --dedup -- and exact black outside it.  Every command line runs in ONE child process (one
model load), started once per module."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from drba_amd import crop, ops, y4m
from drba_amd.crop import Box
from drba_amd.utils import synth
from tests import dedup_common as dc
from tests import yuv_common as yc
from tests import yuv_layouts_common as ylc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 96, 160            # the picture
FH, FW, Y0, X0 = 128, 224, 16, 32  # the frame it is embedded in, and where
BOX = Box(W, H, X0, Y0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ 1. the statistic
def _stat_cases():
    rng = np.random.default_rng(7)
    last = np.zeros((19, 23, 3), np.uint8)
    last[-1, -1, -1] = 201  # the only bright sample is the last sample of the last row
    wide = np.zeros((33, 96), np.uint8)
    wide[:, :70] = rng.integers(0, 256, size=(33, 70), dtype=np.uint8)
    wide[:, 70:] = 255  # what the pitch skips must not be read as picture
    big = rng.integers(0, 120, size=(1080, 1920, 3), dtype=np.uint8)
    big[517, 1203, 1], big[1079, 1919, 2], big[0, 0, 0] = 250, 251, 252
    return {
        "u8_packed_37x50": (rng.integers(0, 256, size=(37, 50, 3), dtype=np.uint8), None),   # pitch 150: byte loads, a column tail
        "u8_packed_36x52": (rng.integers(0, 256, size=(36, 52, 3), dtype=np.uint8), None),   # pitch 156: 4-byte loads
        "u8_plane_33x70_pitch96": (wide, 70),                                                # 16-byte loads, rows with a tail
        "u16_plane_41x77": (rng.integers(0, 1024, size=(41, 77), dtype=np.uint16), None),    # pitch 154 bytes: sample loads
        "u16_plane_40x72": (rng.integers(0, 1024, size=(40, 72), dtype=np.uint16), None),    # pitch 144 bytes: 16-byte loads
        "u16_packed_21x34": (rng.integers(0, 65536, size=(21, 34, 3), dtype=np.uint16), None),
        "1x16": (rng.integers(0, 256, size=(1, 16), dtype=np.uint8), None),
        "16x1": (rng.integers(0, 256, size=(16, 1), dtype=np.uint8), None),
        "last_sample_only": (last, None),
        "all_zero": (np.zeros((24, 40, 3), np.uint8), None),
        "1080p_packed": (big, None),                                                         # grid coverage: 6 strips x 68 bands
        "1080p_plane": (np.ascontiguousarray(big[:, :, 1]), None),
    }


STAT_CASES = _stat_cases()


@pytest.mark.parametrize("name", list(STAT_CASES))
def test_edge_max_equals_the_numpy_reference(dev, name):
    arr, view_cols = STAT_CASES[name]
    t = torch.from_numpy(arr).to(dev)
    if view_cols is not None:
        t, arr = t[:, :view_cols], arr[:, :view_cols]
        assert not t.is_contiguous()
    want_r, want_c = crop.edge_max_numpy(arr)
    # the two arrays hold garbage before the call: the entry writes every element
    got_r, got_c = ops.edge_max(t)
    assert got_r.dtype == got_c.dtype == torch.int32 and got_r.is_cuda and got_c.is_cuda
    assert np.array_equal(got_r.cpu().numpy(), want_r) and np.array_equal(got_c.cpu().numpy(), want_c)
    host, ev, rows = ops.edge_max_async(t)
    ev.synchronize()
    assert rows == arr.shape[0] and np.array_equal(host.numpy()[:rows], want_r) and np.array_equal(host.numpy()[rows:], want_c)
    if arr.ndim == 3:  # the same frame with an explicit group, and as single samples
        flat = t.reshape(t.shape[0], -1)
        r3, c3 = ops.edge_max(flat, group=3)
        assert torch.equal(r3, got_r) and torch.equal(c3, got_c)
        r1, c1 = ops.edge_max(flat)
        assert torch.equal(r1, got_r) and np.array_equal(c1.cpu().numpy(), arr.reshape(arr.shape[0], -1).max(axis=0))


def test_edge_max_overwrites_whatever_the_arrays_held_and_checks_its_arguments(dev):
    import ctypes as C
    from drba_amd import _lib
    lib = _lib.load()
    fr = torch.from_numpy(STAT_CASES["u8_packed_37x50"][0]).to(dev)
    out = torch.full((37 + 50,), 0x7fffffff, dtype=torch.int32, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert lib.drba_edge_max_u8(p(fr), 37, 150, 150, 3, p(out), p(out, 4 * 37), st) == 0
    want_r, want_c = crop.edge_max_numpy(STAT_CASES["u8_packed_37x50"][0])
    assert np.array_equal(out.cpu().numpy(), np.concatenate([want_r, want_c]))
    f16 = torch.zeros(8, 12, dtype=torch.uint16, device=dev)
    for fn, src, args in ((lib.drba_edge_max_u8, fr, (None, 37, 150, 150, 3, p(out), p(out, 148))),
                          (lib.drba_edge_max_u8, fr, (p(fr), 37, 150, 150, 3, None, p(out, 148))),
                          (lib.drba_edge_max_u8, fr, (p(fr), 37, 150, 150, 3, p(out), None)),
                          (lib.drba_edge_max_u8, fr, (p(fr), 0, 150, 150, 3, p(out), p(out, 148))),
                          (lib.drba_edge_max_u8, fr, (p(fr), 37, 0, 150, 3, p(out), p(out, 148))),
                          (lib.drba_edge_max_u8, fr, (p(fr), 37, 150, 149, 3, p(out), p(out, 148))),   # pitch < cols
                          (lib.drba_edge_max_u8, fr, (p(fr), 37, 150, 150, 4, p(out), p(out, 148))),   # cols % g != 0
                          (lib.drba_edge_max_u8, fr, (p(fr), 37, 150, 150, 0, p(out), p(out, 148))),
                          (lib.drba_edge_max_u16, f16, (p(f16, 1), 8, 10, 12, 1, p(out), p(out, 32)))):  # a misaligned u16 pointer
        assert fn(*args, st) == -1, args
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- 2. windowed way in
def _packed(h, w, dtype, maxval, seed):
    return np.random.default_rng(seed).integers(0, maxval + 1, size=(h, w, 3)).astype(dtype)


def _same_input(a, b):
    assert a.shape == b.shape and torch.equal(a, b)
    xa, xb = ops._x4_of(a), ops._x4_of(b)
    assert xa is not None and xb is not None and torch.equal(xa, xb)


PACKED_KINDS = [(np.uint8, None), (np.uint16, 1023), (np.uint16, 65535)]
# (frame, box, network size, fits): the issue's two; then a window as wide as the network tensor, aligned (the rows form) and not
PACKED_IN = [((70, 118), Box(100, 60, 6, 4), (64, 128), ("resize", "pad")), ((70, 118), Box(100, 60, 6, 4), (72, 136), ("pad",)),
             ((70, 120), Box(104, 60, 8, 4), (64, 104), ("resize", "pad")), ((70, 120), Box(104, 60, 7, 4), (64, 104), ("resize", "pad")),
             ((70, 118), Box(104, 60, 8, 4), (64, 104), ("resize", "pad"))]


@pytest.mark.parametrize("dtype,maxval", PACKED_KINDS, ids=["u8", "u16_1023", "u16_65535"])
def test_windowed_packed_input_is_the_cropped_frames_input(dev, dtype, maxval):
    kw = {} if maxval is None else {"maxval": maxval}
    for (fh, fw), b, net, fits in PACKED_IN:
        full = _packed(fh, fw, dtype, maxval or 255, seed=fh + b.x)
        part = np.ascontiguousarray(full[b.y:b.y + b.h, b.x:b.x + b.w])
        tf, tp = torch.from_numpy(full).to(dev), torch.from_numpy(part).to(dev)
        for fit in fits:
            _same_input(ops.to_inp(tf, net, fit=fit, window=b.window, **kw), ops.to_inp(tp, net, fit=fit, **kw))
    # a window equal to the frame equals the call without a window
    _same_input(ops.to_inp(tf, (72, 128), window=(0, 0, fw, fh), **kw), ops.to_inp(tf, (72, 128), **kw))
    for bad in ((0, 0, fw + 1, fh), (-1, 0, 8, 8), (0, 0, 0, 8), (fw - 4, 0, 8, 8), (1, 2, 3)):
        with pytest.raises(ValueError, match="window"):
            ops.to_inp(tf, (72, 128), window=bad, **kw)


def _crop_yuv(fr, b):
    """the window of a YuvFrame as a frame of its own: the chroma rows and columns under it"""
    sx, sy = ylc.LAYOUTS[fr.layout]
    y, u, v = fr.planes()
    cy0, cy1, cx0, cx1 = b.y // sy, -(-(b.y + b.h) // sy), b.x // sx, -(-(b.x + b.w) // sx)
    return y4m.YuvFrame.from_planes(y[b.y:b.y + b.h, b.x:b.x + b.w], u[cy0:cy1, cx0:cx1], v[cy0:cy1, cx0:cx1], depth=fr.depth,
                                    layout=fr.layout)


# (frame, box, network size): an inner window; an odd frame with a window that reaches its right and bottom edge (odd extent); a
# window as wide as the network tensor with everything aligned to 8 (the rows form on both sides)
PLANAR = [((72, 120), Box(100, 60, 8, 6), (64, 128)), ((71, 119), Box(111, 65, 8, 6), (128, 128)), ((72, 120), Box(104, 60, 16, 6), (64, 104))]


@pytest.mark.parametrize("layout", ["420", "422", "444"])
@pytest.mark.parametrize("bits", [8, 10])
def test_windowed_planar_input_is_the_cropped_frames_input(dev, bits, layout):
    mv = {} if bits == 8 else {"maxval": 1023}
    for k, ((fh, fw), b, net) in enumerate(PLANAR):
        fr = ylc.random_frame(fh, fw, bits, 11 + k, layout)
        part = _crop_yuv(fr, b)
        tf, tp = torch.from_numpy(fr.data.copy()).to(dev), torch.from_numpy(part.data.copy()).to(dev)
        for fit in ("resize", "pad"):
            for full_range in (False, True):
                kw = dict(matrix="bt709", full_range=full_range, fit=fit, layout=layout, **mv)
                _same_input(ops.to_inp_yuv(tf, (fh, fw), net, window=b.window, **kw), ops.to_inp_yuv(tp, (b.h, b.w), net, **kw))
    _same_input(ops.to_inp_yuv(tf, (fh, fw), net, window=(0, 0, fw, fh), layout=layout, **mv), ops.to_inp_yuv(tf, (fh, fw), net, layout=layout, **mv))
    if layout != "444":  # a window that splits a chroma sample is refused, the multiple named
        with pytest.raises(ValueError, match="multiples of 2"):
            ops.to_inp_yuv(tf, (fh, fw), net, window=(7, 6, 96, 60), layout=layout, **mv)
        with pytest.raises(ValueError, match="multiples of 2"):
            ops.to_inp_yuv(tf, (fh, fw), net, window=(8, 6, 95, 60), layout=layout, **mv)
    if layout == "420":
        with pytest.raises(ValueError, match="multiples of 2"):
            ops.to_inp_yuv(tf, (fh, fw), net, window=(8, 5, 96, 60), layout=layout, **mv)


# ------------------------------------------------------------------------------------------------------ 3. windowed way out
def _net(net, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((1, 3, *net), generator=g) * 1.02 - 0.01).to(dev)


@pytest.mark.parametrize("dtype,maxval", PACKED_KINDS, ids=["u8", "u16_1023", "u16_65535"])
def test_windowed_packed_output_is_the_boxes_frame_in_black(dev, dtype, maxval):
    kw = {} if maxval is None else {"depth": 16, "maxval": maxval}
    for (fh, fw), b, net, fits in PACKED_IN:
        x, zeros = _net(net, fh + b.x, dev), torch.zeros((1, 3, max(net[0], fh), max(net[1], fw)), device=dev)
        for fit in fits:
            for rgb in (False, True):
                got = ops.to_out(x, (fh, fw), rgb=rgb, fit=fit, window=b.window, **kw).cpu().numpy()
                want = ops.to_out(x, b.size, rgb=rgb, fit=fit, **kw).cpu().numpy()
                assert got.shape == (fh, fw, 3) and got.dtype == dtype
                assert np.array_equal(got[b.y:b.y + b.h, b.x:b.x + b.w], want)
                black = ops.to_out(zeros, (fh, fw), rgb=rgb, fit=fit, **kw).cpu().numpy()  # what the same conversion writes for zeros
                outside = got.copy()
                outside[b.y:b.y + b.h, b.x:b.x + b.w] = black[b.y:b.y + b.h, b.x:b.x + b.w]
                assert np.array_equal(outside, black) and not black.any()
    whole = ops.to_out(x, b.size, window=(0, 0, b.w, b.h), **kw)
    assert torch.equal(whole, ops.to_out(x, b.size, **kw))


@pytest.mark.parametrize("layout", ["420", "422", "444"])
@pytest.mark.parametrize("bits", [8, 10])
def test_windowed_planar_output_is_the_boxes_frame_in_black(dev, bits, layout):
    depth = {"depth": 8} if bits == 8 else {"depth": 16, "maxval": 1023}
    for k, ((fh, fw), b, net) in enumerate(PLANAR):
        x = _net(net, 23 + k, dev)
        for fit in ("resize", "pad"):
            for full_range in (False, True):
                kw = dict(matrix="bt709", full_range=full_range, layout=layout, **depth)
                got = ops.to_out_yuv(x, (fh, fw), fit=fit, window=b.window, **kw).cpu().numpy()
                want = ops.to_out_yuv(x, b.size, fit=fit, **kw).cpu().numpy()
                # black: the samples the same conversion writes for an all-zero network tensor
                black = ops.to_out_yuv(torch.zeros((1, 3, 128, 128), device=dev), (fh, fw), fit=fit, **kw).cpu().numpy()
                fg, fb = ylc.frame_of(got, (fh, fw), bits, layout), ylc.frame_of(black.copy(), (fh, fw), bits, layout)
                inner = _crop_yuv(fg, b)
                assert np.array_equal(inner.data, want), (fit, full_range)
                codes = yc.planted_codes(bits, full_range)["black"]
                sx, sy = ylc.LAYOUTS[layout]
                for plane_g, plane_b, code, (py, px, ph, pw) in zip(
                        fg.planes(), fb.planes(), codes,
                        [(b.y, b.x, b.h, b.w)] + [(b.y // sy, b.x // sx, -(-(b.y + b.h) // sy) - b.y // sy, -(-(b.x + b.w) // sx) - b.x // sx)] * 2):
                    assert (plane_b == code).all()  # the range's black code, mid-grey chroma
                    outside = plane_g.copy()
                    outside[py:py + ph, px:px + pw] = code
                    assert np.array_equal(outside, plane_b), (fit, full_range)
    assert torch.equal(ops.to_out_yuv(x, b.size, window=(0, 0, b.w, b.h), **kw), ops.to_out_yuv(x, b.size, **kw))


# ------------------------------------------------------------------------------------------------------- 4 - 7. the command line
def _embed(frames, value=0, noise=None):
    frames = np.stack(frames)
    out = np.full((len(frames), FH, FW, 3), value, frames.dtype)
    if noise is not None:
        out[:] = noise.integers(0, 9, size=out.shape).astype(frames.dtype)  # amplitude <= 8/255
    out[:, Y0:Y0 + H, X0:X0 + W] = frames
    return out


def _embed_yuv(fr):
    y, u, v = fr.planes()
    Y, U, V = np.full((FH, FW), 16, np.uint8), np.full((FH // 2, FW // 2), 128, np.uint8), np.full((FH // 2, FW // 2), 128, np.uint8)
    Y[Y0:Y0 + H, X0:X0 + W] = y
    U[Y0 // 2:(Y0 + H) // 2, X0 // 2:(X0 + W) // 2] = u
    V[Y0 // 2:(Y0 + H) // 2, X0 // 2:(X0 + W) // 2] = v
    return y4m.YuvFrame.from_planes(Y, U, V, depth=8, layout="420")


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """-> {job: {"frames" | "stream", "written", "stderr"}}, the clips, and the scan's boxes"""
    tmp = tmp_path_factory.mktemp("crop")
    wdir = tmp / "w"
    wdir.mkdir()
    torch.save({"module." + k: v for k, v in synth.ifnet_state_dict(0).items()}, str(wdir / "flownet.pkl"))
    A, D = dc.moving_clip(6, H, W, seed=41), dc.moving_clip(6, H, W, seed=77)
    cut = list(A[:3]) + list(D[3:])                               # one cut
    twos = dc.repeat_clip(A, [i // 2 for i in range(12)])         # held on twos
    a16 = [f.astype(np.uint16) * 4 + 1 for f in A]                # 10-bit samples
    clips = {"A": np.stack(A), "E": _embed(A), "N": _embed(A, noise=np.random.default_rng(5)), "cut": np.stack(cut), "Ecut": _embed(cut),
             "twos": np.stack(twos), "Etwos": _embed(twos), "A16": np.stack(a16), "E16": _embed(a16)}
    for name, fr in clips.items():
        extra = {"maxval": np.int64(1023)} if fr.dtype == np.uint16 else {}
        np.savez(str(tmp / f"{name}.npz"), frames=fr, fps=np.float64(24.0), **extra)
    ay = yc.clip_from_bgr(A, 8)
    ey = [_embed_yuv(f) for f in ay]
    for name, fr, (h, w) in (("Ay", ay, (H, W)), ("Ey", ey, (FH, FW))):
        with open(str(tmp / f"{name}.y4m"), "wb") as f:
            f.write(yc.y4m_bytes(fr, y4m.Header(w, h, (24, 1), interlace="p", chroma="420mpeg2")))
    det, auto = ["-t", "2", "--deterministic"], ["-t", "2", "--deterministic", "--crop", "auto"]
    jobs = [("A_resize", "A.npz", det), ("E_resize", "E.npz", auto), ("A_pad", "A.npz", det + ["--fit", "pad"]),
            ("E_pad", "E.npz", auto + ["--fit", "pad"]), ("N_resize", "N.npz", auto), ("E_explicit", "E.npz", det + ["--crop", f"crop={BOX}"]),
            ("A_auto", "A.npz", auto), ("Ay", "Ay.y4m", det), ("Ey", "Ey.y4m", auto), ("A16", "A16.npz", det), ("E16", "E16.npz", auto),
            ("cut", "cut.npz", det + ["-s"]), ("Ecut", "Ecut.npz", auto + ["-s"]), ("twos", "twos.npz", det + ["--dedup"]),
            ("Etwos", "Etwos.npz", auto + ["--dedup"])]
    ext = lambda src: ".y4m" if src.endswith(".y4m") else ".npz"  # noqa: E731
    argv = [(j, ["-m", "rife", "-i", str(tmp / src), "-o", str(tmp / f"out_{j}{ext(src)}")] + extra) for j, src, extra in jobs]
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import drba_amd.infer as I\n"
        "from drba_amd import crop\n"
        "scan = crop.scan\n"
        "def reporting(*a, **k):\n"
        "    box = scan(*a, **k)\n"
        "    print('scanned', box, file=sys.stderr)\n"
        "    return box\n"
        "crop.scan = reporting\n"
        "m = I.load_model('rife', 1.0, weights=%r)\n"
        "for job, argv in %r:\n"
        "    print('job', job, file=sys.stderr)\n"
        "    print('written', I.inference(m, I.parse_args(argv)), file=sys.stderr)\n" % (ROOT, str(wdir), argv))
    env = dict(os.environ, DRBA_TUNE_CACHE="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for part in r.stderr.decode().split("job ")[1:]:
        job = part.split()[0]
        m = re.search(r"\bwritten (\d+)", part)
        s = re.search(r"\bscanned (\S+)", part)
        out[job] = {"stderr": part, "written": int(m.group(1)), "scanned": s.group(1) if s else None}
    for j, src, _ in jobs:
        path = str(tmp / f"out_{j}{ext(src)}")
        if src.endswith(".y4m"):
            out[j]["stream"] = list(y4m.Reader(open(path, "rb"), accept=y4m.ACCEPT_ALL))
        else:
            out[j]["frames"] = np.load(path)["frames"]
    out["clips"], out["tmp"] = clips, tmp
    return out


def _identity(barred, bare):
    """The run identity: inside the box the embedded clip's run wrote the bare clip's bytes, outside it exact black."""
    assert barred.shape == (len(bare), FH, FW, 3) and barred.dtype == bare.dtype
    inside = barred[:, Y0:Y0 + H, X0:X0 + W]
    differing = int((inside != bare).sum())
    outside = barred.copy()
    outside[:, Y0:Y0 + H, X0:X0 + W] = 0
    print(f"run identity: {differing} differing samples of {bare.size} inside the box, {int((outside != 0).sum())} samples outside it not black")
    assert differing == 0 and not outside.any()


@pytest.mark.parametrize("fit", ["resize", "pad"])
def test_run_identity_packed(runs, fit):
    assert runs[f"E_{fit}"]["scanned"] == str(BOX)  # the scan's box is the embedding rectangle
    assert runs[f"E_{fit}"]["written"] == runs[f"A_{fit}"]["written"] == 12
    _identity(runs[f"E_{fit}"]["frames"], runs[f"A_{fit}"]["frames"])


def test_explicit_box_is_the_scanned_one(runs):
    assert runs["E_explicit"]["scanned"] is None  # no scan for an explicit box
    assert runs["E_explicit"]["frames"].tobytes() == runs["E_resize"]["frames"].tobytes()


def test_noisy_bars_are_found_and_written_as_exact_black(runs):
    assert runs["clips"]["N"][:, :Y0].max() == 8  # the bars carry noise of amplitude 8/255 on the way in
    assert runs["N_resize"]["scanned"] == str(BOX)
    _identity(runs["N_resize"]["frames"], runs["A_resize"]["frames"])


def test_run_identity_y4m_420(runs):
    assert runs["Ey"]["scanned"] == str(BOX) and runs["Ey"]["written"] == runs["Ay"]["written"] == 12
    differing = 0
    for got, want in zip(runs["Ey"]["stream"], runs["Ay"]["stream"]):
        assert (got.height, got.width, got.layout, got.depth) == (FH, FW, "420", 8) and (want.height, want.width) == (H, W)
        for g, w_, code, s in zip(got.planes(), want.planes(), (16, 128, 128), (1, 2, 2)):
            inner = g[Y0 // s:(Y0 + H) // s, X0 // s:(X0 + W) // s]
            differing += int((inner != w_).sum())
            outside = g.copy()
            outside[Y0 // s:(Y0 + H) // s, X0 // s:(X0 + W) // s] = code
            assert (outside == code).all()  # bars: Y = 16, U = V = 128
    print(f"run identity, 4:2:0: {differing} differing samples inside the box")
    assert differing == 0


def test_run_identity_10_bit_packed(runs):
    assert runs["E16"]["scanned"] == str(BOX) and runs["E16"]["frames"].dtype == np.uint16
    _identity(runs["E16"]["frames"], runs["A16"]["frames"])


def test_no_bars_no_change(runs):
    assert runs["A_auto"]["scanned"] == "None"
    assert "--crop auto: no bars found" in runs["A_auto"]["stderr"]
    assert runs["A_auto"]["frames"].tobytes() == runs["A_resize"]["frames"].tobytes()
    assert "no bars found" not in runs["E_resize"]["stderr"]


def test_run_identity_with_scene_detection_and_with_dedup(runs):
    assert runs["Ecut"]["scanned"] == runs["Etwos"]["scanned"] == str(BOX)
    _identity(runs["Ecut"]["frames"], runs["cut"]["frames"])
    assert runs["cut"]["frames"].tobytes() != runs["A_resize"]["frames"].tobytes()
    assert runs["Etwos"]["written"] == runs["twos"]["written"] == 24
    _identity(runs["Etwos"]["frames"], runs["twos"]["frames"])


def test_evaluate_bars_prints_the_box(runs):
    r = subprocess.run([sys.executable, "-m", "drba_amd.evaluate", "bars", str(runs["tmp"] / "E.npz")], capture_output=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().splitlines()
    assert [ln.split()[1] for ln in lines[:6]] == [str(BOX)] * 6
    assert lines[6].startswith(f"crop={BOX} ") and "53.6% of the 224x128 frame" in lines[6]
