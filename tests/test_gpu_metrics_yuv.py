"""GPU: the plane-wise metrics of YUV4MPEG2 clips -- drba_ssim2d (metrics.hip) against float64 and against the reference's recorded
values, its exactness properties, the plane errors of metrics.YuvClipMetrics on the device, the argument checks of the new entry
points and the two commands of drba_amd.evaluate on .y4m files.  Truths, pairs and clips live in tests/metrics_yuv_common.py."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from drba_amd import _lib, evaluate, metrics, ops, y4m
from drba_amd.utils import synth
from tests import metrics_yuv_common as myc
from tests import yuv_common as yc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset)


def _call(dev, ta, tb, n, h, w, row_stride, item_stride, dtype, maxval, offset=0):
    """drba_ssim2d on device tensors (the planes start `offset` samples in) -> float64 [n]"""
    lib = _lib.load()
    ws = torch.empty(max(int(lib.drba_ssim2d_ws_floats(n, h, w)), 1), dtype=torch.float32, device=dev)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    es = ta.element_size()
    _lib.check(lib.drba_ssim2d(_p(ta, offset * es), _p(tb, offset * es), _p(out), _p(ws), n, h, w, row_stride, item_stride, dtype,
                               float(maxval), ops._stream()), "drba_ssim2d")
    return out.cpu().numpy()


def _ssim2d(dev, p, q, maxval):
    """one pair of integer planes [H,W] (uint8, or uint16 with samples in [0, maxval])"""
    h, w = p.shape
    ta, tb = torch.from_numpy(np.ascontiguousarray(p)).to(dev), torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    return float(_call(dev, ta, tb, 1, h, w, w, h * w, 1 if p.dtype == np.uint8 else 2, maxval)[0])


def _assert_rows(rows):
    for name, err, tol, extra in rows:
        print(f"{name:40s} err={err:.3e} tol={tol:.1e} {extra}")
    bad = [(r[0], r[1], r[2]) for r in rows if not r[1] <= r[2]]
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------------- SSIM
def test_ssim2d_against_float64(dev):
    """uint8 and 10-bit planes, noisy and flat, at every shape of SSIM2D_SHAPES ((17, 33) is one past the tile on both axes)"""
    _assert_rows(myc.check_ssim2d(lambda p, q, maxval: _ssim2d(dev, p, q, maxval)))


def test_ssim2d_against_the_reference_recorded_values(dev):
    z = np.load(myc.GOLDEN)
    rows = []
    for key in sorted({k.split("/")[0] for k in z.files}):
        p, q, maxval, want = z[key + "/p"], z[key + "/q"], int(z[key + "/maxval"]), float(z[key + "/ssim"])
        rows.append((key, abs(_ssim2d(dev, p, q, maxval) - want), myc.SSIM_TOL, f"reference={want:.9f}"))
    assert len(rows) == 8
    _assert_rows(rows)


@pytest.mark.parametrize("maxval", [255, 1023])
def test_ssim2d_identical_planes_batches_repeats_and_strides_are_exact(dev, maxval):
    h, w = 45, 71
    frames = [yc.random_frame(h, w, 8 if maxval == 255 else 10, 500 + i) for i in range(3)]
    other = [yc.random_frame(h, w, 8 if maxval == 255 else 10, 600 + i) for i in range(3)]
    per = frames[0].data.size  # the packed frame: Y, U, V
    dtype = 1 if maxval == 255 else 2
    ta = torch.from_numpy(np.concatenate([f.data for f in frames])).to(dev)
    tb = torch.from_numpy(np.concatenate([f.data for f in other])).to(dev)
    # identical planes: exactly 1, noisy and flat
    again = torch.from_numpy(np.concatenate([f.data for f in frames])).to(dev)  # (another buffer with the same samples)
    assert (_call(dev, ta, again, 3, h, w, w, per, dtype, maxval) == 1.0).all()
    flat = myc.flat_planes(17, 33, maxval)[1]
    assert _ssim2d(dev, flat, flat.copy(), maxval) == 1.0
    # the luma planes of a batch of packed frames in one launch (item stride = the packed frame) ...
    batch = _call(dev, ta, tb, 3, h, w, w, per, dtype, maxval)
    assert (batch < 1.0).all() and (batch > -1.0).all()
    for i in range(3):
        truth = myc.ssim2d_truth(frames[i].planes()[0], other[i].planes()[0], maxval)
        assert abs(batch[i] - truth) <= myc.SSIM_TOL, (i, batch[i], truth)
    # ... item 2 of the 3 alone: the same bits
    alone = _call(dev, ta, tb, 1, h, w, w, per, dtype, maxval, offset=per)
    assert alone.tobytes() == batch[1:2].tobytes()
    # 20 repeats: one distinct value
    assert len({_call(dev, ta, tb, 3, h, w, w, per, dtype, maxval).tobytes() for _ in range(20)}) == 1
    # a plane inside a larger buffer (row stride > W, starting at an odd sample) against its contiguous copy
    big = []
    for f in (frames[0], other[0]):
        buf = np.full((h + 4, w + 9), maxval, f.data.dtype)  # (what surrounds the plane must not matter)
        buf[2:2 + h, 3:3 + w] = f.planes()[0]
        big.append(torch.from_numpy(buf).to(dev))
    strided = _call(dev, big[0], big[1], 1, h, w, w + 9, 0, dtype, maxval, offset=2 * (w + 9) + 3)
    assert strided.tobytes() == batch[0:1].tobytes()


def test_ssim2d_fp32_planes_and_the_three_channel_kernel_on_gray_images(dev):
    """An independent cross-check: a plane p against drba_ssim3d of the [1,3,H,W] image whose three channels all hold p / maxval.
    The channel pass of a gray image is a weighted mean with weights summing to 1 within fp32 rounding; in float64 the two
    definitions differ by 2e-9."""
    lib = _lib.load()
    for maxval in (255, 1023):
        p, q = myc.noisy_planes(45, 70, maxval, 700)
        v2 = _ssim2d(dev, p, q, maxval)
        fa, fb = myc.as_unit(p, maxval)[0].to(dev), myc.as_unit(q, maxval)[0].to(dev)   # [1,H,W] fp32
        ga, gb = fa.expand(3, 45, 70)[None].contiguous(), fb.expand(3, 45, 70)[None].contiguous()
        ws = torch.empty(int(lib.drba_ssim3d_ws_floats(1, 45, 70)), dtype=torch.float32, device=dev)
        out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(lib.drba_ssim3d(_p(ga), _p(gb), _p(out), _p(ws), 1, 45, 70, 0, 1.0, ops._stream()), "drba_ssim3d")
        v3 = float(out.cpu()[0])
        print(f"maxval={maxval}: ssim2d={v2:.10f} ssim3d(gray)={v3:.10f} diff={abs(v2 - v3):.2e}")
        assert abs(v2 - v3) <= myc.SSIM_TOL
        # dtype 0: the fp32 plane itself at L = 1 is the integer plane's value (the bound test_gpu_metrics.py holds bytes scaled in
        # the kernel to against the planar / 255 frame)
        vf = float(_call(dev, fa.contiguous(), fb.contiguous(), 1, 45, 70, 70, 45 * 70, 0, 1.0)[0])
        assert abs(vf - v2) <= 1e-9
        # ... and L is the caller's: data and range scaled by 2 together change nothing but rounding
        v2x = float(_call(dev, (fa * 2).contiguous(), (fb * 2).contiguous(), 1, 45, 70, 70, 45 * 70, 0, 2.0)[0])
        assert abs(v2x - v2) <= 1e-12


# ------------------------------------------------------------------------------------------------------------- plane errors
@pytest.mark.parametrize("bits", [8, 10])
def test_yuv_clip_metrics_plane_errors_are_exact_on_the_device(dev, bits):
    """45 x 71: at 8 bits the U plane starts at the odd byte offset 3195 and V at 4023 -- the unaligned ends of the byte kernel."""
    h, w, m = 45, 71, (1 << bits) - 1
    assert (h * w, h * w + 23 * 36) == (3195, 4023)
    g = torch.Generator().manual_seed(80 + bits)
    nets = [torch.rand(1, 3, h, w, generator=g).to(dev) for _ in range(4)]
    emitted = [ops.to_out_yuv(x, (h, w), depth=8 if bits == 8 else 16) for x in nets]          # 1-D device tensors
    assert all(t.is_cuda and t.dim() == 1 and t.numel() == 4851 for t in emitted)
    host = [yc.frame_of(t.cpu().numpy(), (h, w), bits) for t in emitted]
    other = [yc.random_frame(h, w, bits, 90 + i) for i in range(3)] + [yc.frame_of(host[3].data.copy(), (h, w), bits)]
    other[3].planes()[2][22, 35] ^= 1  # the last sample of the frame, one step
    want = myc.expected_figures([f.data for f in host], [f.data for f in other], (h, w), m)
    results = []
    for form in (host, emitted):
        cm = metrics.YuvClipMetrics(capacity=3, maxval=m)  # two chunks of slots
        for a, b in zip(form, other):  # frame by frame
            cm.add(a, b, size=(h, w))
        assert len(cm) == 4
        results.append(cm.result())
    assert results[0] == results[1]  # host YuvFrames and the device tensors of ops.to_out_yuv: the same rows
    per = results[0]["per_frame"]
    assert per["max_lsb"] == want["max_lsb"] and per["differing"] == want["differing"] and per["differing"][3] == 1
    for key in ("psnr_y", "psnr_u", "psnr_v", "psnr"):
        assert per[key] == want[key], key  # host arithmetic on exact integers: the same doubles
    for i in range(4):
        assert abs(per["ssim_y"][i] - myc.ssim2d_truth(host[i].planes()[0], other[i].planes()[0], m)) <= myc.SSIM_TOL
    assert per["ssim_y"][3] == 1.0 and per["psnr_y"][3] == math.inf
    # every integer of the rows against numpy int64, through the back end itself
    be = metrics.HipBackend()
    a, b, kind, shape = metrics._yuv_pair(be, emitted[0], other[0], (h, w))
    slots = be.slots_yuv(1)
    be.measure_yuv(slots, 0, a, b, kind, shape, m, True)
    row = be.collect_yuv([slots], [1])[0]
    assert row[:3] == myc.plane_rows(host[0].data, other[0].data, (h, w))
    # the one-shot helpers
    assert metrics.psnr_yuv(host[1], other[1]) == {k: per[k][1] for k in ("psnr_y", "psnr_u", "psnr_v", "psnr")}
    assert metrics.ssim_y(emitted[1], other[1]) == per["ssim_y"][1]


def test_yuv_clip_metrics_enqueues_without_waiting(dev):
    frames = [torch.from_numpy(yc.random_frame(48, 64, 8, 95 + i).data).to(dev) for i in range(4)]
    cm = metrics.YuvClipMetrics(capacity=2)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # any synchronising call raises
    try:
        for k in range(3):
            cm.add(frames[k], frames[k + 1], size=(48, 64))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert cm.result()["frames"] == 3


# ---------------------------------------------------------------------------------------------------------- argument checks
def test_ssim2d_argument_checks_launch_nothing(dev):
    lib = _lib.load()
    t = torch.from_numpy(np.zeros(4096, np.uint16)).to(dev)
    out, ws = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(1024, dtype=torch.float32, device=dev)
    s = ops._stream()
    ops.trace_begin()
    try:
        assert lib.drba_ssim2d(_p(t), _p(t), _p(out), _p(ws), 1, 10, 16, 16, 256, 2, 1023.0, s) == -2       # H = 10
        assert lib.drba_ssim2d(_p(t), _p(t), _p(out), _p(ws), 1, 16, 10, 16, 256, 1, 255.0, s) == -2        # W = 10
        assert lib.drba_ssim2d(None, _p(t), _p(out), _p(ws), 1, 16, 16, 16, 256, 2, 1023.0, s) == -1        # null pointers
        assert lib.drba_ssim2d(_p(t), None, _p(out), _p(ws), 1, 16, 16, 16, 256, 2, 1023.0, s) == -1
        assert lib.drba_ssim2d(_p(t), _p(t), None, _p(ws), 1, 16, 16, 16, 256, 2, 1023.0, s) == -1
        assert lib.drba_ssim2d(_p(t), _p(t), _p(out), None, 1, 16, 16, 16, 256, 2, 1023.0, s) == -1
        assert lib.drba_ssim2d(_p(t), _p(t), _p(out), _p(ws), 1, 16, 16, 15, 256, 2, 1023.0, s) == -1       # stride < W
        assert lib.drba_ssim2d(_p(t, 1), _p(t), _p(out), _p(ws), 1, 16, 16, 16, 256, 2, 1023.0, s) == -1    # odd address at dtype 2
        assert lib.drba_ssim2d(_p(t), _p(t, 3), _p(out), _p(ws), 1, 16, 16, 16, 256, 2, 1023.0, s) == -1
        assert lib.drba_ssim2d(_p(t), _p(t), _p(out), _p(ws), 1, 16, 16, 16, 256, 2, 255.0, s) == -1        # maxval 255 at dtype 2
        assert lib.drba_ssim2d(_p(t), _p(t), _p(out), _p(ws), 1, 16, 16, 16, 256, 2, 65536.0, s) == -1
        assert lib.drba_ssim2d_ws_floats(1, 10, 16) == 2 and lib.drba_ssim2d_ws_floats(0, 16, 16) == 0       # (a size, never a launch)
        torch.cuda.synchronize()
    finally:
        recs = ops.trace_end()
    assert recs == [], recs
    assert float(out.abs().sum()) == 0.0
    # the same calls made well launch the tile kernel and the fixed-order sum
    ops.trace_begin()
    try:
        assert lib.drba_ssim2d(_p(t, 1), _p(t, 3), _p(out), _p(ws), 1, 16, 16, 16, 256, 1, 255.0, s) == 0   # bytes: any address
        torch.cuda.synchronize()
    finally:
        names = [r["name"] for r in ops.trace_end()]
    assert len(names) == 2 and "ssim2d_tile_kernel" in names[0] and "sum_partials_kernel" in names[1], names
    with pytest.raises(_lib.DrbaHipError):
        metrics.ssim_y(yc.random_frame(10, 16, 8, 1), yc.random_frame(10, 16, 8, 2))  # below the window: refused, not shrunk


# ------------------------------------------------------------------------------------------------------------ command lines
def _run(argv, timeout=900):
    env = dict(os.environ, DRBA_TUNE_CACHE="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "drba_amd.evaluate"] + argv, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    return r, (lines[-1] if lines else None)


_clips = {}


def _clip(bits):
    """12 frames of 128 x 192 as YuvFrames, made once per depth"""
    if bits not in _clips:
        _clips[bits] = yc.clip_from_bgr(synth.make_clip(12, 128, 192, seed=33), bits)
    return _clips[bits]


@pytest.mark.parametrize("bits", [8, 10])
def test_compare_command_line_on_y4m_clips(dev, tmp_path, bits):
    a = _clip(bits)
    b = [y4m.YuvFrame(f.data.copy(), f.height, f.width, f.depth) for f in a]
    b[5].planes()[1][7, 9] += 1  # one planted step, in U
    pa, pb, pj = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m"), str(tmp_path / "rep.json")
    myc.write_clip(pa, a)
    myc.write_clip(pb, b)
    r, line = _run(["compare", pa, pa, "--max-lsb", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(line)
    assert rep["psnr_of_mean_mse"] == "inf" and rep["mean_psnr"] == "inf" and rep["min_psnr"] == "inf"
    assert rep["min_ssim"] == 1.0 and rep["max_lsb"] == 0 and rep["total_differing"] == 0 and rep["frames"] == 12
    assert (rep["pixfmt"], rep["depth"], rep["maxval"], rep["size"]) == ("yuv420", 8 if bits == 8 else 16, (1 << bits) - 1, [128, 192])
    r, line = _run(["compare", pa, pb, "--max-lsb", "0", "--json", pj])
    assert r.returncode == 1, r.stderr[-2000:]
    rep = json.loads(line)
    assert rep["total_differing"] == 1 and rep["max_lsb"] == 1 and rep["worst_frame"] == 5 and rep["ok"] is False
    assert rep["mean_psnr_u"] == pytest.approx(metrics.psnr_of_mse(1.0 / (64 * 96), float((1 << bits) - 1)), rel=1e-12)
    assert rep["mean_psnr_y"] == "inf" and rep["mean_psnr_v"] == "inf" and rep["min_ssim"] == 1.0
    assert json.load(open(pj))["per_frame"]["differing"] == [0] * 5 + [1] + [0] * 6


class _DirectIO:
    """the hold-out procedure written out: keep every k-th frame, pair emission j with original j - half"""

    def __init__(self, src, k, m, kept, held):
        self.src, self.k, self.m, self.half = src, k, m, (k - 1) // 2
        self.src_fps, self.total_frames_count = float(src.fps), m + 1
        self.kept, self.held, self.i, self.j = kept, held, 0, 0

    def read_frame(self):
        self.i += 1
        return self.src.frame((self.i - 1) * self.k) if self.i <= self.m + 1 else None

    def write_frame(self, x):
        p = self.j - self.half
        self.j += 1
        if 0 <= p <= self.m * self.k:
            (self.kept if p % self.k == 0 else self.held).add(x, self.src.frame(p))


def test_holdout_command_line_on_a_y4m_clip_is_reproducible_and_equals_the_procedure_in_process(dev, tmp_path, monkeypatch):
    """--deterministic: two runs print the same line, and it holds the figures of interpolate_stream + YuvClipMetrics driven here
    (no winner store on either side: the mode's choices follow from the shapes alone)."""
    monkeypatch.setenv("DRBA_TUNE_CACHE", "0")
    from drba_amd import infer as drv
    from drba_amd import tune
    from drba_amd.models.utils import tools
    inp = str(tmp_path / "clip.y4m")
    myc.write_clip(inp, _clip(8))
    argv = ["holdout", "-m", "rife", "-i", inp, "-k", "3", "--deterministic"]
    r1, line1 = _run(argv)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2, line2 = _run(argv)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert line1 == line2
    rep = json.loads(line1)
    k, m = 3, 3  # 12 frames: 0, 3, 6, 9 are kept
    assert rep["k"] == k and rep["m"] == m and rep["emissions"] == k * (m + 1) and rep["frames_used"] == 10
    assert rep["kept"]["positions"] == [0, 3, 6, 9] and rep["held_out"]["positions"] == [1, 2, 4, 5, 7, 8]
    assert rep["pixfmt"] == "yuv420" and rep["depth"] == 8 and rep["kept_passthrough"] == "to_out(to_inp(frame))"
    assert "synthetic" in rep["weights"]
    assert math.isfinite(float(rep["kept"]["psnr_of_mean_mse"])) and rep["kept"]["max_lsb"] >= 1  # the chroma of kept frames is filtered
    was = ops.set_deterministic(True)
    try:
        src = evaluate.ClipSource(inp)
        model = drv.load_model("rife", scale=1.0, weights=tune._synthetic_weights("rife"))
        kept, held = metrics.YuvClipMetrics(maxval=255), metrics.YuvClipMetrics(maxval=255)
        io = _DirectIO(src, k, m, kept, held)
        n = drv.interpolate_stream(model, io, src.fps * k, times=k, to_inp=lambda fr, size: tools.to_inp(fr, size),
                                   to_out=lambda x, size: ops.to_out_yuv(x, size))
        assert n == k * (m + 1)
        for name, cm in (("kept", kept), ("held_out", held)):
            want = evaluate._jsonable(cm.result()["summary"])
            got = {key: rep[name][key] for key in want}
            assert got == json.loads(json.dumps(want)), name
    finally:
        ops.set_deterministic(was)


def test_holdout_command_line_on_a_10_bit_y4m_clip(dev, tmp_path):
    inp, pj = str(tmp_path / "clip.y4m"), str(tmp_path / "rep.json")
    myc.write_clip(inp, _clip(10)[:7], color_range="FULL")
    r, line = _run(["holdout", "-m", "rife", "-i", inp, "-k", "3", "--plain", "--yuv-matrix", "bt601", "--json", pj])
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(line)
    assert rep["emissions"] == 9 and rep["m"] == 2 and rep["plain"] is True and rep["depth"] == 16 and rep["maxval"] == 1023
    assert rep["yuv_matrix"] == "bt601" and rep["full_range"] is True and rep["chroma"] == "420p10"
    assert rep["kept"]["frames"] == 3 and rep["held_out"]["frames"] == 4
    for part in ("kept", "held_out"):
        for key in ("mean_psnr", "psnr_of_mean_mse", "mean_psnr_u", "mean_psnr_v", "mean_ssim", "min_ssim"):
            assert math.isfinite(float(rep[part][key])), (part, key)  # (kept frames too: their chroma is filtered)
        assert not math.isnan(float(rep[part]["mean_psnr_y"]))  # (luma may pass through untouched: inf)
    assert float(rep["kept"]["mean_psnr_y"]) > float(rep["held_out"]["mean_psnr_y"])  # a passed-through frame beats an interpolated one
    full = json.load(open(pj))
    assert full["pairs"] == [[j, j - 1] for j in range(1, 8)] and len(full["per_frame"]["held_out"]["ssim_y"]) == 4
    r, _ = _run(["holdout", "-m", "rife", "-i", inp, "-k", "4"])
    assert r.returncode == 2 and "even" in r.stderr
