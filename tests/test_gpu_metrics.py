"""GPU: the picture-metric kernels (metrics.hip) against float64, their exactness properties, the public interface of
drba_amd.metrics and the two commands of drba_amd.evaluate.  The rows and their references live in tests/metric_checks.py."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from drba_amd import _lib, metrics, ops
from drba_amd.utils import synth
from tests import cases
from tests import metric_checks as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _ssim(dev, a, b, val_range=0.0, dtype=0):
    """drba_ssim3d on device copies of a, b (fp32 [N,3,H,W], or uint8 [N,H,W,3] with dtype = 1) -> float64 [N]"""
    lib = _lib.load()
    a, b = a.to(dev).contiguous(), b.to(dev).contiguous()
    n, h, w = (a.shape[0], a.shape[2], a.shape[3]) if dtype == 0 else a.shape[:3]
    ws = torch.empty(max(int(lib.drba_ssim3d_ws_floats(n, h, w)), 1), dtype=torch.float32, device=dev)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    _lib.check(lib.drba_ssim3d(_p(a), _p(b), _p(out), _p(ws), n, h, w, dtype, float(val_range), ops._stream()), "drba_ssim3d")
    return out.cpu().numpy()


def _assert_rows(rows):
    for name, err, tol, extra in rows:
        print(f"{name:60s} err={err:.3e} tol={tol:.1e} {extra}")
    bad = [(r[0], r[1], r[2]) for r in rows if not r[1] <= r[2]]
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------------- SSIM
def test_ssim3d_against_float64(dev):
    _assert_rows(mc.check_ssim(lambda a, b, vr: _ssim(dev, a, b, vr)))


def test_ssim3d_identical_inputs_batches_and_repeats_are_exact(dev):
    items = [mc.noise_pair(45, 70, 1), mc.synth_pair(45, 70), mc.flat_pair(45, 70)]
    a, b = torch.cat([p[0] for p in items]), torch.cat([p[1] for p in items])
    for x in (a, a * 255.0, a * 2 - 1, mc.noise_pair(270, 480, 2)[0], mc.flat_pair(17, 33)[0]):
        assert (_ssim(dev, x, x.clone()) == 1.0).all()                      # exactly 1, whatever the range rule picks
    u8 = torch.from_numpy(np.stack(mc.synth_pair_u8(45, 70)))
    assert (_ssim(dev, u8, u8.clone(), dtype=1) == 1.0).all()
    batch = _ssim(dev, a, b)
    single = np.concatenate([_ssim(dev, a[i:i + 1], b[i:i + 1]) for i in range(3)])
    assert batch.tobytes() == single.tobytes()                                # an item alone = the item in a batch, bit for bit
    assert batch.tobytes() == _ssim(dev, a, b).tobytes()                      # and the same bits on every run
    big = mc.noise_pair(270, 480, 3)
    assert _ssim(dev, *big).tobytes() == _ssim(dev, *big).tobytes()
    assert (batch < 1.0).all() and (batch > 0.0).all()


def test_ssim3d_channel_order_and_input_forms(dev):
    for h, w in ((13, 37), (45, 70)):
        a, b = mc.synth_pair(h, w)
        v = _ssim(dev, a, b)[0]
        assert abs(_ssim(dev, a.flip(1), b.flip(1))[0] - v) <= 1e-12 * abs(v)   # the window is symmetric: BGR = RGB
        a8, b8 = mc.synth_pair_u8(h, w)
        v8 = _ssim(dev, torch.from_numpy(a8)[None], torch.from_numpy(b8)[None], dtype=1)[0]
        assert abs(v8 - v) <= 1e-9                                               # bytes scaled in the kernel = the planar /255 frame


def test_ssim3d_agrees_with_the_scene_detector_on_its_thumbnails(dev, golden_dir):
    """3 x 32 x 32 on the scdet.npz thumbnails: within 1e-5 of ops.ssim_thumb32, the bound that kernel is held to against its
    golden values (the detector keeps the reference's fp32 arithmetic; on textured thumbnails the two agree)."""
    z = np.load(os.path.join(golden_dir, "scdet.npz"))
    T = cases.scdet_frames()
    for k, (i, j) in enumerate(cases.SCDET_PAIRS):
        x1, x2 = T[i].to(dev), T[j].to(dev)
        thumb = ops.ssim_thumb32(x1, x2)
        full = _ssim(dev, ops.resize_bilinear(x1, (32, 32)), ops.resize_bilinear(x2, (32, 32)))[0]
        print(f"pair {k}: ssim3d={full:.8f} thumb32={thumb:.8f} golden={float(z['ssim/values'][k]):.8f}")
        assert abs(full - thumb) <= 1e-5


# -------------------------------------------------------------------------------------------------------- frame differences
def test_frame_error_u8_is_bit_exact(dev):
    lib = _lib.load()

    def fn(a, b, N, n, off_a, off_b):
        bufs = []
        for x, off in ((a, off_a), (b, off_b)):
            t = torch.zeros(off + N * n + 64, dtype=torch.uint8, device=dev)
            t[off:off + N * n] = torch.from_numpy(x).to(dev)
            bufs.append(t[off:off + N * n])
            assert bufs[-1].data_ptr() % 16 == off % 16
        ws = torch.empty(int(lib.drba_frame_error_ws_floats(N, n)), dtype=torch.float32, device=dev)
        out = torch.full((N, 4), -1, dtype=torch.int64, device=dev)
        _lib.check(lib.drba_frame_error_u8(_p(bufs[0]), _p(bufs[1]), _p(out), _p(ws), N, n, ops._stream()), "drba_frame_error_u8")
        return out.cpu().numpy()

    _assert_rows(mc.check_frame_error_u8(fn))


def test_frame_error_f32_against_float64(dev):
    lib = _lib.load()

    def fn(a, b, N, n):
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        ws = torch.empty(int(lib.drba_frame_error_ws_floats(N, n)), dtype=torch.float32, device=dev)
        out = torch.full((N, 4), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(lib.drba_frame_error_f32(_p(ta), _p(tb), _p(out), _p(ws), N, n, ops._stream()), "drba_frame_error_f32")
        again = torch.full((N, 4), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(lib.drba_frame_error_f32(_p(ta), _p(tb), _p(again), _p(ws), N, n, ops._stream()), "drba_frame_error_f32")
        h = out.cpu().numpy()
        assert h.tobytes() == again.cpu().numpy().tobytes()  # fixed summation order
        return h[:, :3], h[:, 3].view(np.int64)

    _assert_rows(mc.check_frame_error_f32(fn))


# --------------------------------------------------------------------------------------------------------- public interface
def test_metrics_functions_take_host_and_device_frames(dev):
    a8, b8 = mc.synth_pair_u8(45, 70)
    d = np.abs(a8.astype(np.int64) - b8.astype(np.int64))
    want = {"sum_sq": int((d * d).sum()), "sum_abs": int(d.sum()), "max_abs": int(d.max()), "differing": int((d != 0).sum()), "n": d.size}
    truth = float(mc.ssim_truth(mc.planar(a8), mc.planar(b8))[0])
    for a, b in ((a8, b8), (torch.from_numpy(a8), torch.from_numpy(b8)), (torch.from_numpy(a8).to(dev), torch.from_numpy(b8).to(dev))):
        assert metrics.frame_error(a, b) == want
        p = metrics.psnr(a, b)
        assert isinstance(p, float) and p == metrics.psnr_of_mse(want["sum_sq"] / d.size, 255.0)
        s = metrics.ssim(a, b)
        assert isinstance(s, float) and abs(s - truth) <= mc.SSIM_TOL
    assert metrics.psnr(a8, a8) == math.inf and metrics.ssim(a8, a8) == 1.0
    fa, fb = mc.planar(a8), mc.planar(b8)
    assert abs(metrics.ssim(fa, fb) - truth) <= mc.SSIM_TOL and abs(metrics.ssim(fa, fb, val_range=1.0) - truth) <= mc.SSIM_TOL
    mse = float(((fa.double() - fb.double()) ** 2).mean())
    assert metrics.psnr(fa, fb) == pytest.approx(10 * math.log10(1.0 / mse), rel=1e-12)
    assert metrics.psnr(fa, fb, peak=2.0) == pytest.approx(10 * math.log10(4.0 / mse), rel=1e-12)
    e = metrics.frame_error(fa, fb)
    assert e["nonfinite"] == 0 and e["max_abs"] == float((fa.double() - fb.double()).abs().max())
    with pytest.raises(_lib.DrbaHipError):
        metrics.ssim(a8[:10], b8[:10])  # below the window: refused, not shrunk


def test_clip_metrics_enqueues_without_waiting_and_reads_once(dev):
    frames = [torch.from_numpy(f).to(dev) for f in synth.make_clip(5, 64, 96, seed=5)]
    cm = metrics.ClipMetrics(capacity=2)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # any synchronising call raises
    try:
        for k in range(4):
            cm.add(frames[k], frames[k + 1])
        cm.add(frames[0], frames[0])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    r = cm.result()
    host = [f.cpu().numpy() for f in frames]
    for k in range(4):
        d = np.abs(host[k].astype(np.int64) - host[k + 1].astype(np.int64))
        assert r["per_frame"]["differing"][k] == int((d != 0).sum()) and r["per_frame"]["max_lsb"][k] == int(d.max())
        assert r["per_frame"]["psnr"][k] == metrics.psnr_of_mse(float((d * d).mean()), 255.0)
        assert abs(r["per_frame"]["ssim"][k] - float(mc.ssim_truth(mc.planar(host[k]), mc.planar(host[k + 1]))[0])) <= mc.SSIM_TOL
    assert r["per_frame"]["psnr"][4] == math.inf and r["per_frame"]["ssim"][4] == 1.0 and r["frames"] == 5
    assert r["summary"]["worst_frame"] == int(np.argmin(r["per_frame"]["psnr"]))


# -------------------------------------------------------------------------------------------------------------- command lines
def _run(argv, timeout=900):
    env = dict(os.environ, DRBA_TUNE_CACHE="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "drba_amd.evaluate"] + argv, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


def test_compare_command_line(dev, tmp_path):
    a = np.stack(synth.make_clip(6, 64, 96, seed=77))
    b = a.copy()
    b[1, 3, 5, 0] ^= 1                      # one byte, 1 LSB
    b[2, 10:20, 30:50, :] //= 2             # a darkened block
    b[4, ::2, ::2, 1] = np.minimum(b[4, ::2, ::2, 1].astype(np.int64) + 3, 255).astype(np.uint8)
    pa, pb, pj = str(tmp_path / "a.npz"), str(tmp_path / "b.npz"), str(tmp_path / "rep.json")
    np.savez(pa, frames=a, fps=np.float64(24.0))
    np.savez(pb, frames=b, fps=np.float64(24.0))
    r, rep = _run(["compare", pa, pb, "--json", pj, "--max-lsb", "255", "--min-psnr", "5", "--min-ssim", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.abs(a.astype(np.int64) - b.astype(np.int64)).reshape(6, -1)
    mse = (d * d).mean(1)
    psnr = [metrics.psnr_of_mse(float(v), 255.0) for v in mse]
    ssim = [float(mc.ssim_truth(mc.planar(a[k]), mc.planar(b[k]))[0]) for k in range(6)]
    fin = [p for p in psnr if math.isfinite(p)]
    assert rep["frames"] == 6 and rep["size"] == [64, 96] and rep["ok"] is True
    assert rep["max_lsb"] == int(d.max()) and rep["total_differing"] == int((d != 0).sum())
    assert rep["mean_psnr"] == pytest.approx(sum(fin) / len(fin), rel=1e-12) and rep["min_psnr"] == pytest.approx(min(psnr), rel=1e-12)
    assert rep["psnr_of_mean_mse"] == pytest.approx(metrics.psnr_of_mse(float(mse.mean()), 255.0), rel=1e-12)
    assert abs(rep["mean_ssim"] - sum(ssim) / 6) <= mc.SSIM_TOL and abs(rep["min_ssim"] - min(ssim)) <= mc.SSIM_TOL
    assert rep["worst_frame"] == int(np.argmin(psnr))
    full = json.load(open(pj))["per_frame"]
    assert [float(v) for v in full["psnr"]] == pytest.approx(psnr, rel=1e-12) and full["psnr"][0] == "inf"
    assert full["differing"] == (d != 0).sum(1).tolist() and full["max_lsb"] == d.max(1).tolist()
    assert np.abs(np.array(full["ssim"]) - np.array(ssim)).max() <= mc.SSIM_TOL and full["ssim"][0] == 1.0
    # each gate on its own, violated: a non-zero exit that names it (one child process runs the three command lines)
    gates = [(["--max-lsb", "1"], "max_lsb"), (["--min-psnr", f"{min(psnr) + 0.5}"], "min_psnr"), (["--min-ssim", f"{min(ssim) + 0.01}"], "min_ssim")]
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from drba_amd import evaluate\n"
            "for argv in %r:\n"
            "    print('exit', evaluate.main(['compare', %r, %r] + argv))\n" % (ROOT, [g[0] for g in gates], pa, pb))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert [ln for ln in lines if ln.startswith("exit")] == ["exit 1"] * 3
    for (argv, gate), rep in zip(gates, [json.loads(ln) for ln in lines if ln.startswith("{")]):
        assert rep["ok"] is False and list(rep["gates"]) == [gate] and rep["gates"][gate]["ok"] is False


@pytest.mark.parametrize("plain", [False, True])
def test_holdout_command_line(dev, tmp_path, plain):
    """Synthetic weights (no weight directory here): the positions, the pass-through of the kept frames and the finiteness of the
    report are checked -- no quality."""
    frames = np.stack(synth.make_clip(7, 128, 192, seed=9))
    inp, pj = str(tmp_path / "in.npz"), str(tmp_path / "rep.json")
    np.savez(inp, frames=frames, fps=np.float64(24.0))
    r, rep = _run(["holdout", "-m", "rife", "-i", inp, "-k", "3", "--json", pj] + (["--plain"] if plain else []))
    assert r.returncode == 0, r.stderr[-2000:]
    assert rep["k"] == 3 and rep["m"] == 2 and rep["frames_used"] == 7 and rep["emissions"] == 9 and rep["plain"] is plain
    assert rep["held_out"]["positions"] == [1, 2, 4, 5] and rep["held_out"]["frames"] == 4
    assert rep["kept"]["positions"] == [0, 3, 6] and rep["kept"]["frames"] == 3
    assert "synthetic" in rep["weights"]
    assert rep["kept"]["max_lsb"] <= 1  # pass-through frames: the conversion round trip stays within 1 LSB
    for part in ("kept", "held_out"):
        for key in ("mean_psnr", "psnr_of_mean_mse", "mean_ssim", "min_ssim", "max_lsb"):
            v = float(rep[part][key])
            assert math.isfinite(v) or v == math.inf, (part, key, v)
    full = json.load(open(pj))
    assert full["pairs"] == [[j, j - 1] for j in range(1, 8)]
    assert len(full["per_frame"]["held_out"]["psnr"]) == 4 and len(full["per_frame"]["kept"]["ssim"]) == 3
    if not plain:
        r, _ = _run(["holdout", "-m", "rife", "-i", inp, "-k", "4"])
        assert r.returncode == 2 and "even" in r.stderr
