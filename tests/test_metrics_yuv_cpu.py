"""CPU (-m "not gpu"): the host side of the YUV4MPEG2 metrics -- the random-access reader of drba_amd/y4m.py, YuvClipMetrics over a
numpy stand-in back end (with and without a planted defect), `compare` and `holdout` of drba_amd.evaluate on .y4m clips, the
argument checks of drba_ssim2d, and the array path of `compare` byte for byte as it was."""
import ctypes as C
import io
import json
import math

import numpy as np
import pytest
import torch

from drba_amd import _lib, evaluate, metrics, y4m
from tests import metric_checks as mc
from tests import metrics_yuv_common as myc
from tests import yuv_common as yc


# ------------------------------------------------------------------------------------------------- the random-access reader
class _Pipe:
    """a file object that reads but cannot seek"""

    def __init__(self, data):
        self._f = io.BytesIO(data)

    def read(self, n=-1):
        return self._f.read(n)

    def readline(self, n=-1):
        return self._f.readline(n)

    def readinto(self, b):
        return self._f.readinto(b)

    def seekable(self):
        return False


@pytest.mark.parametrize("bits", [8, 10])
def test_indexed_reader_returns_the_frames_of_the_sequential_reader(bits):
    frames = myc.random_clip(5, 13, 19, bits, seed=40)
    data = myc.write_clip(None, frames, frame_params={1: b"Ip", 3: b"Xnote=1 Ip"})  # offsets are not uniform
    seq = list(y4m.Reader(io.BytesIO(data)))
    assert len(seq) == 5 and all(np.array_equal(s.data, f.data) for s, f in zip(seq, frames))
    r = y4m.IndexedReader(io.BytesIO(data))
    assert len(r) == 5 and r.header == y4m.Reader(io.BytesIO(data)).header
    for k in (4, 0, 2, 2, 1, 3):  # by index, out of order
        f = r.read_frame(k)
        assert isinstance(f, y4m.YuvFrame) and f.depth == bits and f.shape == (13, 19, 3) and np.array_equal(f.data, frames[k].data), k
    assert [np.array_equal(f.data, g.data) for f, g in zip(r, frames)] == [True] * 5
    for k in (-1, 5):
        with pytest.raises(IndexError):
            r.read_frame(k)
    # a uniform-offset guess would have been wrong here
    assert r._offsets[2] - r._offsets[1] != r._offsets[1] - r._offsets[0]


def test_indexed_reader_refuses_pipes_and_truncated_clips():
    frames = myc.random_clip(3, 12, 16, 8, seed=41)
    data = myc.write_clip(None, frames)
    with pytest.raises(y4m.Y4MError, match="seekable"):
        y4m.IndexedReader(_Pipe(data))
    assert len(list(y4m.Reader(_Pipe(data)))) == 3  # (the sequential reader does read it)
    with pytest.raises(y4m.Y4MError, match="frame 2 is truncated"):
        y4m.IndexedReader(io.BytesIO(data[:-7]))
    with pytest.raises(y4m.Y4MError, match="FRAME"):
        y4m.IndexedReader(io.BytesIO(data + b"FRAM"))
    assert len(y4m.IndexedReader(io.BytesIO(data[:len(y4m.Header(16, 12).format())]))) == 0  # a header alone: no frames


# ---------------------------------------------------------------------------------------------------------- YuvClipMetrics
def _pairs(bits, n=4, h=13, w=19, seed=50):
    a = myc.random_clip(n, h, w, bits, seed)
    b = [y4m.YuvFrame(f.data.copy(), h, w, bits) for f in a]
    m = (1 << bits) - 1
    rng = np.random.default_rng(seed)
    b[1].data[:] = np.clip(b[1].data.astype(np.int64) + rng.integers(-3, 4, b[1].data.size), 0, m).astype(b[1].data.dtype)
    yb, ub, vb = b[2].planes()
    vb[2, 3] ^= 1                                  # one step in V
    ub[:] = np.clip(ub.astype(np.int64) + 9, 0, m)  # U off by up to 9: U and V differ, so a swap shows
    return a, b                                    # frames 0 and 3 identical


@pytest.mark.parametrize("bits", [8, 10])
def test_yuv_clip_metrics_against_numpy(bits):
    a, b = _pairs(bits)
    m = (1 << bits) - 1
    cm = metrics.YuvClipMetrics(backend=myc.NumpyYuvBackend(), capacity=3, maxval=m)  # two chunks of slots
    for fa, fb in zip(a[:2], b[:2]):
        cm.add(fa, fb)
    cm.add(a[2].data, b[2], size=None)            # packed planes beside a YuvFrame: the size comes from the frame
    cm.add(a[3].data, b[3].data, size=(13, 19))   # two packed arrays with their size
    assert len(cm) == 4
    r = cm.result()
    want = myc.expected_figures([f.data for f in a], [f.data for f in b], (13, 19), m)
    per = r["per_frame"]
    assert per["max_lsb"] == want["max_lsb"] and per["differing"] == want["differing"]   # integers: exactly
    for key in ("psnr_y", "psnr_u", "psnr_v", "psnr"):
        for got, exp in zip(per[key], want[key]):
            assert got == exp if math.isinf(exp) else abs(got - exp) <= 1e-12 * abs(exp), (key, got, exp)
    assert r["peak"] == float(m) and r["frames"] == 4
    # identical frames: inf / 1.0 / 0 / 0
    for i in (0, 3):
        assert per["psnr"][i] == per["psnr_y"][i] == per["psnr_u"][i] == per["psnr_v"][i] == math.inf
        assert per["ssim_y"][i] == 1.0 and per["max_lsb"][i] == 0 and per["differing"][i] == 0
    assert per["psnr_y"][2] == math.inf and math.isfinite(per["psnr_v"][2]) and per["ssim_y"][2] == 1.0  # luma untouched there
    assert per["ssim_y"][1] < 1.0
    s = r["summary"]
    fin = [v for v in want["psnr"] if math.isfinite(v)]
    assert s["mean_psnr"] == pytest.approx(sum(fin) / len(fin), rel=1e-12)
    d = [np.abs(fa.data.astype(np.int64) - fb.data.astype(np.int64)) for fa, fb in zip(a, b)]
    assert s["psnr_of_mean_mse"] == pytest.approx(metrics.psnr_of_mse(float(sum((x * x).sum() for x in d)) / sum(x.size for x in d), float(m)), rel=1e-12)
    ny = 13 * 19
    assert s["psnr_of_mean_mse_y"] == pytest.approx(metrics.psnr_of_mse(float(sum((x[:ny] ** 2).sum() for x in d)) / (4 * ny), float(m)), rel=1e-12)
    assert s["max_lsb"] == max(want["max_lsb"]) and s["total_differing"] == sum(want["differing"])
    assert s["worst_frame"] == int(np.argmin(want["psnr"])) and s["min_ssim"] == min(per["ssim_y"])
    assert s["mean_ssim"] == pytest.approx(sum(per["ssim_y"]) / 4, rel=1e-15)
    assert set(s) == {"mean_psnr", "psnr_of_mean_mse", "mean_ssim", "min_ssim", "max_lsb", "total_differing", "worst_frame"} | \
        {f"{k}_{p}" for k in ("mean_psnr", "psnr_of_mean_mse") for p in "yuv"}
    # the one-shot helpers over the same back end
    be = myc.NumpyYuvBackend()
    one = metrics.psnr_yuv(a[1], b[1], backend=be)
    assert one == {k: per[k][1] for k in ("psnr_y", "psnr_u", "psnr_v", "psnr")}
    assert metrics.ssim_y(a[1], b[1], backend=be) == per["ssim_y"][1]
    assert metrics.ssim_y(a[0].data, a[0].data.copy(), size=(13, 19), backend=be, maxval=m) == 1.0
    with pytest.raises(ValueError, match="size"):
        metrics.ssim_y(a[0].data, a[0].data, backend=be)
    with pytest.raises(ValueError):
        cm.add(a[0], yc.random_frame(13, 21, bits, 1))   # another size
    with pytest.raises(ValueError):
        cm.add(yc.random_frame(13, 19, 18 - bits, 1), yc.random_frame(13, 19, 18 - bits, 1))   # another depth in the same clip


def test_yuv_rows_fail_for_a_back_end_that_swaps_u_and_v():
    a, b = _pairs(8)
    good, bad = metrics.YuvClipMetrics(backend=myc.NumpyYuvBackend()), metrics.YuvClipMetrics(backend=myc.NumpyYuvBackend(swap_uv=True))
    for fa, fb in zip(a, b):
        good.add(fa, fb)
        bad.add(fa, fb)
    g, w = good.result()["per_frame"], bad.result()["per_frame"]
    want = myc.expected_figures([f.data for f in a], [f.data for f in b], (13, 19), 255)
    assert g["psnr_u"] == pytest.approx(want["psnr_u"], rel=1e-12) and g["psnr_v"] == pytest.approx(want["psnr_v"], rel=1e-12)
    assert w["psnr_u"] != pytest.approx(want["psnr_u"], rel=1e-12) and w["psnr_u"] == g["psnr_v"]
    assert w["psnr"] == g["psnr"]  # (the pooled figure cannot see the swap: equal plane sizes)


def test_ssim2d_truth_agrees_with_the_reference_fixture_and_fp32_fails_on_flat_content():
    """the dense float64 restatement against the reference's own ssim() recorded in the fixture (4e-10), and the rows CAN fail: the
    fp32 evaluation of the formula misses the bar on every flat pair and meets it on every noisy one"""
    z = np.load(myc.GOLDEN)
    keys = sorted({k.split("/")[0] for k in z.files})
    assert len(keys) == 8
    for key, p, q, maxval in myc.golden_pairs():
        assert np.array_equal(z[key + "/p"], p) and np.array_equal(z[key + "/q"], q) and int(z[key + "/maxval"]) == maxval
        assert max(p.shape) <= 70 and min(p.shape) <= 45
        assert abs(float(z[key + "/ssim"]) - myc.ssim2d_truth(p, q, maxval)) <= 4e-10, key
    bad = [r[0] for r in myc.check_ssim2d(myc.ssim2d_fp32) if not r[1] <= r[2]]
    flat = [c[0] for c in myc.ssim2d_cases() if c[0].endswith("flat")]
    assert sorted(bad) == sorted(flat) and len(flat) == 2 * len(myc.SSIM2D_SHAPES), bad
    assert not [r for r in myc.check_ssim2d(myc.ssim2d_truth) if not r[1] <= r[2]]


# ------------------------------------------------------------------------------------------------------------- entry points
def test_ssim2d_entry_points_validate_arguments_without_gpu():
    lib = _lib.load()
    buf = torch.zeros(4096)
    p = C.c_void_p(buf.data_ptr())
    odd = C.c_void_p(buf.data_ptr() + 1)
    ok = (1, 16, 16, 16, 256)  # N, H, W, row stride, item stride
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.drba_ssim2d(*args, *ok, 1, 255.0, None) == -1
    assert lib.drba_ssim2d(p, p, p, p, 0, 16, 16, 16, 256, 1, 255.0, None) == -1
    assert lib.drba_ssim2d(p, p, p, p, 1, 16, 16, 15, 256, 1, 255.0, None) == -1      # row stride < W
    assert lib.drba_ssim2d(p, p, p, p, *ok, 3, 255.0, None) == -1                      # unknown dtype
    assert lib.drba_ssim2d(p, p, p, p, *ok, 1, 1023.0, None) == -1                     # bytes have maxval 255
    assert lib.drba_ssim2d(odd, p, p, p, *ok, 2, 1023.0, None) == -1                   # uint16 planes: 2-byte aligned
    assert lib.drba_ssim2d(p, odd, p, p, *ok, 2, 1023.0, None) == -1
    for mv in (255.0, 65536.0, 1023.5, 0.0, float("nan")):
        assert lib.drba_ssim2d(p, p, p, p, *ok, 2, mv, None) == -1, mv                 # maxval outside (255, 65535]
    for vr in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.drba_ssim2d(p, p, p, p, *ok, 0, vr, None) == -1, vr                 # fp32: L is the caller's
    for h, w in ((10, 16), (16, 10), (1, 1)):
        for dtype, mv in ((0, 1.0), (1, 255.0), (2, 1023.0)):
            assert lib.drba_ssim2d(p, p, p, p, 1, h, w, 16, 256, dtype, mv, None) == -2   # the reference shrinks its window there
    assert lib.drba_ssim2d_ws_floats(2, 17, 33) == 2 * 4 * 2
    assert lib.drba_ssim2d_ws_floats(1, 1080, 1920) == 60 * 68 * 2
    assert lib.drba_ssim2d_ws_floats(0, 16, 16) == 0
    assert _lib.ABI_VERSION == 16


def test_yuv_metrics_have_no_cpu_fallback():
    if not torch.cuda.is_available():
        f = yc.random_frame(16, 16, 8, 1)
        with pytest.raises(_lib.DrbaHipError):
            metrics.ssim_y(f, f)


# ------------------------------------------------------------------------------------------------------------------ compare
def _last_json(capsys):
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _copy(frames):
    return [y4m.YuvFrame(f.data.copy(), f.height, f.width, f.depth) for f in frames]


@pytest.mark.parametrize("bits", [8, 10])
def test_compare_y4m_gates_and_exit_codes(tmp_path, capsys, bits):
    a = myc.random_clip(4, 14, 22, bits, seed=60)
    b = _copy(a)
    b[2].planes()[2][3, 4] ^= 1  # one sample of V, one step
    pa, pa2, pb, pj = (str(tmp_path / n) for n in ("a.y4m", "a2.y4m", "b.y4m", "rep.json"))
    myc.write_clip(pa, a, frame_params={1: b"Ip"})
    myc.write_clip(pa2, a)
    myc.write_clip(pb, b)
    be = myc.NumpyYuvBackend()
    assert evaluate.main(["compare", pa, pa2, "--max-lsb", "0", "--min-ssim", "1", "--min-psnr", "200"], backend=be) == 0
    rep = _last_json(capsys)
    assert rep["psnr_of_mean_mse"] == "inf" and rep["mean_psnr"] == "inf" and rep["min_psnr"] == "inf"
    assert rep["max_lsb"] == 0 and rep["total_differing"] == 0 and rep["min_ssim"] == 1.0 and rep["ok"] is True
    assert rep["pixfmt"] == "yuv420" and rep["depth"] == (8 if bits == 8 else 16) and rep["maxval"] == (1 << bits) - 1
    assert rep["peak"] == float((1 << bits) - 1) and rep["size"] == [14, 22] and rep["frames"] == 4
    assert evaluate.main(["compare", pa, pb, "--max-lsb", "0"], backend=be) == 1
    rep = _last_json(capsys)
    assert rep["total_differing"] == 1 and rep["max_lsb"] == 1 and rep["gates"]["max_lsb"]["ok"] is False and rep["worst_frame"] == 2
    assert rep["mean_psnr_y"] == "inf" and rep["mean_psnr_u"] == "inf" and math.isfinite(rep["mean_psnr_v"])
    n_all = 14 * 22 + 2 * 7 * 11
    assert rep["min_psnr"] == pytest.approx(metrics.psnr_of_mse(1.0 / n_all, float((1 << bits) - 1)), rel=1e-12)
    assert rep["mean_psnr_v"] == pytest.approx(metrics.psnr_of_mse(1.0 / 77, float((1 << bits) - 1)), rel=1e-12)
    assert evaluate.main(["compare", pa, pb, "--max-lsb", "1", "--json", pj], backend=be) == 0
    assert _last_json(capsys)["total_differing"] == 1
    full = json.load(open(pj))["per_frame"]
    assert set(full) == {"psnr_y", "psnr_u", "psnr_v", "psnr", "ssim_y", "max_lsb", "differing"}
    assert full["differing"] == [0, 0, 1, 0] and full["psnr"][0] == "inf" and len(full["ssim_y"]) == 4
    # the other two gates on the lowest per-frame pooled psnr and the lowest ssim_y
    assert evaluate.main(["compare", pa, pb, "--min-psnr", "200"], backend=be) == 1
    assert _last_json(capsys)["gates"]["min_psnr"]["ok"] is False
    b[1].planes()[0][:] = (1 << bits) - 1 - b[1].planes()[0]
    myc.write_clip(pb, b)
    assert evaluate.main(["compare", pa, pb, "--min-ssim", "0.9"], backend=be) == 1
    rep = _last_json(capsys)
    assert rep["gates"]["min_ssim"]["ok"] is False and rep["gates"]["min_ssim"]["value"] == rep["min_ssim"] < 0.9


def test_compare_y4m_refusals_name_both_sides(tmp_path, capsys):
    a8 = myc.random_clip(3, 14, 22, 8, seed=61)
    paths = {n: str(tmp_path / (n + ".y4m")) for n in ("a", "small", "deep", "full", "limited", "mpeg2", "short")}
    myc.write_clip(paths["a"], a8)
    myc.write_clip(paths["small"], myc.random_clip(3, 12, 22, 8, seed=62))
    myc.write_clip(paths["deep"], myc.random_clip(3, 14, 22, 10, seed=63))
    myc.write_clip(paths["full"], a8, color_range="FULL")
    myc.write_clip(paths["limited"], a8, color_range="LIMITED")
    myc.write_clip(paths["mpeg2"], a8, chroma="420mpeg2")
    myc.write_clip(paths["short"], a8[:2])
    npz = str(tmp_path / "a.npz")
    np.savez(npz, frames=np.zeros((3, 14, 22, 3), np.uint8))
    be = myc.NumpyYuvBackend()
    for other, word in (("small", "frame size"), ("deep", "depth"), ("full", "sample range"), ("short", "length")):
        assert evaluate.main(["compare", paths["a"], paths[other]], backend=be) == 2, other
        err = capsys.readouterr().err
        assert word in err and paths["a"] in err and paths[other] in err, err
    for argv in ([paths["a"], npz], [npz, paths["a"]]):
        assert evaluate.main(["compare"] + argv, backend=be) == 2
        err = capsys.readouterr().err
        assert "convert one of them first" in err and paths["a"] in err and npz in err, err
    # no XCOLORRANGE tag is limited range; two sitings of 4:2:0 may be compared and both tags are reported
    assert evaluate.main(["compare", paths["a"], paths["limited"], "--max-lsb", "0"], backend=be) == 0
    assert _last_json(capsys)["color_range"] == "LIMITED"
    assert evaluate.main(["compare", paths["a"], paths["mpeg2"], "--max-lsb", "0"], backend=be) == 0
    rep = _last_json(capsys)
    assert rep["chroma"] == ["420jpeg", "420mpeg2"] and rep["total_differing"] == 0


def test_compare_y4m_reads_a_stream_from_stdin(tmp_path, capsys, monkeypatch):
    a = myc.random_clip(3, 14, 22, 8, seed=64)
    pa = str(tmp_path / "a.y4m")
    data = myc.write_clip(pa, a)

    class _Stdin:
        buffer = _Pipe(data)

    monkeypatch.setattr(evaluate.sys, "stdin", _Stdin())
    assert evaluate.main(["compare", pa, "-", "--max-lsb", "0"], backend=myc.NumpyYuvBackend()) == 0
    assert _last_json(capsys)["frames"] == 3


def test_clip_source_of_a_y4m_file(tmp_path):
    a = myc.random_clip(4, 14, 22, 10, seed=65)
    pa = str(tmp_path / "a.y4m")
    myc.write_clip(pa, a, color_range="FULL", fps=(30000, 1001))
    src = evaluate.ClipSource(pa)
    assert (src.pixfmt, src.depth, src.maxval, src.random_access, len(src)) == ("yuv420", 16, 1023, True, 4)
    assert src.fps == pytest.approx(30000 / 1001) and src.color_range == "FULL" and src.chroma == "420p10" and src.size == (14, 22)
    assert np.array_equal(src.frame(3).data, a[3].data) and [np.array_equal(f.data, g.data) for f, g in zip(src, a)] == [True] * 4
    npz = str(tmp_path / "a.npz")
    np.savez(npz, frames=np.zeros((2, 4, 4, 3), np.uint8))
    assert evaluate.ClipSource(npz).pixfmt == "bgr"


# The JSON line of `compare a.npz b.npz --max-lsb 1` on the clips of _array_clips with the numpy stand-in, recorded from the commit
# before the YUV4MPEG2 path existed
ARRAY_LINE = ('{"command": "compare", "a": "a.npz", "b": "b.npz", "frames": 4, "size": [16, 20], "peak": 255.0, "mean_psnr": '
              '48.01493441804513, "psnr_of_mean_mse": 24.09694834276194, "mean_ssim": 0.9771943061428106, "min_ssim": '
              '0.908777380888231, "max_lsb": 237, "total_differing": 49, "worst_frame": 2, "min_psnr": 18.076352897015465, "gates": '
              '{"max_lsb": {"limit": 1.0, "value": 237, "ok": false}}, "ok": false}')


def test_compare_on_array_clips_prints_the_line_it_printed_before(tmp_path, capsys, monkeypatch):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (4, 16, 20, 3), dtype=np.uint8)
    b = a.copy()
    b[1, 0, 0, 0] = a[1, 0, 0, 0] ^ 1
    b[2, 5:9, 3:7] = 255 - a[2, 5:9, 3:7]
    monkeypatch.chdir(tmp_path)
    np.savez("a.npz", frames=a, fps=np.float64(30.0))
    np.savez("b.npz", frames=b, fps=np.float64(30.0))
    for be in (mc.NumpyBackend(), myc.NumpyYuvBackend()):  # the 5-word protocol alone is enough for array clips
        assert evaluate.main(["compare", "a.npz", "b.npz", "--max-lsb", "1"], backend=be) == 1
        assert capsys.readouterr().out.strip().splitlines()[-1] == ARRAY_LINE


# ------------------------------------------------------------------------------------------------------------------ hold-out
class _CopyModel:
    """every timestep returns the frame it lies nearest to: no arithmetic, the pairing is what is under test"""
    scale, pad_size = 1.0, 1

    def inference_ts(self, I0, I1, ts):
        return [(I0 if float(t) < 0.5 else I1).clone() for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, **kw):
        return [(I0 if float(t) < 0.5 else I1 if float(t) < 1.5 else I2).clone() for t in ts], None


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("plain", [False, True])
def test_holdout_on_a_y4m_file_pairs_as_the_array_holdout_does(tmp_path, bits, plain):
    k, m, h, w = 3, 2, 32, 48
    rng = np.random.default_rng(70)
    bgr = rng.integers(0, 256, (m * k + 2, h, w, 3), dtype=np.uint8)  # one frame past m k + 1: not used
    frames = yc.clip_from_bgr(bgr, bits)
    path = str(tmp_path / "clip.y4m")
    myc.write_clip(path, frames, frame_params={2: b"Ip"})
    src = evaluate.ClipSource(path)
    to_inp, to_out, check_scene = yc.cpu_hooks(bits, bits)
    be = myc.NumpyYuvBackend()
    res = evaluate.holdout(_CopyModel(), src, k, fps=src.fps, plain=plain, backend=be, to_inp=to_inp, to_out=to_out, check_scene=check_scene)
    # the array hold-out of the same clip
    hooks = (lambda fr, size: torch.from_numpy(np.ascontiguousarray(fr)).float(), lambda x, size: np.rint(x.numpy()).astype(np.uint8))
    arr = evaluate.holdout(_CopyModel(), bgr, k, plain=plain, backend=mc.NumpyBackend(), to_inp=hooks[0], to_out=hooks[1])
    assert res["pairs"] == arr["pairs"] == [(j, j - 1) for j in range(1, k * (m + 1) - 1)]
    for part in ("kept", "held_out"):
        assert res[part]["positions"] == arr[part]["positions"] and res[part]["frames"] == arr[part]["frames"]
    assert res["emissions"] == k * (m + 1) and res["frames_used"] == m * k + 1 and res["plain"] is plain
    assert (res["pixfmt"], res["depth"], res["maxval"]) == ("yuv420", 8 if bits == 8 else 16, (1 << bits) - 1)
    assert res["kept_passthrough"] == "to_out(to_inp(frame))"
    # every compared pair is (emission, the original's planes at its position)
    for (j, p), (got, orig) in zip(res["pairs"], be.pairs):
        assert np.array_equal(orig, frames[p].data), (j, p)
    # kept frames pass through to_out(to_inp(.)): luma comes back within a step, chroma is filtered -- finite PSNR
    ks = res["kept"]["summary"]
    assert math.isfinite(ks["psnr_of_mean_mse"]) and math.isfinite(ks["psnr_of_mean_mse_u"]) and ks["psnr_of_mean_mse_y"] > ks["psnr_of_mean_mse_u"]
    rep = evaluate.holdout_report(res)
    json.dumps(evaluate._jsonable(rep))
    assert rep["kept_passthrough"] == "to_out(to_inp(frame))" and rep["pixfmt"] == "yuv420" and rep["kept"]["frames"] == m + 1
    assert "psnr_of_mean_mse_v" in rep["held_out"] and rep["held_out"]["positions"] == [1, 2, 4, 5]


def test_holdout_refuses_a_stream_that_cannot_seek_before_a_model_is_loaded(tmp_path, capsys, monkeypatch):
    data = myc.write_clip(None, myc.random_clip(7, 14, 22, 8, seed=71))

    class _Stdin:
        buffer = _Pipe(data)

    monkeypatch.setattr(evaluate.sys, "stdin", _Stdin())
    from drba_amd import infer
    monkeypatch.setattr(infer, "load_model", lambda *a, **k: pytest.fail("a model was loaded"))
    assert evaluate.main(["holdout", "-m", "rife", "-i", "-", "-k", "3"], backend=myc.NumpyYuvBackend()) == 2
    assert "needs random access" in capsys.readouterr().err
    # ... and a seekable clip that is too short is refused by the plan, also before a model
    short = str(tmp_path / "short.y4m")
    myc.write_clip(short, myc.random_clip(6, 14, 22, 8, seed=72))
    assert evaluate.main(["holdout", "-m", "rife", "-i", short, "-k", "3"], backend=myc.NumpyYuvBackend()) == 2
    assert "at least 7 frames" in capsys.readouterr().err
