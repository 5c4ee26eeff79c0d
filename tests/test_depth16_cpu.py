"""CPU (-m "not gpu"): the host side of 16-bit frames -- clip IO, sinks, the command line, the sharded run's refusal, compare's
refusals and the "u16" kind of drba_amd.metrics over a numpy back end -- with stand-in hooks and back ends, as
tests/test_clip_cpu.py and tests/test_metrics_cpu.py do for bytes.  The kernels are checked in tests/test_gpu_depth16.py."""
import argparse
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from drba_amd import _lib, evaluate, metrics, ops
from drba_amd import infer as drv
from drba_amd.models.utils import tools
from drba_amd.utils import synth
from tests import depth16_common as d16
from tests import ffmpeg_stub


def _clip16(n=4, h=32, w=48, seed=3, maxval=65535):
    return np.random.default_rng(seed).integers(0, maxval + 1, size=(n, h, w, 3), dtype=np.uint16)


def _run_sink(io, frames):
    for f in frames:
        io.write_frame(f)
    io.close()


class _Copy:  # "interpolates" by repeating the nearer frame: only the plumbing is under test
    scale, pad_size, supports_lookahead = 1.0, 32, False

    def inference_ts(self, I0, I1, ts):
        return [I0 if t < 0.5 else I1 for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False):
        return [I0 if t < 0.5 else (I1 if t < 1.5 else I2) for t in ts], None


@pytest.fixture()
def stub_hooks(monkeypatch):
    """tools.to_inp / to_out replaced by recording pass-throughs (frames stay numpy arrays of their own dtype)"""
    calls = {"to_inp": [], "to_out": []}

    def fake_to_inp(fr, size, device=None, maxval=None):
        calls["to_inp"].append((fr.dtype, maxval))
        return np.asarray(fr)

    def fake_to_out(x, size, rgb=False, depth=8, maxval=None):
        calls["to_out"].append((rgb, depth, maxval))
        if depth == 16 and x.dtype == np.uint8:     # 8-bit in, 16 bits out: full range
            x = x.astype(np.uint16) * np.uint16(257)
        if depth == 8 and x.dtype == np.uint16:
            x = (x >> 8).astype(np.uint8)
        return np.ascontiguousarray(x[:, :, ::-1]) if rgb else x

    monkeypatch.setattr(tools, "to_inp", fake_to_inp)
    monkeypatch.setattr(tools, "to_out", fake_to_out)
    return calls


# ------------------------------------------------------------------------------------------------------------------ clip IO
@pytest.mark.parametrize("form,maxval", [("npz", None), ("npz", 1023), ("npy", 4095), ("npy", None)])
def test_videofi_io_round_trip_of_uint16_clips_keeps_maxval(tmp_path, stub_hooks, form, maxval):
    frames = _clip16(maxval=maxval or 65535)
    inp, out = str(tmp_path / ("in." + form)), str(tmp_path / "out.npz")
    if form == "npz":
        np.savez(inp, frames=frames, fps=np.float64(24.0), **({} if maxval is None else {"maxval": np.int64(maxval)}))
    else:
        np.save(inp, frames)
        json.dump(dict({"fps": 24.0}, **({} if maxval is None else {"maxval": maxval})), open(str(tmp_path / "in.json"), "w"))
    io = tools.VideoFI_IO(inp, str(tmp_path / "probe.npz"))
    assert (io.depth, io.maxval, io.out_depth, io.out_maxval) == (16, maxval or 65535, 16, maxval or 65535) and io.src_fps == 24.0
    got = [io.read_frame() for _ in range(len(frames) + 1)]
    assert got[-1] is None and all(g.dtype == np.uint16 and np.array_equal(g, f) for g, f in zip(got, frames))
    io.close()
    n = drv.inference(_Copy(), drv.parse_args(["-m", "rife", "-i", inp, "-o", out, "-t", "2"]))
    assert n == 8
    z = np.load(out)
    assert z["frames"].dtype == np.uint16 and int(z["maxval"]) == (maxval or 65535) and float(z["fps"]) == 48.0
    assert np.array_equal(z["frames"], np.repeat(frames, 2, axis=0))
    # the hooks got the clip's maxval at both ends, the 8-bit keywords stayed out of an 8-bit run's calls (next test)
    assert set(stub_hooks["to_inp"]) == {(np.dtype(np.uint16), maxval or 65535)}
    assert set(stub_hooks["to_out"]) == {(False, 16, maxval or 65535)}
    # ... and the written clip opens as a 16-bit source with the same maxval (.npy sink: frames only)
    back = tools.VideoFI_IO(out, str(tmp_path / "again.npy"))
    assert (back.depth, back.maxval) == (16, maxval or 65535)
    _run_sink(back, list(frames[:2]))
    assert np.load(str(tmp_path / "again.npy")).dtype == np.uint16


def test_out_depth_crosses_between_8_and_16_bits(tmp_path, stub_hooks):
    f8 = np.random.default_rng(5).integers(0, 256, size=(4, 32, 48, 3), dtype=np.uint8)
    f16 = _clip16(maxval=1023)
    p8, p16 = str(tmp_path / "in8.npz"), str(tmp_path / "in16.npz")
    np.savez(p8, frames=f8, fps=np.float64(24.0))
    np.savez(p16, frames=f16, fps=np.float64(24.0), maxval=np.int64(1023))
    # default on an 8-bit source: today's calls exactly -- no 16-bit hook is built, no depth or maxval is passed
    out = str(tmp_path / "o8.npz")
    drv.inference(_Copy(), drv.parse_args(["-m", "rife", "-i", p8, "-o", out, "-t", "2"]))
    assert np.load(out)["frames"].dtype == np.uint8 and "maxval" not in np.load(out).files
    assert all(c == (np.dtype(np.uint8), None) for c in stub_hooks["to_inp"]) and set(stub_hooks["to_out"]) == {(False, 8, None)}
    # 16 bits out of an 8-bit source: full range
    out = str(tmp_path / "o8to16.npz")
    drv.inference(_Copy(), drv.parse_args(["-m", "rife", "-i", p8, "-o", out, "-t", "2", "--out-depth", "16"]))
    z = np.load(out)
    assert z["frames"].dtype == np.uint16 and int(z["maxval"]) == 65535 and np.array_equal(z["frames"][0], f8[0].astype(np.uint16) * 257)
    assert stub_hooks["to_out"][-1] == (False, 16, 65535)
    # 8 bits out of a 16-bit source
    del stub_hooks["to_out"][:]
    out = str(tmp_path / "o16to8.npz")
    drv.inference(_Copy(), drv.parse_args(["-m", "rife", "-i", p16, "-o", out, "-t", "2", "--out-depth", "8"]))
    z = np.load(out)
    assert z["frames"].dtype == np.uint8 and "maxval" not in z.files and set(stub_hooks["to_out"]) == {(False, 8, None)}
    assert stub_hooks["to_inp"][-1] == (np.dtype(np.uint16), 1023)
    with pytest.raises(ValueError, match="out_depth"):
        tools.VideoFI_IO(p8, str(tmp_path / "x.npz"), out_depth=10)
    with pytest.raises(ValueError, match="maxval"):
        np.savez(str(tmp_path / "bad.npz"), frames=f16, maxval=np.int64(255))
        tools.VideoFI_IO(str(tmp_path / "bad.npz"), str(tmp_path / "x.npz"))


def test_out_depth_parsing_and_default():
    assert drv.parse_args([]).out_depth == "source" and drv.out_depth_of(drv.parse_args([])) is None
    assert drv.out_depth_of(drv.parse_args(["--out-depth", "16"])) == 16 and drv.out_depth_of(drv.parse_args(["--out-depth", "8"])) == 8
    assert drv.out_depth_of(drv.parse_args(["--out-depth", "source"])) is None
    assert drv.out_depth_of(argparse.Namespace()) is None  # a namespace from before the flag
    with pytest.raises(SystemExit):
        drv.parse_args(["--out-depth", "10"])
    with pytest.raises(ValueError):
        drv.out_depth_of(argparse.Namespace(out_depth="12"))


# -------------------------------------------------------------------------------------------------------------------- sinks
def test_raw_sink_writes_little_endian_rgb48_scaled_to_full_range(tmp_path):
    for maxval in (65535, 1023):
        frames = _clip16(3, 8, 12, seed=maxval, maxval=maxval)
        frames[0, 0, 0] = (0, maxval // 2, maxval)  # B, G, R
        inp, out = str(tmp_path / f"in{maxval}.npz"), str(tmp_path / f"out{maxval}.raw")
        np.savez(inp, frames=frames, fps=np.float64(24.0), maxval=np.int64(maxval))
        io = tools.VideoFI_IO(inp, out)
        assert io.wants_rgb and io.out_depth == 16
        _run_sink(io, list(frames))
        data = open(out, "rb").read()
        assert len(data) == frames.size * 2
        rgb = frames[:, :, :, ::-1].astype(np.int64)
        full = (rgb * 65535 + maxval // 2) // maxval  # always scaled to 65535, rounded
        assert data == full.astype("<u2").tobytes()
        first = np.frombuffer(data[:6], dtype="<u2")
        assert first.tolist() == [65535, (maxval // 2 * 65535 + maxval // 2) // maxval, 0]  # R, G, B: the largest sample is all ones
        assert data[0:2] == b"\xff\xff" and data[4:6] == b"\x00\x00"
    # frames the driver already flipped (to_out(..., rgb=True)) are not flipped again
    io = tools.VideoFI_IO(inp, str(tmp_path / "flipped.raw"))
    io.frames_are_rgb = True
    _run_sink(io, list(frames))
    assert open(str(tmp_path / "flipped.raw"), "rb").read() == ((frames.astype(np.int64) * 65535 + 511) // 1023).astype("<u2").tobytes()
    # bytes into the 16-bit sink are an error that close() reports, not a silent reinterpretation
    io = tools.VideoFI_IO(inp, str(tmp_path / "wrong.raw"))
    io.write_frame(np.zeros((8, 12, 3), np.uint8))
    with pytest.raises(RuntimeError, match="uint16"):
        io.close()


@pytest.fixture()
def stub_on_path(tmp_path, monkeypatch):
    d = tmp_path / "bin"
    d.mkdir()
    ffmpeg_stub.write_stub(d)
    monkeypatch.setenv("PATH", str(d) + os.pathsep + os.environ.get("PATH", ""))
    assert tools._have_ffmpeg()
    return d


def test_ffmpeg_argv_at_depth_16_differs_from_depth_8_in_the_two_pixel_formats_only(tmp_path, stub_on_path):
    f16 = _clip16(3, 36, 48)
    p16, p8 = str(tmp_path / "in16.npz"), str(tmp_path / "in8.npz")
    np.savez(p16, frames=f16, fps=np.float64(24.0))
    np.savez(p8, frames=(f16 >> 8).astype(np.uint8), fps=np.float64(24.0))
    argvs = {}
    for name, src, kw, frames in (("d8", p8, {}, (f16 >> 8).astype(np.uint8)), ("d16", p16, {}, f16),
                                  ("d8to16", p8, {"out_depth": 16}, f16), ("d16to8", p16, {"out_depth": 8}, (f16 >> 8).astype(np.uint8))):
        out = str(tmp_path / (name + ".mp4"))
        io = tools.VideoFI_IO(src, out, dst_fps=60, **kw)
        _run_sink(io, list(frames))
        argv, data = ffmpeg_stub.recorded(out)
        assert argv[-1] == out
        assert data == np.ascontiguousarray(frames[:, :, :, ::-1]).astype(frames.dtype.newbyteorder("<")).tobytes()
        argvs[name] = argv[:-1]
    assert argvs["d16to8"] == argvs["d8"] and argvs["d8to16"] == argvs["d16"]
    a16 = argvs["d16"]
    assert a16[a16.index("-pix_fmt") + 1] == "rgb48le" and a16.count("rgb48le") == 1 and a16.count("yuv420p10le") == 1
    assert a16[a16.index("-c:v") + 1] == "libx264" and a16[a16.index("yuv420p10le") - 1] == "-pix_fmt"
    assert [{"rgb48le": "rgb24", "yuv420p10le": "yuv420p"}.get(t, t) for t in a16] == argvs["d8"]  # every other token as today


def test_hwaccel_at_depth_16_is_refused_before_a_frame_is_read(tmp_path, stub_on_path, monkeypatch):
    p16, p8 = str(tmp_path / "in16.npz"), str(tmp_path / "in8.npz")
    np.savez(p16, frames=_clip16(2), fps=np.float64(24.0))
    np.savez(p8, frames=np.zeros((2, 32, 48, 3), np.uint8), fps=np.float64(24.0))
    started = []
    monkeypatch.setattr(tools.threading, "Thread", lambda *a, **k: started.append(k) or pytest.fail("a reader / writer thread was started"))
    monkeypatch.setattr(tools.VideoFI_IO, "_spawn_ffmpeg", lambda self, hw: pytest.fail("an encoder was started"))
    for src, kw in ((p16, {}), (p8, {"out_depth": 16})):
        with pytest.raises(ValueError, match="10-bit") as e:
            tools.VideoFI_IO(src, str(tmp_path / "hw.mp4"), hwaccel=True, **kw)
        assert "h264_vaapi" in str(e.value)
    assert not started and not os.path.exists(str(tmp_path / "hw.mp4.argv.json"))
    with pytest.raises(ValueError, match="10-bit"):  # ... and through the command line's entry
        drv.inference(_Copy(), drv.parse_args(["-m", "rife", "-i", p16, "-o", str(tmp_path / "hw.mp4"), "-t", "2", "-hw"]))


# -------------------------------------------------------------------------------------------------------------- sharded run
def test_sharded_run_refuses_16_bit_before_any_collective(tmp_path, monkeypatch):
    from drba_amd import parallel
    import torch.distributed as dist
    p16, p8, y16 = str(tmp_path / "in16.npz"), str(tmp_path / "in8.npz"), str(tmp_path / "in16.npy")
    np.savez(p16, frames=_clip16(6), fps=np.float64(24.0))
    np.save(y16, _clip16(6))
    np.savez(p8, frames=np.zeros((6, 32, 48, 3), np.uint8), fps=np.float64(24.0))

    def forbidden(*a, **k):
        raise AssertionError("reached the gather / a collective")

    monkeypatch.setattr(parallel, "StreamedGather", forbidden)
    monkeypatch.setattr(parallel, "interpolate_shard", forbidden)
    for name in ("all_gather", "all_reduce", "barrier", "broadcast", "send", "recv", "isend", "irecv", "gather"):
        monkeypatch.setattr(dist, name, forbidden)
    base = dict(output=str(tmp_path / "out.npz"), dst_fps=48.0, times=2, enable_scdet=False, scdet_threshold=0.3, hwaccel=False)
    for inp, depth in ((p16, "source"), (y16, "source"), (p8, "16"), (p16, "8")):
        for rank in (0, 1):
            with pytest.raises(ValueError, match="frame-sharded") as e:
                drv.inference_sharded(_Copy(), argparse.Namespace(input=inp, out_depth=depth, **base), rank, 2)
            assert "8-bit" in str(e.value) and ("uint16" in str(e.value) or depth == "16")
    assert not os.path.exists(base["output"])


# ------------------------------------------------------------------------------------------------------------------ compare
def test_clip_source_and_compare_on_uint16_clips(tmp_path, capsys):
    a = _clip16(4, 16, 20, seed=5)
    b = a.copy()
    b[1, 0, 0, 0] = a[1, 0, 0, 0] ^ 1                     # one 16-bit step in one sample
    b[2, 5:9, 3:7] = 65535 - a[2, 5:9, 3:7]               # a block inverted
    b[3, 2, 2, 1], a[3, 2, 2, 1] = 65535, 0               # the full range: a uint16 difference that wraps is -1 there
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npy")
    np.savez(pa, frames=a, fps=np.float64(30.0))
    np.save(pb, b)
    json.dump({"fps": 30.0, "maxval": 65535}, open(str(tmp_path / "b.json"), "w"))
    sa, sb = evaluate.ClipSource(pa), evaluate.ClipSource(pb)
    assert (sa.depth, sa.maxval, sb.depth, sb.maxval) == (16, 65535, 16, 65535) and next(iter(sa)).dtype == np.uint16
    be = d16.NumpyBackend16()
    assert evaluate.main(["compare", pa, pb, "--max-lsb", "65535"], backend=be) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    d = np.abs(a.astype(np.int64) - b.astype(np.int64)).reshape(4, -1)
    mse = (d * d).mean(1)
    assert rep["depth"] == 16 and rep["maxval"] == 65535 and rep["peak"] == 65535.0 and rep["frames"] == 4
    assert rep["max_lsb"] == 65535 and rep["total_differing"] == int((d != 0).sum())
    assert rep["psnr_of_mean_mse"] == pytest.approx(metrics.psnr_of_mse(mse.mean(), 65535.0), rel=1e-12)
    assert set(be.maxvals) == {65535}
    # the gate counts 16-bit steps: 300 steps pass --max-lsb 300 and fail --max-lsb 255 (an 8-bit reading would pass both ways round)
    c = a.copy()
    c[0, 1, 1, 1] = a[0, 1, 1, 1] + 300 if a[0, 1, 1, 1] < 60000 else a[0, 1, 1, 1] - 300
    pc = str(tmp_path / "c.npz")
    np.savez(pc, frames=c)
    assert evaluate.main(["compare", pa, pc, "--max-lsb", "300"], backend=be) == 0
    assert evaluate.main(["compare", pa, pc, "--max-lsb", "255"], backend=be) == 1
    r = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert r["gates"]["max_lsb"] == {"limit": 255.0, "value": 300, "ok": False}


def test_compare_refuses_mixed_depths_and_mixed_maxval_naming_both(tmp_path, capsys):
    a = _clip16(2, 16, 20, maxval=1023)
    p16, p10, p12, p8 = (str(tmp_path / n) for n in ("a16.npz", "a10.npz", "a12.npz", "a8.npz"))
    np.savez(p16, frames=a)
    np.savez(p10, frames=a, maxval=np.int64(1023))
    np.savez(p12, frames=a, maxval=np.int64(4095))
    np.savez(p8, frames=(a >> 2).astype(np.uint8))
    be = d16.NumpyBackend16()
    for x, y, words in ((p16, p8, ("16-bit", "8-bit", "65535", "255")), (p8, p10, ("8-bit", "16-bit", "255", "1023")),
                        (p16, p10, ("65535", "1023")), (p10, p12, ("1023", "4095"))):
        assert evaluate.main(["compare", x, y], backend=be) == 2
        err = capsys.readouterr().err
        assert "differ in depth" in err and all(w in err for w in words), err
    assert evaluate.main(["compare", p10, p10], backend=be) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["depth"] == 16 and rep["maxval"] == 1023 and rep["peak"] == 1023.0 and rep["mean_psnr"] == "inf"
    with pytest.raises(ValueError, match="differ in form"):  # frames without a source around them: the kinds are compared per pair
        evaluate.compare(iter([a[0]]), iter([(a[0] >> 2).astype(np.uint8)]), backend=be)


# ------------------------------------------------------------------------------------------------------------------ metrics
def test_u16_kind_over_a_numpy_back_end_and_the_wrapping_defect():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 65536, (5, 16, 24, 3), dtype=np.uint16)
    b = a.copy()
    b[1, 2, 3, 1] ^= 4
    b[3, :4] = 65535 - b[3, :4]
    b[4, 0, 0, 0], a[4, 0, 0, 0] = 65535, 0
    d = np.abs(a.astype(np.int64) - b.astype(np.int64)).reshape(5, -1)
    mse = (d * d).mean(1)

    def run(be, **kw):
        cm = metrics.ClipMetrics(backend=be, capacity=2, **kw)
        for k in range(3):
            cm.add(a[k], b[k])
        cm.add(torch.from_numpy(a[3:]), torch.from_numpy(b[3:]))  # two frames in one call, torch tensors
        return cm.result()

    r = run(d16.NumpyBackend16())
    assert r["peak"] == 65535.0 and r["frames"] == 5
    assert r["per_frame"]["differing"] == (d != 0).sum(1).tolist() and r["per_frame"]["max_lsb"] == d.max(1).tolist()  # 16-bit steps
    assert r["per_frame"]["psnr"] == [metrics.psnr_of_mse(v, 65535.0) for v in mse]
    assert r["per_frame"]["ssim"][0] == 1.0 and r["per_frame"]["ssim"][3] < 0.9 and r["per_frame"]["nonfinite"] == [0] * 5
    assert r["summary"]["max_lsb"] == 65535 and r["summary"]["total_differing"] == int((d != 0).sum())
    # the planted defect: differences in uint16 arithmetic wrap; the same rows catch it
    w = run(d16.NumpyBackend16(wrap=True))
    assert w["per_frame"]["max_lsb"] != d.max(1).tolist() and w["per_frame"]["psnr"] != r["per_frame"]["psnr"]
    assert w["per_frame"]["differing"] == r["per_frame"]["differing"]  # (a wrapped difference is still a difference)
    good = d16.check_frame_error_u16(lambda x, y, N, n, oa, ob: d16.err_u16_ref(x, y, N, n))

    def wrapped(x, y, N, n, oa, ob):
        dd = (x - y).astype(np.int64).reshape(N, n)
        return np.stack([(dd * dd).sum(1), dd.sum(1), dd.max(1), (dd != 0).sum(1)], 1)

    def acc48(x, y, N, n, oa, ob):
        return d16.err_u16_ref(x, y, N, n) & ((1 << 48) - 1)

    failed = lambda rows: [x[0] for x in rows if not x[1] <= x[2]]  # noqa: E731
    assert not failed(good) and len(good) == 3 * len(d16.ERR16_SIZES) + 3
    bad = failed(d16.check_frame_error_u16(wrapped))                                  # every row with an a < b somewhere
    assert sum("n=363 N=3 offsets" in n or "n=70000 N=3 offsets" in n for n in bad) == 6 and any("a=0 b=65535" in n for n in bad)
    assert not any("identical" in n for n in bad)
    assert any("2^48" in n for n in failed(d16.check_frame_error_u16(acc48)))         # a 48-bit accumulator is caught
    # peak: maxval by default, ClipMetrics(peak=...) still overrides; the back end is told the clip's maxval
    be = d16.NumpyBackend16()
    r10 = run(be, maxval=1023)
    assert r10["peak"] == 1023.0 and set(be.maxvals) == {1023}
    assert run(d16.NumpyBackend16(), peak=100.0)["peak"] == 100.0
    # the one-shot functions
    be = d16.NumpyBackend16()
    assert metrics.psnr(a[1], b[1], backend=be) == metrics.psnr_of_mse(mse[1], 65535.0)
    assert metrics.psnr(a[1], b[1], backend=be, maxval=1023) == metrics.psnr_of_mse(mse[1], 1023.0)
    assert metrics.psnr(a[0], b[0], backend=be) == math.inf and metrics.ssim(a[2], b[2], backend=be) == 1.0
    assert metrics.frame_error(a[3], b[3], backend=be) == {"sum_sq": int((d[3] ** 2).sum()), "sum_abs": int(d[3].sum()), "max_abs": int(d[3].max()),
                                                          "differing": int((d[3] != 0).sum()), "n": 16 * 24 * 3}
    # kinds do not mix, and maxval belongs to uint16 frames
    with pytest.raises(ValueError, match="differ in form"):
        metrics.psnr(a[0], (a[0] >> 8).astype(np.uint8), backend=be)
    with pytest.raises(ValueError, match="maxval"):
        metrics.psnr((a[0] >> 8).astype(np.uint8), (a[0] >> 8).astype(np.uint8), backend=be, maxval=1023)
    with pytest.raises(ValueError, match="maxval"):
        metrics.psnr(a[0], a[0], backend=be, maxval=255)
    # an 8-bit back end from before the kind is still driven with its own argument list
    from tests import metric_checks as mc
    u8 = (a >> 8).astype(np.uint8)
    assert metrics.psnr(u8[0], u8[0], backend=mc.NumpyBackend()) == math.inf


def test_holdout_on_a_16_bit_clip_emits_and_compares_16_bits():
    k, m = 3, 2
    frames = np.stack([np.full((12, 14, 3), p * 4000 + 123, np.uint16) for p in range(m * k + 1)])
    seen = {"inp": set(), "out": set()}

    class Linear:
        scale, pad_size = 1.0, 1

        def inference_ts(self, I0, I1, ts):
            return [I0 + float(t) * (I1 - I0) for t in ts]

        def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, **kw):
            return [I0 + float(t) * (I1 - I0) if t < 1 else I1 + (float(t) - 1) * (I2 - I1) for t in ts], None

    def to_inp(fr, size):
        seen["inp"].add(fr.dtype)
        return torch.from_numpy(fr.astype(np.float64))

    def to_out(x, size):
        out = np.rint(x.numpy()).astype(np.uint16)
        seen["out"].add(out.dtype)
        return out

    be = d16.NumpyBackend16()
    res = evaluate.holdout(Linear(), frames, k, backend=be, to_inp=to_inp, to_out=to_out, maxval=65535)
    assert res["depth"] == 16 and res["maxval"] == 65535 and seen == {"inp": {np.dtype(np.uint16)}, "out": {np.dtype(np.uint16)}}
    assert res["kept"]["peak"] == 65535.0 and res["kept"]["summary"]["max_lsb"] == 0 and res["held_out"]["summary"]["max_lsb"] == 0
    assert res["kept"]["positions"] == [0, 3, 6] and res["held_out"]["positions"] == [1, 2, 4, 5]
    assert all(o.dtype == np.uint16 for _, o in be.pairs) and set(be.maxvals) == {65535}
    rep = evaluate.holdout_report(res)
    assert rep["depth"] == 16 and rep["maxval"] == 65535
    with pytest.raises(ValueError, match="maxval"):
        evaluate.holdout(Linear(), (frames >> 8).astype(np.uint8), k, backend=be, to_inp=to_inp, to_out=to_out, maxval=1023)


# ------------------------------------------------------------------------------------------------------- library, ops, synth
def test_16_bit_entry_points_validate_arguments_without_gpu():
    lib = _lib.load()
    buf = torch.zeros(4096)
    p = C.c_void_p(buf.data_ptr())
    odd = C.c_void_p(buf.data_ptr() + 1)
    s = None
    assert lib.drba_to_inp16_x4(None, p, p, 8, 8, 8, 8, 1.0, 1.0, 65535.0, s) == -1
    assert lib.drba_to_inp16_x4(p, None, p, 8, 8, 8, 8, 1.0, 1.0, 65535.0, s) == -1
    assert lib.drba_to_inp16_x4(p, p, p, 0, 8, 8, 8, 1.0, 1.0, 65535.0, s) == -1
    assert lib.drba_to_inp16_x4(odd, p, p, 8, 8, 8, 8, 1.0, 1.0, 65535.0, s) == -1        # samples are 2-byte aligned
    assert lib.drba_to_inp16_x4(p, p, C.c_void_p(buf.data_ptr() + 8), 8, 8, 8, 8, 1.0, 1.0, 65535.0, s) == -1  # out_x4: 16 bytes
    assert lib.drba_to_out16(None, p, 8, 8, 8, 8, 1.0, 1.0, 0, 65535.0, s) == -1
    assert lib.drba_to_out16(p, None, 8, 8, 8, 8, 1.0, 1.0, 0, 65535.0, s) == -1
    assert lib.drba_to_out16(p, odd, 8, 8, 8, 8, 1.0, 1.0, 0, 65535.0, s) == -1
    for bad in (255.0, 0.0, -1.0, 65536.0, float("nan"), float("inf")):                    # 255 < maxval <= 65535
        assert lib.drba_to_inp16_x4(p, p, p, 8, 8, 8, 8, 1.0, 1.0, bad, s) == -1
        assert lib.drba_to_out16(p, p, 8, 8, 8, 8, 1.0, 1.0, 0, bad, s) == -1
        assert lib.drba_u16hwc_to_f32nchw(p, p, 8, 8, bad, s) == -1
        assert lib.drba_f32nchw_to_u16hwc(p, p, 8, 8, bad, s) == -1
    assert lib.drba_u16hwc_to_f32nchw(None, p, 8, 8, 1023.0, s) == -1 and lib.drba_f32nchw_to_u16hwc(p, None, 8, 8, 1023.0, s) == -1
    fn = lib.drba_frame_error_u16
    assert fn(None, p, p, p, 1, 16, s) == -1 and fn(p, None, p, p, 1, 16, s) == -1 and fn(p, p, None, p, 1, 16, s) == -1
    assert fn(p, p, p, None, 1, 16, s) == -1 and fn(p, p, p, p, 0, 16, s) == -1 and fn(p, p, p, p, 1, 0, s) == -1
    assert fn(odd, p, p, p, 1, 16, s) == -1 and fn(p, odd, p, p, 1, 16, s) == -1
    assert fn(p, p, p, p, 1, 1 << 32, s) == -2                                            # sum d^2 could pass 2^64
    assert lib.drba_frame_error_u16_ws_floats(3, 1) == 3 * 512 * 8 and lib.drba_frame_error_u16_ws_floats(0, 5) == 0


def test_ops_dispatch_has_no_cpu_path_and_checks_maxval():
    f16 = torch.from_numpy(_clip16(1)[0])
    with pytest.raises(_lib.DrbaHipError, match="uint16"):
        ops.to_inp(f16, (32, 48))                       # a CPU tensor: no fallback
    with pytest.raises(_lib.DrbaHipError):
        ops.to_out(torch.zeros(1, 3, 8, 8), (8, 8), depth=16)
    for bad in (255, 65536, 0, 1023.5):
        with pytest.raises(ValueError, match="maxval"):
            ops._maxval(bad)
    assert ops._maxval(None) == 65535 and ops._maxval(1023) == 1023 and ops._maxval(256) == 256
    with pytest.raises(ValueError, match="depth"):
        ops.to_out(torch.zeros(1, 3, 8, 8), (8, 8), depth=10)
    with pytest.raises(ValueError, match="maxval"):
        ops.to_out(torch.zeros(1, 3, 8, 8), (8, 8), maxval=1023)  # depth 8 has no maxval
    with pytest.raises(ValueError, match="depth"):
        tools.to_out(torch.zeros(1, 3, 8, 8), (8, 8), depth=12)


def test_make_clip16_is_make_clip_with_populated_low_bits():
    f8 = synth.make_clip(3, 32, 48, seed=7, cut_at=2)
    f16 = synth.make_clip16(3, 32, 48, seed=7, cut_at=2)
    assert all(f.dtype == np.uint16 and f.shape == (32, 48, 3) for f in f16)
    assert all(np.array_equal(a >> 8, b) for a, b in zip(f16, f8))                       # make_clip's content in the high byte
    low = np.stack(f16) & 0xff
    assert len(np.unique(low)) == 256 and (np.stack(f16) % 257 != 0).mean() > 0.99       # every low bit is used
    assert all(np.array_equal(a, b) for a, b in zip(f16, synth.make_clip16(3, 32, 48, seed=7, cut_at=2)))  # seeded
    f10 = synth.make_clip16(3, 32, 48, seed=7, cut_at=2, maxval=1023)
    assert max(int(f.max()) for f in f10) <= 1023 and all(np.array_equal(a >> 2, b) for a, b in zip(f10, f8))
    with pytest.raises(ValueError):
        synth.make_clip16(1, 8, 8, maxval=255)


def test_restatement_resize_is_the_oracle_resize_wherever_aten_keeps_its_frame_loop():
    """depth16_common.resize widens small planes so that F.interpolate runs the loop it runs on frames.  Where ATen's choice does
    not change (output H + W > 128, one channel per call) the widening must be invisible, bit for bit -- also with NaN / inf in
    the plane and on an axis whose size stays --, and at frame shapes it is the plain oracle call."""
    from oracle import ops as oops
    g = torch.Generator().manual_seed(16)
    for (h, w), size in (((80, 160), (70, 100)), ((70, 100), (80, 160)), ((64, 100), (60, 100)), ((90, 66), (96, 66)), ((128, 192), (128, 192))):
        x = torch.rand(1, 3, h, w, generator=g)
        x[0, 1, 5, 7], x[0, 2, h - 1, w - 1], x[0, 0, 0, w - 1] = float("nan"), float("inf"), -0.5
        want = torch.cat([oops.resize(x[:, c:c + 1], size) for c in range(3)], 1)
        got = d16.resize(x, size)
        assert got.shape == want.shape and torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0)), (h, w, size)
    # the widened call itself, against the same plane widened by hand at a size where nothing had to be widened
    x = torch.rand(1, 1, 64, 128, generator=g)
    wide = torch.cat([x, x[..., -1:].expand(-1, -1, -1, 128)], 3)
    assert torch.equal(oops.resize(wide, (90, 280))[..., :140], oops.resize(x, (90, 140)))
    assert d16.resize(torch.rand(2, 3, 64, 128, generator=g), (45, 70)).shape == (2, 3, 45, 70)


def test_restatement_round_trip_is_the_identity_and_rounds_half_to_even():
    """The claim the kernels are built on, on the CPU: v / maxval * maxval rounds back to v for every sample value."""
    for maxval in (65535, 1023):
        v = d16.all_values_frame(maxval)
        assert np.array_equal(d16.quantise16(d16.planar16(v, maxval), maxval), v)
        assert np.array_equal(d16.to_out16_ref(d16.to_inp16_ref(v, v.shape[:2], maxval), v.shape[:2], maxval), v)
        assert np.array_equal(d16.to_out16_ref(d16.planar16(v, maxval), v.shape[:2], maxval, rev=True), v[:, :, ::-1])
    # (x / 1024 * 1024 is exact: the halves reach the rounding as halves)
    q = d16.quantise16(torch.tensor([[0.5, 1.5, 2.5, -0.5, float("nan"), float("inf"), float("-inf"), 70000.0]]).view(1, 1, 1, -1).repeat(1, 3, 1, 1) / 1024.0, 1024)
    assert q[0, :, 0].tolist() == [0, 2, 2, 0, 0, 1024, 0, 1024]  # halves to even, negatives and NaN to 0, saturation
