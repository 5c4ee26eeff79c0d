"""CPU: the plumbing of fit = pad -- the --fit flag of infer.py and of `evaluate holdout`, the keyword on every hook `inference`
builds (8-bit, 16-bit, Y4M in, Y4M out, the raw RGB sink), the frame-sharded run's default hooks, and the CPU restatement of the
mode (tests/fit_pad_common.py), which must give a frame back exactly."""
import argparse
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from drba_amd import evaluate, y4m
from drba_amd import infer as drv
from drba_amd.models.utils import tools
from tests import fit_pad_common as fpc
from tests import metric_checks as mc
from tests import yuv_common as yc


# ------------------------------------------------------------------------------------------------------------------- the flag
def test_fit_flag_parsing_and_default():
    assert drv.parse_args([]).fit == "resize" and drv.fit_of(drv.parse_args([])) == "resize"
    assert drv.fit_of(drv.parse_args(["--fit", "pad"])) == "pad" and drv.fit_of(drv.parse_args(["--fit", "resize"])) == "resize"
    assert drv.fit_of(argparse.Namespace()) == "resize"  # a namespace from before the flag
    with pytest.raises(SystemExit):
        drv.parse_args(["--fit", "stretch"])
    with pytest.raises(ValueError):
        drv.fit_of(argparse.Namespace(fit="stretch"))
    a = evaluate.parse_args(["holdout", "-i", "clip.npz"])
    assert a.fit == "resize" and evaluate.parse_args(["holdout", "-i", "clip.npz", "--fit", "pad"]).fit == "pad"
    with pytest.raises(SystemExit):
        evaluate.parse_args(["holdout", "-i", "clip.npz", "--fit", "stretch"])


def test_tools_refuse_an_unknown_fit_before_anything_is_uploaded():
    f = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="fit"):
        tools.to_inp(f, (8, 8), device=torch.device("cpu"), fit="stretch")
    with pytest.raises(ValueError, match="fit"):
        tools.to_out(torch.zeros(1, 3, 8, 8), (8, 8), fit="stretch")


def test_net_size_docstring_names_both_fits():
    doc = tools.get_valid_net_inp_size.__doc__
    assert "resized, not padded" not in " ".join(doc.split()) and "pad" in doc


# ------------------------------------------------------------------------------------------------- every hook carries the keyword
class _Copy:  # "interpolates" by repeating the nearer frame: only the plumbing is under test
    scale, pad_size, supports_lookahead = 1.0, 32, False

    def inference_ts(self, I0, I1, ts):
        return [I0 if t < 0.5 else I1 for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False):
        return [I0 if t < 0.5 else (I1 if t < 1.5 else I2) for t in ts], None


@pytest.fixture()
def recording_hooks(monkeypatch):
    """tools.to_inp / to_out replaced by recorders: what kind of frame came in, what kind of frame was asked for, and the keywords"""
    calls = {"to_inp": [], "to_out": []}

    def fake_to_inp(fr, size, **kw):
        kind = "yuv" if isinstance(fr, y4m.YuvFrame) else ("u16" if fr.dtype == np.uint16 else "u8")
        calls["to_inp"].append((kind, dict(kw)))
        return (fr, tuple(size))

    def fake_to_out(x, size, **kw):
        calls["to_out"].append(dict(kw))
        h, w = size
        dtype = np.uint16 if kw.get("depth", 8) == 16 else np.uint8
        if kw.get("pixfmt", "bgr") == "yuv420":
            return np.zeros(h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2), dtype)
        return np.zeros((h, w, 3), dtype)

    monkeypatch.setattr(tools, "to_inp", fake_to_inp)
    monkeypatch.setattr(tools, "to_out", fake_to_out)
    return calls


def _sources(tmp_path, h=30, w=44, n=4):
    rng = np.random.default_rng(3)
    p8, p16, py = str(tmp_path / "in8.npz"), str(tmp_path / "in16.npz"), str(tmp_path / "in.y4m")
    np.savez(p8, frames=rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8), fps=np.float64(24.0))
    np.savez(p16, frames=rng.integers(0, 1024, size=(n, h, w, 3), dtype=np.uint16), fps=np.float64(24.0), maxval=np.int64(1023))
    hdr = y4m.Header(w, h, (24, 1), interlace="p", chroma="420jpeg")
    open(py, "wb").write(yc.y4m_bytes([yc.random_frame(h, w, 8, seed=k) for k in range(n)], hdr))
    return p8, p16, py


# (source, sink, kind of the frames read, keywords the sink's hook must carry besides fit)
KINDS = [("8", "out.npz", "u8", {}), ("16", "out.npz", "u16", {"depth": 16, "maxval": 1023}),
         ("y4m", "out.y4m", "yuv", {"pixfmt": "yuv420"}), ("8", "out.y4m", "u8", {"pixfmt": "yuv420"}),
         ("y4m", "out.npz", "yuv", {}), ("8", "out.raw", "u8", {"rgb": True}), ("16", "out.raw", "u16", {"rgb": True, "depth": 16})]


@pytest.mark.parametrize("src,sink,kind,sink_kw", KINDS, ids=[f"{k[0]}-to-{k[1]}" for k in KINDS])
def test_inference_passes_fit_to_the_hook_of_every_source_and_sink(tmp_path, recording_hooks, src, sink, kind, sink_kw):
    p8, p16, py = _sources(tmp_path)
    inp, out = {"8": p8, "16": p16, "y4m": py}[src], str(tmp_path / sink)
    argv = ["-m", "rife", "-i", inp, "-o", out, "-t", "2"]
    assert drv.inference(_Copy(), drv.parse_args(argv + ["--fit", "pad"])) == 8
    assert len(recording_hooks["to_inp"]) == 4 and len(recording_hooks["to_out"]) == 8
    assert all(k == kind and kw.get("fit") == "pad" for k, kw in recording_hooks["to_inp"]), recording_hooks["to_inp"]
    for kw in recording_hooks["to_out"]:
        assert kw.get("fit") == "pad" and all(kw.get(a) == b for a, b in sink_kw.items()), kw
    # resize, named or not: the calls carry no `fit` at all -- they are the calls of before
    for ns in (drv.parse_args(argv), drv.parse_args(argv + ["--fit", "resize"])):
        del recording_hooks["to_inp"][:], recording_hooks["to_out"][:]
        assert drv.inference(_Copy(), ns) == 8
        assert len(recording_hooks["to_inp"]) == 4 and len(recording_hooks["to_out"]) == 8
        assert all("fit" not in kw for _, kw in recording_hooks["to_inp"]) and all("fit" not in kw for kw in recording_hooks["to_out"])


def test_a_namespace_without_the_attribute_runs_as_resize(tmp_path, recording_hooks):
    p8, _, _ = _sources(tmp_path)
    ns = drv.parse_args(["-m", "rife", "-i", p8, "-o", str(tmp_path / "o.npz"), "-t", "2"])
    delattr(ns, "fit")
    assert drv.inference(_Copy(), ns) == 8
    assert recording_hooks["to_inp"] and all("fit" not in kw for _, kw in recording_hooks["to_inp"])
    assert recording_hooks["to_out"] and all("fit" not in kw for kw in recording_hooks["to_out"])


# -------------------------------------------------------------------------------------------------------- the CPU restatement
@pytest.mark.parametrize("src,dst", [((45, 71), (64, 128)), ((60, 64), (64, 64)), ((64, 64), (64, 64))])
def test_the_restatement_round_trips_exactly(src, dst):
    f8 = fpc.all_codes_frame(*src, seed=1)
    assert all(np.any(f8[:, :, c] == v) for c in range(3) for v in (0, 1, 127, 128, 254, 255))
    x = fpc.to_inp8(f8, dst)
    assert tuple(x.shape) == (1, 3, *dst) and x.dtype == torch.float32
    assert np.array_equal(fpc.to_out8(x, src), f8) and np.array_equal(fpc.to_out8(x, src, rgb=True), f8[:, :, ::-1])
    # the margins repeat the last row and column, the corner the last pixel
    assert torch.equal(x[:, :, src[0]:, :src[1]], x[:, :, src[0] - 1:src[0], :src[1]].expand(-1, -1, dst[0] - src[0], -1))
    assert torch.equal(x[:, :, :, src[1]:], x[:, :, :, src[1] - 1:src[1]].expand(-1, -1, -1, dst[1] - src[1]))
    for maxval in (1023, 65535):
        f16 = np.random.default_rng(maxval).integers(0, maxval + 1, size=(*src, 3)).astype(np.uint16)
        f16[0, 0], f16[-1, -1] = (0, maxval, maxval // 2), (maxval, 0, 1)
        assert np.array_equal(fpc.to_out16(fpc.to_inp16(f16, dst, maxval), src, maxval), f16)
    for bits in (8, 10):
        f = yc.in_gamut_frame(*src, bits, seed=bits)
        got = yc.split(fpc.to_out_yuv(fpc.to_inp_yuv(f, dst, bits).float(), src, bits), src)
        assert np.array_equal(got[0], f.planes()[0])
        f = yc.in_gamut_frame(*src, bits, seed=3, flat_chroma=True)
        got = yc.split(fpc.to_out_yuv(fpc.to_inp_yuv(f, dst, bits).float(), src, bits), src)
        assert all(np.array_equal(a, b) for a, b in zip(got, f.planes()))


def test_the_restatement_never_reads_the_margin_on_the_way_out():
    src, net = (45, 71), (64, 128)
    x = yc.planted_net_frame(net, seed=7)
    finite = lambda t: torch.nan_to_num(t, nan=0.0).clamp(0.0, 1.0)  # noqa: E731  (bytes: the truncation is defined on [0, 1] only)
    want8, want16, wanty = fpc.to_out8(finite(x), src), fpc.to_out16(x, src, 1023), fpc.to_out_yuv(x, src, 10)
    x[:, :, src[0]:, :], x[:, :, :, src[1]:] = 0.25, float("nan")
    assert np.array_equal(fpc.to_out8(finite(x), src), want8) and np.array_equal(fpc.to_out16(x, src, 1023), want16)
    assert np.array_equal(fpc.to_out_yuv(x, src, 10), wanty)


# --------------------------------------------------------------------------------------------------------------------- hold-out
class _LinearModel:
    scale, pad_size = 1.0, 16

    def inference_ts(self, I0, I1, ts):
        return [I0 if t == 0 else I1 if t == 1 else I0 + float(t) * (I1 - I0) for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False, **kw):
        return [(I0, I1, I2)[int(t)] if t in (0, 1, 2) else I0 + float(t) * (I1 - I0) if t < 1 else I1 + (float(t) - 1) * (I2 - I1)
                for t in ts], None


def test_holdout_names_the_mode_and_kept_frames_come_back_exactly():
    frames = np.random.default_rng(9).integers(0, 256, size=(7, 12, 20, 3), dtype=np.uint8)
    to_inp, to_out, _ = fpc.cpu_hooks8()
    res = evaluate.holdout(_LinearModel(), frames, 3, backend=mc.NumpyBackend(), to_inp=to_inp, to_out=to_out, fit="pad")
    rep = evaluate.holdout_report(res)
    json.dumps(evaluate._jsonable(rep))
    assert res["fit"] == "pad" and rep["fit"] == "pad"
    assert res["kept"]["summary"]["max_lsb"] == 0  # padded to 16 x 32 and cropped: the kept frames are the source's bytes
    res = evaluate.holdout(_LinearModel(), frames, 3, backend=mc.NumpyBackend(), to_inp=to_inp, to_out=to_out)
    assert res["fit"] == "resize" and evaluate.holdout_report(res)["fit"] == "resize"
    with pytest.raises(ValueError, match="fit"):
        evaluate.holdout(_LinearModel(), frames, 3, backend=mc.NumpyBackend(), to_inp=to_inp, to_out=to_out, fit="stretch")


# ------------------------------------------------------------------------------------------------------------ the sharded run
class _FakeModel:
    """tests/test_parallel.py's stand-in: outputs depend on the carried `reuse` state, so a wrong halo or cut state shows"""
    scale, pad_size = 1.0, 16

    def calc_flow(self, a, b):
        return a - b, b - a * 0.5, a * 2.0, b * 3.0

    def inference_ts(self, I0, I1, ts):
        return [I0 if t == 0 else I1 if t == 1 else (1 - t) * I0 + t * I1 for t in ts]

    def inference_ts_drba(self, I0, I1, I2, ts, reuse=None, linear=False):
        flow10, _, f1, _ = self.calc_flow(I1, I0) if not reuse else reuse
        flow12, flow21, f1b, f2 = self.calc_flow(I1, I2)
        out = []
        for t in ts:
            if t in (0, 1, 2):
                out.append((I0, I1, I2)[int(t)])
            else:
                out.append((I1 + 0.1 * flow10 * (1 - t) + 0.05 * flow12 * t + 0.01 * f1).clamp(0, 1))
        return out, (flow21, flow12, f2, f1b)


def _shard_clip():
    return np.random.default_rng(11).integers(0, 256, size=(7, 27, 45, 3), dtype=np.uint8)


def _cpu_tools(seen):
    """tools.to_inp / to_out on the CPU: the restatement where fit says pad, a refusal otherwise (the default hooks of a --fit pad
    run must carry the keyword)"""
    def to_inp(fr, size, fit="resize", **kw):
        assert fit == "pad" and not kw, (fit, kw)
        seen["to_inp"] += 1
        return fpc.to_inp8(fr, size)

    def to_out(x, size, fit="resize", **kw):
        assert fit == "pad" and not kw, (fit, kw)
        seen["to_out"] += 1
        return fpc.to_out8(x, size)

    return to_inp, to_out


def _sharded_worker(rank, world, port, tmp, q):
    import oracle
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    seen = {"to_inp": 0, "to_out": 0}
    tools.to_inp, tools.to_out = _cpu_tools(seen)  # this process only: the defaults inference_sharded builds go through them
    args = argparse.Namespace(input=os.path.join(tmp, "in.npz"), output=os.path.join(tmp, "sharded.npz"), dst_fps=60.0, times=-1,
                              enable_scdet=True, scdet_threshold=0.3, hwaccel=False, fit="pad")
    n = drv.inference_sharded(_FakeModel(), args, rank, world, check_scene=oracle.scdet.check_scene, chunk=2)
    assert seen["to_inp"] > 0 and seen["to_out"] > 0
    if rank == 0:
        from tests.clip_common import ListIO
        io = ListIO(list(_shard_clip()), 24.0)
        to_inp, to_out, check = fpc.cpu_hooks8()
        drv.interpolate_stream(_FakeModel(), io, 60.0, times=-1, enable_scdet=True, to_inp=to_inp, to_out=to_out, check_scene=check)
        z = np.load(args.output)
        same = z["frames"].shape[0] == n == len(io.written) and all(np.array_equal(a, b) for a, b in zip(z["frames"], io.written))
        q.put((same, n, len(io.written), tuple(z["frames"].shape[1:])))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_pad_run_writes_the_sequential_pad_runs_file(tmp_path):
    """gloo, world 2, --fit pad through inference_sharded's own default hooks (27 x 45 frames padded to 32 x 48): rank 0's file
    equals the sequential driver's frames with the CPU pad hooks."""
    np.savez(os.path.join(tmp_path, "in.npz"), frames=_shard_clip(), fps=np.float64(24.0))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    same, n, n_seq, shape = q.get(timeout=10)
    assert n == n_seq and shape == (27, 45, 3)
    assert same, "the sharded --fit pad file differs from the sequential pad run"
