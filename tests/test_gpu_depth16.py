"""GPU: 16-bit frames -- the conversion kernels (frame_io.hip: drba_to_inp16_x4, drba_to_out16 and the no-resize pair) bit for
bit against the CPU restatement of tests/depth16_common.py (and their 8-bit siblings, which share their bodies, at the same
shapes against the same resize), the identity of the round trip, drba_frame_error_u16 against numpy
int64, the "u16" kind of drba_amd.metrics, a whole clip through interpolate_stream against the CPU oracle driver, and the command
lines.  Shapes are the smallest that reach each kernel form (the form a call took is read from the launch trace)."""
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
from drba_amd.models.utils import tools
from drba_amd.utils import synth
from tests import depth16_common as d16
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


def _traced(fn):
    """fn() with the launch trace on -> (its result, the kernel names it launched)"""
    ops.trace_begin()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        recs = ops.trace_end()
    return out, [r["name"] for r in recs]


def _frame16(h, w, maxval, seed):
    f = np.random.default_rng(seed).integers(0, maxval + 1, size=(h, w, 3), dtype=np.uint16)
    f[0, 0], f[-1, -1] = (0, maxval, maxval // 2), (maxval, 0, 1)
    return f


# ------------------------------------------------------------------------------------------------------- conversion kernels
# (src size, net size, the kernel form both directions must take)
GEOMETRIES = [((45, 70), (64, 128), "one-pixel"), ((60, 64), (64, 64), "rows"), ((60, 66), (64, 66), "one-pixel")]


@pytest.mark.parametrize("maxval", [65535, 1023])
@pytest.mark.parametrize("src,net,form", GEOMETRIES)
def test_to_inp16_to_out16_bit_exact_against_the_cpu_restatement(dev, src, net, form, maxval):
    """Every fp32 value of to_inp and every 16-bit sample of to_out(depth=16) equal to the restatement's, in both kernel forms, with
    rev on and off, and with NaN / +inf / -0.5 / 1.5 planted in the frame on the way out.  What a planted value becomes after a
    RESIZE is the restatement's business (ATen blends it with its neighbours, and takes 1 * inf + 0 * inf = NaN on an axis whose
    size does not change); the rule itself -- 0, maxval, 0, maxval -- is asserted where the four taps of an output sample all lie
    inside a planted block (the general geometry) and, sample for sample, through the no-resize pair in the identity test."""
    f = _frame16(src[0], src[1], maxval, seed=src[1] + maxval)
    want = d16.to_inp16_ref(f, net, maxval)
    got, names = _traced(lambda: ops.to_inp(torch.from_numpy(f).to(dev), net, maxval=maxval))
    assert [("rows" if "rows" in n else "one-pixel") for n in names if "to_inp16" in n] == [form], names
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    x4 = ops._x4_of(got)
    assert x4 is not None and tuple(x4.shape) == (net[0], net[1], 4)
    assert torch.equal(x4[:, :, :3].cpu(), want[0].permute(1, 2, 0)) and not bool(x4[:, :, 3].any())
    assert torch.equal(tools.to_inp(f, net, maxval=maxval).cpu(), want)  # the host-frame entry

    x = want.clone()
    x[0, 0, 20:30, 40:56], x[0, 1, 20:30, 40:56], x[0, 2, 20:30, 40:56], x[0, 0, 40:50, 40:56] = float("nan"), float("inf"), -0.5, 1.5
    x[0, 1, 3, 7], x[0, 2, 50, 9], x[0, 0, 63, net[1] - 1], x[0, 2, 0, 0] = float("nan"), float("inf"), -0.5, 1.5  # single samples
    for rev in (False, True):
        ref = d16.to_out16_ref(x, src, maxval, rev=rev)
        back, names = _traced(lambda: ops.to_out(x.to(dev), src, rgb=rev, depth=16, maxval=maxval))
        assert [("rows" if "rows" in n else "one-pixel") for n in names if "to_out16" in n] == [form], names
        assert back.dtype == torch.uint16 and tuple(back.shape) == (src[0], src[1], 3)
        b = back.cpu().numpy()
        assert np.array_equal(b, ref), (rev, int(np.abs(b.astype(np.int64) - ref.astype(np.int64)).max()), int((b != ref).sum()))
        assert np.array_equal(tools.to_out(x.to(dev), src, rgb=rev, depth=16, maxval=maxval), ref)
    if src == (45, 70):  # output (17, 26) reads rows 24, 25 and columns 47, 48; output (31, 26) rows 44, 45: inside the blocks
        b = ops.to_out(x.to(dev), src, depth=16, maxval=maxval).cpu().numpy()
        assert b[17, 26].tolist() == [0, maxval, 0] and b[31, 26, 0] == maxval


@pytest.mark.parametrize("src,net,form", GEOMETRIES)
def test_to_inp_to_out_8bit_bit_exact_in_both_forms(dev, src, net, form):
    """The byte kernels at the shapes of the 16-bit test, in every bit: to_inp against resize(frame / 255) with the loop ATen runs
    on frames (d16.resize), its [H,W,4] copy against its own planar result, and to_out of a finite frame slightly outside [0, 1]
    -- truncation and wrap-around -- with rgb off and on against (resize(x) * 255.).astype(uint8), the form read from the trace."""
    g = torch.Generator().manual_seed(src[0] * 1000 + src[1])
    f = torch.randint(0, 256, (src[0], src[1], 3), dtype=torch.uint8, generator=g)
    want = d16.resize(f.permute(2, 0, 1).unsqueeze(0).float() / 255, net)
    got, names = _traced(lambda: ops.to_inp(f.to(dev), net))
    assert [("rows" if "rows" in n else "one-pixel") for n in names if "to_inp_" in n] == [form] and not [n for n in names if "16" in n], names
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    x4 = ops._x4_of(got)
    assert x4 is not None and tuple(x4.shape) == (net[0], net[1], 4)
    assert torch.equal(x4[:, :, :3], got[0].permute(1, 2, 0)) and not bool(x4[:, :, 3].any())

    x = torch.rand(1, 3, net[0], net[1], generator=g) * 1.02 - 0.01
    assert bool(torch.isfinite(x).all()) and float(x.min()) < 0.0 and float(x.max()) > 1.0
    ref = (d16.resize(x, src)[0].numpy().transpose(1, 2, 0) * 255.).astype(np.uint8)
    for rev in (False, True):
        back, names = _traced(lambda: ops.to_out(x.to(dev), src, rgb=rev))
        assert [("rows" if "rows" in n else "one-pixel") for n in names if "to_out_" in n] == [form] and not [n for n in names if "16" in n], names
        assert back.dtype == torch.uint8 and tuple(back.shape) == (src[0], src[1], 3)
        du = np.abs(back.cpu().numpy().astype(np.int32) - (ref[:, :, ::-1] if rev else ref).astype(np.int32))
        du = np.minimum(du, 256 - du)  # uint8 wrap-around of slightly negative / > 1 values
        assert int(du.max()) == 0, (rev, int(du.max()), int((du != 0).sum()))


@pytest.mark.parametrize("maxval", [65535, 1023])
def test_round_trip_is_the_identity_for_every_sample_value(dev, maxval):
    """A square frame holding each value 0 .. maxval in every channel, same size in and out: to_out16(to_inp16(v)) == v for every
    sample, through the resize kernels (the row form here: W % 4 == 0) and through the no-resize pair; and the rounding rule of
    the way out on planted values, sample for sample."""
    v = d16.all_values_frame(maxval)
    size = v.shape[:2]
    t = torch.from_numpy(v).to(dev)
    x = ops.to_inp(t, size, maxval=maxval)
    assert torch.equal(x.cpu(), d16.planar16(v, maxval))
    for rev in (False, True):
        back = ops.to_out(x, size, rgb=rev, depth=16, maxval=maxval).cpu().numpy()
        assert np.array_equal(back, v[:, :, ::-1] if rev else v)
    y = ops.u16hwc_to_f32nchw(t, maxval)
    assert torch.equal(y.cpu(), d16.planar16(v, maxval))
    assert np.array_equal(ops.f32nchw_to_u16hwc(y, maxval).cpu().numpy(), v)
    assert np.array_equal(tools.to_cv2(tools.to_tensor(v, maxval=maxval), depth=16, maxval=maxval), v)
    # a width that is no multiple of 4 takes the one-pixel kernels: the same identity
    odd = np.ascontiguousarray(v[:, :size[1] - 2])
    assert np.array_equal(ops.to_out(ops.to_inp(torch.from_numpy(odd).to(dev), odd.shape[:2], maxval=maxval), odd.shape[:2], depth=16,
                                     maxval=maxval).cpu().numpy(), odd)
    # the rule: NaN -> 0, +inf -> maxval, -0.5 -> 0, 1.5 -> maxval, -inf -> 0, halves to even
    z = torch.zeros(1, 3, 4, 4)
    vals = [float("nan"), float("inf"), -0.5, 1.5, float("-inf"), 0.5 / maxval, 1.5 / maxval, 2.5 / maxval, 1.0, 0.0, -0.0, 1e-9]
    z.view(-1)[:len(vals)] = torch.tensor(vals)
    got = ops.f32nchw_to_u16hwc(z.to(dev), maxval).cpu().numpy()
    assert np.array_equal(got, d16.quantise16(z, maxval))
    flat = got.transpose(2, 0, 1).reshape(-1)[:len(vals)].tolist()
    assert flat[:5] == [0, maxval, 0, maxval, 0] and flat[8:] == [maxval, 0, 0, 0]
    assert flat[5:8] == d16.quantise16(z, maxval).transpose(2, 0, 1).reshape(-1)[5:8].tolist()
    # through the same-size resize kernel the restatement (ATen) turns an inf into 1 * inf + 0 * inf = NaN -> 0: matched too
    assert np.array_equal(ops.to_out(z.to(dev), (4, 4), depth=16, maxval=maxval).cpu().numpy(), d16.to_out16_ref(z, (4, 4), maxval))


# -------------------------------------------------------------------------------------------------------- frame differences
def test_frame_error_u16_is_bit_exact_and_repeats(dev):
    lib = _lib.load()

    def fn(a, b, N, n, off_a, off_b):
        bufs = []
        for x, off in ((a, off_a), (b, off_b)):
            t = torch.zeros(off + N * n + 64, dtype=torch.int16, device=dev)  # (uint16 bits in int16 storage: slicing, copies)
            t[off:off + N * n] = torch.from_numpy(x.view(np.int16)).to(dev)
            bufs.append(t[off:off + N * n])
            assert bufs[-1].data_ptr() % 16 == (2 * off) % 16
        ws = torch.empty(int(lib.drba_frame_error_u16_ws_floats(N, n)), dtype=torch.float32, device=dev)
        outs = []
        for _ in range(2):
            out = torch.full((N, 4), -1, dtype=torch.int64, device=dev)
            _lib.check(lib.drba_frame_error_u16(_p(bufs[0]), _p(bufs[1]), _p(out), _p(ws), N, n, ops._stream()), "drba_frame_error_u16")
            outs.append(out.cpu().numpy())
        assert outs[0].tobytes() == outs[1].tobytes()  # two runs: the same bits
        return outs[0]

    rows = d16.check_frame_error_u16(fn)
    for name, err, tol, extra in rows:
        print(f"{name:60s} err={err:.3e} tol={tol:.1e} {extra}")
    assert not [(r[0], r[1]) for r in rows if not r[1] <= r[2]]
    big = [r for r in rows if "2^48" in r[0]]
    assert big and 70000 * 65535 ** 2 > 2 ** 48


# --------------------------------------------------------------------------------------------------------- public interface
def test_metrics_take_uint16_host_and_device_frames(dev):
    for maxval in (65535, 1023):
        a, b = (synth.make_clip16(2, 45, 70, seed=31, maxval=maxval)[k] for k in (0, 1))
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        want = {"sum_sq": int((d * d).sum()), "sum_abs": int(d.sum()), "max_abs": int(d.max()), "differing": int((d != 0).sum()), "n": d.size}
        truth = float(mc.ssim_truth(d16.planar16(a, maxval), d16.planar16(b, maxval))[0])
        kw = {} if maxval == 65535 else {"maxval": maxval}
        for x, y in ((a, b), (torch.from_numpy(a), torch.from_numpy(b)), (torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))):
            assert metrics.frame_error(x, y) == want
            p = metrics.psnr(x, y, **kw)
            assert isinstance(p, float) and p == metrics.psnr_of_mse(want["sum_sq"] / d.size, float(maxval))  # exact, from the integer sums
            s = metrics.ssim(x, y, **kw)
            print(f"maxval {maxval}: ssim {s:.8f} truth {truth:.8f}")
            assert isinstance(s, float) and abs(s - truth) <= mc.SSIM_TOL
        assert metrics.psnr(a, a, **kw) == math.inf and metrics.ssim(a, a, **kw) == 1.0
        assert metrics.psnr(a, b, peak=2.0, **kw) == metrics.psnr_of_mse(want["sum_sq"] / d.size, 2.0)
    two = metrics.frame_error(np.stack([a, b]), np.stack([b, b]))
    assert two[0] == want and two[1]["sum_sq"] == 0
    with pytest.raises(ValueError):
        metrics.psnr(a, (a >> 2).astype(np.uint8))  # kinds do not mix


def test_clip_metrics_on_uint16_pairs_enqueues_without_waiting(dev):
    host = synth.make_clip16(5, 64, 96, seed=5)
    frames = [torch.from_numpy(f).to(dev) for f in host]
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
    assert r["peak"] == 65535.0 and r["frames"] == 5
    for k in range(4):
        d = np.abs(host[k].astype(np.int64) - host[k + 1].astype(np.int64))
        assert r["per_frame"]["differing"][k] == int((d != 0).sum()) and r["per_frame"]["max_lsb"][k] == int(d.max())
        assert r["per_frame"]["psnr"][k] == metrics.psnr_of_mse(float((d * d).mean()), 65535.0)
        truth = float(mc.ssim_truth(d16.planar16(host[k]), d16.planar16(host[k + 1]))[0])
        assert abs(r["per_frame"]["ssim"][k] - truth) <= mc.SSIM_TOL
    assert r["per_frame"]["psnr"][4] == math.inf and r["per_frame"]["ssim"][4] == 1.0
    assert max(r["per_frame"]["max_lsb"]) > 255  # 16-bit steps


# ---------------------------------------------------------------------------------------------------------------- whole clip
def test_whole_clip_16_bit_against_the_cpu_oracle_driver(dev):
    """RIFE on synthetic weights, a 6-frame 128 x 192 make_clip16 clip, -t 2, 16 bits in and out, against the same clip through
    the CPU oracle driver with the restatement's hooks.  The bar is the project's 1e-3 frame tolerance in 16-bit steps,
    |d| <= ceil(1e-3 * 65535) = 66; the measured maximum and the share of differing samples are printed (profiles/depth16.md
    records them), no tighter number is fixed.  128 x 192 is its own network size (pad 64): NO resize is involved, so the two
    pass-through emissions (the copies at head and tail) must be bit-identical to their source frames."""
    import oracle
    from drba_amd import infer as drv
    from drba_amd.models.rife import RIFE
    from tests.clip_common import ListIO
    frames = synth.make_clip16(6, 128, 192, seed=1234)
    assert tools.get_valid_net_inp_size(frames[0], 1.0, div=64)["dst_size"] == (128, 192)
    sd = synth.ifnet_state_dict(seed=0)
    io = ListIO(frames, 24.0)
    n = drv.interpolate_stream(RIFE(weights=sd, scale=1.0, device=dev), io, 48.0, times=2,
                               to_inp=lambda fr, size: tools.to_inp(fr, size, maxval=65535),
                               to_out=lambda x, size: tools.to_out(x, size, depth=16, maxval=65535))
    ref_io = ListIO(frames, 24.0)
    to_inp, to_out, check = d16.cpu_hooks16(65535)
    drv.interpolate_stream(oracle.rife.RifeOracle(sd, 1.0), ref_io, 48.0, times=2, to_inp=to_inp, to_out=to_out, check_scene=check)
    got, want = np.stack(io.written), np.stack(ref_io.written)
    assert n == 12 and got.shape == want.shape == (12, 128, 192, 3) and got.dtype == want.dtype == np.uint16
    for out in (got, want):  # the copies at head and tail
        assert np.array_equal(out[0], frames[0]) and np.array_equal(out[-1], frames[-1])
    synthesised = slice(1, 11)
    # the output is really 16-bit: with continuous values 1 sample in 257 is a multiple of 257 -- first on the oracle's own frames
    share_ref = float((want[synthesised] % 257 != 0).mean())
    share = float((got[synthesised] % 257 != 0).mean())
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(f"whole clip: max |d| = {int(d.max())} steps of 65535 (bar {d16.CLIP_TOL_STEPS}), differing samples {float((d != 0).mean()):.4%}, "
          f"mean |d| = {float(d.mean()):.4f}; not multiples of 257: hip {share:.4%}, oracle {share_ref:.4%}")
    assert share_ref > 0.9, share_ref
    assert share > 0.9, share
    assert int(d.max()) <= d16.CLIP_TOL_STEPS, int(d.max())


# -------------------------------------------------------------------------------------------------------------- command lines
def test_command_lines_at_16_bits(dev, tmp_path):
    """One child process: infer.py --out-depth 16 on an 8-bit clip, the default and --out-depth 8 on a 16-bit clip (4 frames,
    128 x 192: the smallest clip with a DRBA step), evaluate compare on two uint16 clips with planted differences and evaluate
    holdout -k 3 on a 7-frame 16-bit clip."""
    wdir = tmp_path / "w"
    wdir.mkdir()
    torch.save({"module." + k: v for k, v in synth.ifnet_state_dict(0).items()}, str(wdir / "flownet.pkl"))
    f8 = np.stack(synth.make_clip(4, 128, 192, seed=21))
    f16 = np.stack(synth.make_clip16(7, 128, 192, seed=9))
    p8, p16, p16_7 = str(tmp_path / "in8.npz"), str(tmp_path / "in16.npz"), str(tmp_path / "in16_7.npz")
    np.savez(p8, frames=f8, fps=np.float64(24.0))
    np.savez(p16, frames=f16[:4], fps=np.float64(24.0))
    np.savez(p16_7, frames=f16, fps=np.float64(24.0), maxval=np.int64(65535))
    b = f16.copy()
    b[1, 3, 5, 0] ^= 1                                           # one sample, one 16-bit step
    b[2, 10:20, 30:50, :] //= 2                                  # a darkened block
    b[4, 7, 7, 2], f16[4, 7, 7, 2] = 65535, 0                    # the full range (both clips are written after this line)
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    np.savez(pa, frames=f16, fps=np.float64(24.0))
    np.savez(pb, frames=b, fps=np.float64(24.0))
    outs = {k: str(tmp_path / f"out_{k}.npz") for k in ("8to16", "16", "16to8")}
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import drba_amd.infer as I\n"
        "from drba_amd import evaluate\n"
        "m = I.load_model('rife', 1.0, weights=%r)\n"
        "for inp, out, extra in %r:\n"
        "    print('written', I.inference(m, I.parse_args(['-m', 'rife', '-i', inp, '-o', out, '-t', '2'] + extra)))\n"
        "print('exit', evaluate.main(['compare', %r, %r, '--max-lsb', '65535']))\n"
        "print('exit', evaluate.main(['holdout', '-m', 'rife', '-i', %r, '-k', '3']))\n"
        % (ROOT, str(wdir), [(p8, outs["8to16"], ["--out-depth", "16"]), (p16, outs["16"], []), (p16, outs["16to8"], ["--out-depth", "8"])],
           pa, pb, p16_7))
    env = dict(os.environ, DRBA_TUNE_CACHE="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert [ln for ln in lines if ln.startswith("written")] == ["written 8"] * 3 and [ln for ln in lines if ln.startswith("exit")] == ["exit 0"] * 2
    z = np.load(outs["8to16"])
    assert z["frames"].dtype == np.uint16 and z["frames"].shape == (8, 128, 192, 3) and int(z["maxval"]) == 65535 and float(z["fps"]) == 48.0
    assert np.array_equal(z["frames"][0], f8[0].astype(np.uint16) * 257)  # the head copy: v / 255 * 65535 = 257 v exactly
    assert float((z["frames"][1:7] % 257 != 0).mean()) > 0.9              # un-banded output of 8-bit input
    z = np.load(outs["16"])
    assert z["frames"].dtype == np.uint16 and int(z["maxval"]) == 65535 and np.array_equal(z["frames"][0], f16[0]) and np.array_equal(z["frames"][-1], f16[3])
    z8 = np.load(outs["16to8"])
    assert z8["frames"].dtype == np.uint8 and z8["frames"].shape == (8, 128, 192, 3) and "maxval" not in z8.files
    assert np.abs(z8["frames"].astype(np.int64) - (z["frames"].astype(np.int64) * 255 // 65535)).max() <= 1  # the same frames, truncated to bytes
    reps = [json.loads(ln) for ln in lines if ln.startswith("{")]
    cmp_rep, hold = reps[0], reps[1]
    d = np.abs(f16.astype(np.int64) - b.astype(np.int64)).reshape(7, -1)
    assert cmp_rep["depth"] == 16 and cmp_rep["maxval"] == 65535 and cmp_rep["peak"] == 65535.0 and cmp_rep["frames"] == 7
    assert cmp_rep["max_lsb"] == int(d.max()) == 65535 and cmp_rep["total_differing"] == int((d != 0).sum()) and cmp_rep["ok"] is True
    assert cmp_rep["psnr_of_mean_mse"] == pytest.approx(metrics.psnr_of_mse(float((d * d).mean()), 65535.0), rel=1e-12)
    assert hold["depth"] == 16 and hold["k"] == 3 and hold["m"] == 2 and hold["frames_used"] == 7 and hold["emissions"] == 9
    assert hold["held_out"]["positions"] == [1, 2, 4, 5] and hold["kept"]["positions"] == [0, 3, 6] and "synthetic" in hold["weights"]
    assert hold["kept"]["max_lsb"] == 0  # pass-through frames, no resize at this size: bit-identical at 16 bits
    for part in ("kept", "held_out"):
        for key in ("mean_psnr", "psnr_of_mean_mse", "mean_ssim", "min_ssim", "max_lsb"):
            v = float(hold[part][key])
            assert math.isfinite(v) or v == math.inf, (part, key, v)
    assert math.isfinite(float(hold["held_out"]["mean_psnr"])) and hold["held_out"]["max_lsb"] > 0
