"""GPU: the fused non-linear DRM of the RIFE path (splat kernels, MODE 2) and the non-linear driver run built on it.

Kernel: against the oracle's two branches under the rule drm_rife_linear is held to (tests/decisions.py), the retimed ratio u
bit for bit against the composition's drm_retime(drm_ratio), the batched entry against the single one, the self-cleaning
accumulator.  Model / driver / CLI: a grouped non-linear run takes the same path as a linear one, launches neither the generic
splat nor drm_retime_kernel and equals the oracle's step-by-step chain; a step computed ahead in one mode is never handed to a
call in the other."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from drba_amd.utils import synth
from tests import decisions
from tests.clip_common import ListIO, cpu_hooks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HS, WS = 70, 150
FLOWS = ("smooth", "tiny", "mid", "long", "nan", "converge", "pinch")


@functools.lru_cache(maxsize=None)
def flows():
    """The seven flows of gpu_checks.check_glue at 70 x 150 (every path of the sorted tile kernel) and the other direction's flow."""
    g = torch.Generator().manual_seed(7)
    ys, xs = torch.meshgrid(torch.arange(HS, dtype=torch.float32), torch.arange(WS, dtype=torch.float32), indexing="ij")
    smooth = F.interpolate(torch.randn(1, 2, 5, 9, generator=g) * 5, size=(HS, WS), mode="bilinear")
    nanf = smooth.clone()
    nanf[0, 0, 7, 9] = float("nan")
    nanf[0, 1, 30, 100] = float("inf")
    out = {"smooth": smooth,
           "tiny": smooth * 0.15, "mid": smooth * 0.45,  # every tile's neighbourhood reaches <= 4 / <= 8 pixels: the smaller source windows
           "long": smooth * 6,                            # beyond the 16-px tile halo: the global-atomic pre-pass
           "nan": nanf,
           "converge": torch.stack([-0.75 * (xs - WS / 2 + 0.3), -0.75 * (ys - HS / 2 + 0.2)]).unsqueeze(0),
           # all sources within the halo of the tile at x 64..95, y 32..47 pulled into it: more records than the 1536 LDS holds
           "pinch": torch.stack([-0.45 * (xs - 79.5), -0.6 * (ys - 39.5)]).unsqueeze(0)}
    other = F.interpolate(torch.randn(1, 2, 5, 9, generator=g) * 4, size=(HS, WS), mode="bilinear")
    return {k: v.contiguous() for k, v in out.items()}, other.contiguous()


@functools.lru_cache(maxsize=None)
def reference(fname, tt):
    """The oracle's two branches of calc_drm_rife(tt, flow, other, linear=False)["drm_t1_t01"], its hole mask and the pixels on
    which the reference alone does not agree with itself (decisions.unstable).  Computed once per (flow, t), never modified."""
    import oracle
    fl, other = flows()[0][fname], flows()[1]

    def hole_of(f_self, f_other):
        d10, d12 = decisions._ratio_maps(f_self, f_other, 1e-4)
        u1 = decisions._retime(d12, tt, False)
        return {"hole": oracle.ops.softsplat(d10 * 0 + 1, f_self * u1, None, "avg") < decisions.HOLE}

    _, d12 = decisions._ratio_maps(fl, other, 1e-4)
    u1 = decisions._retime(d12, tt, False)
    m, u = decisions.unstable(hole_of, [fl, other])
    aligned = oracle.ops.softsplat(u1, fl * u1, None, "avg")
    refd = oracle.drm.calc_drm_rife(tt, fl, other, False)["drm_t1_t01"]
    # the branches ARE the oracle's
    assert torch.equal(torch.nan_to_num(torch.where(m["hole"], u1, aligned)), torch.nan_to_num(refd)), (fname, tt)
    return {"aligned": aligned, "u": u1, "hole": m["hole"], "unstable": u["hole"]}


def _assert_rows(rows):
    for n, e, t, x in rows:
        print(f"{n}: err={e:.3e} tol={t:.1e} {x}")
    bad = [(n, e, t, x) for n, e, t, x in rows if not e <= t]
    assert not bad, "\n".join(f"{n}: err={e:.3e} tol={t:.1e} {x}" for n, e, t, x in bad)


def _accumulator_is_zero(dev):
    """The fused splats' shared workspace past the reach map (scratch): zero on entry, zero again on return."""
    from drba_amd import ops
    zws = ops._zero_workspace(dev, 1)
    head = ops._lib.load().drba_rife_splat_ws_floats(1, 1, 1, 1) - 3
    return float(zws[head:].abs().max()) == 0.0


@pytest.mark.parametrize("fname", FLOWS)
def test_kernel_against_the_oracles_two_branches(hip_backend, fname):
    """2e-5, the linear kernel's tolerance (the arithmetic after u is the same); the unstable share stays a condition."""
    from drba_amd import ops
    dev = hip_backend.dev
    fl, other = flows()[0][fname].to(dev), flows()[1].to(dev)
    rows = []
    for tt in (0.25, 0.8, 0.1) + ((0.5,) if fname == "smooth" else ()):  # 0.5: no move, u = r
        ref = reference(fname, tt)
        got = ops.drm_rife_nonlinear(fl, other, tt, 1e-4)
        assert tuple(got.shape) == (1, 1, HS, WS)
        rows += decisions.two_branch_rows(f"drm_rife_nonlinear {fname} t={tt}", got, ref["aligned"], ref["u"], ref["hole"],
                                          ref["unstable"], 2e-5)
    _assert_rows(rows)
    assert _accumulator_is_zero(dev)


@pytest.mark.parametrize("tt", [0.1, 0.5, 1 / 3])
def test_retimed_ratio_is_the_compositions_bit_for_bit(hip_backend, tt):
    """On a stable hole the kernel stores u itself: it must be drm_retime(drm_ratio(...)) of the composition to the last bit
    (1/3: both updates in every iteration; 0.5: no update)."""
    from drba_amd import ops
    dev = hip_backend.dev
    seen = 0
    for fname in FLOWS:
        ref = reference(fname, tt)
        fl, other = flows()[0][fname].to(dev), flows()[1].to(dev)
        got = ops.drm_rife_nonlinear(fl, other, tt, 1e-4)
        u = ops.drm_retime(ops.drm_ratio(fl, other, 1e-4)[1], tt)
        sel = (ref["hole"] & ~ref["unstable"]).to(dev)
        a, b = got[sel], u[sel]
        same = (a.view(torch.int32) == b.view(torch.int32)) | (a.isnan() & b.isnan())
        assert bool(same.all()), (fname, tt, int((~same).sum()), int(sel.sum()))
        seen += int(sel.sum())
    assert seen > 1000, seen  # (long / converge / pinch leave large uncovered regions)


def test_batch_equals_singles(hip_backend):
    """drba_drm_rife_nonlinear_batch against drba_drm_rife_nonlinear per map, every job with a walk of its own, on the shapes of
    test_drm_maps_of_a_group_in_one_launch_equal_the_single_calls and with its summation-order allowance."""
    from drba_amd import ops
    dev = hip_backend.dev
    g = torch.Generator().manual_seed(17)
    for (h, w, amp, n) in ((70, 90, 3.0, 3), (128, 256, 40.0, 8), (64, 96, 2.0, 11)):
        jobs = []
        for k in range(n):
            a, b = torch.randn(1, 2, h, w, generator=g) * amp, torch.randn(1, 2, h, w, generator=g) * amp
            if k == 1:
                a[0, 0, 5, 7], b[0, 1, 9, 3] = float("nan"), float("inf")
            jobs.append((a.to(dev), b.to(dev), 0.5 if k == 2 else 0.1 + 0.07 * k))
        many = ops.drm_rife_nonlinear_many(jobs, 1e-4)
        assert len(many) == n
        for (a, b, t), m in zip(jobs, many):
            one = ops.drm_rife_nonlinear(a, b, t, 1e-4)
            assert torch.equal(torch.isnan(one), torch.isnan(m)), (h, w, amp, t)
            d = float((torch.nan_to_num(one, nan=0.0) - torch.nan_to_num(m, nan=0.0)).abs().max())
            assert d <= 2e-6 * max(1.0, float(torch.nan_to_num(one, nan=0.0).abs().max())), (h, w, amp, t, d)
    assert _accumulator_is_zero(dev)


def test_accumulator_is_left_zeroed_after_the_atomic_paths(hip_backend):
    """Long flows (pre-pass) and a pinch (spill beyond the LDS records) go through the global accumulator, single and batched."""
    from drba_amd import ops
    dev = hip_backend.dev
    fs, other = flows()
    o = other.to(dev)
    jobs = [(fs[k].to(dev), o, t) for k, t in (("long", 0.1), ("pinch", 0.8), ("converge", 0.25), ("long", 0.5))]
    for a, b, t in jobs:
        ops.drm_rife_nonlinear(a, b, t, 1e-4)
    ops.drm_rife_nonlinear_many(jobs, 1e-4)
    ops.drm_rife_nonlinear(torch.cat([j[0] for j in jobs]), torch.cat([j[1] for j in jobs]), 0.4, 1e-4)  # N = 4, one tensor
    torch.cuda.synchronize()
    assert _accumulator_is_zero(dev)


def test_walk_beyond_the_mask_runs_the_composition(hip_backend):
    """A precision whose walk the 32-bit mask cannot hold: ops answers with the composition of the generic operators."""
    from drba_amd import ops
    dev = hip_backend.dev
    fl, other = flows()[0]["smooth"].to(dev), flows()[1].to(dev)
    assert ops.drm_walk(0.3, 1e-12) is None and ops.drm_walk(0.3, 1e-3) is not None
    got = ops.drm_rife_nonlinear(fl, other, 0.3, 1e-4, precision=1e-12)
    fused = ops.drm_rife_nonlinear(fl, other, 0.3, 1e-4, precision=1e-9)  # 30 moves: still the kernel
    assert float((got - fused).abs().max()) <= 2e-5


# ----------------------------------------------------------------------------------------------------- model, driver, CLI
H, W = 64, 128
KEYS = ("groups_formed", "group_collects", "staged_groups", "single_steps")


def _to_inp(dev):
    def to_inp(fr, size):
        assert tuple(size) == (H, W)
        return torch.from_numpy(np.ascontiguousarray(fr).transpose(2, 0, 1)).unsqueeze(0).float().div(255.0).to(dev)
    return to_inp


def _drive(model, frames, dev, linear):
    from drba_amd import infer as drv
    io = ListIO(list(frames), 24.0)
    drv.interpolate_stream(model, io, 48.0, times=2, to_inp=_to_inp(dev), to_out=lambda x, size: x.detach().float().cpu().clone(),
                           linear=linear)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return io.written


def test_grouped_nonlinear_run(hip_backend, oracle_backend):
    """driver.run at -t 2 over 10 frames, GROUP = 4, linear=False: the path counters of the linear run, no generic-splat and no
    drm_retime_kernel launch, and every emitted frame within test_rife_end_to_end_parity's 1e-3 of the oracle's step-by-step
    non-linear chain."""
    from drba_amd import ops
    dev = hip_backend.dev
    sd = synth.ifnet_state_dict(0)
    frames = synth.make_clip(10, H, W)

    def run(linear, traced=False):
        m = hip_backend.make_rife(sd, 1.0)
        m.GROUP = 4
        if traced:
            ops.trace_begin()
        try:
            out = _drive(m, frames, dev, linear)
        finally:
            recs = ops.trace_end() if traced else None
        return out, dict(m.stats), recs

    lin, st_lin, _ = run(True)   # (the conv tuner meets every shape here)
    got, st_nl, recs = run(False, traced=True)
    print("linear", st_lin, "\nnon-linear", st_nl)
    assert {k: st_nl[k] for k in KEYS} == {k: st_lin[k] for k in KEYS}
    assert st_nl["groups_formed"] >= 1 and st_nl["group_collects"] >= 3 and st_nl["groups_dropped"] == 0
    names = [r["name"] for r in recs]
    assert any(n.startswith("splat_tiled<2>") for n in names) and any(n.startswith("splat_long_prepass<2>") for n in names)
    banned = ("splat_sort", "scan_", "drm_retime_kernel", "drm_ratio_kernel", "fill_holes_kernel", "splat_tiled<1>", "splat_long_prepass<1>")
    assert not [n for n in names if n.startswith(banned)], sorted({n for n in names if n.startswith(banned)})
    want = _drive(oracle_backend.make_rife(sd, 1.0), frames, torch.device("cpu"), False)
    assert len(got) == len(want) == len(lin) == 20
    errs = [float((a - b).abs().max()) for a, b in zip(got, want)]
    print("max |hip - oracle| per frame", errs)
    assert max(errs) <= 1e-3, errs
    assert any(not torch.equal(a, b) for a, b in zip(got, lin))  # (the linear run is another computation)


def test_modes_do_not_mix(hip_backend):
    """A group announced and computed with linear=True; the next step asked with linear=False is not collected: the step
    computed ahead is dropped and the call computes its own, equal to a non-linear chain on a fresh model to what
    test_step_groups_match_single_steps allows between a grouped and a step-by-step computation (1e-5: summation order, the
    tuner's tiling for another batch size) and further than that from the linear frames."""
    dev = hip_backend.dev
    sd = synth.ifnet_state_dict(0)
    ts = np.array([0.6, 1.4])
    base = [_to_inp(dev)(f, (H, W)) for f in synth.make_clip(6, H, W, seed=31)]

    def chain(linear):
        m = hip_backend.make_rife(sd, 1.0)
        fr = [f.clone() for f in base]
        _, r = m.inference_ts_drba(fr[0], fr[1], fr[2], ts, None, linear)
        _, r = m.inference_ts_drba(fr[1], fr[2], fr[3], ts, r, linear)
        out, _ = m.inference_ts_drba(fr[2], fr[3], fr[4], ts, r, linear)
        return out

    m = hip_backend.make_rife(sd, 1.0)
    m.GROUP = 4
    fr = [f.clone() for f in base]
    _, r0 = m.inference_ts_drba(fr[0], fr[1], fr[2], ts, None, True)
    _, r1 = m.inference_ts_drba(fr[1], fr[2], fr[3], ts, r0, True, lookahead=(fr[4], ts, fr[5], ts))
    assert m.stats["groups_formed"] == 1 and len(m._group_out) == 2
    before = dict(m.stats)
    out, _ = m.inference_ts_drba(fr[2], fr[3], fr[4], ts, r1, False)
    assert m.stats["group_collects"] == before["group_collects"] and m.stats["groups_dropped"] == before["groups_dropped"] + 1
    assert m.stats["single_steps"] == before["single_steps"] + 1 and not m._group_out
    want, linear = chain(False), chain(True)
    torch.cuda.synchronize()
    d_nl = max(float((a - b).abs().max()) for a, b in zip(out, want))
    d_lin = max(float((a - b).abs().max()) for a, b in zip(out, linear))
    print("to the non-linear chain", d_nl, "to the linear chain", d_lin)
    assert d_nl <= 1e-5 and d_lin > 1e-5
    # ... and the other way round: the same call in the group's own mode is collected
    m2 = hip_backend.make_rife(sd, 1.0)
    m2.GROUP = 4
    fr = [f.clone() for f in base]
    _, r0 = m2.inference_ts_drba(fr[0], fr[1], fr[2], ts, None, False)
    _, r1 = m2.inference_ts_drba(fr[1], fr[2], fr[3], ts, r0, False, lookahead=(fr[4], ts, fr[5], ts))
    out2, _ = m2.inference_ts_drba(fr[2], fr[3], fr[4], ts, r1, False)
    assert m2.stats["group_collects"] == 1 and m2.stats["groups_dropped"] == 0
    assert max(float((a - b).abs().max()) for a, b in zip(out2, want)) <= 1e-5


def _cli_clip(tmp_path, name, frames, argv):
    wdir = tmp_path / "w"
    wdir.mkdir(exist_ok=True)
    torch.save({"module." + k: v for k, v in synth.ifnet_state_dict(0).items()}, str(wdir / "flownet.pkl"))
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / name)
    np.savez(inp, frames=np.stack(frames), fps=np.float64(24.0))
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import drba_amd.infer as I\n"
        "a = I.parse_args(['-m','rife','-i',%r,'-o',%r] + %r)\n"
        "m = I.load_model(a.model_type, a.scale, weights=%r)\n"
        "print('written', I.inference(m, a))\n" % (ROOT, inp, out, list(argv), str(wdir)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)["frames"]


def test_cli_nonlinear(tmp_path):
    """`infer.py -m rife -t 2 --nonlinear` on a 6-frame 64 x 128 clip: as many frames as without the flag, within 1 LSB of the
    driver run with linear=False on the CPU oracle, and not the linear run's frames."""
    import oracle
    from drba_amd import infer as drv
    frames = synth.make_clip(6, H, W, seed=41)
    got = _cli_clip(tmp_path, "nl.npz", frames, ["-t", "2", "--nonlinear"])
    lin = _cli_clip(tmp_path, "lin.npz", frames, ["-t", "2"])
    assert got.shape == lin.shape == (12, H, W, 3) and got.dtype == np.uint8
    io = ListIO(list(frames), 24.0)
    to_inp, to_out, check = cpu_hooks()
    drv.interpolate_stream(oracle.rife.RifeOracle(synth.ifnet_state_dict(0), 1.0), io, 48.0, times=2, to_inp=to_inp, to_out=to_out,
                           check_scene=check, linear=False)
    want = np.stack(io.written)
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print("max LSB", d.max(), "share differing", (d > 0).mean(), "bytes differing from the linear run", int((got != lin).sum()))
    assert d.max() <= 1, f"max diff {d.max()} LSB"
    assert not np.array_equal(got, lin)
