"""GPU: the deterministic mode (drba_set_deterministic, ops.set_deterministic, --deterministic).

With the mode on, the bits of an output depend on the bits of the inputs, the geometry and the scalar arguments only: not on
timing (20 launches -> one distinct output), not on the other items of a batch, not on what the workspace held before.  The
accuracy bars of the default mode hold unchanged, the deterministic kernels run under names of their own, and a whole clip through
the command line is byte-identical between runs and processes.  Every test that switches the mode on switches it off again."""
import contextlib
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from drba_amd.utils import synth
from tests import det_common as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = 20
T = {"flow_reverse": 0.0, "drm_rife_linear": 0.5, "drm_rife_nonlinear": 0.8}
CASES = ("noise3", "noise7", "noise15", "long", "pinch", "nan")


@contextlib.contextmanager
def mode(on=True):
    from drba_amd import ops
    was = ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(was)
        assert ops.deterministic() == was


def _digest(t):
    return hashlib.sha1(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _distinct(fn, n=LAUNCHES):
    return len({_digest(fn()) for _ in range(n)})


def _bits_equal(a, b):
    return a.shape == b.shape and _digest(a) == _digest(b)


def _run(op, a, b):
    from drba_amd import ops
    if op == "flow_reverse":
        return ops.flow_reverse(a)
    if op == "drm_rife_linear":
        return ops.drm_rife_linear(a, b, T[op], 1e-4)
    return ops.drm_rife_nonlinear(a, b, T[op], 1e-4)


def _accumulator_is_zero(dev):
    """The fused splats' shared workspace past the reach map (scratch): zero on entry, zero again on return -- in either mode."""
    from drba_amd import ops
    torch.cuda.synchronize()
    return float(ops._zero_workspace(dev, 1)[dc.REACH_WORDS:].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------- fused splats
@pytest.mark.parametrize("op", list(T))
def test_fused_splats_repeat_bit_for_bit(hip_backend, op):
    """20 launches on one input, one distinct output, for every path: the three halo variants, the long pre-pass, the tile whose
    records exceed kCAP, NaN / +-inf.  The conditions are computed on the CPU from the flows alone: at least 20 % of the output
    pixels of every case sum two or more records of one key (71 % for sigma = 1 noise when this was written), the long case holds
    long sources and the pinch tile more records than LDS takes.  At the parent commit this gave 20 distinct of 20."""
    dev = hip_backend.dev
    fl, _ = dc.flows()
    variants = set()
    for name in CASES:
        a, b = fl[name], dc.other_for(name)
        sf = dc.splat_flow(op, a, b, T[op])
        share = dc.multi_term_share(sf)
        assert share >= 0.20, (op, name, share)
        if name == "long":
            assert dc.long_share(sf) > 0.05, (op, dc.long_share(sf))
        if name == "pinch":
            assert dc.tile_records(sf, dc.PINCH_TILE) > dc.CAP, (op, dc.tile_records(sf, dc.PINCH_TILE))
        variants.add(dc.halo_variant(sf))
        ad, bd = a.to(dev), b.to(dev)
        default = _distinct(lambda: _run(op, ad, bd))
        with mode():
            got = _distinct(lambda: _run(op, ad, bd))
        print(f"{op} {name}: multi-term share {share:.2f}; distinct of {LAUNCHES}: default {default} (information), deterministic {got}")
        assert got == 1, (op, name, got)
    assert variants == {4, 8, 16}, variants  # together the cases take every halo variant (some tile of the map does)
    assert _accumulator_is_zero(dev)


@pytest.mark.parametrize("op", list(T))
def test_fused_splats_do_not_depend_on_company(hip_backend, op):
    """An item alone == the same item as the second of N = 3 == the same item as job 5 of an 8-job launch whose other jobs hold
    different data (and, 8 items, no tile of which may borrow another item's reach or accumulator)."""
    from drba_amd import ops
    dev = hip_backend.dev
    fl, _ = dc.flows()
    names = ["noise7", "pinch", "long", "noise15", "nan", "noise3", "noise7", "long"]
    with mode():
        for name in ("long", "pinch", "noise15"):
            a, b = fl[name].to(dev), dc.other_for(name).to(dev)
            alone = _run(op, a, b)
            a3 = torch.cat((fl["noise3"].to(dev), a, fl["nan"].to(dev)))
            b3 = torch.cat((dc.other_for("noise3").to(dev), b, dc.other_for("nan").to(dev)))
            assert _bits_equal(_run(op, a3, b3)[1:2], alone), (op, name, "second of N = 3")
            if op == "flow_reverse":  # (no job form: eight items of one tensor)
                a8 = torch.cat([fl[n].to(dev) for n in names[:5]] + [a] + [fl[n].to(dev) for n in names[6:]])
                assert _bits_equal(ops.flow_reverse(a8)[5:6], alone), (op, name, "sixth of N = 8")
                continue
            jobs = [(fl[n].to(dev), dc.other_for(n).to(dev), 0.1 + 0.1 * k) for k, n in enumerate(names)]
            jobs[5] = (a, b, T[op])
            many = ops.drm_rife_linear_many(jobs, 1e-4) if op == "drm_rife_linear" else ops.drm_rife_nonlinear_many(jobs, 1e-4)
            assert _bits_equal(many[5], alone), (op, name, "job 5 of 8")
    assert _accumulator_is_zero(dev)


def test_fused_splats_do_not_depend_on_workspace_history(hip_backend):
    """A default-mode call, then a deterministic call on the same zeroed buffer == the deterministic call on a buffer fresh from
    the allocator (as at process start), and the accumulator reads all-zero afterwards; then a default-mode call again."""
    from drba_amd import ops
    dev = hip_backend.dev
    fl, _ = dc.flows()
    for op in T:
        for name in ("long", "pinch"):
            a, b = fl[name].to(dev), dc.other_for(name).to(dev)
            _run(op, a, b)
            with mode():
                used = _run(op, a, b)
                assert _accumulator_is_zero(dev)
                kept = dict(ops._zero_ws_cache)
                ops._zero_ws_cache.clear()  # the next call allocates and zeroes a new buffer
                try:
                    fresh = _run(op, a, b)
                    torch.cuda.synchronize()
                finally:
                    ops._zero_ws_cache.clear()
                    ops._zero_ws_cache.update(kept)
            assert _bits_equal(used, fresh), (op, name)
            _run(op, a, b)  # ... and the default mode still finds (and leaves) its zeroes where it expects them
            assert _accumulator_is_zero(dev)


def test_workspace_size_follows_the_mode(hip_backend):
    from drba_amd import _lib
    lib = _lib.load()
    off = [lib.drba_rife_splat_ws_floats(n, 70, 100, v) for n in (1, 8) for v in (1, 2)]
    assert off[0] == dc.REACH_WORDS + 70 * 100 * 2 + 5 * 4  # what it has always returned
    with mode():
        assert lib.drba_get_deterministic() == 1
        on = [lib.drba_rife_splat_ws_floats(n, 70, 100, v) for n in (1, 8) for v in (1, 2)]
    assert lib.drba_get_deterministic() == 0
    assert [lib.drba_rife_splat_ws_floats(n, 70, 100, v) for n in (1, 8) for v in (1, 2)] == off
    for (n, v), a, b in zip(((1, 1), (1, 2), (8, 1), (8, 2)), off, on):
        assert b - a == n * 70 * 100 * (v + 1), (n, v, a, b)  # the accumulator words are twice as wide


# ----------------------------------------------------------------------------------------------------- generic softsplat
SH, SW = 37, 53


def _softsplat_inputs(dev, c, n=1, seed=5):
    g = torch.Generator().manual_seed(seed + c)
    flow = torch.randn(n, 2, SH, SW, generator=g) * 1.5
    ys, xs = torch.meshgrid(torch.arange(SH, dtype=torch.float32), torch.arange(SW, dtype=torch.float32), indexing="ij")
    for k in range(25):  # 25 sources converging on pixel (20, 30) of item 0: a 5 x 5 block, each to a point inside that pixel
        y, x = 8 + k // 5, 11 + k % 5
        flow[0, 0, y, x], flow[0, 1, y, x] = 30.0 + 0.03 * k - x, 20.0 + 0.9 - 0.03 * k - y
    x = torch.randn(n, c, SH, SW, generator=g) * 10.0 ** (torch.rand(n, 1, SH, SW, generator=g) * 3 - 2)
    metric = torch.randn(n, 1, SH, SW, generator=g)
    return x.to(dev), flow.to(dev), metric.to(dev)


@pytest.mark.parametrize("c", [3, 16])
@pytest.mark.parametrize("smode", ["sum", "avg", "linear", "soft"])
def test_softsplat_repeats_bit_for_bit(hip_backend, smode, c):
    """37 x 53, sigma = 1.5 noise plus 25 sources converging on one pixel; C = 3 (planar gather) and C = 16 (quad gather) through
    softsplat, softsplat_many(reuse_index=True) and the keep_quad path: one distinct output over 20 launches, and an item alone
    equal to the same item inside N = 2."""
    from drba_amd import ops
    dev = hip_backend.dev
    x, flow, metric = _softsplat_inputs(dev, c)
    m = metric if smode in ("linear", "soft") else None
    assert dc.multi_term_share(flow.cpu()) >= 0.20
    x2, flow2, metric2 = _softsplat_inputs(dev, c, n=2, seed=6)
    x2[1], flow2[1], metric2[1] = x[0], flow[0], metric[0]
    m2 = metric2 if m is not None else None

    def again():  # the index of the previous launch, gathered once more
        ops.softsplat_many([x], flow, m, smode)
        return ops.softsplat_many([x], flow, m, smode, reuse_index=True)[0]

    forms = {"softsplat": lambda: ops.softsplat(x, flow, m, smode), "reuse_index": again,
             "keep_quad": lambda: ops.softsplat(x, flow, m, smode, keep_quad=True)}
    default = _distinct(forms["softsplat"])
    with mode():
        outs = {}
        for name, fn in forms.items():
            outs[name] = fn()
            got = _distinct(fn)
            print(f"softsplat {smode} C={c} {name}: distinct of {LAUNCHES}: default {default} (information, softsplat form), deterministic {got}")
            assert got == 1, (smode, c, name, got)
        assert _bits_equal(outs["reuse_index"], outs["softsplat"]) and _bits_equal(outs["keep_quad"], outs["softsplat"])
        inside = ops.softsplat(x2, flow2, m2, smode)[1:2]
        assert _bits_equal(inside, outs["softsplat"]), (smode, c, "item alone vs second of N = 2")


# ----------------------------------------------------------------------------------------------------- accuracy
def _assert_rows(rows):
    for n, e, t, x in rows:
        print(f"{n}: err={e:.3e} tol={t:.1e} {x}")
    bad = [(n, e, t, x) for n, e, t, x in rows if not e <= t]
    assert not bad, "\n".join(f"{n}: err={e:.3e} tol={t:.1e} {x}" for n, e, t, x in bad)


def test_operator_cases_hold_their_bars_in_the_mode(hip_backend):
    """tests/op_checks.py's operator families once more with the mode on, against their own bars."""
    from tests import op_checks
    with mode():
        for _title, check in op_checks.CHECKS:
            if check not in op_checks.SPLAT_CHECKS:  # (the next test runs those)
                _assert_rows(check(hip_backend.dev))


def test_softsplat_rows_hold_their_bars_in_the_mode(hip_backend):
    """The generic splat's fp64 rows with the mode on, against their own bars: splat_sort_segments then orders every segment of
    the global records before the gathers.  The many-to-one, N = 3 and big-map rows are there, and between them they take
    sort_segment through both of its branches -- computed from the flows: the N = 3 maps hold shared segments of a few records
    and the zoom-out by 4 segments of exactly 16, the last length of the insertion branch; the zoom-out by 5 holds segments of
    25 and the one-target map is one segment of 3071 records (heap)."""
    from tests import cases, op_checks
    h, w = op_checks.SPLAT_MAP
    small = op_checks.splat_segment_sizes(op_checks.splat_inputs(3, 5, h, w, 2060)[1])
    assert 2 <= int(small.max()) <= 16, int(small.max())
    assert int(op_checks.splat_segment_sizes(op_checks.onto_flow(h, w)).max()) == h * w
    assert int(op_checks.splat_segment_sizes(cases.ops_inputs()["flow_converge"]).max()) == 16
    assert 16 < int(op_checks.splat_segment_sizes(op_checks.zoom_flow(h, w)).max()) <= 36
    with mode():
        rows = [r for check in op_checks.SPLAT_CHECKS for r in check(hip_backend.dev)]
    for must in ("every source onto", "zoom-out", "N=3 C=5", "N=3 C=3", "1024x1280"):
        assert sum(must in r[0] for r in rows) >= 2, must
    _assert_rows(rows)


def test_glue_splat_rows_hold_their_bars_in_the_mode(hip_backend):
    """gpu_checks.check_glue's flow_reverse / drm_rife_linear rows (the fixed-point path included: long, converge, pinch) with the
    mode on, against their own bars; the N = 2 vs two N = 1 rows, summation-order allowances in the default mode, are exact here."""
    from tests import gpu_checks
    with mode():
        rows = [r for r in gpu_checks.check_glue(hip_backend.dev) if r[0].startswith(("flow_reverse", "drm_rife", "fused splats"))]
    assert len(rows) > 20
    _assert_rows(rows)
    assert all(e == 0.0 for n, e, t, x in rows if "N=2 vs two N=1" in n), [r for r in rows if "N=2" in r[0]]


@pytest.mark.parametrize("fname", ["smooth", "long", "nan", "converge", "pinch"])
def test_nonlinear_rows_hold_their_bars_in_the_mode(hip_backend, fname):
    """tests/test_gpu_nonlinear.py's rows against the oracle's two branches (its flows, its cached references, its 2e-5)."""
    from drba_amd import ops
    from tests import decisions
    from tests import test_gpu_nonlinear as tn
    dev = hip_backend.dev
    fl, other = tn.flows()[0][fname].to(dev), tn.flows()[1].to(dev)
    rows = []
    with mode():
        for tt in (0.25, 0.8):
            ref = tn.reference(fname, tt)
            got = ops.drm_rife_nonlinear(fl, other, tt, 1e-4)
            rows += decisions.two_branch_rows(f"drm_rife_nonlinear {fname} t={tt}", got, ref["aligned"], ref["u"], ref["hole"],
                                              ref["unstable"], 2e-5)
    _assert_rows(rows)


# ----------------------------------------------------------------------------------------------------- trace names
def test_trace_shows_which_kernels_ran(hip_backend):
    from drba_amd import ops
    dev = hip_backend.dev
    fl, other = dc.flows()
    a, b = fl["long"].to(dev), other.to(dev)
    x, flow, _ = _softsplat_inputs(dev, 3)

    def names():
        ops.trace_begin()
        try:
            for op in T:
                _run(op, a, b)
            ops.softsplat(x, flow, None, "avg")
        finally:
            recs = ops.trace_end()
        return [r["name"] for r in recs]

    with mode():
        on = names()
    off = names()
    for k in (0, 1, 2):
        assert any(f"splat_tiled_det<{k}>" in n for n in on) and any(f"splat_long_prepass_det<{k}>" in n for n in on), on
        assert any(f"splat_tiled<{k}>" in n for n in off) and any(f"splat_long_prepass<{k}>" in n for n in off), off
    assert any("splat_sort_segments" in n for n in on) and not any("splat_tiled<" in n or "splat_long_prepass<" in n for n in on), on
    assert not any("_det" in n or "splat_sort_segments" in n for n in off), off


# ----------------------------------------------------------------------------------------------------- whole clips
def _write_weights(tmp):
    wdir = tmp / "w"
    wdir.mkdir(exist_ok=True)
    torch.save({"module." + k: v for k, v in synth.ifnet_state_dict(0).items()}, str(wdir / "flownet.pkl"))
    return str(wdir)


_CHILD = (
    "import sys; sys.path.insert(0, %r)\n"
    "import drba_amd.infer as I\n"
    "from drba_amd import ops\n"
    "a = I.parse_args(['-m','rife','-i',%r,'-o',%r,'--deterministic'] + %r)\n"
    "m = I.load_model(a.model_type, a.scale, weights=%r)\n"
    "print('written', I.inference(m, a))\n"
    "assert ops.deterministic()\n"
    "print('timing_passes', ops.tune_stats()['timing_passes'])\n")


def _child(inp, out, flags, wdir, store):
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, inp, out, list(flags), wdir)], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=dict(os.environ, DRBA_TUNE_CACHE=store))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "timing_passes 0" in r.stdout, r.stdout[-500:]
    return open(out, "rb").read()


@pytest.mark.parametrize("flags", [("-t", "2"), ("-fps", "60", "-s")], ids=["t2", "fps60_scdet"])
def test_rife_clip_is_byte_identical_between_runs_and_processes(tmp_path, hip_backend, flags, monkeypatch):
    """8 frames of 128 x 192 with a planted cut, synthetic weights, no winner store: two runs in this process and one in a fresh
    child write the same .npz, byte for byte."""
    from drba_amd import infer as I
    from drba_amd import ops
    monkeypatch.setenv("DRBA_TUNE_CACHE", "0")
    wdir, inp = _write_weights(tmp_path), str(tmp_path / "in.npz")
    np.savez(inp, frames=np.stack(synth.make_clip(8, 128, 192, seed=21, cut_at=5)), fps=np.float64(24.0))
    data = []
    try:
        for k in range(2):
            out = str(tmp_path / f"out{k}.npz")
            a = I.parse_args(["-m", "rife", "-i", inp, "-o", out, "--deterministic"] + list(flags))
            before = ops.tune_stats()["timing_passes"]
            I.inference(I.load_model(a.model_type, a.scale, weights=wdir), a)
            assert ops.deterministic() and ops.tune_stats()["timing_passes"] == before
            data.append(open(out, "rb").read())
    finally:
        ops.set_deterministic(False)
    data.append(_child(inp, str(tmp_path / "out_child.npz"), flags, wdir, "0"))
    assert len(data[0]) > 128 * 192 * 3 * 8
    assert data[0] == data[1], "two runs in one process differ"
    assert data[0] == data[2], "a fresh process differs"


def test_rife_clip_is_byte_identical_with_a_populated_store(tmp_path, hip_backend):
    """A store filled by a `python -m drba_amd.tune` child at the clip's size: two further children take its winners (no timing
    pass) and write the same bytes."""
    store = str(tmp_path / "store")
    r = subprocess.run([sys.executable, "-m", "drba_amd.tune", "-m", "rife", "--size", "128x192", "-t", "2", "-s"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT, env=dict(os.environ, DRBA_TUNE_CACHE=store))
    assert r.returncode == 0, r.stderr[-3000:]
    wdir, inp = _write_weights(tmp_path), str(tmp_path / "in.npz")
    np.savez(inp, frames=np.stack(synth.make_clip(8, 128, 192, seed=21, cut_at=5)), fps=np.float64(24.0))
    a = _child(inp, str(tmp_path / "a.npz"), ("-t", "2", "-s"), wdir, store)
    b = _child(inp, str(tmp_path / "b.npz"), ("-t", "2", "-s"), wdir, store)
    assert a == b


def _tensors(obj):
    if torch.is_tensor(obj):
        return [obj]
    if isinstance(obj, dict):
        return [t for k in sorted(obj, key=str) for t in _tensors(obj[k])]
    if isinstance(obj, (list, tuple)):
        return [t for o in obj for t in _tensors(o)]
    return []


def test_gmfss_union_warm_step_is_bit_identical(hip_backend):
    """One warm DRBA step at 128 x 256 from one entering state, three times: frames and the returned reuse, bit for bit."""
    dev = hip_backend.dev
    frames = [torch.from_numpy(f.transpose(2, 0, 1).copy()).unsqueeze(0).float().div(255.0).to(dev)
              for f in synth.make_clip(4, 128, 256, seed=31)]
    ts = np.array([0.75, 1.0, 1.25])
    seen = []
    with mode():
        model = hip_backend.make_gmfss_union(synth.gmfss_union_state_dicts(0), 1.0)
        for _ in range(3):
            reset = getattr(model, "reset_stream_state", None)
            if reset is not None:
                reset()
            _, reuse = model.inference_ts_drba(frames[0], frames[1], frames[2], ts, None, True)
            out, reuse2 = model.inference_ts_drba(frames[1], frames[2], frames[3], ts, reuse, True)
            torch.cuda.synchronize()
            seen.append([_digest(t) for t in _tensors(out) + _tensors(reuse2)])
    assert len(seen[0]) > 3
    assert seen[0] == seen[1] == seen[2]
