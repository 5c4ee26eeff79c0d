"""CPU: --dedup without a device -- the retimed schedule, the driver's calls with a recording fake model, the filter's frame rules
with an injected test, a whole clip through the oracle driver, the flags, the sharded run's refusal and the C entry's argument checks."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from drba_amd import _lib, dedup, driver
from drba_amd import infer as drv
from drba_amd.models.utils import tools
from tests import dedup_common as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("driver_calls_for_dedup", os.path.join(ROOT, "tools", "driver_calls.py"))
rec_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec_mod)

N = 12
KEPT_SETS = {"all": list(range(N)), "twos": list(range(0, N, 2)), "uneven": [0, 2, 4, 5, 7, 11], "ends": [0, N - 1],
             "trailing_drops": [0, 2, 4, 5, 7]}
SCHEDULES = {"t2": (2, 24.0, 48.0), "t3": (3, 24.0, 72.0), "t5": (5, 24.0, 120.0), "fps60_from_24": (-1, 24.0, 60.0),
             "fps60_from_23.976": (-1, 24000 / 1001, 60.0)}


def _calc(schedule):
    times, src, dst = SCHEDULES[schedule]
    mapper = tools.TMapper(src, dst, times)
    return lambda i: tools.calc_t(i, times, mapper)


def _plain_instants(calc, n):
    """What the run without --dedup writes: head t - 1 (calc_t(0)), iteration i: i + t (calc_t(i)), tail (n - 2) + t (calc_t(n - 2))"""
    out = [t - 1 for t in calc(0)]
    for i in range(n - 2):
        out += [i + t for t in calc(i)]
    return out + [(n - 2) + t for t in calc(n - 2)]


# ------------------------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("kept_name", sorted(KEPT_SETS))
def test_retimed_schedule_writes_the_plain_runs_instants(schedule, kept_name):
    """Worked by hand, -t 2 (calc_t = [0.75, 1.25]: the plain run writes j - 0.25 and j + 0.25 around every source frame j), N = 8,
    kept 0 2 4 5 7:
      head       T < 1            : -0.25 (before frame 0: a copy), 0.25, 0.75 -> 1 + T / 2          = 1.125, 1.375
      (0, 2, 4)  1 <= T < 3       : 1.25, 1.75 | 2.25, 2.75 -> 1 - (2 - T) / 2 | 1 + (T - 2) / 2     = 0.625, 0.875, 1.125, 1.375
      (2, 4, 5)  3 <= T < 4.5     : 3.25, 3.75 | 4.25       -> 1 - (4 - T) / 2 | calc_t's own 1.25   = 0.625, 0.875, 1.25
      (4, 5, 7)  4.5 <= T < 6     : 4.75 | 5.25, 5.75       -> calc_t's own 0.75 | 1 + (T - 5) / 2   = 0.75, 1.125, 1.375
      tail       T >= 6           : 6.25, 6.75 | 7.25       -> 1 - (7 - T) / 2 | after frame 7: copy = 0.625, 0.875, (1.25)
    16 instants, two per source frame, as without --dedup."""
    calc, kept = _calc(schedule), KEPT_SETS[kept_name]
    r = dedup.Retimed(calc, kept, lambda: N)
    parts = [(r.head_instants(), r.head(), None)]
    parts += [(r.step_instants(u), r.step(u), u) for u in range(len(kept) - 2)]
    parts += [(r.tail_instants(), r.tail(), None)]
    got = [(j - 1) + t for inst, _, _ in parts for j, t in inst]
    assert got == _plain_instants(calc, N)  # the same floats in the same order, hence the same count
    for inst, ts, u in parts:
        assert len(ts) == len(inst) and ts.dtype == np.float64
        if u is None:
            continue
        a, c, b = kept[u], kept[u + 1], kept[u + 2]
        assert all(0.5 <= t < 1.5 for t in ts), (u, ts)
        for (j, t0), t in zip(inst, ts):  # the timestep names the instant: T = c + (t - 1) * (the interval T lies in)
            T = (j - 1) + t0
            assert abs(c + (t - 1) * ((c - a) if T < c else (b - c)) - T) < 1e-12 and (t < 1) == (T < c)
    # head: copies before frame 0, then the way from k_0 to k_1; tail: the way to the last kept frame, copies after it
    k1, a, c = kept[1], kept[-2], kept[-1]
    for (j, t0), t in zip(*parts[0][:2]):
        T = (j - 1) + t0
        assert (t < 1) if T < 0 else abs((t - 1) * k1 - T) < 1e-12
    for (j, t0), t in zip(*parts[-1][:2]):
        T = (j - 1) + t0
        assert (t > 1) if T > c else abs(c - (1 - t) * (c - a) - T) < 1e-12
    if kept_name == "all":
        assert np.array_equal(r.head(), calc(0)) and np.array_equal(r.tail(), calc(N - 2))
        for u in range(N - 2):
            assert np.array_equal(r.step(u), calc(u)) and r.even_of(u)


def test_retimed_schedule_worked_example():
    r = dedup.Retimed(_calc("t2"), [0, 2, 4, 5, 7], lambda: 8)
    assert r.head().tolist() == [0.75, 1.125, 1.375]
    assert [r.step(u).tolist() for u in range(3)] == [[0.625, 0.875, 1.125, 1.375], [0.625, 0.875, 1.25], [0.75, 1.125, 1.375]]
    assert r.tail().tolist() == [0.625, 0.875, 1.25]
    assert [r.even_of(u) for u in range(3)] == [True, False, False]


# ------------------------------------------------------------------------------------------------------------------ driver calls
def _record(n, kept, surface, schedule="t2", use_dedup=True, max_run=8):
    times, _, dst = SCHEDULES[schedule]
    rec, kept_seen = rec_mod.Recorder(surface, ()), []
    kw = {}
    if use_dedup:
        keep = set(kept)
        kw = dict(dedup=dedup.Settings(max_run=max_run), check_dup=lambda a, b: b.k not in keep, on_kept=kept_seen.append)
    written = drv.interpolate_stream(rec.model, rec_mod._IO(rec_mod.make_frames(n), rec), dst, times=times, to_inp=rec.to_inp,
                                     to_out=rec.to_out, on_step=lambda i: rec.events.append(["step", i]), **kw)
    return rec, written, kept_seen


@pytest.mark.parametrize("surface", ["plain", "lookahead", "group1", "group4"])
def test_driver_calls_over_unequal_gaps(surface):
    rec, written, kept_seen = _record(8, [0, 2, 4, 5, 7], surface)
    assert kept_seen == [0, 2, 4, 5, 7] and written == 16
    calls = rec.model_calls()
    # (entry, left frame, timesteps)
    assert [[c[0], c[1], c[3]] for c in calls if c[0] == "ts"] == [
        ["ts", 0, [0.125, 0.375]],                                  # head: 1 + T / 2, less 1
        ["ts", 2, [0.625, 0.875]], ["ts", 4, [0.25]],               # (2, 4, 5): the two pairs on their own
        ["ts", 4, [0.75]], ["ts", 5, [0.125, 0.375]],               # (4, 5, 7)
        ["ts", 5, [0.625, 0.875]]]                                  # tail
    assert [c[1:3] for c in calls if c[0] == "ts"] == [[0, 2], [2, 4], [4, 5], [4, 5], [5, 7], [5, 7]]
    drba = [c for c in calls if c[0] == "drba"]
    assert len(drba) == 1 and drba[0][1:5] == [0, 2, 4, [0.625, 0.875, 1.125, 1.375]] and drba[0][5] is None
    if drba[0][7] is not None:  # no step is announced across the unequal one that follows
        assert all(not isinstance(x, int) or x <= 4 for x in drba[0][7]) and len(drba[0][7]) <= 2
    # a dropped frame reaches neither the model nor its prefetch hooks, and the writer gets 2 frames per SOURCE frame
    took = [e for e in rec.events if e[0] in ("prefetch_frame", "prefetch_pair")]
    assert all(k in (0, 2, 4, 5, 7) for e in took for k in e[1:])
    if rec_mod.SURFACES[surface][1]:
        assert [e[1] for e in took if e[0] == "prefetch_frame"] == [4, 5, 7]
    assert [e[1] for e in rec.events if e[0] == "step"] == list(range(8))  # once per source frame, frame 7 with the tail


@pytest.mark.parametrize("surface", ["plain", "group4"])
def test_reuse_is_dropped_after_a_pairwise_step(surface):
    rec, _, kept_seen = _record(9, [0, 2, 4, 5, 6, 7, 8], surface)
    assert kept_seen == [0, 2, 4, 5, 6, 7, 8]
    steps = [c for c in rec.model_calls() if c[0] == "drba"]
    assert [c[1:4] for c in steps] == [[0, 2, 4], [4, 5, 6], [5, 6, 7], [6, 7, 8]]   # (2, 4, 5) ran pairwise
    assert steps[0][5] is None and steps[1][5] is None                                   # cold start; the step after the pairwise one
    assert steps[2][5] is not None and steps[3][5] is not None                           # then `reuse` is carried again


@pytest.mark.parametrize("schedule", ["t2", "fps60_from_24"])
@pytest.mark.parametrize("surface", ["plain", "lookahead", "group1", "group4"])
def test_no_drop_makes_the_plain_runs_calls(surface, schedule):
    a, wa, kept_seen = _record(14, list(range(14)), surface, schedule)
    b, wb, _ = _record(14, None, surface, schedule, use_dedup=False)
    assert kept_seen == list(range(14)) and wa == wb
    pick = lambda rec: [e for e in rec.events if e[0] != "inp"]  # noqa: E731  (the filter converts a few frames earlier)
    assert pick(a) == pick(b)
    assert sorted(e[1] for e in a.events if e[0] == "inp") == list(range(14))  # every frame converted once


# ------------------------------------------------------------------------------------------------------------------ filter rules
class _Raw:
    is_cuda = False

    def __init__(self, k):
        self.k = k


def _filter(n, dup_frames, max_run=3):
    """KeptFrames over n frames; frame k repeats its predecessor when k is in dup_frames -> (kept, frames handed out, tests asked)"""
    src = iter([_Raw(k) for k in range(n)] + [None])
    asked = []

    def check(a, b):
        assert b.k == a.k + 1  # always against the previous SOURCE frame
        asked.append(b.k)
        return b.k in dup_frames

    f = driver.KeptFrames(lambda k: next(src), lambda raw: raw, dedup.Settings(max_run=max_run), check_dup=check)
    out = []
    while True:
        x = f.next()
        if x is None:
            break
        out.append(x.k)
    assert f.total == n and out == f.kept
    assert f.kept == dedup.kept_indices([k in dup_frames for k in range(1, n)], max_run)
    return f.kept, asked


def test_filter_rules():
    assert _filter(12, set())[0] == list(range(12))
    assert _filter(12, {1, 3, 5, 7, 9, 11})[0] == [0, 2, 4, 6, 8, 10]
    # a frame after R drops is kept whatever the test says, and is not even tested
    kept, asked = _filter(12, set(range(1, 12)), max_run=3)
    assert kept == [0, 4, 8] and asked == [1, 2, 3, 5, 6, 7, 9, 10, 11]
    assert _filter(12, set(range(1, 12)), max_run=1)[0] == [0, 2, 4, 6, 8, 10]
    # everything repeats and R is large: frame 0 and the last frame
    assert _filter(6, set(range(1, 6)), max_run=99)[0] == [0, 5]
    assert _filter(2, {1})[0] == [0, 1]
    assert _filter(12, set(), max_run=0)[0] == list(range(12))


def test_dup_rule_and_defaults():
    s = dedup.Settings()
    assert (s.hi, s.lo, s.frac, s.max_run) == (12 / 255, 5 / 255, 0.33, 3)
    assert dedup.is_dup(12 / 255, 33, 100) and not dedup.is_dup(12.001 / 255, 0, 100) and not dedup.is_dup(0.0, 34, 100)
    assert dedup.settings_of(None) is None and dedup.settings_of(False) is None and dedup.settings_of(True).max_run == 3
    assert dedup.settings_of({"max_run": 1, "hi": 0.1}).hi == 0.1
    with pytest.raises(ValueError):
        dedup.Settings(frac=1.5)
    # the numpy reference: 8 x 8 blocks at the origin, edge blocks by their own pixel count
    a = np.zeros((3, 9, 17), dtype=np.float32)
    b = a.copy()
    b[:, 8, 16] = 0.6
    m = dc.block_means(a, b)
    assert m.shape == (2, 3) and m[1, 2] == pytest.approx(0.6) and m.sum() == pytest.approx(0.6)
    assert dc.ref_stats(a, b)[:3] == (pytest.approx(0.6), 1, 6)


# ------------------------------------------------------------------------------------------------------------------ whole clip
def test_whole_clip_without_repeats_is_unchanged_and_with_repeats_is_retimed():
    import oracle
    from drba_amd.utils import synth
    from tests.clip_common import ListIO, cpu_hooks
    to_inp, to_out, _ = cpu_hooks()
    frames = dc.moving_clip(12, 64, 96, seed=5)

    def run(clip, **kw):
        io = ListIO(list(clip), 24.0)
        n = drv.interpolate_stream(oracle.rife.RifeOracle(synth.ifnet_state_dict(0), 1.0), io, 48.0, times=2, to_inp=to_inp, to_out=to_out, **kw)
        assert n == len(io.written)
        return np.stack(io.written)

    kept = []
    plain = run(frames)
    same = run(frames, dedup=True, check_dup=dc.check_dup_numpy(), on_kept=kept.append)
    assert kept == list(range(12)), "the synthetic clip has no repeats by the numpy rule"
    assert same.tobytes() == plain.tobytes()
    # the same drawings on twos: 6 frames held for two each -> the same count, every second frame kept
    kept.clear()
    twos = dc.repeat_clip(frames[:6], [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5])
    got = run(twos, dedup=True, check_dup=dc.check_dup_numpy(), on_kept=kept.append)
    assert kept == [0, 2, 4, 6, 8, 10] and got.shape == plain.shape
    assert not np.array_equal(got, run(twos))


# ------------------------------------------------------------------------------------------------------------------ surface
def test_cli_flags_parse():
    a = drv.parse_args(["-i", "x.npz", "-o", "y.npz"])
    assert a.dedup is False and drv.dedup_of(a) is None
    assert (a.dedup_hi, a.dedup_lo, a.dedup_frac, a.dedup_max) == (12 / 255, 5 / 255, 0.33, 3)
    a = drv.parse_args(["-i", "x.npz", "-o", "y.npz", "--dedup", "--dedup-hi", "0.1", "--dedup-lo", "0.05", "--dedup-frac", "0.5",
                        "--dedup-max", "1", "-s", "--nonlinear", "--deterministic", "--fit", "pad", "--out-depth", "16"])
    s = drv.dedup_of(a)
    assert (s.hi, s.lo, s.frac, s.max_run) == (0.1, 0.05, 0.5, 1)
    import argparse
    assert drv.dedup_of(argparse.Namespace()) is None  # a namespace built without the flags


def test_sharded_run_refuses_dedup(tmp_path):
    inp = str(tmp_path / "in.npz")
    np.savez(inp, frames=np.zeros((4, 16, 16, 3), dtype=np.uint8), fps=np.float64(24.0))
    a = drv.parse_args(["-i", inp, "-o", str(tmp_path / "out.npz"), "-t", "2", "--dedup"])
    for rank in (0, 1):
        with pytest.raises(ValueError, match="--dedup"):
            drv.inference_sharded(object(), a, rank, 2)
    assert not os.path.exists(str(tmp_path / "out.npz"))


def test_dup_stats_entry_checks_its_arguments():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = (3, 8, 8)
    for args in ((None, p, *ok, 0.02, p, p), (p, None, *ok, 0.02, p, p), (p, p, *ok, 0.02, None, p), (p, p, *ok, 0.02, p, None)):
        assert lib.drba_dup_stats_f32(*args, None) == -1
    for shape in ((0, 8, 8), (3, 0, 8), (3, 8, 0), (-1, 8, 8)):
        assert lib.drba_dup_stats_f32(p, p, *shape, 0.02, p, p, None) == -1
        assert lib.drba_dup_stats_ws_floats(*shape) == 0
    assert lib.drba_dup_stats_ws_floats(3, 8, 8) == 2                 # one strip, one workgroup: (max, count)
    assert lib.drba_dup_stats_ws_floats(3, 1088, 1920) == 2 * 2040     # 60 x 136 strips of 32 x 8 pixels, four waves per workgroup
    assert lib.drba_dup_stats_ws_floats(3, 4352, 7680) == 2 * 2048     # capped: a grid-stride loop above it
    assert _lib.SIGNATURES["drba_dup_stats_f32"][1][5] is C.c_float


def test_dup_stats_has_no_cpu_fallback():
    from drba_amd import ops
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(_lib.DrbaHipError):
        ops.dup_stats(x, x, 0.02)


# ------------------------------------------------------------------------------------------------------------------ evaluate
def test_evaluate_dups_reports_pairs_runs_and_kept(tmp_path, capsys):
    from drba_amd import evaluate
    from tests.clip_common import cpu_hooks
    base = dc.moving_clip(4, 64, 96, seed=9)
    clip = dc.repeat_clip(base, [0, 0, 1, 1, 1, 1, 1, 2, 3])  # one repeat, then four in a row (--dedup-max 3 keeps the fourth)
    path = str(tmp_path / "c.npz")
    np.savez(path, frames=np.stack(clip), fps=np.float64(24.0))
    to_inp = cpu_hooks()[0]
    stats = lambda a, b, lo: dc.ref_stats(a.numpy(), b.numpy(), lo)[:3]  # noqa: E731
    res = evaluate.dups(evaluate.ClipSource(path), stats=stats, to_inp=to_inp, out=sys.stdout)
    assert [p["dup"] for p in res["pairs"]] == [True, False, True, True, True, True, False, False]
    assert res["runs"] == [[1, 1], [3, 4]] and res["kept"] == [0, 2, 6, 7, 8] and res["frames"] == 9
    assert all(p["n_blocks"] == 8 * 16 for p in res["pairs"])  # 64 x 96 -> the 64 x 128 network input of -m rife
    text = capsys.readouterr().out
    assert "5 of 9 frames kept" in text and "frames 3 .. 6: 4 repeats of frame 2 (at most 3 in a row are dropped)" in text
    assert text.count("repeat\n") == 5 and text.count("new\n") == 3
    a = evaluate.parse_args(["dups", path, "--dedup-hi", "0.1", "--dedup-max", "2", "-m", "gmfss_union"])
    assert (a.command, a.dedup_hi, a.dedup_max, a.model_type) == ("dups", 0.1, 2, "gmfss_union")
    a = evaluate.parse_args(["holdout", "-i", path, "--dedup", "--dedup-frac", "0.5"])
    assert drv.dedup_of(a).frac == 0.5 and drv.dedup_of(evaluate.parse_args(["holdout", "-i", path])) is None
