"""The deterministic mode without a GPU: the command-line flags, the tuner's rule (no timing decides a kernel configuration) driven
with the fake clock of tests/test_tune_cache.py, the C ABI's switch, and the DRBA_DETERMINISTIC=1 import switch."""
import os
import subprocess
import sys

import pytest

from drba_amd import _lib, tunecache
from tests.test_tune_cache import COST, FAMS, KEY, _entries, _Tuner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def cache_dir(tmp_path, monkeypatch):
    d = tmp_path / "store"
    monkeypatch.setenv("DRBA_TUNE_CACHE", str(d))
    monkeypatch.setattr(tunecache, "_default_on", False)
    return d


@pytest.fixture
def det(monkeypatch):
    from drba_amd import ops
    monkeypatch.setattr(ops, "_tuned_det", {})
    was = ops.set_deterministic(True)
    try:
        yield ops
    finally:
        ops.set_deterministic(was)


def test_flags_and_namespace_defaults():
    import argparse

    from drba_amd import evaluate, infer
    assert infer.parse_args([]).deterministic is False
    assert infer.parse_args(["--deterministic", "-t", "2"]).deterministic is True
    h = evaluate.parse_args(["holdout", "-i", "clip.npz"])
    assert h.deterministic is False and evaluate.parse_args(["holdout", "-i", "clip.npz", "--deterministic"]).deterministic is True
    with pytest.raises(SystemExit):
        evaluate.parse_args(["compare", "a.npz", "b.npz", "--deterministic"])  # a comparison computes nothing that has a mode
    # a namespace built without the flag (tests, callers of inference()) means "leave the mode alone"
    from drba_amd import ops
    was = ops.deterministic()
    infer.apply_deterministic(argparse.Namespace())
    assert ops.deterministic() == was


def test_abi_switch_returns_the_previous_setting_and_sizes_the_workspace():
    lib = _lib.load()
    assert lib.drba_get_deterministic() == 0
    off = lib.drba_rife_splat_ws_floats(2, 70, 100, 2)
    assert off == (1 << 18) + 2 * 70 * 100 * 3 + 2 * 4 * 5  # reach map, fp32 accumulator, one flag per tile: as before ABI 15
    try:
        assert lib.drba_set_deterministic(1) == 0 and lib.drba_get_deterministic() == 1
        assert lib.drba_rife_splat_ws_floats(2, 70, 100, 2) == off + 2 * 70 * 100 * 3  # 64-bit accumulator words
        assert lib.drba_set_deterministic(7) == 1 and lib.drba_get_deterministic() == 1
    finally:
        assert lib.drba_set_deterministic(0) == 1
    assert lib.drba_rife_splat_ws_floats(2, 70, 100, 2) == off
    # in this mode a fused splat refuses a workspace that cannot hold 64-bit words (no GPU needed: refused before any launch)


def test_no_timing_decides_a_configuration(monkeypatch, det):
    """No store: the library's pick when it is a candidate that accepts the shape, else the first candidate that does -- the same id
    from every fresh table, with no timing pass, no synchronisation and nothing stored."""
    tu = _Tuner(monkeypatch)
    picks = []
    for _ in range(3):
        tu.new_process()
        monkeypatch.setattr(tu.ops, "_tuned_det", {})
        picks.append(tu.ops._tune(KEY, [3, 4, 5, 6], tu.run(COST), families=FAMS, persist=True, pick=lambda: 6))
        assert tu.runs == [6] and not tu.syncs
        st = tu.ops.tune_stats()
        assert (st["timing_passes"], st["full_tunes"], st["stored"], st["cache_hits"]) == (0, 0, 0, 0)
        assert tu.ops._tuned_get(KEY, FAMS) == 6 and tu.ops._tuned == {}  # kept apart from the timed winners
    assert picks == [6, 6, 6]
    # the pick refuses the shape (4), or is no candidate (9), or there is none: the first candidate that accepts it
    for pick, want, runs in ((lambda: 4, 3, [4, 3]), (lambda: 9, 3, [3]), (None, 3, [3]), (5, 5, [5])):
        tu.new_process()
        monkeypatch.setattr(tu.ops, "_tuned_det", {})
        assert tu.ops._tune(KEY, [3, 4, 5, 6], tu.run(COST), families=FAMS, pick=pick) == want
        assert tu.runs == runs and not tu.syncs and tu.ops.tune_stats()["timing_passes"] == 0
    # the timed tuner would have chosen 5 (the cheapest): the rule is not the clock's
    tu.new_process()
    monkeypatch.setattr(tu.ops, "_tuned_det", {})
    with pytest.raises(tu.ops.NoKernelConfig):
        tu.ops._tune(KEY, [4], tu.run(COST), families=FAMS, pick=lambda: 4)
    with pytest.raises(_lib.DrbaHipError):
        tu.ops._tune(("other",), [7], tu.run({7: -3}), families=FAMS)  # a launch failure is reported, not skipped over


def test_a_stored_winner_is_used_and_nothing_is_written(monkeypatch, cache_dir):
    from drba_amd import ops
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 4, 5, 6], COST) == 5  # default mode: timed, stored
    before = dict(_entries(cache_dir))
    mtime = os.stat(os.path.join(str(cache_dir), os.listdir(str(cache_dir))[0])).st_mtime_ns
    tu.new_process()
    monkeypatch.setattr(ops, "_tuned_det", {})
    was = ops.set_deterministic(True)
    try:
        assert ops._tune(KEY, [3, 4, 5, 6], tu.run(COST), families=FAMS, persist=True, pick=lambda: 6) == 5  # the store's, not the pick
        assert tu.runs == [5] and not tu.syncs
        st = ops.tune_stats()
        assert (st["cache_hits"], st["timing_passes"], st["full_tunes"], st["stored"]) == (1, 0, 0, 0)
        # a shape the store does not know: the shape-only rule, and the store is left as it was
        assert ops._tune(("conv3x3", 1, 8, 8, 5, 5, 1), [3, 6], tu.run(COST), families=FAMS, persist=True, pick=lambda: 6) == 6
        assert ops.tune_stats()["stored"] == 0 and not tu.syncs
    finally:
        ops.set_deterministic(was)
    assert _entries(cache_dir) == before
    assert os.stat(os.path.join(str(cache_dir), os.listdir(str(cache_dir))[0])).st_mtime_ns == mtime


def test_environment_switch_at_import():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from drba_amd import ops, _lib\n"
            "print('py', ops.deterministic())\n"
            "print('lib', _lib.load().drba_get_deterministic())\n" % ROOT)
    for value, py, lib in (("1", "True", "1"), ("0", "False", "0"), (None, "False", "0")):
        env = {k: v for k, v in os.environ.items() if k != "DRBA_DETERMINISTIC"}
        if value is not None:
            env["DRBA_DETERMINISTIC"] = value
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert f"py {py}" in r.stdout and f"lib {lib}" in r.stdout, r.stdout
