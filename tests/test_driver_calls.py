"""CPU: the driver loop's calls against a recording of them (tests/golden/driver_calls.json, made by tools/driver_calls.py
from the commit the file names: the last one with a loop of its own in interpolate_stream and in interpolate_shard).

The sequential driver must repeat the recording event for event: model calls with bit-identical float64 timesteps, `reuse`
and the whole `lookahead` tuple, the order of to_inp, prefetch_frame / prefetch_pair and check_scene among them, the frames
written, the on_step values and the most network inputs alive at an on_step.  Every shard must repeat its model calls
(warm_reuse's calc_flow and every `lookahead` tuple included) and its emissions.  How a shard takes its frames in is the
sequential driver's policy and is checked as such, not against the recording.

The file holds one SHA-256 digest per run (whole event lists would be 400 kB); a mismatch names the command that prints
the full recording of the case, to be run on both commits.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("driver_calls", os.path.join(ROOT, "tools", "driver_calls.py"))
dc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dc)

with open(os.path.join(ROOT, "tests", "golden", "driver_calls.json")) as f:
    GOLD = json.load(f)

CASES = ["/".join(c) for c in dc.grid()]


def test_recording_covers_the_grid():
    assert len(GOLD["made_from"]["commit"]) == 40 and not GOLD["made_from"]["drba_amd_modified"]
    assert sorted(GOLD["cases"]) == sorted(CASES)
    for name in CASES:
        n = dc.CLIPS[name.split("/")[0]][0]
        assert sorted(GOLD["cases"][name]["shards"]) == sorted(str(w) for w in dc.worlds(n))


@pytest.mark.parametrize("name", CASES)
def test_sequential_driver_repeats_the_recording(name):
    gold, got = GOLD["cases"][name], dc.run_sequential(*name.split("/"))
    assert len(got["events"]) == gold["events"]
    assert dc.digest(got["events"]) == gold["sequential"], f"python tools/driver_calls.py --dump {name}"
    assert got["written"] == gold["written"] == sum(1 for e in got["events"] if e[0] == "write")
    assert got["max_alive"] == gold["max_alive"]


@pytest.mark.parametrize("name", CASES)
def test_shards_repeat_the_recording_and_take_frames_in_like_the_sequential_driver(name):
    clip, schedule, surface = name.split("/")
    n = dc.CLIPS[clip][0]
    gold, seq = GOLD["cases"][name], dc.run_sequential(clip, schedule, surface)
    seq_written = [e[1] for e in seq["events"] if e[0] == "write"]  # (pinned by the test above)
    from drba_amd import parallel
    for world in dc.worlds(n):
        runs = [dc.run_shard(clip, schedule, surface, rank, world) for rank in range(world)]  # (also: returned list == the sink's emissions)
        assert dc.digest([[s["model"], s["emitted"]] for s in runs]) == gold["shards"][str(world)], \
            f"world {world}: python tools/driver_calls.py --dump {name}"
        for rank, ((a, b), s) in enumerate(zip(parallel.partition(max(n - 2, 0), world), runs)):
            # the intake policy: every frame of the window [a, hi] after its first two is prefetched once, when it is read
            hi = min(b + 1, n - 1)
            took = [e for e in s["events"] if e[0] in ("prefetch_frame", "prefetch_pair")]
            if dc.SURFACES[surface][1] and s["emitted"]:
                want = [e for j in range(a + 2, hi + 1) for e in (["prefetch_frame", j], ["prefetch_pair", j - 1, j])]
            else:
                want = []
            assert took == want, (world, rank, took, want)
            asked = [e[1] for e in s["events"] if e[0] == "scene"]
            assert len(asked) == len(set(asked)) and all(max(a - 1, 0) <= k < hi for k in asked), (world, rank, asked)
            assert s["max_alive"] <= gold["max_alive"] + 1, (world, rank, s["max_alive"])
        # the ranks' frames, concatenated, are the sequential run's (generated frames are named by the `reuse` they were made with)
        assert [x for s in runs for e in s["emitted"] for x in e] == seq_written, world
