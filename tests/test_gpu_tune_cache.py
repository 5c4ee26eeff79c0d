"""GPU: the conv autotuner's winner store across real processes (drba_amd/tunecache.py, drba_amd/tune.py).

Four fresh child processes, one at a time (each pays torch's import); the chain stops at the first child that fails and
starts no further one.  128 x 192 frames, RIFE with synth.ifnet_state_dict(0).

    A  an empty store: a `-fps 60 -s` clip with one planted cut through drba_amd.infer, then one conv3x3_shuffle call
    B  the same store, the same work: no full tune, no timing pass; then a rehearsal, then the clip once more
    C  a new store: `python -m drba_amd.tune -m rife --size 128x192 -t 2 -s` (synthetic weights)
    D  C's store: a `-t 2 -s` clip with cuts 13, 14, 15 and 16 frames apart: no timing pass
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from drba_amd import parallel
from drba_amd.utils import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 128, 192
N_AB = sum(parallel.emission_counts(12, 24.0, 60.0, -1, 1)[0])  # frames the 12-frame 24 -> 60 fps clip writes

_WORKER = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
mode, inp, out, wdir, report, flags = sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6], sys.argv[7:]
import numpy as np
import torch
import drba_amd.infer as I
from drba_amd import ops, tunecache, tune

rep = {}
a = I.parse_args(["-m", "rife", "-i", inp, "-o", out] + flags)
m = I.load_model(a.model_type, a.scale, weights=wdir)
rep["written"] = I.inference(m, a)
rep["after_clip"] = ops.tune_stats()
if mode in ("A", "B"):
    # RIFE reaches conv3x3 and deconv4x4 but not the shuffle kind: one small GridNet-tail layer (64 -> 256 channels)
    g = torch.Generator().manual_seed(5)
    layer = ops.Conv3x3(torch.randn(256, 64, 3, 3, generator=g) / 17.0, torch.randn(256, generator=g) * 0.1, stride=1, act=False,
                        device=m.device)
    y = ops.conv3x3_shuffle(layer, torch.randn(1, 64, 11, 44, generator=g).to(m.device))
    torch.cuda.synchronize()
    rep["shuffle_shape"] = list(y.shape)
    rep["after_shuffle"] = ops.tune_stats()
    rep["packs_kept"] = len(layer._packed)
if mode == "B":
    stats0 = dict(m.stats)
    rep["rehearsal"] = tune.rehearse(m, tuple(np.load(inp)["frames"].shape[1:3]), 24.0, 60.0, -1, True)
    rep["state_after_rehearsal"] = {"stats_unchanged": m.stats == stats0, "group_out": len(m._group_out),
                                    "look_pending": [getattr(getattr(m, n, None), "pending", None) is not None for n in ("_look", "_look2")]}
    fresh = dict.fromkeys(m.STAT_KEYS, 0)
    m.stats = dict(fresh)
    a2 = I.parse_args(["-m", "rife", "-i", inp, "-o", out.replace(".npz", "_again.npz")] + flags)
    rep["written_again"] = I.inference(m, a2)
    rep["after_again"] = ops.tune_stats()
store = tunecache.active()
rep["store"] = None if store is None else store.path
rep["entries"] = {} if store is None else tunecache.read_file(store.path, store.identity)[1]
with open(report, "w") as f:
    json.dump(rep, f)
print("child", mode, "done")
'''


def _pingpong_clip(n, cuts, seed):
    """Two synthetic scenes that alternate at every planted cut; within a scene the 8 base frames are walked 0 .. 7, 6 .. 1, 0 ..
    (consecutive frames are always neighbours: no cut but the planted ones)."""
    scenes = [synth.make_clip(8, H, W, seed=seed), synth.make_clip(8, H, W, seed=seed + 7919)]
    out = []
    for k in range(n):
        src = scenes[sum(1 for c in cuts if k >= c) % 2]
        j = k % 14
        out.append(src[j if j < 8 else 14 - j])
    return np.stack(out)


class _Chain:
    def __init__(self, tmp):
        self.tmp, self.failed, self.rep, self.secs = tmp, None, {}, {}
        self.wdir = tmp / "w"
        self.wdir.mkdir()
        torch.save({"module." + k: v for k, v in synth.ifnet_state_dict(0).items()}, str(self.wdir / "flownet.pkl"))
        self.worker = str(tmp / "worker.py")
        with open(self.worker, "w") as f:
            f.write(_WORKER)
        self.store_ab, self.store_cd = str(tmp / "store_ab"), str(tmp / "store_cd")
        self.clip_ab, self.clip_d = str(tmp / "ab.npz"), str(tmp / "d.npz")
        np.savez(self.clip_ab, frames=np.stack(synth.make_clip(12, H, W, seed=77, cut_at=6)), fps=np.float64(24.0))
        np.savez(self.clip_d, frames=_pingpong_clip(62, (13, 27, 42, 58), 311), fps=np.float64(24.0))

    def env(self, store):
        return dict(os.environ, DRBA_TUNE_CACHE=store)

    def child(self, name, argv, store, timeout=300):
        """One child process; after a failure no further child is started."""
        import time
        if self.failed is not None:
            pytest.fail(f"child {name} was not started: child {self.failed} failed")
        t0 = time.perf_counter()
        try:
            r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=self.env(store))
        except subprocess.TimeoutExpired:
            self.failed = name
            raise
        self.secs[name] = round(time.perf_counter() - t0, 1)
        print(f"child {name}: {self.secs[name]} s")
        if r.returncode != 0:
            self.failed = name
            pytest.fail(f"child {name} exited with {r.returncode}:\n{r.stderr[-3000:]}")
        return r

    def clip_child(self, name, clip, store, flags):
        out, report = str(self.tmp / f"out_{name}.npz"), str(self.tmp / f"report_{name}.json")
        self.child(name, [sys.executable, self.worker, ROOT, name, clip, out, str(self.wdir), report] + flags, store)
        with open(report) as f:
            self.rep[name] = json.load(f)
        return self.rep[name], out


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    return _Chain(tmp_path_factory.mktemp("tune_cache"))


def _kinds(entries):
    return {json.loads(k)[0] for k in entries}


def _frames(path):
    return np.load(path)["frames"]


def _child_a(chain):
    if "A" not in chain.rep:
        chain.clip_child("A", chain.clip_ab, chain.store_ab, ["-fps", "60", "-s"])
    return chain.rep["A"], str(chain.tmp / "out_A.npz")


def _child_c(chain):
    if "C" not in chain.rep:
        r = chain.child("C", [sys.executable, "-m", "drba_amd.tune", "-m", "rife", "--size", f"{H}x{W}", "-t", "2", "-s"], chain.store_cd)
        chain.rep["C"] = json.loads(r.stdout.strip().splitlines()[-1])
    return chain.rep["C"]


def _assert_same_frames(x, y, what):
    """Two runs of one clip with the same kernel configurations.  They are NOT bit-identical on this pipeline, with or without
    the store: the tiled forward splat behind flow_reverse / drm_rife_linear (splat_warp.hip, splat_tiled) ranks the sources of an
    output pixel by the order in which an LDS atomicAdd hands out slots, so the fp32 sum of a pixel's contributions is taken in
    a different order from launch to launch, and the flow it makes differs in the last bit.  Measured on the MI355X: child B's
    clip twice in ONE process (the same `_tuned`, before and after a rehearsal) differs in 4 of 2 285 568 bytes by 1 LSB, as does
    A against B (profiles/tune_cache.md).  So this comparison allows what tests/test_gpu_cli.py::_assert_frames_close allows
    for two processes -- one LSB on a value sitting on an integer boundary, in few bytes -- and nothing more."""
    assert x.shape == y.shape and x.dtype == y.dtype == np.uint8
    d = np.abs(x.astype(np.int16) - y.astype(np.int16))
    print(f"{what}: {int((d > 0).sum())} of {d.size} bytes differ, max {int(d.max())} LSB")
    assert d.max() <= 1, f"{what}: max diff {d.max()} LSB"
    assert (d > 0).mean() < 2e-3, f"{what}: {(d > 0).mean():.2e} of the bytes differ"


def test_a_empty_store_is_filled(chain):
    rep, out = _child_a(chain)
    st = rep["after_shuffle"]
    print("A:", st, "entries", len(rep["entries"]), "kinds", sorted(_kinds(rep["entries"])))
    assert rep["written"] == N_AB and rep["shuffle_shape"] == [1, 64, 22, 88]
    assert st["full_tunes"] > 0 and st["timing_passes"] > 0 and st["cache_hits"] == 0 and st["rejected"] == 0
    assert st["stored"] == st["full_tunes"] == len(rep["entries"])
    assert rep["after_shuffle"]["full_tunes"] == rep["after_clip"]["full_tunes"] + 1
    assert _kinds(rep["entries"]) == {"conv3x3", "conv3x3_shuffle", "deconv4x4"}
    assert os.path.exists(rep["store"]) and os.path.dirname(rep["store"]) == chain.store_ab
    assert rep["packs_kept"] == 1  # the losing candidates' packings of the shuffle layer are dropped
    assert all(e["best_us"] > 0 and (e["runner_up_us"] is None or e["best_us"] <= e["runner_up_us"]) for e in rep["entries"].values())


def test_b_second_process_tunes_nothing_and_rehearsal_leaves_no_trace(chain):
    a, out_a = _child_a(chain)
    rep, out = chain.clip_child("B", chain.clip_ab, chain.store_ab, ["-fps", "60", "-s"])
    st = rep["after_shuffle"]
    print("B:", st, "rehearsal", rep["rehearsal"], "after the second pass", rep["after_again"])
    assert st["timing_passes"] == 0 and st["full_tunes"] == 0 and st["rejected"] == 0 and st["stored"] == 0
    assert st["cache_hits"] == a["after_shuffle"]["full_tunes"]
    fa, fb, again = _frames(out_a), _frames(out), _frames(out.replace(".npz", "_again.npz"))
    assert fa.shape == fb.shape == (N_AB, H, W, 3)
    _assert_same_frames(fa, fb, "A vs B")  # the same winners, the same kernels
    # the rehearsal: its planted cuts were the ones the scene test saw (rehearse raises otherwise), it took every branch of the
    # loop, and the model is as it was
    r = rep["rehearsal"]
    assert r["cuts"] == [2, 3, 16, 30, 45, 61] and all(r["branches"][k] > 0 for k in ("head", "drba", "cut_left", "cut_right", "cut_both", "tail"))
    assert rep["state_after_rehearsal"] == {"stats_unchanged": True, "group_out": 0, "look_pending": [False, False]}
    _assert_same_frames(fb, again, "B vs B after the rehearsal")
    assert rep["after_again"]["timing_passes"] == r["tune"]["timing_passes"]  # the second pass itself tuned nothing


def test_c_tune_command_fills_a_new_store(chain):
    rep = _child_c(chain)
    print("C:", rep["tune_stats"], rep["rehearsal"], "bytes", rep["bytes"])
    assert rep["entries_before"] == 0 and rep["entries_after"] == rep["tune_stats"]["stored"] > 0
    assert rep["decisions_checked"] is True and rep["rehearsal"]["cuts"] == [2, 3, 16, 30, 45, 61]
    assert rep["weights"].startswith("synthetic") and os.path.dirname(rep["store"]) == chain.store_cd
    path = rep["rehearsal"]["path"]
    assert path["groups_formed"] > 0 and path["group_collects"] > 0 and path["single_steps"] > 0, path


def test_d_clip_after_the_rehearsal_never_synchronises_for_the_tuner(chain):
    _child_c(chain)
    rep, out = chain.clip_child("D", chain.clip_d, chain.store_cd, ["-t", "2", "-s"])
    st = rep["after_clip"]
    print("D:", st, "children took", chain.secs)
    assert rep["written"] == 124
    assert st["timing_passes"] == 0 and st["full_tunes"] == 0 and st["rejected"] == 0 and st["cache_hits"] > 0
