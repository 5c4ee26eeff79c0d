"""The conv autotuner's winner store (drba_amd/tunecache.py) and the tuner's use of it, without a GPU: the store is built
with an injected identity, ops._tune is driven with a fake Event / synchronize (the technique of tests/test_abi.py's tuner
test) and counts what it launches and how often it synchronises."""
import json
import os
import subprocess
import sys
import warnings

import pytest

from drba_amd import _lib, tunecache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = tunecache.make_identity(9, "ab" * 32, "AMD Instinct MI355X", "gfx950:sramecc+:xnack-", 256)
FAMS = (0, 1, 2, 3, 4)
KEY = ("conv3x3", 2, 39, 192, 8, 12, 2)


class _Tuner:
    """ops with a fake clock: run(cfg) advances the time by cost[cfg] (or refuses), synchronisations and launches are counted.
    new_process() is what a fresh process has: no winners in memory, a new store object, counters at zero."""

    def __init__(self, monkeypatch, ident=IDENT):
        from drba_amd import ops
        self.ops, self.mp = ops, monkeypatch
        tuner = self

        class _Ev:
            def __init__(self, enable_timing=True):
                pass

            def record(self):
                self.at = tuner.t

            def synchronize(self):
                pass

            def elapsed_time(self, other):
                return other.at - self.at

        self.t, self.syncs, self.runs = 0.0, [], []
        monkeypatch.setattr(ops.torch.cuda, "Event", _Ev)
        monkeypatch.setattr(ops.torch.cuda, "synchronize", lambda *a: self.syncs.append(1))  # (candidates are timed on an idle device)
        self.ident = ident
        self.new_process()

    def new_process(self, ident=None):
        if ident is not None:
            self.ident = ident
        self.mp.setattr(self.ops, "_tuned", {})
        self.mp.setattr(self.ops, "_no_config", set())
        self.mp.setattr(self.ops, "_tune_stats", dict.fromkeys(self.ops._TUNE_STAT_KEYS, 0))
        self.mp.setattr(tunecache, "_stores", {})
        self.mp.setattr(tunecache, "identity_provider", lambda device=None: dict(self.ident))
        del self.syncs[:], self.runs[:]

    def run(self, cost):
        def f(cfg):
            self.runs.append(cfg)
            if cost.get(cfg) is None:
                return -2  # DRBA_EUNSUPPORTED: the configuration refuses the shape (returns without launching)
            if cost[cfg] < 0:
                return int(cost[cfg])  # another error code of include/drba_hip.h (-3: DRBA_ELAUNCH, -1: DRBA_EINVAL)
            self.t += cost[cfg]
            return 0
        return f

    def tune(self, key, cands, cost, persist=True, families=FAMS):
        return self.ops._tune(key, cands, self.run(cost), families=families, persist=persist)


@pytest.fixture
def cache_dir(tmp_path, monkeypatch):
    d = tmp_path / "store"
    monkeypatch.setenv("DRBA_TUNE_CACHE", str(d))
    monkeypatch.setattr(tunecache, "_default_on", False)
    return d


def _file(d, ident=IDENT):
    return os.path.join(str(d), tunecache.file_name(ident))


def _entries(d, ident=IDENT):
    got_ident, ent = tunecache.read_file(_file(d, ident), ident)
    assert got_ident == ident
    return ent


COST = {3: 5.0, 4: None, 5: 2.0, 6: 3.0}


def test_second_process_takes_the_stored_winner_without_synchronising(monkeypatch, cache_dir):
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 4, 5, 6], COST) == 5
    assert len(tu.syncs) == 6  # two timing passes per candidate that accepted the shape (4 refused it)
    st = tu.ops.tune_stats()
    assert (st["full_tunes"], st["timing_passes"], st["stored"], st["cache_hits"]) == (1, 6, 1, 0)
    ent = _entries(cache_dir)
    assert len(ent) == 1
    (e,) = ent.values()
    assert e["cfg"] == 5 and e["best_us"] == pytest.approx(2.0 * 1e3) and e["runner_up_us"] == pytest.approx(3.0 * 1e3)

    tu.new_process()
    assert tu.tune(KEY, [3, 4, 5, 6], COST) == 5
    assert len(tu.syncs) == 0 and tu.runs == [5]  # the one warm launch of the stored winner, nothing else
    st = tu.ops.tune_stats()
    assert (st["full_tunes"], st["timing_passes"], st["stored"], st["cache_hits"]) == (0, 0, 0, 1)
    assert tu.ops._tuned_get(KEY, FAMS) == 5  # what ConvChain._plan reads
    assert tu.tune(KEY, [3, 4, 5, 6], COST) == 5 and tu.runs == [5]  # in memory from here on


def test_stored_id_that_is_not_a_candidate_is_never_launched(monkeypatch, cache_dir):
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 5, 6], COST) == 5
    tu.new_process()
    assert tu.tune(KEY, [3, 6], COST) == 6  # this process does not offer 5 for the layer
    assert 5 not in tu.runs
    st = tu.ops.tune_stats()
    assert (st["rejected"], st["full_tunes"], st["timing_passes"], st["stored"], st["cache_hits"]) == (1, 1, 4, 1, 0)
    assert [e["cfg"] for e in _entries(cache_dir).values()] == [6]  # the entry is replaced


def test_stored_id_whose_warm_launch_fails_is_rejected(monkeypatch, cache_dir):
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 5, 6], COST) == 5
    tu.new_process()
    assert tu.tune(KEY, [3, 5, 6], {3: 5.0, 5: None, 6: 3.0}) == 6  # 5 refuses the shape now
    st = tu.ops.tune_stats()
    assert (st["rejected"], st["full_tunes"], st["timing_passes"], st["stored"]) == (1, 1, 4, 1)
    assert [e["cfg"] for e in _entries(cache_dir).values()] == [6]


@pytest.mark.parametrize("field,value", [("lib_sha256", "cd" * 32), ("abi", 10), ("device", "AMD Instinct MI300X"), ("cus", 304),
                                         ("arch", "gfx942:sramecc+:xnack-")])
def test_another_identity_misses_and_leaves_the_first_file_alone(monkeypatch, cache_dir, field, value):
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 5, 6], COST) == 5
    with open(_file(cache_dir), "rb") as f:
        first = f.read()
    other = dict(IDENT, **{field: value})
    tu.new_process(other)
    assert tu.tune(KEY, [3, 5, 6], {3: 1.0, 5: 2.0, 6: 3.0}) == 3
    st = tu.ops.tune_stats()
    assert (st["cache_hits"], st["rejected"], st["full_tunes"], st["stored"]) == (0, 0, 1, 1)
    assert _file(cache_dir, other) != _file(cache_dir)
    assert [e["cfg"] for e in _entries(cache_dir, other).values()] == [3]
    with open(_file(cache_dir), "rb") as f:
        assert f.read() == first
    tu.new_process(IDENT)
    assert tu.tune(KEY, [3, 5, 6], COST) == 5 and len(tu.syncs) == 0


def test_another_family_set_misses_within_the_same_file(monkeypatch, cache_dir):
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 5, 6], COST) == 5
    tu.new_process()
    assert tu.tune(KEY, [3, 6], COST, families=(0, 1, 2, 3)) == 6
    assert tu.ops.tune_stats()["cache_hits"] == 0 and tu.ops.tune_stats()["full_tunes"] == 1
    ent = _entries(cache_dir)
    assert sorted(e["cfg"] for e in ent.values()) == [5, 6] and len(os.listdir(str(cache_dir))) == 2  # one file and its lock


def _good_file():
    name = tunecache.encode_key(KEY, FAMS)
    return {"format": 1, "identity": IDENT, "entries": {name: {"cfg": 6, "best_us": 1.0, "runner_up_us": 2.0}}}


def _with_entry(e):
    d = _good_file()
    d["entries"] = {tunecache.encode_key(KEY, FAMS): e}
    return json.dumps(d)


MALFORMED = {
    "truncated": json.dumps(_good_file())[:-25],
    "not json": "\x00\x01 winners \xff",
    "empty": "",
    "a list at the top": json.dumps([_good_file()]),
    "entries is a list": json.dumps(dict(_good_file(), entries=[1, 2])),
    "entry is a list": _with_entry([6]),
    "id as a string": _with_entry({"cfg": "6", "best_us": 1.0}),
    "id as a float": _with_entry({"cfg": 6.0}),
    "id as a bool": _with_entry({"cfg": True}),
    "negative id": _with_entry({"cfg": -1}),
    "huge id": _with_entry({"cfg": 10 ** 12}),
    "another identity's block": json.dumps(dict(_good_file(), identity=dict(IDENT, cus=64))),
    "identity is a string": json.dumps(dict(_good_file(), identity="MI355X")),
    "another format": json.dumps(dict(_good_file(), format=2)),
    "deeply nested": "[" * 100000,
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_file_is_ignored_and_overwritten(monkeypatch, cache_dir, what):
    os.makedirs(str(cache_dir))
    with open(_file(cache_dir), "w", encoding="latin-1") as f:
        f.write(MALFORMED[what])
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 5, 6], COST) == 5  # 6 -- what the damaged file may still name -- is not taken from it
    st = tu.ops.tune_stats()
    assert (st["full_tunes"], st["timing_passes"], st["cache_hits"], st["stored"]) == (1, 6, 0, 1)
    with open(_file(cache_dir)) as f:
        d = json.load(f)
    assert d["identity"] == IDENT and [e["cfg"] for e in d["entries"].values()] == [5]


def test_well_formed_file_of_the_same_shape_is_a_hit(monkeypatch, cache_dir):
    """The control of the test above: the same file without the damage is taken."""
    os.makedirs(str(cache_dir))
    with open(_file(cache_dir), "w") as f:
        json.dump(_good_file(), f)
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 5, 6], COST) == 6 and len(tu.syncs) == 0


@pytest.mark.parametrize("value", [None, "0", ""])
def test_off_means_off(monkeypatch, tmp_path, value):
    home = tmp_path / "home"
    home.mkdir()
    monkeypatch.setenv("HOME", str(home))
    monkeypatch.setenv("XDG_CACHE_HOME", str(home / "xdg"))
    monkeypatch.setattr(tunecache, "_default_on", False)
    if value is None:
        monkeypatch.delenv("DRBA_TUNE_CACHE", raising=False)
    else:
        monkeypatch.setenv("DRBA_TUNE_CACHE", value)
    tu = _Tuner(monkeypatch)
    monkeypatch.setattr(tunecache, "identity_provider", lambda device=None: pytest.fail("the identity is not asked for while the store is off"))
    assert tu.tune(KEY, [3, 5, 6], COST) == 5
    assert tu.ops.tune_stats()["stored"] == 0 and len(tu.syncs) == 6
    assert os.listdir(str(home)) == []


def test_cli_on_a_missing_input_creates_nothing(monkeypatch, tmp_path):
    from drba_amd import infer
    home = tmp_path / "home"
    home.mkdir()
    monkeypatch.setenv("HOME", str(home))
    monkeypatch.setenv("XDG_CACHE_HOME", str(home / "xdg"))
    monkeypatch.delenv("DRBA_TUNE_CACHE", raising=False)
    monkeypatch.setattr(tunecache, "_default_on", False)
    with pytest.raises(FileNotFoundError):
        infer.main(["-m", "rife", "-i", str(tmp_path / "nothing.npz"), "-o", str(tmp_path / "out.npz")])
    assert tunecache.directory() is None  # the input is checked before the store is turned on
    assert os.listdir(str(home)) == []


def test_cli_default_is_on_and_zero_turns_it_off(monkeypatch, tmp_path):
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "xdg"))
    monkeypatch.delenv("DRBA_TUNE_CACHE", raising=False)
    monkeypatch.setattr(tunecache, "_default_on", False)
    assert tunecache.directory() is None
    tunecache.default_on()  # what drba_amd.infer.main does behind the input check
    assert tunecache.directory() == str(tmp_path / "xdg" / "drba_amd")
    monkeypatch.setenv("DRBA_TUNE_CACHE", "0")
    assert tunecache.directory() is None
    monkeypatch.setenv("DRBA_TUNE_CACHE", "1")
    assert tunecache.directory() == str(tmp_path / "xdg" / "drba_amd")
    monkeypatch.delenv("XDG_CACHE_HOME")
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    assert tunecache.directory() == str(tmp_path / "home" / ".cache" / "drba_amd")
    assert not (tmp_path / "xdg").exists() and not (tmp_path / "home").exists()


def test_without_persist_nothing_is_kept(monkeypatch, cache_dir):
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 5, 6], COST, persist=False) == 5
    assert tu.ops._tune(("made", "up"), [3, 5], tu.run(COST)) == 5  # the signature test_abi.py uses
    assert not os.path.exists(str(cache_dir)) and tu.ops.tune_stats()["stored"] == 0


@pytest.mark.parametrize("what", ["lock", "temporary"])
def test_unwritable_directory_costs_persistence_only(monkeypatch, tmp_path, what):
    """A directory that exists and cannot be written (the lock file, or the temporary file, cannot be opened)."""
    d = tmp_path / "store"
    d.mkdir()

    def denied(*a, **k):
        raise PermissionError(13, "Permission denied", str(d))
    if what == "lock":
        real_open = os.open
        monkeypatch.setattr(tunecache.os, "open", lambda path, *a, **k: denied() if str(path).endswith(".lock") else real_open(path, *a, **k))
    else:
        monkeypatch.setattr(tunecache.tempfile, "mkstemp", denied)
    _unwritable(monkeypatch, str(d))
    assert [n for n in os.listdir(str(d)) if n.endswith(".json")] == []


def test_directory_that_cannot_be_created_costs_persistence_only(monkeypatch, tmp_path):
    blocker = tmp_path / "a_file"
    blocker.write_text("not a directory")
    _unwritable(monkeypatch, str(blocker / "store"))


def _unwritable(monkeypatch, where):
    monkeypatch.setenv("DRBA_TUNE_CACHE", where)
    tu = _Tuner(monkeypatch)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert tu.tune(KEY, [3, 5, 6], COST) == 5
        assert tu.tune(("conv3x3", 1, 39, 192, 8, 12, 2), [3, 5, 6], COST) == 5
        assert tu.tune(("deconv4x4", 1, 192, 24, 8, 12, 1), [3], COST) == 3
    assert len([x for x in w if "not kept" in str(x.message)]) == 1  # one warning, not one per shape
    assert tu.ops.tune_stats()["stored"] == 0 and tu.ops.tune_stats()["full_tunes"] == 3


def test_two_interleaved_writers_end_with_the_union(tmp_path):
    a, b = tunecache.Store(str(tmp_path), IDENT), tunecache.Store(str(tmp_path), IDENT)
    assert a.get(KEY, FAMS) is None and b.get(KEY, FAMS) is None  # both have read the (absent) file before either writes
    for k in range(10):
        assert a.put(("conv3x3", 1, k, 16, 8, 8, 1), FAMS, k, 1.0, 2.0)
        assert b.put(("deconv4x4", 1, k, 16, 8, 8, 0), FAMS, 100 + k, 1.0, None)
    assert b.put(("conv3x3_shuffle", 1, 64, 256, 8, 8), (4,), None)
    ent = tunecache.Store(str(tmp_path), IDENT).entries()
    assert len(ent) == 21
    assert sorted(e["cfg"] for e in ent.values() if "cfg" in e) == list(range(10)) + list(range(100, 110))
    assert a.get(("deconv4x4", 1, 3, 16, 8, 8, 0), FAMS)["cfg"] == 103  # a writer learns the other's entries when it writes
    assert [n for n in os.listdir(str(tmp_path)) if n.endswith(".tmp")] == []


_WRITER = """
import sys
sys.path.insert(0, %r)
from drba_amd import tunecache
ident = tunecache.make_identity(9, 'ab' * 32, 'AMD Instinct MI355X', 'gfx950:sramecc+:xnack-', 256)
s = tunecache.Store(sys.argv[1], ident)
base = int(sys.argv[2])
for k in range(50):
    assert s.put(('conv3x3', 1, base + k, 16, 8, 8, 1), (0, 1, 2, 3, 4), (base + k) %% 38, 1.0, 2.0)
"""


def test_two_processes_writing_at_once_lose_nothing(tmp_path):
    procs = [subprocess.Popen([sys.executable, "-c", _WRITER % ROOT, str(tmp_path), str(base)], stderr=subprocess.PIPE)
             for base in (0, 1000)]
    for p in procs:
        _, err = p.communicate(timeout=120)
        assert p.returncode == 0, err.decode()[-2000:]
    ent = tunecache.Store(str(tmp_path), tunecache.make_identity(9, "ab" * 32, "AMD Instinct MI355X", "gfx950:sramecc+:xnack-", 256)).entries()
    dims = sorted(json.loads(k)[1][1] for k in ent)
    assert dims == list(range(50)) + list(range(1000, 1050))


def test_no_configuration_accepts_is_remembered(monkeypatch, cache_dir):
    tu = _Tuner(monkeypatch)
    skey = ("conv3x3_shuffle", 1, 64, 256, 8, 10)
    with pytest.raises(tu.ops.NoKernelConfig):
        tu.tune(skey, [30, 31], {}, families=(4,))
    assert tu.runs == [30, 31] and tu.ops.tune_stats()["stored"] == 1
    assert list(_entries(cache_dir).values()) == [{"none": True}]
    del tu.runs[:]
    with pytest.raises(tu.ops.NoKernelConfig):  # the same process: not one launch
        tu.tune(skey, [30, 31], {}, families=(4,))
    assert tu.runs == []
    tu.new_process()
    with pytest.raises(tu.ops.NoKernelConfig) as e:  # another process
        tu.tune(skey, [30, 31], {30: 1.0, 31: 2.0}, families=(4,))
    assert tu.runs == [] and len(tu.syncs) == 0 and tu.ops.tune_stats()["negative_hits"] == 1
    assert isinstance(e.value, _lib.DrbaHipError) and "no kernel configuration accepts" in str(e.value)


@pytest.mark.parametrize("code", [-3, -1])
def test_launch_failure_is_not_remembered_as_no_configuration(monkeypatch, cache_dir, code):
    """Every warm launch fails with something other than DRBA_EUNSUPPORTED (a launch failure, a sticky earlier error): that is
    not a property of the shape -- an error, but not NoKernelConfig, and nothing is remembered in the process or in the store."""
    tu = _Tuner(monkeypatch)
    skey = ("conv3x3_shuffle", 1, 64, 256, 8, 10)
    for _ in range(2):
        del tu.runs[:]
        with pytest.raises(_lib.DrbaHipError) as e:
            tu.tune(skey, [30, 31], {30: code, 31: code}, families=(4,))
        assert not isinstance(e.value, tu.ops.NoKernelConfig) and tu.runs == [30, 31]  # asked again the second time
    with pytest.raises(_lib.DrbaHipError) as e:  # one refusal, one failure: still not "no configuration accepts"
        tu.tune(KEY, [3, 5], {3: None, 5: code})
    assert not isinstance(e.value, tu.ops.NoKernelConfig)
    assert tu.ops.tune_stats()["stored"] == 0 and not os.path.exists(str(cache_dir)) and tu.ops._no_config == set()
    assert tu.tune(skey, [30, 31], {30: 2.0, 31: 1.0}, families=(4,)) == 31  # the failure gone, the shape tunes as usual
    assert tu.tune(KEY, [3, 5], {3: 2.0, 5: code}) == 3  # a failing candidate beside a working one is simply not a candidate


def test_launch_failure_of_a_stored_winner_raises_and_keeps_the_entry(monkeypatch, cache_dir):
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 5, 6], COST) == 5
    before = _entries(cache_dir)
    tu.new_process()
    with pytest.raises(_lib.DrbaHipError):
        tu.tune(KEY, [3, 5, 6], {3: 5.0, 5: -3, 6: 3.0})
    st = tu.ops.tune_stats()
    assert tu.runs == [5] and (st["rejected"], st["full_tunes"], st["stored"], st["cache_hits"]) == (0, 0, 0, 0)
    assert _entries(cache_dir) == before
    assert tu.tune(KEY, [3, 5, 6], COST) == 5 and tu.ops.tune_stats()["cache_hits"] == 1  # the failure gone: a hit


def test_range_check_build_neither_reads_nor_writes_the_store(monkeypatch, cache_dir):
    """DRBA_CHECK_RANGE=1: a launch can answer DRBA_EUNSUPPORTED for what is in the data, so nothing such a process sees is kept."""
    tu = _Tuner(monkeypatch)
    assert tu.tune(KEY, [3, 5, 6], COST) == 5
    before = _entries(cache_dir)
    tu.new_process()
    monkeypatch.setenv("DRBA_CHECK_RANGE", "1")
    assert tu.tune(KEY, [3, 5, 6], {3: 5.0, 5: None, 6: 3.0}) == 6
    with pytest.raises(tu.ops.NoKernelConfig):
        tu.tune(("deconv4x4", 1, 192, 24, 8, 12, 1), [3], {})
    st = tu.ops.tune_stats()
    assert (st["cache_hits"], st["rejected"], st["stored"], st["full_tunes"]) == (0, 0, 0, 2) and _entries(cache_dir) == before


class _FakeLayer:
    """What conv3x3_shuffle reads of a Conv3x3, with packings of three candidates left behind by a tune."""
    stride, pre_slope, beta, bias, force_cfg, two_term_ok, act, post_slope = 1, None, None, None, None, True, 0, 0.0
    cin, cout = 4, 8

    def __init__(self):
        self._packed, self._keep, self.calls = {30: "p30", 31: "p31", 32: "p32"}, {31}, 0

    def __call__(self, x):
        self.calls += 1
        return "conv(x)"


class _FakeLib:
    def drba_conv3x3_num_cfgs(self):
        return 40

    def drba_conv3x3_cfg_stride(self, c):
        return 1

    def drba_conv3x3_cfg_family(self, c):
        return 4 if c >= 30 else 0

    def drba_conv3x3_packed_floats(self, cin, cout, c):
        return 16


def _fake_shuffle(monkeypatch, tune):
    import types

    from drba_amd import ops
    monkeypatch.setattr(ops._lib, "load", lambda: _FakeLib())
    monkeypatch.setattr(ops, "_f32", lambda x: x)
    monkeypatch.setattr(ops, "pixel_shuffle2", lambda y: ("shuffled", y))
    monkeypatch.setattr(ops, "_tune", tune)
    x = types.SimpleNamespace(shape=(1, 4, 6, 8), is_cuda=True, device=ops.torch.device("cpu"))
    layer = _FakeLayer()
    return ops, layer, x


def test_shuffle_falls_back_on_no_configuration_and_prunes_the_packings(monkeypatch):
    seen = {}

    def tune(key, cands, run, **kw):
        seen.update(key=key, cands=list(cands), kw=kw)
        raise ops.NoKernelConfig("no kernel configuration accepts this")
    ops, layer, x = _fake_shuffle(monkeypatch, tune)
    assert ops.conv3x3_shuffle(layer, x) == ("shuffled", "conv(x)") and layer.calls == 1  # the two kernels, as before
    assert seen["key"] == ("conv3x3_shuffle", 1, 4, 8, 6, 8) and seen["cands"] == list(range(30, 40))
    assert seen["kw"]["persist"] is True and tuple(seen["kw"]["families"]) == (4,)
    assert layer._packed == {31: "p31"}  # the packings the refused candidates left are dropped, the kept one stays


def test_shuffle_lets_any_other_error_through(monkeypatch):
    """conv3x3_shuffle used to catch every DrbaHipError of the tuner: a launch failure read as 'shape not supported'."""
    def tune(key, cands, run, **kw):
        raise _lib.DrbaHipError("drba_conv3x3_shuffle failed: launch failure (-3)")
    ops, layer, x = _fake_shuffle(monkeypatch, tune)
    with pytest.raises(_lib.DrbaHipError) as e:
        ops.conv3x3_shuffle(layer, x)
    assert not isinstance(e.value, ops.NoKernelConfig) and layer.calls == 0


def _tune_cli(args, env):
    r = subprocess.run([sys.executable, "-m", "drba_amd.tune"] + args, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_tune_command_lists_and_clears(tmp_path):
    d = tmp_path / "store"
    other = dict(IDENT, cus=64)
    s = tunecache.Store(str(d), IDENT)
    s.put(KEY, FAMS, 7, 41.5, 43.0)
    s.put(("conv3x3_shuffle", 1, 64, 256, 8, 10), (4,), None)
    tunecache.Store(str(d), other).put(("deconv4x4", 1, 192, 24, 8, 12, 1), FAMS, 2, 10.0, None)
    (d / "notes.txt").write_text("not the store's")
    env = dict(os.environ, DRBA_TUNE_CACHE=str(d))
    out = _tune_cli(["--list"], env)
    assert out["store"] == str(d) and len(out["files"]) == 2
    by_cus = {f["identity"]["cus"]: f for f in out["files"]}
    assert by_cus[256]["entries"][tunecache.encode_key(KEY, FAMS)] == {"cfg": 7, "best_us": 41.5, "runner_up_us": 43.0}
    assert {"none": True} in by_cus[256]["entries"].values() and len(by_cus[64]["entries"]) == 1
    out = _tune_cli(["--clear"], env)
    assert len([n for n in out["removed"] if n.endswith(".json")]) == 2
    assert os.listdir(str(d)) == ["notes.txt"]  # only what the store wrote is removed
    assert _tune_cli(["--list"], env)["files"] == []
    assert _tune_cli(["--list"], dict(env, DRBA_TUNE_CACHE="0"))["store"] is None


def test_rehearsal_reads_the_planted_cuts_off_the_driver_calls():
    """observed_cuts on the call pattern interpolate_stream makes for cuts at frames 2, 3 and 6 of an 8-frame clip."""
    from drba_amd import tune
    seg = [[("ts", 0, 1)],                      # head
           [("ts", 0, 1)],                      # centre 1: cut on the right (1 | 2)
           [],                                  # centre 2: both
           [("ts", 3, 4)],                      # centre 3: cut on the left
           [("drba", 4, 0)],
           [("ts", 4, 5)],                      # centre 5: cut on the right (5 | 6)
           [("ts", 6, 7)],                      # centre 6: cut on the left
           [("ts", 6, 7)]]                      # tail
    cuts, branches = tune.observed_cuts(seg, 8)
    assert cuts == [2, 3, 6]
    assert branches == {"head": 1, "head_cut": 0, "drba": 1, "cut_left": 2, "cut_right": 2, "cut_both": 1, "tail": 1}
    n, planted = tune.plan_clip(24.0, 60.0, -1, True)
    assert n == tune.MAX_FRAMES and [b - a for a, b in zip(planted[1:], planted[2:])] == [13, 14, 15, 16]
    assert tune.schedule_period(24.0, 60.0, -1) == 2 and tune.schedule_period(24.0, 48.0, 2) == 1
