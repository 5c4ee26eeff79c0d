"""CPU: what drba_amd/ops.py hands to the C ABI against a recording of it (tests/golden/ops_calls.json, made by
tools/ops_calls.py from the commit the file names: the last one before the layer / chain / stage-item host glue of ops.py
was folded into one copy each).

Every scenario must repeat the recording call for call: entry-point names, every integer and float argument, the identity
of every pointer (the ordinal of its first appearance), every field of the structs and arrays handed over (stage items,
flow terms, DRM jobs, chain layer descriptors), the algorithmic-work tags of a traced run and the shapes returned.

The file holds one SHA-256 per scenario; a mismatch names the command that prints the full recording, to be run on both
commits and diffed.
"""
import ast
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("ops_calls", os.path.join(ROOT, "tools", "ops_calls.py"))
oc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oc)

with open(os.path.join(ROOT, "tests", "golden", "ops_calls.json")) as f:
    GOLD = json.load(f)


def test_recording_covers_the_scenarios():
    assert len(GOLD["made_from"]["commit"]) == 40 and not GOLD["made_from"]["drba_amd_modified"]
    assert sorted(GOLD["scenarios"]) == sorted(oc.SCENARIOS)


@pytest.mark.parametrize("name", list(oc.SCENARIOS))
def test_ops_repeat_the_recording(name):
    gold, got = GOLD["scenarios"][name], oc.summarise(oc.record(name))
    assert (got["calls"], got["pointers"], got["tags"]) == (gold["calls"], gold["pointers"], gold["tags"]), \
        f"python tools/ops_calls.py --dump {name}"
    assert got["sha256"] == gold["sha256"], f"python tools/ops_calls.py --dump {name}"


def test_switches_and_tuner_state_are_put_back():
    from drba_amd import _lib, ops
    before = {k: getattr(ops, k) for k in oc._SWITCHES}, dict(ops._tuned), _lib.load, ops._f32
    oc.record("chain_plan")
    oc.record("rife/24bit")
    assert before == ({k: getattr(ops, k) for k in oc._SWITCHES}, dict(ops._tuned), _lib.load, ops._f32)


def test_linear_split_width_is_written_by_the_constructor_only():
    """LinearSplit.cat used to overwrite self.k twice (and put it back) so that _rows checked the right width, on an object the
    main, lookahead and prefetch call paths share.  The recording cannot see that (k before == k after on both sides)."""
    with open(os.path.join(ROOT, "drba_amd", "ops.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "LinearSplit")
    writers = set()
    for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef)):
        for node in ast.walk(fn):
            targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, (ast.AugAssign, ast.AnnAssign)) else []
            for t in targets:
                for a in ast.walk(t):
                    if isinstance(a, ast.Attribute) and a.attr == "k" and isinstance(a.value, ast.Name) and a.value.id == "self":
                        writers.add(fn.name)
    assert writers == {"__init__"}, writers
