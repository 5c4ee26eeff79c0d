"""GPU: the kernels two small model steps launch, against a recording (tests/golden/ops_launches.json: names and numbers, made
by this file's --record from a build of the commit the file names, on an MI355X).

tests/test_ops_calls.py pins what ops.py hands to the library on CPU tensors; this covers the routing only a device reaches:
the is_cuda branches (the fused encoder, the tuner), the pair-only feature layout and the convolution chains as one
library call.  Per launch the kernel's name and grid are compared.  A launch tagged conv3x3 / deconv4x4 is the exception:
which configuration (and so which kernel and grid) runs it is the tuner's timing-dependent choice, so its tag is compared
instead -- work, unit and label with the configuration id (the label's first tuple element) removed.

    python tests/test_gpu_ops_launches.py --record [out.json]
"""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "ops_launches.json")
TS = np.array([0.75, 1.25])


def _frames(n, h, w, dev):
    import torch

    from drba_amd.utils import synth
    return [torch.from_numpy(f.transpose(2, 0, 1)).unsqueeze(0).float().div(255.0).to(dev) for f in synth.make_clip(n, h, w, seed=1234)]


def _rife(dev):
    """-> a function of a fresh model: a cold step and a warm one (the `reuse` of the first) over three 64x128 frames."""
    from drba_amd.models.rife import RIFE
    from drba_amd.utils import synth

    def steps():
        fr = _frames(3, 64, 128, dev)  # (new tensors per run: what the models keep on a frame tensor belongs to one run)
        m = RIFE(weights=synth.ifnet_state_dict(seed=0), scale=1.0, device=dev)
        m.GROUP = 1  # no side-stream staging of a group of steps: launches in call order
        _, reuse = m.inference_ts_drba(fr[0], fr[1], fr[2], TS, None, True)
        m.inference_ts_drba(fr[1], fr[2], fr[0], TS, reuse, True)
    return steps


def _gmfss_union(dev):
    from drba_amd.models.gmfss_union import GMFSS_UNION
    from drba_amd.utils import synth

    def steps():
        fr = _frames(3, 128, 256, dev)
        m = GMFSS_UNION(weights=synth.gmfss_union_state_dicts(0), scale=1.0, device=dev)
        m.inference_ts_drba(fr[0], fr[1], fr[2], TS, None, True)
    return steps


SCENARIOS = {"rife": _rife, "gmfss_union": _gmfss_union}


def launches(name):
    """The launches of the scenario's steps on a fresh model, after one untraced run (another model) in which the tuner met every
    shape and so every chain plans at its first call -> [[kernel name, grid] or ["conv", work, unit, label without cfg], ...]."""
    import torch

    from drba_amd import ops
    steps = SCENARIOS[name](torch.device("cuda:0"))
    steps()
    torch.cuda.synchronize()
    ops.trace_begin()
    try:
        steps()
        torch.cuda.synchronize()
    finally:
        recs = ops.trace_end()
    out = []
    for r in recs:
        m = re.match(r"^((?:de)?conv[34]x[34]) \((\d+), (.*)\)$", r["label"] or "")
        out.append(["conv", repr(r["work"]), r["unit"], f"{m.group(1)} ({m.group(3)})"] if m else [r["name"], list(r["grid"])])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_launches_repeat_the_recording(name):
    with open(GOLDEN) as f:
        gold = json.load(f)["scenarios"][name]
    got = launches(name)
    print(f"{name}: {len(got)} launches, {sum(1 for g in got if g[0] == 'conv')} of them tagged convolutions")
    first = next((k for k, (a, b) in enumerate(zip(got, gold)) if a != b), None)
    assert first is None, f"launch {first}: {got[first]} != recorded {gold[first]}"
    assert len(got) == len(gold)


if __name__ == "__main__":
    assert len(sys.argv) > 1 and sys.argv[1] == "--record", __doc__
    import subprocess
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or os.environ.get("DRBA_COMMIT", "")
    data = {name: launches(name) for name in SCENARIOS}
    with open(path, "w") as f:  # one line per launch
        f.write('{"made_from": %s,\n "scenarios": {\n' % json.dumps({"commit": head, "by": "python tests/test_gpu_ops_launches.py --record"}))
        f.write(",\n".join('  %s: [\n%s\n  ]' % (json.dumps(k), ",\n".join("   " + json.dumps(l) for l in v)) for k, v in data.items()))
        f.write("\n }}\n")
    print(f"wrote {path}: " + ", ".join(f"{k} {len(v)} launches" for k, v in data.items()))
