#!/usr/bin/env python3
"""SHA-256 of the packed weights of every drba_conv3x3 / drba_deconv4x4s2 configuration on a few layer shapes (host code
only: no GPU).  tests/test_conv_cfg_table.py recomputes them, so a change of the host glue that moves one packed byte shows.

    python tools/pack_digests.py [out.json]      (default: tests/golden/conv_pack_digests.json)

The weights are an integer recurrence (no RNG: the bytes do not depend on a library version).  Regenerate the file only
from a build whose packing is known good -- when a configuration is ADDED, from the commit before the change plus the new ids."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONV_SHAPES = [(32, 32), (64, 40), (96, 96), (192, 192), (52, 16)]  # (Cin, Cout)
DECONV_SHAPES = [(64, 52), (96, 64)]
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "conv_pack_digests.json")


def weights(n):
    """n fp32 weights in (-2, 2): x <- (75 x + 74) mod 65537, every step exact in float64."""
    x, out = 1.0, np.empty(n, dtype=np.float64)
    for k in range(n):
        x = (x * 75.0 + 74.0) % 65537.0
        out[k] = x
    return ((out / 65537.0 - 0.5) * 4.0).astype(np.float32)


def digests(lib):
    """{"conv" | "deconv": {"<Cin>x<Cout>": {"<cfg>": sha256 hex}}} over every (cfg, shape) with packed_floats > 0."""
    kinds = (("conv", CONV_SHAPES, 9, lib.drba_conv3x3_num_cfgs, lib.drba_conv3x3_packed_floats, lib.drba_conv3x3_pack),
             ("deconv", DECONV_SHAPES, 16, lib.drba_deconv4x4_num_cfgs, lib.drba_deconv4x4_packed_floats, lib.drba_deconv4x4_pack))
    pool = weights(max(cin * cout * taps for _, shapes, taps, *_ in kinds for cin, cout in shapes))
    out = {}
    for kind, shapes, taps, num_cfgs, packed_floats, pack in kinds:
        for cin, cout in shapes:
            w = np.ascontiguousarray(pool[:cin * cout * taps])
            per_cfg = out.setdefault(kind, {}).setdefault(f"{cin}x{cout}", {})
            for cfg in range(num_cfgs()):
                n = packed_floats(cin, cout, cfg)
                if n == 0:
                    continue
                buf = np.full(n, np.float32(-1.0))
                rc = pack(C.c_void_p(w.ctypes.data), C.c_void_p(buf.ctypes.data), cin, cout, cfg)
                assert rc == 0, (kind, cin, cout, cfg, rc)
                per_cfg[str(cfg)] = hashlib.sha256(buf.tobytes()).hexdigest()
    return out


if __name__ == "__main__":
    from drba_amd import _lib

    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    with open(path, "w") as f:
        json.dump(digests(_lib.load()), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}")
