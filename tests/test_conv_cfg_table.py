"""CPU: the public configuration ids of drba_conv3x3 / drba_deconv4x4s2 are pinned -- count, family, stride and packed size
of every id, the codes of the error paths, and (tests/golden/conv_pack_digests.json, tools/pack_digests.py) every packed
byte.  The table functions and the packers are host code: the library runs them without a device."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np

from drba_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONV_FAMILIES = [0] * 14 + [1] * 5 + [2, 3] + [4] * 17
CONV_STRIDES = [1] * 8 + [2] * 6 + [1] * 14 + [2, 2, 2, 2, 1, 1, 2, 2, 2, 1]
CONV_PACKED = {
    (32, 32): [9216, 9216, 9216, 18432, 9216, 9216, 9216, 9216, 9216, 9216, 9216, 9216, 9216, 9216, 13824, 27648, 41472, 13824,
               13824, 13824, 0, 9216, 18432, 27648, 9216, 9216, 9216, 0, 9216, 18432, 9216, 18432, 18432, 27648, 18432, 18432,
               27648, 27648],
    (64, 40): [36864, 36864, 36864, 36864, 27648, 36864, 36864, 27648, 27648, 36864, 36864, 36864, 27648, 36864, 55296, 55296,
               82944, 55296, 55296, 0, 55296, 36864, 36864, 55296, 36864, 36864, 0, 36864, 36864, 36864, 36864, 36864, 36864,
               55296, 36864, 36864, 55296, 55296],
    (52, 16): [16128, 16128, 16128, 32256, 8064, 16128, 16128, 8064, 7488, 14976, 14976, 14976, 7488, 14976] + [0] * 14 +
              [18432, 36864, 18432, 36864, 0, 0, 36864, 36864, 55296, 0],
}
DECONV_FAMILIES = [0] * 6 + [1] * 2 + [4] * 7
DECONV_PACKED = {(64, 52): [65536] * 6 + [98304] * 2 + [65536] * 7, (20, 52): [24576] * 6 + [0] * 9}


def test_conv_table_is_pinned():
    lib = _lib.load()
    n = lib.drba_conv3x3_num_cfgs()
    assert n == 38
    assert [lib.drba_conv3x3_cfg_family(c) for c in range(n)] == CONV_FAMILIES
    assert [lib.drba_conv3x3_cfg_stride(c) for c in range(n)] == CONV_STRIDES
    for (cin, cout), want in CONV_PACKED.items():
        assert [lib.drba_conv3x3_packed_floats(cin, cout, c) for c in range(n)] == want, (cin, cout)


def test_deconv_table_is_pinned():
    lib = _lib.load()
    n = lib.drba_deconv4x4_num_cfgs()
    assert n == 15
    assert [lib.drba_deconv4x4_cfg_family(c) for c in range(n)] == DECONV_FAMILIES
    for (cin, cout), want in DECONV_PACKED.items():
        assert [lib.drba_deconv4x4_packed_floats(cin, cout, c) for c in range(n)] == want, (cin, cout)


def test_ids_outside_the_table_and_error_codes():
    lib = _lib.load()
    n, nd = lib.drba_conv3x3_num_cfgs(), lib.drba_deconv4x4_num_cfgs()
    for cfg in (-1, n):
        assert lib.drba_conv3x3_cfg_family(cfg) == -1
        assert lib.drba_conv3x3_cfg_stride(cfg) == -1
        assert lib.drba_conv3x3_packed_floats(32, 32, cfg) == 0
    for cfg in (-1, nd):
        assert lib.drba_deconv4x4_cfg_family(cfg) == -1
        assert lib.drba_deconv4x4_packed_floats(64, 52, cfg) == 0
    w = np.ones(32 * 32 * 9, dtype=np.float32)
    buf = np.zeros(32 * 32 * 9 * 8, dtype=np.float32)
    wp, bp = C.c_void_p(w.ctypes.data), C.c_void_p(buf.ctypes.data)
    assert lib.drba_conv3x3_pack(wp, bp, 32, 32, n) == -1
    assert lib.drba_conv3x3(None, bp, None, None, None, None, bp, 1, 32, 8, 8, 32, 1, 0, 0.0, 0, 0.0, 0, None) == -1
    # Cout % 4 != 0: refused before anything is launched (the pointers are never read)
    assert lib.drba_conv3x3_shuffle(wp, bp, None, bp, 1, 32, 8, 8, 30, 0, 0.0, 23, None) == -2
    assert lib.drba_conv3x3_pick_cfg(3, 16, 8, 8, 3) == -2


def test_packed_bytes_match_the_recorded_digests():
    spec = importlib.util.spec_from_file_location("pack_digests", os.path.join(ROOT, "tools", "pack_digests.py"))
    pack_digests = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pack_digests)
    with open(os.path.join(ROOT, "tests", "golden", "conv_pack_digests.json")) as f:
        want = json.load(f)
    got = pack_digests.digests(_lib.load())
    assert sorted(got) == sorted(want) == ["conv", "deconv"]
    for kind in want:
        assert sorted(got[kind]) == sorted(want[kind]), kind
        for shape in want[kind]:
            assert sorted(got[kind][shape], key=int) == sorted(want[kind][shape], key=int), (kind, shape)  # the same ids pack
            wrong = [cfg for cfg in want[kind][shape] if got[kind][shape][cfg] != want[kind][shape][cfg]]
            assert not wrong, (kind, shape, wrong)
