#!/usr/bin/env python3
"""What drba_amd/ops.py hands to the C ABI, recorded on CPU tensors with the library's launches stubbed (host code only: no
GPU): entry-point name and every argument of every call, over the dry-run plumbing cases of tests/test_dryrun.py and direct
calls of the wrappers those cannot reach.  tests/test_ops_calls.py replays the scenarios on the tree and compares, so a
swapped pointer, a dropped struct field or a changed algorithmic-work tag (bench.py's roofline numerators) shows.

    python tools/ops_calls.py [out.json]      (default: tests/golden/ops_calls.json)
    python tools/ops_calls.py --dump NAME     (the full recording of one scenario on stdout)
    python tools/ops_calls.py --list

How a call is written down:
  * the stub is the one of tests/test_dryrun.py: pure host entry points (*_pack, *_packed_floats, *_pick_cfg, ...) run for
    real, every other call is checked against its ctypes prototype and returns 0.  The launches and the *_pack calls (they
    take pointers) are logged;
  * integers by value, floats and doubles by repr;
  * a pointer as "null" or "p<k>", k the ordinal of its first appearance in the scenario: identity, not address.  That is
    reproducible only if no address is used twice, so a scenario runs inside a TorchFunctionMode that keeps every result of a
    torch call alive until the recording is done;
  * an argument that points at ctypes memory (drba_stage_item_t[n], drba_flow_terms_t, drba_drm_job_t[n],
    drba_conv_layer_t[n], the void*[n] of drba_ifblock_update_batch, the float[3] of drba_channel_normalize3) is decoded
    field by field: that memory is freed and reused between calls;
  * each scenario runs a second time with ops.TRACE = [] and a drba_trace_count that returns the number of launches logged
    so far: the TRACE list (first index, [(work, unit, label)]) is part of the record;
  * the shapes of what the wrappers return.

The file keeps one SHA-256 per scenario; when the test reports one, --dump on the two commits shows what differs.  The
tool refuses to write the file unless two recordings of every scenario agree.

Regenerate the file only from a commit whose ops.py is known good (the GPU suite passes); the file names the commit."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import types

import numpy as np
import torch
from torch.overrides import TorchFunctionMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from drba_amd import _lib, ops  # noqa: E402
from drba_amd.utils import synth  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "ops_calls.json")
CPU = torch.device("cpu")
_HOST = ("_pick_cfg", "_packed_floats", "_pack", "_ws_floats", "_supported", "drba_abi_version", "drba_error_string")

# entry point -> {argument index: (what the pointer is, index of the argument that holds the count or None)}
_ITEMS, _TERMS = ("items", 1), ("terms", None)
DECODE = {
    "drba_ifblock_input_batch": {0: _ITEMS},
    "drba_ifblock_input_lds_batch": {0: _ITEMS},
    "drba_ifblock_input_lazy_batch": {0: _ITEMS, 2: _TERMS},
    "drba_stage_conv0_batch": {0: _ITEMS, 2: _TERMS},
    "drba_stage_conv16_batch": {0: _ITEMS, 2: _TERMS},
    "drba_warp_blend_lazy_batch": {0: _ITEMS, 2: _TERMS},
    "drba_drm_rife_linear_batch": {0: ("jobs", 1)},
    "drba_conv_chain": {4: ("layers", 5)},
    "drba_ifblock_update_batch": {0: ("ptrs", 3), 1: ("ptrs", 3), 2: ("ptrs", 3)},
    "drba_channel_normalize3": {4: ("float3", None), 5: ("float3", None)},
}


class Keep(TorchFunctionMode):
    """Every result of a torch call stays referenced (`kept` outlives the recording): no address is handed out twice."""

    def __init__(self, kept):
        super().__init__()
        self.kept = kept

    def __torch_function__(self, func, types, args=(), kwargs=None):
        r = func(*args, **(kwargs or {}))
        self.kept.append(r)
        return r


class Recorder:
    """The stub library of one recording: the call log, the pointer ordinals and the launch count."""

    def __init__(self, real):
        self._real, self.calls, self.ptrs, self.launches = real, [], {}, 0

    def ptr(self, v):
        if isinstance(v, C.c_void_p):
            v = v.value
        elif v is not None and not isinstance(v, int):
            v = C.cast(v, C.c_void_p).value
        return "null" if not v else "p%d" % self.ptrs.setdefault(v, len(self.ptrs))

    def note(self, *entry):
        """A line of the log that is not a library call (what a planner returned, an attribute read)."""
        self.calls.append(list(entry))

    def _struct(self, s, pointers, values):
        d = {f: self.ptr(getattr(s, f)) for f in pointers}
        d.update({f: getattr(s, f) for f in values})
        return d

    def decode(self, kind, a, n):
        addr = a.value if isinstance(a, C.c_void_p) else (C.cast(a, C.c_void_p).value if a is not None else None)
        if not addr:
            return "null"
        if kind == "items":
            out = []
            for it in (_lib.StageItem * n).from_address(addr):
                d = self._struct(it, ("img0", "img1", "f0", "f1", "f0_pair", "f1_pair", "timestep_map", "flow", "tmp_prev", "flow_out",
                                      "out", "img0_x4", "img1_x4"), ())
                d["timestep_scalar"] = repr(float(it.timestep_scalar))
                d["term"] = [self.ptr(t) for t in it.term]
                out.append(d)
            return out
        if kind == "terms":
            ft = _lib.FlowTerms.from_address(addr)
            return {"n": ft.n, "h": list(ft.h), "w": list(ft.w), "scale": [repr(float(s)) for s in ft.scale]}
        if kind == "jobs":
            return [{"flow_self": self.ptr(j.flow_self), "flow_other": self.ptr(j.flow_other), "t": repr(float(j.t)), "out": self.ptr(j.out)}
                    for j in (_lib.DrmJob * n).from_address(addr)]
        if kind == "layers":
            return [self._struct(l, ("packed_w", "bias", "beta"), ("cin", "cout", "stride", "act", "cfg", "residual", "deconv", "pixel_shuffle"))
                    for l in (_lib.ConvLayer * n).from_address(addr)]
        if kind == "ptrs":
            return [self.ptr(p) for p in (C.c_void_p * n).from_address(addr)]
        assert kind == "float3", kind
        return [repr(float(v)) for v in (C.c_float * 3).from_address(addr)]

    def _log(self, name, args, argtypes):
        row = [name]
        for k, (a, t) in enumerate(zip(args, argtypes)):
            if k in DECODE.get(name, ()):
                kind, cnt = DECODE[name][k]
                row.append(self.decode(kind, a, None if cnt is None else int(args[cnt])))
            elif t is C.c_void_p:
                row.append(self.ptr(a))
            elif t in (C.c_float, C.c_double):
                row.append(repr(float(a.value if isinstance(a, t) else a)))
            else:
                row.append(int(a.value if isinstance(a, t) else a))
        self.calls.append(row)

    def __getattr__(self, name):
        real = getattr(self._real, name)
        host = name.endswith(_HOST)
        if host and not name.endswith("_pack"):
            return real  # pure host functions of numbers: run for real, not logged
        if name == "drba_trace_count":
            return lambda: self.launches
        argtypes = real.argtypes

        def stub(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} args, prototype has {len(argtypes)}"
            for a, t in zip(args, argtypes):
                if not isinstance(a, t):
                    t(a)  # raises if not convertible (e.g. a float passed for c_int)
            self._log(name, args, argtypes)
            if host:
                return real(*args)
            self.launches += 1
            return 0
        return stub


_SWITCHES = ("AUTOTUNE", "CONV_FAMILIES", "LAZY_FLOW", "STAGE_CONV_FUSED", "STAGE_CONV_TWO_TERM", "STAGE_CONV_S2", "HEAD_TWO_TERM", "HEAD_FUSED",
             "ATTN_TWO_TERM", "PAIR_FEATURES", "IMG_X4", "LDS_STAGE_INPUT", "TRACE")


@contextlib.contextmanager
def dry(rec):
    """tests/test_dryrun.py's `dry` fixture around one recording; the module's switches and tuner state are put back after it."""
    saved = {k: getattr(ops, k) for k in _SWITCHES + ("_f32", "_stream", "default_device", "_workspace", "_zero_workspace")}
    tuned, noc, load = dict(ops._tuned), set(ops._no_config), _lib.load
    ops._ws_token.clear()
    _lib.load = lambda: rec
    ops._f32 = lambda t, name="tensor": t.float().contiguous()
    ops._stream = lambda: C.c_void_p(0)
    ops.default_device = lambda: CPU
    ops._workspace = lambda dev, n, keep_token=False: torch.empty(int(n), dtype=torch.float32)
    ops._zero_workspace = lambda dev, n: torch.zeros(int(n), dtype=torch.float32)
    try:
        yield
    finally:
        _lib.load = load
        for k, v in saved.items():
            setattr(ops, k, v)
        ops._tuned.clear(), ops._tuned.update(tuned)
        ops._no_config.clear(), ops._no_config.update(noc)
        ops._ws_token.clear()


def shapes(x):
    """The shape of every tensor of a (nested) return value; numbers and strings as they are."""
    if torch.is_tensor(x):
        return list(x.shape)
    if isinstance(x, (list, tuple)):
        return [shapes(v) for v in x]
    if isinstance(x, dict):
        return {str(k): shapes(v) for k, v in sorted(x.items())}
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, float):
        return repr(x)
    return type(x).__name__


# ----------------------------------------------------------------------------- the scenarios: f(rec) -> what to keep of the returns
def _ifnet():
    from drba_amd.models.rife_426_heavy.IFNet_HDv3 import IFNet
    net = IFNet().to(CPU).eval()
    net.load_state_dict(synth.ifnet_state_dict(0))
    return net


def _rife(families=None, **switches):
    def run(rec):
        from drba_amd.models import rife as rife_mod
        for k, v in switches.items():
            setattr(ops, k, v)
        if families is not None:
            ops.set_precision(families)
        m = rife_mod.RIFE.__new__(rife_mod.RIFE)
        m.device = CPU
        m.ifnet = _ifnet()
        m.scale, m.scale_list, m.pad_size = 1.0, [16, 8, 4, 2, 1], 64
        I = [torch.rand(1, 3, 64, 128) for _ in range(3)]
        out, reuse = m.inference_ts_drba(I[0], I[1], I[2], np.array([0.75, 1.0, 1.25]), None, True)
        assert out[1] is I[1]
        out2, reuse2 = m.inference_ts_drba(I[0], I[1], I[2], np.array([0.6]), reuse, False)  # non-linear DRM composition
        r = m.inference_ts(I[0], I[1], np.array([0.0, 0.5, 1.0]))
        assert r[0] is I[0] and r[2] is I[1]
        return [out, reuse, out2, reuse2, r]
    return run


def _forward_pairs(scale, n_items):
    def run(rec):
        net = _ifnet()
        sl = [16 / scale, 8 / scale, 4 / scale, 2 / scale, 1 / scale]
        H, W = 128, 128
        img = [torch.rand(1, 3, H, W) for _ in range(2)]
        f = [torch.rand(1, 16, H, W) for _ in range(2)]
        items = [(img[0], img[1], 0.1 * (k + 1), f[0], f[1]) for k in range(n_items)]
        frames = net.forward_pairs(items, sl)
        state = net.forward_pairs(items, sl, 0, 3)
        assert (state[3] == "lazy") == (scale <= 1)
        return [frames, state, net.forward_pairs(items, sl, 3, 5, state)]
    return run


def _gmfss(rec):
    from drba_amd.models import gmfss as g
    from drba_amd.models.model_gmfss_union.GMFSS import Model
    sds = synth.gmfss_union_state_dicts(0)
    fusion = synth.seeded_state_dict(synth.gridnet_shapes(12, "head"), 0, "grid.")
    m = g.GMFSS.__new__(g.GMFSS)
    m.model = Model(union=False)
    m.model.load_state_dicts(sds["flownet"], sds["metric"], sds["feat"], fusion, CPU)
    m.scale, m.pad_size = 1.0, 64
    I = [torch.rand(1, 3, 128, 256) for _ in range(3)]
    out, reuse = m.inference_ts_drba(I[0], I[1], I[2], np.array([0.75, 1.25]), None, True)
    return [out, reuse, m.inference_ts(I[0], I[1], np.array([0.5]))]


def _gmfss_union(scale, size):
    def run(rec):
        from drba_amd.models import gmfss_union as gu
        from drba_amd.models.model_gmfss_union.GMFSS import Model
        from drba_amd.models.rife_426_heavy.IFNet_HDv3 import IFNet
        sds = synth.gmfss_union_state_dicts(0)
        m = gu.GMFSS_UNION.__new__(gu.GMFSS_UNION)
        m.model = Model(union=True)
        m.model.load_state_dicts(sds["flownet"], sds["metric"], sds["feat"], sds["fusion"], CPU)
        m.ifnet = IFNet().to(CPU).eval()
        m.ifnet.load_state_dict(sds["rife"])
        m.scale, m.pad_size = scale, 128
        m.scale_list = [16 / scale, 8 / scale, 4 / scale, 2 / scale, 1 / scale]
        H, W = size
        I = [torch.rand(1, 3, H, W) for _ in range(3)]
        out, reuse = m.inference_ts_drba(I[0], I[1], I[2], np.array([0.75, 1.0, 1.25]), None, True)
        out2, reuse2 = m.inference_ts_drba(I[0], I[1], I[2], np.array([1.4]), reuse, False)
        return [out, reuse, out2, reuse2, m.inference_ts(I[0], I[1], np.array([0.0, 0.5, 1.0]))]
    return run


def _operator_surface(rec):
    from drba_amd.models import drm
    from drba_amd.models.rife_426_heavy.IFNet_HDv3 import IFBlock
    from drba_amd.models.rife_426_heavy.warplayer import warp
    from drba_amd.models.softsplat.softsplat import softsplat
    from drba_amd.models.utils import tools
    x, f, mt = torch.rand(1, 3, 16, 24), torch.rand(1, 2, 16, 24), torch.rand(1, 1, 16, 24)
    res = [warp(x, f)]
    for mode, metric in (("sum", None), ("avg", None), ("linear", mt), ("soft-zeroeps", mt)):
        res.append(softsplat(x, f, metric, mode))
    for fn in (drm.calc_drm_gmfss, drm.calc_drm_rife_auxiliary):
        for lin in (True, False):
            for mm in ((mt, mt), (None, None)):
                res.append(fn(0.3, f, f, mm[0], mm[1], lin))
    res += [drm.calc_drm_rife(0.3, f, f, True), tools.distance_calculator(f), tools.resize(x, (20, 30))]
    blk = IFBlock(synth.ifnet_state_dict(0), "block1.", CPU)
    res.append(blk(torch.rand(1, 48, 64, 64), torch.rand(1, 4, 64, 64), scale=2))
    return res


def _non_union(rec):
    from models.model_gmfss.GMFSS import Model
    sds = synth.gmfss_union_state_dicts(0)
    fusion12 = synth.seeded_state_dict(synth.gridnet_shapes(12, "head"), 0, "grid.")
    m = Model()
    m.load_state_dicts(sds["flownet"], sds["metric"], sds["feat"], fusion12, CPU)
    I0, I1 = torch.rand(1, 3, 128, 256), torch.rand(1, 3, 128, 256)
    return m.fusion_inputs(I0, I1, m.reuse(I0, I1, 1.0), 0.4, 0.6)


def _head_fused(rec):
    enc = _ifnet().encode
    layers = (enc.cnn0, enc.cnn1, enc.cnn2, enc.cnn3)
    img, res = torch.rand(1, 3, 64, 128), []
    for two in (True, False):
        ops.HEAD_TWO_TERM = two
        holder = types.SimpleNamespace()
        for planar in (True, False):
            f = ops.head_fused(img, layers, holder, planar=planar)
            res.append([f, getattr(f, "_drba_pair", None), bool(getattr(f, "_drba_is_pair", False))])
        f = ops.head_fused(img, layers, holder)  # packed once per holder and precision: no second *_pack
        res.append([f, sorted(vars(holder))])
    ops.HEAD_TWO_TERM = None
    res.append(ops.head_fused(torch.rand(1, 3, 63, 128), layers, types.SimpleNamespace()))  # odd height: refused
    assert res[-1] is None
    return res


def _items(B, H, W, x4=()):
    """B stage items over two frames each (odd items: the timestep as a map); `x4`: per item, which of its frames get an [H,W,4] copy."""
    items = []
    for k in range(B):
        i0, i1 = torch.rand(1, 3, H, W), torch.rand(1, 3, H, W)
        for img, want in zip((i0, i1), x4[k] if k < len(x4) else (False, False)):
            if want:
                ops.rgbx(img)
        t = torch.full((1, 1, H, W), 0.25 * (k + 1)) if k % 2 else 0.25 * (k + 1)
        items.append((i0, i1, t, torch.rand(1, 16, H, W), torch.rand(1, 16, H, W)))
    return items


def _stage_conv0(rec):
    H, W, res = 64, 128, []
    for two in (True, False):
        ops.STAGE_CONV_TWO_TERM = two
        conv = _ifnet().block[4].conv0_0
        tmp = lambda B, s: torch.rand(B, 13, H // s, W // s)  # noqa: E731
        # scale 1, the materialised flow with the previous stage's update folded in
        items = _items(2, H, W, x4=[(True, True), (True, True)])
        res.append(ops.stage_conv0(items, [torch.rand(1, 4, H, W), None], tmp(2, 2), 2, conv, fold=True))
        # scale 1, the flow as terms (the frames of one item without their [H,W,4] copies: no item of the launch gets them)
        items = _items(2, H, W, x4=[(True, True), (True, False)])
        terms = [(tmp(2, 8), 8), (tmp(2, 4), 4)]
        res.append(ops.stage_conv0(items, None, tmp(2, 2), 2, conv, terms=terms, scale=1))
        res.append(ops.stage_conv0_ok(conv, H, W, 1, 2, items=items))
        if two:  # scale 2: the two-term kernel only, every frame with its [H,W,4] copy
            items = _items(2, H, W, x4=[(True, True), (True, True)])
            res.append(ops.stage_conv0_ok(conv, H, W, 2, 4, items=items))
            res.append(ops.stage_conv0(items, None, tmp(2, 4), 4, conv, terms=[(tmp(2, 8), 8)], scale=2))
        # three items into batch slices of a wider tensor
        items = _items(3, H, W, x4=[(True, True)] * 3)
        wide = torch.empty(5, conv.cout, H // 2, W // 2)
        res.append(ops.stage_conv0(items, None, tmp(3, 2), 2, conv, terms=[(tmp(3, 4), 4)], scale=1, out=wide[1:4]))
        res.append(sorted(a for a in vars(conv) if a.startswith("_stage_pack")))
    return res


def _stage_inputs(rec):
    H, W, res = 64, 128, []
    for scale in (8, 2, 1):
        h, w = H // scale, W // scale
        tmp = lambda B, s: torch.rand(B, 13, H // s, W // s)  # noqa: E731
        # item 0: both frames with their [H,W,4] copies; item 1: only one of the two (the planes are read)
        items = _items(2, H, W, x4=[(True, True), (True, False)])
        res.append(ops.stage_inputs(items, None, None, 1.0, scale, torch.empty(2, 39, h, w), lds=False))
        flows = [torch.rand(1, 4, H, W) for _ in range(2)]
        res.append(ops.stage_inputs(items, flows, tmp(2, 2 * scale), 2 * scale, scale, torch.empty(2, 52, h, w), lds=False))
        res.append(ops.stage_inputs(items, flows, tmp(2, 2 * scale), 2 * scale, scale, torch.empty(2, 52, h, w)))
        res.append(ops.stage_inputs(items, [flows[0], None], tmp(2, 2 * scale), 2 * scale, scale, torch.empty(2, 52, h, w), fold=True))
        terms = [(tmp(2, 8 * scale), 8 * scale), (tmp(2, 4 * scale), 4 * scale)]
        res.append(ops.stage_inputs(items, None, tmp(2, 2 * scale), 2 * scale, scale, torch.empty(2, 52, h, w), terms=terms))
    # the single-item forms
    (i0, i1, t, f0, f1), (j0, j1, tm, g0, g1) = _items(2, H, W)
    res.append(ops.ifblock_input(i0, i1, f0, f1, t, None, None, 1.0, 8))
    res.append(ops.ifblock_input(j0, j1, g0, g1, tm, torch.rand(1, 4, H, W), torch.rand(1, 13, H // 8, W // 8), 8, 4))
    res.append(ops.ifblock_input_lds(i0, i1, f0, f1, t, torch.rand(1, 4, H, W), torch.rand(1, 13, H // 4, W // 4), 4, 2))
    res.append(ops.ifblock_input_lds(j0, j1, g0, g1, tm, None, torch.rand(1, 13, H // 2, W // 2), 2, 1, fold=True))
    return res


def _warp_blend_lazy(rec):
    H, W = 64, 128
    items = _items(3, H, W, x4=[(True, True), (True, False), (False, False)])
    terms = [(torch.rand(3, 13, H // 4, W // 4), 4), (torch.rand(3, 13, H // 2, W // 2), 2)]
    return ops.warp_blend_lazy(items, terms, torch.rand(3, 13, H, W), 1)


def _flow_updates(rec):
    tmp, H, W = torch.rand(3, 13, 16, 32), 64, 128
    flows = [torch.rand(1, 4, H, W), None, torch.rand(1, 4, H, W)]
    return [ops.flow_updates(tmp, flows, H, W, 4, whole=True), ops.flow_updates(tmp, flows, H, W, 4)]


def _drm_many(rec):
    fl = [torch.rand(1, 2, 16, 24) for _ in range(4)]
    return ops.drm_rife_linear_many([(fl[k % 4], fl[(k + 1) % 4], 0.1 * (k + 1)) for k in range(9)])


def _softsplat_many(rec):
    n, h, w = 1, 16, 24
    xs = [torch.rand(n, c, h, w) for c in (3, 16, 32)]
    flow, metric = torch.rand(n, 2, h, w), torch.rand(n, 1, h, w)
    # (the dry-run's workspace is a new buffer per call; the index lives in the workspace, so this scenario keeps one)
    ws = torch.empty(int(max(_lib.load().drba_softsplat_ws_floats(n, x.shape[1], h, w) for x in xs)), dtype=torch.float32)
    ops._workspace = lambda dev, nfloats, keep_token=False: ws
    res = [ops.softsplat_many(xs, flow, metric, "soft")]
    res.append(ops.softsplat_many(xs, flow, metric, "soft", reuse_index=True))   # honoured: no input rebuilds the index
    flow.add_(1.0)
    res.append(ops.softsplat_many(xs, flow, metric, "soft", reuse_index=True))   # refused: the flow was written in place
    res.append(ops.softsplat_many(xs, flow, metric, "soft", keep_quad=True))
    res.append(ops.softsplat_many(xs, flow, metric, "soft", reuse_index=True, keep_quad=True))
    return res


def _chain_plan(rec):
    from drba_amd.models.rife_426_heavy.IFNet_HDv3 import IFBlock
    lib, res = rec._real, []  # (the tuner's candidate lists are numbers of the library itself)

    def plan(tag, chain):
        p = chain._plan(2, 38, 54, CPU)
        if p is None:
            rec.note("plan", tag, None)
        else:
            rec.note("plan", tag, sorted(p), rec.decode("layers", p["descs"], len(chain.layers)), [rec.ptr(t.data_ptr()) for t in p["keep"]],
                     p["scratch"], list(p["out_shape"]), [[repr(wk), u, lb] for wk, u, lb in p["tags"]], shapes(p["bufs"]))
        res.append(None if p is None else list(p["out_shape"]))

    ops.AUTOTUNE = False
    blk = IFBlock(synth.ifnet_state_dict(0), "block3.", CPU)
    plan("cost model", blk.chain)
    plan("cost model, tail5", blk.chain_tail5)
    ops.AUTOTUNE = True
    blk = IFBlock(synth.ifnet_state_dict(0), "block3.", CPU)
    plan("nothing tuned yet", blk.chain)
    hh, ww = 38, 54
    for layer, _ in blk.chain.layers:  # plant a winner per layer: the highest configuration id its tuner would time
        fam = ops._families(layer.two_term_ok)
        if isinstance(layer, ops.Deconv4x4):
            key = ("deconv4x4", 2, layer.cin, layer.cout, hh, ww, layer.ps)
            cands = [c for c in range(lib.drba_deconv4x4_num_cfgs()) if lib.drba_deconv4x4_cfg_family(c) in fam
                     and lib.drba_deconv4x4_packed_floats(layer.cin, layer.cout, c) > 0]
            hh, ww = 2 * hh, 2 * ww
        else:
            key = ("conv3x3", 2, layer.cin, layer.cout, hh, ww, layer.stride)
            cands = [c for c in range(lib.drba_conv3x3_num_cfgs()) if lib.drba_conv3x3_cfg_stride(c) == layer.stride
                     and lib.drba_conv3x3_cfg_family(c) in fam and lib.drba_conv3x3_packed_floats(layer.cin, layer.cout, c) > 0]
            hh, ww = (hh - 1) // layer.stride + 1, (ww - 1) // layer.stride + 1
        ops._tuned[(key, tuple(sorted(fam)))] = cands[-1]
    plan("winners planted", blk.chain)
    rec.note("kept", [sorted(l._keep) for l, _ in blk.chain.layers], [sorted(l._packed) for l, _ in blk.chain.layers])
    blk.conv0_1.pre_slope = 0.25
    plan("a layer with a pre_slope", blk.chain)
    return res


def _shuffle_ragged(rec):
    w = synth.seeded_state_dict({"w": (32, 16, 3, 3), "b": (32,)}, 0, "")
    layer = ops.Conv3x3(w["w"], w["b"], stride=1, act=None, device=CPU)
    return ops.conv3x3_shuffle(layer, torch.rand(1, 16, 12, 18))  # width 18: no multiple of 4


def _linear_split(families):
    def run(rec):
        ops.set_precision(families)
        sd = synth.seeded_state_dict({"w": (128, 64), "b": (128,), "lw": (128,), "lb": (128,)}, 0, "")
        lin = ops.LinearSplit(sd["w"], sd["b"], device=CPU)
        wide = torch.rand(2, 12, 160)
        res = []
        for x in (torch.rand(2, 12, 64), wide[..., 32:96]):
            res.append(lin(x))
            res.append(lin.layernorm(x, sd["lw"], sd["lb"], residual=torch.rand(2, 12, 128)))
        for a, b in ((torch.rand(2, 12, 32), torch.rand(2, 12, 32)), (wide[..., :48], wide[..., 144:])):
            k0 = lin.k
            res.append(lin.cat(a, b))
            rec.note("lin.k", k0, lin.k)
        rec.note("packs", sorted(lin._packs), lin.terms)
        return res
    return run


def _attention(rec):
    h, w, res = 8, 16, []
    qkv = torch.rand(2, h * w, 384)
    q, k, v = qkv[..., :128], qkv[..., 128:256], qkv[..., 256:]
    for fams in ({0, 1, 2, 3, 4}, {0, 1, 2, 3}):
        ops.set_precision(fams)
        res.append(ops.window_attention(q, k, v, h, w, 2, True, 128 ** 0.5))
    res.append(ops.window_attention(q, k, v, h, w, 1, False, 128 ** 0.5, terms=3))
    qk = torch.rand(h * w, 256)
    res.append(ops.global_expect2(qk[:, :128], qk[:, 128:], None, w, 128 ** 0.5))
    res.append(ops.global_expect2(qk[:, :128], qk[:, 128:], torch.rand(2, h * w), w, 128 ** 0.5))
    return res


def _ssim_thumb32(rec):
    ops.ssim_thumb32(torch.rand(1, 3, 64, 128), torch.rand(1, 3, 64, 128))  # (the value read back is uninitialised memory here)


SCENARIOS = {
    "rife/default": _rife(),
    "rife/no_lazy_flow": _rife(LAZY_FLOW=False),
    "rife/no_lazy_flow_no_stage_conv": _rife(LAZY_FLOW=False, STAGE_CONV_FUSED=False),
    "rife/24bit": _rife(families={0, 1, 2, 3}),
    "forward_pairs/7_at_1": _forward_pairs(1.0, 7),
    "forward_pairs/2_at_2": _forward_pairs(2.0, 2),
    "forward_pairs/9_at_0.5": _forward_pairs(0.5, 9),
    "gmfss": _gmfss,
    "gmfss_union/1.0": _gmfss_union(1.0, (128, 256)),
    "gmfss_union/0.5": _gmfss_union(0.5, (256, 512)),
    "operator_surface": _operator_surface,
    "non_union": _non_union,
    "head_fused": _head_fused,
    "stage_conv0": _stage_conv0,
    "stage_inputs": _stage_inputs,
    "warp_blend_lazy": _warp_blend_lazy,
    "flow_updates": _flow_updates,
    "drm_rife_linear_many": _drm_many,
    "softsplat_many": _softsplat_many,
    "chain_plan": _chain_plan,
    "conv3x3_shuffle_ragged": _shuffle_ragged,
    "linear_split/two_term": _linear_split({0, 1, 2, 3, 4}),
    "linear_split/24bit": _linear_split({0, 1, 2, 3}),
    "attention": _attention,
    "ssim_thumb32": _ssim_thumb32,
}

def _run(name, traced):
    rec, kept = Recorder(_lib.load()), []  # `kept` outlives the scenario: the pointer ordinals are all assigned by then
    with dry(rec), Keep(kept):
        if traced:
            ops.TRACE = []
        ret = shapes(SCENARIOS[name](rec))
        trace = None if not traced else [[first, [None if it is None else [repr(it[0]), it[1], it[2]] for it in items]]
                                         for first, items in ops.TRACE]
    return rec, ret, trace


def record(name):
    """-> {"calls": the log, "returns": shapes of the return values, "trace": ops.TRACE of the traced run, "pointers": distinct pointers}"""
    rec, ret, _ = _run(name, False)
    rec2, _, trace = _run(name, True)
    return {"calls": rec.calls, "returns": ret, "trace": trace, "traced_calls": digest(rec2.calls), "pointers": len(rec.ptrs)}


def digest(x):
    """SHA-256 of the canonical JSON of a recording; floats are written with repr, so exactly."""
    return hashlib.sha256(json.dumps(x, separators=(",", ":"), sort_keys=True).encode()).hexdigest()


def summarise(r):
    """What the file keeps of a scenario: the digest of the whole record and the counts that say where to look when it differs."""
    return {"sha256": digest(r), "calls": len(r["calls"]), "pointers": r["pointers"], "tags": len(r["trace"])}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--list":
        print("\n".join(SCENARIOS))
        sys.exit(0)
    if len(sys.argv) > 2 and sys.argv[1] == "--dump":  # the full recording of one scenario, to diff two commits with
        r = record(sys.argv[2])
        sys.stdout.write("{\n")
        for k in ("returns", "pointers", "traced_calls"):
            sys.stdout.write(' %s: %s,\n' % (json.dumps(k), json.dumps(r[k], sort_keys=True)))
        for k in ("calls", "trace"):
            sys.stdout.write(' %s: [\n%s\n ]%s\n' % (json.dumps(k), ",\n".join("  " + json.dumps(c, sort_keys=True) for c in r[k]),
                                                   "," if k == "calls" else ""))
        sys.stdout.write("}\n")
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "drba_amd"], capture_output=True, text=True,
                           check=True).stdout.strip()
    cases = {}
    for name in SCENARIOS:
        cases[name] = summarise(record(name))
        again = summarise(record(name))
        if again != cases[name]:  # the stability gate: a recording that does not repeat pins nothing
            sys.exit(f"{name}: two recordings in one run differ ({cases[name]} / {again}): nothing written")
    with open(path, "w") as f:  # one line per scenario
        f.write('{"made_from": %s,\n "scenarios": {\n' % json.dumps({"commit": head, "drba_amd_modified": bool(dirty),
                                                                   "by": "python tools/ops_calls.py"}))
        f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(cases.items())))
        f.write("\n }}\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(cases)} scenarios) from {head}")
